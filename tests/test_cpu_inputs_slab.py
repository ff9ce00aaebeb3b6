"""CPU suite: ns.spectral_distributed of the inputs front end -- the switch of the slab-decomposed transform of the spectra and the
budget on several ranks (the library's registry key SPECTRUM_DIST; iamr_amd/run.py sets it before the first spectrum)."""
import os
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TG16 = os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")


def test_the_key_is_parsed_and_defaults_to_the_gather():
    from iamr_amd.inputs import Inputs
    off = Inputs([TG16]).problem()
    assert off["spectral_distributed"] == 0
    assert Inputs([TG16], ["ns.spectral_distributed=0"]).problem() == off
    on = Inputs([TG16], ["ns.spectral_distributed=1"]).problem()
    assert on["spectral_distributed"] == 1
    assert {k: v for k, v in on.items() if k != "spectral_distributed"} == {k: v for k, v in off.items() if k != "spectral_distributed"}
    assert not any("spectral_distributed" in k for k in on["params"])
    with pytest.raises(ValueError, match=r"ns.spectral_distributed = 2: 0 \(the gather\) or 1"):
        Inputs([TG16], ["ns.spectral_distributed=2"]).problem()
    with pytest.raises(KeyError, match="ns.spectral_distribute"):                    # an unknown neighbour key still raises
        Inputs([TG16], ["ns.spectral_distribute=1"]).problem()


def test_a_two_dimensional_run_refuses_it():
    from iamr_amd.inputs import Inputs
    assert Inputs([POIS2D]).problem()["spectral_distributed"] == 0
    assert Inputs([POIS2D], ["ns.spectral_distributed=0"]).problem()["spectral_distributed"] == 0
    with pytest.raises(NotImplementedError, match=r"ns.spectral_distributed = 1 in a two-dimensional run"):
        Inputs([POIS2D], ["ns.spectral_distributed=1"]).problem()
