"""GPU: the ORDER of what iamr_amd.run.main does, for a single level and for a hierarchy.  Several ranks execute the main loop in lock-step
and most of its operations are collective (sums, profile, spectrum, plotfile, checkpoint): two of them swapped pass every one-rank test
and hang on two ranks.  Every line a run prints is reduced to its kind (numbers other than step counters are dropped, paths are kept
relative to the run's directory) and the sequence is compared with the literal lists below.  They were taken from the output of the
driver while it still had two separate loops, one per kind of run, before these became one."""
import os
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEVEL = [os.path.join(GOLD, "inputs.3d.taylorgreen_stats16"), "ns.profile_interval=1", "ns.spectrum_interval=1", "amr.plot_int=2", "amr.check_int=2"]
HIERARCHY = [os.path.join(GOLD, "inputs.3d.tracer_regrid16"), "ns.sum_interval=1", "ns.profile_interval=1", "ns.profile_level=2", "amr.plot_int=2",
             "amr.check_int=2"]


LEVEL_START = ["SUMS", "PROFILE prof00000", "SPECTRUM spec00000", "PLOTFILE plt00000"]
LEVEL_STEPS = {1: ["STEP 1", "SUMS", "PROFILE prof00001", "SPECTRUM spec00001"],
               2: ["STEP 2", "SUMS", "PROFILE prof00002", "SPECTRUM spec00002", "PLOTFILE plt00002", "CHECKPOINT chk00002"],
               3: ["STEP 3", "SUMS", "PROFILE prof00003", "SPECTRUM spec00003"],
               4: ["STEP 4", "SUMS", "PROFILE prof00004", "SPECTRUM spec00004", "PLOTFILE plt00004", "CHECKPOINT chk00004"]}
HIERARCHY_START = ["SUMS", "PROFILE prof00000", "PLOTFILE plt00000"]
HIERARCHY_STEPS = {1: ["STEP 1", "SUMS", "PROFILE prof00001"],
                   2: ["STEP 2", "SUMS", "PROFILE prof00002", "PLOTFILE plt00002", "CHECKPOINT chk00002"],
                   3: ["STEP 3", "SUMS", "PROFILE prof00003"],
                   4: ["STEP 4", "SUMS", "PROFILE prof00004", "PLOTFILE plt00004", "CHECKPOINT chk00004"]}


def kinds(out, root):
    """the kinds of the lines of a run's stdout; the blank line and the three TIME= lines of the integrated quantities are one SUMS"""
    lines = out.splitlines()
    seq, q = [], 0
    while q < len(lines):
        l = lines[q]
        if l == "" and [x.startswith("TIME= ") for x in lines[q + 1:q + 4]] == [True] * 3:
            assert [x.split("= ")[1].rsplit(" ", 1)[1] for x in lines[q + 1:q + 4]] == ["MASS", "TRAC", "ENERGY"], lines[q + 1:q + 4]
            seq.append("SUMS")
            q += 3
        elif l.startswith("STEP = "):
            seq.append("STEP " + l.split()[2])
        elif l.split(":")[0] in ("PROFILE", "SPECTRUM", "PLOTFILE", "CHECKPOINT"):
            seq.append(l.split(":")[0] + " " + os.path.relpath(l.split(": ", 1)[1], root))
        elif l.startswith("PARTICLES:"):
            seq.append("PARTICLES")
        elif l.startswith("RESTART from "):
            seq.append("RESTART")
        elif l.startswith("inputs: ignored"):
            seq.append("inputs: ignored")
        elif l.startswith("Run time = "):
            seq.append("Run time")
        else:
            seq.append(l)               # a line of no known kind: kept, so that it fails the comparison
        q += 1
    return seq


def transcript(argv, tmp_path, capsys, *more):
    from iamr_amd import run as R
    root = str(tmp_path)
    capsys.readouterr()
    files = [f"amr.plot_file={root}/plt", f"amr.check_file={root}/chk", f"ns.profile_file={root}/prof", f"ns.spectrum_file={root}/spec"]
    assert R.main(argv + files + list(more)) == 0
    out = capsys.readouterr().out
    print(out)
    return out, kinds(out, root)


def _without_ignored(seq):
    return [k for k in seq if k != "inputs: ignored"]


def test_single_level(gpu, tmp_path, capsys):
    """case: TaylorGreen 16^3 on one level with sums, time averages, profiles, spectra, plotfiles and checkpoints, 4 steps; then its
    restart from the checkpoint of step 2"""
    out, seq = transcript(LEVEL, tmp_path, capsys)
    assert seq == LEVEL_START + sum((LEVEL_STEPS[n] for n in (1, 2, 3, 4)), []) + ["Run time"], seq
    steps = [l for l in out.splitlines() if l.startswith("STEP = ")]
    assert len(steps) == 4 and not [l for l in steps if "LEVELS" in l or "GRIDS" in l], steps
    first = seq.index("STEP 1")
    assert [k.split()[0] for k in seq[:first] if k != "inputs: ignored"][:3] == ["SUMS", "PROFILE", "SPECTRUM"], seq[:first]
    out, seq = transcript(LEVEL, tmp_path, capsys, f"amr.restart={tmp_path}/chk00002")
    assert seq[0] == "RESTART" and _without_ignored(seq)[1] == "STEP 3", seq
    assert not [k for k in seq if k.endswith("00000") or k in ("STEP 1", "STEP 2")], seq
    assert _without_ignored(seq) == ["RESTART"] + LEVEL_STEPS[3] + LEVEL_STEPS[4] + ["Run time"], seq
    assert "LEVELS" not in out and "levels" not in out.splitlines()[0], out.splitlines()[0]


def test_hierarchy(gpu, tmp_path, capsys):
    """case: the tracer blob on three levels with regrids, sums and profiles binned on the finest level, 4 coarse steps"""
    out, seq = transcript(HIERARCHY, tmp_path, capsys)
    assert seq == HIERARCHY_START + sum((HIERARCHY_STEPS[n] for n in (1, 2, 3, 4)), []) + ["Run time"], seq
    steps = [l for l in out.splitlines() if l.startswith("STEP = ")]
    assert len(steps) == 4 and all(" LEVELS = " in l and " GRIDS = [" in l for l in steps), steps
    first = seq.index("STEP 1")
    assert [k.split()[0] for k in seq[:first]][:2] == ["SUMS", "PROFILE"], seq[:first]


def test_hierarchy_with_spectrum(gpu, tmp_path, capsys):
    """the hierarchy case asks for no spectra; with ns.spectrum_interval = 1 added, one step: the spectrum follows the profile, for the
    initial data (before the first STEP line) and after the step"""
    out, seq = transcript(HIERARCHY, tmp_path, capsys, "ns.spectrum_interval=1", "max_step=1", "amr.plot_int=-1", "amr.check_int=-1")
    assert _without_ignored(seq) == ["SUMS", "PROFILE prof00000", "SPECTRUM spec00000", "STEP 1", "SUMS", "PROFILE prof00001", "SPECTRUM spec00001",
                                     "Run time"], seq
