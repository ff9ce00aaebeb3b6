"""CPU: the helper every multi-rank test starts its rank processes with (tests/ranks.py).  Two ranks that open no device and never load the
library: a spawn returns when its ranks have, fails at its time limit, hands on a rank's exception -- and leaves no child behind in any
of the three cases."""
import multiprocessing
import os
import socket
import sys
import time
import pytest
import ranks

NAP = 60.0          # seconds a rank sleeps that is meant to be ended from outside: far beyond anything the tests wait for


def returns(rank, world, out_dir):
    with open(os.path.join(out_dir, f"r{rank}_of_{world}"), "w"):
        pass


def rank_one_sleeps(rank, world):
    if rank == 1:
        time.sleep(NAP)


def rank_one_raises(rank, world):
    if rank == 1:
        raise ValueError("rank 1 gives up")
    time.sleep(NAP)


def test_spawn_returns_when_the_ranks_have(tmp_path):
    ranks.spawn(returns, 2, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["r0_of_2", "r1_of_2"]
    assert multiprocessing.active_children() == []


def test_spawn_fails_at_its_limit_and_ends_the_ranks():
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match=r"^2 rank\(s\) did not finish within 3 s$"):
        ranks.spawn(rank_one_sleeps, 2, limit=3)
    assert time.monotonic() - t0 <= 3 + 5
    assert multiprocessing.active_children() == []


def test_a_rank_that_raises_surfaces_and_its_sibling_is_ended():
    from torch.multiprocessing import ProcessRaisedException
    t0 = time.monotonic()
    with pytest.raises(ProcessRaisedException, match="rank 1 gives up"):
        ranks.spawn(rank_one_raises, 2)
    assert time.monotonic() - t0 < NAP / 2          # nobody waited for the sleeping sibling
    assert multiprocessing.active_children() == []


def test_more_ranks_than_allowed_are_refused():
    with pytest.raises(AssertionError):
        ranks.spawn(returns, ranks.MAX_RANKS + 1, "")
    assert multiprocessing.active_children() == []


def test_free_port_can_be_bound():
    port = ranks.free_port()
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", port))


def test_rank_env_sets_the_documented_variables():
    names = {"IAMRX_COALESCE", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "IAMRX_RUN_TRANSPORT", "IAMRX_RUN_TIMEOUT"}
    env, path = dict(os.environ), list(sys.path)
    try:
        for k in names | {"MASTER_PORT"}:
            os.environ.pop(k, None)
        before = dict(os.environ)
        sys.path[:] = [p for p in sys.path if p not in (ranks.ROOT, os.path.join(ranks.ROOT, "tests"))]
        ranks.rank_env(1, 3)
        assert {k: v for k, v in os.environ.items() if before.get(k) != v} == dict(
            IAMRX_COALESCE="0", RANK="1", WORLD_SIZE="3", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", IAMRX_RUN_TRANSPORT="gloo",
            IAMRX_RUN_TIMEOUT=str(int(ranks.LIMIT)))
        assert set(before) - set(os.environ) == set()
        ranks.rank_env(0, 2, port=23456, merge=True)
        assert {k: v for k, v in os.environ.items() if before.get(k) != v} == dict(
            IAMRX_COALESCE="1", RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", IAMRX_RUN_TRANSPORT="gloo",
            IAMRX_RUN_TIMEOUT=str(int(ranks.LIMIT)), MASTER_PORT="23456")
        assert {ranks.ROOT, os.path.join(ranks.ROOT, "tests")} <= set(sys.path)
    finally:
        os.environ.clear()
        os.environ.update(env)
        sys.path[:] = path
