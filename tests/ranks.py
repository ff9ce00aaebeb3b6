"""The rank processes of the multi-rank tests: their environment, their start-up and end (iamr_amd.comm.start / stop over the gloo callback
transport: several ranks share the one GPU of the test machine), the loop of `iamr_amd.run.main` calls one group of ranks makes, and the
spawn that starts them -- under a time limit of its own, and leaving no child behind however it ends."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rank processes started at once.  The machines that run this suite stop a job in which more than 6 processes have the GPU open; the
# pytest process holds the device as well, so 4 ranks keep a margin.  An 8-member world runs on the CPU instead
# (tests/test_cpu_dist.py::test_eight_rank_gloo_halo_exchange_of_the_bench_layout).
MAX_RANKS = 4
# seconds: the ranks of one spawn (its callers say where a spawn needs longer), and a collective's wait for a rank that never arrives
LIMIT = 120.0


def free_port():
    """a TCP port nobody listens on right now (a port derived from the pid collided with a lingering socket once in round 6: the rendezvous
    of one test then waited ten minutes inside the driver's time budget)"""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def rank_env(rank, world, port=None, merge=False):
    """what `torch.distributed.run -m iamr_amd.run` would have put into the environment of this rank, with the gloo transport on device 0;
    merge: the library's default box mode (IAMRX_COALESCE = 1) instead of the callers' boxes kept"""
    for p in (os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(IAMRX_COALESCE="1" if merge else "0", RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      IAMRX_RUN_TRANSPORT="gloo", IAMRX_RUN_TIMEOUT=str(int(LIMIT)))
    if port is not None:
        os.environ["MASTER_PORT"] = str(port)


def start_rank(rank, world, port, merge=False):
    """the library, initialised on device 0, with the ranks connected (one rank: the library alone) -> iamr_amd.lib"""
    rank_env(rank, world, port, merge)
    from iamr_amd import comm, lib
    comm.start(rank, world, 0, "gloo", LIMIT)
    return lib


def stop_rank():
    from iamr_amd import comm
    comm.stop()


def run_jobs(rank, ports, jobs, log_dir, group, observe=None, after=None):
    """this rank's part of R.main once per job, the way `python -m iamr_amd.run` under torchrun calls it: a fresh rendezvous port per job,
    stdout of job q kept in <log_dir>/<group>_job<q>_r<rank>.txt.  observe: R.main's; after(q): called when job q has returned"""
    from iamr_amd import run as R
    for q, (port, argv) in enumerate(zip(ports, jobs)):
        os.environ["MASTER_PORT"] = str(port)
        with open(os.path.join(log_dir, f"{group}_job{q}_r{rank}.txt"), "w") as f:
            keep, sys.stdout = sys.stdout, f
            try:
                rc = R.main(argv, observe)
            finally:
                sys.stdout = keep
        assert rc == 0, (q, rc)
        if after:
            after(q)


def spawn(fn, world, *args, limit=LIMIT, max_ranks=MAX_RANKS):
    """fn(rank, world, *args) in `world` fresh processes.  Returns when all have; past `limit` seconds it fails.  However it ends -- the
    limit, a rank's exception (torch's ProcessRaisedException / ProcessExitedException), an exception delivered to this process -- no rank
    process outlives the call."""
    import torch.multiprocessing as mp
    assert world <= max_ranks
    ctx = mp.spawn(fn, args=(world,) + args, nprocs=world, join=False)
    end = time.monotonic() + limit
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                raise AssertionError(f"{world} rank(s) did not finish within {limit:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()
