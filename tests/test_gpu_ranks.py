"""mail_sieve_e.core with the product engine (GpuEngine) on several ranks, all
on one GPU: the lead builds the table, the followers receive its
table[:prime_bytes] view by broadcast and complete it (finish_table), every
rank sieves its chunk into its own torch tensors, the last rank sieves the
dropped tail into count slot 1, the counts are all-reduced, every rank writes
its primes{k}.txt.

One fresh child process per machine, as in tests/test_dist.py. The process
group is gloo, which carries the device tensors itself (RCCL refuses two ranks
on one device; tests/test_gpu_rccl.py covers the RCCL collectives themselves):
the code under test is the engine and _run_machine's call sequence, not the
collective.
"""
import hashlib
import multiprocessing as mp
import os
import socket
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine_factory(my_num):
    """core.GpuEngine, unchanged but for its process-group backend."""
    from mail_sieve_e import core

    class GlooGpuEngine(core.GpuEngine):
        backend = "gloo"
    return GlooGpuEngine(my_num)


def _machine(role, args, out_dir, q):
    os.environ["DSE_DEVICE"] = "0"
    sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-sieve-e_amd"), os.path.join(ROOT, "tests")]
    try:
        from mail_sieve_e import core
        start = core.lead_start if role == "lead" else core.client_start
        r = start(*args, out_dir=out_dir, engine_factory=_engine_factory, timeout_s=120)
        q.put(("ok", r.my_num, r.count, r.pi_ref, r.pi_full))
    except BaseException as e:  # reported to the parent
        q.put(("err", repr(e)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(P, N, out_dir):
    assert P <= 4
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_machine, args=("lead", (P, N, port), str(out_dir), q))]
    procs += [ctx.Process(target=_machine, args=("follower", ("127.0.0.1", port), str(out_dir), q))
              for _ in range(P - 1)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=180))
            if res[-1][0] != "ok":
                break  # its peers would wait for it in a collective: no point in waiting for them
    finally:
        for p in procs:
            if len(res) == len(procs):
                p.join(timeout=60)
            if p.is_alive():
                p.kill()
    errs = [r for r in res if r[0] != "ok"]
    assert not errs, errs
    res.sort(key=lambda r: r[1])
    assert [r[1] for r in res] == list(range(1, P + 1))
    return res


def test_run_lead_bat_three_gpu_ranks(tmp_path):
    """Run Lead.bat:1 (3 machines, N = 1,000,000): the figures test_dist.py pins for the oracle engine."""
    res = _run(3, 1_000_000, tmp_path)
    assert [r[2] for r in res] == [28664, 25404, 24429]
    assert all(r[3] == 78498 for r in res)
    sha = [hashlib.sha256((tmp_path / f"primes{k}.txt").read_bytes()).hexdigest()[:16] for k in (1, 2, 3)]
    assert sha == ["893331a3af40a499", "7f807e9baa0ff67e", "15254ce843ba8339"]


def test_four_gpu_ranks_ragged_chunks_and_prime_tail(tmp_path, oracle):
    """P = 4, N = 16,000,079: cs = 2,000,009 is one full segment plus 33,929 candidates
    (cs mod 64 = 9, cs mod 480 = 329), so every rank's chunk starts at another word and
    block alignment and ends in a partial word; the dropped tail {16000075, 16000077,
    16000079} holds the prime 16,000,079, so pi_full = pi_ref + 1. Counts and files
    against the oracle's faithful restatement."""
    N, P = 16_000_079, 4
    cs, masks, counts, _ = oracle.sieve(N, P)
    assert (cs, cs - 1966080, cs % 64, cs % 480) == (2_000_009, 33_929, 9, 329)
    assert oracle.tail_range(N, P) == (P * cs, 3) and 3 + 2 * (P * cs + 2) == N
    assert oracle.fast_sieve_range(P * cs, 3)[1] == 1
    res = _run(P, N, tmp_path)
    want = [int(c) for c in counts]
    assert [r[2] for r in res] == want
    assert all(r[3] == 1 + sum(want) and r[4] == r[3] + 1 for r in res), res
    for k in range(1, P + 1):
        ref = tmp_path / f"ref{k}.txt"
        oracle.finish(str(ref), k, N, P, masks[k - 1])
        assert (tmp_path / f"primes{k}.txt").read_bytes() == ref.read_bytes(), k
