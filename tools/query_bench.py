#!/usr/bin/env python3
"""Rank and select at P=1: pi(x), the n-th prime, next / prev prime and membership from the mask
dse_sieve_all leaves resident, against the only route before (extract every prime, search on the host).

  (a) the index build alone (HIP events) on a mask sieved into device memory
  (a0) the count-only launches of dse_primes_dev_async (out_cap = 0) on the same mask: the same
       two launches as (a)
  (b) each kind's launch alone (HIP events) on --nq uniformly random queries; for RANK the mask
      bytes per second (nq x 2 KiB over the launch time)
  (c) dse_query_resident end to end (host clock): the first call after a dse_sieve_all (it builds
      the index) and the second, per kind
  (d) N <= --host-max only: Context.resident_primes(1) + numpy.searchsorted for the same queries;
      the answers of (b), (c) and (d) must be equal

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU.

  python tools/query_bench.py [--n 1000000000] [--nq 1048576] [--reps 5] [--step-limit 120] [--host-max 2000000000]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time

from bench_common import events, ms, step_limit, timed  # also: the package path, DSE_LIB

KINDS = ("RANK", "SELECT", "NEXT", "PREV", "TEST")
TILE_BYTES = 2048


def host_answers(np, primes, kind, q, none):
    """The answers from the extracted odd primes by numpy.searchsorted."""
    padded = np.concatenate([primes, np.array([none], dtype=np.uint64)])
    n = len(primes)
    if kind == 0:
        return np.searchsorted(primes, q, side="right").astype(np.uint64)
    if kind == 1:
        return padded[np.minimum(q, np.uint64(n)).astype(np.int64)]
    if kind == 2:
        return padded[np.searchsorted(primes, q, side="right")]
    i = np.searchsorted(primes, q, side="left")
    if kind == 3:
        return np.where(i > 0, padded[np.maximum(i, 1) - 1], np.uint64(none))
    return ((i < n) & (padded[i] == q)).astype(np.uint64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--seed", type=int, default=12)
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import sieve as S

    N, P, nq, lim = args.n, 1, args.nq, args.step_limit
    with_host = N <= args.host_max
    print(f"query_bench: N={N} P={P} nq={nq} reps={args.reps} seed={args.seed} device={torch.cuda.get_device_name(0)}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    tiles = (nbits + S._dse.PRIMES_TILE_BITS - 1) // S._dse.PRIMES_TILE_BITS
    out = {"N": N, "P": P, "nq": nq, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8,
           "index_bytes": S.query_index_bytes(nbits), "tiles": tiles}
    rng = np.random.default_rng(args.seed)
    values = rng.integers(0, hi + 2, nq).astype(np.uint64)  # uniform over the covered values
    res_c, res_b = {}, {}
    equal = True

    # (c), (d): the resident run
    with S.Context(num_gpus=1) as ctx:
        with step_limit("sieve_all", lim):
            _, pi_ref, _ = ctx.sieve_all(N, P)
        ranks = rng.integers(0, pi_ref - 1, nq).astype(np.uint64)  # uniform over the entries' ranks
        queries = [values, ranks, values, values, values]
        first, second = [], []
        with step_limit("(c) first and second call", lim):
            for _ in range(args.reps + 1):
                ctx.sieve_all(10**6, P)  # another run: the masks and the index are replaced
                ctx.sieve_all(N, P)
                b0 = ctx.debug_get_stat("query_index_builds")
                t0 = time.perf_counter()
                ctx.resident_query(S.QUERY_RANK, values)
                t1 = time.perf_counter()
                ctx.resident_query(S.QUERY_RANK, values)
                t2 = time.perf_counter()
                assert ctx.debug_get_stat("query_index_builds") == b0 + 1
                first.append(t1 - t0)
                second.append(t2 - t1)
        first, second = first[1:], second[1:]  # the first round is the warm-up
        print(f"(c) resident_query(RANK), first call (builds the index)  median {statistics.median(first) * 1e3:9.3f} ms"
              f"   all {ms(first, 3)}")
        print(f"(c) resident_query(RANK), second call                    median {statistics.median(second) * 1e3:9.3f} ms"
              f"   all {ms(second, 3)}")
        out.update(c_first_ms=statistics.median(first) * 1e3, c_second_ms=statistics.median(second) * 1e3)
        for kind, name in enumerate(KINDS):
            def call(kind=kind):
                res_c[kind] = ctx.resident_query(kind, queries[kind])
            with step_limit(f"(c) {name}", lim):
                med, every = timed(call, args.reps)
            print(f"(c) resident_query({name:6s}) end to end, index built      median {med * 1e3:9.3f} ms   all {ms(every, 3)}")
            out[f"c_{name.lower()}_ms"] = med * 1e3
        if with_host:
            got = {}

            def path_d():
                primes = ctx.resident_primes(1)
                for kind in range(len(KINDS)):
                    got[kind] = host_answers(np, primes, kind, queries[kind], S.QUERY_NONE)
            with step_limit("(d) extract and search on the host", lim):
                d_med, d_all = timed(path_d, args.reps)
            eq_d = all(bool(np.array_equal(got[k], res_c[k])) for k in range(len(KINDS)))
            equal = equal and eq_d
            c_all = sum(out[f"c_{n.lower()}_ms"] for n in KINDS)
            print(f"(d) resident_primes(1) + numpy.searchsorted, all five kinds  median {d_med * 1e3:9.2f} ms   all {ms(d_all)}")
            print(f"(d) == (c): {eq_d}   (d) / (c, five kinds) = {d_med * 1e3 / c_all:.1f}")
            out.update(d_host_ms=d_med * 1e3, d_over_c=d_med * 1e3 / c_all)

    # (a), (a0), (b): the launches alone, on a mask sieved into device memory
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        ib = S.query_index_bytes(nbits)
        index = torch.zeros(ib // 8, dtype=torch.int64, device="cuda")
        dq = [torch.from_numpy(q.view(np.int64)).cuda() for q in (values, ranks)]
        dq = [dq[0], dq[1], dq[0], dq[0], dq[0]]
        dout = torch.zeros(nq, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()
        with step_limit("(a) index build", lim):
            a_med, a_all = events(lambda: ctx.query_index_dev_async(0, nbits, mask.data_ptr(), index.data_ptr(), ib, sp),
                                  args.reps)
        with step_limit("(a0) count only", lim):
            a0_med, a0_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, 0, 0, tot.data_ptr(), sp),
                                    args.reps)
        mb = mask.numel() * 8
        equal = equal and int(index[tiles].item()) == int(tot[0].item()) == pi_ref - 1
        print(f"(a)  index build                     median {a_med * 1e3:8.3f} ms   all {ms(a_all, 3)}"
              f"   (mask read: {mb / a_med / 1e9:.1f} GB/s)")
        print(f"(a0) count-only dse_primes_dev_async median {a0_med * 1e3:8.3f} ms   all {ms(a0_all, 3)}"
              f"   (mask read: {mb / a0_med / 1e9:.1f} GB/s)   (a) / (a0) = {a_med / a0_med:.3f}")
        out.update(a_index_ms=a_med * 1e3, a0_count_only_ms=a0_med * 1e3)
        for kind, name in enumerate(KINDS):
            with step_limit(f"(b) {name}", lim):
                b_med, b_all = events(lambda: ctx.query_dev_async(kind, 0, nbits, mask.data_ptr(), index.data_ptr(),
                                                                  dq[kind].data_ptr(), nq, dout.data_ptr(), sp), args.reps)
                res_b[kind] = dout.cpu().numpy().view(np.uint64).copy()
            eq_b = bool(np.array_equal(res_b[kind], res_c[kind]))
            equal = equal and eq_b
            extra = f"   (mask read: {nq * TILE_BYTES / b_med / 1e9:.1f} GB/s)" if name == "RANK" else ""
            print(f"(b)  {name:6s} launch, {nq} queries  median {b_med * 1e3:8.3f} ms   all {ms(b_all, 3)}"
                  f"   {nq / b_med / 1e6:8.1f} M queries/s   equals (c): {eq_b}{extra}")
            out[f"b_{name.lower()}_ms"] = b_med * 1e3
        out["b_rank_mask_gbs"] = nq * TILE_BYTES / (out["b_rank_ms"] * 1e-3) / 1e9
    out["answers_equal"] = equal
    print(json.dumps(out))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
