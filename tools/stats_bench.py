#!/usr/bin/env python3
"""Constellation counts and gap statistics at P=1: host arithmetic on extracted primes against the
device statistics.

  (a) dse_sieve_all + Context.resident_primes(1) + numpy on the host: diff / bincount for the gaps,
      shifted compares of the prime array for the constellations (their members are consecutive
      primes): the only route before dse_stats_*; skipped above --host-max (the values would not fit)
  (b) dse_sieve_all + Context.resident_stats() with CONSTELLATIONS   (one dse_stats to the host)
  (c) the two statistics launches alone (HIP events) on a mask sieved into device memory
  (c0) the count-only launches of dse_primes_dev_async (out_cap = 0) on the same mask: they read
       the same bytes and do nothing else, the floor for one pass
  (e) the three extraction launches that write every prime as a uint64 (N <= --host-max)

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. The numbers of (a), (b) and (c) must be equal.

  python tools/stats_bench.py [--n 1000000000] [--reps 5] [--step-limit 120] [--host-max 2000000000]
"""
from __future__ import annotations

import argparse
import json
import sys

from bench_common import events, ms, step_limit, timed  # also: the package path, DSE_LIB


def host_numbers(np, primes, patterns):
    """(matches, gap histogram[1024], max_gap, lower prime of the first maximal gap) from the odd primes."""
    p = primes.astype(np.int64)
    matches = []
    for pat in patterns:
        diffs = [2 * j for j in range(32) if pat >> j & 1]
        n = len(p) - len(diffs) + 1
        ok = np.ones(max(n, 0), dtype=bool)
        for m in range(1, len(diffs)):
            ok &= (p[m:m + n] - p[:n]) == diffs[m]
        matches.append(int(ok.sum()))
    d = np.diff(p) // 2
    hist = np.bincount(d, minlength=1024)
    k = int(np.argmax(d))
    return matches, hist[:1024].astype(np.uint64), 2 * int(d[k]), int(p[k])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    N, P, lim = args.n, 1, args.step_limit
    with_host = N <= args.host_max
    print(f"stats_bench: N={N} P={P} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    res = {}
    out = {"N": N, "P": P, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8}

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_a():
            ctx.sieve_all(N, P)
            res["a"] = host_numbers(np, ctx.resident_primes(1), S.CONSTELLATIONS)

        def path_b():
            ctx.sieve_all(N, P)
            res["b"] = ctx.resident_stats()

        with step_limit("sieve_all", lim):
            s_med, _ = timed(sieve_only, args.reps)
        print(f"sieve_all alone                               median {s_med * 1e3:10.2f} ms")
        with step_limit("(b) device statistics", lim):
            b_med, b_all = timed(path_b, args.reps)
        st = res["b"]
        print(f"(b) sieve_all + resident_stats()              median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}")
        print(f"    primes {st.primes}  matches {st.matches}  max_gap {st.max_gap} at {st.max_gap_prime}"
              f"  non-zero bins {int(np.count_nonzero(st.gaps))}  overflow {st.gap_overflow}")
        out.update(sieve_all_ms=s_med * 1e3, b_device_ms=b_med * 1e3, primes=st.primes, matches=st.matches,
                   max_gap=st.max_gap, max_gap_prime=st.max_gap_prime)
        equal_ab = True
        if with_host:
            with step_limit("(a) host arithmetic", lim):
                a_med, a_all = timed(path_a, args.reps)
            m, hist, mg, mgp = res["a"]
            equal_ab = (m == st.matches and bool(np.array_equal(hist, st.gaps)) and mg == st.max_gap
                        and mgp == st.max_gap_prime)
            print(f"(a) sieve_all + resident_primes(1) + numpy    median {a_med * 1e3:10.2f} ms   all {ms(a_all)}")
            print(f"(a) == (b): {equal_ab}   (a) / (b) = {a_med / b_med:.1f}")
            out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / b_med)
        out["numbers_equal"] = equal_ab

    # (c), (c0), (e): the launches alone, on a mask sieved into device memory
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.zeros(_dse.STATS_WORDS, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()

        mb = mask.numel() * 8
        with step_limit("(c) statistics launches", lim):
            c_med, c_all = events(lambda: ctx.stats_dev_async(0, nbits, mask.data_ptr(), S.CONSTELLATIONS,
                                                              dst.data_ptr(), sp), args.reps)
            equal_c = bool(np.array_equal(dst.cpu().numpy().view(np.uint64), st.words))
        with step_limit("(c1) statistics launches, no patterns", lim):
            c1_med, c1_all = events(lambda: ctx.stats_dev_async(0, nbits, mask.data_ptr(), (), dst.data_ptr(), sp),
                                    args.reps)
        with step_limit("(c0) count only", lim):
            c0_med, c0_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, 0, 0, tot.data_ptr(), sp),
                                    args.reps)
            equal_c = equal_c and int(tot[0].item()) == st.primes
        print(f"(c) statistics launches, 7 patterns  median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
              f"   (mask read: {mb / c_med / 1e9:.1f} GB/s); equals (b): {equal_c}")
        print(f"(c1) statistics launches, no pattern median {c1_med * 1e3:8.3f} ms   all {ms(c1_all, 3)}"
              f"   (mask read: {mb / c1_med / 1e9:.1f} GB/s)")
        print(f"(c0) count-only launches (the floor) median {c0_med * 1e3:8.3f} ms   all {ms(c0_all, 3)}"
              f"   (mask read: {mb / c0_med / 1e9:.1f} GB/s)")
        print(f"(c) / floor = {c_med / c0_med:.2f}")
        out.update(c_launches_ms=c_med * 1e3, c1_no_patterns_ms=c1_med * 1e3, c0_floor_ms=c0_med * 1e3,
                   c_over_floor=c_med / c0_med, launch_output_equal=equal_c)
        if with_host:
            vals = torch.zeros(st.primes, dtype=torch.int64, device="cuda")
            with step_limit("(e) extraction launches", lim):
                e_med, e_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, vals.data_ptr(),
                                                                   st.primes, tot.data_ptr(), sp), args.reps)
            print(f"(e) extraction launches, {8 * st.primes / 1e6:.1f} MB written median {e_med * 1e3:8.3f} ms"
                  f"   all {ms(e_all, 3)}   (c) <= (e): {c_med <= e_med}")
            out.update(e_extraction_ms=e_med * 1e3)
    print(json.dumps(out))
    return 0 if equal_ab and equal_c else 1


if __name__ == "__main__":
    sys.exit(main())
