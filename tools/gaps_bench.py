#!/usr/bin/env python3
"""First occurrence of every prime gap at P=1: host arithmetic on extracted primes against the device
table.

  (a) dse_sieve_all + Context.resident_primes(1) + numpy on the host (diff, the first index of every
      distinct difference): the only general route before dse_gaps_*; "none" above --host-max (the
      values would not fit)
  (b) dse_sieve_all + Context.resident_gaps()   (one dse_gaps to the host)
  (c) the two gaps launches alone (HIP events) on a mask sieved into device memory
  next to them, on the same mask:
  (c1) the two dse_stats launches with no pattern (the gap histogram and the maximal gap)
  (c0) the count-only launches of dse_primes_dev_async (out_cap = 0)
  (cp) a device-to-device copy of the mask: reads it once and writes it once, the floor

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. (a), (b) and (c) must be equal, the maximal gap must be resident_stats',
and at N = 1e9, 1e10 and 1e11 the last records must be the published ones.

  python tools/gaps_bench.py [--n 1000000000] [--reps 5] [--step-limit 120] [--host-max 2000000000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys

from bench_common import Record, events, ms, step_limit, timed  # also: the package path, DSE_LIB

# N -> the last maximal gaps below it (gap, lower prime), A005250 at A002386
LAST_RECORDS = {10**9: [(250, 387096133), (282, 436273009)], 10**10: [(336, 3842610773), (354, 4302407359)],
                10**11: [(456, 25056082087), (464, 42652618343)]}


def host_table(np, primes):
    """(first[1024] as odd indices, NONE where there is none; max_gap; its lower prime) from the odd primes."""
    p = primes.astype(np.int64)
    d = np.diff(p) // 2
    vals, at = np.unique(d, return_index=True)
    first = np.full(1024, (1 << 64) - 1, dtype=np.uint64)
    for v, k in zip(vals, at):
        if v < 1024:
            first[int(v)] = (int(p[k]) - 3) // 2
    k = int(np.argmax(d))
    return first, 2 * int(d[k]), int(p[k])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    say = Record()
    N, P, lim = args.n, 1, args.step_limit
    with_host = N <= args.host_max
    say(f"gaps_bench: N={N} P={P} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    res = {}
    out = {"N": N, "P": P, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8}

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_a():
            ctx.sieve_all(N, P)
            res["a"] = host_table(np, ctx.resident_primes(1))

        def path_b():
            ctx.sieve_all(N, P)
            res["b"] = ctx.resident_gaps()

        with step_limit("sieve_all", lim):
            s_med, _ = timed(sieve_only, args.reps)
        say(f"sieve_all alone                               median {s_med * 1e3:10.2f} ms")
        with step_limit("(b) device table", lim):
            b_med, b_all = timed(path_b, args.reps)
        g = res["b"]
        with step_limit("resident_stats", lim):
            st = ctx.resident_stats(patterns=())
        rec = g.records()
        say(f"(b) sieve_all + resident_gaps()               median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}")
        say(f"    primes {g.primes}  found {g.found}  max_gap {g.max_gap} at {g.max_gap_prime}  records {len(rec)}"
            f"  last {rec[-2:]}")
        ok_stats = ((g.max_gap, g.max_gap_g, g.primes) == (st.max_gap, st.max_gap_g, st.primes)
                    and bool(np.array_equal(g.first != np.uint64(_dse.GAPS_NONE), st.gaps > 0)))
        ok_rec = N not in LAST_RECORDS or rec[-2:] == LAST_RECORDS[N]
        say(f"    maximal gap and found bins equal resident_stats': {ok_stats}   published last records: {ok_rec}")
        out.update(sieve_all_ms=s_med * 1e3, b_device_ms=b_med * 1e3, primes=g.primes, found=g.found,
                   max_gap=g.max_gap, max_gap_prime=g.max_gap_prime, records=len(rec))
        equal_ab = True
        if with_host:
            with step_limit("(a) host arithmetic", lim):
                a_med, a_all = timed(path_a, args.reps)
            first, mg, mgp = res["a"]
            equal_ab = bool(np.array_equal(first, g.first)) and mg == g.max_gap and mgp == g.max_gap_prime
            say(f"(a) sieve_all + resident_primes(1) + numpy    median {a_med * 1e3:10.2f} ms   all {ms(a_all)}"
                f"   ({8 * g.primes / 1e6:.1f} MB of values)")
            say(f"(a) == (b): {equal_ab}   (a) / (b) = {a_med / b_med:.1f}")
            out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / b_med)
        else:
            say(f"(a) the route before: none ({8 * g.primes / 1e9:.1f} GB of values)")
        out["numbers_equal"] = equal_ab and ok_stats and ok_rec

    # (c), (c1), (c0), (cp): the launches alone, on a mask sieved into device memory
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        copy = torch.zeros_like(mask)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.zeros(_dse.GAPS_WORDS, dtype=torch.int64, device="cuda")
        sdst = torch.zeros(_dse.STATS_WORDS, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()

        mb = mask.numel() * 8
        with step_limit("(c) gaps launches", lim):
            c_med, c_all = events(lambda: ctx.gaps_dev_async(0, nbits, mask.data_ptr(), dst.data_ptr(), sp), args.reps)
            equal_c = bool(np.array_equal(dst.cpu().numpy().view(np.uint64), g.words))
        with step_limit("(c1) statistics launches, no patterns", lim):
            c1_med, c1_all = events(lambda: ctx.stats_dev_async(0, nbits, mask.data_ptr(), (), sdst.data_ptr(), sp),
                                    args.reps)
        with step_limit("(c0) count only", lim):
            c0_med, c0_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, 0, 0, tot.data_ptr(), sp),
                                    args.reps)
            equal_c = equal_c and int(tot[0].item()) == g.primes
        with step_limit("(cp) device-to-device copy", lim):
            cp_med, cp_all = events(lambda: copy.copy_(mask), args.reps)
        say(f"(c)  gaps launches                     median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
            f"   (mask read: {mb / c_med / 1e9:.1f} GB/s); equals (b): {equal_c}")
        say(f"(c1) statistics launches, no pattern   median {c1_med * 1e3:8.3f} ms   all {ms(c1_all, 3)}"
            f"   (mask read: {mb / c1_med / 1e9:.1f} GB/s)")
        say(f"(c0) count-only launches               median {c0_med * 1e3:8.3f} ms   all {ms(c0_all, 3)}"
            f"   (mask read: {mb / c0_med / 1e9:.1f} GB/s)")
        say(f"(cp) device-to-device copy (the floor) median {cp_med * 1e3:8.3f} ms   all {ms(cp_all, 3)}"
            f"   (read + write: {2 * mb / cp_med / 1e9:.1f} GB/s)")
        say(f"(c) / (c1) = {c_med / c1_med:.2f}   (c) / (c0) = {c_med / c0_med:.2f}   (c) / (cp) = {c_med / cp_med:.2f}")
        out.update(c_launches_ms=c_med * 1e3, c1_stats_no_patterns_ms=c1_med * 1e3, c0_count_ms=c0_med * 1e3,
                   cp_copy_ms=cp_med * 1e3, c_over_c1=c_med / c1_med, c_over_copy=c_med / cp_med,
                   launch_output_equal=equal_c)
    say(json.dumps(out))
    if args.out:
        say()
        say.write(args.out, append=True)
    return 0 if out["numbers_equal"] and equal_c else 1


if __name__ == "__main__":
    sys.exit(main())
