#!/usr/bin/env python3
"""Power and reciprocal sums over the primes and the twins at P=1: host arithmetic on extracted
primes against the device sums.

  (a) dse_sieve_all + Context.resident_primes(1) + Python integers on the host (the sums of p, of p^2
      and of floor(2^126 / p)): the only route before dse_sums_*; "none" above --host-max (the values
      would not fit)
  (b) dse_sieve_all + Context.sums_resident()   (one dse_sums to the host)
  (c) the two sums launches alone (HIP events) on a mask sieved into device memory, for flags 1
      (POWER), 2 (RECIP) and 3, over the primes (require = 1) and over the twins (require = 3)
  next to them, on the same mask, in the same run:
  (c1) the two dse_stats launches with no pattern
  (cp) a device-to-device copy of the mask: reads it once and writes it once, the floor

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. (a), (b) and (c) must be equal, and the matches must be resident_stats'.

  python tools/sums_bench.py [--n 1000000000] [--reps 5] [--step-limit 120] [--host-max 2000000000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys

from bench_common import Record, events, ms, step_limit, timed  # also: the package path, DSE_LIB

# N -> (sum of the odd primes <= N: A046731 less 2)
KNOWN_SUM1 = {10**6: 37550402021, 10**8: 279209790387274}


def host_sums(np, primes):
    """(count, sum p, sum p^2, sum floor(2^126 / p)) from the odd primes, exactly: Python integers, a
    block of values at a time."""
    one = 1 << 126
    s1 = s2 = rc = 0
    for i in range(0, len(primes), 1 << 22):
        p = primes[i:i + (1 << 22)].tolist()
        s1 += sum(p)
        s2 += sum(map(int.__mul__, p, p))
        rc += sum(map(one.__floordiv__, p))
    return len(primes), s1, s2, rc


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--host-reps", type=int, default=1, help="runs of (a): its Python divisions take a minute at 1e9")
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    say = Record()
    N, P, lim = args.n, 1, args.step_limit
    with_host = N <= args.host_max
    say(f"sums_bench: N={N} P={P} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    res = {}
    out = {"N": N, "P": P, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8}

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_a():
            ctx.sieve_all(N, P)
            res["a"] = host_sums(np, ctx.resident_primes(1))

        def path_b():
            ctx.sieve_all(N, P)
            res["b"] = ctx.sums_resident()

        with step_limit("sieve_all", lim):
            s_med, _ = timed(sieve_only, args.reps)
        say(f"sieve_all alone                               median {s_med * 1e3:10.2f} ms")
        with step_limit("(b) device sums", lim):
            b_med, b_all = timed(path_b, args.reps)
        s = res["b"]
        with step_limit("resident_stats", lim):
            st = ctx.resident_stats(patterns=[S.TWINS])
            tw = ctx.sums_resident(None, 3, 0)
        say(f"(b) sieve_all + sums_resident()               median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}")
        say(f"    primes {s.matches}  sum1 {s.sum1}  sum2 {s.sum2}  recip {s.recip}  sum 1/p = {s.reciprocal!r}")
        say(f"    twins {tw.matches}  B2 partial sum = {tw.reciprocal!r}")
        ok_stats = s.matches == st.primes and tw.matches == st.matches[0]
        ok_known = N not in KNOWN_SUM1 or s.sum1 == KNOWN_SUM1[N]
        say(f"    matches equal resident_stats': {ok_stats}   published sum of primes: {ok_known}")
        out.update(sieve_all_ms=s_med * 1e3, b_device_ms=b_med * 1e3, primes=s.matches, sum1=s.sum1, sum2=s.sum2,
                   recip=s.recip, twins=tw.matches, twins_recip=tw.recip)
        equal_ab = True
        if with_host:
            with step_limit("(a) host arithmetic", max(lim, 600)):
                a_med, a_all = timed(path_a, args.host_reps)
            equal_ab = res["a"] == (s.matches, s.sum1, s.sum2, s.recip)
            say(f"(a) sieve_all + resident_primes(1) + host arithmetic  median {a_med * 1e3:10.2f} ms   all {ms(a_all)}"
                f"   ({8 * s.matches / 1e6:.1f} MB of values)")
            say(f"(a) == (b): {equal_ab}   (a) / (b) = {a_med / b_med:.1f}")
            out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / b_med)
        else:
            say(f"(a) the route before: none ({8 * s.matches / 1e9:.1f} GB of values)")
        out["numbers_equal"] = bool(equal_ab and ok_stats and ok_known)

    # (c), (c1), (cp): the launches alone, on a mask sieved into device memory
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        copy = torch.zeros_like(mask)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.zeros(_dse.SUMS_WORDS, dtype=torch.int64, device="cuda")
        sdst = torch.zeros(_dse.STATS_WORDS, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()

        mb = mask.numel() * 8
        with step_limit("(c1) statistics launches, no patterns", lim):
            c1_med, c1_all = events(lambda: ctx.stats_dev_async(0, nbits, mask.data_ptr(), (), sdst.data_ptr(), sp),
                                    args.reps)
        with step_limit("(cp) device-to-device copy", lim):
            cp_med, cp_all = events(lambda: copy.copy_(mask), args.reps)
        say(f"(c1) statistics launches, no pattern   median {c1_med * 1e3:8.3f} ms   all {ms(c1_all, 3)}"
            f"   (mask read: {mb / c1_med / 1e9:.1f} GB/s)")
        say(f"(cp) device-to-device copy (the floor) median {cp_med * 1e3:8.3f} ms   all {ms(cp_all, 3)}"
            f"   (read + write: {2 * mb / cp_med / 1e9:.1f} GB/s)")
        out.update(c1_stats_no_patterns_ms=c1_med * 1e3, cp_copy_ms=cp_med * 1e3)
        equal_c = True
        for name, require, want in (("primes", 1, s), ("twins", 3, tw)):
            for flags in (1, 2, 3):
                with step_limit(f"(c) sums launches, {name}, flags {flags}", lim):
                    c_med, c_all = events(lambda: ctx.sums_dev_async(0, nbits, mask.data_ptr(), require, 0, 0, 0, 0,
                                                                     flags, dst.data_ptr(), sp), args.reps)
                    got = S.Sums(dst.cpu().numpy().view(np.uint64))
                eq = (got.matches == want.matches and (not flags & 1 or (got.sum1, got.sum2) == (want.sum1, want.sum2))
                      and (not flags & 2 or got.recip == want.recip))
                equal_c = equal_c and eq
                div = got.matches * bin(require).count("1") if flags & 2 else 0
                rate = f"   {div / c_med / 1e9:6.2f} G divisions/s" if div else ""
                say(f"(c)  sums launches {name:6s} flags {flags}    median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
                    f"   (mask read: {mb / c_med / 1e9:7.1f} GB/s){rate}   / (c1) = {c_med / c1_med:6.2f}"
                    f"   / (cp) = {c_med / cp_med:6.2f}   equals (b): {eq}")
                out[f"c_{name}_flags{flags}_ms"] = c_med * 1e3
                out[f"c_{name}_flags{flags}_over_c1"] = c_med / c1_med
                out[f"c_{name}_flags{flags}_over_copy"] = c_med / cp_med
        out["launch_output_equal"] = bool(equal_c)
    say(json.dumps(out))
    if args.out:
        say()
        say.write(args.out, append=True)
    return 0 if out["numbers_equal"] and equal_c else 1


if __name__ == "__main__":
    sys.exit(main())
