#!/usr/bin/env python3
"""Residue-class counts and a prime race (class a against class b mod q): the primes on the host
and a numpy cumsum against the device kernels.

  (a) dse_sieve_all + dse_primes_resident + numpy (bincount of v mod q, cumsum of +-1 over the
      entries of the two classes, argmax / argmin): the only route before dse_race_*; skipped above
      --host-max. Its numbers must equal the device's. It also says which share of the words that
      hold a step the main kernel's fast path decides (the sign of D cannot change inside them).
  (b) dse_sieve_all + Context.resident_race()               (one dse_race to the host)
  (c) the three race launches alone (HIP events) on a mask sieved into device memory
  (c1) the count and closing launches alone (a == b: counts only), same mask
  (s) the two statistics launches (tools/stats_bench.py's (c), 7 patterns) on the same mask: the
      yardstick, a kernel with the same per-tile scan
  (d) a device-to-device copy of the mask's bytes

With --P above 1 (all chunks on one device) only (b) runs: the chunks' class counts first, then the
races chained through their d_end.

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. The record is printed and written to --out.

The prime 2 is in no mask: a race that involves its class (2 mod q, q odd) starts from --d-start -1
(or 1) to count it.

  python tools/race_bench.py [--n 1000000000] [--P 1] [--q 4 --a 1 --b 3] [--d-start 0] [--reps 5]
                             [--step-limit 300] [--host-max 2000000000] [--out FILE] [--append]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from bench_common import ROOT, Record, events, ms, step_limit, timed  # also: the package path, DSE_LIB


def host_numbers(np, primes, q, a, b, d_start=0):
    """From the primes as values: (counts, the race's numbers as a dict, the fast-path share)."""
    v = primes.astype(np.int64)
    cls = v % q
    counts = np.bincount(cls, minlength=q)
    step = (cls == a) | (cls == b)
    sv = v[step]
    up = cls[step] == a
    D = d_start + np.cumsum(np.where(up, 1, -1), dtype=np.int64)
    r = {"steps": int(len(D)), "a_ahead": int((D > 0).sum()), "b_ahead": int((D < 0).sum()), "ties": int((D == 0).sum()),
         "first_a_ahead": int(sv[np.argmax(D > 0)]) if (D > 0).any() else None,
         "first_b_ahead": int(sv[np.argmax(D < 0)]) if (D < 0).any() else None,
         "max_d": int(D.max()), "max_at": int(sv[np.argmax(D)]), "min_d": int(D.min()), "min_at": int(sv[np.argmin(D)]),
         "d_end": int(D[-1])}
    # per mask word that holds a step: D at its start, its steps up and down; the sign is decided when
    # D0 > steps down or -D0 > steps up (csrc/dse_race_word.h race_same_sign)
    word = (sv - 3) >> 7
    first = np.flatnonzero(np.concatenate([[True], word[1:] != word[:-1]]))
    d0 = np.concatenate([[d_start], D])[first]
    na = np.add.reduceat(up.astype(np.int64), first)
    nb = np.add.reduceat((~up).astype(np.int64), first)
    fast = (d0 > nb) | (-d0 > na)
    return counts, r, float(fast.mean()), int(len(first))


def race_numbers(r):
    return {k: getattr(r, k) for k in ("steps", "a_ahead", "b_ahead", "ties", "first_a_ahead", "first_b_ahead", "max_d",
                                       "max_at", "min_d", "min_at", "d_end")}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--P", type=int, default=1)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--a", type=int, default=1)
    ap.add_argument("--b", type=int, default=3)
    ap.add_argument("--d-start", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "race_gpu.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    N, P, lim, q, a, b, d0 = args.n, args.P, args.step_limit, args.q, args.a, args.b, args.d_start
    with_host = P == 1 and N <= args.host_max
    say = Record()
    say(f"race_bench: N={N} P={P} q={q} a={a} b={b} d_start={d0} reps={args.reps} device={torch.cuda.get_device_name(0)}"
        f" lib={_dse.LIB_PATH.rsplit('/', 1)[-1]}")
    cs = (N - 1) // 2 // P
    nbits = P * cs
    res = {}
    out = {"N": N, "P": P, "q": q, "a": a, "b": b, "d_start": d0, "reps": args.reps, "mask_bytes": P * ((cs + 63) // 64 * 8)}
    equal_ab = equal_c = True

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_b():
            ctx.sieve_all(N, P)
            res["b"] = ctx.resident_race(None, q, a, b, d0)

        with step_limit("sieve_all", lim):
            s_med, _ = timed(sieve_only, args.reps)
        say(f"sieve_all alone                               median {s_med * 1e3:10.2f} ms")
        with step_limit("(b) device race", lim):
            b_med, b_all = timed(path_b, args.reps)
        rc = res["b"]
        say(f"(b) sieve_all + resident_race()               median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}")
        say(f"    {rc!r}")
        say(f"    counts {[int(c) for c in rc.counts]}")
        out.update(sieve_all_ms=s_med * 1e3, b_device_ms=b_med * 1e3, counts=[int(c) for c in rc.counts], **race_numbers(rc))
        if with_host:
            def path_a():
                ctx.sieve_all(N, P)
                res["a"] = host_numbers(np, ctx.resident_primes(1), q, a, b, d0)

            with step_limit("(a) host arithmetic", lim):
                a_med, a_all = timed(path_a, args.reps)
            counts, r, share, words = res["a"]
            equal_ab = r == race_numbers(rc) and [int(c) for c in counts] == [int(c) for c in rc.counts]
            say(f"(a) sieve_all + resident_primes(1) + numpy    median {a_med * 1e3:10.2f} ms   all {ms(a_all)}")
            say(f"(a) == (b): {equal_ab}   (a) / (b) = {a_med / b_med:.1f}")
            say(f"    words that hold a step: {words}; the sign fast path decides {100 * share:.3f}% of them")
            out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / b_med, step_words=words, fast_path_share=share)
        out["numbers_equal"] = equal_ab

    if P == 1:
        # (c), (c1), (s), (d): the launches alone, on a mask sieved into device memory
        with S.Context(num_gpus=1) as ctx:
            limit = S.base_limit_for_range(0, nbits)
            table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
            mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
            copy = torch.zeros_like(mask)
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            dst = torch.zeros(_dse.RACE_WORDS, dtype=torch.int64, device="cuda")
            sdst = torch.zeros(_dse.STATS_WORDS, dtype=torch.int64, device="cuda")
            sp = torch.cuda.current_stream().cuda_stream
            with step_limit("sieve into device memory", lim):
                ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
                ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
                torch.cuda.synchronize()
                ctx.device_status()
            mb = mask.numel() * 8
            with step_limit("(c) race launches", lim):
                c_med, c_all = events(lambda: ctx.race_dev_async(0, nbits, mask.data_ptr(), q, a, b, d0, dst.data_ptr(), sp),
                                      args.reps)
                equal_c = bool(np.array_equal(dst.cpu().numpy().view(np.uint64), rc.words))
            with step_limit("(c1) count and closing launches", lim):
                c1_med, c1_all = events(lambda: ctx.race_dev_async(0, nbits, mask.data_ptr(), q, a, a, 0, dst.data_ptr(), sp),
                                        args.reps)
                equal_c = equal_c and bool(np.array_equal(dst.cpu().numpy().view(np.uint64)[17:], rc.words[17:]))
            with step_limit("(s) statistics launches", lim):
                st_med, st_all = events(lambda: ctx.stats_dev_async(0, nbits, mask.data_ptr(), S.CONSTELLATIONS,
                                                                    sdst.data_ptr(), sp), args.reps)
            with step_limit("(d) device-to-device copy", lim):
                d_med, d_all = events(lambda: copy.copy_(mask), args.reps)
            say(f"(c) race launches (count, main, close)  median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
                f"   ({nbits / c_med / 1e9:.1f} G candidates/s; two reads of the mask: {2 * mb / c_med / 1e9:.1f} GB/s);"
                f" equals (b): {equal_c}")
            say(f"(c1) count + close launches (a == b)    median {c1_med * 1e3:8.3f} ms   all {ms(c1_all, 3)}"
                f"   (mask read: {mb / c1_med / 1e9:.1f} GB/s)   main pass = (c) - (c1) = {(c_med - c1_med) * 1e3:.3f} ms")
            say(f"(s) statistics launches, 7 patterns     median {st_med * 1e3:8.3f} ms   all {ms(st_all, 3)}"
                f"   (c) / (s) = {c_med / st_med:.2f}")
            say(f"(d) device-to-device copy of the mask   median {d_med * 1e3:8.3f} ms   all {ms(d_all, 3)}"
                f"   ({mb / d_med / 1e9:.1f} GB/s read + as much written)   (c1) / (d) = {c1_med / d_med:.2f}")
            out.update(c_launches_ms=c_med * 1e3, c1_count_ms=c1_med * 1e3, main_pass_ms=(c_med - c1_med) * 1e3,
                       stats_launches_ms=st_med * 1e3, c_over_stats=c_med / st_med, d2d_copy_ms=d_med * 1e3,
                       count_over_copy=c1_med / d_med, launch_output_equal=equal_c)
    say(json.dumps(out))
    say()
    say.write(args.out, args.append)
    return 0 if equal_ab and equal_c else 1


if __name__ == "__main__":
    sys.exit(main())
