#!/usr/bin/env python3
"""Residue pairs of consecutive primes mod q at P=1: numpy on extracted primes against the device
matrix.

  (a) dse_sieve_all + Context.resident_primes(1) + numpy on the host (bincount of v[:-1] % q * q +
      v[1:] % q): the only route before dse_consec_*; "none" above --host-max (the values would not
      fit)
  (b) dse_sieve_all + Context.resident_consec()   (one dse_consec to the host)
  (c) the two consec launches alone (HIP events) on a mask sieved into device memory, at --q
  (cq) the same launches at q = 3, 4, 12, 30, 63: both in-word bodies and the threshold between them
  next to them, on the same mask:
  (c1) the two dse_stats launches with no pattern (the gap histogram and the maximal gap)
  (cp) a device-to-device copy of the mask: reads it once and writes it once, the floor
  --ab: the launches under the bit-parallel and under the per-entry body at every period both are
        built for (T = 2 .. 6), the test option "consec_body"; written to --ab-out

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. (a), (b) and (c) must be equal, the row sums must be resident_race's
class counts less the last prime, and the A/B's two bodies must give the same words.

  python tools/consec_bench.py [--n 1000000000] [--q 10] [--reps 5] [--step-limit 120]
                               [--host-max 2000000000] [--out FILE] [--ab] [--ab-out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from bench_common import ROOT, Record, events, ms, step_limit, timed  # also: the package path, DSE_LIB

OTHER_QS = (3, 4, 12, 30, 63)
AB_QS = (4, 3, 8, 5, 12)  # the periods 2 .. 6


def host_matrix(np, primes, q):
    v = primes.astype(np.int64) % q
    return np.bincount(v[:-1] * q + v[1:], minlength=q * q).reshape(q, q).astype(np.uint64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--q", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "consec_gpu.txt"))
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "r20", "ab_consec_threshold.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    say = Record()
    N, P, q, lim = args.n, 1, args.q, args.step_limit
    with_host = N <= args.host_max
    say(f"consec_bench: N={N} P={P} q={q} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    res = {}
    out = {"N": N, "P": P, "q": q, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8}

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_a():
            ctx.sieve_all(N, P)
            res["a"] = host_matrix(np, ctx.resident_primes(1), q)

        def path_b():
            ctx.sieve_all(N, P)
            res["b"] = ctx.resident_consec(None, q)

        with step_limit("sieve_all", lim):
            s_med, _ = timed(sieve_only, args.reps)
        say(f"sieve_all alone                               median {s_med * 1e3:10.2f} ms")
        with step_limit("(b) device matrix", lim):
            b_med, b_all = timed(path_b, args.reps)
        c = res["b"]
        with step_limit("resident_race", lim):
            cls = ctx.resident_race(None, q, 1, 1).counts.astype(np.int64)
        say(f"(b) sieve_all + resident_consec()             median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}")
        say(f"    {c!r}")
        live = [r for r in range(q) if c.matrix[r].any() or c.matrix[:, r].any()]
        for r in live:
            say(f"    N({r:2d}, .) " + " ".join(f"{int(c.matrix[r, s]):12d}" for s in live))
        last = np.zeros(q, np.int64)
        last[(3 + 2 * c.last_g) % q] = 1
        ok_rows = bool(np.array_equal(c.matrix.astype(np.int64).sum(axis=1), cls - last))
        ok_rows = ok_rows and int(c.matrix.astype(np.int64).sum()) == c.pairs == c.primes - 1
        say(f"    row sums equal resident_race's class counts less the last prime, sum = pairs = primes - 1: {ok_rows}")
        out.update(sieve_all_ms=s_med * 1e3, b_device_ms=b_med * 1e3, primes=c.primes, pairs=c.pairs,
                   bytes_to_host=8 * _dse.CONSEC_WORDS)
        equal_ab = True
        if with_host:
            with step_limit("(a) host arithmetic", lim):
                a_med, a_all = timed(path_a, args.reps)
            equal_ab = bool(np.array_equal(res["a"], c.matrix))
            say(f"(a) sieve_all + resident_primes(1) + numpy    median {a_med * 1e3:10.2f} ms   all {ms(a_all)}"
                f"   ({8 * c.primes / 1e6:.1f} MB of values)")
            say(f"(a) == (b): {equal_ab}   (a) / (b) = {a_med / b_med:.1f}")
            out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / b_med)
        else:
            say(f"(a) the route before: none ({8 * c.primes / 1e9:.1f} GB of values)")
        out["numbers_equal"] = equal_ab and ok_rows

    # (c), (cq), (c1), (cp): the launches alone, on a mask sieved into device memory
    equal_c = True
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        copy = torch.zeros_like(mask)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.zeros(_dse.CONSEC_WORDS, dtype=torch.int64, device="cuda")
        sdst = torch.zeros(_dse.STATS_WORDS, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()

        def launches(qq):
            return events(lambda: ctx.consec_dev_async(0, nbits, mask.data_ptr(), qq, dst.data_ptr(), sp), args.reps)

        def words():
            return dst.cpu().numpy().view(np.uint64).copy()

        mb = mask.numel() * 8
        with step_limit("(c) consec launches", lim):
            c_med, c_all = launches(q)
            equal_c = bool(np.array_equal(words(), c.words))
        with step_limit("(c1) statistics launches, no patterns", lim):
            c1_med, c1_all = events(lambda: ctx.stats_dev_async(0, nbits, mask.data_ptr(), (), sdst.data_ptr(), sp),
                                    args.reps)
        with step_limit("(cp) device-to-device copy", lim):
            cp_med, cp_all = events(lambda: copy.copy_(mask), args.reps)
        say(f"(c)  consec launches, q = {q:2d} (T = {q if q & 1 else q // 2:2d})     median {c_med * 1e3:8.3f} ms   "
            f"all {ms(c_all, 3)}   (mask read: {mb / c_med / 1e9:.1f} GB/s); equals (b): {equal_c}")
        say(f"(c1) statistics launches, no pattern   median {c1_med * 1e3:8.3f} ms   all {ms(c1_all, 3)}"
            f"   (mask read: {mb / c1_med / 1e9:.1f} GB/s)")
        say(f"(cp) device-to-device copy (the floor) median {cp_med * 1e3:8.3f} ms   all {ms(cp_all, 3)}"
            f"   (read + write: {2 * mb / cp_med / 1e9:.1f} GB/s)")
        say(f"(c) / (c1) = {c_med / c1_med:.2f}   (c) / (cp) = {c_med / cp_med:.2f}")
        out.update(c_launches_ms=c_med * 1e3, c1_stats_no_patterns_ms=c1_med * 1e3, cp_copy_ms=cp_med * 1e3,
                   c_over_c1=c_med / c1_med, c_over_copy=c_med / cp_med)
        other = {}
        for qq in OTHER_QS:
            with step_limit(f"(cq) consec launches, q = {qq}", lim):
                m, a = launches(qq)
                w = words()
            ok = int(w[3]) == c.primes and int(w[7:].astype(np.int64).sum()) == c.pairs
            equal_c = equal_c and ok
            say(f"(cq) consec launches, q = {qq:2d} (T = {qq if qq & 1 else qq // 2:2d})     median {m * 1e3:8.3f} ms   "
                f"all {ms(a, 3)}   / (c1) = {m / c1_med:.2f}   / (cp) = {m / cp_med:.2f}   sums to pairs: {ok}")
            other[str(qq)] = m * 1e3
        out.update(cq_launches_ms=other, launch_output_equal=equal_c)

        if args.ab:
            ab = Record()
            ab(f"consec_bench --ab: N={N} reps={args.reps} device={torch.cuda.get_device_name(0)}")
            ab("the two consec launches under the test option consec_body: 1 = the bit-parallel body (S_c = (~w + "
               "((w & M_c) << 1)) & w, T^2 popcounts into registers), 2 = the per-entry body (one LDS add per pair)")
            try:
                for qq in AB_QS:
                    t = {}
                    w = {}
                    for body in (1, 2):
                        ctx.debug_set_option("consec_body", body)
                        with step_limit(f"A/B q = {qq} body {body}", lim):
                            t[body], _ = launches(qq)
                            w[body] = words()
                    same = bool(np.array_equal(w[1], w[2]))
                    equal_c = equal_c and same
                    ab(f"q = {qq:2d}  T = {qq if qq & 1 else qq // 2}   bit-parallel {t[1] * 1e3:8.3f} ms   per-entry "
                       f"{t[2] * 1e3:8.3f} ms   bit-parallel / per-entry = {t[1] / t[2]:.2f}   same words: {same}")
            finally:
                ctx.debug_set_option("consec_body", 0)
            ab()
            ab.write(args.ab_out, append=True)
    say(json.dumps(out))
    say()
    say.write(args.out, append=True)
    return 0 if out["numbers_equal"] and equal_c else 1


if __name__ == "__main__":
    sys.exit(main())
