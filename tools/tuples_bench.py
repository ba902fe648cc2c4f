#!/usr/bin/env python3
"""Twins and sextuplets of a resident mask as values: the primes on the host and numpy against
the device kernels.

  (a) dse_primes_resident + numpy (differences of the prime values): the only route before
      dse_tuples_*; skipped above --host-max. Its lists must equal the device's.
  (b) Context.resident_tuples(): count, then every value to the host (end to end, on a mask that
      dse_sieve_all left resident; sieve_all's own time is printed beside it)
  (c) the three launches alone (HIP events) on a mask sieved into device memory: size + scan + emit
      of every match into device memory
  (c0) the size + scan launches alone: a count-only call
  (p0) the count-only call of dse_primes_dev_async on the same mask, in the same run: the yardstick,
       the same launches with the mask word in place of the match word

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. The record is printed and written to --out.

  python tools/tuples_bench.py [--n 1000000000] [--reps 5] [--step-limit 300] [--host-max 2000000000]
                               [--out FILE] [--append]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from bench_common import ROOT, Record, events, ms, step_limit, timed  # also: the package path, DSE_LIB


def host_matches(np, primes, require):
    """The lowest members of the matches of a forbid-free pattern, from the primes as values."""
    offs = [2 * j for j in range(1, 32) if (require >> j) & 1]
    # the first other member by differences over the whole array: p + o is the k-th prime after p, k <= o / 2
    hit = np.zeros(len(primes), bool)
    for k in range(1, offs[0] // 2 + 1):
        hit[:-k] |= (primes[k:] - primes[:-k]) == np.uint64(offs[0])
    cand = primes[hit]
    for o in offs[1:]:  # the others by binary search, for the few survivors
        want = cand + np.uint64(o)
        j = np.minimum(np.searchsorted(primes, want), len(primes) - 1)
        cand = cand[primes[j] == want]
    return cand


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "tuples_gpu.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    N, P, lim = args.n, 1, args.step_limit
    with_host = N <= args.host_max
    say = Record()
    say(f"tuples_bench: N={N} P={P} reps={args.reps} device={torch.cuda.get_device_name(0)}"
        f" lib={_dse.LIB_PATH.rsplit('/', 1)[-1]}")
    nbits = (N - 1) // 2
    pats = (("twins", S.TWINS), ("sextuplets", S.SEXTUPLETS))
    out = {"N": N, "P": P, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8}
    res = {}
    ok = True

    with S.Context(num_gpus=1) as ctx:
        with step_limit("sieve_all", lim):
            s_med, _ = timed(lambda: ctx.sieve_all(N, P), args.reps)
        say(f"sieve_all alone                                median {s_med * 1e3:10.2f} ms")
        out["sieve_all_ms"] = s_med * 1e3
        for name, pat in pats:
            def path_b():
                res[name] = ctx.resident_tuples(pat)

            with step_limit(f"(b) {name}", lim):
                b_med, b_all = timed(path_b, args.reps)
            v = res[name]
            say(f"(b) resident_tuples({name})".ljust(46) + f" median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}"
                f"   {len(v)} values ({8 * len(v) / 1e6:.2f} MB), first {[int(x) for x in v[:3]]}, last {int(v[-1])}")
            out[f"{name}_count"] = len(v)
            out[f"{name}_b_ms"] = b_med * 1e3
        if with_host:
            def path_a():
                p = ctx.resident_primes(1)
                for name, pat in pats:
                    res["host_" + name] = host_matches(np, p, pat)
                res["primes"] = len(p)

            with step_limit("(a) host arithmetic", lim):
                a_med, a_all = timed(path_a, args.reps)
            equal = all(np.array_equal(res["host_" + name], res[name]) for name, _ in pats)
            ok = ok and equal
            both = sum(out[f"{name}_b_ms"] for name, _ in pats) * 1e-3
            say(f"(a) resident_primes(1) + numpy, both patterns  median {a_med * 1e3:10.2f} ms   all {ms(a_all)}"
                f"   {res['primes']} primes ({8 * res['primes'] / 1e6:.1f} MB) cross the bus")
            say(f"(a) == (b): {equal}   (a) / (b, both patterns) = {a_med / both:.1f}")
            out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / both, lists_equal=equal)

    # (c), (c0), (p0): the launches alone, on a mask sieved into device memory
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()
        mb = mask.numel() * 8
        mp, tp = mask.data_ptr(), tot.data_ptr()
        with step_limit("(p0) primes count only", lim):
            p0_med, p0_all = events(lambda: ctx.primes_dev_async(0, nbits, mp, 0, 0, 0, tp, sp), args.reps)
        say(f"(p0) primes: size + scan alone".ljust(46) + f" median {p0_med * 1e3:8.3f} ms   all {ms(p0_all, 3)}"
            f"   (mask read: {mb / p0_med / 1e9:.1f} GB/s)")
        out["p0_primes_count_ms"] = p0_med * 1e3
        for name, pat in pats:
            n = out[f"{name}_count"]
            dst = torch.zeros(n, dtype=torch.int64, device="cuda")
            with step_limit(f"(c) {name} launches", lim):
                c_med, c_all = events(lambda: ctx.tuples_dev_async(0, nbits, mp, pat, 0, 0, 0, 0, 0, dst.data_ptr(), n, tp,
                                                                   sp), args.reps)
                totals = [int(x) for x in tot.cpu()]
                equal_c = totals == [n, n] and bool(np.array_equal(dst.cpu().numpy().view(np.uint64), res[name]))
            with step_limit(f"(c0) {name} count only", lim):
                c0_med, c0_all = events(lambda: ctx.tuples_dev_async(0, nbits, mp, pat, 0, 0, 0, 0, 0, 0, 0, tp, sp),
                                        args.reps)
            ok = ok and equal_c
            say(f"(c) {name}: size + scan + emit".ljust(46) + f" median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
                f"   ({nbits / c_med / 1e9:.1f} G candidates/s); equals (b): {equal_c}")
            say(f"(c0) {name}: size + scan alone".ljust(46) + f" median {c0_med * 1e3:8.3f} ms   all {ms(c0_all, 3)}"
                f"   (mask read: {mb / c0_med / 1e9:.1f} GB/s)   (c0) / (p0) = {c0_med / p0_med:.2f}")
            out.update({f"{name}_c_launches_ms": c_med * 1e3, f"{name}_c0_count_ms": c0_med * 1e3,
                        f"{name}_c0_over_p0": c0_med / p0_med, f"{name}_launch_output_equal": equal_c})
    say(json.dumps(out))
    say()
    say.write(args.out, args.append)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
