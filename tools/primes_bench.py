#!/usr/bin/env python3
"""The primes of chunk 1 at N=1e9, P=1 as a uint64 array: host unpack against device extraction.

  (a) dse_sieve_all + dse_copy_chunk_mask + Chunk.primes()   (numpy unpack on the host: the only
                                                              route before dse_primes_*)
  (b) dse_sieve_all + Context.resident_primes(1)             (extracted on the GPU, slabs to the host)
  (c) the three launches alone (HIP events): size + scan + emit of the whole mask into device memory
  (c0) the size + scan launches alone (HIP events): a count-only call
  (d) a device-to-device copy of (c)'s output bytes (HIP events): the yardstick for (c), which
      cannot beat a plain copy of what it writes by much

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU. The arrays of (a) and (b) must be equal, and (c)'s output equal to them.

  python tools/primes_bench.py [--n 1000000000] [--reps 5] [--step-limit 120]
"""
from __future__ import annotations

import argparse
import json
import sys

from bench_common import events, ms, step_limit, timed  # also: the package path, DSE_LIB


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import sieve as S

    N, P, lim = args.n, 1, args.step_limit
    print(f"primes_bench: N={N} P={P} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    res = {}

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_a():
            ctx.sieve_all(N, P)
            ch = S.Chunk(lo, hi, mask=ctx.copy_chunk_mask(N, P, 1))
            res["a"] = ch.primes()

        def path_b():
            ctx.sieve_all(N, P)
            res["b"] = ctx.resident_primes(1)

        with step_limit("sieve_all", lim):
            s_med, _ = timed(sieve_only, args.reps)
        with step_limit("(a) host unpack", lim):
            a_med, a_all = timed(path_a, args.reps)
        with step_limit("(b) device extraction", lim):
            b_med, b_all = timed(path_b, args.reps)
        count = len(res["b"])
        equal_ab = bool(np.array_equal(res["a"].astype(np.uint64), res["b"]))
        out_bytes = 8 * count
        print(f"sieve_all alone                              median {s_med * 1e3:10.2f} ms")
        print(f"(a) sieve_all + copy mask + Chunk.primes()   median {a_med * 1e3:10.2f} ms   all {ms(a_all)}")
        print(f"(b) sieve_all + resident_primes(1)           median {b_med * 1e3:10.2f} ms   all {ms(b_all)}")
        print(f"values: {count} ({out_bytes / 1e6:.1f} MB); (a) == (b): {equal_ab}; last {int(res['b'][-1])}")

        # (c), (c0), (d): the launches on a device copy of the mask, into device memory
        mask = torch.from_numpy(ctx.copy_chunk_mask(N, P, 1).view(np.int64)).cuda()
        out = torch.zeros(count, dtype=torch.int64, device="cuda")
        dup = torch.empty_like(out)
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream

        with step_limit("(c) launches", lim):
            c_med, c_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, out.data_ptr(), count,
                                                               tot.data_ptr(), sp), args.reps)
            totals = [int(x) for x in tot.cpu()]
            equal_c = bool(np.array_equal(out.cpu().numpy().view(np.uint64), res["b"]))
        with step_limit("(c0) count only", lim):
            c0_med, c0_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, 0, 0, tot.data_ptr(), sp),
                                    args.reps)
        with step_limit("(d) device copy", lim):
            d_med, d_all = events(lambda: dup.copy_(out, non_blocking=True), args.reps)
            equal_d = bool(torch.equal(dup, out))
        ratio = c_med / d_med
        print(f"(c) size + scan + emit launches   median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
              f"   {out_bytes / c_med / 1e9:.1f} GB/s of values written; totals {totals}; equals (b): {equal_c}")
        print(f"(c0) size + scan alone            median {c0_med * 1e3:8.3f} ms   all {ms(c0_all, 3)}"
              f"   (mask read: {mask.numel() * 8 / c0_med / 1e9:.1f} GB/s)")
        print(f"(d) device-to-device copy, {out_bytes / 1e6:.1f} MB median {d_med * 1e3:8.3f} ms   all {ms(d_all, 3)}"
              f"   {out_bytes / d_med / 1e9:.1f} GB/s written; copy equal: {equal_d}")
        print(f"(b) < (a): {b_med < a_med}   (a) / (b) = {a_med / b_med:.2f}   (c) / (d) = {ratio:.2f}")
        print(json.dumps({"N": N, "P": P, "reps": args.reps, "values": count, "value_bytes": out_bytes,
                          "arrays_equal": equal_ab, "launch_output_equal": equal_c, "sieve_all_ms": s_med * 1e3,
                          "a_host_unpack_ms": a_med * 1e3, "b_device_ms": b_med * 1e3, "c_launches_ms": c_med * 1e3,
                          "c0_size_scan_ms": c0_med * 1e3, "d_copy_ms": d_med * 1e3, "c_over_d": ratio}))
    return 0 if equal_ab and equal_c and equal_d and totals == [count, count] else 1


if __name__ == "__main__":
    sys.exit(main())
