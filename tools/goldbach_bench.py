#!/usr/bin/env python3
"""Minimal Goldbach partitions at P=1: the mask on the host and a numpy loop over the small primes
against the device kernel.

  (a) dse_sieve_all + dse_copy_chunk_mask + a vectorised numpy loop over the small primes on the
      mask's uint64 words (shifted windows, the words that still hold an unresolved even kept as an
      index list): the only route before dse_goldbach_*; one run (--host-reps), skipped above
      --host-max. Its struct must equal the device's.
  (b) dse_sieve_all + Context.resident_goldbach()           (one dse_goldbach to the host)
  (c) the two Goldbach launches alone (HIP events) on a mask sieved into device memory
  (c0) the count-only launches of dse_primes_dev_async (out_cap = 0) on the same mask: one read of
       the same bytes, for scale

and the accounting of (c) from the histogram: the window tests the evens need one by one, the depth
a wave of 64 words x 64 evens has to walk when the ranks are independent draws from the histogram,
and the tests per second that (c) therefore ran.

One process; each figure is the median of --reps runs after one warm-up; every step runs under a
time limit of its own (--step-limit seconds): a step that overruns ends the process, and nothing
more is started on the GPU.

  python tools/goldbach_bench.py [--n 1000000000] [--reps 5] [--nprimes 0] [--step-limit 300]
                                 [--host-max 2000000000] [--launches-only]
"""
from __future__ import annotations

import argparse
import json
import sys
import time

from bench_common import events, ms, step_limit, timed  # also: the package path, DSE_LIB

WAVE_EVENS = 64 * 64


def small_h(count):
    """h_i = (P_i - 3) / 2 of the first `count` odd primes, by trial division."""
    ps, q = [], 3
    while len(ps) < count:
        if all(q % p for p in ps if p * p <= q):
            ps.append(q)
        q += 2
    return [(p - 3) // 2 for p in ps]


def host_goldbach(np, mask, nbits, nprimes):
    """The dse_goldbach words of [0, nbits) from the host mask: per small prime one shifted window
    over the words that still hold an unresolved even."""
    H = small_h(nprimes)
    words = (nbits + 63) // 64
    low = (H[-1] + 63) // 64 + 1
    W = np.zeros(low + words + 1, dtype=np.uint64)  # `low` zero words below candidate 0, one behind
    W[low:low + words] = mask[:words]
    if nbits % 64:
        W[low + words - 1] &= np.uint64((1 << (nbits % 64)) - 1)
    U = np.full(words, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    if nbits % 64:
        U[-1] = np.uint64((1 << (nbits % 64)) - 1)
    idx = np.arange(words, dtype=np.int64)  # the words with unresolved evens
    hist = np.zeros(2048, dtype=np.uint64)
    max_rank = max_c = (1 << 64) - 1
    for i, h in enumerate(H):
        if not len(idx):
            break
        q, s = -(-h // 64), (-h) % 64
        k = idx + (low - q)
        win = W[k] >> np.uint64(s)
        if s:
            win |= W[k + 1] << np.uint64(64 - s)
        hit = U[idx] & win
        nz = np.flatnonzero(hit)
        if len(nz):
            hist[i] = int(np.bitwise_count(hit[nz]).sum())
            w0 = int(hit[nz[0]])
            max_rank, max_c = i, int(idx[nz[0]]) * 64 + ((w0 & -w0).bit_length() - 1)
            U[idx[nz]] ^= hit[nz]
        if i % 8 == 7 or len(idx) < 4096:
            idx = idx[U[idx] != 0]
    out = np.zeros(8 + 2048, dtype=np.uint64)
    unres = int(np.bitwise_count(U).sum())
    first = (1 << 64) - 1
    if unres:
        w = int(np.flatnonzero(U)[0])
        first = w * 64 + ((int(U[w]) & -int(U[w])).bit_length() - 1)
    out[:8] = [0, nbits, nprimes, nbits - unres, unres, first, max_rank, max_c]
    out[8:] = hist
    return out


def accounting(np, hist, nbits):
    """From the histogram: tests if every even walked alone, and the expected depth of a wave of
    4096 evens whose ranks are independent draws from it."""
    h = hist.astype(np.float64)
    tot = h.sum()
    depth = np.arange(1, len(h) + 1)
    alone = float((h * depth).sum())               # an even of rank i needs i + 1 tests
    F = np.cumsum(h) / tot                          # P(rank <= d)
    top = int(np.flatnonzero(h)[-1])
    wave_depth = 1.0 + float((1.0 - F[:top] ** WAVE_EVENS).sum())   # E[max] + 1
    return {"mean_tests_per_even": alone / tot, "max_rank": top, "expected_wave_depth": wave_depth,
            "word_tests": wave_depth * ((nbits + 63) // 64)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--nprimes", type=int, default=0)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--host-max", type=int, default=2 * 10**9)
    ap.add_argument("--launches-only", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    N, P, lim, npr = args.n, 1, args.step_limit, args.nprimes
    n_eff = npr or _dse.GOLDBACH_PRIMES
    with_host = N <= args.host_max and not args.launches_only
    print(f"goldbach_bench: N={N} P={P} nprimes={n_eff} reps={args.reps} device={torch.cuda.get_device_name(0)}"
          f" lib={_dse.LIB_PATH.rsplit('/', 1)[-1]}")
    lo, hi = S.spread_work(N, P)[0]
    nbits = (hi - lo) // 2
    res = {}
    out = {"N": N, "P": P, "nprimes": n_eff, "reps": args.reps, "mask_bytes": (nbits + 63) // 64 * 8}
    equal_ab = True
    gb = None

    if not args.launches_only:
        with S.Context(num_gpus=1) as ctx:
            def sieve_only():
                ctx.sieve_all(N, P)

            def path_b():
                ctx.sieve_all(N, P)
                res["b"] = ctx.resident_goldbach(nprimes=npr)

            with step_limit("sieve_all", lim):
                s_med, _ = timed(sieve_only, args.reps)
            print(f"sieve_all alone                               median {s_med * 1e3:10.2f} ms")
            with step_limit("(b) device partitions", lim):
                b_med, b_all = timed(path_b, args.reps)
            gb = res["b"]
            print(f"(b) sieve_all + resident_goldbach()           median {b_med * 1e3:10.2f} ms   all {ms(b_all, 2)}")
            print(f"    evens {gb.nbits}  unresolved {gb.unresolved}  max prime {gb.max_prime} first at {gb.max_even}"
                  f"  hist[:6] {[int(v) for v in gb.hist[:6]]}")
            out.update(sieve_all_ms=s_med * 1e3, b_device_ms=b_med * 1e3, unresolved=gb.unresolved,
                       max_prime=gb.max_prime, max_even=gb.max_even)
            if with_host:
                def path_a():
                    ctx.sieve_all(N, P)
                    res["a"] = host_goldbach(np, ctx.copy_chunk_mask(N, P, 1), nbits, n_eff)

                with step_limit("(a) host loop", lim):
                    ts = []
                    for _ in range(args.host_reps):
                        t0 = time.perf_counter()
                        path_a()
                        ts.append(time.perf_counter() - t0)
                a_med = sorted(ts)[len(ts) // 2]
                equal_ab = bool(np.array_equal(res["a"], gb.words))
                print(f"(a) sieve_all + copy_chunk_mask + numpy loop  {args.host_reps} run(s), no warm-up"
                      f" {a_med * 1e3:10.2f} ms   all {ms(ts)}")
                print(f"(a) == (b): {equal_ab}   (a) / (b) = {a_med / b_med:.1f}")
                out.update(a_host_ms=a_med * 1e3, a_over_b=a_med / b_med)
            out["structs_equal"] = equal_ab

    # (c), (c0): the launches alone, on a mask sieved into device memory
    with S.Context(num_gpus=1) as ctx:
        limit = S.base_limit_for_range(0, nbits)
        table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
        mask = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.zeros(_dse.GOLDBACH_WORDS, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        with step_limit("sieve into device memory", lim):
            ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
            ctx.sieve_range_dev_async(table.data_ptr(), 0, nbits, mask.data_ptr(), cnt.data_ptr(), sp)
            torch.cuda.synchronize()
            ctx.device_status()
        mb = mask.numel() * 8
        with step_limit("(c) goldbach launches", lim):
            c_med, c_all = events(lambda: ctx.goldbach_dev_async(0, nbits, mask.data_ptr(), 0, 0, 0, npr,
                                                                 dst.data_ptr(), sp), args.reps)
            words = dst.cpu().numpy().view(np.uint64)
            equal_c = gb is None or bool(np.array_equal(words, gb.words))
        with step_limit("(c0) count only", lim):
            c0_med, c0_all = events(lambda: ctx.primes_dev_async(0, nbits, mask.data_ptr(), 0, 0, 0, tot.data_ptr(), sp),
                                    args.reps)
        acc = accounting(np, words[8:], nbits)
        print(f"(c) goldbach launches                median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
              f"   ({nbits / c_med / 1e9:.2f} G evens/s); equals (b): {equal_c}")
        print(f"(c0) count-only launches (one read)  median {c0_med * 1e3:8.3f} ms   all {ms(c0_all, 3)}"
              f"   (mask read: {mb / c0_med / 1e9:.1f} GB/s)   (c) / (c0) = {c_med / c0_med:.1f}")
        print(f"    accounting: max rank {acc['max_rank']}, tests per even walking alone {acc['mean_tests_per_even']:.2f},"
              f" expected depth of a wave of {WAVE_EVENS} evens {acc['expected_wave_depth']:.1f}")
        print(f"    word tests (depth x words) {acc['word_tests']:.3e} -> {acc['word_tests'] / c_med / 1e9:.1f} G word tests/s"
              f" = {acc['word_tests'] / 64 / c_med / 1e9:.2f} G wave tests/s")
        out.update(c_launches_ms=c_med * 1e3, c0_floor_ms=c0_med * 1e3, launch_output_equal=equal_c,
                   evens_per_s=nbits / c_med, **acc, word_tests_per_s=acc["word_tests"] / c_med)
    print(json.dumps(out))
    return 0 if equal_ab and equal_c else 1


if __name__ == "__main__":
    sys.exit(main())
