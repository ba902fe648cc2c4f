#!/usr/bin/env python3
"""End-to-end time of primes1.txt at N=1e9, P=1: host finish against device finish.

  (a) dse_sieve_all + dse_copy_chunk_mask + dse_write_primes_file   (the host writer's path)
  (b) dse_sieve_all + dse_finish_resident_file                      (text formatted on the GPU)
  (c) the three finish launches alone (HIP events), one slab that fills a 64 MiB text buffer
  (d) the D2H copy of that slab's text alone (HIP events, pinned host memory)

Each figure is the median of --reps runs after one warm-up. The files of (a)
and (b) must have the same SHA-256. (c) is also given as text GB/s next to
the 8 TB/s HBM figure of DESIGN.md section 6. Run on one box; the files go to
--dir (default: the system temporary directory), whose filesystem is printed.

  python tools/finish_bench.py [--n 1000000000] [--reps 5] [--dir DIR]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import tempfile

from bench_common import events, ms, timed  # also: the package path, DSE_LIB

HBM_TBS = 8.0
SLAB_BYTES = 64 << 20


def filesystem_of(path: str) -> str:
    best = ("", "unknown")
    try:
        for line in open("/proc/mounts"):
            _, mnt, fs = line.split()[:3]
            if os.path.realpath(path).startswith(mnt) and len(mnt) > len(best[0]):
                best = (mnt, fs)
    except OSError:
        pass
    return f"{best[1]} (mounted at {best[0] or '?'})"


def sha256_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    args = ap.parse_args()

    import numpy as np
    import torch

    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S

    N, P = args.n, 1
    L = _dse.lib()
    pa, pb = os.path.join(args.dir, "finish_bench_host.txt"), os.path.join(args.dir, "finish_bench_gpu.txt")
    print(f"finish_bench: N={N} P={P} reps={args.reps} device={torch.cuda.get_device_name(0)}")
    print(f"files in {args.dir}: {filesystem_of(args.dir)}")

    with S.Context(num_gpus=1) as ctx:
        def sieve_only():
            ctx.sieve_all(N, P)

        def path_a():
            ctx.sieve_all(N, P)
            m = ctx.copy_chunk_mask(N, P, 1)
            _dse.check(L.dse_write_primes_file(pa.encode(), 1, N, P, _dse.u64p(m)), "dse_write_primes_file")

        def path_b():
            ctx.sieve_all(N, P)
            ctx.finish_resident(pb, 1)

        s_med, _ = timed(sieve_only, args.reps)
        a_med, a_all = timed(path_a, args.reps)
        b_med, b_all = timed(path_b, args.reps)
        size = os.path.getsize(pa)
        ha, hb = sha256_file(pa), sha256_file(pb)
        print(f"sieve_all alone                       median {s_med * 1e3:10.2f} ms")
        print(f"(a) sieve_all + copy mask + host writer median {a_med * 1e3:10.2f} ms   all {ms(a_all)}")
        print(f"(b) sieve_all + finish_resident         median {b_med * 1e3:10.2f} ms   all {ms(b_all)}")
        print(f"file: {size} bytes; sha256 (a) {ha}")
        print(f"                    sha256 (b) {hb}   equal: {ha == hb}")

        # (c), (d): one slab of the chunk's mask whose text fills the pipeline's buffer
        cs = S.spread_work(N, P)[0]
        nbits_all = (cs[1] - cs[0]) // 2
        mask = torch.from_numpy(ctx.copy_chunk_mask(N, P, 1).view(np.int64)).cuda()
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        flags = S.FINISH_DOUBLES | S.FINISH_HACK

        def need(words):
            ctx.finish_text_dev_async(flags, 0, min(nbits_all, words * 64), mask.data_ptr(), 0, 0, 0, tot.data_ptr(), sp)
            torch.cuda.synchronize()
            return int(tot[1])

        words = min(mask.numel(), SLAB_BYTES // 128)
        for _ in range(4):  # grow the slab until its text fills the buffer
            words = min(mask.numel(), int(words * (SLAB_BYTES * 0.99) / max(need(words), 1)))
        while need(words) > SLAB_BYTES:
            words -= max(words // 200, 1)
        nbits, text_bytes = min(nbits_all, words * 64), need(words)
        text = torch.empty(SLAB_BYTES, dtype=torch.uint8, device="cuda")
        pinned = torch.empty(SLAB_BYTES, dtype=torch.uint8).pin_memory()

        c_med, c_all = events(lambda: ctx.finish_text_dev_async(flags, 0, nbits, mask.data_ptr(), 0, text.data_ptr(),
                                                                SLAB_BYTES, tot.data_ptr(), sp), args.reps)
        d_med, d_all = events(lambda: pinned[:text_bytes].copy_(text[:text_bytes], non_blocking=True), args.reps)
        assert int(tot[1]) == text_bytes
        want = open(pa, "rb").read(text_bytes)
        slab_ok = pinned[:text_bytes].numpy().tobytes() == want
        gbs = text_bytes / c_med / 1e9
        print(f"slab: {words} mask words, {int(tot[0])} entries, {text_bytes} text bytes; equals the file's head: {slab_ok}")
        print(f"(c) size + scan + emit launches  median {c_med * 1e3:8.3f} ms   all {ms(c_all, 3)}"
              f"   {gbs:.1f} GB/s of text ({gbs / (HBM_TBS * 1e3):.4f} of the {HBM_TBS:g} TB/s HBM figure)")
        print(f"(d) D2H copy of the slab's text  median {d_med * 1e3:8.3f} ms   all {ms(d_all, 3)}"
              f"   {text_bytes / d_med / 1e9:.1f} GB/s")
        print(f"(b) < (a): {b_med < a_med}   (c) < (d): {c_med < d_med}")
        print(json.dumps({"N": N, "P": P, "reps": args.reps, "file_bytes": size, "sha256_equal": ha == hb,
                          "sieve_all_ms": s_med * 1e3, "a_host_ms": a_med * 1e3, "b_gpu_ms": b_med * 1e3,
                          "slab_text_bytes": text_bytes, "c_kernels_ms": c_med * 1e3, "d_d2h_ms": d_med * 1e3,
                          "c_text_GBps": gbs, "slab_equals_file_head": slab_ok}))
    for p in (pa, pb):
        os.remove(p)
    return 0 if ha == hb and slab_ok else 1


if __name__ == "__main__":
    sys.exit(main())
