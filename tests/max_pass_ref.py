"""What the tests of bucketed passes at the planner's largest size share
(tests/test_gpu_max_pass.py, the max_top case of tests/test_gpu_top_of_range.py):
the fixtures of tests/golden/max_pass.json (make_golden.py --maxpass), the
device memory a pass takes by launch_bucketed's own layout, a sieve into a
torch tensor, per-segment prime counts by torch arithmetic alone, and the
comparison with a fixture entry. A plain module, like primes_ref.py.
"""
import hashlib
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "max_pass.json")))

SEG = 1_966_080                 # odd candidates per wheel segment (15 * 2^17)
SEG_WORDS = SEG // 64           # 30,720 mask words
SUP_SEGS = 128                  # segments per super-bucket (csrc kSupSegs) and per hashed piece of a fixture
MAX_PASS = 8192                 # segments of the planner's largest pass (csrc kBucketMaxSegs)
LDS_OPT_IN = 65_536             # dynamic LDS above this needs hipFuncSetAttribute(MaxDynamicSharedMemorySize)
assert FIX["seg_bits"] == SEG and FIX["piece_segments"] == SUP_SEGS and SEG % 64 == 0


def stage_lds_bytes(pass_segs):
    """4 * stage_lds_words(nsup) of csrc/dse_bucket.hip: nsup region cursors and,
    for each of the 4 waves, nsup stage fills and nsup stages of 64 keys."""
    nsup = -(-pass_segs // SUP_SEGS)
    return 4 * (nsup + 4 * nsup * 65)


# ---- launch_bucketed's planner and scratch, from its own formulas (csrc/dse_bucket.hip) ----

_SPAN = 30 << 17                # integers per segment
_GRID0, _GRID1, _THREADS = 1024, 4096, 256   # band-0 and band-1 workgroups, threads of each
_I_LO = {19: 43_389, 20: 82_024}   # odd primes <= 2^k: the table index of the first bucketed prime
MAX_ENTRIES = 2**31             # kBucketMaxEntries: band-1 capacity of a pass
MAX_REGION_BYTES = 24 << 30     # kBucketMaxRegionBytes: band-0 regions of a pass


def _bucket_cap(span, a, b):
    if b <= a:
        return 64
    la, lb = math.log(a), math.log(b)
    return int(8.0 * span / 30.0 * (math.log(lb / la) + 1.0 / (la * la)) + 8.0 * 1.25506 * b / lb) + 1024


def _bucket_k0(i_lo, a, b):
    if b <= a:
        return 0
    S = float(_GRID0 * _THREADS)
    n_band = 1.25506 * b / math.log(b) - i_lo
    lam, r = 0.0, 0.0
    while r * S < n_band:
        n = i_lo + r * S + 2
        lam += 8.0 * _SPAN / 30.0 * _THREADS / max(a, n * (math.log(n) + math.log(math.log(n)) - 1.0))
        r += 1
    return (int(lam + 10.0 * math.sqrt(lam + 4.0 * _THREADS) + 64.0) + 15) & ~15


def planned_passes(g0, nb, pass_segs=0, lo_log2=19, split_log2=28):
    """launch_bucketed's plan for the range under the options (0 / the defaults:
    production): [(segments, scratch bytes, band-1 capacity in entries, dynamic
    LDS bytes of the fill-and-stage launch)] per pass. A pass is the smaller of
    bucket_pass_segments (8,192 by default) and what is left, halved while its
    band-1 capacity passes 2^31 entries or its band-0 regions 24 GiB."""
    total = -(-nb // SEG)
    max_segs = pass_segs if 1 <= pass_segs < MAX_PASS else MAX_PASS
    root = math.isqrt(3 + 2 * (g0 + nb - 1))
    split, lo_p = float(min(2**split_log2, 30 << 24)), float(2**lo_log2)
    k0 = _bucket_k0(_I_LO[lo_log2], lo_p, min(split, float(root)))

    def al(x):
        return (x + 255) & ~255
    out, s0 = [], 0
    while s0 < total:
        ns = min(max_segs, total - s0)
        while ns > 1 and (_bucket_cap(ns * _SPAN, split, float(root)) > MAX_ENTRIES or 4 * ns * _GRID0 * k0 > MAX_REGION_BYTES):
            ns //= 2
        root_p = math.isqrt(3 + 2 * (g0 + min(nb, (s0 + ns) * SEG) - 1))
        band0, band1 = split > lo_p, split < root_p
        span = ns * _SPAN
        cap = _bucket_cap(span, split, float(root_p)) if band1 else 64
        spill_cap = _bucket_cap(span, lo_p, min(split, float(root_p))) if band0 else 0
        o_tot = 256 + 4 * _GRID1 * ns
        o_start = o_tot + 4 * ns + 256
        o_ent = al(o_start + 4 * (ns + 1))
        o_tmp = al(o_ent + 4 * cap)
        o_reg = al(o_tmp + 4 * cap) if band1 else al(o_tmp)
        o_n0 = al(o_reg + 4 * ns * _GRID0 * (k0 if band0 else 0))
        o_spill = al(o_n0 + (4 * ns * _GRID0 if band0 else 0))
        lds = max(4 * ns if band0 else 0, stage_lds_bytes(ns) if band1 else 0)
        out.append((ns, o_spill + 8 * spill_cap, cap, lds))
        s0 += ns
    return out


def need_device_memory(g0, nb, masks=1, **opts):
    """Skip the test (the only skip these tests have) when the device reports
    less free memory than the case takes: the scratch of its largest pass, its
    masks and 2 GiB for the counting and comparing temporaries."""
    import torch
    need = max(p[1] for p in planned_passes(g0, nb, **opts)) + masks * 8 * SEG_WORDS * -(-nb // SEG) + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the case takes {need / 1e9:.1f} GB of device memory ({need} bytes), {free / 1e9:.1f} GB are free")


# ---- sieve, count, compare -------------------------------------------------------

def sieve_dev(c, table_ptr, g0, nb):
    """dse_sieve_range_dev_async into a zeroed tensor of whole segments ->
    (int64 mask tensor, count). The context's status must be clean (no
    overflow flag) and bit 63 of the count clear."""
    import torch
    mask = torch.zeros(-(-nb // SEG) * SEG_WORDS, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.sieve_range_dev_async(table_ptr, g0, nb, mask.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c.device_status()
    count = int(cnt.item())
    assert count >= 0, f"bit 63 of the count is set: {count & (2**64 - 1):#x}"
    return mask, count


def segment_counts(mask):
    """Set bits of every SEG candidates of the device mask (SWAR popcount in
    torch int64; the masks after each arithmetic shift drop the copied sign
    bits), 512 segments at a time."""
    import torch
    rows = mask.view(-1, SEG_WORDS)
    out = []
    for r in range(0, rows.shape[0], 512):
        x = rows[r:r + 512]
        x = x - ((x >> 1) & 0x5555555555555555)
        x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
        x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0F
        out.append(((x * 0x0101010101010101) >> 56).sum(dim=1))
    return torch.cat(out).cpu().numpy()


def piece_hashes(host_mask, pieces):
    """SHA-256 of the pieces (SUP_SEGS segments of mask each, the last one up
    to the end) with the given indices, hashed side by side (hashlib releases
    the interpreter lock)."""
    pw = SUP_SEGS * SEG_WORDS
    raw = host_mask.view(np.uint8)
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda i: hashlib.sha256(raw[8 * pw * i:8 * pw * (i + 1)]).hexdigest(), pieces))


def check_entry(mask, count, e, nb=None, passes=None, what=""):
    """The device mask and count of e's range (or of its first nb candidates,
    whole segments) against the fixture entry: every segment's primes, the
    total, the returned count, nothing set past nb, and every piece's SHA-256
    from one host copy. passes: the segments of each pass (planned_passes), for
    the failure message."""
    g0 = e["g0"]
    whole = nb is None
    nb = e["nb"] if whole else nb
    nseg = -(-nb // SEG)
    words = (nb + 63) // 64
    assert whole or (nb % SEG == 0 and nb < e["nb"])   # a prefix of whole segments: pieces end on whole words
    want = np.array(e["segment_counts"][:nseg], dtype=np.int64)
    got = segment_counts(mask)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    if len(bad):
        s = int(bad[0])
        ends = np.cumsum(passes if passes else [nseg])
        p = int(np.searchsorted(ends, s, side="right"))
        in_pass = s - (int(ends[p - 1]) if p else 0)
        pytest.fail(f"{what}: segment {s} of the range (segment {in_pass} in super-bucket {in_pass // SUP_SEGS} of pass "
                    f"{p}, passes of {list(passes) if passes else [nseg]} segments, values from {3 + 2 * (g0 + s * SEG)}): "
                    f"{int(got[s])} primes, {int(want[s])} expected; {len(bad)} of {nseg} segments differ, "
                    f"the last one {int(bad[-1])}", pytrace=False)
    total = int(want.sum())
    assert total == (e["count"] if whole else sum(e["segment_counts"][:nseg]))
    assert int(got.sum()) == total == count, (what, int(got.sum()), total, count)
    assert not bool(mask[words:].any()), f"{what}: words past the range were written"
    host = mask[:words].cpu().numpy()
    npieces = -(-nseg // SUP_SEGS)
    assert npieces == (len(e["piece_sha256"]) if whole else nseg // SUP_SEGS)
    hashes = piece_hashes(host, range(npieces))
    badp = [i for i in range(npieces) if hashes[i] != e["piece_sha256"][i]]
    assert not badp, (f"{what}: the mask of piece {badp[0]} (the {SUP_SEGS} segments from {badp[0] * SUP_SEGS}) differs "
                      f"from the oracle's although every segment's count agrees; {len(badp)} of {npieces} pieces differ")
