"""The sieve at the top of the range it accepts: values just below 2^62, base
primes up to M = 2^31 - 1 (kBigBaseLimitMax), and the base table pinned whole.

The references are independent of the kernels and of the C oracle:
deterministic Miller-Rabin in Python integers (tests/primes_ref.py) for every
window, an independent numpy sieve's count / last / SHA-256 for the table's
primes, Python-integer arithmetic for the Barrett factors and wheel offsets.
GOLDEN["top"] (make_golden.py --top) holds what the oracle computes for the
same things; the several-segment range is compared with it bit for bit.

The 2^31 - 1 table takes S.base_table_bytes(2**31 - 1) bytes (6.5 GB), so
this module owns its context and frees it at the end: the session-wide ctx
never builds it.
"""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from primes_ref import is_prime_mr, mask_bits, mr_window

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))

M = 2**31 - 1               # the last prime of the largest table (a Mersenne prime)
SEG = 1_966_080             # odd candidates per wheel segment (15 * 2^17)
W = 1 << 16                 # window of tests a-c
G_M2 = (M * M - 3) // 2 - (1 << 15)   # (a): M^2 = 2^62 - 2^32 + 1 in the middle
G_LAST = 2**61 - 1 - W      # (b): last index 2^61 - 2, value 2^62 - 1
NB_D = 5 * SEG + 777        # (d): ragged start and end, 6 segments
G_D = 2**61 - 1 - NB_D

# Odd primes <= limit: count, last, SHA-256 of the little-endian uint32 values,
# from a numpy segmented sieve independent of this project (the issue's figures).
PRIMES_REF = {
    10**9: (50_847_533, 999_999_937, "c9e48b9bd5c9785325539063d7eee9a8bd4335d46ba7d9c6ceb4afd0e0ba65e2"),
    M: (105_097_564, M, "d07523aece0b2d1ad87107f0537fe13a7e336d6b75aef24bf34271bd77dfcfd4"),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def top_ctx():
    from mail_sieve_e.sieve import Context
    c = Context(num_gpus=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref_last():
    """Miller-Rabin over the last legal window (b), computed once."""
    r = mr_window(G_LAST, W)
    r.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def table_m():
    """The 2^31 - 1 base table in a torch buffer (dse_base_primes_dev_async),
    built once for the module: {"t": uint8 tensor, "count", "cap"}."""
    import torch
    from mail_sieve_e import sieve as S
    from mail_sieve_e.sieve import Context
    t = torch.empty(S.base_table_bytes(M), dtype=torch.uint8, device="cuda")
    with Context(num_gpus=1) as c:
        c.base_primes_dev_async(M, t.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    hdr = t[:16].cpu().numpy()
    d = {"t": t, "count": int(hdr[:4].view(np.uint32)[0]), "cap": int(hdr[4:8].view(np.uint32)[0])}
    yield d
    d.clear()
    del t
    torch.cuda.empty_cache()


def _check_window(m, c, g0, nb, ref):
    bits = mask_bits(m, nb)
    bad = np.flatnonzero(bits != ref)
    assert len(bad) == 0, [(3 + 2 * (g0 + int(j)), bool(bits[j])) for j in bad[:8]]
    assert c == int(ref.sum())
    assert not mask_bits(m, 64 * len(m))[nb:].any()  # bits past nbits stay zero


def test_window_on_m_squared(top_ctx):
    """(a) 2^16 candidates centred on M^2: the whole mask and the count against
    Miller-Rabin, and the bit of M^2 on its own: of all sieving primes only the
    table's last one clears it, as its own first hit p^2. CPU figures: 2,990
    primes, the oracle and Miller-Rabin agree on every bit."""
    ref = mr_window(G_M2, W)
    assert int(ref.sum()) == 2990 and not ref[1 << 15]
    m, c = top_ctx.sieve_odd_range(G_M2, W)
    bits = mask_bits(m, W)
    assert 3 + 2 * (G_M2 + (1 << 15)) == M * M
    assert not bits[1 << 15], "M^2 = (2^31 - 1)^2 left set: the table's last prime did not mark its square"
    _check_window(m, c, G_M2, W, ref)


def test_last_legal_window(top_ctx, table_m, ref_last):
    """(b) the 2^16 candidates ending at 2^62 - 1 (last index 2^61 - 2) through
    dse_sieve_odd_range, dse_sieve_window (count) and dse_sieve_range_dev_async
    on a caller-owned table, against Miller-Rabin."""
    import torch
    assert 3 + 2 * (G_LAST + W - 1) == 2**62 - 1
    m, c = top_ctx.sieve_odd_range(G_LAST, W)
    _check_window(m, c, G_LAST, W, ref_last)
    assert top_ctx.sieve_window(2**62 - 2**17, 2**62 - 1) == int(ref_last.sum())
    mask = torch.zeros(W // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    top_ctx.sieve_range_dev_async(table_m["t"].data_ptr(), G_LAST, W, mask.data_ptr(), cnt.data_ptr(), sp)
    torch.cuda.synchronize()
    top_ctx.device_status()
    _check_window(mask.cpu().numpy().view(np.uint64), int(cnt.item()), G_LAST, W, ref_last)


def test_edge_of_acceptance(top_ctx, ref_last, tmp_path):
    """(c) one candidate further: a range whose largest value is 2^62 + 1 needs
    base primes to 2^31 and is refused with DSE_ERANGE by dse_sieve_odd_range,
    dse_sieve_window and dse_finish_range_file; after each refusal the same
    context still returns the last legal window."""
    from mail_sieve_e import _dse
    g_over = G_LAST + 1  # last index 2^61 - 1: value 2^62 + 1
    assert 3 + 2 * (g_over + W - 1) == 2**62 + 1
    calls = [lambda: top_ctx.sieve_odd_range(g_over, W),
             lambda: top_ctx.sieve_window(2**62 - 2**17, 2**62 + 1),
             lambda: top_ctx.finish_range(str(tmp_path / "primes2.txt"), 2, g_over, W)]
    for call in calls:
        with pytest.raises(_dse.DseError) as e:
            call()
        assert e.value.code == -6
        m, c = top_ctx.sieve_odd_range(G_LAST, W)
        _check_window(m, c, G_LAST, W, ref_last)


@pytest.fixture(scope="module")
def mr_cache():
    return {}


@pytest.mark.parametrize("option,value", [(None, 0), ("bucket_pass_segments", 3), ("bucket_split_log2", 20),
                                          ("bucket_split_log2", 63)])
def test_segments_at_the_top(top_ctx, mr_cache, option, value):
    """(d) 5 segments + 777 candidates ending at 2^62 - 1 (ragged start and
    end): with the production options, in passes of 3 segments, with every
    bucketed prime in band 1 (split 2^20) and with the split clamped to
    kFillMaxSplit (63). Count and mask SHA-256 against GOLDEN["top"] (the
    oracle), Miller-Rabin on 2,000 random bits, on the first 2,000 set bits and
    on the 2^12 candidates each side of every segment seam."""
    g = GOLDEN["top"]["segments"]
    assert (g["g0"], g["nb"]) == (G_D, NB_D) and 3 + 2 * (G_D + NB_D - 1) == 2**62 - 1
    if option:
        top_ctx.debug_set_option(option, value)
    try:
        m, c = top_ctx.sieve_odd_range(G_D, NB_D)
    finally:
        if option:
            top_ctx.debug_set_option(option, 0)
    bits = mask_bits(m, NB_D)
    rng = random.Random(62)
    idx = [rng.randrange(NB_D) for _ in range(2000)] + [int(j) for j in np.flatnonzero(bits)[:2000]]
    for s in range(1, 6):
        idx += range(s * SEG - 4096, min(s * SEG + 4096, NB_D))  # the last seam has 777 candidates after it
    for j in idx:
        if j not in mr_cache:
            mr_cache[j] = is_prime_mr(3 + 2 * (G_D + j))
        assert bool(bits[j]) == mr_cache[j], (option, value, 3 + 2 * (G_D + j))
    assert c == g["count"] == int(bits.sum())
    assert sha(m) == g["mask_sha256"]


def test_largest_passes_at_the_top(top_ctx, table_m):
    """8,192 + 2,049 segments ending at 2^62 - 1 (tests/golden/max_pass.json
    "max_top", the oracle's window sieve with base primes to 2^31 - 1) with the
    production options on the 2^31 - 1 table. The planner halves what would be
    passes of 8,192 and 6,145 segments (band-0 regions above 24 GiB) and runs
    4,096 + 3,072 + 3,073: where primes reach 2^31 a pass has the most entries
    a production pass has, 4.4e8 in band 1 and 1.7e9 in band 0, in the 32-bit
    sums of the bucket kernels, in 45 GiB of scratch. Every segment's primes,
    the count and a SHA-256 per 128 segments of mask (tests/max_pass_ref.py)."""
    import max_pass_ref as R
    e = R.FIX["max_top"]
    g0, nb = e["g0"], e["nb"]
    assert 3 + 2 * (g0 + nb - 1) == 2**62 - 1 and len(e["segment_counts"]) == R.MAX_PASS + 2049
    # read from the fixture, so that another range cannot quietly make the case small
    assert e["band1_entries"] > 2**30 and e["first_pass_band1_entries"] > 2**29
    R.need_device_memory(g0, nb)
    passes = R.planned_passes(g0, nb)
    assert [p[0] for p in passes] == [4096, 3072, 3073] and max(p[2] for p in passes) <= R.MAX_ENTRIES
    mask, c = R.sieve_dev(top_ctx, table_m["t"].data_ptr(), g0, nb)
    plan = tuple(top_ctx.debug_get_stat(k) for k in ("plan_bucket_passes", "plan_bucket_max_pass_segments",
                                                     "plan_bucket_max_lds_bytes"))
    assert plan == (3, 4096, R.stage_lds_bytes(4096)) and plan[2] == 33_408, plan
    R.check_entry(mask, c, e, passes=[p[0] for p in passes], what="8,192 + 2,049 segments ending at 2^62 - 1")


# ---- the base table, pinned whole ------------------------------------------

def _hash_primes(t, count, step=1 << 24):
    """SHA-256 of p[0..count) (little-endian uint32) and its last value, copied
    to the host slice by slice; also checks the slices ascend."""
    h = hashlib.sha256()
    last = 0
    for i in range(0, count, step):
        n = min(step, count - i)
        p = t[16 + 4 * i:16 + 4 * (i + n)].cpu().numpy().view("<u4")
        assert int(p[0]) > last and np.all(p[1:] > p[:-1])
        h.update(memoryview(p).cast("B"))
        last = int(p[-1])
    return h.hexdigest(), last


def test_golden_top_primes_agree():
    """The oracle's figures (GOLDEN["top"]) are the independent sieve's."""
    for name, limit in (("primes_1e9", 10**9), ("primes_2p31m1", M)):
        g = GOLDEN["top"][name]
        assert (g["count"], g["last"], g["values_sha256"]) == PRIMES_REF[limit] and g["limit"] == limit


def test_table_primes_1e9(top_ctx):
    import torch
    from mail_sieve_e import sieve as S
    limit = 10**9
    t = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    top_ctx.base_primes_dev_async(limit, t.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    count = int(t[:4].cpu().numpy().view(np.uint32)[0])
    assert count == PRIMES_REF[limit][0]
    assert _hash_primes(t, count)[::-1] == PRIMES_REF[limit][1:]


def test_table_primes_2p31m1(table_m):
    """Every one of the 105,097,564 odd primes <= 2^31 - 1, by hash."""
    assert table_m["count"] == PRIMES_REF[M][0] <= table_m["cap"]
    assert _hash_primes(table_m["t"], table_m["count"])[::-1] == PRIMES_REF[M][1:]


def _np_odd_primes_upto(n):
    s = np.ones(n // 2 + 1, dtype=bool)  # s[i]: 2i + 1
    s[0] = False
    for i in range(1, int(n ** 0.5) // 2 + 1):
        if s[i]:
            s[2 * i * (i + 1)::2 * i + 1] = False
    return 2 * np.flatnonzero(s) + 1


@pytest.fixture(scope="module")
def rows_ref():
    """p, m[] and a[] of every odd prime <= 2^20 in Python-integer arithmetic."""
    R30 = (1, 7, 11, 13, 17, 19, 23, 29)
    P = [int(p) for p in _np_odd_primes_upto(1 << 20)]
    assert len(P) == 82_024
    m = np.array([(2**64 - 1) // p for p in P], dtype=np.uint64)
    a = np.zeros((len(P), 8), dtype=np.uint32)
    for i, p in enumerate(P):
        if p < 7:
            continue
        inv = pow(30, -1, p)
        for j in range(8):
            k = (-R30[(j + i) & 7] * inv) % p
            a[i, j] = k
    i = len(P) - 1  # spot check of the formula itself: the least k >= 0 with p | R30[..] + 30 k
    assert all((R30[(j + i) & 7] + 30 * int(a[i, j])) % P[i] == 0 and a[i, j] < P[i] for j in range(8))
    return np.array(P, dtype=np.uint32), m, a


def _check_rows(t, cap, rows_ref):
    P, m, a = rows_ref
    n = len(P)
    m_off = (16 + 4 * cap + 7) & ~7
    a_off = (m_off + 8 * cap + 31) & ~31
    l_off = a_off + 32 * cap
    assert np.array_equal(t[16:16 + 4 * n].cpu().numpy().view(np.uint32), P)
    assert int(t[16 + 4 * n:16 + 4 * n + 4].cpu().numpy().view(np.uint32)[0]) > 1 << 20  # the rows end here
    got_m = t[m_off:m_off + 8 * n].cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got_m != m)
    assert len(bad) == 0, [(int(P[i]), int(got_m[i]), int(m[i])) for i in bad[:4]]
    got_a = t[a_off:a_off + 32 * n].cpu().numpy().view(np.uint32).reshape(n, 8)
    bad = np.flatnonzero((got_a != a).any(axis=1))
    assert len(bad) == 0, [(int(P[i]), got_a[i].tolist(), a[i].tolist()) for i in bad[:4]]
    for g in range(2):
        pl = t[l_off + 4 * cap * g:l_off + 4 * cap * g + 4 * n].cpu().numpy().view(np.uint32)
        assert np.array_equal(pl & np.uint32(0xFFFFF), P), g
        assert not (pl >> np.uint32(31)).any(), g


def test_table_rows_limit_above_2p20(top_ctx, rows_ref):
    """m[], a[] and pl[] of every prime <= 2^20 (not samples) in the table for
    limit 1,048,583, whose last prime is the first one without a row.
    wheel_offsets_kernel fills indices [0, n_rows), n_rows = the table's primes
    <= kWheelMaxPrime = 2^20 (82,024 odd primes): each thread of its
    grid-stride loop stops at its first prime above 2^20, and p[] ascends.
    m[i] = (2^64 - 1) // p; a[8i + j] = (-R30[(j + i) & 7] / 30) mod p (0 for
    p = 3, 5); pl[0][i], pl[1][i]: low 20 bits = p, bit 31 clear (the plan
    bits in between are not asserted)."""
    import torch
    from mail_sieve_e import sieve as S
    limit = 1_048_583
    t = torch.zeros(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    top_ctx.base_primes_dev_async(limit, t.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hdr = t[:16].cpu().numpy()
    count, cap = int(hdr[:4].view(np.uint32)[0]), int(hdr[4:8].view(np.uint32)[0])
    assert count == 82_025
    assert int(t[16 + 4 * 82_024:16 + 4 * 82_025].cpu().numpy().view(np.uint32)[0]) == limit
    _check_rows(t, cap, rows_ref)


def test_table_rows_inside_2p31m1(table_m, rows_ref):
    """The same rows, factors and pl[] words inside the 2^31 - 1 table (its
    capacity moves every region's offset past 2^31 bytes)."""
    _check_rows(table_m["t"], table_m["cap"], rows_ref)
