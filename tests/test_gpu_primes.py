"""Primes as numbers (csrc/dse_primes.hip): a device-resident mask compacted
into uint64 prime values on the GPU, through dse_primes_dev_async (torch
tensors), dse_primes_range and dse_primes_resident (host buffers, in slabs).

Expected values are numpy arithmetic on the same bits, 3 + 2 (g_start +
flatnonzero(bits)), with the bits from the test's own patterns, from the
oracle's CPU sieve, or from Miller-Rabin (tests/primes_ref.py); never from the
extractor. Every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

from mail_sieve_e._dse import PRIMES_TILE_BITS as T
from primes_ref import mask_bits, mr_window

pytestmark = pytest.mark.gpu
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pack(bits):
    """bool array -> uint64 mask words (zero past the end)."""
    by = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    out = np.zeros((len(bits) + 63) // 64 * 8, dtype=np.uint8)
    out[:len(by)] = by
    return out.view(np.uint64)


def values(bits, g_start):
    """uint64 values of the set bits (every one below 2^62: no wrap)."""
    return np.uint64(3) + np.uint64(2) * (np.uint64(g_start) + np.flatnonzero(bits).astype(np.uint64))


def to_dev(torch, mask):
    return torch.from_numpy(np.ascontiguousarray(mask).view(np.int64).copy()).cuda()


def device_primes(torch, ctx, g_start, nbits, m, first=0, cap=None, lead=3, guard=64):
    """Two calls on device mask m: the count alone (no buffer), then the values into an
    0xA5-filled tensor at element offset `lead` that holds exactly the values the call
    must write and a guard behind; -> (values, total, written)."""
    tot = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ctx.primes_dev_async(g_start, nbits, m.data_ptr(), first, 0, 0, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    total, w0 = (int(x) for x in tot.cpu())
    assert w0 == 0
    exact = max(total - first, 0)
    if cap is None:
        cap = exact
    want_written = min(cap, exact)
    buf = torch.full((lead + want_written + guard,), A5_I64, dtype=torch.int64, device="cuda")
    tot.fill_(-1)
    ctx.primes_dev_async(g_start, nbits, m.data_ptr(), first, (buf.data_ptr() + 8 * lead) if cap else 0, cap,
                         tot.data_ptr(), 0)
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [total, want_written], (first, cap)
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:lead] == A5).all() and (h[lead + want_written:] == A5).all(), "wrote outside [out, out + written)"
    return h[lead:lead + want_written], total, want_written


def test_tile_constant_is_the_librarys(ctx):
    assert ctx.debug_get_stat("primes_tile_bits") == T and T % 64 == 0


# -- 1. arbitrary masks ----------------------------------------------------------
# MANY tiles and more: the single-workgroup scan over the tile counts has 1,024 threads. At 1,024
# tiles every thread owns exactly one count; at 1,025 a thread owns two (or the last one, or none:
# the slices' ends are clamped), the smallest range at which a scan thread loops.
MANY = 1024 * T
NBITS = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37, 2**20 + 37, MANY, MANY + T + 37]


def patterns(nbits, seed):
    rng = np.random.default_rng(seed)
    if nbits >= MANY:  # about one bit in 1,000, so the values stay a few hundred KB; both ends set
        bits = rng.random(nbits) < 1 / 1000
        bits[0] = bits[-1] = True
        return {"thousandth": bits}
    out = {"half": rng.random(nbits) < 0.5, "twentieth": rng.random(nbits) < 1 / 20,
           "zero": np.zeros(nbits, bool), "ones": np.ones(nbits, bool)}
    for name, pos in (("first", 0), ("last", nbits - 1), ("seam-", T - 1), ("seam+", T)):
        if 0 <= pos < nbits:
            out[name] = np.zeros(nbits, bool)
            out[name][pos] = True
    return out


def g_starts(nbits):
    # 0; the value 2^32 + 1 (odd index 2^31 - 1) in the middle of the first tile; the last value 2^62 - 1
    return [0, 2**31 - 1 - min(nbits, T) // 2, 2**61 - 1 - nbits]


@pytest.mark.parametrize("nbits", NBITS)
def test_arbitrary_masks(torch, ctx, nbits):
    assert 8 * T > 2048 * 8  # an all-ones tile exceeds the 16 KiB staging window: the window loop runs
    for name, bits in patterns(nbits, 7000 + nbits).items():
        mask = pack(bits)
        if nbits % 64:  # garbage past nbits in the last word is ignored
            mask[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(nbits % 64)
        m = to_dev(torch, mask)
        for g in g_starts(nbits):
            want = values(bits, g)
            got, total, written = device_primes(torch, ctx, g, nbits, m)
            assert total == written == len(want), (name, g)
            assert np.array_equal(got, want), (name, g)
    g = g_starts(nbits)[2]
    assert int(values(np.ones(nbits, bool), g)[-1]) == 2**62 - 1


# -- 2. rank window ------------------------------------------------------------------
def test_rank_window(torch, ctx):
    nbits = 3 * T - 100
    bits = np.random.default_rng(21).random(nbits) < 0.5
    g = 10**9
    full = values(bits, g)
    total = len(full)
    cum = np.cumsum(bits)
    w = 300  # a word of the first tile's second half with at least three entries
    while bits[64 * w:64 * w + 64].sum() < 3:
        w += 1
    mid_word = int(cum[64 * w - 1]) + 1
    tile_first = int(cum[T - 1])  # the second tile's first rank
    m = to_dev(torch, pack(bits))
    for first in (0, 1, mid_word, tile_first, total - 1, total, total + 5):
        exact = max(total - first, 0)
        for cap in (0, 1, exact, exact - 1, 2**40):
            if cap < 0:
                continue
            got, tot, written = device_primes(torch, ctx, g, nbits, m, first=first, cap=cap)
            assert tot == total and written == min(cap, exact), (first, cap)
            assert np.array_equal(got, full[first:first + cap]), (first, cap)


# -- 3. stream order -------------------------------------------------------------------
def stream_sieve_then_primes(torch, ctx, S, g0, nb):
    """base table, sieve and extraction enqueued on one non-default stream, no host sync between."""
    limit = S.base_limit_for_range(g0, nb)
    table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((nb + 63) // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    cap = nb // 2 + 16
    out = torch.full((cap,), A5_I64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    assert sp != 0
    ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
    ctx.sieve_range_dev_async(table.data_ptr(), g0, nb, mask.data_ptr(), cnt.data_ptr(), sp)
    ctx.primes_dev_async(g0, nb, mask.data_ptr(), 0, out.data_ptr(), cap, tot.data_ptr(), sp)
    s.synchronize()
    total, written = (int(x) for x in tot.cpu())
    assert total == written == int(cnt.item())
    h = out.cpu().numpy().view(np.uint64)
    assert (h[written:] == A5).all()
    ctx.device_status()
    return h[:written]


def test_stream_order_from_zero(torch, ctx, S, oracle):
    nb = 3 * 1966080 + 777
    m_ref, c_ref = oracle.fast_sieve_range(0, nb)
    got = stream_sieve_then_primes(torch, ctx, S, 0, nb)
    assert len(got) == c_ref and np.array_equal(got, values(mask_bits(m_ref, nb), 0))


def test_stream_order_bucketed_window(torch, ctx, S):
    g0, nb = (10**18 + 1 - 3) // 2, 4096
    got = stream_sieve_then_primes(torch, ctx, S, g0, nb)
    assert np.array_equal(got, values(mr_window(g0, nb), g0))


# -- 4. resident chunks ------------------------------------------------------------------
@pytest.mark.parametrize("logical", [None, 3])
def test_resident_chunks(S, logical):
    from mail_sieve_e import _dse
    N, P = 10**8, 3
    cs = (N - 1) // 2 // P
    with S.Context(num_gpus=1, logical=logical) as c:
        counts, _, _ = c.sieve_all(N, P)
        for k in range(1, P + 1):
            bits = mask_bits(c.copy_chunk_mask(N, P, k), cs)
            got = c.resident_primes(k)
            assert got.dtype == np.uint64 and len(got) == int(counts[k - 1]), k
            assert np.array_equal(got, values(bits, (k - 1) * cs)), k
        c.sieve_all(10**6, 2)
        with pytest.raises(_dse.DseError) as e:
            c.resident_primes(3)
        assert e.value.code == EINVAL and "not resident" in str(e.value)
        assert [int(v) for v in c.resident_primes(1, first=0, count=4)] == [3, 5, 7, 11]


# -- 5. paging a large mask ----------------------------------------------------------------
def test_paging_1e9(ctx):
    from mail_sieve_e import _dse
    counts, _, _ = ctx.sieve_all(10**9, 1)
    tot, wr = ctypes.c_uint64(), ctypes.c_uint64(7)
    _dse.check(_dse.lib().dse_primes_resident(ctx.ptr, 1, 0, None, 0, ctypes.byref(tot), ctypes.byref(wr)), "count")
    total = tot.value
    assert total == 50_847_533 == int(counts[0]) and wr.value == 0
    assert [int(v) for v in ctx.resident_primes(1, first=total - 1, count=1)] == [999999937]
    assert [int(v) for v in ctx.resident_primes(1, first=0, count=4)] == [3, 5, 7, 11]
    assert len(ctx.resident_primes(1, first=total, count=3)) == 0


# -- 6. host entry points and slab seams -----------------------------------------------------
@pytest.mark.parametrize("slab", [1, 7, 1000])
def test_slab_seams(S, oracle, slab):
    from mail_sieve_e import _dse
    nb = 2**20 + 37
    with S.Context(num_gpus=1) as c:
        c.debug_set_option("primes_slab_entries", slab)
        for g0 in (0, 123456789):
            m_ref, c_ref = oracle.fast_sieve_range(g0, nb)
            want = values(mask_bits(m_ref, nb), g0)
            assert len(want) == c_ref
            got = c.primes_range(g0, nb, count=c_ref + 9)
            assert got.dtype == np.uint64 and np.array_equal(got, want), g0
            # windows that start and end inside a slab, at a slab's start, past the end
            for first, count in ((0, 1), (3, 5), (slab, slab), (slab + slab // 2 + 1, 2 * slab + 1), (5 * slab - 1, 30),
                                 (c_ref - 10, None), (c_ref - 3, 100), (c_ref, None), (c_ref + 5, 4)):
                got = c.primes_range(g0, nb, first=first, count=count)
                hi = c_ref if count is None else first + count
                assert np.array_equal(got, want[first:hi]), (g0, first, count)
        with pytest.raises(_dse.DseError):
            c.debug_set_option("primes_slab_entries", -1)


def test_primes_window_matches_sieve_window(ctx):
    for lo, hi in ((10, 1000), (11, 999), (10, 999), (11, 1000), (1, 100), (0, 2), (2, 3), (3, 3), (4, 4), (100, 50),
                   (10**12, 10**12 + 10**5)):
        got = ctx.primes_window(lo, hi)
        assert got.dtype == np.uint64 and len(got) == ctx.sieve_window(lo, hi), (lo, hi)
        a = max(lo, 3) | 1
        if hi >= a:
            nb = ((hi if hi & 1 else hi - 1) - a) // 2 + 1
            assert np.array_equal(got, values(mr_window((a - 3) // 2, nb), (a - 3) // 2)), (lo, hi)
        else:
            assert len(got) == 0


# -- 7. errors -----------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        out = torch.full((64,), A5_I64, dtype=torch.int64, device="cuda")
        mp, tp, op = m.data_ptr(), tot.data_ptr(), out.data_ptr()
        dev_cases = [
            (EINVAL, (None, 0, 64, mp, 0, op, 8, tp, None)),             # null ctx
            (EINVAL, (p, 0, 64, mp, 0, op, 8, None, None)),              # null totals
            (EINVAL, (p, 0, 64, None, 0, op, 8, tp, None)),              # null mask with nbits > 0
            (EINVAL, (p, 0, 64, mp, 0, None, 8, tp, None)),              # null out with a capacity
            (EINVAL, (p, 0, 64, mp, 0, op + 4, 8, tp, None)),            # misaligned out
            (ERANGE, (p, 2**62 - 10, 64, mp, 0, op, 8, tp, None)),       # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 64, mp, 0, op, 8, tp, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, 0, op, 8, tp, None)),         # more than 2^44 candidates
        ]
        for code, args in dev_cases:
            assert L.dse_primes_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((out == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(64, A5, dtype=np.uint64)
        t, w = ctypes.c_uint64(), ctypes.c_uint64()
        tw = (ctypes.byref(t), ctypes.byref(w))
        ho = _dse.u64p(hout)
        range_cases = [
            (EINVAL, (None, 0, 64, 0, ho, 8) + tw),
            (EINVAL, (p, 0, 64, 0, None, 8) + tw),
            (ERANGE, (p, 2**62 - 10, 64, 0, ho, 8) + tw),
            (ERANGE, (p, 0, 2**44 + 1, 0, ho, 8) + tw),
            (ERANGE, (p, 2**61, 64, 0, ho, 8) + tw),                     # values above 2^62: dse_sieve_odd_range's rule
        ]
        for code, args in range_cases:
            assert L.dse_primes_range(*args) == code, args
            assert (hout == A5).all(), args
        resident_cases = [
            (EINVAL, (None, 1, 0, ho, 8) + tw),
            (EINVAL, (p, 1, 0, ho, 8) + tw),                             # nothing resident yet
        ]
        for code, args in resident_cases:
            assert L.dse_primes_resident(*args) == code, args
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 0, 0, ho, 8) + tw), (EINVAL, (p, 4, 0, ho, 8) + tw),
                           (EINVAL, (p, 1, 0, None, 8) + tw)]:
            assert L.dse_primes_resident(*args) == code, args
            assert (hout == A5).all(), args
        # and the context still works
        assert [int(v) for v in c.resident_primes(1, count=4)] == [3, 5, 7, 11]
        assert len(c.resident_primes(1)) + len(c.resident_primes(2)) + len(c.resident_primes(3)) == 78497
