"""Where the prime gaps are, on the GPU (csrc/dse_gaps.hip): the first occurrence of
every gap of a device-resident mask as one dse_gaps, through dse_gaps_dev_async
(torch tensors), dse_gaps_range and dse_gaps_resident (host results, the chunks'
results merged on the host).

Expected values are numpy on bool arrays (tests/gaps_ref.py), with the bits from
the test's own patterns, from a numpy sieve, from Miller-Rabin (tests/primes_ref.py)
or from dse_copy_chunk_mask, and published first occurrences and maximal gaps;
never from the gaps code. Every word of the struct is compared, exactly. The
planted cases put two occurrences of one gap where waves of a workgroup are a
barrier apart; each runs under the default grid and under caps of 1 and 3
workgroups.
"""
import ctypes

import numpy as np
import pytest

import gaps_ref as R
from primes_ref import mask_bits, mr_window

pytestmark = pytest.mark.gpu
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD, SKEW = 5, 64, 3
GRIDS = (0, 1, 3)


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def gctx(S):
    """A context of this module's own: the tests change its gaps_grid."""
    with S.Context(num_gpus=1) as c:
        yield c


@pytest.fixture(scope="module")
def T(gctx):
    return gctx.debug_get_stat("gaps_tile_bits")


def to_dev(torch, mask):
    """The mask SKEW words into a larger 0xA5-filled tensor -> (tensor, pointer to the mask)."""
    m = np.ascontiguousarray(mask).view(np.int64)
    big = torch.full((SKEW + len(m) + 2,), A5_I64, dtype=torch.int64, device="cuda")
    big[SKEW:SKEW + len(m)] = torch.from_numpy(m.copy()).cuda()
    return big, big.data_ptr() + 8 * SKEW


def guarded(torch):
    return torch.full((LEAD + R.WORDS + GUARD,), A5_I64, dtype=torch.int64, device="cuda")


def device_gaps(torch, ctx, g_start, nbits, mptr, stream=0):
    """One call on the device mask at mptr into an 0xA5-filled tensor with guards on both sides -> the words."""
    buf = guarded(torch)
    ctx.gaps_dev_async(g_start, nbits, mptr, buf.data_ptr() + 8 * LEAD, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all(), "wrote outside the dse_gaps"
    return h[LEAD:LEAD + R.WORDS]


def check_all_grids(torch, S, ctx, bits, g, what, garbage=True, grids=GRIDS):
    """bits at g_start g under every grid against the reference and the host hook -> the reference."""
    mask = R.pack_garbage(bits) if garbage else R.pack(bits)
    want = R.brute(bits, g)
    assert not R.diff(S.gaps_host(mask, g, len(bits)).words, want), what
    keep, mptr = to_dev(torch, mask)
    try:
        for grid in grids:
            ctx.debug_set_option("gaps_grid", grid)
            got = device_gaps(torch, ctx, g, len(bits), mptr)
            assert not R.diff(got, want), (what, grid)
    finally:
        ctx.debug_set_option("gaps_grid", 0)
    del keep
    return want


def test_tile_constant_is_the_librarys(gctx, T):
    assert T == 256 * 64


# -- 1. the synthetic family --------------------------------------------------------------------
@pytest.mark.parametrize("k", range(9))
def test_synthetic_masks(torch, S, gctx, T, k):
    nbits = R.sizes(T)[k]
    for name, bits in R.masks(nbits, 7000 + nbits).items():
        for g in R.g_starts():
            check_all_grids(torch, S, gctx, bits, g, (nbits, name, g))


def test_empty_range(torch, gctx):
    got = device_gaps(torch, gctx, 17, 0, 0)
    assert not R.diff(got, R.brute(np.zeros(0, bool), 17))


@pytest.mark.parametrize("tiles,extra,grids", [(40, 3, (3, 7)), (1024, 0, (0,)), (1025, 0, (0,))])
def test_many_tiles(torch, S, gctx, T, tiles, extra, grids):
    rng = np.random.default_rng(tiles)
    nbits = tiles * T + extra
    bits = rng.random(nbits) < 1 / 24
    bits[5 * T - 700:5 * T + 800] = False  # an overflow gap over a tile seam
    bits[-1] = True
    want = check_all_grids(torch, S, gctx, bits, 2**40 + 5, (tiles, extra), grids=grids)
    assert int(want[8]) != R.NONE and int(want[5]) > 60


# -- 2. planted gaps: two occurrences a barrier apart ------------------------------------------------
@pytest.mark.parametrize("d", R.PLANTED_D)
def test_planted_twice_keeps_the_lower(torch, S, gctx, T, d):
    for name, bits in R.planted(T, d).items():
        idx = np.flatnonzero(bits)
        at = idx[:-1][np.diff(idx) == d]
        assert len(at) == 2, (d, name)
        want = check_all_grids(torch, S, gctx, bits, 11, (d, name), garbage=False)
        assert int(want[9 + d] if d < R.BINS else want[8]) == 11 + int(at[0]), (d, name)


def test_a_thousand_empty_tiles_inside_one_gap(torch, S, gctx, T):
    want = check_all_grids(torch, S, gctx, R.long_gap(T), 3, "long gap", garbage=False)
    assert int(want[6]) == 2 * (1001 * T + 17) and int(want[7]) == 3 + T // 2


# -- 3. stream order ------------------------------------------------------------------------------------
def test_stream_order(torch, gctx, S):
    """base table, sieve and the table enqueued on one non-default stream, no host sync between."""
    g0, nb = 0, 3 * 1966080 + 777
    limit = S.base_limit_for_range(g0, nb)
    table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((nb + 63) // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = guarded(torch)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    assert sp != 0
    gctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
    gctx.sieve_range_dev_async(table.data_ptr(), g0, nb, mask.data_ptr(), cnt.data_ptr(), sp)
    gctx.gaps_dev_async(g0, nb, mask.data_ptr(), buf.data_ptr() + 8 * LEAD, sp)
    s.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all()
    gctx.device_status()
    assert int(h[LEAD + 2]) == int(cnt.item())
    assert not R.diff(h[LEAD:LEAD + R.WORDS], R.brute(R.real_bits()[:nb], 0))


# -- 4. ranges of real primes -----------------------------------------------------------------------------
def test_range_below_21e6(gctx, S):
    bits = R.real_bits()
    try:
        for grid in GRIDS:
            gctx.debug_set_option("gaps_grid", grid)
            got = gctx.gaps_range(0, len(bits))
            assert not R.diff(got.words, R.real_brute()), grid
    finally:
        gctx.debug_set_option("gaps_grid", 0)
    fp = dict(got.first_primes())
    for gap, p in R.FIRST.items():
        assert fp[gap] == p, gap
    assert got.records() == R.RECORDS_21M
    assert gctx.gaps_window(0, R.REAL_LIMIT) == got and gctx.gaps_window(100, 50).nbits == 0


def test_range_at_1e15_and_at_the_top(gctx, S, T):
    for g0, nb in (((10**15 + 1 - 3) // 2, 2 * T + 100), (2**61 - 1 - 4096, 4096)):
        want = R.brute(mr_window(g0, nb), g0)
        try:
            for grid in GRIDS:
                gctx.debug_set_option("gaps_grid", grid)
                assert not R.diff(gctx.gaps_range(g0, nb).words, want), (g0, grid)
        finally:
            gctx.debug_set_option("gaps_grid", 0)
    from mail_sieve_e import _dse
    with pytest.raises(_dse.DseError) as e:
        gctx.gaps_range(2**61 - 10, 64)
    assert e.value.code == ERANGE


# -- 5. resident masks -----------------------------------------------------------------------------------
def test_records_1e9(ctx, S):
    ctx.sieve_all(10**9, 1)
    g, st = ctx.resident_gaps(), ctx.resident_stats(patterns=())
    assert g.records() == R.RECORDS_1E9 and len(R.RECORDS_1E9) == 29
    assert np.array_equal(g.first != np.uint64(R.NONE), st.gaps > 0) and g.found == 129
    assert (g.max_gap, g.max_gap_g, g.primes, g.first_g, g.last_g) == (st.max_gap, st.max_gap_g, st.primes,
                                                                       st.first_g, st.last_g)
    assert g.overflow_g is None and g == ctx.resident_gaps(1)
    fp = dict(g.first_primes())
    for gap, p in R.FIRST.items():
        assert fp[gap] == p, gap


def test_records_1e10_in_8_chunks(ctx, S):
    ctx.sieve_all(10**10, 8)
    g, st = ctx.resident_gaps(), ctx.resident_stats(patterns=())
    assert g.records() == R.RECORDS_1E10
    assert np.array_equal(g.first != np.uint64(R.NONE), st.gaps > 0)
    assert (g.max_gap, g.max_gap_g, g.primes) == (st.max_gap, st.max_gap_g, st.primes)


# (N, P, the primes of a first occurrence that a chunk seam cuts): found by a search over spread_work
SEAMS = ((467_821, 3, 155_921, 156_007), (961_761, 8, 360_653, 360_749))


@pytest.mark.parametrize("logical", [None, 3, 8])
def test_resident_chunks_and_seams(S, logical):
    with S.Context(num_gpus=1, logical=logical) as c:
        for N, P, p, q in SEAMS:
            chunks = S.spread_work(N, P)
            cs = (chunks[0][1] - chunks[0][0]) // 2
            bits = R.real_bits()[:P * cs]
            whole = R.brute(bits, 0)
            gp, gq = (p - 3) // 2, (q - 3) // 2
            # the shape still produces what the case is about: the first gap of its size, cut by a seam
            assert int(whole[9 + gq - gp]) == gp and gp // cs + 1 == gq // cs < P, (N, P)
            c.sieve_all(N, P)
            assert not R.diff(c.resident_gaps().words, whole), (N, P)
            per = []
            for k in range(1, P + 1):
                got = c.resident_gaps(k)
                assert not R.diff(got.words, R.brute(bits[(k - 1) * cs:k * cs], (k - 1) * cs)), (N, P, k)
                assert np.array_equal(mask_bits(c.copy_chunk_mask(N, P, k), cs), bits[(k - 1) * cs:k * cs])
                per.append(got)
            assert all(int(x.first[gq - gp]) != gp for x in per)  # no chunk has it: the merge's seam does
            assert not R.diff(c.gaps_range(0, P * cs).words, whole)


# -- 6. errors --------------------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf = guarded(torch)
        mp, op = m.data_ptr(), buf.data_ptr() + 8 * LEAD
        for code, args in [
            (EINVAL, (None, 0, 64, mp, op, None)),            # null ctx
            (EINVAL, (p, 0, 64, mp, None, None)),             # null result
            (EINVAL, (p, 0, 64, None, op, None)),             # null mask with nbits > 0
            (EINVAL, (p, 0, 64, mp, op + 4, None)),           # misaligned result
            (ERANGE, (p, 2**62 - 10, 64, mp, op, None)),      # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 64, mp, op, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, op, None)),        # more than 2^44 candidates
        ]:
            assert L.dse_gaps_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((buf == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(R.WORDS, A5, dtype=np.uint64)
        ho = _dse.u64p(hout)
        for code, args in [(EINVAL, (None, 0, 64, ho)), (EINVAL, (p, 0, 64, None)), (ERANGE, (p, 2**62 - 10, 64, ho)),
                           (ERANGE, (p, 0, 2**44 + 1, ho)),
                           (ERANGE, (p, 2**61, 64, ho))]:      # values above 2^62: dse_sieve_odd_range's rule
            assert L.dse_gaps_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, ho)), (EINVAL, (p, 1, ho)), (EINVAL, (p, 0, ho))]:
            assert L.dse_gaps_resident(*args) == code, args   # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, ho)), (EINVAL, (p, -1, ho)), (EINVAL, (p, 1, None))]:
            assert L.dse_gaps_resident(*args) == code, args
            assert (hout == A5).all(), args
        for bad in (1025, -1):
            with pytest.raises(_dse.DseError):
                c.debug_set_option("gaps_grid", bad)
        # and the context still works
        g = c.resident_gaps()
        assert (g.primes, g.first_g, 3 + 2 * g.last_g, g.max_gap, g.max_gap_prime) == (78497, 0, 999_983, 114, 492_113)
        assert not R.diff(device_gaps(torch, c, 0, 64, mp), R.brute(np.zeros(64, bool), 0))
