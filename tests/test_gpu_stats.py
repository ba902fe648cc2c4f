"""Statistics of a mask on the GPU (csrc/dse_stats.hip): constellation counts,
the gap histogram and the maximal gap of a device-resident mask as one
dse_stats, through dse_stats_dev_async (torch tensors), dse_stats_range and
dse_stats_resident (host results, the chunks' results merged on the host).

Expected values are numpy brute force on bool arrays (tests/stats_ref.py), with
the bits from the test's own patterns, from the oracle's CPU sieve, from
Miller-Rabin (tests/primes_ref.py) or from dse_copy_chunk_mask; never from the
statistics code. Every member of the struct is compared, exactly.
"""
import ctypes

import numpy as np
import pytest

import stats_ref as R
from primes_ref import mask_bits, mr_window

pytestmark = pytest.mark.gpu
T = 256 * 64
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD = 5, 64


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def sctx(S):
    """A context of this module's own: the tests change its stats_grid."""
    with S.Context(num_gpus=1) as c:
        yield c


def to_dev(torch, mask):
    return torch.from_numpy(np.ascontiguousarray(mask).view(np.int64).copy()).cuda()


def guarded(torch):
    return torch.full((LEAD + R.WORDS + GUARD,), A5_I64, dtype=torch.int64, device="cuda")


def device_stats(torch, ctx, g_start, nbits, m, pats, stream=0):
    """One call on device mask m into an 0xA5-filled tensor with guards on both sides -> the struct's words."""
    buf = guarded(torch)
    ctx.stats_dev_async(g_start, nbits, m.data_ptr() if m is not None else 0, pats, buf.data_ptr() + 8 * LEAD, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all(), "wrote outside the dse_stats"
    return h[LEAD:LEAD + R.WORDS]


def test_tile_constant_is_the_librarys(sctx):
    assert sctx.debug_get_stat("stats_tile_bits") == T


# -- 1. arbitrary masks -------------------------------------------------------------------
@pytest.mark.parametrize("nbits", R.sizes(T) + [2**20 + 37])
def test_arbitrary_masks(torch, sctx, nbits):
    try:
        for name, bits in R.masks(nbits, T, 9000 + nbits).items():
            m = to_dev(torch, R.pack_garbage(bits))
            for g in R.g_starts(nbits, T):
                for pats in R.PATTERN_LISTS:
                    want = R.brute(bits, g, pats)
                    for grid in (0, 1, 3):
                        sctx.debug_set_option("stats_grid", grid)
                        got = device_stats(torch, sctx, g, nbits, m, pats)
                        assert not R.diff(got, want), (name, g, pats, grid)
    finally:
        sctx.debug_set_option("stats_grid", 0)


def test_empty_range(torch, sctx):
    for pats in ((), (3, 1)):
        got = device_stats(torch, sctx, 17, 0, None, pats)
        assert not R.diff(got, R.brute(np.zeros(0, bool), 17, pats))


@pytest.mark.parametrize("gap", [3, 16, 17, 70, 1500])
def test_max_gap_tie_keeps_the_lower(torch, sctx, gap):
    try:
        for start in (0, 63, T - gap - 1, T - 1, 2 * T - 1):
            bits = np.zeros(4 * T + 5, bool)
            bits[[start, start + gap, start + gap + 1, start + 2 * gap + 1, start + 2 * gap + 3]] = True
            m = to_dev(torch, R.pack(bits))
            want = R.brute(bits, 7, (1,))
            assert int(want[24]) == 2 * gap and int(want[25]) == 7 + start
            for grid in (0, 1, 3):
                sctx.debug_set_option("stats_grid", grid)
                assert not R.diff(device_stats(torch, sctx, 7, len(bits), m, (1,)), want), (gap, start, grid)
    finally:
        sctx.debug_set_option("stats_grid", 0)


# -- 2. stream order ------------------------------------------------------------------------
def stream_sieve_then_stats(torch, ctx, S, g0, nb, pats):
    """base table, sieve and statistics enqueued on one non-default stream, no host sync between."""
    limit = S.base_limit_for_range(g0, nb)
    table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((nb + 63) // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = guarded(torch)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    assert sp != 0
    ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
    ctx.sieve_range_dev_async(table.data_ptr(), g0, nb, mask.data_ptr(), cnt.data_ptr(), sp)
    ctx.stats_dev_async(g0, nb, mask.data_ptr(), pats, buf.data_ptr() + 8 * LEAD, sp)
    s.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all()
    ctx.device_status()
    assert int(h[LEAD + 2]) == int(cnt.item())
    return h[LEAD:LEAD + R.WORDS]


def test_stream_order_from_zero(torch, sctx, S, oracle):
    nb = 3 * 1966080 + 777
    m_ref, c_ref = oracle.fast_sieve_range(0, nb)
    got = stream_sieve_then_stats(torch, sctx, S, 0, nb, S.CONSTELLATIONS)
    assert int(got[2]) == c_ref
    assert not R.diff(got, R.brute(mask_bits(m_ref, nb), 0, S.CONSTELLATIONS))


def test_stream_order_bucketed_window(torch, sctx, S):
    g0, nb = (10**18 + 1 - 3) // 2, 4096
    got = stream_sieve_then_stats(torch, sctx, S, g0, nb, S.CONSTELLATIONS)
    assert not R.diff(got, R.brute(mr_window(g0, nb), g0, S.CONSTELLATIONS))


# -- 3. resident chunks and seams ----------------------------------------------------------------
def resident_against_brute(c, S, N, P):
    """-> (merged Stats, per-chunk Stats); every one equal to brute force on the masks the context copies out."""
    cs = (N - 1) // 2 // P
    c.sieve_all(N, P)
    chunks = [mask_bits(c.copy_chunk_mask(N, P, k), cs) for k in range(1, P + 1)]
    merged = c.resident_stats()
    assert not R.diff(merged.words, R.brute(np.concatenate(chunks), 0, S.CONSTELLATIONS)), (N, P)
    per = []
    for k in range(1, P + 1):
        st = c.resident_stats(k)
        assert not R.diff(st.words, R.brute(chunks[k - 1], (k - 1) * cs, S.CONSTELLATIONS)), (N, P, k)
        per.append(st)
    return merged, per


@pytest.mark.parametrize("logical", [None, 3])
def test_resident_seams(S, logical):
    with S.Context(num_gpus=1, logical=logical) as c:
        # (N, P, the prime a straddling constellation starts at, its index in CONSTELLATIONS)
        for N, P, p0, which in ((1_636_885, 3, 1_091_257, 6), (1_003_261, 3, 334_421, 3), (1_247_153, 8, 1_091_257, 6)):
            cs = (N - 1) // 2 // P
            g = (p0 - 3) // 2
            span = S.CONSTELLATIONS[which].bit_length()
            assert g // cs < (g + span - 1) // cs < P, "the constellation straddles two chunks"
            merged, per = resident_against_brute(c, S, N, P)
            assert sum(st.matches[which] for st in per) < merged.matches[which], (N, P)
            assert sum(st.primes for st in per) == merged.primes


@pytest.mark.parametrize("logical", [None, 3])
def test_resident_1e8(S, logical):
    with S.Context(num_gpus=1, logical=logical) as c:
        merged, _ = resident_against_brute(c, S, 10**8, 3)
        assert merged.primes == 5_761_454
        assert merged.matches == [440312, 55600, 55556, 4768, 697, 686, 82]
        assert (merged.max_gap, merged.max_gap_prime) == (220, 47_326_693)
        assert [int(v) for v in merged.gaps[1:7]] == [440312, 440257, 768752, 334180, 430016, 538382]
        assert (merged.first, merged.last, merged.gap_overflow) == (3, 99_999_989, 0)


# -- 4. N = 1e9: anchors only -----------------------------------------------------------------------
def test_anchors_1e9(ctx, S):
    ctx.sieve_all(10**9, 1)
    st = ctx.resident_stats()
    assert st.primes == 50_847_533
    assert st.patterns == list(S.CONSTELLATIONS)
    assert st.matches == [3424506, 379508, 379748, 28388, 3633, 3588, 317]
    assert (st.max_gap, st.max_gap_prime) == (282, 436_273_009)
    assert [int(v) for v in st.gaps[1:4]] == [3424506, 3424679, 6089791]
    assert st.gap_overflow == 0 and int(np.count_nonzero(st.gaps)) == 129
    assert int(st.gaps.sum()) == st.primes - 1 and (st.first, st.last) == (3, 999_999_937)
    assert st == ctx.resident_stats(1)


# -- 5. windows ------------------------------------------------------------------------------------------
def test_stats_window_matches_brute_force(ctx, S):
    for lo, hi in ((10, 1000), (11, 999), (10, 999), (11, 1000), (1, 100), (0, 2), (2, 3), (3, 3), (4, 4), (100, 50),
                   (10**12, 10**12 + 10**5)):
        got = ctx.stats_window(lo, hi)
        a = max(lo, 3) | 1
        if hi >= a:
            nb = ((hi if hi & 1 else hi - 1) - a) // 2 + 1
            g0 = (a - 3) // 2
            assert not R.diff(got.words, R.brute(mr_window(g0, nb), g0, S.CONSTELLATIONS)), (lo, hi)
            assert got.primes == ctx.sieve_window(lo, hi)
        else:
            assert not R.diff(got.words, R.brute(np.zeros(0, bool), (a - 3) // 2, S.CONSTELLATIONS)), (lo, hi)
            assert (got.primes, got.first, got.max_gap_prime) == (0, None, None)
    assert ctx.stats_window(3, 13, (S.TWINS,) + S.TRIPLETS).matches == [3, 1, 1]


# -- 6. errors -----------------------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf = guarded(torch)
        mp, op = m.data_ptr(), buf.data_ptr() + 8 * LEAD
        ok = (ctypes.c_uint32 * 9)(*([3] * 9))
        zero, even = (ctypes.c_uint32 * 2)(3, 0), (ctypes.c_uint32 * 2)(3, 6)
        dev_cases = [
            (EINVAL, (None, 0, 64, mp, ok, 2, op, None)),            # null ctx
            (EINVAL, (p, 0, 64, mp, ok, 2, None, None)),             # null stats
            (EINVAL, (p, 0, 64, None, ok, 2, op, None)),             # null mask with nbits > 0
            (EINVAL, (p, 0, 64, mp, ok, 2, op + 4, None)),           # misaligned stats
            (EINVAL, (p, 0, 64, mp, ok, 9, op, None)),               # more than 8 patterns
            (EINVAL, (p, 0, 64, mp, None, 1, op, None)),             # null patterns with a count
            (EINVAL, (p, 0, 64, mp, zero, 2, op, None)),             # a pattern that is 0
            (EINVAL, (p, 0, 64, mp, even, 2, op, None)),             # a pattern with bit 0 clear
            (ERANGE, (p, 2**62 - 10, 64, mp, ok, 2, op, None)),      # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 64, mp, ok, 2, op, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, ok, 2, op, None)),        # more than 2^44 candidates
        ]
        for code, args in dev_cases:
            assert L.dse_stats_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((buf == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(R.WORDS, A5, dtype=np.uint64)
        ho = _dse.u64p(hout)
        range_cases = [
            (EINVAL, (None, 0, 64, ok, 2, ho)),
            (EINVAL, (p, 0, 64, ok, 2, None)),
            (EINVAL, (p, 0, 64, ok, 9, ho)),
            (EINVAL, (p, 0, 64, None, 1, ho)),
            (EINVAL, (p, 0, 64, even, 2, ho)),
            (ERANGE, (p, 2**62 - 10, 64, ok, 2, ho)),
            (ERANGE, (p, 0, 2**44 + 1, ok, 2, ho)),
            (ERANGE, (p, 2**61, 64, ok, 2, ho)),                     # values above 2^62: dse_sieve_odd_range's rule
        ]
        for code, args in range_cases:
            assert L.dse_stats_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, ok, 2, ho)), (EINVAL, (p, 1, ok, 2, ho)), (EINVAL, (p, 0, ok, 2, ho))]:
            assert L.dse_stats_resident(*args) == code, args         # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, ok, 2, ho)), (EINVAL, (p, -1, ok, 2, ho)), (EINVAL, (p, 1, ok, 2, None)),
                           (EINVAL, (p, 1, ok, 9, ho)), (EINVAL, (p, 0, zero, 2, ho))]:
            assert L.dse_stats_resident(*args) == code, args
            assert (hout == A5).all(), args
        with pytest.raises(_dse.DseError):
            c.debug_set_option("stats_grid", 1025)
        with pytest.raises(_dse.DseError):
            c.debug_set_option("stats_grid", -1)
        # and the context still works
        st = c.resident_stats(patterns=(1, S.TWINS))
        assert (st.primes, st.matches[0], st.first, st.last) == (78497, 78497, 3, 999_983)
        assert st.matches[1] == 8169 and c.stats_range(0, 6, (S.TWINS,)).matches == [3]
        got = device_stats(torch, c, 0, 64, m, (3,))
        assert not R.diff(got, R.brute(np.zeros(64, bool), 0, (3,)))
