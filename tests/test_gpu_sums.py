"""Power and reciprocal sums on the GPU (csrc/dse_sums.hip): the sums over the matches
of a pattern in a device-resident mask as one dse_sums, through dse_sums_dev_async
(torch tensors), dse_sums_range and dse_sums_resident (host results, the chunks'
results merged on the host). Device equals host hook equals reference.

Expected values are Python ints over the test's own bits (tests/sums_ref.py), the
bits from the test's own fills, from a numpy sieve or from Miller-Rabin
(tests/primes_ref.py); never from the sums code. Every word of the struct is compared,
exactly. Each synthetic case runs under the default grid and under caps of 1 and 3
workgroups, so a workgroup walks several tiles and the closing launch adds several
slabs.
"""
import functools

import numpy as np
import pytest

import sums_ref as R
import tuples_ref as TR
from primes_ref import mr_window

pytestmark = pytest.mark.gpu
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD, SKEW = 5, 64, 3
GRIDS = (0, 1, 3)
T = R.T


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
    """A context of this module's own: the tests change its sums_grid."""
    with S.Context(num_gpus=1) as c:
        yield c


def to_dev(torch, mask):
    """The mask SKEW words into a larger 0xA5-filled tensor -> (tensor, pointer to the mask)."""
    m = np.ascontiguousarray(mask).view(np.int64)
    big = torch.full((SKEW + len(m) + 2,), A5_I64, dtype=torch.int64, device="cuda")
    big[SKEW:SKEW + len(m)] = torch.from_numpy(m.copy()).cuda()
    return big, big.data_ptr() + 8 * SKEW


def guarded(torch):
    return torch.full((LEAD + R.WORDS + GUARD,), A5_I64, dtype=torch.int64, device="cuda")


def device_sums(torch, ctx, g_start, nbits, mptr, require=1, forbid=0, aptr=0, shift=0, nab=0, flags=3, stream=0):
    """One call on the device mask at mptr into an 0xA5-filled tensor with guards on both sides -> the words."""
    buf = guarded(torch)
    ctx.sums_dev_async(g_start, nbits, mptr, require, forbid, aptr, shift, nab, flags, buf.data_ptr() + 8 * LEAD, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all(), "wrote outside the dse_sums"
    return h[LEAD:LEAD + R.WORDS]


def check_all_grids(torch, S, ctx, bits, g, want, what, require=1, forbid=0, flags=3, grids=GRIDS):
    """bits at g_start g, nothing above them, under every grid against `want` and the host hook."""
    mask = R.pack_garbage(bits)
    assert not R.diff(S.sums_host(mask, g, len(bits), require, forbid, flags=flags), want), what
    keep, mptr = to_dev(torch, mask)
    try:
        for grid in grids:
            ctx.debug_set_option("sums_grid", grid)
            got = device_sums(torch, ctx, g, len(bits), mptr, require, forbid, flags=flags)
            assert not R.diff(got, want), (what, grid)
    finally:
        ctx.debug_set_option("sums_grid", 0)
    del keep


def test_tile_constant_is_the_librarys(sctx):
    assert sctx.debug_get_stat("sums_tile_bits") == T == 256 * 64


# -- 1. the synthetic family --------------------------------------------------------------------
SIZES = {"word": 64, "tile": T, "3 tiles": 3 * T - 37, "1025 tiles": 1025 * T}


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("fill", ["ones", "8%", "1/4096", "empty run"])
def test_synthetic_masks(torch, S, sctx, size, fill):
    nbits = SIZES[size]
    rng = np.random.default_rng(nbits)
    g = 2**40 + 5
    if fill == "ones":  # the compaction's batches are full
        bits = np.ones(nbits, bool)
        want = R.ones_words(g, nbits, with_recip=False)
        a = 3 + 2 * g
        want[14:17] = R.limbs(sum(map(R.ONE.__floordiv__, range(a, a + 2 * nbits, 2))), 3)
    else:
        if fill == "empty run":  # a thousand empty tiles in a row (fewer in the shorter masks)
            bits = rng.random(nbits) < 0.08
            bits[min(T, nbits // 2):max(nbits - 24 * T, nbits // 2 + 1)] = False
        else:
            bits = rng.random(nbits) < (0.08 if fill == "8%" else 1 / 4096)
        want = R.brute(bits, g)
    if size == "1025 tiles" and fill == "empty run":
        assert not bits[T:1001 * T].any() and bits[:T].any() and bits[1001 * T:].any()
    check_all_grids(torch, S, sctx, bits, g, want, (size, fill))


def test_empty_range(torch, sctx):
    assert not R.diff(device_sums(torch, sctx, 17, 0, 0), R.brute(np.zeros(0, bool), 17))
    assert not R.diff(device_sums(torch, sctx, 17, 0, 0, 3, 4, flags=2), R.brute(np.zeros(0, bool), 17, 3, 4, (), 2))


# -- 2. limb carries ---------------------------------------------------------------------------------
def test_carries(torch, S, sctx):
    n = 2 * T
    want = R.ones_words(R.TOP - n, n, flags=R.POWER)
    assert want[10] != 0 and want[13] != 0  # sum1 carries into limb 1, sum2 into limb 2
    check_all_grids(torch, S, sctx, np.ones(n, bool), R.TOP - n, want, "top", flags=R.POWER)
    want = R.ones_words(0, T)
    assert want[16] == 1  # recip passes 2^128
    check_all_grids(torch, S, sctx, np.ones(T, bool), 0, want, "recip")


# -- 3. flags, patterns and `above` pointing into a larger mask -----------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_each_flags_value(torch, S, sctx, flags):
    rng = np.random.default_rng(77)
    bits = rng.random(3 * T + 5) < 0.3
    for pat in ((1, 0), TR.TWINS):
        want = R.brute(bits, 9, *pat, (), flags)
        if not flags & R.POWER:
            assert want[9:14] == [0] * 5
        if not flags & R.RECIP:
            assert want[14:17] == [0] * 3
        check_all_grids(torch, S, sctx, bits, 9, want, (pat, flags), *pat, flags=flags)


@pytest.mark.parametrize("pat", [TR.TWINS, TR.SEXT, (1 | 1 << 31, 0), TR.exact_gap_ref(3), TR.exact_gap_ref(31)])
def test_patterns_with_above_in_a_larger_mask(torch, S, sctx, pat):
    rng = np.random.default_rng(pat[0])
    total = 3 * T + 64 + 50
    big = rng.random(total) < 0.4
    sp = TR.span(*pat)
    # one device mask; every range is a prefix of it, and its `above` points into the same mask
    for nbits in (2 * T + 64 + 5, T + 37, 2 * T, 30):
        bits = big.copy()
        spare = np.zeros(0, bool)
        for pos in (64 - sp + 1, T - 1, T - sp + 1, nbits - 1, nbits - sp // 2 - 1):
            if 0 <= pos < nbits:
                TR.plant(bits, spare, pos, *pat)
        keep, mptr = to_dev(torch, TR.pack(bits))
        for nab in (0, 1, 17, 31):
            want = R.brute(bits[:nbits], 1000, *pat, bits[nbits:nbits + nab])
            aptr, shift = mptr + 8 * (nbits // 64), nbits % 64
            host = S.sums_host(TR.pack(bits[:nbits]), 1000, nbits, *pat, TR.pack(bits)[nbits // 64:], shift, nab)
            assert not R.diff(host, want), (nbits, nab)
            try:
                for grid in GRIDS:
                    sctx.debug_set_option("sums_grid", grid)
                    got = device_sums(torch, sctx, 1000, nbits, mptr, *pat, aptr, shift, nab)
                    assert not R.diff(got, want), (nbits, nab, grid)
            finally:
                sctx.debug_set_option("sums_grid", 0)
        del keep


# -- 4. ranges of real primes -----------------------------------------------------------------------
def test_range_below_1e8(sctx, S):
    s = sctx.sums_window(0, 10**8)
    assert (s.matches, s.sum1) == (5_761_454, 279_209_790_387_274)
    assert (s.g_start, s.nbits, s.first, s.last, s.above_bits) == (0, (10**8 - 3) // 2 + 1, 3, 99_999_989, 31)
    tw = sctx.sums_range(0, s.nbits, 3, 0)
    st = sctx.stats_range(0, s.nbits + 1, patterns=[S.TWINS])  # its twins lie inside the range: one more candidate
    assert tw.matches == st.matches[0] == 440_312
    lo, hi = tw.reciprocal_bounds()
    assert lo < hi and 1.7588156 < float(lo) <= float(hi) < 1.7588157  # B2(1e8) = 1.758815621...
    assert sctx.sums_window(100, 50).nbits == 0 and sctx.sums_window(100, 50).matches == 0


def test_window_below_1e6_every_word(sctx, S):
    bits = R.odd_sieve(10**6 + 64)
    n = 499_999
    for pat in ((1, 0), TR.TWINS, TR.exact_gap_ref(3)):
        for flags in (0, 1, 2, 3):
            want = R.brute(bits[:n], 0, *pat, bits[n:n + 31], flags)
            assert not R.diff(sctx.sums_window(0, 10**6, *pat, flags), want), (pat, flags)
    s = sctx.sums_window(0, 10**6)
    assert (s.matches, s.sum1, s.sum2, s.recip) == (
        78_497, 37_550_402_021, 24_693_298_341_834_529, 203_091_414_084_438_379_867_552_348_341_623_506_040)


def test_range_at_1e15_and_at_the_top(sctx, S):
    for g0, nb in (((10**15 + 1 - 3) // 2, 2 * T + 100), (2**61 - 1 - 4096, 4096)):
        ext = min(31, 2**61 - 1 - (g0 + nb))
        ref = mr_window(g0, nb + ext)
        for pat in ((1, 0), TR.TWINS, TR.exact_gap_ref(9)):
            want = R.brute(ref[:nb], g0, *pat, ref[nb:])
            try:
                for grid in GRIDS:
                    sctx.debug_set_option("sums_grid", grid)
                    assert not R.diff(sctx.sums_range(g0, nb, *pat), want), (g0, pat, grid)
            finally:
                sctx.debug_set_option("sums_grid", 0)
    from mail_sieve_e import _dse
    with pytest.raises(_dse.DseError) as e:
        sctx.sums_range(2**61 - 10, 64)
    assert e.value.code == ERANGE


# -- 5. resident masks ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_bits():
    return R.odd_sieve(10**7 + 100)


@functools.lru_cache(maxsize=None)
def resident_ref(cs, P, pat):
    bits = real_bits()
    whole = R.brute(bits[:P * cs], 0, *pat)
    parts = [R.brute(bits[(k - 1) * cs:k * cs], (k - 1) * cs, *pat, bits[k * cs:k * cs + 31] if k < P else ())
             for k in range(1, P + 1)]
    return whole, parts


# (N, P, cs, a twin whose lower member is the last candidate of chunk k: the pairs of tests/test_gpu_tuples.py)
RESIDENT = ((10**7, 8, None, None, None), (1_000_306, 8, 62_519, 437_632, 7), (1_003_634, 3, 167_272, 334_543, 2))


@pytest.mark.parametrize("logical", [1, 3, 8])
def test_resident_chunks_and_seams(S, logical):
    bits = real_bits()
    with S.Context(num_gpus=1, logical=logical) as c:
        for N, P, cs_want, p, k_seam in RESIDENT:
            cs = (N - 1) // 2 // P
            assert cs_want is None or cs == cs_want
            c.sieve_all(N, P)
            for pat in ((1, 0), TR.TWINS):
                whole, parts = resident_ref(cs, P, pat)
                if p is not None and pat == TR.TWINS:
                    # the shape still has what the case is about: a twin that starts in chunk k and ends in k + 1
                    assert bits[p] and bits[p + 1] and p == k_seam * cs - 1
                    assert parts[k_seam - 1][8] == p
                got = [c.sums_resident(k, *pat) for k in range(1, P + 1)]
                for k in range(P):
                    assert not R.diff(got[k], parts[k]), (N, P, pat, k + 1)
                every = c.sums_resident(None, *pat)
                assert not R.diff(every, whole), (N, P, pat)
                assert functools.reduce(lambda a, b: a.merge(b), got) == every
            assert c.sums_resident(None, 3, 0, flags=0).matches == c.resident_stats(patterns=[S.TWINS]).matches[0]


# -- 6. errors ----------------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf = guarded(torch)
        mp, op = m.data_ptr(), buf.data_ptr() + 8 * LEAD
        for code, args in [
            (EINVAL, (None, 0, 64, mp, 1, 0, None, 0, 0, 3, op, None)),        # null ctx
            (EINVAL, (p, 0, 64, mp, 1, 0, None, 0, 0, 3, None, None)),         # null result
            (EINVAL, (p, 0, 64, None, 1, 0, None, 0, 0, 3, op, None)),         # null mask with nbits > 0
            (EINVAL, (p, 0, 64, mp, 1, 0, None, 0, 0, 3, op + 4, None)),       # misaligned result
            (EINVAL, (p, 0, 64, mp, 1, 0, None, 0, 0, 4, op, None)),           # unknown flags
            (EINVAL, (p, 0, 64, mp, 2, 0, None, 0, 0, 3, op, None)),           # require without bit 0
            (EINVAL, (p, 0, 64, mp, 3, 2, None, 0, 0, 3, op, None)),           # require & forbid
            (EINVAL, (p, 0, 64, mp, 1, 0, mp, 0, 32, 3, op, None)),            # above_bits > 31
            (EINVAL, (p, 0, 64, mp, 1, 0, mp, 64, 1, 3, op, None)),            # above_shift > 63
            (EINVAL, (p, 0, 64, mp, 1, 0, None, 0, 1, 3, op, None)),           # null above
            (EINVAL, (p, 0, 64, mp, 1, 0, mp + 4, 0, 1, 3, op, None)),         # misaligned above
            (ERANGE, (p, 2**62 - 10, 64, mp, 1, 0, None, 0, 0, 3, op, None)),  # g_start + nbits > 2^62
            (ERANGE, (p, 2**62 - 64, 64, mp, 1, 0, mp, 0, 1, 3, op, None)),    # the visible candidates pass it
            (ERANGE, (p, 0, 2**44 + 1, mp, 1, 0, None, 0, 0, 3, op, None)),    # more than 2^44 candidates
        ]:
            assert L.dse_sums_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((buf == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(R.WORDS, A5, dtype=np.uint64)
        ho = _dse.u64p(hout)
        for code, args in [(EINVAL, (None, 0, 64, 1, 0, 3, ho)), (EINVAL, (p, 0, 64, 1, 0, 3, None)),
                           (EINVAL, (p, 0, 64, 1, 0, 4, ho)), (EINVAL, (p, 0, 64, 2, 0, 3, ho)),
                           (EINVAL, (p, 0, 64, 3, 1, 3, ho)), (ERANGE, (p, 2**62 - 10, 64, 1, 0, 3, ho)),
                           (ERANGE, (p, 0, 2**44 + 1, 1, 0, 3, ho)),
                           (ERANGE, (p, 2**61, 64, 1, 0, 3, ho))]:  # values above 2^62: dse_sieve_odd_range's rule
            assert L.dse_sums_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, 1, 0, 3, ho)), (EINVAL, (p, 1, 1, 0, 3, ho)),
                           (EINVAL, (p, 0, 1, 0, 3, ho))]:
            assert L.dse_sums_resident(*args) == code, args  # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, 1, 0, 3, ho)), (EINVAL, (p, -1, 1, 0, 3, ho)), (EINVAL, (p, 1, 1, 0, 3, None)),
                           (EINVAL, (p, 1, 1, 0, 8, ho)), (EINVAL, (p, 1, 2, 0, 3, ho))]:
            assert L.dse_sums_resident(*args) == code, args
            assert (hout == A5).all(), args
        for bad in (1025, -1):
            with pytest.raises(_dse.DseError):
                c.debug_set_option("sums_grid", bad)
        # and the context still works
        s = c.sums_resident()
        assert (s.matches, s.first, s.last, s.sum1) == (78_497, 3, 999_983, 37_550_402_021)
        assert not R.diff(device_sums(torch, c, 0, 64, mp), R.brute(np.zeros(64, bool), 0))
