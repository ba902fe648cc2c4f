"""Residue pairs of consecutive primes, on the GPU (csrc/dse_consec.hip): the q x q
matrix of a device-resident mask as one dse_consec, through dse_consec_dev_async
(torch tensors), dse_consec_range and dse_consec_resident (host results, the chunks'
results merged on the host).

Expected values are numpy on bool arrays (tests/consec_ref.py), with the bits from
the test's own patterns, from the oracle's CPU sieve, from a numpy sieve, from
Miller-Rabin (tests/primes_ref.py) or from dse_copy_chunk_mask, and entries pinned
from an independent numpy sieve; never from the consec code. Every word of the
struct is compared, exactly. The cases run under the default grid and under caps of
1 and 3 workgroups; the moduli take both in-word bodies of the main kernel.
"""
import numpy as np
import pytest

import consec_ref as R
from primes_ref import mask_bits, mr_window

pytestmark = pytest.mark.gpu
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD, SKEW = 5, 64, 3
GRIDS = (0, 1, 3)
T = R.T
NB_4M = 2_000_001  # the candidates of 3 .. 4,000,003


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
    """A context of this module's own: the tests change its consec options."""
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


def device_consec(torch, ctx, g_start, nbits, mptr, q, stream=0):
    """One call on the device mask at mptr into an 0xA5-filled tensor with guards on both sides -> the words."""
    buf = guarded(torch)
    ctx.consec_dev_async(g_start, nbits, mptr, q, buf.data_ptr() + 8 * LEAD, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all(), "wrote outside the dse_consec"
    return h[LEAD:LEAD + R.WORDS]


def check_all_grids(torch, ctx, bits, cases, what, garbage=True, grids=GRIDS, flush=(0,), bodies=(0,)):
    """bits under every (g_start, q) of cases, grid, flush interval and body against the reference."""
    mask = R.pack_garbage(bits) if garbage else R.pack(bits)
    keep, mptr = to_dev(torch, mask)
    try:
        for g, q in cases:
            want = R.brute(bits, g, q)
            for grid in grids:
                ctx.debug_set_option("consec_grid", grid)
                for f in flush:
                    ctx.debug_set_option("consec_flush_tiles", f)
                    for body in bodies:
                        ctx.debug_set_option("consec_body", body)
                        got = device_consec(torch, ctx, g, len(bits), mptr, q)
                        assert not R.diff(got, want), (what, g, q, grid, f, body)
    finally:
        for name in ("consec_grid", "consec_flush_tiles", "consec_body"):
            ctx.debug_set_option(name, 0)
    del keep


def test_tile_constant_is_the_librarys(gctx):
    assert gctx.debug_get_stat("gaps_tile_bits") == T == 256 * 64


# -- 1. the synthetic family --------------------------------------------------------------------
@pytest.mark.parametrize("k", range(9))
def test_synthetic_masks(torch, gctx, k):
    nbits = R.SIZES[k]
    for i, name in enumerate(R.FILLS):
        check_all_grids(torch, gctx, R.fill(name, nbits, 8000 + nbits), R.thinned(nbits, i), (nbits, name))


def test_both_bodies_at_every_period_they_share(torch, gctx):
    """Every period the bit-parallel body is built for (2 .. 6: q = 4, 3, 8, 5, 12) and the ones above
    (q = 7, 16, 9, 30, 63, 64) under the default body, the bit-parallel body wherever it is built and
    the per-entry body."""
    for name, nbits in (("half", 2 * T + 5), ("16th", 3 * T + 77), ("ones", T + 1)):
        bits = R.fill(name, nbits, 8100 + nbits)
        cases = [(g, q) for q in (4, 3, 8, 5, 12, 7, 16, 9, 30, 63, 64) for g in (1, 2**40 + 11)]
        check_all_grids(torch, gctx, bits, cases, (name, nbits), grids=(0, 3), bodies=(0, 1, 2))


def test_empty_range(torch, gctx):
    for q in (3, 10, 64):
        got = device_consec(torch, gctx, 17, 0, 0, q)
        assert not R.diff(got, R.brute(np.zeros(0, bool), 17, q))


# -- 2. the flush of the 32-bit counters ------------------------------------------------------------
@pytest.mark.parametrize("name", ["ones", "half"])
def test_flush_path(torch, gctx, name):
    nbits = 7 * T + 3
    bits = R.fill(name, nbits, 8000 + nbits)
    cases = [(3, 4), (2**40 + 5, 10), (1, 12), (5, 7), (2, 63)]
    check_all_grids(torch, gctx, bits, cases, ("flush", name), grids=(1, 3), flush=(0, 1, 2), bodies=(0,))
    # the body the threshold does not pick: bit-parallel at the period 6, per-entry at the period 2
    check_all_grids(torch, gctx, bits, [(1, 12)], ("flush", name), grids=(1, 3), flush=(1, 2), bodies=(1,))
    check_all_grids(torch, gctx, bits, [(3, 4)], ("flush", name), grids=(1, 3), flush=(1, 2), bodies=(2,))


# -- 3. planted pairs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PLANTED)
def test_planted_pairs(torch, gctx, name):
    bits, p, p2 = R.planted(name)
    cases = [(g, q) for q in (4, 10, 7, 63) for g in (1, 2**40 + 11)]
    for g, q in cases:
        assert g % R.period(q)  # a wrong phase shows
        assert R.entry(R.brute(bits, g, q), (3 + 2 * (g + p)) % q, (3 + 2 * (g + p2)) % q) >= 1
    check_all_grids(torch, gctx, bits, cases, name, garbage=False)


@pytest.mark.parametrize("tiles", [1024, 1025])
def test_many_tiles(torch, gctx, tiles):
    """The grid at and over its largest: 1,024 workgroups of one tile, 513 of two; and 7 of 147."""
    bits = R.fill("16th", tiles * T, tiles)
    bits[5 * T - 700:7 * T + 800] = False  # an empty tile, so an empty run of one tile
    check_all_grids(torch, gctx, bits, [(2**40 + 5, 10), (3, 63)], tiles, grids=(0, 7))


# -- 4. stream order ------------------------------------------------------------------------------------
def test_stream_order(torch, gctx, S):
    """base table, sieve and the matrix enqueued on one non-default stream, no host sync between."""
    g0, nb = 0, 499_999
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
    gctx.consec_dev_async(g0, nb, mask.data_ptr(), 10, buf.data_ptr() + 8 * LEAD, sp)
    s.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all()
    gctx.device_status()
    assert int(h[LEAD + 3]) == int(cnt.item()) == 78_497
    assert not R.diff(h[LEAD:LEAD + R.WORDS], R.brute(R.sieve_bits(10**6), 0, 10))


# -- 5. ranges of real primes -----------------------------------------------------------------------------
def test_range_to_4e6(gctx, oracle):
    m, _ = oracle.fast_sieve_range(0, NB_4M)
    bits = mask_bits(m, NB_4M)
    gaps = gctx.gaps_range(0, NB_4M)
    for q in (3, 4, 10, 30):
        want = R.brute(bits, 0, q)
        try:
            for grid in GRIDS:
                gctx.debug_set_option("consec_grid", grid)
                got = gctx.consec_range(0, NB_4M, q)
                assert not R.diff(got.words, want), (q, grid)
        finally:
            gctx.debug_set_option("consec_grid", 0)
        # the rows and columns against the class counts, the scalars against the gaps unit's
        cls = np.zeros(64, np.int64)
        cls[:q] = gctx.race_range(0, NB_4M, q, 1, 1).counts
        first, last = np.zeros(64, np.int64), np.zeros(64, np.int64)
        first[(3 + 2 * got.first_g) % q] = 1
        last[(3 + 2 * got.last_g) % q] = 1
        cm = got.counts.astype(np.int64)
        assert np.array_equal(cm.sum(axis=1), cls - last) and np.array_equal(cm.sum(axis=0), cls - first), q
        assert (got.primes, got.first_g, got.last_g) == (gaps.primes, gaps.first_g, gaps.last_g)
        assert got.pairs == got.primes - 1 == int(cm.sum())
    assert gctx.consec_window(0, 4_000_003, 10) == gctx.consec_range(0, NB_4M, 10)
    assert gctx.consec_window(100, 50, 10).nbits == 0 and gctx.consec_window(100, 50, 10).pairs == 0


@pytest.mark.parametrize("q", [3, 4, 10])
def test_window_to_1e8(gctx, q):
    got = gctx.consec_window(3, 10**8, q)
    assert (got.primes, got.pairs, got.first_g) == (5_761_454, 5_761_453, 0)
    for (a, b), n in R.PINNED_1E8[q].items():
        assert int(got.matrix[a, b]) == n, (q, a, b)
    assert int(got.matrix.astype(np.int64).sum()) == got.pairs


def test_window_to_the_1e8th_prime(gctx):
    """The range of Lemke Oliver and Soundararajan's table: the first 10^8 primes, less the prime 2."""
    got = gctx.consec_window(3, R.LOS_HI, 10)
    assert (got.primes, got.pairs, 3 + 2 * got.last_g) == (10**8 - 1, 10**8 - 2, R.LOS_HI)
    for (a, b), n in R.PINNED_LOS.items():
        assert int(got.matrix[a, b]) == n, (a, b)
    # what the 16 entries leave: 3 -> 5 and 5 -> 7
    assert int(got.matrix.astype(np.int64).sum()) - sum(R.PINNED_LOS.values()) == 2
    assert int(got.matrix[3, 5]) == int(got.matrix[5, 7]) == 1


def test_range_at_1e15_and_at_the_top(gctx):
    for g0, nb in (((10**15 + 1 - 3) // 2, 2 * T + 100), (2**61 - 1 - 4096, 4096)):
        bits = mr_window(g0, nb)
        for q in (10, 63):
            want = R.brute(bits, g0, q)
            try:
                for grid in GRIDS:
                    gctx.debug_set_option("consec_grid", grid)
                    assert not R.diff(gctx.consec_range(g0, nb, q).words, want), (g0, q, grid)
            finally:
                gctx.debug_set_option("consec_grid", 0)
    from mail_sieve_e import _dse
    with pytest.raises(_dse.DseError) as e:
        gctx.consec_range(2**61 - 10, 64, 10)
    assert e.value.code == ERANGE


# -- 6. resident masks -----------------------------------------------------------------------------------
# (N, P, two consecutive primes that a chunk seam cuts): test_gpu_gaps.py's, found by a search over spread_work
SEAMS = ((467_821, 3, 155_921, 156_007), (961_761, 8, 360_653, 360_749))


@pytest.mark.parametrize("logical", [None, 3, 8])
def test_resident_chunks_and_seams(S, logical):
    with S.Context(num_gpus=1, logical=logical) as c:
        for N, P, p, p2 in SEAMS:
            chunks = S.spread_work(N, P)
            cs = (chunks[0][1] - chunks[0][0]) // 2
            bits = R.sieve_bits(2 * 10**6)[:P * cs]
            gp, gq = (p - 3) // 2, (p2 - 3) // 2
            # the shape still produces what the case is about: a pair of consecutive primes cut by a seam
            assert bits[gp] and bits[gq] and not bits[gp + 1:gq].any() and gp // cs + 1 == gq // cs < P, (N, P)
            c.sieve_all(N, P)
            for q in (10, 63):
                whole = R.brute(bits, 0, q)
                assert not R.diff(c.resident_consec(q=q).words, whole), (N, P, q)
                inside = 0
                for k in range(1, P + 1):
                    got = c.resident_consec(k, q)
                    assert not R.diff(got.words, R.brute(bits[(k - 1) * cs:k * cs], (k - 1) * cs, q)), (N, P, k, q)
                    inside += got.pairs
                assert inside == int(whole[4]) - (P - 1)  # every seam's pair is the merge's
                assert not R.diff(c.consec_range(0, P * cs, q).words, whole)
            for k in range(1, P + 1):
                assert np.array_equal(mask_bits(c.copy_chunk_mask(N, P, k), cs), bits[(k - 1) * cs:k * cs])


# -- 7. errors --------------------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf = guarded(torch)
        mp, op = m.data_ptr(), buf.data_ptr() + 8 * LEAD
        for code, args in [
            (EINVAL, (None, 0, 64, mp, 10, op, None)),            # null ctx
            (EINVAL, (p, 0, 64, mp, 10, None, None)),             # null result
            (EINVAL, (p, 0, 64, None, 10, op, None)),             # null mask with nbits > 0
            (EINVAL, (p, 0, 64, mp, 10, op + 4, None)),           # misaligned result
            (EINVAL, (p, 0, 64, mp + 4, 10, op, None)),           # misaligned mask
            (EINVAL, (p, 0, 64, mp, 2, op, None)),                # q outside 3..64
            (EINVAL, (p, 0, 64, mp, 65, op, None)),
            (ERANGE, (p, 2**62 - 10, 64, mp, 10, op, None)),      # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 64, mp, 10, op, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, 10, op, None)),        # more than 2^44 candidates
        ]:
            assert L.dse_consec_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((buf == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(R.WORDS, A5, dtype=np.uint64)
        ho = _dse.u64p(hout)
        for code, args in [(EINVAL, (None, 0, 64, 10, ho)), (EINVAL, (p, 0, 64, 10, None)),
                           (EINVAL, (p, 0, 64, 2, ho)), (EINVAL, (p, 0, 64, 65, ho)),
                           (ERANGE, (p, 2**62 - 10, 64, 10, ho)), (ERANGE, (p, 0, 2**44 + 1, 10, ho)),
                           (ERANGE, (p, 2**61, 64, 10, ho))]:      # values above 2^62: dse_sieve_odd_range's rule
            assert L.dse_consec_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, 10, ho)), (EINVAL, (p, 1, 10, ho)), (EINVAL, (p, 0, 10, ho))]:
            assert L.dse_consec_resident(*args) == code, args   # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, 10, ho)), (EINVAL, (p, -1, 10, ho)), (EINVAL, (p, 1, 10, None)),
                           (EINVAL, (p, 1, 2, ho)), (EINVAL, (p, 0, 65, ho))]:
            assert L.dse_consec_resident(*args) == code, args
            assert (hout == A5).all(), args
        for name, bad in (("consec_grid", 1025), ("consec_grid", -1), ("consec_flush_tiles", -1),
                          ("consec_flush_tiles", 2**18), ("consec_body", 3)):
            with pytest.raises(_dse.DseError):
                c.debug_set_option(name, bad)
        # and the context still works
        g = c.resident_consec()
        assert (g.primes, g.pairs, g.first_g, 3 + 2 * g.last_g, g.q) == (78_497, 78_496, 0, 999_983, 10)
        for (a, b), n in R.PINNED_1E6[10].items():
            assert int(g.matrix[a, b]) == n, (a, b)
        assert not R.diff(device_consec(torch, c, 0, 64, mp, 10), R.brute(np.zeros(64, bool), 0, 10))
