"""Constellations as numbers (csrc/dse_tuples.hip): the matches of a pattern
(require, forbid) in a device-resident mask as uint64 values on the GPU,
through dse_tuples_dev_async (torch tensors), dse_tuples_resident and
dse_tuples_range (host buffers, in slabs).

Expected values are tests/tuples_ref.py's numpy ANDs of shifted slices, over
the test's own bits, over the values dse_primes_resident lists, or over
Miller-Rabin bits (tests/primes_ref.py); never from the tuples kernels. Every
comparison is exact.
"""
import numpy as np
import pytest

import tuples_ref as R
from primes_ref import mr_window
from tuples_ref import T

pytestmark = pytest.mark.gpu
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
ALL64 = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def to_dev(torch, mask):
    return torch.from_numpy(np.ascontiguousarray(mask).view(np.int64).copy()).cuda()


def device_tuples(torch, ctx, g_start, nbits, m, pat, a=None, shift=0, ab=0, first=0, cap=None, lead=3, guard=64):
    """Two calls on device mask m with `above` tensor a: the count alone (no buffer), then the
    values into an 0xA5-filled tensor at element offset `lead` that holds exactly the values the
    call must write and a guard behind; -> (values, total, written)."""
    req, fb = pat
    ap = a.data_ptr() if a is not None else 0
    tot = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ctx.tuples_dev_async(g_start, nbits, m.data_ptr(), req, fb, ap, shift, ab, first, 0, 0, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    total, w0 = (int(x) for x in tot.cpu())
    assert w0 == 0
    exact = max(total - first, 0)
    if cap is None:
        cap = exact
    want_written = min(cap, exact)
    buf = torch.full((lead + want_written + guard,), A5_I64, dtype=torch.int64, device="cuda")
    tot.fill_(-1)
    ctx.tuples_dev_async(g_start, nbits, m.data_ptr(), req, fb, ap, shift, ab, first,
                         (buf.data_ptr() + 8 * lead) if cap else 0, cap, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [total, want_written], (first, cap)
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:lead] == A5).all() and (h[lead + want_written:] == A5).all(), "wrote outside [out, out + written)"
    return h[lead:lead + want_written], total, want_written


def garbage_mask(bits):
    mask = R.pack(bits)
    if len(bits) % 64:  # garbage past nbits in the last word is ignored
        mask[-1] |= ALL64 << np.uint64(len(bits) % 64)
    return mask


def g_starts(nbits, ab):
    # 0; the value 2^32 + 1 (odd index 2^31 - 1) in the middle of the first tile; the last visible
    # candidate of value 2^62 - 1 (odd index 2^61 - 2)
    return [0, 2**31 - 1 - min(nbits, T) // 2, 2**61 - 1 - nbits - ab]


# -- 1. arbitrary masks ----------------------------------------------------------
NBITS = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37]
ABOVE = [(0, 0)] + [(b, s) for b in (1, 17, 31) for s in (0, 5, 40, 63)]


@pytest.mark.parametrize("nbits", NBITS)
def test_arbitrary_masks(torch, ctx, nbits):
    rng = np.random.default_rng(8100 + nbits)
    k = 0
    for name, bits in R.fills(nbits, 8000 + nbits).items():
        m = to_dev(torch, garbage_mask(bits))
        for ab, sh in ABOVE:
            above = rng.random(ab) < 0.5
            if name in ("zero", "last") and ab:
                above[:] = name == "last"
            a = to_dev(torch, R.pack_above(above, sh, rng))
            k += 1
            g = g_starts(nbits, ab)[k % 3]  # every fill meets every g_start, in turn over the shapes of `above`
            for pat in R.PATTERNS:
                want = R.values(bits, above, *pat, g)
                got, total, written = device_tuples(torch, ctx, g, nbits, m, pat, a, sh, ab)
                assert total == written == len(want), (name, g, ab, sh, pat)
                assert np.array_equal(got, want), (name, g, ab, sh, pat)
    assert 3 + 2 * (g_starts(nbits, 31)[2] + nbits + 31 - 1) == 2**62 - 1


# 1,024 tiles: every thread of the single-workgroup scan owns exactly one tile count; one tile
# more and a thread owns two. A sparse fill keeps the lists small; matches are planted at the seams.
MANY = 1024 * T


@pytest.mark.parametrize("nbits", [MANY, MANY + T + 37])
def test_many_tiles(torch, ctx, nbits):
    rng = np.random.default_rng(8200 + nbits % 1000)
    base = rng.random(nbits) < 1 / 1000
    for pat in ((1, 0), R.TWINS, R.exact_gap_ref(31)):
        bits = base.copy()
        above = rng.random(31) < 0.5
        spots = [0, 63, 64 * 64 - 1, T - 1, MANY - 1, nbits - 40]  # MANY - 1 is the last position of the first size
        for p in spots:
            R.plant(bits, above, p, *pat)
        pos = R.positions(bits, above, *pat)
        assert set(spots) <= set(pos.tolist())
        m, a = to_dev(torch, garbage_mask(bits)), to_dev(torch, R.pack_above(above, 40, rng))
        for g in (0, 2**61 - 1 - nbits - 31):
            got, total, _ = device_tuples(torch, ctx, g, nbits, m, pat, a, 40, 31)
            assert total == len(pos) and np.array_equal(got, np.uint64(3) + np.uint64(2) * (np.uint64(g) + pos.astype(np.uint64))), (pat, g)


# -- 2. matches planted across the seams ---------------------------------------------
def test_planted_across_seams(torch, ctx):
    nbits = 2 * T + 64 + 5  # nbits % 64 < 31: the second-last word's window reaches into `above`
    for pat in (R.TWINS, R.SEXT, (1 | 1 << 31, 0), R.exact_gap_ref(3), R.exact_gap_ref(31)):
        sp = R.span(*pat)
        bits = np.zeros(nbits, bool)
        above = np.zeros(31, bool)
        # the last member just behind, and the first member just before, a word seam, a wave seam
        # (words 64 and 128) and the tile seam; and matches that end in `above`: one that starts in the
        # last word, one that starts in the word before it (both only where they do not forbid each other)
        starts = [3 * 64 - sp + 1, 5 * 64 - 1, 64 * 64 - sp + 1, 128 * 64 - 1, T - sp + 1, 2 * T - 1]
        ends = [nbits - 1, nbits - 6] if sp > 6 and not pat[1] else [nbits - 6] if sp > 6 else [nbits - 1]
        for p in starts + ends:
            R.plant(bits, above, p, *pat)
        pos = R.positions(bits, above, *pat)
        assert set(starts + ends) <= set(pos.tolist()), pat
        assert all(p + sp - 1 >= nbits for p in ends) and (sp <= 6 or nbits - 6 < nbits - nbits % 64)
        m = to_dev(torch, garbage_mask(bits))
        for sh in (0, 40):
            got, total, _ = device_tuples(torch, ctx, 77, nbits, m, pat,
                                          to_dev(torch, R.pack_above(above, sh, np.random.default_rng(sh))), sh, 31)
            assert np.array_equal(got, R.values(bits, above, *pat, 77)), (pat, sh)
        # without `above` the matches that end there are gone, the others stay
        got, total, _ = device_tuples(torch, ctx, 77, nbits, m, pat)
        assert np.array_equal(got, R.values(bits, [], *pat, 77)) and total <= len(pos) - len(ends), pat


def test_short_range_matches_only_through_above(torch, ctx):
    req, fb = R.SEXT
    for nbits in (1, 2, 8):
        vis = np.array([(req >> j) & 1 for j in range(9)] + [0] * 31, bool)
        bits, above = vis[:nbits], vis[nbits:nbits + 31]
        got, total, _ = device_tuples(torch, ctx, 50, nbits, to_dev(torch, R.pack(bits)), (req, fb),
                                      to_dev(torch, R.pack(above)), 0, 31)
        assert total == 1 and got.tolist() == [103]
        got, total, _ = device_tuples(torch, ctx, 50, nbits, to_dev(torch, R.pack(bits)), (req, fb),
                                      to_dev(torch, R.pack(above)), 0, 8 - nbits)
        assert total == 0


def test_all_ones_tile_loops_the_staging_window(torch, ctx):
    assert T > 2048  # 16,384 entries through a 2,048-entry window
    m = to_dev(torch, np.full(T // 64, ALL64, dtype=np.uint64))
    got, total, _ = device_tuples(torch, ctx, 10**12, T, m, (1, 0))
    assert total == T and np.array_equal(got, np.uint64(3) + np.uint64(2) * (np.uint64(10**12) + np.arange(T, dtype=np.uint64)))


# -- 3. rank windows ------------------------------------------------------------------
def test_rank_windows_paged(torch, ctx):
    nbits, g = 3 * T - 100, 10**9
    bits = np.random.default_rng(21).random(nbits) < 0.6
    above = np.random.default_rng(22).random(31) < 0.6
    m, a = to_dev(torch, R.pack(bits)), to_dev(torch, R.pack(above))
    for pat in (R.TWINS, R.exact_gap_ref(3)):
        full = R.values(bits, above, *pat, g)
        total = len(full)
        pieces, first = [], 0
        for cap in [1, 2, 61, 64, 700, 2047, 2048, 2049, 5, total]:  # unequal pieces, the last one past the end
            got, tot, written = device_tuples(torch, ctx, g, nbits, m, pat, a, 0, 31, first=first, cap=cap)
            assert tot == total and written == min(cap, max(total - first, 0))
            pieces.append(got)
            first += cap
        assert first > total and np.array_equal(np.concatenate(pieces), full), pat
        for first in (total - 1, total, total + 5):
            for cap in (0, 1, 2**40):
                got, tot, written = device_tuples(torch, ctx, g, nbits, m, pat, a, 0, 31, first=first, cap=cap)
                assert tot == total and np.array_equal(got, full[first:first + cap]), (first, cap)


# -- 4. real primes ---------------------------------------------------------------------
def chunk_bits(c, P, cs):
    """bool[P * cs] from the values dse_primes_resident lists, chunk by chunk."""
    bits = np.zeros(P * cs, bool)
    for k in range(1, P + 1):
        v = c.resident_primes(k)
        assert len(v) == 0 or (3 + 2 * (k - 1) * cs <= int(v[0]) and int(v[-1]) < 3 + 2 * k * cs)
        bits[((v - np.uint64(3)) // np.uint64(2)).astype(np.int64)] = True
    return bits


def test_real_primes_1e6(S, ctx):
    ctx.sieve_all(10**6, 1)
    cs = (10**6 - 1) // 2
    bits = chunk_bits(ctx, 1, cs)
    gap3 = S.exact_gap(3)
    pats = [S.TWINS, S.QUADRUPLETS, S.SEXTUPLETS]
    st = ctx.resident_stats(patterns=pats)
    for k, (pat, published) in enumerate(zip(pats, (8169, 166, None))):
        got = ctx.resident_tuples(pat)
        assert got.dtype == np.uint64 and np.array_equal(got, R.values(bits, [], pat, 0, 0)), hex(pat)
        assert len(got) == st.matches[k] and (published is None or len(got) == published)
        assert np.array_equal(got, ctx.resident_tuples(pat, my_num=1))
    assert [int(v) for v in ctx.resident_tuples(S.QUADRUPLETS, count=3)] == [5, 11, 101]
    assert S.tuple_members(ctx.resident_tuples(S.QUADRUPLETS, first=1, count=1), S.QUADRUPLETS).tolist() == [[11, 13, 17, 19]]
    for d in (1, 2, 3, 15, 31):
        got = ctx.resident_tuples(*S.exact_gap(d))
        assert np.array_equal(got, R.values(bits, [], *R.exact_gap_ref(d), 0)) and len(got) == int(st.gaps[d]), d
    assert len(ctx.resident_tuples(*gap3)) == 13549


CHUNKED = {
    (1_000_306, 8): dict(cs=62_519, twins=8172, quads=166, gap3=13_551,
                         straddle=[(R.TWINS, 437_632, 7), (R.QUADS, 437_629, 7), (R.exact_gap_ref(3), 187_555, 3)]),
    (1_003_634, 3): dict(cs=167_272, twins=8202, quads=None, gap3=13_592,
                         straddle=[(R.TWINS, 334_543, 2), (R.exact_gap_ref(3), 167_269, 1)]),
}


@pytest.mark.parametrize("logical", [1, 3, 8])
@pytest.mark.parametrize("case", sorted(CHUNKED))
def test_several_chunks(S, case, logical):
    n, P = case
    E = CHUNKED[case]
    cs = E["cs"]
    with S.Context(num_gpus=1, logical=logical) as c:
        c.sieve_all(n, P)
        assert (n - 1) // 2 // P == cs
        bits = chunk_bits(c, P, cs)
        # the shape covers the seams: each of these matches starts in chunk k and ends in chunk k + 1
        for pat, p, k in E["straddle"]:
            assert p in R.positions(bits, [], *pat) and p < k * cs <= p + R.span(*pat) - 1, (pat, p)
        st = c.resident_stats(patterns=[S.TWINS, S.QUADRUPLETS])
        for pat, count, stat in ((R.TWINS, E["twins"], st.matches[0]), (R.QUADS, E["quads"], st.matches[1]),
                                 (R.exact_gap_ref(3), E["gap3"], int(st.gaps[3]))):
            whole = R.values(bits, [], *pat, 0)
            assert len(whole) == stat and (count is None or len(whole) == count), pat
            parts = []
            for k in range(1, P + 1):
                part = c.resident_tuples(*pat, my_num=k)
                head = bits[k * cs:k * cs + 31]  # empty behind chunk P
                assert np.array_equal(part, R.values(bits[(k - 1) * cs:k * cs], head, *pat, (k - 1) * cs)), (pat, k)
                parts.append(part)
            assert np.array_equal(np.concatenate(parts), whole), pat
            assert np.array_equal(c.resident_tuples(*pat), whole), pat
            # a rank window that starts in chunk 1 and ends in chunk 3 (or in the last one)
            lo, hi = len(parts[0]) - 3, len(parts[0]) + len(parts[1]) + 2
            assert np.array_equal(c.resident_tuples(*pat, first=lo, count=hi - lo), whole[lo:hi]), pat
            assert len(c.resident_tuples(*pat, first=len(whole), count=4)) == 0
        # slabs of 5 values: slab seams inside and between the chunks
        c.debug_set_option("primes_slab_entries", 5)
        whole = R.values(bits, [], *R.TWINS, 0)
        assert np.array_equal(c.resident_tuples(*R.TWINS), whole)
        n1 = len(R.positions(bits[:cs], bits[cs:cs + 31], *R.TWINS))
        assert np.array_equal(c.resident_tuples(*R.TWINS, first=n1 - 7, count=23), whole[n1 - 7:n1 + 16])
        assert np.array_equal(c.resident_tuples(*R.TWINS, my_num=2, first=2, count=11),
                              R.values(bits[cs:2 * cs], bits[2 * cs:2 * cs + 31], *R.TWINS, cs)[2:13])
        # primes as numbers go through the same pipeline, as before
        assert np.array_equal(c.resident_primes(2, first=3, count=12), 3 + 2 * (cs + np.flatnonzero(bits[cs:2 * cs])[3:15]))


# -- 5. dse_tuples_range -------------------------------------------------------------------
def test_range_near_1e15(S, ctx):
    g0, nb = (10**15 + 1 - 3) // 2, 3 * 4096 + 11
    ref = mr_window(g0, nb + 31)
    bits, above = ref[:nb], ref[nb:]
    for pat in ((1, 0), R.TWINS, (0b101, 0), R.exact_gap_ref(3), R.exact_gap_ref(9), R.exact_gap_ref(31)):
        want = R.values(bits, above, *pat, g0)
        assert np.array_equal(ctx.tuples_range(g0, nb, *pat), want), pat
        assert np.array_equal(ctx.tuples_range(g0, nb, *pat, first=1, count=3), want[1:4]), pat
    assert len(R.values(bits, above, 0b101, 0, g0)) > 0
    # a window helper: the lowest members in [lo, hi], the other members may lie above hi
    lo = 3 + 2 * g0
    got = ctx.tuples_window(lo - 1, lo + 2 * nb - 2, 0b101)
    assert np.array_equal(got, R.values(bits, above, 0b101, 0, g0))
    assert len(ctx.tuples_window(100, 50, 3)) == 0
    assert ctx.tuples_window(0, 20, S.TWINS).tolist() == [3, 5, 11, 17]


def test_range_at_the_top(S):
    """Fewer than 31 candidates remain above the range: the last sieved candidate has the value
    2^62 - 1 (odd index 2^61 - 2). The 2^31 - 1 base table is this context's alone."""
    nb = 2048
    top = 2**61 - 1  # one past the last candidate
    ref = mr_window(top - nb - 31, nb + 31)
    with S.Context(num_gpus=1) as c:
        for left in (31, 9, 0):
            g0 = top - nb - left
            bits = ref[31 - left:31 - left + nb]
            above = ref[31 - left + nb:]
            assert len(above) == left
            for pat in ((1, 0), (1 | 1 << 4, 0), R.exact_gap_ref(12), (1, 0xFFFFFFFE)):
                want = R.values(bits, above, *pat, g0)
                assert np.array_equal(c.tuples_range(g0, nb, *pat, count=nb), want), (left, pat)


# -- 6. errors -----------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    import ctypes
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        ab = torch.zeros(2, dtype=torch.int64, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        out = torch.full((64,), A5_I64, dtype=torch.int64, device="cuda")
        mp, ap, tp, op = m.data_ptr(), ab.data_ptr(), tot.data_ptr(), out.data_ptr()
        dev_cases = [
            (EINVAL, (None, 0, 64, mp, 3, 0, ap, 0, 0, 0, op, 8, tp, None)),         # null ctx
            (EINVAL, (p, 0, 64, mp, 3, 0, ap, 0, 0, 0, op, 8, None, None)),          # null totals
            (EINVAL, (p, 0, 64, None, 3, 0, ap, 0, 0, 0, op, 8, tp, None)),          # null mask with nbits > 0
            (EINVAL, (p, 0, 64, mp, 3, 0, ap, 0, 0, 0, None, 8, tp, None)),          # null out with a capacity
            (EINVAL, (p, 0, 64, mp, 3, 0, ap, 0, 0, 0, op + 4, 8, tp, None)),        # misaligned out
            (EINVAL, (p, 0, 64, mp, 2, 0, ap, 0, 0, 0, op, 8, tp, None)),            # require with bit 0 clear
            (EINVAL, (p, 0, 64, mp, 3, 2, ap, 0, 0, 0, op, 8, tp, None)),            # require & forbid != 0
            (EINVAL, (p, 0, 64, mp, 3, 0, ap, 0, 32, 0, op, 8, tp, None)),           # above_bits > 31
            (EINVAL, (p, 0, 64, mp, 3, 0, ap, 64, 4, 0, op, 8, tp, None)),           # above_shift > 63
            (EINVAL, (p, 0, 64, mp, 3, 0, None, 0, 4, 0, op, 8, tp, None)),          # null above with above_bits > 0
            (EINVAL, (p, 0, 64, mp, 3, 0, ap + 4, 0, 4, 0, op, 8, tp, None)),        # misaligned above
            (ERANGE, (p, 2**62 - 10, 64, mp, 3, 0, ap, 0, 0, 0, op, 8, tp, None)),   # g_start + nbits > 2^62
            (ERANGE, (p, 2**62 - 64, 64, mp, 3, 0, ap, 0, 1, 0, op, 8, tp, None)),   # a visible candidate beyond
            (ERANGE, (p, 2**63, 64, mp, 3, 0, ap, 0, 0, 0, op, 8, tp, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, 3, 0, ap, 0, 0, 0, op, 8, tp, None)),     # more than 2^44 candidates
        ]
        for code, args in dev_cases:
            assert L.dse_tuples_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((out == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()
        # nbits = 0 writes totals 0, 0; a null above is legal with above_bits = 0
        tot.fill_(-1)
        c.tuples_dev_async(5, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, tp, 0)
        torch.cuda.synchronize()
        assert tot.tolist() == [0, 0]

        hout = np.full(64, A5, dtype=np.uint64)
        t, w = ctypes.c_uint64(), ctypes.c_uint64()
        tw = (ctypes.byref(t), ctypes.byref(w))
        ho = _dse.u64p(hout)
        range_cases = [
            (EINVAL, (None, 0, 64, 3, 0, 0, ho, 8) + tw),
            (EINVAL, (p, 0, 64, 3, 0, 0, None, 8) + tw),
            (EINVAL, (p, 0, 64, 2, 0, 0, ho, 8) + tw),
            (EINVAL, (p, 0, 64, 3, 1, 0, ho, 8) + tw),
            (ERANGE, (p, 2**62 - 10, 64, 3, 0, 0, ho, 8) + tw),
            (ERANGE, (p, 0, 2**44 + 1, 3, 0, 0, ho, 8) + tw),
            (ERANGE, (p, 2**61, 64, 3, 0, 0, ho, 8) + tw),                           # values above 2^62
        ]
        for code, args in range_cases:
            assert L.dse_tuples_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, 3, 0, 0, ho, 8) + tw), (EINVAL, (p, 1, 3, 0, 0, ho, 8) + tw)]:
            assert L.dse_tuples_resident(*args) == code, args                        # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, 3, 0, 0, ho, 8) + tw), (EINVAL, (p, -1, 3, 0, 0, ho, 8) + tw),
                           (EINVAL, (p, 1, 3, 0, 0, None, 8) + tw), (EINVAL, (p, 0, 2, 0, 0, ho, 8) + tw),
                           (EINVAL, (p, 0, 3, 3, 0, ho, 8) + tw)]:
            assert L.dse_tuples_resident(*args) == code, args
            assert (hout == A5).all(), args
        # and the context still works
        assert [int(v) for v in c.resident_tuples(S.TWINS, count=4)] == [3, 5, 11, 17]
        assert len(c.resident_tuples(S.TWINS)) == 8169
