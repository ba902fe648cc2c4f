"""The resident-mask units past 2^32 candidates and past 2^32 entries: stats, gaps,
consec, race, sums, goldbach, primes and tuples as values, query and the finish text on
caller-owned device masks through the *_dev_async entry points, every struct word and
every value compared exactly.

Three masks, built with torch on the device and never held as host bool arrays:
  F "far"       2^33 + 2 T + 37 candidates (1 GiB), zero but for dense islands around the
                positions 2^31, 2^32 and 2^33 and a few planted bits; expected values from
                tests/sparse_ref.py over its ~5 10^4 sorted positions;
  O "ones"      2^32 + 3 T + 37 candidates, all ones: more than 2^32 entries; expected
                values from sparse_ref's closed forms ones_*;
  L "long run"  (2^20 + 2) T + 37 candidates, all ones (2 GiB): with a grid of 1 one
                workgroup walks more than 2^20 tiles, past the point at which the main
                kernels of stats, race and goldbach empty their 32-bit register counters.
O is the front of L's buffer, so the bits behind O's last one are all set: they must be
ignored. tests/test_sparse_ref.py ties sparse_ref to the dense references on the CPU.

The finish text with DOUBLES is compared at g_start 0 only: at the high start the values
lie above Double printing's domain (DSE_ERANGE). The exact gaps listed as values are those
of 3 and 31 places (a pattern spans at most 32 candidates); the planted gaps of 777 and 901
places are checked through dse_gaps and dse_stats.
"""
import numpy as np
import pytest

import consec_ref as CR
import gaps_ref as GR
import goldbach_ref as GB
import query_ref as QR
import race_ref as RR
import sparse_ref as X
import stats_ref as SR
import sums_ref as UR
import tuples_ref as TR

pytestmark = pytest.mark.gpu
T = 256 * 64
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
M64 = (1 << 64) - 1
LEAD, GUARD = 5, 64
ISLAND = 3 * T + 37
NBITS_F = 2**33 + 2 * T + 37
NBITS_O = 2**32 + 3 * T + 37
NBITS_L = (2**20 + 2) * T + 37
G_F = (0, 2**61 - 1 - NBITS_F)   # the values of the second end at 2^62 - 1, its start is 0 mod no period
G_O = (0, 2**31 + 12345)
GAP_BOTH, GAP_HIGH = 777, 901    # longer than any gap inside an island (0.95^777 < 1e-17), below the overflow bin
GRIDS = (0, 64)                  # the production grid and a capped one
SPAN32 = 1 | 1 << 31
RACES = ((4, 1, 3, 0), (3, 1, 2, -1), (4, 1, 1, 0))  # the last: counts only


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lctx(S):
    """A context of this module's own: the tests change its grids."""
    with S.Context(num_gpus=1) as c:
        yield c


def far_positions():
    """int64, sorted: bit 0 and the last bit; islands of ISLAND bits at 1/2, 1/20 and 1/2 with 2^31,
    2^32 and 2^33 inside a word in their middle, the last island ending at the range's last bit; a
    twin and a span-32 pair across the two ends of the word that holds 2^32; the gap GAP_BOTH below
    and above 2^32, the gap GAP_HIGH above it only."""
    rng = np.random.default_rng(20330)
    parts = [np.array([0, NBITS_F - 1, 2**32 - 1, 2**32, 2**32 + 48, 2**32 + 48 + 31,
                       2**30, 2**30 + GAP_BOTH, 2**32 + 2**30, 2**32 + 2**30 + GAP_BOTH,
                       2**32 + 2**29, 2**32 + 2**29 + GAP_HIGH], dtype=np.int64)]
    for start, p in ((2**31 - ISLAND // 2 - 7, 1 / 2), (2**32 - ISLAND // 2 - 7, 1 / 20), (NBITS_F - ISLAND, 1 / 2)):
        assert start % 64 or start == NBITS_F - ISLAND
        parts.append(start + np.flatnonzero(rng.random(ISLAND) < p).astype(np.int64))
    pos = np.unique(np.concatenate(parts))
    assert len(pos) < 3 * 10**5 and pos[0] == 0 and pos[-1] == NBITS_F - 1
    return pos


def device_mask(torch, pos, nbits):
    """The device mask of the positions: only the words that hold a bit cross from the host. The
    bits past nbits in the last word are set: they must be ignored."""
    words = (nbits + 63) // 64
    m = torch.zeros(words, dtype=torch.int64, device="cuda")
    uw, at = np.unique(pos >> 6, return_index=True)
    vals = np.bitwise_or.reduceat(np.uint64(1) << (pos & 63).astype(np.uint64), at)
    assert uw[-1] == words - 1 and nbits % 64
    vals[-1] |= np.uint64((M64 << (nbits % 64)) & M64)
    m[torch.from_numpy(uw).cuda()] = torch.from_numpy(vals.view(np.int64)).cuda()
    return m


@pytest.fixture(scope="module")
def far(torch):
    pos = far_positions()
    m = device_mask(torch, pos, NBITS_F)
    assert int((m != 0).sum()) == len(np.unique(pos >> 6))
    yield pos, m
    del m
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def run(torch):
    """L's buffer, every bit set; O is its front."""
    m = torch.full(((NBITS_L + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    yield m
    del m
    torch.cuda.empty_cache()


def struct(torch, words, call):
    """call(out pointer) into an 0xA5-filled tensor with guards on both sides -> the struct's words."""
    buf = torch.full((LEAD + words + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
    call(buf.data_ptr() + 8 * LEAD)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + words:] == A5).all(), "wrote outside the struct"
    return h[LEAD:LEAD + words]


def check(got, want, diff, what):
    """Every word of a struct, by the names of the members that differ."""
    d = diff(got, want)
    assert not d, (what, d)


def gridded(ctx, option, grids, body):
    """body(grid) under every grid of the unit's option, which is restored."""
    try:
        for grid in grids:
            ctx.debug_set_option(option, grid)
            body(grid)
    finally:
        ctx.debug_set_option(option, 0)


def values_call(torch, call, first, cap):
    """call(first, out pointer, cap, totals pointer) -> (values written, total); cap 0: the count alone."""
    tot = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    buf = torch.full((LEAD + cap + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
    call(first, buf.data_ptr() + 8 * LEAD if cap else 0, cap, tot.data_ptr())
    torch.cuda.synchronize()
    total, written = (int(x) for x in tot.cpu())
    h = buf.cpu().numpy().view(np.uint64)
    assert written <= cap and (h[:LEAD] == A5).all() and (h[LEAD + written:] == A5).all(), "wrote outside the values"
    return h[LEAD:LEAD + written], total


def device_text(torch, ctx, flags, g, nbits, m, first_rank):
    """The sizes alone, then the text into a buffer of exactly that size with guards -> (bytes, entries)."""
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.finish_text_dev_async(flags, g, nbits, m.data_ptr(), first_rank, 0, 0, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    cnt, need = (int(x) for x in tot.cpu())
    buf = torch.full((LEAD + need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    tot.zero_()
    ctx.finish_text_dev_async(flags, g, nbits, m.data_ptr(), first_rank, buf.data_ptr() + LEAD, need, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [cnt, need]
    h = buf.cpu().numpy()
    assert (h[:LEAD] == 0xA5).all() and (h[LEAD + need:] == 0xA5).all(), "wrote outside the text"
    return h[LEAD:LEAD + need].tobytes(), cnt


def to_dev(torch, q):
    return torch.from_numpy(np.ascontiguousarray(q).view(np.int64).copy()).cuda()


def device_query(torch, ctx, kind, g, nbits, m, idx, q):
    qd = to_dev(torch, q)
    buf = torch.full((LEAD + len(q) + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
    ctx.query_dev_async(kind, g, nbits, m.data_ptr(), idx.data_ptr(), qd.data_ptr(), len(q), buf.data_ptr() + 8 * LEAD, 0)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + len(q):] == A5).all(), "wrote outside the answers"
    return h[LEAD:LEAD + len(q)]


def build_index(torch, ctx, S, g, nbits, m):
    words = S.query_index_bytes(nbits) // 8
    idx = torch.full((words + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
    ctx.query_index_dev_async(g, nbits, m.data_ptr(), idx.data_ptr(), 8 * words, 0)
    torch.cuda.synchronize()
    assert bool((idx[words:] == A5_I64).all()), "wrote behind the index"
    return idx


# -- F: positions past 2^31, 2^32 and 2^33 --------------------------------------------------------------
def test_far_mask_is_what_the_cases_need(far):
    pos, _ = far
    st, gp = X.stats(pos, 0, NBITS_F, (1,)), X.gaps(pos, 0, NBITS_F)
    assert int(st[24]) > 2**32 and int(st[26]) >= 6, "max_gap exceeds 2^32, long gaps land in the overflow bin"
    assert int(st[25]) == 2**32 + 2**30 + GAP_BOTH, "and its lower prime lies above 2^32, inside the upper half's run"
    assert int(gp[9 + GAP_BOTH]) == 2**30, "of the two equal gaps the one below 2^32 is the first"
    assert int(gp[9 + GAP_HIGH]) == 2**32 + 2**29, "a first occurrence above 2^32"
    assert 2**32 - 1 in X.matches(pos, NBITS_F, 0b11) and 2**32 + 48 in X.matches(pos, NBITS_F, SPAN32)
    assert int(X.goldbach(pos, 0, NBITS_F, 64)[4]) > 2**32


@pytest.mark.parametrize("g", G_F)
def test_far_stats(torch, lctx, far, g):
    pos, m = far
    for pats in SR.PATTERN_LISTS:
        want = X.stats(pos, g, NBITS_F, pats)
        # Under GRIDS the maximal gap spans whole empty runs, so the closing kernel finds it at a seam. A grid of 2
        # cuts the range at 2^32 + 2 T: the maximal gap, its lower prime at position 2^32 + 2^30 + 777, lies inside
        # the second workgroup's run, and the main kernel itself carries a position above 2^32 (once is enough)
        grids = GRIDS + (2,) if pats is SR.PATTERN_LISTS[-1] else GRIDS
        gridded(lctx, "stats_grid", grids, lambda grid: check(
            struct(torch, SR.WORDS, lambda out: lctx.stats_dev_async(g, NBITS_F, m.data_ptr(), pats, out)), want,
            SR.diff, (pats, grid)))


@pytest.mark.parametrize("g", G_F)
def test_far_gaps(torch, lctx, far, g):
    pos, m = far
    want = X.gaps(pos, g, NBITS_F)
    gridded(lctx, "gaps_grid", GRIDS, lambda grid: check(
        struct(torch, GR.WORDS, lambda out: lctx.gaps_dev_async(g, NBITS_F, m.data_ptr(), out)), want, GR.diff, grid))


@pytest.mark.parametrize("q", [3, 10, 64])
@pytest.mark.parametrize("g", G_F)
def test_far_consec(torch, lctx, far, g, q):
    pos, m = far
    want = X.consec(pos, g, NBITS_F, q)
    try:
        for body in (0, 1, 2):  # the threshold's choice, then each in-word body forced
            lctx.debug_set_option("consec_body", body)
            gridded(lctx, "consec_grid", GRIDS, lambda grid: check(
                struct(torch, CR.WORDS, lambda out: lctx.consec_dev_async(g, NBITS_F, m.data_ptr(), q, out)), want,
                CR.diff, (body, grid)))
    finally:
        lctx.debug_set_option("consec_body", 0)


@pytest.mark.parametrize("g", G_F)
def test_far_race(torch, lctx, far, g):
    pos, m = far
    for q, a, b, d in RACES:
        want = X.race(pos, g, NBITS_F, q, a, b, d)
        gridded(lctx, "race_grid", GRIDS, lambda grid: check(
            struct(torch, RR.WORDS, lambda out: lctx.race_dev_async(g, NBITS_F, m.data_ptr(), q, a, b, d, out)), want,
            RR.diff, (q, a, b, d, grid)))


@pytest.mark.parametrize("g", G_F)
def test_far_sums(torch, lctx, far, g):
    pos, m = far
    cases = [((1, 0), f) for f in (0, UR.POWER, UR.RECIP, UR.POWER | UR.RECIP)]
    cases += [(TR.TWINS, f) for f in (UR.POWER, UR.RECIP, UR.POWER | UR.RECIP)]
    for (req, forb), flags in cases:
        want = X.sums(pos, g, NBITS_F, req, forb, flags)
        gridded(lctx, "sums_grid", GRIDS, lambda grid: check(
            struct(torch, UR.WORDS, lambda out: lctx.sums_dev_async(g, NBITS_F, m.data_ptr(), req, forb, 0, 0, 0, flags,
                                                                    out)), want, UR.diff, (req, flags, grid)))


@pytest.mark.parametrize("g", G_F)
def test_far_goldbach(torch, lctx, far, g):
    pos, m = far
    want = X.goldbach(pos, g, NBITS_F, 64)
    assert int(want[4]) > 2**32 and int(want[5]) != X.NONE
    gridded(lctx, "goldbach_grid", GRIDS, lambda grid: check(
        struct(torch, GB.WORDS, lambda out: lctx.goldbach_dev_async(g, NBITS_F, m.data_ptr(), 0, 0, 0, 64, out)), want,
        GB.diff, grid))


@pytest.mark.parametrize("g", G_F)
def test_far_primes_as_values(torch, lctx, far, g):
    pos, m = far
    want = X.values(pos, g)
    n = len(want)

    def call(first, out, cap, tot):
        lctx.primes_dev_async(g, NBITS_F, m.data_ptr(), first, out, cap, tot)
    got, total = values_call(torch, call, 0, 0)
    assert (len(got), total) == (0, n)
    got, total = values_call(torch, call, 0, n)
    assert total == n and np.array_equal(got, want)
    first = 0
    for cap in (1, 7, 1000, 12289, 3, n):  # unequal pages, the last one past the end
        got, total = values_call(torch, call, first, cap)
        assert total == n and np.array_equal(got, want[first:first + cap]), (first, cap)
        first += cap
    assert first > n


@pytest.mark.parametrize("g", G_F)
def test_far_tuples(torch, lctx, far, g):
    pos, m = far
    for req, forb in (TR.TWINS, (SPAN32, 0), TR.exact_gap_ref(3), TR.exact_gap_ref(31)):
        want = X.tuples(pos, g, NBITS_F, req, forb)
        assert len(want)

        def call(first, out, cap, tot):
            lctx.tuples_dev_async(g, NBITS_F, m.data_ptr(), req, forb, 0, 0, 0, first, out, cap, tot)
        got, total = values_call(torch, call, 0, len(want))
        assert total == len(want) and np.array_equal(got, want), (req, forb)
        k = len(want) // 3
        got, total = values_call(torch, call, k, 5)
        assert total == len(want) and np.array_equal(got, want[k:k + 5]), (req, forb)


@pytest.mark.parametrize("g", G_F)
def test_far_query(torch, lctx, S, far, g):
    pos, m = far
    vals = X.values(pos, g)
    v = vals.astype(object)
    around = np.unique(np.concatenate([v + d for d in (-2, -1, 0, 1, 2)]))
    xs = [int(x) for x in around if 0 <= x <= M64] + [0, int(vals[0]) - 1, int(vals[-1]) + 3, 2**63, M64]
    xs = QR.u64(sorted(set(x for x in xs if x >= 0)))
    ks = QR.u64(list(range(len(vals) + 1)) + [len(vals) + 5, 2**32, M64])

    def ask(grid):
        idx = build_index(torch, lctx, S, g, NBITS_F, m)
        for kind in QR.KINDS:
            q = ks if kind == QR.SELECT else xs
            got = device_query(torch, lctx, kind, g, NBITS_F, m, idx, q)
            assert np.array_equal(got, X.query(pos, g, kind, q)), (kind, grid)
    gridded(lctx, "query_grid", GRIDS, ask)


@pytest.mark.parametrize("g", G_F)
def test_far_finish_text(torch, lctx, far, g):
    pos, m = far
    for first_rank in (0, 2**32 - 3, 2**32 + 7):
        for flags in (X.LAST, X.DOUBLES | X.LAST):
            if flags & X.DOUBLES and g:
                continue  # above Double printing's domain (module docstring)
            want = X.finish_text(pos, g, NBITS_F, first_rank, flags)
            assert device_text(torch, lctx, flags, g, NBITS_F, m, first_rank) == want, (first_rank, flags)


# -- O: more than 2^32 entries ------------------------------------------------------------------------
@pytest.mark.parametrize("g", G_O)
def test_ones_stats(torch, lctx, run, g):
    for pats in SR.PATTERN_LISTS:
        got = struct(torch, SR.WORDS, lambda out: lctx.stats_dev_async(g, NBITS_O, run.data_ptr(), pats, out))
        check(got, X.ones_stats(g, NBITS_O, pats), SR.diff, pats)


@pytest.mark.parametrize("g", G_O)
def test_ones_race(torch, lctx, run, g):
    for q, a, b, d in RACES:
        got = struct(torch, RR.WORDS, lambda out: lctx.race_dev_async(g, NBITS_O, run.data_ptr(), q, a, b, d, out))
        check(got, X.ones_race(g, NBITS_O, q, a, b, d), RR.diff, (q, a, b, d))


@pytest.mark.parametrize("g", G_O)
def test_ones_consec(torch, lctx, run, g):
    got = struct(torch, CR.WORDS, lambda out: lctx.consec_dev_async(g, NBITS_O, run.data_ptr(), 10, out))
    check(got, X.ones_consec(g, NBITS_O, 10), CR.diff, 10)


@pytest.mark.parametrize("g", G_O)
def test_ones_sums(torch, lctx, run, g):
    want = X.ones_sums(g, NBITS_O, UR.POWER)
    assert want[10] > 0, "the sum of the values crosses a 64-bit limb"
    got = struct(torch, UR.WORDS, lambda out: lctx.sums_dev_async(g, NBITS_O, run.data_ptr(), 1, 0, 0, 0, 0, UR.POWER, out))
    check(got, want, UR.diff, "power")


@pytest.mark.parametrize("g", G_O)
def test_ones_goldbach(torch, lctx, run, g):
    got = struct(torch, GB.WORDS, lambda out: lctx.goldbach_dev_async(g, NBITS_O, run.data_ptr(), 0, 0, 0, 0, out))
    check(got, X.ones_goldbach(g, NBITS_O), GB.diff, "hist[0] > 2^32")


@pytest.mark.parametrize("g", G_O)
def test_ones_values_around_rank_2_32(torch, lctx, run, g):
    def primes(first, out, cap, tot):
        lctx.primes_dev_async(g, NBITS_O, run.data_ptr(), first, out, cap, tot)

    def twins(first, out, cap, tot):
        lctx.tuples_dev_async(g, NBITS_O, run.data_ptr(), 0b11, 0, 0, 0, 0, first, out, cap, tot)
    for call, n in ((primes, NBITS_O), (twins, NBITS_O - 1)):  # every position but the last starts a twin
        got, total = values_call(torch, call, 0, 0)
        assert (len(got), total) == (0, n)
        got, total = values_call(torch, call, 2**32 - 8, 16)
        assert total == n and np.array_equal(got, X.ones_values(g, 2**32 - 8, 16))
        got, total = values_call(torch, call, n - 3, 16)
        assert total == n and np.array_equal(got, X.ones_values(g, n - 3, 3))


@pytest.mark.parametrize("g", G_O)
def test_ones_query(torch, lctx, S, run, g):
    a, n = 3 + 2 * g, NBITS_O
    xs = [a + 2 * k + d for k in (0, 2**32 - 1, 2**32, 2**32 + 1, n - 1) for d in (-2, -1, 0, 1, 2)] + [0, 2**63, M64]
    xs = QR.u64(sorted(set(x for x in xs if x >= 0)))
    ks = QR.u64([0, 1, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, n - 2, n - 1, n, n + 1, M64])
    idx = build_index(torch, lctx, S, g, n, run)
    for kind in (QR.RANK, QR.SELECT, QR.NEXT, QR.PREV):
        q = ks if kind == QR.SELECT else xs
        got = device_query(torch, lctx, kind, g, n, run, idx, q)
        assert np.array_equal(got, X.ones_query(g, n, kind, q)), kind


# -- L: one workgroup walks more than 2^20 tiles ------------------------------------------------------------
def test_long_run_stats(torch, lctx, run):
    pats = (1, 0b11)
    gridded(lctx, "stats_grid", (1,), lambda grid: check(
        struct(torch, SR.WORDS, lambda out: lctx.stats_dev_async(0, NBITS_L, run.data_ptr(), pats, out)),
        X.ones_stats(0, NBITS_L, pats), SR.diff, "grid 1"))


def test_long_run_race_counts(torch, lctx, run):
    gridded(lctx, "race_grid", (1,), lambda grid: check(
        struct(torch, RR.WORDS, lambda out: lctx.race_dev_async(0, NBITS_L, run.data_ptr(), 4, 1, 1, 0, out)),
        X.ones_race(0, NBITS_L, 4, 1, 1), RR.diff, "grid 1"))


def test_long_run_goldbach(torch, lctx, run):
    gridded(lctx, "goldbach_grid", (1,), lambda grid: check(
        struct(torch, GB.WORDS, lambda out: lctx.goldbach_dev_async(0, NBITS_L, run.data_ptr(), 0, 0, 0, 0, out)),
        X.ones_goldbach(0, NBITS_L), GB.diff, "grid 1"))
