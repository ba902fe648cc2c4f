"""Residue-class counts and prime races on the GPU (csrc/dse_race.hip): the entries of
a device-resident mask per class mod q and the race of class a against class b as
one dse_race, through dse_race_dev_async (torch tensors), dse_race_range and
dse_race_resident (host results; the chunks chained through their d_end and merged
on the host).

Expected values are numpy on bool arrays (tests/race_ref.py), with the bits from the
test's own patterns, from the oracle's CPU sieve or from Miller-Rabin
(tests/primes_ref.py); never from the library. Every word of the struct is compared,
exactly.
"""

import numpy as np
import pytest

import race_ref as R
from primes_ref import mask_bits, mr_window

pytestmark = pytest.mark.gpu
T = R.T
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD = 5, 64
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
def rctx(S):
    """A context of this module's own: the tests change its race_grid."""
    with S.Context(num_gpus=1) as c:
        yield c


@pytest.fixture(scope="module")
def real(oracle):
    """The odd candidates 3 .. 4,000,003, once for the module."""
    m, _ = oracle.fast_sieve_range(0, NB_4M)
    return mask_bits(m, NB_4M)


def to_dev(torch, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()


def guarded(torch):
    return torch.full((LEAD + R.WORDS + GUARD,), A5_I64, dtype=torch.int64, device="cuda")


def device_race(torch, ctx, g_start, nbits, mask_ptr, q, a, b, d_start, stream=0):
    """One call into an 0xA5-filled tensor with guards on both sides -> the struct's words."""
    buf = guarded(torch)
    ctx.race_dev_async(g_start, nbits, mask_ptr, q, a, b, d_start, buf.data_ptr() + 8 * LEAD, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all(), "wrote outside the dse_race"
    return h[LEAD:LEAD + R.WORDS]


def in_larger(torch, words):
    """The mask as a pointer into a larger tensor, 0xA5 words on both sides."""
    big = to_dev(torch, np.concatenate([np.full(3, A5, np.uint64), words, np.full(2, A5, np.uint64)]))
    return big, big.data_ptr() + 24


# -- 1. the synthetic family ------------------------------------------------------------------
@pytest.mark.parametrize("nbits", R.SIZES)
def test_synthetic_family(torch, rctx, nbits):
    try:
        for k, name in enumerate(R.FILLS):
            fixed = None if name == "alternating" else R.fill(name, nbits, 9000 + nbits)
            keep = None if fixed is None else in_larger(torch, R.pack_garbage(fixed))
            for g, q, a, b, d in R.thinned(nbits, k):
                bits = R.fill(name, nbits, 0, g, q, a, b) if fixed is None else fixed
                hold, mp = keep if keep is not None else in_larger(torch, R.pack_garbage(bits))
                want = R.brute(bits, g, q, a, b, d)
                for grid in (0, 1, 3):
                    rctx.debug_set_option("race_grid", grid)
                    got = device_race(torch, rctx, g, nbits, mp, q, a, b, d)
                    assert not R.diff(got, want), (name, g, q, a, b, d, grid)
    finally:
        rctx.debug_set_option("race_grid", 0)


def test_forty_tiles_fast_path_and_exact_walk(torch, rctx):
    """40 tiles (and 3 bits) over 3 and 7 workgroups: several tiles per workgroup, a workgroup's D from
    the slabs before its own. d_start = +-2^40 decides the sign of every word, d_start = 0 on the
    alternating fill has D cross 0 inside the words; a non-default stream."""
    n = 40 * T + 3
    s = torch.cuda.Stream()
    cases = [("half", 2**40 + 5, 4, 1, 3, 2**40), ("half", 6, 4, 1, 3, -2**40), ("16th", 1, 63, 62, 1, 2**40),
             ("alternating", 6, 4, 3, 1, 0), ("alternating", 2**40 + 5, 7, 3, 5, 0), ("alternating", 3, 64, 63, 1, 0),
             ("half", 0, 12, 3, 1, 0), ("4096th", 5, 30, 7, 2, -3), ("ones", 4, 5, 0, 4, -70), ("zero", 2, 8, 3, 1, 3)]
    try:
        for name, g, q, a, b, d in cases:
            bits = R.fill(name, n, 77, g, q, a, b)
            m = to_dev(torch, R.pack_garbage(bits))
            torch.cuda.synchronize()
            want = R.brute(bits, g, q, a, b, d)
            if abs(d) == 2**40:
                assert (int(want[8]), int(want[9])) == ((int(want[7]), 0) if d > 0 else (0, int(want[7])))
            if name == "alternating":
                assert int(want[10]) == int(want[7]) // 2 > n // 64      # a tie at every second step
            for grid in (3, 7):
                rctx.debug_set_option("race_grid", grid)
                with torch.cuda.stream(s):
                    got = device_race(torch, rctx, g, n, m.data_ptr(), q, a, b, d, s.cuda_stream)
                assert not R.diff(got, want), (name, g, q, a, b, d, grid)
    finally:
        rctx.debug_set_option("race_grid", 0)


def test_counts_only_and_empty_range(torch, rctx):
    bits = R.fill("half", 2 * T + 5, 5)
    m = to_dev(torch, R.pack_garbage(bits))
    try:
        for grid in (0, 2):
            rctx.debug_set_option("race_grid", grid)
            for q, r in ((3, 0), (4, 2), (12, 5), (63, 62), (64, 1)):
                got = device_race(torch, rctx, 11, len(bits), m.data_ptr(), q, r, r, 0)
                assert not R.diff(got, R.brute(bits, 11, q, r, r)), (q, r, grid)
                assert [int(v) for v in got[5:11]] == [0] * 6 and int(got[13]) == 0 and int(got[15]) == 0
                assert [int(got[i]) for i in (11, 12, 14, 16)] == [R.NONE] * 4
                assert int(got[17:].sum()) == int(bits.sum())
    finally:
        rctx.debug_set_option("race_grid", 0)
    for q, a, b, d in ((4, 1, 3, 0), (5, 1, 2, -7), (12, 5, 5, 0)):
        got = device_race(torch, rctx, 17, 0, 0, q, a, b, d)
        assert not R.diff(got, R.brute(np.zeros(0, bool), 17, q, a, b, d))


# -- 2. dse_race_range --------------------------------------------------------------------------------
def test_range_to_4e6(rctx, real):
    got = rctx.race_range(0, NB_4M, 4, 1, 3)
    assert not R.diff(got.words, R.brute(real, 0, 4, 1, 3))
    assert (got.steps, got.a_ahead, got.ties, got.b_ahead) == (283_145, 239, 111, 282_795)
    assert (got.first_a_ahead, got.max_d, got.max_at, got.min_d, got.min_at, got.d_end) == (26_861, 8, 623_681, -260, 3_039_859, -141)
    for q, a, b, d in ((3, 1, 2, 0), (5, 1, 2, 0), (12, 5, 7, 3), (63, 3, 1, -3), (64, 63, 2, 0), (30, 7, 7, 0)):
        got = rctx.race_range(0, NB_4M, q, a, b, d)
        assert not R.diff(got.words, R.brute(real, 0, q, a, b, d)), (q, a, b, d)
    assert rctx.race_range(0, NB_4M, 5, 1, 2).first_a_ahead == 6_781


def test_range_high_window_and_top_of_range(rctx):
    g0, nb = (10**15 + 1 - 3) // 2, 3 * T + 77
    bits = mr_window(g0, nb)
    try:
        for grid in (0, 2):
            rctx.debug_set_option("race_grid", grid)
            for q, a, b, d in ((4, 1, 3, 0), (7, 3, 5, -3), (64, 1, 63, 2**40)):
                got = rctx.race_range(g0, nb, q, a, b, d)
                assert not R.diff(got.words, R.brute(bits, g0, q, a, b, d)), (q, a, b, d, grid)
    finally:
        rctx.debug_set_option("race_grid", 0)
    # the range that ends at the value 2^62 - 1
    nb = 1000
    g0 = 2**61 - 1 - nb
    assert 3 + 2 * (g0 + nb - 1) == 2**62 - 1
    bits = mr_window(g0, nb)
    for q, a, b, d in ((4, 1, 3, 0), (3, 2, 1, 5), (63, 1, 62, 0), (64, 63, 63, 0)):
        got = rctx.race_range(g0, nb, q, a, b, d)
        assert not R.diff(got.words, R.brute(bits, g0, q, a, b, d)), (q, a, b, d)
    assert got.counts.sum() == bits.sum() > 10


def test_window(rctx, real):
    for lo, hi in ((3, 1000), (0, 999), (8, 1002), (26_000, 27_000), (5, 5), (4, 4), (100, 50)):
        got = rctx.race_window(lo, hi, 4, 1, 3, -2)
        x = max(lo, 3) | 1
        y = hi if hi & 1 else hi - 1
        g0 = (x - 3) // 2
        n = (y - x) // 2 + 1 if y >= x else 0
        assert not R.diff(got.words, R.brute(real[g0:g0 + n], g0, 4, 1, 3, -2)), (lo, hi)


# -- 3. resident chunks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("logical,P", [(None, 1), (3, 3), (8, 8)])
def test_resident(S, real, logical, P):
    N = 4_000_004
    cs = (N - 1) // 2 // P
    with S.Context(num_gpus=1, logical=logical) as c:
        c.sieve_all(N, P)
        for grid in (0, 2) if P == 3 else (0,):
            c.debug_set_option("race_grid", grid)
            for q, a, b, d in ((4, 1, 3, 0), (3, 1, 2, -3), (12, 5, 7, 2**40), (64, 2, 63, 0), (30, 7, 7, 0)):
                merged = c.resident_race(None, q, a, b, d)
                assert not R.diff(merged.words, R.brute(real[:P * cs], 0, q, a, b, d)), (P, q, a, b, d, grid)
            # each chunk alone, from an arbitrary d_start
            for k in range(1, P + 1):
                one = c.resident_race(k, 4, 1, 3, 7 - k)
                assert not R.diff(one.words, R.brute(real[(k - 1) * cs:k * cs], (k - 1) * cs, 4, 1, 3, 7 - k)), (P, k, grid)
        whole = c.resident_race()
        assert (whole.first_a_ahead, whole.max_d, whole.max_at, whole.min_d, whole.min_at) == (26_861, 8, 623_681, -260, 3_039_859)
        # the chunks chained by hand merge to the same struct
        acc = None
        for k in range(1, P + 1):
            one = c.resident_race(k, 4, 1, 3, 0 if acc is None else acc.d_end)
            acc = one if acc is None else acc.merge(one)
        assert acc == whole


# -- 4. errors ---------------------------------------------------------------------------------------------
def test_errors(torch, S, real):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf = guarded(torch)
        mp, op = m.data_ptr(), buf.data_ptr() + 8 * LEAD
        dev_cases = [
            (EINVAL, (None, 100, 64, mp, 4, 1, 3, 0, op, None)),          # null ctx
            (EINVAL, (p, 100, 64, mp, 4, 1, 3, 0, None, None)),           # null out
            (EINVAL, (p, 100, 64, None, 4, 1, 3, 0, op, None)),           # null mask with nbits > 0
            (EINVAL, (p, 100, 64, mp, 4, 1, 3, 0, op + 4, None)),         # misaligned out
            (EINVAL, (p, 100, 64, mp + 4, 4, 1, 3, 0, op, None)),         # misaligned mask
            (EINVAL, (p, 100, 64, mp, 2, 1, 0, 0, op, None)),             # q outside 3..64
            (EINVAL, (p, 100, 64, mp, 65, 1, 3, 0, op, None)),
            (EINVAL, (p, 100, 64, mp, 4, 4, 3, 0, op, None)),             # a or b >= q
            (EINVAL, (p, 100, 64, mp, 4, 1, 4, 0, op, None)),
            (EINVAL, (p, 100, 64, mp, 4, 1, 1, -1, op, None)),            # a == b with d_start != 0
            (ERANGE, (p, 100, 64, mp, 4, 1, 3, 2**45 + 1, op, None)),     # |d_start| above 2^45
            (ERANGE, (p, 100, 64, mp, 4, 1, 3, -2**45 - 1, op, None)),
            (ERANGE, (p, 2**62 - 10, 64, mp, 4, 1, 3, 0, op, None)),      # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 64, mp, 4, 1, 3, 0, op, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, 4, 1, 3, 0, op, None)),        # more than 2^44 candidates
        ]
        for code, args in dev_cases:
            assert L.dse_race_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((buf == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(R.WORDS, A5, dtype=np.uint64)
        ho = _dse.u64p(hout)
        for code, args in [(EINVAL, (None, 0, 64, 4, 1, 3, 0, ho)), (EINVAL, (p, 0, 64, 4, 1, 3, 0, None)),
                           (EINVAL, (p, 0, 64, 66, 1, 3, 0, ho)), (EINVAL, (p, 0, 64, 4, 5, 3, 0, ho)),
                           (EINVAL, (p, 0, 64, 4, 3, 3, 1, ho)), (ERANGE, (p, 0, 64, 4, 1, 3, 2**46, ho)),
                           (ERANGE, (p, 2**62 - 10, 64, 4, 1, 3, 0, ho)), (ERANGE, (p, 0, 2**44 + 1, 4, 1, 3, 0, ho)),
                           (ERANGE, (p, 2**61, 64, 4, 1, 3, 0, ho))]:      # values above 2^62: dse_sieve_odd_range's rule
            assert L.dse_race_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, 4, 1, 3, 0, ho)), (EINVAL, (p, 1, 4, 1, 3, 0, ho)),
                           (EINVAL, (p, 0, 4, 1, 3, 0, ho))]:
            assert L.dse_race_resident(*args) == code, args               # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, 4, 1, 3, 0, ho)), (EINVAL, (p, -1, 4, 1, 3, 0, ho)),
                           (EINVAL, (p, 1, 4, 1, 3, 0, None)), (EINVAL, (p, 1, 2, 1, 0, 0, ho)),
                           (EINVAL, (p, 0, 4, 1, 1, 5, ho)), (ERANGE, (p, 0, 4, 1, 3, -2**46, ho))]:
            assert L.dse_race_resident(*args) == code, args
            assert (hout == A5).all(), args
        with pytest.raises(_dse.DseError):
            c.debug_set_option("race_grid", 1025)
        with pytest.raises(_dse.DseError):
            c.debug_set_option("race_grid", -1)
        # and the context still works: 3 chunks of 166,666 candidates, the values 3 .. 999,997
        r = c.resident_race()
        assert not R.diff(r.words, R.brute(real[:499_998], 0, 4, 1, 3))
        assert (r.nbits, r.first_a_ahead, r.max_d) == (499_998, 26_861, 8)
        got = device_race(torch, c, 0, 64, mp, 4, 1, 3, 0)
        assert not R.diff(got, R.brute(np.zeros(64, bool), 0, 4, 1, 3))
