"""Minimal Goldbach partitions on the GPU (csrc/dse_goldbach.hip): the histogram of
the minimal ranks, the maximum and the unresolved evens of a device-resident mask
as one dse_goldbach, through dse_goldbach_dev_async (torch tensors),
dse_goldbach_range and dse_goldbach_resident (host results, the chunks' results
merged on the host).

Expected values are numpy brute force on bool arrays (tests/goldbach_ref.py), with
the bits from the test's own patterns, from the oracle's CPU sieve or from
Miller-Rabin (tests/primes_ref.py); never from the library. Every word of the
struct is compared, exactly.
"""

import numpy as np
import pytest

import goldbach_ref as R
from primes_ref import mask_bits, mr_window

pytestmark = pytest.mark.gpu
T = R.T
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD = 5, 64


def stride(nbits):
    """Every 11th case of the family, from another start for every fill; every 31st and 41st of
    the two largest sizes, whose cases cost most."""
    return 11 if nbits <= T + 1 else 31 if nbits <= 2 * T + 5 else 41


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
    """A context of this module's own: the tests change its goldbach_grid."""
    with S.Context(num_gpus=1) as c:
        yield c


@pytest.fixture(scope="module")
def real(oracle):
    """The odd candidates 3 .. 4,000,003 and their minimal ranks, once for the module."""
    nb = 2_000_001
    m, _ = oracle.fast_sieve_range(0, nb)
    bits = mask_bits(m, nb)
    return bits, R.ranks(bits)


def to_dev(torch, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()


def guarded(torch):
    return torch.full((LEAD + R.WORDS + GUARD,), A5_I64, dtype=torch.int64, device="cuda")


def device_goldbach(torch, ctx, g_start, nbits, mask_ptr, below_ptr, shift, bb, nprimes, stream=0):
    """One call into an 0xA5-filled tensor with guards on both sides -> the struct's words."""
    buf = guarded(torch)
    ctx.goldbach_dev_async(g_start, nbits, mask_ptr, below_ptr, shift, bb, nprimes, buf.data_ptr() + 8 * LEAD, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all(), "wrote outside the dse_goldbach"
    return h[LEAD:LEAD + R.WORDS]


# -- 1. the synthetic family ------------------------------------------------------------------
def thinned(nbits, k):
    cases = [(g, bb, shift, n) for n in R.NPRIMES for g in R.g_starts(nbits) for bb in R.below_sizes(n, g)
             for shift in R.SHIFTS]
    return cases[k % stride(nbits)::stride(nbits)]


def test_thinned_family_covers_every_value():
    for nbits in R.SIZES:
        seen = [c for k in range(len(R.FILLS)) for c in thinned(nbits, 3 * k)]
        assert {c[0] for c in seen} == set(R.g_starts(nbits))
        assert {c[2] for c in seen} == set(R.SHIFTS) and {c[3] for c in seen} == set(R.NPRIMES)
        for n in R.NPRIMES:
            assert {c[1] for c in seen if c[3] == n} >= set(R.below_sizes(n, 2**40 + 5)), (nbits, n)


@pytest.mark.parametrize("nbits", R.SIZES)
def test_synthetic_family(torch, gctx, nbits):
    try:
        for k, name in enumerate(R.FILLS):
            bits, low = R.fill(name, nbits, 7000 + nbits)
            packed = R.pack_garbage(bits)
            m = to_dev(torch, packed)
            rank = {}
            for j, (g, bb, shift, nprimes) in enumerate(thinned(nbits, 3 * k)):
                if bb not in rank:
                    rank[bb] = R.ranks(bits, low[len(low) - bb:])
                want = R.struct(rank[bb], g, nprimes)
                bw = R.pack_below(low[len(low) - bb:], shift)
                mp = m.data_ptr()
                if bb and (shift + bb) % 64 == 0:
                    # one tensor: the range's mask directly behind its `below`
                    both = to_dev(torch, np.concatenate([bw, packed]))
                    bp, mp = both.data_ptr(), both.data_ptr() + 8 * len(bw)
                elif j % 2:
                    # a pointer into a larger tensor
                    big = to_dev(torch, np.concatenate([np.full(3, A5, np.uint64), bw, np.full(2, A5, np.uint64)]))
                    bp = big.data_ptr() + 24
                else:
                    sep = to_dev(torch, bw)
                    bp = sep.data_ptr() if bb or j % 4 else 0   # NULL is allowed without below_bits
                for grid in (0, 1, 3):
                    gctx.debug_set_option("goldbach_grid", grid)
                    got = device_goldbach(torch, gctx, g, nbits, mp, bp, shift, bb, nprimes)
                    assert not R.diff(got, want), (name, g, bb, shift, nprimes, grid)
    finally:
        gctx.debug_set_option("goldbach_grid", 0)


def test_empty_range(torch, gctx):
    for nprimes in (0, 5):
        got = device_goldbach(torch, gctx, 17, 0, 0, 0, 0, 0, nprimes)
        assert not R.diff(got, R.brute(np.zeros(0, bool), 17, nprimes))


# -- 2. stream order ------------------------------------------------------------------------------
def stream_sieve_then_goldbach(torch, ctx, S, g0, nb, ext, nprimes):
    """base table, the sieves of [g0 - ext, g0) and [g0, g0 + nb) and the partitions enqueued on one
    non-default stream, no host sync between."""
    limit = S.base_limit_for_range(g0, nb)
    table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((nb + 63) // 64, dtype=torch.int64, device="cuda")
    below = torch.zeros((ext + 63) // 64 + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    buf = guarded(torch)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    assert sp != 0
    ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
    if ext:
        ctx.sieve_range_dev_async(table.data_ptr(), g0 - ext, ext, below.data_ptr(), cnt.data_ptr() + 8, sp)
    ctx.sieve_range_dev_async(table.data_ptr(), g0, nb, mask.data_ptr(), cnt.data_ptr(), sp)
    ctx.goldbach_dev_async(g0, nb, mask.data_ptr(), below.data_ptr(), 0, ext, nprimes, buf.data_ptr() + 8 * LEAD, sp)
    s.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + R.WORDS:] == A5).all()
    ctx.device_status()
    return h[LEAD:LEAD + R.WORDS]


def test_stream_order_from_zero(torch, gctx, S, real):
    bits, rank = real
    nb = 1966080 + 777
    got = stream_sieve_then_goldbach(torch, gctx, S, 0, nb, 0, 0)
    assert not R.diff(got, R.struct(rank[:nb], 0, 0))
    assert int(got[4]) == 0


def test_stream_order_high_window(torch, gctx, S):
    g0, nb, ext = (10**12 + 1 - 3) // 2, T + 4096, R.REACH
    vis = mr_window(g0 - ext, ext + nb)
    got = stream_sieve_then_goldbach(torch, gctx, S, g0, nb, ext, 0)
    assert not R.diff(got, R.brute(vis[ext:], g0, 0, vis[:ext]))
    assert int(got[4]) == 0


# -- 3. dse_goldbach_range ----------------------------------------------------------------------------
def test_range_to_4e6(gctx, real):
    bits, rank = real
    nb = 1_999_998
    got = gctx.goldbach_range(0, nb)
    assert not R.diff(got.words, R.struct(rank[:nb], 0, 0))
    assert (got.unresolved, got.max_prime, got.max_rank, got.max_even) == (0, 751, 131, 3_807_404)
    few = gctx.goldbach_range(0, nb, 17)
    assert not R.diff(few.words, R.struct(rank[:nb], 0, 17)) and few.unresolved > 0


def test_range_high_window_sees_below_its_start(gctx):
    g0, nb = (10**15 + 1 - 3) // 2, 3 * T + 77
    vis = mr_window(g0 - R.REACH, R.REACH + nb)   # the extended window
    want = R.brute(vis[R.REACH:], g0, 0, vis[:R.REACH])
    try:
        for grid in (0, 2):
            gctx.debug_set_option("goldbach_grid", grid)
            got = gctx.goldbach_range(g0, nb)
            assert not R.diff(got.words, want), grid
    finally:
        gctx.debug_set_option("goldbach_grid", 0)
    # the evens within reach of the start resolve only through what lies below it
    assert got.unresolved == 0
    blind = R.brute(vis[R.REACH:], g0, 0)
    assert blind[4] > 0 and int(blind[5]) == g0
    # a window that starts within reach of candidate 0 is extended down to it and no further
    lo = gctx.goldbach_range(100, 5000)
    sm = mr_window(0, 5100)
    assert not R.diff(lo.words, R.brute(sm[100:], 100, 0, sm[:100]))


def test_window(gctx):
    sm = mr_window(0, 3000)
    for lo, hi in ((6, 1000), (0, 999), (7, 1001), (500, 4000), (6, 6), (4, 5), (100, 50)):
        got = gctx.goldbach_window(lo, hi)
        a = max(lo, 6) + (max(lo, 6) & 1)
        b = hi - (hi & 1)
        c0 = (a - 6) // 2
        n = (b - a) // 2 + 1 if b >= a else 0
        assert not R.diff(got.words, R.brute(sm[c0:c0 + n], c0, 0, sm[:c0])), (lo, hi)
    assert gctx.goldbach_window(6, 100, 3).max_prime == 7


# -- 4. resident chunks ------------------------------------------------------------------------------------
def resident_against_brute(c, real, N, P, nprimes=0):
    bits, rank = real
    cs = (N - 1) // 2 // P
    c.sieve_all(N, P)
    merged = c.resident_goldbach(nprimes=nprimes)
    assert not R.diff(merged.words, R.struct(rank[:P * cs], 0, nprimes)), (N, P)
    acc = None
    for k in range(1, P + 1):
        one = c.resident_goldbach(k, nprimes)
        # the bits before the chunk are visible: the true ranks
        assert not R.diff(one.words, R.struct(rank[(k - 1) * cs:k * cs], (k - 1) * cs, nprimes)), (N, P, k)
        acc = one if acc is None else acc.merge(one)
    assert acc == merged
    return merged


@pytest.mark.parametrize("logical,P", [(None, 1), (3, 3), (8, 8)])
def test_resident(S, real, logical, P):
    with S.Context(num_gpus=1, logical=logical) as c:
        merged = resident_against_brute(c, real, 4_000_003, P)
        assert (merged.unresolved, merged.max_prime, merged.max_even) == (0, 751, 3_807_404)
        if P == 3:
            c.debug_set_option("goldbach_grid", 2)
            resident_against_brute(c, real, 4_000_003, P, 17)


def test_resident_short_chunks(S, real):
    from mail_sieve_e import _dse
    with S.Context(num_gpus=1, logical=8) as c:
        N, P = 100_000, 8
        assert (N - 1) // 2 // P == 6249 and R.reach(1024) == 4082
        c.sieve_all(N, P)
        for my_num in (None, 2, 8):
            with pytest.raises(_dse.DseError) as e:     # reach 8939 above cs
                c.resident_goldbach(my_num, 2048)
            assert e.value.code == EINVAL and "reach" in str(e.value)
        resident_against_brute(c, real, N, P, 1024)
        # the first chunk needs no `below`
        assert not R.diff(c.resident_goldbach(1, 2048).words, R.struct(real[1][:6249], 0, 2048))


# -- 5. errors ---------------------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf = guarded(torch)
        mp, op = m.data_ptr(), buf.data_ptr() + 8 * LEAD
        dev_cases = [
            (EINVAL, (None, 100, 64, mp, mp, 0, 10, 0, op, None)),        # null ctx
            (EINVAL, (p, 100, 64, mp, mp, 0, 10, 0, None, None)),         # null out
            (EINVAL, (p, 100, 64, None, mp, 0, 10, 0, op, None)),         # null mask with nbits > 0
            (EINVAL, (p, 100, 64, mp, mp, 0, 10, 0, op + 4, None)),       # misaligned out
            (EINVAL, (p, 100, 64, mp + 4, mp, 0, 10, 0, op, None)),       # misaligned mask
            (EINVAL, (p, 100, 64, mp, mp + 4, 0, 10, 0, op, None)),       # misaligned below
            (EINVAL, (p, 100, 64, mp, mp, 0, 10, 2049, op, None)),        # nprimes above 2048
            (EINVAL, (p, 100, 64, mp, mp, 64, 10, 0, op, None)),          # below_shift above 63
            (EINVAL, (p, 100, 64, mp, mp, 0, 101, 0, op, None)),          # below_bits above g_start
            (EINVAL, (p, 100, 64, mp, None, 0, 10, 0, op, None)),         # null below with below_bits > 0
            (ERANGE, (p, 2**62 - 10, 64, mp, None, 0, 0, 0, op, None)),   # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 64, mp, None, 0, 0, 0, op, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, None, 0, 0, 0, op, None)),     # more than 2^44 candidates
        ]
        for code, args in dev_cases:
            assert L.dse_goldbach_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((buf == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()

        hout = np.full(R.WORDS, A5, dtype=np.uint64)
        ho = _dse.u64p(hout)
        for code, args in [(EINVAL, (None, 0, 64, 0, ho)), (EINVAL, (p, 0, 64, 0, None)), (EINVAL, (p, 0, 64, 2049, ho)),
                           (ERANGE, (p, 2**62 - 10, 64, 0, ho)), (ERANGE, (p, 0, 2**44 + 1, 0, ho)),
                           (ERANGE, (p, 2**61, 64, 0, ho))]:          # values above 2^62: dse_sieve_odd_range's rule
            assert L.dse_goldbach_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, 0, ho)), (EINVAL, (p, 1, 0, ho)), (EINVAL, (p, 0, 0, ho))]:
            assert L.dse_goldbach_resident(*args) == code, args      # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, 0, ho)), (EINVAL, (p, -1, 0, ho)), (EINVAL, (p, 1, 0, None)),
                           (EINVAL, (p, 1, 2049, ho))]:
            assert L.dse_goldbach_resident(*args) == code, args
            assert (hout == A5).all(), args
        with pytest.raises(_dse.DseError):
            c.debug_set_option("goldbach_grid", 1025)
        with pytest.raises(_dse.DseError):
            c.debug_set_option("goldbach_grid", -1)
        # and the context still works
        g = c.resident_goldbach()
        assert (g.nbits, g.unresolved, g.max_prime, g.max_even) == (499_998, 0, 523, 503_222)
        got = device_goldbach(torch, c, 0, 64, mp, 0, 0, 0, 3)
        assert not R.diff(got, R.brute(np.zeros(64, bool), 0, 3))
