"""A witness for each side of each prime-class threshold.

Every sieving prime belongs to one class, fixed by a threshold T: L units in
LDS or bucketed (2^19, or 2^17..2^20 with bucket_lo_log2), with or without
Barrett factors and offset rows (kWheelMaxPrime = 2^20, also the pooled /
bucketed dispatch), from a one-level or a two-level table build (2,457,601),
band 0 or band 1 of the bucketed pass (2^28), below or above the kFillMaxSplit
clamp (30 * 2^24), and the ends of what the suite reached before (1e9) and of
the table (2^31). For the largest prime <= T and the smallest prime > T the
tests sieve a small window that holds witness(p, V) = p * c, c the smallest
prime >= max(p, V / p): a composite whose least factor is p, so only p's walk
clears its bit, and a lost or mis-walked p fails an assertion that names it.
Every window is compared whole with Miller-Rabin (tests/primes_ref.py).
"""
import random
from contextlib import contextmanager

import numpy as np
import pytest

from primes_ref import is_prime_mr, mask_bits, mr_window, next_prime, prev_prime, witness

pytestmark = pytest.mark.gpu

SEG = 1_966_080  # odd candidates per wheel segment
NB = 1 << 14     # candidates per window
M = 2**31 - 1

# T, what splits there, (largest prime <= T, smallest prime > T), the option
# sets that make the pair straddle the live threshold ({}: production)
ROWS = [
    (2**17, "bucket_lo_log2 = 17", (131_071, 131_101), [{"bucket_lo_log2": 17}]),
    (2**18, "bucket_lo_log2 = 18", (262_139, 262_147), [{"bucket_lo_log2": 18}]),
    (2**19, "production bucket threshold", (524_287, 524_309), [{}]),
    (2**20, "kWheelMaxPrime / bucket_lo_log2 = 20", (1_048_573, 1_048_583), [{}, {"bucket_lo_log2": 20}]),
    (2_457_601, "one-level / two-level table build", (2_457_569, 2_457_607), [{}]),
    (2**28, "band 0 / band 1", (268_435_399, 268_435_459), [{}]),
    (30 * 2**24, "kFillMaxSplit clamp", (503_316_469, 503_316_511),
     [{"bucket_split_log2": 29}, {"bucket_split_log2": 63}]),
    (10**9, "where the suite stopped before", (999_999_937, 1_000_000_007), [{}]),
    (2**31, "end of the table", (2_147_483_629, 2_147_483_647), [{}]),
]
MAGNITUDES = [10**13, 10**16, 10**18, 46 * 10**17]
TABLE_PRIMES = [p for row in ROWS for p in row[2]]


def test_threshold_primes_are_the_neighbours():
    for T, _, (a, b), _ in ROWS[:-1]:
        assert prev_prime(T) == a and next_prime(T + 1) == b, T
    assert prev_prime(2**31) == M == ROWS[-1][2][1] and prev_prime(M - 1) == ROWS[-1][2][0]
    assert is_prime_mr(M)


@pytest.fixture(scope="module")
def cls_ctx():
    """One context for the module: its table grows to the 2^31 - 1 one
    (6.5 GB), which the session-wide ctx should not keep."""
    from mail_sieve_e.sieve import Context
    c = Context(num_gpus=1)
    yield c
    c.close()


@contextmanager
def options(ctx, opts):
    for k, v in opts.items():
        ctx.debug_set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            ctx.debug_set_option(k, 0)


_MR = {}


def mr_ref(g0, nb=NB):
    if (g0, nb) not in _MR:
        _MR[g0, nb] = mr_window(g0, nb)
    return _MR[g0, nb]


def check_window(bits, c, g0, what):
    ref = mr_ref(g0, len(bits))
    bad = np.flatnonzero(bits != ref)
    assert len(bad) == 0, (what, [(3 + 2 * (g0 + int(j)), bool(bits[j])) for j in bad[:8]])
    if c is not None:
        assert c == int(ref.sum()), what


def witness_window(p, V):
    """(g0, j): a window of NB candidates from index g0 whose bit j is
    witness(p, V), at an offset drawn from a generator seeded by the case."""
    w = witness(p, V)
    assert w % p == 0 and w >= max(V, p * p) and is_prime_mr(w // p) and w // p >= p
    j = random.Random(f"{p}:{V}").randrange(NB)
    return (w - 3) // 2 - j, j


def cases_at(V):
    return [(T, what, p, opts) for T, what, pair, optsets in ROWS for p in pair if V >= p * p for opts in optsets]


@pytest.mark.parametrize("V", MAGNITUDES)
def test_witness_windows(cls_ctx, V):
    """Each threshold prime's witness at magnitude V (those with p^2 <= V), in
    one pass with the options of its row: the whole window against
    Miller-Rabin, and the witness bit by name."""
    cases = cases_at(V)
    assert cases
    for T, what, p, opts in cases:
        g0, j = witness_window(p, V)
        with options(cls_ctx, opts):
            m, c = cls_ctx.sieve_odd_range(g0, NB)
        bits = mask_bits(m, NB)
        assert not bits[j], (f"witness {3 + 2 * (g0 + j)} = {p} * {(3 + 2 * (g0 + j)) // p} left set: prime {p} "
                             f"beside T = {T} ({what}) was lost or mis-walked at V = {V:.1e}, options {opts}")
        check_window(bits, c, g0, (p, T, V, opts))


def _multi_pass_cases():
    out = []
    for T, what, pair, optsets in ROWS:
        p = pair[1]
        vs = [V for V in MAGNITUDES if V >= p * p]
        if vs:
            out.append(pytest.param(T, what, p, vs[0], optsets[-1], id=f"T{T}-p{p}-V{vs[0]:.0e}"))
    return out


@pytest.mark.parametrize("T,what,p,V,opts", _multi_pass_cases())
def test_witness_in_last_of_four_segments(cls_ctx, T, what, p, V, opts):
    """One case per row in passes of 3 segments (bucket_pass_segments): a range
    of 4 segments whose last NB candidates are the witness window, so the
    witness sits in the second pass's only segment."""
    g0, j = witness_window(p, V)
    gs, nb = g0 + NB - 4 * SEG, 4 * SEG
    with options(cls_ctx, dict(opts, bucket_pass_segments=3)):
        m, c = cls_ctx.sieve_odd_range(gs, nb)
    bits = mask_bits(m, nb)
    tail = bits[nb - NB:]
    assert not tail[j], f"witness of prime {p} beside T = {T} ({what}) left set in the second pass, V = {V:.1e}"
    check_window(tail, None, g0, (p, T, V, opts, "4 segments"))
    with options(cls_ctx, opts):
        m1, c1 = cls_ctx.sieve_odd_range(gs, nb)  # the same range in one pass
    assert c == c1 and np.array_equal(m, m1)


@pytest.mark.parametrize("q", TABLE_PRIMES)
def test_square_edges(cls_ctx, q):
    """Ranges of NB candidates that begin exactly at q^2, end exactly at q^2
    (vmax = q^2: the table limit is q, the inclusive p^2 <= vmax edge) and end
    at q^2 - 2 (limit q - 1: q is absent from the table)."""
    from mail_sieve_e import sieve as S
    gq = (q * q - 3) // 2
    for g0, j, limit in ((gq, 0, None), (gq - (NB - 1), NB - 1, q), (gq - NB, None, q - 1)):
        if limit is not None:
            assert S.base_limit_for_range(g0, NB) == limit
        m, c = cls_ctx.sieve_odd_range(g0, NB)
        bits = mask_bits(m, NB)
        if j is not None:
            assert not bits[j], f"{q}^2 left set in the range that {'begins' if j == 0 else 'ends'} at it"
        check_window(bits, c, g0, (q, j))


@pytest.mark.parametrize("vmax", [2**40 - 1, 2**40 + 1, (2**20 + 1)**2 - 2, (2**20 + 1)**2, 1_048_583**2])
def test_dispatch_edges_at_2p40(cls_ctx, vmax):
    """Both sides of the pooled / bucketed dispatch, isqrt(vmax) <=
    kWheelMaxPrime: roots 2^20 - 1, 2^20 and 2^20 (pooled), then 2^20 + 1
    = 17 * 61681 (a bucketed pass with no prime above 2^20 to bucket) and
    1,048,583 (bucketed, the first prime above 2^20 hits only its square, the
    range's last candidate)."""
    from mail_sieve_e import sieve as S
    import math
    g0 = (vmax - 3) // 2 - (NB - 1)
    assert S.base_limit_for_range(g0, NB) == math.isqrt(vmax)
    m, c = cls_ctx.sieve_odd_range(g0, NB)
    bits = mask_bits(m, NB)
    if vmax == 1_048_583**2:
        assert not bits[NB - 1], "1048583^2 left set"
    check_window(bits, c, g0, vmax)
