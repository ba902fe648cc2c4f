"""The wheel kernel's unit loop: the L list's length, the interleave of the unit
queue, the pre-assigned first positions, the roots a workgroup's thread 0
leaves per segment, and the bucket units between L units.

In the kernels without bucket units every wave takes queue positions w and w +
16 without a claim (the counter starts at 32) and reads isqrt(Vs) and
isqrt(Vend - 1) from two LDS words that thread 0 wrote before the segment's
first barrier; the bucket kernel claims every position and takes the roots per
wave, in the same unit loop. A set of 64
L primes is skipped if its first prime exceeds isqrt(Vend - 1) and takes the
per-lane path if its last prime exceeds isqrt(Vs), so a root off by one loses a
prime's first marks or marks a set that is not live: both show in the mask.

Every case compares the whole mask and the count with the CPU oracle
(oracle.fast_sieve_range). The helpers are test_gpu_rounds's.

Values: a range from candidate g0 has V0 = 2 + 2 g0, and its segment s starts
at Vs = V0 + s W, W = 30 * 2^17 in the full geometry (wheel_geometry = 1) and
30 * 2^16 in the half one (2). Vs is even and Vend - 1 = Vs + W - 1 odd, so
around an (odd) square p^2 the nearest a segment comes is Vs = p^2 - 1 or p^2 +
1 and Vend - 1 = p^2 - 2, p^2 or p^2 + 2: the cases below take Vs in {p^2 - 3,
p^2 - 1, p^2 + 1, p^2 + 3} and with it Vend - 1 in {p^2 - 4, p^2 - 2, p^2, p^2
+ 2}. A segment's end lies at least W above 0, so Vend - 1 near p^2 needs p^2 >
W: every L prime from 1987 on, a B2 prime (p <= 1536) only in the half
geometry (p >= 1409), no B1 prime (p <= 640); for those the cases put Vs there.
"""
import numpy as np
import pytest

import test_gpu_rounds as R
from test_gpu_rounds import G  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu

SEG = R.SEG                 # odd candidates per full segment; W = 2 SEG values
TA, TB1, TB = 96, 640, 1536  # dse_wheel_geometry.h: A | B1 | B2 | L
GEOMETRIES = [1, 2]


def _odd_primes_upto(n):
    s = np.ones(n // 2 + 1, dtype=bool)  # s[i]: 2i + 1
    s[0] = False
    for i in range(1, int(n ** 0.5) // 2 + 1):
        if s[i]:
            s[2 * i * (i + 1)::2 * i + 1] = False
    return [int(p) for p in 2 * np.flatnonzero(s) + 1]


PRIMES = _odd_primes_upto(1 << 20)
L_PRIMES = [p for p in PRIMES if p > TB]  # the L list of a table that reaches past TB


def test_shapes_are_what_the_cases_need():
    """The thresholds the shapes below are built on (CPU-only arithmetic, in
    this module so that a change of TB fails here and not as a vacuous pass)."""
    assert L_PRIMES[0] == 1543 and PRIMES[-1] == 1_048_573
    n1 = sum(79 < p <= TA for p in PRIMES) + (sum(TA < p <= TB1 for p in PRIMES) + 1) // 2 + \
        (sum(TB1 < p <= TB for p in PRIMES) + 3) // 4
    assert n1 == 80                                   # mid units of a table past TB
    assert 0 < _n2(10**9) < n1 and _n2(14 * 10**10) > n1 + 32


def _n2(v):
    """L units (128 primes each) of a segment near value v with every L set live."""
    r = int(v ** 0.5)
    return -(-sum(TB < p <= r for p in PRIMES) // 128)


@pytest.fixture(scope="module")
def lctx():
    from mail_sieve_e.sieve import Context
    c = Context(num_gpus=1)
    yield c
    c.close()


def _run(lctx, oracle, G, g0, nb, geometry, what, **opts):
    with R._options(lctx, wheel_geometry=geometry, **opts):
        m, c = lctx.sieve_odd_range(g0, nb)
    R._check(m, c, oracle, g0, nb, G, what=f"{what}, geometry {geometry}", seg_bits=SEG // geometry)


# ---- the L list's length -------------------------------------------------------

@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("n", [0, 1, 2, 64, 65, 128, 129])
def test_l_list_of_n_primes(lctx, oracle, G, n, geometry):
    """A window of 2^15 candidates that ends at q^2 - 2, q the (n + 1)-th prime
    above TB: the table ends with the n-th, so the L list holds n primes -- no
    set, one lane of one set, a full set, a second set of one lane (one unit of
    two sets), two full sets, and a third set (a second unit) of one lane; the
    lanes past the table's end load its last row and mark nothing. Just above
    (TB + 2)^2 every L prime's square lies inside the segment."""
    from mail_sieve_e import sieve as S
    q = L_PRIMES[n]
    vmax, nb = q * q - 2, 1 << 15
    g0 = (vmax - 3) // 2 - (nb - 1)
    assert g0 > 0 and S.base_limit_for_range(g0, nb) == q - 1
    _run(lctx, oracle, G, g0, nb, geometry, f"L list of {n} primes")


# ---- interleave shapes -----------------------------------------------------------

@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("start", ["1e9", "7e10"])
def test_interleave_of_mid_and_l_units(lctx, oracle, G, start, geometry):
    """Two segments and 777 candidates (four and a piece in the half geometry).
    From 1e9 + 7 the 25 L units are fewer than the 80 mid units (n2 < n1): the
    queue ends in a run of mid units, and an L unit's operands are requested
    across them. From 7e10 + 7 (values 1.4e11, V / 30 >= 2^32) the 247 L units
    exceed the mid units by more than 32: the queue ends in a long run of L
    units, longer than the 32 pre-assigned positions."""
    g0 = R._ragged({"1e9": R.G0_1E9, "7e10": R.G0_7E10}[start])
    _run(lctx, oracle, G, g0, 2 * SEG + 777, geometry, f"interleave from {start}")


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("g0,nb,units", [(0, 4000, 2), (29_000, 20_000, 23), (73_000, 20_000, 32), (76_500, 20_000, 33)])
def test_fewer_units_than_preassigned_positions(lctx, oracle, G, g0, nb, units, geometry):
    """Tables that end below TB: 2 units (base primes to 89: the two A primes),
    23, and 32 and 33 on either side of the 32 positions the 16 waves take
    without a claim: the positions past the queue's end decode to nothing, and
    the first claimed position is 32."""
    from mail_sieve_e import sieve as S
    lim = S.base_limit_for_range(g0, nb)
    assert lim <= TB
    n = sum(79 < p <= min(lim, TA) for p in PRIMES) + (sum(TA < p <= min(lim, TB1) for p in PRIMES) + 1) // 2 + \
        (sum(TB1 < p <= lim for p in PRIMES) + 3) // 4
    assert n == units, (lim, n)
    _run(lctx, oracle, G, g0, nb, geometry, f"{units} units")


# ---- several rounds ----------------------------------------------------------------

def test_three_rounds_pooled_over_three_chunks(lctx, oracle, G):
    """dse_sieve_all over P = 3 chunks and a dropped tail, N about 7.9e6 G [2.0e9
    on 256 CUs]: 2 G + 5 or more full segments in one launch, three rounds. A
    workgroup's next segment is in the same chunk (the roots of a segment G W
    further on) or in the next one (another V0)."""
    ns = -(-(2 * G + 5) // 3)
    with R._options(lctx, wheel_geometry=1):
        plan = R._sieve_all_vs_oracle(lctx, oracle, G, (ns - 1) * SEG + 777, 3, lambda k: k * ns)
    assert (plan["plan_max_rounds"], plan["plan_full_segments"], plan["plan_half_segments"],
            plan["plan_wheel_launches"]) == (3, 3 * ns + 1, 0, 1), plan


# ---- squares at a segment's start and end --------------------------------------------

@pytest.mark.parametrize("d", [-3, -1, 1, 3])
@pytest.mark.parametrize("p,geometry", [(1987, 1), (1987, 2), (1409, 2), (1_048_573, 1), (1_048_573, 2)],
                         ids=["L1987-full", "L1987-half", "B2-1409-half", "L1048573-full", "L1048573-half"])
def test_square_at_a_segment_seam(lctx, oracle, G, p, geometry, d):
    """Two segments whose seam is at p^2 + d: segment 0 has Vend - 1 = p^2 + d
    - 1 (p^2 - 4, p^2 - 2, p^2, p^2 + 2: p's set is live in it from d = 1 on),
    segment 1 has Vs = p^2 + d (p^2 inside it for d < 0, every mark from the
    segment's first period for d > 0), and ends after 777 candidates. p = 1987
    is the first prime with p^2 > W, 1409 a B2 prime with p^2 > W / 2, and
    1,048,573 the last prime of the largest table with rows: its seam is the
    top of the ranges without bucketed primes."""
    W = 2 * SEG // geometry
    assert p * p + d > W and (p * p + d) % 2 == 0
    g0 = (p * p + d - W - 2) // 2
    nb = W // 2 + 777
    assert 2 + 2 * g0 + W == p * p + d and 3 + 2 * (g0 + nb - 1) < (2**20 + 1)**2
    _run(lctx, oracle, G, g0, nb, geometry, f"seam at {p}^2 {d:+d}")


@pytest.mark.parametrize("d", [-3, -1, 1, 3])
@pytest.mark.parametrize("p", [1409, 631], ids=["B2-1409", "B1-631"])
def test_square_at_a_range_start(lctx, oracle, G, p, d):
    """Vs = p^2 + d in a range's first segment, for a B2 and a B1 prime (their
    squares lie below W, so no segment ends there), both geometries."""
    assert TB1 < 1409 <= TB and TA < 631 <= TB1
    g0 = (p * p + d - 2) // 2
    for geometry in GEOMETRIES:
        _run(lctx, oracle, G, g0, 1 << 15, geometry, f"range from {p}^2 {d:+d}")


# ---- the bucket instantiation ------------------------------------------------------------

@pytest.mark.parametrize("opts", [{}, {"bucket_lo_log2": 17}, {"bucket_pass_segments": 2}],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "production")
def test_bucket_units_between_l_units(lctx, oracle, G, opts):
    """Two segments and 777 candidates at 1e13 (V / 30 >= 2^38: the L units
    take their Barrett factors, need_m): bucket units interleave with the mid
    and L units from the queue's first position, every one of them claimed; with
    the primes above 2^17 bucketed the last L set
    is cut short, and in passes of two segments the second pass is one short
    segment."""
    g0, nb = R._ragged(R.G0_1E13), 2 * SEG + 777
    assert (2 + 2 * g0) // 30 >= 2**38
    with R._options(lctx, **opts):
        m, c = lctx.sieve_odd_range(g0, nb)
    assert lctx.debug_get_stat("plan_bucket_passes") == (2 if opts.get("bucket_pass_segments") else 1)
    R._check(m, c, oracle, g0, nb, G, what=f"1e13 {opts}")
