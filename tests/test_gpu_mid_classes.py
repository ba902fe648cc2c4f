"""The wheel kernel's mid classes B1 (TA < p <= TB1, two primes per wave) and B2
(TB1 < p <= TB, four primes per wave), which mark every hit class to the
segment end and let the LDS drop the marks past it, at the places where their
plan changes: the first segments (every p^2 inside: the one-at-a-time path) and
the first fast one; both sides of TB^2; the top of the plain kernel's range and
1e11; base tables that end inside the mid lists, so the last unit is partly
filled; and, for the first and last B2 unit, a witness of every prime in every
plane. Every case runs with wheel_geometry 1 (2^17 periods per segment) and 2
(2^16) and compares the whole mask and the count with the CPU oracle
(oracle.fast_sieve_range), or with Miller-Rabin (tests/primes_ref.py) for the
tiny ranges. Launches of several rounds are tests/test_gpu_rounds.py's.
"""
import numpy as np
import pytest

from primes_ref import is_prime_mr, mask_bits, mr_window, next_prime, prev_prime, witness

pytestmark = pytest.mark.gpu

SEG = {1: 1_966_080, 2: 983_040}   # odd candidates per segment of wheel_geometry 1 and 2
R30 = (1, 7, 11, 13, 17, 19, 23, 29)
GEOMETRIES = [1, 2]


@pytest.fixture(scope="module")
def gctx():
    """One context per wheel_geometry, and the build's thresholds."""
    from mail_sieve_e.sieve import Context
    cs = {}
    for g in GEOMETRIES:
        cs[g] = Context(num_gpus=1)
        cs[g].debug_set_option("wheel_geometry", g)
    thr = {k: cs[1].debug_get_stat("wheel_" + k) for k in ("ta", "tb1", "tb", "max_prime")}
    assert 79 < thr["ta"] < thr["tb1"] < thr["tb"] < thr["max_prime"]
    yield cs, thr
    for c in cs.values():
        c.close()


_REF = {}


def ref_of(oracle, g0, nb):
    """The oracle's (mask, count) of a range, computed once and read-only."""
    if (g0, nb) not in _REF:
        m, c = oracle.fast_sieve_range(g0, nb)
        m.setflags(write=False)
        _REF[g0, nb] = (m, int(c))
    return _REF[g0, nb]


def least_factor(v, bound=1 << 21):
    for d in range(3, bound, 2):
        if v % d == 0:
            return d
    return v


def compare(m, c, m_ref, c_ref, g0, nb, what):
    """Whole masks; the first wrong candidate by value, with its least prime factor."""
    x = np.asarray(m).view(np.uint64) ^ np.asarray(m_ref).view(np.uint64)
    bad = np.flatnonzero(x)
    if len(bad):
        w = int(bad[0])
        low = int(x[w])
        j = 64 * w + ((low & -low).bit_length() - 1)
        v = 3 + 2 * (g0 + j)
        left = bool(int(np.asarray(m).view(np.uint64)[w]) >> (j & 63) & 1)
        how = f"a composite left set, least prime factor {least_factor(v)}" if left else "a prime cleared"
        pytest.fail(f"{what}: {len(bad)} wrong words; first wrong value {v} (candidate {j} of {nb} from g0 = {g0}): {how}",
                    pytrace=False)
    assert int(c) == int(c_ref), (what, int(c), int(c_ref))


def run_case(gctx, oracle, geo, g0, nb, what):
    cs, _ = gctx
    m_ref, c_ref = ref_of(oracle, g0, nb)
    m, c = cs[geo].sieve_odd_range(g0, nb)
    compare(m, c, m_ref, c_ref, g0, nb, f"{what}, wheel_geometry {geo}")
    return m


def g_of(v):
    """Candidate index of the odd value v."""
    assert v % 2 == 1 and v >= 3
    return (v - 3) // 2


# ---- 1. the first segments --------------------------------------------------------

@pytest.mark.parametrize("geo", GEOMETRIES)
def test_first_two_segments(gctx, oracle, geo):
    """g_start = 0: every mid prime has its square inside the first segment of
    2^17 periods (of 3.9e6 values; the first two of 2^16), where the units walk
    one hit at a time from p^2, and the last segment is on the class path for
    all but the largest B2 primes of the half geometry."""
    _, thr = gctx
    assert thr["tb"] ** 2 < 3 + 2 * SEG[1] and thr["tb1"] ** 2 < 3 + 2 * SEG[2]
    run_case(gctx, oracle, geo, 0, 2 * SEG[geo], "two segments from 3")


# ---- 2. both sides of TB^2 ----------------------------------------------------------

@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_three_segments_at_tb_squared(gctx, oracle, geo, side):
    """Three segments from just below / just above the value TB^2: below, the
    largest B2 primes' squares lie inside the first segment (the unit decides
    by pmax), above, every mid unit of every segment is on the class path."""
    _, thr = gctx
    v = thr["tb"] ** 2 + (-211 if side == "below" else 211)
    run_case(gctx, oracle, geo, g_of(v | 1), 3 * SEG[geo] + 777, f"three segments from just {side} TB^2")


# ---- 3. the top of the plain kernel's range, and 1e11 --------------------------------

@pytest.mark.parametrize("where", ["2p40", "1e11"])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_two_segments_high(gctx, oracle, geo, where):
    """Two segments that end just below (2^20)^2 (every L set live, the largest
    Kb the plain kernel meets), and two that end at 1e11 (the benchmark's top)."""
    top = 2**40 - 1 if where == "2p40" else 10**11 - 1
    nb = 2 * SEG[geo]
    run_case(gctx, oracle, geo, g_of(top) - nb + 1, nb, f"two segments ending at {top}")


# ---- 4. tables that end inside the mid lists ------------------------------------------

def _odd_primes(lo, hi):
    return [p for p in range(lo + 1 | 1, hi + 1, 2) if is_prime_mr(p)]


TINY_Q = [97, 101, 103, 641, 643, 647, 653, 659, 1531]


@pytest.mark.parametrize("q", TINY_Q)
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_table_ends_inside_a_mid_list(gctx, geo, q):
    """The range (q^2, q'^2), q' the next prime: its base table ends at q, and
    every table prime has its square below the range, so the mid units run the
    class path with a last unit of 1 (q = 97, 103), 2 (101) primes in B1, and of
    1, 2, 3, 4, 1 primes in B2 (q = 641 .. 659); q = 1531 is the whole B2 list
    with no L prime. Against Miller-Rabin."""
    from mail_sieve_e import sieve as S
    cs, thr = gctx
    if (thr["ta"], thr["tb1"], thr["tb"]) != (96, 640, 1536):
        pytest.fail("TINY_Q is chosen for the thresholds 96 / 640 / 1536: choose new q for this build")
    g0, g1 = g_of(q * q) + 1, g_of(next_prime(q + 1) ** 2)   # candidates q^2 + 2 .. q'^2 - 2
    nb = g1 - g0
    limit = S.base_limit_for_range(g0, nb)
    assert prev_prime(limit) == q, (q, limit)
    n_b1 = len(_odd_primes(thr["ta"], min(thr["tb1"], limit)))
    n_b2 = len(_odd_primes(thr["tb1"], min(thr["tb"], limit)))
    n_l = len(_odd_primes(thr["tb"], limit))
    want = {97: (1, 0), 101: (2, 0), 103: (3, 0), 641: (None, 1), 643: (None, 2), 647: (None, 3), 653: (None, 4),
            659: (None, 5), 1531: (None, len(_odd_primes(640, 1536)))}[q]
    assert n_l == 0 and n_b2 == want[1] and (want[0] is None or n_b1 == want[0]), (q, n_b1, n_b2, n_l)
    m, c = cs[geo].sieve_odd_range(g0, nb)
    bits, ref = mask_bits(m, nb), mr_window(g0, nb)
    bad = np.flatnonzero(bits != ref)
    assert len(bad) == 0, (q, geo, [(3 + 2 * (g0 + int(j)), bool(bits[j]), least_factor(3 + 2 * (g0 + int(j)), 2000))
                                    for j in bad[:8]])
    assert c == int(ref.sum())


# ---- 5. a witness of every prime of the first and last B2 unit in every plane ---------

def plane_witnesses(p, V):
    """{residue mod 30: witness(p, V')} for the 8 residues coprime to 30: the
    witnesses of p from V upwards, until each residue class has one."""
    out = {}
    while len(out) < 8:
        w = witness(p, V)
        if w % 30 in R30:
            out.setdefault(w % 30, w)
        V = w + 1
    assert sorted(out) == list(R30)
    return out


@pytest.mark.parametrize("unit", ["first", "last"])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_b2_unit_witnesses(gctx, oracle, geo, unit):
    """One window from V = 1e9 + 1 that holds, for each prime of the B2 list's
    first (last) unit of four and each of the 8 planes, a composite whose least
    prime factor is that prime: only its quarter-wave's lanes of that plane
    clear the bit, so a lost quarter-wave, plane or j names its prime."""
    _, thr = gctx
    b2 = _odd_primes(thr["tb1"], thr["tb"])
    units = [b2[i:i + 4] for i in range(0, len(b2), 4)]
    primes = units[0] if unit == "first" else units[-1]
    V = 10**9 + 1
    g0 = g_of(V)
    ws = {p: plane_witnesses(p, V) for p in primes}
    nb = max(g_of(w) for d in ws.values() for w in d.values()) - g0 + 1
    nb = -(-nb // SEG[2]) * SEG[2] + 777
    assert nb <= 4 * SEG[1], nb   # a handful of segments
    m = run_case(gctx, oracle, geo, g0, nb, f"witness window of the {unit} B2 unit {primes}")
    bits = mask_bits(m, nb)
    for p, d in ws.items():
        for r, w in d.items():
            assert w % p == 0 and is_prime_mr(w // p) and w // p >= p
            assert not bits[g_of(w) - g0], (f"witness {w} = {p} * {w // p} (residue {r} mod 30) left set: prime {p} of the "
                                            f"{unit} B2 unit {primes} lost in that plane, wheel_geometry {geo}")
