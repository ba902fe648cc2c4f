"""The marking plan of the wheel kernel's mid classes B1 and B2, restated in
Python integers (dse_wheel_kernel.h unit_B1, unit_B2).

Both classes mark every hit class to the segment end with a wave-uniform mark
count taken from the unit's first prime: B1 lane (prime, plane, j = 0..3) issues
the hits n = 32j + r + 128t, t < T = floor(floor((KP - 1) / pmin) / 128) + 1, of
k = kp + n p; B2 lane (prime, plane, j = 0..1) issues n = 32j + r + 64t, t < T2 =
floor(floor((KP - 1) / pmin) / 64) + 1. A mark with k >= KP has no hit and must
land past the image, where the LDS drops it. For both geometries (KP = 2^17,
2^16), every unit the kernel forms from the build's thresholds and a range of
first hits kp, the tests check that
  - the lanes of a prime issue every hit index below S T exactly once, and every
    hit inside the segment is among them;
  - T stays within the cases class_marks_k has;
  - every issued mark without a hit has KP <= k < 2^31 - 32768 (the byte
    address k | plane + kImgOff stays a positive 32-bit offset, inside the
    range the out-of-range microbenchmark covered).
The thresholds come from the build (dse_debug_get_stat "wheel_*") where a
context can be made, else from the header's defaults.
"""
import os
import re

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-sieve-e_amd", "csrc")
K_LIMIT = 2**31 - 32768
GEOMETRIES = [1 << 17, 1 << 16]


def _header_defaults():
    s = open(os.path.join(CSRC, "dse_wheel_geometry.h")).read()
    return {k: int(re.search(rf"#define DSE_{k.upper()} (\d+)", s).group(1)) for k in ("ta", "tb1", "tb")}


@pytest.fixture(scope="module")
def thr():
    """TA, TB1, TB of the build; the header's defaults without a device."""
    try:
        from mail_sieve_e.sieve import Context
        with Context(num_gpus=1) as c:
            d = {k: c.debug_get_stat("wheel_" + k) for k in ("ta", "tb1", "tb")}
    except Exception:
        d = _header_defaults()
    assert 79 < d["ta"] < d["tb1"] <= d["tb"]
    return d


def class_marks_cases():
    s = open(os.path.join(CSRC, "dse_wheel_kernel.h")).read()
    body = s[s.index("void class_marks_k("):]
    body = body[:body.index("__builtin_unreachable")]
    cases = [int(a) for a, b in re.findall(r"case (\d+): class_marks<(\d+)>", body) if a == b]
    assert cases == list(range(1, len(cases) + 1))
    return cases[-1]


def primes_in(lo, hi):
    """Odd primes p with lo < p <= hi."""
    return [p for p in range(lo + 1 | 1, hi + 1, 2) if all(p % d for d in range(3, int(p**0.5) + 1, 2))]


def units_of(primes, size):
    return [primes[i:i + size] for i in range(0, len(primes), size)]


def check_unit(KP, unit, lanes_j, kps_of, max_case):
    """One unit: stride S = 32 lanes_j hits per class step, T from its first prime."""
    S = 32 * lanes_j
    pmin = unit[0]
    assert unit == sorted(unit)
    T = ((KP - 1) // pmin) // S + 1
    assert 1 <= T <= max_case, (KP, unit, T)
    j, r, t = np.meshgrid(np.arange(lanes_j), np.arange(32), np.arange(T), indexing="ij")
    n = (32 * j + r + S * t).ravel().astype(np.int64)
    assert np.array_equal(np.sort(n), np.arange(S * T)), "the lanes issue every hit index below S T once"
    checked = 0
    for p in unit:
        assert (S * p) % 32 == 0  # a class's marks share their bit: the stride is whole blocks
        for kp in kps_of(p):
            assert 0 <= kp < p
            k = kp + n * p
            hits = np.arange(kp, KP, p)                       # the hits inside the segment
            assert len(hits) and (len(hits) - 1) < S * T, (KP, p, kp, T)
            assert np.array_equal(np.sort(k[k < KP]), hits), (KP, p, kp)
            extra = k[k >= KP]                                # issued, no hit: dropped
            assert len(extra) == S * T - len(hits)
            if len(extra):
                assert KP <= int(extra.min()) and int(extra.max()) < K_LIMIT, (KP, p, kp)
                assert int(extra.max()) < S * T * unit[-1]
            checked += 1
    return checked


def run_class(KP, primes, size, lanes_j, max_case):
    units = units_of(primes, size)
    assert units
    total = 0
    for i, u in enumerate(units):
        if i in (0, len(units) - 1):
            kps = lambda p, u=u: range(u[0])                   # every kp < p_min
        else:
            kps = lambda p: (0, p - 1)
        total += check_unit(KP, u, lanes_j, kps, max_case)
    return len(units), total


@pytest.mark.parametrize("KP", GEOMETRIES)
def test_b1_plan(thr, KP):
    """Units of two consecutive primes of (TA, TB1], four lanes per plane."""
    nu, total = run_class(KP, primes_in(thr["ta"], thr["tb1"]), 2, 4, class_marks_cases())
    print(f"B1 KP={KP}: {nu} units, {total} (prime, kp) walks")


@pytest.mark.parametrize("KP", GEOMETRIES)
def test_b2_plan(thr, KP):
    """Units of four consecutive primes of (TB1, TB], two lanes per plane."""
    nu, total = run_class(KP, primes_in(thr["tb1"], thr["tb"]), 4, 2, class_marks_cases())
    print(f"B2 KP={KP}: {nu} units, {total} (prime, kp) walks")


def test_largest_mark_count_is_the_static_bound(thr):
    """T is largest for the smallest B1 prime in the full geometry, and the
    header's bound floor((KP - 1) / (128 (TA + 1))) + 1 covers it."""
    KP = GEOMETRIES[0]
    p0 = primes_in(thr["ta"], thr["tb1"])[0]
    T = ((KP - 1) // p0) // 128 + 1
    assert T <= (KP - 1) // (128 * (thr["ta"] + 1)) + 1 <= class_marks_cases()
    if thr == _header_defaults():
        assert (p0, T) == (97, 11)
