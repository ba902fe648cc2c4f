"""tests/wheel_arith_ref.py against Python ints, on the CPU: every reference the
device tests of the wheel kernel's arithmetic compare with
(tests/test_gpu_wheel_arith.py), and the input families, which must really
hold the boundary cases they are there for -- a generator bug that empties a
family would otherwise leave the device tests passing on nothing."""
import random

import numpy as np

import wheel_arith_ref as R

TB, PMAX = 1536, 1 << 20  # the shipped build's thresholds; any values would do here


def _pairs(rng, n, xmax, pmin, pmax):
    x = [rng.randrange(xmax) for _ in range(n)] + [0, 1, xmax - 1]
    p = [rng.randrange(pmin, pmax) for _ in range(n)] + [pmin, pmax - 1, pmin]
    return x, p


def test_references_match_python_ints():
    rng = random.Random(0xA71)
    for xmax, pmin, pmax in ((2**32, TB + 1, PMAX + 1), (2**38, TB + 1, PMAX + 1), (2**63, 2, 2**32), (2**24, 7, TB + 1)):
        x, p = _pairs(rng, 3000, xmax, pmin, pmax)
        assert R.ref_mod(x, p).tolist() == [a % b for a, b in zip(x, p)]
        assert R.ref_div(x, p).tolist() == [a // b for a, b in zip(x, p)]
        assert R.ref_div_ceil(x, p).tolist() == [-(-a // b) for a, b in zip(x, p)]
    p = [rng.randrange(2, 2**32) for _ in range(3000)] + [2, 3, 2**32 - 1, 2**31, 2**31 + 1]
    assert R.ref_barrett_factor(p).tolist() == [(2**64 - 1) // q for q in p]
    p = [rng.randrange(7, TB + 1) for _ in range(3000)]
    a, b = [rng.randrange(q) for q in p], [rng.randrange(q) for q in p]
    assert R.ref_mulmod(a, b, p).tolist() == [u * v % q for u, v, q in zip(a, b, p)]
    x = R.pack(a, b)
    assert x.tolist() == [u | v << 32 for u, v in zip(a, b)]
    start = [rng.randrange(2**23) for _ in p]
    got = R.ref_first_at_or_after(a, start, p).tolist()
    for k, kp, s, q in zip(got, a, start, p):
        assert k >= s and k >= kp and k % q == kp and (k - q < s or k == kp)


def test_rows_by_definition():
    primes = R.odd_primes_upto(5000)
    primes = primes[primes >= 7]
    rows = R.ref_rows(np.concatenate([primes, R.odd_primes_upto(PMAX)[-50:]]))
    allp = np.concatenate([primes, R.odd_primes_upto(PMAX)[-50:]]).tolist()
    for q, row in zip(allp, rows.tolist()):
        for r, k in zip(R.R30, row):
            assert 0 <= k < q and (r + 30 * k) % q == 0
            assert k == (-r * pow(30, -1, q)) % q
    assert R.inv30([7, 11, 1048573]).tolist() == [pow(30, -1, 7), pow(30, -1, 11), pow(30, -1, 1048573)]


def test_plane_first_check_accepts_the_answer_only():
    rng = random.Random(5)
    primes = [int(q) for q in R.odd_primes_upto(TB) if q > 79]
    for q in rng.sample(primes, 40):
        for rho in R.R30:
            Xs = rng.randrange(q)
            k = next(k for k in range(q) if (Xs + rho + 30 * k) % q == 0)
            assert len(R.plane_first_violations([Xs], [rho], [q], [k])) == 0
            for wrong in (k + 1, k + q, (k - 1) % q, 2**40 + k):
                assert len(R.plane_first_violations([Xs], [rho], [q], [wrong])) == 1


def test_primes_are_the_odd_primes():
    p = R.odd_primes_upto(2000).tolist()
    assert p == [n for n in range(3, 2001) if all(n % d for d in range(2, int(n**0.5) + 1))]
    assert len(R.odd_primes_upto(PMAX)) == 82024 and len(R.odd_primes_upto(2)) == 0


def test_families_hold_their_boundary_cases():
    rng = np.random.default_rng(11)
    primes = R.odd_primes_upto(PMAX)
    lprimes = primes[primes > TB]
    sample = np.concatenate([lprimes[:40], lprimes[-40:]])
    top62 = (2**62 - 1) // 30 + 1
    for lo, hi in ((0, 2**32), (0, 2**38), (0, 2**38 + 2**20), (2**38 - 2**20, 2**38 + 2**20), (2**38, top62),
                   (0, 2**63)):
        nj = 64
        x, p = R.residue_family(sample, lo, hi, nj, rng)
        assert x.shape == p.shape == (len(sample), 3 * (nj + R.TOP_J) + len(R.powers_in(lo, hi)) + 1 + R.RANDOM_X)
        assert x.dtype == p.dtype == np.uint64
        for xi, pi in zip(x.tolist(), p.tolist()):
            q = pi[0]
            assert all(v == q for v in pi) and all(lo <= v < hi for v in xi)
            res = {v % q for v in xi}
            assert {0, 1, q - 1} <= res                              # multiples of p and both neighbours
            js = {v // q for v in xi}
            for t in range(min(R.TOP_J, (hi - 1) // q - lo // q + 1)):   # the largest quotients, each as a multiple
                assert ((hi - 1) // q - t) * q in xi or ((hi - 1) // q - t) * q < lo
            assert (hi - 1) // q in js and hi - 1 in xi
            for k in range(64):
                if lo <= 2**k < hi:
                    assert 2**k in xi and (2**k - 1 in xi or 2**k == lo) and (2**k + 1 in xi or 2**k + 1 == hi)
            # the random quotients spread over the whole range, not one end of it
            if (hi - lo) // q > 1000:
                mid = (lo // q + (hi - 1) // q) // 2
                drawn = [v // q for v in xi[:nj]]
                assert min(drawn) < mid < max(drawn)
            assert len(set(xi[-R.RANDOM_X:])) > R.RANDOM_X // 2
    assert R.powers_in(0, 2**32)[:4] == [0, 1, 2, 1] and len(R.powers_in(0, 2**32)) == 96
    assert R.powers_in(2**38 - 2**20, 2**38 + 2**20) == [2**38 - 1, 2**38, 2**38 + 1]
