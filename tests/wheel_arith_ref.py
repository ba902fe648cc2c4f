"""Exact references and input families for the wheel kernel's integer helpers
(tests/test_gpu_wheel_arith.py runs the helpers on the device through
dse_debug_wheel_arith_dev; tests/test_wheel_arith_ref.py ties this module to
Python ints on the CPU).

Everything here is numpy uint64 arithmetic on operands below 2^63 (or a
Python-int pow for the modular inverse of 30), so it is exact by construction:
%, //, np.uint64(2**64 - 1) // p. Nothing is taken from the library."""
import numpy as np

U64 = np.uint64
R30 = (1, 7, 11, 13, 17, 19, 23, 29)
TOP_J = 8          # the largest quotients of every prime, always in a family
RANDOM_X = 64      # uniform values per prime


def odd_primes_upto(n):
    """Odd primes <= n, ascending, as uint64."""
    if n < 3:
        return np.zeros(0, dtype=U64)
    s = np.ones(n + 1, dtype=bool)
    s[:2] = False
    s[4::2] = False
    for i in range(3, int(n ** 0.5) + 1, 2):
        if s[i]:
            s[i * i::2 * i] = False
    p = np.nonzero(s)[0]
    return p[p > 2].astype(U64)


def u64(a):
    return np.ascontiguousarray(a, dtype=U64)


def ref_mod(x, p):
    return u64(x) % u64(p)


def ref_div(t, p):
    return u64(t) // u64(p)


def ref_div_ceil(t, p):
    t, p = u64(t), u64(p)
    return t // p + (t % p != 0).astype(U64)


def ref_mulmod(a, b, p):
    """a b mod p for a, b < 2^31 (the product is exact in uint64)."""
    return (u64(a) * u64(b)) % u64(p)


def ref_barrett_factor(p):
    return U64(2**64 - 1) // u64(p)


def ref_first_at_or_after(kp, start, p):
    """Smallest k >= start with k = kp (mod p), kp < p."""
    kp, start, p = u64(kp), u64(start), u64(p)
    d = np.where(start > kp, start - kp, U64(0))
    return kp + p * ref_div_ceil(d, p)


def inv30(p):
    """30^-1 mod p for each p coprime to 30 (Python-int pow), uint64."""
    return np.array([pow(30, -1, int(q)) for q in np.asarray(p).ravel()], dtype=U64).reshape(np.shape(p))


def ref_rows(p):
    """rows[i, j] = (-R30[j] * 30^-1) mod p[i]: the first k >= 0 with
    p | R30[j] + 30k. p coprime to 30, below 2^31."""
    p = u64(p)
    inv = inv30(p)
    r = np.array(R30, dtype=U64)[None, :] % p[:, None]
    neg = (p[:, None] - r) % p[:, None]
    return (neg * inv[:, None]) % p[:, None]


def plane_first_violations(Xs, rho, p, k):
    """Indices where k is not the smallest k >= 0 with p | Xs + rho + 30k. For
    p coprime to 30 the solutions are one residue class mod p, so the smallest
    is the one below p: k < p and p | Xs + rho + 30k say it all."""
    Xs, rho, p, k = u64(Xs), u64(rho), u64(p), u64(k)
    bad = (k >= p) | ((Xs + rho + U64(30) * np.minimum(k, p)) % p != 0)
    return np.flatnonzero(bad)


def pack(lo, hi):
    """lo | hi << 32, the two-operand ops' x."""
    return u64(lo) | (u64(hi) << U64(32))


def powers_in(lo, hi):
    """2^k - 1, 2^k, 2^k + 1 for every k with lo <= 2^k < hi."""
    out = []
    for k in range(64):
        if lo <= 2**k < hi:
            out += [2**k - 1, 2**k, 2**k + 1]
    return out


def residue_family(primes, lo, hi, nj, rng):
    """(x, p) pairs for a residue op with x in [lo, hi), hi <= 2^63. For each
    prime p: j p + d for d in {-1, 0, +1} with nj values of j drawn over the
    whole quotient range [lo // p, (hi - 1) // p] and the TOP_J largest j;
    2^k - 1, 2^k, 2^k + 1 for every 2^k in [lo, hi), where the float rounding
    of x changes step; hi - 1; RANDOM_X uniform values. All clipped into
    [lo, hi - 1]. Row i of the returned (len(primes), m) arrays belongs to
    primes[i]."""
    assert 0 <= lo < hi <= 2**63
    p = u64(primes)[:, None]
    n = p.shape[0]
    jlo, jhi = U64(lo) // p, U64(hi - 1) // p
    span = jhi - jlo + U64(1)
    j = jlo + rng.integers(0, 2**63, size=(n, nj), dtype=U64) % span
    top = jhi - np.minimum(np.arange(TOP_J, dtype=U64)[None, :], jhi - jlo)
    base = np.concatenate([j, top], axis=1) * p                       # <= hi - 1 < 2^63
    below = np.where(base > 0, base - U64(1), U64(0))
    fixed = np.array(powers_in(lo, hi) + [hi - 1], dtype=U64)
    rnd = U64(lo) + rng.integers(0, 2**63, size=(n, RANDOM_X), dtype=U64) % U64(hi - lo)
    x = np.concatenate([below, base, base + U64(1), np.broadcast_to(fixed, (n, len(fixed))), rnd], axis=1)
    x = np.clip(x, U64(lo), U64(hi - 1))
    return u64(x), u64(np.broadcast_to(p, x.shape))
