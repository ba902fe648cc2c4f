"""Reference primality for the tests, independent of the kernels and of the C
oracle: deterministic Miller-Rabin in Python integers, and what the
top-of-range and prime-class tests build from it. A plain module (like
clj_reader.py), imported by the test modules that need it.
"""
import numpy as np

# the first 12 primes: as Miller-Rabin bases they leave no strong pseudoprime
# below 3.3e24 (Sorenson & Webster 2015)
MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def is_prime_mr(n):
    """Deterministic Miller-Rabin for n < 3.3e24 (first 12 prime bases)."""
    if n < 2:
        return False
    for p in MR_BASES:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prev_prime(n):
    """Largest prime <= n (n >= 2)."""
    if n < 2:
        raise ValueError("no prime below 2")
    while not is_prime_mr(n):
        n -= 1
    return n


def next_prime(n):
    """Smallest prime >= n."""
    n = max(n, 2)
    while not is_prime_mr(n):
        n += 1
    return n


# odd primes below 256, by trial division: mr_window strikes their multiples
# before it runs Miller-Rabin on what is left (about a quarter of a window)
_SMALL = [q for q in range(3, 256, 2) if all(q % d for d in range(3, q, 2))]


def mr_window(g0, nb):
    """bool[nb]: element j is True iff the odd value 3 + 2 (g0 + j) is prime.
    Every value is a Python integer (no 64-bit wrap at any offset)."""
    v0 = 3 + 2 * g0
    live = np.ones(nb, dtype=bool)
    for q in _SMALL:
        # first j with q | v0 + 2j: j = -v0 / 2 mod q
        j = (-v0 * ((q + 1) // 2)) % q
        if v0 + 2 * j == q:  # the prime itself stays
            j += q
        live[j::q] = False
    out = np.zeros(nb, dtype=bool)
    for j in np.flatnonzero(live):
        out[j] = is_prime_mr(v0 + 2 * int(j))
    return out


def witness(p, V):
    """p * c with c the smallest prime >= max(p, ceil(V / p)): a composite at
    or just above max(V, p^2) whose least prime factor is p, so of all the
    sieving primes only p's walk clears its bit."""
    return p * next_prime(max(p, -(-V // p)))


def mask_bits(mask, nb):
    """The first nb bits of a little-endian uint64 mask as bool[nb]."""
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:nb].astype(bool)
