"""Reference for the power and reciprocal sums (include/dse.h "power and reciprocal
sums"), independent of the library: Python ints over numpy.flatnonzero of the test's
own bits, the pattern applied by tuples_ref's shifted ANDs. A plain module (like
tuples_ref.py), imported by the test modules that need it.
"""
import numpy as np

import tuples_ref as TR

T = TR.T
WORDS, NONE, POWER, RECIP, SHIFT = 17, (1 << 64) - 1, 1, 2, 126
ONE = 1 << SHIFT
TOP = 1 << 62  # the odd-index bound of every entry point
pack = TR.pack


def limbs(x, n):
    assert 0 <= x < 1 << (64 * n)
    return [(x >> (64 * k)) & NONE for k in range(n)]


def members(require):
    return [j for j in range(32) if (require >> j) & 1]


def brute(bits, g_start, require=1, forbid=0, above=(), flags=POWER | RECIP):
    """The 17 words of the dse_sums of bits ++ above at g_start, as a list of Python ints."""
    pos = TR.positions(bits, np.asarray(above, bool), require, forbid).tolist()
    base = 3 + 2 * g_start
    vals = [base + 2 * p for p in pos]
    s1 = sum(vals) if flags & POWER else 0
    s2 = sum(map(int.__mul__, vals, vals)) if flags & POWER else 0
    rc = sum(sum(map(ONE.__floordiv__, [v + 2 * j for v in vals])) for j in members(require)) if flags & RECIP else 0
    return ([g_start, len(bits), require, forbid, len(above), flags, len(pos),
             g_start + pos[0] if pos else NONE, g_start + pos[-1] if pos else NONE]
            + limbs(s1, 2) + limbs(s2, 3) + limbs(rc, 3))


def brute_values(vals, g_start, nbits, require=1, forbid=0, above_bits=0, flags=POWER | RECIP):
    """The same from the matches' values (a sorted list of Python ints)."""
    s1 = sum(vals) if flags & POWER else 0
    s2 = sum(v * v for v in vals) if flags & POWER else 0
    rc = sum(ONE // (v + 2 * j) for v in vals for j in members(require)) if flags & RECIP else 0
    return ([g_start, nbits, require, forbid, above_bits, flags, len(vals),
             (vals[0] - 3) // 2 if vals else NONE, (vals[-1] - 3) // 2 if vals else NONE]
            + limbs(s1, 2) + limbs(s2, 3) + limbs(rc, 3))


def ones_words(g_start, nbits, flags=POWER | RECIP, with_recip=True):
    """brute() of an all-ones mask with pattern 1 in closed form for the power sums (the masks of
    the carry cases are too long for a list of Python ints to be quick); recip by a loop."""
    a, n = 3 + 2 * g_start, nbits  # the values a, a + 2, ..., a + 2 (n - 1)
    s1 = n * a + n * (n - 1)
    s2 = n * a * a + 2 * a * n * (n - 1) + 4 * ((n - 1) * n * (2 * n - 1) // 6)
    rc = sum(ONE // v for v in range(a, a + 2 * n, 2)) if flags & RECIP and with_recip else 0
    return ([g_start, n, 1, 0, 0, flags, n, g_start if n else NONE, g_start + n - 1 if n else NONE]
            + limbs(s1 if flags & POWER else 0, 2) + limbs(s2 if flags & POWER else 0, 3) + limbs(rc, 3))


def words_of(s):
    """A Sums (or its words) as a list of Python ints."""
    return [int(x) for x in getattr(s, "words", s)]


NAMES = ("g_start", "nbits", "require", "forbid", "above_bits", "flags", "matches", "first_g", "last_g",
         "sum1[0]", "sum1[1]", "sum2[0]", "sum2[1]", "sum2[2]", "recip[0]", "recip[1]", "recip[2]")


def diff(got, want):
    """The members that differ, as text; empty when every word is equal."""
    g, w = words_of(got), words_of(want)
    assert len(g) == len(w) == WORDS
    return [f"{NAMES[i]}: got {g[i]:#x}, want {w[i]:#x}" for i in range(WORDS) if g[i] != w[i]]


def pack_garbage(bits):
    """pack() with every bit past the end of the last word set: the library must ignore them."""
    m = pack(bits).copy()
    if len(bits) & 63:
        m[-1] |= np.uint64(NONE ^ ((1 << (len(bits) & 63)) - 1))
    return m


def g_starts():
    return (0, 1, 37, 1 << 40)


def masks(nbits, seed):
    """Synthetic masks from all ones to one bit in 4096, and the empty mask."""
    rng = np.random.default_rng(seed)
    out = {"ones": np.ones(nbits, bool), "zero": np.zeros(nbits, bool)}
    for name, p in (("half", 0.5), ("8%", 0.08), ("1/4096", 1 / 4096)):
        out[name] = rng.random(nbits) < p
    return out


def odd_sieve(n):
    """bool array over the odd candidates 3, 5, ... < n: prime or not (numpy sieve)."""
    m = (n - 3 + 1) // 2
    s = np.ones(m, bool)
    for p in range(3, int(n ** 0.5) + 1, 2):
        if s[(p - 3) // 2]:
            s[(p * p - 3) // 2::p] = False
    return s
