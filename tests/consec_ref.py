"""Reference residue-pair matrices of consecutive entries of a bit string for the
tests, independent of the library: numpy on bool arrays (flatnonzero, the values'
classes mod q, np.bincount over the pairs of neighbours), laid out as the uint64
words of a dse_consec (include/dse.h). A plain module (like gaps_ref.py), imported
by test_consec_host.py and test_gpu_consec.py, which share its fills, sizes,
planted cases and pinned values. test_consec_host.py ties brute() to a plain
Python loop.

Bit i of a range that starts at g_start is the candidate g = g_start + i of value
3 + 2 g.
"""
import functools

import numpy as np

from race_ref import pack, pack_garbage  # noqa: F401  (shared with the callers)

MAX_MODULUS, NONE = 64, (1 << 64) - 1
BINS = MAX_MODULUS * MAX_MODULUS
WORDS = 7 + BINS
FIELDS = ([(n, i, i + 1) for i, n in enumerate(("g_start", "nbits", "q", "primes", "pairs", "first_g", "last_g"))]
          + [("counts", 7, WORDS)])
T = 256 * 64  # candidates per tile of the main kernel

FILLS = ("ones", "zero", "4096th", "half", "16th")
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 7 * T + 3]
G_STARTS = [0, 1, 2, 3, 4, 5, 6, 2**40 + 5]
# the periods T = 3, 2, 5, 7, 4, 6, 15, 63, 32: both in-word bodies, and one modulus on each side of
# the threshold between them (the period 5 is the last of the bit-parallel body, 6 the first of the other)
QS = [3, 4, 5, 7, 8, 12, 30, 63, 64]
REAL_LIMIT = 1_000_000

# N(a, b) of the odd primes 3 .. 10^6, by an odd-only numpy sieve and bincount
PINNED_1E6 = {
    3: {(0, 2): 1, (1, 1): 16_394, (1, 2): 22_837, (2, 1): 22_837, (2, 2): 16_427},
    4: {(1, 1): 16_603, (1, 3): 22_572, (3, 1): 22_572, (3, 3): 16_749},
    10: {(1, 1): 3_213, (1, 3): 6_299, (1, 7): 6_550, (1, 9): 3_555, (9, 1): 6_948, (9, 9): 3_155, (3, 5): 1,
         (5, 7): 1},
}
# of the odd primes 3 .. 10^8 (5,761,454 of them)
PINNED_1E8 = {
    3: {(1, 1): 1_264_047, (1, 2): 1_616_470, (2, 1): 1_616_470, (2, 2): 1_264_465, (0, 2): 1},
    4: {(1, 1): 1_277_323, (1, 3): 1_603_180, (3, 1): 1_603_181, (3, 3): 1_277_769},
    10: {(1, 1): 254_927, (1, 9): 300_650, (9, 1): 476_348, (9, 9): 254_684},
}
# of the 10^8 - 1 odd primes up to the 10^8-th prime 2,038,074,743 (Lemke Oliver and Soundararajan's range)
LOS_HI = 2_038_074_743
PINNED_LOS = {(1, 1): 4_623_041, (1, 3): 7_429_438, (1, 7): 7_504_612, (1, 9): 5_442_344,
              (3, 1): 6_010_981, (3, 3): 4_442_561, (3, 7): 7_043_695, (3, 9): 7_502_896,
              (7, 1): 6_373_982, (7, 3): 6_755_195, (7, 7): 4_439_355, (7, 9): 7_431_870,
              (9, 1): 7_991_431, (9, 3): 6_372_940, (9, 7): 6_012_739, (9, 9): 4_622_916}


def period(q):
    return q if q % 2 else q // 2


def brute(bits, g_start, q):
    """The dse_consec of the candidates [g_start, g_start + len(bits)) as uint64[WORDS]."""
    bits = np.asarray(bits, dtype=bool)
    g = g_start + np.flatnonzero(bits).astype(np.int64)
    v = (3 + 2 * g) % q
    w = np.zeros(WORDS, dtype=np.uint64)
    w[0], w[1], w[2], w[3] = g_start, len(bits), q, len(g)
    w[4] = max(len(g) - 1, 0)
    w[5] = w[6] = NONE
    if len(g):
        w[5], w[6] = int(g[0]), int(g[-1])
    w[7:] = np.bincount(v[:-1] * 64 + v[1:], minlength=BINS).astype(np.uint64)
    return w


def entry(words, a, b):
    return int(words[7 + 64 * a + b])


def diff(got, want):
    """Names of the struct members in which two word arrays differ."""
    return [n for n, a, b in FIELDS if not np.array_equal(got[a:b], want[a:b])]


def fill(name, nbits, seed):
    rng = np.random.default_rng(seed)
    if name == "ones":
        return np.ones(nbits, bool)
    if name == "zero":
        return np.zeros(nbits, bool)
    return rng.random(nbits) < {"4096th": 1 / 4096, "half": 0.5, "16th": 1 / 16}[name]


def stride(nbits):
    """Every 5th (g_start, q) of the family, from another start for every fill; every 11th and 17th of
    the two largest sizes, whose cases cost most. Up to T + 1 the five fills' starts 0, 3, 1, 4, 2
    cover all 72 cases; test_consec_host.py checks that every size sees every start and modulus."""
    return 5 if nbits <= T + 1 else 11 if nbits <= 2 * T + 5 else 17


def cases():
    return [(g, q) for q in QS for g in G_STARTS]


def thinned(nbits, k):
    """(g_start, q) of the thinned family of one size, for the k-th fill (race_ref.thinned's rule)."""
    return cases()[(3 * k) % stride(nbits)::stride(nbits)]


def planted(name):
    """bool[n]: two entries whose pair crosses the named seam, a few more entries around them so that
    a wrong class of either prime shows in another bin. Five or six tiles, so a cap of 3 workgroups
    gives runs of two tiles (2T and 4T are workgroup seams); the thousand empty tiles make runs of 335,
    the middle one empty."""
    lay = {
        "word seam": (4 * T + 5, 3 * 64 - 2, 3 * 64 + 9),
        "wave seam": (4 * T + 5, T + 64 * 64 - 1, T + 64 * 64 + 30),  # words 63 | 64 of tile 1
        "tile seam": (4 * T + 5, T - 20, T + 45),
        "workgroup seam": (4 * T + 5, 2 * T - 7, 2 * T + 100),
        "a thousand empty tiles": (1003 * T, T // 2, T // 2 + 1001 * T + 17),
        "an empty workgroup run": (6 * T, 2 * T - 300, 4 * T + 77),  # six tiles, grid 3: tiles 2 and 3 are one run
    }
    n, p, q = lay[name]
    bits = np.zeros(n, bool)
    bits[[5, 9, p - 64 - 3, p, q, q + 4, q + 64 + 11, n - 2]] = True
    return bits, p, q


PLANTED = ("word seam", "wave seam", "tile seam", "workgroup seam", "a thousand empty tiles",
           "an empty workgroup run")


@functools.lru_cache(maxsize=None)
def sieve_bits(limit):
    """bool: element g is True iff 3 + 2g <= limit is prime (an odd-only numpy sieve, independent of
    the oracle's)."""
    n = (limit - 3) // 2 + 1
    sv = np.ones(n, dtype=bool)
    g = 0
    while (3 + 2 * g) ** 2 <= limit:
        if sv[g]:
            p = 3 + 2 * g
            sv[(p * p - 3) // 2::p] = False
        g += 1
    sv.setflags(write=False)
    return sv
