"""Reference residue-class counts and prime races of a bit string for the tests,
independent of the library: numpy on bool arrays, np.bincount(v % q) for the
classes, np.cumsum of +-1 over the entries of the two classes for the race,
argmax / argmin for first attainment, laid out as the uint64 words of a dse_race
(include/dse.h). A plain module (like goldbach_ref.py), imported by
test_race_host.py and test_gpu_race.py, which share its fills, sizes and cases.

Bit i of a range that starts at g_start is the candidate g = g_start + i of value
3 + 2 g.
"""
import numpy as np

MAX_MODULUS, NONE = 64, (1 << 64) - 1
WORDS = 17 + MAX_MODULUS
FIELDS = [(n, i, i + 1) for i, n in enumerate(
    ("g_start", "nbits", "q", "a", "b", "d_start", "d_end", "steps", "a_ahead", "b_ahead", "ties", "first_a_ahead",
     "first_b_ahead", "max_d", "max_g", "min_d", "min_g"))] + [("counts", 17, WORDS)]
T = 256 * 64
M64 = (1 << 64) - 1


def brute(bits, g_start, q, a, b, d_start=0):
    """The dse_race of the bits: uint64[WORDS]."""
    bits = np.asarray(bits, dtype=bool)
    g = g_start + np.flatnonzero(bits).astype(np.int64)
    cls = (3 + 2 * g) % q
    w = [0] * WORDS
    w[0], w[1], w[2], w[3], w[4] = g_start, len(bits), q, a, b
    w[17:17 + q] = [int(c) for c in np.bincount(cls, minlength=q)]
    w[11] = w[12] = w[14] = w[16] = NONE
    if a != b:
        step = (cls == a) | (cls == b)
        sg = g[step]
        D = d_start + np.cumsum(np.where(cls[step] == a, 1, -1), dtype=np.int64)
        w[5] = d_start & M64
        w[7] = len(D)
        w[6] = w[13] = w[15] = d_start & M64
        if len(D):
            w[6] = int(D[-1]) & M64
            w[8], w[9], w[10] = int((D > 0).sum()), int((D < 0).sum()), int((D == 0).sum())
            if (D > 0).any():
                w[11] = int(sg[np.argmax(D > 0)])
            if (D < 0).any():
                w[12] = int(sg[np.argmax(D < 0)])
            w[13], w[14] = int(D.max()) & M64, int(sg[np.argmax(D)])
            w[15], w[16] = int(D.min()) & M64, int(sg[np.argmin(D)])
    return np.array(w, dtype=np.uint64)


def signed(v):
    v = int(v)
    return v - (1 << 64) if v >> 63 else v


def diff(got, want):
    """Names of the struct members in which two word arrays differ."""
    return [n for n, a, b in FIELDS if not np.array_equal(got[a:b], want[a:b])]


def pack(bits):
    """bool array -> uint64 mask words (zero past the end)."""
    by = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    out = np.zeros((len(bits) + 63) // 64 * 8, dtype=np.uint8)
    out[:len(by)] = by
    return out.view(np.uint64)


def pack_garbage(bits):
    """pack, with every bit past the end of the last word set: they must be ignored."""
    m = pack(bits)
    if len(bits) % 64:
        m[-1] |= np.uint64(M64) << np.uint64(len(bits) % 64)
    return m


# -- the synthetic family -------------------------------------------------------------------
FILLS = ("ones", "zero", "4096th", "half", "16th", "alternating")
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 7 * T + 3]
# 0, 1, every residue mod T for q = 7 (T = 7) and q = 12 (T = 6), and a high start
G_STARTS = [0, 1, 2, 3, 4, 5, 6, 2**40 + 5]
QS = [3, 4, 5, 7, 8, 12, 30, 63, 64]
D_STARTS = [0, 3, -3, -70, 2**40, -2**40]


def prime_factors(q):
    return [p for p in range(2, q + 1) if q % p == 0 and all(p % d for d in range(2, p))]


def pairs(q):
    """(a, b) of the family for q: 1 against -1, the class of every prime that divides q against 1
    (for q even the class of 2 holds no odd candidate), and -1 against the class of 2 (0 for q = 3)."""
    return [(1, q - 1)] + [(p % q, 1) for p in prime_factors(q)] + [(q - 1, 2 if q > 3 else 0)]


def has_candidates(q, r):
    return q % 2 == 1 or r % 2 == 1


def fill(name, nbits, seed, g_start=0, q=4, a=1, b=3):
    """bool[nbits]. "alternating" depends on the case: of the candidates of the classes a and b it
    keeps the first of every run of one class, so the steps alternate and, from d_start = 0, D
    returns to 0 at every second step, inside most words."""
    rng = np.random.default_rng(seed)
    if name == "ones":
        return np.ones(nbits, bool)
    if name == "zero":
        return np.zeros(nbits, bool)
    if name == "4096th":
        return rng.random(nbits) < 1 / 4096
    if name == "half":
        return rng.random(nbits) < 0.5
    if name == "16th":
        return rng.random(nbits) < 1 / 16
    cls = (3 + 2 * (g_start + np.arange(nbits, dtype=np.int64))) % q
    pos = np.flatnonzero((cls == a) | (cls == b))
    s = np.zeros(nbits, bool)
    if len(pos):
        c = cls[pos]
        s[pos[np.concatenate([[True], c[1:] != c[:-1]])]] = True
    return s


def stride(nbits):
    """Every 13th case of the family, from another start for every fill; every 61st and 89th of the
    two largest sizes, whose cases cost most."""
    return 13 if nbits <= T + 1 else 61 if nbits <= 2 * T + 5 else 89


def cases():
    return [(g, q, a, b, d) for q in QS for a, b in pairs(q) for g in G_STARTS for d in D_STARTS]


def thinned(nbits, k):
    """(g_start, q, a, b, d_start) of the thinned family of one size, for the k-th fill."""
    return cases()[(5 * k) % stride(nbits)::stride(nbits)]
