"""Reference statistics of a bit string for the tests, independent of the
library: numpy brute force on bool arrays (shifted ANDs for the patterns, diff
of flatnonzero for the gaps), laid out as the uint64 words of a dse_stats
(include/dse.h). A plain module (like primes_ref.py), imported by
test_stats_host.py and test_gpu_stats.py, which share its sizes, masks, range
starts and patterns.
"""
import numpy as np

WORDS, BINS, NONE = 27 + 1024, 1024, (1 << 64) - 1
FIELDS = ([(n, i, i + 1) for i, n in enumerate(("g_start", "nbits", "primes", "first_g", "last_g", "head", "tail",
                                                "npatterns"))] +
          [("pattern", 8, 16), ("matches", 16, 24), ("max_gap", 24, 25), ("max_gap_g", 25, 26),
           ("gap_overflow", 26, 27), ("gaps", 27, WORDS)])

CONSTELLATIONS = (0b11, 0b1011, 0b1101, 0b11011, 0b1011011, 0b1101101, 0b101101101)
# the named patterns cannot all ride with two more in one call of 8: two lists cover them
PATTERN_LISTS = (CONSTELLATIONS + (1,), (1 | 1 << 31, 0b11, 1, 0b101101101))


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
        m[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(len(bits) % 64)
    return m


def brute(bits, g_start, patterns):
    """The dse_stats of the candidates [g_start, g_start + len(bits)) as uint64[WORDS]."""
    bits = np.asarray(bits, dtype=bool)
    n = len(bits)
    w = [0] * WORDS
    w[0], w[1] = g_start, n
    idx = np.flatnonzero(bits)
    w[2] = len(idx)
    w[3] = g_start + int(idx[0]) if len(idx) else NONE
    w[4] = g_start + int(idx[-1]) if len(idx) else NONE
    k = min(64, n)
    w[5] = sum(1 << i for i in range(k) if bits[i])
    w[6] = sum(1 << (63 - i) for i in range(k) if bits[n - 1 - i])
    w[7] = len(patterns)
    for p, pat in enumerate(patterns):
        m = bits.copy()
        for j in range(1, 32):
            if pat >> j & 1:
                sh = np.zeros(n, dtype=bool)
                if j < n:
                    sh[:n - j] = bits[j:]
                m &= sh
        w[8 + p] = pat
        w[16 + p] = int(m.sum())
    d = np.diff(idx)
    w[25] = NONE
    if len(d):
        kmax = int(np.argmax(d))  # the first of the largest
        w[24] = 2 * int(d[kmax])
        w[25] = g_start + int(idx[kmax])
        w[26] = int((d >= BINS).sum())
        hist = np.bincount(d[d < BINS], minlength=BINS)
        for i in np.flatnonzero(hist):
            w[27 + int(i)] = int(hist[i])
    return np.array(w, dtype=np.uint64)


def diff(got, want):
    """Names of the struct members in which two word arrays differ."""
    return [n for n, a, b in FIELDS if not np.array_equal(got[a:b], want[a:b])]


def sizes(T):
    return [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T + 37]


def masks(nbits, T, seed):
    """name -> bool[nbits]"""
    rng = np.random.default_rng(seed)
    out = {"half": rng.random(nbits) < 0.5, "twentieth": rng.random(nbits) < 1 / 20,
           "zero": np.zeros(nbits, bool), "ones": np.ones(nbits, bool)}
    for name, pos in (("first", 0), ("last", nbits - 1), ("seam-", T - 1), ("seam+", T)):
        if 0 <= pos < nbits:
            out[name] = np.zeros(nbits, bool)
            out[name][pos] = True
    if nbits > 2048 + 7:  # two primes 2048 + 5 places apart: the overflow bin, max_gap exact
        out["far"] = np.zeros(nbits, bool)
        out["far"][[3, 3 + 2048 + 5]] = True
    if nbits > 2 * 2100:  # and with ordinary gaps around them
        out["far+"] = rng.random(nbits) < 1 / 20
        out["far+"][1000:1000 + 2100] = False
    return out


def g_starts(nbits, T):
    # 0; the value 2^32 + 1 (odd index 2^31 - 1) in the middle of the first tile; the last value 2^62 - 1
    return [0, 2**31 - 1 - min(nbits, T) // 2, 2**61 - 1 - nbits]
