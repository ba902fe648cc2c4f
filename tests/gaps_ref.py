"""Reference first-occurrence tables of a bit string for the tests, independent of
the library: numpy on bool arrays (flatnonzero, diff, the first index of every
distinct difference), laid out as the uint64 words of a dse_gaps (include/dse.h).
A plain module (like stats_ref.py), imported by test_gaps_host.py and
test_gpu_gaps.py, which share its sizes, masks, range starts, planted cases and
published values. test_gaps_host.py ties brute() to a plain Python loop.
"""
import functools

import numpy as np

from stats_ref import pack, pack_garbage  # noqa: F401  (shared with the callers)

BINS, NONE = 1024, (1 << 64) - 1
WORDS = 9 + BINS
FIELDS = ([(n, i, i + 1) for i, n in enumerate(("g_start", "nbits", "primes", "first_g", "last_g", "found", "max_gap",
                                                "max_gap_g", "overflow_g"))] + [("first", 9, WORDS)])

# gap value -> lower prime of its first occurrence (A000230), as far as the tests go
FIRST = {2: 3, 4: 7, 6: 23, 8: 89, 10: 139, 12: 199, 14: 113, 16: 1831, 18: 523, 20: 887, 22: 1129, 24: 1669,
         26: 2477, 28: 2971, 30: 4297, 32: 5591, 34: 1327, 36: 9551, 38: 30593, 40: 19333, 72: 31397, 74: 404597,
         80: 542603}
# the maximal gaps (A005250 at A002386) below 2.1e7, below 1e9, below 1e10 and the two that end the list at 1e11
RECORDS_21M = [(2, 3), (4, 7), (6, 23), (8, 89), (14, 113), (18, 523), (20, 887), (22, 1129), (34, 1327), (36, 9551),
               (44, 15683), (52, 19609), (72, 31397), (86, 155921), (96, 360653), (112, 370261), (114, 492113),
               (118, 1349533), (132, 1357201), (148, 2010733), (154, 4652353), (180, 17051707), (210, 20831323)]
RECORDS_1E9 = RECORDS_21M + [(220, 47326693), (222, 122164747), (234, 189695659), (248, 191912783),
                             (250, 387096133), (282, 436273009)]
RECORDS_1E10 = RECORDS_1E9 + [(288, 1294268491), (292, 1453168141), (320, 2300942549), (336, 3842610773),
                              (354, 4302407359)]
REAL_LIMIT = 21_000_000
PLANTED_D = (3, 16, 17, 31, 32, 63, 64, 200, 1023, 1024)


def brute(bits, g_start):
    """The dse_gaps of the candidates [g_start, g_start + len(bits)) as uint64[WORDS]."""
    bits = np.asarray(bits, dtype=bool)
    w = np.full(WORDS, NONE, dtype=np.uint64)
    idx = np.flatnonzero(bits)
    w[0], w[1], w[2] = g_start, len(bits), len(idx)
    if len(idx):
        w[3], w[4] = g_start + int(idx[0]), g_start + int(idx[-1])
    w[5] = w[6] = 0
    d = np.diff(idx)
    if len(d):
        vals, at = np.unique(d, return_index=True)  # the first index of every distinct difference
        for v, k in zip(vals, at):
            if v < BINS:
                w[9 + int(v)] = g_start + int(idx[k])
        big = np.flatnonzero(d >= BINS)
        if len(big):
            w[8] = g_start + int(idx[big[0]])
        kmax = int(np.argmax(d))  # the first of the largest
        w[6], w[7] = 2 * int(d[kmax]), g_start + int(idx[kmax])
        w[5] = int((vals < BINS).sum())
    return w


def records(words):
    """[(gap value, lower prime)] of the maximal gaps of a dse_gaps' words, by gap: the bins that no
    longer gap (a higher bin, the overflow bin) precedes."""
    first = [int(v) for v in words[9:WORDS]]
    out = []
    for d in range(1, BINS):
        if first[d] == NONE:
            continue
        later = [first[e] for e in range(d + 1, BINS)] + [int(words[8])]
        if all(first[d] < x for x in later):
            out.append((2 * d, 3 + 2 * first[d]))
    return out


def first_primes(words):
    return [(2 * d, 3 + 2 * int(words[9 + d])) for d in range(BINS) if int(words[9 + d]) != NONE]


def diff(got, want):
    """Names of the struct members in which two word arrays differ."""
    return [n for n, a, b in FIELDS if not np.array_equal(got[a:b], want[a:b])]


def sizes(T):
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 7 * T + 3]


def masks(nbits, seed):
    """name -> bool[nbits]: from all ones to one bit in 4096 (the overflow bin), empty, one and two primes."""
    rng = np.random.default_rng(seed)
    out = {"ones": np.ones(nbits, bool), "zero": np.zeros(nbits, bool)}
    for name, p in (("half", 1 / 2), ("tenth", 1 / 10), ("1/64", 1 / 64), ("1/300", 1 / 300), ("1/4096", 1 / 4096)):
        out[name] = rng.random(nbits) < p
    out["one"] = np.zeros(nbits, bool)
    out["one"][nbits // 2] = True
    out["two"] = np.zeros(nbits, bool)
    out["two"][[0, nbits - 1]] = True
    return out


def g_starts():
    return [0, 1, 2**40 + 5]


def _pair(n, T, d, p, q, dense):
    """bool[n] with a gap of d places at p and at q > p + d and no other gap of d places: the rest is
    empty, or (dense) all ones, whose gaps of one place settle bin 1 around the planted ones."""
    assert 0 <= p and p + d < q and q + d < n and q - p - d != d
    if dense:
        bits = np.ones(n, bool)
        bits[p + 1:p + d] = False
        bits[q + 1:q + d] = False
    else:
        bits = np.zeros(n, bool)
        bits[[p, p + d, q, q + d]] = True
    return bits


def planted(T, d):
    """name -> bool[4T + 5]: the gap of d places twice, the lower occurrence the expected one. Five
    tiles, so a cap of 3 workgroups gives runs of two tiles: 2T and 4T are workgroup seams."""
    n = 4 * T + 5
    lay = {
        "tile0 low word / last word": (64 + 5, T - 4 - d),
        "tile1 low word / last word": (T + 3 * 64 + 7, 2 * T - 2 - d),
        "ends in the last word of tile 0 / starts in the first of tile 1": (T - 3 - d, T + 2),
        "ends in the last word of tile 1 / starts in the first of tile 2": (2 * T - 3 - d, 2 * T + 2),
        "straddles a word seam": (3 * 64 - 1 - min(d // 2, 150), 2 * T + 500),
        "straddles a tile seam": (T - 1 - d // 2, 3 * T + 100),
        "straddles a workgroup seam": (2 * T - 1 - d // 2, 3 * T + 100),
    }
    out = {}
    for name, (p, q) in lay.items():
        for dense in (False, True):
            out[name + (" dense" if dense else "")] = _pair(n, T, d, p, q, dense)
    return out


def long_gap(T):
    """bool[1003 T]: 1,000 empty tiles inside one gap, ordinary gaps on both sides."""
    bits = np.zeros(1003 * T, bool)
    bits[[5, 9, T // 2]] = True
    hi = T // 2 + 1001 * T + 17
    bits[[hi, hi + 4, hi + 11, hi + 15]] = True
    return bits


@functools.lru_cache(maxsize=None)
def real_bits(limit=REAL_LIMIT):
    """bool: element g is True iff 3 + 2g <= limit is prime (a numpy sieve)."""
    sv = np.ones(limit + 1, dtype=bool)
    sv[:2] = False
    for i in range(2, int(limit**0.5) + 1):
        if sv[i]:
            sv[i * i::i] = False
    out = sv[3::2].copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def real_brute(limit=REAL_LIMIT):
    w = brute(real_bits(limit), 0)
    w.setflags(write=False)
    return w
