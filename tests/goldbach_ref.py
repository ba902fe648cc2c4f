"""Reference minimal Goldbach partitions of a bit string for the tests, independent
of the library: numpy brute force on bool arrays, a loop over the small primes on
the VISIBLE bits, laid out as the uint64 words of a dse_goldbach (include/dse.h).
The small primes are this module's own (trial division), never the library's. A
plain module (like stats_ref.py), imported by test_goldbach_host.py and
test_gpu_goldbach.py, which share its fills, sizes and range starts.

Positions: the range's candidates are 0 .. nbits - 1, the candidates below it
-len(low) .. -1 (low[-1] is position -1). The even of position c has the partition
of rank i iff position c - H[i] is a visible set bit.
"""
import numpy as np

PRIMES, NONE = 2048, (1 << 64) - 1
WORDS = 8 + PRIMES
FIELDS = [(n, i, i + 1) for i, n in enumerate(("g_start", "nbits", "nprimes", "resolved", "unresolved",
                                               "first_unresolved", "max_rank", "max_c"))] + [("hist", 8, WORDS)]
T = 256 * 64


def _odd_primes(count):
    ps, q = [], 3
    while len(ps) < count:
        if all(q % p for p in ps if p * p <= q):
            ps.append(q)
        q += 2
    return ps


P = _odd_primes(PRIMES)                              # P[0] = 3 ... P[2047] = 17881
H = np.array([(p - 3) // 2 for p in P], dtype=np.int64)


def reach(nprimes):
    return int(H[(nprimes or PRIMES) - 1])


REACH = reach(0)  # 8939


def ranks(bits, low=()):
    """int64[len(bits)]: the minimal rank of every even of the range among all 2048 small
    primes, -1 where none holds; low = the visible bits below the range."""
    bits, low = np.asarray(bits, dtype=bool), np.asarray(low, dtype=bool)
    n, nl = len(bits), len(low)
    vis = np.concatenate([low, bits])
    rank = np.full(n, -1, dtype=np.int64)
    if n * PRIMES <= 1 << 21:   # all (even, prime) pairs at once
        idx = np.arange(n)[:, None] - H[None, :] + nl
        ok = (idx >= 0) & vis[np.clip(idx, 0, None)]
        has = ok.any(axis=1)
        rank[has] = ok.argmax(axis=1)[has]
        return rank
    if int(vis.sum()) * 16 <= len(vis):   # few visible entries: from each of them to the evens it resolves
        pos = np.flatnonzero(vis) - nl
        for i in range(PRIMES - 1, -1, -1):   # downwards, so the smallest rank is written last
            c = pos + int(H[i])
            rank[c[(c >= 0) & (c < n)]] = i
        return rank
    left = np.arange(n)         # many: from the evens still unresolved to the entry each needs
    for i in range(PRIMES):
        if not len(left):
            break
        idx = left - int(H[i]) + nl
        hit = np.zeros(len(left), dtype=bool)
        ok = idx >= 0
        hit[ok] = vis[idx[ok]]
        rank[left[hit]] = i
        left = left[~hit]
    return rank


def struct(rank, g_start, nprimes):
    """The dse_goldbach of a call with `nprimes` (0: all) from ranks(): uint64[WORDS]."""
    n = nprimes or PRIMES
    res = (rank >= 0) & (rank < n)
    w = np.zeros(WORDS, dtype=np.uint64)
    w[0], w[1], w[2] = g_start, len(rank), n
    w[3] = int(res.sum())
    w[4] = len(rank) - int(res.sum())
    un = np.flatnonzero(~res)
    w[5] = g_start + int(un[0]) if len(un) else NONE
    w[6] = w[7] = NONE
    if res.any():
        m = int(rank[res].max())
        w[6] = m
        w[7] = g_start + int(np.flatnonzero(res & (rank == m))[0])
        w[8:] = np.bincount(rank[res], minlength=PRIMES).astype(np.uint64)
    return w


def brute(bits, g_start, nprimes=0, low=()):
    return struct(ranks(bits, low), g_start, nprimes)


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
        m[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(len(bits) % 64)
    return m


def pack_below(low, shift):
    """The bits `low` as a `below` string that starts `shift` bits into its first word, every
    unused bit (the first `shift`, and those behind the last) set: they must be ignored. At
    least one word, also for an empty `low`."""
    s = np.concatenate([np.ones(shift, bool), np.asarray(low, dtype=bool)])
    pad = (-len(s)) % 64 if len(s) else 64
    return pack(np.concatenate([s, np.ones(pad, bool)]))


# -- the synthetic family -------------------------------------------------------------------
FILLS = ("half", "64th", "4096th", "ones", "zero", "one")
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 3 * T + 8939 + 3]
LOW_MAX = 3 * REACH
NPRIMES = [1, 2, 17, 2047, 2048, 0]
SHIFTS = [0, 1, 63]


def fill(name, nbits, seed):
    """-> (bits bool[nbits], low bool[LOW_MAX]): one string, the range behind its `low`."""
    rng = np.random.default_rng(seed)
    n = LOW_MAX + nbits
    if name == "half":
        s = rng.random(n) < 0.5
    elif name == "64th":
        s = rng.random(n) < 1 / 64
    elif name == "4096th":      # full-depth searches and unresolved evens
        s = rng.random(n) < 1 / 4096
    elif name == "ones":
        s = np.ones(n, bool)
    elif name == "zero":
        s = np.zeros(n, bool)
    else:                       # one bit, in the range
        s = np.zeros(n, bool)
        s[LOW_MAX + nbits // 3] = True
    return s[LOW_MAX:], s[:LOW_MAX]


def g_starts(nbits):
    return [0, 1, 63, T - 1, 2**40 + 5, 2**61 - 2 - nbits + 1]


def below_sizes(nprimes, g_start):
    """The below_bits of the family for a call's reach, capped at g_start, in increasing order."""
    r = reach(nprimes)
    return sorted({min(b, g_start) for b in (0, 1, 63, 64, r - 1, r, r + 1, 3 * r) if b >= 0})
