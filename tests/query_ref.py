"""Reference answers of the rank and select queries (include/dse.h DSE_QUERY_*)
for the tests, independent of the library: numpy.searchsorted over the entry
values 3 + 2 (g_start + flatnonzero(bits)) of the test's own bits. A plain
module (like stats_ref.py, whose sizes, masks and range starts it shares),
imported by test_query_host.py and test_gpu_query.py.
"""
import numpy as np

from stats_ref import g_starts, masks, pack, pack_garbage  # noqa: F401  (the tests take them from here)

NONE = (1 << 64) - 1
RANK, SELECT, NEXT, PREV, TEST = range(5)
KINDS = (RANK, SELECT, NEXT, PREV, TEST)
VALUE_KINDS = (RANK, NEXT, PREV, TEST)
T = 256 * 64


def u64(xs):
    """Python integers (up to 2^64 - 1) -> uint64 array, exactly."""
    return np.array([int(x) for x in xs], dtype=object).astype(np.uint64) if len(xs) else np.zeros(0, np.uint64)


def values(bits, g_start):
    """The entry values of the bits, increasing, as uint64."""
    return np.uint64(3 + 2 * g_start) + np.uint64(2) * np.flatnonzero(bits).astype(np.uint64)  # below 2^62 + 3


def expect(vals, kind, q):
    """The answers of `kind` to the uint64 queries q over the increasing uint64 entry values."""
    q = np.asarray(q, dtype=np.uint64)
    n = len(vals)
    padded = np.concatenate([vals, np.array([NONE], dtype=np.uint64)])
    if kind == RANK:
        return np.searchsorted(vals, q, side="right").astype(np.uint64)
    if kind == SELECT:
        return padded[np.minimum(q, np.uint64(n)).astype(np.int64)]
    if kind == NEXT:
        return padded[np.searchsorted(vals, q, side="right")]
    if kind == PREV:
        i = np.searchsorted(vals, q, side="left")
        return np.where(i > 0, padded[np.maximum(i, 1) - 1], np.uint64(NONE))
    i = np.searchsorted(vals, q, side="left")
    return ((i < n) & (padded[i] == q)).astype(np.uint64)


def value_queries(bits, g_start, every_word_seam=True):
    """The value queries of a range: around 0, both ends of the range, the first and
    last entry, every word seam (bits 63 / 64) and tile seam, 2^63 and 2^64 - 1."""
    n = len(bits)
    v0, vl = 3 + 2 * g_start, 3 + 2 * (g_start + max(n, 1) - 1)
    qs = {0, 1, 2, 3, 2**63, NONE, v0 - 1, v0, v0 + 1}
    qs |= {vl + d for d in (-2, -1, 0, 1, 2)}
    pos = set()
    idx = np.flatnonzero(bits)
    if len(idx):
        pos |= {int(idx[0]), int(idx[-1])}
    step = 64 if every_word_seam else T
    for s in range(step, n + 1, step):
        pos |= {s - 1, s}
    if not every_word_seam:  # the word seams of the first, a middle and the last tile
        for t0 in {0, (n // T // 2) * T, (n - 1) // T * T}:
            for s in range(t0 + 64, min(t0 + T, n) + 1, 64):
                pos |= {s - 1, s}
    for p in pos:
        if 0 <= p < n:
            v = 3 + 2 * (g_start + p)
            qs |= {v - 1, v, v + 1}
    return u64(sorted(x for x in qs if 0 <= x <= NONE))


def rank_queries(bits):
    """0, 1, every tile's first rank and the one before it, total - 1, total, total + 5, 2^64 - 1."""
    n = len(bits)
    total = int(np.count_nonzero(bits))
    qs = {0, 1, total - 1, total, total + 5, NONE}
    if n:
        first = np.concatenate([[0], np.cumsum(np.add.reduceat(np.asarray(bits, dtype=np.int64), np.arange(0, n, T)))])
        for r in first:
            qs |= {int(r) - 1, int(r)}
    return u64(sorted(x for x in qs if 0 <= x <= NONE))


def queries(bits, g_start, kind, every_word_seam=True):
    return rank_queries(bits) if kind == SELECT else value_queries(bits, g_start, every_word_seam)


def tile_index(bits):
    """The rank index of the bits: uint64[tiles + 1], entries in the tiles before t."""
    n = len(bits)
    if not n:
        return np.zeros(1, np.uint64)
    per = np.add.reduceat(np.asarray(bits, dtype=np.int64), np.arange(0, n, T))
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
