"""Reference for the constellations as numbers (include/dse.h "constellations as
numbers"), independent of the library: numpy ANDs of shifted slices of the
test's own bool array. A plain module (like primes_ref.py), imported by the
test modules that need it.
"""
import numpy as np

T = 256 * 64  # candidates per tile (csrc/dse_mask.h), checked against the library by test_gpu_primes

TWINS = (0b11, 0)
QUADS = (0b11011, 0)
SEXT = (1 | 1 << 2 | 1 << 3 | 1 << 5 | 1 << 6 | 1 << 8, 0)


def exact_gap_ref(d):
    return (1 | 1 << d, sum(1 << j for j in range(1, d)))


# the patterns every fill is run with: entries; twins; the sextuplet; span 32 with two members; an entry
# with 31 non-entries above it; consecutive entries 3 and 31 places apart
PATTERNS = [(1, 0), TWINS, SEXT, (1 | 1 << 31, 0), (1, 0xFFFFFFFE), exact_gap_ref(3), exact_gap_ref(31)]


def span(require, forbid):
    return (require | forbid).bit_length()


def positions(bits, above, require, forbid):
    """Match positions i < len(bits): i + span <= len(bits) + len(above), every required
    candidate an entry and every forbidden one not, over bits ++ above."""
    nbits = len(bits)
    vis = np.concatenate([np.asarray(bits, bool), np.asarray(above, bool)])
    n = min(nbits, len(vis) - span(require, forbid) + 1)
    if n <= 0:
        return np.empty(0, dtype=np.int64)
    ok = np.ones(n, bool)
    for j in range(32):
        if (require >> j) & 1:
            ok &= vis[j:j + n]
        if (forbid >> j) & 1:
            ok &= ~vis[j:j + n]
    return np.flatnonzero(ok)


def values(bits, above, require, forbid, g_start):
    return np.uint64(3) + np.uint64(2) * (np.uint64(g_start) + positions(bits, above, require, forbid).astype(np.uint64))


def pack(bits):
    """bool array -> uint64 mask words (zero past the end)."""
    by = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    out = np.zeros((len(bits) + 63) // 64 * 8, dtype=np.uint8)
    out[:len(by)] = by
    return out.view(np.uint64)


def pack_above(above, shift, rng):
    """The `above` bits from bit `shift` on of a string of whole words, random bits around them."""
    n = len(above)
    words = max(1, (shift + n + 63) // 64)
    s = rng.random(64 * words) < 0.5
    s[shift:shift + n] = above
    return pack(s)


def fills(nbits, seed):
    rng = np.random.default_rng(seed)
    out = {"ones": np.ones(nbits, bool), "zero": np.zeros(nbits, bool), "half": rng.random(nbits) < 0.5,
           "twentieth": rng.random(nbits) < 1 / 20}
    for name, pos in (("first", 0), ("last", nbits - 1), ("seam-", T - 1), ("seam+", T)):
        if 0 <= pos < nbits:
            out[name] = np.zeros(nbits, bool)
            out[name][pos] = True
    return out


def plant(bits, above, pos, require, forbid):
    """Make position pos of bits ++ above a match: required candidates set, forbidden ones cleared."""
    for j in range(32):
        arr, i = (bits, pos + j) if pos + j < len(bits) else (above, pos + j - len(bits))
        if (require >> j) & 1:
            arr[i] = True
        elif (forbid >> j) & 1:
            arr[i] = False
