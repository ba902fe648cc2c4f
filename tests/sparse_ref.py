"""References for the resident-mask units that work from POSITIONS, not from a bool
array, so that ranges of 2^33 candidates and more can be checked: every result of
these units is a function of the sorted set-bit positions, g_start and nbits.

Two sets, both independent of the library:
  the functions named after the units (stats, gaps, consec, race, sums, goldbach,
      values, tuples, query, finish_text) take a sorted position array of at most a
      few 10^5 entries: numpy int64 on the positions (diff, isin, searchsorted,
      bincount), Python ints for values, sums and the reciprocals;
  ones_* are closed forms for an all-ones range [g_start, g_start + n), each
      derived from the period of its unit by counting over one period in Python ints.
Both produce the word layouts of stats_ref, gaps_ref, consec_ref, race_ref, sums_ref
and goldbach_ref, whose diff() reads them. tests/test_sparse_ref.py ties both sets to
those dense references.

Bit i of a range that starts at g_start is the candidate g = g_start + i of value
3 + 2 g. Positions are below 2^44 and g below 2^62, so int64 holds every g and value.
"""
import numpy as np

import consec_ref as CR
import gaps_ref as GR
import goldbach_ref as GB
import query_ref as QR
import race_ref as RR
import stats_ref as SR
import sums_ref as UR

NONE, M64 = (1 << 64) - 1, (1 << 64) - 1
DOUBLES, HACK, LAST = 1, 2, 4


def _pos(pos):
    p = np.asarray(pos).astype(np.int64)
    assert p.ndim == 1 and (len(p) < 2 or (np.diff(p) > 0).all()), "sorted, distinct positions"
    return p


def u64_words(ws):
    """Python ints below 2^64 -> uint64 array, exactly."""
    return np.array([int(x) for x in ws], dtype=object).astype(np.uint64)


def matches(pos, nbits, require, forbid=0):
    """The positions at which (require, forbid) matches inside the range (nothing visible above it)."""
    p = _pos(pos)
    ok = p + (require | forbid).bit_length() <= nbits
    for j in range(1, 32):
        if require >> j & 1:
            ok &= np.isin(p + j, p)
        if forbid >> j & 1:
            ok &= ~np.isin(p + j, p)
    return p[ok]


# -- the units, from positions ------------------------------------------------------------------
def stats(pos, g_start, nbits, patterns):
    p = _pos(pos)
    w = [0] * SR.WORDS
    w[0], w[1], w[2] = g_start, nbits, len(p)
    w[3] = g_start + int(p[0]) if len(p) else NONE
    w[4] = g_start + int(p[-1]) if len(p) else NONE
    k = min(64, nbits)
    w[5] = sum(1 << int(i) for i in p[p < k])
    w[6] = sum(1 << (63 - (nbits - 1 - int(i))) for i in p[p >= nbits - k])
    w[7] = len(patterns)
    for i, pat in enumerate(patterns):
        w[8 + i], w[16 + i] = pat, len(matches(p, nbits, pat))
    d = np.diff(p)
    w[25] = NONE
    if len(d):
        kmax = int(np.argmax(d))  # the first of the largest
        w[24], w[25] = 2 * int(d[kmax]), g_start + int(p[kmax])
        w[26] = int((d >= SR.BINS).sum())
        w[27:] = [int(c) for c in np.bincount(d[d < SR.BINS], minlength=SR.BINS)]
    return u64_words(w)


def gaps(pos, g_start, nbits):
    p = _pos(pos)
    w = [NONE] * GR.WORDS
    w[0], w[1], w[2] = g_start, nbits, len(p)
    if len(p):
        w[3], w[4] = g_start + int(p[0]), g_start + int(p[-1])
    w[5] = w[6] = 0
    d = np.diff(p)
    if len(d):
        vals, at = np.unique(d, return_index=True)  # the first index of every distinct difference
        for v, k in zip(vals, at):
            if v < GR.BINS:
                w[9 + int(v)] = g_start + int(p[k])
        big = np.flatnonzero(d >= GR.BINS)
        if len(big):
            w[8] = g_start + int(p[big[0]])
        kmax = int(np.argmax(d))
        w[6], w[7] = 2 * int(d[kmax]), g_start + int(p[kmax])
        w[5] = int((vals < GR.BINS).sum())
    return u64_words(w)


def consec(pos, g_start, nbits, q):
    g = g_start + _pos(pos)
    v = (3 + 2 * g) % q
    w = [0] * CR.WORDS
    w[0], w[1], w[2], w[3], w[4] = g_start, nbits, q, len(g), max(len(g) - 1, 0)
    w[5] = w[6] = NONE
    if len(g):
        w[5], w[6] = int(g[0]), int(g[-1])
    w[7:] = [int(c) for c in np.bincount(v[:-1] * 64 + v[1:], minlength=CR.BINS)]
    return u64_words(w)


def race(pos, g_start, nbits, q, a, b, d_start=0):
    g = g_start + _pos(pos)
    cls = (3 + 2 * g) % q
    w = [0] * RR.WORDS
    w[0], w[1], w[2], w[3], w[4] = g_start, nbits, q, a, b
    w[17:17 + q] = [int(c) for c in np.bincount(cls, minlength=q)]
    w[11] = w[12] = w[14] = w[16] = NONE
    if a != b:
        step = (cls == a) | (cls == b)
        sg = g[step]
        D = d_start + np.cumsum(np.where(cls[step] == a, 1, -1), dtype=np.int64)
        w[5] = w[6] = w[13] = w[15] = d_start & M64
        w[7] = len(D)
        if len(D):
            w[6] = int(D[-1]) & M64
            w[8], w[9], w[10] = int((D > 0).sum()), int((D < 0).sum()), int((D == 0).sum())
            if (D > 0).any():
                w[11] = int(sg[np.argmax(D > 0)])
            if (D < 0).any():
                w[12] = int(sg[np.argmax(D < 0)])
            w[13], w[14] = int(D.max()) & M64, int(sg[np.argmax(D)])
            w[15], w[16] = int(D.min()) & M64, int(sg[np.argmin(D)])
    return u64_words(w)


def _sums_words(vals, g_start, nbits, require, forbid, flags):
    mem = [j for j in range(32) if require >> j & 1]
    s1 = sum(vals) if flags & UR.POWER else 0
    s2 = sum(v * v for v in vals) if flags & UR.POWER else 0
    rc = sum((1 << 126) // (v + 2 * j) for v in vals for j in mem) if flags & UR.RECIP else 0
    return ([g_start, nbits, require, forbid, 0, flags, len(vals),
             (vals[0] - 3) // 2 if vals else NONE, (vals[-1] - 3) // 2 if vals else NONE]
            + UR.limbs(s1, 2) + UR.limbs(s2, 3) + UR.limbs(rc, 3))


def sums(pos, g_start, nbits, require=1, forbid=0, flags=UR.POWER | UR.RECIP):
    """The 17 words of a dse_sums with no `above`, as Python ints (sums_ref.diff reads them)."""
    vals = [3 + 2 * (g_start + i) for i in matches(pos, nbits, require, forbid).tolist()]
    return _sums_words(vals, g_start, nbits, require, forbid, flags)


def goldbach(pos, g_start, nbits, nprimes=0):
    """No `below`: the even of position c has the partition of rank i iff c - H[i] is a set position."""
    p = _pos(pos)
    n = nprimes or GB.PRIMES
    cs, rs = np.zeros(0, np.int64), np.zeros(0, np.int64)
    for i0 in range(0, n, 64):  # 64 ranks at a time, in increasing rank: the first occurrence is the minimal rank
        h = GB.H[i0:min(i0 + 64, n)]
        c = (p[None, :] + h[:, None]).ravel()
        r = np.repeat(np.arange(i0, i0 + len(h), dtype=np.int64), len(p))
        keep = (c < nbits) & ~np.isin(c, cs)
        u, at = np.unique(c[keep], return_index=True)
        cs, rs = np.concatenate([cs, u]), np.concatenate([rs, r[keep][at]])
    order = np.argsort(cs)
    cs, rs = cs[order], rs[order]
    w = [0] * GB.WORDS
    w[0], w[1], w[2], w[3], w[4] = g_start, nbits, n, len(cs), nbits - len(cs)
    hole = np.flatnonzero(cs != np.arange(len(cs)))  # the resolved positions stop being 0, 1, 2, ... here
    first = int(hole[0]) if len(hole) else len(cs)
    w[5] = g_start + first if first < nbits else NONE
    w[6] = w[7] = NONE
    if len(cs):
        m = int(rs.max())
        w[6], w[7] = m, g_start + int(cs[np.argmax(rs == m)])
        w[8:] = [int(x) for x in np.bincount(rs, minlength=GB.PRIMES)]
    return u64_words(w)


def values(pos, g_start):
    """The entries as uint64 values, increasing."""
    return (3 + 2 * (g_start + _pos(pos))).astype(np.uint64)


def tuples(pos, g_start, nbits, require, forbid=0):
    return values(matches(pos, nbits, require, forbid), g_start)


def query(pos, g_start, kind, q):
    """The answers of a DSE_QUERY_* kind to the uint64 queries q: searchsorted over the values."""
    return QR.expect(values(pos, g_start), kind, q)


def format_long(v):
    return str(v)


def format_double(v):
    """Double.toString of an integer below 2^53."""
    assert v < 1 << 53
    if v < 10**7:
        return f"{v}.0"
    s = str(v)
    return s[0] + "." + (s[1:].rstrip("0") or "0") + "E" + str(len(s) - 1)


def finish_text(pos, g_start, nbits, first_rank, flags):
    """-> (bytes, entries): the slice of a finish file whose first entry has rank first_rank. Ten
    entries a line: the entry of rank k follows ", " unless k = 0 (mod 10), and "\\n" follows it when
    k = 9 (mod 10); LAST closes a partial last line. HACK: 2 3 5 7 for the candidates 0 .. 3."""
    vals = (3 + 2 * (g_start + _pos(pos))).tolist()
    if flags & HACK:
        assert g_start == 0 and nbits >= 4
        vals = [2, 3, 5, 7] + [v for v in vals if v >= 3 + 2 * 4]
    fmt = format_double if flags & DOUBLES else format_long
    out = []
    for k, v in enumerate(vals, first_rank):
        out.append((", " if k % 10 else "") + fmt(v) + ("\n" if k % 10 == 9 else ""))
    if flags & LAST and (first_rank + len(vals)) % 10:
        out.append("\n")
    return "".join(out).encode(), len(vals)


# -- all ones: closed forms ----------------------------------------------------------------------
def ones_stats(g_start, n, patterns):
    """Every candidate an entry: a pattern of span s matches at the n - s + 1 positions that leave it
    room, every gap is one place, and the first of these equal gaps is the maximal one."""
    assert n >= 1
    w = [0] * SR.WORDS
    k = min(64, n)
    w[0], w[1], w[2], w[3], w[4] = g_start, n, n, g_start, g_start + n - 1
    w[5], w[6], w[7] = (1 << k) - 1, ((1 << k) - 1) << (64 - k), len(patterns)
    for i, pat in enumerate(patterns):
        w[8 + i], w[16 + i] = pat, max(0, n - pat.bit_length() + 1)
    w[25] = NONE
    if n >= 2:
        w[24], w[25], w[27 + 1] = 2, g_start, n - 1
    return u64_words(w)


def ones_gaps(g_start, n):
    assert n >= 1
    w = [NONE] * GR.WORDS
    w[0], w[1], w[2], w[3], w[4], w[5], w[6] = g_start, n, n, g_start, g_start + n - 1, 0, 0
    if n >= 2:  # one gap value, one place, first at the range's start
        w[5], w[6], w[7], w[9 + 1] = 1, 2, g_start, g_start
    return u64_words(w)


def _period(q):
    """The least T > 0 with 3 + 2 (g + T) = 3 + 2 g (mod q)."""
    return next(T for T in range(1, q + 1) if 2 * T % q == 0)


def _count_phase(n, T, ph):
    """How many i in [0, n) are ph (mod T), 0 <= ph < T."""
    return (n - ph + T - 1) // T if n > ph else 0


def ones_consec(g_start, n, q):
    """The pair of position i (i < n - 1) is (v, v + 2) mod q with v = 3 + 2 (g_start + i): one
    pair per phase of the period, as often as that phase occurs among the n - 1 positions."""
    assert n >= 1
    T = _period(q)
    w = [0] * CR.WORDS
    w[0], w[1], w[2], w[3], w[4], w[5], w[6] = g_start, n, q, n, n - 1, g_start, g_start + n - 1
    for ph in range(T):
        v = (3 + 2 * (g_start + ph)) % q
        w[7 + 64 * v + (v + 2) % q] += _count_phase(n - 1, T, ph)
    return u64_words(w)


def _count_positive(x, d, K):
    """How many k in [0, K) have x + k d > 0, and the least of them (None: none)."""
    if K <= 0:
        return 0, None
    if d == 0:
        return (K, 0) if x > 0 else (0, None)
    if d > 0:
        k0 = max(0, (-x) // d + 1)
        return (K - k0, k0) if k0 < K else (0, None)
    c = min(K, max(0, -((-x) // -d)))  # k < x / -d
    return (c, 0) if c else (0, None)


def ones_race(g_start, n, q, a, b, d_start=0):
    """Counts: every phase of the period, as often as it occurs. The race: the steps of one period
    (offset, +-1) and the drift d of a whole period; step j of period k leaves D = d_start + s_j + k d,
    an arithmetic progression in k for every j, counted and searched in Python ints."""
    assert n >= 1
    T = _period(q)
    w = [0] * RR.WORDS
    w[0], w[1], w[2], w[3], w[4] = g_start, n, q, a, b
    w[11] = w[12] = w[14] = w[16] = NONE
    steps = []  # (offset in the period, +1 | -1), by offset
    for ph in range(T):
        c = (3 + 2 * (g_start + ph)) % q
        w[17 + c] += _count_phase(n, T, ph)
        if a != b and c in (a, b):
            steps.append((ph, 1 if c == a else -1))
    if a == b:
        return u64_words(w)
    drift = sum(s for _, s in steps)
    w[5] = w[6] = w[13] = w[15] = d_start & M64
    pos_first, neg_first, best_max, best_min, acc = [], [], [], [], 0
    for ph, s in steps:
        acc += s
        K = _count_phase(n, T, ph)  # the periods in which this step happens
        if K == 0:
            continue
        x = d_start + acc
        w[7] += K
        c, k = _count_positive(x, drift, K)
        w[8] += c
        if c:
            pos_first.append(g_start + k * T + ph)
        c, k = _count_positive(-x, -drift, K)
        w[9] += c
        if c:
            neg_first.append(g_start + k * T + ph)
        if drift == 0:
            w[10] += K if x == 0 else 0
        elif x % drift == 0 and 0 <= -x // drift < K:
            w[10] += 1
        kmax, kmin = (K - 1, 0) if drift > 0 else (0, K - 1) if drift < 0 else (0, 0)
        best_max.append((-(x + kmax * drift), g_start + kmax * T + ph))  # largest, then lowest g
        best_min.append((x + kmin * drift, g_start + kmin * T + ph))
    if w[7]:
        last_k = (n - 1) // T  # D after the last step: whole periods, then the steps of the last, partial one
        w[6] = (d_start + drift * last_k + sum(s for ph, s in steps if ph <= (n - 1) % T)) & M64
        if pos_first:
            w[11] = min(pos_first)
        if neg_first:
            w[12] = min(neg_first)
        (d, g) = min(best_max)
        w[13], w[14] = -d & M64, g
        (d, g) = min(best_min)
        w[15], w[16] = d & M64, g
    return u64_words(w)


def ones_sums(g_start, n, flags=UR.POWER):
    """Pattern 1, POWER only: the values a + 2 i, i < n, a = 3 + 2 g_start; sum of i = n (n - 1) / 2,
    sum of i^2 = (n - 1) n (2 n - 1) / 6."""
    assert n >= 1 and not flags & UR.RECIP
    a = 3 + 2 * g_start
    s1 = n * a + n * (n - 1)
    s2 = n * a * a + 2 * a * n * (n - 1) + 4 * ((n - 1) * n * (2 * n - 1) // 6)
    if not flags & UR.POWER:
        s1 = s2 = 0
    return [g_start, n, 1, 0, 0, flags, n, g_start, g_start + n - 1] + UR.limbs(s1, 2) + UR.limbs(s2, 3) + [0, 0, 0]


def ones_goldbach(g_start, n, nprimes=0):
    """The smallest prime is 3, whose distance H[0] is 0: the even of position c is 3 + (3 + 2 c), so
    every even of an all-ones range has rank 0 through its own position, at both ends of the range
    too (nothing below the range is ever needed), and the first of them holds the maximal rank."""
    assert n >= 1 and GB.H[0] == 0
    w = [0] * GB.WORDS
    w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8] = g_start, n, nprimes or GB.PRIMES, n, 0, NONE, 0, g_start, n
    return u64_words(w)


def ones_query(g_start, n, kind, qs):
    """The values are a, a + 2, ..., a + 2 (n - 1), a = 3 + 2 g_start: rank and select by division."""
    a, out = 3 + 2 * g_start, []
    last = a + 2 * (n - 1)
    for x in (int(v) for v in qs):
        rank = 0 if x < a else min(n, (x - a) // 2 + 1)  # the values <= x
        if kind == QR.RANK:
            out.append(rank)
        elif kind == QR.SELECT:
            out.append(a + 2 * x if x < n else NONE)
        elif kind == QR.NEXT:
            out.append(a + 2 * rank if rank < n else NONE)
        elif kind == QR.PREV:
            below = 0 if x <= a else min(n, (x - 1 - a) // 2 + 1)  # the values < x
            out.append(a + 2 * (below - 1) if below else NONE)
        else:
            out.append(int(a <= x <= last and (x - a) % 2 == 0))
    return u64_words(out)


def ones_values(g_start, first, count):
    """The values of the ranks [first, first + count) of an all-ones range."""
    return (3 + 2 * (g_start + np.arange(first, first + count, dtype=np.int64))).astype(np.uint64)
