"""Where the prime gaps are, on the CPU: dse_debug_gaps_host runs the gaps kernels'
own __host__ __device__ per-word bodies (csrc/dse_gaps_word.h) in a plain loop over
tiles and words, with the main kernel's settled bins refreshed per tile;
dse_gaps_merge joins adjacent results and dse_gaps_records reads the maximal gaps
off one, both by host arithmetic.

Expected values are numpy on bool arrays (tests/gaps_ref.py: flatnonzero, diff,
the first index of every distinct difference), tied below to a plain Python loop,
and published first occurrences and maximal gaps; never the library. Every word
of the struct is compared, exactly.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gaps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_gaps_dev_async", "dse_gaps_range", "dse_gaps_resident", "dse_gaps_merge", "dse_gaps_records",
       "dse_debug_gaps_host")
T = 256 * 64  # "gaps_tile_bits" (a context reports the library's: tests/test_gpu_gaps.py checks it is this)
EINVAL, ERANGE = -1, -6
A5 = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


def host(S, bits, g, garbage=True):
    return S.gaps_host(R.pack_garbage(bits) if garbage else R.pack(bits), g, len(bits))


def loop_ref(bits, g_start):
    """brute()'s result by a plain Python loop over the candidates."""
    w = [R.NONE] * R.WORDS
    w[0], w[1], w[2], w[5], w[6] = g_start, len(bits), 0, 0, 0
    prev = None
    for i, b in enumerate(bits):
        if not b:
            continue
        w[2] += 1
        if prev is None:
            w[3] = g_start + i
        else:
            d = i - prev
            if d < R.BINS:
                if w[9 + d] == R.NONE:
                    w[9 + d] = g_start + prev
                    w[5] += 1
            elif w[8] == R.NONE:
                w[8] = g_start + prev
            if 2 * d > w[6]:
                w[6], w[7] = 2 * d, g_start + prev
        prev = i
        w[4] = g_start + i
    return np.array(w, dtype=np.uint64)


def test_header_declares_and_library_exports_the_entry_points(S):
    from mail_sieve_e import _dse
    hdr = open(os.path.join(ROOT, "include", "dse.h")).read()
    declared = set(re.findall(r"\b(dse_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = _dse.lib()
    for s in NEW:
        assert s in declared, f"include/dse.h does not declare {s}"
        assert hasattr(L, s), f"libdse.so does not export {s}"
        assert s in _dse.SIGNATURES, f"ctypes binding misses {s}"
    assert "gaps_grid" in hdr and "gaps_tile_bits" in hdr
    assert (_dse.GAPS_WORDS, _dse.GAPS_BINS, _dse.GAPS_NONE) == (R.WORDS, R.BINS, R.NONE)
    m = re.search(r"typedef struct dse_gaps \{(.*?)\} dse_gaps;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert set(re.findall(r"^\s*(\w+)\s", body, flags=re.M)) == {"uint64_t"}
    members = [x.strip() for decl in re.findall(r"uint64_t([^;]*);", body) for x in decl.split(",")]
    words = sum(R.BINS if "[DSE_GAPS_BINS]" in x else 1 for x in members)
    assert 8 * words == 8 * 1033 == 8 * _dse.GAPS_WORDS  # sizeof(dse_gaps): uint64 members only, no padding


def test_reference_is_the_plain_loop():
    rng = np.random.default_rng(0x6A95)
    for n, p in ((0, 0.5), (1, 1.0), (2, 1.0), (300, 0.5), (5000, 0.02), (9000, 1 / 2000), (4000, 0.0)):
        bits = rng.random(n) < p
        for g in R.g_starts():
            assert np.array_equal(R.brute(bits, g), loop_ref(bits, g)), (n, p, g)
    far = np.zeros(3000, bool)
    far[[3, 10, 10 + 1024, 2900, 2999]] = True
    assert np.array_equal(R.brute(far, 7), loop_ref(far, 7))
    assert int(R.brute(far, 7)[8]) == 7 + 10 and int(R.brute(far, 7)[6]) == 2 * 1866


# -- 1. the per-word bodies against the reference ----------------------------------------------
@pytest.mark.parametrize("nbits", R.sizes(T))
def test_host_matches_reference(S, nbits):
    for name, bits in R.masks(nbits, 7000 + nbits).items():
        for g in R.g_starts():
            got = host(S, bits, g)
            assert not R.diff(got.words, R.brute(bits, g)), (name, g)
    assert not R.diff(host(S, np.zeros(0, bool), 5).words, R.brute(np.zeros(0, bool), 5))


def test_accessors(S):
    bits = np.zeros(100, bool)
    bits[[0, 1, 2, 4, 10, 12]] = True  # 3 5 7 11 23 27 at g_start 0
    g = host(S, bits, 0)
    assert (g.primes, g.first_g, g.last_g, g.found, g.max_gap, g.max_gap_prime, g.overflow_g) == (6, 0, 12, 3, 12, 11,
                                                                                                 None)
    assert g.first.dtype == np.uint64 and g.first.shape == (1024,)
    assert g.first_primes() == [(2, 3), (4, 7), (12, 11)] and g.records() == [(2, 3), (4, 7), (12, 11)]
    assert int(g.first[0]) == R.NONE and "max_gap=12 at 11" in repr(g)
    assert g == S.Gaps(g.words.copy()) and g != host(S, bits, 1)
    empty = host(S, np.zeros(7, bool), 5)
    assert (empty.primes, empty.first_g, empty.last_g, empty.found, empty.max_gap, empty.max_gap_prime) == (
        0, None, None, 0, 0, None)
    assert empty.first_primes() == [] and empty.records() == []
    with pytest.raises(ValueError):
        S.Gaps(np.zeros(5, dtype=np.uint64))


# -- 2. planted gaps: the lower of two occurrences -------------------------------------------------
@pytest.mark.parametrize("d", R.PLANTED_D)
def test_planted_twice_keeps_the_lower(S, d):
    for name, bits in R.planted(T, d).items():
        idx = np.flatnonzero(bits)
        at = idx[:-1][np.diff(idx) == d]
        assert len(at) == 2, (d, name)
        want = R.brute(bits, 11)
        got = host(S, bits, 11, garbage=False)
        assert not R.diff(got.words, want), (d, name)
        lower = 11 + int(at[0])
        assert (int(got.first[d]) if d < R.BINS else got.overflow_g) == lower, (d, name)


def test_a_thousand_empty_tiles_inside_one_gap(S):
    bits = R.long_gap(T)
    want = R.brute(bits, 3)
    got = host(S, bits, 3, garbage=False)
    assert not R.diff(got.words, want)
    assert got.max_gap == 2 * (1001 * T + 17) and got.max_gap_g == 3 + T // 2 and got.overflow_g == 3 + 9


# -- 3. real primes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(S):
    bits = R.real_bits()
    return bits, S.gaps_host(R.pack(bits), 0, len(bits))


def test_real_primes_table_and_records(S, real):
    bits, got = real
    want = R.real_brute()
    assert not R.diff(got.words, want)
    fp = dict(got.first_primes())
    for gap, p in R.FIRST.items():
        assert fp[gap] == p, gap
    assert got.records() == R.RECORDS_21M == R.records(want)
    assert (got.max_gap, got.max_gap_prime, got.primes) == (210, 20831323, 1329942)


def test_real_primes_against_the_neighbouring_units(S, real):
    bits, got = real
    m = R.pack(bits)
    st = S.stats_host(m, 0, len(bits), ())
    assert (got.primes, got.first_g, got.last_g, got.max_gap, got.max_gap_g) == (st.primes, st.first_g, st.last_g,
                                                                                 st.max_gap, st.max_gap_g)
    assert np.array_equal(got.first != np.uint64(R.NONE), st.gaps > 0)
    assert (got.overflow_g is not None) == (st.gap_overflow > 0)
    nb = 2**20  # the tuples' first values over a smaller range: every gap up to 62 occurs below 2^21
    small = S.gaps_host(m, 0, nb)
    for d in range(1, 32):
        vals, total = S.tuples_host(m, 0, nb, *S.exact_gap(d), count=1)
        assert total > 0 and 3 + 2 * int(small.first[d]) == int(vals[0]), d


def test_synthetic_against_stats(S):
    for nbits in (65, T + 1, 7 * T + 3):
        for name, bits in R.masks(nbits, 7000 + nbits).items():
            m = R.pack_garbage(bits)
            got, st = S.gaps_host(m, 9, nbits), S.stats_host(m, 9, nbits, ())
            assert (got.primes, got.first_g, got.last_g, got.max_gap, got.max_gap_g) == (
                st.primes, st.first_g, st.last_g, st.max_gap, st.max_gap_g), (nbits, name)
            assert np.array_equal(got.first != np.uint64(R.NONE), st.gaps > 0), (nbits, name)
            assert (got.overflow_g is not None) == (st.gap_overflow > 0), (nbits, name)


# -- 4. merge equals union ------------------------------------------------------------------------------
def fold(S, bits, g, cuts):
    """The tables of the pieces of bits cut at `cuts` (the reference's, not the library's), merged by
    the library as a left and as a right fold."""
    edges = [0] + list(cuts) + [len(bits)]
    parts = [S.Gaps(R.brute(bits[a:b], g + a)) for a, b in zip(edges, edges[1:])]
    left = parts[0]
    for p in parts[1:]:
        left = left.merge(p)
    right = parts[-1]
    for p in reversed(parts[:-1]):
        right = p.merge(right)
    return left, right


def random_cuts(rng, n):
    """1 to 5 sorted cuts of [0, n]: random places, repeats (empty pieces) and pieces of one candidate."""
    k = int(rng.integers(1, 6))
    cuts = [int(c) for c in rng.integers(0, n + 1, size=k)]
    for i in range(1, k):
        if rng.random() < 0.5:
            cuts[i] = min(n, cuts[i - 1] + int(rng.choice([0, 1, 2, 40])))
    return sorted(cuts)


def test_merge_equals_union(S):
    rng = np.random.default_rng(0x6A95)
    cases = [("real", R.real_bits()[:200_000]), ("real tail", R.real_bits()[10_000_000:10_060_000])]
    for nbits in (65, T + 1, 2 * T + 5):
        cases += [(f"{name} {nbits}", bits) for name, bits in R.masks(nbits, 7000 + nbits).items()]
    splits = 0
    for k, (name, bits) in enumerate(cases):
        g = R.g_starts()[k % 3]
        whole = R.brute(bits, g)
        for _ in range(11):
            cuts = random_cuts(rng, len(bits))
            for got in fold(S, bits, g, cuts):
                assert not R.diff(got.words, whole), (name, cuts)
            splits += 1
    assert splits >= 300


def test_merge_with_a_seam_inside_a_first_occurrence(S):
    bits = R.real_bits()[:200_000]
    whole = R.brute(bits, 0)
    # 113 -> 127 (7 places), 1327 -> 1361 (17), 31397 -> 31469 (36): the first gaps of their sizes
    for p, q in ((113, 127), (1327, 1361), (31397, 31469)):
        gp, gq = (p - 3) // 2, (q - 3) // 2
        assert int(whole[9 + gq - gp]) == gp
        for cut in (gp + 1, (gp + gq) // 2, gq):
            for cuts in ([cut], [cut, cut], [gp + 1, gq], [0, cut, len(bits)]):
                for got in fold(S, bits, 0, cuts):
                    assert not R.diff(got.words, whole), (p, cuts)
            a, b = R.brute(bits[:cut], 0), R.brute(bits[cut:], cut)
            assert int(a[9 + gq - gp]) != gp and int(b[9 + gq - gp]) != gp  # neither side has it: the seam does
    far = np.zeros(5000, bool)
    far[[3, 10, 10 + 1500, 4000, 4001]] = True  # an overflow gap cut by the seam
    for cuts in ([11], [700, 1511], [1510], [4, 11, 1511, 4001]):
        for got in fold(S, far, 2**40, cuts):
            assert not R.diff(got.words, R.brute(far, 2**40)), cuts


def test_merge_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    bits = np.random.default_rng(4).random(300) < 0.3
    a, b = host(S, bits[:100], 0), host(S, bits[100:], 100)
    assert not R.diff(a.merge(b).words, R.brute(bits, 0))
    for code, x, y in [(EINVAL, a, host(S, bits[100:], 101)),  # a hole between them
                       (EINVAL, a, host(S, bits[100:], 99)),   # an overlap
                       (EINVAL, b, a)]:                        # the wrong order
        out = np.full(R.WORDS, A5, dtype=np.uint64)
        assert L.dse_gaps_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == code
        assert (out == A5).all()
        with pytest.raises(_dse.DseError) as e:
            x.merge(y)
        assert e.value.code == code
    assert L.dse_gaps_merge(None, _dse.u64p(b.words), _dse.u64p(a.words.copy())) == EINVAL
    assert L.dse_gaps_merge(_dse.u64p(a.words), None, _dse.u64p(a.words.copy())) == EINVAL
    assert L.dse_gaps_merge(_dse.u64p(a.words), _dse.u64p(b.words), None) == EINVAL
    # a union that ends above 2^62
    x, y = S.Gaps(a.words.copy()), S.Gaps(b.words.copy())
    x.words[0], x.words[1] = 2**62 - 100, 100
    y.words[0], y.words[1] = 2**62, 200
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    assert L.dse_gaps_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == ERANGE
    assert (out == A5).all()
    # out may alias either side
    aw, bw = a.words.copy(), b.words.copy()
    assert L.dse_gaps_merge(_dse.u64p(aw), _dse.u64p(b.words), _dse.u64p(aw)) == 0
    assert L.dse_gaps_merge(_dse.u64p(a.words), _dse.u64p(bw), _dse.u64p(bw)) == 0
    assert np.array_equal(aw, bw) and not R.diff(aw, R.brute(bits, 0))


def test_host_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(2, dtype=np.uint64)
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    mp, op = _dse.u64p(m), _dse.u64p(out)
    for code, args in [(EINVAL, (mp, 0, 64, None)), (EINVAL, (None, 0, 64, op)), (ERANGE, (mp, 2**62 - 10, 64, op)),
                       (ERANGE, (mp, 2**63, 64, op)), (ERANGE, (mp, 0, 2**44 + 1, op))]:
        assert L.dse_debug_gaps_host(*args) == code, args
        assert (out == A5).all()
    assert L.dse_debug_gaps_host(None, 5, 0, op) == 0 and not R.diff(out, R.brute(np.zeros(0, bool), 5))


# -- 5. records ---------------------------------------------------------------------------------------------
def lib_records(S, words, cap):
    from mail_sieve_e import _dse
    n = ctypes.c_uint32(0xA5A5)
    d = (ctypes.c_uint32 * (cap + 1))(*([0xA5A5] * (cap + 1)))
    rc = _dse.lib().dse_gaps_records(_dse.u64p(words), d if cap else None, cap, ctypes.byref(n))
    assert rc == 0 and d[cap] == 0xA5A5
    return n.value, list(d[:min(cap, n.value)])


def test_records_caps_and_overflow(S):
    from mail_sieve_e import _dse
    want = [g // 2 for g, _ in R.RECORDS_21M]
    w = np.array(R.real_brute())
    assert lib_records(S, w, 0) == (len(want), [])
    assert lib_records(S, w, 5) == (len(want), want[:5])
    assert lib_records(S, w, len(want)) == (len(want), want)
    assert lib_records(S, w, 1024) == (len(want), want)
    # an overflow gap below a binned one hides it and every shorter later one; above it, it hides nothing
    bits = np.zeros(40_000, bool)
    bits[[0, 2, 7, 7 + 2000, 7 + 2000 + 300, 7 + 2000 + 303, 30_000, 30_000 + 400]] = True
    g = S.Gaps(R.brute(bits, 0))
    assert g.overflow_g == 7 and g.records() == [(4, 3), (10, 7)] == R.records(g.words)
    bits = np.zeros(40_000, bool)
    bits[[0, 2, 7, 307, 310, 20_000, 20_400, 20_401, 20_401 + 3000]] = True
    g = S.Gaps(R.brute(bits, 0))
    assert g.overflow_g == 310 and g.records() == [(4, 3), (10, 7), (600, 17)] == R.records(g.words)
    L = _dse.lib()
    n = ctypes.c_uint32(0)
    d = (ctypes.c_uint32 * 4)()
    assert L.dse_gaps_records(None, d, 4, ctypes.byref(n)) == EINVAL
    assert L.dse_gaps_records(_dse.u64p(w), d, 4, None) == EINVAL
    assert L.dse_gaps_records(_dse.u64p(w), None, 4, ctypes.byref(n)) == EINVAL
