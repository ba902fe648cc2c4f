"""Statistics of a mask on the CPU: dse_debug_stats_host runs the statistics
kernels' own __host__ __device__ per-word bodies (csrc/dse_stats_word.h) in a
plain loop, and dse_stats_merge joins adjacent results by host arithmetic.

Expected values are numpy brute force on bool arrays (tests/stats_ref.py):
shifted ANDs for the patterns, diff of flatnonzero for the gaps; never the
library. Every member of the struct is compared, exactly.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_stats_dev_async", "dse_stats_range", "dse_stats_resident", "dse_stats_merge", "dse_debug_stats_host")
T = 256 * 64  # "stats_tile_bits" (a context reports the library's: tests/test_gpu_stats.py checks it is this)
EINVAL, ERANGE = -1, -6


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


def test_header_declares_and_library_exports_the_entry_points(S):
    from mail_sieve_e import _dse
    hdr = open(os.path.join(ROOT, "include", "dse.h")).read()
    declared = set(re.findall(r"\b(dse_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = _dse.lib()
    for s in NEW:
        assert s in declared, f"include/dse.h does not declare {s}"
        assert hasattr(L, s), f"libdse.so does not export {s}"
        assert s in _dse.SIGNATURES, f"ctypes binding misses {s}"
    assert "stats_grid" in hdr and "stats_tile_bits" in hdr
    assert (_dse.STATS_WORDS, _dse.STATS_GAP_BINS, _dse.STATS_NONE) == (R.WORDS, R.BINS, R.NONE)


def test_constants(S):
    assert S.pattern(0, 2, 6) == 0b1011 and S.pattern(0) == 1 and S.pattern(0, 62) == 1 | 1 << 31
    assert S.CONSTELLATIONS == R.CONSTELLATIONS
    assert S.CONSTELLATIONS == (S.TWINS, *S.TRIPLETS, S.QUADRUPLETS, *S.QUINTUPLETS, S.SEXTUPLETS)
    for bad in ((2,), (0, 3), (0, 64)):
        with pytest.raises(ValueError):
            S.pattern(*bad)


def host(S, bits, g, pats, garbage=True):
    return S.stats_host(R.pack_garbage(bits) if garbage else R.pack(bits), g, len(bits), pats)


# -- 1. the per-word bodies against brute force ------------------------------------------
@pytest.mark.parametrize("nbits", R.sizes(T))
def test_host_matches_brute_force(S, nbits):
    for name, bits in R.masks(nbits, T, 9000 + nbits).items():
        for g in R.g_starts(nbits, T):
            for pats in R.PATTERN_LISTS:
                got = host(S, bits, g, pats)
                assert not R.diff(got.words, R.brute(bits, g, pats)), (name, g, pats)
    far = R.masks(2 * T + 37, T, 1)["far"]
    st = host(S, far, 0, (1,))
    assert (st.gap_overflow, st.max_gap, st.max_gap_prime, st.primes) == (1, 2 * 2053, 9, 2)


def test_stats_accessors(S):
    bits = np.zeros(100, bool)
    bits[[0, 1, 2, 4, 10]] = True  # 3 5 7 11 23 at g_start 0
    st = host(S, bits, 0, (S.TWINS, 1))
    assert (st.primes, st.first, st.last) == (5, 3, 23)
    assert st.patterns == [S.TWINS, 1] and st.matches == [2, 5]
    assert st.gaps.dtype == np.uint64 and st.gaps.shape == (1024,)
    assert [int(v) for v in st.gaps[:7]] == [0, 2, 1, 0, 0, 0, 1] and st.gap_overflow == 0
    assert (st.max_gap, st.max_gap_prime) == (12, 11)
    empty = host(S, np.zeros(7, bool), 5, ())
    assert (empty.primes, empty.first, empty.last, empty.max_gap, empty.max_gap_prime) == (0, None, None, 0, None)
    one = host(S, np.ones(1, bool), 5, (1,))
    assert (one.primes, one.first, one.last, one.max_gap, one.max_gap_prime) == (1, 13, 13, 0, None)
    assert host(S, np.zeros(0, bool), 5, (1,)).nbits == 0


# -- 2. a tie of the maximal gap ------------------------------------------------------------
@pytest.mark.parametrize("gap", [3, 16, 17, 40, 70, 1500])
def test_max_gap_tie_keeps_the_lower(S, gap):
    for start in (0, 50, 63, T - gap - 1, T - 1):
        bits = np.zeros(3 * T, bool)
        # two gaps of `gap` places with shorter ones between and around them
        pos = [start, start + gap, start + gap + 1, start + 2 * gap + 1, start + 2 * gap + 3]
        bits[pos] = True
        st = host(S, bits, 7, (1,))
        assert not R.diff(st.words, R.brute(bits, 7, (1,))), (gap, start)
        assert st.max_gap == 2 * gap and st.max_gap_g == 7 + start, (gap, start)


# -- 3. merge equals union ---------------------------------------------------------------------
def fold(S, bits, g, pats, cuts):
    """The statistics of the pieces of bits cut at `cuts`, merged as a left and as a right fold."""
    edges = [0] + list(cuts) + [len(bits)]
    parts = [host(S, bits[a:b], g + a, pats) for a, b in zip(edges, edges[1:])]
    left = parts[0]
    for p in parts[1:]:
        left = left.merge(p)
    right = parts[-1]
    for p in reversed(parts[:-1]):
        right = p.merge(right)
    return left, right


def random_cuts(rng, n):
    """1 to 5 sorted cuts of [0, n]: random places, repeats (empty pieces), and pieces of 1, 5, 30, 31, 63."""
    k = int(rng.integers(1, 6))
    cuts = [int(c) for c in rng.integers(0, n + 1, size=k)]
    for i in range(1, k):
        if rng.random() < 0.5:
            cuts[i] = min(n, cuts[i - 1] + int(rng.choice([0, 1, 5, 30, 31, 63])))
    return sorted(cuts)


def test_merge_equals_union(S):
    rng = np.random.default_rng(0x57A7)
    splits = 0
    for nbits in R.sizes(T):
        for name, bits in R.masks(nbits, T, 9000 + nbits).items():
            pats = R.PATTERN_LISTS[splits % 2]
            g = R.g_starts(nbits, T)[splits % 3]
            whole = host(S, bits, g, pats)
            for _ in range(3):
                cuts = random_cuts(rng, nbits)
                for got in fold(S, bits, g, pats, cuts):
                    assert not R.diff(got.words, whole.words), (nbits, name, cuts)
                splits += 1
    assert splits >= 200


def test_merge_with_members_in_three_pieces(S):
    rng = np.random.default_rng(3)
    n = 400
    for at in (60, 100, 127, 200):
        bits = rng.random(n) < 0.3
        bits[at:at + 40] = False
        bits[[at + j for j in range(9) if 0b101101101 >> j & 1]] = True  # a sextuplet at `at`
        bits[[at + 9, at + 40]] = True                                   # and a 32-span pair behind it
        pats = (0b101101101, 0b1101101, 0b11011, 0b1011, 0b11, 1 | 1 << 31, 1)
        whole = host(S, bits, 11, pats)
        assert not R.diff(whole.words, R.brute(bits, 11, pats))
        assert whole.matches[0] >= 1 and whole.matches[5] >= 1
        for cuts in ([at + 1, at + 4], [at + 3, at + 8], [at + 1, at + 2, at + 5, at + 6, at + 8],
                     [at + 10, at + 40], [at + 10, at + 15, at + 20], [at, at, at + 5], [at + 5, at + 5, n],
                     [0, at + 3, at + 3 + 63], [at + 2, at + 2 + 30], [at + 2, at + 2 + 31], [at + 8, at + 9]):
            for got in fold(S, bits, 11, pats, cuts):
                assert not R.diff(got.words, whole.words), (at, cuts)
            # the seam matters: the pieces' own counts miss the sextuplet that is cut
            if at < cuts[0] <= at + 8:
                edges = [0] + cuts + [n]
                own = sum(host(S, bits[a:b], 11 + a, pats).matches[0] for a, b in zip(edges, edges[1:]))
                assert own < whole.matches[0], (at, cuts)


# -- 4. merge refusals -----------------------------------------------------------------------------
def test_merge_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    bits = np.random.default_rng(4).random(300) < 0.3
    a, b = host(S, bits[:100], 0, (3, 1)), host(S, bits[100:], 100, (3, 1))
    assert not R.diff(a.merge(b).words, R.brute(bits, 0, (3, 1)))
    cases = [(EINVAL, a, host(S, bits[100:], 101, (3, 1))),      # a hole between them
             (EINVAL, a, host(S, bits[100:], 99, (3, 1))),       # an overlap
             (EINVAL, b, a),                                     # the wrong order
             (EINVAL, a, host(S, bits[100:], 100, (3,))),        # fewer patterns
             (EINVAL, a, host(S, bits[100:], 100, (1, 3))),      # the same patterns in another order
             (EINVAL, a, host(S, bits[100:], 100, (3, 5)))]
    for code, x, y in cases:
        out = np.full(R.WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        assert L.dse_stats_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == code
        assert (out == 0xA5A5A5A5A5A5A5A5).all()
        with pytest.raises(_dse.DseError) as e:
            x.merge(y)
        assert e.value.code == code
    assert L.dse_stats_merge(None, _dse.u64p(b.words), _dse.u64p(a.words.copy())) == EINVAL
    # a union that ends above 2^62
    x, y = S.Stats(a.words.copy()), S.Stats(b.words.copy())
    x.words[0], x.words[1] = 2**62 - 100, 100
    y.words[0], y.words[1] = 2**62, 200
    out = np.full(R.WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert L.dse_stats_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == ERANGE
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    # out may alias either side
    aw, bw = a.words.copy(), b.words.copy()
    assert L.dse_stats_merge(_dse.u64p(aw), _dse.u64p(b.words), _dse.u64p(aw)) == 0
    assert L.dse_stats_merge(_dse.u64p(a.words), _dse.u64p(bw), _dse.u64p(bw)) == 0
    assert np.array_equal(aw, bw) and not R.diff(aw, R.brute(bits, 0, (3, 1)))


def test_host_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(2, dtype=np.uint64)
    out = np.full(R.WORDS, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    pats = (ctypes.c_uint32 * 9)(*([3] * 9))
    bad0, bad2 = (ctypes.c_uint32 * 2)(3, 0), (ctypes.c_uint32 * 2)(3, 2)
    mp, op = _dse.u64p(m), _dse.u64p(out)
    for code, args in [(EINVAL, (mp, 0, 64, pats, 1, None)), (EINVAL, (None, 0, 64, pats, 1, op)),
                       (EINVAL, (mp, 0, 64, pats, 9, op)), (EINVAL, (mp, 0, 64, None, 1, op)),
                       (EINVAL, (mp, 0, 64, bad0, 2, op)), (EINVAL, (mp, 0, 64, bad2, 2, op)),
                       (ERANGE, (mp, 2**62 - 10, 64, pats, 1, op)), (ERANGE, (mp, 0, 2**44 + 1, pats, 1, op))]:
        assert L.dse_debug_stats_host(*args) == code, args
        assert (out == 0xA5A5A5A5A5A5A5A5).all()


# -- 5. real primes ---------------------------------------------------------------------------------
def test_real_primes(S, oracle):
    from primes_ref import mask_bits
    nb = 2**20 + 37
    m, c = oracle.fast_sieve_range(0, nb)
    bits = mask_bits(m, nb)
    st = S.stats_host(m, 0, nb, S.CONSTELLATIONS)
    want = R.brute(bits, 0, S.CONSTELLATIONS)
    assert not R.diff(st.words, want)
    assert st.primes == c and st.matches[0] == int((bits[:-1] & bits[1:]).sum())
    # (3,5) and (5,7) are both twins; (3,5,7) is no triplet
    first = S.stats_host(m, 0, 3, (S.TWINS,) + S.TRIPLETS)
    assert first.matches == [2, 0, 0] and first.primes == 3
    assert S.stats_host(m, 0, 6, (S.TWINS,) + S.TRIPLETS).matches == [3, 1, 1]  # 3 .. 13: (11,13) too; (5,7,11), (7,11,13)
