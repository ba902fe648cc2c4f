"""Residue-class counts and prime races of a mask on the CPU: dse_debug_race_host
runs the race kernels' own __host__ __device__ per-word bodies
(csrc/dse_race_word.h) in a plain loop, and dse_race_merge joins adjacent results
by host arithmetic.

Expected values are numpy on bool arrays (tests/race_ref.py): np.bincount(v % q),
np.cumsum of +-1 over the entries of the two classes, argmax / argmin for first
attainment; never the library. Every word of the struct is compared, exactly.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import race_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_race_dev_async", "dse_race_range", "dse_race_resident", "dse_race_merge", "dse_debug_race_host")
T = R.T
A5 = 0xA5A5A5A5A5A5A5A5
EINVAL, ERANGE = -1, -6
NB_4M = 2_000_001  # the candidates of 3 .. 4,000,003


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
    assert "race_grid" in hdr and "residue classes and races" in hdr
    assert (_dse.RACE_WORDS, _dse.RACE_MAX_MODULUS, _dse.RACE_NONE) == (R.WORDS, R.MAX_MODULUS, R.NONE) == (81, 64, 2**64 - 1)


# -- 1. synthetic fills: the per-word bodies against numpy ------------------------------------------
def test_family_is_what_it_says():
    assert R.SIZES == [1, 63, 64, 65, 16383, 16384, 16385, 2 * 16384 + 5, 7 * 16384 + 3]
    assert set(R.G_STARTS) == {0, 1, 2**40 + 5} | set(range(7)) | set(range(6))
    assert R.QS == [3, 4, 5, 7, 8, 12, 30, 63, 64] and R.D_STARTS == [0, 3, -3, -70, 2**40, -2**40]
    assert R.pairs(4) == [(1, 3), (2, 1), (3, 2)] and R.pairs(3) == [(1, 2), (0, 1), (2, 0)]
    assert R.pairs(12) == [(1, 11), (2, 1), (3, 1), (11, 2)] and R.pairs(63) == [(1, 62), (3, 1), (7, 1), (62, 2)]
    # the alternating fill from d_start 0: D is 1 or 0 (or -1 and 0) after every step, and most words see a 0
    bits = R.fill("alternating", 7 * T + 3, 0, 5, 4, 1, 3)
    w = R.brute(bits, 5, 4, 1, 3)
    assert int(w[7]) > 7 * T // 3 and abs(int(w[10]) - int(w[7]) / 2) <= 1 and {R.signed(w[13]), R.signed(w[15])} <= {-1, 0, 1}
    # the reference against plain Python
    bits = R.fill("half", 300, 9)
    for q, a, b, d0 in ((4, 1, 3, 0), (12, 3, 1, -3), (63, 62, 2, 3)):
        D, seen, cnt = d0, [], [0] * q
        for i in np.flatnonzero(bits):
            v = 3 + 2 * (77 + int(i))
            cnt[v % q] += 1
            if v % q in (a, b):
                D += 1 if v % q == a else -1
                seen.append((D, 77 + int(i)))
        w = R.brute(bits, 77, q, a, b, d0)
        assert [int(x) for x in w[17:17 + q]] == cnt and int(w[7]) == len(seen) and R.signed(w[6]) == D
        ds = [d for d, _ in seen]
        assert (int(w[8]), int(w[9]), int(w[10])) == (sum(d > 0 for d in ds), sum(d < 0 for d in ds), ds.count(0))
        assert (R.signed(w[13]), int(w[14])) == (max(ds), seen[ds.index(max(ds))][1])
        assert (R.signed(w[15]), int(w[16])) == (min(ds), seen[ds.index(min(ds))][1])
        assert int(w[11]) == next((g for d, g in seen if d > 0), R.NONE)
        assert int(w[12]) == next((g for d, g in seen if d < 0), R.NONE)


def test_thinned_family_covers_every_value():
    for nbits in R.SIZES:
        seen = [c for k in range(len(R.FILLS)) for c in R.thinned(nbits, k)]
        assert {c[0] for c in seen} == set(R.G_STARTS), nbits
        assert {c[1] for c in seen} == set(R.QS), nbits
        assert {c[4] for c in seen} == set(R.D_STARTS), nbits
        assert any(not R.has_candidates(q, a) for _, q, a, b, _ in seen), nbits      # an empty class
        assert any(not R.has_candidates(q, b) for _, q, a, b, _ in seen), nbits
        assert any(a in R.prime_factors(q) and R.has_candidates(q, a) for _, q, a, b, _ in seen), nbits
        assert any((q, a, b) == (4, 1, 3) for _, q, a, b, _ in seen), nbits


@pytest.mark.parametrize("nbits", R.SIZES)
def test_host_matches_numpy(S, nbits):
    for k, name in enumerate(R.FILLS):
        fixed = None if name == "alternating" else R.fill(name, nbits, 9000 + nbits)
        for g, q, a, b, d in R.thinned(nbits, k):
            bits = R.fill(name, nbits, 0, g, q, a, b) if fixed is None else fixed
            got = S.race_host(R.pack_garbage(bits), g, nbits, q, a, b, d)
            assert not R.diff(got.words, R.brute(bits, g, q, a, b, d)), (name, g, q, a, b, d)


def test_fast_path_and_exact_walk(S):
    """d_start = +-2^40 decides the sign of every word; d_start = 0 on the alternating fill has D
    cross 0 inside the words."""
    n = 2 * T + 5
    for d in (2**40, -2**40):
        bits = R.fill("half", n, 3)
        got = S.race_host(R.pack(bits), 6, n, 4, 1, 3, d)
        assert not R.diff(got.words, R.brute(bits, 6, 4, 1, 3, d))
        assert (got.a_ahead, got.b_ahead) == ((got.steps, 0) if d > 0 else (0, got.steps)) and got.steps > n // 3
        assert (got.first_a_ahead is None) == (d < 0) and (got.first_b_ahead is None) == (d > 0)
    for q, a, b in ((4, 1, 3), (7, 3, 5), (64, 63, 1)):
        bits = R.fill("alternating", n, 0, 6, q, a, b)
        got = S.race_host(R.pack(bits), 6, n, q, a, b, 0)
        assert not R.diff(got.words, R.brute(bits, 6, q, a, b, 0))
        assert got.ties == got.steps // 2 and got.steps > 0


def test_counts_only_and_accessors(S):
    bits = R.fill("half", 1000, 5)
    got = S.race_host(R.pack_garbage(bits), 11, 1000, 12, 5, 5)
    assert not R.diff(got.words, R.brute(bits, 11, 12, 5, 5))
    assert (got.steps, got.a_ahead, got.b_ahead, got.ties, got.max_d, got.min_d, got.d_end, got.d_start) == (0,) * 8
    assert (got.first_a_ahead, got.first_b_ahead, got.max_at, got.min_at) == (None,) * 4
    assert got.counts.shape == (12,) and int(got.counts.sum()) == int(bits.sum()) and int(got.counts[::2].sum()) == 0
    # 3 5 7 11 13 17 19 23 mod 4: 3 1 3 3 1 1 3 3 -> D -1 0 -1 -2 -1 0 -1 -2
    small = np.zeros(11, bool)
    small[[0, 1, 2, 4, 5, 7, 8, 10]] = True
    r = S.race_host(R.pack(small), 0, 11, 4, 1, 3)
    assert (r.q, r.a, r.b, r.steps, r.a_ahead, r.b_ahead, r.ties, r.d_end) == (4, 1, 3, 8, 0, 6, 2, -2)
    assert (r.first_a_ahead, r.first_b_ahead, r.max_d, r.max_at, r.min_d, r.min_at) == (None, 3, 0, 5, -2, 11)
    assert [int(c) for c in r.counts] == [0, 3, 0, 5]
    # 3 is in class 0 mod 3, and with d_start = 1 the lead is a's from the first step
    r = S.race_host(R.pack(small), 0, 11, 3, 0, 1, 1)
    assert [int(c) for c in r.counts] == [1, 3, 4] and (r.d_start, r.d_end, r.first_a_ahead, r.max_d, r.max_at) == (1, -1, 3, 2, 3)
    e = S.race_host(np.zeros(0, np.uint64), 9, 0, 5, 1, 2, -7)
    assert (e.g_start, e.nbits, e.steps, e.d_start, e.d_end, e.max_d, e.min_d, e.max_at, e.min_at) == (9, 0, 0, -7, -7, -7, -7, None, None)
    assert not R.diff(e.words, R.brute(np.zeros(0, bool), 9, 5, 1, 2, -7))


# -- 2. real primes ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(oracle):
    from primes_ref import mask_bits
    m, _ = oracle.fast_sieve_range(0, NB_4M)
    return m, mask_bits(m, NB_4M)


def test_real_primes_to_4e6(S, real):
    m, bits = real
    want = R.brute(bits, 0, 4, 1, 3)
    # the figures of the issue, recomputed by the reference
    assert int(want[7]) == 283_145
    assert (int(want[8]), int(want[10]), int(want[9])) == (239, 111, 282_795)
    assert 3 + 2 * int(want[11]) == 26_861
    assert (R.signed(want[13]), 3 + 2 * int(want[14])) == (8, 623_681)
    assert (R.signed(want[15]), 3 + 2 * int(want[16])) == (-260, 3_039_859)
    assert R.signed(want[6]) == -141
    got = S.race_host(m, 0, NB_4M, 4, 1, 3)
    assert not R.diff(got.words, want)
    assert (got.first_a_ahead, got.max_d, got.max_at, got.min_d, got.min_at, got.d_end) == (26_861, 8, 623_681, -260, 3_039_859, -141)
    # on [3, 616,841) pi(x; 4, 1) leads exactly once: at the single prime 26,861
    nb = (616_841 - 3) // 2
    lead = S.race_host(m, 0, nb, 4, 1, 3)
    assert not R.diff(lead.words, R.brute(bits[:nb], 0, 4, 1, 3))
    assert (lead.a_ahead, lead.first_a_ahead, lead.max_d, lead.max_at) == (1, 26_861, 1, 26_861)
    assert S.race_host(m, 0, nb + 1, 4, 1, 3).a_ahead == 2      # and next at 616,841
    r3 = S.race_host(m, 0, NB_4M, 3, 1, 2)
    assert not R.diff(r3.words, R.brute(bits, 0, 3, 1, 2))
    assert (r3.a_ahead, r3.ties, r3.d_end, r3.first_a_ahead) == (0, 9, -248, None)
    r5 = S.race_host(m, 0, NB_4M, 5, 1, 2)
    assert not R.diff(r5.words, R.brute(bits, 0, 5, 1, 2))
    assert r5.first_a_ahead == 6_781
    for q, a, b in ((8, 3, 1), (12, 3, 1), (30, 7, 2), (63, 62, 1), (64, 1, 63)):
        assert not R.diff(S.race_host(m, 0, NB_4M, q, a, b).words, R.brute(bits, 0, q, a, b)), (q, a, b)


# -- 3. merge equals the whole ----------------------------------------------------------------------
def test_merge_equals_whole(S, real):
    m, real_bits = real
    n = 3 * T + 77
    ranges = [("half", 5, 4, 1, 3, 0), ("alternating", 2**40 + 5, 7, 3, 5, 0), ("16th", 1, 12, 3, 1, -3),
              ("4096th", 6, 63, 62, 2, 2**40), ("zero", 3, 5, 1, 2, 3), ("ones", 0, 64, 63, 2, -70),
              ("half", 2, 30, 7, 7, 0)]
    cuts = (0, 1, 63, 64, 65, 100, T - 1, T, T + 1, 2 * T, 2 * T + 33, n - 1, n)   # inside a word, at a tile seam, an empty side
    for name, g, q, a, b, d in ranges:
        bits = R.fill(name, n, 21, g, q, a, b)
        whole = S.race_host(R.pack_garbage(bits), g, n, q, a, b, d)
        assert not R.diff(whole.words, R.brute(bits, g, q, a, b, d))
        for cut in cuts:
            left = S.race_host(R.pack_garbage(bits[:cut]), g, cut, q, a, b, d)
            right = S.race_host(R.pack_garbage(bits[cut:]), g + cut, n - cut, q, a, b, left.d_end)
            got = left.merge(right)
            assert not R.diff(got.words, whole.words), (name, q, a, b, cut)
            assert got == whole
    # real primes: the record at 26,861 on either side of the cut
    whole = S.race_host(m, 0, NB_4M, 4, 1, 3)
    for cut in (13_000, 13_429, 13_430, 311_839, 1_519_928, 1_519_929):
        left = S.race_host(R.pack(real_bits[:cut]), 0, cut, 4, 1, 3)
        right = S.race_host(R.pack(real_bits[cut:]), cut, NB_4M - cut, 4, 1, 3, left.d_end)
        assert left.merge(right) == whole, cut


def test_merge_ties_keep_the_first(S):
    # D: 1 0 1 0 | 1 0 1 0: the maximum 1 and the minimum 0 are attained on both sides
    bits = R.fill("alternating", 64, 0, 0, 4, 3, 1)
    a, b = S.race_host(R.pack(bits[:32]), 0, 32, 4, 3, 1), S.race_host(R.pack(bits[32:]), 32, 32, 4, 3, 1)
    assert (a.d_end, a.max_d, b.max_d, a.min_d, b.min_d) == (0, 1, 1, 0, 0) and b.max_at > a.max_at
    mm = a.merge(b)
    assert (mm.max_d, mm.max_at, mm.min_d, mm.min_at) == (1, a.max_at, 0, a.min_at)
    assert (mm.first_a_ahead, mm.first_b_ahead) == (a.first_a_ahead, None)
    # a side without steps takes no part: its max_d = min_d = d_start would otherwise win
    none = S.race_host(np.zeros(1, np.uint64), 0, 40, 4, 1, 3, 5)
    fall = np.zeros(40, bool)
    fall[[0, 2, 4]] = True                        # 83 87 91: three b-steps
    down = S.race_host(R.pack(fall), 40, 40, 4, 1, 3, 5)
    mm = none.merge(down)
    assert (none.max_d, none.max_at, down.max_d, mm.max_d, mm.max_at, mm.min_d, mm.min_at) == (5, None, 4, 4, 83, 2, 91)
    up = S.race_host(np.zeros(1, np.uint64), 80, 40, 4, 1, 3, 2)
    mm2 = mm.merge(up)
    assert (mm2.max_d, mm2.max_at, mm2.min_d, mm2.min_at, mm2.d_end, mm2.nbits) == (4, 83, 2, 91, 2, 120)
    both = none.merge(S.race_host(np.zeros(1, np.uint64), 40, 40, 4, 1, 3, 5))
    assert (both.max_d, both.min_d, both.max_at, both.min_at, both.steps) == (5, 5, None, None, 0)


def test_merge_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    bits = np.random.default_rng(4).random(300) < 0.5
    a = S.race_host(R.pack(bits[:100]), 0, 100, 4, 1, 3)
    b = S.race_host(R.pack(bits[100:]), 100, 200, 4, 1, 3, a.d_end)
    assert not R.diff(a.merge(b).words, R.brute(bits, 0, 4, 1, 3))
    tail = R.pack(bits[100:])
    cases = [(EINVAL, a, S.race_host(tail, 101, 200, 4, 1, 3, a.d_end)),          # a gap between the ranges
             (EINVAL, a, S.race_host(tail, 99, 200, 4, 1, 3, a.d_end)),           # an overlap
             (EINVAL, b, a),                                                      # the wrong order
             (EINVAL, a, S.race_host(tail, 100, 200, 8, 1, 3, a.d_end)),          # another q
             (EINVAL, a, S.race_host(tail, 100, 200, 4, 2, 3, a.d_end)),          # another a
             (EINVAL, a, S.race_host(tail, 100, 200, 4, 1, 2, a.d_end)),          # another b
             (EINVAL, a, S.race_host(tail, 100, 200, 4, 1, 3, a.d_end + 1))]      # a d_start that does not chain
    for code, x, y in cases:
        out = np.full(R.WORDS, A5, dtype=np.uint64)
        assert L.dse_race_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == code
        assert (out == A5).all()
        with pytest.raises(_dse.DseError) as e:
            x.merge(y)
        assert e.value.code == code
    assert L.dse_race_merge(None, _dse.u64p(b.words), _dse.u64p(a.words.copy())) == EINVAL
    assert L.dse_race_merge(_dse.u64p(a.words), _dse.u64p(b.words), None) == EINVAL
    # a union that ends above 2^62
    x, y = S.Race(a.words.copy()), S.Race(b.words.copy())
    x.words[0], x.words[1] = 2**62 - 100, 100
    y.words[0], y.words[1] = 2**62, 200
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    assert L.dse_race_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == ERANGE
    assert (out == A5).all()
    # out may alias either side
    aw, bw = a.words.copy(), b.words.copy()
    assert L.dse_race_merge(_dse.u64p(aw), _dse.u64p(b.words), _dse.u64p(aw)) == 0
    assert L.dse_race_merge(_dse.u64p(a.words), _dse.u64p(bw), _dse.u64p(bw)) == 0
    assert np.array_equal(aw, bw) and not R.diff(aw, R.brute(bits, 0, 4, 1, 3))


# -- 4. argument errors -----------------------------------------------------------------------------
def test_host_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(4, dtype=np.uint64)
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    mp, op = _dse.u64p(m), _dse.u64p(out)
    odd = ctypes.cast(ctypes.c_void_p(m.ctypes.data + 4), ctypes.POINTER(ctypes.c_uint64))
    for code, args in [(EINVAL, (mp, 100, 64, 4, 1, 3, 0, None)),            # null out
                       (EINVAL, (None, 100, 64, 4, 1, 3, 0, op)),            # null mask with nbits > 0
                       (EINVAL, (odd, 100, 64, 4, 1, 3, 0, op)),             # misaligned mask
                       (EINVAL, (mp, 100, 64, 2, 1, 0, 0, op)),              # q outside 3..64
                       (EINVAL, (mp, 100, 64, 65, 1, 3, 0, op)),
                       (EINVAL, (mp, 100, 64, 0, 0, 0, 0, op)),
                       (EINVAL, (mp, 100, 64, 4, 4, 3, 0, op)),              # a or b >= q
                       (EINVAL, (mp, 100, 64, 4, 1, 4, 0, op)),
                       (EINVAL, (mp, 100, 64, 4, 1, 2**32 - 1, 0, op)),
                       (EINVAL, (mp, 100, 64, 4, 1, 1, 1, op)),              # a == b with d_start != 0
                       (ERANGE, (mp, 100, 64, 4, 1, 3, 2**45 + 1, op)),      # |d_start| above 2^45
                       (ERANGE, (mp, 100, 64, 4, 1, 3, -2**45 - 1, op)),
                       (ERANGE, (mp, 2**62 - 10, 64, 4, 1, 3, 0, op)),       # g_start + nbits > 2^62
                       (ERANGE, (mp, 2**63, 64, 4, 1, 3, 0, op)),
                       (ERANGE, (mp, 0, 2**44 + 1, 4, 1, 3, 0, op))]:        # more than 2^44 candidates
        assert L.dse_debug_race_host(*args) == code, args
        assert (out == A5).all(), args
    assert L.dse_last_status() == ERANGE and L.dse_last_error()
    # the bounds themselves are fine, and nbits = 0 needs no mask
    assert L.dse_debug_race_host(mp, 100, 64, 64, 63, 0, 2**45, op) == 0
    assert L.dse_debug_race_host(mp, 100, 64, 3, 2, 0, -2**45, op) == 0
    assert L.dse_debug_race_host(None, 100, 0, 4, 3, 3, 0, op) == 0
    assert not R.diff(out, R.brute(np.zeros(0, bool), 100, 4, 3, 3))
