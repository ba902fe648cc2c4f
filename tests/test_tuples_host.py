"""Constellations as numbers on the host: dse_debug_tuples_host runs the tuples
kernels' own per-word body (csrc/dse_tuples_word.h) in a plain loop, and the
Python helpers around the pattern.

Expected values come from tests/tuples_ref.py (numpy ANDs of shifted slices of
the test's own bits); the cross-checks count the same bits with
dse_debug_stats_host. Every comparison is exact. No GPU.
"""
import ctypes

import numpy as np
import pytest

import tuples_ref as R
from tuples_ref import T

EINVAL, ERANGE = -1, -6
A5 = 0xA5A5A5A5A5A5A5A5
NBITS = [1, 31, 32, 33, 63, 64, 65, 95, 96, T - 1, T, T + 1, 2 * T + 37]
ABOVE = [(b, s) for b in (0, 1, 17, 31) for s in (0, 5, 40, 63)]


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


def garbage_mask(bits):
    mask = R.pack(bits)
    if len(bits) % 64:  # garbage past nbits in the last word is ignored
        mask[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(len(bits) % 64)
    return mask


def test_python_helpers(S):
    assert S.exact_gap(1) == (0b11, 0) and S.exact_gap(3) == (0b1001, 0b0110)
    for d in range(1, 32):
        assert S.exact_gap(d) == R.exact_gap_ref(d)
    for d in (0, 32):
        with pytest.raises(ValueError):
            S.exact_gap(d)
    m = S.tuple_members(np.array([5, 11, 101], dtype=np.uint64), S.QUADRUPLETS)
    assert m.dtype == np.uint64 and m.tolist() == [[5, 7, 11, 13], [11, 13, 17, 19], [101, 103, 107, 109]]
    assert S.tuple_members(np.empty(0, dtype=np.uint64), S.TWINS).shape == (0, 2)
    assert S.tuple_members([2**62 - 3], 1 | 1 << 1).tolist() == [[2**62 - 3, 2**62 - 1]]


@pytest.mark.parametrize("nbits", NBITS)
def test_fills_patterns_and_above(S, nbits):
    rng = np.random.default_rng(9100 + nbits)
    for name, bits in R.fills(nbits, 9000 + nbits).items():
        mask = garbage_mask(bits)
        for g in (0, 2**31 - 1 - min(nbits, T) // 2):
            for ab, sh in ABOVE:
                above = rng.random(ab) < 0.5
                if name in ("zero", "last") and ab:
                    above[:] = name == "last"  # forbid patterns see entries right behind the range
                aw = R.pack_above(above, sh, rng)
                for req, fb in R.PATTERNS:
                    want = R.values(bits, above, req, fb, g)
                    got, total = S.tuples_host(mask, g, nbits, req, fb, aw, sh, ab)
                    assert total == len(want), (name, g, ab, sh, hex(req), hex(fb))
                    assert np.array_equal(got, want), (name, g, ab, sh, hex(req), hex(fb))
                    if (req, fb) == (1, 0):  # the primes' values
                        assert np.array_equal(got, 3 + 2 * (g + np.flatnonzero(bits)))


def test_null_above_when_empty(S):
    bits = np.random.default_rng(3).random(200) < 0.5
    got, total = S.tuples_host(R.pack(bits), 7, 200, *R.TWINS)
    assert np.array_equal(got, R.values(bits, [], *R.TWINS, 7)) and total == len(got) > 0


def test_top_of_range(S):
    nbits, ab = 100, 31
    g = 2**62 - nbits - ab  # the last visible candidate is 2^62 - 1, of value 2^63 + 1: no wrap
    bits, above = np.ones(nbits, bool), np.ones(ab, bool)
    for req, fb in ((1, 0), R.TWINS, (1 | 1 << 31, 0)):
        got, _ = S.tuples_host(R.pack(bits), g, nbits, req, fb, R.pack(above), 0, ab)
        assert [int(v) for v in got] == [3 + 2 * (g + int(i)) for i in R.positions(bits, above, req, fb)]


def test_short_range_matches_only_through_above(S):
    req, fb = R.SEXT
    for nbits in (1, 2, 8):
        bits = np.zeros(nbits, bool)
        above = np.zeros(31, bool)
        for j in range(9):
            if (req >> j) & 1:
                (bits if j < nbits else above)[j if j < nbits else j - nbits] = True
        assert R.positions(bits, above, req, fb).tolist() == [0]
        got, total = S.tuples_host(R.pack(bits), 50, nbits, req, fb, R.pack(above), 0, 31)
        assert total == 1 and got.tolist() == [103]
        got, total = S.tuples_host(R.pack(bits), 50, nbits, req, fb, R.pack(above), 0, 8 - nbits)
        assert total == 0  # the last member is one place past the visible candidates


def test_second_last_word_reaches_above(S):
    # nbits % 64 < 31: a match that starts in the second-last word ends in `above`
    nbits = 3 * 64 + 5
    req, fb = 1 | 1 << 31, 0
    bits = np.zeros(nbits, bool)
    bits[2 * 64 + 60] = True  # its other member is position 3 * 64 + 27 = nbits + 22
    above = np.zeros(31, bool)
    above[22] = True
    assert R.positions(bits, above, req, fb).tolist() == [188]
    for sh in (0, 40, 63):
        got, total = S.tuples_host(R.pack(bits), 0, nbits, req, fb, R.pack_above(above, sh, np.random.default_rng(sh)),
                                   sh, 31)
        assert total == 1 and got.tolist() == [3 + 2 * 188]
    # an entry of `above` is forbidden the same way
    got, total = S.tuples_host(R.pack(bits), 0, nbits, 1, 0xFFFFFFFE, R.pack(above), 0, 31)
    assert total == 0
    above[22] = False
    got, total = S.tuples_host(R.pack(bits), 0, nbits, 1, 0xFFFFFFFE, R.pack(above), 0, 31)
    assert got.tolist() == [3 + 2 * 188]


def test_rank_windows(S):
    nbits, g = 3 * T - 100, 10**9
    bits = np.random.default_rng(21).random(nbits) < 0.6
    above = np.random.default_rng(22).random(31) < 0.6
    mask, aw = R.pack(bits), R.pack(above)
    for req, fb in (R.TWINS, R.exact_gap_ref(3)):
        pos = R.positions(bits, above, req, fb)
        full = R.values(bits, above, req, fb, g)
        total = len(full)
        w = 300  # a word with at least three matches: windows that start and end inside it
        while ((pos >= 64 * w) & (pos < 64 * w + 64)).sum() < 3:
            w += 1
        mid = int((pos < 64 * w).sum()) + 1
        for first in (0, 1, mid, int((pos < T).sum()), total - 1, total, total + 5):
            exact = max(total - first, 0)
            for cap in (0, 1, 2, exact, exact - 1, 2**40):
                if cap < 0:
                    continue
                out = np.full(min(cap, exact) + 4, A5, dtype=np.uint64)
                tot = np.zeros(2, dtype=np.uint64)
                from mail_sieve_e import _dse
                _dse.check(_dse.lib().dse_debug_tuples_host(_dse.u64p(mask), g, nbits, req, fb, _dse.u64p(aw), 0, 31,
                                                            first, _dse.u64p(out), cap, _dse.u64p(tot)), "host")
                n = min(cap, exact)
                assert tot.tolist() == [total, n], (first, cap)
                assert np.array_equal(out[:n], full[first:first + n]) and (out[n:] == A5).all(), (first, cap)


@pytest.mark.parametrize("nbits", [65, T + 1, 2 * T + 37])
def test_cross_check_with_stats(S, nbits):
    rng = np.random.default_rng(500 + nbits)
    for p in (0.5, 0.2, 0.05):
        bits = rng.random(nbits) < p
        mask = garbage_mask(bits)
        pats = [1, R.TWINS[0], R.QUADS[0], R.SEXT[0], 1 | 1 << 31, 0b111, 0b1011, 0b1101]
        st = S.stats_host(mask, 5, nbits, pats)
        for k, pat in enumerate(pats):
            assert S.tuples_host(mask, 5, nbits, pat)[1] == st.matches[k], hex(pat)
        for d in range(1, 32):
            assert S.tuples_host(mask, 5, nbits, *S.exact_gap(d))[1] == int(st.gaps[d]), d


def test_splitting(S):
    nbits, g = 2 * T + 37, 12345
    rng = np.random.default_rng(77)
    seams = sorted({1, 2, 5, 8, 9, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1,
                    2 * T + 36, nbits - 1})
    for p in (0.7, 0.15):
        bits = rng.random(nbits) < p
        for req, fb in R.PATTERNS:
            whole, _ = S.tuples_host(R.pack(bits), g, nbits, req, fb)
            assert np.array_equal(whole, R.values(bits, [], req, fb, g))
            assert any(s < R.span(req, fb) for s in seams) or R.span(req, fb) == 1
            for s in seams:
                a, b = bits[:s], bits[s:]
                head = b[:31]  # b's head is a's `above`, as a pointer into the whole mask
                la, _ = S.tuples_host(R.pack(a), g, s, req, fb, R.pack(bits)[s // 64:], s % 64, len(head))
                lb, _ = S.tuples_host(R.pack(b), g + s, nbits - s, req, fb)
                assert np.array_equal(np.concatenate([la, lb]), whole), (s, hex(req), hex(fb))


def test_errors():
    from mail_sieve_e import _dse
    L = _dse.lib()
    mask = np.zeros(4, dtype=np.uint64)
    above = np.zeros(2, dtype=np.uint64)
    out = np.full(64, A5, dtype=np.uint64)
    tot = np.zeros(2, dtype=np.uint64)
    m, a, o, t = _dse.u64p(mask), _dse.u64p(above), _dse.u64p(out), _dse.u64p(tot)
    a_mis = ctypes.cast(ctypes.c_void_p(above.ctypes.data + 4), ctypes.POINTER(ctypes.c_uint64))
    cases = [
        (EINVAL, (m, 0, 64, 3, 0, a, 0, 0, 0, o, 8, None)),            # null totals
        (EINVAL, (None, 0, 64, 3, 0, a, 0, 0, 0, o, 8, t)),            # null mask with nbits > 0
        (EINVAL, (m, 0, 64, 3, 0, a, 0, 0, 0, None, 8, t)),            # null out with a capacity
        (EINVAL, (m, 0, 64, 2, 0, a, 0, 0, 0, o, 8, t)),               # require with bit 0 clear
        (EINVAL, (m, 0, 64, 0, 0, a, 0, 0, 0, o, 8, t)),
        (EINVAL, (m, 0, 64, 3, 2, a, 0, 0, 0, o, 8, t)),               # require & forbid != 0
        (EINVAL, (m, 0, 64, 3, 1, a, 0, 0, 0, o, 8, t)),
        (EINVAL, (m, 0, 64, 3, 0, a, 0, 32, 0, o, 8, t)),              # above_bits > 31
        (EINVAL, (m, 0, 64, 3, 0, a, 64, 4, 0, o, 8, t)),              # above_shift > 63
        (EINVAL, (m, 0, 64, 3, 0, None, 0, 4, 0, o, 8, t)),            # null above with above_bits > 0
        (EINVAL, (m, 0, 64, 3, 0, a_mis, 0, 4, 0, o, 8, t)),           # misaligned above
        (ERANGE, (m, 2**62 - 10, 64, 3, 0, a, 0, 0, 0, o, 8, t)),      # g_start + nbits > 2^62
        (ERANGE, (m, 2**62 - 64, 64, 3, 0, a, 0, 1, 0, o, 8, t)),      # a visible candidate beyond 2^62
        (ERANGE, (m, 2**63, 64, 3, 0, a, 0, 0, 0, o, 8, t)),
        (ERANGE, (m, 0, 2**44 + 1, 3, 0, a, 0, 0, 0, o, 8, t)),        # more than 2^44 candidates
    ]
    for code, args in cases:
        assert L.dse_debug_tuples_host(*args) == code, args
        assert (out == A5).all() and L.dse_last_status() == code and L.dse_last_error(), args
    # legal edges: nbits = 0, a null above with above_bits = 0, a count with no buffer
    tot[:] = 9
    assert L.dse_debug_tuples_host(None, 5, 0, 3, 0, None, 0, 0, 0, None, 0, t) == 0 and tot.tolist() == [0, 0]
    mask[:] = 0xFFFFFFFFFFFFFFFF
    assert L.dse_debug_tuples_host(m, 0, 200, 3, 0, None, 63, 0, 0, None, 0, t) == 0 and tot.tolist() == [199, 0]
    assert (out == A5).all()
