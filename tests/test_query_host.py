"""Rank and select on the host (csrc/dse_query_word.h through
dse_debug_query_host): the query kernel's per-word and per-tile bodies over a
host mask, no device call.

Expected answers are numpy.searchsorted over the entry values of the test's own
bits (tests/query_ref.py); every comparison is exact.
"""
import ctypes
import random

import numpy as np
import pytest

import query_ref as R

T = R.T
EINVAL, ERANGE = -1, -6
A5 = 0xA5A5A5A5A5A5A5A5
KIND_NAMES = ("RANK", "SELECT", "NEXT", "PREV", "TEST")


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


def test_constants_are_the_headers(S):
    assert (S.QUERY_RANK, S.QUERY_SELECT, S.QUERY_NEXT, S.QUERY_PREV, S.QUERY_TEST) == R.KINDS
    assert S.QUERY_NONE == R.NONE
    for nbits, tiles in ((0, 0), (1, 1), (T, 1), (T + 1, 2), (10 * T, 10)):
        assert S.query_index_bytes(nbits) >= 8 * (tiles + 1)
        assert S.query_index_bytes(nbits) % 8 == 0


@pytest.mark.parametrize("nbits", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37])
def test_patterns_against_searchsorted(S, nbits):
    for name, bits in R.masks(nbits, T, 4100 + nbits).items():
        m = R.pack_garbage(bits)  # every bit past nbits in the last word set: ignored
        for g in R.g_starts(nbits, T):
            vals = R.values(bits, g)
            for kind in R.KINDS:
                q = R.queries(bits, g, kind)
                got = S.query_host(m, g, nbits, kind, q)
                want = R.expect(vals, kind, q)
                bad = np.flatnonzero(got != want)
                assert not len(bad), (name, g, KIND_NAMES[kind], int(q[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


def test_next_prev_are_right_whatever_the_gap(S):
    """Two entries 3 T + 5 places apart: NEXT and PREV cross the empty tiles between them."""
    nbits = 5 * T
    bits = np.zeros(nbits, bool)
    bits[[T - 3, 4 * T + 2]] = True
    m, g = R.pack(bits), 1000
    a, b = 3 + 2 * (g + T - 3), 3 + 2 * (g + 4 * T + 2)
    q = R.u64([a - 1, a, a + 1, (a + b) // 2, b - 1, b, b + 1])
    assert [int(v) for v in S.query_host(m, g, nbits, R.NEXT, q)] == [a, b, b, b, b, R.NONE, R.NONE]
    assert [int(v) for v in S.query_host(m, g, nbits, R.PREV, q)] == [R.NONE, R.NONE, a, a, a, a, b]
    assert [int(v) for v in S.query_host(m, g, nbits, R.SELECT, R.u64([0, 1, 2]))] == [a, b, R.NONE]


def test_empty_range(S):
    q = R.u64([0, 3, 5, 2**63, R.NONE])
    for kind, want in ((R.RANK, 0), (R.SELECT, R.NONE), (R.NEXT, R.NONE), (R.PREV, R.NONE), (R.TEST, 0)):
        assert [int(v) for v in S.query_host(np.zeros(0, np.uint64), 17, 0, kind, q)] == [want] * len(q)
    assert len(S.query_host(np.zeros(1, np.uint64), 0, 64, R.RANK, [])) == 0


def select64_by_clearing(w, k):
    for _ in range(k):
        w &= w - 1
    return (w & -w).bit_length() - 1


def test_select_in_word_every_k(S):
    """select inside a word: every k of 1,000 random words and of 0, 1, 1 << 63, ~0, through
    SELECT on one-word ranges (the value of rank k is 3 + 2 * bit index)."""
    rng = random.Random(0x5E1EC7)
    words = [0, 1, 1 << 63, (1 << 64) - 1] + [rng.getrandbits(64) for _ in range(1000)]
    words += [rng.getrandbits(64) & rng.getrandbits(64) & rng.getrandbits(64) for _ in range(100)]  # sparse ones
    q = R.u64(range(65))
    for w in words:
        got = S.query_host(R.u64([w]), 0, 64, R.SELECT, q)
        pop = bin(w).count("1")
        want = [3 + 2 * select64_by_clearing(w, k) for k in range(pop)] + [R.NONE] * (65 - pop)
        assert [int(v) for v in got] == want, hex(w)


def test_x_to_odd_index_does_not_wrap(S):
    """The range that ends at the last legal candidate, and every x around 2^63 and 2^64."""
    nbits = 130
    g = 2**62 - nbits
    bits = np.ones(nbits, bool)
    vals = R.values(bits, g)
    q = R.u64([2**63 - 2, 2**63 - 1, 2**63, 2**63 + 1, 2**63 + 2, 2**63 + 3, 2**64 - 2, 2**64 - 1, int(vals[0]) - 1,
               int(vals[0]), int(vals[-1]), int(vals[-1]) + 1])
    for kind in R.VALUE_KINDS:
        got = S.query_host(R.pack(bits), g, nbits, kind, q)
        assert np.array_equal(got, R.expect(vals, kind, q)), KIND_NAMES[kind]


def test_error_codes(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(4, dtype=np.uint64)
    q = np.zeros(3, dtype=np.uint64)
    out = np.full(3, A5, dtype=np.uint64)
    mp, qp, op = _dse.u64p(m), _dse.u64p(q), _dse.u64p(out)
    cases = [
        (EINVAL, (mp, 0, 64, 5, qp, 3, op)),             # unknown kind
        (EINVAL, (mp, 0, 64, 0xFFFFFFFF, qp, 3, op)),
        (EINVAL, (None, 0, 64, 0, qp, 3, op)),           # null mask with nbits > 0
        (EINVAL, (mp, 0, 64, 0, None, 3, op)),           # null queries with nq > 0
        (EINVAL, (mp, 0, 64, 0, qp, 3, None)),           # null answers with nq > 0
        (ERANGE, (mp, 2**62 - 10, 64, 0, qp, 3, op)),    # g_start + nbits > 2^62
        (ERANGE, (mp, 2**63, 64, 0, qp, 3, op)),
        (ERANGE, (mp, 0, 2**44 + 1, 0, qp, 3, op)),      # more than 2^44 candidates
    ]
    for code, args in cases:
        assert L.dse_debug_query_host(*args) == code, args
        assert (out == A5).all(), args
    assert L.dse_last_status() == ERANGE and L.dse_last_error()
    assert L.dse_debug_query_host(None, 5, 0, 0, None, 0, None) == 0  # nothing to read, nothing to answer
    assert L.dse_debug_query_host(mp, 0, 256, 0, qp, 3, op) == 0 and not out.any()
