"""Minimal Goldbach partitions of a mask on the CPU: dse_debug_goldbach_host runs
the Goldbach kernel's own __host__ __device__ per-word bodies
(csrc/dse_goldbach_word.h) in a plain loop, and dse_goldbach_merge joins adjacent
results by host arithmetic.

Expected values are numpy brute force on bool arrays (tests/goldbach_ref.py): a
loop over the small primes on the visible bits, with the module's own prime list;
never the library. Every word of the struct is compared, exactly.
"""
import os
import re

import numpy as np
import pytest

import goldbach_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_goldbach_prime", "dse_goldbach_reach", "dse_goldbach_dev_async", "dse_goldbach_range",
       "dse_goldbach_resident", "dse_goldbach_merge", "dse_debug_goldbach_host")
T = R.T
A5 = 0xA5A5A5A5A5A5A5A5
EINVAL, ERANGE = -1, -6

# first even with a minimal prime above every earlier one -> that prime, up to 4,000,000
RECORDS = [(6, 3), (12, 5), (30, 7), (98, 19), (220, 23), (308, 31), (556, 47), (992, 73), (2642, 103), (5372, 139),
           (7426, 173), (43532, 211), (54244, 233), (63274, 293), (113672, 313), (128168, 331), (194428, 359),
           (194470, 383), (413572, 389), (503222, 523), (1077422, 601), (3526958, 727), (3807404, 751)]
NB_4M = 1_999_998  # the evens 6 .. 4,000,000


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
    assert "goldbach_grid" in hdr and "additive questions" in hdr
    assert (_dse.GOLDBACH_WORDS, _dse.GOLDBACH_PRIMES, _dse.GOLDBACH_NONE) == (R.WORDS, R.PRIMES, R.NONE)


def test_small_primes_and_reach(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    assert L.dse_goldbach_prime(1023) == 8167 and L.dse_goldbach_prime(2047) == 17881
    assert L.dse_goldbach_reach(2048) == 8939
    assert [L.dse_goldbach_prime(i) for i in range(R.PRIMES)] == R.P
    assert L.dse_goldbach_prime(2048) == 0 and L.dse_goldbach_prime(2**32 - 1) == 0
    assert L.dse_goldbach_reach(0) == 8939 and L.dse_goldbach_reach(1) == 0 and L.dse_goldbach_reach(2) == 1
    assert [L.dse_goldbach_reach(n) for n in (17, 1024, 2047)] == [R.reach(17), R.reach(1024), R.reach(2047)]


# -- 1. real primes ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(oracle):
    from primes_ref import mask_bits
    m, _ = oracle.fast_sieve_range(0, NB_4M)
    bits = mask_bits(m, NB_4M)
    return m, bits, R.ranks(bits)


def test_real_primes_to_4e6(S, real):
    m, bits, rank = real
    got = S.goldbach_host(m, 0, NB_4M)
    assert not R.diff(got.words, R.struct(rank, 0, 0))
    assert (got.unresolved, got.resolved, got.first_unresolved_even) == (0, NB_4M, None)
    assert (got.max_prime, got.max_rank, got.max_even) == (751, 131, 3_807_404)
    assert int(got.hist.sum()) == NB_4M and int(got.hist[132:].sum()) == 0
    # the reference's own records are the pinned table
    best, rec = -1, []
    for c in np.flatnonzero(np.maximum.accumulate(rank) > np.concatenate([[-1], np.maximum.accumulate(rank)[:-1]])):
        assert rank[c] > best
        best = int(rank[c])
        rec.append((6 + 2 * int(c), R.P[best]))
    assert rec == RECORDS


def test_record_evens_by_prefix_calls(S, real):
    m, bits, rank = real
    for k, (even, prime) in enumerate(RECORDS):
        c = (even - 6) // 2
        got = S.goldbach_host(m, 0, c + 1)   # the evens 6 .. even: the record is the last of them
        assert (got.max_even, got.max_prime, got.unresolved) == (even, prime, 0), even
        if c:                                # and one even fewer still has the record before
            before = S.goldbach_host(m, 0, c)
            assert (before.max_even, before.max_prime) == RECORDS[k - 1], even
        if k in (3, 11, 22):
            assert not R.diff(got.words, R.struct(rank[:c + 1], 0, 0)), even


def test_record_evens_by_split_and_merge(S, real):
    """The range cut at every record even; a part sees the bits before it through a pointer and a
    shift into the same mask. After each merge the maximum is the record just added."""
    m, bits, rank = real
    cuts = [(e - 6) // 2 for e, _ in RECORDS] + [NB_4M]
    acc = None
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        bb = min(a, R.REACH + 70)
        lo = a - bb
        part = S.goldbach_host(R.pack_garbage(bits[a:b]), a, b - a, m[lo >> 6:], lo & 63, bb)
        acc = part if acc is None else acc.merge(part)
        assert (acc.g_start, acc.nbits) == (0, b)
        assert (acc.max_even, acc.max_prime, acc.unresolved) == (*RECORDS[k], 0), k
    assert not R.diff(acc.words, R.struct(rank, 0, 0))


# -- 2. synthetic masks: the per-word bodies against brute force ----------------------------------
def family_cases(nbits):
    """(g_start, below_bits, below_shift, nprimes) of the family for one size."""
    for nprimes in R.NPRIMES:
        for g in R.g_starts(nbits):
            for bb in R.below_sizes(nprimes, g):
                for shift in R.SHIFTS:
                    yield g, bb, shift, nprimes


@pytest.mark.parametrize("nbits", R.SIZES)
def test_host_matches_brute_force(S, nbits):
    ncases = 0
    for name in R.FILLS:
        bits, low = R.fill(name, nbits, 7000 + nbits)
        mask = R.pack_garbage(bits)
        rank, below = {}, {}
        for g, bb, shift, nprimes in family_cases(nbits):
            if bb not in rank:
                rank[bb] = R.ranks(bits, low[len(low) - bb:])
            if (bb, shift) not in below:
                below[bb, shift] = R.pack_below(low[len(low) - bb:], shift)
            got = S.goldbach_host(mask, g, nbits, below[bb, shift], shift, bb, nprimes)
            assert not R.diff(got.words, R.struct(rank[bb], g, nprimes)), (name, g, bb, shift, nprimes)
            ncases += 1
    assert ncases == 6 * 3 * sum(len(R.below_sizes(n, g)) for n in R.NPRIMES for g in R.g_starts(nbits))


def test_family_is_what_it_says():
    assert R.SIZES == [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 3 * T + 8939 + 3]
    assert R.g_starts(65) == [0, 1, 63, T - 1, 2**40 + 5, 2**61 - 2 - 65 + 1]
    assert R.below_sizes(0, 2**40 + 5) == [0, 1, 63, 64, 8938, 8939, 8940, 3 * 8939]
    assert R.below_sizes(17, 2**40 + 5) == [0, 1, 28, 29, 30, 63, 64, 87] and R.below_sizes(0, 63) == [0, 1, 63]
    n = 3 * T + 8939 + 3
    full_depth = R.brute(*R.fill("4096th", n, 7000 + n)[:1], 0)
    assert full_depth[4] > 0 and full_depth[6] > 1500    # unresolved evens, and a search over 1500 ranks deep
    assert R.brute(np.ones(10, bool), 5, 0, np.ones(3, bool))[8] == 10
    # the three ways of ranks() (all pairs at once up to 1024 evens; above that from the entries when they
    # are few, from the unresolved evens when they are many) against plain Python
    for n, name in ((900, "64th"), (1100, "64th"), (1100, "half")):
        bits, low = R.fill(name, n, 5)
        vis = np.concatenate([low[-100:], bits])
        plain = np.full(n, -1)
        for c in range(n):
            for i in range(R.PRIMES):
                j = c - int(R.H[i]) + 100
                if j >= 0 and vis[j]:
                    plain[c] = i
                    break
        assert np.array_equal(R.ranks(bits, low[-100:]), plain), (n, name)


def test_accessors(S):
    bits = np.zeros(40, bool)
    bits[[0, 1, 2, 4, 5]] = True           # 3 5 7 11 13 at g_start 0
    g = S.goldbach_host(R.pack(bits), 0, 40, nprimes=3)
    # 6=3+3 8=3+5 10=3+7 12=5+7 14=3+11 16=3+13 18=5+13 20=7+13 22: 3+19 5+17 7+.. none visible
    assert [int(v) for v in g.hist[:4]] == [5, 2, 1, 0]
    assert (g.nprimes, g.resolved, g.unresolved, g.first_unresolved_even) == (3, 8, 32, 22)
    assert (g.max_rank, g.max_prime, g.max_even, g.max_c) == (2, 7, 20, 7)
    assert g.hist.dtype == np.uint64 and g.hist.shape == (2048,)
    e = S.goldbach_host(np.zeros(0, np.uint64), 9, 0)
    assert (e.g_start, e.nbits, e.nprimes, e.resolved, e.unresolved) == (9, 0, 2048, 0, 0)
    assert (e.first_unresolved_even, e.max_prime, e.max_even) == (None, None, None)
    assert not R.diff(e.words, R.brute(np.zeros(0, bool), 9))


# -- 3. merge equals the whole ----------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FILLS)
def test_merge_equals_whole(S, name):
    nbits = 3 * T + 8939 + 3
    bits, low = R.fill(name, nbits, 31)
    for g, bb0 in ((0, 0), (2**40 + 5, R.REACH + 1), (T - 1, 77)):
        vis = np.concatenate([low[len(low) - bb0:], bits])      # position p is vis[bb0 + p]
        for nprimes in (0, 17):
            whole = S.goldbach_host(R.pack_garbage(bits), g, nbits, R.pack_below(vis[:bb0], 5), 5, bb0, nprimes)
            assert not R.diff(whole.words, R.brute(bits, g, nprimes, vis[:bb0]))
            for cut in (1, 64, T, T + 1, R.REACH - 1, nbits - 1):
                a = S.goldbach_host(R.pack_garbage(bits[:cut]), g, cut, R.pack_below(vis[:bb0], 0), 0, bb0, nprimes)
                bbb = min(bb0 + cut, g + cut)                    # everything visible before the cut
                b = S.goldbach_host(R.pack_garbage(bits[cut:]), g + cut, nbits - cut,
                                    R.pack_below(vis[bb0 + cut - bbb:bb0 + cut], 63), 63, bbb, nprimes)
                got = a.merge(b)
                assert not R.diff(got.words, whole.words), (name, g, nprimes, cut)
                assert got == whole
    # the tie rules: "ones" has its maximum (rank 0) and "zero" an unresolved even on both sides of every cut


def test_merge_ties_keep_the_first(S):
    ones = R.pack(np.ones(200, bool))
    a, b = S.goldbach_host(ones, 0, 100), S.goldbach_host(ones, 100, 100, ones, 0, 100)
    assert (a.max_rank, a.max_c, b.max_rank, b.max_c) == (0, 0, 0, 100)
    assert (a.merge(b).max_rank, a.merge(b).max_c) == (0, 0)
    zero = np.zeros(4, np.uint64)
    a, b = S.goldbach_host(zero, 7, 100), S.goldbach_host(zero, 107, 100)
    assert (a.first_unresolved, b.first_unresolved, a.merge(b).first_unresolved) == (7, 107, 7)
    # a has none: b's; a strictly greater maximum on the right wins
    a = S.goldbach_host(ones, 0, 100)
    bits = np.zeros(100, bool)
    bits[50] = True
    b = S.goldbach_host(R.pack(bits), 100, 100)
    m = a.merge(b)
    assert (a.first_unresolved, m.first_unresolved) == (None, 100)
    assert (b.max_rank, m.max_rank, m.max_c) == (b.max_rank, b.max_rank, b.max_c) and b.max_rank > 0


def test_merge_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    bits = np.random.default_rng(4).random(300) < 0.3
    m = R.pack(bits)
    a, b = S.goldbach_host(R.pack(bits[:100]), 0, 100), S.goldbach_host(R.pack(bits[100:]), 100, 200, m, 0, 100)
    assert not R.diff(a.merge(b).words, R.brute(bits, 0))
    cases = [(EINVAL, a, S.goldbach_host(R.pack(bits[100:]), 101, 200)),           # a hole between them
             (EINVAL, a, S.goldbach_host(R.pack(bits[100:]), 99, 200)),            # an overlap
             (EINVAL, b, a),                                                       # the wrong order
             (EINVAL, a, S.goldbach_host(R.pack(bits[100:]), 100, 200, nprimes=2047))]
    for code, x, y in cases:
        out = np.full(R.WORDS, A5, dtype=np.uint64)
        assert L.dse_goldbach_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == code
        assert (out == A5).all()
        with pytest.raises(_dse.DseError) as e:
            x.merge(y)
        assert e.value.code == code
    assert L.dse_goldbach_merge(None, _dse.u64p(b.words), _dse.u64p(a.words.copy())) == EINVAL
    assert L.dse_goldbach_merge(_dse.u64p(a.words), _dse.u64p(b.words), None) == EINVAL
    # a union that ends above 2^62
    x, y = S.Goldbach(a.words.copy()), S.Goldbach(b.words.copy())
    x.words[0], x.words[1] = 2**62 - 100, 100
    y.words[0], y.words[1] = 2**62, 200
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    assert L.dse_goldbach_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == ERANGE
    assert (out == A5).all()
    # out may alias either side
    aw, bw = a.words.copy(), b.words.copy()
    assert L.dse_goldbach_merge(_dse.u64p(aw), _dse.u64p(b.words), _dse.u64p(aw)) == 0
    assert L.dse_goldbach_merge(_dse.u64p(a.words), _dse.u64p(bw), _dse.u64p(bw)) == 0
    assert np.array_equal(aw, bw) and not R.diff(aw, R.brute(bits, 0))


# -- 4. argument errors ---------------------------------------------------------------------------------
def test_host_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(4, dtype=np.uint64)
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    mp, op = _dse.u64p(m), _dse.u64p(out)
    import ctypes
    odd = ctypes.cast(ctypes.c_void_p(m.ctypes.data + 4), ctypes.POINTER(ctypes.c_uint64))
    for code, args in [(EINVAL, (mp, 100, 64, mp, 0, 10, 0, None)),        # null out
                       (EINVAL, (None, 100, 64, mp, 0, 10, 0, op)),        # null mask with nbits > 0
                       (EINVAL, (mp, 100, 64, mp, 0, 10, 2049, op)),       # nprimes above 2048
                       (EINVAL, (mp, 100, 64, mp, 64, 10, 0, op)),         # below_shift above 63
                       (EINVAL, (mp, 100, 64, mp, 0, 101, 0, op)),         # below_bits above g_start
                       (EINVAL, (mp, 0, 64, mp, 0, 1, 0, op)),
                       (EINVAL, (mp, 100, 64, None, 0, 10, 0, op)),        # null below with below_bits > 0
                       (EINVAL, (mp, 100, 64, odd, 0, 10, 0, op)),         # misaligned below
                       (ERANGE, (mp, 2**62 - 10, 64, None, 0, 0, 0, op)),  # g_start + nbits > 2^62
                       (ERANGE, (mp, 2**63, 64, None, 0, 0, 0, op)),
                       (ERANGE, (mp, 0, 2**44 + 1, None, 0, 0, 0, op))]:   # more than 2^44 candidates
        assert L.dse_debug_goldbach_host(*args) == code, args
        assert (out == A5).all(), args
    assert L.dse_last_status() == ERANGE and L.dse_last_error()
    # a null below is fine without below_bits, and nbits = 0 needs no mask
    assert L.dse_debug_goldbach_host(mp, 100, 64, None, 63, 0, 1, op) == 0
    assert L.dse_debug_goldbach_host(None, 100, 0, None, 0, 0, 2048, op) == 0
    assert not R.diff(out, R.brute(np.zeros(0, bool), 100))
