"""Residue pairs of consecutive primes, on the CPU: dse_debug_consec_host runs the
consec kernels' own __host__ __device__ per-word bodies (csrc/dse_consec_word.h) in
a plain loop over tiles and words; dse_consec_merge joins adjacent results by host
arithmetic.

Expected values are numpy on bool arrays (tests/consec_ref.py: flatnonzero, the
classes of the values, bincount over the pairs of neighbours), tied below to a plain
Python loop, the class counts of tests/race_ref.py, and entries pinned from an
independent numpy sieve; never the library. Every word of the struct is compared,
exactly.
"""
import os
import re

import numpy as np
import pytest

import consec_ref as R
import race_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_consec_dev_async", "dse_consec_range", "dse_consec_resident", "dse_consec_merge",
       "dse_debug_consec_host")
T = R.T
EINVAL, ERANGE = -1, -6
A5 = 0xA5A5A5A5A5A5A5A5
NB_1E6 = (10**6 - 3) // 2 + 1  # the candidates of 3 .. 10^6


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


def host(S, bits, g, q, garbage=True):
    return S.consec_host(R.pack_garbage(bits) if garbage else R.pack(bits), g, len(bits), q)


def loop_ref(bits, g_start, q):
    """brute()'s result by a plain Python loop over the candidates."""
    w = [0] * R.WORDS
    w[0], w[1], w[2], w[5], w[6] = g_start, len(bits), q, R.NONE, R.NONE
    prev = None
    for i, b in enumerate(bits):
        if not b:
            continue
        w[3] += 1
        v = (3 + 2 * (g_start + i)) % q
        if prev is None:
            w[5] = g_start + i
        else:
            w[7 + 64 * prev + v] += 1
            w[4] += 1
        prev = v
        w[6] = g_start + i
    return np.array(w, dtype=np.uint64)


def identities(words, bits, g, q):
    """The sums every dse_consec obeys, against the class counts of race_ref.brute."""
    m = words[7:].reshape(64, 64).astype(np.int64)
    primes, pairs = int(words[3]), int(words[4])
    assert int(m.sum()) == pairs == max(primes - 1, 0)
    assert not m[q:].any() and not m[:, q:].any()
    cls = race_ref.brute(bits, g, q, 1, 1)[17:17 + 64].astype(np.int64)
    idx = np.flatnonzero(bits)
    first = np.zeros(64, np.int64)
    last = np.zeros(64, np.int64)
    if len(idx):
        first[(3 + 2 * (g + int(idx[0]))) % q] = 1
        last[(3 + 2 * (g + int(idx[-1]))) % q] = 1
    assert np.array_equal(m.sum(axis=1), cls - last)
    assert np.array_equal(m.sum(axis=0), cls - first)
    for r in range(q):
        if not race_ref.has_candidates(q, r):
            assert not m[r].any() and not m[:, r].any()


def test_header_declares_and_library_exports_the_entry_points(S):
    from mail_sieve_e import _dse
    hdr = open(os.path.join(ROOT, "include", "dse.h")).read()
    declared = set(re.findall(r"\b(dse_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = _dse.lib()
    for s in NEW:
        assert s in declared, f"include/dse.h does not declare {s}"
        assert hasattr(L, s), f"libdse.so does not export {s}"
        assert s in _dse.SIGNATURES, f"ctypes binding misses {s}"
    assert "consec_grid" in hdr and "consec_flush_tiles" in hdr and "residue pairs of consecutive primes" in hdr
    assert (_dse.CONSEC_WORDS, _dse.CONSEC_MAX_MODULUS, _dse.CONSEC_NONE) == (R.WORDS, R.MAX_MODULUS, R.NONE)
    m = re.search(r"typedef struct dse_consec \{(.*?)\} dse_consec;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert set(re.findall(r"^\s*(\w+)\s", body, flags=re.M)) == {"uint64_t"}
    members = [x.strip() for decl in re.findall(r"uint64_t([^;]*);", body) for x in decl.split(",")]
    words = sum(R.BINS if "[DSE_CONSEC_MAX_MODULUS * DSE_CONSEC_MAX_MODULUS]" in x else 1 for x in members)
    assert 8 * words == 8 * 4103 == 8 * _dse.CONSEC_WORDS  # sizeof(dse_consec): uint64 members only, no padding


def test_reference_is_the_plain_loop():
    rng = np.random.default_rng(0xC0115EC)
    n = 0
    for size, p in ((0, 0.5), (1, 1.0), (2, 1.0), (130, 0.5), (400, 0.05), (700, 1 / 300), (90, 0.0)):
        for _ in range(12):
            bits = rng.random(size) < p
            for q in (3, 4, 10, 63, 64):
                g = int(rng.choice(R.G_STARTS))
                assert np.array_equal(R.brute(bits, g, q), loop_ref(bits, g, q)), (size, p, g, q)
                n += 1
    assert n >= 300
    w = R.brute(np.array([1, 1, 1, 0, 1], bool), 0, 3)  # 3 5 7 11
    assert (R.entry(w, 0, 2), R.entry(w, 2, 1), R.entry(w, 1, 2), int(w[3]), int(w[4])) == (1, 1, 1, 4, 3)


def test_thinned_family_covers_every_value():
    assert [R.period(q) for q in R.QS] == [3, 2, 5, 7, 4, 6, 15, 63, 32]
    for nbits in R.SIZES:
        seen = [c for k in range(len(R.FILLS)) for c in R.thinned(nbits, k)]
        assert {c[0] for c in seen} == set(R.G_STARTS), nbits
        assert {c[1] for c in seen} == set(R.QS), nbits
    assert sorted(c for k in range(len(R.FILLS)) for c in R.thinned(T + 1, k)) == sorted(R.cases())


# -- 1. the per-word bodies against the reference ----------------------------------------------
@pytest.mark.parametrize("nbits", R.SIZES)
def test_host_matches_reference(S, nbits):
    for k, name in enumerate(R.FILLS):
        bits = R.fill(name, nbits, 8000 + nbits)
        for g, q in R.thinned(nbits, k):
            got = host(S, bits, g, q)
            assert not R.diff(got.words, R.brute(bits, g, q)), (name, g, q)
            identities(got.words, bits, g, q)
    for q in (3, 10, 64):
        assert not R.diff(host(S, np.zeros(0, bool), 5, q).words, R.brute(np.zeros(0, bool), 5, q))


def test_every_modulus_and_start(S):
    bits = R.fill("16th", 2 * T + 700, 77)
    dense = R.fill("half", 900, 78)
    for q in range(3, 65):
        for g in (0, q - 1, 2**40 + q):
            assert not R.diff(host(S, bits, g, q).words, R.brute(bits, g, q)), (q, g)
            assert not R.diff(host(S, dense, g, q).words, R.brute(dense, g, q)), (q, g)


def test_accessors(S):
    bits = np.zeros(100, bool)
    bits[[0, 1, 2, 4, 10, 12]] = True  # 3 5 7 11 23 27 at g_start 0
    c = host(S, bits, 0, 10)
    assert (c.g_start, c.nbits, c.q, c.primes, c.pairs, c.first_g, c.last_g) == (0, 100, 10, 6, 5, 0, 12)
    assert c.matrix.dtype == np.uint64 and c.matrix.shape == (10, 10) and c.counts.shape == (64, 64)
    want = np.zeros((10, 10), np.uint64)
    for a, b in ((3, 5), (5, 7), (7, 1), (1, 3), (3, 7)):
        want[a, b] += 1
    assert np.array_equal(c.matrix, want) and "q=10" in repr(c) and "pairs=5" in repr(c)
    assert c == S.Consec(c.words.copy()) and c != host(S, bits, 1, 10) and c != host(S, bits, 0, 12)
    one = np.zeros(300, bool)
    one[177] = True
    c = host(S, one, 9, 7)
    assert (c.primes, c.pairs, c.first_g, c.last_g) == (1, 0, 186, 186) and not c.counts.any()
    empty = host(S, np.zeros(7, bool), 5, 7)
    assert (empty.primes, empty.pairs, empty.first_g, empty.last_g) == (0, 0, None, None)
    with pytest.raises(ValueError):
        S.Consec(np.zeros(5, dtype=np.uint64))


# -- 2. planted pairs ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PLANTED)
def test_planted_pairs(S, name):
    bits, p, q2 = R.planted(name)
    for q in (4, 10, 7, 63):
        for g in (1, 2**40 + 11):  # not 0 mod the period
            assert g % R.period(q)
            want = R.brute(bits, g, q)
            got = host(S, bits, g, q, garbage=False)
            assert not R.diff(got.words, want), (name, q, g)
            assert R.entry(want, (3 + 2 * (g + p)) % q, (3 + 2 * (g + q2)) % q) >= 1
            identities(got.words, bits, g, q)


# -- 3. the top of the range -----------------------------------------------------------------------
def test_top_of_the_range(S):
    rng = np.random.default_rng(62)
    nb = 3 * 64 + 17
    bits = rng.random(nb) < 0.3
    bits[-1] = True
    g = 2**62 - nb  # the last candidate is 2^62 - 1
    for q in (3, 10, 63, 64):
        got = host(S, bits, g, q)
        assert not R.diff(got.words, loop_ref(bits, g, q)), q
        assert got.last_g == 2**62 - 1
    from mail_sieve_e import _dse
    with pytest.raises(_dse.DseError) as e:
        host(S, bits, g + 1, 10)
    assert e.value.code == ERANGE
    assert host(S, bits[:-1], g + 1, 10).last_g is not None  # and one candidate fewer is accepted


# -- 4. real primes ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(oracle):
    from primes_ref import mask_bits
    m, _ = oracle.fast_sieve_range(0, NB_1E6)
    return m, mask_bits(m, NB_1E6)


def test_real_primes_to_1e6(S, real):
    m, bits = real
    assert np.array_equal(bits, R.sieve_bits(10**6))
    for q, pinned in R.PINNED_1E6.items():
        got = S.consec_host(m, 0, NB_1E6, q)
        want = R.brute(bits, 0, q)
        assert not R.diff(got.words, want), q
        assert (got.primes, got.pairs, got.first_g, 3 + 2 * got.last_g) == (78_497, 78_496, 0, 999_983)
        for (a, b), n in pinned.items():
            assert int(got.matrix[a, b]) == n, (q, a, b)
        identities(got.words, bits, 0, q)
    for q in (30, 63, 64):
        assert not R.diff(S.consec_host(m, 0, NB_1E6, q).words, R.brute(bits, 0, q)), q
    los = S.consec_host(m, 0, NB_1E6, 10).matrix  # the diagonal is depressed: the bias of the paper
    for a in (1, 3, 7, 9):
        assert all(los[a, a] < los[a, b] for b in (1, 3, 7, 9) if b != a)


# -- 5. merge equals union ------------------------------------------------------------------------------
def fold(S, bits, g, q, cuts):
    """The results of the pieces of bits cut at `cuts` (the reference's, not the library's), merged by
    the library as a left and as a right fold."""
    edges = [0] + list(cuts) + [len(bits)]
    parts = [S.Consec(R.brute(bits[a:b], g + a, q)) for a, b in zip(edges, edges[1:])]
    left = parts[0]
    for p in parts[1:]:
        left = left.merge(p)
    right = parts[-1]
    for p in reversed(parts[:-1]):
        right = p.merge(right)
    return left, right


def random_cuts(rng, n):
    """1 or 2 sorted cuts of [0, n]: random places, inside words, repeats (empty pieces) and pieces of
    one candidate."""
    k = int(rng.integers(1, 3))
    cuts = [int(c) for c in rng.integers(0, n + 1, size=k)]
    if k == 2 and rng.random() < 0.5:
        cuts[1] = min(n, cuts[0] + int(rng.choice([0, 1, 2, 40])))
    return sorted(cuts)


def test_merge_equals_union(S, real):
    rng = np.random.default_rng(0xC0115EC)
    cases = [("real", real[1][:60_000]), ("real tail", real[1][440_000:])]
    for nbits in (65, 1000, T + 1):
        cases += [(f"{name} {nbits}", R.fill(name, nbits, 8000 + nbits)) for name in R.FILLS]
    cases += [("one", np.arange(500) == 250), ("two", np.isin(np.arange(500), (0, 499)))]
    splits = 0
    for k, (name, bits) in enumerate(cases):
        g, q = R.G_STARTS[k % 8], R.QS[k % 9]
        whole = R.brute(bits, g, q)
        for _ in range(17):
            cuts = random_cuts(rng, len(bits))
            for got in fold(S, bits, g, q, cuts):
                assert not R.diff(got.words, whole), (name, q, cuts)
            splits += 1
    assert splits >= 300


def test_merge_with_a_seam_inside_a_named_pair(S, real):
    bits = real[1][:200_000]
    for q in (3, 4, 10, 30):
        whole = R.brute(bits, 0, q)
        # 113 -> 127, 1327 -> 1361, 31397 -> 31469, 155921 -> 156007, 360653 -> 360749
        for p, p2 in ((113, 127), (1327, 1361), (31397, 31469), (155_921, 156_007), (360_653, 360_749)):
            gp, gq = (p - 3) // 2, (p2 - 3) // 2
            assert bits[gp] and bits[gq] and not bits[gp + 1:gq].any()
            for cut in (gp + 1, (gp + gq) // 2, gq):
                for cuts in ([cut], [cut, cut], [gp + 1, gq], [0, cut, len(bits)]):
                    for got in fold(S, bits, 0, q, cuts):
                        assert not R.diff(got.words, whole), (q, p, cuts)
                a, b = R.brute(bits[:cut], 0, q), R.brute(bits[cut:], cut, q)
                # neither side has the pair: the seam does, once
                assert R.entry(a, p % q, p2 % q) + R.entry(b, p % q, p2 % q) + 1 == R.entry(whole, p % q, p2 % q)


def test_merge_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    bits = np.random.default_rng(4).random(300) < 0.3
    a, b = host(S, bits[:100], 0, 10), host(S, bits[100:], 100, 10)
    assert not R.diff(a.merge(b).words, R.brute(bits, 0, 10))
    for code, x, y in [(EINVAL, a, host(S, bits[100:], 101, 10)),  # a hole between them
                       (EINVAL, a, host(S, bits[100:], 99, 10)),   # an overlap
                       (EINVAL, b, a),                             # the wrong order
                       (EINVAL, a, host(S, bits[100:], 100, 12))]:  # another modulus
        out = np.full(R.WORDS, A5, dtype=np.uint64)
        assert L.dse_consec_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == code
        assert (out == A5).all()
        with pytest.raises(_dse.DseError) as e:
            x.merge(y)
        assert e.value.code == code
    for bad in (2, 65, 0):  # equal, but no modulus
        x, y = S.Consec(a.words.copy()), S.Consec(b.words.copy())
        x.words[2] = y.words[2] = bad
        out = np.full(R.WORDS, A5, dtype=np.uint64)
        assert L.dse_consec_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == EINVAL
        assert (out == A5).all()
    assert L.dse_consec_merge(None, _dse.u64p(b.words), _dse.u64p(a.words.copy())) == EINVAL
    assert L.dse_consec_merge(_dse.u64p(a.words), None, _dse.u64p(a.words.copy())) == EINVAL
    assert L.dse_consec_merge(_dse.u64p(a.words), _dse.u64p(b.words), None) == EINVAL
    # a union that ends above 2^62
    x, y = S.Consec(a.words.copy()), S.Consec(b.words.copy())
    x.words[0], x.words[1] = 2**62 - 100, 100
    y.words[0], y.words[1] = 2**62, 200
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    assert L.dse_consec_merge(_dse.u64p(x.words), _dse.u64p(y.words), _dse.u64p(out)) == ERANGE
    assert (out == A5).all()
    # out may alias either side
    aw, bw = a.words.copy(), b.words.copy()
    assert L.dse_consec_merge(_dse.u64p(aw), _dse.u64p(b.words), _dse.u64p(aw)) == 0
    assert L.dse_consec_merge(_dse.u64p(a.words), _dse.u64p(bw), _dse.u64p(bw)) == 0
    assert np.array_equal(aw, bw) and not R.diff(aw, R.brute(bits, 0, 10))


# -- 6. argument errors of what runs without a GPU -----------------------------------------------------
def test_host_refusals(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(2, dtype=np.uint64)
    out = np.full(R.WORDS, A5, dtype=np.uint64)
    mp, op = _dse.u64p(m), _dse.u64p(out)
    for code, args in [(EINVAL, (mp, 0, 64, 10, None)), (EINVAL, (None, 0, 64, 10, op)),
                       (EINVAL, (mp, 0, 64, 2, op)), (EINVAL, (mp, 0, 64, 65, op)), (EINVAL, (mp, 0, 64, 0, op)),
                       (ERANGE, (mp, 2**62 - 10, 64, 10, op)), (ERANGE, (mp, 2**63, 64, 10, op)),
                       (ERANGE, (mp, 0, 2**44 + 1, 10, op))]:
        assert L.dse_debug_consec_host(*args) == code, args
        assert (out == A5).all()
    assert L.dse_debug_consec_host(None, 5, 0, 10, op) == 0 and not R.diff(out, R.brute(np.zeros(0, bool), 5, 10))
    # the entry points that need a context refuse a null one before any device call
    for rc in (L.dse_consec_dev_async(None, 0, 64, None, 10, None, None), L.dse_consec_range(None, 0, 64, 10, op),
               L.dse_consec_resident(None, 0, 10, op)):
        assert rc == EINVAL
