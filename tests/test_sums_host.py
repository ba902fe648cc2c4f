"""Power and reciprocal sums, on the CPU: dse_debug_sums_host runs the sums kernels'
own __host__ __device__ per-word and per-entry bodies (csrc/dse_sums_word.h) in a
plain loop over the words of a host mask, the device's division routine included;
dse_debug_sums_recip runs that routine alone; dse_sums_merge adds adjacent results
by host arithmetic.

Expected values are Python ints over numpy.flatnonzero of the test's own bits, the
pattern applied by tests/tuples_ref.py's shifted ANDs (tests/sums_ref.py); never the
library. Every word of the struct is compared, exactly.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import sums_ref as R
import tuples_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_sums_dev_async", "dse_sums_range", "dse_sums_resident", "dse_sums_merge", "dse_debug_sums_host",
       "dse_debug_sums_recip")
T = R.T  # "sums_tile_bits" (a context reports the library's: tests/test_gpu_sums.py checks it is this)
EINVAL, ERANGE = -1, -6
SPAN32 = (1 | 1 << 31, 0)
PATTERNS = [(1, 0), TR.TWINS, TR.SEXT, SPAN32, TR.exact_gap_ref(3), TR.exact_gap_ref(31)]


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


def host(S, bits, g, require=1, forbid=0, above=(), shift=0, flags=3, rng=None, garbage=True):
    a = TR.pack_above(np.asarray(above, bool), shift, rng or np.random.default_rng(1)) if len(above) else None
    return S.sums_host(R.pack_garbage(bits) if garbage else R.pack(bits), g, len(bits), require, forbid, a, shift,
                       len(above), flags)


def test_header_declares_and_library_exports_the_entry_points(S):
    from mail_sieve_e import _dse
    hdr = open(os.path.join(ROOT, "include", "dse.h")).read()
    declared = set(re.findall(r"\b(dse_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = _dse.lib()
    for s in NEW:
        assert s in declared, f"include/dse.h does not declare {s}"
        assert hasattr(L, s), f"libdse.so does not export {s}"
        assert s in _dse.SIGNATURES, f"ctypes binding misses {s}"
    assert "sums_grid" in hdr and "sums_tile_bits" in hdr
    assert (_dse.SUMS_WORDS, _dse.SUMS_NONE, _dse.SUMS_POWER, _dse.SUMS_RECIP, _dse.SUMS_RECIP_SHIFT) == \
        (R.WORDS, R.NONE, R.POWER, R.RECIP, R.SHIFT)
    for name, val in (("DSE_SUMS_POWER", "1u"), ("DSE_SUMS_RECIP", "2u"), ("DSE_SUMS_NONE", "UINT64_MAX"),
                      ("DSE_SUMS_RECIP_SHIFT", "126"), ("DSE_SUMS_WORDS", "17")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, val), hdr), name
    m = re.search(r"typedef struct dse_sums \{(.*?)\} dse_sums;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert set(re.findall(r"^\s*(\w+)\s", body, flags=re.M)) == {"uint64_t"}
    members = [x.strip() for decl in re.findall(r"uint64_t([^;]*);", body) for x in decl.split(",")]
    words = sum(int(re.search(r"\[(\d+)\]", x).group(1)) if "[" in x else 1 for x in members)
    assert 8 * words == 8 * 17 == 8 * _dse.SUMS_WORDS  # sizeof(dse_sums): uint64 members only, no padding
    assert [re.sub(r"\[.*", "", x) for x in members] == ["g_start", "nbits", "require", "forbid", "above_bits", "flags",
                                                         "matches", "first_g", "last_g", "sum1", "sum2", "recip"]


# -- 1. the division routine alone ---------------------------------------------------------------
def check_recip(S, vs):
    got = S.sums_recip_host(np.array(vs, dtype=np.uint64))
    want = [R.ONE // v for v in vs]
    if got != want:
        bad = [(v, g, w) for v, g, w in zip(vs, got, want) if g != w]
        raise AssertionError(f"{len(bad)} quotients differ, first: v={bad[0][0]} got {bad[0][1]} want {bad[0][2]}")


def test_recip_small_and_edges(S):
    check_recip(S, [3, 5, 7])
    check_recip(S, list(range(3, 1 << 16, 2)))
    edges = [x for k in range(2, 63) for x in ((1 << k) - 1, (1 << k) + 1)]
    edges += [(1 << b) - d for b in (32, 53, 62) for d in (1, 3, 5)]
    edges += [(1 << 63) + 1, (1 << 63) - 1, (1 << 64) - 1]  # values up to the odd-index bound, and the routine's own
    check_recip(S, edges)


@pytest.mark.parametrize("lo", range(2, 63, 8))
def test_recip_random_per_bit_length(S, lo):
    rng = np.random.default_rng(0x5EC1 + lo)
    for bl in range(lo, min(lo + 8, 63)):  # odd v of bit length bl: 2 .. 62
        n = min(100_000, 1 << (bl - 2)) if bl > 2 else 1
        v = (rng.integers(1 << (bl - 1), 1 << bl, size=n, dtype=np.uint64) | np.uint64(1))
        check_recip(S, v.tolist())


def test_recip_refusals(S):
    from mail_sieve_e import _dse
    for v in (0, 1, 2):
        with pytest.raises(_dse.DseError) as e:
            S.sums_recip_host([5, v])
        assert e.value.code == ERANGE


# -- 2. the per-word bodies against the reference ------------------------------------------------
@pytest.mark.parametrize("nbits", [1, 63, 64, 65, 1000, T - 1, T, T + 1, 2 * T + 77])
def test_host_matches_reference_on_synthetic_masks(S, nbits):
    for name, bits in R.masks(nbits, 9100 + nbits).items():
        for g in R.g_starts() + (R.TOP - nbits,):
            if name in ("ones", "half") and nbits > 2000 and g not in (37, R.TOP - nbits):
                continue  # the dense fills: one misaligned start and the top are enough at this length
            assert not R.diff(host(S, bits, g), R.brute(bits, g)), (name, g)


def test_empty_range(S):
    for g in (0, 5, R.TOP):
        assert not R.diff(host(S, np.zeros(0, bool), g), R.brute(np.zeros(0, bool), g))
        assert not R.diff(host(S, np.zeros(0, bool), g, 3, 0, flags=2), R.brute(np.zeros(0, bool), g, 3, 0, (), 2))


def test_accessors(S):
    bits = np.zeros(100, bool)
    bits[[0, 1, 2, 4, 5, 7]] = True  # 3 5 7 11 13 17
    s = host(S, bits, 0, 3, 0)
    assert (s.matches, s.first, s.last, s.first_g, s.last_g, s.require, s.forbid, s.flags) == (3, 3, 11, 0, 4, 3, 0, 3)
    assert s.sum1 == 3 + 5 + 11 and s.sum2 == 9 + 25 + 121
    assert s.recip == sum(R.ONE // v for v in (3, 5, 5, 7, 11, 13))
    lo, hi = s.reciprocal_bounds()
    true = sum(Fraction(1, v) for v in (3, 5, 5, 7, 11, 13))
    assert isinstance(lo, Fraction) and lo <= true <= hi and hi - lo == Fraction(6, R.ONE)
    assert abs(s.reciprocal - float(true)) < 1e-15
    e = host(S, np.zeros(10, bool), 7)
    assert (e.matches, e.first, e.last, e.sum1, e.sum2, e.recip) == (0, None, None, 0, 0, 0)


# -- 3. limb carries, each asserted to occur in the reference ------------------------------------
def test_carries_at_the_top_of_the_range(S):
    n = 2 * T
    g = R.TOP - n
    want = R.ones_words(g, n, flags=R.POWER)
    assert want[10] != 0 and want[13] != 0  # sum1 carries into limb 1, sum2 into limb 2
    got = S.sums_host(np.full(n // 64, R.NONE, dtype=np.uint64), g, n, 1, 0, flags=R.POWER)
    assert not R.diff(got, want)
    # the additions themselves carry: the sums of the two tiles, merged
    a = S.sums_host(np.full(T // 64, R.NONE, dtype=np.uint64), g, T, 1, 0, flags=R.POWER)
    b = S.sums_host(np.full(T // 64, R.NONE, dtype=np.uint64), g + T, T, 1, 0, flags=R.POWER)
    lo = lambda s: (int(s.words[9]), int(s.words[11]), int(s.words[12]))
    assert lo(a)[0] + lo(b)[0] >= 1 << 64 or lo(a)[1] + lo(b)[1] >= 1 << 64 or lo(a)[2] + lo(b)[2] >= 1 << 64
    assert not R.diff(a.merge(b), want)


def test_recip_carries_into_the_top_limb(S):
    want = R.ones_words(0, T)
    assert want[16] == 1  # the sum of 1/v over the odd v in [3, 32771) is above 4: recip passes 2^128
    assert not R.diff(S.sums_host(np.full(T // 64, R.NONE, dtype=np.uint64), 0, T), want)


# -- 4. patterns and the candidates above the range ----------------------------------------------
@pytest.mark.parametrize("require,forbid", PATTERNS)
def test_patterns_with_above_strings(S, require, forbid):
    rng = np.random.default_rng(0xAB0 + require)
    span = TR.span(require, forbid)
    for nbits in (5, 40, 64, 200, T + 70):
        for nab, shift in ((0, 0), (1, 63), (17, 50), (31, 40), (31, 0)):
            bits = rng.random(nbits) < 0.5
            above = rng.random(nab) < 0.5
            # matches planted across the word seams, the tile seam and the range's end
            for pos in (0, 63, 64 - span // 2, T - 1, T - span // 2, nbits - 1, nbits - span // 2):
                if 0 <= pos < nbits and pos + span <= nbits + nab:
                    TR.plant(bits, above, pos, require, forbid)
            for flags in (0, 1, 2, 3):
                want = R.brute(bits, 123, require, forbid, above, flags)
                got = host(S, bits, 123, require, forbid, above, shift, flags, rng)
                assert not R.diff(got, want), (nbits, nab, shift, flags)
                if not flags & R.POWER:
                    assert want[9:14] == [0] * 5 and R.words_of(got)[9:14] == [0] * 5
                if not flags & R.RECIP:
                    assert want[14:17] == [0] * 3 and R.words_of(got)[14:17] == [0] * 3
    assert R.brute(np.ones(20, bool), 0, *SPAN32)[6] == 0  # a range shorter than the span, nothing above
    assert not R.diff(host(S, np.ones(20, bool), 0, *SPAN32), R.brute(np.ones(20, bool), 0, *SPAN32))
    assert R.brute(np.ones(20, bool), 0, *SPAN32, above=np.ones(30, bool))[6] == 19
    assert host(S, np.ones(20, bool), 0, *SPAN32, above=np.ones(30, bool), shift=60).matches == 19


# -- 5. merge -------------------------------------------------------------------------------------
def pieces(S, bits, g, cuts, require, forbid, flags, tail=()):
    """The sums of bits[c0:c1], each seeing min(31, what is left) candidates above it."""
    vis = np.concatenate([bits, np.asarray(tail, bool)])
    out = []
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        ab = vis[c1:c1 + 31]
        out.append(host(S, bits[c0:c1], g + c0, require, forbid, ab, int(c1 % 64), flags))
    return out


def test_merge_equals_the_whole(S):
    rng = np.random.default_rng(0x3E46E)
    n = 3000
    for trial in range(300):
        require, forbid = PATTERNS[trial % len(PATTERNS)]
        flags = trial % 4
        bits = rng.random(n) < (0.5 if trial % 3 else 0.9)
        g = int(rng.choice([0, 11, 1 << 40]))
        tail = rng.random(31) < 0.5 if trial % 2 else np.zeros(0, bool)
        c = sorted(int(x) for x in rng.integers(0, n + 1, size=2))
        if trial % 10 == 0:
            c[1] = c[0]  # an empty piece in the middle
        if trial % 10 == 1:
            c[0] = 0     # an empty piece in front
        if trial % 10 == 2:
            c[1] = n     # an empty piece behind
        a, b, cc = pieces(S, bits, g, [0] + c + [n], require, forbid, flags, tail)
        whole = R.brute(bits, g, require, forbid, tail, flags)
        assert not R.diff(a.merge(b).merge(cc), whole), (trial, c)
        assert not R.diff(a.merge(b.merge(cc)), whole), (trial, c)


def test_merge_refusals(S):
    from mail_sieve_e import _dse
    rng = np.random.default_rng(5)
    bits = rng.random(400) < 0.5

    def refused(a, b, code=EINVAL):
        out = np.full(R.WORDS, 0x77, dtype=np.uint64)
        rc = _dse.lib().dse_sums_merge(_dse.u64p(a.words), _dse.u64p(b.words), _dse.u64p(out))
        assert rc == code and (out == 0x77).all()

    a, b = pieces(S, bits, 9, [0, 200, 400], 3, 0, 3)
    assert not R.diff(a.merge(b), R.brute(bits, 9, 3, 0, (), 3))
    refused(b, a)                                            # not adjacent
    refused(a, host(S, bits[201:], 9 + 201, 3, 0))           # a hole
    refused(a, pieces(S, bits, 9, [0, 200, 400], 3, 0, 1)[1])            # other flags
    refused(a, pieces(S, bits, 9, [0, 200, 400], 1, 0, 3)[1])            # other require
    refused(a, pieces(S, bits, 9, [0, 200, 400], 3, 4, 3)[1])            # other forbid
    blind = host(S, bits[:200], 9, 3, 0)                     # saw nothing above it
    refused(blind, b)
    short = host(S, bits[:200], 9, *SPAN32, above=bits[200:230], shift=3)  # 30 of the 31 it needs
    refused(short, host(S, bits[200:], 209, *SPAN32))
    one = host(S, bits[:200], 9, *SPAN32, above=bits[200:205], shift=3)    # b and its above are 5 in all: enough
    five = host(S, bits[200:203], 209, *SPAN32, above=bits[203:205], shift=11)
    assert not R.diff(one.merge(five), R.brute(bits[:203], 9, *SPAN32, above=bits[203:205]))
    # pattern 1 needs nothing across the seam
    assert not R.diff(host(S, bits[:200], 9).merge(host(S, bits[200:], 209)), R.brute(bits, 9))
    # a union that ends above 2^62: two results that each lie inside the bound but overlap it together
    top = host(S, bits[:64], R.TOP - 64)
    far = R.words_of(host(S, bits[:64], R.TOP - 64))
    far[0] = R.TOP
    refused(top, S.Sums(np.array(far, dtype=np.uint64)), ERANGE)


# -- 6. real primes -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def million():
    return R.odd_sieve(10 ** 6)


def test_primes_below_a_million(S, million):
    bits = million
    assert len(bits) == 499_999
    p = [3 + 2 * int(i) for i in np.flatnonzero(bits)]
    known = (78_497, 37_550_402_021, 24_693_298_341_834_529, 203_091_414_084_438_379_867_552_348_341_623_506_040)
    assert (len(p), sum(p), sum(x * x for x in p), sum(R.ONE // x for x in p)) == known
    s = host(S, bits, 0)
    assert (s.matches, s.sum1, s.sum2, s.recip) == known
    assert not R.diff(s, R.brute_values(p, 0, len(bits)))
    assert (s.first, s.last) == (3, 999_983)


def test_twins_below_a_million(S, million):
    bits = million
    s = host(S, bits, 0, 3, 0)
    pos = TR.positions(bits, np.zeros(0, bool), 3, 0)
    assert len(pos) == 8_169 == s.matches
    true = sum(Fraction(1, 3 + 2 * int(i)) + Fraction(1, 5 + 2 * int(i)) for i in pos)
    lo, hi = s.reciprocal_bounds()
    assert lo <= true <= hi and hi - lo == Fraction(2 * 8_169, R.ONE)
    assert abs(float(true) - 1.710776930804) < 1e-12 and abs(s.reciprocal - 1.710776930804) < 1e-12
    assert not R.diff(s, R.brute(bits, 0, 3, 0))


# -- 7. error codes -----------------------------------------------------------------------------
def test_error_codes(S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    m = np.zeros(4, dtype=np.uint64)
    out = np.zeros(R.WORDS, dtype=np.uint64)
    up, mp, op = _dse.u64p, _dse.u64p(m), _dse.u64p(out)

    def rc(mask=mp, g=0, nbits=100, require=1, forbid=0, above=None, shift=0, nab=0, flags=3, o=op):
        return L.dse_debug_sums_host(mask, g, nbits, require, forbid, above, shift, nab, flags, o)

    assert rc() == 0
    assert rc(o=None) == EINVAL
    assert rc(mask=None) == EINVAL and rc(mask=None, nbits=0) == 0
    assert rc(flags=4) == EINVAL and rc(flags=8 | 1) == EINVAL and rc(flags=0) == 0
    assert rc(require=2) == EINVAL and rc(require=0) == EINVAL
    assert rc(require=3, forbid=2) == EINVAL
    assert rc(nab=32, above=mp) == EINVAL and rc(nab=31, above=mp) == 0
    assert rc(shift=64, above=mp, nab=1) == EINVAL
    assert rc(nab=1, above=None) == EINVAL
    odd = np.zeros(3, dtype=np.uint64).view(np.uint8)[4:12]
    mis = odd.ctypes.data_as(type(mp))
    assert rc(nab=1, above=mis) == EINVAL
    assert rc(g=R.TOP + 1, nbits=0) == ERANGE and rc(g=R.TOP, nbits=0) == 0
    assert rc(g=R.TOP - 99) == ERANGE and rc(g=R.TOP - 100) == 0
    assert rc(g=R.TOP - 100, nab=1, above=mp) == ERANGE  # the visible candidates pass the bound
    assert rc(nbits=(1 << 44) + 1) == ERANGE
    assert L.dse_sums_merge(None, op, op) == EINVAL
    assert L.dse_debug_sums_recip(None, 1, op) == EINVAL and L.dse_debug_sums_recip(None, 0, None) == 0
    # the device entry points refuse a null context before anything else
    assert L.dse_sums_dev_async(None, 0, 0, None, 1, 0, None, 0, 0, 3, None, None) == EINVAL
    assert L.dse_sums_range(None, 0, 0, 1, 0, 3, op) == EINVAL
    assert L.dse_sums_resident(None, 0, 1, 0, 3, op) == EINVAL
