"""What the six result classes of mail_sieve_e.sieve share (Stats, Gaps, Consec, Sums,
Goldbach, Race: one base class) and Context's window arithmetic, on the CPU.

One table drives every class: a mask of three words with thirteen bits set, among
them a pair across bit 70, where it is split. The whole range's result by the unit's
*_host must equal the merge of the two halves' results, each half seeing what the
unit lets it see of the other: sums' lower half the candidates above it, Goldbach's
upper half those below it, the race's upper half the lower one's d_end.
"""
import numpy as np
import pytest

from mail_sieve_e import _dse
from mail_sieve_e import sieve as S

NBITS, CUT = 192, 70
SET = (0, 1, 5, 30, 63, 64, 69, 70, 72, 100, 128, 150, 191)
BITS = np.zeros(NBITS, dtype=np.uint8)
BITS[list(SET)] = 1
TWINS = 0b11


def pack(bits):
    """the bits as uint64 words, bit 0 of word 0 first"""
    padded = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


LOW, HIGH = pack(BITS[:CUT]), pack(BITS[CUT:])


def _race_high(g):
    d_end = S.race_host(LOW, g, CUT, 4, 1, 3).d_end
    return S.race_host(HIGH, g + CUT, NBITS - CUT, 4, 1, 3, d_start=d_end)


# class -> (g_start, words, host(mask, g, nbits), the lower half, the upper half)
CASES = {
    S.Stats: (1000, _dse.STATS_WORDS, lambda m, g, n: S.stats_host(m, g, n), None, None),
    S.Gaps: (1000, _dse.GAPS_WORDS, lambda m, g, n: S.gaps_host(m, g, n), None, None),
    S.Consec: (1000, _dse.CONSEC_WORDS, lambda m, g, n: S.consec_host(m, g, n, 10), None, None),
    S.Sums: (1000, _dse.SUMS_WORDS, lambda m, g, n: S.sums_host(m, g, n, require=TWINS),
             lambda g: S.sums_host(LOW, g, CUT, require=TWINS, above=HIGH, above_bits=31), None),
    S.Goldbach: (0, _dse.GOLDBACH_WORDS, lambda m, g, n: S.goldbach_host(m, g, n), None,
                 lambda g: S.goldbach_host(HIGH, g + CUT, NBITS - CUT, below=LOW, below_bits=CUT)),
    S.Race: (1000, _dse.RACE_WORDS, lambda m, g, n: S.race_host(m, g, n, 4, 1, 3), None, _race_high),
}
IDS = [c.__name__ for c in CASES]


@pytest.fixture(scope="module")
def wholes():
    return {cls: host(pack(BITS), g, NBITS) for cls, (g, _, host, _, _) in CASES.items()}


@pytest.mark.parametrize("cls", CASES, ids=IDS)
def test_whole_is_the_merge_of_its_halves(cls, wholes):
    g, _, host, low, high = CASES[cls]
    lo = low(g) if low else host(LOW, g, CUT)
    hi = high(g) if high else host(HIGH, g + CUT, NBITS - CUT)
    whole, merged = wholes[cls], lo.merge(hi)
    assert type(whole) is type(merged) is cls
    assert (whole.g_start, whole.nbits) == (g, NBITS) and (lo.nbits, hi.g_start) == (CUT, g + CUT)
    assert np.array_equal(whole.words, merged.words), np.flatnonzero(whole.words != merged.words)
    assert whole == merged and not whole != merged
    assert lo != whole and hi != whole


def test_the_pair_across_the_cut_is_seen(wholes):
    """The split is no trivial one: a twin pair, a gap and a consecutive pair span it."""
    assert BITS[CUT - 1] and BITS[CUT]
    whole = wholes[S.Sums]
    assert whole.matches == S.sums_host(LOW, 1000, CUT, require=TWINS).matches + \
        S.sums_host(HIGH, 1000 + CUT, NBITS - CUT, require=TWINS).matches + 1
    assert wholes[S.Stats].primes == wholes[S.Gaps].primes == wholes[S.Consec].primes == len(SET)


@pytest.mark.parametrize("cls", CASES, ids=IDS)
def test_a_wrong_length_is_refused(cls):
    words = CASES[cls][1]
    assert cls.WORDS == words
    for n in (0, words - 1, words + 1):
        with pytest.raises(ValueError, match=r"\b%d uint64 words" % words):
            cls(np.zeros(n, dtype=np.uint64))
    with pytest.raises(ValueError, match=r"\b%d uint64 words" % words):
        cls(np.zeros((1, words), dtype=np.uint64))
    assert cls(np.zeros(words, dtype=np.uint64)).words.shape == (words,)


@pytest.mark.parametrize("cls", CASES, ids=IDS)
def test_equal_only_to_its_own_class(cls, wholes):
    x = wholes[cls]
    assert x == cls(x.words.copy())
    for other, y in wholes.items():
        if other is not cls:
            assert x != y and not x == y
    assert not x == x.words and x != x.words
    assert x != None and x != 0  # noqa: E711
    with pytest.raises(TypeError):
        hash(x)


@pytest.mark.parametrize("cls", CASES, ids=IDS)
def test_repr_names_the_class(cls, wholes):
    assert repr(wholes[cls]).startswith(cls.__name__ + "(")


def test_merge_refuses_what_the_library_refuses(wholes):
    """merge goes through dse_<unit>_merge: a range that is not adjacent to itself is DSE_EINVAL."""
    for cls, x in wholes.items():
        with pytest.raises(_dse.DseError) as e:
            x.merge(x)
        assert e.value.code == -1 and "dse_%s_merge" % cls.UNIT in str(e.value), cls


def window_ref(lo, hi, base):
    """(g_start, nbits) of the values of base's parity in [max(lo, base), hi], by listing them"""
    vals = [v for v in range(max(lo, base), hi + 1) if (v - base) % 2 == 0]
    if vals:
        return (vals[0] - base) // 2, len(vals)
    a = max(lo, base)
    a += (a - base) % 2  # the first value of the window, had it one
    return min((a - base) // 2, 1 << 62), 0


@pytest.mark.parametrize("base", [3, 6])
def test_window_arithmetic(base):
    """Context's windows: odd values from 3 (every unit but Goldbach, whose evens start at 6).
    lo even and odd, below the base, hi even and odd, hi < lo: against a listing of the values."""
    for lo in range(-3, 16):
        for hi in range(-3, 20):
            assert S.Context._window(lo, hi, base) == window_ref(lo, hi, base), (lo, hi)


def test_window_documented_cases():
    W = S.Context._window
    assert W(3, 3) == (0, 1) and W(0, 3) == (0, 1) and W(-5, 4) == (0, 1)
    assert W(4, 9) == (1, 3) and W(5, 9) == (1, 3) and W(5, 10) == (1, 3)  # 5, 7, 9
    assert W(10, 10) == (4, 0) and W(9, 7) == (3, 0) and W(0, 2) == (0, 0) and W(100, 0) == (49, 0)
    assert W(1 << 70, 0) == (1 << 62, 0)  # the empty window's g_start stays in the library's range
    assert W((1 << 63) + 1, (1 << 63) + 5) == ((1 << 62) - 1, 3)
    # Goldbach's evens 6 + 2c
    assert W(0, 6, base=6) == (0, 1) and W(7, 12, base=6) == (1, 3) and W(6, 5, base=6) == (0, 0)
    assert W(13, 13, base=6) == (4, 0)
