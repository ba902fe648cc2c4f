"""tests/sparse_ref.py against the dense references, on the CPU: the references from
positions against numpy brute force on bool arrays (stats_ref and its siblings) over
stats_ref's sizes, fills and range starts; the all-ones closed forms against the same
brute force for every n from 1 to 200 and around the tile size; the finish formatter
against the host writer (dse_write_range_file, which test_abi.py pins to the reference's
files) at test_gpu_finish.py's sizes and flags and for first_rank 0 to 9.

test_gpu_large_masks.py relies on sparse_ref where bool arrays no longer fit.
"""
import numpy as np
import pytest

import consec_ref as CR
import gaps_ref as GR
import goldbach_ref as GB
import query_ref as QR
import race_ref as RR
import sparse_ref as X
import stats_ref as SR
import sums_ref as UR
import tuples_ref as TR

T = 256 * 64
QS = (3, 4, 10, 64)
RACES = ((4, 1, 3, 0), (3, 1, 2, -1), (3, 2, 0, 5), (10, 9, 1, -70), (8, 3, 3, 0), (64, 1, 63, 2**40), (12, 5, 2, 0))
PATTERNS = [TR.TWINS, (1 | 1 << 31, 0), TR.exact_gap_ref(3), TR.exact_gap_ref(31), (1, 0xFFFFFFFE)]


def same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64))


# -- 1. from positions --------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", SR.sizes(T))
def test_positions_against_dense(nbits):
    for name, bits in SR.masks(nbits, T, 4000 + nbits).items():
        pos = np.flatnonzero(bits).astype(np.uint64)
        rank = GB.ranks(bits)
        for g in SR.g_starts(nbits, T):
            at = (name, g)
            for pats in SR.PATTERN_LISTS:
                assert not SR.diff(X.stats(pos, g, nbits, pats), SR.brute(bits, g, pats)), at
            assert not GR.diff(X.gaps(pos, g, nbits), GR.brute(bits, g)), at
            for q in QS:
                assert not CR.diff(X.consec(pos, g, nbits, q), CR.brute(bits, g, q)), at + (q,)
            for q, a, b, d in RACES:
                assert not RR.diff(X.race(pos, g, nbits, q, a, b, d), RR.brute(bits, g, q, a, b, d)), at + (q, a, b, d)
            for np_ in (1, 64, 0):
                assert not GB.diff(X.goldbach(pos, g, nbits, np_), GB.struct(rank, g, np_)), at + (np_,)
            assert same(X.values(pos, g), QR.values(bits, g)), at
            for req, forb in PATTERNS:
                assert same(X.tuples(pos, g, nbits, req, forb), TR.values(bits, (), req, forb, g)), at + (req, forb)
            for kind in QR.KINDS:
                qs = QR.queries(bits, g, kind, every_word_seam=nbits <= T)
                assert same(X.query(pos, g, kind, qs), QR.expect(QR.values(bits, g), kind, qs)), at + (kind,)
        # the sums' Python ints are the slow part: one high and one low start
        for g in (0, 2**61 - 1 - nbits):
            for (req, forb), flags in (((1, 0), UR.POWER | UR.RECIP), ((1, 0), UR.POWER), ((1, 0), UR.RECIP), ((1, 0), 0),
                                       (TR.TWINS, UR.POWER | UR.RECIP), (TR.TWINS, UR.RECIP)):
                assert not UR.diff(X.sums(pos, g, nbits, req, forb, flags), UR.brute(bits, g, req, forb, (), flags)), \
                    (name, g, req, flags)


# -- 2. all ones ------------------------------------------------------------------------------------
ONES_SIZES = list(range(1, 201)) + [T - 1, T, T + 1, 2 * T + 37]


@pytest.mark.parametrize("start", ["0", "odd", "top"])
def test_ones_against_dense(start):
    for n in ONES_SIZES:
        g = {"0": 0, "odd": 2**31 + 12345, "top": 2**61 - 1 - n}[start]
        bits = np.ones(n, bool)
        for pats in SR.PATTERN_LISTS + ((1, 0b11),):
            assert not SR.diff(X.ones_stats(g, n, pats), SR.brute(bits, g, pats)), (n, g, pats)
        assert not GR.diff(X.ones_gaps(g, n), GR.brute(bits, g)), (n, g)
        for q in QS + (5, 7, 12, 63):
            assert not CR.diff(X.ones_consec(g, n, q), CR.brute(bits, g, q)), (n, g, q)
        for q, a, b, d in RACES + ((4, 3, 1, -3), (4, 1, 2, -100), (4, 2, 3, 150), (7, 0, 3, 0)):
            assert not RR.diff(X.ones_race(g, n, q, a, b, d), RR.brute(bits, g, q, a, b, d)), (n, g, q, a, b, d)
        for flags in (UR.POWER, 0):
            assert not UR.diff(X.ones_sums(g, n, flags), UR.brute(bits, g, 1, 0, (), flags)), (n, g, flags)
        for np_ in (1, 64, 0):
            assert not GB.diff(X.ones_goldbach(g, n, np_), GB.brute(bits, g, np_)), (n, g, np_)
        for kind in QR.KINDS:
            qs = QR.queries(bits, g, kind, every_word_seam=n <= 200)
            assert same(X.ones_query(g, n, kind, qs), QR.expect(QR.values(bits, g), kind, qs)), (n, g, kind)
        assert same(X.ones_values(g, 0, n), QR.values(bits, g))
        assert same(X.ones_values(g, n // 3, n - n // 3), QR.values(bits, g)[n // 3:])


# -- 3. the finish formatter ------------------------------------------------------------------------
def host_file(tmp_path, my_num, g_start, nbits, bits):
    from mail_sieve_e import _dse
    p = tmp_path / "host.txt"
    mask = np.ascontiguousarray(SR.pack(bits), dtype=np.uint64)
    _dse.check(_dse.lib().dse_write_range_file(str(p).encode(), my_num, g_start, nbits, _dse.u64p(mask)), "host writer")
    return p.read_bytes()


def finish_masks(nbits, seed):
    rng = np.random.default_rng(seed)
    first, last = np.zeros(nbits, bool), np.zeros(nbits, bool)
    first[0] = last[-1] = True
    return {"zero": np.zeros(nbits, bool), "ones": np.ones(nbits, bool), "first": first, "last": last,
            "half": rng.random(nbits) < 0.5, "sixteenth": rng.random(nbits) < 1 / 16}


FINISH_NBITS = [1, 4, 5, 63, 64, 65, 640, 2**20 + 37]
FINISH_POINTS = [10, 10**2, 10**5, 10**7, 10**10, 10**15, 10**16, 2**53, 2**62]


@pytest.mark.parametrize("nbits", FINISH_NBITS)
def test_finish_text_against_the_host_writer(tmp_path, nbits):
    for point in FINISH_POINTS:
        if point == 2**53:
            g0 = min((2**53 - 2**12 - 3) // 2 + 1, (2**53 - 3) // 2 - nbits)
        elif point == 2**62:
            g0 = 2**62 - 2**21
        else:
            g0 = max(0, (point - 3) // 2 - nbits // 2)
        for name, bits in finish_masks(nbits, 1000 + nbits).items():
            if nbits > 2**20 and (name in ("ones", "half") or point not in (10, 10**7, 2**53, 2**62)):
                continue  # the large size: the sparse fills, at the points where the printing changes
            pos = np.flatnonzero(bits)
            # Longs, as chunk my_num = 2
            assert X.finish_text(pos, g0, nbits, 0, X.LAST) == (host_file(tmp_path, 2, g0, nbits, bits), len(pos)), \
                (point, name)
            # Doubles: chunk 1's file of the range moved down by its four ignored bits prints 2 3 5 7 first
            g = max(g0, 4)
            if 3 + 2 * (g + nbits - 1) < 2**53:
                t = host_file(tmp_path, 1, g - 4, nbits + 4, np.concatenate([np.zeros(4, bool), bits]))
                assert t[:18] == b"2.0, 3.0, 5.0, 7.0"
                assert X.finish_text(pos, g, nbits, 4, X.DOUBLES | X.LAST) == (t[18:], len(pos)), (point, name)
    if nbits >= 4:  # the hack, both printings
        bits = np.random.default_rng(nbits).random(nbits) < 0.5
        pos = np.flatnonzero(bits)
        n = int(bits[4:].sum()) + 4
        assert X.finish_text(pos, 0, nbits, 0, X.DOUBLES | X.HACK | X.LAST) == (host_file(tmp_path, 1, 0, nbits, bits), n)
        b = bits.copy()
        b[:4] = True
        assert X.finish_text(pos, 0, nbits, 0, X.HACK | X.LAST) == (b"2, 3, 5, 7" + host_file(tmp_path, 2, 0, nbits, b)[10:], n)


@pytest.mark.parametrize("g,nbits,p", [(1000, 640, 0.3), (10**9, 1025 * 16384 + 37, 1 / 1000)])
def test_finish_text_first_rank_0_to_9(tmp_path, g, nbits, p):
    """first_rank r: r entries printed in front by the host writer, then cut off."""
    bits = np.random.default_rng(5).random(nbits) < p
    bits[0] = bits[-1] = True
    pos = np.flatnonzero(bits)
    for r in range(10):
        full = host_file(tmp_path, 2, g - r, nbits + r, np.concatenate([np.ones(r, bool), bits]))
        prefix = host_file(tmp_path, 2, g - r, r, np.ones(r, bool)) if r else b""
        skip = len(prefix) - 1 if r else 0  # the prefix's entries without its closing "\n"
        assert full[:skip] == prefix[:skip]
        for flags in (X.LAST, 0):
            want = full[skip:] if flags or (r + len(pos)) % 10 == 0 else full[skip:-1]
            assert X.finish_text(pos, g, nbits, r, flags) == (want, len(pos)), (r, flags)
