"""Launches of more segments than the device has CUs, and bucketed passes of
more than one super-bucket, bit for bit.

The wheel kernel is persistent: a launch has min(segments, CUs) workgroups,
and workgroup b sieves launch segments b, b + grid, b + 2 grid, ... What a
workgroup carries from one of its segments to the next -- the mid primes'
residues (mid_x, mid_inc, x_seg and its two validity conditions), the next
segment's init issued straight after the expand, the unit counter's reset, the
per-range counters across a range change -- runs only in such launches. A
bucketed pass of more than 128 segments has several super-buckets in the
two-level fill and the sort.

Every case compares whole masks and counts with the CPU oracle
(oracle.fast_sieve_range), or with GOLDEN["rounds"] (make_golden.py --rounds)
where the oracle takes minutes, and asserts the plan statistics
(dse_debug_get_stat "plan_*", include/dse.h) it exists for: a shape that stops
producing later rounds, the full / half split or several super-buckets -- on
another CU count, or after a change of the split's cost constants -- fails
instead of passing for nothing. New shapes are then chosen; the assertions are
not relaxed.

G is the device's CU count (256 on an MI355X; the figures in brackets are for
it) and SEG the candidates of a full segment. Ranges start and end ragged (g0
no multiple of 15 or 64, nb = k SEG + 777) unless a case says otherwise.
"""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))

SEG = 1_966_080             # odd candidates per full segment (15 * 2^17); a half segment is SEG / 2
MAX_RANGES = 9              # ranges per wheel launch (kMaxRanges): longer lists go in batches
PLAN = ("plan_wheel_launches", "plan_full_segments", "plan_half_segments", "plan_max_rounds",
        "plan_bucket_passes", "plan_bucket_max_pass_segments")
G0_1E9 = 10**9 + 7
G0_7E10 = 7 * 10**10 + 7    # V / 30 >= 2^32: the L units' two-quotient path
G0_1E13 = (10**13 + 1 - 3) // 2 + 12345   # base primes to 3.16e6 = 2^21.6: bucketed
_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)


@pytest.fixture(scope="module")
def G():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def rctx():
    """This module's context: its resident masks and scratch go with it."""
    from mail_sieve_e.sieve import Context
    c = Context(num_gpus=1)
    yield c
    c.close()


@contextlib.contextmanager
def _options(c, **opts):
    for k, v in opts.items():
        c.debug_set_option(k, v)
    try:
        yield c
    finally:
        for k in opts:
            c.debug_set_option(k, 0)


_REF = {}


def _ref(oracle, g0, nb):
    """The oracle's (mask, count) of a range, computed once per module and read-only."""
    if (g0, nb) not in _REF:
        m, c = oracle.fast_sieve_range(g0, nb)
        m.setflags(write=False)
        _REF[g0, nb] = (m, int(c))
    return _REF[g0, nb]


def _ragged(g0):
    assert g0 % 15 and g0 % 64, g0
    return g0


def _plan(c):
    return {k: c.debug_get_stat(k) for k in PLAN}


def _assert_plan(c, **want):
    got = _plan(c)
    assert {k: got["plan_" + k] for k in want} == want, got


_PRIMES = []


def _least_factor(v):
    """Least prime factor of odd v < 1e14 by trial division (numpy primes to 1e7)."""
    if not _PRIMES:
        s = np.ones(5_000_001, dtype=bool)  # s[i]: 2i + 1
        s[0] = False
        for i in range(1, 1582):
            if s[i]:
                s[2 * i * (i + 1)::2 * i + 1] = False
        _PRIMES.append((2 * np.flatnonzero(s) + 1).astype(np.uint64))
    p = _PRIMES[0]
    hit = p[np.uint64(v) % p == 0]
    return int(hit[0]) if len(hit) else v


def first_difference(mask, ref, g0, G, seg0=0, seg_bits=SEG):
    """None when the masks agree; otherwise a line naming the first candidate
    on which they differ: its value, its segment (of seg_bits candidates)
    within the range and the round (launch segment seg0 + segment, divided by
    G) in which a workgroup reached it, which way the device is wrong, and for
    a composite below 1e14 its least prime factor: the class of the prime that
    was lost."""
    mask, ref = np.asarray(mask).view(np.uint64), np.asarray(ref).view(np.uint64)
    if mask.shape != ref.shape:
        return f"mask of {len(mask)} words, reference of {len(ref)}"
    x = mask ^ ref
    bad = np.flatnonzero(x)
    if not len(bad):
        return None
    w = int(bad[0])
    low = int(x[w])
    j = 64 * w + ((low & -low).bit_length() - 1)
    v = 3 + 2 * (g0 + j)
    seg = j // seg_bits
    left_set = bool(int(mask[w]) >> (j & 63) & 1)
    msg = (f"first of {int(_POP8[x.view(np.uint8)].sum(dtype=np.int64))} wrong bits: value {v} (candidate {j} of the "
           f"range from g0 = {g0}), segment {seg} of the range, launch segment {seg0 + seg}, "
           f"round {(seg0 + seg) // G} of G = {G}: ")
    if left_set:
        msg += "the device left a composite set"
        if v < 10**14:
            msg += f", least prime factor {_least_factor(v)}"
    else:
        msg += "the device cleared a prime"
    return msg


def _check(m, c, oracle, g0, nb, G, seg0=0, what="", keep=True, seg_bits=SEG):
    """The whole mask and the count against the oracle's (keep: cached for the module's other cases)."""
    m_ref, c_ref = _ref(oracle, g0, nb) if keep else oracle.fast_sieve_range(g0, nb)
    diff = first_difference(m, m_ref, g0, G, seg0, seg_bits)
    if diff:
        pytest.fail(f"{what}: {diff}", pytrace=False)
    assert int(c) == int(c_ref), (what, int(c), int(c_ref))


# ---- (a) the plain kernel, full geometry, later rounds ----------------------

def _start_below_2p40(nb):
    """A start whose range ends three segments below the value 2^40, the last
    magnitude without bucketed primes (base primes to 2^20: every L set live)."""
    g0 = (2**40 - 3) // 2 - 3 * SEG - nb
    while g0 % 15 == 0 or g0 % 64 == 0:
        g0 -= 1
    return g0


@pytest.mark.parametrize("start", ["0", "1e9", "7e10", "2p40"])
def test_full_geometry_second_round(rctx, oracle, G, start):
    """(a) One range of G + 3 full segments [259], wheel_geometry = 1: three
    workgroups sieve a second segment with carried residues. From 0 (not
    ragged at the start: the first segments lie below TB^2, where the carry is
    refused), from 1e9 + 7, from 7e10 + 7 (V / 30 >= 2^32) and ending three
    segments below 2^40."""
    nb = (G + 2) * SEG + 777
    g0 = {"0": 0, "1e9": _ragged(G0_1E9), "7e10": _ragged(G0_7E10), "2p40": _ragged(_start_below_2p40(nb))}[start]
    assert 3 + 2 * (g0 + nb - 1) < 2**40
    with _options(rctx, wheel_geometry=1):
        m, c = rctx.sieve_odd_range(g0, nb)
    _assert_plan(rctx, max_rounds=2, full_segments=G + 3, half_segments=0, wheel_launches=1, bucket_passes=0)
    _check(m, c, oracle, g0, nb, G, what=f"full geometry from {start}")


def test_full_geometry_third_round(rctx, oracle, G):
    """(a) 2 G + 5 full segments [517] from 1e9 + 7: five workgroups carry
    residues twice."""
    g0, nb = _ragged(G0_1E9), (2 * G + 4) * SEG + 777
    with _options(rctx, wheel_geometry=1):
        m, c = rctx.sieve_odd_range(g0, nb)
    _assert_plan(rctx, max_rounds=3, full_segments=2 * G + 5, half_segments=0, wheel_launches=1)
    _check(m, c, oracle, g0, nb, G, what="three rounds")


# ---- (b) the half geometry, later rounds --------------------------------------

@pytest.mark.parametrize("start", ["1e9", "7e10"])
def test_half_geometry_third_round(rctx, oracle, G, start):
    """(b) The ranges of (a) as 2 G + 5 half-size segments [517],
    wheel_geometry = 2: three rounds of the half kernel."""
    g0, nb = _ragged({"1e9": G0_1E9, "7e10": G0_7E10}[start]), (G + 2) * SEG + 777
    with _options(rctx, wheel_geometry=2):
        m, c = rctx.sieve_odd_range(g0, nb)
    _assert_plan(rctx, max_rounds=3, full_segments=0, half_segments=2 * G + 5, wheel_launches=1)
    _check(m, c, oracle, g0, nb, G, what=f"half geometry from {start}", seg_bits=SEG // 2)


# ---- (c) a table larger than the range needs ---------------------------------

def test_table_beyond_range_root_over_rounds(rctx, oracle, G):
    """(c) (a)'s range from 0 on a caller's table of the primes to 1,000,003
    (dse_sieve_range_dev_async): the bound on the large units (WheelRange::lcap)
    moves from piece to piece of the range while workgroups carry residues."""
    import torch
    from mail_sieve_e import sieve as S
    limit, nb = 1_000_003, (G + 2) * SEG + 777
    table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((nb + 63) // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    rctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
    with _options(rctx, wheel_geometry=1):
        rctx.sieve_range_dev_async(table.data_ptr(), 0, nb, mask.data_ptr(), cnt.data_ptr(), sp)
    torch.cuda.synchronize()
    rctx.device_status()
    _assert_plan(rctx, max_rounds=2, full_segments=G + 3, half_segments=0, wheel_launches=1)
    _check(mask.cpu().numpy().view(np.uint64), int(cnt.item()), oracle, 0, nb, G, what="table to 1,000,003")


# ---- (d), (e) pooled ranges ------------------------------------------------------

def _sieve_all_vs_oracle(c, oracle, G, cs, P, seg_of_chunk=None):
    """dse_sieve_all over P chunks of cs candidates and a dropped tail of P - 1:
    every chunk's mask and count and the tail's count against the oracle."""
    N = 2 * (P * cs + P - 1) + 1
    tail_g, tail_n = oracle.tail_range(N, P)
    assert (N - 1) // 2 // P == cs and (tail_g, tail_n) == (P * cs, P - 1)
    counts, pi_ref, pi_full = c.sieve_all(N, P)
    plan = _plan(c)
    for k in range(P):
        _check(c.copy_chunk_mask(N, P, k + 1), counts[k], oracle, k * cs, cs, G,
               seg0=seg_of_chunk(k) if seg_of_chunk else 0, what=f"chunk {k + 1} of {P}", keep=False)
    t_ref = oracle.fast_sieve_range(tail_g, tail_n, want_mask=False)[1] if tail_n else 0
    assert pi_full - pi_ref == t_ref
    assert pi_ref == 1 + sum(int(x) for x in counts)
    return plan


def test_pooled_two_chunks_cross_in_different_rounds(rctx, oracle, G):
    """(d) Two chunks of G + 24 full segments and the tail in one launch: a
    workgroup's carry is valid inside a chunk, the first 24 workgroups cross
    into chunk 2 in their third round, the others in their second."""
    ns = G + 24
    with _options(rctx, wheel_geometry=1):
        plan = _sieve_all_vs_oracle(rctx, oracle, G, (ns - 1) * SEG + 777, 2, lambda k: k * ns)
    assert (plan["plan_max_rounds"], plan["plan_full_segments"], plan["plan_half_segments"],
            plan["plan_wheel_launches"]) == (3, 2 * ns + 1, 0, 1), plan


def test_pooled_seven_chunks_change_range_every_round(rctx, oracle, G):
    """(d) Seven chunks of ceil(G / 3) + 5 full segments [91]: every workgroup
    is in another range each round, so no carry is valid (r1 != r0) and every
    per-range counter of a workgroup is used. Three rounds for G >= 54."""
    ns = -(-G // 3) + 5
    with _options(rctx, wheel_geometry=1):
        plan = _sieve_all_vs_oracle(rctx, oracle, G, (ns - 1) * SEG + 777, 7, lambda k: k * ns)
    assert (plan["plan_max_rounds"], plan["plan_full_segments"], plan["plan_half_segments"],
            plan["plan_wheel_launches"]) == (3, 7 * ns + 1, 0, 1), plan


def _split_case(rctx, oracle, G, ns, P):
    return _sieve_all_vs_oracle(rctx, oracle, G, ns * SEG - 12345, P)


def _batches(ranges):
    return -(-ranges // MAX_RANGES)


def test_split_one_range(rctx, oracle, G):
    """(e) The automatic split (wheel_geometry = 0) of one range of G + 5
    segments: G full, the other five as 10 half segments in a second launch."""
    plan = _split_case(rctx, oracle, G, G + 5, 1)
    assert (plan["plan_full_segments"], plan["plan_half_segments"], plan["plan_wheel_launches"]) == (G, 10, 2), plan


def test_split_on_a_range_boundary(rctx, oracle, G):
    """(e) Five chunks of G / 4 segments [5 x 64]: the cut after G segments is
    the boundary between chunks 4 and 5; the half list is chunk 5 and the tail."""
    assert G % 4 == 0
    plan = _split_case(rctx, oracle, G, G // 4, 5)
    assert (plan["plan_full_segments"], plan["plan_half_segments"], plan["plan_wheel_launches"]) == \
        (G, 2 * (G // 4) + 1, 2), plan


def test_split_inside_a_range_with_several_half_ranges(rctx, oracle, G):
    """(e) Seven chunks of G // 5 - 1 segments [7 x 50]: chunk 6 is cut [6 full,
    44 as half segments], chunk 7 and the tail are all half."""
    ns = G // 5 - 1
    assert 5 * ns < G < 6 * ns
    plan = _split_case(rctx, oracle, G, ns, 7)
    assert (plan["plan_full_segments"], plan["plan_half_segments"], plan["plan_wheel_launches"]) == \
        (G, 2 * (7 * ns - G) + 1, 2), plan


def test_split_lists_longer_than_a_launch(rctx, oracle, G):
    """(e) Chunks of 10 segments, as many as keep the half list within one
    round [38: 380 segments]: the full list is ceil(G / 10) ranges [26, in 3
    launches of at most 9], the half list the rest of the cut chunk, the
    chunks after it and the tail [14 ranges, 2 launches]."""
    P = (3 * G // 2 - 4) // 10
    assert G % 10, "the cut must fall inside a chunk"
    plan = _split_case(rctx, oracle, G, 10, P)
    launches = _batches(-(-G // 10)) + _batches(P - G // 10 + 1)
    assert launches >= 4
    assert (plan["plan_full_segments"], plan["plan_half_segments"], plan["plan_wheel_launches"]) == \
        (G, 2 * (10 * P - G) + 1, launches), plan


def test_split_declined(rctx, oracle, G):
    """(e) One range of G + G / 2 + 1 segments [385]: the segments past the
    first round would take two rounds of half segments, which is slower than a
    second round of full ones, so the whole range stays in the full geometry."""
    ns = G + G // 2 + 1
    plan = _split_case(rctx, oracle, G, ns, 1)
    assert (plan["plan_full_segments"], plan["plan_half_segments"], plan["plan_max_rounds"],
            plan["plan_wheel_launches"]) == (ns, 0, 2, 1), plan


# ---- (f), (g), (h) the bucketed kernel at 1e13, live oracle ------------------------

_ONE_PASS = {}


def _bucketed_1e13(rctx, oracle, G, **opts):
    """(f)'s range, G + 3 segments [259] from 1e13, with the options; checked
    against the oracle. -> mask"""
    g0, nb = _ragged(G0_1E13), (G + 2) * SEG + 777
    with _options(rctx, **opts):
        m, c = rctx.sieve_odd_range(g0, nb)
    plan = _plan(rctx)
    _check(m, c, oracle, g0, nb, G, what=f"1e13 {opts}")
    return m, plan


def test_bucketed_second_round(rctx, oracle, G):
    """(f) The bucketed instantiation with the production options over G + 3
    segments in one pass: three workgroups carry residues into a second
    segment, with bucket units in the claim queue and bk_start[s] per segment."""
    _, plan = _bucketed_1e13(rctx, oracle, G)
    assert (plan["plan_bucket_passes"], plan["plan_bucket_max_pass_segments"], plan["plan_max_rounds"],
            plan["plan_full_segments"], plan["plan_half_segments"]) == (1, G + 3, 2, 0, 0), plan


@pytest.mark.parametrize("opts", [{"bucket_split_log2": 20}, {"bucket_split_log2": 21}, {"bucket_split_log2": 63},
                                  {"bucket_lo_log2": 17}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_bucketed_pass_of_three_super_buckets(rctx, oracle, G, opts):
    """(g) The same pass [3 super-buckets of 128 segments] with every band
    arrangement: all of (2^20, sqrt V] through the two-level fill and the sort
    (split 20), a split inside (21), all one-level (63); and with the primes
    above 2^17 bucketed, so the last L set is truncated while residues carry."""
    m, plan = _bucketed_1e13(rctx, oracle, G, **opts)
    assert G + 3 > 128
    assert (plan["plan_bucket_passes"], plan["plan_bucket_max_pass_segments"], plan["plan_max_rounds"]) == \
        (1, G + 3, 2), plan
    if opts == {"bucket_split_log2": 20}:
        _ONE_PASS[20] = m


def test_bucketed_passes_cut_past_a_super_bucket(rctx, oracle, G):
    """(h) Passes of 130 segments, split 20 [130 + 129]: each pass has a second
    super-bucket of a few segments. Equal to the one-pass result of (g) and to
    the oracle."""
    if 20 not in _ONE_PASS:
        _ONE_PASS[20] = _bucketed_1e13(rctx, oracle, G, bucket_split_log2=20)[0]
    m, plan = _bucketed_1e13(rctx, oracle, G, bucket_split_log2=20, bucket_pass_segments=130)
    assert (plan["plan_bucket_passes"], plan["plan_bucket_max_pass_segments"]) == (-(-(G + 3) // 130), 130), plan
    assert np.array_equal(m, _ONE_PASS[20])


# ---- (i) the production band 1 (p > 2^28), fixtures --------------------------------

@pytest.mark.parametrize("pass_segments", [0, 130])
@pytest.mark.parametrize("name", ["1e16", "1e18"])
def test_band_one_over_super_buckets_and_rounds(rctx, G, name, pass_segments):
    """(i) 261 segments at 1e16 (base primes to 1e8: band 0 only in production)
    and at 1e18 (to 1e9: the production band 1, p > 2^28, over three
    super-buckets), in one pass -- a second round on any device of at most 260
    CUs -- and in passes of 130 [130 + 130 + 1]. Count, the mask's SHA-256 and
    the primes of every segment against GOLDEN["rounds"]."""
    g = GOLDEN["rounds"][name]
    g0, nb = g["g0"], g["nb"]
    assert nb == 260 * SEG + 777 and len(g["segment_counts"]) == 261
    with _options(rctx, bucket_pass_segments=pass_segments):
        m, c = rctx.sieve_odd_range(_ragged(g0), nb)
    plan = _plan(rctx)
    if pass_segments:
        assert (plan["plan_bucket_passes"], plan["plan_bucket_max_pass_segments"]) == (3, 130), plan
    else:
        assert plan["plan_bucket_passes"] == 1 and plan["plan_bucket_max_pass_segments"] == 261, plan
        assert plan["plan_max_rounds"] >= 2, plan  # G <= 260
    seg = np.add.reduceat(_POP8[m.view(np.uint8)], np.arange(0, nb, SEG) // 8, dtype=np.int64)
    bad = np.flatnonzero(seg != np.array(g["segment_counts"]))
    assert len(bad) == 0, (f"segment {int(bad[0])} (round {int(bad[0]) // G} of G = {G}, values from "
                           f"{3 + 2 * (g0 + int(bad[0]) * SEG)}): {int(seg[bad[0]])} primes, "
                           f"{g['segment_counts'][int(bad[0])]} expected; {len(bad)} segments differ")
    assert c == g["count"]
    assert hashlib.sha256(m.view(np.uint8).tobytes()).hexdigest() == g["mask_sha256"]
