"""The largest bucketed passes the planner runs, bit for bit.

launch_bucketed cuts a range into passes of at most 8,192 segments
(kBucketMaxSegs) and halves a pass while its band-1 capacity passes 2^31
entries or its band-0 regions 24 GiB. With the production options a band-0
region has 1,296 slots from values of 2^56 on (976 at 1e13, 1,168 at 1e15),
so 4,854 segments is the most a pass gets there (6,445 at 1e13): a range of 8,192 + 131 segments at 1e18 runs as 4,096 + 4,227 (34
super-buckets, 21 GB of regions, 2.9e8 band-1 and 1.7e9 band-0 entries in
32-bit sums), sixteen times the largest pass any other test compares by mask.

A pass of 8,192 segments -- 64 super-buckets, 4,096 sort jobs, 32 KiB of
per-segment counters, segment indices up to 8,191 in every bucket kernel, and
a band-1 stage of 66,816 bytes of dynamic LDS, for which launch_bucketed calls
hipFuncSetAttribute(MaxDynamicSharedMemorySize): the opt-in runs for passes of
more than 7,936 segments and nowhere else -- runs only under test options that
keep band 0 narrow or away, so that its regions stay below 24 GiB, and where
the band-1 capacity fits. At 1e15 these are bucket_lo_log2 = 20 with
bucket_split_log2 = 20 (every bucketed prime in band 1: 1.9e9 entries in the
pass, nine tenths of what the kernels' 32-bit sums and addresses are allowed,
2^31), 21 (band 0 = (2^20, 2^21], regions of 688 slots, 21.5 GiB) or 22 (752
slots, 23.5 GiB): with 21 and 22 the band-0 fill walks its chunk groups over
8,192 segments, addresses regions of segments up to 8,191 and writes 8,192 x
1,024 region fills back. No production pass has more than 7,936 segments.

The bench window [1e18, 1e18 + 1e10] (one pass of 2,544 segments) is compared
here by mask, not by count alone.

The reference is tests/golden/max_pass.json (make_golden.py --maxpass: the
oracle's window sieve, oracle.mask_window): the primes of every segment, the
total, and a SHA-256 per 128 segments of mask. Every case sieves into a device
tensor (dse_sieve_range_dev_async on a table built once for the module),
counts per segment with torch arithmetic alone, copies the mask to the host
once for the hashes, and asserts the plan statistics (dse_debug_get_stat
"plan_*") against the planner's formulas restated in tests/max_pass_ref.py,
which holds the shared code, and against the literal figures. The range ending
at 2^62 - 1 is in tests/test_gpu_top_of_range.py, beside the table it needs.

The passes at 1e18 take 41 GiB of scratch (max_pass_ref.planned_passes); the
module owns its context and frees it at the end.
"""
import contextlib

import pytest

import max_pass_ref as R
from max_pass_ref import FIX, MAX_PASS, SEG

pytestmark = pytest.mark.gpu

PLAN = ("plan_bucket_passes", "plan_bucket_max_pass_segments", "plan_bucket_max_lds_bytes")


@pytest.fixture(scope="module")
def mctx():
    """This module's context: its scratch of tens of GB goes with it."""
    import torch
    from mail_sieve_e.sieve import Context
    c = Context(num_gpus=1)
    yield c
    c.close()
    torch.cuda.empty_cache()


def _table(c, limit):
    import torch
    from mail_sieve_e import sieve as S
    t = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    c.base_primes_dev_async(limit, t.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def table(mctx):
    """The base table both 1e18 fixtures need (primes to 1e9 and a little), built once."""
    import torch
    from mail_sieve_e import sieve as S
    limit = max(S.base_limit_for_range(FIX[n]["g0"], FIX[n]["nb"]) for n in ("window_1e18", "max_1e18"))
    assert 10**9 < limit < 10**9 + 100
    t = _table(mctx, limit)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def table15(mctx):
    """The base table of the 1e15 fixture (primes to 3.2e7)."""
    import torch
    from mail_sieve_e import sieve as S
    e = FIX["max_1e15"]
    t = _table(mctx, S.base_limit_for_range(e["g0"], e["nb"]))
    yield t
    del t
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _options(c, **opts):
    for k, v in opts.items():
        c.debug_set_option(k, v)
    try:
        yield c
    finally:
        for k in opts:
            c.debug_set_option(k, 0)


def _plan(c):
    return tuple(c.debug_get_stat(k) for k in PLAN)


def test_bench_window_mask(mctx, table):
    """[1e18, 1e18 + 1e10] with the production options: one pass of 2,544
    segments (20 super-buckets), below the LDS opt-in. Every segment's primes
    and every piece's hash, where test_window_1e18_full has the count."""
    e = FIX["window_1e18"]
    R.need_device_memory(e["g0"], e["nb"])
    mask, c = R.sieve_dev(mctx, table.data_ptr(), e["g0"], e["nb"])
    plan = _plan(mctx)
    assert plan == (1, 2544, R.stage_lds_bytes(2544)) and plan[2] <= R.LDS_OPT_IN, plan
    R.check_entry(mask, c, e, what="window [1e18, 1e18 + 1e10]")


def _planned(e, nb=None, **opts):
    """(passes, largest pass, largest LDS size) the planner's formulas give, and the passes' segments."""
    p = R.planned_passes(e["g0"], e["nb"] if nb is None else nb, **opts)
    return (len(p), max(x[0] for x in p), max(x[3] for x in p)), [x[0] for x in p]


def test_largest_production_passes(mctx, table):
    """8,192 + 131 segments from a ragged start at 1e18, production options.
    The planner halves the first 8,192 (their band-0 regions would take 40.5
    GiB, above its 24 GiB) and runs 4,096 + 4,227 segments: 35,496 bytes of
    LDS, below the opt-in. Then the same range over a scratch full of 0xFF
    bytes (two passes of different layouts over stale contents), and with
    bucket_pass_segments = 7936 (3,968 + 4,355, other cuts): both equal to the
    verified mask, word for word on the device."""
    import torch
    e = FIX["max_1e18"]
    g0, nb = e["g0"], e["nb"]
    R.need_device_memory(g0, nb, masks=2)
    plan, passes = _planned(e)
    assert plan == (2, 4227, 35_496) and passes == [4096, 4227] and plan[2] <= R.LDS_OPT_IN
    mask, c = R.sieve_dev(mctx, table.data_ptr(), g0, nb)
    assert _plan(mctx) == plan, _plan(mctx)
    R.check_entry(mask, c, e, passes=passes, what="8,192 + 131 segments at 1e18")
    with _options(mctx, scratch_poison=1):
        m2, c2 = R.sieve_dev(mctx, table.data_ptr(), g0, nb)
    assert _plan(mctx) == plan, _plan(mctx)
    assert c2 == c and torch.equal(m2, mask), "the result depends on stale scratch contents"
    del m2
    with _options(mctx, bucket_pass_segments=7936):
        m3, c3 = R.sieve_dev(mctx, table.data_ptr(), g0, nb)
    assert _plan(mctx) == _planned(e, pass_segs=7936)[0] == (2, 4355, 36_540), _plan(mctx)
    assert c3 == c and torch.equal(m3, mask), "other pass cuts give another mask"


def test_first_8192_segments_alone(mctx, table):
    """The first 8,192 segments of that range on their own, production options:
    two passes of 4,096, no ragged end, the last segment's last word full. The
    fixture's first 8,192 segment counts and first 64 piece hashes serve: a
    piece is 128 segments of 30,720 whole words, so no piece straddles the cut."""
    e = FIX["max_1e18"]
    nb = MAX_PASS * SEG
    assert nb % 64 == 0 and (128 * SEG) % 64 == 0 and MAX_PASS % 128 == 0
    R.need_device_memory(e["g0"], nb)
    plan, passes = _planned(e, nb=nb)
    assert plan == (2, 4096, 33_408) and passes == [4096, 4096]
    mask, c = R.sieve_dev(mctx, table.data_ptr(), e["g0"], nb)
    assert _plan(mctx) == plan, _plan(mctx)
    R.check_entry(mask, c, e, nb=nb, passes=passes, what="the first 8,192 segments at 1e18")


BAND1_ONLY = {"bucket_lo_log2": 20, "bucket_split_log2": 20}
_B1 = {"lo_log2": 20, "split_log2": 20}


def test_pass_of_8192_segments(mctx, table15):
    """8,192 + 131 segments from a ragged start at 1e15 with every bucketed
    prime (p > 2^20) in band 1: the first pass is the largest the planner has,
    1.9e9 entries (above 2^30, read from the fixture) in a capacity of 1.95e9,
    and it runs the dynamic-LDS opt-in: 66,816 bytes = 4 (64 + 4 * 64 * 65).
    Then over a scratch full of 0xFF bytes, and in passes of 7,936 segments,
    the largest below the opt-in (62 super-buckets, 64,728 bytes, then a
    ragged pass of 387): both equal to the verified mask."""
    import torch
    e = FIX["max_1e15"]
    g0, nb = e["g0"], e["nb"]
    assert (e["bucket_lo_log2"], e["bucket_split_log2"]) == (20, 20) and e["band0_entries"] == 0
    assert 2**30 < e["first_pass_band1_entries"] < R.planned_passes(g0, nb, **_B1)[0][2] <= R.MAX_ENTRIES
    R.need_device_memory(g0, nb, masks=2, **_B1)
    plan, passes = _planned(e, **_B1)
    assert plan == (2, MAX_PASS, 66_816) and passes == [MAX_PASS, 131] and plan[2] > R.LDS_OPT_IN
    with _options(mctx, **BAND1_ONLY):
        mask, c = R.sieve_dev(mctx, table15.data_ptr(), g0, nb)
        assert _plan(mctx) == (2, MAX_PASS, 4 * (64 + 4 * 64 * 65)), _plan(mctx)
        R.check_entry(mask, c, e, passes=passes, what="8,192 + 131 segments at 1e15, band 1 only")
        with _options(mctx, scratch_poison=1):
            m2, c2 = R.sieve_dev(mctx, table15.data_ptr(), g0, nb)
        assert _plan(mctx) == plan, _plan(mctx)
        assert c2 == c and torch.equal(m2, mask), "the result depends on stale scratch contents"
        del m2
        with _options(mctx, bucket_pass_segments=7936):
            m3, c3 = R.sieve_dev(mctx, table15.data_ptr(), g0, nb)
        assert _plan(mctx) == (2, 7936, 64_728) and 64_728 <= R.LDS_OPT_IN, _plan(mctx)
        assert c3 == c and torch.equal(m3, mask), "passes of 7,936 segments differ from passes of 8,192"


@pytest.mark.parametrize("split_log2", [21, 22])
def test_pass_of_8192_segments_both_bands(mctx, table15, split_log2):
    """The same range with bucket_lo_log2 = 20 and the split at 2^21 or 2^22:
    band-0 regions of 688 or 752 slots, 8,192 x 1,024 of them in 21.5 or 23.5
    GiB, below the planner's 24 GiB, so the first pass keeps its 8,192 segments
    with both bands: the one-level fill (bucket_fill_wg) over segment indices
    up to 8,191 beside the staged band 1 with the LDS opt-in. The mask does
    not depend on the split: the same fixture entry, segment by segment and
    piece by piece, and once more over a scratch full of 0xFF bytes."""
    import torch
    e = FIX["max_1e15"]
    g0, nb = e["g0"], e["nb"]
    opts = {"lo_log2": 20, "split_log2": split_log2}
    R.need_device_memory(g0, nb, masks=2, **opts)
    planned = R.planned_passes(g0, nb, **opts)
    plan, passes = _planned(e, **opts)
    assert plan == (2, MAX_PASS, 66_816) and passes == [MAX_PASS, 131]
    k0 = {21: 688, 22: 752}[split_log2]
    assert R._bucket_k0(R._I_LO[20], 2.0**20, 2.0**split_log2) == k0 and 4 * MAX_PASS * 1024 * k0 <= R.MAX_REGION_BYTES
    assert planned[0][1] > 4 * MAX_PASS * 1024 * k0   # the scratch holds the regions: band 0 is there
    with _options(mctx, bucket_lo_log2=20, bucket_split_log2=split_log2):
        mask, c = R.sieve_dev(mctx, table15.data_ptr(), g0, nb)
        assert _plan(mctx) == (2, MAX_PASS, 66_816), _plan(mctx)
        R.check_entry(mask, c, e, passes=passes, what=f"8,192 + 131 segments at 1e15, split 2^{split_log2}")
        with _options(mctx, scratch_poison=1):
            m2, c2 = R.sieve_dev(mctx, table15.data_ptr(), g0, nb)
        assert _plan(mctx) == (2, MAX_PASS, 66_816), _plan(mctx)
        assert c2 == c and torch.equal(m2, mask), "the result depends on stale scratch contents"


def test_pass_of_8192_segments_alone(mctx, table15):
    """The first 8,192 segments of the 1e15 range on their own: one pass with
    the opt-in, no ragged end, the last segment's last word full; the fixture's
    first 8,192 counts and first 64 piece hashes."""
    e = FIX["max_1e15"]
    nb = MAX_PASS * SEG
    R.need_device_memory(e["g0"], nb, **_B1)
    with _options(mctx, **BAND1_ONLY):
        mask, c = R.sieve_dev(mctx, table15.data_ptr(), e["g0"], nb)
        assert _plan(mctx) == (1, MAX_PASS, 66_816), _plan(mctx)
    R.check_entry(mask, c, e, nb=nb, passes=[MAX_PASS], what="one pass of 8,192 segments at 1e15")
