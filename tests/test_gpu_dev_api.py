"""Contract of the *_dev_async entry points on caller-owned device memory
(include/dse.h): the path a one-process-per-GPU rank takes (mail_sieve_e.core,
GpuEngine), whose table, mask and count are torch tensors from a caching
allocator, i.e. used memory with live neighbours.

Every mask is sieved into the middle of a poisoned tensor (0xA5 bytes, then all
ones: the second shows an OR-only store, a skipped zero word and unmasked bits
past nbits) whose words in front and behind must survive; every count sits
between poisoned neighbours; every table is built into 0x00-, 0xA5- and
0xFF-filled memory with a guard behind. The reference for every mask and count
is the oracle's CPU sieve (fast_sieve_range), for a table's primes a numpy
sieve; every comparison is exact.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A5 = 0xA5A5A5A5A5A5A5A5
ONES = 0xFFFFFFFFFFFFFFFF
POISONS = (A5, ONES)
EINVAL, ERANGE = -1, -6
SEG = 1966080          # candidates of a full segment (15 * 2^17); a half segment is 983040
GUARD = 512            # words behind (and the least in front of) every mask


def i64(x):
    """A uint64 bit pattern as the int64 torch stores."""
    return x - (1 << 64) if x >> 63 else x


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def geo(S):
    """One context per wheel_geometry (0: production split, 1: full segments only, 2: half only)."""
    cs = {}
    for g in (0, 1, 2):
        cs[g] = S.Context(num_gpus=1)
        cs[g].debug_set_option("wheel_geometry", g)
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's (mask, count) of a range, computed once per module."""
    seen = {}

    def get(g_start, nbits):
        if (g_start, nbits) not in seen:
            seen[g_start, nbits] = oracle.fast_sieve_range(g_start, nbits)
        return seen[g_start, nbits]
    return get


@functools.lru_cache(maxsize=None)
def _odd_primes_upto(n):
    if n < 3:
        return np.zeros(0, dtype=np.int64)
    s = np.ones(n + 1, dtype=bool)
    s[:2] = False
    s[4::2] = False
    for i in range(3, int(n ** 0.5) + 1, 2):
        if s[i]:
            s[i * i::2 * i] = False
    p = np.nonzero(s)[0]
    return p[p > 2]


def build_table(torch, S, ctx, limit, fill=0xA5, guard=4096):
    """A base table for `limit` built into `fill`-filled bytes with a guard behind:
    nothing behind dse_base_table_bytes is written, the header is {count, cap, limit}
    and p[0..count) equals a host sieve. -> (tensor, count)"""
    tbytes = S.base_table_bytes(limit)
    t = torch.full((tbytes + guard,), fill, dtype=torch.uint8, device="cuda")
    ctx.base_primes_dev_async(limit, t.data_ptr(), tbytes, 0)
    torch.cuda.synchronize()
    assert bool((t[tbytes:] == fill).all()), ("table build wrote past dse_base_table_bytes", limit, fill)
    want = _odd_primes_upto(limit)
    hdr = t[:16].cpu().numpy()
    count, cap = (int(x) for x in hdr[:8].view(np.uint32))
    assert count == len(want) <= cap and 16 + 4 * cap == S.base_table_prime_bytes(limit), (limit, fill, count, cap)
    assert int(hdr[8:16].view(np.uint64)[0]) == limit
    p = t[16:16 + 4 * count].cpu().numpy().view(np.uint32)
    assert np.array_equal(p.astype(np.int64), want), ("p[0..count) differs from a host sieve", limit, fill)
    return t, count


@pytest.fixture(scope="module")
def table_1e9(torch, S, geo):
    """Covers every plain-path range of this file (values up to 2e9 + 2e7)."""
    return build_table(torch, S, geo[0], S.base_limit_for_range(10**9 + 11, 4 * SEG))[0]


def guarded_sieve(torch, c, table, g_start, nbits, poison, lead=3, guard=GUARD, preset=0):
    """dse_sieve_range_dev_async into a poison-filled int64 tensor at element offset
    `lead` (8-byte aligned only) with `guard` words behind, the count into the middle
    of [poison, preset, poison]: -> (the ceil(nbits/64) mask words, what the count
    grew by). Every word in front of and behind the mask and both neighbours of the
    count must still hold the poison."""
    words = (nbits + 63) // 64
    buf = torch.full((lead + words + guard,), i64(poison), dtype=torch.int64, device="cuda")
    cnt = torch.tensor([i64(poison), preset, i64(poison)], dtype=torch.int64, device="cuda")
    c.sieve_range_dev_async(table.data_ptr(), g_start, nbits, buf.data_ptr() + 8 * lead, cnt.data_ptr() + 8, 0)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    where = (g_start, nbits, hex(poison), lead)
    front, behind = np.flatnonzero(h[:lead] != poison), np.flatnonzero(h[lead + words:] != poison)
    assert front.size == 0, ("wrote in front of mask_dev, word", int(front[0]) - lead, where)
    assert behind.size == 0, ("wrote behind mask_dev + ceil(nbits/64), word", words + int(behind[0]), where)
    k = [int(x) for x in cnt.cpu()]
    assert k[0] == k[2] == i64(poison), ("wrote beside *count_dev", k, where)
    return h[lead:lead + words], k[1] - preset


def check_range(torch, c, table, ref, g_start, nbits, poison, lead=3, preset=0, tag=None):
    """The four assertions of a mask case: guards (guarded_sieve), mask, tail bits, count."""
    m_ref, c_ref = ref(g_start, nbits)
    m, cnt = guarded_sieve(torch, c, table, g_start, nbits, poison, lead=lead, preset=preset)
    where = (tag, g_start, nbits, hex(poison), lead)
    if nbits % 64:
        assert int(m[-1]) >> (nbits % 64) == 0, ("bits past nbits in the last word", hex(int(m[-1])), where)
    bad = np.flatnonzero(m != m_ref)
    assert bad.size == 0, ("mask differs from the oracle: words", bad[:8].tolist(), "of", len(m), where)
    assert cnt == c_ref, ("count", cnt, c_ref, where)


# -- 1. masks, plain path ---------------------------------------------------------
# partial 32- and 64-bit words, the 480-bit block, the half and the full segment each +-1,
# a range the half/full split cuts, three segments and a ragged end
NBITS = [1, 31, 32, 33, 63, 64, 65, 479, 480, 481, SEG // 2 - 1, SEG // 2, SEG // 2 + 1, SEG - 1, SEG, SEG + 1,
         SEG + SEG // 2 + 1, 3 * SEG + 17]
G_STARTS = [0, 7, 10**9 + 11]   # the small-prime fix-up word at index 0, inside it, and none
LEADS = [0, 1, 3]


@pytest.mark.parametrize("i", range(len(NBITS)), ids=[str(n) for n in NBITS])
def test_mask_in_poisoned_memory(torch, geo, ref, table_1e9, i):
    """Every nbits with every geometry and both poisons (6 launches); g_start and lead
    rotate so that each nbits meets all three g_start and all three leads."""
    nbits = NBITS[i]
    for g in (0, 1, 2):
        for pi, poison in enumerate(POISONS):
            check_range(torch, geo[g], table_1e9, ref, G_STARTS[(i + g) % 3], nbits, poison,
                        lead=LEADS[(i + 2 * g + pi) % 3], tag=("geometry", g))


# -- 2. masks, bucketed path -------------------------------------------------------
@pytest.mark.parametrize("pass_segments", [0, 2])
def test_mask_bucketed_in_poisoned_memory(torch, S, ref, pass_segments):
    """A 1e13 range (base primes to 3.16e6, those above 2^19 bucketed) of four
    segments, in one pass and in passes of two, so a pass seam (launch_bucketed's
    out + s0 * words-per-segment) falls inside the guarded buffer."""
    g_start, nbits = (10**13 - 2) // 2, 3 * SEG + 777
    with S.Context(num_gpus=1) as c:
        c.debug_set_option("bucket_pass_segments", pass_segments)
        table, _ = build_table(torch, S, c, S.base_limit_for_range(g_start, nbits))
        for poison, lead in zip(POISONS, (1, 3)):
            check_range(torch, c, table, ref, g_start, nbits, poison, lead=lead, tag=("passes", pass_segments))
        c.device_status()


# -- 3. counts ----------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISONS, ids=["a5", "ones"])
def test_count_is_incremented_beside_live_neighbours(torch, S, geo, ref, table_1e9, poison):
    """*count_dev is INCREMENTED: element 1 of [poison, 1000, poison, poison] (core.py's
    counts.data_ptr() + 8 * slot) takes a masked call and a count-only call of another
    range and ends at 1000 + c1 + c2; then the count-only call of the first range and
    the masked call of the second add what their twins added. A third range goes
    through the bucketed pass, count-only, into the same slot."""
    c = geo[0]
    a, b = (7, SEG + SEG // 2 + 1), (10**9 + 11, 481)
    ca, cb = ref(*a)[1], ref(*b)[1]
    cnt = torch.tensor([i64(poison), 1000, i64(poison), i64(poison)], dtype=torch.int64, device="cuda")
    mask = torch.empty((a[1] + 63) // 64 + GUARD, dtype=torch.int64, device="cuda")

    def call(rng, with_mask, table=table_1e9):
        before = int(cnt[1].item())
        c.sieve_range_dev_async(table.data_ptr(), rng[0], rng[1], mask.data_ptr() if with_mask else 0,
                                cnt.data_ptr() + 8, 0)
        torch.cuda.synchronize()
        k = [int(x) for x in cnt.cpu()]
        assert k[0] == k[2] == k[3] == i64(poison), (k, rng, with_mask)
        return k[1] - before

    assert call(a, True) == ca
    assert call(b, False) == cb
    assert int(cnt[1].item()) == 1000 + ca + cb
    assert call(a, False) == ca
    assert call(b, True) == cb
    assert int(cnt[1].item()) == 1000 + 2 * (ca + cb)
    big = ((10**13 - 2) // 2, SEG + 777)
    t13, _ = build_table(torch, S, c, S.base_limit_for_range(*big))
    assert call(big, False, t13) == ref(*big)[1]
    assert int(cnt[1].item()) == 1000 + 2 * (ca + cb) + ref(*big)[1]
    c.device_status()


# -- 4. nothing to do, and refusals ---------------------------------------------------
@pytest.mark.parametrize("g_start", [0, 7, 10**9 + 11, 2**62])
def test_nbits_zero_launches_nothing(torch, ctx, table_1e9, g_start):
    """nbits = 0: DSE_OK, and neither the mask (no word of it exists) nor the count is written."""
    from mail_sieve_e import _dse
    buf = torch.full((GUARD,), i64(A5), dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), i64(A5), dtype=torch.int64, device="cuda")
    rc = _dse.lib().dse_sieve_range_dev_async(ctx.ptr, table_1e9.data_ptr(), g_start, 0, buf.data_ptr() + 8,
                                              cnt.data_ptr() + 8, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf == i64(A5)).all()) and bool((cnt == i64(A5)).all())


@pytest.mark.parametrize("g_start,nbits", [(2**62 - 10, 11), (2**62, 1), (2**62 + 1, 0), (0, 2**62 + 1),
                                           (2**64 - 1, 2)])
def test_range_beyond_2_62_is_refused(torch, ctx, table_1e9, g_start, nbits):
    """g_start + nbits > 2^62 (also where the sum wraps): DSE_ERANGE before any launch."""
    from mail_sieve_e import _dse
    buf = torch.full((GUARD,), i64(A5), dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), i64(A5), dtype=torch.int64, device="cuda")
    with pytest.raises(_dse.DseError) as e:
        ctx.sieve_range_dev_async(table_1e9.data_ptr(), g_start, nbits, buf.data_ptr() + 8, cnt.data_ptr() + 8, 0)
    torch.cuda.synchronize()
    assert e.value.code == ERANGE
    assert bool((buf == i64(A5)).all()) and bool((cnt == i64(A5)).all())


# -- 5. tables in poisoned memory ------------------------------------------------------
def table_ranges(limit):
    """(g_start, nbits, wheel_geometry) to sieve with a table of the odd primes <= limit:
    2,004,321 candidates ending 8,642 above limit^2, start clipped at 0. A table serves
    values below (limit + 1)^2 only (its primes must reach the root of the range's
    largest value), so for the limits 3 and 97, whose whole domain is 7 and 4,801
    candidates, the end is clipped there too."""
    g = max(limit * limit // 2 - 2_000_000, 0)
    covered = ((limit + 1) ** 2 - 4) // 2 + 1      # odd indices whose value is below (limit + 1)^2
    out = [(g, min(2_000_000 + 4321, covered - g), 0)]
    if limit == 1_000_003:
        out += [(10**9 + 7, 2 * SEG + 5, 0), (10**9 + 7, 2 * SEG + 5, 2)]
    return out


@pytest.mark.parametrize("limit", [3, 97, 1_000_003, 2_457_601, 2_457_603])
def test_table_in_poisoned_memory(torch, S, geo, ref, limit):
    """The one-level build (up to 2,457,601) and the first two-level build into 0x00,
    0xA5 and 0xFF bytes: nothing behind dse_base_table_bytes is written (build_table),
    the header and p[0..count) do not depend on the fill and equal a host sieve, and
    each table sieves like the oracle, whatever its unwritten slots hold (p[count..cap),
    the M / A / PL entries past the last prime, the last partial set of 64 of the L
    list). The ranges of 2,457,601 and 2,457,603 go through the bucketed pass. Then the
    broadcast route into 0xFF bytes: only dse_base_table_prime_bytes arrive, the rest
    is completed in place."""
    import math
    tbytes, pbytes = S.base_table_bytes(limit), S.base_table_prime_bytes(limit)
    ranges = table_ranges(limit)
    g_start, nbits, _ = ranges[0]
    assert nbits >= 1 and math.isqrt(3 + 2 * (g_start + nbits - 1)) == limit   # needs the table's last prime
    built = {fill: build_table(torch, S, geo[0], limit, fill) for fill in (0x00, 0xA5, 0xFF)}
    tables = {fill: t for fill, (t, _) in built.items()}
    count = built[0x00][1]
    heads = [t[:16 + 4 * count].cpu() for t in tables.values()]
    assert torch.equal(heads[0], heads[1]) and torch.equal(heads[0], heads[2])
    for i, (fill, t) in enumerate(tables.items()):
        for g_start, nbits, g in ranges:
            check_range(torch, geo[g], t, ref, g_start, nbits, POISONS[i % 2], lead=LEADS[i], tag=("fill", fill))
    # the broadcast route: the prime bytes of the 0xFF table (its p[count..cap) still 0xFF) into 0xFF bytes
    src = tables[0xFF]
    part = torch.full((tbytes + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    part[:pbytes] = src[:pbytes]
    geo[0].base_table_finish_dev_async(limit, part.data_ptr(), tbytes, 0)
    torch.cuda.synchronize()
    assert torch.equal(part[:pbytes], src[:pbytes]), "base_table_finish changed the prime bytes"
    assert bool((part[tbytes:] == 0xFF).all()), "base_table_finish wrote past dse_base_table_bytes"
    for g_start, nbits, g in ranges:
        check_range(torch, geo[g], part, ref, g_start, nbits, ONES, lead=1, tag="broadcast route")
    geo[0].device_status()


@pytest.mark.parametrize("limit", [3, 1_000_003, 2_457_603])
def test_table_buffer_one_byte_short_is_refused(torch, S, ctx, limit):
    from mail_sieve_e import _dse
    tbytes = S.base_table_bytes(limit)
    t = torch.full((tbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    for call in (ctx.base_primes_dev_async, ctx.base_table_finish_dev_async):
        with pytest.raises(_dse.DseError) as e:
            call(limit, t.data_ptr(), tbytes - 1, 0)
        assert e.value.code == EINVAL
    torch.cuda.synchronize()
    assert bool((t == 0xA5).all())
