"""finish on the device (csrc/dse_finish.hip): the text of primes{k}.txt formatted
from a device-resident mask, against the product's own host writer
(dse_write_range_file / dse_write_primes_file, pinned to the reference's files
by tests/test_abi.py) on the same mask, or against the golden file hashes.
Every comparison is of exact bytes.

The host writer knows two flag sets only: my_num == 1 (DOUBLES|HACK) and
my_num >= 2 (neither). The other two are still compared against its output:
  DOUBLES alone: the host file of my_num = 1 for the range moved down by four
      candidates (its four ignored bits), which is "2.0, 3.0, 5.0, 7.0"
      followed by exactly what the device prints with first_rank = 4;
  HACK alone: the host file of my_num = 2 at g_start = 0 with bits 0..3 set
      prints "3, 5, 7, 9" where the hack prints "2, 3, 5, 7" (ten bytes each).
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))
DOUBLES, HACK, LAST = 1, 2, 4


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pack(bits):
    """bool array -> uint64 mask words (zero past the end)."""
    by = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    out = np.zeros((len(bits) + 63) // 64 * 8, dtype=np.uint8)
    out[:len(by)] = by
    return out.view(np.uint64)


def host_file(tmp_path, my_num, g_start, nbits, mask):
    from mail_sieve_e import _dse
    p = tmp_path / "host.txt"
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    _dse.check(_dse.lib().dse_write_range_file(str(p).encode(), my_num, g_start, nbits, _dse.u64p(mask)), "host writer")
    return p.read_bytes()


def host_text(tmp_path, flags, g_start, nbits, bits):
    """What the device must print for these bits with DSE_FINISH_LAST (first_rank 0,
    or 4 for DOUBLES alone), from the host writer; -> (text, entries, first_rank)."""
    bits = np.asarray(bits, dtype=bool)
    if flags & HACK:
        assert g_start == 0 and nbits >= 4
        n = int(bits[4:].sum()) + 4
        if flags & DOUBLES:
            return host_file(tmp_path, 1, 0, nbits, pack(bits)), n, 0
        b = bits.copy()
        b[:4] = True
        t = host_file(tmp_path, 2, 0, nbits, pack(b))
        assert t[:10] == b"3, 5, 7, 9"
        return b"2, 3, 5, 7" + t[10:], n, 0
    n = int(bits.sum())
    if flags & DOUBLES:
        assert g_start >= 4
        t = host_file(tmp_path, 1, g_start - 4, nbits + 4, pack(np.concatenate([np.zeros(4, bool), bits])))
        assert t[:18] == b"2.0, 3.0, 5.0, 7.0"
        return t[18:], n, 4
    return host_file(tmp_path, 2, g_start, nbits, pack(bits)), n, 0


def device_text(torch, ctx, flags, g_start, nbits, mask, first_rank=0, lead=0, guard=256):
    """Two calls: sizes only (no buffer), then the text into a 0xA5-filled buffer at
    byte offset `lead` with the exact capacity; guards in front and behind must survive."""
    m = torch.from_numpy(np.ascontiguousarray(mask).view(np.int64).copy()).cuda()
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.finish_text_dev_async(flags, g_start, nbits, m.data_ptr(), first_rank, 0, 0, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    cnt, need = (int(x) for x in tot.cpu())
    buf = torch.full((lead + need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    tot.zero_()
    ctx.finish_text_dev_async(flags, g_start, nbits, m.data_ptr(), first_rank, buf.data_ptr() + lead, need,
                              tot.data_ptr(), 0)
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [cnt, need]
    h = buf.cpu().numpy()
    assert (h[:lead] == 0xA5).all() and (h[lead + need:] == 0xA5).all(), "wrote outside [offset, offset + bytes)"
    return h[lead:lead + need].tobytes(), cnt


def file_triplet(b):
    return len(b), b.count(b"\n"), hashlib.sha256(b).hexdigest()


# -- 1. golden files -----------------------------------------------------------
def test_golden_files_from_resident_masks(ctx, tmp_path):
    runs = sorted({(f["N"], f["P"]) for f in GOLDEN["files"]})
    assert runs
    for N, P in runs:
        ctx.sieve_all(N, P)
        for f in GOLDEN["files"]:
            if (f["N"], f["P"]) != (N, P):
                continue
            p = ctx.finish_resident(str(tmp_path / f"primes{f['my_num']}.txt"), f["my_num"])
            assert file_triplet(open(p, "rb").read()) == (f["bytes"], f["lines"], f["sha256"]), (N, P, f["my_num"])


# -- 2. arbitrary masks ----------------------------------------------------------
NBITS = [1, 4, 5, 63, 64, 65, 640, 2**20 + 37]
# values to straddle; the last two are placed by their end / start instead
STRADDLE = [10, 10**2, 10**5, 10**7, 10**10, 10**15, 10**16, "2^53", "2^62"]


def g_start_for(point, nbits):
    if point == "2^53":  # DOUBLES' last decade: from 2^53 - 2^12 when that fits, always ending below 2^53
        return min((2**53 - 2**12 - 3) // 2 + 1, (2**53 - 3) // 2 - nbits)
    if point == "2^62":  # 19 digits, the top of the supported range
        return 2**62 - 2**21
    return max(0, (point - 3) // 2 - nbits // 2)


def masks_for(nbits, seed):
    rng = np.random.default_rng(seed)
    first, last = np.zeros(nbits, bool), np.zeros(nbits, bool)
    first[0] = last[-1] = True
    return {"zero": np.zeros(nbits, bool), "ones": np.ones(nbits, bool), "first": first, "last": last,
            "half": rng.random(nbits) < 0.5, "sixteenth": rng.random(nbits) < 1 / 16}


@pytest.mark.parametrize("point", STRADDLE, ids=str)
@pytest.mark.parametrize("nbits", NBITS)
def test_arbitrary_masks(torch, ctx, tmp_path, nbits, point):
    g0 = g_start_for(point, nbits)
    for name, bits in masks_for(nbits, 1000 + nbits).items():
        for dbl in (0, DOUBLES):
            # DOUBLES alone is compared through the host's chunk-1 file, which needs four
            # candidates below the range (module docstring)
            g = max(g0, 4) if dbl else g0
            if dbl and 3 + 2 * (g + nbits - 1) >= 2**53:
                continue  # 10^16 and 2^62: above Double printing's domain (DSE_ERANGE, test_errors_*)
            want, n, r0 = host_text(tmp_path, dbl, g, nbits, bits)
            mask = pack(bits)
            if nbits % 64:  # bits past nbits in the last word are ignored
                mask[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(nbits % 64)
            got, cnt = device_text(torch, ctx, dbl | LAST, g, nbits, mask, first_rank=r0)
            assert cnt == n, (name, dbl)
            assert got == want, (name, dbl, g, nbits)


@pytest.mark.parametrize("nbits", [4, 5, 64, 65, 640])
def test_hack_ignores_bits_0_to_3(torch, ctx, tmp_path, nbits):
    rng = np.random.default_rng(nbits)
    for pattern in range(16):
        for dbl in (0, DOUBLES):
            bits = rng.random(nbits) < 0.5
            bits[:4] = [(pattern >> j) & 1 for j in range(4)]
            want, n, _ = host_text(tmp_path, dbl | HACK, 0, nbits, bits)
            got, cnt = device_text(torch, ctx, dbl | HACK | LAST, 0, nbits, pack(bits))
            assert (got, cnt) == (want, n), (pattern, dbl)


def test_hack_on_a_large_range(torch, ctx, tmp_path):
    nbits = 2**20 + 37
    bits = np.random.default_rng(3).random(nbits) < 1 / 16
    for dbl in (0, DOUBLES):
        want, n, _ = host_text(tmp_path, dbl | HACK, 0, nbits, bits)
        got, cnt = device_text(torch, ctx, dbl | HACK | LAST, 0, nbits, pack(bits))
        assert cnt == n and got == want, dbl


@pytest.mark.parametrize("r", [0, 7])
def test_more_tiles_than_scan_threads(torch, ctx, tmp_path, r):
    """1,025 tiles of 16,384 candidates and 37 more: the single-workgroup scan over the tiles'
    (entries, bytes) pairs has 1,024 threads, so here a thread owns two tiles, one or none. A
    mask of about one bit in 1,000, first_rank 0 and 7, byte for byte against the host writer
    (first_rank r as in test_first_rank_0_to_9: r entries printed in front, then cut off)."""
    g, nbits = 10**9, 1025 * 16384 + 37
    bits = np.random.default_rng(17).random(nbits) < 1 / 1000
    bits[0] = bits[-1] = True
    full = host_file(tmp_path, 2, g - r, nbits + r, pack(np.concatenate([np.ones(r, bool), bits])))
    prefix = host_file(tmp_path, 2, g - r, r, pack(np.ones(r, bool))) if r else b""
    skip = len(prefix) - 1 if r else 0  # the prefix's entries without its closing "\n"
    assert full[:skip] == prefix[:skip]
    got, cnt = device_text(torch, ctx, LAST, g, nbits, pack(bits), first_rank=r)
    assert cnt == int(bits.sum()) and got == full[skip:]


# -- 3. rank carry -----------------------------------------------------------------
def test_rank_carries_across_a_split(torch, ctx, tmp_path):
    """Every word holds 11 entries, so a first part of k words holds 11k = k (mod 10)."""
    rng = np.random.default_rng(11)
    words = 24
    bits = np.zeros(words * 64, bool)
    for w in range(words):
        bits[w * 64 + rng.choice(64, size=11, replace=False)] = True
    g, nbits = 49_999_000, words * 64  # values cross 10^8
    mask = pack(bits)
    whole, n = device_text(torch, ctx, LAST, g, nbits, mask)
    assert whole == host_text(tmp_path, 0, g, nbits, bits)[0] and n == 11 * words
    seen = set()
    for k in range(1, 11):
        a, ca = device_text(torch, ctx, 0, g, 64 * k, mask[:k])
        b, cb = device_text(torch, ctx, LAST, g + 64 * k, nbits - 64 * k, mask[k:], first_rank=ca)
        assert a + b == whole and ca + cb == n, k
        seen.add(ca % 10)
    assert seen == set(range(10))


def test_first_rank_0_to_9(torch, ctx, tmp_path):
    g, nbits = 1000, 640
    bits = np.random.default_rng(5).random(nbits) < 0.3
    for r in range(10):
        full = host_file(tmp_path, 2, g - r, nbits + r, pack(np.concatenate([np.ones(r, bool), bits])))
        prefix = host_file(tmp_path, 2, g - r, r, pack(np.ones(r, bool))) if r else b""
        skip = len(prefix) - 1 if r else 0  # the prefix's entries without its closing "\n"
        assert full[:skip] == prefix[:skip]
        got, cnt = device_text(torch, ctx, LAST, g, nbits, pack(bits), first_rank=r)
        assert got == full[skip:] and cnt == int(bits.sum()), r


# -- 4. slabs ------------------------------------------------------------------------
@pytest.mark.parametrize("slab_words", [1, 7, 64])
def test_slab_seams(S, tmp_path, slab_words):
    from mail_sieve_e import _dse
    N, P = 10**6, 3
    files = {f["my_num"]: f for f in GOLDEN["files"] if (f["N"], f["P"]) == (N, P)}
    assert len(files) == P
    with S.Context(num_gpus=1) as c:
        c.debug_set_option("finish_slab_words", slab_words)
        c.sieve_all(N, P)
        for k in range(1, P + 1):
            b = open(c.finish_resident(str(tmp_path / f"p{k}.txt"), k), "rb").read()
            assert file_triplet(b) == (files[k]["bytes"], files[k]["lines"], files[k]["sha256"]), k
        lo, hi = S.spread_work(N, P)[0]
        nbits = P * ((hi - lo) // 2)
        n = c.finish_range(str(tmp_path / "all.txt"), 1, 0, nbits)
        m, n_ref = c.sieve_odd_range(0, nbits)
        assert n == n_ref
        assert (tmp_path / "all.txt").read_bytes() == host_file(tmp_path, 1, 0, nbits, m)
        with pytest.raises(_dse.DseError):
            c.debug_set_option("finish_slab_words", -1)


# -- 5. capacity -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DOUBLES | HACK])
def test_capacity_and_guards(torch, ctx, tmp_path, flags):
    nbits = 64 * 300 + 17  # two tiles
    bits = np.random.default_rng(9).random(nbits) < 0.4
    g = 0 if flags else 4_999_000  # values cross 10^7
    want, n, _ = host_text(tmp_path, flags, g, nbits, bits)
    m = torch.from_numpy(pack(bits).view(np.int64).copy()).cuda()
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    buf = torch.full((len(want) + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    # one byte short: totals are right, and not one byte of the buffer is touched
    ctx.finish_text_dev_async(flags | LAST, g, nbits, m.data_ptr(), 0, buf.data_ptr(), len(want) - 1, tot.data_ptr(), 0)
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [n, len(want)]
    assert bool((buf == 0xA5).all())
    # exact capacity, at every byte alignment: text right, guards in front and behind intact
    for lead in (0, 1, 2, 3):
        got, cnt = device_text(torch, ctx, flags | LAST, g, nbits, pack(bits), lead=lead)
        assert got == want and cnt == n, lead


# -- 6. no host mask ---------------------------------------------------------------------
@pytest.mark.parametrize("g_start", [5 * 10**7, (10**18 - 3) // 2], ids=["plain", "bucketed"])
def test_finish_range_without_a_host_mask(ctx, tmp_path, g_start):
    nbits = 2 * 10**6
    n = ctx.finish_range(str(tmp_path / "gpu.txt"), 2, g_start, nbits)
    m, n_ref = ctx.sieve_odd_range(g_start, nbits)
    assert n == n_ref > 0
    assert (tmp_path / "gpu.txt").read_bytes() == host_file(tmp_path, 2, g_start, nbits, m)


# -- 7. logical devices -------------------------------------------------------------------
def test_finish_resident_on_logical_devices(S, tmp_path):
    from mail_sieve_e import _dse
    N, P = 10**6, 8
    with S.Context(logical=8) as c:
        c.sieve_all(N, P)
        for k in (1, 2, 8):
            m = c.copy_chunk_mask(N, P, k)
            ref = tmp_path / f"ref{k}.txt"
            _dse.check(_dse.lib().dse_write_primes_file(str(ref).encode(), k, N, P, _dse.u64p(m)), "host writer")
            got = c.finish_resident(str(tmp_path / f"gpu{k}.txt"), k)
            assert open(got, "rb").read() == ref.read_bytes(), k


# -- 8. errors ------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(S, torch, tmp_path):
    from mail_sieve_e import _dse

    def sieves(c):
        assert c.sieve_all(10**6, 3)[1] == 78498

    def raises(code, fn, *a):
        with pytest.raises(_dse.DseError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, code)

    missing = str(tmp_path / "no_such_dir" / "primes.txt")
    with S.Context(num_gpus=1) as c:
        raises(-1, c.finish_resident, str(tmp_path / "a.txt"), 1)  # nothing resident yet
        sieves(c)
        raises(-1, c.finish_resident, str(tmp_path / "a.txt"), 4)  # chunk 4 of 3
        sieves(c)
        raises(-1, c.finish_resident, str(tmp_path / "a.txt"), 0)
        raises(-5, c.finish_resident, missing, 2)
        sieves(c)
        raises(-5, c.finish_range, missing, 2, 1000, 1000)
        sieves(c)
        raises(-1, c.finish_range, str(tmp_path / "a.txt"), 1, 0, 3)  # the hack needs four candidates
        sieves(c)
        raises(-6, c.finish_range, str(tmp_path / "a.txt"), 1, (2**53 - 3) // 2 - 10, 100)  # Doubles reach 2^53
        sieves(c)
        raises(-6, c.finish_range, str(tmp_path / "a.txt"), 2, 2**62 - 10, 100)  # beyond 2^62
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        m = torch.zeros(2, dtype=torch.int64, device="cuda")
        raises(-6, c.finish_text_dev_async, DOUBLES, (2**53 - 3) // 2 - 10, 100, m.data_ptr(), 0, 0, 0,
               tot.data_ptr(), 0)
        raises(-1, c.finish_text_dev_async, HACK, 0, 3, m.data_ptr(), 0, 0, 0, tot.data_ptr(), 0)
        raises(-1, c.finish_text_dev_async, 8, 0, 64, m.data_ptr(), 0, 0, 0, tot.data_ptr(), 0)
        sieves(c)
        # and the device finish still works
        b = open(c.finish_resident(str(tmp_path / "ok.txt"), 2), "rb").read()
        f = [f for f in GOLDEN["files"] if (f["N"], f["P"], f["my_num"]) == (10**6, 3, 2)][0]
        assert file_triplet(b) == (f["bytes"], f["lines"], f["sha256"])


# -- 9. sieve_e(gpu_finish=True) ------------------------------------------------------------
def test_sieve_e_gpu_finish_writes_the_same_file(S, ctx, tmp_path):
    N, P = 10_000, 2
    for k, bounds in enumerate(S.spread_work(N, P), start=1):
        a = S.sieve_e(k, k == 1, None, S.gen_table(bounds), None, ctx=ctx, path=str(tmp_path / f"host{k}.txt"))
        b = S.sieve_e(k, k == 1, None, S.gen_table(bounds), None, ctx=ctx, path=str(tmp_path / f"gpu{k}.txt"),
                      gpu_finish=True)
        assert (tmp_path / f"gpu{k}.txt").read_bytes() == (tmp_path / f"host{k}.txt").read_bytes(), k
        assert b.n_primes == a.n_primes and np.array_equal(a.mask, b.mask)
        f = [f for f in GOLDEN["files"] if (f["N"], f["P"], f["my_num"]) == (N, P, k)][0]
        assert file_triplet((tmp_path / f"gpu{k}.txt").read_bytes()) == (f["bytes"], f["lines"], f["sha256"])
