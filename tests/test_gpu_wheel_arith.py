"""The wheel kernel's integer arithmetic, run on the device by the kernel's own
functions (dse_debug_wheel_arith_dev -> dse_arith_probe.hip ->
dse_wheel_kernel.h) and compared with exact integers (tests/wheel_arith_ref.py):
Kb mod p of the L units in its three regimes, the Barrett reduction and its
factor, and the float-quotient helpers of the A, B1 and B2 units. These rest on
the hardware reciprocal, a 24-bit multiply written as asm, the u64 -> f32
conversion and fixed (not looping) correction steps; a result one step outside
the bound argued in the kernel's comments is a wrong residue that nothing
repairs, and a mask comparison sees only about one such error in ten.

The domains come from the build (dse_debug_get_stat "wheel_*"). A launch holds
at most 2^24 pairs. The families are compared on the host with numpy uint64, the
exhaustive sweeps on the device with torch int64 (every operand is below 2^63).
Every test prints how many pairs it checked."""
import numpy as np
import pytest

import wheel_arith_ref as R
from mail_sieve_e import _dse

pytestmark = pytest.mark.gpu
LAUNCH = 1 << 24
U64 = np.uint64


@pytest.fixture(scope="module")
def dom(ctx):
    """The build's thresholds and its prime lists (computed once, never changed)."""
    d = {k: ctx.debug_get_stat("wheel_" + k) for k in ("ta", "tb1", "tb", "max_prime", "log_kp")}
    assert 79 < d["ta"] < d["tb1"] <= d["tb"] < d["max_prime"] <= 1 << 20 and d["log_kp"] == 17
    primes = R.odd_primes_upto(d["max_prime"])
    d["lprimes"] = primes[primes > d["tb"]]
    d["mid"] = primes[(primes > 79) & (primes <= d["tb"])]
    d["small"] = primes[(primes >= 7) & (primes <= d["tb"])]
    for v in (d["lprimes"], d["mid"], d["small"]):
        v.setflags(write=False)
    return d


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_dev(ctx, op, xd, yd):
    """One launch over device int64 tensors (their bits are the uint64 operands)."""
    import torch
    assert xd.dtype == yd.dtype == torch.int64 and xd.shape == yd.shape and xd.numel() <= LAUNCH
    od = torch.empty_like(xd)
    ctx.debug_wheel_arith_dev(op, xd.data_ptr(), yd.data_ptr(), xd.numel(), od.data_ptr(), _stream())
    return od


def run_host(ctx, op, x, y):
    """op over numpy uint64 arrays of one shape, in launches of at most 2^24 pairs."""
    import torch
    x, y = R.u64(x).ravel(), R.u64(y).ravel()
    out = np.empty_like(x)
    for s in range(0, len(x), LAUNCH):
        xd = torch.from_numpy(x[s:s + LAUNCH].view(np.int64)).cuda()
        yd = torch.from_numpy(y[s:s + LAUNCH].view(np.int64)).cuda()
        out[s:s + LAUNCH] = run_dev(ctx, op, xd, yd).cpu().numpy().view(U64)
    return out


def expect_equal(what, x, y, got, want):
    x, y, got, want = (np.asarray(a).ravel() for a in (x, y, got, want))
    bad = np.flatnonzero(got != want)
    print(f"{what}: {len(got)} pairs, {len(bad)} mismatches")
    assert len(bad) == 0, (what, [(int(x[i]), int(y[i]), int(got[i]), int(want[i])) for i in bad[:8]])
    return len(got)


def check_residues(ctx, what, op, primes, lo, hi, nj, seed):
    """op against x % p over residue_family(primes, [lo, hi)), some primes at a time."""
    rng = np.random.default_rng(seed)
    per = 3 * (nj + R.TOP_J) + len(R.powers_in(lo, hi)) + 1 + R.RANDOM_X
    step = max(1, LAUNCH // per)
    total = 0
    for s in range(0, len(primes), step):
        x, p = R.residue_family(primes[s:s + step], lo, hi, nj, rng)
        total += expect_equal(what, x, p, run_host(ctx, op, x, p), R.ref_mod(x, p))
    print(f"{what}: {total} pairs in all")


def both_families(ctx, what, op, primes, lo, hi, seed):
    """Every prime with 64 quotients; the 2,000 smallest (the largest quotients,
    the tight end of the float bound) with 4,096."""
    check_residues(ctx, what + " (every prime, 64 j)", op, primes, lo, hi, 64, seed)
    check_residues(ctx, what + " (2000 smallest, 4096 j)", op, primes[:2000], lo, hi, 4096, seed + 1)


# ---- Kb mod p ---------------------------------------------------------------

def test_kbmod_f32(ctx, dom):
    """One float quotient, two min steps: Kb in [0, 2^32), every L prime."""
    both_families(ctx, "KBMOD_F32 [0, 2^32)", _dse.ARITH_KBMOD_F32, dom["lprimes"], 0, 2**32, 1)


def test_kbmod_f38(ctx, dom):
    """The instantiation without Barrett factors over [0, 2^38), everything a
    launch without bucketed primes may meet: two float quotients above 2^32."""
    both_families(ctx, "KBMOD_F38 [0, 2^38)", _dse.ARITH_KBMOD_F38, dom["lprimes"], 0, 2**38, 3)


@pytest.mark.parametrize("name,lo,hi", [("below and across the switch", 0, 2**38 + 2**20),
                                        ("at the switch", 2**38 - 2**20, 2**38 + 2**20),
                                        ("the Barrett regime", 2**38, (2**62 - 1) // 30 + 1)])
def test_kbmod_barrett(ctx, dom, name, lo, hi):
    """The instantiation of the bucketed launches: the regime chosen by Kb as in
    production, up to the largest Kb a value below 2^62 gives."""
    both_families(ctx, f"KBMOD_BARRETT {name}", _dse.ARITH_KBMOD_BARRETT, dom["lprimes"], lo, hi, 5)


def test_kbmod_barrett_every_kb_at_the_switch(ctx, dom):
    """Every Kb in [2^38 - 2^20, 2^38 + 2^20) for the four smallest and the four
    largest L primes: one launch, compared on the device."""
    import torch
    ps = np.concatenate([dom["lprimes"][:4], dom["lprimes"][-4:]]).astype(np.int64)
    x = torch.arange(2**38 - 2**20, 2**38 + 2**20, dtype=torch.int64, device="cuda").repeat(len(ps))
    p = torch.from_numpy(ps).cuda().repeat_interleave(2**21)
    got = run_dev(ctx, _dse.ARITH_KBMOD_BARRETT, x, p)
    bad = torch.nonzero(got != x % p).flatten()
    print(f"KBMOD_BARRETT every Kb at the switch: {x.numel()} pairs, {bad.numel()} mismatches")
    assert bad.numel() == 0, [(int(x[i]), int(p[i]), int(got[i])) for i in bad[:8]]


def test_mod_barrett(ctx, dom):
    """x mod p for x < 2^63: the mid primes (mid_residue, the table kernel) and
    the L primes (unit_L from 2^38 on); for the mid primes also x = u 30^-1 for
    every u < p, the products the table kernel reduces."""
    op = _dse.ARITH_MOD_BARRETT
    check_residues(ctx, "MOD_BARRETT mid primes (4096 j)", op, dom["mid"], 0, 2**63, 4096, 7)
    both_families(ctx, "MOD_BARRETT L primes", op, dom["lprimes"], 0, 2**63, 8)
    mid = dom["mid"]
    p = np.repeat(mid, mid.astype(np.int64))
    u = np.arange(len(p), dtype=U64) - np.repeat(np.cumsum(mid) - mid, mid.astype(np.int64))
    x = u * np.repeat(R.inv30(mid), mid.astype(np.int64))
    assert int(u.max()) == int(mid[-1]) - 1 and np.all(u < p)
    expect_equal("MOD_BARRETT u 30^-1, every u < p", x, p, run_host(ctx, op, x, p), R.ref_mod(x, p))


def test_barrett_factor(ctx, dom):
    """floor((2^64 - 1) / p): every odd p up to the largest wheel prime, 2^20
    random p below 2^32, and the edges of the double quotient's correction."""
    rng = np.random.default_rng(9)
    small = R.odd_primes_upto(65536)
    big = []
    for top in (2**31, 2**32):                        # the 64 largest primes below each
        cand = np.arange(top - 1, top - 4000, -2, dtype=U64)
        big += cand[(cand[:, None] % small[None, :] != 0).all(axis=1)][:64].tolist()
    assert len(big) == 128 and big[0] == 2**31 - 1 and big[64] == 2**32 - 5
    edges = [2, 3, 2**32 - 1] + [2**k + d for k in range(2, 32) for d in (-1, 1)] + [2**32 - 1, 2**31] + big
    p = np.concatenate([np.arange(3, dom["max_prime"] + 1, 2, dtype=U64),
                        rng.integers(2, 2**32, size=2**20, dtype=U64), np.array(edges, dtype=U64)])
    got = run_host(ctx, _dse.ARITH_BARRETT_FACTOR, np.zeros_like(p), p)
    expect_equal("BARRETT_FACTOR", p, p, got, R.ref_barrett_factor(p))


# ---- the A / B1 / B2 helpers --------------------------------------------------

def _segments(counts, limit=LAUNCH):
    """Split range(len(counts)) into runs whose counts sum to at most limit."""
    runs, s, tot = [], 0, 0
    for i, c in enumerate(counts):
        assert c <= limit
        if tot + c > limit:
            runs.append((s, i))
            s, tot = i, 0
        tot += c
    runs.append((s, len(counts)))
    return runs


def _ragged(ps, counts):
    """Device tensors (p of each element, its index within its p's run) for runs
    of counts[i] elements of ps[i]."""
    import torch
    ps = torch.as_tensor(np.asarray(ps, dtype=np.int64), device="cuda")
    cn = torch.as_tensor(np.asarray(counts, dtype=np.int64), device="cuda")
    p = ps.repeat_interleave(cn)
    idx = torch.arange(p.numel(), dtype=torch.int64, device="cuda") - (cn.cumsum(0) - cn).repeat_interleave(cn)
    return p, idx


@pytest.mark.parametrize("op,ceil", [(_dse.ARITH_DIV_SMALL, 0), (_dse.ARITH_DIV_CEIL_SMALL, 1)])
def test_div_small(ctx, dom, op, ceil):
    """floor(t / p) and ceil(t / p): every t < 2^18 for every odd p in [7, TB];
    from 2^18 to 2^24 every multiple of p with both neighbours, and 2^24 - 1."""
    import torch
    name = "DIV_CEIL_SMALL" if ceil else "DIV_SMALL"
    ps = np.arange(7, dom["tb"] + 1, 2, dtype=np.int64)
    total = nbad = 0

    def check(t, p):
        nonlocal total, nbad
        got = run_dev(ctx, op, t, p)
        want = (t + (p - 1) * ceil) // p
        bad = torch.nonzero(got != want).flatten()
        total, nbad = total + t.numel(), nbad + bad.numel()
        assert bad.numel() == 0, (name, [(int(t[i]), int(p[i]), int(got[i]), int(want[i])) for i in bad[:8]])

    per = LAUNCH >> 18
    t18 = torch.arange(1 << 18, dtype=torch.int64, device="cuda")
    for s in range(0, len(ps), per):
        g = torch.as_tensor(ps[s:s + per], device="cuda")
        check(t18.repeat(len(g)), g.repeat_interleave(1 << 18))
    counts = (1 << 24) // ps + 1                     # j = 0 .. floor(2^24 / p)
    for a, b in _segments(counts, LAUNCH // 3):
        p, j = _ragged(ps[a:b], counts[a:b])
        t = torch.cat([j * p - 1, j * p, j * p + 1])
        keep = (t >= 1 << 18) & (t < 1 << 24)
        check(t[keep], p.repeat(3)[keep])
    top = torch.full((len(ps),), (1 << 24) - 1, dtype=torch.int64, device="cuda")
    check(top, torch.as_tensor(ps, device="cuda"))
    print(f"{name}: {total} pairs, {nbad} mismatches")
    assert total > len(ps) << 18


def test_mulmod_small_exhaustive(ctx, dom):
    """a b mod p for every a, b < p and every odd prime 7 <= p <= TB."""
    import torch
    ps = dom["small"].astype(np.int64)
    total = 0
    for a, b in _segments(ps * ps):
        p, idx = _ragged(ps[a:b], (ps * ps)[a:b])
        u, v = idx // p, idx % p
        got = run_dev(ctx, _dse.ARITH_MULMOD_SMALL, u | v << 32, p)
        bad = torch.nonzero(got != u * v % p).flatten()
        assert bad.numel() == 0, [(int(u[i]), int(v[i]), int(p[i]), int(got[i])) for i in bad[:8]]
        total += p.numel()
    print(f"MULMOD_SMALL: {total} pairs, 0 mismatches")
    assert total == int((ps * ps).sum())


def test_plane_first(ctx, dom):
    """Every (Xs < p, rho in R30) of every mid prime, by definition: the result k
    is below p and p | Xs + rho + 30k (which makes it the smallest such k)."""
    mid = dom["mid"]
    n = mid.astype(np.int64)
    p = np.repeat(mid, n)
    Xs = np.arange(len(p), dtype=U64) - np.repeat(np.cumsum(mid) - mid, n)
    p, Xs = np.tile(p, 8), np.tile(Xs, 8)
    rho = np.repeat(np.array(R.R30, dtype=U64), len(p) // 8)
    k = run_host(ctx, _dse.ARITH_PLANE_FIRST, R.pack(Xs, rho), p)
    bad = R.plane_first_violations(Xs, rho, p, k)
    print(f"PLANE_FIRST: {len(p)} pairs, {len(bad)} mismatches")
    assert len(bad) == 0, [(int(Xs[i]), int(rho[i]), int(p[i]), int(k[i])) for i in bad[:8]]
    assert len(p) == 8 * int(mid.sum())


def test_first_at_or_after(ctx, dom):
    """Every mid prime; kp in {0, 1, p - 1, random}; start in {0, kp, kp +- 1,
    2^23 - 1} and j p, j p + kp with both neighbours (the values where
    ceil((start - kp) / p) steps) for the 3 smallest, the 8 largest and 256
    random j with j p < 2^23."""
    rng = np.random.default_rng(13)
    xs, ys, ws = [], [], []
    for q in dom["mid"].tolist():
        kps = [0, 1, q - 1] + rng.integers(0, q, size=5).tolist()
        jmax = (2**23 - 1) // q
        jp = q * np.concatenate([np.arange(3), jmax - np.arange(8), rng.integers(0, jmax + 1, size=256)])
        for kp in kps:
            st = np.concatenate([jp + kp - 1, jp + kp, jp + kp + 1, jp - 1, jp, jp + 1,
                                 np.array([0, kp, kp - 1, kp + 1, 2**23 - 1])])
            st = np.unique(np.clip(st, 0, 2**23 - 1)).astype(U64)
            xs.append(R.pack(np.full(len(st), kp, dtype=U64), st))
            ys.append(np.full(len(st), q, dtype=U64))
            ws.append(R.ref_first_at_or_after(np.full(len(st), kp), st, ys[-1]))
    x, y, want = np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)
    expect_equal("FIRST_AT_OR_AFTER", x, y, run_host(ctx, _dse.ARITH_FIRST_AT_OR_AFTER, x, y), want)


# ---- the comparison can fail, and the call keeps its contract -------------------

def test_control_f32_outside_its_domain_disagrees(ctx, dom):
    """KBMOD_F32 reduces the low 32 bits of Kb: on Kb = 2^32 + r it returns
    r mod p, which differs from Kb mod p for every odd prime (2^32 mod p != 0).
    So the probe computes from its inputs and the comparison above can fail."""
    rng = np.random.default_rng(17)
    r, p = (a.ravel() for a in R.residue_family(dom["lprimes"][::16], 0, 2**32, 16, rng))
    kb = r + U64(2**32)
    got = run_host(ctx, _dse.ARITH_KBMOD_F32, kb, p)
    ndiff = int(np.count_nonzero(got != R.ref_mod(kb, p)))
    print(f"control: {got.size} pairs, {ndiff} differ from Kb mod p (expected: all)")
    assert np.array_equal(got, R.ref_mod(r, p).ravel())
    assert ndiff == got.size


def test_call_contract(ctx):
    import torch
    L = _dse.lib()
    n = 1000
    x = torch.arange(n, dtype=torch.int64, device="cuda") + 2**33
    y = torch.full((n,), 1543, dtype=torch.int64, device="cuda")
    buf = torch.full((n + 512,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    out = buf[256:256 + n]
    s = _stream()
    # n = 0: nothing is launched or read, whatever the pointers
    assert L.dse_debug_wheel_arith_dev(ctx.ptr, 0, None, None, 0, None, s) == 0
    assert L.dse_debug_wheel_arith_dev(ctx.ptr, 0, x.data_ptr(), y.data_ptr(), 0, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0x5A5A5A5A5A5A5A5A).all())
    for args in ((None, 0, x.data_ptr(), y.data_ptr(), n, out.data_ptr(), s),            # null ctx
                 (ctx.ptr, 10, x.data_ptr(), y.data_ptr(), n, out.data_ptr(), s),          # unknown op
                 (ctx.ptr, 2**32 - 1, x.data_ptr(), y.data_ptr(), n, out.data_ptr(), s),
                 (ctx.ptr, 0, None, y.data_ptr(), n, out.data_ptr(), s),                    # null pointers
                 (ctx.ptr, 0, x.data_ptr(), None, n, out.data_ptr(), s),
                 (ctx.ptr, 0, x.data_ptr(), y.data_ptr(), n, None, s),
                 (ctx.ptr, 0, x.data_ptr() + 4, y.data_ptr(), n, out.data_ptr(), s),        # misaligned
                 (ctx.ptr, 0, x.data_ptr(), y.data_ptr() + 4, n, out.data_ptr(), s),
                 (ctx.ptr, 0, x.data_ptr(), y.data_ptr(), n, out.data_ptr() + 4, s)):
        assert L.dse_debug_wheel_arith_dev(*args) == -1, args
    torch.cuda.synchronize()
    assert bool((buf == 0x5A5A5A5A5A5A5A5A).all())
    # a guard band on both sides of out stays untouched, for every op
    for op in range(10):
        buf.fill_(0x5A5A5A5A5A5A5A5A)
        ctx.debug_wheel_arith_dev(op, x.data_ptr(), y.data_ptr(), n, out.data_ptr(), s)
        torch.cuda.synchronize()
        assert bool((buf[:256] == 0x5A5A5A5A5A5A5A5A).all()) and bool((buf[256 + n:] == 0x5A5A5A5A5A5A5A5A).all()), op
        assert not bool((out == 0x5A5A5A5A5A5A5A5A).any()), op
    # a modulus outside every domain (below 2, above 2^32 - 1) gives 0 without running the op
    y2 = torch.tensor([0, 1, 2**32, 2**63 - 1, -1], dtype=torch.int64, device="cuda")
    for op in range(10):
        o2 = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        ctx.debug_wheel_arith_dev(op, x.data_ptr(), y2.data_ptr(), 5, o2.data_ptr(), s)
        assert o2.tolist() == [0] * 5, op
    with pytest.raises(_dse.DseError):
        ctx.debug_get_stat("wheel_nothing")


# ---- the whole table, exactly -------------------------------------------------

def _table(ctx, limit, route):
    """The table's columns as numpy arrays: (count, P, M, A, PL0, PL1)."""
    import torch
    from mail_sieve_e import sieve as S
    tbytes, pbytes = S.base_table_bytes(limit), S.base_table_prime_bytes(limit)
    t = torch.full((tbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.base_primes_dev_async(limit, t.data_ptr(), tbytes, _stream())
    if route == "finish":
        torch.cuda.synchronize()
        part = torch.full((tbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        part[:pbytes] = t[:pbytes]
        ctx.base_table_finish_dev_async(limit, part.data_ptr(), tbytes, _stream())
        t = part
    torch.cuda.synchronize()
    raw = t.cpu().numpy()
    count, cap = (int(v) for v in raw[:8].view(np.uint32))
    assert cap == (pbytes - 16) // 4 and count <= cap
    m_off = (16 + 4 * cap + 7) & ~7
    a_off = (m_off + 8 * cap + 31) & ~31
    l_off = a_off + 32 * cap
    assert tbytes == l_off + 8 * cap
    P = raw[16:16 + 4 * count].view(np.uint32).astype(np.int64)
    M = raw[m_off:m_off + 8 * count].view(U64)
    A = raw[a_off:a_off + 32 * count].view(np.uint32).astype(np.int64).reshape(count, 8)
    PL0 = raw[l_off:l_off + 4 * count].view(np.uint32).astype(np.int64)
    PL1 = raw[l_off + 4 * cap:l_off + 4 * cap + 4 * count].view(np.uint32).astype(np.int64)
    return count, P, M, A, PL0, PL1


def _full_last_set_limit(dom):
    """A limit whose table ends exactly at the end of an L set of 64."""
    primes = R.odd_primes_upto(20000)
    kL0 = int(np.count_nonzero(primes <= dom["tb"]))
    return int(primes[kL0 + 4 * 64 - 1])


@pytest.mark.parametrize("route", ["build", "finish"])
@pytest.mark.parametrize("limit", [97, 1_000, "full_last_set", 1_048_573, 1_048_583, 2_000_003, 5_000_011])
def test_table_columns(ctx, dom, limit, route):
    """m[], a[] and pl[] of every table prime up to the largest wheel prime,
    against exact values: both build routes; limits below the L list, at the
    largest wheel prime (1,048,573) and just past it, past it with a set of 64
    that straddles it, one two-level build (5,000,011), and one whose last set
    of 64 is full (the others' is partial)."""
    label = limit
    if limit == "full_last_set":
        limit = _full_last_set_limit(dom)
    count, P, M, A, PL0, PL1 = _table(ctx, limit, route)
    want_p = R.odd_primes_upto(limit).astype(np.int64)
    assert count == len(want_p) and np.array_equal(P, want_p)
    n = int(np.count_nonzero(P <= dom["max_prime"]))      # rows, factors and plans exist up to here
    kL0 = int(np.count_nonzero(want_p <= dom["tb"]))
    p = P[:n]
    # Barrett factors
    assert np.array_equal(M[:n], R.ref_barrett_factor(p))
    # rows: a[8i + ((j - i) & 7)] = (-R30[j] / 30) mod p, zero rows for 3 and 5
    n35 = int(np.count_nonzero(p < 7))
    assert n35 == min(n, 2) and not A[:n35].any()
    rows = R.ref_rows(p[n35:]).astype(np.int64)
    i = np.arange(n35, n)[:, None]
    j = np.arange(8)[None, :]
    got = A[i, (j - i) & 7]
    bad = np.argwhere(got != rows)
    assert len(bad) == 0, [(int(p[n35 + r]), int(c), int(got[r, c]), int(rows[r, c])) for r, c in bad[:8]]
    # pl[] words: the prime in the low 20 bits, bit 31 clear, one safe plan per set of 64
    nsets = partial = 0
    for PL, kp in ((PL0, 1 << 17), (PL1, 1 << 16)):
        w = PL[:n]
        assert np.array_equal(w & 0xFFFFF, p) and not (w >> 31).any()
        plan = w >> 20
        assert not plan[:min(n, kL0)].any()
        for s0 in range(kL0, n, 64):
            pl = plan[s0:min(s0 + 64, n)]
            assert (pl == pl[0]).all(), (kp, s0)
            pmin, pmax = int(P[s0]), int(P[min(s0 + 63, count - 1)])
            mode, tail, run = int(pl[0]) & 3, int(pl[0]) & 4, int(pl[0]) >> 3
            assert (mode == 2) == (pmin > kp), (kp, s0, pl[0])
            assert (mode == 1) == (kp // 2 < pmin <= kp), (kp, s0, pl[0])
            assert mode in (0, 1, 2)
            if mode == 0 and not tail:
                assert run >= -(-kp // pmin), (kp, s0, pl[0])          # every lane's hit count is at most this
            if mode == 0 and tail:
                assert run <= kp // pmax, (kp, s0, pl[0])              # every lane has at least this many hits
            nsets += 1
            partial += s0 + 64 > count
    print(f"table {limit} {route}: {n} primes, {8 * (n - n35)} row entries, {nsets} plans ({partial} of partial sets)")
    if label == "full_last_set":     # the table ends with a full set, in both pl[] columns
        assert n == count > kL0 and (count - kL0) % 64 == 0 and partial == 0 and nsets == 8
    if label == 1_048_573:           # ... and here inside one
        assert n == count and (count - kL0) % 64 != 0 and partial == 2
