"""Rank and select on the GPU (csrc/dse_query.hip): pi(x), the n-th entry, the
entry after or before x and membership from a device-resident mask and its rank
index, through dse_query_index_dev_async / dse_query_dev_async (torch tensors),
dse_query_range and dse_query_resident (host arrays, the queries routed to the
chunks on the host), and the Python layer on top (prime_pi, nth_prime,
next_prime, prev_prime, is_prime).

Expected answers are numpy.searchsorted over the entry values of the test's own
bits (tests/query_ref.py), the bits from the test's patterns, from the oracle's
CPU sieve or from Miller-Rabin (tests/primes_ref.py); never from dse_primes_* or
the query code. Every comparison is exact.
"""
import numpy as np
import pytest

import primes_ref
import query_ref as R
from primes_ref import mask_bits

pytestmark = pytest.mark.gpu
T = R.T
A5 = 0xA5A5A5A5A5A5A5A5
A5_I64 = A5 - (1 << 64)
EINVAL, ERANGE = -1, -6
LEAD, GUARD = 5, 64
KIND_NAMES = ("RANK", "SELECT", "NEXT", "PREV", "TEST")


@pytest.fixture(scope="module")
def S():
    from mail_sieve_e import sieve
    return sieve


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def qctx(S):
    """A context of this module's own: the tests change its query_grid."""
    with S.Context(num_gpus=1) as c:
        yield c


@pytest.fixture(scope="module")
def bits_1e8(oracle):
    """The oracle's bits of the candidates of N = 1e8, shared and never changed."""
    nb = (10**8 - 1) // 2
    b = mask_bits(oracle.fast_sieve_range(0, nb)[0], nb)
    b.setflags(write=False)
    return b


def to_dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).cuda()


def build_index(torch, ctx, S, g, nbits, m, bits=None, stream=0):
    """The rank index of device mask m in a tensor of its own; with `bits`, checked word for word."""
    words = S.query_index_bytes(nbits) // 8
    idx = torch.full((words + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
    ctx.query_index_dev_async(g, nbits, m.data_ptr() if m is not None else 0, idx.data_ptr(), 8 * words, stream)
    if bits is not None:
        torch.cuda.synchronize()
        h = idx.cpu().numpy().view(np.uint64)
        want = R.tile_index(bits)
        assert np.array_equal(h[:len(want)], want), "the index is not the cumulative tile counts"
        assert (h[words:] == A5).all(), "wrote behind the index"
    return idx


def device_query(torch, ctx, kind, g, nbits, m, idx, q, stream=0):
    """One call into an 0xA5-filled tensor at an element offset with a guard behind -> the answers."""
    nq = len(q)
    qd = to_dev(torch, q) if nq else None
    buf = torch.full((LEAD + nq + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
    ctx.query_dev_async(kind, g, nbits, m.data_ptr() if m is not None else 0, idx.data_ptr() if idx is not None else 0,
                        qd.data_ptr() if nq else 0, nq, buf.data_ptr() + 8 * LEAD if nq else 0, stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:LEAD] == A5).all() and (h[LEAD + nq:] == A5).all(), "wrote outside [out, out + nq)"
    return h[LEAD:LEAD + nq]


def shuffled_with_duplicates(q, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(np.concatenate([q, q[:max(1, len(q) // 3)]]))


def check_all_kinds(torch, ctx, S, bits, g, m, idx, tag, every_word_seam=True, grids=(0, 1)):
    nbits = len(bits)
    vals = R.values(bits, g)
    for kind in R.KINDS:
        q = shuffled_with_duplicates(R.queries(bits, g, kind, every_word_seam), 77 + kind)
        want = R.expect(vals, kind, q)
        for grid in grids:
            ctx.debug_set_option("query_grid", grid)
            got = device_query(torch, ctx, kind, g, nbits, m, None if kind == R.TEST else idx, q)
            bad = np.flatnonzero(got != want)
            assert not len(bad), (tag, g, KIND_NAMES[kind], grid, int(q[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


# -- 1. the device API on arbitrary masks ----------------------------------------------------
@pytest.mark.parametrize("nbits", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37])
def test_arbitrary_masks(torch, qctx, S, nbits):
    try:
        for name, bits in R.masks(nbits, T, 4100 + nbits).items():
            m = to_dev(torch, R.pack_garbage(bits))
            for g in R.g_starts(nbits, T):
                idx = build_index(torch, qctx, S, g, nbits, m, bits)
                check_all_kinds(torch, qctx, S, bits, g, m, idx, name)
    finally:
        qctx.debug_set_option("query_grid", 0)


@pytest.mark.parametrize("nbits", [1024 * T, 1025 * T + 37])
def test_many_tiles(torch, qctx, S, nbits):
    """About one bit in 1,000 with both ends set, and a last-bit-only mask: SELECT crosses 1,000 empty tiles."""
    rng = np.random.default_rng(nbits)
    sparse = rng.random(nbits) < 1e-3
    sparse[[0, nbits - 1]] = True
    last = np.zeros(nbits, bool)
    last[nbits - 1] = True
    try:
        for name, bits in (("thousandth", sparse), ("last only", last)):
            # the mask one word into its allocation: 8-byte aligned and no more, as the ABI allows
            m = to_dev(torch, np.concatenate([np.array([A5], dtype=np.uint64), R.pack_garbage(bits)]))[1:]
            assert m.data_ptr() % 16 == 8
            for g in (0, 2**61 - 1 - nbits):
                idx = build_index(torch, qctx, S, g, nbits, m, bits)
                check_all_kinds(torch, qctx, S, bits, g, m, idx, name, every_word_seam=False)
    finally:
        qctx.debug_set_option("query_grid", 0)


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 4099])
def test_batch_sizes(torch, qctx, S, nq):
    nbits, g = 2 * T + 37, 12345
    bits = R.masks(nbits, T, 5)["twentieth"]
    m = to_dev(torch, R.pack_garbage(bits))
    idx = build_index(torch, qctx, S, g, nbits, m, bits)
    vals = R.values(bits, g)
    rng = np.random.default_rng(nq)
    try:
        for kind in R.KINDS:
            pool = R.queries(bits, g, kind)
            q = pool[rng.integers(0, len(pool), nq)]
            for grid in (0, 1):
                qctx.debug_set_option("query_grid", grid)
                got = device_query(torch, qctx, kind, g, nbits, m, idx, q)
                assert np.array_equal(got, R.expect(vals, kind, q)), (KIND_NAMES[kind], grid)
    finally:
        qctx.debug_set_option("query_grid", 0)


def test_empty_range(torch, qctx, S):
    idx = build_index(torch, qctx, S, 17, 0, None, np.zeros(0, bool))
    q = R.u64([0, 3, 5, 2**63, R.NONE])
    for kind, want in ((R.RANK, 0), (R.SELECT, R.NONE), (R.NEXT, R.NONE), (R.PREV, R.NONE), (R.TEST, 0)):
        assert [int(v) for v in device_query(torch, qctx, kind, 17, 0, None, idx, q)] == [want] * len(q)


# -- 2. the kernel against its host body -----------------------------------------------------
def test_kernel_equals_host_body(torch, qctx, S, bits_1e8):
    rng = np.random.default_rng(2)
    for bits, g in ((R.masks(3 * T + 11, T, 3)["half"], 2**40 + 1), (np.array(bits_1e8[:5 * T + 999]), 0)):
        nbits = len(bits)
        mh = R.pack_garbage(bits)
        m = to_dev(torch, mh)
        idx = build_index(torch, qctx, S, g, nbits, m, bits)
        lo, hi = 3 + 2 * g, 3 + 2 * (g + nbits)
        for kind in R.KINDS:
            q = rng.integers(0, 2 * nbits, 5000).astype(np.uint64) if kind == R.SELECT else \
                rng.integers(max(lo - 500, 0), hi + 500, 5000).astype(np.uint64)
            assert np.array_equal(device_query(torch, qctx, kind, g, nbits, m, idx, q),
                                  S.query_host(mh, g, nbits, kind, q)), KIND_NAMES[kind]


# -- 3. stream order ---------------------------------------------------------------------------
def stream_sieve_index_query(torch, ctx, S, g0, nb, asks):
    """base table, sieve, index and every query batch enqueued on one non-default stream, no host
    sync in between. asks: [(kind, uint64 queries)] -> their answers."""
    limit = S.base_limit_for_range(g0, nb)
    table = torch.empty(S.base_table_bytes(limit), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((nb + 63) // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    words = S.query_index_bytes(nb) // 8
    idx = torch.zeros(words, dtype=torch.int64, device="cuda")
    qs = [to_dev(torch, q) for _, q in asks]
    outs = [torch.full((len(q) + GUARD,), A5_I64, dtype=torch.int64, device="cuda") for _, q in asks]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    assert sp != 0
    ctx.base_primes_dev_async(limit, table.data_ptr(), table.numel(), sp)
    ctx.sieve_range_dev_async(table.data_ptr(), g0, nb, mask.data_ptr(), cnt.data_ptr(), sp)
    ctx.query_index_dev_async(g0, nb, mask.data_ptr(), idx.data_ptr(), 8 * words, sp)
    for (kind, q), qd, out in zip(asks, qs, outs):
        ctx.query_dev_async(kind, g0, nb, mask.data_ptr(), idx.data_ptr(), qd.data_ptr(), len(q), out.data_ptr(), sp)
    s.synchronize()
    ctx.device_status()
    got = []
    for (_, q), out in zip(asks, outs):
        h = out.cpu().numpy().view(np.uint64)
        assert (h[len(q):] == A5).all()
        got.append(h[:len(q)])
    assert int(idx[mask_tiles(nb)].item()) == int(cnt.item())
    return got


def mask_tiles(nb):
    return (nb + T - 1) // T


def test_stream_order_from_zero(torch, qctx, S, oracle):
    nb = 3 * 1966080 + 777
    bits = mask_bits(oracle.fast_sieve_range(0, nb)[0], nb)
    vals = R.values(bits, 0)
    rng = np.random.default_rng(31)
    asks = []
    for kind in R.KINDS:
        rnd = rng.integers(0, len(vals) + 50 if kind == R.SELECT else 2 * nb + 50, 3000).astype(np.uint64)
        asks.append((kind, np.concatenate([R.queries(bits, 0, kind, every_word_seam=False), rnd])))
    for (kind, q), got in zip(asks, stream_sieve_index_query(torch, qctx, S, 0, nb, asks)):
        assert np.array_equal(got, R.expect(vals, kind, q)), KIND_NAMES[kind]


def test_stream_order_bucketed_window(torch, qctx, S):
    x = 10**18
    g0, nb = (x - 4095 - 3) // 2, 4096  # the odd values x - 4095 .. x + 4095
    nxt, prv = stream_sieve_index_query(torch, qctx, S, g0, nb, [(R.NEXT, R.u64([x])), (R.PREV, R.u64([x]))])
    assert int(nxt[0]) == primes_ref.next_prime(x + 1)
    assert int(prv[0]) == primes_ref.prev_prime(x - 1)


# -- 4. resident chunks ----------------------------------------------------------------------------
def resident_checks(c, bits, N, P, nrandom, seed):
    """Every kind over all chunks (my_num=None) and per chunk, against the bits of the covered range."""
    cs = (N - 1) // 2 // P
    bits = bits[:P * cs]
    vals = R.values(bits, 0)
    end = 3 + 2 * P * cs  # the first value behind the covered range
    rng = np.random.default_rng(seed)
    # hand-placed: both sides of every chunk seam, and past the covered end
    hand_v, hand_r = {0, 1, 2, 3, 4, end - 3, end - 2, end - 1, end, end + 1, end + 10**6, 2**63, R.NONE}, set()
    ranks_before = [int(np.searchsorted(vals, 3 + 2 * k * cs)) for k in range(P + 1)]  # entries before chunk k + 1
    for k in range(1, P):
        seam = 3 + 2 * k * cs  # the first value of chunk k + 1
        r = ranks_before[k]
        around = {seam - 2, seam}
        if r > 0:
            around.add(int(vals[r - 1]))  # the last entry before the seam
        if r < len(vals):
            around.add(int(vals[r]))  # the first entry behind it
        for v in around:
            hand_v |= {v - 1, v, v + 1}
        hand_r |= {r - 2, r - 1, r, r + 1}
    hand_r |= {0, 1, len(vals) - 1, len(vals), len(vals) + 5, R.NONE}
    hand_v = R.u64(sorted(v for v in hand_v if 0 <= v <= R.NONE))
    hand_r = R.u64(sorted(v for v in hand_r if 0 <= v <= R.NONE))
    for kind in R.KINDS:
        if kind == R.SELECT:
            q = np.concatenate([hand_r, rng.integers(0, len(vals) + 100, nrandom).astype(np.uint64)])
        else:
            q = np.concatenate([hand_v, rng.integers(0, end + 1000, nrandom).astype(np.uint64)])
        q = rng.permutation(q)
        got = c.resident_query(kind, q)
        want = R.expect(vals, kind, q)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (N, P, KIND_NAMES[kind], int(q[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
    # per chunk: the chunk's own entries and ranks
    for k in sorted({1, (P + 1) // 2, P}):
        cv = vals[ranks_before[k - 1]:ranks_before[k]]
        lo, hi = 3 + 2 * (k - 1) * cs, 3 + 2 * k * cs
        for kind in R.KINDS:
            if kind == R.SELECT:
                q = R.u64(sorted({0, 1, max(len(cv), 1) - 1, len(cv), len(cv) + 5, R.NONE}))
            else:
                q = R.u64(sorted(v for v in {0, 3, lo - 2, lo - 1, lo, lo + 1, hi - 3, hi - 2, hi - 1, hi, hi + 1, R.NONE}
                                 if v >= 0))
            q = np.concatenate([q, rng.integers(0, len(cv) + 10 if kind == R.SELECT else hi + 100,
                                                min(nrandom, 200)).astype(np.uint64)])
            assert np.array_equal(c.resident_query(kind, q, my_num=k), R.expect(cv, kind, q)), (N, P, k, KIND_NAMES[kind])


@pytest.mark.parametrize("logical,P", [(None, 1), (None, 3), (3, 1), (3, 3), (3, 8), (8, 1), (8, 3), (8, 8)])
def test_resident_1e8(S, bits_1e8, logical, P):
    with S.Context(num_gpus=1, logical=logical) as c:
        c.sieve_all(10**8, P)
        resident_checks(c, bits_1e8, 10**8, P, 2000, 100 + P)


@pytest.mark.parametrize("logical,N,P", [(None, 1000, 7), (3, 1000, 7), (3, 521, 64)])
def test_resident_tiny_chunks(S, bits_1e8, logical, N, P):
    """Chunks of a handful of entries (N = 521, P = 64: four candidates each, seven of them empty):
    NEXT and PREV hop chunks, every value and every rank asked."""
    cs = (N - 1) // 2 // P
    bits = bits_1e8[:P * cs]
    if N == 521:
        per = bits.reshape(P, cs).sum(axis=1)
        assert (per[1:-1] == 0).sum() >= 5, "the run has empty chunks between non-empty ones"
    vals = R.values(bits, 0)
    with S.Context(num_gpus=1, logical=logical) as c:
        c.sieve_all(N, P)
        for kind in R.KINDS:
            q = R.u64(list(range(0, len(vals) + 4 if kind == R.SELECT else N + 40)) + [2**63, R.NONE])
            got = c.resident_query(kind, q)
            want = R.expect(vals, kind, q)
            bad = np.flatnonzero(got != want)
            assert not len(bad), (N, P, KIND_NAMES[kind], int(q[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
        resident_checks(c, bits_1e8, N, P, 50, N)


# -- 5. anchors at N = 1e9 -----------------------------------------------------------------------------
def test_anchors_1e9(ctx, oracle):
    _, pi_ref, _ = ctx.sieve_all(10**9, 1)
    assert [ctx.prime_pi(10**k) for k in range(1, 10)] == [4, 25, 168, 1229, 9592, 78498, 664579, 5761455, 50847534]
    assert [int(v) for v in ctx.nth_prime([10**k for k in range(8)])] == [2, 29, 541, 7919, 104729, 1299709, 15485863,
                                                                          179424673]
    cs = (10**9 - 1) // 2
    top = mask_bits(oracle.fast_sieve_range(cs - 5000, 5000)[0], 5000)
    assert ctx.nth_prime(pi_ref) == 3 + 2 * (cs - 5000 + int(np.flatnonzero(top)[-1])) == 999_999_937
    assert pi_ref == 50847534 and ctx.prime_pi(999_999_937) == pi_ref and ctx.prime_pi(999_999_936) == pi_ref - 1


# -- 6. the index lives as long as the masks ------------------------------------------------------------
def test_index_lifetime(S, bits_1e8):
    from mail_sieve_e import _dse
    with S.Context(num_gpus=1, logical=3) as c:
        P = 5
        q = R.u64([10**6, 10**5 + 3, 999_983, 7])
        with pytest.raises(_dse.DseError) as e:
            c.resident_query(R.RANK, q)  # nothing resident yet
        assert e.value.code == EINVAL
        def want(N, kind):
            cs = (N - 1) // 2 // P
            return [int(v) for v in R.expect(R.values(bits_1e8[:P * cs], 0), kind, q)]

        c.sieve_all(10**6, P)
        assert c.debug_get_stat("query_index_builds") == 0
        assert [int(v) for v in c.resident_query(R.TEST, q)] == want(10**6, R.TEST) == [0, 1, 1, 1]
        assert c.debug_get_stat("query_index_builds") == 0  # TEST needs no index
        assert [int(v) for v in c.resident_query(R.RANK, q, my_num=2)][3] == 0
        assert c.debug_get_stat("query_index_builds") == 1
        assert [int(v) for v in c.resident_query(R.RANK, q)] == want(10**6, R.RANK) == [78497, 9592, 78497, 3]
        assert c.debug_get_stat("query_index_builds") == P
        assert [int(v) for v in c.resident_query(R.NEXT, q)] == want(10**6, R.NEXT) == [R.NONE, 100_019, R.NONE, 11]
        assert c.debug_get_stat("query_index_builds") == P
        # another run: the answers are the new masks', a stale index would give the old ones
        c.sieve_all(3 * 10**6, P)
        q = R.u64([10**6, 10**5 + 3, 999_983, 7, 2 * 10**6, 0, 150_000, 3 * 10**6])
        for kind in R.KINDS:
            assert [int(v) for v in c.resident_query(kind, q)] == want(3 * 10**6, kind), KIND_NAMES[kind]
        assert [int(v) for v in c.resident_query(R.NEXT, q)][:4] == [1_000_003, 100_019, 1_000_003, 11]
        assert c.debug_get_stat("query_index_builds") == 2 * P
        for k in (P + 1, -1):
            with pytest.raises(_dse.DseError) as e:
                c.resident_query(R.RANK, q, my_num=k)
            assert e.value.code == EINVAL


# -- 7. the Python layer ------------------------------------------------------------------------------------
def test_python_layer(S, bits_1e8):
    N, P = 10**6, 3
    cs = (N - 1) // 2 // P
    bound = 1 + 2 * P * cs  # the last covered value
    primes = [2] + [int(v) for v in R.values(bits_1e8[:P * cs], 0)]
    with S.Context(num_gpus=1) as c:
        with pytest.raises(ValueError):
            c.prime_pi(10)  # no run yet
        _, pi_ref, _ = c.sieve_all(N, P)
        assert pi_ref == len(primes) and primes[-1] <= bound
        # scalars, around 2 and 3
        assert [c.prime_pi(x) for x in (0, 1, 2, 3, 4, 5, 100, bound, bound + 1)] == [0, 0, 1, 2, 2, 3, 25, pi_ref, pi_ref]
        assert [c.nth_prime(n) for n in (1, 2, 3, 4, 25, pi_ref)] == [2, 3, 5, 7, 97, primes[-1]]
        assert [c.next_prime(x) for x in (0, 1, 2, 3, 4, 96, 97, primes[-1] - 1)] == [2, 2, 3, 5, 5, 97, 101, primes[-1]]
        assert [c.prev_prime(x) for x in (0, 1, 2, 3, 4, 5, 98, bound + 2)] == [None, None, None, 2, 3, 3, 97, primes[-1]]
        assert [c.is_prime(x) for x in (0, 1, 2, 3, 4, 9, 97, bound, bound + 1)] == \
            [False, False, True, True, False, False, True, primes[-1] == bound, False]
        assert isinstance(c.prime_pi(100), int) and isinstance(c.is_prime(7), bool)
        # arrays
        xs = np.arange(0, 2000)
        pa = np.array(primes)
        assert np.array_equal(c.prime_pi(xs), np.searchsorted(pa, xs, side="right"))
        assert np.array_equal(c.is_prime(xs), np.isin(xs, pa))
        assert np.array_equal(c.next_prime(xs), pa[np.searchsorted(pa, xs, side="right")])
        assert np.array_equal(c.prev_prime(xs[3:]), pa[np.searchsorted(pa, xs[3:], side="left") - 1])
        assert [int(v) for v in c.prev_prime([0, 2, 3])] == [0, 0, 2]
        ns = np.arange(1, 3000)
        assert np.array_equal(c.nth_prime(ns), pa[ns - 1])
        # what the masks cannot answer
        for call, arg in ((c.prime_pi, bound + 2), (c.is_prime, bound + 2), (c.prime_pi, [5, 2**64 - 1]),
                          (c.nth_prime, pi_ref + 1), (c.nth_prime, 0), (c.nth_prime, [1, pi_ref + 1]),
                          (c.next_prime, primes[-1]), (c.next_prime, [3, bound]), (c.prev_prime, bound + 3),
                          (c.prime_pi, -1)):
            with pytest.raises(ValueError) as e:
                call(arg)
            if arg not in (0, -1):  # those two are wrong whatever is covered
                assert str(bound) in str(e.value), (call.__name__, arg)
        with pytest.raises(ValueError) as e:
            c.prime_pi([5, bound + 7, bound + 9])
        assert str(bound + 7) in str(e.value) and str(bound + 9) not in str(e.value)  # the first offending query


def test_query_range(ctx, S, bits_1e8):
    g, nbits = 10**6, 2 * T + 5
    vals = R.values(bits_1e8[g:g + nbits], g)
    for kind in R.KINDS:
        q = R.queries(bits_1e8[g:g + nbits], g, kind)
        assert np.array_equal(ctx.query_range(kind, g, nbits, q), R.expect(vals, kind, q)), KIND_NAMES[kind]
    assert len(ctx.query_range(R.RANK, g, nbits, [])) == 0
    assert [int(v) for v in ctx.query_range(R.RANK, 5, 0, [0, 100])] == [0, 0]
    # a window far above the wheel kernel's primes: the bucketed pass feeds the same index
    x = 10**15
    got = ctx.query_range(R.NEXT, (x - 3) // 2 - 100, 4096, [x])
    assert int(got[0]) == primes_ref.next_prime(x + 1)


# -- 8. errors ---------------------------------------------------------------------------------------------------
def test_errors(torch, S):
    from mail_sieve_e import _dse
    L = _dse.lib()
    with S.Context(num_gpus=1) as c:
        p = c.ptr
        m = torch.zeros(4, dtype=torch.int64, device="cuda")
        need = S.query_index_bytes(256)
        idx = torch.full((need // 8 + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
        qd = torch.zeros(8, dtype=torch.int64, device="cuda")
        out = torch.full((LEAD + 8 + GUARD,), A5_I64, dtype=torch.int64, device="cuda")
        mp, ip, qp, op = m.data_ptr(), idx.data_ptr(), qd.data_ptr(), out.data_ptr() + 8 * LEAD
        index_cases = [
            (EINVAL, (None, 0, 256, mp, ip, need, None)),            # null ctx
            (EINVAL, (p, 0, 256, mp, None, need, None)),             # null index
            (EINVAL, (p, 0, 256, None, ip, need, None)),             # null mask with nbits > 0
            (EINVAL, (p, 0, 256, mp, ip + 4, need, None)),           # misaligned index
            (EINVAL, (p, 0, 256, mp, ip, need - 1, None)),           # index_bytes too small
            (EINVAL, (p, 0, 256, mp, ip, 0, None)),
            (ERANGE, (p, 2**62 - 10, 256, mp, ip, need, None)),      # g_start + nbits > 2^62
            (ERANGE, (p, 2**63, 256, mp, ip, need, None)),
            (ERANGE, (p, 0, 2**44 + 1, mp, ip, 2**40, None)),        # more than 2^44 candidates
        ]
        for code, args in index_cases:
            assert L.dse_query_index_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((idx == A5_I64).all()), args
        assert L.dse_last_status() == ERANGE and L.dse_last_error()
        query_cases = [
            (EINVAL, (None, 0, 0, 256, mp, ip, qp, 8, op, None)),    # null ctx
            (EINVAL, (p, 5, 0, 256, mp, ip, qp, 8, op, None)),       # unknown kind
            (EINVAL, (p, 0, 0, 256, mp, ip, None, 8, op, None)),     # null queries with nq > 0
            (EINVAL, (p, 0, 0, 256, mp, ip, qp, 8, None, None)),     # null answers with nq > 0
            (EINVAL, (p, 0, 0, 256, mp, ip, qp + 4, 8, op, None)),   # misaligned queries
            (EINVAL, (p, 0, 0, 256, mp, ip, qp, 8, op + 4, None)),   # misaligned answers
            (EINVAL, (p, 0, 0, 256, mp, ip + 4, qp, 8, op, None)),   # misaligned index
            (EINVAL, (p, 0, 0, 256, None, ip, qp, 8, op, None)),     # null mask with nbits > 0
            (EINVAL, (p, 0, 0, 256, mp, None, qp, 8, op, None)),     # null index: RANK needs it
            (EINVAL, (p, 1, 0, 256, mp, None, qp, 8, op, None)),     # SELECT
            (EINVAL, (p, 2, 0, 256, mp, None, qp, 8, op, None)),     # NEXT
            (EINVAL, (p, 3, 0, 256, mp, None, qp, 8, op, None)),     # PREV
            (ERANGE, (p, 0, 2**62 - 10, 256, mp, ip, qp, 8, op, None)),
            (ERANGE, (p, 0, 0, 2**44 + 1, mp, ip, qp, 8, op, None)),
        ]
        for code, args in query_cases:
            assert L.dse_query_dev_async(*args) == code, args
            torch.cuda.synchronize()
            assert bool((out == A5_I64).all()), args
        assert L.dse_query_dev_async(p, 4, 0, 256, mp, None, qp, 8, op, None) == 0  # TEST reads no index
        assert L.dse_query_dev_async(p, 0, 0, 256, mp, ip, None, 0, None, None) == 0  # nq = 0 launches nothing
        torch.cuda.synchronize()
        h = out.cpu().numpy().view(np.uint64)
        assert not h[LEAD:LEAD + 8].any() and (h[:LEAD] == A5).all() and (h[LEAD + 8:] == A5).all()

        hq = np.arange(8, dtype=np.uint64)
        hout = np.full(8, A5, dtype=np.uint64)
        hp, ho = _dse.u64p(hq), _dse.u64p(hout)
        range_cases = [
            (EINVAL, (None, 0, 0, 64, hp, 8, ho)),
            (EINVAL, (p, 5, 0, 64, hp, 8, ho)),
            (EINVAL, (p, 0, 0, 64, None, 8, ho)),
            (EINVAL, (p, 0, 0, 64, hp, 8, None)),
            (ERANGE, (p, 0, 2**62 - 10, 64, hp, 8, ho)),
            (ERANGE, (p, 0, 0, 2**44 + 1, hp, 8, ho)),
            (ERANGE, (p, 0, 2**61, 64, hp, 8, ho)),                  # values above 2^62: dse_sieve_odd_range's rule
        ]
        for code, args in range_cases:
            assert L.dse_query_range(*args) == code, args
            assert (hout == A5).all(), args
        for code, args in [(EINVAL, (None, 1, 0, hp, 8, ho)), (EINVAL, (p, 1, 0, hp, 8, ho)), (EINVAL, (p, 0, 0, hp, 8, ho))]:
            assert L.dse_query_resident(*args) == code, args         # nothing resident yet
            assert (hout == A5).all(), args
        c.sieve_all(10**6, 3)
        for code, args in [(EINVAL, (p, 4, 0, hp, 8, ho)), (EINVAL, (p, -1, 0, hp, 8, ho)), (EINVAL, (p, 1, 5, hp, 8, ho)),
                           (EINVAL, (p, 1, 0, None, 8, ho)), (EINVAL, (p, 0, 0, hp, 8, None))]:
            assert L.dse_query_resident(*args) == code, args
            assert (hout == A5).all(), args
        with pytest.raises(_dse.DseError):
            c.debug_set_option("query_grid", 1025)
        with pytest.raises(_dse.DseError):
            c.debug_set_option("query_grid", -1)
        # and the context still works
        assert [int(v) for v in c.resident_query(R.RANK, hq)] == [0, 0, 0, 1, 1, 2, 2, 3]
        assert [int(v) for v in c.query_range(R.PREV, 0, 64, hq)] == [R.NONE] * 4 + [3, 3, 5, 5]
