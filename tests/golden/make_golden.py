"""Generate tests/golden/golden.json from the CPU oracle (oracle/dse_oracle.c).

Run from the repo root:  python tests/golden/make_golden.py [--big]

Every value here comes from the faithful restatement of sieve.clj (ref_*),
except the N >= 1e10 mask hashes, which come from the independent fast
segmented sieve (fast_*) after it was checked against ref_* at 1e9. The
reference itself cannot run in this image (Clojure/JVM absent), so these are
restatement outputs, cross-checked in tests/test_oracle.py against published
pi(10^k), sympy and the SURVEY.md section 4 table.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as o  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden.json")


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def sweep(seed: int = 0x5EED, n_cases: int = 120):
    """Seeded (N, P) sweep, N in [20, 1e7], P in [1, 8], cs >= 4."""
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < n_cases:
        lo_exp = rng.uniform(np.log10(20), 7)
        N = int(10 ** lo_exp)
        P = int(rng.integers(1, 9))
        cs, _ = o.spread_work(N, P)
        if cs < 4:
            continue
        cs, masks, counts, msgs = o.sieve(N, P)
        cases.append({"N": N, "P": P, "cs": cs, "counts": [int(c) for c in counts],
                      "pi_ref": o.pi_ref(counts), "mask_sha256": [sha(m) for m in masks],
                      "prime_messages": int(msgs)})
    return cases


def files():
    out = []
    import tempfile
    for N, P in [(10_000, 2), (1_000_000, 3)]:
        cs, masks, counts, _ = o.sieve(N, P)
        for k in range(P):
            with tempfile.NamedTemporaryFile(delete=False) as f:
                path = f.name
            o.finish(path, k + 1, N, P, masks[k])
            b = open(path, "rb").read()
            os.unlink(path)
            out.append({"N": N, "P": P, "my_num": k + 1, "bytes": len(b), "lines": b.count(b"\n"),
                        "sha256": hashlib.sha256(b).hexdigest(), "nonzero": int(counts[k]) + (1 if k == 0 else 0)})
    return out


def big(include_1e10: bool):
    res = {}
    t = time.time()
    cs, masks, counts, msgs = o.sieve(10**9, 1)
    m_fast, c_fast = o.fast_sieve_range(0, cs)
    assert np.array_equal(m_fast, masks[0]) and c_fast == int(counts[0]), "fast sieve disagrees with ref at 1e9"
    res["1e9_P1"] = {"N": 10**9, "P": 1, "cs": cs, "counts": [int(counts[0])], "pi_ref": o.pi_ref(counts),
                     "mask_sha256": [sha(masks[0])], "source": "ref_sieve (faithful) == fast_sieve_range"}
    print(f"1e9 done in {time.time() - t:.1f}s", flush=True)
    if include_1e10:
        for P in (2, 4, 8):
            t = time.time()
            N = 10**10
            cs, _ = o.spread_work(N, P)
            entry = {"N": N, "P": P, "cs": cs, "counts": [], "mask_sha256": [], "source": "fast_sieve_range"}
            for k in range(P):
                m, c = o.fast_sieve_range(k * cs, cs)
                entry["counts"].append(int(c))
                entry["mask_sha256"].append(sha(m))
            g, nb = o.tail_range(N, P)
            _, ct = o.fast_sieve_range(g, nb, want_mask=False)
            entry["pi_ref"] = 1 + sum(entry["counts"])
            entry["pi_full"] = entry["pi_ref"] + int(ct)
            res[f"1e10_P{P}"] = entry
            print(f"1e10 P={P} done in {time.time() - t:.1f}s", flush=True)
    return res


def chunk_hash(g0: int, nbits: int, piece: int = 1 << 30):
    """SHA-256 of the odd-only mask of indices [g0, g0+nbits) (ceil(nbits/64)
    LE uint64 words, bits past nbits zero) and its popcount, streamed through
    fast_sieve_range in pieces of `piece` bits (a multiple of 64), so the
    whole mask never sits in memory."""
    assert piece % 64 == 0
    h = hashlib.sha256()
    cnt = 0
    off = 0
    while off < nbits:
        nb = min(piece, nbits - off)
        m, c = o.fast_sieve_range(g0 + off, nb)
        h.update(m.view(np.uint8))
        cnt += int(c)
        off += nb
    return h.hexdigest(), cnt


def big_streamed(N: int, Ps) -> dict:
    """Per-chunk mask SHA-256 and counts of (N, P) runs, streamed (SURVEY 8(d)
    headline and 1e12 configs: masks of 6.25 GB per P at 1e11, 62.5 GB at 1e12)."""
    res = {}
    for P in Ps:
        t = time.time()
        cs, _ = o.spread_work(N, P)
        entry = {"N": N, "P": P, "cs": cs, "counts": [], "mask_sha256": [],
                 "source": "fast_sieve_range (streamed), checked against ref_sieve at 1e9 and 1e10"}
        for k in range(P):
            hx, c = chunk_hash(k * cs, cs)
            entry["counts"].append(c)
            entry["mask_sha256"].append(hx)
        g, nb = o.tail_range(N, P)
        _, ct = o.fast_sieve_range(g, nb, want_mask=False)
        entry["pi_ref"] = 1 + sum(entry["counts"])
        entry["pi_full"] = entry["pi_ref"] + int(ct)
        res[f"1e{len(str(N)) - 1}_P{P}"] = entry
        print(f"N={N:.0e} P={P} done in {time.time() - t:.1f}s pi_full={entry['pi_full']}", flush=True)
    return res


def ref_check_1e10(g: dict) -> None:
    """The faithful restatement (ref_sieve) at N=1e10, P=2/4/8 must reproduce
    the fast sieve's golden chunk hashes: pins fast_sieve_range, which alone
    reaches 1e11 and 1e12, to the restatement at 1e10 as well as 1e9."""
    for P in (2, 4, 8):
        t = time.time()
        e = g["big"][f"1e10_P{P}"]
        cs, masks, counts, _ = o.sieve(10**10, P)
        assert [int(c) for c in counts] == e["counts"], P
        assert [sha(m) for m in masks] == e["mask_sha256"], P
        del masks
        e["source"] = "ref_sieve (faithful) == fast_sieve_range"
        print(f"1e10 P={P}: ref_sieve == fast_sieve_range ({time.time() - t:.1f}s)", flush=True)


def window(g: dict) -> None:
    lo, hi = 10**18, 10**18 + 10**10
    t = time.time()
    c = o.count_window(lo, hi)
    g["big"]["window_1e18"] = {"lo": lo, "hi": hi, "count": c,
                               "source": "fast_count_window (OpenMP CPU sieve, independent of the GPU path)"}
    print(f"window [1e18, 1e18+1e10]: {c} ({time.time() - t:.1f}s)", flush=True)


def prime_values_hash(limit: int, piece_words: int = 1 << 22):
    """Count, last value and SHA-256 (of the little-endian uint32 values, in
    order) of the odd primes <= limit < 2^32: fast_sieve_range(0, nbits), then
    the set bits, then the values 3 + 2 g, hashed piece by piece."""
    nbits = (limit - 3) // 2 + 1
    m, c = o.fast_sieve_range(0, nbits)
    h = hashlib.sha256()
    n, last = 0, 0
    for w0 in range(0, len(m), piece_words):
        bits = np.unpackbits(m[w0:w0 + piece_words].view(np.uint8), bitorder="little")
        g = np.flatnonzero(bits) + 64 * w0
        if len(g):
            v = (3 + 2 * g).astype("<u4")
            h.update(v.tobytes())
            n += len(v)
            last = int(v[-1])
    assert n == int(c)
    return n, last, h.hexdigest()


TOP_SEG_BITS = 1_966_080                      # odd candidates per wheel segment
TOP_NB = 5 * TOP_SEG_BITS + 777               # tests/test_gpu_top_of_range.py, several segments at the top
TOP_G0 = 2**61 - 1 - TOP_NB                   # last index 2^61 - 2: value 2^62 - 1


def top(g: dict) -> None:
    """The top of the accepted range: the base table's primes up to 1e9 and up
    to 2^31 - 1 (count, last, hash of the values), and the mask of the last
    5 segments + 777 candidates below 2^62."""
    res = {}
    for name, limit in (("primes_1e9", 10**9), ("primes_2p31m1", 2**31 - 1)):
        t = time.time()
        n, last, hx = prime_values_hash(limit)
        res[name] = {"limit": limit, "count": n, "last": last, "values_sha256": hx,
                     "source": "fast_sieve_range(0, nbits) -> set bits -> uint32 LE values"}
        print(f"{name}: {n} odd primes, last {last} ({time.time() - t:.1f}s)", flush=True)
    t = time.time()
    m, c = o.fast_sieve_range(TOP_G0, TOP_NB)
    res["segments"] = {"g0": TOP_G0, "nb": TOP_NB, "count": int(c), "mask_sha256": sha(m),
                       "source": "fast_sieve_range (base primes to 2^31 - 1), window (2a) checked against "
                                 "Miller-Rabin in tests/test_oracle.py"}
    print(f"top segments: {int(c)} primes ({time.time() - t:.1f}s)", flush=True)
    g["top"] = res


ROUNDS_NB = 260 * TOP_SEG_BITS + 777         # tests/test_gpu_rounds.py (i): 261 segments, ragged start and end
ROUNDS_G0 = {"1e16": 10**16 // 2 + 12345, "1e18": (10**18 + 1 - 3) // 2 + 12345}


def rounds(g: dict) -> None:
    """Bucketed ranges of more segments than a device has CUs, at 1e16 and 1e18
    (the production band 1, p > 2^28): count, mask SHA-256 and the prime count
    of every segment of 1,966,080 candidates from g0 on. Before an entry is
    written, 4,096 seeded random candidates of its range are checked against
    deterministic Miller-Rabin (tests/primes_ref.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from primes_ref import is_prime_mr, mask_bits
    res = {}
    for name, g0 in ROUNDS_G0.items():
        t = time.time()
        m, c = o.fast_sieve_range(g0, ROUNDS_NB)
        bits = mask_bits(m, ROUNDS_NB)
        rng = np.random.default_rng(0x5EED)
        for j in rng.integers(0, ROUNDS_NB, 4096):
            assert bool(bits[j]) == is_prime_mr(3 + 2 * (g0 + int(j))), (name, 3 + 2 * (g0 + int(j)))
        seg = np.add.reduceat(bits.astype(np.int64), np.arange(0, ROUNDS_NB, TOP_SEG_BITS))
        assert int(seg.sum()) == int(c) == int(bits.sum())
        res[name] = {"g0": g0, "nb": ROUNDS_NB, "count": int(c), "mask_sha256": sha(m),
                     "segment_counts": [int(x) for x in seg],
                     "source": "fast_sieve_range, 4,096 seeded random candidates checked against Miller-Rabin "
                               "(tests/primes_ref.py) when generated"}
        print(f"rounds {name}: {int(c)} primes ({time.time() - t:.1f}s)", flush=True)
    g["rounds"] = res


MAXPASS_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "max_pass.json")
MAXPASS_PIECE_SEGS = 128                     # segments per hashed piece: one super-bucket of a pass from g0
_G0_1E18 = (10**18 + 1 - 3) // 2
MAXPASS = {                                  # name: (g0, nb, bucket_lo_log2, bucket_split_log2 of the entry counts)
    "window_1e18": (_G0_1E18, (10**18 + 10**10 - 1 - (10**18 + 1)) // 2 + 1, 19, 28),   # bench.py --window's range
    "max_1e18": (_G0_1E18 + 12345, 8192 * TOP_SEG_BITS + 130 * TOP_SEG_BITS + 777, 19, 28),
    # ends at 2^62 - 1. Its first 8,192 segments have 8.7e8 band-1 entries (the 1.9e9 of a pass's capacity
    # there is a bound, not a count), so the range runs on for 2,049 segments more: above 2^30 in all
    "max_top": (2**61 - 1 - ((8192 + 2048) * TOP_SEG_BITS + 777), (8192 + 2048) * TOP_SEG_BITS + 777, 19, 28),
    # where a pass of 8,192 segments can run at all: with every bucketed prime in band 1 (both test options
    # 2^20) the planner keeps it up to values of 1.7e15; at 1e15 it holds 1.9e9 band-1 entries
    "max_1e15": (10**15 // 2 + 12345, 8192 * TOP_SEG_BITS + 130 * TOP_SEG_BITS + 777, 20, 20),
}
MAXPASS_SEGS = 8192                          # the planner's largest pass (csrc kBucketMaxSegs)


def maxpass_entry(name: str, g0: int, nb: int, lo_log2: int, split_log2: int) -> dict:
    """One entry of max_pass.json from oracle.mask_window: the count, the primes
    of every segment of 1,966,080 candidates from g0 on, one SHA-256 per 128
    segments of mask (the last piece shorter) and the exact bucket entries of
    the two bands (mail_sieve_e.work). 4,096 seeded random candidates are
    checked against deterministic Miller-Rabin before anything is returned.
    The entries are those of the bucketed primes above 2^lo_log2, split into
    the bands at 2^split_log2 (19 and 28: production); first_pass_*: those of
    the first 8,192 segments."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "distributed-sieve-e_amd"))
    from mail_sieve_e import work
    from primes_ref import is_prime_mr
    t = time.time()
    m, c = o.mask_window(g0, nb)
    t_mask = time.time() - t
    for j in np.random.default_rng(0x5EED).integers(0, nb, 4096):
        j = int(j)
        assert bool(int(m[j >> 6]) >> (j & 63) & 1) == is_prime_mr(3 + 2 * (g0 + j)), (name, 3 + 2 * (g0 + j))
    seg_words = TOP_SEG_BITS // 64
    piece_words = MAXPASS_PIECE_SEGS * seg_words
    seg, hashes = [], []
    for w0 in range(0, len(m), piece_words):
        piece = m[w0:w0 + piece_words]
        hashes.append(sha(piece))
        pc = np.bitwise_count(piece).astype(np.int64)
        pc = np.concatenate([pc, np.zeros(-len(pc) % seg_words, dtype=np.int64)])  # the ragged last segment
        seg += [int(x) for x in pc.reshape(-1, seg_words).sum(axis=1)]
    assert len(seg) == -(-nb // TOP_SEG_BITS) and sum(seg) == int(c)
    t = time.time()
    lo_p, split = 2**lo_log2, 2**split_log2
    band0, band1 = work.bucket_band_entries_for_range(g0, nb, lo_p, split)
    first = work.bucket_band_entries_for_range(g0, min(nb, MAXPASS_SEGS * TOP_SEG_BITS), lo_p, split) \
        if len(seg) > MAXPASS_SEGS else (band0, band1)
    t_entries = time.time() - t
    print(f"maxpass {name}: {int(c)} primes in {len(seg)} segments, band-0 entries {band0}, band-1 entries {band1} "
          f"({first[0]} and {first[1]} in the first pass; mask {t_mask:.1f}s, entries {t_entries:.1f}s)", flush=True)
    return {"g0": g0, "nb": nb, "count": int(c), "segment_counts": seg, "piece_sha256": hashes,
            "bucket_lo_log2": lo_log2, "bucket_split_log2": split_log2,
            "band0_entries": band0, "band1_entries": band1,
            "first_pass_band0_entries": first[0], "first_pass_band1_entries": first[1],
            "source": "oracle.mask_window (fast_mask_window, the body of fast_count_window), 4,096 seeded random "
                      "candidates checked against Miller-Rabin (tests/primes_ref.py) when generated; entries by "
                      "mail_sieve_e.work.bucket_band_entries_for_range"}


def maxpass_json(res: dict) -> str:
    """max_pass.json's text: one line per field, a list of 10,000 counts on one
    line too, so the file is a few dozen lines."""
    def field(k, v, pad):
        return f'{pad}{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}'
    lines = []
    for k, v in res.items():
        if isinstance(v, dict):
            lines.append(f' {json.dumps(k)}: {{\n' + ",\n".join(field(a, b, "  ") for a, b in v.items()) + "\n }")
        else:
            lines.append(field(k, v, " "))
    return "{\n" + ",\n".join(lines) + "\n}\n"


def maxpass() -> None:
    """tests/golden/max_pass.json: the bench window and two ranges of more than
    8,192 segments (kBucketMaxSegs), at 1e18, ending at 2^62 - 1 and at 1e15."""
    res = {"generator": "tests/golden/make_golden.py --maxpass", "oracle": "oracle/dse_oracle.c",
           "seg_bits": TOP_SEG_BITS, "piece_segments": MAXPASS_PIECE_SEGS}
    for name, (g0, nb, lo_log2, split_log2) in MAXPASS.items():
        res[name] = maxpass_entry(name, g0, nb, lo_log2, split_log2)
    assert res["window_1e18"]["count"] == 241_272_176, res["window_1e18"]["count"]
    assert 3 + 2 * (res["max_top"]["g0"] + res["max_top"]["nb"] - 1) == 2**62 - 1
    assert res["max_top"]["band1_entries"] > 2**30, res["max_top"]["band1_entries"]
    # the pass whose 32-bit sums are the largest the planner allows
    assert res["max_1e15"]["first_pass_band1_entries"] > 2**30, res["max_1e15"]["first_pass_band1_entries"]
    with open(MAXPASS_OUT, "w") as f:
        f.write(maxpass_json(res))
    print("wrote", MAXPASS_OUT)


def main():
    """Default: regenerate the small fixtures (sweep, files, 1e9). Flags add or
    refresh sections of the existing golden.json in place:
      --big      1e10 P=2/4/8 (fast sieve, in memory)
      --ref1e10  check the 1e10 entries with the faithful restatement
      --big11    1e11 P=1/2/4/8 (streamed)
      --big12    1e12 P=8 (streamed, ~10 min on 8 cores)
      --window   the [1e18, 1e18+1e10] count
      --top      base-table primes to 1e9 and 2^31 - 1, and the last segments below 2^62
      --rounds   261 bucketed segments at 1e16 and at 1e18 (about 3 min of oracle time)
    --maxpass alone writes tests/golden/max_pass.json and leaves golden.json as it is: the bench
    window (2,544 segments), 8,192 + 131 segments at 1e18 and at 1e15, and 8,192 + 2,049 ending at
    2^62 - 1. Measured on 8 cores: masks 15 s, 25 s, 11 s and 38 s (the last with base primes to
    2^31 - 1), entry counts 13 s, 26 s, 1 s and 55 s of numpy; 3.5 min in all, 5 GB of memory."""
    flags = set(sys.argv[1:])
    if "--maxpass" in flags:
        assert flags == {"--maxpass"}, "--maxpass runs alone"
        maxpass()
        return
    incremental = flags & {"--ref1e10", "--big11", "--big12", "--window", "--top", "--rounds"}
    if incremental and os.path.exists(OUT):
        g = json.load(open(OUT))
    else:
        g = {"generator": "tests/golden/make_golden.py", "oracle": "oracle/dse_oracle.c",
             "sweep_seed": "0x5EED", "sweep": sweep(), "files": files(), "big": big("--big" in flags)}
    if "--ref1e10" in flags:
        ref_check_1e10(g)
    if "--big11" in flags:
        g["big"].update(big_streamed(10**11, (1, 2, 4, 8)))
    if "--big12" in flags:
        g["big"].update(big_streamed(10**12, (8,)))
    if "--window" in flags:
        window(g)
    if "--top" in flags:
        top(g)
    if "--rounds" in flags:
        rounds(g)
    with open(OUT, "w") as f:
        json.dump(g, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
