"""bench.py's contract: one JSON line with the BASELINE metric, a roofline and
cpu_baseline object, and pi verified; the N-rank path (broadcast, all-reduce,
max-over-ranks timing) rehearsed with 2 ranks on one GPU over gloo
(DSE_BENCH_REHEARSE=1; the driver's real N-GPU runs use RCCL). The roofline,
kernel times, pipelined steps and cpu_baseline belong to `--full`; a plain run
prints the headline alone, and `--dump-outputs` writes the last step's results."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_json(out: str) -> dict:
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def _check_line(d: dict, n_gpus: int):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == n_gpus and d["verified"] is True and d["value"] > 0
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-6 * rf["frac"] + 1e-12
    assert 0 < rf["frac"] <= 1
    assert 0 < rf["frac_ds_or"] < rf["frac"] and rf["cycles_per_mark_instr"] > 2.6
    # the world the run formed: one entry per rank
    w = d["world"]
    assert w["size"] == n_gpus and [x["rank"] for x in w["ranks"]] == list(range(n_gpus))
    # every rank's own figures (all-gathered, not only the max), so an N-GPU
    # line can be checked rank by rank; the headline is the max over ranks
    for x in w["ranks"]:
        assert x["step_ms"] > 0 and x["kernel_ms"] > 0 and x["bracketed_ms"] > 0 and x["pipelined_ms"] > 0
        assert x["nbits"] == d["config"]["cs"]
    assert sorted(x["g_start"] for x in w["ranks"]) == [r * d["config"]["cs"] for r in range(n_gpus)]
    assert abs(d["roofline"]["kernel_ms"] - max(x["kernel_ms"] for x in w["ranks"])) < 1e-9 + 1e-9 * d["roofline"]["kernel_ms"]
    # chunk configs broadcast the primes (109 KB at 1e11, the reference's broadcast)
    assert w["base_table"]["path"] == "broadcast" and 0 < w["base_table"]["bytes"] <= 8 << 20
    # the headline is the median of per-step times, each from the call to the counts on the host
    assert d["ms_per_step"] > 0 and d["ms_per_step_bracketed"] > 0 and d["ms_per_step_pipelined"] > 0
    assert abs(d["value"] - d["config"]["N"] / (d["ms_per_step"] / 1e3)) < 1e-6 * d["value"]
    # the line names the library it loaded (the id pmc_build.json records for a profiled build)
    assert d["build"]["libdse"].endswith("libdse.so") and len(d["build"]["libdse_sha256_16"]) == 16


@pytest.mark.gpu
def test_bench_single_gpu_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--n", "1e10", "--steps", "3",
                        "--warmup", "1", "--cpu-baseline", "on", "--cpu-max-n", "1e7"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_line(d, 1)
    cb = d["cpu_baseline"]
    # the reference's lead + 2 followers as threads + the relay thread (P = 3)
    assert cb["cores"] == 4 and cb["value"] > 0 and cb["kind"] == "port"
    assert {(x["N"], x["P"]) for x in cb["runs"]} == {(n, p) for n in (10**4, 10**6, 10**7) for p in (2, 3)}


@pytest.mark.gpu
def test_bench_window_two_rank_rehearsal():
    """--window over 2 ranks on one GPU (gloo): table built on rank 0 and
    broadcast, two slices, count all-reduced == the oracle's window count."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DSE_BENCH_REHEARSE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--full", "--gpus", "2", "--window", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["verified"] is True and d["pi_full"] == 241272176
    assert d["config"]["P"] == 2 and d["value"] > 0
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] <= 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    # the window's 203 MB of primes are not broadcast: every rank builds its table
    t = d["world"]["base_table"]
    assert t["path"] == "local" and t["bytes"] > 8 << 20
    assert [x["rank"] for x in d["world"]["ranks"]] == [0, 1] and all(x["kernel_ms"] > 0 for x in d["world"]["ranks"])


@pytest.mark.gpu
def test_bench_window_single_gpu_line():
    """BASELINE config 5 on one GPU: the count verified and an HBM roofline of
    the bucketed pass (8 B per bucket entry, WINDOW_BUCKET_ENTRIES of them)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--window", "--steps", "3",
                        "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["verified"] is True and d["pi_full"] == 241272176 and d["n_gpus"] == 1
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] <= 1
    assert abs(rf["achieved"] - 8 * 1_208_549_165 / (rf["kernel_ms"] / 1e3) / 1e9) < 1e-6 * rf["achieved"]
    # one rank: nothing to share, the table is built where it is used
    assert d["world"]["base_table"]["path"] == "local"


@pytest.mark.gpu
def test_bench_two_rank_rehearsal():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DSE_BENCH_REHEARSE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--full", "--gpus", "2", "--N", "1e10", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_line(d, 2)
    assert d["config"]["P"] == 2 and d["pi_full"] == 455052511


@pytest.mark.gpu
def test_bench_single_rank_rccl_line():
    """--rccl-single: the step's dist.broadcast of the primes and dist.all_reduce
    of the counts run through a real 1-rank nccl (RCCL) process group, formed
    by the same init_process_group("nccl", device_id=...) call an N-GPU rank
    makes; pi stays verified and the line names the nccl backend."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--n", "1e10", "--steps", "3",
                        "--warmup", "1", "--cpu-baseline", "off", "--rccl-single"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_line(d, 1)
    assert d["world"]["backend"] == "nccl" and d["world"]["rccl_single"] is True
    assert d["pi_full"] == 455052511


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(oracle, tmp_path):
    """A plain run: --steps sets the timed steps, the line carries the headline
    and none of the --full figures, and --dump-outputs writes the last step's
    counts and mask figures, equal to the oracle's chunk. N=1e8: 781,250 mask
    words (a sampled mask, a partial last popcount block) of which the last
    holds 63 valid bits."""
    import numpy as np
    N = 10**8
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "1e8", "--steps", "4",
                        "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["metric"].startswith("sieved integers/sec at N=1e11") and d["unit"] == "integers/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["pi_full"] == 5761455  # pi(1e8)
    assert d["ms_per_step"] > 0 and abs(d["value"] - N / (d["ms_per_step"] / 1e3)) < 1e-6 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["ms_per_step_pipelined"] is None
    assert all("kernel_ms" not in x and "pipelined_ms" not in x for x in d["world"]["ranks"])
    out = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(out) == ["counts", "mask_block_popcount", "mask_sample_bits", "mask_sample_index"]
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    cs = (N - 1) // 2
    words = (cs + 63) // 64
    m_ref, c_ref = oracle.fast_sieve_range(0, cs)
    assert cs % 64 == 63 and out["counts"].tolist() == [float(c_ref), 0.0] and c_ref == 5761455 - 1
    bits = np.unpackbits(np.asarray(m_ref, dtype=np.uint64).view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
    bits[-1, cs % 64:] = 0
    pc = bits.sum(axis=1)
    want = np.add.reduceat(pc, np.arange(0, words, 4096))
    assert out["mask_block_popcount"].shape == (-(-words // 4096),)
    assert np.array_equal(out["mask_block_popcount"], want.astype(np.float32))
    assert out["mask_block_popcount"].sum(dtype=np.float64) == c_ref
    idx = out["mask_sample_index"].astype(np.int64)
    assert 60000 < len(idx) <= 65536 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < words
    assert out["mask_sample_bits"].shape == (len(idx), 64)
    assert np.array_equal(out["mask_sample_bits"], bits[idx].astype(np.float32))


def test_dump_outputs_matches_numpy(tmp_path):
    """bench.dump_outputs on a host tensor (CPU only): random 64-bit words, the
    sign bit included, reduced over several chunks with a partial last block
    and a partial last word; the sample's indices repeat from call to call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(7)
    words = 2 * 3 * 4096 + 1000            # chunks of 2 blocks: 3 full chunks and a partial one
    w = rng.integers(0, 2**64, words, dtype=np.uint64)
    w[-1] = np.uint64(2**64 - 1)
    nbits = 64 * (words - 1) + 5
    mask = torch.from_numpy(w.view(np.int64).copy())
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, 1, [123, 4], mask, nbits, chunk_blocks=2)
    assert np.array_equal(mask.numpy().view(np.uint64), w)  # the mask itself is left alone
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert a["counts"].dtype == np.float64 and a["counts"].tolist() == [123.0, 4.0]
    bits = np.unpackbits(w.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
    bits[-1, 5:] = 0
    want = np.add.reduceat(bits.sum(axis=1), np.arange(0, words, bench.DUMP_BLOCK_WORDS))
    assert a["mask_block_popcount"].dtype == np.float32 and np.array_equal(a["mask_block_popcount"], want)
    idx = a["mask_sample_index"].astype(np.int64)
    assert np.array_equal(idx, np.arange(words))  # fewer words than the sample: all of them
    assert a["mask_sample_bits"].dtype == np.float32 and np.array_equal(a["mask_sample_bits"], bits)
    # count-only paths (no mask) write the counts alone; other ranks write no counts
    bench.dump_outputs(str(tmp_path / "c"), 0, 1, [9, 0], None, 0)
    assert os.listdir(tmp_path / "c") == ["counts.npy"]
    bench.dump_outputs(str(tmp_path / "e"), 1, 2, [9, 0], mask, nbits, chunk_blocks=2)
    assert sorted(os.listdir(tmp_path / "e")) == ["mask_block_popcount_rank1.npy", "mask_sample_bits_rank1.npy",
                                                  "mask_sample_index_rank1.npy"]


def test_watchdog_names_rank_and_phase():
    """A stuck phase ends the rank with status 3 and its rank, world size and
    phase on stderr (bench.Watchdog), instead of running into the driver's
    time limit. CPU only: no GPU call is made."""
    code = ("import sys, time; sys.path.insert(0, %r); import bench; "
            "w = bench.Watchdog(1, 8, 1.0); w.phase('timed steps'); time.sleep(30)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "bench.py rank 1/8 in phase 'timed steps': no progress for 1 s" in r.stderr


def test_lib_build_id_is_the_library_sha():
    """bench.lib_build(): the loaded library's path and SHA-256 prefix (CPU only:
    hashing the file, no GPU call)."""
    import hashlib
    sys.path.insert(0, ROOT)
    import bench
    b = bench.lib_build()
    path = os.path.join(ROOT, b["libdse"])
    assert os.path.exists(path)
    assert b["libdse_sha256_16"] == hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
