"""What finish_bench.py, primes_bench.py, stats_bench.py, query_bench.py, goldbach_bench.py, race_bench.py and tuples_bench.py share: the package on sys.path, the
DSE_LIB override (A/B another build of the library, as bench.py does), a per-step time limit and
the two timers (host clock and HIP events), each the median of `reps` runs after one warm-up."""
from __future__ import annotations

import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-sieve-e_amd"))

from mail_sieve_e import _dse  # noqa: E402

if os.environ.get("DSE_LIB"):  # before the first load
    _dse.LIB_PATH = os.environ["DSE_LIB"]

TOOL = os.path.splitext(os.path.basename(sys.argv[0]))[0]


class step_limit:
    """SIGALRM after `seconds`: the process exits 124 at once (no further GPU work)."""

    def __init__(self, name: str, seconds: int):
        self.name, self.seconds = name, seconds

    def _expired(self, *_):
        sys.stderr.write(f"{TOOL}: step '{self.name}' exceeded {self.seconds} s; stopping\n")
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def timed(fn, reps):
    """(median, all) seconds of fn() by the host clock."""
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def events(fn, reps):
    """(median, all) seconds of what fn() enqueues on the current stream, by HIP events."""
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(ts), ts


def ms(ts, nd=1):
    return [round(t * 1e3, nd) for t in ts]


class Record:
    """race_bench.py: print() that also keeps the lines: record.write(path) leaves them in a file (a tool's
    --out), its directory created."""

    def __init__(self):
        self.lines = []

    def __call__(self, line: str = ""):
        print(line, flush=True)
        self.lines.append(line)

    def write(self, path: str, append: bool = False):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a" if append else "w") as f:
            f.write("\n".join(self.lines) + "\n")
