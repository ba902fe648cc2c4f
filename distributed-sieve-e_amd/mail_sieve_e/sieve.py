"""Mirror of mail-sieve-e.sieve (/root/reference/src/mail_sieve_e/sieve.clj).

Same names and argument meaning as the reference's public functions; the
chunk vector with zeroed composites becomes a bit-packed odd-only mask
produced by libdse.so's gfx950 kernels:

  gen-table    (sieve.clj:9-13)   -> gen_table: a Chunk descriptor [lower, upper)
  spread-work  (sieve.clj:15-34)  -> spread_work: exact integer bounds
  sieve-e      (sieve.clj:118-172)-> sieve_e: segmented sieve of the chunk on a GPU
  finish       (sieve.clj:82-108) -> finish: byte-exact ~/primes{k}.txt

indices / mark-composites / find-next-non-zero / find-first-prime
(sieve.clj:36-80,110-116) are the reference's inner loop; they have no
counterpart here because the kernel replaces them (DESIGN.md "Path").
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _dse
from ._dse import check, lib, u64p


# Constellation patterns (include/dse.h "statistics of a mask"): bit j set means
# the candidate j places above, the value p + 2j, must be prime too.
def pattern(*diffs: int) -> int:
    """The pattern of the primes p + d for the even differences d: pattern(0, 2, 6) == 0b1011."""
    m = 0
    for d in diffs:
        if d < 0 or d > 62 or d % 2:
            raise ValueError("differences are even and in 0..62")
        m |= 1 << (d // 2)
    if not m & 1:
        raise ValueError("a pattern starts at difference 0")
    return m


TWINS = pattern(0, 2)
TRIPLETS = (pattern(0, 2, 6), pattern(0, 4, 6))
QUADRUPLETS = pattern(0, 2, 6, 8)
QUINTUPLETS = (pattern(0, 2, 6, 8, 12), pattern(0, 4, 6, 10, 12))
SEXTUPLETS = pattern(0, 4, 6, 10, 12, 16)
CONSTELLATIONS = (TWINS,) + TRIPLETS + (QUADRUPLETS,) + QUINTUPLETS + (SEXTUPLETS,)


def exact_gap(d: int):
    """(require, forbid) of the consecutive primes exactly 2d apart (include/dse.h
    "constellations as numbers"): p and p + 2d prime, nothing prime between them."""
    if d < 1 or d > 31:
        raise ValueError("d is in 1..31")
    return 1 | 1 << d, (1 << d) - 2


def tuple_members(values, require: int) -> np.ndarray:
    """The (n, k) uint64 array of all members of the matches whose lowest members
    are ``values``: column c is values + 2j for the c-th set bit j of require."""
    offs = np.array([2 * j for j in range(32) if (int(require) >> j) & 1], dtype=np.uint64)
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 1)
    return v + offs.reshape(1, -1)


def tuples_host(mask: np.ndarray, g_start: int, nbits: int, require: int, forbid: int = 0,
                above: Optional[np.ndarray] = None, above_shift: int = 0, above_bits: int = 0, first: int = 0,
                count: Optional[int] = None):
    """Test-only: the tuples kernels' per-word body run on the host over a host mask
    and a host ``above`` (include/dse.h dse_debug_tuples_host). -> (values, total):
    the matches of ranks [first, first + count) (count=None: every one from `first` on)."""
    m = np.ascontiguousarray(mask, dtype=np.uint64)
    a = None if above is None else np.ascontiguousarray(above, dtype=np.uint64)
    tot = np.zeros(2, dtype=np.uint64)

    def call(out, cap):
        check(lib().dse_debug_tuples_host(u64p(m) if len(m) else None, g_start, nbits, require, forbid,
                                          u64p(a) if a is not None and len(a) else None, above_shift, above_bits,
                                          first, out, cap, u64p(tot)), "dse_debug_tuples_host")
    if count is None:
        call(None, 0)
        count = max(0, int(tot[0]) - first)
    out = np.empty(count, dtype=np.uint64)
    call(u64p(out) if count else None, count)
    return out[:int(tot[1])], int(tot[0])


def _patterns(patterns):
    """-> (ctypes uint32 array or None, count)"""
    pats = [int(p) for p in patterns]
    return ((ctypes.c_uint32 * len(pats))(*pats) if pats else None), len(pats)


class _Result:
    """What the results of the six slab units share: ``words``, the struct of
    include/dse.h as its WORDS uint64 words, with NONE for "no such candidate", and
    dse_<UNIT>_merge for the results of adjacent ranges."""

    UNIT: str
    WORDS: int
    NONE: int

    def __init__(self, words: np.ndarray):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.shape != (self.WORDS,):
            raise ValueError("a dse_%s is %d uint64 words" % (self.UNIT, self.WORDS))
        self.words = w

    @classmethod
    def _opt(cls, v):
        return None if v == cls.NONE else v

    @classmethod
    def _filled(cls, fn: str, *args):
        """The result that the libdse call ``fn(*args, out)`` writes; a uint64 array
        among args goes as the pointer to its words, an empty one as None."""
        out = np.zeros(cls.WORDS, dtype=np.uint64)
        ptrs = [(u64p(a) if len(a) else None) if isinstance(a, np.ndarray) else a for a in args]
        check(getattr(lib(), fn)(*ptrs, u64p(out)), fn)
        return cls(out)

    def merge(self, other):
        """The result of this range followed by the adjacent ``other`` (dse_<unit>_merge;
        a Race's ``other`` started from this one's d_end)."""
        return self._filled("dse_%s_merge" % self.UNIT, self.words, other.words)

    def __eq__(self, other):
        return isinstance(other, type(self)) and np.array_equal(self.words, other.words)


def _words(bits):
    """A host mask (or ``above`` / ``below``, which may be None) as contiguous uint64 words."""
    return None if bits is None else np.ascontiguousarray(bits, dtype=np.uint64)


class Stats(_Result):
    """One dse_stats (include/dse.h): the constellation counts and gap statistics
    of the odd candidates [g_start, g_start + nbits). ``words`` is the struct as
    its uint64 words."""

    UNIT, WORDS, NONE = "stats", _dse.STATS_WORDS, _dse.STATS_NONE

    g_start = property(lambda s: int(s.words[0]))
    nbits = property(lambda s: int(s.words[1]))
    primes = property(lambda s: int(s.words[2]))
    first_g = property(lambda s: s._opt(int(s.words[3])))
    last_g = property(lambda s: s._opt(int(s.words[4])))
    head = property(lambda s: int(s.words[5]))
    tail = property(lambda s: int(s.words[6]))
    gap_overflow = property(lambda s: int(s.words[26]))
    max_gap = property(lambda s: int(s.words[24]))
    max_gap_g = property(lambda s: s._opt(int(s.words[25])))

    @property
    def first(self) -> Optional[int]:
        """The first prime of the range, or None."""
        return None if self.first_g is None else 3 + 2 * self.first_g

    @property
    def last(self) -> Optional[int]:
        return None if self.last_g is None else 3 + 2 * self.last_g

    @property
    def patterns(self) -> List[int]:
        return [int(v) for v in self.words[8:8 + int(self.words[7])]]

    @property
    def matches(self) -> List[int]:
        """Matches of each pattern, aligned with ``patterns``."""
        return [int(v) for v in self.words[16:16 + int(self.words[7])]]

    @property
    def gaps(self) -> np.ndarray:
        """uint64[1024]: gaps[d] = number of gaps equal to 2d."""
        return self.words[27:27 + _dse.STATS_GAP_BINS]

    @property
    def max_gap_prime(self) -> Optional[int]:
        """The lower prime of the first maximal gap, or None with fewer than two primes."""
        return None if self.max_gap_g is None else 3 + 2 * self.max_gap_g

    def __repr__(self):
        return (f"Stats(g_start={self.g_start}, nbits={self.nbits}, primes={self.primes}, matches={self.matches}, "
                f"max_gap={self.max_gap} at {self.max_gap_prime})")


def stats_host(mask: np.ndarray, g_start: int, nbits: int, patterns=CONSTELLATIONS) -> Stats:
    """Test-only: the statistics kernels' per-word bodies run on the host over a
    host mask (include/dse.h dse_debug_stats_host)."""
    pats, n = _patterns(patterns)
    return Stats._filled("dse_debug_stats_host", _words(mask), g_start, nbits, pats, n)


class Gaps(_Result):
    """One dse_gaps (include/dse.h "where the gaps are"): the first occurrence of
    every prime gap of the odd candidates [g_start, g_start + nbits). ``words`` is
    the struct as its uint64 words."""

    UNIT, WORDS, NONE = "gaps", _dse.GAPS_WORDS, _dse.GAPS_NONE

    g_start = property(lambda s: int(s.words[0]))
    nbits = property(lambda s: int(s.words[1]))
    primes = property(lambda s: int(s.words[2]))
    first_g = property(lambda s: s._opt(int(s.words[3])))
    last_g = property(lambda s: s._opt(int(s.words[4])))
    found = property(lambda s: int(s.words[5]))
    max_gap = property(lambda s: int(s.words[6]))
    max_gap_g = property(lambda s: s._opt(int(s.words[7])))
    overflow_g = property(lambda s: s._opt(int(s.words[8])))

    @property
    def first(self) -> np.ndarray:
        """uint64[1024]: first[d] = g of the lower prime of the first gap equal to 2d,
        _dse.GAPS_NONE where the range has none."""
        return self.words[9:9 + _dse.GAPS_BINS]

    @property
    def max_gap_prime(self) -> Optional[int]:
        """The lower prime of the first maximal gap, or None with fewer than two primes."""
        return None if self.max_gap_g is None else 3 + 2 * self.max_gap_g

    def _pairs(self, ds) -> List[Tuple[int, int]]:
        f = self.first
        return [(2 * int(d), 3 + 2 * int(f[int(d)])) for d in ds]

    def first_primes(self) -> List[Tuple[int, int]]:
        """(gap value 2d, lower prime of its first occurrence) for the found bins, by gap."""
        return self._pairs(np.flatnonzero(self.first != np.uint64(_dse.GAPS_NONE)))

    def records(self) -> List[Tuple[int, int]]:
        """The same pairs for the maximal gaps of the range (dse_gaps_records): the gaps
        that no longer gap precedes."""
        n = ctypes.c_uint32(0)
        d = (ctypes.c_uint32 * _dse.GAPS_BINS)()
        check(lib().dse_gaps_records(u64p(self.words), d, _dse.GAPS_BINS, ctypes.byref(n)), "dse_gaps_records")
        return self._pairs(d[:n.value])

    def __repr__(self):
        return (f"Gaps(g_start={self.g_start}, nbits={self.nbits}, primes={self.primes}, found={self.found}, "
                f"max_gap={self.max_gap} at {self.max_gap_prime})")


def gaps_host(mask: np.ndarray, g_start: int, nbits: int) -> Gaps:
    """Test-only: the gaps kernels' per-word bodies run on the host over a host mask
    (include/dse.h dse_debug_gaps_host)."""
    return Gaps._filled("dse_debug_gaps_host", _words(mask), g_start, nbits)


class Consec(_Result):
    """One dse_consec (include/dse.h "residue pairs of consecutive primes"): for the
    modulus q the pairs of consecutive primes of the odd candidates [g_start, g_start
    + nbits) by the classes of the lower and the upper prime. ``words`` is the struct
    as its uint64 words."""

    UNIT, WORDS, NONE = "consec", _dse.CONSEC_WORDS, _dse.CONSEC_NONE

    g_start = property(lambda s: int(s.words[0]))
    nbits = property(lambda s: int(s.words[1]))
    q = property(lambda s: int(s.words[2]))
    primes = property(lambda s: int(s.words[3]))
    pairs = property(lambda s: int(s.words[4]))
    first_g = property(lambda s: s._opt(int(s.words[5])))
    last_g = property(lambda s: s._opt(int(s.words[6])))

    @property
    def counts(self) -> np.ndarray:
        """uint64[64, 64]: the struct's counts[a * 64 + b]."""
        return self.words[7:].reshape(_dse.CONSEC_MAX_MODULUS, _dse.CONSEC_MAX_MODULUS)

    @property
    def matrix(self) -> np.ndarray:
        """uint64[q, q]: matrix[a, b] = pairs of consecutive primes p < p' with p = a
        and p' = b (mod q)."""
        return self.counts[:self.q, :self.q]

    def __repr__(self):
        return (f"Consec(g_start={self.g_start}, nbits={self.nbits}, q={self.q}, primes={self.primes}, "
                f"pairs={self.pairs})")


def consec_host(mask: np.ndarray, g_start: int, nbits: int, q: int) -> Consec:
    """Test-only: the consec kernels' per-word bodies run on the host over a host mask
    (include/dse.h dse_debug_consec_host)."""
    return Consec._filled("dse_debug_consec_host", _words(mask), g_start, nbits, q)


class Sums(_Result):
    """One dse_sums (include/dse.h "power and reciprocal sums"): the matches of a
    pattern in the odd candidates [g_start, g_start + nbits), the sum of their values
    and of the squares, and the fixed-point sum of the reciprocals of their required
    members, all exact integers. ``words`` is the struct as its uint64 words."""

    UNIT, WORDS, NONE = "sums", _dse.SUMS_WORDS, _dse.SUMS_NONE

    def _limbs(self, at: int, n: int) -> int:
        return sum(int(self.words[at + k]) << (64 * k) for k in range(n))

    g_start = property(lambda s: int(s.words[0]))
    nbits = property(lambda s: int(s.words[1]))
    require = property(lambda s: int(s.words[2]))
    forbid = property(lambda s: int(s.words[3]))
    above_bits = property(lambda s: int(s.words[4]))
    flags = property(lambda s: int(s.words[5]))
    matches = property(lambda s: int(s.words[6]))
    first_g = property(lambda s: s._opt(int(s.words[7])))
    last_g = property(lambda s: s._opt(int(s.words[8])))
    sum1 = property(lambda s: s._limbs(9, 2), doc="the sum of the matches' values (0 without SUMS_POWER)")
    sum2 = property(lambda s: s._limbs(11, 3), doc="the sum of their squares (0 without SUMS_POWER)")
    recip = property(lambda s: s._limbs(14, 3),
                     doc="the sum of floor(2^126 / member) over the required members (0 without SUMS_RECIP)")

    @property
    def first(self) -> Optional[int]:
        """The value of the lowest match (its lowest member), or None."""
        return None if self.first_g is None else 3 + 2 * self.first_g

    @property
    def last(self) -> Optional[int]:
        return None if self.last_g is None else 3 + 2 * self.last_g

    def reciprocal_bounds(self):
        """(lo, hi) as fractions.Fraction: the true sum of the reciprocals of the
        required members lies in [lo, hi]; every floor loses less than 1."""
        from fractions import Fraction
        one = 1 << _dse.SUMS_RECIP_SHIFT
        return (Fraction(self.recip, one),
                Fraction(self.recip + self.matches * bin(self.require).count("1"), one))

    @property
    def reciprocal(self) -> float:
        """The sum of the reciprocals as a float (the lower bound, rounded)."""
        return self.recip / (1 << _dse.SUMS_RECIP_SHIFT)

    def __repr__(self):
        return (f"Sums(g_start={self.g_start}, nbits={self.nbits}, require={self.require:#x}, forbid={self.forbid:#x}, "
                f"flags={self.flags}, matches={self.matches}, sum1={self.sum1}, sum2={self.sum2}, "
                f"reciprocal={self.reciprocal!r})")


def sums_host(mask: np.ndarray, g_start: int, nbits: int, require: int = 1, forbid: int = 0,
              above: Optional[np.ndarray] = None, above_shift: int = 0, above_bits: int = 0,
              flags: int = _dse.SUMS_POWER | _dse.SUMS_RECIP) -> Sums:
    """Test-only: the sums kernels' per-word and per-entry bodies run on the host over
    a host mask and a host ``above`` (include/dse.h dse_debug_sums_host)."""
    return Sums._filled("dse_debug_sums_host", _words(mask), g_start, nbits, require, forbid,
                        _words(above), above_shift, above_bits, flags)


def sums_recip_host(values) -> List[int]:
    """Test-only: floor(2^126 / v) for every v by the sums kernels' division routine,
    run on the host (include/dse.h dse_debug_sums_recip)."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    out = np.zeros(2 * len(v), dtype=np.uint64)
    check(lib().dse_debug_sums_recip(u64p(v) if len(v) else None, len(v), u64p(out) if len(v) else None),
          "dse_debug_sums_recip")
    lo, hi = out[0::2].tolist(), out[1::2].tolist()
    return [l | h << 64 for l, h in zip(lo, hi)]


class Goldbach(_Result):
    """One dse_goldbach (include/dse.h "additive questions"): the minimal Goldbach
    partitions of the evens 6 + 2c of the odd candidates [g_start, g_start +
    nbits). ``words`` is the struct as its uint64 words."""

    UNIT, WORDS, NONE = "goldbach", _dse.GOLDBACH_WORDS, _dse.GOLDBACH_NONE

    g_start = property(lambda s: int(s.words[0]))
    nbits = property(lambda s: int(s.words[1]))
    nprimes = property(lambda s: int(s.words[2]))
    resolved = property(lambda s: int(s.words[3]))
    unresolved = property(lambda s: int(s.words[4]))
    first_unresolved = property(lambda s: s._opt(int(s.words[5])))
    max_rank = property(lambda s: s._opt(int(s.words[6])))
    max_c = property(lambda s: s._opt(int(s.words[7])))

    @property
    def hist(self) -> np.ndarray:
        """uint64[2048]: hist[i] = evens whose minimal partition uses the i-th odd prime."""
        return self.words[8:8 + _dse.GOLDBACH_PRIMES]

    @property
    def first_unresolved_even(self) -> Optional[int]:
        """The lowest even of the range with no partition among the primes used, or None."""
        return None if self.first_unresolved is None else 6 + 2 * self.first_unresolved

    @property
    def max_prime(self) -> Optional[int]:
        """The largest minimal prime over the resolved evens, or None."""
        return None if self.max_rank is None else int(lib().dse_goldbach_prime(self.max_rank))

    @property
    def max_even(self) -> Optional[int]:
        """The first even whose minimal prime is ``max_prime``, or None."""
        return None if self.max_c is None else 6 + 2 * self.max_c

    def __repr__(self):
        return (f"Goldbach(g_start={self.g_start}, nbits={self.nbits}, nprimes={self.nprimes}, "
                f"unresolved={self.unresolved}, max_prime={self.max_prime} at {self.max_even})")


def goldbach_host(mask: np.ndarray, g_start: int, nbits: int, below: Optional[np.ndarray] = None,
                  below_shift: int = 0, below_bits: int = 0, nprimes: int = 0) -> Goldbach:
    """Test-only: the Goldbach kernel's per-word bodies run on the host over a host
    mask and a host ``below`` (include/dse.h dse_debug_goldbach_host)."""
    return Goldbach._filled("dse_debug_goldbach_host", _words(mask), g_start, nbits,
                            _words(below), below_shift, below_bits, nprimes)


class Race(_Result):
    """One dse_race (include/dse.h "residue classes and races"): the entries of the
    odd candidates [g_start, g_start + nbits) per class mod q, and the race of class
    a against class b from d_start. ``words`` is the struct as its uint64 words."""

    UNIT, WORDS, NONE = "race", _dse.RACE_WORDS, _dse.RACE_NONE

    def _signed(self, i):
        v = int(self.words[i])
        return v - (1 << 64) if v >> 63 else v

    def _value(self, i):
        g = int(self.words[i])
        return None if g == _dse.RACE_NONE else 3 + 2 * g

    g_start = property(lambda s: int(s.words[0]))
    nbits = property(lambda s: int(s.words[1]))
    q = property(lambda s: int(s.words[2]))
    a = property(lambda s: int(s.words[3]))
    b = property(lambda s: int(s.words[4]))
    d_start = property(lambda s: s._signed(5))
    d_end = property(lambda s: s._signed(6))
    steps = property(lambda s: int(s.words[7]))
    a_ahead = property(lambda s: int(s.words[8]))
    b_ahead = property(lambda s: int(s.words[9]))
    ties = property(lambda s: int(s.words[10]))
    first_a_ahead = property(lambda s: s._value(11), doc="value of the first step after which D > 0, or None")
    first_b_ahead = property(lambda s: s._value(12), doc="value of the first step after which D < 0, or None")
    max_d = property(lambda s: s._signed(13))
    max_at = property(lambda s: s._value(14), doc="value of the first step that attains max_d, or None")
    min_d = property(lambda s: s._signed(15))
    min_at = property(lambda s: s._value(16), doc="value of the first step that attains min_d, or None")

    @property
    def counts(self) -> np.ndarray:
        """uint64[q]: counts[r] = entries whose value is r mod q."""
        return self.words[17:17 + self.q]

    def __repr__(self):
        return (f"Race(g_start={self.g_start}, nbits={self.nbits}, q={self.q}, a={self.a}, b={self.b}, "
                f"d_start={self.d_start}, d_end={self.d_end}, steps={self.steps}, a_ahead={self.a_ahead}, "
                f"b_ahead={self.b_ahead}, ties={self.ties}, first_a_ahead={self.first_a_ahead}, "
                f"first_b_ahead={self.first_b_ahead}, max_d={self.max_d} at {self.max_at}, "
                f"min_d={self.min_d} at {self.min_at})")


def race_host(mask: np.ndarray, g_start: int, nbits: int, q: int, a: int, b: int, d_start: int = 0) -> Race:
    """Test-only: the race kernels' per-word bodies run on the host over a host mask
    (include/dse.h dse_debug_race_host)."""
    return Race._filled("dse_debug_race_host", _words(mask), g_start, nbits, q, a, b, d_start)


class Context:
    """A libdse context: one process driving ``num_gpus`` devices, or one
    device (``device=``) for one-process-per-GPU ranks. ``logical=k`` (tests
    only, include/dse.h dse_debug_init_logical): k logical devices on device 0,
    the multi-device code path with the collectives replaced by copies."""

    def __init__(self, num_gpus: int = 1, device: Optional[int] = None, logical: Optional[int] = None):
        L = lib()
        if logical is not None:
            self._ptr = L.dse_debug_init_logical(logical)
        else:
            self._ptr = L.dse_init_device(device) if device is not None else L.dse_init(num_gpus)
        if not self._ptr:
            raise _dse.DseError(L.dse_last_status(), "dse_init", L.dse_last_error().decode(errors="replace"))
        self._run = None  # (n, P, cs, pi_ref) of the last sieve_all: what prime_pi and its kin answer about

    @property
    def ptr(self):
        if not self._ptr:
            raise RuntimeError("context closed")
        return self._ptr

    @property
    def num_devices(self) -> int:
        return lib().dse_ctx_num_devices(self.ptr)

    def close(self) -> None:
        if self._ptr:
            lib().dse_destroy(self._ptr)
            self._ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-buffer entry points ------------------------------------------
    def sieve_odd_range(self, g_start: int, nbits: int, want_mask: bool = True):
        mask = np.zeros((nbits + 63) // 64, dtype=np.uint64) if want_mask else None
        cnt = ctypes.c_uint64()
        check(lib().dse_sieve_odd_range(self.ptr, g_start, nbits, u64p(mask), ctypes.byref(cnt)),
              "dse_sieve_odd_range")
        return mask, cnt.value

    def sieve_chunk(self, n: int, P: int, my_num: int, want_mask: bool = True):
        cs, _ = _spread(n, P)
        mask = np.zeros((cs + 63) // 64, dtype=np.uint64) if want_mask else None
        cnt = ctypes.c_uint64()
        check(lib().dse_sieve_chunk(self.ptr, n, P, my_num, u64p(mask), ctypes.byref(cnt)),
              "dse_sieve_chunk")
        return mask, cnt.value

    def sieve_all(self, n: int, P: int):
        """-> (per-chunk counts, pi_ref, pi_full); masks stay on the devices."""
        counts = np.zeros(P, dtype=np.uint64)
        pr, pf = ctypes.c_uint64(), ctypes.c_uint64()
        self._run = None
        check(lib().dse_sieve_all(self.ptr, n, P, u64p(counts), ctypes.byref(pr), ctypes.byref(pf)),
              "dse_sieve_all")
        self._run = (n, P, _spread(n, P)[0], pr.value)
        return counts, pr.value, pf.value

    def copy_chunk_mask(self, n: int, P: int, my_num: int) -> np.ndarray:
        cs, _ = _spread(n, P)
        mask = np.zeros((cs + 63) // 64, dtype=np.uint64)
        check(lib().dse_copy_chunk_mask(self.ptr, my_num, u64p(mask)), "dse_copy_chunk_mask")
        return mask

    def sieve_window(self, lo: int, hi: int) -> int:
        cnt = ctypes.c_uint64()
        check(lib().dse_sieve_window(self.ptr, lo, hi, ctypes.byref(cnt)), "dse_sieve_window")
        return cnt.value

    def device_status(self) -> None:
        """Raise DseError (DSE_EINTERNAL) if a device pass of this context broke
        an invariant since the last check (the *_dev_async calls report here)."""
        check(lib().dse_device_status(self.ptr), "dse_device_status")

    def debug_set_option(self, name: str, value: int) -> None:
        """Test-only knob of this context (include/dse.h dse_debug_set_option)."""
        check(lib().dse_debug_set_option(self.ptr, name.encode(), int(value)), "dse_debug_set_option")

    def debug_get_stat(self, name: str) -> int:
        """Test-only statistic of this context (include/dse.h dse_debug_get_stat)."""
        v = ctypes.c_int64(0)
        check(lib().dse_debug_get_stat(self.ptr, name.encode(), ctypes.byref(v)), "dse_debug_get_stat")
        return v.value

    def debug_wheel_arith_dev(self, op: int, x_ptr: int, y_ptr: int, n: int, out_ptr: int, stream_ptr: int = 0):
        """Test-only: out[i] = op(x[i], y[i]) by the wheel kernel's own integer
        helpers, on device uint64 arrays (include/dse.h dse_debug_wheel_arith_dev)."""
        check(lib().dse_debug_wheel_arith_dev(self.ptr, op, x_ptr or None, y_ptr or None, n, out_ptr or None,
                                              stream_ptr or None), "dse_debug_wheel_arith_dev")

    # -- device-buffer entry points (torch tensors' data_ptr()) --------------
    def base_primes_dev_async(self, limit: int, table_ptr: int, table_bytes: int, stream_ptr: int = 0):
        check(lib().dse_base_primes_dev_async(self.ptr, limit, table_ptr, table_bytes, stream_ptr or None),
              "dse_base_primes_dev_async")

    def base_table_finish_dev_async(self, limit: int, table_ptr: int, table_bytes: int, stream_ptr: int = 0):
        """Barrett factors + wheel offsets for a table whose primes arrived by broadcast."""
        check(lib().dse_base_table_finish_dev_async(self.ptr, limit, table_ptr, table_bytes, stream_ptr or None),
              "dse_base_table_finish_dev_async")

    def sieve_range_dev_async(self, table_ptr: int, g_start: int, nbits: int, mask_ptr: int,
                              count_ptr: int, stream_ptr: int = 0):
        check(lib().dse_sieve_range_dev_async(self.ptr, table_ptr, g_start, nbits, mask_ptr or None,
                                              count_ptr, stream_ptr or None),
              "dse_sieve_range_dev_async")

    # -- finish on the device -------------------------------------------------
    def finish_text_dev_async(self, flags: int, g_start: int, nbits: int, mask_ptr: int, first_rank: int,
                              text_ptr: int, text_cap: int, totals_ptr: int, stream_ptr: int = 0):
        """The device mask's entries as file text in device memory (include/dse.h
        dse_finish_text_dev_async): totals[0] = entries, totals[1] = bytes needed."""
        check(lib().dse_finish_text_dev_async(self.ptr, flags, g_start, nbits, mask_ptr or None, first_rank,
                                              text_ptr or None, text_cap, totals_ptr, stream_ptr or None),
              "dse_finish_text_dev_async")

    def finish_resident(self, path: str, my_num: int) -> str:
        """finish for a chunk the last sieve_all left on its device: the file's
        text is formatted on the GPU, the mask never reaches the host."""
        check(lib().dse_finish_resident_file(self.ptr, os.fsencode(path), my_num), "dse_finish_resident_file")
        return path

    def finish_range(self, path: str, my_num: int, g_start: int, nbits: int) -> int:
        """gen-table + sieve-e + finish of an odd-index range on the device -> its prime count."""
        cnt = ctypes.c_uint64()
        check(lib().dse_finish_range_file(self.ptr, os.fsencode(path), my_num, g_start, nbits, ctypes.byref(cnt)),
              "dse_finish_range_file")
        return cnt.value

    # -- primes as numbers ------------------------------------------------------
    def primes_dev_async(self, g_start: int, nbits: int, mask_ptr: int, first: int, out_ptr: int, out_cap: int,
                         totals_ptr: int, stream_ptr: int = 0):
        """The device mask's set bits as uint64 values 3 + 2 (g_start + bit) in
        device memory (include/dse.h dse_primes_dev_async): out[i] = the entry of
        rank first + i; totals[0] = entries of the range, totals[1] = written."""
        check(lib().dse_primes_dev_async(self.ptr, g_start, nbits, mask_ptr or None, first, out_ptr or None,
                                         out_cap, totals_ptr, stream_ptr or None),
              "dse_primes_dev_async")

    def _primes(self, where: str, call, first: int, count: Optional[int]) -> np.ndarray:
        """call(first, out, cap, total, written) with an exactly sized buffer:
        count=None asks for the total first (a call with no output)."""
        tot, wr = ctypes.c_uint64(), ctypes.c_uint64()
        if count is None:
            check(call(first, None, 0, ctypes.byref(tot), ctypes.byref(wr)), where)
            count = max(0, tot.value - first)
        out = np.empty(count, dtype=np.uint64)
        check(call(first, u64p(out) if count else None, count, ctypes.byref(tot), ctypes.byref(wr)), where)
        return out[:wr.value]

    def primes_range(self, g_start: int, nbits: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """gen-table + sieve-e of an odd-index range, and its primes as uint64
        values extracted on the device: the entries of ranks [first, first +
        count) in increasing order (count=None: every one from `first` on)."""
        L = lib()
        return self._primes("dse_primes_range",
                            lambda f, o, c, t, w: L.dse_primes_range(self.ptr, g_start, nbits, f, o, c, t, w),
                            first, count)

    def resident_primes(self, my_num: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The same for a chunk the last sieve_all left on its device: the mask
        never reaches the host, only the values asked for do."""
        L = lib()
        return self._primes("dse_primes_resident",
                            lambda f, o, c, t, w: L.dse_primes_resident(self.ptr, my_num, f, o, c, t, w),
                            first, count)

    def primes_window(self, lo: int, hi: int) -> np.ndarray:
        """The odd primes in [max(lo, 3), hi] (sieve_window's convention: its
        count is this array's length)."""
        g, n = self._window(lo, hi)
        return self.primes_range(g, n) if n else np.empty(0, dtype=np.uint64)

    # -- what the slab units' methods share -----------------------------------------
    def _result(self, cls, fn: str, *args):
        """The ``cls`` that the libdse call ``fn(ctx, *args, out)`` fills."""
        return cls._filled(fn, self.ptr, *args)

    @staticmethod
    def _window(lo: int, hi: int, base: int = 3):
        """-> (g_start, nbits) of the values of base's parity in [max(lo, base), hi],
        g counting them from base; an empty window is (min(g_start, 2^62), 0)."""
        a = max(lo, base)
        a += (a ^ base) & 1
        b = hi - ((hi ^ base) & 1)
        if b < a:
            return min((a - base) // 2, 1 << 62), 0
        return (a - base) // 2, (b - a) // 2 + 1

    # -- statistics of a mask -----------------------------------------------------
    def stats_dev_async(self, g_start: int, nbits: int, mask_ptr: int, patterns, stats_ptr: int,
                        stream_ptr: int = 0):
        """The device mask's constellation counts and gap statistics as one
        dse_stats (_dse.STATS_WORDS uint64 words) in device memory at stats_ptr
        (include/dse.h dse_stats_dev_async)."""
        pats, n = _patterns(patterns)
        check(lib().dse_stats_dev_async(self.ptr, g_start, nbits, mask_ptr or None, pats, n, stats_ptr or None,
                                        stream_ptr or None),
              "dse_stats_dev_async")

    def stats_range(self, g_start: int, nbits: int, patterns=CONSTELLATIONS) -> Stats:
        """gen-table + sieve-e of an odd-index range and its statistics, computed
        on the device: only the dse_stats reaches the host."""
        return self._result(Stats, "dse_stats_range", g_start, nbits, *_patterns(patterns))

    def resident_stats(self, my_num: Optional[int] = None, patterns=CONSTELLATIONS) -> Stats:
        """The statistics of a chunk the last sieve_all left on its device, or
        (my_num=None) of all its chunks: the per-chunk results merged in order."""
        return self._result(Stats, "dse_stats_resident", my_num or 0, *_patterns(patterns))

    def stats_window(self, lo: int, hi: int, patterns=CONSTELLATIONS) -> Stats:
        """The statistics of the odd values in [max(lo, 3), hi] (primes_window's
        convention); an empty window gives the empty result."""
        return self.stats_range(*self._window(lo, hi), patterns)

    # -- where the gaps are -----------------------------------------------------------
    def gaps_dev_async(self, g_start: int, nbits: int, mask_ptr: int, out_ptr: int, stream_ptr: int = 0):
        """The first occurrence of every gap of the device mask as one dse_gaps
        (_dse.GAPS_WORDS uint64 words) in device memory at out_ptr (include/dse.h
        dse_gaps_dev_async)."""
        check(lib().dse_gaps_dev_async(self.ptr, g_start, nbits, mask_ptr or None, out_ptr or None,
                                       stream_ptr or None),
              "dse_gaps_dev_async")

    def gaps_range(self, g_start: int, nbits: int) -> Gaps:
        """gen-table + sieve-e of an odd-index range and the first occurrence of every
        gap in it, computed on the device: only the dse_gaps reaches the host."""
        return self._result(Gaps, "dse_gaps_range", g_start, nbits)

    def resident_gaps(self, my_num: Optional[int] = None) -> Gaps:
        """The table of a chunk the last sieve_all left on its device, or (my_num=None)
        of all its chunks: the per-chunk results merged in order."""
        return self._result(Gaps, "dse_gaps_resident", my_num or 0)

    def gaps_window(self, lo: int, hi: int) -> Gaps:
        """The table of the odd values in [max(lo, 3), hi] (primes_window's convention);
        an empty window gives the empty result."""
        return self.gaps_range(*self._window(lo, hi))

    # -- residue pairs of consecutive primes ------------------------------------------
    def consec_dev_async(self, g_start: int, nbits: int, mask_ptr: int, q: int, out_ptr: int, stream_ptr: int = 0):
        """The pairs of consecutive primes of the device mask by their classes mod q as
        one dse_consec (_dse.CONSEC_WORDS uint64 words) in device memory at out_ptr
        (include/dse.h dse_consec_dev_async)."""
        check(lib().dse_consec_dev_async(self.ptr, g_start, nbits, mask_ptr or None, q, out_ptr or None,
                                         stream_ptr or None),
              "dse_consec_dev_async")

    def consec_range(self, g_start: int, nbits: int, q: int) -> Consec:
        """gen-table + sieve-e of an odd-index range and the pairs of its consecutive
        primes by their classes mod q, computed on the device: only the dse_consec
        reaches the host."""
        return self._result(Consec, "dse_consec_range", g_start, nbits, q)

    def resident_consec(self, my_num: Optional[int] = None, q: int = 10) -> Consec:
        """The matrix of a chunk the last sieve_all left on its device, or (my_num=None)
        of all its chunks: the per-chunk results merged in order."""
        return self._result(Consec, "dse_consec_resident", my_num or 0, q)

    def consec_window(self, lo: int, hi: int, q: int) -> Consec:
        """The matrix of the odd values in [max(lo, 3), hi] (primes_window's convention);
        an empty window gives the empty result."""
        return self.consec_range(*self._window(lo, hi), q)

    # -- power and reciprocal sums ----------------------------------------------------
    def sums_dev_async(self, g_start: int, nbits: int, mask_ptr: int, require: int, forbid: int, above_ptr: int,
                       above_shift: int, above_bits: int, flags: int, out_ptr: int, stream_ptr: int = 0):
        """The sums over the matches of (require, forbid) in the device mask as one
        dse_sums (_dse.SUMS_WORDS uint64 words) in device memory at out_ptr; the
        above_bits candidates behind the range are the bits from above_shift on of the
        device bit string at above_ptr (include/dse.h dse_sums_dev_async)."""
        check(lib().dse_sums_dev_async(self.ptr, g_start, nbits, mask_ptr or None, require, forbid,
                                       above_ptr or None, above_shift, above_bits, flags, out_ptr or None,
                                       stream_ptr or None),
              "dse_sums_dev_async")

    def sums_range(self, g_start: int, nbits: int, require: int = 1, forbid: int = 0,
                   flags: int = _dse.SUMS_POWER | _dse.SUMS_RECIP) -> Sums:
        """gen-table + sieve-e of an odd-index range (and of the 31 candidates above
        it) and the sums over its matches of (require, forbid), computed on the
        device: only the dse_sums reaches the host."""
        return self._result(Sums, "dse_sums_range", g_start, nbits, require, forbid, flags)

    def sums_resident(self, my_num: Optional[int] = None, require: int = 1, forbid: int = 0,
                      flags: int = _dse.SUMS_POWER | _dse.SUMS_RECIP) -> Sums:
        """The sums of a chunk the last sieve_all left on its device, or (my_num=None)
        of all its chunks: the per-chunk results merged in order."""
        return self._result(Sums, "dse_sums_resident", my_num or 0, require, forbid, flags)

    def sums_window(self, lo: int, hi: int, require: int = 1, forbid: int = 0,
                    flags: int = _dse.SUMS_POWER | _dse.SUMS_RECIP) -> Sums:
        """The sums over the matches whose lowest member is an odd value in
        [max(lo, 3), hi] (primes_window's convention); an empty window gives the
        empty result."""
        return self.sums_range(*self._window(lo, hi), require, forbid, flags)

    # -- constellations as numbers -------------------------------------------------
    def tuples_dev_async(self, g_start: int, nbits: int, mask_ptr: int, require: int, forbid: int, above_ptr: int,
                         above_shift: int, above_bits: int, first: int, out_ptr: int, out_cap: int, totals_ptr: int,
                         stream_ptr: int = 0):
        """The positions of the device mask at which (require, forbid) matches, as
        uint64 values 3 + 2 (g_start + position) in device memory; the above_bits
        candidates behind the range are the bits from above_shift on of the device
        bit string at above_ptr (include/dse.h dse_tuples_dev_async): out[i] = the
        match of rank first + i; totals[0] = matches of the range, totals[1] = written."""
        check(lib().dse_tuples_dev_async(self.ptr, g_start, nbits, mask_ptr or None, require, forbid,
                                         above_ptr or None, above_shift, above_bits, first, out_ptr or None, out_cap,
                                         totals_ptr, stream_ptr or None),
              "dse_tuples_dev_async")

    def tuples_range(self, g_start: int, nbits: int, require: int, forbid: int = 0, first: int = 0,
                     count: Optional[int] = None) -> np.ndarray:
        """gen-table + sieve-e of an odd-index range (and of the 31 candidates above
        it) and the lowest members of its matches of (require, forbid), extracted
        on the device: ranks [first, first + count) (count=None: all from `first`)."""
        L = lib()
        return self._primes("dse_tuples_range",
                            lambda f, o, c, t, w: L.dse_tuples_range(self.ptr, g_start, nbits, require, forbid,
                                                                     f, o, c, t, w),
                            first, count)

    def resident_tuples(self, require: int, forbid: int = 0, my_num: Optional[int] = None, first: int = 0,
                        count: Optional[int] = None) -> np.ndarray:
        """The same for a chunk the last sieve_all left on its device (it sees the
        head of the chunk after it), or (my_num=None) for all its chunks as one range."""
        L = lib()
        k = 0 if my_num is None else my_num
        return self._primes("dse_tuples_resident",
                            lambda f, o, c, t, w: L.dse_tuples_resident(self.ptr, k, require, forbid, f, o, c, t, w),
                            first, count)

    def tuples_window(self, lo: int, hi: int, require: int, forbid: int = 0) -> np.ndarray:
        """The matches whose lowest member lies in the odd values of [max(lo, 3), hi]
        (primes_window's convention); the other members may lie above hi."""
        g, n = self._window(lo, hi)
        return self.tuples_range(g, n, require, forbid) if n else np.empty(0, dtype=np.uint64)


    # -- additive questions -------------------------------------------------------
    def goldbach_dev_async(self, g_start: int, nbits: int, mask_ptr: int, below_ptr: int, below_shift: int,
                           below_bits: int, nprimes: int, out_ptr: int, stream_ptr: int = 0):
        """The minimal Goldbach partitions of a device mask as one dse_goldbach
        (_dse.GOLDBACH_WORDS uint64 words) in device memory at out_ptr; the
        below_bits candidates below g_start are the bits from below_shift on of
        the device bit string at below_ptr (include/dse.h dse_goldbach_dev_async)."""
        check(lib().dse_goldbach_dev_async(self.ptr, g_start, nbits, mask_ptr or None, below_ptr or None, below_shift,
                                           below_bits, nprimes, out_ptr or None, stream_ptr or None),
              "dse_goldbach_dev_async")

    def goldbach_range(self, g_start: int, nbits: int, nprimes: int = 0) -> Goldbach:
        """gen-table + sieve-e of an odd-index range (and of what the small primes
        reach below it) and the minimal Goldbach partitions of its evens 6 + 2c,
        computed on the device: only the dse_goldbach reaches the host."""
        return self._result(Goldbach, "dse_goldbach_range", g_start, nbits, nprimes)

    def goldbach_window(self, lo: int, hi: int, nprimes: int = 0) -> Goldbach:
        """The minimal Goldbach partitions of the evens in [max(lo, 6), hi]; an
        empty window gives the empty result."""
        return self.goldbach_range(*self._window(lo, hi, base=6), nprimes)

    def resident_goldbach(self, my_num: Optional[int] = None, nprimes: int = 0) -> Goldbach:
        """The minimal Goldbach partitions of a chunk the last sieve_all left on
        its device (it sees the tail of the chunk before it), or (my_num=None) of
        all its chunks: the per-chunk results merged in order."""
        return self._result(Goldbach, "dse_goldbach_resident", my_num or 0, nprimes)

    # -- residue classes and races -------------------------------------------------
    def race_dev_async(self, g_start: int, nbits: int, mask_ptr: int, q: int, a: int, b: int, d_start: int,
                       out_ptr: int, stream_ptr: int = 0):
        """The class counts mod q and the race of class a against class b of a device
        mask as one dse_race (_dse.RACE_WORDS uint64 words) in device memory at
        out_ptr (include/dse.h dse_race_dev_async)."""
        check(lib().dse_race_dev_async(self.ptr, g_start, nbits, mask_ptr or None, q, a, b, d_start, out_ptr or None,
                                       stream_ptr or None), "dse_race_dev_async")

    def race_range(self, g_start: int, nbits: int, q: int, a: int, b: int, d_start: int = 0) -> Race:
        """gen-table + sieve-e of an odd-index range and its class counts and race,
        computed on the device: only the dse_race reaches the host."""
        return self._result(Race, "dse_race_range", g_start, nbits, q, a, b, d_start)

    def race_window(self, lo: int, hi: int, q: int, a: int, b: int, d_start: int = 0) -> Race:
        """The class counts and race of the odd values in [max(lo, 3), hi]
        (primes_window's convention); an empty window gives the empty result."""
        return self.race_range(*self._window(lo, hi), q, a, b, d_start)

    def resident_race(self, my_num: Optional[int] = None, q: int = 4, a: int = 1, b: int = 3,
                      d_start: int = 0) -> Race:
        """The class counts and race of a chunk the last sieve_all left on its
        device, or (my_num=None) of all its chunks as one range: every chunk starts
        from the d_end of the one before it, and the results are merged in order."""
        return self._result(Race, "dse_race_resident", my_num or 0, q, a, b, d_start)

    # -- rank and select ---------------------------------------------------------
    def query_index_dev_async(self, g_start: int, nbits: int, mask_ptr: int, index_ptr: int, index_bytes: int,
                              stream_ptr: int = 0):
        """The rank index of a device mask into query_index_bytes(nbits) bytes of
        device memory (include/dse.h dse_query_index_dev_async): index[t] = entries
        in the tiles before t, index[tiles] = the total."""
        check(lib().dse_query_index_dev_async(self.ptr, g_start, nbits, mask_ptr or None, index_ptr or None,
                                              index_bytes, stream_ptr or None),
              "dse_query_index_dev_async")

    def query_dev_async(self, kind: int, g_start: int, nbits: int, mask_ptr: int, index_ptr: int, q_ptr: int,
                        nq: int, out_ptr: int, stream_ptr: int = 0):
        """out[i] = the answer of QUERY_* `kind` to q[i], all in device memory
        (include/dse.h dse_query_dev_async)."""
        check(lib().dse_query_dev_async(self.ptr, kind, g_start, nbits, mask_ptr or None, index_ptr or None,
                                        q_ptr or None, nq, out_ptr or None, stream_ptr or None),
              "dse_query_dev_async")

    def query_range(self, kind: int, g_start: int, nbits: int, q) -> np.ndarray:
        """gen-table + sieve-e of an odd-index range, its rank index and the
        answers of `kind` to the queries q, computed on the device."""
        qa, out = _queries(q)
        check(lib().dse_query_range(self.ptr, kind, g_start, nbits, u64p(qa) if len(qa) else None, len(qa),
                                    u64p(out) if len(qa) else None), "dse_query_range")
        return out

    def resident_query(self, kind: int, q, my_num: Optional[int] = None) -> np.ndarray:
        """The answers of `kind` to the queries q from a chunk the last sieve_all
        left on its device, or (my_num=None) from all its chunks as the one
        range [3, 3 + 2 P cs): only queries and answers cross to the host."""
        qa, out = _queries(q)
        check(lib().dse_query_resident(self.ptr, 0 if my_num is None else my_num, kind,
                                       u64p(qa) if len(qa) else None, len(qa), u64p(out) if len(qa) else None),
              "dse_query_resident")
        return out

    # What the run left by sieve_all knows about the primes, the prime 2 counted:
    # each takes one integer or an array of them and answers in kind. The masks
    # cover the odd values up to `bound` = 3 + 2 P cs - 2, so every integer up to
    # bound + 1 (an even number) is known; a question that needs a value above
    # that raises ValueError and names the first such query.
    def _covered(self):
        """-> (last covered value 3 + 2 P cs - 2, pi_ref) of the last sieve_all"""
        if self._run is None:
            raise ValueError("no sieve_all run is resident in this context")
        _, P, cs, pi_ref = self._run
        return 1 + 2 * P * cs, pi_ref

    @staticmethod
    def _ints(x, what: str):
        """-> (Python ints, x was a scalar); every one in 0 .. 2^64 - 1"""
        scalar = np.ndim(x) == 0
        vals = [int(v) for v in np.atleast_1d(np.asarray(x, dtype=object)).ravel()]
        for v in vals:
            if v < 0 or v >= 1 << 64:
                raise ValueError(f"{what}({v}): outside 0 .. 2^64 - 1")
        return vals, scalar

    def _ask(self, kind: int, vals) -> List[int]:
        return [int(v) for v in self.resident_query(kind, np.array(vals, dtype=np.uint64))]

    def prime_pi(self, x):
        """The number of primes <= x, from the resident masks."""
        bound, _ = self._covered()
        vals, scalar = self._ints(x, "prime_pi")
        for v in vals:
            if v > bound + 1:
                raise ValueError(f"prime_pi({v}): the resident masks cover the values up to {bound}")
        got = [r + (v >= 2) for r, v in zip(self._ask(QUERY_RANK, vals), vals)]
        return got[0] if scalar else np.array(got, dtype=np.uint64)

    def nth_prime(self, n):
        """The n-th prime, 1-based: nth_prime(1) == 2."""
        bound, pi_ref = self._covered()
        vals, scalar = self._ints(n, "nth_prime")
        for v in vals:
            if v < 1:
                raise ValueError("nth_prime(0): ranks start at 1")
            if v > pi_ref:
                raise ValueError(f"nth_prime({v}): the resident masks hold the first {pi_ref} primes (up to {bound})")
        got = self._ask(QUERY_SELECT, [max(v, 2) - 2 for v in vals])
        got = [2 if v == 1 else g for g, v in zip(got, vals)]
        return got[0] if scalar else np.array(got, dtype=np.uint64)

    def next_prime(self, x):
        """The smallest prime > x."""
        bound, _ = self._covered()
        vals, scalar = self._ints(x, "next_prime")
        got = [2 if v < 2 else g for g, v in zip(self._ask(QUERY_NEXT, vals), vals)]
        for g, v in zip(got, vals):
            if g == QUERY_NONE:
                raise ValueError(f"next_prime({v}): no prime above it among the covered values up to {bound}")
        return got[0] if scalar else np.array(got, dtype=np.uint64)

    def prev_prime(self, x):
        """The largest prime < x; None for x <= 2 (in an array: 0)."""
        bound, _ = self._covered()
        vals, scalar = self._ints(x, "prev_prime")
        for v in vals:
            if v > bound + 2:  # bound + 1 is even: every value below bound + 2 is covered
                raise ValueError(f"prev_prime({v}): the resident masks cover the values up to {bound}")
        got = [(None if v <= 2 else 2) if g == QUERY_NONE else g for g, v in zip(self._ask(QUERY_PREV, vals), vals)]
        return got[0] if scalar else np.array([g or 0 for g in got], dtype=np.uint64)

    def is_prime(self, x):
        """Whether x is prime."""
        bound, _ = self._covered()
        vals, scalar = self._ints(x, "is_prime")
        for v in vals:
            if v > bound + 1:
                raise ValueError(f"is_prime({v}): the resident masks cover the values up to {bound}")
        got = [bool(t) or v == 2 for t, v in zip(self._ask(QUERY_TEST, vals), vals)]
        return got[0] if scalar else np.array(got, dtype=bool)


# include/dse.h DSE_QUERY_*
QUERY_NONE = _dse.QUERY_NONE
QUERY_RANK, QUERY_SELECT, QUERY_NEXT, QUERY_PREV, QUERY_TEST = (_dse.QUERY_RANK, _dse.QUERY_SELECT, _dse.QUERY_NEXT,
                                                                _dse.QUERY_PREV, _dse.QUERY_TEST)


def _queries(q):
    """-> (the queries as a contiguous uint64 array, an answer array of the same length)"""
    if not (isinstance(q, np.ndarray) and q.dtype == np.uint64):
        q = np.asarray(q, dtype=object).astype(np.uint64)  # Python integers up to 2^64 - 1, exactly
    qa = np.ascontiguousarray(np.atleast_1d(q)).ravel()
    return qa, np.empty(len(qa), dtype=np.uint64)


def query_index_bytes(nbits: int) -> int:
    """Bytes of the rank index of a range of nbits candidates."""
    return int(lib().dse_query_index_bytes(nbits))


def query_host(mask: np.ndarray, g_start: int, nbits: int, kind: int, q) -> np.ndarray:
    """Test-only: the query kernel's per-word and per-tile bodies run on the host
    over a host mask (include/dse.h dse_debug_query_host)."""
    qa, out = _queries(q)
    m = np.ascontiguousarray(mask, dtype=np.uint64)
    check(lib().dse_debug_query_host(u64p(m) if len(m) else None, g_start, nbits, kind,
                                     u64p(qa) if len(qa) else None, len(qa), u64p(out) if len(qa) else None),
          "dse_debug_query_host")
    return out


def base_table_bytes(limit: int) -> int:
    return int(lib().dse_base_table_bytes(limit))


def base_table_prime_bytes(limit: int) -> int:
    """Leading bytes of a base table that hold the primes: what ranks broadcast."""
    return int(lib().dse_base_table_prime_bytes(limit))


def base_table_broadcast_bytes(limit: int) -> int:
    """Bytes rank 0 broadcasts for a table of odd primes <= limit, or 0 when
    every rank builds its own table (include/dse.h dse_base_table_broadcast_bytes:
    the primes move while they fit in 8 MiB; the 1e18 window's 203 MB are
    rebuilt on every device, which is faster than moving them)."""
    return int(lib().dse_base_table_broadcast_bytes(limit))


def base_limit_for_range(g_start: int, nbits: int) -> int:
    return int(lib().dse_base_limit_for_range(g_start, nbits))


# include/dse.h DSE_FINISH_*
FINISH_DOUBLES, FINISH_HACK, FINISH_LAST = 1, 2, 4


def finish_text_bound(g_start: int, nbits: int, count: int, flags: int = 0) -> int:
    """Rigorous upper bound on the text bytes of ``count`` entries of the range."""
    return int(lib().dse_finish_text_bound(g_start, nbits, count, flags))


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(num_gpus=1)
    return _default_ctx


def _spread(n: int, P: int):
    lo_hi = np.zeros(2 * P, dtype=np.int64)
    cs = ctypes.c_int64()
    check(lib().dse_spread_work(n, P, lo_hi.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                ctypes.byref(cs)), "dse_spread_work")
    return cs.value, [[int(lo_hi[2 * k]), int(lo_hi[2 * k + 1])] for k in range(P)]


def spread_work(n: int, num_comps: int) -> List[List[int]]:
    """sieve.clj:15-34: P equal chunks [lo, hi) of the odd numbers from 3,
    cs = floor(floor((n-1)/2)/P); the remainder is dropped. Exact integers
    (the reference computes Doubles, identical below 2^53)."""
    return _spread(n, num_comps)[1]


def tail_range(n: int, P: int):
    """Odd indices [g, g+len) that spread-work drops (len <= P-1)."""
    g, nb = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().dse_tail_range(n, P, ctypes.byref(g), ctypes.byref(nb)), "dse_tail_range")
    return g.value, nb.value


@dataclass
class Chunk:
    """gen-table's result (sieve.clj:9-13): the odd numbers in [lower, upper).

    ``mask`` (after sieve_e) holds bit j = 1 iff element j (value lower+2j)
    is still non-zero, i.e. prime."""

    lower: int
    upper: int
    mask: Optional[np.ndarray] = None
    n_primes: Optional[int] = None

    @property
    def cs(self) -> int:  # (count chunk), sieve.clj:128
        return len(range(self.lower, self.upper, 2))

    @property
    def g_start(self) -> int:
        return (self.lower - 3) // 2

    def primes(self) -> np.ndarray:
        """Non-zero elements of the chunk in order (before finish's hack)."""
        if self.mask is None:
            raise ValueError("chunk not sieved")
        bits = np.unpackbits(self.mask.view(np.uint8), bitorder="little")[: self.cs]
        return (self.lower + 2 * np.flatnonzero(bits)).astype(np.int64)


def gen_table(bounds: Sequence[int]) -> Chunk:
    """sieve.clj:9-13: [lower upper] -> the chunk of odd values in [lower, upper)."""
    lower, upper = int(bounds[0]), int(bounds[1])
    if lower < 3 or lower % 2 == 0:
        raise ValueError("chunks start at an odd number >= 3 (spread-work bounds)")
    return Chunk(lower, upper)


def finish(raw_chunk: Chunk, my_num: int, *, path: Optional[str] = None) -> str:
    """sieve.clj:82-108: write the chunk's primes to user.home/primes{my_num}.txt
    (chunk 1 as Doubles with the 2/3/5/7 hack), 10 per line, ", "-joined."""
    if raw_chunk.mask is None:
        raise ValueError("chunk not sieved")
    if path is None:
        path = os.path.join(os.path.expanduser("~"), f"primes{my_num}.txt")
    mask = np.ascontiguousarray(raw_chunk.mask, dtype=np.uint64)
    check(lib().dse_write_range_file(path.encode(), my_num, raw_chunk.g_start, raw_chunk.cs, u64p(mask)),
          "dse_write_range_file")
    return path


def sieve_e(my_num: int, lead: bool, in_channel, chunk: Chunk, out_channel, *,
            ctx: Optional[Context] = None, write_file: bool = True, path: Optional[str] = None,
            gpu_finish: bool = False) -> Chunk:
    """sieve.clj:118-172: sieve this machine's chunk, then finish it.

    The reference marks the chunk prime by prime, receiving earlier chunks'
    primes on ``in_channel`` and reporting its own on ``out_channel``. Here the
    chunk is sieved in one pass on a GPU with the base primes <= sqrt(upper)
    computed on the device, so the channels carry nothing; they are accepted
    for call compatibility. ``lead`` likewise no longer orders the work.

    ``gpu_finish``: write the file with Context.finish_range (the text is
    formatted on the device) instead of the host writer; same bytes."""
    del lead, in_channel, out_channel
    ctx = ctx or default_context()
    if chunk.cs < 1:
        raise ValueError("empty chunk (find-first-prime would throw)")
    chunk.mask, chunk.n_primes = ctx.sieve_odd_range(chunk.g_start, chunk.cs, want_mask=True)
    if write_file and gpu_finish:
        if path is None:
            path = os.path.join(os.path.expanduser("~"), f"primes{my_num}.txt")
        ctx.finish_range(path, my_num, chunk.g_start, chunk.cs)
    elif write_file:
        finish(chunk, my_num, path=path)
    return chunk
