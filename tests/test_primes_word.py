"""The prime-value extractor's per-word body, on the CPU.

dse_debug_primes_word runs the emit kernel's own __host__ __device__ body
(csrc/dse_primes_word.h) on the host. It is compared against a numpy model on
the same bits: the word's values 3 + 2 (g + flatnonzero(bits)) have the ranks
rank0, rank0 + 1, ..., and those with first <= rank < first + cap come out, in
order. The header must declare the new entry points and libdse.so export them.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_primes_dev_async", "dse_primes_range", "dse_primes_resident", "dse_debug_primes_word")
M64 = (1 << 64) - 1


def test_header_declares_and_library_exports_the_entry_points():
    from mail_sieve_e import _dse
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dse.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dse_[a-z0-9_]+)\s*\(", txt))
    L = _dse.lib()
    for s in NEW:
        assert s in declared, f"include/dse.h does not declare {s}"
        assert hasattr(L, s), f"libdse.so does not export {s}"
        assert s in _dse.SIGNATURES, f"ctypes binding misses {s}"
    assert "primes_slab_entries" in open(os.path.join(ROOT, "include", "dse.h")).read()


def word_values(word, g, rank0, first, cap):
    from mail_sieve_e import _dse
    out = (ctypes.c_uint64 * 64)(*([0xA5A5A5A5A5A5A5A5] * 64))
    n = _dse.lib().dse_debug_primes_word(word, g, rank0, first, cap, out)
    assert 0 <= n <= 64, (word, g, rank0, first, cap, n)
    assert all(v == 0xA5A5A5A5A5A5A5A5 for v in out[n:]), "wrote past the values it reports"
    return [int(v) for v in out[:n]]


def model(word, g, rank0, first, cap):
    bits = np.unpackbits(np.array([word], dtype=np.uint64).view(np.uint8), bitorder="little")
    vals = [3 + 2 * (g + int(b)) for b in np.flatnonzero(bits)]  # Python integers: no wrap
    a = max(first - rank0, 0)
    b = max(min(first + cap, 1 << 64) - rank0, 0)
    return vals[a:b]


def windows(rank0, c):
    """(first, cap) pairs that cut before, inside and after a word of c entries at rank0."""
    out = [(0, 0), (0, M64), (rank0, c), (rank0, 0), (rank0 + c, 5), (rank0 + c + 3, 5), (0, rank0), (0, rank0 + 1),
           (rank0 + c - 1 if c else rank0, 1), (rank0 + c - 1 if c else rank0, 2**40), (rank0 + 1, M64), (M64, M64)]
    if rank0:
        out += [(rank0 - 1, 1), (rank0 - 1, 2), (rank0 - 1, c + 2), (0, rank0 + c // 2)]
    for a in range(0, c + 1, max(c // 5, 1)):
        for n in (1, 2, c // 3, c):
            out.append((rank0 + a, n))
    return out


def check_word(word, g, rank0):
    c = bin(word).count("1")
    for first, cap in windows(rank0, c):
        assert word_values(word, g, rank0, first, cap) == model(word, g, rank0, first, cap), \
            (hex(word), g, rank0, first, cap)


def test_random_words():
    rng = np.random.default_rng(0x9121)
    for i in range(60):
        word = int(rng.integers(0, 1 << 63, dtype=np.uint64)) << 1 | int(rng.integers(0, 2))
        if i % 3 == 1:  # sparse, like a prime mask
            word &= int(rng.integers(0, 1 << 63, dtype=np.uint64)) & int(rng.integers(0, 1 << 63, dtype=np.uint64))
        g = int(rng.integers(0, 1 << 40)) * 64
        check_word(word, g, int(rng.integers(0, 1 << 30)) if i % 2 else 0)


@pytest.mark.parametrize("word", [0, M64, 1, 1 << 63, (1 << 63) | 1], ids=hex)
def test_edge_words(word):
    for g, rank0 in ((0, 0), (640, 17), (10**12 * 64, 2**40 + 3)):
        check_word(word, g, rank0)


def test_values_cross_2_32_inside_the_word():
    # 3 + 2 (g + b) = 2^32 + 1 at g + b = 2^31 - 1: bit 31, bit 1 and bit 63 of three words
    for g in (2**31 - 32, 2**31 - 2, 2**31 - 64):
        vals = word_values(M64, g, 0, 0, M64)
        assert vals[0] < 2**32 < vals[-1]
        check_word(M64, g, 5)
        check_word(0x8000_0001_8000_0001, g, 0)


def test_top_of_range():
    g = 2**61 - 1 - 64  # the word's bit 63 is odd index 2^61 - 2: value 2^62 - 1
    assert word_values(1 << 63, g, 0, 0, 1) == [2**62 - 1]
    assert word_values(M64, g, 0, 0, M64)[-1] == 2**62 - 1
    check_word(M64, g, 0)
    check_word(0xDEADBEEF_12345678, g, 2**44)


def test_refusals():
    from mail_sieve_e import _dse
    L = _dse.lib()
    out = (ctypes.c_uint64 * 64)()
    assert L.dse_debug_primes_word(1, 0, 0, 0, 1, None) == -1
    assert L.dse_debug_primes_word(1, 2**62, 0, 0, 1, out) == -6
    assert L.dse_debug_primes_word(1, 0, 2**62 + 1, 0, 1, out) == -6
    assert _dse.PRIMES_TILE_BITS % 64 == 0
