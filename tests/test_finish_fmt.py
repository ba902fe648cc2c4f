"""The device finish's per-value formatter and text bound, on the CPU.

dse_debug_finish_format runs the emit kernel's own __host__ __device__
formatter (csrc/dse_finish_fmt.h) on the host; it is compared against a Python
restatement of Long printing and of Double.toString for integer-valued
doubles. dse_finish_text_bound is compared against the host writer's files.
"""
import ctypes
import os

import numpy as np
import pytest

DOUBLES, HACK, LAST = 1, 2, 4


def fmt(v, flags):
    from mail_sieve_e import _dse
    out = ctypes.create_string_buffer(32)
    n = _dse.lib().dse_debug_finish_format(v, flags, out)
    assert 0 < n <= 24, (v, flags, n)
    return out.raw[:n].decode()


def want_long(v):
    return str(v)


def want_double(v):
    if v < 10**7:
        return f"{v}.0"
    s = str(v)
    frac = s[1:].rstrip("0") or "0"
    return s[0] + "." + frac + "E" + str(len(s) - 1)


def values():
    vs = list(range(1, 100))
    for k in range(1, 19):
        for d in (1, 3, 7, 9):
            vs += [10**k - d, 10**k + d]
    vs += [10**7 - 1, 10**7 + 1, 2**53 - 1]
    # even values: the trailing-zero trim of the E form
    vs += [10**7, 12 * 10**8, 10**9, 10**10, 10**15, 123_000_000, 1_000_000_010, 5 * 10**15, 10**18,
           123456789 * 10**9, 9_007_199_254_740_990]
    return vs


def test_long_printing():
    for v in values() + [2**63 - 1, 2**63 + 1, 10**19 - 1, 10**19 + 1, 2**64 - 1]:
        assert fmt(v, 0) == want_long(v), v


def test_double_printing():
    for v in values():
        if v < 2**53:
            assert fmt(v, DOUBLES) == want_double(v), v
    assert fmt(10**7, DOUBLES) == "1.0E7"
    assert fmt(12 * 10**8, DOUBLES) == "1.2E9"
    assert fmt(10_000_019, DOUBLES) == "1.0000019E7"
    assert fmt(10**10 + 1, DOUBLES) == "1.0000000001E10"


def test_random_values_both_printings():
    rng = np.random.default_rng(7)
    for bits in range(1, 64):
        for v in rng.integers(1 << (bits - 1), 1 << bits, size=40, dtype=np.uint64):
            v = int(v)
            assert fmt(v, 0) == want_long(v), v
            if v < 2**53:
                assert fmt(v, DOUBLES) == want_double(v), v


def test_format_rejects_other_flags():
    from mail_sieve_e import _dse
    out = ctypes.create_string_buffer(32)
    assert _dse.lib().dse_debug_finish_format(5, HACK, out) == -1
    assert _dse.lib().dse_debug_finish_format(5, 0, None) == -1


@pytest.mark.parametrize("N,P", [(10_000, 2), (10**6, 3)])
def test_text_bound_covers_the_host_writers_files(oracle, tmp_path, N, P):
    from mail_sieve_e import _dse
    from mail_sieve_e import sieve as S
    cs, masks, counts, _ = oracle.sieve(N, P)
    for k in range(1, P + 1):
        p = tmp_path / f"primes{k}.txt"
        _dse.check(_dse.lib().dse_write_primes_file(str(p).encode(), k, N, P, _dse.u64p(masks[k - 1])), "write")
        size = os.path.getsize(p)
        flags = (DOUBLES | HACK if k == 1 else 0) | LAST
        entries = int(np.unpackbits(masks[k - 1].view(np.uint8), bitorder="little")[4 if k == 1 else 0:cs].sum())
        entries += 4 if k == 1 else 0
        bound = S.finish_text_bound((k - 1) * cs, cs, entries, flags)
        assert size <= bound <= 2 * size + 16, (k, size, bound)


def test_text_bound_is_monotone_in_count():
    from mail_sieve_e import sieve as S
    for flags in (0, DOUBLES, DOUBLES | HACK | LAST):
        for g, nb in ((0, 10**6), (5 * 10**7, 2 * 10**6), ((10**18 - 3) // 2, 10**6)):
            if flags & DOUBLES and 3 + 2 * (g + nb) >= 2**53:
                continue
            prev = 0
            for c in list(range(0, 200)) + [10**3, 10**6, 10**9, 2**40, 2**60, 2**62]:
                b = S.finish_text_bound(g, nb, c, flags)
                assert b >= prev, (flags, g, c)
                prev = b
            # every entry costs at least its separator and one digit
            assert S.finish_text_bound(g, nb, 1000, flags) >= 3000
