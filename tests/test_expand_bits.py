"""The expand phase's block transform (csrc/dse_expand_bits.h) through its
host entry dse_debug_expand_block, against the definition: output bit
15 k + slot_i is set exactly when bit k of plane i is clear, slot_i the i-th
smallest of ((r - 1)/2 - variant) mod 15 over the residues r coprime to 30.
No GPU call."""
import ctypes

import numpy as np
import pytest

R30 = (1, 7, 11, 13, 17, 19, 23, 29)
_U32P = ctypes.POINTER(ctypes.c_uint32)


def _slots(variant):
    return sorted(((r - 1) // 2 - variant) % 15 for r in R30)


def _expand(variant, planes):
    from mail_sieve_e import _dse
    p = np.ascontiguousarray(planes, dtype=np.uint32)
    out = np.full(15, 0xDEADBEEF, dtype=np.uint32)
    rc = _dse.lib().dse_debug_expand_block(variant, p.ctypes.data_as(_U32P), out.ctypes.data_as(_U32P))
    return rc, out


def _definition(variant, planes):
    """planes: (n, 8) uint32 -> (n, 15) uint32."""
    planes = np.asarray(planes, dtype=np.uint32)
    n = planes.shape[0]
    bits = np.zeros((n, 480), dtype=np.uint8)
    k = np.arange(32)
    for i, slot in enumerate(_slots(variant)):
        clear = ((planes[:, i, None] >> k.astype(np.uint32)) & 1) == 0  # (n, 32)
        bits[:, 15 * k + slot] = clear
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(n, 15)


def _blocks():
    rng = np.random.default_rng(0xE7BA)
    blocks = [rng.integers(0, 2**32, size=(500, 8), dtype=np.uint64).astype(np.uint32),
              np.zeros((1, 8), dtype=np.uint32), np.full((1, 8), 0xFFFFFFFF, dtype=np.uint32)]
    single = np.zeros((256, 8), dtype=np.uint32)  # one composite bit
    for i in range(8):
        for k in range(32):
            single[32 * i + k, i] = np.uint32(1) << np.uint32(k)
    blocks += [single, ~single]  # and one prime bit
    return np.concatenate(blocks)


BLOCKS = _blocks()


def test_slots_are_the_wheel_residues():
    """The slot table of the definition: for V0 = 2 variant the planes are the
    odd rho with V0 + rho coprime to 30, in ascending order."""
    from math import gcd
    for variant in range(15):
        rhos = [rho for rho in range(1, 30, 2) if gcd(2 * variant + rho, 30) == 1]
        assert [(rho - 1) // 2 for rho in rhos] == _slots(variant)


@pytest.mark.parametrize("variant", range(15))
def test_expand_block_matches_definition(variant):
    want = _definition(variant, BLOCKS)
    for planes, w in zip(BLOCKS, want):
        rc, got = _expand(variant, planes)
        assert rc == 0
        assert np.array_equal(got, w), (variant, [hex(int(x)) for x in planes])


@pytest.mark.parametrize("variant", [-1, 15])
def test_expand_block_rejects_bad_variant(variant):
    rc, out = _expand(variant, np.zeros(8, dtype=np.uint32))
    assert rc == -1  # DSE_EINVAL
    assert (out == 0xDEADBEEF).all()  # nothing written
