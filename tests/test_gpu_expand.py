"""The wheel kernel's expand phase on the device: masks and counts against the
oracle for every variant (V0 mod 30) of the register block transform
(csrc/dse_expand_bits.h) in both segment geometries, the range's first block,
ranges of different variants pooled into one launch, and a bucketed range."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEG = 15 * 2**17  # output bits of a full segment


@pytest.mark.parametrize("geometry", [1, 2])
def test_every_variant_vs_oracle(oracle, geometry):
    """g0 = 1e9 + r, r = 0..14: V0 = 2 + 2 g0 takes every even residue mod 30,
    so every variant runs; one full segment, a ragged second one, and an end
    inside a block and inside a word."""
    from mail_sieve_e import sieve as S
    nb = SEG + 4096 * 3 + 37
    seen = set()
    with S.Context(num_gpus=1) as c:
        c.debug_set_option("wheel_geometry", geometry)
        for r in range(15):
            g0 = 10**9 + r
            seen.add((2 + 2 * g0) % 30 // 2)
            m_ref, c_ref = oracle.fast_sieve_range(g0, nb)
            m, cnt = c.sieve_odd_range(g0, nb)
            assert cnt == c_ref, (geometry, r)
            assert np.array_equal(m, m_ref), (geometry, r)
    assert seen == set(range(15))


@pytest.mark.parametrize("nb", [1, 479, 480, 481])
def test_first_block(ctx, oracle, nb):
    """g0 = 0: the small primes put back by the range's fix bits, the count
    taken from the output words, and an end inside the first block."""
    m_ref, c_ref = oracle.fast_sieve_range(0, nb)
    m, cnt = ctx.sieve_odd_range(0, nb)
    assert cnt == c_ref and np.array_equal(m, m_ref), nb


def test_pooled_ranges_of_different_variants(ctx, oracle):
    """N = 30,000,011, P = 7: cs = 2,142,857 = 2 (mod 15), so the seven chunks
    of the one launch start in seven different variants."""
    N, P = 30_000_011, 7
    cs, m_ref, c_ref, _ = oracle.sieve(N, P)
    assert cs == 2_142_857 and len({(1 + k * cs) % 15 for k in range(P)}) == P
    counts, _, _ = ctx.sieve_all(N, P)
    assert [int(x) for x in counts] == [int(x) for x in c_ref]
    for k in range(1, P + 1):
        assert np.array_equal(ctx.copy_chunk_mask(N, P, k), m_ref[k - 1]), k


def test_bucketed_range(oracle):
    """A range at 1e13 (base primes above 2^20: the bucketed instantiation of
    the kernel) in passes of 3 segments."""
    from mail_sieve_e import sieve as S
    g0, nb = (10**13 + 1 - 3) // 2, 7 * SEG + 12345
    m_ref, c_ref = oracle.fast_sieve_range(g0, nb)
    with S.Context(num_gpus=1) as c:
        c.debug_set_option("bucket_pass_segments", 3)
        m, cnt = c.sieve_odd_range(g0, nb)
        assert cnt == c_ref and np.array_equal(m, m_ref)
