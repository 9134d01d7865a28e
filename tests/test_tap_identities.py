"""The two bit identities the wavetable taps rest on (audiality2_amd/csrc/a2amd_taps.h), checked in numpy.

hermite_step(): a2_Hermite's Horner step, (v * (frac << 7) wrapped to 32 bits) >> 15, is bits 8..24 of the exact
product v * frac, sign extended - what a 24 bit multiply and a signed bit-field extract (offset 8, width 17) return.
tap_phase(): (lo + ldph) >> 16 is the upper 16 bit word of the 32 bit sum, zero extended."""
import numpy as np


def wrap32(x):
    """int64 -> the value of its low 32 bits as a signed 32 bit integer"""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def sbfe(x, offset, width):
    """signed bit-field extract of the low 32 bits of x (v_bfe_i32)"""
    f = (x >> offset) & ((1 << width) - 1)
    return f - ((f >> (width - 1)) << width)


def mul24(v, b):
    """v_mul_i32_i24: the low 32 bits of the product of the operands' low 24 bits, sign extended"""
    return wrap32(sbfe(v, 0, 24) * sbfe(b, 0, 24))


def test_hermite_step_is_bits_8_to_24_of_the_24_bit_product():
    # every operand the kernels can have is below 2^19 in magnitude (a2amd_taps.h); the identity needs |v| < 2^23
    v = np.arange(-(1 << 19), (1 << 19) + 1, dtype=np.int64)
    v24 = sbfe(v, 0, 24)                                    # (what the 24 bit multiplier sees of v)
    for frac in range(256):
        want = wrap32(v * (frac << 7)) >> 15
        got = sbfe(wrap32(v24 * frac), 8, 17)
        assert np.array_equal(got, want), frac
    # ... and at the edge of the 24 bit multiplier's range
    edge = np.array([-(1 << 23), -(1 << 23) + 1, (1 << 23) - 1], dtype=np.int64)
    for frac in (0, 1, 127, 128, 255):
        assert np.array_equal(sbfe(mul24(edge, np.int64(frac)), 8, 17), wrap32(edge * (frac << 7)) >> 15)


def test_the_multiply_reads_the_fraction_as_the_low_byte_of_the_phase():
    # SDWA BYTE_0, zero extended: whatever the phase holds above its low byte does not reach the product
    rng = np.random.default_rng(1)
    ph = rng.integers(0, 1 << 32, 4096, dtype=np.int64)
    v = rng.integers(-(1 << 19), 1 << 19, 4096, dtype=np.int64)
    assert np.array_equal(sbfe(mul24(v, ph & 0xFF), 8, 17), wrap32(v * ((ph & 0xFF) << 7)) >> 15)


def test_tap_phase_carry_is_the_upper_word_of_the_sum():
    rng = np.random.default_rng(2)
    ldph = np.concatenate([np.array([0, 1, (1 << 16) - 1, 1 << 16, (1 << 31) - (1 << 16)], dtype=np.int64),
                           rng.integers(0, 1 << 31, 4000, dtype=np.int64)])
    lo = np.arange(1 << 16, dtype=np.int64)
    for d in ldph:
        s = lo + d
        assert int(s.max()) < (1 << 32)                     # the 32 bit add does not wrap
        word1 = (s & 0xFFFFFFFF).astype(np.uint32).view(np.uint16).reshape(-1, 2)[:, 1]     # (little endian: WORD_1)
        assert np.array_equal(word1.astype(np.int64), s >> 16), int(d)
