"""The uniform of the Philox noise (sim_device.hpp u01): the two-instruction form gives the bits of the fma form for every input.

Both compute (n + 0.5) 2^-23 with n = bits >> 9.  The old form is fma(float(n), 2^-23, 2^-24); the new one puts n under the exponent of
1.0 with v_alignbit_b32 ((0x7F:bits) >> 9 = 0x3F800000 | n) and subtracts 1 - 2^-24.  Checked here for all 2^23 values of n, with the
constant read from the header, so that the step noise, the initial draw and the dropout stream keep their bits."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "sde_sampler_lrds_amd", "csrc", "sim_device.hpp")


def _u01_source():
    text = open(HDR).read()
    m = re.search(r"float u01\(uint32_t bits\) \{ return __uint_as_float\(__builtin_amdgcn_alignbit\(0x7Fu, bits, 9\)\) - ([0-9a-fx.p+-]+)f; \}",
                  text)
    assert m, "u01() in sim_device.hpp is no longer the alignbit form this test checks"
    return np.float32(float.fromhex(m.group(1)))


def _alignbit(hi, lo, shift):
    """v_alignbit_b32: the low 32 bits of the 64-bit value hi:lo shifted right by shift (0..31)"""
    return (((np.uint64(hi) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(shift)).astype(np.uint32)


def test_u01_alignbit_form_is_bit_exact_for_every_mantissa():
    c = _u01_source()
    assert c == np.float32(1.0) - np.float32(2.0 ** -24)
    n = np.arange(1 << 23, dtype=np.uint32)
    # the old form: every step exact, so the fp64 value rounds to itself in fp32
    old = ((n.astype(np.float64) * 2.0 ** -23) + 2.0 ** -24).astype(np.float32)
    assert np.array_equal(old.astype(np.float64), (n.astype(np.float64) + 0.5) * 2.0 ** -23)
    # the new form on words whose low 9 bits are set (alignbit must drop them)
    bits = (n << np.uint32(9)) | np.uint32(0x1FF)
    one_plus = _alignbit(0x7F, bits, 9)
    assert np.array_equal(one_plus, np.uint32(0x3F800000) | n)
    new = one_plus.view(np.float32) - c  # one fp32 subtraction, rounded to nearest
    assert new.dtype == np.float32
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))
    assert new.min() > 0.0 and new.max() < 1.0
