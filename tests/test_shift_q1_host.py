"""Host form of the shift products 2^E, 32 < E < 64 (gl::mul_pow2 through Goldilocks::mad_eps_less_eps: one multiply-add whose carry
selects the lanes that are done, + p on the others, a second + p where that wrapped) against Python integers, for every exponent of
the class and ANY 64-bit operand.  The same source compiles for the device; tests/test_shift_q1_gpu.py compares the two.  CPU only."""
import ctypes

import shift_q1_words as W
from stark_rings_amd import _lib


def test_host_shift_products_of_the_middle_class_are_exact_and_canonical():
    lib = _lib.load()
    A = (ctypes.c_uint64 * 4)()
    B = (ctypes.c_uint64 * 4)()
    out = (ctypes.c_uint64 * 4)()
    repaired = 0
    for e in W.EXPONENTS:
        r = e - 32
        xs = W.words(e)
        # the words on which the second + p is taken must be among the inputs: x 2^r with two empty low words, x != 0
        rep = [x for x in W.repair_words(e) if x]
        assert rep and all(x in xs for x in rep) and all((x << r) % (1 << 64) == 0 for x in rep), e
        repaired += len(rep)
        B[0] = e
        for x in xs:
            A[0] = x
            assert lib.sr_selftest_field_op(0, 5, A, B, out) == 0, _lib.last_error()
            assert out[0] == (x << e) % W.P, (hex(x), e, hex(out[0]))
            assert out[0] < W.P
    assert repaired >= 2 * len(W.EXPONENTS)
