"""The operands of the shift-product tests (tests/test_shift_q1_host.py, tests/test_shift_q1_gpu.py): for every exponent E in 33 .. 63
(r = E - 32) the words 0, 1, p - 1, p, p + 1, 2^64 - 1, the words m 2^(64 - r) for m = 1, 2, 2^r - 1 -- x 2^r then has nothing in its
two low 32-bit words, the only case in which Goldilocks::mad_eps_less_eps takes its second + p -- their neighbours +- 1, and 10^4
seeded uniform 64-bit words.  Any 64-bit word is a legal operand of gl::mul_pow2."""
import random

P = (1 << 64) - (1 << 32) + 1
M64 = 1 << 64
EXPONENTS = range(33, 64)
RANDOM_WORDS = 10_000


def repair_words(e):
    """m 2^(64 - r), m = 1, 2, 2^r - 1, modulo 2^64 (m = 2 at r = 1 is the word 0)"""
    r = e - 32
    return [(m << (64 - r)) % M64 for m in (1, 2, (1 << r) - 1)]


def words(e):
    rep = repair_words(e)
    fixed = [0, 1, P - 1, P, P + 1, M64 - 1] + rep + [(x + 1) % M64 for x in rep] + [(x - 1) % M64 for x in rep]
    rng = random.Random(0x5F1 + e)
    return fixed + [rng.getrandbits(64) for _ in range(RANDOM_WORDS)]
