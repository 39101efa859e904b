"""CPU checks of the norm entry points (include/stark_rings_hip.h: sr_norm_plan, sr_norm_batch_dev, sr_norm_batch): the exports, the
plan arithmetic for every ring id, every refusal that needs no device, the absence of a CPU fallback, and the Python restatement of the
reference's norms (tools/model_norms.py, the oracle of tests/test_norms_gpu.py) on the reference's own decomposition KAT and on hand
values."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_norms as M  # noqa: E402

NEW = ("sr_norm_plan", "sr_norm_batch_dev", "sr_norm_batch")
LINF, L2SQ = 1, 2
LIMBS = {0: 1, 1: 1, 2: 4, 3: 1, 4: 1, 5: 1}
MODULUS = {0: 2**64 - 2**32 + 1, 1: 2013265921, 2: 2**251 + 17 * 2**192 + 1, 3: 2**64 - 2**32 + 1, 4: 2013265921, 5: 15912092521325583641}
WIDE_MIN = 1024          # csrc/norms.hpp kWideMin: groups below it run in one launch without a workspace
MAX_PARTS = 1 << 15      # csrc/norms.hpp kMaxParts: partial records of one call at most


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    assert re.search(r"#define\s+SR_NORM_LINF\s+1\b", header) and re.search(r"#define\s+SR_NORM_L2SQ\s+2\b", header)
    for text in ("2^190", "2^566", "NTT-form data is accepted and meaningless", "outside the contract"):
        assert text in header, "the header does not state: %s" % text
    hpp = open(os.path.join(ROOT, "include", "stark_rings.hpp")).read()
    for name in NEW:
        assert name in hpp, "include/stark_rings.hpp does not bind %s" % name


def _plan(ring, n, group, which):
    lib = _lib.load()
    wpg, work, launches = ctypes.c_size_t(1 << 60), ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_norm_plan(ring, n, group, which, ctypes.byref(wpg), ctypes.byref(work), ctypes.byref(launches))
    return rc, wpg.value, work.value, launches.value


@pytest.mark.parametrize("ring", range(6))
def test_plan_widths_launches_and_workspace_for_every_ring(ring):
    limbs = LIMBS[ring]
    lw, sw = (1, 3) if limbs == 1 else (4, 9)
    for which, wpg in ((LINF, lw), (L2SQ, sw), (LINF | L2SQ, lw + sw)):
        # narrow groups: one launch, no workspace
        for group in (1, 16, 24, 72, 3 * 64, WIDE_MIN - 1):
            for mult in (1, 3, 1 << 12):
                rc, w, work, launches = _plan(ring, group * mult, group, which)
                assert (rc, w, work, launches) == (0, wpg, 0, 1), (group, mult, which, _lib.last_error())
        # every shape: at most two launches; a single launch needs no workspace; the workspace holds at most MAX_PARTS records
        for n, group in ((1 << 10, 1 << 10), (1 << 20, 1 << 10), (1 << 20, 1 << 20), (3 << 16, 3 << 16), (3 << 20, 3 << 10), (1 << 30, 1 << 16),
                         (1 << 30, 1 << 30), (4097, 4097), (1 << 33, 1 << 33)):
            rc, w, work, launches = _plan(ring, n, group, which)
            where = "ring %d n %d group %d which %d: work %d launches %d" % (ring, n, group, which, work, launches)
            assert rc == 0 and w == wpg, where
            assert 1 <= launches <= 2, where
            assert (work == 0) == (launches == 1), where
            assert work % wpg == 0 and work // wpg <= MAX_PARTS, where
        # the whole slice: the workspace never shrinks as the slice grows
        prev = 0
        for lg in range(0, 36):
            for n in ((1 << lg) - 1, 1 << lg, (1 << lg) + 1):
                if n == 0:
                    continue
                rc, w, work, launches = _plan(ring, n, n, which)
                assert rc == 0 and work >= prev, (ring, n, which, work, prev)
                prev = work
    # the 8 GiB slice of config 2 (2^14 elements of degree 2^16, 8-byte coefficients): MAX_PARTS records of at most 4 words = 1 MiB for the
    # one-limb fields; 13 words = 3.25 MiB for the four-limb field
    rc, w, work, launches = _plan(ring, 1 << 30, 1 << 30, LINF | L2SQ)
    assert rc == 0 and launches == 2
    assert work * 8 <= MAX_PARTS * (lw + sw) * 8 <= (1 << 20 if limbs == 1 else 13 << 18), work
    # an empty slice has an l2sq (zero: one record) and no linf
    assert _plan(ring, 0, 1, L2SQ) == (0, sw, 0, 1)
    assert _plan(ring, 0, 5, L2SQ) == (0, sw, 0, 1)


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 64, 64, 0), "which"), ((0, 64, 64, 4), "which"), ((0, 64, 0, 1), "group must be at least 1"),
                      ((0, 64, 24, 1), "group must divide n_coeffs"), ((0, 0, 1, 1), "empty slice"), ((0, 0, 1, 3), "empty slice"),
                      ((6, 64, 64, 1), "unknown ring"), ((-1, 64, 64, 1), "unknown ring"), ((0, 1 << 50, 1, 1), "too large")):
        assert lib.sr_norm_plan(*args, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    for ptrs in ((None, ctypes.byref(b), ctypes.byref(c)), (ctypes.byref(a), None, ctypes.byref(c)), (ctypes.byref(a), ctypes.byref(b), None)):
        assert lib.sr_norm_plan(0, 64, 64, 1, *ptrs) == 1
        assert "null" in _lib.last_error()


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    # every other argument is bad as well: the context is looked at first
    assert lib.sr_norm_batch(None, p, p, 7, 0, 9) == 1 and "null context" in _lib.last_error()
    assert lib.sr_norm_batch_dev(None, buf.ctypes.data, buf.ctypes.data, 7, 0, 9, None, 0, None) == 1
    assert "null context" in _lib.last_error()


def test_no_cpu_fallback_for_the_norm_calls():
    """Without a HIP device there is no context, hence no norm: the host-pointer call cannot quietly compute on the CPU."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    from stark_rings_amd import CyclotomicRing, RingError

    with pytest.raises(RingError, match="no HIP device|no CPU fallback"):
        ring = CyclotomicRing("goldilocks", 6)
        ring.linf_norm(np.zeros(64, dtype=np.uint64))


# ---- the restatement the GPU tests use as their oracle ----------------------------------------------------------------------------
def test_model_on_the_reference_decomposition_kat(kats):
    """stark_prime/decomposition.rs:73-99 pins the signed digits of one element; the norms of those digits, stored as field elements
    (a negative digit d is p + d), follow from the signed representative alone."""
    kat = kats["decomposition"]["stark_prime_fq"]
    p = MODULUS[2]
    digits = [int(d) for d in kat["digits"]]
    assert digits[:4] == [-27323, -17255, -17793, 901] and not any(digits[4:])
    xs = [d % p for d in digits]
    assert [M.signed(x, p) for x in xs] == digits
    assert M.linf(xs, p) == 27323
    assert M.l2sq(xs, p) == 27323**2 + 17255**2 + 17793**2 + 901**2
    assert M.records(xs, p, len(xs), 3, 4) == M.words(27323, 4) + M.words(27323**2 + 17255**2 + 17793**2 + 901**2, 9)


@pytest.mark.parametrize("ring", range(6))
def test_model_on_hand_values(ring):
    p, limbs = MODULUS[ring], LIMBS[ring]
    h = (p - 1) // 2
    assert (M.linf([p - 1], p), M.l2sq([p - 1], p)) == (1, 1)
    assert (M.linf([h, h + 1], p), M.l2sq([h, h + 1], p)) == (h, 2 * h * h)
    assert (M.linf([0], p), M.l2sq([0], p), M.l2sq([], p)) == (0, 0, 0)
    with pytest.raises(ValueError):
        M.linf([], p)
    # the widths the header derives: a square below 2^126 (2^502), hence a sum of 2^64 of them below 2^190 (2^566)
    assert h * h < 1 << (126 if limbs == 1 else 502)
    assert (1 << 64) * h * h < 1 << (190 if limbs == 1 else 566)
    recs = M.records([1, p - 2, h, 0, 3, p - 3], p, 3, 3, limbs)
    wpg = len(recs) // 2
    assert wpg == (4 if limbs == 1 else 13)
    assert recs[:limbs] == M.words(h, limbs) and recs[wpg:wpg + limbs] == M.words(3, limbs)
    assert recs[limbs:wpg] == M.words(1 + 4 + h * h, wpg - limbs) and recs[wpg + limbs:] == M.words(18, wpg - limbs)
