"""Device form of the shift products 2^E, 32 < E < 64, on the words of tests/test_shift_q1_host.py: one launch of
tools/ubench/field_check --mid (an exponent per word), whose results must be bit-equal to the host form of the same source (compared
inside the tool) and to Python integers (compared here).  What this guards is device-only: the inline-asm statement's EXEC masks,
the carry-out of the multiply-add, the compare under a reduced mask."""
import os
import subprocess

import numpy as np
import pytest

import shift_q1_words as W
from test_device_field_check import DEPS, EXE, ROOT, _build

pytestmark = pytest.mark.gpu


def test_device_shift_products_of_the_middle_class_equal_the_host_form(tmp_path):
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        _build()
    pairs, repaired = [], 0
    for e in W.EXPONENTS:
        xs = W.words(e)
        repaired += sum(1 for x in W.repair_words(e) if x and x in xs)
        pairs += [(x, e) for x in xs]
    assert repaired >= 2 * len(W.EXPONENTS)
    src, dst = tmp_path / "pairs.bin", tmp_path / "out.bin"
    np.array(pairs, dtype=np.uint64).tofile(src)
    r = subprocess.run([EXE, "--mid", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=ROOT)
    out = r.stdout.decode()
    assert r.returncode == 0 and "field_check --mid: %d words, 0 mismatches" % len(pairs) in out, out[-2000:]
    got = np.fromfile(dst, dtype=np.uint64)
    assert len(got) == len(pairs)
    want = np.array([(x << e) % W.P for x, e in pairs], dtype=np.uint64)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(hex(pairs[i][0]), pairs[i][1], hex(int(got[i]))) for i in bad[:8]]
