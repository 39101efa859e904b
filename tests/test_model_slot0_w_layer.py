"""tools/model_fast_goldilocks.py on REPRESENTATIVES for the three changes of DESIGN.md 6.3c: the shift product 2^32 .. 2^63 word for
word (with its no-further-wrap assertions, on the words m 2^(64 - r) that take the second + p), the DFT_16 networks whose slot-0
butterflies are lazy too (slot 0 any representative in and out, slots 1 .. 15 still canonical in: a non-canonical word there must trip
an assertion), the rows256 inverse without G::canon on crafted blocks, and the column pass with its W layer on the register side of
the exchange, both directions, equal to the canonical model.  CPU only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import model_fast_goldilocks as M


def test_middle_class_shift_product_model_holds_its_wrap_conditions():
    assert M.check_shift_q1(seed=32, rounds=1000)


def test_lazy_slot0_chain_and_register_side_w_layer_keep_their_invariants():
    assert M.check_slot0_chain_and_w_layer(seed=34)
