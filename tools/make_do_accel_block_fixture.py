#!/usr/bin/env python3
"""tests/golden/do_accel_block.json: the answers of the reference's own do_accel_block (src/hwlm/hwlm.c:80-99, exported
from oracle/_ref by oracle/ref_build/accel_block_shim.c) and its forward-accel image for the seeded cases of
tests/test_accel_build.py (do_accel_block_cases), so that the test of the model needs no compiled reference.
Run where oracle/_ref is built (__graft_entry__.build())."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import oracle_binding as ob  # noqa: E402
from tests.test_accel_build import DO_ACCEL_BLOCK_GOLDEN, do_accel_block_cases, reference_accel_image  # noqa: E402

R = ob.href()
sets = []
for lits, _fa, cases in do_accel_block_cases():
    raw = reference_accel_image(R, lits)
    img = (C.c_uint8 * 80).from_buffer_copy(raw)
    want = [int(R.hsref_do_accel_block(img, blk.ctypes.data, n, start)) for n, _trial, blk, starts in cases for start in starts]
    sets.append({"image_hex": raw.hex(), "want": want})
with open(DO_ACCEL_BLOCK_GOLDEN, "w") as f:
    json.dump({"source": "do_accel_block (src/hwlm/hwlm.c) of the compiled reference, oracle/_ref/libhsref.so", "sets": sets}, f)
    f.write("\n")
print(sum(len(s["want"]) for s in sets), "answers ->", DO_ACCEL_BLOCK_GOLDEN)
