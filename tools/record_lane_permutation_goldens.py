#!/usr/bin/env python3
"""Records the fixtures of tests/test_board_lane_permutation_gpu.py (dev tool; needs a GPU):

    MRCAL_AMD_LIB=<libmrcal_amd.so of the commit to record from> python tools/record_lane_permutation_goldens.py [DIR]

One .npz per case (variant x board) into DIR, tests/golden/lane_permutation by default: the normal equations and x at
the seed and after two solver steps, b_packed after them - evaluate_case() of the test, run on the library that
MRCAL_AMD_LIB names. The test then asks any later library for the same bits."""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mrcal_amd
import test_board_lane_permutation_gpu as T

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
os.makedirs(out, exist_ok=True)
print("recording from", mrcal_amd._libpath)
total = 0
for variant in T.VARIANTS:
    for W, H in T.BOARDS:
        path = os.path.join(out, T.case_name(W, H, variant) + ".npz")
        np.savez_compressed(path, **T.evaluate_case(mrcal_amd._api, W, H, variant))
        total += os.path.getsize(path)
        print(f"{path}: {os.path.getsize(path)} bytes")
print(f"{len(T.VARIANTS)*len(T.BOARDS)} cases, {total} bytes")
