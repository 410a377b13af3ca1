#!/usr/bin/env python3
"""Generate tests/golden/color_coeffs_ref.npz from the reference's OWN compute_color_coeffs (oracle/_ref/libugref.so, `make -C oracle ref`).
Run where the reference tree exists:  python tests/golden/make_color_coeffs_golden.py
tests/test_lavc_conv.py::test_compute_color_coeffs compares the library with these vectors even where oracle/_ref is absent."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_lavc_conv as T

coeffs = np.array([[T.ref_compute_color_coeffs(kr, kb, d) for d in T.COEFF_DEPTHS] for kr, kb in T.COEFF_WEIGHTS], np.int32)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "color_coeffs_ref.npz"),
                    weights=np.array(T.COEFF_WEIGHTS, np.float64), depths=np.array(T.COEFF_DEPTHS, np.int32), coeffs=coeffs)
print("color_coeffs_ref.npz:", coeffs.shape)
