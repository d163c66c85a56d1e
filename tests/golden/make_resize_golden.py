#!/usr/bin/env python
"""Generate tests/golden/imresize_float.npz from the REFERENCE ITSELF (runs only in the build container).

Imports the reference's utils/imresize.py from /root/reference/codes (read-only, never copied) and records, for the nine cases of
tests/resize_oracle.py::CASES, a seeded float64 image in [0, 1) with C = 3 and ``imresize``'s float64 output of it (float input,
'bicubic', scalar scale: no clipping, no rounding). The image is stored [3, H, W]; the reference is called on its [H, W, 3]
view. Data only: no reference text.

    python tests/golden/make_resize_golden.py
"""
import importlib.util as ilu
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/codes"

from tests.resize_oracle import CASES, case_name, scale_of  # noqa: E402


def main():
    spec = ilu.spec_from_file_location("ref_utils_imresize", os.path.join(REF, "utils", "imresize.py"))
    ref = ilu.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for n, (H, W, s, up) in enumerate(CASES):
        rng = np.random.RandomState(20260 + n)
        x = rng.random_sample((3, H, W))
        y = ref.imresize(np.ascontiguousarray(x.transpose(1, 2, 0)), scalar_scale=scale_of(s, up))     # method: its default, 'bicubic'
        assert y.dtype == np.float64
        out["x_" + case_name(H, W, s, up)] = x
        out["y_" + case_name(H, W, s, up)] = np.ascontiguousarray(y.transpose(2, 0, 1))
    path = os.path.join(HERE, "imresize_float.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
