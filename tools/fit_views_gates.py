#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_views.py records as E32: the error of the multi-view fit's oracle
(tests/_fit_views_oracle.py) run in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.
The GPU gates are 4 x these.  Then the recovery cases: what the fp64 and the fp32 oracle reach from the triangulated start
on noise-free keypoints (the GPU gate is 4 x the fp32 figures, per sample), and the split that one view of outliers makes
between the robust and the quadratic loss.  Needs no GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_views_cases as C
    import test_gpu_fit_views as G

    np.set_printoptions(precision=6, linewidth=200)
    for key in G.e32_keys():
        if key == ("tri", "validity"):
            e = C.validity_case()[3]
        elif key[0] in ("tri", "start"):
            e = C.start_case(*key[1:])[4 if key[0] == "tri" else 5]
        elif key[0] == "step":
            e = C.step_e32(*key[1:])
            assert C.run(*key[1:], 1)[2].tolist() == [1] * key[3], key
        else:
            e = C.cost_e32(*G.COST)[key[1]]
        print(f"{key!r}: {e:.3e},")
    for name in ("quad", "gm_outliers", "quad_outliers"):
        (_, a3, a2), (_, b3, b2) = C.recovery(name), C.recovery(name, torch.float32)
        print(f"recovery {name}: joint RMS mm, fp64 {1e3 * a3}, fp32 {1e3 * b3}; pixel RMS, fp64 {a2}, fp32 {b2}")
    _, g3, g2 = C.recovery("gm_outliers", torch.float32)
    _, q3, q2 = C.recovery("quad_outliers")
    print("one view of outliers: the quadratic fit is outside 4 x the robust fit's figures on every hand:",
          bool((q3 > 4 * g3).all() and (q2 > 4 * g2).all()))


if __name__ == "__main__":
    main()
