#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_kp.py records as E32: the error of the keypoint fit's oracle (tests/_fit_kp_oracle.py) run
in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.  The GPU gates are 4 x these.
Then the builder's check of the recovery cases (the fp32 oracle must meet every recovery gate on every sample with a
factor 1.5 to spare) and the conditions (a), (b), (c) on the fixed inputs, with their figures for DESIGN.md 13.  Needs no
GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_kp_cases as C
    import test_gpu_fit_kp as G

    np.set_printoptions(precision=4, linewidth=200)
    for key in G.E32:
        if key[0] == "start":
            e = C.start_case(*key[1:])[2]
        elif key[0] == "step":
            e = C.run32(key[1], key[2], 1, key[3])[1]
            assert C.run(key[1], key[2], 1, key[3])[2].tolist() == [1] * key[3], key
        elif key[0] == "cost":
            e = C.cost_e32("gm_limits", 37)[key[1]]
        else:
            e = C.run32("limits", 37, 2)[1]
        print(f"{key!r}: {e:.3e},")
    ok = True
    for name, V in G.RECOVERY:
        w3, w2 = C.recovery_figures(name, V, C.run(name, V, 20)[0])
        g3, g2 = C.recovery_figures(name, V, C.run32(name, V, 20)[0])
        floor = C.px_floor(V)
        spare2 = (2 * w2 + floor) / g2
        line = f"recovery {name} V {V}: reprojection RMS px, fp64 {w2}, fp32 {g2}, gate / fp32 {spare2.min():.2f}"
        ok = ok and bool((spare2 >= 1.5).all())
        if w3 is not None:
            spare3 = (2 * w3 + 1e-5) / g3
            line += f"; joint RMS mm, fp64 {1e3 * w3}, fp32 {1e3 * g3}, gate / fp32 {spare3.min():.2f}"
            ok = ok and bool((spare3 >= 1.5).all())
        print(line)
    print("every recovery gate is met by the fp32 oracle with a factor 1.5 to spare:", ok)
    V = 37
    for dt in (torch.float64, torch.float32):
        tag = "fp64" if dt == torch.float64 else "fp32"
        gm, qd = (C.run if dt == torch.float64 else C.run32)("gm", V, 20)[0], (C.run if dt == torch.float64 else C.run32)("quad_outliers", V, 20)[0]
        a3, q3 = C.recovery_figures("gm", V, gm)[0], C.recovery_figures("quad_outliers", V, qd)[0]
        print(f"(a) {tag}: inlier RMS mm, Geman-McClure {1e3 * a3}, quadratic {1e3 * q3}, below a quarter: {bool((a3 < 0.25 * q3).all())}")
        _, start, end = C.condition_c(V, dt)
        print(f"(c) {tag}: reprojection RMS px, start {start}, after 40 iterations {end}, halved: {bool((end <= 0.5 * start).all())}")
    viol = {n: (C.run(n, V, 20)[0][:, 3:48].abs() - C.BOX).clamp_min(0).max(1).values.numpy() for n in ("limits", "both")}
    print(f"(b) fp64: largest violation rad, with limits {viol['limits']}, without {viol['both']}, smaller: "
          f"{bool((viol['limits'] < viol['both']).all())}")


if __name__ == "__main__":
    main()
