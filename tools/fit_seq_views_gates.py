#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_seq_views.py records as E32: the error of the multi-view track fit's oracle
(tests/_fit_seq_views_oracle.py) run in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.
The GPU gates are 4 x these.  Then the recovery cases: what the fp64 and the fp32 oracle reach (the GPU gate is 4 x the fp32
figures, per sequence), and the acceleration error of the track against the frame-by-frame fit.  Needs no GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_seq_views_cases as C
    import _fit_seq_views_oracle as QO
    import test_gpu_fit_seq_views as G
    from _fit_cases import JOINT_MAP, host_model

    np.set_printoptions(precision=6, linewidth=200)
    for key in G.e32_keys():
        if key[0] == "start":
            e = C.start_case(*key[1:])[3]
        elif key[0] == "step":
            e = C.step_e32(*key[1:])
            assert C.run(*key[1:], 1)[2].tolist() == [1] * key[3], key
        else:
            e = C.cost_e32(*G.COST)[key[1]]
        print(f"{key!r}: {e:.3e},")
    for name in C.RECOVERY_CASES:
        (_, a3, a2, ag, _), (_, b3, b2, bg, _) = C.recovery(name), C.recovery(name, torch.float32)
        print(f"recovery {name}: joint RMS mm, fp64 {1e3 * a3}, fp32 {1e3 * b3}; pixel RMS, fp64 {a2}, fp32 {b2}; "
              f"frame {C.GAP_FRAME} joint RMS mm, fp64 {1e3 * ag}, fp32 {1e3 * bg}")
    m, X3 = host_model(C.RECOVERY["V"]), C.recovery_problem("noise")[1]
    print(f"acceleration error mm / frame^2 on the noisy case: track {1e3 * QO.accel(m, C.recovery('noise')[0], JOINT_MAP, X3).numpy()}, "
          f"frame by frame {1e3 * QO.accel(m, C.per_frame('noise'), JOINT_MAP, X3).numpy()}")


if __name__ == "__main__":
    main()
