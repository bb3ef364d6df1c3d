#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_seq.py records as E32: the error of the sequence fit's oracle
(tests/_fit_seq_oracle.py) run in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.
The GPU gates are 4 x these.  Also prints the conditions tests/test_fit_seq.py holds the fixed inputs to: (a) the
smoothing case's accel_error figures, (b) the gap case's distances.  Needs no GPU."""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_oracle as FO
    import _fit_seq_cases as G
    import _fit_seq_oracle as SO

    JM, sm = G.JOINT_MAP, G.sm(G.SMOOTH)
    # one step: the accepted p after one LM step from step_case(V, S, T) (lambda 1e-2, SMOOTH)
    for V, S, T in ((37, 2, 1), (37, 2, 2), (37, 2, 3), (37, 2, 5), (778, 2, 3)):
        m = G.host_model(V)
        X, P1, Ps, c = G.step_case(V, S, T)
        P32, _, acc = SO.lm(m, X, G.ones(S, T).float(), JM, P1.float(), 1, sm, lambda0=1e-2)
        print(f'("step", {V}, {T}): {FO.rel(P32.numpy(), Ps.numpy()):.3e},   # accepted {acc.tolist()}')
    m = G.host_model(37)
    # the cost: the oracle's cost function in fp32 against fp64 at the oracle's own iterate after k iterations
    P, X, P0 = G.start_case()
    w = G.ones(2, 5)
    for k in (1, 2, 5, 10):
        Pk = SO.lm(m, X.double(), w, JM, P0, k, sm)[0].float()
        with torch.no_grad():
            c32 = SO.cost(m, Pk, X, w.float(), JM, 1e-6, 1e-6, sm)
            c64 = SO.cost(m, Pk.double(), X.double(), w, JM, 1e-6, 1e-6, sm)
        print(f'("cost", {k}): {FO.rel(c32.numpy(), c64.numpy()):.3e},')
    # the start: the oracle's start from zero-pose joints in fp32 (what the kernel has) against fp64; the Procrustes
    # itself is fp64 in both, and in the kernel
    for name, case, w in (("start", G.start_case(), G.ones(2, 5)), ("start_pi", G.pi_case(), G.ones(1, 5))):
        P, X, P0 = case
        P32 = SO.start(m, X, w, JM, torch.float32)
        print(f'("{name}",): {FO.rel(P32.numpy(), P0.numpy()):.3e},   # |rots| of sequence 0: '
              f'{P0[0, :, :3].norm(dim=1).numpy().round(3).tolist()} rad')
    X, Xn, out = G.noisy_case()
    print(f"(a) smoothing case: noise {G.NOISE} m, T {G.NOISE_T}, S {G.NOISE_S}, {G.NOISE_ITERS} iterations, smooth {G.SMOOTH_NOISY}")
    for dt in ("fp64", "fp32"):
        print(f"    {dt}: accel_error in mm, sequence {(1e3 * out['seq', dt]).round(4).tolist()}, per frame "
              f"{(1e3 * out['frame', dt]).round(4).tolist()}, ratio {(out['frame', dt] / out['seq', dt]).round(2).tolist()} "
              f"(the condition wants 3)")
    X, w, r0, rf = G.gap_case()
    print(f"(b) gap case: frame {G.GAP_AT} of {G.GAP_T} without weight, joint RMS from the truth {1e3 * r0:.3f} mm at the start, "
          f"{1e3 * rf:.4f} mm after {G.GAP_ITERS} iterations of the fp64 oracle")


if __name__ == "__main__":
    main()
