#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_seq_kp.py records as E32: the error of the keypoint-track fit's oracle
(tests/_fit_seq_kp_oracle.py) run in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.
The GPU gates are 4 x these.  Also prints the oracle's recovery figures that tests/test_fit_seq_kp.py holds the fixed inputs
to and DESIGN.md 18 quotes: the noisy tracks' accel_error, the gap's distances, the outlier tracks' reprojection RMS.
Needs no GPU."""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_kp_oracle as KO
    import _fit_seq_cases as SC
    import _fit_seq_kp_cases as G
    import _fit_seq_kp_oracle as QO

    # one step: the accepted p after one LM step from step_case(name, V, 2, T) (lambda 1e-2, SMOOTH)
    for name, V, T in [(n, 37, T) for n in ("both", "2d", "robust") for T in (1, 2, 3, 5)] + [("both", 778, 3)]:
        Ps = G.step_case(name, V, 2, T)[4]
        r32 = G.step_case(name, V, 2, T, torch.float32)
        print(f'("step", "{name}", {V}, {T}): {QO.rel(r32[4].numpy(), Ps.numpy()):.3e},   # accepted {r32[6].tolist()}')
    for k, e in G.cost_e32().items():
        print(f'("cost", {k}): {e:.3e},')
    for kind in ("pi", "gap0", "gap_mid"):
        pr, S, T, P64, e = G.start_case(kind)
        print(f'("start", "{kind}"): {e:.3e},   # |rots| of sequence 0: {P64[0, :, :3].norm(dim=1).numpy().round(3).tolist()} rad')
    # the reduction to scat_mano_fit_seq: 3-D only, no robust loss, no limits, the camera frozen, _fit_seq_cases' step
    m = G.host_model(37)
    X, P1, Ps, _ = SC.step_case(37, 2, 3)
    pr = KO.Problem(G.JOINT_MAP, T3=X, half=G.HALF)
    P65 = torch.cat([P1, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).expand(2, 3, 3)], dim=2)
    P32, _, acc = QO.lm(m, pr, P65.float(), 1, SC.sm(SC.SMOOTH) + (0.0, 0.0), 1e-2, G.ALL, 0)
    print(f'("step", "3d", 37, 3): {QO.rel(P32[..., :62].numpy(), Ps.numpy()):.3e},   # accepted {acc.tolist()}')
    X, T2n, out = G.noisy_case()
    print(f"noisy tracks: {G.NOISE_PX} px, 2-D only, T {G.NOISE_T}, S {G.NOISE_S}, {G.NOISE_ITERS} iterations, smooth {G.SMOOTH_NOISY}")
    for dt in ("fp64", "fp32"):
        print(f"    {dt}: accel_error in mm, sequence {(1e3 * out['seq', dt]).round(4).tolist()}, per frame "
              f"{(1e3 * out['frame', dt]).round(4).tolist()}")
    X, pr, r0, rf = G.gap_case()
    print(f"gap: frame {G.GAP_AT} of {G.GAP_T} without weight, joint RMS from the truth {1e3 * r0:.3f} mm at the start, "
          f"{1e3 * rf:.4f} mm after {G.GAP_ITERS} iterations of the fp64 oracle")
    _, _, _, inl, r = G.robust_case()
    at = G.outlier_frame(G.ROBUST_T)
    print(f"outliers: three keypoints of frame {at} moved by {G.OUTLIER_PX} px, {G.ROBUST_ITERS} iterations; reprojection RMS over the "
          f"inliers on that frame in px, sigma2 = {G.SIGMA2}: {r['gm'][:, at].round(4).tolist()}, sigma2 = 0: "
          f"{r['quad'][:, at].round(4).tolist()}; over all frames {r['gm'].mean(1).round(4).tolist()} against "
          f"{r['quad'].mean(1).round(4).tolist()}; floor {G.px_floor(G.ROBUST_S).round(5).tolist()} px")


if __name__ == "__main__":
    main()
