#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_points.py records as E32: the error of the point-cloud fit's oracle
(tests/_fit_points_oracle.py on tests/_fit_verts_oracle.py) run in fp32 on the CPU against its own fp64 run on the test's
inputs, max |a - b| / max |b|.  The GPU gates are 4 x these.  Needs no GPU; also prints the oracle's recovery figures
for DESIGN.md 17, the clouds of points between vertices included.

  pts    the model points exp(log_scale) x + trans on the inputs of param_case(B, V)
  cost   the data cost of the assignment at the oracle's iterate after k rounds of icp_case(V, "shuffled"), the model
         points computed in fp32 against fp64 (both searched in fp64, as the kernel does)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def between(V, G, PO):
    """N = 2 V points on the segments from every vertex to its nearest neighbour, at 1/3 and 2/3"""
    Tv = G.seeded(V)[2].numpy().astype(np.float64)
    out = []
    for b in range(G.NB):
        t = PO.d2_table(Tv[b], Tv[b])
        np.fill_diagonal(t, np.inf)
        nb = Tv[b][t.argmin(1)]
        out.append(np.concatenate([Tv[b] + (nb - Tv[b]) / 3.0, Tv[b] + 2.0 * (nb - Tv[b]) / 3.0]))
    return np.stack(out).astype(np.float32)


def main():
    import _fit_points_cases as G
    import _fit_points_oracle as PO
    import _fit_verts_oracle as VO

    T_ = G.T_
    for V in G.PARAM_V:
        for B in G.PARAM_B:
            P, x, _, _ = G.param_case(B, V)
            with torch.no_grad():
                x32 = VO.model_verts(G.host_model(V), T_(P)).numpy()
            print(f'("pts", {B}, {V}): {VO.rel(x32, x):.3e},')
    for V in G.FIT_V:
        m = G.host_model(V)
        Ps = G.icp_case(V, "shuffled", None)[5]
        for k in G.MONOTONE_ROUNDS:
            Pk = Ps[k].float()
            with torch.no_grad():
                c32 = PO.assign(VO.model_verts(m, Pk).numpy(), G.cloud(V, "shuffled"))["stats"][:, 3]
                c64 = PO.assign(VO.model_verts(m, Pk.double()).numpy(), G.cloud(V, "shuffled"))["stats"][:, 3]
            print(f'("cost", {V}, {k}): {VO.rel(c32, c64):.3e},')
    mm = lambda a: (1e3 * a).round(4).tolist()
    for V, kind, md in ((37, "shuffled", None), (37, "shuffled", G.TRIM), (778, "shuffled", None), (778, "shuffled", G.TRIM),
                        (778, "half", None)):
        Pf, r0, rf, costs, rec, _ = G.icp_case(V, kind, md)
        print(f"V {V} {kind} max_dist {md}: vertex RMS in mm, start {mm(r0)}, fp64 oracle after {G.ROUNDS} x {G.ITERS} {mm(rf)}, "
              f"recoverable {rec.tolist()}")
    _, rf, rec = G.layer_cloud_case()
    print(f"layer cloud case: fp64 oracle after {G.ROUNDS} x {G.ITERS} {mm(rf)} mm, recoverable {rec.tolist()}")
    V = 778
    m, Tv = G.host_model(V), G.seeded(V)[2]
    for name, pts in (("shuffled", G.cloud(V, "shuffled")), ("half", G.cloud(V, "half")), ("between", between(V, G, PO))):
        P, _, costs, _, Ps = PO.icp(m, pts, None, G.start(V), 10, 4, history=True)
        r = np.stack([VO.rms(m, p, Tv).numpy() for p in Ps])
        done = [int(np.argmax(r[:, b] <= 1.01 * r[-1, b])) for b in range(G.NB)]
        print(f"10 x 4, {name} (N = {pts.shape[1]}): vertex RMS in mm {mm(r[-1])}, within 1 % of it from round {done}")


if __name__ == "__main__":
    main()
