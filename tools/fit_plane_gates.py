#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_plane.py records as E32: the error of the point-to-plane fit's oracle
(tests/_fit_plane_oracle.py) run in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.
The GPU gates are 4 x these.  Needs no GPU; also prints the oracle's quality table for DESIGN.md 19.

  step   the accepted p after one metric LM step from metric_case(V) (lambda 1e-2), per tau
  cost   the oracle's metric cost function at its own iterate after 20 iterations of metric_case(V), per tau

The quality table, on quality_inputs() of tests/_fit_plane_cases.py (the smooth model on the hand surface, 4 hands, 2048
points on the faces): vertex RMS against the true mesh in mm after 5 / 10 / 20 rounds x 4 iterations, nearest-vertex ICP
against point-to-plane at tau 0 / 0.01 / 0.1 (no state but p passes between rounds, so the rows of 5 and 10 rounds are
read off the run of 20), the round from which a method stays within 10 % of its own plateau (its RMS after 20 rounds),
and the same methods on the mesh's own vertices, shuffled."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TABLE_TAUS = (0.0, 0.01, 0.1)
TABLE_ROUNDS = (5, 10, 20)


def plateau_round(r):
    """per hand, the first round from which the RMS [rounds + 1, B] stays within 10 % of its last value"""
    ok = r <= 1.1 * r[-1]
    return [int(next(k for k in range(len(r)) if ok[k:, b].all())) for b in range(r.shape[1])]


def main():
    import _fit_plane_cases as G
    import _fit_plane_oracle as LO
    import _fit_points_oracle as PO
    import _fit_verts_oracle as VO

    for V in G.FIT_V:
        m = G.host_model(V)
        Tv, w, n, P1 = G.metric_case(V)
        for tau in G.TAUS:
            Ps, P20, _ = G.metric_runs(V, tau)
            P32, _, acc = LO.lm(m, Tv, w, n, tau, P1.float(), 1, lambda0=1e-2)
            print(f'("step", {V}, {tau}): {VO.rel(P32.numpy(), Ps.numpy()):.3e},   # accepted {acc.tolist()}')
            with torch.no_grad():
                c32 = LO.cost(m, P20.float(), Tv, w, n, tau, 1e-6, 1e-6)
                c64 = LO.cost(m, P20, Tv.double(), w.double(), n.double(), tau, 1e-6, 1e-6)
            print(f'("cost", {V}, {tau}): {VO.rel(c32.numpy(), c64.numpy()):.3e},')
    mm = lambda a: (1e3 * np.asarray(a)).round(3).tolist()
    m, topo = G.smooth_model(), G.topology(778)
    _, mesh, pts, P0 = G.quality_inputs()
    own = np.ascontiguousarray(mesh.numpy()[:, np.random.default_rng(5400).permutation(778)]).astype(np.float32)
    print(f"quality: {G.QB} hands, N = {G.QN} on the faces, start {mm(G.vertex_rms(P0, mesh))} mm vertex RMS")
    for name, cloud, rounds in (("surface cloud", pts, max(TABLE_ROUNDS)), ("own vertices, shuffled", own, 10)):
        runs = [("nearest vertex", PO.icp(m, cloud, None, P0, rounds, G.ITERS, history=True)[4])]
        runs += [(f"plane tau {tau}", LO.icp(m, cloud, None, P0, topo, rounds, G.ITERS, tau, history=True)[4]) for tau in TABLE_TAUS]
        for method, Ps in runs:
            r = np.stack([G.vertex_rms(p, mesh) for p in Ps])
            rows = [k for k in TABLE_ROUNDS if k <= rounds] if rounds > 10 else [rounds]
            print(f"{name}, {method}: " + "; ".join(f"{k} x {G.ITERS}: {mm(r[k])}" for k in rows) +
                  f" mm; within 10 % of the last from round {plateau_round(r)}")
    jr, left, want = G.layer_plane_case()[2:]
    print(f"layer plane case: the joints fit alone {mm(left)} mm, fp64 oracle after {G.ROUNDS} x {G.ITERS} at tau {G.TAU} {mm(want)} mm")


if __name__ == "__main__":
    main()
