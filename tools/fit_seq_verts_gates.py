#!/usr/bin/env python
"""CPU only.  Prints (1) the error of the oracle of tests/_fit_seq_verts_oracle.py run in fp32 against its own fp64 run on
the inputs of tests/_fit_seq_verts_cases.py, normalised max |a - b| / max |b|: the E32 table of
tests/test_gpu_fit_seq_verts.py, whose gates are 4 x these figures (the rule of tests/test_gpu_fit_seq.py; none of them
comes from a kernel); (2) whether the fp32 oracle reaches a rejected step on hard_case(), which the determinism test needs;
(3) the quality table of DESIGN 20: acceleration error and vertex RMS of the track ICP against per-frame point-to-plane
ICP on the smooth model, and the occluded frame, for Q_SMOOTH and for the weight sets of SWEEP it was chosen among."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


SWEEP = (dict(rots=3e-2, poses=3e-2, trans=10.0), dict(rots=1e-1, poses=3e-2, trans=30.0), dict(rots=3e-3, poses=3e-3, trans=1.0))


def main():
    import _fit_oracle as FO
    import _fit_seq_verts_cases as G
    import _fit_seq_verts_oracle as QO
    from _fit_cases import host_model

    f32, f64 = torch.float32, torch.float64
    sm = G.sm(G.SMOOTH)
    print("E32 = {")
    for V, T, metric in [(37, T, k) for T in (1, 2, 3, 5) for k in (False, True)] + [(778, 3, False)]:
        m = host_model(V)
        X, w, n, P1, Ps, _ = G.step_case(V, 2, T, metric)
        ww = G.ones(2, T, V) if w is None else w
        P32, _, acc = QO.lm(m, X, ww.float(), P1.float(), 1, sm, None if n is None else n.float(), G.TAU, lambda0=1e-2)
        assert bool((acc == 1).all())
        print(f'    ("step", {V}, {T}, {metric}): {FO.rel(P32.numpy(), Ps.numpy()):.3e},')
    m = host_model(37)
    P, X, P0 = G.start_case()
    w = G.ones(2, 5, 37)
    for k in (1, 2, 5, 10):
        Pk = QO.lm(m, X, w.float(), P0.float(), k, sm)[0]
        with torch.no_grad():
            c32 = QO.cost(m, Pk, X, w.float(), None, 1.0, 1e-6, 1e-6, sm)
            c64 = QO.cost(m, Pk.double(), X.double(), w, None, 1.0, 1e-6, 1e-6, sm)
        print(f'    ("cost", {k}): {FO.rel(c32.numpy(), c64.numpy()):.3e},')
    print(f'    ("start",): {FO.rel(QO.start(m, X, w, f32).numpy(), P0.numpy()):.3e},')
    for gap in (None, 1):
        for plane in (False, True):
            pts, Pi, topo = G.icp_case(2, 3, gap)
            Po, acc, dc, _, margin = G.icp_run(2, 3, plane, gap)
            P32, a32, dc32, _ = QO.icp(m, pts, None, Pi, topo if plane else None, G.ICP_ROUNDS, G.ICP_ITERS, G.sm(G.ICP_SMOOTH),
                                       G.TAU, G.ICP_TRIM, dt=f32)
            assert a32.tolist() == acc.tolist(), (a32, acc)      # one accept / reject path in both precisions
            print(f'    ("icp", {plane}, {gap}): {FO.rel(P32.numpy(), Po.numpy()):.3e},      # accepted {acc.tolist()}, margin {margin:.2e}')
    import _fit_plane_cases as LC

    ms, topo = LC.smooth_model(), LC.topology(778)
    mesh, qpts, Q0 = G.quality_inputs()
    q = G.quality_case()
    Q32 = QO.icp(ms, qpts, None, Q0, topo, G.Q_ROUNDS, G.Q_ITERS, G.sm(G.Q_SMOOTH), G.TAU, G.Q_TRIM, dt=f32)[0]
    print(f'    ("quality", "accel"): {FO.rel(QO.accel(ms, Q32, mesh).numpy(), q["accel", "track"]):.3e},')
    print(f'    ("quality", "rms"): {FO.rel(QO.rms(ms, Q32, mesh).numpy(), q["rms", "track"]):.3e},      # per frame; smallest margin '
          f'of a matched point {q["margin"]:.2e}')
    print("}")

    X, P1 = G.hard_case()
    for dt in (f32, f64):
        _, c, acc, hist = QO.lm(m, X.to(dt), G.ones(2, 3, 37).to(dt), P1.to(dt), G.HARD_ITERS, sm, lambda0=G.HARD_LAMBDA0,
                                history=True)
        print(f"hard_case {dt}: accepted {acc.tolist()} of {G.HARD_ITERS}, costs per iteration {hist.numpy().tolist()}")

    print(f"quality: {G.QS} x {G.QT} frames, {G.QN} points, noise {G.Q_NOISE} m, frame {G.Q_GAP} occluded, {G.Q_ROUNDS} x "
          f"{G.Q_ITERS}; acceleration error, vertex RMS over the visible frames and of the occluded one, mm")
    vis = [t for t in range(G.QT) if t != G.Q_GAP]
    row = lambda name, a, r: print(f"  {name:58s} accel {1e3 * a}   rms visible {1e3 * r[:, vis].mean(1)}   occluded {1e3 * r[:, G.Q_GAP]}")
    for name in ("start", "frame", "track"):
        row(f"{name} {G.Q_SMOOTH if name == 'track' else ''}", q["accel", name], q["rms", name])
    for sweep in SWEEP:      # the weights that Q_SMOOTH was chosen among
        Pq = QO.icp(ms, qpts, None, Q0, topo, G.Q_ROUNDS, G.Q_ITERS, G.sm(dict(G.Q_SMOOTH, **sweep)), G.TAU, G.Q_TRIM)[0]
        row(f"track {dict(G.Q_SMOOTH, **sweep)}", QO.accel(ms, Pq, mesh).numpy(), QO.rms(ms, Pq, mesh).numpy())


if __name__ == "__main__":
    main()
