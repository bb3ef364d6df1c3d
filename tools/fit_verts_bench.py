#!/usr/bin/env python
"""The on-device MANO fit to a full mesh, V = 778, batch 1 / 96 / 1024, 20 iterations from the same start: device events
after warm-up, medians over alternated repeats.

  fit_vertices  ManoFitter.fit_vertices from a given start: one launch (scat_mano_fit_verts), 3 V x 62 Jacobian, normal
                equations, Cholesky and the trial cost's forward pass inside it
  fit_joints    ManoFitter.fit on the 21 joints of the same hands, from its own start: what the 778 vertices cost over
                21 points (tools/fit_bench.py's kernel)
  torch_lm64    the oracle's Levenberg-Marquardt (tests/_fit_verts_oracle.py) written in fp64 torch on the device: per
                iteration a forward-mode Jacobian of the layer's formulas (58 vectorised tangents), J^T J by matmul,
                torch.linalg.cholesky_ex / cholesky_solve, one more forward for the trial cost, accept / reject as
                torch.where (no host synchronisation inside the loop)

Every case is a window of ``inner`` fits between two events (host launch time included); the cases alternate inside every
repeat so that drift hits all alike.  With --tiles (needs the diag build, python -m scat_amd.build --diag, and
SCAT_LIBPATH pointing at it) the kernel is also timed with tiles of 8 and 16 vertices instead of 32: the tile changes the
number of barriers and the width of the vertex pass, never the number of rows the accumulation adds, so what moves with it
is the vertex pass and the barriers and what stays is the accumulation and the solve.  --iters-sweep times 1 and 20
iterations to separate the start from an iteration.  With --out also writes the table to a file
(profiles/fit_verts_bench.txt is such a run)."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


class TorchLM64:
    """the fit of include/scat_mano_fit_verts.h in fp64 torch on the device, the formulas of tests/_mano_oracle.py"""

    def __init__(self, model, w_pose, w_beta, lambda0, dev):
        D = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)
        self.vt, self.sd, self.pd = D(model.v_template), D(model.shapedirs), D(model.posedirs)
        self.Jr, self.W, self.hm = D(model.J_regressor), D(model.weights), D(model.hands_mean)
        self.parents, self.dev = list(model.parents), dev
        self.w_pose, self.w_beta, self.lambda0 = w_pose, w_beta, lambda0
        self.prior = torch.zeros(62, dtype=torch.float64, device=dev)
        self.prior[3:48], self.prior[48:58] = w_pose, w_beta

    def rodrigues(self, r):
        t = (r * r).sum(-1)
        small = t < 1e-8
        ts = torch.where(small, torch.ones_like(t), t)
        th = ts.sqrt()
        a = torch.where(small, 1.0 - t / 6.0 + t * t / 120.0, torch.sin(th) / th)
        b = torch.where(small, 0.5 - t / 24.0 + t * t / 720.0, 2.0 * torch.sin(0.5 * th) ** 2 / ts)
        x, y, z = r[:, 0], r[:, 1], r[:, 2]
        o = torch.zeros_like(x)
        S = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(-1, 3, 3)
        eye = torch.eye(3, dtype=r.dtype, device=r.device).unsqueeze(0)
        S2 = r.unsqueeze(2) * r.unsqueeze(1) - t.reshape(-1, 1, 1) * eye
        return eye + a.reshape(-1, 1, 1) * S + b.reshape(-1, 1, 1) * S2

    def verts(self, P):
        B = P.shape[0]
        pose = torch.cat([torch.zeros(B, 1, 3, dtype=P.dtype, device=P.device), (self.hm.reshape(1, 45) + P[:, 3:48]).reshape(B, 15, 3)],
                         dim=1)
        R = self.rodrigues(pose.reshape(-1, 3)).reshape(B, 16, 3, 3)
        v_shaped = self.vt.unsqueeze(0) + torch.einsum("vck,bk->bvc", self.sd, P[:, 48:58])
        J = torch.einsum("jv,bvc->bjc", self.Jr, v_shaped)
        pw = (R[:, 1:] - torch.eye(3, dtype=P.dtype, device=P.device)).reshape(B, 135)
        vp = v_shaped + torch.einsum("vck,bk->bvc", self.pd, pw)
        RG, t = [R[:, 0]], [J[:, 0]]
        for i in range(1, 16):
            p = self.parents[i]
            RG.append(RG[p] @ R[:, i])
            t.append((RG[p] @ (J[:, i] - J[:, p]).unsqueeze(2)).squeeze(2) + t[p])
        RG, t = torch.stack(RG, 1), torch.stack(t, 1)
        a = t - (RG @ J.unsqueeze(3)).squeeze(3)
        v = (torch.einsum("vi,birc->bvrc", self.W, RG) @ vp.unsqueeze(3)).squeeze(3) + torch.einsum("vi,bir->bvr", self.W, a)
        Rg = self.rodrigues(P[:, 0:3]).transpose(1, 2)
        return v @ Rg - t[:, 1:2] @ Rg

    def cost(self, P, T):
        with torch.no_grad():
            r = torch.exp(P[:, 61]).reshape(-1, 1, 1) * self.verts(P) + P[:, None, 58:61] - T
        return (r * r).sum((1, 2)) + self.w_pose * (P[:, 3:48] ** 2).sum(1) + self.w_beta * (P[:, 48:58] ** 2).sum(1)

    def fit(self, T, P0, iters):
        P, B = P0.clone(), P0.shape[0]
        V = T.shape[1]
        lam = torch.full((B,), self.lambda0, dtype=torch.float64, device=self.dev)
        eye3 = torch.eye(3, dtype=torch.float64, device=self.dev).repeat(V, 1).unsqueeze(0)
        eye = torch.eye(62, dtype=torch.float64, device=self.dev).expand(B, 62, 62)
        zero = torch.zeros(58, dtype=torch.float64, device=self.dev)
        for _ in range(iters):
            Pm = P[:, :58].detach()
            pad = P[:, 58:].detach()
            jm = torch.autograd.functional.jacobian(lambda e: self.verts(torch.cat([Pm + e, pad], dim=1)), zero,
                                                    strategy="forward-mode", vectorize=True).reshape(B, 3 * V, 58)
            with torch.no_grad():
                x = self.verts(P)
            s = torch.exp(P[:, 61]).reshape(B, 1, 1)
            J = torch.cat([s * jm, eye3.expand(B, 3 * V, 3), (s * x).reshape(B, 3 * V, 1)], dim=2)
            r = (s * x + P[:, None, 58:61] - T).reshape(B, 3 * V)
            c = (r * r).sum(1) + self.w_pose * (P[:, 3:48] ** 2).sum(1) + self.w_beta * (P[:, 48:58] ** 2).sum(1)
            A = J.transpose(1, 2) @ J + torch.diag(self.prior)
            g = (J.transpose(1, 2) @ r.unsqueeze(2)).squeeze(2) + self.prior * P
            L, info = torch.linalg.cholesky_ex(A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2)))
            ok = info == 0
            Pt = P - torch.cholesky_solve(g.unsqueeze(2), torch.where(ok.reshape(B, 1, 1), L, eye)).squeeze(2)
            take = ok & torch.isfinite(Pt).all(1) & (self.cost(Pt, T) < c)
            P = torch.where(take.unsqueeze(1), Pt, P)
            lam = torch.where(take, (lam * 0.1).clamp_min(1e-12), (lam * 10).clamp_max(1e12))
        return P


def tile_entry():
    """scat_mano_fit_verts_tile of the diag build, or None: the product library has no such symbol"""
    from scat_amd._lib import lib, parse_header
    from scat_amd.fit import FIT_VERTS_HEADER

    L = lib()
    if not hasattr(L.cdll, "scat_mano_fit_verts_tile"):
        return None
    fn = L.cdll.scat_mano_fit_verts_tile
    at = [t for t, _ in parse_header(FIT_VERTS_HEADER)["scat_mano_fit_verts"][1]]
    fn.restype, fn.argtypes = ctypes.c_int, at[:-1] + [ctypes.c_int, ctypes.c_void_p]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8, help="fits per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="leave the fp64 torch loop out")
    ap.add_argument("--tiles", action="store_true", help="also time tiles of 8 and 16 vertices (the diag build)")
    ap.add_argument("--iters-sweep", action="store_true", help="also time 1 iteration")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter
    from scat_amd.mano import ManoLayer, ManoModel, _model_args
    from scat_amd.ops import _p, _stream

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    host = ManoModel.synthetic(1)
    model = ManoModel.synthetic(1).to(dev)
    jmap = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)
    fitter = ManoFitter(model, joint_map=jmap, iters=a.iters)
    layer = ManoLayer(model)
    plain = TorchLM64(host, fitter.w_pose, fitter.w_beta, fitter.lambda0, dev)
    tile_fn = tile_entry() if a.tiles else None
    if a.tiles and tile_fn is None:
        raise SystemExit("--tiles needs the diag build: python -m scat_amd.build --diag, then SCAT_LIBPATH=tools/_bin/libscat_hip_diag.so")
    lines = [f"V = {model.V}, {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} fits, cases alternated; ms per "
             f"fit, device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        true = torch.cat([T_(synth.normal_like(90 + B, n, (B, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.2))],
                         dim=1).to(dev)
        with torch.no_grad():
            out = torch.exp(true[:, 61]).reshape(-1, 1, 1) * layer(true[:, 0:3].contiguous(), true[:, 3:48].contiguous(),
                                                                    true[:, 48:58].contiguous()) + true[:, None, 58:61]
        Tv, Tj = out[:, 21:].contiguous(), out[:, :21][:, list(jmap)].contiguous()
        P0 = fitter.fit_vertices(Tv, iters=1, free=0).p      # the Procrustes start, nothing solved for: the same start for all
        Pj0 = fitter.fit(Tj, iters=1, free=0).p
        cases = [("fit_vertices", lambda: fitter.fit_vertices(Tv, init=P0).p), ("fit_joints", lambda: fitter.fit(Tj, init=Pj0).p)]
        if a.iters_sweep:
            cases.append(("fit_vertices_i1", lambda: fitter.fit_vertices(Tv, init=P0, iters=1).p))
        if tile_fn is not None:
            def with_tile(tile):
                def run():
                    p = P0.clone()
                    cost = torch.empty((B,), dtype=torch.float32, device=dev)
                    acc = torch.empty((B,), dtype=torch.int32, device=dev)
                    rc = tile_fn(*_model_args(model), _p(Tv), None, _p(p), _p(cost), _p(acc), B, model.V, model.parents_packed,
                                 a.iters, 0, fitter.lambda0, fitter.w_pose, fitter.w_beta, (1 << 62) - 1, tile, _stream())
                    assert rc == 0, rc
                    return p
                return run
            cases += [(f"tile_{t}", with_tile(t)) for t in (8, 16, 32)]
        if not a.no_torch:
            Tv64, P064 = Tv.double(), P0.double()
            cases.append(("torch_lm64", lambda: plain.fit(Tv64, P064, a.iters)))
        for _ in range(a.warmup):
            for _, fn in cases:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in cases}
        for _ in range(a.repeats):
            for name, fn in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.inner)

        def rms(P):
            with torch.no_grad():
                d = torch.exp(P[:, 61]).reshape(-1, 1, 1) * plain.verts(P.double()) + P[:, None, 58:61].double() - Tv.double()
            return (d * d).sum(2).mean(1).sqrt() * 1e3

        reached = [("start", rms(P0))] + [(name, rms(fn())) for name, fn in cases if not name.endswith("_i1")]
        lines.append(f"batch {B}: vertex RMS in mm, median (max) over the batch: " +
                     "; ".join(f"{name} {r.median():.4f} ({r.max():.4f})" for name, r in reached))
        med = {}
        for name, _ in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:16s} median {med[name]:10.4f} ms  min {t[0]:10.4f}  max {t[-1]:10.4f}")
        lines.append(f"  fit_vertices / fit_joints: {med['fit_vertices'] / med['fit_joints']:.2f}" +
                     ("" if a.no_torch else f"; fit_vertices / torch_lm64: {med['fit_vertices'] / med['torch_lm64']:.5f}"))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
