"""fp64 torch statement of the MANO fit to a full mesh of include/scat_mano_fit_verts.h on top of _mano_oracle.forward:
the model vertices, the cost, the Jacobian (torch.autograd.functional.jacobian, forward mode: 58 columns are fewer than
3 V rows), the Procrustes start over the vertices and the Levenberg-Marquardt loop with the schedule of
_fit_oracle.lm (Marquardt scaling, accept only if the cost drops, lambda / 10 or x 10 within 1e-12..1e12, a failed
Cholesky is a rejection, frozen unknowns are unit rows).  Test-only: imports none of scat_amd's kernels.

Everything takes a dtype.  In fp64 the vertices are _mano_oracle.forward's; in fp32 they come from verts_any below, the
same formulas in the tensors' own dtype, which exists only to measure what fp32 rounding does to a result: the GPU gates
are 4 x the error of this fp32 run against the fp64 run on the same inputs (tests/test_fit_verts.py holds verts_any to
_mano_oracle.forward in fp64)."""
import numpy as np
import torch

import _fit_oracle as FO
import _mano_oracle as MO

U, NM = FO.U, FO.NM
LAMBDA_MIN, LAMBDA_MAX = FO.LAMBDA_MIN, FO.LAMBDA_MAX


def verts_any(model, rots, poses, betas):
    """rows 21.. of _mano_oracle.forward in the inputs' dtype; the model's fp32 arrays are exact in either"""
    dt = rots.dtype
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    vt, sd, pd = T(model.v_template), T(model.shapedirs), T(model.posedirs)
    Jr, W, hm = T(model.J_regressor), T(model.weights), T(model.hands_mean)
    parents = list(model.parents)
    B = rots.shape[0]
    pose = torch.cat([torch.zeros(B, 1, 3, dtype=dt), (hm.reshape(1, 45) + poses).reshape(B, 15, 3)], dim=1)
    R = FO.rodrigues_any(pose.reshape(-1, 3)).reshape(B, 16, 3, 3)
    v_shaped = vt.unsqueeze(0) + torch.einsum("vck,bk->bvc", sd, betas)
    J = torch.einsum("jv,bvc->bjc", Jr, v_shaped)
    pw = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, 135)
    vp = v_shaped + torch.einsum("vck,bk->bvc", pd, pw)
    RG, t = [R[:, 0]], [J[:, 0]]
    for i in range(1, 16):
        p = parents[i]
        RG.append(RG[p] @ R[:, i])
        t.append((RG[p] @ (J[:, i] - J[:, p]).unsqueeze(2)).squeeze(2) + t[p])
    RG, t = torch.stack(RG, 1), torch.stack(t, 1)
    a = t - (RG @ J.unsqueeze(3)).squeeze(3)
    TR = torch.einsum("vi,birc->bvrc", W, RG)
    Ta = torch.einsum("vi,bir->bvr", W, a)
    v = (TR @ vp.unsqueeze(3)).squeeze(3) + Ta
    Rg = FO.rodrigues_any(rots).transpose(1, 2)
    return v @ Rg - t[:, 1:2] @ Rg


def verts(model, P):
    """x(p) [B,V,3] of the first 58 unknowns, joint 1 subtracted, in P's dtype"""
    r, p, b = P[:, 0:3], P[:, 3:48], P[:, 48:58]
    if P.dtype == torch.float64:
        return MO.forward(model, r, p, b)[:, 21:]
    return verts_any(model, r, p, b)


def verts_jac(model, P):
    """-> x [B,V,3], jac [B,3V,58].  Sample b's vertices depend on row b of P alone, so the Jacobian by a perturbation e[58]
    added to every row is every sample's own: 58 forward-mode columns instead of 3 V reverse-mode rows"""
    P = P[:, :NM].detach()
    B = P.shape[0]
    jac = torch.autograd.functional.jacobian(lambda e: verts(model, P + e), torch.zeros(NM, dtype=P.dtype),
                                             strategy="forward-mode", vectorize=True)      # [B,V,3,58]
    with torch.no_grad():
        x = verts(model, P)
    return x, jac.reshape(B, -1, NM).contiguous()


def model_verts(model, P):
    """exp(log_scale) x[v] + trans, [B,V,3]"""
    return torch.exp(P[:, 61]).reshape(-1, 1, 1) * verts(model, P) + P[:, None, 58:61]


def cost(model, P, targets, w, w_pose, w_beta):
    r = model_verts(model, P) - targets
    return (w * (r * r).sum(2)).sum(1) + w_pose * (P[:, 3:48] ** 2).sum(1) + w_beta * (P[:, 48:58] ** 2).sum(1)


def rms(model, P, targets):
    """per sample, the root of the mean squared vertex distance: what the recovery gates hold"""
    with torch.no_grad():
        d = model_verts(model, P.double()) - targets.double()
    return (d * d).sum(2).mean(1).sqrt()


def procrustes_start(model, targets, w):
    """init = 1: zeros for pose and shape, the weighted similarity Procrustes (SVD form) of the zero-pose vertices onto the
    targets for rots, trans, log_scale.  fp64 whatever the targets' dtype, as in the kernel."""
    T, w = targets.double(), w.double()
    B = T.shape[0]
    P = torch.zeros(B, U, dtype=torch.float64)
    X = verts(model, P)
    W = w.sum(1).reshape(B, 1)
    mx, my = (w.unsqueeze(2) * X).sum(1) / W, (w.unsqueeze(2) * T).sum(1) / W
    Xc, Tc = X - mx.unsqueeze(1), T - my.unsqueeze(1)
    K = torch.einsum("bj,bja,bjc->bac", w, Xc, Tc)           # sum_v w x y^T
    Uu, S, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(Vh.transpose(1, 2) @ Uu.transpose(1, 2)))
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1))
    R = Vh.transpose(1, 2) @ D @ Uu.transpose(1, 2)          # y ~ R x
    var = (w * (Xc * Xc).sum(2)).sum(1)
    sc = torch.einsum("bca,bac->b", R, K) / var
    P[:, 0:3] = FO.rot_to_axis_angle(R)
    P[:, 58:61] = my - sc.reshape(B, 1) * (R @ mx.unsqueeze(2)).squeeze(2)
    P[:, 61] = torch.log(sc)
    return P


def normal_equations(model, P, targets, w, w_pose, w_beta, free):
    """-> A [B,62,62] (undamped), g [B,62], cost [B] at P, the frozen unknowns as unit rows with g = 0"""
    B, dt = P.shape[0], P.dtype
    x, jm = verts_jac(model, P)
    V = x.shape[1]
    s = torch.exp(P[:, 61]).reshape(B, 1, 1)
    Jf = torch.zeros(B, 3 * V, U, dtype=dt)
    Jf[:, :, :NM] = s * jm
    Jf[:, :, 58:61] = torch.eye(3, dtype=dt).repeat(V, 1).unsqueeze(0)
    Jf[:, :, 61] = (s * x).reshape(B, 3 * V)
    r = (s * x + P[:, None, 58:61] - targets).reshape(B, 3 * V)
    wr = w.repeat_interleave(3, dim=1)
    prior = torch.zeros(U, dtype=dt)
    prior[3:48], prior[48:58] = w_pose, w_beta
    A = Jf.transpose(1, 2) @ (wr.unsqueeze(2) * Jf) + torch.diag(prior)
    g = (Jf.transpose(1, 2) @ (wr * r).unsqueeze(2)).squeeze(2) + prior * P
    c = (wr * r * r).sum(1) + w_pose * (P[:, 3:48] ** 2).sum(1) + w_beta * (P[:, 48:58] ** 2).sum(1)
    fr = torch.tensor([(free >> i) & 1 for i in range(U)], dtype=torch.bool)
    keep = (fr[:, None] & fr[None, :]).to(dt)
    A = A * keep + torch.diag((~fr).to(dt))
    return A, g * fr.to(dt), c


def lm(model, targets, w, P0, iters, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << U) - 1, history=False):
    """-> P [B,62], cost [B], accepted [B] (and the per-iteration costs [iters,B]) in P0's dtype; _fit_oracle.lm's schedule"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    P = P0.clone()
    B = P.shape[0]
    lam = torch.full((B,), lambda0, dtype=dt)
    acc = torch.zeros(B, dtype=torch.int32)
    fr = torch.tensor([(free >> i) & 1 for i in range(U)], dtype=dt)
    hist, c = [], None
    for _ in range(iters):
        A, g, _ = normal_equations(model, P, targets, w, w_pose, w_beta, free)
        with torch.no_grad():      # by the same expression as the trial's, so that a rejected step leaves the same bits
            c = cost(model, P, targets, w, w_pose, w_beta)
        Ad = A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(Ad)
        ok = info == 0
        L = torch.where(ok.reshape(B, 1, 1), L, torch.eye(U, dtype=dt).expand(B, U, U))
        delta = -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2) * fr
        Pt = P + delta
        with torch.no_grad():
            ct = cost(model, Pt, targets, w, w_pose, w_beta)
        take = ok & torch.isfinite(Pt).all(1) & (ct < c)
        P = torch.where(take.unsqueeze(1), Pt, P)
        c = torch.where(take, ct, c)
        acc += take.to(torch.int32)
        lam = torch.where(take, (lam * 0.1).clamp_min(LAMBDA_MIN), (lam * 10).clamp_max(LAMBDA_MAX))
        hist.append(c.clone())
    return (P, c, acc, torch.stack(hist)) if history else (P, c, acc)


def rel(a, b):
    return MO.rel(a, b)
