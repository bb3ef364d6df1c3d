"""fp64 torch statement of the MANO fit of include/scat_mano_fit.h on top of _mano_oracle.forward: the model joints, the
cost, the Jacobian (torch.autograd.functional.jacobian), the Procrustes start and the Levenberg-Marquardt loop with the
kernel's rules (Marquardt scaling, accept only if the cost drops, lambda / 10 or x 10 within 1e-12..1e12, a failed
Cholesky is a rejection, frozen unknowns are unit rows).  Test-only: imports none of scat_amd's kernels.

Everything takes a dtype.  In fp64 the joints are _mano_oracle.forward's; in fp32 they come from joints_any below, the
same formulas in the tensors' own dtype, which exists only to measure what fp32 rounding does to a result: the GPU gates
are 4 x the error of this fp32 run against the fp64 run on the same inputs (tests/test_fit.py holds joints_any to
_mano_oracle.forward in fp64)."""
import numpy as np
import torch

import _mano_oracle as MO

U, NM = 62, 58
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12


def rodrigues_any(r):
    """_mano_oracle.rodrigues in r's dtype, the kernel's series switch (theta^2 = 0.25, terms to theta^8) in fp32"""
    if r.dtype == torch.float64:
        return MO.rodrigues(r)
    t = (r * r).sum(-1)
    small = t < 0.25
    ts = torch.where(small, torch.ones_like(t), t)
    th = ts.sqrt()
    a = torch.where(small, 1 + t * (-1 / 6 + t * (1 / 120 + t * (-1 / 5040 + t * (1 / 362880)))), torch.sin(th) / th)
    b = torch.where(small, 0.5 + t * (-1 / 24 + t * (1 / 720 + t * (-1 / 40320 + t * (1 / 3628800)))),
                    2.0 * torch.sin(0.5 * th) ** 2 / ts)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    o = torch.zeros_like(x)
    S = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=r.dtype).unsqueeze(0)
    S2 = r.unsqueeze(2) * r.unsqueeze(1) - t.reshape(-1, 1, 1) * eye
    return eye + a.reshape(-1, 1, 1) * S + b.reshape(-1, 1, 1) * S2


def joints_any(model, rots, poses, betas):
    """the first 21 rows of _mano_oracle.forward in the inputs' dtype; the model's fp32 arrays are exact in either"""
    dt = rots.dtype
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    vt, sd, pd = T(model.v_template), T(model.shapedirs), T(model.posedirs)
    Jr, W, hm = T(model.J_regressor), T(model.weights), T(model.hands_mean)
    parents, tips = list(model.parents), list(model.tips)
    B = rots.shape[0]
    pose = torch.cat([torch.zeros(B, 1, 3, dtype=dt), (hm.reshape(1, 45) + poses).reshape(B, 15, 3)], dim=1)
    R = rodrigues_any(pose.reshape(-1, 3)).reshape(B, 16, 3, 3)
    v_shaped = vt.unsqueeze(0) + torch.einsum("vck,bk->bvc", sd, betas)
    J = torch.einsum("jv,bvc->bjc", Jr, v_shaped)
    pw = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, 135)
    vp = v_shaped[:, tips] + torch.einsum("vck,bk->bvc", pd[tips], pw)
    RG, t = [R[:, 0]], [J[:, 0]]
    for i in range(1, 16):
        p = parents[i]
        RG.append(RG[p] @ R[:, i])
        t.append((RG[p] @ (J[:, i] - J[:, p]).unsqueeze(2)).squeeze(2) + t[p])
    RG, t = torch.stack(RG, 1), torch.stack(t, 1)
    a = t - (RG @ J.unsqueeze(3)).squeeze(3)
    TR = torch.einsum("vi,birc->bvrc", W[tips], RG)
    Ta = torch.einsum("vi,bir->bvr", W[tips], a)
    v = (TR @ vp.unsqueeze(3)).squeeze(3) + Ta
    x = torch.cat([t, v], dim=1) @ rodrigues_any(rots).transpose(1, 2)
    return x - x[:, 1:2]


def joints(model, P):
    """x(p) [B,21,3] of the first 58 unknowns, joint 1 at the origin, in P's dtype"""
    r, p, b = P[:, 0:3], P[:, 3:48], P[:, 48:58]
    if P.dtype == torch.float64:
        return MO.forward(model, r, p, b)[:, :21]
    return joints_any(model, r, p, b)


def joints_jac(model, P):
    """-> x [B,21,3], jac [B,63,58]; one reverse pass per output row over the whole batch (samples are independent)"""
    P = P[:, :NM].detach()
    B = P.shape[0]
    jac = torch.autograd.functional.jacobian(lambda q: joints(model, q).reshape(B, 63).sum(0), P)      # [63,B,58]
    with torch.no_grad():
        x = joints(model, P)
    return x, jac.permute(1, 0, 2).contiguous()


def model_joints(model, P, joint_map):
    """exp(log_scale) x[joint_map[j]] + trans, [B,21,3]"""
    return torch.exp(P[:, 61]).reshape(-1, 1, 1) * joints(model, P)[:, list(joint_map)] + P[:, None, 58:61]


def cost(model, P, targets, w, joint_map, w_pose, w_beta):
    r = model_joints(model, P, joint_map) - targets
    return (w * (r * r).sum(2)).sum(1) + w_pose * (P[:, 3:48] ** 2).sum(1) + w_beta * (P[:, 48:58] ** 2).sum(1)


def rms(model, P, targets, joint_map):
    """per sample, the root of the mean squared joint distance: what the recovery gates hold"""
    with torch.no_grad():
        d = model_joints(model, P.double(), joint_map) - targets.double()
    return (d * d).sum(2).mean(1).sqrt()


def rot_to_axis_angle(R):
    """[B,3,3] -> [B,3] through the unit quaternion with w >= 0: 2 atan2(|v|, w) v / |v|, accurate at 0 and at pi"""
    out = []
    for M in R.double().numpy():
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr > 0:
            S = 2 * np.sqrt(tr + 1)
            q = [S / 4, (M[2, 1] - M[1, 2]) / S, (M[0, 2] - M[2, 0]) / S, (M[1, 0] - M[0, 1]) / S]
        elif M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
            S = 2 * np.sqrt(1 + M[0, 0] - M[1, 1] - M[2, 2])
            q = [(M[2, 1] - M[1, 2]) / S, S / 4, (M[0, 1] + M[1, 0]) / S, (M[0, 2] + M[2, 0]) / S]
        elif M[1, 1] > M[2, 2]:
            S = 2 * np.sqrt(1 + M[1, 1] - M[0, 0] - M[2, 2])
            q = [(M[0, 2] - M[2, 0]) / S, (M[0, 1] + M[1, 0]) / S, S / 4, (M[1, 2] + M[2, 1]) / S]
        else:
            S = 2 * np.sqrt(1 + M[2, 2] - M[0, 0] - M[1, 1])
            q = [(M[1, 0] - M[0, 1]) / S, (M[0, 2] + M[2, 0]) / S, (M[1, 2] + M[2, 1]) / S, S / 4]
        q = np.array(q) * (1.0 if q[0] >= 0 else -1.0)
        n = np.linalg.norm(q[1:])
        out.append(q[1:] * (2 * np.arctan2(n, q[0]) / n if n > 1e-12 else 2.0))
    return torch.tensor(np.array(out), dtype=torch.float64)


def procrustes_start(model, targets, w, joint_map):
    """init = 1: zeros for pose and shape, the weighted similarity Procrustes (SVD form) of the zero-pose joints onto the
    targets for rots, trans, log_scale.  fp64 whatever the targets' dtype, as in the kernel."""
    T, w = targets.double(), w.double()
    B = T.shape[0]
    P = torch.zeros(B, U, dtype=torch.float64)
    X = joints(model, P)[:, list(joint_map)]
    W = w.sum(1).reshape(B, 1)
    mx, my = (w.unsqueeze(2) * X).sum(1) / W, (w.unsqueeze(2) * T).sum(1) / W
    Xc, Tc = X - mx.unsqueeze(1), T - my.unsqueeze(1)
    K = torch.einsum("bj,bja,bjc->bac", w, Xc, Tc)           # sum_j w x y^T
    Uu, S, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(Vh.transpose(1, 2) @ Uu.transpose(1, 2)))
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1))
    R = Vh.transpose(1, 2) @ D @ Uu.transpose(1, 2)          # y ~ R x
    var = (w * (Xc * Xc).sum(2)).sum(1)
    sc = torch.einsum("bca,bac->b", R, K) / var
    P[:, 0:3] = rot_to_axis_angle(R)
    P[:, 58:61] = my - sc.reshape(B, 1) * (R @ mx.unsqueeze(2)).squeeze(2)
    P[:, 61] = torch.log(sc)
    return P


def normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, free):
    """-> A [B,62,62] (undamped), g [B,62], cost [B] at P, the frozen unknowns as unit rows with g = 0"""
    B, dt = P.shape[0], P.dtype
    x, jm = joints_jac(model, P)
    jmap = list(joint_map)
    s = torch.exp(P[:, 61]).reshape(B, 1, 1)
    xm = x[:, jmap]
    Jf = torch.zeros(B, 63, U, dtype=dt)
    Jf[:, :, :NM] = s * jm.reshape(B, 21, 3, NM)[:, jmap].reshape(B, 63, NM)
    Jf[:, :, 58:61] = torch.eye(3, dtype=dt).repeat(21, 1).unsqueeze(0)
    Jf[:, :, 61] = (s * xm).reshape(B, 63)
    r = (s * xm + P[:, None, 58:61] - targets).reshape(B, 63)
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


def lm(model, targets, w, joint_map, P0, iters, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << U) - 1, history=False):
    """-> P [B,62], cost [B], accepted [B] (and the per-iteration costs [iters,B]) in P0's dtype"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    P = P0.clone()
    B = P.shape[0]
    lam = torch.full((B,), lambda0, dtype=dt)
    acc = torch.zeros(B, dtype=torch.int32)
    fr = torch.tensor([(free >> i) & 1 for i in range(U)], dtype=dt)
    hist, c = [], None
    for _ in range(iters):
        A, g, _ = normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, free)
        with torch.no_grad():      # by the same expression as the trial's, so that a rejected step leaves the same bits
            c = cost(model, P, targets, w, joint_map, w_pose, w_beta)
        Ad = A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(Ad)
        ok = info == 0
        L = torch.where(ok.reshape(B, 1, 1), L, torch.eye(U, dtype=dt).expand(B, U, U))
        delta = -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2) * fr
        Pt = P + delta
        with torch.no_grad():
            ct = cost(model, Pt, targets, w, joint_map, w_pose, w_beta)
        take = ok & torch.isfinite(Pt).all(1) & (ct < c)
        P = torch.where(take.unsqueeze(1), Pt, P)
        c = torch.where(take, ct, c)
        acc += take.to(torch.int32)
        lam = torch.where(take, (lam * 0.1).clamp_min(LAMBDA_MIN), (lam * 10).clamp_max(LAMBDA_MAX))
        hist.append(c.clone())
    return (P, c, acc, torch.stack(hist)) if history else (P, c, acc)


def seeded_case(seed, B, model, joint_map):
    """the recovery distributions: rots sd 0.8, poses sd 0.4, betas sd 1, trans sd 0.05, log_scale sd 0.2 -> the true
    parameters P [B,62] (fp64, exactly representable in fp32) and the targets they give, rounded to fp32"""
    from scat_amd import synth

    P = np.concatenate([synth.normal_like(seed, "fit.rots", (B, 3), 0.8), synth.normal_like(seed, "fit.poses", (B, 45), 0.4),
                        synth.normal_like(seed, "fit.betas", (B, 10), 1.0), synth.normal_like(seed, "fit.trans", (B, 3), 0.05),
                        synth.normal_like(seed, "fit.log_scale", (B, 1), 0.2)], axis=1)
    P = torch.from_numpy(P.astype(np.float32)).double()
    with torch.no_grad():
        T = model_joints(model, P, joint_map).float()
    return P, T


def rel(a, b):
    return MO.rel(a, b)
