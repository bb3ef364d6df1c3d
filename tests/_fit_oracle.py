"""fp64 torch statement of the MANO fit of include/scat_mano_fit.h on top of _mano_oracle.forward: the model joints, the
cost, the Jacobian (torch.autograd.functional.jacobian) and the normal equations; the Procrustes start and the
Levenberg-Marquardt loop with the kernel's rules are _lm_oracle's, which every fit oracle shares.  Test-only: imports
none of scat_amd's kernels.

Everything takes a dtype.  In fp64 the joints are _mano_oracle.forward's; in fp32 they come from joints_any below, the
same formulas in the tensors' own dtype, which exists only to measure what fp32 rounding does to a result: the GPU gates
are 4 x the error of this fp32 run against the fp64 run on the same inputs (tests/test_fit.py holds joints_any to
_mano_oracle.forward in fp64)."""
import numpy as np
import torch

import _lm_oracle as L
import _mano_oracle as MO

U, NM = 62, 58
LAMBDA_MIN, LAMBDA_MAX = L.LAMBDA_MIN, L.LAMBDA_MAX
rel, rot_to_axis_angle = MO.rel, L.rot_to_axis_angle


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


def skinned_any(model, rots, poses, betas, rows):
    """what joints_any and _fit_verts_oracle.verts_any share, in the inputs' dtype (the model's fp32 arrays are exact in either):
    the chain joints t [B,16,3] and the skinned vertices v of rows (a list, or slice(None): all) before the global rotation"""
    dt = rots.dtype
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    vt, sd, pd = T(model.v_template), T(model.shapedirs), T(model.posedirs)
    Jr, W, hm = T(model.J_regressor), T(model.weights), T(model.hands_mean)
    parents = list(model.parents)
    B = rots.shape[0]
    pose = torch.cat([torch.zeros(B, 1, 3, dtype=dt), (hm.reshape(1, 45) + poses).reshape(B, 15, 3)], dim=1)
    R = rodrigues_any(pose.reshape(-1, 3)).reshape(B, 16, 3, 3)
    v_shaped = vt.unsqueeze(0) + torch.einsum("vck,bk->bvc", sd, betas)
    J = torch.einsum("jv,bvc->bjc", Jr, v_shaped)
    pw = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, 135)
    vp = v_shaped[:, rows] + torch.einsum("vck,bk->bvc", pd[rows], pw)
    RG, t = [R[:, 0]], [J[:, 0]]
    for i in range(1, 16):
        p = parents[i]
        RG.append(RG[p] @ R[:, i])
        t.append((RG[p] @ (J[:, i] - J[:, p]).unsqueeze(2)).squeeze(2) + t[p])
    RG, t = torch.stack(RG, 1), torch.stack(t, 1)
    a = t - (RG @ J.unsqueeze(3)).squeeze(3)
    TR = torch.einsum("vi,birc->bvrc", W[rows], RG)
    Ta = torch.einsum("vi,bir->bvr", W[rows], a)
    return t, (TR @ vp.unsqueeze(3)).squeeze(3) + Ta


def joints_any(model, rots, poses, betas):
    """the first 21 rows of _mano_oracle.forward in the inputs' dtype: rotated as one array, then joint 1 subtracted"""
    t, v = skinned_any(model, rots, poses, betas, list(model.tips))
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


def similarity_start(X, targets, w):
    """zeros for pose and shape [B,62] fp64; rots, trans, log_scale: the weighted similarity Procrustes of X onto the targets"""
    P = torch.zeros(targets.shape[0], U, dtype=torch.float64)
    P[:, 0:3], P[:, 58:61], P[:, 61] = L.procrustes(X, targets, w)
    return P


def procrustes_start(model, targets, w, joint_map):
    """init = 1: similarity_start of the zero-pose joints, computed in fp64; fp64 whatever the targets' dtype, as in the kernel"""
    X = joints(model, torch.zeros(targets.shape[0], U, dtype=torch.float64))[:, list(joint_map)]
    return similarity_start(X, targets.double(), w.double())


def prior_vec(n, dt, w_pose, w_beta):
    """the n priors' weights: w_pose on the 45 poses, w_beta on the 10 betas"""
    return L.group_vec(((3, 0.0), (45, w_pose), (10, w_beta), (n - NM, 0.0)), dt)


def rows(x, jm, P, targets):
    """the model's points x [B,K,3] and their Jacobian jm [B,3K,58] -> the rows Jf [B,K,3,62] and residuals r [B,K,3] of
    exp(log_scale) x + trans - targets (targets 0.0: the scaled and moved points themselves)"""
    B, K, dt = x.shape[0], x.shape[1], P.dtype
    s = torch.exp(P[:, 61]).reshape(B, 1, 1)
    Jf = torch.zeros(B, 3 * K, U, dtype=dt)
    Jf[:, :, :NM] = s * jm
    Jf[:, :, 58:61] = torch.eye(3, dtype=dt).repeat(K, 1).unsqueeze(0)
    Jf[:, :, 61] = (s * x).reshape(B, 3 * K)
    return Jf.reshape(B, K, 3, U), s * x + P[:, None, 58:61] - targets


def row_equations(Jf, r, w, P, w_pose, w_beta, free):
    """rows' Jf, r and the points' weights w [B,K] -> A [B,62,62] (undamped), g [B,62], cost [B] at P: the Gauss-Newton
    product with the priors, the frozen unknowns as unit rows with g = 0"""
    B = P.shape[0]
    Jf, r, wr = Jf.reshape(B, -1, U), r.reshape(B, -1), w.repeat_interleave(3, dim=1)
    A, g = L.gauss_newton(Jf, wr, r, prior_vec(U, P.dtype, w_pose, w_beta), P)
    c = (wr * r * r).sum(1) + w_pose * (P[:, 3:48] ** 2).sum(1) + w_beta * (P[:, 48:58] ** 2).sum(1)
    return L.freeze(A, g, L.mask_vec(free, U, P.dtype)) + (c,)


def normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, free):
    """-> A [B,62,62] (undamped), g [B,62], cost [B] at P: row_equations of the mapped joints"""
    x, jm = joints_jac(model, P)
    jmap = list(joint_map)
    Jf, r = rows(x[:, jmap], jm.reshape(-1, 21, 3, NM)[:, jmap].reshape(-1, 63, NM), P, targets)
    return row_equations(Jf, r, w, P, w_pose, w_beta, free)


def lm(model, targets, w, joint_map, P0, iters, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << U) - 1, history=False):
    """-> P [B,62], cost [B], accepted [B] (and the per-iteration costs [iters,B]) in P0's dtype: _lm_oracle.lm"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    return L.lm(P0, iters, lambda0, lambda P: normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, free)[:2],
                lambda P: cost(model, P, targets, w, joint_map, w_pose, w_beta), L.mask_vec(free, U, dt))[:4 if history else 3]


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
