"""fp64 torch statement of the MANO fit to multi-view keypoints of include_ext/scat_mano_fit_views.h on top of
_fit_oracle.model_joints: the joints in every calibrated camera and their pinhole projection, the robust cost with priors
and limits, the IRLS normal equations from the STACKED 42 C rows (Jacobian by torch.autograd.functional.jacobian; the
per-joint 3 x 3 form of the kernel is metric_equations, held to the stacked form by tests/test_fit_views.py), the
triangulation, the start and _lm_oracle's Levenberg-Marquardt loop with the kernel's rules.  Test-only: imports none of
scat_amd's kernels.

Everything takes a dtype, as _fit_oracle does: the fp32 run exists only to measure what fp32 rounding does to a result (the
GPU gates are 4 x the error of this fp32 run against the fp64 run on the same inputs).  The triangulation and the
Procrustes are solved in fp64 whatever the dtype, as in the kernel; the triangulated joints are rounded to the dtype, as
the kernel stores them in fp32, and so is the start."""
from typing import NamedTuple, Optional

import numpy as np
import torch

import _fit_kp_oracle as KO
import _fit_oracle as FO
import _lm_oracle as L
import _mano_oracle as MO

U = 62
model_joints, rel, rho, rho_prime, excess = FO.model_joints, MO.rel, KO.rho, KO.rho_prime, KO.excess


class Problem(NamedTuple):
    """one call's data and settings; w2 None means all ones; cams [1,C,16] is one rig for the batch"""
    joint_map: tuple
    cams: torch.Tensor                      # [Bc,C,16]: R row-major, t, fx, fy, cx, cy
    T2: torch.Tensor                        # [B,C,21,2] pixels
    w2: Optional[torch.Tensor] = None       # [B,C,21]
    lo: Optional[torch.Tensor] = None       # [45]
    hi: Optional[torch.Tensor] = None
    w_pose: float = 1e-2
    w_beta: float = 1e-2
    w_limit: float = 0.0
    sigma2: float = 0.0
    z_near: float = 1e-3


def rig(pr, B, dt):
    """-> R [B,C,3,3], t [B,C,3], K [B,C,4] in dt"""
    c = pr.cams.to(dt).expand(B, -1, -1)
    return c[:, :, :9].reshape(B, -1, 3, 3), c[:, :, 9:12], c[:, :, 12:16]


def weights(pr, dt):
    return torch.ones(pr.T2.shape[:3], dtype=dt) if pr.w2 is None else pr.w2.to(dt)


def in_camera(m3, R, t):
    """q = R_c m_j + t_c, [B,C,21,3]"""
    return torch.einsum("bcik,bjk->bcji", R, m3) + t[:, :, None, :]


def pinhole(q, K, z=None):
    """u = (fx q.x / q.z + cx, fy q.y / q.z + cy), [B,C,21,2]; z: what to divide by instead of q.z"""
    z = q[..., 2] if z is None else z
    return torch.stack([K[:, :, None, 0] * q[..., 0] / z + K[:, :, None, 2], K[:, :, None, 1] * q[..., 1] / z + K[:, :, None, 3]], dim=-1)


def reproject(model, P, pr):
    """the model joints at P in every view, [B,C,21,2], no rule applied"""
    R, t, K = rig(pr, P.shape[0], P.dtype)
    return pinhole(in_camera(model_joints(model, P, pr.joint_map), R, t), K)


def terms(model, P, pr):
    """-> r [B,C,21,2], w [B,C,21] with zero for a view-joint that does not count, behind [B]: a view-joint of positive
    weight has q.z <= z_near (its rows are left out of r's sums: the sample's cost is +inf anyway)"""
    B, dt = P.shape[0], P.dtype
    R, t, K = rig(pr, B, dt)
    q = in_camera(model_joints(model, P, pr.joint_map), R, t)
    w = weights(pr, dt)
    front = q[..., 2] > pr.z_near
    live = (w > 0) & front
    u = pinhole(q, K, torch.where(live, q[..., 2], torch.ones_like(q[..., 2])))
    r = torch.where(live.unsqueeze(-1), u - pr.T2.to(dt), torch.zeros_like(u))
    return r, torch.where(live, w, torch.zeros_like(w)), ((w > 0) & ~front).flatten(1).any(1)


def cost(model, P, pr):
    """[B]; +inf for a sample with a view-joint behind a camera.  Views ascending inside a joint, joints ascending"""
    r, w, behind = terms(model, P, pr)
    c = (w * rho((r * r).sum(3), pr.sigma2)).sum(1).sum(1)
    c = c + pr.w_pose * (P[:, 3:48] ** 2).sum(1) + pr.w_beta * (P[:, 48:58] ** 2).sum(1)
    c = c + pr.w_limit * (excess(P, pr) ** 2).sum(1)
    return torch.where(behind, torch.full_like(c, float("inf")), c)


def _limits(P, pr):
    ex = excess(P, pr)
    d, g = torch.zeros_like(P), torch.zeros_like(P)
    d[:, 3:48], g[:, 3:48] = pr.w_limit * (ex != 0).to(P.dtype), pr.w_limit * ex
    return torch.diag_embed(d), g


def stacked_rows(model, P, pr):
    """-> J [B,42C,62], r [B,42C], wr [B,42C]: every view-joint's two rows, view-major, with their IRLS weights"""
    B = P.shape[0]
    P = P.detach()
    J = torch.autograd.functional.jacobian(lambda q: terms(model, q, pr)[0].reshape(B, -1).sum(0), P, vectorize=True).permute(1, 0, 2)
    with torch.no_grad():
        r, w, _ = terms(model, P, pr)
        wr = (w * rho_prime((r * r).sum(3), pr.sigma2)).repeat_interleave(2, dim=2)
    return J, r.reshape(B, -1), wr.reshape(B, -1)


def normal_equations(model, P, pr, free=(1 << U) - 1):
    """-> A [B,62,62] (undamped), g [B,62]: IRLS at P from the stacked rows, the frozen unknowns as unit rows with g = 0"""
    J, r, wr = stacked_rows(model, P, pr)
    with torch.no_grad():
        A, g = L.gauss_newton(J, wr, r, FO.prior_vec(U, P.dtype, pr.w_pose, pr.w_beta), P.detach())
        dA, dg = _limits(P.detach(), pr)
        return L.freeze(A + dA, g + dg, L.mask_vec(free, U, P.dtype))


def metric_equations(model, P, pr, free=(1 << U) - 1):
    """the same from the kernel's form: M_j = sum_c wi P^T P, h_j = sum_c wi P^T r with P = D R_c, then
    A = sum_j G_j^T M_j G_j, g = sum_j G_j^T h_j on the 63 x 62 Jacobian G of the model joints"""
    B, dt = P.shape[0], P.dtype
    P = P.detach()
    G = torch.autograd.functional.jacobian(lambda q: model_joints(model, q, pr.joint_map).reshape(B, 63).sum(0), P,
                                           vectorize=True).permute(1, 0, 2).reshape(B, 21, 3, U)
    with torch.no_grad():
        R, t, K = rig(pr, B, dt)
        q = in_camera(model_joints(model, P, pr.joint_map), R, t)
        r, w, _ = terms(model, P, pr)
        wi = w * rho_prime((r * r).sum(3), pr.sigma2)
        z = torch.where(w > 0, q[..., 2], torch.ones_like(q[..., 2]))
        D = torch.zeros(B, q.shape[1], 21, 2, 3, dtype=dt)
        D[..., 0, 0], D[..., 0, 2] = K[:, :, None, 0] / z, -K[:, :, None, 0] * q[..., 0] / z ** 2
        D[..., 1, 1], D[..., 1, 2] = K[:, :, None, 1] / z, -K[:, :, None, 1] * q[..., 1] / z ** 2
        Pm = D @ R[:, :, None]                                                           # [B,C,21,2,3]
        M = (wi[..., None, None] * (Pm.transpose(-1, -2) @ Pm)).sum(1)                   # [B,21,3,3]
        h = (wi[..., None] * (Pm.transpose(-1, -2) @ r.unsqueeze(-1)).squeeze(-1)).sum(1)   # [B,21,3]
        A = (G.transpose(-1, -2) @ M @ G).sum(1) + torch.diag(FO.prior_vec(U, dt, pr.w_pose, pr.w_beta))
        g = (G.transpose(-1, -2) @ h.unsqueeze(-1)).squeeze(-1).sum(1) + FO.prior_vec(U, dt, pr.w_pose, pr.w_beta) * P
        dA, dg = _limits(P, pr)
        return L.freeze(A + dA, g + dg, L.mask_vec(free, U, dt))


def usable(pr):
    """[B] bool: every keypoint, weight and camera entry of the sample is finite and no weight is negative"""
    B = pr.T2.shape[0]
    ok = torch.isfinite(pr.T2).flatten(1).all(1) & torch.isfinite(pr.cams).expand(B, -1, -1).flatten(1).all(1)
    if pr.w2 is not None:
        ok = ok & (torch.isfinite(pr.w2) & (pr.w2 >= 0)).flatten(1).all(1)
    return ok


def lm(model, pr, P0, iters, lambda0=1e-3, free=(1 << U) - 1, history=False):
    """-> P [B,62], cost [B], accepted [B] (and the per-iteration costs and iterates) in P0's dtype: _lm_oracle.lm.  A
    sample that is unusable, or behind a camera at P0, is not fitted: P0, +inf, 0.  A trial behind a camera costs +inf
    and is rejected."""
    out = list(L.lm(P0, iters, lambda0, lambda P: normal_equations(model, P, pr, free), lambda P: cost(model, P, pr),
                    L.mask_vec(free, U, P0.dtype), finite_factor=True, no_grad=True))
    with torch.no_grad():
        skip = ~usable(pr) | ~torch.isfinite(cost(model, P0, pr))
    out[0] = torch.where(skip[:, None], P0, out[0])
    out[1] = torch.where(skip, torch.full_like(out[1], float("inf")), out[1])
    out[2] = torch.where(skip, torch.zeros_like(out[2]), out[2])
    return tuple(out[:5 if history else 3])


def triangulate(pr, dtype=torch.float64):
    """-> points [B,21,3] in dtype, valid [B,21] bool: per joint the least squares point of its views' rays, in fp64 (numpy)
    whatever the dtype and rounded to it at the end, with the kernel's three conditions; an unusable sample has no valid joint"""
    B, C = pr.T2.shape[:2]
    R, t, K = (a.numpy() for a in rig(pr, B, torch.float64))
    T2, w = pr.T2.double().numpy(), weights(pr, torch.float64).numpy()
    ok = usable(pr).numpy()
    pts, valid = np.zeros((B, 21, 3)), np.zeros((B, 21), dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            for j in range(21):
                views = [c for c in range(C) if w[b, c, j] > 0]
                if not ok[b] or len(views) < 2:
                    continue
                S, rhs = np.zeros((3, 3)), np.zeros(3)
                for c in views:
                    d = R[b, c].T @ np.array([(T2[b, c, j, 0] - K[b, c, 2]) / K[b, c, 0], (T2[b, c, j, 1] - K[b, c, 3]) / K[b, c, 1], 1.0])
                    d /= np.linalg.norm(d)
                    Pm = np.eye(3) - np.outer(d, d)
                    S += w[b, c, j] * Pm
                    rhs += w[b, c, j] * Pm @ (-R[b, c].T @ t[b, c])
                floor, Lf, good = 1e-6 * np.trace(S), np.zeros((3, 3)), True
                for k in range(3):      # the factor by columns, every pivot held against the trace
                    piv = S[k, k] - (Lf[k, :k] ** 2).sum()
                    if not piv > floor:
                        good = False
                        break
                    Lf[k, k] = np.sqrt(piv)
                    for i in range(k + 1, 3):
                        Lf[i, k] = (S[i, k] - (Lf[i, :k] * Lf[k, :k]).sum()) / Lf[k, k]
                if not good:
                    continue
                X = np.linalg.solve(Lf.T, np.linalg.solve(Lf, rhs))
                if all((R[b, c] @ X + t[b, c])[2] > pr.z_near for c in views):
                    pts[b, j], valid[b, j] = X, True
    return torch.from_numpy(pts).to(dtype), torch.from_numpy(valid)


def start(model, pr, dtype=torch.float64):
    """init = 1 -> P [B,62] in dtype, fitted [B] bool: Procrustes (fp64) of the zero-pose joints, computed in dtype, onto the
    triangulated joints with weight 1 where valid; fewer than 3 valid joints: zeros, not fitted"""
    B = pr.T2.shape[0]
    pts, valid = triangulate(pr, dtype)
    pts = pts.double()
    with torch.no_grad():
        X = FO.joints(model, torch.zeros(B, U, dtype=dtype))[:, list(pr.joint_map)].double()
    fitted = valid.sum(1) >= 3
    P = torch.zeros(B, U, dtype=torch.float64)
    if bool(fitted.any()):
        P[fitted] = FO.similarity_start(X[fitted], pts[fitted], valid[fitted].double())
    return P.to(dtype), fitted


def joint_rms(model, P, pr, X3):
    """per sample, the root of the mean squared distance of the model joints at P to X3 [B,21,3], fp64"""
    return FO.rms(model, P.double(), X3, pr.joint_map)


def pixel_rms(model, P, pr, T2, sel=None):
    """per sample, the root of the mean squared reprojection distance to T2 [B,C,21,2] in pixels, fp64; sel [B,C,21] bool:
    those view-joints only"""
    with torch.no_grad():
        d = ((reproject(model, P.double(), pr) - T2.double()) ** 2).sum(3)
    if sel is None:
        return d.flatten(1).mean(1).sqrt()
    return ((d * sel).flatten(1).sum(1) / sel.flatten(1).sum(1)).sqrt()
