"""fp64 torch statement of the MANO fit to keypoints of include/scat_mano_fit_kp.h on top of _fit_oracle.joints: the 3-D
model joints and their weak-perspective projection, the robust cost with priors and limits, the IRLS normal equations
(Jacobian of all 105 residual rows by torch.autograd.functional.jacobian), both closed-form starts and _lm_oracle's
Levenberg-Marquardt loop with the kernel's rules.  Test-only: imports none of scat_amd's kernels.

Everything takes a dtype, as _fit_oracle does: the fp32 run exists only to measure what fp32 rounding does to a result (the
GPU gates are 4 x the error of this fp32 run against the fp64 run on the same inputs).  The starts are solved in fp64
whatever the dtype, as in the kernel, from zero-pose joints computed in the dtype, and their result is rounded to it."""
from typing import NamedTuple, Optional

import numpy as np
import torch

import _fit_oracle as FO
import _lm_oracle as L
import _mano_oracle as MO

U, U3 = 65, 62
LAMBDA_MIN, LAMBDA_MAX = FO.LAMBDA_MIN, FO.LAMBDA_MAX
model_joints, rel = FO.model_joints, MO.rel


class Problem(NamedTuple):
    """one call's data and settings; T3 / T2 None leaves the term out, w3 / w2 None means all ones"""
    joint_map: tuple
    T3: Optional[torch.Tensor] = None       # [B,21,3]
    w3: Optional[torch.Tensor] = None       # [B,21]
    T2: Optional[torch.Tensor] = None       # [B,21,2] pixels
    w2: Optional[torch.Tensor] = None
    lo: Optional[torch.Tensor] = None       # [45]
    hi: Optional[torch.Tensor] = None
    w_pose: float = 1e-6
    w_beta: float = 1e-6
    w_limit: float = 0.0
    sigma3: float = 0.0
    sigma2: float = 0.0
    half: tuple = (112.0, 112.0)            # (half_w, half_h)


def _terms(pr, B, dt):
    """targets and weights of both terms in dt; an absent term has zero targets and zero weights"""
    T3 = torch.zeros(B, 21, 3, dtype=dt) if pr.T3 is None else pr.T3.to(dt)
    T2 = torch.zeros(B, 21, 2, dtype=dt) if pr.T2 is None else pr.T2.to(dt)
    w3 = torch.zeros(B, 21, dtype=dt) if pr.T3 is None else (torch.ones(B, 21, dtype=dt) if pr.w3 is None else pr.w3.to(dt))
    w2 = torch.zeros(B, 21, dtype=dt) if pr.T2 is None else (torch.ones(B, 21, dtype=dt) if pr.w2 is None else pr.w2.to(dt))
    return T3, w3, T2, w2


def project(P, m3, half):
    """u = (cs (m.x + ctx) half_w + half_w, cs (m.y + cty) half_h + half_h), [B,21,2]"""
    h = torch.tensor(half, dtype=P.dtype)
    return (P[:, 62].reshape(-1, 1, 1) * (m3[:, :, :2] + P[:, None, 63:65])) * h + h


def reproject(model, P, joint_map, half):
    return project(P, model_joints(model, P, joint_map), half)


def rho(e, sigma):
    return e if sigma == 0 else (sigma * sigma) * e / (sigma * sigma + e)


def rho_prime(e, sigma):
    return torch.ones_like(e) if sigma == 0 else ((sigma * sigma) / (sigma * sigma + e)) ** 2


def excess(P, pr):
    """signed distance of every pose outside its limits [B,45]: > 0 above hi, < 0 below lo; not finite: no limit"""
    po = P[:, 3:48]
    if pr.lo is None:
        return torch.zeros_like(po)
    lo, hi = pr.lo.to(P.dtype), pr.hi.to(P.dtype)
    lo = torch.where(torch.isfinite(lo), lo, torch.full_like(lo, -float("inf")))
    hi = torch.where(torch.isfinite(hi), hi, torch.full_like(hi, float("inf")))
    return torch.clamp(po - hi, min=0) - torch.clamp(lo - po, min=0)


def residuals(model, P, pr):
    """-> r3 [B,21,3], r2 [B,21,2]"""
    T3, _, T2, _ = _terms(pr, P.shape[0], P.dtype)
    m3 = model_joints(model, P, pr.joint_map)
    return m3 - T3, project(P, m3, pr.half) - T2


def cost(model, P, pr):
    _, w3, _, w2 = _terms(pr, P.shape[0], P.dtype)
    r3, r2 = residuals(model, P, pr)
    c = (w3 * rho((r3 * r3).sum(2), pr.sigma3)).sum(1) + (w2 * rho((r2 * r2).sum(2), pr.sigma2)).sum(1)
    c = c + pr.w_pose * (P[:, 3:48] ** 2).sum(1) + pr.w_beta * (P[:, 48:58] ** 2).sum(1)
    return c + pr.w_limit * (excess(P, pr) ** 2).sum(1)


def free_bits(free, free_cam):
    return [(free >> i) & 1 for i in range(U3)] + [(free_cam >> i) & 1 for i in range(3)]


def normal_equations(model, P, pr, free=(1 << U3) - 1, free_cam=7):
    """-> A [B,65,65] (undamped), g [B,65]: IRLS at P, the frozen unknowns as unit rows with g = 0.  g is half the gradient
    of cost() in the free unknowns."""
    B, dt = P.shape[0], P.dtype
    P = P.detach()
    _, w3, _, w2 = _terms(pr, B, dt)

    def rows(q):
        r3, r2 = residuals(model, q, pr)
        return torch.cat([r3.reshape(B, 63), r2.reshape(B, 42)], dim=1)

    J = torch.autograd.functional.jacobian(lambda q: rows(q).sum(0), P, vectorize=True).permute(1, 0, 2)      # [B,105,65]
    with torch.no_grad():
        r = rows(P)
        e3, e2 = (r[:, :63].reshape(B, 21, 3) ** 2).sum(2), (r[:, 63:].reshape(B, 21, 2) ** 2).sum(2)
        wr = torch.cat([(w3 * rho_prime(e3, pr.sigma3)).repeat_interleave(3, dim=1),
                        (w2 * rho_prime(e2, pr.sigma2)).repeat_interleave(2, dim=1)], dim=1)
        ex = excess(P, pr)
        lim_d, lim_g = torch.zeros(B, U, dtype=dt), torch.zeros(B, U, dtype=dt)
        lim_d[:, 3:48], lim_g[:, 3:48] = pr.w_limit * (ex != 0).to(dt), pr.w_limit * ex
        A, g = L.gauss_newton(J, wr, r, FO.prior_vec(U, dt, pr.w_pose, pr.w_beta), P)
        return L.freeze(A + torch.diag_embed(lim_d), g + lim_g, torch.tensor(free_bits(free, free_cam)))


def lm(model, pr, P0, iters, lambda0=1e-3, free=(1 << U3) - 1, free_cam=7, history=False):
    """-> P [B,65], cost [B], accepted [B] (and the per-iteration costs [iters,B] and iterates [iters,B,65]) in P0's
    dtype: _lm_oracle.lm, which here also rejects a factor that is not finite and runs without gradients throughout"""
    return L.lm(P0, iters, lambda0, lambda P: normal_equations(model, P, pr, free, free_cam), lambda P: cost(model, P, pr),
                torch.tensor(free_bits(free, free_cam), dtype=P0.dtype), finite_factor=True, no_grad=True)[:5 if history else 3]


def _procrustes(X, T, w):
    """weighted similarity of X [21,3] onto T (numpy, fp64) -> R, t, scale; no weight: the identity"""
    W = w.sum()
    if not W > 0:
        return np.eye(3), np.zeros(3), 1.0
    mx, my = (w[:, None] * X).sum(0) / W, (w[:, None] * T).sum(0) / W
    Xc, Tc = X - mx, T - my
    K = np.einsum("j,ja,jc->ac", w, Xc, Tc)
    Uu, S, Vh = np.linalg.svd(K)
    d = np.sign(np.linalg.det(Vh.T @ Uu.T))
    R = Vh.T @ np.diag([1.0, 1.0, d]) @ Uu.T
    sc = np.einsum("ca,ac->", R, K) / (w * (Xc * Xc).sum(1)).sum()
    if not 1e-30 < sc < 1e30:
        sc = 1.0
    return R, my - sc * R @ mx, sc


def _complex_fit(a, y, w):
    """weighted y ~ z a + t over complex a, y -> z, t, residual"""
    W = w.sum()
    ab, yb = (w * a).sum() / W, (w * y).sum() / W
    z = (w * np.conj(a - ab) * (y - yb)).sum() / (w * np.abs(a - ab) ** 2).sum()
    return z, yb - z * ab, (w * np.abs((y - yb) - z * (a - ab)) ** 2).sum()


def start(model, pr, B, dtype=torch.float64, info=None):
    """init = 1 -> P [B,65] in dtype.  The zero-pose joints in dtype, the solve in fp64, the result rounded to dtype.
    info: a list that receives, per sample, "3d" or the index 0 / 1 of the winning 2-D candidate."""
    T3, w3, T2, w2 = (t.double().numpy() for t in _terms(pr, B, torch.float64))
    with torch.no_grad():
        X = FO.joints(model, torch.zeros(B, U3, dtype=dtype))[:, list(pr.joint_map)].double().numpy()
    hw = np.array(pr.half, dtype=np.float64)
    P = torch.zeros(B, U, dtype=torch.float64)
    P[:, 62] = 1.0
    with np.errstate(all="ignore"):
        for b in range(B):
            Y = (T2[b] - hw) / hw
            if w3[b].sum() > 0 or pr.T2 is None:
                R, t, sc = _procrustes(X[b], T3[b], w3[b])
                P[b, 0:3] = FO.rot_to_axis_angle(torch.from_numpy(R).unsqueeze(0))[0]
                P[b, 58:61], P[b, 61] = torch.from_numpy(t), float(np.log(sc))
                tag = "3d"
                if pr.T2 is not None:      # the camera from the model joints at the start as it is stored
                    q = P[b:b + 1].to(dtype).double()
                    Rq = MO.rodrigues(q[:, 0:3])[0].numpy()
                    a = (float(torch.exp(q[0, 61])) * X[b] @ Rq.T + q[0, 58:61].numpy())[:, :2]
                    W = w2[b].sum()
                    ab, yb = (w2[b][:, None] * a).sum(0) / W, (w2[b][:, None] * Y).sum(0) / W
                    cs = (w2[b][:, None] * (a - ab) * (Y - yb)).sum() / (w2[b][:, None] * (a - ab) ** 2).sum()
                    if 1e-30 < cs < 1e30:
                        P[b, 62], P[b, 63:65] = float(cs), torch.from_numpy(yb / cs - ab)
            else:
                y = Y[:, 0] + 1j * Y[:, 1]
                fits = [_complex_fit(sx * X[b][:, 0] + 1j * X[b][:, 1], y, w2[b]) for sx in (1.0, -1.0)]
                k = 1 if fits[1][2] < fits[0][2] else 0
                z, t, _ = fits[k]
                tag = k
                if 1e-30 < abs(z) < 1e30:
                    phi = np.arctan2(z.imag, z.real)
                    c, s = np.cos(phi), np.sin(phi)
                    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) if k == 0 else np.array([[-c, -s, 0], [-s, c, 0], [0, 0, -1.0]])
                    P[b, 0:3] = FO.rot_to_axis_angle(torch.from_numpy(R).unsqueeze(0))[0]
                    P[b, 62], P[b, 63], P[b, 64] = abs(z), (t / abs(z)).real, (t / abs(z)).imag
            if info is not None:
                info.append(tag)
    return P.to(dtype)


def rms3(model, P, T3, joint_map):
    """per sample, the root of the mean squared 3-D joint distance, fp64"""
    return FO.rms(model, P.double(), T3, joint_map)


def rms2(model, P, T2, joint_map, half, sel=None):
    """per sample, the root of the mean squared reprojection distance in pixels, fp64; sel [B,21] bool: those joints only"""
    with torch.no_grad():
        d = ((reproject(model, P.double(), joint_map, half) - T2.double()) ** 2).sum(2)
    if sel is None:
        return d.mean(1).sqrt()
    return ((d * sel).sum(1) / sel.sum(1)).sqrt()
