"""fp64 torch statement of the MANO fit to a full mesh of include/scat_mano_fit_verts.h on top of _mano_oracle.forward:
the model vertices, the cost, the Jacobian (torch.autograd.functional.jacobian, forward mode: 58 columns are fewer than
3 V rows), the vertex rows and the normal equations; the Procrustes start over the vertices and the Levenberg-Marquardt
loop are _lm_oracle's, as for _fit_oracle.  Test-only: imports none of scat_amd's kernels.

Everything takes a dtype.  In fp64 the vertices are _mano_oracle.forward's; in fp32 they come from verts_any below, the
same formulas in the tensors' own dtype, which exists only to measure what fp32 rounding does to a result: the GPU gates
are 4 x the error of this fp32 run against the fp64 run on the same inputs (tests/test_fit_verts.py holds verts_any to
_mano_oracle.forward in fp64)."""
import torch

import _fit_oracle as FO
import _lm_oracle as L
import _mano_oracle as MO

U, NM = FO.U, FO.NM
LAMBDA_MIN, LAMBDA_MAX = FO.LAMBDA_MIN, FO.LAMBDA_MAX
rel = MO.rel


def verts_any(model, rots, poses, betas):
    """rows 21.. of _mano_oracle.forward in the inputs' dtype: the rotated joint 1 subtracted from the rotated vertices"""
    t, v = FO.skinned_any(model, rots, poses, betas, slice(None))
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
    """init = 1: _fit_oracle.similarity_start of the zero-pose vertices, computed in fp64; fp64 whatever the targets' dtype"""
    X = verts(model, torch.zeros(targets.shape[0], U, dtype=torch.float64))
    return FO.similarity_start(X, targets.double(), w.double())


def rows(model, P, targets):
    """_fit_oracle.rows of every vertex: Jf [B,V,3,62] and r [B,V,3]"""
    return FO.rows(*verts_jac(model, P), P, targets)


def normal_equations(model, P, targets, w, w_pose, w_beta, free):
    """-> A [B,62,62] (undamped), g [B,62], cost [B] at P: _fit_oracle.row_equations of the vertices"""
    return FO.row_equations(*rows(model, P, targets), w, P, w_pose, w_beta, free)


def lm(model, targets, w, P0, iters, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << U) - 1, history=False):
    """-> P [B,62], cost [B], accepted [B] (and the per-iteration costs [iters,B]) in P0's dtype: _lm_oracle.lm"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    return L.lm(P0, iters, lambda0, lambda P: normal_equations(model, P, targets, w, w_pose, w_beta, free)[:2],
                lambda P: cost(model, P, targets, w, w_pose, w_beta), L.mask_vec(free, U, dt))[:4 if history else 3]
