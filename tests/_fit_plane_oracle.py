"""fp64 statement of the MANO fit to a surface point cloud of include/scat_mano_fit_plane.h: the vertex normals (numpy,
np.add.at in CSR order), the metric normal equations and Levenberg-Marquardt with _fit_verts_oracle.lm's schedule, the
point-to-plane ICP loop around _fit_points_oracle.assign, and the per-point metric normal equations that the per-vertex
form replaces.  Test-only: imports none of scat_amd's kernels.

normals follows the header rule for rule: differences, cross products (each product and difference rounded once), their
sum over vf_idx[vf_off[v] : vf_off[v+1]] in that order (np.add.at is unbuffered and walks its indices in order),
|s|^2 = (sx sx + sy sy) + sz sz, the quotients s / |s|; zero where |s|^2 is zero or not finite.  round32 rounds the
quotients to fp32 as the kernel does.  The solver's functions take a dtype like _fit_verts_oracle's, to measure what fp32
rounding does to a result."""
import numpy as np
import torch

import _fit_oracle as FO
import _fit_points_oracle as PO
import _fit_verts_oracle as VO
import _lm_oracle as L

U = VO.U


def normals(verts, faces, vf_off, vf_idx, round32=False):
    """verts [B,V,3] of any float dtype, taken to fp64 as they are; faces [F,3], vf_off [V+1], vf_idx [3F] -> [B,V,3] fp64"""
    x = np.asarray(verts, dtype=np.float64)
    B, V = x.shape[:2]
    faces, vf_off, vf_idx = (np.asarray(a, dtype=np.int64) for a in (faces, vf_off, vf_idx))
    F = faces.shape[0]
    off = np.clip(vf_off, 0, 3 * F)
    own = np.repeat(np.arange(V), np.maximum(np.diff(off), 0))          # the vertex of every CSR entry, ascending
    ent = np.concatenate([np.arange(off[v], max(off[v + 1], off[v])) for v in range(V)]) if V else np.zeros(0, np.int64)
    f = vf_idx[ent.astype(np.int64)]
    ok = (f >= 0) & (f < F)
    fc = faces[np.where(ok, f, 0)]
    ok &= ((fc >= 0) & (fc < V)).all(1)
    own, fc = own[ok], fc[ok]
    out = np.zeros((B, V, 3))
    for b in range(B):
        s = np.zeros((V, 3))
        with np.errstate(invalid="ignore", over="ignore"):
            u, w = x[b, fc[:, 1]] - x[b, fc[:, 0]], x[b, fc[:, 2]] - x[b, fc[:, 0]]
            cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                           u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
            np.add.at(s, own, cr)
            l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
            good = (l2 > 0) & np.isfinite(l2)
            out[b] = np.where(good[:, None], s / np.sqrt(np.where(good, l2, 1.0))[:, None], 0.0)
    return out.astype(np.float32).astype(np.float64) if round32 else out


def brute_normals(verts, faces, vf_off, vf_idx):
    """the same by a loop over python floats: what normals is held to at a small size"""
    x = np.asarray(verts, dtype=np.float64)
    B, V = x.shape[:2]
    F = len(faces)
    out = np.zeros((B, V, 3))
    for b in range(B):
        for v in range(V):
            s = [0.0, 0.0, 0.0]
            for k in range(max(int(vf_off[v]), 0), min(int(vf_off[v + 1]), 3 * F)):
                f = int(vf_idx[k])
                if not 0 <= f < F:
                    continue
                ia, ib, ic = (int(i) for i in faces[f])
                if not (0 <= ia < V and 0 <= ib < V and 0 <= ic < V):
                    continue
                a = [float(t) for t in x[b, ia]]
                u = [float(x[b, ib, c]) - a[c] for c in range(3)]
                w = [float(x[b, ic, c]) - a[c] for c in range(3)]
                s[0] += u[1] * w[2] - u[2] * w[1]
                s[1] += u[2] * w[0] - u[0] * w[2]
                s[2] += u[0] * w[1] - u[1] * w[0]
            l2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
            if l2 > 0 and np.isfinite(l2):
                out[b, v] = [c / np.sqrt(l2) for c in s]
    return out


def flat(n):
    """[B,V] bool: the zero normals, whose metric is the identity"""
    return (n == 0).all(-1)


def metric(n, tau):
    """M = n n^T + tau (I - n n^T) [B,V,3,3]; I for a zero normal"""
    nn = n.unsqueeze(-1) * n.unsqueeze(-2)
    eye = torch.eye(3, dtype=n.dtype).expand_as(nn)
    return torch.where(flat(n)[..., None, None], eye, nn + tau * (eye - nn))


def sqrt_metric(n, tau):
    """a I + (1 - a) n n^T, a = sqrt(tau) [B,V,3,3]; I for a zero normal"""
    a = float(np.sqrt(tau))
    nn = n.unsqueeze(-1) * n.unsqueeze(-2)
    eye = torch.eye(3, dtype=n.dtype).expand_as(nn)
    return torch.where(flat(n)[..., None, None], eye, a * eye + (1.0 - a) * nn)


def rho(r, n, tau):
    """tau |r|^2 + (1 - tau) (n . r)^2 [B,V]; |r|^2 for a zero normal"""
    r2, nr = (r * r).sum(-1), (n * r).sum(-1)
    return torch.where(flat(n), r2, tau * r2 + (1.0 - tau) * nr * nr)


def priors(P, w_pose, w_beta):
    return w_pose * (P[:, 3:48] ** 2).sum(1) + w_beta * (P[:, 48:58] ** 2).sum(1)


def cost(model, P, targets, w, n, tau, w_pose, w_beta):
    return (w * rho(VO.model_verts(model, P) - targets, n, tau)).sum(1) + priors(P, w_pose, w_beta)


def normal_equations(model, P, targets, w, n, tau, w_pose, w_beta, free):
    """-> A [B,62,62] (undamped), g [B,62], cost [B] at P: the weighted rows of every vertex through sqrt(M_v), the frozen
    unknowns as unit rows with g = 0"""
    B = P.shape[0]
    Jf, r = VO.rows(model, P, targets)
    S = sqrt_metric(n, tau)
    Jt, rt = (S @ Jf).reshape(B, -1, U), (S @ r.unsqueeze(-1)).squeeze(-1).reshape(B, -1)
    A, g = L.gauss_newton(Jt, w.repeat_interleave(3, dim=1), rt, FO.prior_vec(U, P.dtype, w_pose, w_beta), P)
    return L.freeze(A, g, L.mask_vec(free, U, P.dtype)) + ((w * rho(r, n, tau)).sum(1) + priors(P, w_pose, w_beta),)


def lm(model, targets, w, n, tau, P0, iters, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << U) - 1, history=False):
    """-> P [B,62], cost [B], accepted [B] (and the per-iteration costs [iters,B]) in P0's dtype: _lm_oracle.lm"""
    dt = P0.dtype
    targets, w, n = targets.to(dt), w.to(dt), n.to(dt)
    return L.lm(P0, iters, lambda0, lambda P: normal_equations(model, P, targets, w, n, tau, w_pose, w_beta, free)[:2],
                lambda P: cost(model, P, targets, w, n, tau, w_pose, w_beta), L.mask_vec(free, U, dt))[:4 if history else 3]


def assign_cost(verts, points, weights, idx, matched, n, tau):
    """the metric data cost [B] of an assignment, by the header's expressions on the numbers it is given: d2 as
    _fit_points_oracle.d2_table, nr = (nx rx + ny ry) + nz rz with r = q - x, rho = tau d2 + (1 - tau) (nr nr), d2 for a
    zero normal; +inf where the assignment is unusable (its idx are all -1 and nothing is matched is NOT that: 0)"""
    verts, points, n = (np.asarray(a, dtype=np.float64) for a in (verts, points, n))
    B, N = points.shape[:2]
    w = np.ones((B, N)) if weights is None else np.asarray(weights, dtype=np.float64)
    tau = np.float64(tau)
    out = np.zeros(B)
    for b in range(B):
        m = np.nonzero(matched[b])[0]
        c = idx[b, m]
        r = points[b, m] - verts[b, c]
        d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        nv = n[b, c]
        nr = (nv[:, 0] * r[:, 0] + nv[:, 1] * r[:, 1]) + nv[:, 2] * r[:, 2]
        zero = (nv == 0).all(1)
        out[b] = (w[b, m] * np.where(zero, d2, tau * d2 + (1.0 - tau) * (nr * nr))).sum()
    return out


def icp(model, points, weights, P0, topo, rounds, iters, tau, max_dist=np.inf, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6,
        free=(1 << U) - 1, history=False):
    """-> P [B,62] fp64, accepted [B], the metric data cost of every assignment [rounds + 1, B] (the last one at the
    returned P) and that last assignment; with history also the P of every assignment.  A round: _fit_points_oracle.assign
    at P's model points (fp64), their normals for topo = (faces, vf_off, vf_idx), then lm above on (vtarget, vw, normals);
    a hand with a NaN vw row keeps its P"""
    return PO.icp_loop(model, points, weights, P0, rounds, max_dist, history,
                       lambda vt, vw, n, P: lm(model, vt, vw, torch.from_numpy(n), tau, P, iters, lambda0, w_pose, w_beta, free),
                       lambda x: normals(x, *topo),
                       lambda x, a, n: assign_cost(x, points, weights, a["idx"], a["matched"], n, tau))


def point_normal_equations(model, P, points, weights, idx, matched, n, tau, w_pose, w_beta):
    """the Gauss-Newton system of sum_n w_n r_n^T M_c(n) r_n + priors with one row triple per matched point (rows J_c(n),
    residual model_c(n) - q_n, the metric M itself between them) -> A [B,62,62], g [B,62], cost [B]: what the per-vertex
    form with sqrt(M) on its rows must reproduce"""
    Jf, mv = VO.rows(model, P, 0.0)
    M = metric(n, tau)
    prior = FO.prior_vec(U, P.dtype, w_pose, w_beta)
    A, g, c = [], [], []
    for b in range(P.shape[0]):
        m = np.nonzero(matched[b])[0]
        cv = torch.from_numpy(idx[b, m].astype(np.int64))
        w = torch.from_numpy(np.asarray(weights[b, m], dtype=np.float64))
        J, Mb = Jf[b][cv], M[b][cv]                                   # [n,3,62], [n,3,3]
        r = mv[b][cv] - torch.from_numpy(np.asarray(points[b, m], dtype=np.float64))
        MJ, Mr = Mb @ J, (Mb @ r.unsqueeze(-1)).squeeze(-1)
        A.append(torch.einsum("n,nci,ncj->ij", w, J, MJ) + torch.diag(prior))
        g.append(torch.einsum("n,nci,nc->i", w, J, Mr) + prior * P[b])
        c.append((w * (r * Mr).sum(1)).sum() + priors(P[b:b + 1], w_pose, w_beta)[0])
    return torch.stack(A), torch.stack(g), torch.stack(c)
