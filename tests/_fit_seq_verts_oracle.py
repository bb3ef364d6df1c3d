"""fp64 torch statement of the MANO fit to a track of meshes and to a track of point clouds
(include/scat_mano_fit_seq_verts.h): the cost, the dense (62 T)^2 normal equations with the per-frame blocks of
_fit_verts_oracle (Euclidean) or _fit_plane_oracle (the plane metric) and the smoothness exactly where
_fit_seq_oracle.normal_equations places it, Levenberg-Marquardt with one lambda and one accept / reject per sequence and a
dense Cholesky as _fit_seq_oracle.lm, the start (_fit_verts_oracle.procrustes_start per frame, then _fit_seq_oracle.start's
scan), and the ICP loop over a track with its bridging rule.  Test-only: imports none of scat_amd's kernels.

P is [S,T,62], targets [S,T,V,3], w [S,T,V], n (normals) [S,T,V,3] or None; smooth is the five weights."""
import math

import numpy as np
import torch

import _fit_oracle as FO
import _fit_plane_oracle as LO
import _fit_points_oracle as PO
import _fit_seq_oracle as SO
import _fit_verts_oracle as VO

U = FO.U
ALL = (1 << U) - 1


def _flat(P, targets, w, n):
    S, T = P.shape[:2]
    V = targets.shape[2]
    return (P.reshape(S * T, U), targets.reshape(S * T, V, 3), w.reshape(S * T, V), None if n is None else n.reshape(S * T, V, 3))


def frame_costs(model, P, targets, w, n, tau, w_pose, w_beta):
    """[S,T]: every frame's data term and priors"""
    S, T = P.shape[:2]
    Pf, X, wf, nf = _flat(P, targets, w, n)
    c = VO.cost(model, Pf, X, wf, w_pose, w_beta) if n is None else LO.cost(model, Pf, X, wf, nf, tau, w_pose, w_beta)
    return c.reshape(S, T)


def cost(model, P, targets, w, n, tau, w_pose, w_beta, smooth):
    """[S]: the frames' costs, then the smoothness terms (a frozen unknown's count too)"""
    c = frame_costs(model, P, targets, w, n, tau, w_pose, w_beta).sum(1)
    if P.shape[1] > 1:
        e = P[:, 1:] - P[:, :-1]
        c = c + (SO.dvec(smooth, P.dtype) * e * e).sum((1, 2))
    return c


def frame_equations(model, P, targets, w, n, tau, w_pose, w_beta, free=ALL):
    """-> A [S,T,62,62] (undamped), g [S,T,62]: the frames' own normal equations"""
    S, T = P.shape[:2]
    Pf, X, wf, nf = _flat(P, targets, w, n)
    if n is None:
        A, g, _ = VO.normal_equations(model, Pf, X, wf, w_pose, w_beta, free)
    else:
        A, g, _ = LO.normal_equations(model, Pf, X, wf, nf, tau, w_pose, w_beta, free)
    return A.reshape(S, T, U, U), g.reshape(S, T, U)


def normal_equations(model, P, targets, w, n, tau, w_pose, w_beta, smooth, free=ALL):
    """-> H [S,62T,62T] (undamped, dense), g [S,62T], cost [S] at P: the frames' A_t and g_t on the diagonal, c_t D added to
    A_t's diagonal and D ((p_t - p_t-1) + (p_t - p_t+1)) to g_t, -D beside the diagonal; D has a zero where the unknown is
    frozen"""
    S, T = P.shape[:2]
    dt = P.dtype
    A, g = frame_equations(model, P, targets, w, n, tau, w_pose, w_beta, free)
    g = g.clone()
    d = SO.dvec(smooth, dt) * SO.free_vec(free, dt)
    H = torch.zeros(S, T * U, T * U, dtype=dt)
    for t in range(T):
        sl = slice(t * U, (t + 1) * U)
        nb = (t > 0) + (t < T - 1)
        H[:, sl, sl] = A[:, t] + torch.diag(nb * d)
        if t > 0:
            g[:, t] += d * (P[:, t] - P[:, t - 1]).detach()
            H[:, sl, (t - 1) * U:t * U] = torch.diag(-d)
            H[:, (t - 1) * U:t * U, sl] = torch.diag(-d)
        if t < T - 1:
            g[:, t] += d * (P[:, t] - P[:, t + 1]).detach()
    with torch.no_grad():
        c = cost(model, P, targets, w, n, tau, w_pose, w_beta, smooth)
    return H, g.reshape(S, T * U), c


def lm(model, targets, w, P0, iters, smooth, n=None, tau=1.0, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=ALL, history=False):
    """-> P [S,T,62], cost [S], accepted [S] (and the per-iteration costs [iters,S]) in P0's dtype: _fit_seq_oracle.lm's
    loop on the equations above"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    n = None if n is None else n.to(dt)
    P = P0.clone()
    S, T = P.shape[:2]
    N = T * U
    lam = torch.full((S,), lambda0, dtype=dt)
    acc = torch.zeros(S, dtype=torch.int32)
    fr = SO.free_vec(free, dt).repeat(T)
    hist, c = [], None
    for _ in range(iters):
        H, g, c = normal_equations(model, P, targets, w, n, tau, w_pose, w_beta, smooth, free)
        Hd = H + lam.reshape(S, 1, 1) * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(Hd)
        ok = info == 0
        L = torch.where(ok.reshape(S, 1, 1), L, torch.eye(N, dtype=dt).expand(S, N, N))
        delta = -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2) * fr
        Pt = P + delta.reshape(S, T, U)
        with torch.no_grad():
            ct = cost(model, Pt, targets, w, n, tau, w_pose, w_beta, smooth)
        take = ok & torch.isfinite(Pt).reshape(S, -1).all(1) & (ct < c)
        P = torch.where(take.reshape(S, 1, 1), Pt, P)
        c = torch.where(take, ct, c)
        acc += take.to(torch.int32)
        lam = torch.where(take, (lam * 0.1).clamp_min(FO.LAMBDA_MIN), (lam * 10).clamp_max(FO.LAMBDA_MAX))
        hist.append(c.clone())
    return (P, c, acc, torch.stack(hist)) if history else (P, c, acc)


def procrustes(model, targets, w, dt=torch.float64):
    """_fit_verts_oracle.procrustes_start's formulas [B,62] fp64, on zero-pose vertices computed in dt (the kernel's are
    fp32; the Procrustes itself is fp64 whatever dt, as in the kernel); tests/test_fit_seq_verts.py holds the fp64 form to
    _fit_verts_oracle.procrustes_start"""
    Y, w = targets.double(), w.double()
    B = Y.shape[0]
    with torch.no_grad():
        X = VO.verts(model, torch.zeros(1, U, dtype=dt)).double().expand(B, -1, 3)
    W = w.sum(1).reshape(B, 1)
    mx, my = (w.unsqueeze(2) * X).sum(1) / W, (w.unsqueeze(2) * Y).sum(1) / W
    Xc, Yc = X - mx.unsqueeze(1), Y - my.unsqueeze(1)
    K = torch.einsum("bj,bja,bjc->bac", w, Xc, Yc)
    Uu, _, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(Vh.transpose(1, 2) @ Uu.transpose(1, 2)))
    R = Vh.transpose(1, 2) @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1)) @ Uu.transpose(1, 2)
    sc = torch.einsum("bca,bac->b", R, K) / (w * (Xc * Xc).sum(2)).sum(1)
    P = torch.zeros(B, U, dtype=torch.float64)
    P[:, 0:3] = FO.rot_to_axis_angle(R)
    P[:, 58:61] = my - sc.reshape(B, 1) * (R @ mx.unsqueeze(2)).squeeze(2)
    P[:, 61] = torch.log(sc)
    return P


def start(model, targets, w, dt=torch.float64):
    """init = 1: the Procrustes start over the vertices frame by frame; a frame of total weight zero takes the start of the
    frame before it, frame 0 that of the first frame with weight, zeros if there is none; then for t >= 1 rots_t becomes
    r (1 - 2 pi / |r|) when that is closer to rots_t-1: _fit_seq_oracle.start's scan.  -> [S,T,62] in dt"""
    S, T, V = targets.shape[:3]
    w = w.double()
    has = w.sum(2) > 0
    wf = torch.where(has.unsqueeze(2), w, torch.ones_like(w)).reshape(S * T, V)
    P = procrustes(model, targets.reshape(S * T, V, 3), wf, dt).reshape(S, T, U)
    for s in range(S):
        idx = [t for t in range(T) if bool(has[s, t])]
        if not idx:
            P[s] = 0.0
            continue
        for t in range(T):
            if not bool(has[s, t]):
                P[s, t] = P[s, t - 1] if t > 0 else P[s, idx[0]]
            elif t > 0:
                r = P[s, t, :3]
                nr = float(r.norm())
                if nr > 0.0:
                    alt = r * (1.0 - 2.0 * math.pi / nr)
                    if float(((alt - P[s, t - 1, :3]) ** 2).sum()) < float(((r - P[s, t - 1, :3]) ** 2).sum()):
                        P[s, t, :3] = alt
    return P.to(dt)


def meshes(model, P):
    """the model's vertices of every frame [S,T,V,3], in fp64"""
    S, T = P.shape[:2]
    with torch.no_grad():
        return VO.model_verts(model, P.double().reshape(S * T, U)).reshape(S, T, -1, 3)


def accel(model, P, truth):
    """the mean over frame triples and vertices of |x_t-1 - 2 x_t + x_t+1 - (the same of the truth)|, per sequence: the
    acceleration error of the fitted meshes against the true ones [S,T,V,3], in the meshes' unit"""
    X = meshes(model, P) - truth.double()
    a = X[:, :-2] - 2.0 * X[:, 1:-1] + X[:, 2:]
    return a.norm(dim=3).mean((1, 2))


def rms(model, P, truth):
    """[S,T]: the root of the mean squared vertex distance from the true meshes"""
    d = meshes(model, P) - truth.double()
    return (d * d).sum(3).mean(2).sqrt()


def icp(model, points, weights, P0, topo, rounds, iters, smooth, tau=1.0, max_dist=np.inf, lambda0=1e-3, w_pose=1e-6,
        w_beta=1e-6, free=ALL, dt=torch.float64):
    """-> P [S,T,62] in dt (fp32 only measures what rounding does to the solves; the assignment stays fp64), accepted [S], the data cost of the last assignment [S,T] (the metric one with topo) and that
    assignment.  A round: _fit_points_oracle.assign over the S T frames at P's model points, with topo = (faces, vf_off,
    vf_idx) their normals, then lm above on (vtarget, vw, normals).  A frame where nothing matched (a NaN vw row with
    stats[.][0] == 0) is bridged: its weights are zero.  A frame the assignment found unusable (stats[.][0] != 0) refuses
    its sequence, which keeps its P."""
    points = np.asarray(points)
    S, T, N = points.shape[:3]
    B = S * T
    pts = points.reshape(B, N, 3)
    wts = None if weights is None else np.asarray(weights).reshape(B, N)
    P = P0.to(dt).clone()
    acc = torch.zeros(S, dtype=torch.int32)
    for r in range(rounds + 1):
        with torch.no_grad():
            x = VO.model_verts(model, P.reshape(B, U)).double().numpy()
        a = PO.assign(x, pts, wts, max_dist)
        n = None if topo is None else LO.normals(x, *topo)
        bad = a["stats"][:, 0] != 0
        if r == rounds:
            dc = a["stats"][:, 3] if topo is None else LO.assign_cost(x, pts, wts, a["idx"], a["matched"], n, tau)
            return P, acc, np.where(bad, np.inf, dc).reshape(S, T), a
        ok = torch.from_numpy(~bad.reshape(S, T).any(1))
        vw = torch.from_numpy(np.where(np.isfinite(a["vw"]), a["vw"], 0.0)).reshape(S, T, -1)
        vt = torch.from_numpy(a["vtarget"]).reshape(S, T, -1, 3)
        nn = None if n is None else torch.from_numpy(n).reshape(S, T, -1, 3)
        Pn, _, an = lm(model, vt, vw, P, iters, smooth, nn, tau, lambda0, w_pose, w_beta, free)
        P = torch.where(ok.reshape(S, 1, 1), Pn, P)
        acc += torch.where(ok, an, torch.zeros_like(an))
