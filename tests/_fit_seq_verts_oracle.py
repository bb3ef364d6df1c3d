"""fp64 torch statement of the MANO fit to a track of meshes and to a track of point clouds
(include/scat_mano_fit_seq_verts.h): the cost, the dense (62 T)^2 normal equations with the per-frame blocks of
_fit_verts_oracle (Euclidean) or _fit_plane_oracle (the plane metric) and the smoothness where _lm_oracle.chain places it
for every track oracle, _lm_oracle.lm with one lambda and one accept / reject per sequence and a dense Cholesky, the start
(the Procrustes over the vertices per frame, then _fit_seq_oracle.track_start's scan), and the ICP loop over a track with
its bridging rule.  Test-only: imports none of scat_amd's kernels.

P is [S,T,62], targets [S,T,V,3], w [S,T,V], n (normals) [S,T,V,3] or None; smooth is the five weights."""
import numpy as np
import torch

import _fit_oracle as FO
import _fit_plane_oracle as LO
import _fit_points_oracle as PO
import _fit_seq_oracle as SO
import _fit_verts_oracle as VO
import _lm_oracle as L

U = FO.U
ALL = (1 << U) - 1


def _flat(P, targets, w, n):
    S, T = P.shape[:2]
    V = targets.shape[2]
    return (P.reshape(S * T, U), targets.reshape(S * T, V, 3), w.reshape(S * T, V), None if n is None else n.reshape(S * T, V, 3))


def cost(model, P, targets, w, n, tau, w_pose, w_beta, smooth):
    """[S]: the frames' costs (data term and priors), then the smoothness terms (a frozen unknown's count too)"""
    S, T = P.shape[:2]
    Pf, X, wf, nf = _flat(P, targets, w, n)
    c = VO.cost(model, Pf, X, wf, w_pose, w_beta) if n is None else LO.cost(model, Pf, X, wf, nf, tau, w_pose, w_beta)
    return c.reshape(S, T).sum(1) + L.smooth_cost(P, SO.dvec(smooth, P.dtype))


def equations(model, P, targets, w, n, tau, w_pose, w_beta, smooth, free=ALL):
    """-> H [S,62T,62T] (undamped, dense), g [S,62T]: _lm_oracle.chain of the frames' own A_t and g_t with D =
    _fit_seq_oracle.dvec, which has a zero where the unknown is frozen"""
    S, T = P.shape[:2]
    Pf, X, wf, nf = _flat(P, targets, w, n)
    if n is None:
        A, g, _ = VO.normal_equations(model, Pf, X, wf, w_pose, w_beta, free)
    else:
        A, g, _ = LO.normal_equations(model, Pf, X, wf, nf, tau, w_pose, w_beta, free)
    return L.chain(A.reshape(S, T, U, U), g.reshape(S, T, U), P, SO.dvec(smooth, P.dtype) * SO.free_vec(free, P.dtype))


def normal_equations(model, P, targets, w, n, tau, w_pose, w_beta, smooth, free=ALL):
    """-> H, g of equations above and the cost [S] at P"""
    with torch.no_grad():
        c = cost(model, P, targets, w, n, tau, w_pose, w_beta, smooth)
    return equations(model, P, targets, w, n, tau, w_pose, w_beta, smooth, free) + (c,)


def lm(model, targets, w, P0, iters, smooth, n=None, tau=1.0, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=ALL, history=False):
    """-> P [S,T,62], cost [S], accepted [S] (and the per-iteration costs [iters,S]) in P0's dtype: _lm_oracle.lm"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    n = None if n is None else n.to(dt)
    return L.lm(P0, iters, lambda0, lambda P: equations(model, P, targets, w, n, tau, w_pose, w_beta, smooth, free),
                lambda P: cost(model, P, targets, w, n, tau, w_pose, w_beta, smooth), SO.free_vec(free, dt))[:4 if history else 3]


def procrustes(model, targets, w, dt=torch.float64):
    """_fit_verts_oracle.procrustes_start's formulas [B,62] fp64, on zero-pose vertices computed in dt (the kernel's are
    fp32; the Procrustes itself is fp64 whatever dt, as in the kernel); tests/test_fit_seq_verts.py holds the fp64 form to
    _fit_verts_oracle.procrustes_start"""
    X = VO.verts(model, torch.zeros(1, U, dtype=dt)).double().expand(targets.shape[0], -1, 3)
    return FO.similarity_start(X, targets.double(), w.double())


def start(model, targets, w, dt=torch.float64):
    """init = 1 -> [S,T,62] in dt: _fit_seq_oracle.track_start (the Procrustes start frame by frame, then the scan for the
    frames without weight and the rotations' unwrapping) on the zero-pose vertices computed in dt"""
    return SO.track_start(VO.verts(model, torch.zeros(1, U, dtype=dt)), targets, w).to(dt)


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
