"""fp64 torch statement of the MANO fit to a track of frames (include/scat_mano_fit_seq.h) on top of _fit_oracle: the
cost, the dense (62 T)^2 normal equations, the start, and the Levenberg-Marquardt loop with the kernel's rules, one
lambda and one accept / reject per sequence.  The solve is a dense Cholesky: the dense factor of a block-tridiagonal
matrix has exactly the kernel's blocks (L_t on the diagonal, M_t below it, zeros elsewhere), so the fp32 run of this
oracle is the kernel's algorithm up to the order of the sums.  Test-only: imports none of scat_amd's kernels.

P is [S,T,62], targets [S,T,21,3], w [S,T,21]; smooth is the five weights (rots, poses, betas, trans, scale)."""
import math

import torch

import _fit_oracle as FO

U = FO.U
ALL = (1 << U) - 1


def dvec(smooth, dt):
    """the 62 smoothness weights d_i from the five of the groups"""
    s = [float(v) for v in smooth]
    return torch.tensor([s[0]] * 3 + [s[1]] * 45 + [s[2]] * 10 + [s[3]] * 3 + [s[4]], dtype=dt)


def free_vec(free, dt):
    return torch.tensor([(free >> i) & 1 for i in range(U)], dtype=dt)


def cost(model, P, targets, w, joint_map, w_pose, w_beta, smooth):
    """[S]: the frames' costs, then the smoothness terms (a frozen unknown's count too)"""
    S, T = P.shape[:2]
    c = FO.cost(model, P.reshape(S * T, U), targets.reshape(S * T, 21, 3), w.reshape(S * T, 21), joint_map, w_pose, w_beta)
    c = c.reshape(S, T).sum(1)
    if T > 1:
        e = P[:, 1:] - P[:, :-1]
        c = c + (dvec(smooth, P.dtype) * e * e).sum((1, 2))
    return c


def normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, smooth, free=ALL):
    """-> H [S,62T,62T] (undamped, dense), g [S,62T], cost [S] at P: _fit_oracle's A_t and g_t on the diagonal, c_t D
    added to A_t's diagonal and D ((p_t - p_t-1) + (p_t - p_t+1)) to g_t, -D beside the diagonal; D has a zero where the
    unknown is frozen"""
    S, T = P.shape[:2]
    dt = P.dtype
    A, g, _ = FO.normal_equations(model, P.reshape(S * T, U), targets.reshape(S * T, 21, 3), w.reshape(S * T, 21), joint_map,
                                  w_pose, w_beta, free)
    A, g = A.reshape(S, T, U, U), g.reshape(S, T, U).clone()
    d = dvec(smooth, dt) * free_vec(free, dt)
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
        c = cost(model, P, targets, w, joint_map, w_pose, w_beta, smooth)
    return H, g.reshape(S, T * U), c


def lm(model, targets, w, joint_map, P0, iters, smooth, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=ALL, history=False):
    """-> P [S,T,62], cost [S], accepted [S] (and the per-iteration costs [iters,S]) in P0's dtype"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    P = P0.clone()
    S, T = P.shape[:2]
    N = T * U
    lam = torch.full((S,), lambda0, dtype=dt)
    acc = torch.zeros(S, dtype=torch.int32)
    fr = free_vec(free, dt).repeat(T)
    hist, c = [], None
    for _ in range(iters):
        H, g, c = normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, smooth, free)
        Hd = H + lam.reshape(S, 1, 1) * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(Hd)
        ok = info == 0
        L = torch.where(ok.reshape(S, 1, 1), L, torch.eye(N, dtype=dt).expand(S, N, N))
        delta = -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2) * fr
        Pt = P + delta.reshape(S, T, U)
        with torch.no_grad():
            ct = cost(model, Pt, targets, w, joint_map, w_pose, w_beta, smooth)
        take = ok & torch.isfinite(Pt).reshape(S, -1).all(1) & (ct < c)
        P = torch.where(take.reshape(S, 1, 1), Pt, P)
        c = torch.where(take, ct, c)
        acc += take.to(torch.int32)
        lam = torch.where(take, (lam * 0.1).clamp_min(FO.LAMBDA_MIN), (lam * 10).clamp_max(FO.LAMBDA_MAX))
        hist.append(c.clone())
    return (P, c, acc, torch.stack(hist)) if history else (P, c, acc)


def start(model, targets, w, joint_map, dt=torch.float64):
    """init = 1: _fit_oracle's Procrustes start frame by frame (the same formulas, on zero-pose joints computed in dt:
    the kernel's are fp32; the Procrustes itself is fp64 whatever dt, as in the kernel); a frame of total weight zero
    takes the start of the frame before it, frame 0 that of the first frame with weight, zeros if there is none; then
    for t >= 1 rots_t becomes r (1 - 2 pi / |r|) when that is closer to rots_t-1.  -> [S,T,62] in dt"""
    S, T = targets.shape[:2]
    B = S * T
    w = w.double()
    has = w.sum(2) > 0
    wf = torch.where(has.unsqueeze(2), w, torch.ones_like(w)).reshape(B, 21)
    Y = targets.double().reshape(B, 21, 3)
    with torch.no_grad():
        X = FO.joints(model, torch.zeros(1, U, dtype=dt))[:, list(joint_map)].double().expand(B, 21, 3)
    W = wf.sum(1).reshape(B, 1)
    mx, my = (wf.unsqueeze(2) * X).sum(1) / W, (wf.unsqueeze(2) * Y).sum(1) / W
    Xc, Yc = X - mx.unsqueeze(1), Y - my.unsqueeze(1)
    K = torch.einsum("bj,bja,bjc->bac", wf, Xc, Yc)
    Uu, _, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(Vh.transpose(1, 2) @ Uu.transpose(1, 2)))
    R = Vh.transpose(1, 2) @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1)) @ Uu.transpose(1, 2)
    sc = torch.einsum("bca,bac->b", R, K) / (wf * (Xc * Xc).sum(2)).sum(1)
    P = torch.zeros(B, U, dtype=torch.float64)
    P[:, 0:3] = FO.rot_to_axis_angle(R)
    P[:, 58:61] = my - sc.reshape(B, 1) * (R @ mx.unsqueeze(2)).squeeze(2)
    P[:, 61] = torch.log(sc)
    P = P.reshape(S, T, U)
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
                n = float(r.norm())
                if n > 0.0:
                    alt = r * (1.0 - 2.0 * math.pi / n)
                    if float(((alt - P[s, t - 1, :3]) ** 2).sum()) < float(((r - P[s, t - 1, :3]) ** 2).sum()):
                        P[s, t, :3] = alt
    return P.to(dt)


def frame_joints(model, P, joint_map):
    """the model joints of every frame [S,T,21,3], in fp64"""
    S, T = P.shape[:2]
    with torch.no_grad():
        return FO.model_joints(model, P.double().reshape(S * T, U), joint_map).reshape(S, T, 21, 3)


def accel(model, P, joint_map, truth):
    """scat_amd.metrics.accel_error of the fitted joints against the true ones, per sequence: the mean over the frame
    triples, in the joints' unit"""
    from scat_amd.metrics import accel_error

    X = frame_joints(model, P, joint_map)
    return torch.stack([accel_error(truth[s].double(), X[s]).mean() for s in range(P.shape[0])])
