"""fp64 torch statement of the MANO fit to a track of keypoints (include/scat_mano_fit_seq_kp.h) on top of _fit_kp_oracle
(the frame: 3-D and 2-D terms, the camera, the robust loss, the limits) and _fit_seq_oracle (the track: the smoothness, the
start's scan, accel): the cost, the dense (65 T)^2 normal equations, the start, and the Levenberg-Marquardt loop with the
header's rules, one lambda and one accept / reject per sequence.  The solve is a dense Cholesky, whose factor has exactly
the kernel's blocks (_fit_seq_oracle has why).  Test-only: imports none of scat_amd's kernels.

P is [S,T,65]; a Problem is _fit_kp_oracle's with T3 [S,T,21,3], w3 [S,T,21], T2 [S,T,21,2], w2 [S,T,21]; smooth is the seven
weights (rots, poses, betas, trans, scale, cam_scale, cam_trans).  Everything takes a dtype, as the two oracles do."""
import math

import numpy as np
import torch

import _fit_kp_oracle as KO
import _fit_seq_oracle as SO

U, U3 = KO.U, KO.U3
ALL = (1 << U3) - 1
KEYS = ("rots", "poses", "betas", "trans", "scale", "cam_scale", "cam_trans")


def sm(smooth):
    """the seven weights in the entry point's order from a dict; a missing key is 0"""
    return tuple(float(smooth.get(k, 0.0)) for k in KEYS)


def dvec(smooth, dt):
    """the 65 smoothness weights d_i from the seven of the groups"""
    s = [float(v) for v in smooth]
    return torch.tensor([s[0]] * 3 + [s[1]] * 45 + [s[2]] * 10 + [s[3]] * 3 + [s[4]] + [s[5]] + [s[6]] * 2, dtype=dt)


def free_vec(free, free_cam, dt):
    return torch.tensor(KO.free_bits(free, free_cam), dtype=dt)


def flat(pr):
    """the Problem of the S T frames as one batch"""
    f = lambda t: None if t is None else t.reshape(-1, *t.shape[2:])
    return pr._replace(T3=f(pr.T3), w3=f(pr.w3), T2=f(pr.T2), w2=f(pr.w2))


def cost(model, P, pr, smooth):
    """[S]: the frames' costs, then the smoothness terms (a frozen unknown's count too)"""
    S, T = P.shape[:2]
    c = KO.cost(model, P.reshape(S * T, U), flat(pr)).reshape(S, T).sum(1)
    if T > 1:
        e = P[:, 1:] - P[:, :-1]
        c = c + (dvec(smooth, P.dtype) * e * e).sum((1, 2))
    return c


def normal_equations(model, P, pr, smooth, free=ALL, free_cam=7):
    """-> H [S,65T,65T] (undamped, dense), g [S,65T], cost [S] at P: _fit_kp_oracle's A_t and g_t on the diagonal (IRLS
    weights at P, limits included), c_t D added to A_t's diagonal and D ((p_t - p_t-1) + (p_t - p_t+1)) to g_t, -D beside
    the diagonal; D has a zero where the unknown is frozen"""
    S, T = P.shape[:2]
    dt = P.dtype
    P = P.detach()
    A, g = KO.normal_equations(model, P.reshape(S * T, U), flat(pr), free, free_cam)
    A, g = A.reshape(S, T, U, U), g.reshape(S, T, U).clone()
    d = dvec(smooth, dt) * free_vec(free, free_cam, dt)
    H = torch.zeros(S, T * U, T * U, dtype=dt)
    for t in range(T):
        sl = slice(t * U, (t + 1) * U)
        nb = (t > 0) + (t < T - 1)
        H[:, sl, sl] = A[:, t] + torch.diag(nb * d)
        if t > 0:
            g[:, t] += d * (P[:, t] - P[:, t - 1])
            H[:, sl, (t - 1) * U:t * U] = torch.diag(-d)
            H[:, (t - 1) * U:t * U, sl] = torch.diag(-d)
        if t < T - 1:
            g[:, t] += d * (P[:, t] - P[:, t + 1])
    with torch.no_grad():
        c = cost(model, P, pr, smooth)
    return H, g.reshape(S, T * U), c


def lm(model, pr, P0, iters, smooth, lambda0=1e-3, free=ALL, free_cam=7, history=False):
    """-> P [S,T,65], cost [S], accepted [S] (and the per-iteration costs [iters,S] and iterates [iters,S,T,65]) in P0's
    dtype"""
    dt = P0.dtype
    P = P0.clone()
    S, T = P.shape[:2]
    N = T * U
    lam = torch.full((S,), lambda0, dtype=dt)
    acc = torch.zeros(S, dtype=torch.int32)
    fr = free_vec(free, free_cam, dt).repeat(T)
    hist, trace, c = [], [], None
    for _ in range(iters):
        H, g, c = normal_equations(model, P, pr, smooth, free, free_cam)
        with torch.no_grad():
            Hd = H + lam.reshape(S, 1, 1) * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
            L, info = torch.linalg.cholesky_ex(Hd)
            ok = (info == 0) & torch.isfinite(L).all(2).all(1)
            L = torch.where(ok.reshape(S, 1, 1), L, torch.eye(N, dtype=dt).expand(S, N, N))
            delta = -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2) * fr
            Pt = P + delta.reshape(S, T, U)
            ct = cost(model, Pt, pr, smooth)
            take = ok & torch.isfinite(Pt).reshape(S, -1).all(1) & (ct < c)
            P = torch.where(take.reshape(S, 1, 1), Pt, P)
            c = torch.where(take, ct, c)
            acc += take.to(torch.int32)
            lam = torch.where(take, (lam * 0.1).clamp_min(KO.LAMBDA_MIN), (lam * 10).clamp_max(KO.LAMBDA_MAX))
            hist.append(c.clone())
            trace.append(P.clone())
    return (P, c, acc, torch.stack(hist), torch.stack(trace)) if history else (P, c, acc)


def has_weight(pr, S, T):
    """[S,T] bool: sum w3 + sum w2 > 0, an absent term counting nothing and absent weights of a present term as ones"""
    _, w3, _, w2 = KO._terms(flat(pr), S * T, torch.float64)
    return ((w3.sum(1) + w2.sum(1)) > 0).reshape(S, T)


def start(model, pr, S, T, dtype=torch.float64):
    """init = 1 -> [S,T,65] in dtype: _fit_kp_oracle.start frame by frame, then _fit_seq_oracle.start's scan on the rounded
    values, in fp64 as in the kernel: a frame of total weight zero takes the rots, trans, log_scale and camera of the frame
    before it, frame 0 those of the first frame with weight; then for t >= 1 rots_t becomes r (1 - 2 pi / |r|) when that
    is closer to rots_t-1.  The 2-D-only mirror candidate of a frame is not revisited."""
    P = KO.start(model, flat(pr), S * T, dtype).double().reshape(S, T, U)
    has = has_weight(pr, S, T)
    keep = list(range(3)) + list(range(58, U))
    for s in range(S):
        idx = [t for t in range(T) if bool(has[s, t])]
        if not idx:
            continue
        for t in range(T):
            if not bool(has[s, t]):
                P[s, t, keep] = P[s, t - 1 if t > 0 else idx[0], keep]
            elif t > 0:
                r = P[s, t, :3].clone()
                n = float(r.norm())
                if n > 0.0:
                    alt = (r * (1.0 - 2.0 * math.pi / n)).to(dtype).double()
                    if float(((r * (1.0 - 2.0 * math.pi / n) - P[s, t - 1, :3]) ** 2).sum()) < float(((r - P[s, t - 1, :3]) ** 2).sum()):
                        P[s, t, :3] = alt
    return P.to(dtype)


def frame_joints(model, P, joint_map):
    """the model joints of every frame [S,T,21,3], in fp64"""
    return SO.frame_joints(model, P[..., :U3], joint_map)


def accel(model, P, joint_map, truth):
    """_fit_seq_oracle.accel of the first 62 unknowns: the camera plays no part in the 3-D joints"""
    return SO.accel(model, P[..., :U3], joint_map, truth)


def rms2(model, P, T2, joint_map, half, sel=None):
    """[S,T]: _fit_kp_oracle.rms2 frame by frame, pixels"""
    S, T = P.shape[:2]
    f = lambda t: None if t is None else t.reshape(S * T, *t.shape[2:])
    return KO.rms2(model, P.reshape(S * T, U), f(T2), joint_map, half, f(sel)).reshape(S, T)


def rel(a, b):
    return KO.rel(np.asarray(a), np.asarray(b))
