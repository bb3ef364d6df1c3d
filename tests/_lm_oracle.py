"""What the eight fit oracles (tests/_fit*_oracle.py) share, each piece once, and nothing of MANO: the Levenberg-Marquardt
loop with the kernels' rules, the frozen unknowns, the Gauss-Newton product, the dense assembly of a track's
block-tridiagonal equations with its smoothness cost, the batched similarity Procrustes and the start's scan along a
track.  Test-only: imports none of scat_amd's kernels.

The fp32 bits of these functions are the GPU gates (4 x the error of an oracle's fp32 run against its own fp64 run), so
where the oracles differ the difference is a parameter here, with its reason, and not made uniform."""
import contextlib
import math

import numpy as np
import torch

LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12


def group_vec(groups, dt):
    """(count, value) pairs -> the vector with every value repeated count times: a prior's or a smoothness's weights"""
    return torch.tensor([float(v) for n, v in groups for _ in range(n)], dtype=dt)


def mask_vec(free, n, dt):
    """bit i of the mask free -> 1 (free) or 0 (frozen) for unknown i of n"""
    return torch.tensor([(free >> i) & 1 for i in range(n)], dtype=dt)


def freeze(A, g, fr):
    """the frozen unknowns (0 in fr, a mask_vec) as unit rows of A with g = 0"""
    fr = fr.bool()
    keep = (fr[:, None] & fr[None, :]).to(A.dtype)
    return A * keep + torch.diag((~fr).to(A.dtype)), g * fr.to(A.dtype)


def gauss_newton(J, wr, r, prior, P):
    """rows J [B,R,U], their weights wr and residuals r [B,R] -> J^T W J + diag(prior) [B,U,U], J^T W r + prior * P [B,U]"""
    A = J.transpose(1, 2) @ (wr.unsqueeze(2) * J) + torch.diag(prior)
    return A, (J.transpose(1, 2) @ (wr * r).unsqueeze(2)).squeeze(2) + prior * P


def lm(P0, iters, lambda0, equations, cost, free_vec, finite_factor=False, no_grad=False):
    """-> P, cost [B], accepted [B], the costs [iters,B] and the iterates [iters,B,...] after every iteration, in P0's dtype.
    P0 is [B, ...]: one lambda and one accept / reject per leading index, the trailing dimensions flattened into its
    unknowns, so a hand [B,U] and a track [S,T,U] take the same path.  equations(P) -> the dense undamped A [B,N,N],
    g [B,N]; cost(P) -> [B], evaluated here without gradients for P and for the trial by one expression, so that a
    rejected step leaves the same bits; free_vec [U]: 1 / 0 per unknown.  The rules: Marquardt scaling, a failed Cholesky
    is a rejection, the trial is taken only if the cost drops, lambda / 10 or x 10 within LAMBDA_MIN..LAMBDA_MAX.
    finite_factor: a factor that is not finite has failed too (only the keypoint kernels check theirs).
    no_grad: all after the equations runs without gradients (the keypoint oracles' loops do)."""
    P, dt = P0.clone(), P0.dtype
    B, N = P.shape[0], P[0].numel()
    each = (B,) + (1,) * (P.dim() - 1)
    lam, acc = torch.full((B,), lambda0, dtype=dt), torch.zeros(B, dtype=torch.int32)
    fr = free_vec.expand(P.shape[1:]).reshape(N)
    hist, trace, c = [], [], None
    for _ in range(iters):
        A, g = equations(P)
        with torch.no_grad():
            c = cost(P)
        with torch.no_grad() if no_grad else contextlib.nullcontext():
            Ad = A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
            L, info = torch.linalg.cholesky_ex(Ad)
            ok = info == 0
            if finite_factor:
                ok = ok & torch.isfinite(L).all(2).all(1)
            L = torch.where(ok.reshape(B, 1, 1), L, torch.eye(N, dtype=dt).expand(B, N, N))
            delta = -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2) * fr
            Pt = P + delta.reshape(P.shape)
            with torch.no_grad():
                ct = cost(Pt)
            take = ok & torch.isfinite(Pt).reshape(B, N).all(1) & (ct < c)
            P = torch.where(take.reshape(each), Pt, P)
            c = torch.where(take, ct, c)
            acc += take.to(torch.int32)
            lam = torch.where(take, (lam * 0.1).clamp_min(LAMBDA_MIN), (lam * 10).clamp_max(LAMBDA_MAX))
            hist.append(c.clone())
            trace.append(P.clone())
    return P, c, acc, torch.stack(hist) if hist else None, torch.stack(trace) if trace else None


def chain(A, g, P, d):
    """the frames' A [S,T,U,U] and g [S,T,U] and the smoothness weights d [U] (zero where frozen) -> the dense
    H [S,TU,TU], g [S,TU] of a track: A_t + nb D on the diagonal (nb the number of t's neighbours), -D beside it,
    D ((p_t - p_t-1) + (p_t - p_t+1)) added to g_t, the earlier neighbour's term first"""
    S, T, U = g.shape
    P, g = P.detach(), g.clone()
    H = torch.zeros(S, T * U, T * U, dtype=P.dtype)
    for t in range(T):
        sl, lo = slice(t * U, (t + 1) * U), slice((t - 1) * U, t * U)
        H[:, sl, sl] = A[:, t] + torch.diag(((t > 0) + (t < T - 1)) * d)
        if t > 0:
            H[:, sl, lo] = H[:, lo, sl] = torch.diag(-d)
            g[:, t] += d * (P[:, t] - P[:, t - 1])
            g[:, t - 1] += d * (P[:, t - 1] - P[:, t])
    return H, g.reshape(S, T * U)


def smooth_cost(P, d):
    """[S]: sum_t sum_i d_i (p_t+1 - p_t)_i^2 of P [S,T,U], a frozen unknown's too; exactly 0 for T = 1"""
    e = P[:, 1:] - P[:, :-1]
    return (d * e * e).sum((1, 2))


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


def procrustes(X, Y, w):
    """the weighted similarity (SVD form) of X [B,J,3] onto Y with weights w [B,J], all fp64 -> the axis-angle of R
    [B,3], t [B,3] and log s [B] of y ~ s R x + t: an oracle's rots, trans and log_scale columns"""
    B = Y.shape[0]
    W = w.sum(1).reshape(B, 1)
    mx, my = (w.unsqueeze(2) * X).sum(1) / W, (w.unsqueeze(2) * Y).sum(1) / W
    Xc, Yc = X - mx.unsqueeze(1), Y - my.unsqueeze(1)
    K = torch.einsum("bj,bja,bjc->bac", w, Xc, Yc)           # sum_j w x y^T
    Uu, _, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(Vh.transpose(1, 2) @ Uu.transpose(1, 2)))
    R = Vh.transpose(1, 2) @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1)) @ Uu.transpose(1, 2)
    sc = torch.einsum("bca,bac->b", R, K) / (w * (Xc * Xc).sum(2)).sum(1)
    return rot_to_axis_angle(R), my - sc.reshape(B, 1) * (R @ mx.unsqueeze(2)).squeeze(2), torch.log(sc)


def scan_start(P, has, carry=slice(None), zero_empty=True, store=None):
    """the start's scan along every track of P [S,T,U] (fp64, changed in place and returned): a frame without weight
    (has [S,T] False) takes the carry columns of the frame before it, frame 0 those of the first frame with weight; then
    for t >= 1 the rotation r = P[s,t,:3] becomes r (1 - 2 pi / |r|) when that is closer to the frame before's.
    zero_empty: a track without weight anywhere becomes zeros (joint and mesh tracks) or stays (the keypoint track, whose
    camera start is not zero).  carry: every column, or the keypoint track's rots, trans, log_scale and camera.
    store: the dtype the unwrapped rotation is rounded to as it is stored (the keypoint track scans values rounded to it
    and compares the unrounded candidate); None stores it as it is."""
    S, T = has.shape
    for s in range(S):
        idx = [t for t in range(T) if bool(has[s, t])]
        if not idx:
            if zero_empty:
                P[s] = 0.0
            continue
        for t in range(T):
            if not bool(has[s, t]):
                P[s, t, carry] = P[s, t - 1 if t > 0 else idx[0], carry]
            elif t > 0:
                r, prev = P[s, t, :3].clone(), P[s, t - 1, :3]
                n = float(r.norm())
                if n > 0.0:
                    alt = r * (1.0 - 2.0 * math.pi / n)
                    if float(((alt - prev) ** 2).sum()) < float(((r - prev) ** 2).sum()):
                        P[s, t, :3] = alt if store is None else alt.to(store).double()
    return P
