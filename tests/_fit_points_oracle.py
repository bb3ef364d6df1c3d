"""fp64 statement of the MANO fit to a point cloud of include/scat_mano_fit_points.h: the nearest-vertex assignment with
its per-vertex reduction (numpy), the ICP loop around _fit_verts_oracle.lm, and the per-point normal equations that the
per-vertex form replaces.  Test-only: imports none of scat_amd's kernels.

assign follows the header rule for rule: d2 = (dx dx + dy dy) + dz dz in IEEE fp64 on the numbers it is given (numpy
rounds every product and sum once), the lowest index on a tie (argmin returns the first minimum), matched iff w > 0 and
d2 <= max_dist^2 with max_dist squared in fp64, and W_v, S_v summed over the matched points with n ascending
(np.add.at is unbuffered and walks its indices in order)."""
import math

import numpy as np
import torch

import _fit_oracle as FO
import _fit_verts_oracle as VO

U = VO.U
CHUNK = 512      # points per block of the distance table


def d2_table(q, x):
    """q [n,3], x [V,3] fp64 -> [n,V], the header's expression"""
    dx, dy, dz = (q[:, None, c] - x[None, :, c] for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def assign(verts, points, weights=None, max_dist=np.inf, margins=False):
    """verts [B,V,3], points [B,N,3], weights [B,N] or None: arrays of any float dtype, taken to fp64 as they are ->
    dict(idx [B,N] int32, dist [B,N] fp64, vw [B,V] fp64, vtarget [B,V,3] fp64, stats [B,4], matched [B,N] bool) and with
    margins also margin [B,N]: (second-best d2 - best d2) / best-or-second d2, inf for V = 1"""
    verts, points = np.asarray(verts, dtype=np.float64), np.asarray(points, dtype=np.float64)
    B, V, N = verts.shape[0], verts.shape[1], points.shape[1]
    w = np.ones((B, N)) if weights is None else np.asarray(weights, dtype=np.float64)
    md2 = np.float64(max_dist) * np.float64(max_dist)
    out = dict(idx=np.full((B, N), -1, np.int32), dist=np.zeros((B, N)), vw=np.full((B, V), np.nan), vtarget=np.zeros((B, V, 3)),
               stats=np.zeros((B, 4)), matched=np.zeros((B, N), bool), margin=np.full((B, N), np.inf))
    for b in range(B):
        if not (np.isfinite(points[b]).all() and np.isfinite(w[b]).all() and (w[b] >= 0).all() and np.isfinite(verts[b]).all()):
            out["stats"][b] = (2.0, 0.0, 0.0, np.inf)
            continue
        best = np.zeros(N)
        for n0 in range(0, N, CHUNK):
            t = d2_table(points[b, n0:n0 + CHUNK], verts[b])
            i = t.argmin(1)
            out["idx"][b, n0:n0 + CHUNK] = i
            best[n0:n0 + CHUNK] = t[np.arange(len(i)), i]
            if margins and V > 1:
                t[np.arange(len(i)), i] = np.inf
                second = t.min(1)
                out["margin"][b, n0:n0 + CHUNK] = (second - best[n0:n0 + CHUNK]) / np.maximum(second, 1e-300)
        live = w[b] > 0
        out["idx"][b, ~live] = -1
        out["dist"][b] = np.where(live, np.sqrt(best), 0.0)
        m = live & (best <= md2)
        out["matched"][b] = m
        n = np.nonzero(m)[0]                      # ascending
        c = out["idx"][b, n]
        W, S = np.zeros(V), np.zeros((V, 3))
        np.add.at(W, c, w[b, n])
        np.add.at(S, c, w[b, n, None] * points[b, n])
        with np.errstate(invalid="ignore", divide="ignore"):
            out["vtarget"][b] = np.where(W[:, None] > 0, S / W[:, None], 0.0)
        mw = W.sum()
        out["vw"][b] = W if mw > 0 else np.nan
        out["stats"][b] = (0.0, mw, float(len(n)), float((w[b, n] * best[n]).sum()))
    if not margins:
        del out["margin"]
    return out


def brute_assign(verts, points, weights, max_dist):
    """the same by a double loop over python floats: what assign is held to at a small size"""
    verts, points = np.asarray(verts, dtype=np.float64), np.asarray(points, dtype=np.float64)
    B, V, N = verts.shape[0], verts.shape[1], points.shape[1]
    idx, dist = np.full((B, N), -1, np.int32), np.zeros((B, N))
    vw, vt, stats = np.zeros((B, V)), np.zeros((B, V, 3)), np.zeros((B, 4))
    md2 = float(max_dist) * float(max_dist)
    for b in range(B):
        W, S = [0.0] * V, [[0.0, 0.0, 0.0] for _ in range(V)]
        for n in range(N):
            w = 1.0 if weights is None else float(weights[b, n])
            if not w > 0:
                continue
            bd, bi = float("inf"), 0
            for v in range(V):
                dx, dy, dz = (float(points[b, n, c]) - float(verts[b, v, c]) for c in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 < bd:
                    bd, bi = d2, v
            idx[b, n], dist[b, n] = bi, math.sqrt(bd)
            if bd <= md2:
                W[bi] += w
                for c in range(3):
                    S[bi][c] += w * float(points[b, n, c])
                stats[b, 1] += w
                stats[b, 2] += 1
                stats[b, 3] += w * bd
        for v in range(V):
            vw[b, v] = W[v]
            vt[b, v] = [s / W[v] for s in S[v]] if W[v] > 0 else 0.0
        if not stats[b, 1] > 0:
            vw[b] = np.nan
    return idx, dist, vw, vt, stats


def icp(model, points, weights, P0, rounds, iters, max_dist=np.inf, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << U) - 1,
        history=False):
    """-> P [B,62] fp64, accepted [B], the data cost of every assignment [rounds + 1, B] (the last one at the returned P)
    and that last assignment; with history also the P of every assignment [rounds + 1, B, 62].  A round: assign at P's model points (fp64), then _fit_verts_oracle.lm on (vtarget, vw); a
    hand with a NaN vw row keeps its P."""
    return icp_loop(model, points, weights, P0, rounds, max_dist, history,
                    lambda vt, vw, n, P: VO.lm(model, vt, vw, P, iters, lambda0, w_pose, w_beta, free))


def icp_loop(model, points, weights, P0, rounds, max_dist, history, solve, normals=None, assign_cost=None):
    """the per-hand ICP of icp above and of _fit_plane_oracle.icp, which imports this module.  solve(vtarget, vw, n, P) ->
    P, cost, accepted: the fit of a round.  normals(x) -> n, the model points' normals for the solve and the cost, and
    assign_cost(x, a, n) -> [B], the data cost of an assignment in place of its stats[:, 3] (the plane fit's); an
    unusable hand's is +inf in either."""
    P = P0.double().clone()
    acc, costs, Ps = torch.zeros(P.shape[0], dtype=torch.int32), [], []
    for r in range(rounds + 1):
        Ps.append(P.clone())
        with torch.no_grad():
            x = VO.model_verts(model, P).numpy()
        a = assign(x, points, weights, max_dist)
        n = None if normals is None else normals(x)
        costs.append(np.where(a["stats"][:, 0] != 0, np.inf, a["stats"][:, 3] if assign_cost is None else assign_cost(x, a, n)))
        if r == rounds:
            break
        ok = torch.from_numpy(np.isfinite(a["vw"]).all(1))
        vw = torch.from_numpy(np.where(np.isfinite(a["vw"]), a["vw"], 0.0))
        Pn, _, an = solve(torch.from_numpy(a["vtarget"]), vw, n, P)
        P = torch.where(ok.unsqueeze(1), Pn, P)
        acc += torch.where(ok, an, torch.zeros_like(an))
    return (P, acc, np.stack(costs), a) + ((torch.stack(Ps),) if history else ())


def point_normal_equations(model, P, points, weights, idx, matched, w_pose, w_beta):
    """the Gauss-Newton system of sum_n w_n |model_c(n) - q_n|^2 + priors with one row triple per matched point (rows
    J_c(n), residual model_c(n) - q_n) -> A [B,62,62], g [B,62], cost [B]: what the per-vertex form must reproduce"""
    Jf, mv = VO.rows(model, P, 0.0)
    prior = FO.prior_vec(U, P.dtype, w_pose, w_beta)
    A, g, c = [], [], []
    for b in range(P.shape[0]):
        n = np.nonzero(matched[b])[0]
        cv = torch.from_numpy(idx[b, n].astype(np.int64))
        w = torch.from_numpy(np.asarray(weights[b, n], dtype=np.float64)).repeat_interleave(3)
        J = Jf[b][cv].reshape(-1, U)
        r = (mv[b][cv] - torch.from_numpy(np.asarray(points[b, n], dtype=np.float64))).reshape(-1)
        A.append(J.T @ (w.unsqueeze(1) * J) + torch.diag(prior))
        g.append(J.T @ (w * r) + prior * P[b])
        c.append((w * r * r).sum() + w_pose * (P[b, 3:48] ** 2).sum() + w_beta * (P[b, 48:58] ** 2).sum())
    return torch.stack(A), torch.stack(g), torch.stack(c)
