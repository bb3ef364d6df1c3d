"""fp64 torch statement of the MANO fit to a track of frames (include/scat_mano_fit_seq.h) on top of _fit_oracle: the
cost, the dense (62 T)^2 normal equations and the start; the assembly of the track's equations, the
Levenberg-Marquardt loop with the kernel's rules, one lambda and one accept / reject per sequence, the Procrustes and
the start's scan are _lm_oracle's.  The solve is a dense Cholesky: the dense factor of a block-tridiagonal matrix has
exactly the kernel's blocks (L_t on the diagonal, M_t below it, zeros elsewhere), so the fp32 run of this oracle is the
kernel's algorithm up to the order of the sums.  Test-only: imports none of scat_amd's kernels.

P is [S,T,62], targets [S,T,21,3], w [S,T,21]; smooth is the five weights (rots, poses, betas, trans, scale)."""
import torch

import _fit_oracle as FO
import _lm_oracle as L

U = FO.U
ALL = (1 << U) - 1


def dvec(smooth, dt):
    """the 62 smoothness weights d_i from the five of the groups"""
    return L.group_vec(zip((3, 45, 10, 3, 1), smooth), dt)


def free_vec(free, dt):
    return L.mask_vec(free, U, dt)


def cost(model, P, targets, w, joint_map, w_pose, w_beta, smooth):
    """[S]: the frames' costs, then the smoothness terms (a frozen unknown's count too)"""
    S, T = P.shape[:2]
    c = FO.cost(model, P.reshape(S * T, U), targets.reshape(S * T, 21, 3), w.reshape(S * T, 21), joint_map, w_pose, w_beta)
    return c.reshape(S, T).sum(1) + L.smooth_cost(P, dvec(smooth, P.dtype))


def equations(model, P, targets, w, joint_map, w_pose, w_beta, smooth, free=ALL):
    """-> H [S,62T,62T] (undamped, dense), g [S,62T]: _lm_oracle.chain of _fit_oracle's A_t and g_t with D = dvec, which
    has a zero where the unknown is frozen"""
    S, T = P.shape[:2]
    A, g, _ = FO.normal_equations(model, P.reshape(S * T, U), targets.reshape(S * T, 21, 3), w.reshape(S * T, 21), joint_map,
                                  w_pose, w_beta, free)
    return L.chain(A.reshape(S, T, U, U), g.reshape(S, T, U), P, dvec(smooth, P.dtype) * free_vec(free, P.dtype))


def normal_equations(model, P, targets, w, joint_map, w_pose, w_beta, smooth, free=ALL):
    """-> H, g of equations above and the cost [S] at P"""
    with torch.no_grad():
        c = cost(model, P, targets, w, joint_map, w_pose, w_beta, smooth)
    return equations(model, P, targets, w, joint_map, w_pose, w_beta, smooth, free) + (c,)


def lm(model, targets, w, joint_map, P0, iters, smooth, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=ALL, history=False):
    """-> P [S,T,62], cost [S], accepted [S] (and the per-iteration costs [iters,S]) in P0's dtype: _lm_oracle.lm"""
    dt = P0.dtype
    targets, w = targets.to(dt), w.to(dt)
    return L.lm(P0, iters, lambda0, lambda P: equations(model, P, targets, w, joint_map, w_pose, w_beta, smooth, free),
                lambda P: cost(model, P, targets, w, joint_map, w_pose, w_beta, smooth), free_vec(free, dt))[:4 if history else 3]


def track_start(X, targets, w):
    """what start below and _fit_seq_verts_oracle.start share -> [S,T,62] fp64: the Procrustes in fp64 of the zero-pose points
    X [1,J,3] (any dtype) onto every frame of targets [S,T,J,3], a frame of total weight zero with unit weights, then
    _lm_oracle.scan_start: such a frame takes every column of its neighbour's, a track without weight is zeros"""
    S, T, J = w.shape
    w = w.double()
    has = w.sum(2) > 0
    wf = torch.where(has.unsqueeze(2), w, torch.ones_like(w)).reshape(S * T, J)
    P = FO.similarity_start(X.double().expand(S * T, J, 3), targets.double().reshape(S * T, J, 3), wf)
    return L.scan_start(P.reshape(S, T, U), has)


def start(model, targets, w, joint_map, dt=torch.float64):
    """init = 1 -> [S,T,62] in dt: _fit_oracle's Procrustes start frame by frame (on zero-pose joints computed in dt: the
    kernel's are fp32; the Procrustes itself is fp64 whatever dt, as in the kernel), then track_start's scan: a frame of
    total weight zero takes its neighbour's start, and for t >= 1 rots_t is unwrapped towards rots_t-1"""
    return track_start(FO.joints(model, torch.zeros(1, U, dtype=dt))[:, list(joint_map)], targets, w).to(dt)


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
