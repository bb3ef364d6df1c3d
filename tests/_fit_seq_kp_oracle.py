"""fp64 torch statement of the MANO fit to a track of keypoints (include/scat_mano_fit_seq_kp.h) on top of _fit_kp_oracle
(the frame: 3-D and 2-D terms, the camera, the robust loss, the limits), _fit_seq_oracle (accel) and _lm_oracle (the track:
the smoothness, the dense assembly, the start's scan, and the Levenberg-Marquardt loop with the header's rules, one lambda
and one accept / reject per sequence): the cost, the dense (65 T)^2 normal equations and the start.  The solve is a dense
Cholesky, whose factor has exactly the kernel's blocks (_fit_seq_oracle has why).  Test-only: imports none of scat_amd's
kernels.

P is [S,T,65]; a Problem is _fit_kp_oracle's with T3 [S,T,21,3], w3 [S,T,21], T2 [S,T,21,2], w2 [S,T,21]; smooth is the seven
weights (rots, poses, betas, trans, scale, cam_scale, cam_trans).  Everything takes a dtype, as the two oracles do."""
import numpy as np
import torch

import _fit_kp_oracle as KO
import _fit_seq_oracle as SO
import _lm_oracle as L

U, U3 = KO.U, KO.U3
ALL = (1 << U3) - 1
KEYS = ("rots", "poses", "betas", "trans", "scale", "cam_scale", "cam_trans")


def sm(smooth):
    """the seven weights in the entry point's order from a dict; a missing key is 0"""
    return tuple(float(smooth.get(k, 0.0)) for k in KEYS)


def dvec(smooth, dt):
    """the 65 smoothness weights d_i from the seven of the groups"""
    return L.group_vec(zip((3, 45, 10, 3, 1, 1, 2), smooth), dt)


def free_vec(free, free_cam, dt):
    return torch.tensor(KO.free_bits(free, free_cam), dtype=dt)


def flat(pr):
    """the Problem of the S T frames as one batch"""
    f = lambda t: None if t is None else t.reshape(-1, *t.shape[2:])
    return pr._replace(T3=f(pr.T3), w3=f(pr.w3), T2=f(pr.T2), w2=f(pr.w2))


def cost(model, P, pr, smooth):
    """[S]: the frames' costs, then the smoothness terms (a frozen unknown's count too)"""
    S, T = P.shape[:2]
    return KO.cost(model, P.reshape(S * T, U), flat(pr)).reshape(S, T).sum(1) + L.smooth_cost(P, dvec(smooth, P.dtype))


def equations(model, P, pr, smooth, free=ALL, free_cam=7):
    """-> H [S,65T,65T] (undamped, dense), g [S,65T]: _lm_oracle.chain of _fit_kp_oracle's A_t and g_t (IRLS weights at P,
    limits included) with D = dvec, which has a zero where the unknown is frozen"""
    S, T = P.shape[:2]
    A, g = KO.normal_equations(model, P.detach().reshape(S * T, U), flat(pr), free, free_cam)
    return L.chain(A.reshape(S, T, U, U), g.reshape(S, T, U), P, dvec(smooth, P.dtype) * free_vec(free, free_cam, P.dtype))


def normal_equations(model, P, pr, smooth, free=ALL, free_cam=7):
    """-> H, g of equations above and the cost [S] at P"""
    with torch.no_grad():
        c = cost(model, P, pr, smooth)
    return equations(model, P, pr, smooth, free, free_cam) + (c,)


def lm(model, pr, P0, iters, smooth, lambda0=1e-3, free=ALL, free_cam=7, history=False):
    """-> P [S,T,65], cost [S], accepted [S] (and the costs [iters,S] and iterates [iters,S,T,65]): _fit_kp_oracle.lm's loop"""
    return L.lm(P0, iters, lambda0, lambda P: equations(model, P, pr, smooth, free, free_cam), lambda P: cost(model, P, pr, smooth),
                free_vec(free, free_cam, P0.dtype), finite_factor=True, no_grad=True)[:5 if history else 3]


def has_weight(pr, S, T):
    """[S,T] bool: sum w3 + sum w2 > 0, an absent term counting nothing and absent weights of a present term as ones"""
    _, w3, _, w2 = KO._terms(flat(pr), S * T, torch.float64)
    return ((w3.sum(1) + w2.sum(1)) > 0).reshape(S, T)


def start(model, pr, S, T, dtype=torch.float64):
    """init = 1 -> [S,T,65] in dtype: _fit_kp_oracle.start frame by frame, then _lm_oracle.scan_start on the rounded
    values, in fp64 as in the kernel: a frame of total weight zero takes the rots, trans, log_scale and camera of the frame
    before it, frame 0 those of the first frame with weight, and a track without weight keeps its frames' starts (the
    camera's is not zero); then for t >= 1 rots_t is unwrapped towards rots_t-1 and stored rounded to dtype.  The
    2-D-only mirror candidate of a frame is not revisited."""
    P = KO.start(model, flat(pr), S * T, dtype).double().reshape(S, T, U)
    return L.scan_start(P, has_weight(pr, S, T), carry=list(range(3)) + list(range(58, U)), zero_empty=False, store=dtype).to(dtype)


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
