"""fp64 torch statement of the MANO fit to a track of multi-view keypoints (include_ext/scat_mano_fit_seq_views.h) on top
of _fit_views_oracle (what a frame is: the cost, the IRLS normal equations, the triangulated start), _lm_oracle (chain,
smooth_cost, scan_start, lm) and _fit_seq_oracle (dvec, accel): the cost, the dense (62 T)^2 equations, the
Levenberg-Marquardt loop with the kernel's not-fitted rules, and the start (triangulation flag -> scan).  The solve is a
dense Cholesky, whose factor of a block-tridiagonal matrix has exactly the kernel's blocks.  Test-only: imports none of
scat_amd's kernels.

P is [S,T,62], T2 [S,T,C,21,2], w2 [S,T,C,21], cams [Sc,C,16] with Sc 1 or S: the rig is fixed along a track."""
from typing import NamedTuple, Optional

import torch

import _fit_seq_oracle as SO
import _fit_views_oracle as VO
import _lm_oracle as L

U = 62
ALL = (1 << U) - 1
rel, dvec, accel, frame_joints = VO.rel, SO.dvec, SO.accel, SO.frame_joints


class Problem(NamedTuple):
    """one call's data and settings; w2 None means all ones; cams [1,C,16] is one rig for all sequences"""
    joint_map: tuple
    cams: torch.Tensor                      # [Sc,C,16]
    T2: torch.Tensor                        # [S,T,C,21,2] pixels
    w2: Optional[torch.Tensor] = None       # [S,T,C,21]
    lo: Optional[torch.Tensor] = None       # [45]
    hi: Optional[torch.Tensor] = None
    w_pose: float = 1e-2
    w_beta: float = 1e-2
    w_limit: float = 0.0
    sigma2: float = 0.0
    z_near: float = 1e-3
    smooth: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)      # rots, poses, betas, trans, scale


def frames(pr):
    """the S T frames as one batch of _fit_views_oracle: the rig of a sequence for each of its frames"""
    S, T = pr.T2.shape[:2]
    cams = pr.cams if pr.cams.shape[0] == 1 else pr.cams.repeat_interleave(T, dim=0)
    return VO.Problem(pr.joint_map, cams, pr.T2.flatten(0, 1), None if pr.w2 is None else pr.w2.flatten(0, 1), pr.lo, pr.hi,
                      pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma2, pr.z_near)


def cost(model, P, pr):
    """[S]: the frames' costs (+inf with a view-joint behind a camera in any frame), then the smoothness terms"""
    S, T = P.shape[:2]
    return VO.cost(model, P.reshape(S * T, U), frames(pr)).reshape(S, T).sum(1) + L.smooth_cost(P, dvec(pr.smooth, P.dtype))


def frame_equations(model, P, pr, free=ALL):
    """-> A [S,T,62,62], g [S,T,62]: _fit_views_oracle.normal_equations of every frame"""
    S, T = P.shape[:2]
    A, g = VO.normal_equations(model, P.reshape(S * T, U), frames(pr), free)
    return A.reshape(S, T, U, U), g.reshape(S, T, U)


def equations(model, P, pr, free=ALL):
    """-> H [S,62T,62T] (undamped, dense), g [S,62T]: _lm_oracle.chain of the frames' blocks with D = dvec, zero where frozen"""
    A, g = frame_equations(model, P, pr, free)
    return L.chain(A, g, P, dvec(pr.smooth, P.dtype) * L.mask_vec(free, U, P.dtype))


def usable(pr):
    """[S] bool: every keypoint, weight and camera entry of every frame is finite and no weight is negative"""
    S, T = pr.T2.shape[:2]
    return VO.usable(frames(pr)).reshape(S, T).all(1)


def lm(model, pr, P0, iters, lambda0=1e-3, free=ALL, history=False):
    """-> P [S,T,62], cost [S], accepted [S] (and the per-iteration costs and iterates) in P0's dtype: _lm_oracle.lm with
    one lambda and one accept / reject per sequence.  A sequence that is unusable, or behind a camera at P0 in any frame,
    is not fitted: P0, +inf, 0.  A trial behind a camera in any frame costs +inf and is rejected."""
    out = list(L.lm(P0, iters, lambda0, lambda P: equations(model, P, pr, free), lambda P: cost(model, P, pr),
                    L.mask_vec(free, U, P0.dtype), finite_factor=True, no_grad=True))
    with torch.no_grad():
        skip = ~usable(pr) | ~torch.isfinite(cost(model, P0, pr))
    out[0] = torch.where(skip[:, None, None], P0, out[0])
    out[1] = torch.where(skip, torch.full_like(out[1], float("inf")), out[1])
    out[2] = torch.where(skip, torch.zeros_like(out[2]), out[2])
    return tuple(out[:5 if history else 3])


def start(model, pr, dtype=torch.float64):
    """init = 1 -> P [S,T,62] in dtype, has [S,T] bool (the frame has at least 3 triangulated joints), fitted [S] bool:
    _fit_views_oracle.start frame by frame, rounded to dtype as the start kernel stores it, then _lm_oracle.scan_start with
    that flag: a frame without a start takes its neighbour's, rots is unwrapped along t.  A sequence without any start
    (an unusable one among them) is zeros and not fitted."""
    S, T = pr.T2.shape[:2]
    P, has = VO.start(model, frames(pr), dtype)
    has = has.reshape(S, T) & usable(pr)[:, None]
    P = L.scan_start(P.double().reshape(S, T, U), has, store=dtype)
    return P.to(dtype), has, has.any(1)


def joint_rms(model, P, pr, X3):
    """per sequence, the root of the mean squared distance of every frame's model joints at P to X3 [S,T,21,3], fp64"""
    d = ((frame_joints(model, P, pr.joint_map) - X3.double()) ** 2).sum(3)
    return d.flatten(1).mean(1).sqrt()


def frame_joint_rms(model, P, pr, X3):
    """the same per frame, [S,T]"""
    return ((frame_joints(model, P, pr.joint_map) - X3.double()) ** 2).sum(3).mean(2).sqrt()


def pixel_rms(model, P, pr, T2, sel=None):
    """per sequence, the root of the mean squared reprojection distance to T2 [S,T,C,21,2] in pixels, fp64; sel [S,T,C,21]
    bool: those view-joints only"""
    S, T = P.shape[:2]
    with torch.no_grad():
        d = ((VO.reproject(model, P.double().reshape(S * T, U), frames(pr)) - T2.double().flatten(0, 1)) ** 2).sum(3).reshape(S, -1)
    if sel is None:
        return d.mean(1).sqrt()
    sel = sel.reshape(S, -1)
    return ((d * sel).sum(1) / sel.sum(1)).sqrt()
