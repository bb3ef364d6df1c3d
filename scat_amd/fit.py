"""The inverse of the MANO layer on the device (include/scat_mano_fit.h, csrc/mano_fit.hip): pose, shape and a
similarity fitted to 21 joints by Levenberg-Marquardt, one launch for the whole batch.  It connects the headline networks,
which predict [B,66] (camera + 21 joints), to ManoLayer and MeshRenderer, which want the MANO parameters:

    fitter = ManoFitter(ManoModel.synthetic(1).to("cuda"))
    res = fitter.fit_outputs(out66)                    # FitResult(rots, poses, betas, trans, scale, cost, accepted)
    verts = fitter.mesh(res)                           # [B,V,3] in the frame of the predicted joints
    frames = renderer.render(verts, out66[:, :3])      # with the predicted camera

fit_keypoints (include/scat_mano_fit_kp.h, csrc/mano_fit_kp.hip) takes 2-D keypoints in pixels, 3-D joints or both, with a
Geman-McClure loss and joint limits, and solves for the weak-perspective camera as well:

    res = fitter.fit_keypoints(joints2d=kp2d, sigma2=10.0)     # KeypointFitResult(..., cam, cost, accepted, p)
    frames = renderer.render(fitter.mesh(res), res.cam)        # lands on the keypoints

fit_sequence (include/scat_mano_fit_seq.h, csrc/mano_fit_seq.hip) fits a track of frames in one solve, consecutive frames
tied by a smoothness penalty that decides what 21 joints leave free (twist, a shape that flickers) and bridges frames
without data:

    res = fitter.fit_sequence(joints, smooth=dict(rots=1e-4, poses=1e-4, betas=1e-2, trans=1e-1, scale=1e-1))
    verts = fitter.mesh(res)                           # [S,T,V,3]

fit_keypoints_sequence (include/scat_mano_fit_seq_kp.h, csrc/mano_fit_seq_kp.hip) is the two together, what video needs:
a track of 2-D keypoints (and / or 3-D joints) with outliers and gaps, the camera among the unknowns, one solve per track:

    res = fitter.fit_keypoints_sequence(joints2d=kp, sigma2=10.0,      # from 2-D alone the data term is in pixels squared
                                        smooth=dict(rots=6e3, poses=2e3, betas=2e4, cam_scale=1e3, cam_trans=4e5))
    frames = renderer.render(fitter.mesh(res).flatten(0, 1), res.cam.flatten(0, 1))

fit_vertices (include/scat_mano_fit_verts.h, csrc/mano_fit_verts.hip) takes a mesh in the model's topology, which decides
the twist and the shape that 21 joints leave open; a joints fit of the same hand is its natural warm start:

    res = fitter.fit_vertices(verts)                   # FitResult; verts [B,V,3], vertex v is the model's vertex v
    res = fitter.fit_vertices(verts, init=fitter.fit(joints))

fit_points (include/scat_mano_fit_points.h, csrc/mano_fit_points.hip) takes an unordered cloud, a depth camera's or a
scanner's: nearest-vertex ICP from the caller's start, every round one assignment launch and one fit_vertices launch:

    res = fitter.fit_points(cloud, init=fitter.fit(joints), max_dist=0.03)     # PointFitResult; cloud [B,N,3]
    corr = fitter.nearest_vertices(res, cloud)         # Correspondences(idx, dist, vertex_weight, vertex_target, ...)

fit_points_plane (include/scat_mano_fit_plane.h, the same two sources) is point-to-plane ICP for a cloud of points on the
surface, which never hits the vertices: the residual counts along the matched vertex's normal and little across it.  It
needs the model's faces (an array, or the MeshRenderer that draws the hand):

    res = fitter.fit_points_plane(cloud, init=fitter.fit(joints), faces=renderer)      # PointFitResult, plane metric
    normals = fitter.vertex_normals(res, renderer)     # [B,V,3]

fit_vertices_sequence and fit_points_sequence (include/scat_mano_fit_seq_verts.h, csrc/mano_fit_seq_verts.hip) are the
last two over a track, what a depth camera's clip needs: the frames are assembled side by side, one workgroup each, and
one workgroup per track eliminates along the frames; a frame in which nothing matches is bridged by its neighbours:

    res = fitter.fit_vertices_sequence(meshes, smooth=dict(rots=4e-3, poses=4e-3, trans=4.0))   # meshes [S,T,V,3]
    res = fitter.fit_points_sequence(clouds, init=fitter.fit_sequence(joints), faces=renderer, max_dist=0.03)
    frames = renderer.render(fitter.mesh(res).flatten(0, 1), cams)

fit_keypoints_views (include_ext/scat_mano_fit_views.h, csrc/mano_fit_views.hip) takes 2-D keypoints seen by C calibrated
pinhole cameras, what a capture rig gives: no camera unknowns, depth and metric scale observable, a detection that is wrong in
one view voted down by the others; the start is triangulated:

    cams = Cameras(R, t, K)                            # [Bc,C,3,3], [Bc,C,3], [Bc,C,4] = fx, fy, cx, cy; Bc is 1 or B
    res = fitter.fit_keypoints_views(kp, cams, sigma2=10.0)      # FitResult in the rig's frame; kp [B,C,21,2] pixels
    points, valid = fitter.triangulate(kp, cams)       # [B,21,3], [B,21] bool
    uv = fitter.project_views(res, cams)               # [B,C,21,2]

fit_keypoints_views_sequence (include_ext/scat_mano_fit_seq_views.h, csrc/mano_fit_seq_views.hip) is that frame inside
fit_sequence's track, what a rig's clip needs: one solve per track, a frame that only one camera sees (or none) bridged by
its neighbours, twist and shape steady over time:

    res = fitter.fit_keypoints_views_sequence(kp, cams, sigma2=10.0,       # SequenceFitResult; kp [S,T,C,21,2] pixels
                                              smooth=dict(rots=1e2, poses=1e2, betas=1e3, trans=1e6, scale=1e4))
    uv = fitter.project_views(res, cams)               # [S,T,C,21,2]

There is no CPU fallback: CPU tensors raise ScatError."""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import numpy as np
import torch

from ._lib import HERE, ScatError, lib
from .mano import BETAS, MAX_V, POSE, ManoModel, _model_args, _need_gpu, mano_fwd
from .ops import _p, _stream

UNKNOWNS = 62                  # rots 3, poses 45, betas 10, trans 3, log_scale 1: SCAT_FIT_UNKNOWNS
MAX_ITERS = 64                 # SCAT_FIT_MAX_ITERS
ALL_FREE = (1 << UNKNOWNS) - 1
KP_UNKNOWNS = 65               # the 62, then the camera cs, ctx, cty: SCAT_FIT_KP_UNKNOWNS
SEQ_MAX_T = 256                # SCAT_FIT_SEQ_MAX_T
SMOOTH_KEYS = ("rots", "poses", "betas", "trans", "scale")      # s_rots .. s_scale, in the entry point's order
# s_rots .. s_ct of scat_mano_fit_seq_kp, in the entry point's order: the five, then the camera's scale and its offsets
SMOOTH_KP_KEYS = SMOOTH_KEYS + ("cam_scale", "cam_trans")
# bound on first use by lib().bind, beside _lib.py's tables: the MANO fits to a full mesh, a point cloud, a track of keypoints
FIT_VERTS_HEADER, FIT_POINTS_HEADER, FIT_SEQ_KP_HEADER, FIT_PLANE_HEADER = (
    os.path.join(HERE, "..", "include", f"scat_mano_fit_{n}.h") for n in ("verts", "points", "seq_kp", "plane"))
# the MANO fit to a track of meshes and to a track of point clouds
FIT_SEQ_VERTS_HEADER = os.path.join(HERE, "..", "include", "scat_mano_fit_seq_verts.h")
# the MANO fit to keypoints in calibrated views; include_ext/ holds the headers added since the suite counts include/'s
FIT_VIEWS_HEADER = os.path.join(HERE, "..", "include_ext", "scat_mano_fit_views.h")
# the MANO fit to a track of keypoints in calibrated views
FIT_SEQ_VIEWS_HEADER = os.path.join(HERE, "..", "include_ext", "scat_mano_fit_seq_views.h")
VIEWS_MAX_C = 8                # SCAT_FIT_VIEWS_MAX_C
MAX_F = 4096                   # SCAT_RENDER_MAX_F
POINTS_MAX_N = 8192            # SCAT_FIT_POINTS_MAX_N
POINTS_MAX_ROUNDS = 64         # SCAT_FIT_POINTS_MAX_ROUNDS
POINTS_MAX_STEPS = 256         # SCAT_FIT_POINTS_MAX_STEPS: rounds * iters
SLICES = {"rots": slice(0, 3), "poses": slice(3, 48), "betas": slice(48, 58), "trans": slice(58, 61), "log_scale": slice(61, 62)}


def free_mask(**free):
    """the mask with the named groups frozen: free_mask(betas=False, log_scale=False)"""
    m = ALL_FREE
    for k, on in free.items():
        s = SLICES[k]
        if not on:
            m &= ~(((1 << (s.stop - s.start)) - 1) << s.start)
    return m


class FitResult(NamedTuple):
    rots: torch.Tensor       # [B,3]
    poses: torch.Tensor      # [B,45]
    betas: torch.Tensor      # [B,10]
    trans: torch.Tensor      # [B,3]
    scale: torch.Tensor      # [B]
    cost: torch.Tensor       # [B], +inf for a sample whose targets were not finite
    accepted: torch.Tensor   # [B] int32
    p: torch.Tensor          # [B,62]: the five groups as the kernel holds them (log_scale last)


class KeypointFitResult(NamedTuple):
    rots: torch.Tensor       # [B,3]
    poses: torch.Tensor      # [B,45]
    betas: torch.Tensor      # [B,10]
    trans: torch.Tensor      # [B,3]
    scale: torch.Tensor      # [B]
    cam: torch.Tensor        # [B,3]: (s, tx, ty), the camera of project_outputs and MeshRenderer.render
    cost: torch.Tensor       # [B], +inf for a sample whose targets were not finite
    accepted: torch.Tensor   # [B] int32
    p: torch.Tensor          # [B,65]: the six groups as the kernel holds them (log_scale, then the camera, last)


class SequenceFitResult(NamedTuple):
    rots: torch.Tensor       # [S,T,3]
    poses: torch.Tensor      # [S,T,45]
    betas: torch.Tensor      # [S,T,10]
    trans: torch.Tensor      # [S,T,3]
    scale: torch.Tensor      # [S,T]
    cost: torch.Tensor       # [S], +inf for a sequence with a target or weight that was not finite
    accepted: torch.Tensor   # [S] int32
    p: torch.Tensor          # [S,T,62]: the five groups as the kernel holds them (log_scale last)


class KeypointSequenceFitResult(NamedTuple):
    rots: torch.Tensor       # [S,T,3]
    poses: torch.Tensor      # [S,T,45]
    betas: torch.Tensor      # [S,T,10]
    trans: torch.Tensor      # [S,T,3]
    scale: torch.Tensor      # [S,T]
    cam: torch.Tensor        # [S,T,3]: (s, tx, ty) per frame, the camera of project_outputs and MeshRenderer.render
    cost: torch.Tensor       # [S], +inf for a sequence with a target or weight that was not finite
    accepted: torch.Tensor   # [S] int32
    p: torch.Tensor          # [S,T,65]: the six groups as the kernel holds them (log_scale, then the camera, last)


class Correspondences(NamedTuple):
    idx: torch.Tensor             # [B,N] int32: the nearest vertex, -1 for a point of weight 0
    dist: torch.Tensor            # [B,N]: the distance to it, 0 for a point of weight 0
    vertex_weight: torch.Tensor   # [B,V]: the matched weight per vertex; a NaN row: unusable, or nothing matched
    vertex_target: torch.Tensor   # [B,V,3]: the weighted centroid of a vertex's matched points, 0 where it has none
    matched: torch.Tensor         # [B] int64: matched points
    matched_weight: torch.Tensor  # [B] fp64
    data_cost: torch.Tensor       # [B] fp64: sum w d^2 over the matched points, no priors; +inf for an unusable hand


class PointFitResult(NamedTuple):
    rots: torch.Tensor       # [B,3]
    poses: torch.Tensor      # [B,45]
    betas: torch.Tensor      # [B,10]
    trans: torch.Tensor      # [B,3]
    scale: torch.Tensor      # [B]
    data_cost: torch.Tensor  # [B]: sum w d^2 over the matched points at p, no priors; +inf for an unusable hand
    accepted: torch.Tensor   # [B] int32: accepted steps, summed over the rounds
    p: torch.Tensor          # [B,62]: the five groups as the kernel holds them (log_scale last)
    matched: torch.Tensor    # [B] int64: matched points at p
    rms: torch.Tensor        # [B]: sqrt(data_cost / matched weight), +inf when nothing matched
    idx: torch.Tensor        # [B,N] int32: the nearest vertex at p, -1 for a point of weight 0
    dist: torch.Tensor       # [B,N]


class PointSequenceFitResult(NamedTuple):
    rots: torch.Tensor       # [S,T,3]
    poses: torch.Tensor      # [S,T,45]
    betas: torch.Tensor      # [S,T,10]
    trans: torch.Tensor      # [S,T,3]
    scale: torch.Tensor      # [S,T]
    data_cost: torch.Tensor  # [S,T]: sum w d^2 (with faces: the plane metric) over a frame's matched points at p; +inf: unusable
    accepted: torch.Tensor   # [S] int32: accepted steps of the sequence, summed over the rounds
    p: torch.Tensor          # [S,T,62]: the five groups as the kernel holds them (log_scale last)
    matched: torch.Tensor    # [S,T] int64: matched points at p
    rms: torch.Tensor        # [S,T]: sqrt(data_cost / matched weight), +inf when nothing matched
    idx: torch.Tensor        # [S,T,N] int32: the nearest vertex at p, -1 for a point of weight 0
    dist: torch.Tensor       # [S,T,N]


class Cameras(NamedTuple):
    """C calibrated pinhole cameras: a point m of the world is q = R m + t in a camera, which looks along +z, and lands on
    the pixel (fx q.x / q.z + cx, fy q.y / q.z + cy).  Bc = 1 is one rig for the whole batch, Bc = B one rig per sample."""
    R: torch.Tensor          # [Bc,C,3,3]
    t: torch.Tensor          # [Bc,C,3]
    K: torch.Tensor          # [Bc,C,4]: fx, fy, cx, cy

    def check(self, what="Cameras"):
        """shapes, dtype and device -> (Bc, C)"""
        R, t, K = self
        if not all(isinstance(a, torch.Tensor) for a in self) or R.dim() != 4:
            raise ScatError(f"{what} needs tensors R [Bc,C,3,3], t [Bc,C,3], K [Bc,C,4]")
        Bc, C = int(R.shape[0]), int(R.shape[1])
        if Bc < 1 or not 1 <= C <= VIEWS_MAX_C or tuple(R.shape) != (Bc, C, 3, 3) or tuple(t.shape) != (Bc, C, 3) \
                or tuple(K.shape) != (Bc, C, 4):
            raise ScatError(f"{what} needs R [Bc,C,3,3], t [Bc,C,3], K [Bc,C,4] with Bc >= 1 and C in 1..{VIEWS_MAX_C}, got "
                            f"{tuple(R.shape)}, {tuple(t.shape)}, {tuple(K.shape)}")
        if not all(a.dtype == torch.float32 for a in self):
            raise ScatError(f"{what} needs fp32 tensors, got {R.dtype}, {t.dtype}, {K.dtype}")
        if not (R.device == t.device == K.device):
            raise ScatError(f"{what}: R, t and K are on {R.device}, {t.device} and {K.device}")
        return Bc, C

    def packed(self):
        """-> [Bc,C,16] fp32, as scat_mano_fit_views.h takes the cameras: R row-major, t, fx, fy, cx, cy"""
        Bc, C = self.check()
        return torch.cat([self.R.reshape(Bc, C, 9), self.t, self.K], dim=2).contiguous()

    def weak_perspective(self, view, depth, size):
        """-> (R [Bc,3,3], t [Bc,3], cam [Bc,3]): camera `view` as MeshRenderer.render and project_outputs take one, for a
        hand at the distance `depth` (a number, or [Bc]) in a frame of size = (H, W).  The mesh goes into the camera's
        frame, verts @ R^T + t, and cam = (cs, ctx, cty) with cs = fx / (depth W / 2), ctx = (cx - W / 2) / (cs W / 2),
        cty = (cy - H / 2) / (cs H / 2) agrees with the pinhole on the plane z = depth.  The renderer has one scale, so
        cameras whose fx / (W / 2) and fy / (H / 2) differ by more than 1e-6 relative are refused."""
        Bc, C = self.check("Cameras.weak_perspective")
        if not 0 <= int(view) < C:
            raise ScatError(f"Cameras.weak_perspective: view {view} outside 0..{C - 1}")
        H, W = (float(v) for v in size)
        if not (H > 0 and W > 0):
            raise ScatError(f"Cameras.weak_perspective: size {size} must be positive")
        K = self.K[:, int(view)]
        sx, sy = K[:, 0] / (0.5 * W), K[:, 1] / (0.5 * H)
        if bool(((sx - sy).abs() > 1e-6 * torch.maximum(sx.abs(), sy.abs())).any()):
            raise ScatError("Cameras.weak_perspective: fx / (W / 2) and fy / (H / 2) differ, and the renderer has one scale")
        depth = torch.as_tensor(depth, dtype=torch.float32, device=K.device).expand(Bc)
        if not bool((depth > 0).all()):
            raise ScatError("Cameras.weak_perspective: depth must be positive")
        cs = sx / depth
        cam = torch.stack([cs, (K[:, 2] - 0.5 * W) / (cs * 0.5 * W), (K[:, 3] - 0.5 * H) / (cs * 0.5 * H)], dim=1)
        return self.R[:, int(view)].contiguous(), self.t[:, int(view)].contiguous(), cam.contiguous()


def project_points(points, cameras):
    """points [B,J,3] of the world through every camera of a Cameras -> [B,C,J,2] pixels; plain torch, any device and
    floating dtype, no rule about points behind a camera"""
    q = torch.einsum("bcik,bjk->bcji", cameras.R, points) + cameras.t[:, :, None, :]
    K = cameras.K[:, :, None, :]
    return (K[..., 0:2] * q[..., 0:2] / q[..., 2:3] + K[..., 2:4]).contiguous()


def _check_model(what, model, ref):
    if model.device is None or model.device != ref.device:
        raise ScatError(f"{what}: the model is on {model.device}, the inputs on {ref.device}: call ManoModel.to first")


def _start(what, init, result_types, shape, device):
    """the p of `shape` a kernel reads and writes: empty for init None, else a checked copy of init (a tensor, or the p of a
    result of one of result_types)"""
    if init is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    p0 = init.p if isinstance(init, result_types) else init
    _need_gpu(what, p0)
    if tuple(p0.shape) != tuple(shape) or p0.dtype != torch.float32:
        raise ScatError(f"{what} needs an fp32 start [{','.join(str(n) for n in shape)}], got {p0.dtype} {tuple(p0.shape)}")
    return p0.clone().contiguous()


def _weights(what, weights, shape):
    """the checked weights of `shape`, contiguous, or None"""
    if weights is None:
        return None
    if tuple(weights.shape) != tuple(shape) or weights.dtype != torch.float32:
        raise ScatError(f"{what} needs fp32 weights [{','.join(str(n) for n in shape)}], got {weights.dtype} "
                        f"{tuple(weights.shape)}")
    return weights.contiguous()


def _results(n, device):
    """cost [n] and accepted [n] int32 for a kernel to write"""
    return torch.empty((n,), dtype=torch.float32, device=device), torch.empty((n,), dtype=torch.int32, device=device)


def _workspace(query, sizes, device, least=16):
    """(ws, nbytes): a workspace of the size query(*sizes) gives (0 for sizes the launch refuses), never empty"""
    nbytes = int(query(*sizes))
    return torch.empty((max(nbytes, least),), dtype=torch.uint8, device=device), nbytes


def _model_inputs(what, model, rots, poses, betas):
    """the checked rots [B,3], poses [B,45], betas [B,10] of a Jacobian's entry point, contiguous, and B"""
    _need_gpu(what, rots, poses, betas)
    _check_model(what, model, rots)
    B = rots.shape[0]
    if B == 0 or tuple(rots.shape) != (B, 3) or tuple(poses.shape) != (B, POSE) or tuple(betas.shape) != (B, BETAS):
        raise ScatError(f"{what} needs rots [B,3], poses [B,45], betas [B,10] with B >= 1, got {tuple(rots.shape)}, "
                        f"{tuple(poses.shape)}, {tuple(betas.shape)}")
    if not all(t.dtype == torch.float32 for t in (rots, poses, betas)):
        raise ScatError(f"{what} needs fp32 tensors")
    return rots.contiguous(), poses.contiguous(), betas.contiguous(), B


def _check_ranges(what, iters, masks_ok, and_cam=""):
    if not 1 <= iters <= MAX_ITERS:
        raise ScatError(f"{what}: {iters} iterations outside 1..{MAX_ITERS}")
    if not masks_ok:
        raise ScatError(f"{what}: free has bits above {UNKNOWNS - 1} set{and_cam}")


def _smooth(what, smooth, keys=SMOOTH_KEYS):
    """the smoothness weights in the entry point's order, from a dict with keys among `keys`"""
    smooth = {} if smooth is None else dict(smooth)
    unknown = sorted(set(smooth) - set(keys))
    if unknown:
        raise ScatError(f"{what}: unknown smooth keys {unknown}, the groups are {list(keys)}")
    out = tuple(float(smooth.get(k, 0.0)) for k in keys)
    for k, v in zip(keys, out):
        if not (math.isfinite(v) and v >= 0.0):
            raise ScatError(f"{what}: smooth[{k!r}] = {v} must be finite and not negative")
    return out


def _groups(p):
    """rots, poses, betas, trans, scale: the five groups every fit's p begins with"""
    return p[..., 0:3], p[..., 3:48], p[..., 48:58], p[..., 58:61], torch.exp(p[..., 61])


def mano_joints_jac(model, rots, poses, betas):
    """-> (joints [B,21,3], jac [B,63,58]): the 21 joints of mano_fwd and d joints / d (rots, poses, betas), one launch"""
    rots, poses, betas, B = _model_inputs("mano_joints_jac", model, rots, poses, betas)
    joints = torch.empty((B, 21, 3), dtype=torch.float32, device=rots.device)
    jac = torch.empty((B, 63, 58), dtype=torch.float32, device=rots.device)
    lib().scat_mano_joints_jac(*_model_args(model), _p(rots), _p(poses), _p(betas), _p(joints), _p(jac), B, model.V,
                               model.parents_packed, *model.tips, _stream())
    return joints, jac


def mano_fit(model, targets, weights, joint_map, p, iters, init, lambda0, w_pose, w_beta, free=ALL_FREE):
    """scat_mano_fit as it is declared: targets [B,21,3], weights [B,21] or None, joint_map int32 [21] on the device,
    p [B,62] (read when init = 0, written) -> (cost [B], accepted [B] int32)"""
    B = targets.shape[0]
    cost, accepted = _results(B, targets.device)
    lib().scat_mano_fit(*_model_args(model), _p(targets), _p(weights), _p(joint_map), _p(p), _p(cost), _p(accepted), B, model.V,
                        model.parents_packed, *model.tips, int(iters), int(init), float(lambda0), float(w_pose), float(w_beta),
                        int(free), _stream())
    return cost, accepted


def mano_verts_jac(model, rots, poses, betas):
    """-> (verts [B,V,3], jac [B,3V,58]): the mesh of mano_fwd (its rows 21..) and d verts / d (rots, poses, betas), one
    launch"""
    rots, poses, betas, B = _model_inputs("mano_verts_jac", model, rots, poses, betas)
    verts = torch.empty((B, model.V, 3), dtype=torch.float32, device=rots.device)
    jac = torch.empty((B, 3 * model.V, 58), dtype=torch.float32, device=rots.device)
    lib().bind(FIT_VERTS_HEADER).scat_mano_verts_jac(*_model_args(model), _p(rots), _p(poses), _p(betas), _p(verts), _p(jac), B,
                                                     model.V, model.parents_packed, _stream())
    return verts, jac


def mano_fit_verts(model, targets, weights, p, iters, init, lambda0, w_pose, w_beta, free=ALL_FREE):
    """scat_mano_fit_verts as it is declared: targets [B,V,3], weights [B,V] or None, p [B,62] (read when init = 0,
    written) -> (cost [B], accepted [B] int32)"""
    B = targets.shape[0]
    cost, accepted = _results(B, targets.device)
    lib().bind(FIT_VERTS_HEADER).scat_mano_fit_verts(*_model_args(model), _p(targets), _p(weights), _p(p), _p(cost), _p(accepted), B,
                                                     model.V, model.parents_packed, int(iters), int(init), float(lambda0),
                                                     float(w_pose), float(w_beta), int(free), _stream())
    return cost, accepted


def _max_dist(what, max_dist):
    d = math.inf if max_dist is None else float(max_dist)
    if not d > 0.0:
        raise ScatError(f"{what}: max_dist {max_dist} must be positive (None: no trim)")
    return d


def _cloud_outputs(B, N, V, device):
    return (torch.empty((B, N), dtype=torch.int32, device=device), torch.empty((B, N), dtype=torch.float32, device=device),
            torch.empty((B, V), dtype=torch.float32, device=device), torch.empty((B, V, 3), dtype=torch.float32, device=device),
            torch.empty((B, 4), dtype=torch.float64, device=device))


def _correspondences(idx, dist, vw, vtarget, stats):
    return Correspondences(idx, dist, vw, vtarget, stats[:, 2].long(), stats[:, 1], stats[:, 3])


def cloud_assign(verts, points, weights, max_dist):
    """scat_cloud_assign as it is declared: verts [B,V,3], points [B,N,3], weights [B,N] or None, max_dist > 0 (inf: no
    trim) -> Correspondences"""
    B, V, N = verts.shape[0], verts.shape[1], points.shape[1]
    idx, dist, vw, vtarget, stats = _cloud_outputs(B, N, V, points.device)
    lib().bind(FIT_POINTS_HEADER).scat_cloud_assign(_p(verts), _p(points), _p(weights), float(max_dist), _p(idx), _p(dist), _p(vw),
                                                    _p(vtarget), _p(stats), B, N, V, _stream())
    return _correspondences(idx, dist, vw, vtarget, stats)


def mano_cloud_assign(model, p, points, weights, max_dist, want_model_pts=False):
    """scat_mano_cloud_assign as it is declared: p [B,62], points [B,N,3], weights [B,N] or None -> Correspondences, and
    with want_model_pts (Correspondences, model_pts [B,V,3])"""
    B, V, N = p.shape[0], model.V, points.shape[1]
    idx, dist, vw, vtarget, stats = _cloud_outputs(B, N, V, points.device)
    mp = torch.empty((B, V, 3), dtype=torch.float32, device=points.device) if want_model_pts else None
    lib().bind(FIT_POINTS_HEADER).scat_mano_cloud_assign(*_model_args(model), _p(p), _p(points), _p(weights), float(max_dist), _p(mp),
                                                         _p(idx), _p(dist), _p(vw), _p(vtarget), _p(stats), B, N, V,
                                                         model.parents_packed, _stream())
    c = _correspondences(idx, dist, vw, vtarget, stats)
    return (c, mp) if want_model_pts else c


def _icp_launch(query, entry, model, points, weights, topo_ptrs, p, n_accepted, sizes, tail):
    """The launch of every ICP loop: allocates data_cost (the points' leading shape), accepted [n_accepted], idx, dist and
    the workspace, at the size query(*sizes) gives (0 for sizes the launch refuses), and calls entry with the model, points,
    weights, topo_ptrs, p, these, sizes, the tree and tail -> (data_cost, accepted int32, idx int32, dist, stats [...,4] fp64
    of the last assignment, which is the head of the workspace)"""
    lead, N, dev = tuple(int(n) for n in points.shape[:-2]), int(points.shape[-2]), points.device
    hands = math.prod(lead)
    cost = torch.empty(lead, dtype=torch.float32, device=dev)
    accepted = torch.empty((n_accepted,), dtype=torch.int32, device=dev)
    idx = torch.empty(lead + (N,), dtype=torch.int32, device=dev)
    dist = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(query, sizes, dev, max(32 * hands, 16))
    entry(*_model_args(model), _p(points), _p(weights), *topo_ptrs, _p(p), _p(cost), _p(accepted), _p(idx), _p(dist), _p(ws), nbytes,
          *sizes, model.parents_packed, *tail, _stream())
    return cost, accepted, idx, dist, ws[:32 * hands].view(torch.float64).reshape(*lead, 4).clone()


def mano_fit_points(model, points, weights, p, rounds, iters, max_dist, lambda0, w_pose, w_beta, free=ALL_FREE):
    """scat_mano_fit_points as it is declared: points [B,N,3], weights [B,N] or None, p [B,62] read and written ->
    (data_cost [B], accepted [B] int32, idx [B,N] int32, dist [B,N], stats [B,4] fp64 of the last assignment).  The
    workspace is allocated here, at the size scat_mano_fit_points_ws gives (0 for sizes the launch refuses)."""
    B, N = int(points.shape[0]), int(points.shape[1])
    ns = lib().bind(FIT_POINTS_HEADER)
    return _icp_launch(ns.scat_mano_fit_points_ws, ns.scat_mano_fit_points, model, points, weights, (), p, B, (B, N, model.V),
                       (int(rounds), int(iters), float(max_dist), float(lambda0), float(w_pose), float(w_beta), int(free)))


class Topology(NamedTuple):
    """a mesh topology on the device, as scat_render.h and scat_mano_fit_plane.h take it"""
    faces: torch.Tensor      # [F,3] int32
    vf_off: torch.Tensor     # [V+1] int32
    vf_idx: torch.Tensor     # [3F] int32: vf_idx[vf_off[v]:vf_off[v+1]] are the faces that name vertex v

    @property
    def F(self):
        return int(self.faces.shape[0])

    @property
    def ptrs(self):
        return _p(self.faces), _p(self.vf_off), _p(self.vf_idx)


def mesh_normals(verts, topo):
    """scat_mesh_normals as it is declared: verts [B,V,3], topo a Topology -> normals [B,V,3]"""
    B, V = int(verts.shape[0]), int(verts.shape[1])
    normals = torch.empty((B, V, 3), dtype=torch.float32, device=verts.device)
    lib().bind(FIT_PLANE_HEADER).scat_mesh_normals(_p(verts), *topo.ptrs, _p(normals), B, V, topo.F, _stream())
    return normals


def mano_fit_verts_metric(model, targets, weights, normals, p, iters, w_tangent, lambda0, w_pose, w_beta, free=ALL_FREE):
    """scat_mano_fit_verts_metric as it is declared: targets [B,V,3], weights [B,V] or None, normals [B,V,3], p [B,62] read
    and written -> (cost [B], accepted [B] int32)"""
    B = targets.shape[0]
    cost, accepted = _results(B, targets.device)
    lib().bind(FIT_PLANE_HEADER).scat_mano_fit_verts_metric(*_model_args(model), _p(targets), _p(weights), _p(normals), _p(p), _p(cost),
                                                            _p(accepted), B, model.V, model.parents_packed, int(iters),
                                                            float(w_tangent), float(lambda0), float(w_pose), float(w_beta),
                                                            int(free), _stream())
    return cost, accepted


def mano_cloud_assign_plane(model, p, points, weights, topo, max_dist, w_tangent, want_model_pts=False):
    """scat_mano_cloud_assign_plane as it is declared: p [B,62], points [B,N,3], weights [B,N] or None, topo a Topology ->
    (Correspondences with the metric data cost, normals [B,V,3]), and with want_model_pts also model_pts [B,V,3]"""
    B, V, N = p.shape[0], model.V, points.shape[1]
    idx, dist, vw, vtarget, stats = _cloud_outputs(B, N, V, points.device)
    normals = torch.empty((B, V, 3), dtype=torch.float32, device=points.device)
    mp = torch.empty((B, V, 3), dtype=torch.float32, device=points.device) if want_model_pts else None
    lib().bind(FIT_PLANE_HEADER).scat_mano_cloud_assign_plane(*_model_args(model), _p(p), _p(points), _p(weights), *topo.ptrs,
                                                              float(max_dist), float(w_tangent), _p(mp), _p(normals), _p(idx), _p(dist),
                                                              _p(vw), _p(vtarget), _p(stats), B, N, V, topo.F, model.parents_packed,
                                                              _stream())
    c = _correspondences(idx, dist, vw, vtarget, stats)
    return (c, normals, mp) if want_model_pts else (c, normals)


def mano_fit_points_plane(model, points, weights, topo, p, rounds, iters, max_dist, w_tangent, lambda0, w_pose, w_beta,
                          free=ALL_FREE):
    """scat_mano_fit_points_plane as it is declared: mano_fit_points with a Topology and w_tangent -> (data_cost [B] in the
    plane metric, accepted [B] int32, idx [B,N] int32, dist [B,N], stats [B,4] fp64 of the last assignment).  The workspace
    is allocated here, at the size scat_mano_fit_points_plane_ws gives (0 for sizes the launch refuses)."""
    B, N = int(points.shape[0]), int(points.shape[1])
    ns = lib().bind(FIT_PLANE_HEADER)
    return _icp_launch(ns.scat_mano_fit_points_plane_ws, ns.scat_mano_fit_points_plane, model, points, weights, topo.ptrs, p, B,
                       (B, N, model.V, topo.F), (int(rounds), int(iters), float(max_dist), float(w_tangent), float(lambda0),
                                                 float(w_pose), float(w_beta), int(free)))


def mano_fit_kp(model, targets3, weights3, targets2, weights2, joint_map, pose_lo, pose_hi, p, iters, init, lambda0, w_pose,
                w_beta, w_limit, sigma3, sigma2, half_w, half_h, free=ALL_FREE, free_cam=7):
    """scat_mano_fit_kp as it is declared: targets3 [B,21,3] / weights3 [B,21], targets2 [B,21,2] / weights2 [B,21] (None
    leaves a term out, or means all ones), joint_map int32 [21] on the device, pose_lo / pose_hi [45] or None, p [B,65]
    (read when init = 0, written) -> (cost [B], accepted [B] int32)"""
    B = p.shape[0]
    cost, accepted = _results(B, p.device)
    lib().scat_mano_fit_kp(*_model_args(model), _p(targets3), _p(weights3), _p(targets2), _p(weights2), _p(joint_map), _p(pose_lo),
                           _p(pose_hi), _p(p), _p(cost), _p(accepted), B, model.V, model.parents_packed, *model.tips, int(iters),
                           int(init), float(lambda0), float(w_pose), float(w_beta), float(w_limit), float(sigma3), float(sigma2),
                           float(half_w), float(half_h), int(free), int(free_cam), _stream())
    return cost, accepted


def mano_fit_views(model, cams, targets2, weights2, joint_map, pose_lo, pose_hi, p, iters, init, lambda0, w_pose, w_beta, w_limit,
                   sigma2, z_near, free=ALL_FREE):
    """scat_mano_fit_views as it is declared: cams [Bc,C,16] with Bc 1 or B, targets2 [B,C,21,2], weights2 [B,C,21] or None
    (all ones), joint_map int32 [21] on the device, pose_lo / pose_hi [45] or None, p [B,62] (read when init = 0, written)
    -> (cost [B], accepted [B] int32)"""
    B, C = int(targets2.shape[0]), int(targets2.shape[1])
    cost, accepted = _results(B, targets2.device)
    lib().bind(FIT_VIEWS_HEADER).scat_mano_fit_views(*_model_args(model), _p(cams), int(cams.shape[0]), _p(targets2), _p(weights2),
                                                     _p(joint_map), _p(pose_lo), _p(pose_hi), _p(p), _p(cost), _p(accepted), B, C,
                                                     model.V, model.parents_packed, *model.tips, int(iters), int(init),
                                                     float(lambda0), float(w_pose), float(w_beta), float(w_limit), float(sigma2),
                                                     float(z_near), int(free), _stream())
    return cost, accepted


def mano_fit_seq_views(model, cams, targets2, weights2, joint_map, pose_lo, pose_hi, p, iters, init, lambda0, w_pose, w_beta,
                       w_limit, sigma2, z_near, smooth5, free=ALL_FREE):
    """scat_mano_fit_seq_views as it is declared: cams [Sc,C,16] with Sc 1 or S, targets2 [S,T,C,21,2], weights2 [S,T,C,21]
    or None (all ones), joint_map int32 [21] on the device, pose_lo / pose_hi [45] or None, p [S,T,62] (read when init = 0,
    written), smooth5 = (s_rots, s_poses, s_betas, s_trans, s_scale) -> (cost [S], accepted [S] int32).  The workspace is
    allocated here, at the size scat_mano_fit_seq_views_ws gives (0 for sizes the launch refuses)."""
    S, T, C = (int(n) for n in targets2.shape[:3])
    cost, accepted = _results(S, targets2.device)
    ns = lib().bind(FIT_SEQ_VIEWS_HEADER)
    ws, nbytes = _workspace(ns.scat_mano_fit_seq_views_ws, (S, T), targets2.device)
    ns.scat_mano_fit_seq_views(*_model_args(model), _p(cams), int(cams.shape[0]), _p(targets2), _p(weights2), _p(joint_map),
                               _p(pose_lo), _p(pose_hi), _p(p), _p(cost), _p(accepted), _p(ws), nbytes, S, T, C, model.V,
                               model.parents_packed, *model.tips, int(iters), int(init), float(lambda0), float(w_pose),
                               float(w_beta), float(w_limit), float(sigma2), float(z_near), *(float(v) for v in smooth5),
                               int(free), _stream())
    return cost, accepted


def triangulate_views(cams, targets2, weights2, z_near):
    """scat_triangulate as it is declared: cams [Bc,C,16] with Bc 1 or B, targets2 [B,C,21,2], weights2 [B,C,21] or None
    (all ones) -> (points [B,21,3], valid [B,21] int32)"""
    B, C = int(targets2.shape[0]), int(targets2.shape[1])
    points = torch.empty((B, 21, 3), dtype=torch.float32, device=targets2.device)
    valid = torch.empty((B, 21), dtype=torch.int32, device=targets2.device)
    lib().bind(FIT_VIEWS_HEADER).scat_triangulate(_p(cams), int(cams.shape[0]), _p(targets2), _p(weights2), _p(points), _p(valid), B, C,
                                                  float(z_near), _stream())
    return points, valid


def mano_fit_seq(model, targets, weights, joint_map, p, iters, init, lambda0, w_pose, w_beta, s_rots, s_poses, s_betas, s_trans,
                 s_scale, free=ALL_FREE):
    """scat_mano_fit_seq as it is declared: targets [S,T,21,3], weights [S,T,21] or None, joint_map int32 [21] on the
    device, p [S,T,62] (read when init = 0, written) -> (cost [S], accepted [S] int32).  The workspace is allocated here,
    at the size scat_mano_fit_seq_ws gives (0 for sizes the launch refuses)."""
    S, T = int(targets.shape[0]), int(targets.shape[1])
    cost, accepted = _results(S, targets.device)
    L = lib()
    ws, nbytes = _workspace(L.scat_mano_fit_seq_ws, (S, T), targets.device)
    L.scat_mano_fit_seq(*_model_args(model), _p(targets), _p(weights), _p(joint_map), _p(p), _p(cost), _p(accepted), _p(ws), nbytes, S,
                        T, model.V, model.parents_packed, *model.tips, int(iters), int(init), float(lambda0), float(w_pose),
                        float(w_beta), float(s_rots), float(s_poses), float(s_betas), float(s_trans), float(s_scale), int(free),
                        _stream())
    return cost, accepted


def mano_fit_seq_verts(model, targets, weights, normals, p, iters, init, w_tangent, lambda0, w_pose, w_beta, smooth5,
                       free=ALL_FREE):
    """scat_mano_fit_seq_verts as it is declared: targets [S,T,V,3], weights [S,T,V] or None, normals [S,T,V,3] or None
    (which selects the plane metric with w_tangent), p [S,T,62] (read when init = 0, written), smooth5 = (s_rots, s_poses,
    s_betas, s_trans, s_scale) -> (cost [S], accepted [S] int32).  The workspace is allocated here, at the size
    scat_mano_fit_seq_verts_ws gives (0 for sizes the launch refuses)."""
    S, T = int(targets.shape[0]), int(targets.shape[1])
    cost, accepted = _results(S, targets.device)
    ns = lib().bind(FIT_SEQ_VERTS_HEADER)
    ws, nbytes = _workspace(ns.scat_mano_fit_seq_verts_ws, (S, T, model.V), targets.device)
    ns.scat_mano_fit_seq_verts(*_model_args(model), _p(targets), _p(weights), _p(normals), _p(p), _p(cost), _p(accepted), _p(ws),
                               nbytes, S, T, model.V, model.parents_packed, int(iters), int(init), float(w_tangent), float(lambda0),
                               float(w_pose), float(w_beta), *(float(v) for v in smooth5), int(free), _stream())
    return cost, accepted


def mano_fit_points_seq(model, points, weights, topo, p, rounds, iters, max_dist, w_tangent, lambda0, w_pose, w_beta, smooth5,
                        free=ALL_FREE):
    """scat_mano_fit_points_seq as it is declared: points [S,T,N,3], weights [S,T,N] or None, topo a Topology or None
    (nearest vertex), p [S,T,62] read and written -> (data_cost [S,T], accepted [S] int32, idx [S,T,N] int32, dist [S,T,N],
    stats [S,T,4] fp64 of the last assignment).  The workspace is allocated here, at the size scat_mano_fit_points_seq_ws
    gives (0 for sizes the launch refuses)."""
    S, T, N = (int(n) for n in points.shape[:3])
    ns = lib().bind(FIT_SEQ_VERTS_HEADER)
    return _icp_launch(ns.scat_mano_fit_points_seq_ws, ns.scat_mano_fit_points_seq, model, points, weights,
                       (0, 0, 0) if topo is None else topo.ptrs, p, S, (S, T, N, model.V, 0 if topo is None else topo.F),
                       (int(rounds), int(iters), float(max_dist), float(w_tangent), float(lambda0), float(w_pose), float(w_beta),
                        *(float(v) for v in smooth5), int(free)))


def mano_fit_seq_kp(model, targets3, weights3, targets2, weights2, joint_map, pose_lo, pose_hi, p, iters, init, lambda0, w_pose,
                    w_beta, w_limit, sigma3, sigma2, half_w, half_h, smooth7, free=ALL_FREE, free_cam=7):
    """scat_mano_fit_seq_kp as it is declared: targets3 [S,T,21,3] / weights3 [S,T,21], targets2 [S,T,21,2] / weights2
    [S,T,21] (None leaves a term out, or means all ones), joint_map int32 [21] on the device, pose_lo / pose_hi [45] or
    None, p [S,T,65] (read when init = 0, written), smooth7 = (s_rots, s_poses, s_betas, s_trans, s_scale, s_cs, s_ct)
    -> (cost [S], accepted [S] int32).  The workspace is allocated here, at the size scat_mano_fit_seq_kp_ws gives (0 for
    sizes the launch refuses)."""
    S, T = int(p.shape[0]), int(p.shape[1])
    cost, accepted = _results(S, p.device)
    ns = lib().bind(FIT_SEQ_KP_HEADER)
    ws, nbytes = _workspace(ns.scat_mano_fit_seq_kp_ws, (S, T), p.device)
    ns.scat_mano_fit_seq_kp(*_model_args(model), _p(targets3), _p(weights3), _p(targets2), _p(weights2), _p(joint_map), _p(pose_lo),
                            _p(pose_hi), _p(p), _p(cost), _p(accepted), _p(ws), nbytes, S, T, model.V, model.parents_packed,
                            *model.tips, int(iters), int(init), float(lambda0), float(w_pose), float(w_beta), float(w_limit),
                            float(sigma3), float(sigma2), float(half_w), float(half_h), *(float(v) for v in smooth7), int(free),
                            int(free_cam), _stream())
    return cost, accepted


def _icp_front(what, lead, init, w_tangent, rounds, iters, free, max_dist):
    """What every ICP method checks before it looks at a tensor: the start is required (lead: what the error calls it),
    w_tangent in [0, 1], iters and free in range, rounds in 1..POINTS_MAX_ROUNDS with at most POINTS_MAX_STEPS steps,
    max_dist positive or None -> tau, rounds, iters, max_dist as the numbers the launch takes"""
    if init is None:
        raise ScatError(f"{what} needs a start: {lead}")
    tau = float(w_tangent)
    if not 0.0 <= tau <= 1.0:
        raise ScatError(f"{what}: w_tangent {w_tangent} outside 0..1")
    rounds, iters = int(rounds), int(iters)
    _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE)
    if not 1 <= rounds <= POINTS_MAX_ROUNDS or rounds * iters > POINTS_MAX_STEPS:
        raise ScatError(f"{what}: {rounds} rounds of {iters} iterations: rounds outside 1..{POINTS_MAX_ROUNDS} or more than "
                        f"{POINTS_MAX_STEPS} steps")
    return tau, rounds, iters, _max_dist(what, max_dist)


def _icp_back(result_type, p, cost, accepted, idx, dist, stats):
    """the result of an ICP method from what its launch returned: matched and rms from the last assignment's stats"""
    mw = stats[..., 1]
    rms = torch.where(mw > 0, (stats[..., 3] / mw).sqrt(), torch.full_like(mw, float("inf"))).float()
    return result_type(*_groups(p), cost, accepted, p, stats[..., 2].long(), rms, idx, dist)


class ManoFitter:
    """Fits rots, poses, betas, a translation and a scale to 21 joints.  model: a ManoModel already moved to the device.
    joint_map: a permutation of 0..20, target joint j is the model's joint joint_map[j] (None: the model's own order).
    w_pose, w_beta: the priors' weights; for targets in metres they are of the 1e-6 order, larger ones pull a 0.1 m hand
    millimetres off its targets.  lambda0: the first damping."""

    def __init__(self, model: ManoModel, joint_map=None, w_pose=1e-6, w_beta=1e-6, iters=20, lambda0=1e-3):
        jm = list(range(21)) if joint_map is None else [int(j) for j in joint_map]
        if sorted(jm) != list(range(21)):
            raise ScatError("ManoFitter: joint_map must be a permutation of 0..20")
        if not 1 <= int(iters) <= MAX_ITERS:
            raise ScatError(f"ManoFitter: {iters} iterations outside 1..{MAX_ITERS}")
        if w_pose < 0 or w_beta < 0 or not lambda0 > 0:
            raise ScatError("ManoFitter: the priors' weights must not be negative and lambda0 must be positive")
        self.model, self.joint_map = model, tuple(jm)
        self.joint_map_d = None      # uploaded by the first fit
        self.w_pose, self.w_beta, self.iters, self.lambda0 = float(w_pose), float(w_beta), int(iters), float(lambda0)

    def fit(self, joints, weights=None, init=None, free=ALL_FREE, iters=None):
        """joints [B,21,3] fp32 -> FitResult.  weights: [B,21] or None (all ones).  init: None for the Procrustes start, or
        p [B,62] / a FitResult to start from (it is not modified).  free: bit i clear freezes unknown i (free_mask()).
        A sample whose targets or weights are not finite, or that has a negative weight, is not fitted: its cost is +inf,
        its accepted count 0 and its p the start (zeros for the Procrustes start)."""
        _need_gpu("ManoFitter.fit", joints, *(() if weights is None else (weights,)))
        _check_model("ManoFitter.fit", self.model, joints)
        B = joints.shape[0]
        if B == 0 or tuple(joints.shape) != (B, 21, 3) or joints.dtype != torch.float32:
            raise ScatError(f"ManoFitter.fit needs fp32 joints [B,21,3] with B >= 1, got {joints.dtype} {tuple(joints.shape)}")
        weights = _weights("ManoFitter.fit", weights, (B, 21))
        p = _start("ManoFitter.fit", init, (FitResult, PointFitResult), (B, UNKNOWNS), joints.device)
        iters = self.iters if iters is None else int(iters)
        _check_ranges("ManoFitter.fit", iters, 0 <= int(free) <= ALL_FREE)
        cost, accepted = mano_fit(self.model, joints.contiguous(), weights, self._map_on(joints.device), p, iters,
                                  0 if init is not None else 1, self.lambda0, self.w_pose, self.w_beta, free)
        return FitResult(*_groups(p), cost, accepted, p)

    def _map_on(self, device):
        if self.joint_map_d is None or self.joint_map_d.device != device:
            self.joint_map_d = torch.tensor(self.joint_map, dtype=torch.int32, device=device)
        return self.joint_map_d

    def fit_outputs(self, out66, weights=None):
        """out66 [B,66]: the network's camera and 21 root-relative joints; the joints are fitted, the camera is the
        caller's to pass on to the renderer"""
        _need_gpu("ManoFitter.fit_outputs", out66)
        if out66.dim() != 2 or out66.shape[1] != 66:
            raise ScatError(f"fit_outputs needs the network's output [B,66], got {tuple(out66.shape)}")
        return self.fit(out66.detach()[:, 3:].reshape(-1, 21, 3).contiguous(), weights)

    def fit_vertices(self, verts, weights=None, init=None, free=ALL_FREE, iters=None):
        """verts [B,V,3] fp32, a mesh in the model's topology (vertex v is the model's vertex v; joint_map plays no part)
        -> FitResult.  weights: [B,V] or None (all ones); a vertex of weight 0 does not count.  init: None for the
        Procrustes start over the vertices, or p [B,62] / any FitResult to start from (it is not modified): a joints fit
        of the same hand is the natural warm start.  free: bit i clear freezes unknown i (free_mask()).  A hand whose
        vertices or weights are not finite, or that has a negative weight, is not fitted: its cost is +inf, its accepted
        count 0 and its p the start (zeros for the Procrustes start)."""
        what = "ManoFitter.fit_vertices"
        _need_gpu(what, verts, *(() if weights is None else (weights,)))
        _check_model(what, self.model, verts)
        B, V = verts.shape[0], self.model.V
        if B == 0 or tuple(verts.shape) != (B, V, 3) or verts.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 verts [B,{V},3] with B >= 1, got {verts.dtype} {tuple(verts.shape)}")
        weights = _weights(what, weights, (B, V))
        p = _start(what, init, (FitResult, PointFitResult), (B, UNKNOWNS), verts.device)
        iters = self.iters if iters is None else int(iters)
        _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE)
        cost, accepted = mano_fit_verts(self.model, verts.contiguous(), weights, p, iters, 0 if init is not None else 1,
                                        self.lambda0, self.w_pose, self.w_beta, free)
        return FitResult(*_groups(p), cost, accepted, p)

    def _cloud(self, what, points, weights):
        """the checked points [B,N,3] and weights [B,N] or None of fit_points and nearest_vertices, contiguous"""
        _need_gpu(what, points, *(() if weights is None else (weights,)))
        _check_model(what, self.model, points)
        if points.dim() != 3 or points.shape[0] == 0 or not 1 <= points.shape[1] <= POINTS_MAX_N or points.shape[2] != 3 \
                or points.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 points [B,N,3] with B >= 1 and N in 1..{POINTS_MAX_N}, got {points.dtype} "
                            f"{tuple(points.shape)}")
        return points.contiguous(), _weights(what, weights, tuple(points.shape[:2]))

    def fit_points(self, points, init, weights=None, rounds=5, iters=4, max_dist=None, free=ALL_FREE):
        """points [B,N,3] fp32, an unordered cloud with N <= 8192 -> PointFitResult.  Nearest-vertex ICP: `rounds` times
        {every point to its nearest model vertex; `iters` Levenberg-Marquardt iterations of fit_vertices on the
        per-vertex centroids}, then one more assignment that the result's idx, dist, matched, data_cost and rms describe.
        init: the start, required, p [B,62] or any fit result (it is not modified; of a KeypointFitResult the first 62):
        ICP is local and finds the hand only from nearby, a joints fit of the same hand is the natural start.
        weights: [B,N] or None (all ones); a point of weight 0 does not count.  max_dist: points farther than this from
        the model do not count in a round (a hard trim, in the points' unit); None keeps all.  free: bit i clear freezes
        unknown i.  rounds in 1..64, rounds x iters <= 256.  A hand with a point, weight or start that is not finite, or
        a negative weight, is not fitted: data_cost +inf, accepted 0, p the start; a hand with nothing matched keeps its
        p too."""
        what = "ManoFitter.fit_points"
        _, rounds, iters, max_dist = _icp_front(what, "p [B,62] or a fit result", init, 1.0, rounds, iters, free, max_dist)
        points, weights = self._cloud(what, points, weights)
        B = points.shape[0]
        if isinstance(init, KeypointFitResult):
            init = init.p[:, :UNKNOWNS]
        p = _start(what, init, (FitResult, PointFitResult), (B, UNKNOWNS), points.device)
        return _icp_back(PointFitResult, p, *mano_fit_points(self.model, points, weights, p, rounds, iters, max_dist, self.lambda0,
                                                            self.w_pose, self.w_beta, free))

    def nearest_vertices(self, result_or_verts, points, weights=None, max_dist=None):
        """-> Correspondences of the cloud points [B,N,3] with the model at a fit result or p [B,62] (the vertices are
        posed inside the launch) or with the caller's vertices [B,V,3] (any V <= 1536): per point the nearest vertex and its distance,
        per vertex the weight and centroid of its matched points, which are fit_vertices' weights and targets."""
        what = "ManoFitter.nearest_vertices"
        points, weights = self._cloud(what, points, weights)
        B, d = points.shape[0], _max_dist(what, max_dist)
        if isinstance(result_or_verts, torch.Tensor) and result_or_verts.dim() != 2:
            verts = result_or_verts
            _need_gpu(what, verts)
            if verts.dim() != 3 or verts.shape[0] != B or not 1 <= verts.shape[1] <= MAX_V or verts.shape[2] != 3 \
                    or verts.dtype != torch.float32 or verts.device != points.device:
                raise ScatError(f"{what} needs fp32 verts [{B},V,3] with V in 1..{MAX_V} on {points.device}, got "
                                f"{verts.dtype} {tuple(verts.shape)} on {verts.device}")
            return cloud_assign(verts.contiguous(), points, weights, d)
        r = result_or_verts
        p = r.p[:, :UNKNOWNS] if isinstance(r, KeypointFitResult) else r if isinstance(r, torch.Tensor) else getattr(r, "p", None)
        if not isinstance(p, torch.Tensor) or tuple(p.shape) != (B, UNKNOWNS) or p.dtype != torch.float32:
            raise ScatError(f"{what} needs a fit result or fp32 p [{B},{UNKNOWNS}], or fp32 verts [{B},V,3]")
        _need_gpu(what, p)
        return mano_cloud_assign(self.model, p.contiguous(), points, weights, d)

    def _topology(self, what, faces, device):
        """the Topology on `device` of faces: a MeshRenderer of the model's V (its uploaded arrays), or a [F,3] integer
        array or tensor (the table from render.vertex_face_csr, uploaded once per object and cached by it)"""
        from .render import MeshRenderer

        if isinstance(faces, MeshRenderer):
            self._host_topology(what, faces)
            if faces.device != device:
                faces.to(device)
            return Topology(faces.faces_d, faces.vf_off_d, faces.vf_idx_d)
        entry = self._host_topology(what, faces)
        if str(device) not in entry[2]:
            entry[2][str(device)] = Topology(*(torch.from_numpy(a).to(device) for a in entry[1]))
        return entry[2][str(device)]

    def _host_topology(self, what, faces):
        """the host half of _topology, before any tensor is looked at: the checks, and for an array the CSR table, cached
        by the object -> [faces, (f, vf_off, vf_idx) int32, {device: Topology}]; None for a MeshRenderer, which has its own"""
        from .render import MeshRenderer, _int_array, vertex_face_csr

        V = self.model.V
        if isinstance(faces, MeshRenderer):
            if faces.V != V:
                raise ScatError(f"{what}: the renderer has {faces.V} vertices, the model {V}")
            return None
        cache = self.__dict__.setdefault("_topologies", {})
        hit = cache.get(id(faces))
        if hit is not None and hit[0] is faces:
            return hit
        try:
            f = _int_array(f"{what}: faces", faces, (3,))
        except ValueError as e:
            raise ScatError(str(e)) from None
        if not 1 <= f.shape[0] <= MAX_F:
            raise ScatError(f"{what}: {f.shape[0]} faces outside 1..{MAX_F}")
        if f.min() < 0 or f.max() >= V:
            raise ScatError(f"{what}: face indices {f.min()}..{f.max()} outside 0..{V - 1}")
        off, idx = vertex_face_csr(f, V)
        if len(cache) >= 8:      # a caller that makes a new array per call is not to grow the fitter
            cache.pop(next(iter(cache)))
        # the object is kept, so its id stays its own
        cache[id(faces)] = [faces, tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (f, off, idx)), {}]
        return cache[id(faces)]

    def fit_points_plane(self, points, init, faces, weights=None, rounds=10, iters=4, max_dist=None, w_tangent=0.01, free=ALL_FREE):
        """points [B,N,3] fp32, a cloud of points ON THE SURFACE (a depth camera's, a scanner's) with N <= 8192 ->
        PointFitResult.  Point-to-plane ICP: fit_points' loop, where the residual of a point counts fully along the normal
        of the model vertex it is matched to and with the weight w_tangent across it, so that points between the model's
        vertices can slide on the surface instead of pulling the vertices under them.  faces: the model's topology, a
        [F,3] integer array or tensor (F <= 4096, indices below V; uploaded once per object and cached by it: do not
        modify it in place) or a MeshRenderer of the model's V.  w_tangent in [0, 1]: 1 is fit_points' cost, 0 the pure
        point-to-plane cost, which leaves a sparse cloud's system rank-deficient; the default suits a dense cloud.
        The result's data_cost and rms are IN THE PLANE METRIC, sum w (w_tangent |r|^2 + (1 - w_tangent) (n . r)^2) over the
        matched points and sqrt(data_cost / matched weight): not comparable with fit_points' figures.  idx and dist are
        Euclidean, to the nearest vertex.  init, weights, rounds, iters, max_dist, free, the limits and what makes a hand
        unusable are fit_points'.  On a cloud that IS the model's vertices fit_points is the better method."""
        what = "ManoFitter.fit_points_plane"
        tau, rounds, iters, max_dist = _icp_front(what, "p [B,62] or a fit result", init, w_tangent, rounds, iters, free, max_dist)
        self._host_topology(what, faces)
        points, weights = self._cloud(what, points, weights)
        B = points.shape[0]
        topo = self._topology(what, faces, points.device)
        if isinstance(init, KeypointFitResult):
            init = init.p[:, :UNKNOWNS]
        p = _start(what, init, (FitResult, PointFitResult), (B, UNKNOWNS), points.device)
        return _icp_back(PointFitResult, p, *mano_fit_points_plane(self.model, points, weights, topo, p, rounds, iters, max_dist, tau,
                                                                  self.lambda0, self.w_pose, self.w_beta, free))

    def vertex_normals(self, result_or_verts, faces):
        """-> [B,V,3] fp32, the area-weighted unit vertex normals of the fitted mesh of a result (mesh(result)) or of the
        caller's vertices [B,V,3], for the topology `faces` (as in fit_points_plane): fp64 sums rounded to fp32 once, a
        zero vector for a vertex in no face or of zero area"""
        what = "ManoFitter.vertex_normals"
        self._host_topology(what, faces)
        verts =result_or_verts if isinstance(result_or_verts, torch.Tensor) and result_or_verts.dim() == 3 else None
        if verts is None:
            if not hasattr(result_or_verts, "p") or result_or_verts.p.dim() != 2:
                raise ScatError(f"{what} needs a fit result of a batch or fp32 verts [B,{self.model.V},3]")
            verts = self.mesh(result_or_verts)
        _need_gpu(what, verts)
        if verts.shape[0] == 0 or tuple(verts.shape[1:]) != (self.model.V, 3) or verts.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 verts [B,{self.model.V},3] with B >= 1, got {verts.dtype} {tuple(verts.shape)}")
        return mesh_normals(verts.contiguous(), self._topology(what, faces, verts.device))

    def fit_mesh_outputs(self, out, weights=None):
        """out [B,21+V,3]: joints and mesh in the layout of ManoLayer / scat_mano_fwd; the V vertex rows are fitted"""
        _need_gpu("ManoFitter.fit_mesh_outputs", out)
        if out.dim() != 3 or tuple(out.shape[1:]) != (21 + self.model.V, 3):
            raise ScatError(f"fit_mesh_outputs needs the layer's output [B,{21 + self.model.V},3], got {tuple(out.shape)}")
        return self.fit_vertices(out.detach()[:, 21:].contiguous(), weights)

    def fit_sequence(self, joints, weights=None, smooth=None, init=None, free=ALL_FREE, iters=None):
        """joints [S,T,21,3] fp32, S sequences of T <= 256 frames -> SequenceFitResult.  The frames of a sequence are fitted
        in one Levenberg-Marquardt solve, with the penalty sum_i d_i (p_t,i - p_t-1,i)^2 between consecutive frames.
        smooth: dict(rots=, poses=, betas=, trans=, scale=), the weight d of each group; a key left out is 0, and all
        zero decouples the frames.  UNITS: the data term is in the joints' unit squared, and each weight multiplies a
        squared difference in the unknown's own unit: radians squared for rots and poses (the penalty is on the
        axis-angle numbers, not on the rotations), the shape coefficients' for betas, the joints' unit for trans, a
        log-ratio for scale.  With joints in metres, rots = 1e-4 counts 0.1 rad per frame like a 1 mm residual.
        weights: [S,T,21] or None (all ones).  A frame whose weights are all zero is legal whatever its finite joints:
        it has no data term and is bridged by its neighbours; this is also how a short clip is padded to T frames.
        init: None for the frame-by-frame Procrustes start (continuous in rots; a zero-weight frame takes its
        neighbour's), or p [S,T,62] / a SequenceFitResult (it is not modified).  free: bit i clear freezes unknown i in
        every frame.  A sequence with a joint or weight that is not finite, or a negative weight, in any frame is not
        fitted: cost +inf, accepted 0, p its start (zeros for the Procrustes start)."""
        what = "ManoFitter.fit_sequence"
        sm = _smooth(what, smooth)
        _need_gpu(what, joints, *(() if weights is None else (weights,)))
        _check_model(what, self.model, joints)
        if joints.dim() != 4 or joints.shape[0] == 0 or not 1 <= joints.shape[1] <= SEQ_MAX_T or tuple(joints.shape[2:]) != (21, 3) \
                or joints.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 joints [S,T,21,3] with S >= 1 and T in 1..{SEQ_MAX_T}, got {joints.dtype} "
                            f"{tuple(joints.shape)}")
        S, T = int(joints.shape[0]), int(joints.shape[1])
        weights = _weights(what, weights, (S, T, 21))
        p = _start(what, init, (SequenceFitResult, PointSequenceFitResult), (S, T, UNKNOWNS), joints.device)
        iters = self.iters if iters is None else int(iters)
        _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE)
        cost, accepted = mano_fit_seq(self.model, joints.contiguous(), weights, self._map_on(joints.device), p, iters,
                                      0 if init is not None else 1, self.lambda0, self.w_pose, self.w_beta, *sm, free)
        return SequenceFitResult(*_groups(p), cost, accepted, p)

    def _start_sequence(self, what, init, S, T, device):
        """the p [S,T,62] of a mesh or cloud track: of a KeypointSequenceFitResult the first 62"""
        if isinstance(init, KeypointSequenceFitResult):
            init = init.p[..., :UNKNOWNS]
        return _start(what, init, (SequenceFitResult, PointSequenceFitResult), (S, T, UNKNOWNS), device)

    def fit_vertices_sequence(self, verts, weights=None, smooth=None, init=None, free=ALL_FREE, iters=None):
        """verts [S,T,V,3] fp32, S tracks of T <= 256 meshes in the model's topology -> SequenceFitResult.  fit_vertices'
        data term in every frame and fit_sequence's penalty sum_i d_i (p_t,i - p_t-1,i)^2 between consecutive frames, one
        Levenberg-Marquardt per track: one lambda, one accept / reject.  The frames are assembled side by side, one
        workgroup each, and only the elimination along the track runs one workgroup per sequence: 2 iters + 2 launches
        (two more for the Procrustes start), no synchronisation with the host.
        smooth: dict(rots=, poses=, betas=, trans=, scale=) as in fit_sequence.  UNITS: each weight multiplies a squared
        difference in the unknown's own unit (radians squared for rots and poses, on the axis-angle numbers), and the data
        term it is weighed against is in the vertices' unit squared SUMMED OVER V VERTICES: V / 21 times a joints track's
        at the same residual, so weights that suit fit_sequence are about V / 21 times too small here.
        weights: [S,T,V] or None (all ones).  A frame whose weights are all zero is legal whatever its finite vertices:
        it has no data term and is bridged by its neighbours; this is also how a short clip is padded to T frames.
        init: None for the Procrustes start over the vertices frame by frame (continuous in rots; a zero-weight frame takes
        its neighbour's), or p [S,T,62] / a SequenceFitResult, KeypointSequenceFitResult (its first 62) or
        PointSequenceFitResult (it is not modified): a joints track of the same hands is the natural warm start.
        free: bit i clear freezes unknown i in every frame.  A sequence with a vertex or weight that is not finite, a
        negative weight or a start that is not finite, in any frame, is not fitted: cost +inf, accepted 0, p its start
        (zeros for the Procrustes start)."""
        what = "ManoFitter.fit_vertices_sequence"
        sm = _smooth(what, smooth)
        _need_gpu(what, verts, *(() if weights is None else (weights,)))
        _check_model(what, self.model, verts)
        V = self.model.V
        if verts.dim() != 4 or verts.shape[0] == 0 or not 1 <= verts.shape[1] <= SEQ_MAX_T or tuple(verts.shape[2:]) != (V, 3) \
                or verts.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 verts [S,T,{V},3] with S >= 1 and T in 1..{SEQ_MAX_T}, got {verts.dtype} "
                            f"{tuple(verts.shape)}")
        S, T = int(verts.shape[0]), int(verts.shape[1])
        weights = _weights(what, weights, (S, T, V))
        p = self._start_sequence(what, init, S, T, verts.device)
        iters = self.iters if iters is None else int(iters)
        _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE)
        cost, accepted = mano_fit_seq_verts(self.model, verts.contiguous(), weights, None, p, iters, 0 if init is not None else 1,
                                            1.0, self.lambda0, self.w_pose, self.w_beta, sm, free)
        return SequenceFitResult(*_groups(p), cost, accepted, p)

    def fit_points_sequence(self, points, init, faces=None, weights=None, smooth=None, rounds=None, iters=4, max_dist=None,
                            w_tangent=0.01, free=ALL_FREE):
        """points [S,T,N,3] fp32, S tracks of T <= 256 unordered clouds with N <= 8192 (a depth camera's clip) ->
        PointSequenceFitResult.  ICP over the track: `rounds` times {every point of every frame to its nearest model
        vertex, one launch over the S T frames; `iters` iterations of fit_vertices_sequence's solve on the per-vertex
        centroids}, then one more assignment that the result's idx, dist, matched, data_cost and rms describe.
        faces: the model's topology (an array or a MeshRenderer, as in fit_points_plane) selects point-to-plane ICP with
        w_tangent, for points ON THE SURFACE; None is nearest-vertex ICP (fit_points).  rounds: None is 10 with faces
        and 5 without.  init: the start, required, p [S,T,62] or a sequence result (it is not modified): a joints track
        is the natural start.  smooth: as in fit_vertices_sequence; the data term is summed over the matched points.
        A frame in which nothing is matched (an occluded hand: every point beyond max_dist or of weight 0) is BRIDGED by
        its neighbours, as a zero-weight frame is; its matched is 0 and its rms +inf.  A sequence with a point, weight or
        start that is not finite, or a negative weight, in any frame is not fitted: p its start, accepted 0, and
        data_cost +inf in the frames concerned.  The other sequences are not affected.
        weights, max_dist, free and the limits (rounds in 1..64, rounds x iters <= 256) are fit_points'."""
        what = "ManoFitter.fit_points_sequence"
        tau, rounds, iters, max_dist = _icp_front(what, "p [S,T,62] or a sequence fit result", init, w_tangent,
                                                  (10 if faces is not None else 5) if rounds is None else rounds, iters, free, max_dist)
        sm = _smooth(what, smooth)
        if faces is not None:
            self._host_topology(what, faces)
        _need_gpu(what, points, *(() if weights is None else (weights,)))
        _check_model(what, self.model, points)
        if points.dim() != 4 or points.shape[0] == 0 or not 1 <= points.shape[1] <= SEQ_MAX_T \
                or not 1 <= points.shape[2] <= POINTS_MAX_N or points.shape[3] != 3 or points.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 points [S,T,N,3] with S >= 1, T in 1..{SEQ_MAX_T} and N in 1..{POINTS_MAX_N}, "
                            f"got {points.dtype} {tuple(points.shape)}")
        S, T = int(points.shape[0]), int(points.shape[1])
        weights = _weights(what, weights, tuple(points.shape[:3]))
        topo = None if faces is None else self._topology(what, faces, points.device)
        p = self._start_sequence(what, init, S, T, points.device)
        return _icp_back(PointSequenceFitResult, p, *mano_fit_points_seq(self.model, points.contiguous(), weights, topo, p, rounds,
                                                                        iters, max_dist, tau, self.lambda0, self.w_pose,
                                                                        self.w_beta, sm, free))

    def fit_outputs_sequence(self, out66, weights=None, smooth=None):
        """out66 [S,T,66]: the network's camera and 21 root-relative joints for every frame of S tracks; the joints are
        fitted as sequences (fit_sequence), the cameras are the caller's to pass on to the renderer"""
        _need_gpu("ManoFitter.fit_outputs_sequence", out66)
        if out66.dim() != 3 or out66.shape[2] != 66:
            raise ScatError(f"fit_outputs_sequence needs the network's outputs [S,T,66], got {tuple(out66.shape)}")
        S, T = out66.shape[:2]
        return self.fit_sequence(out66.detach()[:, :, 3:].reshape(S, T, 21, 3).contiguous(), weights, smooth)

    def fit_keypoints(self, joints3d=None, joints2d=None, w3=None, w2=None, size=(224, 224), sigma3=0.0, sigma2=0.0, limits=None,
                      w_limit=0.0, init=None, free=None, free_cam=7, iters=None):
        """joints3d [B,21,3] and / or joints2d [B,21,2] (pixels of a frame of size = (H, W)) -> KeypointFitResult.
        w3, w2: [B,21] or None (all ones).  UNITS: the 3-D term is in the joints' unit squared and the 2-D term in pixels
        squared, and w2 balances them: with joints in metres, w2 = 1e-6 makes a pixel count like a millimetre.
        sigma3, sigma2: the Geman-McClure scales in the joints' unit and in pixels, 0 for the quadratic loss.
        limits: (lo[45], hi[45]) on poses with the weight w_limit; an entry that is not finite is no limit.
        init: None for the closed-form start, or p [B,65] / a KeypointFitResult (it is not modified).
        free: bit i clear freezes unknown i < 62; None frees everything, or everything but trans and log_scale when
        joints3d is None (they are a gauge of the camera then).  free_cam: bits 0, 1, 2 free cs, ctx, cty; without
        joints2d the camera has no rows and stays frozen.  A sample with a target or weight that is not finite, or a
        negative weight, is not fitted: cost +inf, accepted 0, p its start."""
        p, args, frees = self._keypoint_args("ManoFitter.fit_keypoints", "B", (KeypointFitResult, PointFitResult), joints3d,
                                             joints2d, w3, w2, size, sigma3, sigma2, limits, w_limit, init, free, free_cam, iters)
        cost, accepted = mano_fit_kp(*args, *frees)
        return KeypointFitResult(*_groups(p), p[:, 62:65], cost, accepted, p)

    def _keypoint_args(self, what, lead, result_types, joints3d, joints2d, w3, w2, size, sigma3, sigma2, limits, w_limit, init,
                       free, free_cam, iters):
        """The checks that fit_keypoints (lead "B": [B,21,.]) and fit_keypoints_sequence (lead "S,T": [S,T,21,.], T <= 256)
        share -> (p, the arguments of mano_fit_kp / mano_fit_seq_kp from the model up to half_h, (free, free_cam))"""
        if joints3d is None and joints2d is None:
            raise ScatError(f"{what} needs joints3d, joints2d or both")
        _need_gpu(what, *(t for t in (joints3d, joints2d, w3, w2) if t is not None))
        ref = joints3d if joints3d is not None else joints2d
        _check_model(what, self.model, ref)
        n = 1 + lead.count(",")
        if ref.dim() != n + 2 or 0 in ref.shape[:n] or (n == 2 and ref.shape[1] > SEQ_MAX_T):
            raise ScatError(f"{what} needs fp32 joints3d [{lead},21,3] and / or joints2d [{lead},21,2] with "
                            f"{'B >= 1' if n == 1 else f'S >= 1 and T in 1..{SEQ_MAX_T}'}, got {tuple(ref.shape)}")
        dims = tuple(int(d) for d in ref.shape[:n])
        for name, t, shape in (("joints3d", joints3d, (*dims, 21, 3)), ("joints2d", joints2d, (*dims, 21, 2)),
                               ("w3", w3, (*dims, 21)), ("w2", w2, (*dims, 21))):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != ref.device):
                raise ScatError(f"{what} needs fp32 {name} {list(shape)} on {ref.device}, got {t.dtype} {tuple(t.shape)} on "
                                f"{t.device}")
        if (w3 is not None and joints3d is None) or (w2 is not None and joints2d is None):
            raise ScatError(f"{what}: weights given without their joints")
        lo = hi = None
        if limits is not None:
            lo, hi = (torch.as_tensor(t, dtype=torch.float32).to(ref.device).contiguous() for t in limits)
            if tuple(lo.shape) != (POSE,) or tuple(hi.shape) != (POSE,):
                raise ScatError(f"{what} needs limits (lo[45], hi[45]), got {tuple(lo.shape)}, {tuple(hi.shape)}")
        H, W = (float(v) for v in size)
        if not (H > 0 and W > 0):
            raise ScatError(f"{what}: size {size} must be positive")
        p = _start(what, init, result_types, (*dims, KP_UNKNOWNS), ref.device)
        iters = self.iters if iters is None else int(iters)
        if free is None:
            free = ALL_FREE if joints3d is not None else free_mask(trans=False, log_scale=False)
        _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE and 0 <= int(free_cam) <= 7, ", or free_cam is outside 0..7")
        if min(float(sigma3), float(sigma2), float(w_limit)) < 0:
            raise ScatError(f"{what}: sigma3, sigma2 and w_limit must not be negative")
        c = lambda t: None if t is None else t.contiguous()
        return p, (self.model, c(joints3d), c(w3), c(joints2d), c(w2), self._map_on(ref.device), lo, hi, p, iters,
                   0 if init is not None else 1, self.lambda0, self.w_pose, self.w_beta, w_limit, sigma3, sigma2, 0.5 * W,
                   0.5 * H), (free, int(free_cam) if joints2d is not None else 0)

    def fit_keypoints_sequence(self, joints3d=None, joints2d=None, w3=None, w2=None, size=(224, 224), sigma3=0.0, sigma2=0.0,
                               limits=None, w_limit=0.0, smooth=None, init=None, free=None, free_cam=7, iters=None):
        """joints3d [S,T,21,3] and / or joints2d [S,T,21,2] (pixels of a frame of size = (H, W)), S tracks of T <= 256
        frames -> KeypointSequenceFitResult.  fit_keypoints' problem in every frame (w3, w2 [S,T,21] or None; sigma3, sigma2,
        limits, w_limit, size, free, free_cam as there, the same for every frame) and fit_sequence's coupling between
        consecutive frames, solved as one Levenberg-Marquardt per track: one lambda, one accept / reject.
        smooth: dict(rots=, poses=, betas=, trans=, scale=, cam_scale=, cam_trans=), the weight d of each group in
        sum_i d_i (p_t,i - p_t-1,i)^2; a key left out is 0.  UNITS: as in fit_sequence each weight multiplies a squared
        difference in the unknown's own unit: radians squared for rots and poses (the penalty is on the axis-angle numbers),
        the joints' unit for trans, a log-ratio for scale; cam_scale is on the camera's s, a pure number, and cam_trans on
        tx, ty, in the joints' unit.  The data term they are weighed against is in the joints' unit squared where joints3d is
        given (w2 = 1e-6 makes a pixel count like a millimetre) and in pixels squared from joints2d alone, where weights
        about (cs W / 2)^2 times larger do the same.  A constant shape over the track is a large betas; there is no hard constraint.
        A frame whose weights are all zero (w2 and w3) is legal whatever its finite keypoints: it has no data term and is
        bridged by its neighbours, which is how an occluded hand and a padded clip are passed.
        init: None for fit_keypoints' closed-form start frame by frame, made continuous in rots (a zero-weight frame takes
        its neighbour's); from 2-D alone each frame picks its own mirror candidate, which is not revisited along the track.
        Or p [S,T,65] / a KeypointSequenceFitResult (it is not modified).
        free: bit i clear freezes unknown i < 62 in every frame; None frees everything, or everything but trans and
        log_scale when joints3d is None.  free_cam: bits 0, 1, 2 free cs, ctx, cty; without joints2d the camera stays
        frozen.  A sequence with a keypoint or weight that is not finite, or a negative weight, in any frame is not
        fitted: cost +inf, accepted 0, p its start."""
        what = "ManoFitter.fit_keypoints_sequence"
        sm = _smooth(what, smooth, SMOOTH_KP_KEYS)
        p, args, frees = self._keypoint_args(what, "S,T", KeypointSequenceFitResult, joints3d, joints2d, w3, w2, size, sigma3,
                                             sigma2, limits, w_limit, init, free, free_cam, iters)
        cost, accepted = mano_fit_seq_kp(*args, sm, *frees)
        return KeypointSequenceFitResult(*_groups(p), p[..., 62:65], cost, accepted, p)

    def _views_sequence(self, what, joints2d, cameras, w2):
        """the checked joints2d [S,T,C,21,2], packed cameras [Sc,C,16] with Sc 1 or S and w2 [S,T,C,21] or None, contiguous"""
        if not isinstance(cameras, Cameras):
            raise ScatError(f"{what} needs cameras as a Cameras(R, t, K)")
        Sc, C = cameras.check(what)
        _need_gpu(what, joints2d, *cameras, *(() if w2 is None else (w2,)))
        _check_model(what, self.model, joints2d)
        S, T = (int(joints2d.shape[0]), int(joints2d.shape[1])) if joints2d.dim() == 5 else (0, 0)
        if S == 0 or not 1 <= T <= SEQ_MAX_T or tuple(joints2d.shape) != (S, T, C, 21, 2) or joints2d.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 joints2d [S,T,{C},21,2] with S >= 1 and T in 1..{SEQ_MAX_T} for {C} cameras, got "
                            f"{joints2d.dtype} {tuple(joints2d.shape)}")
        if Sc not in (1, S):
            raise ScatError(f"{what}: {Sc} rigs for {S} sequences: one rig for all or one per sequence")
        if cameras.R.device != joints2d.device or (w2 is not None and w2.device != joints2d.device):
            raise ScatError(f"{what}: the cameras and w2 must be on {joints2d.device}")
        return joints2d.contiguous(), cameras.packed(), _weights(what, w2, (S, T, C, 21))

    def _views(self, what, joints2d, cameras, w2):
        """the checked joints2d [B,C,21,2], packed cameras [Bc,C,16] with Bc 1 or B and w2 [B,C,21] or None, contiguous"""
        if not isinstance(cameras, Cameras):
            raise ScatError(f"{what} needs cameras as a Cameras(R, t, K)")
        Bc, C = cameras.check(what)
        _need_gpu(what, joints2d, *cameras, *(() if w2 is None else (w2,)))
        _check_model(what, self.model, joints2d)
        B = int(joints2d.shape[0]) if joints2d.dim() == 4 else 0
        if B == 0 or tuple(joints2d.shape) != (B, C, 21, 2) or joints2d.dtype != torch.float32:
            raise ScatError(f"{what} needs fp32 joints2d [B,{C},21,2] with B >= 1 for {C} cameras, got {joints2d.dtype} "
                            f"{tuple(joints2d.shape)}")
        if Bc not in (1, B):
            raise ScatError(f"{what}: {Bc} rigs for a batch of {B}: one rig for the batch or one per sample")
        if cameras.R.device != joints2d.device or (w2 is not None and w2.device != joints2d.device):
            raise ScatError(f"{what}: the cameras and w2 must be on {joints2d.device}")
        return joints2d.contiguous(), cameras.packed(), _weights(what, w2, (B, C, 21))

    @staticmethod
    def _z_near(what, z_near):
        z = float(z_near)
        if not (z > 0.0 and math.isfinite(z)):
            raise ScatError(f"{what}: z_near {z_near} must be positive and finite")
        return z

    def fit_keypoints_views(self, joints2d, cameras, w2=None, sigma2=0.0, limits=None, w_limit=0.0, init=None, free=ALL_FREE,
                            iters=None, z_near=1e-3):
        """joints2d [B,C,21,2] fp32, the pixels of the 21 keypoints in C <= 8 calibrated views (cameras: a Cameras with one
        rig for the batch or one per sample) -> FitResult, in the cameras' world frame and unit: mesh(), joints(),
        MeshEvaluator and every fit's init take it as it is.  There are no camera unknowns; with two or more views depth,
        metric scale and most of the twist are observable.
        w2: [B,C,21] or None (all ones); a view-joint of weight 0 does not count, whatever its finite pixel: this is how a
        joint that a view does not see is passed.  sigma2: the Geman-McClure scale in pixels, 0 for the quadratic loss; a
        detection that is wrong in one view is voted down by the others.  limits: (lo[45], hi[45]) on poses with the weight
        w_limit; an entry that is not finite is no limit.
        UNITS: the cost is in pixels squared, summed over up to 21 C view-joints, and the fitter's w_pose and w_beta and
        w_limit multiply squared radians and shape coefficients beside it.  A pose moves a joint by fx s / z pixels per
        radian (about 100 px for fx = 600, a 0.08 m hand at 0.5 m), so w_pose = 1e2 counts 0.1 rad like a pixel; the
        fitter's default of 1e-6, chosen beside metres squared, is no prior at all here.
        init: None for the closed-form start (every joint triangulated from its views of positive weight, see
        triangulate(), then the Procrustes of the zero-pose joints onto the triangulated ones), or p [B,62] / a FitResult,
        PointFitResult or KeypointFitResult (its first 62) to start from (it is not modified).  C = 1 needs an init: depth
        and scale cannot be told apart from one view, and nothing is triangulated.  free: bit i clear freezes unknown i.
        BEHIND THE CAMERA: a view-joint of positive weight at q.z <= z_near at the start makes the sample not fitted, and a
        trial step with one is rejected.  Not fitted means cost +inf, accepted 0 and p the start (zeros for a closed-form
        start that found fewer than 3 joints); so is a sample with a pixel, weight or camera entry that is not finite, or
        a negative weight."""
        what = "ManoFitter.fit_keypoints_views"
        joints2d, cams, w2 = self._views(what, joints2d, cameras, w2)
        B, C = int(joints2d.shape[0]), int(joints2d.shape[1])
        if init is None and C < 2:
            raise ScatError(f"{what}: one view needs a start (init): nothing can be triangulated")
        lo = hi = None
        if limits is not None:
            lo, hi = (torch.as_tensor(t, dtype=torch.float32).to(joints2d.device).contiguous() for t in limits)
            if tuple(lo.shape) != (POSE,) or tuple(hi.shape) != (POSE,):
                raise ScatError(f"{what} needs limits (lo[45], hi[45]), got {tuple(lo.shape)}, {tuple(hi.shape)}")
        if isinstance(init, KeypointFitResult):
            init = init.p[:, :UNKNOWNS]
        p = _start(what, init, (FitResult, PointFitResult), (B, UNKNOWNS), joints2d.device)
        iters = self.iters if iters is None else int(iters)
        _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE)
        if min(float(sigma2), float(w_limit)) < 0:
            raise ScatError(f"{what}: sigma2 and w_limit must not be negative")
        cost, accepted = mano_fit_views(self.model, cams, joints2d, w2, self._map_on(joints2d.device), lo, hi, p, iters,
                                        0 if init is not None else 1, self.lambda0, self.w_pose, self.w_beta, w_limit, sigma2,
                                        self._z_near(what, z_near), free)
        return FitResult(*_groups(p), cost, accepted, p)

    def fit_keypoints_views_sequence(self, joints2d, cameras, w2=None, smooth=None, sigma2=0.0, limits=None, w_limit=0.0,
                                     init=None, free=ALL_FREE, iters=None, z_near=1e-3):
        """joints2d [S,T,C,21,2] fp32, S tracks of T <= 256 frames seen by C <= 8 calibrated views (cameras: a Cameras with
        one rig for all tracks or one per track; the rig is fixed along a track) -> SequenceFitResult in the cameras' world
        frame: joints(), mesh(), project_views(), every track fit's init and MeshRenderer (via flatten(0, 1)) take it as it
        is.  fit_keypoints_views' problem in every frame (w2 [S,T,C,21] or None; sigma2, limits, w_limit, free, z_near as
        there, the same for every frame) and fit_sequence's coupling between consecutive frames, solved as one
        Levenberg-Marquardt per track: one lambda, one accept / reject.
        smooth: dict(rots=, poses=, betas=, trans=, scale=), the weight d of each group in sum_i d_i (p_t,i - p_t-1,i)^2; a
        key left out is 0, and all zero decouples the frames.  UNITS: the data term is in pixels squared, summed over up to
        21 C view-joints per frame, while each smoothness weight multiplies a squared difference in the unknown's own unit:
        radians squared for rots and poses (the penalty is on the axis-angle numbers), the shape coefficients' for betas,
        metres squared (the cameras' unit of length) for trans, a log-ratio for scale.  A hand moves by fx s / z pixels per
        radian and fx / z pixels per metre (about 100 and 1200 for fx = 600, a 0.08 m hand at 0.5 m), so rots = 1e2 counts
        0.1 rad per frame like one pixel and trans = 1e6 does so for 1 mm per frame; fit_sequence's figures, chosen beside
        metres squared, are no smoothness at all here.  As in fit_keypoints_views, w_pose = 1e2 counts 0.1 rad like a pixel.
        A frame whose weights are all zero is legal whatever its finite pixels: it has no data term and is bridged by its
        neighbours, which is how a hand that no camera sees and a padded clip are passed.  A frame with weight in only one
        view is legal too: its rows count, which fitting frame by frame cannot offer.
        init: None for the closed-form start frame by frame (fit_keypoints_views' triangulation and Procrustes; a frame
        with fewer than 3 triangulated joints takes rots, trans and scale of the frame before it, frame 0 those of the first
        frame that has a start; rots is made continuous along the track), or p [S,T,62] / a SequenceFitResult,
        PointSequenceFitResult or KeypointSequenceFitResult (its first 62) to start from (it is not modified).  C = 1 needs
        an init.  free: bit i clear freezes unknown i in every frame.
        BEHIND THE CAMERA: a view-joint of positive weight at q.z <= z_near at the start, in any frame, makes the track
        not fitted, and a trial step with one in any frame is rejected.  Not fitted means cost +inf, accepted 0 and p the
        start (the scanned closed-form start; zeros when no frame of the track has one); so is a track with a pixel,
        weight or camera entry that is not finite, or a negative weight, in any frame (p zeros for init None).  The other
        tracks are not affected."""
        what = "ManoFitter.fit_keypoints_views_sequence"
        sm = _smooth(what, smooth)
        joints2d, cams, w2 = self._views_sequence(what, joints2d, cameras, w2)
        S, T, C = (int(n) for n in joints2d.shape[:3])
        if init is None and C < 2:
            raise ScatError(f"{what}: one view needs a start (init): nothing can be triangulated")
        lo = hi = None
        if limits is not None:
            lo, hi = (torch.as_tensor(t, dtype=torch.float32).to(joints2d.device).contiguous() for t in limits)
            if tuple(lo.shape) != (POSE,) or tuple(hi.shape) != (POSE,):
                raise ScatError(f"{what} needs limits (lo[45], hi[45]), got {tuple(lo.shape)}, {tuple(hi.shape)}")
        p = self._start_sequence(what, init, S, T, joints2d.device)
        iters = self.iters if iters is None else int(iters)
        _check_ranges(what, iters, 0 <= int(free) <= ALL_FREE)
        if min(float(sigma2), float(w_limit)) < 0:
            raise ScatError(f"{what}: sigma2 and w_limit must not be negative")
        cost, accepted = mano_fit_seq_views(self.model, cams, joints2d, w2, self._map_on(joints2d.device), lo, hi, p, iters,
                                            0 if init is not None else 1, self.lambda0, self.w_pose, self.w_beta, w_limit,
                                            sigma2, self._z_near(what, z_near), sm, free)
        return SequenceFitResult(*_groups(p), cost, accepted, p)

    def triangulate(self, joints2d, cameras, w2=None, z_near=1e-3):
        """joints2d [B,C,21,2], cameras, w2 as in fit_keypoints_views -> (points [B,21,3] fp32, valid [B,21] bool): per joint
        the point nearest to the rays of its views of positive weight (weighted least squares, in fp64).  A joint is valid
        iff at least two of its views have positive weight, the rays are not parallel (closer than about 3 mrad) and the
        point is in front of every contributing camera (q.z > z_near); an invalid joint's point is 0.  A sample with a
        pixel, weight or camera entry that is not finite, or a negative weight, has no valid joint.
        joints2d [S,T,C,21,2] with w2 [S,T,C,21] and one rig for all tracks or one per track is a clip: every frame is
        triangulated with its track's rig -> (points [S,T,21,3], valid [S,T,21])."""
        what = "ManoFitter.triangulate"
        if isinstance(joints2d, torch.Tensor) and joints2d.dim() == 5:
            joints2d, cams, w2 = self._views_sequence(what, joints2d, cameras, w2)
            S, T, C = (int(n) for n in joints2d.shape[:3])
            if cams.shape[0] != 1:   # the rig of a track for each of its frames
                cams = cams[:, None].expand(S, T, C, 16).reshape(S * T, C, 16).contiguous()
            points, valid = triangulate_views(cams, joints2d.reshape(S * T, C, 21, 2), None if w2 is None else w2.reshape(S * T, C, 21),
                                              self._z_near(what, z_near))
            return points.reshape(S, T, 21, 3), valid.bool().reshape(S, T, 21)
        joints2d, cams, w2 = self._views(what, joints2d, cameras, w2)
        points, valid = triangulate_views(cams, joints2d, w2, self._z_near(what, z_near))
        return points, valid.bool()

    def project_views(self, result, cameras):
        """the fitted joints of a result (joints(result), [B,21,3]) in every camera -> [B,C,21,2] pixels; plain torch, no
        rule about joints behind a camera.  For the result of a track fit ([S,T,21,3]) with one rig for all tracks or one
        per track -> [S,T,C,21,2]"""
        what = "ManoFitter.project_views"
        if not isinstance(cameras, Cameras):
            raise ScatError(f"{what} needs cameras as a Cameras(R, t, K)")
        Bc, C = cameras.check(what)
        j = self.joints(result)
        if j.dim() == 4:
            S, T = int(j.shape[0]), int(j.shape[1])
            if Bc not in (1, S) or cameras.R.device != j.device:
                raise ScatError(f"{what} needs the result of {S} tracks and one rig, or one per track, on {j.device}")
            rig = Cameras(*(a[:, None].expand(Bc, T, *a.shape[1:]).reshape(Bc * T, *a.shape[1:]) for a in cameras)) if Bc != 1 \
                else cameras
            return project_points(j.reshape(S * T, 21, 3), rig).reshape(S, T, C, 21, 2)
        if j.dim() != 3 or Bc not in (1, int(j.shape[0])) or cameras.R.device != j.device:
            raise ScatError(f"{what} needs the result of a batch and one rig, or one per sample, on {j.device}")
        return project_points(j, cameras)

    def project(self, result, size=(224, 224)):
        """the fitted joints of a KeypointFitResult through its camera -> [B,21,2] pixels of a frame of size = (H, W):
        project_outputs on (result.cam, joints(result)); [S,T,21,2] for a KeypointSequenceFitResult"""
        from .render import project_outputs

        j = self.joints(result)
        lead = j.shape[:-2]
        out = project_outputs(torch.cat([result.cam.reshape(-1, 3), j.reshape(-1, 63)], dim=1), int(size[0]), int(size[1]))
        return out.reshape(*lead, 21, 2)

    def joints(self, result):
        """the fitted joints [B,21,3] in the targets' frame and order; [S,T,21,3] for a SequenceFitResult or a
        KeypointSequenceFitResult"""
        return self._posed(result)[0]

    def mesh(self, result):
        """the fitted mesh [B,V,3] in the targets' frame: scale x vertices + trans, through scat_mano_fwd; [S,T,V,3] for a
        SequenceFitResult or a KeypointSequenceFitResult"""
        return self._posed(result)[1]

    def _posed(self, r):
        _need_gpu("ManoFitter.mesh", r.p)
        _check_model("ManoFitter.mesh", self.model, r.p)
        if isinstance(r, (SequenceFitResult, KeypointSequenceFitResult, PointSequenceFitResult)):      # every frame as one batch, then back to [S,T,...]
            S, T = r.p.shape[:2]
            p = r.p[..., :UNKNOWNS].reshape(S * T, UNKNOWNS)
            j, v = self._posed(FitResult(*_groups(p), None, r.accepted, p))
            return j.reshape(S, T, 21, 3), v.reshape(S, T, -1, 3)
        out = mano_fwd(self.model, r.rots.contiguous(), r.poses.contiguous(), r.betas.contiguous())
        out = r.scale[:, None, None] * out + r.trans[:, None, :]
        return out[:, :21][:, self._map_on(out.device).long()], out[:, 21:].contiguous()
