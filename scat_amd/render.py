"""Looking at a prediction without leaving the device (include/scat_render.h, csrc/render.hip): the MANO mesh over the
frame, and joints and bones over the frame.  Stands in for data_utils/render.py:10-88 of the reference (pyrender, which
needs an OpenGL/EGL context) and for debug_pred_gt / plot_2d_hand (train.py:211-222, eval.py:715-742: matplotlib on the
host):

    renderer = MeshRenderer.from_pickle("extra_data/MANO_RIGHT.pkl", device="cuda")      # or MeshRenderer(faces, V)
    x3d = layer.rot_pose_beta_to_mesh(rot, theta, beta)                                   # [B, 21 + V, 3], scat_amd.mano
    rgb = renderer.overlay_outputs(x3d, cam, frames_u8)["rgb"]                            # [B,H,W,3] uint8
    SkeletonOverlay().draw_outputs(rgb, out66)                                            # joints and bones, in place

Lambert shading of interpolated vertex normals: no pixel parity with pyrender's physically based shading is claimed; the
parity target is tests/_render_oracle.py.  There is no CPU fallback: CPU tensors raise ScatError."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import ScatError
from .mano import MANO_PARENTS

MAX_V, MAX_F, MAX_HW, MAX_LIGHTS, MAX_J, MAX_BONES = 1536, 4096, 1024, 4, 32, 32      # include/scat_render.h
AMBIENT = 0.3                                    # render.py:25
BASE_RGB = (1.0, 1.0, 0.9)                       # render.py:39
LIGHT_INTENSITY = 0.4
# the three light positions of render.py:29-37 ((0,-1,1), (0,1,1), (1,1,2) in pyrender's frame, y up and the camera looking
# along -z) as directions toward the light in this frame (y down, the camera looking along +z)
LIGHT_DIRECTIONS = ((0.0, 1.0, -1.0), (0.0, -1.0, -1.0), (1.0, -1.0, -2.0))
# (parent[i], i) for the 15 chain joints, then the five tips on the last joint of their chains: joints 16..20 follow the
# chain order (include/scat_mano.h)
MANO_BONES = tuple((MANO_PARENTS[i], i) for i in range(1, 16)) + tuple((3 * k, 15 + k) for k in range(1, 6))
_FINGER_RGB = ((255, 64, 64), (64, 200, 64), (64, 96, 255), (240, 200, 40), (220, 64, 220))


def default_lights():
    """[3,4] fp32: unit direction toward the light, intensity"""
    d = np.asarray(LIGHT_DIRECTIONS, dtype=np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([d, np.full((3, 1), LIGHT_INTENSITY)], axis=1).astype(np.float32)


def _need_gpu(what, *ts):
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise ScatError(f"{what} needs GPU tensors (no CPU fallback on the product path)")


def _int_array(what, a, shape_tail):
    """a host array of integers of shape [n, *shape_tail] as int64, or ValueError"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: integer indices needed, got dtype {a.dtype}")
    if a.ndim != 1 + len(shape_tail) or tuple(a.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{what}: shape {a.shape}, expected [n, {', '.join(str(s) for s in shape_tail)}]")
    return a.astype(np.int64)


def vertex_face_csr(faces, n_vertices):
    """faces [F,3] -> (vf_off [V+1], vf_idx [3F]) int32: vf_idx[vf_off[v]:vf_off[v+1]] are the faces that name vertex v,
    ascending; every face appears three times (once per corner)"""
    flat = np.asarray(faces, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")      # stable: the faces of a vertex stay in ascending order
    vf_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_vertices))])
    return vf_off.astype(np.int32), (order // 3).astype(np.int32)


def to_uint8_hwc(x):
    """fp32 [B,3,H,W] in [-1,1] (what ops.preprocess_u8 / DeviceAugment give) -> uint8 [B,H,W,3] on the same device"""
    _need_gpu("to_uint8_hwc", x)
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ScatError(f"to_uint8_hwc needs fp32 [B,3,H,W], got {x.dtype} {tuple(x.shape)}")
    return ((x + 1.0) * 127.5).round_().clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class MeshRenderer:
    """One topology, one image size.  faces: [F,3] integers in 0..n_vertices-1 (an array, a nested list or a tensor);
    size = (H, W).  The topology is validated on the host, and the vertex -> face table built, before any HIP call; both are
    uploaded by ``to(device)``, which the constructor calls when a device is given and ``render`` calls otherwise.
    ``lights`` ([L,4], L <= 4: unit direction toward the light, intensity), ``ambient`` and ``base_rgb`` may be set."""

    def __init__(self, faces, n_vertices, size=(224, 224), device=None, lights=None, ambient=AMBIENT, base_rgb=BASE_RGB):
        f = _int_array("MeshRenderer: faces", faces, (3,))
        V, F = int(n_vertices), f.shape[0]
        if not 1 <= V <= MAX_V:
            raise ValueError(f"MeshRenderer: {V} vertices outside 1..{MAX_V}")
        if not 1 <= F <= MAX_F:
            raise ValueError(f"MeshRenderer: {F} faces outside 1..{MAX_F}")
        if f.min() < 0 or f.max() >= V:
            raise ValueError(f"MeshRenderer: face indices {f.min()}..{f.max()} outside 0..{V - 1}")
        H, W = (int(s) for s in size)
        if not (1 <= H <= MAX_HW and 1 <= W <= MAX_HW):
            raise ValueError(f"MeshRenderer: size {H} x {W} outside 1..{MAX_HW}")
        lights = default_lights() if lights is None else np.asarray(lights, dtype=np.float32).reshape(-1, 4)
        if lights.shape[0] > MAX_LIGHTS:
            raise ValueError(f"MeshRenderer: {lights.shape[0]} lights, at most {MAX_LIGHTS}")
        self.V, self.F, self.H, self.W = V, F, H, W
        self.faces = f.astype(np.int32)
        self.vf_off, self.vf_idx = vertex_face_csr(f, V)
        self.lights, self.ambient, self.base_rgb = lights, float(ambient), tuple(float(c) for c in base_rgb)
        self.device = None
        if device is not None:
            self.to(device)

    @classmethod
    def from_arrays(cls, d, **kw):
        """d: a mapping with ``f`` (faces) and ``v_template`` or ``v`` (for the vertex count), or ``n_vertices``"""
        n = d["n_vertices"] if "n_vertices" in d else len(d["v_template"] if "v_template" in d else d["v"])
        f = d["f"]
        return cls(np.asarray(f.r if hasattr(f, "r") else f), int(n), **kw)

    @classmethod
    def from_pickle(cls, path, **kw):
        """the ``f`` array of a MANO pickle, as data_utils/render.py:14-15 reads it.  NOT tested against the real asset,
        which is licence-gated and which this project does not have: only against dictionaries of the same shape."""
        import pickle

        with open(path, "rb") as fh:
            dd = pickle.load(fh, encoding="latin1")
        return cls.from_arrays(dd, **kw)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ScatError("MeshRenderer needs a GPU device (no CPU fallback on the product path)")
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.faces_d, self.vf_off_d, self.vf_idx_d = T(self.faces), T(self.vf_off), T(self.vf_idx)
        self.lights_d = T(self.lights) if len(self.lights) else None
        self.device = self.faces_d.device
        return self

    def render(self, verts, cam, img=None, cull=False, want=("rgb", "mask", "depth", "face_id")):
        """verts [B,V,3] fp32, cam [B,3] fp32 = (s, tx, ty), img [B,H,W,3] uint8 or None -> a dict with the entries named
        in ``want``: rgb [B,H,W,3] uint8, mask [B,H,W] bool, depth [B,H,W] fp32 (+inf background), face_id [B,H,W] int32
        (-1 background), proj [B,V,8] int32 (the projected vertices, include/scat_render.h).  Two launches on the current
        stream; nothing leaves the device."""
        unknown = set(want) - {"rgb", "mask", "depth", "face_id", "proj"}
        if unknown:
            raise ValueError(f"MeshRenderer.render: unknown outputs {sorted(unknown)}")
        _need_gpu("MeshRenderer.render", verts, cam, *(() if img is None else (img,)))
        if self.device is None:
            self.to(verts.device)
        if verts.device != self.device:
            raise ScatError(f"MeshRenderer: the topology is on {self.device}, the vertices on {verts.device}")
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (self.V, 3) or verts.shape[0] == 0:
            raise ScatError(f"MeshRenderer.render needs verts [B,{self.V},3] with B >= 1, got {tuple(verts.shape)}")
        B = verts.shape[0]
        if tuple(cam.shape) != (B, 3):
            raise ScatError(f"MeshRenderer.render needs cam [{B},3], got {tuple(cam.shape)}")
        if verts.dtype != torch.float32 or cam.dtype != torch.float32:
            raise ScatError("MeshRenderer.render needs fp32 verts and cam")
        if img is not None and (img.dtype != torch.uint8 or tuple(img.shape) != (B, self.H, self.W, 3)):
            raise ScatError(f"MeshRenderer.render needs img uint8 [{B},{self.H},{self.W},3], got {img.dtype} {tuple(img.shape)}")
        proj = ops.render_project(verts.contiguous(), cam.contiguous(), self.faces_d, self.vf_off_d, self.vf_idx_d, self.H,
                                  self.W)
        face_id, depth, rgb = ops.render_raster(proj, self.faces_d, self.H, self.W, None if img is None else img.contiguous(),
                                                self.lights_d, self.base_rgb, self.ambient, bool(cull), "rgb" in want)
        out = {"rgb": rgb, "depth": depth, "face_id": face_id, "proj": proj}
        if "mask" in want:
            out["mask"] = face_id >= 0
        return {k: out[k] for k in want}

    def overlay_outputs(self, mano_out, cam, img=None, cull=False, want=("rgb", "mask", "depth", "face_id")):
        """mano_out: the [B, 21 + V, 3] tensor of ManoLayer (joints first); renders rows 21 onward"""
        _need_gpu("MeshRenderer.overlay_outputs", mano_out)
        if mano_out.dim() != 3 or tuple(mano_out.shape[1:]) != (21 + self.V, 3):
            raise ScatError(f"overlay_outputs needs the layer's output [B,{21 + self.V},3], got {tuple(mano_out.shape)}")
        return self.render(mano_out.detach()[:, 21:], cam.detach(), img, cull, want)


class SkeletonOverlay:
    """Joints and bones painted over uint8 frames.  bones: [NB,2] joint indices; colors: [NB + J, 3] uint8, bones first
    (default: one colour per finger, white for the wrist); radii in pixels."""

    def __init__(self, bones=MANO_BONES, colors=None, n_joints=21, radius_bone=1.5, radius_joint=2.5):
        J = int(n_joints)
        if not 1 <= J <= MAX_J:
            raise ValueError(f"SkeletonOverlay: {J} joints outside 1..{MAX_J}")
        b = _int_array("SkeletonOverlay: bones", bones, (2,)) if len(bones) else np.zeros((0, 2), dtype=np.int64)
        if len(b) > MAX_BONES:
            raise ValueError(f"SkeletonOverlay: {len(b)} bones, at most {MAX_BONES}")
        if len(b) and (b.min() < 0 or b.max() >= J):
            raise ValueError(f"SkeletonOverlay: bone ends {b.min()}..{b.max()} outside 0..{J - 1}")
        if colors is None:
            colors = self.default_colors(b, J)
        c = np.asarray(colors)
        if c.dtype != np.uint8 or c.shape != (len(b) + J, 3):
            raise ValueError(f"SkeletonOverlay: colors must be uint8 [{len(b) + J},3], got {c.dtype} {c.shape}")
        self.J, self.NB = J, len(b)
        self.bones, self.colors = b.astype(np.int32), np.ascontiguousarray(c)
        self.radius_bone, self.radius_joint = float(radius_bone), float(radius_joint)
        self.device = None

    @staticmethod
    def default_colors(bones, J):
        """MANO's order: joint 0 the wrist, chains of three from joint 1, the tips after them in chain order"""
        def finger(j):
            return None if j == 0 else ((j - 1) // 3 if j <= 15 else j - 16) % 5

        rows = [_FINGER_RGB[finger(int(b))] if finger(int(b)) is not None else (255, 255, 255) for _, b in bones]
        rows += [_FINGER_RGB[finger(j)] if finger(j) is not None else (255, 255, 255) for j in range(J)]
        return np.asarray(rows, dtype=np.uint8).reshape(-1, 3)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ScatError("SkeletonOverlay needs a GPU device (no CPU fallback on the product path)")
        self.bones_d = torch.from_numpy(self.bones).to(device) if self.NB else None
        self.colors_d = torch.from_numpy(self.colors).to(device)
        self.device = self.colors_d.device
        return self

    def draw(self, rgb, j2d):
        """rgb [B,H,W,3] uint8, painted in place and returned; j2d [B,J,2] fp32 pixel coordinates.  One launch."""
        _need_gpu("SkeletonOverlay.draw", rgb, j2d)
        if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or not rgb.is_contiguous():
            raise ScatError(f"SkeletonOverlay.draw needs contiguous uint8 frames [B,H,W,3], got {rgb.dtype} {tuple(rgb.shape)}")
        if j2d.dtype != torch.float32 or tuple(j2d.shape) != (rgb.shape[0], self.J, 2):
            raise ScatError(f"SkeletonOverlay.draw needs fp32 j2d [{rgb.shape[0]},{self.J},2], got {j2d.dtype} {tuple(j2d.shape)}")
        if self.device != rgb.device:
            self.to(rgb.device)
        ops.render_skeleton(rgb, j2d.contiguous(), self.bones_d, self.colors_d, self.radius_bone, self.radius_joint)
        return rgb

    def draw_outputs(self, rgb, out66):
        """out66 [B,66] = camera, then 21 joints (what scat_loss and ops.eval_accumulate take), projected as the loss does
        (train.py:112-120: (s (xy + t)) half + half, half = 112 for a 224-pixel frame)"""
        _need_gpu("SkeletonOverlay.draw_outputs", rgb, out66)
        if out66.dim() != 2 or out66.shape[1] != 3 + 3 * self.J or out66.dtype != torch.float32:
            raise ScatError(f"draw_outputs needs fp32 outputs [B,{3 + 3 * self.J}], got {out66.dtype} {tuple(out66.shape)}")
        return self.draw(rgb, project_outputs(out66.detach(), rgb.shape[1], rgb.shape[2]))


def project_outputs(out66, H=224, W=224):
    """[B, 3 + 3J] -> j2d [B,J,2] fp32 pixels: u = (s (x + tx)) W/2 + W/2, v = (s (y + ty)) H/2 + H/2"""
    cam, j3 = out66[:, :3], out66[:, 3:].reshape(out66.shape[0], -1, 3)
    half = torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32, device=out66.device)
    return ((cam[:, None, :1] * (j3[:, :, :2] + cam[:, None, 1:])) * half + half).contiguous()
