"""The MANO layer on the device: joints and mesh from the 3 + 45 + 10 parameters H3DWEncoder predicts, forward and
backward (include/scat_mano.h, csrc/mano.hip).  Stands in for ``rot_pose_beta_to_mesh`` of the reference
(models/mano.py:280-391), which loads a licence-gated pickle at import; here the model's arrays are data:

    model = ManoModel.from_pickle("extra_data/MANO_RIGHT.pkl").to("cuda")      # or .synthetic(seed) / .from_arrays(d)
    layer = ManoLayer(model)
    x3d = layer.rot_pose_beta_to_mesh(rot, theta, beta)                        # [B, 21 + V, 3], as test.py:347
    out = layer.params_to_outputs(pred_params)                                 # [B,66] for scat_loss / eval_accumulate

There is no CPU fallback: CPU tensors raise ScatError.  ``ManoHand`` (the PCA-pose class, mano.py:83-201) is called by
none of the reference's scripts and has no counterpart here."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import synth
from ._lib import ScatError, lib
from .ops import _p, _stream

JOINTS, TIPS, BETAS, POSE = 16, 5, 10, 45
# kintree_table[0] of MANO with the root's parent written 0 (the root is recognised by its index)
MANO_PARENTS = (0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
MANO_TIPS = (320, 443, 671, 554, 744)            # index, middle, pinky, ring, thumb: mano.py:374-378
MAX_V = 1536                                     # SCAT_MANO_MAX_V of include/scat_mano.h


def _dense(a):
    """a numpy array from what a MANO pickle holds: arrays, scipy sparse matrices (.todense()), chumpy objects (.r)"""
    if hasattr(a, "todense"):
        a = a.todense()
    elif hasattr(a, "r"):
        a = a.r
    return np.asarray(a)


class ManoModel:
    """The arrays of one hand model, fp32 on the host: v_template[V,3], shapedirs[V,3,10], posedirs[V,3,135], dense
    J_regressor[16,V], weights[V,16], hands_mean[45], parents[16], tips[5].  ``to(device)`` adds the kernel's layouts."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, hands_mean, parents=MANO_PARENTS,
                 tips=MANO_TIPS):
        f = lambda a: np.ascontiguousarray(_dense(a), dtype=np.float32)
        self.v_template, self.shapedirs, self.posedirs = f(v_template), f(shapedirs), f(posedirs)
        self.J_regressor, self.weights, self.hands_mean = f(J_regressor), f(weights), f(hands_mean).reshape(-1)
        self.parents = tuple(int(p) for p in parents)
        self.tips = tuple(int(t) for t in tips)
        V = self.v_template.shape[0] if self.v_template.ndim == 2 else -1
        want = {"v_template": (V, 3), "shapedirs": (V, 3, BETAS), "posedirs": (V, 3, 9 * (JOINTS - 1)),
                "J_regressor": (JOINTS, V), "weights": (V, JOINTS), "hands_mean": (POSE,)}
        for k, shape in want.items():
            if getattr(self, k).shape != shape:
                raise ValueError(f"ManoModel: {k} has shape {getattr(self, k).shape}, expected {shape}")
        if not 1 <= V <= MAX_V:
            raise ValueError(f"ManoModel: {V} vertices outside 1..{MAX_V}")
        if len(self.parents) != JOINTS or self.parents[0] != 0 or any(not 0 <= p < i for i, p in enumerate(self.parents) if i):
            raise ValueError(f"ManoModel: parents {self.parents}: 16 entries, parents[0] = 0, 0 <= parents[i] < i")
        if len(self.tips) != TIPS or any(not 0 <= t < V for t in self.tips):
            raise ValueError(f"ManoModel: tips {self.tips}: 5 vertex indices in 0..{V - 1}")
        self.V = V
        self.parents_packed = sum(p << (4 * i) for i, p in enumerate(self.parents))      # one nibble each: scat_mano.h
        self.device = None

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, d):
        """d: a mapping with v_template, shapedirs, posedirs, J_regressor, weights, hands_mean and optionally parents
        (or kintree_table) and tips"""
        kw = {k: d[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean")}
        if "parents" in d:
            kw["parents"] = d["parents"]
        elif "kintree_table" in d:
            kw["parents"] = _parents_of(d["kintree_table"])
        if "tips" in d:
            kw["tips"] = d["tips"]
        return cls(**kw)

    @classmethod
    def from_pickle(cls, path):
        """The keys models/mano.py:220-232 reads from MANO_RIGHT.pkl (kintree_table, v_template, shapedirs, posedirs,
        J_regressor, weights, hands_mean); values may be arrays, sparse matrices or chumpy objects.  NOT tested against
        the real asset, which is licence-gated and which this project does not have: only against dictionaries of the
        same shape."""
        import pickle

        with open(path, "rb") as f:
            dd = pickle.load(f, encoding="latin1")
        return cls.from_arrays(dd)

    @classmethod
    def synthetic(cls, seed, V=778, tips=None):
        """A model of MANO's shape from scat_amd.synth: the same seed gives the same bytes on every machine.  Template
        uniform in +-0.1 m, shapedirs ~5 mm, posedirs ~2 mm, J_regressor rows with 8 non-zeros and weights rows with 4,
        each summing to 1, MANO's parent table, hands_mean ~ N(0, 0.2).  tips: MANO's own where they fit, else five
        vertices spread over the mesh."""
        if tips is None:
            tips = MANO_TIPS if V > max(MANO_TIPS) else tuple(((i + 1) * V) // 6 for i in range(TIPS))
        vt = synth.uniform(seed, "mano.v_template", (V, 3), -0.1, 0.1)
        sdirs = synth.normal_like(seed, "mano.shapedirs", (V, 3, BETAS), 0.005)
        pdirs = synth.normal_like(seed, "mano.posedirs", (V, 3, 9 * (JOINTS - 1)), 0.002)
        hm = synth.normal_like(seed, "mano.hands_mean", (POSE,), 0.2)

        def rows(name, n_rows, n_cols, nnz):
            nnz = min(nnz, n_cols)
            step = max(1, n_cols // nnz)
            base = np.floor(synth.uniform(seed, name + ".base", (n_rows,), 0.0, 1.0).astype(np.float64) * n_cols).astype(np.int64)
            val = synth.uniform(seed, name + ".val", (n_rows, nnz), 0.1, 1.0).astype(np.float64)
            val /= val.sum(axis=1, keepdims=True)
            m = np.zeros((n_rows, n_cols), dtype=np.float32)
            for j in range(nnz):
                m[np.arange(n_rows), (base + j * step) % n_cols] = val[:, j].astype(np.float32)
            return m

        return cls(vt, sdirs, pdirs, rows("mano.J_regressor", JOINTS, V, 8), rows("mano.weights", V, JOINTS, 4), hm,
                   MANO_PARENTS, tips)

    # ------------------------------------------------------------------ the kernel's layouts
    def to(self, device):
        """Prepares, once per model and with torch ops (not hot), what csrc/mano.hip reads: the vertex-minor blend table
        [146,3,V] (v_template, shapedirs, posedirs), J_regressor folded into a joint template [16,3] and joint shape
        directions [16,3,10] (in fp64, rounded once), weights transposed [16,V], hands_mean."""
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        vt, sd, pd = T(self.v_template), T(self.shapedirs), T(self.posedirs)
        blend = torch.cat([vt.t().unsqueeze(0), sd.permute(2, 1, 0), pd.permute(2, 1, 0)], dim=0).contiguous()
        Jr = T(self.J_regressor).double()
        joint_t = (Jr @ vt.double()).float().contiguous()
        joint_s = torch.einsum("jv,vck->jck", Jr, sd.double()).float().contiguous()
        self.blend = blend.to(device)
        self.joint_t, self.joint_s = joint_t.to(device), joint_s.to(device)
        self.weights_t = T(self.weights).t().contiguous().to(device)
        self.hands_mean_d = T(self.hands_mean).to(device)
        assert self.blend.shape == (1 + BETAS + 9 * (JOINTS - 1), 3, self.V)
        self.device = self.blend.device
        return self


def _parents_of(kintree_table):
    """mano.py:221-223: parent[i] = column of the joint whose id is kintree_table[0, i]; the root's entry becomes 0"""
    kt = np.asarray(kintree_table)
    id_to_col = {int(kt[1, i]): i for i in range(kt.shape[1])}
    return (0,) + tuple(id_to_col[int(kt[0, i])] for i in range(1, kt.shape[1]))


def _need_gpu(what, *ts):
    if not all(t.is_cuda for t in ts):
        raise ScatError(f"{what} needs GPU tensors (no CPU fallback on the product path)")


def _model_args(m):
    return (_p(m.blend), _p(m.joint_t), _p(m.joint_s), _p(m.weights_t), _p(m.hands_mean_d))


def mano_fwd(model, rots, poses, betas):
    """-> out [B, 21 + V, 3] (include/scat_mano.h scat_mano_fwd); rots [B,3], poses [B,45], betas [B,10] contiguous fp32"""
    B = rots.shape[0]
    out = torch.empty((B, 21 + model.V, 3), dtype=torch.float32, device=rots.device)
    lib().scat_mano_fwd(*_model_args(model), _p(rots), _p(poses), _p(betas), _p(out), B, model.V, model.parents_packed,
                        *model.tips, _stream())
    return out


def mano_bwd(model, rots, poses, betas, dout):
    """-> (drots, dposes, dbetas) (include/scat_mano.h scat_mano_bwd): the forward is recomputed from the inputs"""
    B = rots.shape[0]
    drots, dposes, dbetas = torch.empty_like(rots), torch.empty_like(poses), torch.empty_like(betas)
    lib().scat_mano_bwd(*_model_args(model), _p(rots), _p(poses), _p(betas), _p(dout), _p(drots), _p(dposes), _p(dbetas), B,
                        model.V, model.parents_packed, *model.tips, _stream())
    return drots, dposes, dbetas


class _ManoFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rots, poses, betas, model):
        rots, poses, betas = rots.contiguous(), poses.contiguous(), betas.contiguous()
        ctx.save_for_backward(rots, poses, betas)      # the inputs only: the backward recomputes the forward
        ctx.model = model
        return mano_fwd(model, rots, poses, betas)

    @staticmethod
    def backward(ctx, dout):
        rots, poses, betas = ctx.saved_tensors
        drots, dposes, dbetas = mano_bwd(ctx.model, rots, poses, betas, dout.contiguous())
        return drots, dposes, dbetas, None


class ManoLayer(nn.Module):
    """rot_pose_beta_to_mesh of models/mano.py:280-391 as one kernel each way.  model: a ManoModel already moved to the
    device with ``.to``.  The model's arrays get no gradient."""

    def __init__(self, model: ManoModel):
        super().__init__()
        self.model = model

    def forward(self, rots, poses, betas):
        _need_gpu("ManoLayer", rots, poses, betas)
        m = self.model
        if m.device is None or m.device != rots.device:
            raise ScatError(f"ManoLayer: the model is on {m.device}, the inputs on {rots.device}: call ManoModel.to first")
        B = rots.shape[0]
        if B == 0 or tuple(rots.shape) != (B, 3) or tuple(poses.shape) != (B, POSE) or tuple(betas.shape) != (B, BETAS):
            raise ScatError(f"ManoLayer needs rots [B,3], poses [B,45], betas [B,10] with B >= 1, got {tuple(rots.shape)}, "
                            f"{tuple(poses.shape)}, {tuple(betas.shape)}")
        if not all(t.dtype == torch.float32 for t in (rots, poses, betas)):
            raise ScatError("ManoLayer needs fp32 tensors")
        return _ManoFn.apply(rots, poses, betas, m)

    def rot_pose_beta_to_mesh(self, rots, poses, betas):
        """the reference's name and argument order (test.py:347)"""
        return self.forward(rots, poses, betas)

    def params_to_outputs(self, pred_params, joint_map=None):
        """pred_params [B,61] = 3 camera, 3 global rotation, 45 finger pose, 10 shape (test.py:335-346) -> [B,66] = camera,
        then the 21 joints flattened, optionally re-ordered by joint_map, a permutation of 0..20 that the caller passes as
        data (test.py:20-25 has such maps): the tensor scat_loss and ops.eval_accumulate take.  Differentiable."""
        _need_gpu("params_to_outputs", pred_params)
        if pred_params.dim() != 2 or pred_params.shape[1] != 3 + 3 + POSE + BETAS:
            raise ScatError(f"params_to_outputs needs pred_params [B,61], got {tuple(pred_params.shape)}")
        x3d = self.forward(pred_params[:, 3:6], pred_params[:, 6:51], pred_params[:, 51:61])
        joints = x3d[:, :21]
        if joint_map is not None:
            if sorted(int(j) for j in joint_map) != list(range(21)):
                raise ScatError("params_to_outputs: joint_map must be a permutation of 0..20")
            joints = joints[:, torch.as_tensor([int(j) for j in joint_map], device=joints.device)]
        return torch.cat([pred_params[:, :3], joints.reshape(-1, 63)], dim=1)

