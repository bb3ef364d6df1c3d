"""Writes tests/golden/mano.npz from the reference's own rot_pose_beta_to_mesh (models/mano.py:280-391), on the CPU:

    python tools/gen_mano_golden.py /path/to/reference/checkout

The reference module loads extra_data/MANO_RIGHT.pkl at import and moves everything to the GPU.  Three stubs let it
run here without either: pickle.load returns a dictionary made from ManoModel.synthetic(seed), open() of that pickle's
path returns an empty stream, and torch.Tensor.cuda is the identity.  The model is not stored: tests regenerate it from
the seed.  Stored: the seed, B = 4 ordinary inputs, the reference's fp32 output and its three autograd gradients for a
cotangent regenerated from the same seed (golden_dout of tests/_mano_oracle.py, which also holds the inputs' recipe).

Also prints the reference's own fp32 error against the fp64 oracle of tests/_mano_oracle.py, forward and per gradient
(max |ref - oracle| / max |oracle|, over the batch and, worst case, sample by sample): the gates of
tests/test_gpu_mano.py are 4 x these."""
import builtins
import importlib.util
import io
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mano_oracle as MO  # noqa: E402
from scat_amd.mano import MANO_PARENTS, ManoModel  # noqa: E402

SEED, B = 2024, 4


class _Dense:
    def __init__(self, a):
        self.a = a

    def todense(self):
        return self.a


def load_reference(ref_root, model):
    """models/mano.py of the checkout as a module, fed the synthetic model"""
    kt = np.array([[4294967295] + list(MANO_PARENTS[1:]), list(range(16))], dtype=np.int64)
    dd = dict(kintree_table=kt, v_template=model.v_template, shapedirs=model.shapedirs, posedirs=model.posedirs,
              J_regressor=_Dense(model.J_regressor), weights=model.weights, hands_mean=model.hands_mean,
              hands_components=np.eye(45, dtype=np.float32))      # read at import, unused by the function
    real_open, real_load = builtins.open, pickle.load
    builtins.open = lambda p, *a, **k: io.BytesIO(b"") if str(p).endswith("MANO_RIGHT.pkl") else real_open(p, *a, **k)
    pickle.load = lambda *a, **k: dd
    torch.Tensor.cuda = lambda self, *a, **k: self      # stays: the function calls .cuda() on every constant it builds
    try:
        spec = importlib.util.spec_from_file_location("reference_mano", os.path.join(ref_root, "models", "mano.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        builtins.open, pickle.load = real_open, real_load
    return mod


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    model = ManoModel.synthetic(SEED)
    assert model.V == 778 and model.tips == (320, 443, 671, 554, 744)
    ref = load_reference(sys.argv[1], model)
    rots, poses, betas = MO.golden_inputs(SEED, B)
    angles = np.linalg.norm((model.hands_mean[None] + poses).reshape(B, 15, 3), axis=2)
    assert angles.min() >= MO.MIN_ANGLE and np.linalg.norm(rots, axis=1).min() >= MO.MIN_ANGLE, \
        (angles.min(), np.linalg.norm(rots, axis=1).min())
    dout = MO.golden_dout(SEED, B, model.V)
    r, p, b = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (rots, poses, betas))
    out = ref.rot_pose_beta_to_mesh(r, p, b)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 21 + model.V, 3)
    out.backward(torch.from_numpy(dout))
    got = [out.detach().numpy(), r.grad.numpy(), p.grad.numpy(), b.grad.numpy()]
    assert all(np.isfinite(g).all() for g in got)
    want = MO.forward_backward(model, rots, poses, betas, dout)
    for name, g, w in zip(("e_fwd", "e_drots", "e_dposes", "e_dbetas"), got, want):
        worst = max(MO.rel(g[i], w[i]) for i in range(B))
        print(f"{name} = {MO.rel(g, w):.3e}   (max |oracle| {np.abs(w).max():.3e}); sample by sample, each with its own "
              f"max |oracle|, worst {worst:.3e}")
    print(f"smallest finger angle {angles.min():.3f} rad, smallest |rots| {np.linalg.norm(rots, axis=1).min():.3f} rad")
    path = os.path.join(ROOT, "tests", "golden", "mano.npz")
    np.savez_compressed(path, seed=np.int64(SEED), rots=rots, poses=poses, betas=betas, out=got[0], drots=got[1],
                        dposes=got[2], dbetas=got[3])
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
