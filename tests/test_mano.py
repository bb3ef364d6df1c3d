"""The MANO layer, the parts that need no GPU: the third public header and its binding, argument errors of both entry
points, ManoModel's constructors, and the fp64 oracle of tests/_mano_oracle.py pinned to the reference's own output and
gradients (tests/golden/mano.npz, written by tools/gen_mano_golden.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mano_oracle as MO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANO_H = os.path.join(ROOT, "include", "scat_mano.h")

# tools/gen_mano_golden.py prints the reference's own fp32 error against the oracle on the golden's inputs,
# max |ref - oracle| / max |oracle|: forward, drots, dposes, dbetas.  "To the reference's own rounding" is taken as 4 x
# these, the factor the GPU tests give the kernel, so the check fails if either side moves by more than rounding.
E_REF = {"out": 1.611e-07, "drots": 1.561e-07, "dposes": 1.495e-07, "dbetas": 2.168e-07}


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_mano_header_is_bound(built):
    from scat_amd._lib import HEADERS, MANO_HEADER, lib, parse_header

    assert os.path.samefile(HEADERS[-1], MANO_H)
    protos = parse_header(MANO_H)
    assert set(protos) == {"scat_mano_fwd", "scat_mano_bwd"}
    L = lib()
    for name, (rt, args) in protos.items():
        assert hasattr(L.cdll, name), name
        assert callable(getattr(L, name)), name
        assert rt is ctypes.c_int and args[-1][1] == "stream", name
        names = [an for _, an in args]
        assert "ws" not in names and "ws_bytes" not in names and not name.endswith("_ws")
        # the tree and the tips travel by value
        assert dict((an, ty) for ty, an in args)["parents"] is ctypes.c_uint64
        assert [ty for ty, an in args if an.startswith("tip")] == [ctypes.c_int] * 5
    assert L.by_header[MANO_HEADER] == protos and list(L.by_header) == list(HEADERS) and not set(protos) & set(L.protos)
    assert not set(protos) & set(parse_header())
    src = open(MANO_H).read()
    assert src.count("mano.py:") >= 12      # the header cites the reference lines it stands in for
    from scat_amd import mano

    assert f"#define SCAT_MANO_MAX_V {mano.MAX_V}\n" in src and mano.MAX_V >= 1030


PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))


def _with_parent(i, p):
    return (PARENTS & ~(15 << (4 * i))) | (p << (4 * i))


@pytest.mark.parametrize("entry", ["scat_mano_fwd", "scat_mano_bwd"])
def test_mano_errors_surface_without_a_gpu(built, entry):
    """argument validation of both entry points happens before any HIP call: made-up pointers are never followed, each
    refusal carries its SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib

    L = lib()
    nptr = 9 if entry == "scat_mano_fwd" else 12
    good = dict(ptrs=[8 * (i + 1) for i in range(nptr)], B=4, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744])

    def call(**kw):
        a = dict(good, **kw)
        return getattr(L, entry)(*a["ptrs"], a["B"], a["V"], a["parents"], *a["tips"], 0)

    label = L.scat_last_kernel()

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            call(**kw)
        assert L.scat_last_kernel() == label

    for i in range(nptr):
        ptrs = list(good["ptrs"])
        ptrs[i] = 0
        refused(-2, "null pointer", ptrs=ptrs)
    ptrs = list(good["ptrs"])
    ptrs[5] = 10
    refused(-2, "4-byte aligned", ptrs=ptrs)
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    for j in range(5):
        tips = list(good["tips"])
        tips[j] = 778
        refused(-1, rf"tip {j} = 778", tips=tips)
    refused(-1, "tip 0 = -1", tips=[-1, 443, 671, 554, 744])
    refused(-1, "tip 4 = 744", V=744)
    for i, p in ((1, 1), (3, 3), (3, 7), (15, 15)):
        refused(-2, rf"parent\[{i}\] = {p}", parents=_with_parent(i, p))
    refused(-2, r"parent\[0\] = 5", parents=_with_parent(0, 5))


def test_mano_layer_has_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.mano import ManoLayer, ManoModel

    layer = ManoLayer(ManoModel.synthetic(1, V=37))
    with pytest.raises(ScatError, match="no CPU fallback"):
        layer(torch.zeros(2, 3), torch.zeros(2, 45), torch.zeros(2, 10))
    with pytest.raises(ScatError, match="no CPU fallback"):
        layer.rot_pose_beta_to_mesh(torch.zeros(2, 3), torch.zeros(2, 45), torch.zeros(2, 10))
    with pytest.raises(ScatError, match="no CPU fallback"):
        layer.params_to_outputs(torch.zeros(1, 61))


def test_synthetic_model_is_deterministic_and_normalised():
    from scat_amd.mano import MANO_PARENTS, MANO_TIPS, ManoModel

    a, b, c = ManoModel.synthetic(7), ManoModel.synthetic(7), ManoModel.synthetic(8)
    names = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean")
    for k in names:
        assert getattr(a, k).dtype == np.float32
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
        assert getattr(a, k).tobytes() != getattr(c, k).tobytes(), k
    assert a.V == 778 and a.parents == MANO_PARENTS and a.tips == MANO_TIPS
    for V in (778, 37, 1030):
        m = ManoModel.synthetic(7, V)
        assert np.abs(m.J_regressor.astype(np.float64).sum(1) - 1).max() < 1e-6
        assert np.abs(m.weights.astype(np.float64).sum(1) - 1).max() < 1e-6
        assert ((m.J_regressor != 0).sum(1) == 8).all() and ((m.weights != 0).sum(1) == 4).all()
        assert (m.J_regressor >= 0).all() and (m.weights >= 0).all()
        assert len(set(m.tips)) == 5 and all(0 < t < V - 1 for t in m.tips)      # placed inside
        assert np.abs(m.v_template).max() <= 0.1
        assert 0.004 < m.shapedirs.std() < 0.006 and 0.0015 < m.posedirs.std() < 0.0025
        assert 0.15 < m.hands_mean.std() < 0.25
    # the prepared layouts, on the host: the regressor folds exactly (it is linear)
    m = ManoModel.synthetic(7, 37).to("cpu")
    assert m.blend.shape == (146, 3, 37) and m.weights_t.shape == (16, 37)
    assert torch.equal(m.blend[0], torch.from_numpy(m.v_template).t())
    assert torch.equal(m.blend[1 + 4, 2], torch.from_numpy(m.shapedirs[:, 2, 4].copy()))
    assert torch.equal(m.blend[11 + 77, 1], torch.from_numpy(m.posedirs[:, 1, 77].copy()))
    beta = np.linspace(-1, 1, 10)
    J = m.J_regressor.astype(np.float64) @ (m.v_template + m.shapedirs.astype(np.float64) @ beta)
    Jf = m.joint_t.double().numpy() + m.joint_s.double().numpy() @ beta
    assert np.abs(J - Jf).max() < 1e-7
    assert m.parents_packed == PARENTS


def test_from_arrays_and_from_pickle(tmp_path):
    import pickle

    from scat_amd.mano import MANO_PARENTS, ManoModel

    src = ManoModel.synthetic(5, 37)
    d = {k: getattr(src, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean")}
    d["tips"] = src.tips
    m = ManoModel.from_arrays(d)
    assert m.V == 37 and m.parents == MANO_PARENTS and m.tips == src.tips
    for k, bad in (("v_template", (37, 2)), ("shapedirs", (37, 3, 9)), ("posedirs", (37, 3, 134)), ("J_regressor", (37, 16)),
                   ("weights", (36, 16)), ("hands_mean", (44,))):
        with pytest.raises(ValueError, match=k):
            ManoModel.from_arrays(dict(d, **{k: np.zeros(bad, np.float32)}))
    with pytest.raises(ValueError, match="tips"):
        ManoModel.from_arrays(dict(d, tips=(1, 2, 3, 4, 37)))
    with pytest.raises(ValueError, match="parents"):
        ManoModel.from_arrays(dict(d, parents=(0, 0, 2) + MANO_PARENTS[3:]))
    with pytest.raises(ValueError, match="vertices"):
        ManoModel.from_arrays(dict(v_template=np.zeros((1537, 3)), shapedirs=np.zeros((1537, 3, 10)),
                                   posedirs=np.zeros((1537, 3, 135)), J_regressor=np.zeros((16, 1537)),
                                   weights=np.zeros((1537, 16)), hands_mean=np.zeros(45)))

    class Dense:                                       # what scipy's sparse matrices and chumpy's arrays offer
        def __init__(self, a):
            self.a = a

        def todense(self):
            return self.a

    class Ch:
        def __init__(self, a):
            self.r = a

    kt = np.array([[4294967295] + list(MANO_PARENTS[1:]), list(range(16))], dtype=np.int64)
    dd = dict(kintree_table=kt, v_template=Ch(src.v_template.astype(np.float64)), shapedirs=Ch(src.shapedirs),
              posedirs=src.posedirs, J_regressor=Dense(src.J_regressor), weights=src.weights, hands_mean=src.hands_mean,
              hands_components=np.eye(45))
    p = ManoModel.from_arrays(dict(dd, tips=src.tips))
    assert p.parents == MANO_PARENTS and p.J_regressor.tobytes() == src.J_regressor.tobytes()
    assert p.v_template.tobytes() == src.v_template.tobytes()
    path = tmp_path / "hand.pkl"
    plain = dict(dd, v_template=src.v_template, shapedirs=src.shapedirs, J_regressor=src.J_regressor)
    with open(path, "wb") as f:
        pickle.dump(plain, f)
    with pytest.raises(ValueError, match="tips"):      # MANO's own tips do not fit 37 vertices
        ManoModel.from_pickle(str(path))
    big = ManoModel.synthetic(5)
    plain = {k: getattr(big, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean")}
    plain["kintree_table"] = kt
    with open(path, "wb") as f:
        pickle.dump(plain, f)
    q = ManoModel.from_pickle(str(path))
    assert q.V == 778 and q.parents == MANO_PARENTS and q.weights.tobytes() == big.weights.tobytes()


def test_oracle_reproduces_the_reference(golden):
    """the fp64 restatement against the reference's fp32 output and autograd gradients: pins it to models/mano.py, not to
    the kernel"""
    from scat_amd.mano import ManoModel

    g = golden("mano")
    seed = int(g["seed"])
    model = ManoModel.synthetic(seed)
    rots, poses, betas = MO.golden_inputs(seed, g["rots"].shape[0])
    assert rots.tobytes() == g["rots"].tobytes() and poses.tobytes() == g["poses"].tobytes()
    assert betas.tobytes() == g["betas"].tobytes()
    angles = np.linalg.norm((model.hands_mean[None] + poses).reshape(-1, 15, 3), axis=2)
    assert angles.min() >= MO.MIN_ANGLE and np.linalg.norm(rots, axis=1).min() >= MO.MIN_ANGLE
    B = rots.shape[0]
    assert g["out"].shape == (B, 21 + 778, 3) and g["out"].dtype == np.float32
    want = MO.forward_backward(model, rots, poses, betas, MO.golden_dout(seed, B, model.V))
    for k, w in zip(("out", "drots", "dposes", "dbetas"), want):
        e = MO.rel(g[k], w)
        print(f"{k}: reference vs oracle {e:.3e} (recorded {E_REF[k]:.3e})")
        assert e <= 4 * E_REF[k], k
    assert np.abs(g["out"][:, 1]).max() == 0.0      # joint 1 is the origin


def test_oracle_gradients_at_zero_pose_agree_with_central_differences():
    """full pose exactly zero (poses = -hands_mean, rots = 0, betas = 0): finite gradients, and equal to central differences
    of the oracle's own fp64 forward (step 1e-6: truncation ~1e-12, rounding ~1e-10 relative)"""
    from scat_amd import synth
    from scat_amd.mano import ManoModel

    model = ManoModel.synthetic(11, V=37)
    rots, betas = np.zeros((1, 3)), np.zeros((1, 10))
    poses = -model.hands_mean.astype(np.float64).reshape(1, 45)
    dout = synth.normal_like(11, "dout", (1, 21 + 37, 3), 1.0).astype(np.float64)
    out, dr, dp, db = MO.forward_backward(model, rots, poses, betas, dout)
    assert all(np.isfinite(a).all() for a in (out, dr, dp, db))
    assert np.abs(dr).max() > 0 and np.abs(dp).max() > 0 and np.abs(db).max() > 0
    x0 = np.concatenate([rots, poses, betas], axis=1)

    def f(x):
        t = torch.from_numpy(x)
        with torch.no_grad():
            return float((MO.forward(model, t[:, :3], t[:, 3:48], t[:, 48:]) * torch.from_numpy(dout)).sum())

    h = 1e-6
    fd = np.zeros(58)
    for i in range(58):
        e = np.zeros((1, 58))
        e[0, i] = h
        fd[i] = (f(x0 + e) - f(x0 - e)) / (2 * h)
    an = np.concatenate([dr, dp, db], axis=1)[0]
    assert np.abs(fd - an).max() / np.abs(an).max() < 1e-7
