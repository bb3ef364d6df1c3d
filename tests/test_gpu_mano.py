"""The MANO layer on a real MI355X (include/scat_mano.h, scat_amd/mano.py) against the fp64 oracle of
tests/_mano_oracle.py, against the reference's own fp32 output and gradients in tests/golden/mano.npz, and inside guard
bands.  Inputs and models come from scat_amd.synth."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from scat_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mano_oracle as MO  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The reference's own fp32 error against the fp64 oracle on the golden's inputs, max |ref - oracle| / max |oracle|, as
# tools/gen_mano_golden.py measured and printed it on the CPU: forward, drots, dposes, dbetas.
E_REF = {"out": 1.611e-07, "drots": 1.561e-07, "dposes": 1.495e-07, "dbetas": 2.168e-07}
# The kernel's gate is 4 x that, same normalisation, for every shape and the edge batch: the factor covers the kernel's
# different summation order (folded regressor, tree reductions over the vertices) and device sin / cos being a unit or two
# in the last place off libm.  6.444e-07, 6.244e-07, 5.980e-07, 8.672e-07.
GATE = {k: 4.0 * v for k, v in E_REF.items()}
# The same with each sample normalised by its own max |oracle| (a 3-vector like drots[b] can be small beside the batch's
# largest): the reference's worst sample of the golden's four, as the generator prints it, and 4 x that for the kernel:
# 7.120e-07, 1.094e-06, 9.744e-07, 1.320e-06.
E_REF_SAMPLE = {"out": 1.780e-07, "drots": 2.736e-07, "dposes": 2.436e-07, "dbetas": 3.300e-07}
GATE_SAMPLE = {k: 4.0 * v for k, v in E_REF_SAMPLE.items()}
NAMES = ("out", "drots", "dposes", "dbetas")

T_ = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def model(V, seed=300):
    from scat_amd.mano import ManoModel

    return ManoModel.synthetic(seed + V, V).to(DEV)


@pytest.fixture(scope="module")
def layer():
    from scat_amd._lib import lib
    from scat_amd.mano import ManoLayer

    lib().scat_check_device()
    return lambda V: ManoLayer(model(V))


def ordinary(seed, B, V):
    """rots ~ N(0, 0.8), poses ~ N(0, 0.4), betas ~ N(0, 1), dout ~ N(0, 1): the golden's distributions"""
    return [synth.normal_like(seed, "rots", (B, 3), 0.8), synth.normal_like(seed, "poses", (B, 45), 0.4),
            synth.normal_like(seed, "betas", (B, 10), 1.0), synth.normal_like(seed, "dout", (B, 21 + V, 3), 1.0)]


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def case(B, V):
    inp = frozen(ordinary(5000 + 7 * B + V, B, V))
    return inp, frozen(list(MO.forward_backward(model(V), *inp)))


def run(layer, V, rots, poses, betas, dout):
    r, p, b = (T_(a).to(DEV).requires_grad_(True) for a in (rots, poses, betas))
    out = layer(V)(r, p, b)
    out.backward(T_(dout).to(DEV))
    return [t.cpu().numpy() for t in (out.detach(), r.grad, p.grad, b.grad)]


def held(tag, got, want, gates=GATE, per_sample=False):
    """every output within its gate, max |got - want| / max |want| over the batch; per_sample: also sample by sample with
    the sample's own max |want| as the normaliser (GATE_SAMPLE), so that a large sample can not carry a small one"""
    errs = {k: MO.rel(g, w) for k, g, w in zip(NAMES, got, want)}
    print(f"{tag}: " + "  ".join(f"{k} {e:.3e} (gate {gates[k]:.3e})" for k, e in errs.items()))
    for k, g in zip(NAMES, got):
        assert np.isfinite(g).all(), k
    for k, e in errs.items():
        assert e <= gates[k], (tag, k, e, gates[k])
    if per_sample:
        each = [{k: MO.rel(g[b], w[b]) for k, g, w in zip(NAMES, got, want)} for b in range(got[0].shape[0])]
        for b, e in enumerate(each):
            print(f"  sample {b}: " + "  ".join(f"{k} {v:.3e} (gate {GATE_SAMPLE[k]:.3e})" for k, v in e.items()))
        for b, e in enumerate(each):
            for k, v in e.items():
                assert v <= GATE_SAMPLE[k], (tag, b, k, v, GATE_SAMPLE[k])


# V = 778: MANO.  V = 37: less than one wavefront and odd, tips inside.  V = 1030: more than the workgroup's 1024 threads,
# so the vertex loop takes a second trip and the strided sums have ragged tails.
@pytest.mark.parametrize("B,V", [(1, 778), (2, 778), (5, 778), (64, 778), (97, 778), (3, 37), (3, 1030)])
def test_matches_the_oracle(layer, B, V):
    inp, want = case(B, V)
    got = run(layer, V, *inp)
    assert got[0].shape == (B, 21 + V, 3) and got[1].shape == (B, 3) and got[2].shape == (B, 45) and got[3].shape == (B, 10)
    held(f"B {B} V {V}", got, want)
    assert np.abs(got[0][:, 1]).max() == 0.0      # joint 1 is the origin
    tips = model(V).tips
    assert np.array_equal(got[0][:, 16:21], got[0][:, [21 + t for t in tips]])


@functools.lru_cache(maxsize=None)
def edge_batch():
    """B = 8, one sample each: 0 full pose, rots and betas exactly zero; 1 angles of 1e-20 (rots; the finger angles are
    hands_mean + poses in fp32, where 1e-20 is absorbed: exactly zero again); 2 angles of 1e-6; 3 angles of 1e-3;
    4 |rots| = pi along x; 5 every angle 3.5; 6 betas = +-3; 7 ordinary.  hands_mean + poses is exact in fp32 for the tiny
    angles (the two nearly cancel), so the oracle sees the same angles as the kernel."""
    V = 778
    m = model(V)
    hm = m.hands_mean
    rots, poses, betas, dout = ordinary(6100, 8, V)
    rots[0], poses[0], betas[0] = 0.0, -hm, 0.0
    for b, eps in ((1, 1e-20), (2, 1e-6), (3, 1e-3)):
        rots[b] = np.float32(eps)
        poses[b] = (np.float32(eps) - hm).astype(np.float32)
    assert np.all(hm + poses[0] == 0) and np.all(hm + poses[1] == 0) and np.all(rots[1] > 0)
    assert np.all(np.abs((hm + poses[2]) / 1e-6 - 1) < 0.05) and np.all(np.abs((hm + poses[3]) / 1e-3 - 1) < 1e-4)
    rots[4] = (np.float32(np.pi), 0.0, 0.0)
    rots[5] *= 3.5 / np.linalg.norm(rots[5])
    full = (hm + poses[5]).reshape(15, 3).astype(np.float64)
    poses[5] = ((full * (3.5 / np.linalg.norm(full, axis=1, keepdims=True))).reshape(45) - hm).astype(np.float32)
    betas[6] = 3.0 * np.where(np.arange(10) % 2 == 0, 1.0, -1.0)
    inp = frozen([rots, poses, betas, dout])
    return inp, frozen(list(MO.forward_backward(m, *inp)))


def test_edge_batch(layer):
    """held to the oracle, not to the reference, whose gradient is NaN or noise at the tiny angles; every sample also with
    its own normaliser"""
    inp, want = edge_batch()
    held("edge batch", run(layer, 778, *inp), want, per_sample=True)


@functools.lru_cache(maxsize=None)
def zero_mean_model(V=37):
    """hands_mean = 0: the finger angles are poses themselves, so 1e-20 reaches the 15 chain rotations (with a non-zero
    hands_mean fp32 absorbs it)"""
    from scat_amd.mano import ManoModel

    m = ManoModel.synthetic(341, V)
    arrays = {k: getattr(m, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    return ManoModel.from_arrays(dict(arrays, hands_mean=np.zeros(45, np.float32), tips=m.tips)).to(DEV)


def test_tiny_finger_angles(layer):
    """B = 4 on a model with hands_mean = 0: every angle, the 15 fingers' included, 1e-20, 1e-6, 1e-3 and (series /
    closed form switch at theta^2 = 0.25) 0.5 / sqrt(3) per component, i.e. theta = 0.5 exactly at the switch"""
    from scat_amd.mano import ManoLayer

    m = zero_mean_model()
    rots, poses, betas, dout = ordinary(6200, 4, m.V)
    for b, eps in enumerate((1e-20, 1e-6, 1e-3, 0.5 / np.sqrt(3.0))):
        rots[b], poses[b] = np.float32(eps), np.float32(eps)
    want = MO.forward_backward(m, rots, poses, betas, dout)
    r, p, be = (T_(a).to(DEV).requires_grad_(True) for a in (rots, poses, betas))
    out = ManoLayer(m)(r, p, be)
    out.backward(T_(dout).to(DEV))
    held("tiny finger angles", [t.cpu().numpy() for t in (out.detach(), r.grad, p.grad, be.grad)], want, per_sample=True)


def test_matches_the_reference_golden(layer, golden):
    """the kernel on the inputs of tests/golden/mano.npz against the reference's own fp32 output and autograd gradients"""
    from scat_amd.mano import ManoLayer, ManoModel

    g = golden("mano")
    seed, B = int(g["seed"]), g["rots"].shape[0]
    lay = ManoLayer(ManoModel.synthetic(seed).to(DEV))
    r, p, b = (T_(g[k]).to(DEV).requires_grad_(True) for k in ("rots", "poses", "betas"))
    out = lay.rot_pose_beta_to_mesh(r, p, b)
    out.backward(T_(MO.golden_dout(seed, B, 778)).to(DEV))
    got = [t.cpu().numpy() for t in (out.detach(), r.grad, p.grad, b.grad)]
    held("golden", got, [g[k] for k in NAMES])


def test_same_call_same_bits(layer):
    inp, _ = case(5, 778)
    a, b = run(layer, 778, *inp), run(layer, 778, *inp)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    inp, _ = case(3, 1030)
    a, b = run(layer, 1030, *inp), run(layer, 1030, *inp)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_both_kernels_inside_guard_bands(fill):
    """every operand of both entry points between poisoned bands at pointer skews 0, 1 and 3 floats: bands intact, every
    output element written, results equal to the skew-0 run bit for bit and within the gates"""
    from scat_amd._lib import lib

    L = lib()
    L.scat_check_device()
    B, V = 3, 1030
    m = model(V)
    inp, want = case(B, V)
    stream = torch.cuda.current_stream().cuda_stream
    arena = Arena(DEV, fill, nbytes=16 << 20)
    runs = {}
    for skew in (0, 1, 3):
        arena.reset()
        mod = [arena.place(t.cpu(), skew, name=n) for n, t in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                               ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        r, p, b, dy = (arena.place(T_(a), skew, name=n) for n, a in zip(("rots", "poses", "betas", "dout"), inp))
        out = arena.place((B, 21 + V, 3), skew, name="out", out=True)
        dr = arena.place((B, 3), skew, name="drots", out=True)
        dp = arena.place((B, 45), skew, name="dposes", out=True)
        db = arena.place((B, 10), skew, name="dbetas", out=True)
        assert all(t.data_ptr() % 16 == 4 * skew for t in mod + [r, p, b, dy, out, dr, dp, db])
        mp = [t.data_ptr() for t in mod]
        L.scat_mano_fwd(*mp, r.data_ptr(), p.data_ptr(), b.data_ptr(), out.data_ptr(), B, V, m.parents_packed, *m.tips, stream)
        assert L.scat_last_kernel() == b"mano_fwd_v1030"
        L.scat_mano_bwd(*mp, r.data_ptr(), p.data_ptr(), b.data_ptr(), dy.data_ptr(), dr.data_ptr(), dp.data_ptr(),
                        db.data_ptr(), B, V, m.parents_packed, *m.tips, stream)
        assert L.scat_last_kernel() == b"mano_bwd_v1030"
        torch.cuda.synchronize()
        arena.check()
        runs[skew] = [t.cpu().numpy().copy() for t in (out, dr, dp, db)]
    held(f"guard {fill}", runs[0], want)
    for skew in (1, 3):
        for x, y in zip(runs[0], runs[skew]):
            assert x.tobytes() == y.tobytes(), skew


def _loss64(out, labels, w3d=100000.0, w2d=10.0):
    """train.py:165-203 in torch fp64: orthographic projection * 112 + 112, w3d MSE(3-D) + w2d L1(2-D)"""
    cam, j3 = out[:, :3].reshape(-1, 1, 3), out[:, 3:66].reshape(-1, 21, 3)
    j2 = (cam[:, :, :1] * (j3[:, :, :2] + cam[:, :, 1:])) * 112.0 + 112.0
    g3, g2 = labels[:, :63], labels[:, 63:]
    return w3d * (j3.reshape(-1, 63) - g3).square().mean() + w2d * (j2.reshape(-1, 42) - g2).abs().mean()


def test_h3dw_to_loss_composition(layer):
    """H3DWEncoder at batch 1 -> params_to_outputs -> scat_loss -> backward(): the retained pred_params.grad against the
    fp64 oracle composed with the loss restated in fp64, on the detached parameters.  The network is the one of
    tests/test_gpu_model.py::test_h3dw_encoder_golden with the head's weights scaled to give hand-like parameters.  Gate:
    1e-4, the bar the project holds
    the loss kernel's gradient to (tests/test_gpu_ops.py), plus the largest of the layer's own gradient gates: the
    cotangent the layer receives is that kernel's output, and the layer adds its own rounding to it."""
    from scat_amd import ops
    from scat_amd.models.hand_net import H3DWEncoder
    from scat_amd.trainer import scat_loss
    from tests.test_gpu_model import opt_ns

    net = H3DWEncoder(opt_ns(), T_(synth.normal_like(81, "mean61", (1, 61))) * 0.1)
    sd = {k: v for k, v in synth.to_torch(synth.encoder_transformer_state(81, 8)).items() if k.startswith("main_encoder.")}
    for k, shp, s in (("feat_encoder.1.weight", (1024, 1024), 1024 ** -0.5), ("feat_encoder.1.bias", (1024,), 0.05),
                      ("regressor.0.weight", (61, 1085), 1e-4 * 1085 ** -0.5), ("regressor.0.bias", (61,), 0.05)):
        sd[k] = T_(synth.normal_like(82, k, shp)) * s
    # (the synthetic backbone's features have a standard deviation of 1.4e3 (tests/golden/h3dw.npz): with unit-gain
    # head weights the "parameters" are rotations of 1e4 rad and betas of 7e3, where one fp32 ulp of an angle is 1e-3 rad
    # and no fp32 layer, the reference's included, is comparable with fp64.  1e-4 on the head's weights makes them
    # hand-like, |rots| ~ 0.6, finger pose ~ N(0, 0.6), betas ~ N(0, 0.5): the regime the gates were measured in.)
    net.load_state_dict(sd, strict=True)
    net.cuda().train()
    net.main_encoder.eval()
    for q in net.main_encoder.parameters():
        q.requires_grad_(False)
    lay = layer(778)
    labels = T_(synth.labels(85, 1)).to(DEV)
    # a joint order passed as data: a fixed permutation of 0..20 without a fixed point (7 is coprime to 21)
    for jmap in (None, tuple((7 + 8 * j) % 21 for j in range(21))):
        _, pred = net(T_(synth.images(83, 1)).to(DEV))
        assert tuple(pred.shape) == (1, 61)
        assert 0.05 < float(pred.detach()[0, 3:6].norm()) < 3.5 and float(pred.detach()[0, 6:].abs().max()) < 3.5      # hand-like, see above
        pred.retain_grad()
        out = lay.params_to_outputs(pred, jmap)
        assert tuple(out.shape) == (1, 66)
        loss, parts = scat_loss(out, labels)
        loss.backward()
        p64 = pred.detach().cpu().double().requires_grad_(True)
        x = MO.forward(model(778), p64[:, 3:6], p64[:, 6:51], p64[:, 51:61])[:, :21]
        if jmap is not None:
            x = x[:, list(jmap)]
        out64 = torch.cat([p64[:, :3], x.reshape(1, 63)], dim=1)
        loss64 = _loss64(out64, labels.cpu().double())
        loss64.backward()
        e_out, e_loss = MO.rel(out.detach().cpu().numpy(), out64.detach().numpy()), abs(loss.item() - loss64.item()) / loss64.item()
        e_grad = MO.rel(pred.grad.cpu().numpy(), p64.grad.numpy())
        # (measured on an MI355X: pred_params.grad 1.791e-07 without a joint map, 9.994e-08 with one; out 4.362e-08)
        gate = 1e-4 + max(GATE["drots"], GATE["dposes"], GATE["dbetas"])
        print(f"composition map {jmap is not None}: out {e_out:.3e} loss {e_loss:.3e} pred_params.grad {e_grad:.3e} (gate {gate:.3e})")
        assert e_out <= GATE["out"] and e_loss < 1e-5 and e_grad <= gate
        # the same [B,66] is what the evaluation takes
        rec, _, _ = ops.eval_accumulate(out.detach().contiguous(), labels, [20.0, 30.0, 50.0])
        rec = rec.cpu().numpy()
        assert rec[0] == 1 and rec[1] == 1 and rec[3] == 0 and np.isfinite(rec).all()
