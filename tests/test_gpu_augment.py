"""Device augmentation on a real MI355X against the fp64 numpy oracle of tests/_augment_oracle.py,
against the library's own preprocess_u8, against a geometry check that trusts no formula, and through DeviceAugment into
a train step.  Tolerances are norm-wise relative (oracle.util.rel_err)."""
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.util import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_oracle as AO  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
W, H, B = 640, 480, 96


@pytest.fixture(scope="module")
def ops():
    from scat_amd import ops as o
    from scat_amd._lib import lib

    lib().scat_check_device()
    return o


def _params(rng, n):
    """every combination of flip / blur (both directions, odd and even k) / rotation occurs, and the right angles too"""
    p = np.zeros((n, 4), dtype=np.int32)
    blurred = 0
    for i in range(n):
        p[i, 0] = i & 1
        if (i >> 1) & 1:
            p[i, 1] = 1 + blurred % 10
            p[i, 2] = (i >> 3) & 1
            blurred += 1
        if (i >> 2) & 1:
            p[i, 3] = int(rng.integers(1, 361))
    for i, a in zip((4, 5, 6, 7, 12), (90, 180, 270, 360, 45)):
        p[i, 3] = a
    return p


@pytest.fixture(scope="module")
def batch():
    """B = 96 seeded samples of 640 x 480: joints (hand centre well inside the frame, extent 40-110 pixels), random uint8
    frames, parameters, and the oracle's labels / plans / images"""
    rng = np.random.default_rng(17)
    j2, j3 = AO.seeded_joints(rng, B, W, H)
    params = _params(rng, B)
    combos = {(int(p[0]), int(p[1] > 0), int(p[2]), int(p[3] > 0)) for p in params}
    assert len(combos) == 12 and {int(k) for k in params[:, 1]} >= {0, 1, 2, 9, 10}    # vert only counts with a blur
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    labels, plans, images = [], [], []
    for i in range(B):
        lab, plan = AO.labels_and_plan(j2[i], j3[i], W, H, params[i, 0], params[i, 3])
        labels.append(lab)
        plans.append(plan)
        images.append(AO.image(frames[i], params[i, 0], params[i, 1], params[i, 2], plan))
    return SimpleNamespace(j2=j2, j3=j3, params=params, frames=frames, labels=np.stack(labels), plans=plans,
                           images=np.stack(images))


def _plan(ops, batch, normalize_3d=True):
    return ops.augment_plan(torch.from_numpy(batch.j2).to(DEV), torch.from_numpy(batch.j3).to(DEV),
                            torch.from_numpy(batch.params).to(DEV), (W, H), normalize_3d)


def test_labels_and_plan(ops, batch):
    """labels to 1e-6 of the fp64 oracle, the 63 3-D entries (about 0.03) and the 42 2-D entries (about 100) separately;
    the integer part of the plan exactly.  Input condition: every un-rounded box coordinate is at least 1e-6 away from a
    half-integer, so a last-bit difference cannot flip PIL's rounding."""
    assert min(AO.half_distance(p) for p in batch.plans) >= 1e-6
    labels, plan = _plan(ops, batch)
    torch.cuda.synchronize()
    from scat_amd._lib import lib

    assert lib().scat_last_kernel() == b"augment_plan"
    assert labels.shape == (B, 105) and labels.dtype == torch.float32 and plan.shape == (B, ops.AUGMENT_PLAN_FLOATS)
    e3, e2 = rel_err(labels[:, :63], batch.labels[:, :63]), rel_err(labels[:, 63:], batch.labels[:, 63:])
    print(f"labels rel-err 3-D {e3:.2e} 2-D {e2:.2e}")
    assert e3 < 1e-6 and e2 < 1e-6
    got = plan.cpu().numpy()
    exp = np.array([[p["L"], p["T"], p["nw"], p["nh"], p["n"]] for p in batch.plans], dtype=np.float32)
    assert np.array_equal(got[:, 12:17], exp)
    assert np.array_equal(got[:, 17:20], np.stack([batch.params[:, 0], batch.params[:, 1], batch.params[:, 2]], 1))
    assert {int(v) for v in exp[:, 4]} >= {1, 2}          # the supersampled path is in the batch
    # the map itself: the oracle's sample points at the output's four corners
    A = got[:, :12].copy().view(np.float64)
    for i, p in enumerate(batch.plans):
        X, Y = AO.sample_points(p, 0, 0, p["n"])
        for oy, ox in ((0, 0), (0, 223), (223, 0), (223, 223)):
            pq = np.array([ox + 0.5 / p["n"], oy + 0.5 / p["n"], 1.0])
            assert abs(A[i, :3] @ pq - X[oy, ox]) < 1e-9 and abs(A[i, 3:] @ pq - Y[oy, ox]) < 1e-9, i
    # without normalize_3d the 3-D joints are only rotated
    lab_raw, _ = _plan(ops, batch, normalize_3d=False)
    exp_raw = np.stack([AO.labels_and_plan(batch.j2[i], batch.j3[i], W, H, batch.params[i, 0], batch.params[i, 3],
                                           norm3d=False)[0] for i in range(B)])
    assert rel_err(lab_raw[:, :63], exp_raw[:, :63]) < 1e-6 and rel_err(lab_raw[:, 63:], exp_raw[:, 63:]) < 1e-6


@pytest.mark.parametrize("hwc", [True, False])
def test_image_against_oracle(ops, batch, hwc):
    """random uint8 frames, all parameter combinations: 1e-5, the bar test_preprocess_u8 holds the same arithmetic to.  The
    kernel evaluates the map in fp64 and interpolates in fp32."""
    _, plan = _plan(ops, batch)
    src = torch.from_numpy(batch.frames if hwc else np.ascontiguousarray(batch.frames.transpose(0, 3, 1, 2))).to(DEV)
    out = ops.augment_warp_u8(src, plan, (224, 224), hwc=hwc)
    torch.cuda.synchronize()
    from scat_amd._lib import lib

    assert lib().scat_last_kernel() == (b"augment_warp_u8_hwc" if hwc else b"augment_warp_u8_chw")
    assert out.shape == (B, 3, 224, 224) and out.dtype == torch.float32
    got = out.cpu().numpy()
    worst = max(rel_err(got[i], batch.images[i]) for i in range(B))
    print(f"image rel-err, worst sample: {worst:.2e}")
    for i in range(B):
        assert rel_err(got[i], batch.images[i]) < 1e-5, (i, batch.params[i], batch.plans[i]["nw"])


def test_identity_plan_is_preprocess_u8(ops):
    """The identity plan on a 256 x 256 source is preprocess_u8's formula, and the two kernels agree to 1e-5, the bar
    test_preprocess_u8 holds that kernel to; a 224 x 224 window plan samples lattice points only and is src/127.5 - 1 on
    the window to 1e-6 (random bytes).

    The source of the first comparison is smooth (a slope of at most 7 grey levels per pixel), for a reason that is
    preprocess_u8's, not this kernel's: it forms (ox + .5) * (256/224) - .5 in fp32, where the rounded ratio is off by 5e-8
    (1.1e-5 of a pixel at ox = 223) and the product near 255 rounds to 8e-6 more, per axis.  On random bytes (steps of up
    to 2.0 between neighbours after normalisation) that alone is up to 4e-5 per axis.  Measured on an MI355X on the random
    source below: preprocess_u8 is 5.7e-5 from the fp64 evaluation of its own formula, this kernel 6e-7, the two 5.7e-5
    from each other, so no result can be within 1e-5 of both there.  The test therefore holds this kernel to 1e-5 of the
    fp64 formula on the random source, and to 1e-5 of preprocess_u8 where that kernel's coordinate rounding is worth at
    most 2 * 2e-5 pixel * 7/127.5 = 2e-6.  A slip of 1e-3 of a pixel in either convention still shows as 5e-5 there."""
    from scat_amd import synth
    from scat_amd.augment import pack_plan

    eye = [[1, 0, 0], [0, 1, 0]]
    plan = torch.from_numpy(np.stack([pack_plan(eye, 0, 0, 256, 256)] * 4)).to(DEV)
    assert plan[0, 16] == 1
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    ph = np.arange(12).reshape(4, 3, 1, 1) * 0.9
    smooth = torch.from_numpy(np.round(127.5 + 100 * np.sin(2 * np.pi * (xx / 113 + yy / 157) + ph)).astype(np.uint8))
    assert int((smooth[..., 1:].int() - smooth[..., :-1].int()).abs().max()) <= 7
    assert int((smooth[..., 1:, :].int() - smooth[..., :-1, :].int()).abs().max()) <= 7
    ref = ops.preprocess_u8(smooth.to(DEV))
    assert rel_err(ops.augment_warp_u8(smooth.to(DEV), plan, hwc=False), ref) < 1e-5
    assert rel_err(ops.augment_warp_u8(smooth.permute(0, 2, 3, 1).contiguous().to(DEV), plan, hwc=True), ref) < 1e-5

    u8 = torch.from_numpy(synth.randint_u8(3, "augment_identity", (4, 3, 256, 256)))
    hwc = u8.permute(0, 2, 3, 1).contiguous()
    exact = np.stack([AO.image(hwc[i].numpy(), 0, 0, 0, dict(M=np.array(eye, dtype=np.float64), L=0, T=0, nw=256, nh=256))
                      for i in range(4)])
    got, par = ops.augment_warp_u8(u8.to(DEV), plan, hwc=False), ops.preprocess_u8(u8.to(DEV))
    print(f"random source: warp vs fp64 {rel_err(got, exact):.2e}, preprocess_u8 vs fp64 {rel_err(par, exact):.2e}, "
          f"warp vs preprocess_u8 {rel_err(got, par):.2e}")
    assert rel_err(got, exact) < 1e-5
    assert rel_err(ops.augment_warp_u8(hwc.to(DEV), plan, hwc=True), exact) < 1e-5

    win = torch.from_numpy(np.stack([pack_plan(eye, 16, 16, 224, 224)] * 4)).to(DEV)
    exp = u8[:, :, 16:240, 16:240].float() / 127.5 - 1.0
    assert rel_err(ops.augment_warp_u8(u8.to(DEV), win, hwc=False), exp) < 1e-6
    assert rel_err(ops.augment_warp_u8(hwc.to(DEV), win, hwc=True), exp) < 1e-6


def test_wide_crops_use_the_3x3_and_4x4_grid(ops):
    """crops of 600-1000 pixels (n = 3 and 4, which hands of the seeded batch's size do not reach) from host-built plans,
    rotated, mirrored and blurred, partly outside the frame: 1e-5 against the oracle as above"""
    from scat_amd.augment import pack_plan

    rng = np.random.default_rng(29)
    j2, j3 = AO.seeded_joints(rng, 1, W, H)
    frames = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    cases = [(600, 33, 1, 0, 0), (672, 250, 0, 4, 1), (800, 0, 1, 7, 0), (1000, 117, 1, 10, 1)]   # nw, angle, flip, k, vert
    recs, exp = [], []
    for i, (nw, angle, flip, k, vert) in enumerate(cases):
        _, plan = AO.labels_and_plan(j2[0], j3[0], W, H, flip, angle)
        plan.update(L=plan["nW"] // 2 - nw // 2 + 3, T=plan["nH"] // 2 - nw // 2 - 5, nw=nw, nh=nw - 1, n=None)
        minv = np.linalg.inv(np.vstack([plan["M"], [0, 0, 1]]))[:2]
        recs.append(pack_plan(minv, plan["L"], plan["T"], plan["nw"], plan["nh"], flip=flip, k=k, vert=vert))
        exp.append(AO.image(frames[i], flip, k, vert, plan))
    assert [int(r[16]) for r in recs] == [3, 3, 4, 4]
    out = ops.augment_warp_u8(torch.from_numpy(frames).to(DEV), torch.from_numpy(np.stack(recs)).to(DEV), hwc=True)
    for i in range(4):
        assert rel_err(out[i], exp[i]) < 1e-5, cases[i]


def test_marker_lands_on_its_label(ops):
    """Geometry without trusting the formulas: a black frame with one 5 x 5 white marker centred on one integer-rounded
    joint, with flip, rotation and blur drawn; the intensity centroid of the output must lie within 4 (224/nw) + 1 output
    pixels, per axis, of that joint's entry in the device's labels.  In source space the reference's own quirks account
    for 1 pixel (W - x) and up to 1 across / 0.5 along the blur direction for an even k, which a rotation mixes into
    either axis (norm at most 2.3); on the canvas 0.5 from the un-rounded box origin and up to 1 from nw serving the y
    axis; each times the scale, plus 1 output pixel for the marker's discretisation.  Every sample counts: the marker's
    joint is chosen so that its label lies at least 4 scale + 6 pixels inside the 224 frame."""
    n = 48
    rng = np.random.default_rng(23)
    j2, j3 = AO.seeded_joints(rng, n, W, H)
    params = np.zeros((n, 4), dtype=np.int32)
    params[:, 0] = 1
    params[::7, 0] = 0
    frames = np.zeros((n, H, W, 3), dtype=np.uint8)
    chosen = []
    for i in range(n):
        if i % 4:
            params[i, 3] = int(rng.integers(1, 361))
        if i % 3 == 0:
            params[i, 1], params[i, 2] = int(rng.integers(1, 11)), int(rng.integers(0, 2))
        for q in [(i + d) % 21 for d in range(21)]:
            jj = j2[i].copy()
            jj[q] = np.round(jj[q])
            lab, plan = AO.labels_and_plan(jj, j3[i], W, H, params[i, 0], params[i, 3])
            scale = 224 / plan["nw"]
            lj = lab[63:].reshape(21, 2)[q]
            if lj.min() >= 4 * scale + 6 and lj.max() <= 224 - 4 * scale - 6:
                break
        else:
            raise AssertionError(f"test input: sample {i} has no joint whose label lies inside the frame")
        j2[i] = jj
        px = jj[q].astype(int)
        assert 2 <= px[0] < W - 2 and 2 <= px[1] < H - 2
        frames[i, px[1] - 2:px[1] + 3, px[0] - 2:px[0] + 3] = 255
        chosen.append((q, scale))
    assert len({q for q, _ in chosen}) > 5
    labels, plan = ops.augment_plan(torch.from_numpy(j2).to(DEV), torch.from_numpy(j3).to(DEV),
                                    torch.from_numpy(params).to(DEV), (W, H))
    out = ops.augment_warp_u8(torch.from_numpy(frames).to(DEV), plan, hwc=True).cpu().numpy().astype(np.float64)
    labels = labels.cpu().numpy()
    yy, xx = np.mgrid[0:224, 0:224]
    worst = 0.0
    for i, (q, scale) in enumerate(chosen):
        w = (out[i, 0] + 1) / 2
        tot = w.sum()
        assert tot > 1.0, f"sample {i}: the marker is not in the output"
        c = np.array([(w * xx).sum() / tot, (w * yy).sum() / tot])
        err = np.abs(c - labels[i, 63:].reshape(21, 2)[q]).max()
        worst = max(worst, err / (4 * scale + 1))
        assert err <= 4 * scale + 1, (i, params[i], scale, c, labels[i, 63:].reshape(21, 2)[q])
    print(f"marker centroid: worst error / bound {worst:.2f} over {n} samples")


def test_device_augment_feeds_train_step():
    """DeviceAugment(rotation, motion_blur) in front of TrainStep of the headline network, batch 8, two steps"""
    from scat_amd import synth
    from scat_amd.augment import DeviceAugment
    from scat_amd.models.hand_net import EncoderTransformer
    from scat_amd.trainer import TrainStep

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    seed, n = 5, 8
    opt = SimpleNamespace(vit_heads=8, pl_reg=True, iteration=3, pos_embed=True, mask_rate=0.2)
    net = EncoderTransformer(opt, T(synth.mean_params(seed)))
    net.load_state_dict(synth.to_torch(synth.encoder_transformer_state(seed, 8)), strict=True)
    ts = TrainStep(net.to(DEV).train())
    rng = np.random.default_rng(31)
    j2, j3 = AO.seeded_joints(rng, n, W, H)
    u8 = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(DEV)
    j2, j3 = torch.from_numpy(j2).to(DEV), torch.from_numpy(j3).to(DEV)
    aug = DeviceAugment(rotation=True, motion_blur=True)
    random.seed(7)
    x0, l0 = aug(u8, j2, j3)
    random.seed(7)
    x1, l1 = aug(u8, j2, j3)
    assert torch.equal(x0, x1) and torch.equal(l0, l1)
    random.seed(7)
    for _ in range(2):
        x, lab = aug(u8, j2, j3)
        assert x.shape == (n, 3, 224, 224) and x.dtype == torch.float32 and x.is_contiguous()
        assert lab.shape == (n, 105) and lab.dtype == torch.float32
        assert float(x.min()) >= -1.0 and float(x.max()) <= 1.0
        loss, parts, lpl, pred = ts(x, lab)
        assert torch.isfinite(loss).all() and torch.isfinite(pred).all()
    # CHW frames give the same batch
    random.seed(7)
    x2, l2 = aug(u8.permute(0, 3, 1, 2).contiguous(), j2, j3)
    assert torch.equal(x0, x2) and torch.equal(l0, l2)
