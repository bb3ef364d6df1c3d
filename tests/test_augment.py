"""Device augmentation, the part that needs no GPU: the random draws, argument validation through the built library,
and the oracle's own pixel conventions against PIL (an independent implementation of the mirror / crop / resize half)."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_oracle as AO  # noqa: E402


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


@pytest.mark.parametrize("rotation", [False, True])
@pytest.mark.parametrize("motion_blur", [False, True])
def test_draw_params_is_the_reference_sequence(rotation, motion_blur):
    from scat_amd.augment import draw_params

    B = 64
    random.seed(3)
    got = draw_params(B, rotation, motion_blur)
    state_got = random.getstate()
    random.seed(3)
    rows = AO.draw_sequence(B, rotation, motion_blur)
    state_ref = random.getstate()
    assert got.dtype == np.int32 and got.shape == (B, 4)
    ref = np.array([[1, k, int(choice == 0), angle] for k, choice, angle in rows], dtype=np.int32)
    assert np.array_equal(got, ref)
    assert state_got == state_ref
    if motion_blur:
        assert (got[:, 1] > 0).any() and (got[:, 1] == 0).any() and got[:, 1].max() <= 10
        assert set(got[got[:, 1] == 0, 2]) == {0}
    else:
        assert not got[:, 1:3].any()
    assert (got[:, 3] >= 1).all() and (got[:, 3] <= 360).all() if rotation else not got[:, 3].any()
    random.seed(3)
    assert not draw_params(4, rotation, motion_blur, flip=False)[:, 0].any()


def test_errors_surface_without_a_gpu(built):
    """argument validation of both entry points happens before any HIP call"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    with pytest.raises(ScatError, match="null pointer"):
        L.scat_augment_plan(0, 8, 8, 8, 8, 4, 640, 480, 1, 0)
    with pytest.raises(ScatError, match="must be positive"):
        L.scat_augment_plan(8, 8, 8, 8, 8, 0, 640, 480, 1, 0)
    with pytest.raises(ScatError, match="outside 11"):
        L.scat_augment_plan(8, 8, 8, 8, 8, 4, 640, 4, 1, 0)
    with pytest.raises(ScatError, match="normalize_3d"):
        L.scat_augment_plan(8, 8, 8, 8, 8, 4, 640, 480, 2, 0)
    with pytest.raises(ScatError, match="8-byte aligned"):
        L.scat_augment_plan(8, 8, 8, 8, 12, 4, 640, 480, 1, 0)
    with pytest.raises(ScatError, match="null pointer"):
        L.scat_augment_warp_u8(16, 0, 16, 4, 480, 640, 224, 224, 1, 0)
    with pytest.raises(ScatError, match="outside 1"):
        L.scat_augment_warp_u8(16, 16, 16, 0, 480, 640, 224, 224, 1, 0)
    with pytest.raises(ScatError, match="unsupported"):
        L.scat_augment_warp_u8(16, 16, 16, 4, 480, 640, 224, 192, 1, 0)
    with pytest.raises(ScatError, match="unsupported"):
        L.scat_augment_warp_u8(16, 16, 16, 4, 480, 640, 256, 256, 1, 0)
    with pytest.raises(ScatError, match="outside 11"):
        L.scat_augment_warp_u8(16, 16, 16, 4, 8, 640, 224, 224, 1, 0)
    with pytest.raises(ScatError, match="hwc"):
        L.scat_augment_warp_u8(16, 16, 16, 4, 480, 640, 224, 224, 3, 0)
    with pytest.raises(ScatError, match="aligned"):
        L.scat_augment_warp_u8(16, 16, 8, 4, 480, 640, 224, 224, 1, 0)


def test_ops_have_no_cpu_fallback():
    import torch

    from scat_amd import ops
    from scat_amd._lib import ScatError

    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.augment_plan(torch.zeros(2, 21, 2), torch.zeros(2, 21, 3), torch.zeros(2, 4, dtype=torch.int32), (640, 480))
    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.augment_warp_u8(torch.zeros(2, 480, 640, 3, dtype=torch.uint8), torch.zeros(2, ops.AUGMENT_PLAN_FLOATS))
    txt = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scat_amd", "augment.py")).read()
    assert "import oracle" not in txt and "from oracle" not in txt


def test_pack_plan_layout():
    """the host-built record has the layout the header documents: six fp64 map coefficients, then the box as floats"""
    from scat_amd import ops
    from scat_amd.augment import pack_plan

    rec = pack_plan([[1, 0, 0], [0, 1, 0]], 16, 16, 224, 224)
    assert rec.dtype == np.float32 and rec.shape == (ops.AUGMENT_PLAN_FLOATS,)
    assert np.array_equal(rec[:12].view(np.float64), [1, 0, 15.5, 0, 1, 15.5])
    assert list(rec[12:]) == [16, 16, 224, 224, 1, 0, 0, 0, 0, 0, 0, 0]
    assert pack_plan([[1, 0, 0], [0, 1, 0]], 0, 0, 600, 600)[16] == 3 and pack_plan(np.eye(3)[:2], 0, 0, 1000, 1000)[16] == 4


def _smooth_image(rng, W=640, H=480):
    """a few low-frequency waves per channel (period >= 24 pixels): smooth enough that PIL's uint8 rounding, not the
    resampling filter, dominates the difference"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(3):
            fx, fy = rng.uniform(-1, 1, 2) * 2 * np.pi / 24
            img[..., c] += rng.uniform(0.3, 1) * np.sin(fx * xx + fy * yy + rng.uniform(0, 6.28))
    img -= img.min()
    return np.round(img / img.max() * 255).astype(np.uint8)


def test_oracle_geometry_against_pil():
    """The oracle's flip-only samples against ImageOps.mirror + Image.crop + Image.resize(BILINEAR): six smooth 640 x 480
    images, seeded hands of extent 25-50 pixels whose crop boxes (112-172 pixels) lie inside the frame; the test asserts
    that, because at the black border PIL's crop-then-filter and the operator's single sample meet a discontinuity, which
    is not what this test is about.  It pins the pixel-centre convention u = L + (ox + .5) nw/224 - .5, the mirror as
    S(W-1-x) and PIL's half-to-even box rounding against an independent implementation.

    Differences expected by construction: PIL rounds its output to uint8 (a quarter of a step, 0.002, on average) and
    clamps at the crop's edge where the operator reads the neighbouring source pixel.  Measured with this file's seeded
    images (PIL 12.2): mean absolute difference 0.0023-0.0029, maximum 0.019-0.035 over the six.  The bounds are twice
    the worst of each: 0.0059 and 0.070.  Moving the oracle's L by half a source pixel gives means of 0.015-0.031 on the
    same images, 5 to 10 times the clean figure."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps

    rng = np.random.default_rng(11)
    j2s, j3s = AO.seeded_joints(rng, 6, ext=(25, 50))
    worst_mean = worst_max = 0.0
    for i in range(6):
        src = _smooth_image(rng)
        lab, plan = AO.labels_and_plan(j2s[i], j3s[i], 640, 480, 1, 0)
        l, t, r, b = plan["box"]
        assert l >= 0 and t >= 0 and r <= 640 and b <= 480, "test input: the crop must lie inside the frame"
        pil = ImageOps.mirror(Image.fromarray(src)).crop((l, t, r, b))        # load_STB.py:70, 85
        assert pil.size == (plan["nw"], plan["nh"])
        pil = np.asarray(pil.resize((224, 224), Image.BILINEAR), dtype=np.float64) / 127.5 - 1      # load_STB.py:88
        got = AO.image(src, 1, 0, 0, plan).transpose(1, 2, 0)
        d = np.abs(got - pil)
        print(f"sample {i}: crop {plan['nw']} n {plan['n']} mean |d| {d.mean():.5f} max |d| {d.max():.5f}")
        worst_mean, worst_max = max(worst_mean, d.mean()), max(worst_max, d.max())
    assert worst_mean < 0.0059 and worst_max < 0.070, (worst_mean, worst_max)


def test_pil_box_rounding():
    """Image.crop's size for fractional boxes is rint (half to even) of each coordinate, as the oracle assumes"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2)
    im = Image.new("RGB", (64, 48))
    for _ in range(300):
        l, t = rng.uniform(-30, 30, 2)
        s = rng.uniform(5, 40)
        box = [l, t, l + 2 * s, t + 2 * s]
        if rng.integers(0, 4) == 0:
            box = [np.floor(v) + 0.5 for v in box]       # exact ties
        L, T, R, B = (int(np.rint(v)) for v in box)
        assert im.crop(tuple(box)).size == (R - L, B - T), box
