"""Per-kernel parity on a real MI355X: every C-ABI op against the plain PyTorch fp32/fp64 CPU op
it replaces, on seeded inputs. Tolerance (norm-wise relative, max|a-b|/max|b|): 2e-5 for
contractions (fp32 fma chains in a different order), 1e-5 for element-wise / normalisation."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.util import rel_err
from scat_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"


def t(seed, name, shape, std=1.0):
    return torch.from_numpy(synth.normal_like(seed, name, shape, std))


def g(x):
    return x.to(DEV).contiguous()


@pytest.fixture
def math_mode(ops):
    """set the product mode for one test (0 fp32 MFMA, 1 bf16x3 split) and restore the default afterwards"""
    saved = ops.get_math_mode()
    yield ops.set_math_mode
    ops.set_math_mode(saved)


@pytest.fixture(scope="module")
def ops():
    from scat_amd import ops as o
    from scat_amd._lib import lib

    lib().scat_check_device()
    return o


# every distinct conv geometry of the ResNet-50 path + stem + 1x1 reduction
CONVS = [
    # Cin, Cout, k, s, p, H
    (3, 64, 7, 2, 3, 224), (64, 64, 1, 1, 0, 56), (64, 64, 3, 1, 1, 56), (64, 256, 1, 1, 0, 56),
    (256, 64, 1, 1, 0, 56), (256, 128, 1, 1, 0, 56), (128, 128, 3, 2, 1, 56), (128, 512, 1, 1, 0, 28),
    (256, 512, 1, 2, 0, 56), (512, 128, 1, 1, 0, 28), (128, 128, 3, 1, 1, 28), (512, 256, 1, 1, 0, 28),
    (256, 256, 3, 2, 1, 28), (256, 1024, 1, 1, 0, 14), (512, 1024, 1, 2, 0, 28), (1024, 256, 1, 1, 0, 14),
    (256, 256, 3, 1, 1, 14), (1024, 512, 1, 1, 0, 14), (512, 512, 3, 2, 1, 14), (512, 2048, 1, 1, 0, 7),
    (1024, 2048, 1, 2, 0, 14), (2048, 512, 1, 1, 0, 7), (512, 512, 3, 1, 1, 7), (512, 21, 1, 1, 0, 28),
]


@pytest.mark.parametrize("cin,cout,k,s,p,H", CONVS)
def test_conv_fwd_dgrad_wgrad(ops, cin, cout, k, s, p, H):
    B = 3 if H <= 56 else 2
    x = t(1, "x", (B, cin, H, H)).requires_grad_(True)
    w = t(2, "w", (cout, cin, k, k), std=(2.0 / (cin * k * k)) ** 0.5).requires_grad_(True)
    y = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    dy = t(3, "dy", tuple(y.shape))
    dx_ref, dw_ref = torch.autograd.grad(y, (x, w), dy.double())
    yg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), s, p)
    assert rel_err(yg, y) < 2e-5
    dwg = ops.conv2d_wgrad(g(dy), g(x.detach()), tuple(w.shape), s, p)
    assert rel_err(dwg, dw_ref) < 2e-5
    if k != 7:
        wt = ops.conv2d_wt(g(w.detach()))
        dxg = ops.conv2d_dgrad(g(dy), wt, tuple(x.shape), tuple(w.shape), s, p)
        assert rel_err(dxg, dx_ref) < 2e-5
        # accumulate form
        base = g(t(4, "acc", tuple(x.shape)))
        dxa = ops.conv2d_dgrad(g(dy), wt, tuple(x.shape), tuple(w.shape), s, p, out=base.clone(), accumulate=True)
        assert rel_err(dxa, dx_ref + base.cpu().double()) < 2e-5
        # from the original weights: stride-2 geometries take the parity-decomposed kernels
        dxw = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), s, p)
        assert rel_err(dxw, dx_ref) < 2e-5
        dxwa = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), s, p, out=base.clone(), accumulate=True)
        assert rel_err(dxwa, dx_ref + base.cpu().double()) < 2e-5


def test_conv_fused_input_transform(ops):
    """conv reading relu(x*scale+shift): zero padding must stay zero AFTER the transform."""
    B, cin, cout, H = 2, 32, 48, 14
    x = t(5, "x", (B, cin, H, H))
    w = t(6, "w", (cout, cin, 3, 3), std=0.1)
    sc = torch.from_numpy(synth.uniform(7, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(8, "sh", (cin,), -0.5, 0.5))
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    for s in (1, 2):
        y = F.conv2d(a.double(), w.double(), stride=s, padding=1)
        yg = ops.conv2d_fwd(g(x), g(w), s, 1, g(sc), g(sh), True)
        assert rel_err(yg, y) < 2e-5
        dy = t(9, "dy", tuple(y.shape))
        dw_ref = torch.nn.grad.conv2d_weight(a.double(), tuple(w.shape), dy.double(), stride=s, padding=1)
        dwg = ops.conv2d_wgrad(g(dy), g(x), tuple(w.shape), s, 1, g(sc), g(sh), True)
        assert rel_err(dwg, dw_ref) < 2e-5


@pytest.mark.parametrize("B,cin,cout,H,W,tf", [(3, 32, 32, 20, 56, False), (2, 64, 64, 9, 44, True), (5, 32, 64, 7, 40, True),
                                               (2, 64, 32, 5, 52, False), (4, 32, 32, 2, 64, True), (7, 64, 64, 3, 36, False)])
def test_wgrad3x3_rows(ops, B, cin, cout, H, W, tf):
    _wgrad3x3_rows(ops, B, cin, cout, H, W, tf)


ROWS64 = [(2, 64, 64, 9, 28, True), (3, 128, 64, 14, 14, False), (5, 64, 128, 7, 7, True), (2, 64, 64, 5, 32, False),
          (3, 128, 128, 3, 20, True), (4, 64, 64, 2, 12, False), (9, 64, 64, 7, 7, False)]


@pytest.mark.parametrize("B,cin,cout,H,W,tf", [(2, 128, 128, 9, 28, True), (3, 256, 256, 5, 14, False), (2, 128, 256, 3, 20, True)])
def test_wgrad3x3_rows64(ops, B, cin, cout, H, W, tf):
    """64 x 64 blocks on rows of at most 32 pixels (the shapes the default rule sends there); two rows per interval for
    W <= 16, rows that are not 16-byte multiples."""
    _wgrad3x3_rows(ops, B, cin, cout, H, W, tf)


def test_wgrad3x3_rows64_every_shape():
    """The same kernel forced onto the shapes the default rule leaves to the 128 x 128 kernel (SCAT_WG_ROWS=3, read once
    per process, hence the child): odd row counts, image boundaries inside a row pair, 7-pixel rows."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_ops as T\nfrom scat_amd import ops\n"
            "for a in T.ROWS64:\n    T._wgrad3x3_rows(ops, *a)\nprint('ROWS64 OK')\n") % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SCAT_WG_ROWS="3"), capture_output=True, text=True,
                       timeout=300, cwd=root)
    assert "ROWS64 OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def _wgrad3x3_rows(ops, B, cin, cout, H, W, tf):
    """The row-walking 3x3 weight gradient of the 32/64-channel layers (csrc/conv_wgrad_rows.hip): image borders,
    partial last octets (W % 8 == 4), three and four 16-pixel steps per row, workgroups whose row range starts / ends
    inside an image, fused input transform."""
    x = t(31, "x", (B, cin, H, W))
    dy = t(32, "dy", (B, cout, H, W))
    sc = torch.from_numpy(synth.uniform(33, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(34, "sh", (cin,), -0.5, 0.5))
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if tf else x
    dw_ref = torch.nn.grad.conv2d_weight(a.double(), (cout, cin, 3, 3), dy.double(), stride=1, padding=1)
    args = (g(sc), g(sh), True) if tf else ()
    dwg = ops.conv2d_wgrad(g(dy), g(x), (cout, cin, 3, 3), 1, 1, *args)
    assert ops.lib().scat_last_kernel().decode().startswith("wgrad3x3_rows"), ops.lib().scat_last_kernel()
    assert rel_err(dwg, dw_ref) < 2e-5


@pytest.mark.parametrize("H,W", [(13, 9), (8, 14), (7, 7)])
def test_dgrad_s2_odd_sizes(ops, H, W):
    """parity classes with ragged class grids (odd heights/widths)"""
    for cout in (20, 48):       # 48: multiple of 16 -> the split-operand taps kernel; 20 -> the fp32 engine
        for k, p in ((3, 1), (1, 0)):
            x = t(50, "x", (2, 12, H, W)).requires_grad_(True)
            w = t(51, "w", (cout, 12, k, k), std=0.2).requires_grad_(True)
            y = F.conv2d(x.double(), w.double(), stride=2, padding=p)
            dy = t(52, "dy", tuple(y.shape))
            (dx_ref,) = torch.autograd.grad(y, x, dy.double())
            assert rel_err(ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 2, p), dx_ref) < 2e-5
            base = g(t(53, "acc", tuple(x.shape)))
            got = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 2, p, out=base.clone(), accumulate=True)
            assert rel_err(got, dx_ref + base.cpu().double()) < 2e-5


@pytest.mark.parametrize("B,cin,cout,H,W", [(2, 20, 72, 9, 13), (1, 16, 200, 5, 63), (3, 36, 64, 7, 7),
                                             (2, 64, 132, 30, 4), (5, 128, 128, 14, 14), (3, 32, 32, 20, 24),
                                             (2, 48, 24, 11, 9)])
@pytest.mark.parametrize("math", [0, 1])
def test_conv3x3_halo(ops, math_mode, math, B, cin, cout, H, W):
    """3x3/s1/p1 LDS-halo kernel: ragged channel counts (C % 16 != 0, Cout % 64 != 0), tiles that straddle
    images, rows shorter than the pixel vector, the widest supported row; forward (+fused input transform)
    and data gradient (+accumulate) against fp64 torch and against the generic gather kernel."""
    assert ops.HALO
    math_mode(math)
    label = "conv3x3_split" if math else "conv3x3_halo"
    x = t(60, "x", (B, cin, H, W)).requires_grad_(True)
    w = t(61, "w", (cout, cin, 3, 3), std=(2.0 / (cin * 9)) ** 0.5).requires_grad_(True)
    y = F.conv2d(x.double(), w.double(), padding=1)
    dy = t(62, "dy", tuple(y.shape))
    (dx_ref,) = torch.autograd.grad(y, x, dy.double())
    yg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 1)
    assert ops.lib().scat_last_kernel().decode().startswith(label)
    assert rel_err(yg, y) < 2e-5
    dxg = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 1, 1)
    assert ops.lib().scat_last_kernel().decode().startswith(label)
    assert rel_err(dxg, dx_ref) < 2e-5
    base = g(t(63, "acc", tuple(x.shape)))
    dxa = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 1, 1, out=base.clone(), accumulate=True)
    assert rel_err(dxa, dx_ref + base.cpu().double()) < 2e-5
    sc = torch.from_numpy(synth.uniform(64, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(65, "sh", (cin,), -0.5, 0.5))
    a = F.relu(x.detach() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    yt = F.conv2d(a.double(), w.detach().double(), padding=1)
    ytg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 1, g(sc), g(sh), True)
    assert rel_err(ytg, yt) < 2e-5
    try:      # same answers as the generic gather path
        ops.HALO = False
        assert rel_err(ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 1, g(sc), g(sh), True), ytg.cpu()) < 2e-5
    finally:
        ops.HALO = True


@pytest.mark.parametrize("B,cout,H,W", [(2, 64, 224, 224), (3, 64, 38, 54), (1, 96, 32, 18), (2, 160, 16, 16),
                                        (3, 64, 30, 64), (5, 64, 22, 32)])
def test_stem_conv7x7_split(ops, math_mode, B, cout, H, W):
    """models/resnet.py:105: Conv2d(3, 64, 7, stride 2, padding 3) on the split-operand kernel (k-octet = 8 consecutive
    input pixels of one (kh, c)): left / right / top / bottom padding, ragged pixel tiles, more than one row tile,
    against fp64 torch and against the fp32 engine."""
    math_mode(1)
    x = t(90, "x", (B, 3, H, W))
    w = t(91, "w", (cout, 3, 7, 7), std=(2.0 / 147) ** 0.5)
    y = F.conv2d(x.double(), w.double(), stride=2, padding=3)
    yg = ops.conv2d_fwd(g(x), g(w), 2, 3)
    assert ops.lib().scat_last_kernel().decode().startswith("conv7x7_s2_split")
    assert rel_err(yg, y) < 2e-5
    try:
        ops.STEM_SPLIT = False
        y0 = ops.conv2d_fwd(g(x), g(w), 2, 3)
        assert not ops.lib().scat_last_kernel().decode().startswith("conv7x7_s2_split")
    finally:
        ops.STEM_SPLIT = True
    assert rel_err(yg, y0.cpu()) < 2e-5
    # its weight gradient (Cout = 64, output width a multiple of 16): rows in LDS, both operands split in registers
    if cout == 64 and (W // 2) % 16 == 0:
        dy = t(92, "dy", tuple(y.shape))
        xx, ww = x.double().requires_grad_(True), w.double().requires_grad_(True)
        (dw_ref,) = torch.autograd.grad(F.conv2d(xx, ww, stride=2, padding=3), ww, dy.double())
        dwg = ops.conv2d_wgrad(g(dy), g(x), tuple(w.shape), 2, 3)
        assert ops.lib().scat_last_kernel().decode().startswith("wgrad7x7_s2_split")
        assert rel_err(dwg, dw_ref) < 2e-5


@pytest.mark.parametrize("B,cin,cout,H,W", [(2, 48, 80, 9, 13), (1, 16, 208, 5, 64), (3, 32, 64, 7, 7),
                                             (2, 64, 144, 30, 4), (5, 256, 128, 14, 14)])
@pytest.mark.parametrize("math", [0, 1])
def test_conv1x1_pointwise(ops, monkeypatch, math_mode, math, B, cin, cout, H, W):
    """1x1/s1 weights-in-registers kernel: vector and scalar pixel staging (HW % 4), channel counts that are
    odd multiples of 16, ragged row/pixel tiles; forward (+bias, +fused input transform) and data gradient
    (+accumulate) against fp64 torch and against the generic gather kernel."""
    assert ops.PW
    monkeypatch.setattr(ops, "PW_MIN_C", 0)
    math_mode(math)
    label = "conv1x1_split" if math else "conv1x1_pw"
    x = t(70, "x", (B, cin, H, W)).requires_grad_(True)
    w = t(71, "w", (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5).requires_grad_(True)
    bias = t(72, "b", (cout,))
    y = F.conv2d(x.double(), w.double(), bias.double())
    dy = t(73, "dy", tuple(y.shape))
    (dx_ref,) = torch.autograd.grad(y, x, dy.double())
    yg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 0, bias=g(bias))
    assert ops.lib().scat_last_kernel().decode().startswith(label)
    assert rel_err(yg, y) < 2e-5
    dxg = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 1, 0)
    assert ops.lib().scat_last_kernel().decode().startswith(label)
    assert rel_err(dxg, dx_ref) < 2e-5
    base = g(t(74, "acc", tuple(x.shape)))
    dxa = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 1, 0, out=base.clone(), accumulate=True)
    assert rel_err(dxa, dx_ref + base.cpu().double()) < 2e-5
    sc = torch.from_numpy(synth.uniform(75, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(76, "sh", (cin,), -0.5, 0.5))
    a = F.relu(x.detach() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    yt = F.conv2d(a.double(), w.detach().double())
    ytg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 0, g(sc), g(sh), True)
    assert rel_err(ytg, yt) < 2e-5
    try:      # same answers as the generic gather path
        ops.PW = False
        assert rel_err(ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 0, g(sc), g(sh), True), ytg.cpu()) < 2e-5
    finally:
        ops.PW = True


def test_split_products_are_as_accurate_as_fp32(ops, math_mode):
    """The bf16x3 split (six bf16 MFMA terms per product) must not be a precision downgrade: against an fp64
    reference its error is within a small factor of the fp32-MFMA kernel's own rounding error, on well-scaled
    data, on data with a 2^20 dynamic range inside every dot product, and far inside the 2e-5 gate."""
    B, cin, cout, H = 4, 256, 128, 14
    for name, spread in (("unit", 0.0), ("wide", 20.0)):
        x = t(90, "x" + name, (B, cin, H, H))
        w = t(91, "w" + name, (cout, cin, 3, 3), std=(2.0 / (cin * 9)) ** 0.5)
        if spread:
            x = x * torch.exp2(torch.from_numpy(synth.uniform(92, "e", tuple(x.shape), -spread / 2, spread / 2)))
        y = F.conv2d(x.double(), w.double(), padding=1)
        errs = {}
        for mode in (0, 1):
            math_mode(mode)
            yg = ops.conv2d_fwd(g(x), g(w), 1, 1).cpu().double()
            errs[mode] = ((yg - y).abs().max() / y.abs().max()).item(), ((yg - y).norm() / y.norm()).item()
        assert errs[1][0] < 2e-5 and errs[0][0] < 2e-5, errs                  # the op-level gate, both modes
        assert errs[1][1] < 1.5 * errs[0][1] + 1e-8, errs                     # split is no less accurate than fp32 MFMA
        assert errs[1][0] < 1.5 * errs[0][0] + 1e-8, errs


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("B,cin,cout,H,W,k", [(2, 20, 136, 9, 13, 3), (3, 36, 64, 7, 7, 3), (2, 64, 132, 30, 4, 3),
                                               (5, 128, 128, 14, 14, 3), (2, 144, 136, 9, 13, 1), (3, 160, 112, 7, 7, 1),
                                               (1, 96, 208, 5, 64, 1), (4, 3, 5, 6, 5, 3), (2, 40, 48, 9, 13, 1),
                                               (6, 72, 32, 28, 28, 3), (1, 32, 64, 5, 64, 1), (3, 64, 64, 56, 56, 1)])
def test_wgrad_stride1(ops, math_mode, math, B, cin, cout, H, W, k):
    """weight gradient of 1x1/pad 0 and 3x3/pad 1: planes that are not a multiple of 8 pixels (ragged octets), rows
    shorter than an octet (taps wrap inside a vector, first/last vectors poke outside the tensor), ragged
    row/column tiles, with and without the fused input transform; both product modes."""
    math_mode(math)
    x = t(80, "x", (B, cin, H, W))
    w_shape = (cout, cin, k, k)
    dy = t(81, "dy", (B, cout, H, W))
    sc = torch.from_numpy(synth.uniform(82, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(83, "sh", (cin,), -0.5, 0.5))
    for tf in (False, True):
        a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if tf else x
        ref = torch.nn.grad.conv2d_weight(a.double(), w_shape, dy.double(), padding=k // 2)
        got = ops.conv2d_wgrad(g(dy), g(x), w_shape, 1, k // 2, *((g(sc), g(sh), True) if tf else ()))
        assert ("_split_" in ops.lib().scat_last_kernel().decode()) == bool(math)
        assert rel_err(got, ref) < 2e-5, tf


@pytest.mark.parametrize("B,cin,cout,H,W,k", [(2, 32, 72, 9, 13, 3), (3, 48, 64, 7, 7, 3), (2, 64, 136, 30, 5, 1),
                                               (4, 16, 40, 14, 14, 3), (1, 80, 200, 11, 6, 1)])
def test_conv_stride2_split(ops, B, cin, cout, H, W, k):
    """stride-2 forward on the taps kernel (contraction ordered tap-major): odd and even planes, channel counts that
    are odd multiples of 16, ragged tiles, bias, fused input transform (padding must stay zero after it)."""
    assert ops.get_math_mode() == 1
    x = t(95, "x", (B, cin, H, W))
    w = t(96, "w", (cout, cin, k, k), std=(2.0 / (cin * k * k)) ** 0.5)
    bias = t(97, "b", (cout,))
    y = F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=k // 2)
    yg = ops.conv2d_fwd(g(x), g(w), 2, k // 2, bias=g(bias))
    assert "_split_" in ops.lib().scat_last_kernel().decode()
    assert rel_err(yg, y) < 2e-5
    sc = torch.from_numpy(synth.uniform(98, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(99, "sh", (cin,), 0.1, 0.6))     # positive shift: relu(0*s+t) != 0 on padding
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    yt = F.conv2d(a.double(), w.double(), stride=2, padding=k // 2)
    assert rel_err(ops.conv2d_fwd(g(x), g(w), 2, k // 2, g(sc), g(sh), True), yt) < 2e-5


@pytest.mark.parametrize("B,cin,cout,H,W,k", [(2, 20, 136, 9, 13, 3), (3, 36, 64, 7, 7, 3), (2, 144, 136, 8, 14, 1),
                                               (5, 128, 128, 14, 14, 3), (1, 96, 208, 5, 63, 1)])
def test_wgrad_stride2_split(ops, B, cin, cout, H, W, k):
    """weight gradient of the stride-2 convolutions on the split-operand kernel (strided source gather)."""
    assert ops.get_math_mode() == 1
    x = t(84, "x", (B, cin, H, W))
    w_shape = (cout, cin, k, k)
    OH, OW = ops.conv_out_hw(H, W, k, 2, k // 2)
    dy = t(85, "dy", (B, cout, OH, OW))
    sc = torch.from_numpy(synth.uniform(86, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(87, "sh", (cin,), 0.1, 0.6))
    for tf in (False, True):
        a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if tf else x
        ref = torch.nn.grad.conv2d_weight(a.double(), w_shape, dy.double(), stride=2, padding=k // 2)
        got = ops.conv2d_wgrad(g(dy), g(x), w_shape, 2, k // 2, *((g(sc), g(sh), True) if tf else ()))
        assert ("_s2_split_" in ops.lib().scat_last_kernel().decode()) == (k == 3)   # 1x1/s2 stays on the fp32 engine
        assert rel_err(got, ref) < 2e-5, tf


def test_prepared_weights(ops):
    """ops.WeightPrep (scat_wprep_jobs / scat_wprep_run): after one registering pass, a single batched launch re-lays
    the weights of every (convolution, direction) and the entry points run with w_ready = 1 — results must be
    BIT-identical to the self-preparing calls, for all six kinds, and must follow an in-place weight update."""
    assert ops.get_math_mode() == 1
    B = 2
    cases = [  # cin, cout, k, stride, H
        (32, 48, 1, 1, 9), (48, 32, 3, 1, 10), (32, 64, 3, 2, 11), (64, 32, 1, 2, 12), (16, 80, 3, 2, 8)]
    ws, xs, dys = [], [], []
    for n, (cin, cout, k, s, H) in enumerate(cases):
        ws.append(g(t(300 + n, "w", (cout, cin, k, k), std=0.1)))
        xs.append(g(t(310 + n, "x", (B, cin, H, H))))
        OH, _ = ops.conv_out_hw(H, H, k, s, k // 2)
        dys.append(g(t(320 + n, "dy", (B, cout, OH, OH))))

    def run_all(wp):
        outs = []
        for (cin, cout, k, s, H), w, x, dy in zip(cases, ws, xs, dys):
            outs.append(ops.conv2d_fwd(x, w, s, k // 2, wp=wp))
            outs.append(ops.conv2d_dgrad_w(dy, w, tuple(x.shape), s, k // 2, wp=wp))
        return outs

    ref = run_all(None)
    wp = ops.WeightPrep()
    wp.run(False)                                   # nothing registered yet: no-op
    first = run_all(wp)                             # registers; every call still prepares for itself
    assert len(wp.entries) == 2 * len(cases) and not any(e[2] for e in wp.entries.values())
    wp.run(False)                                   # builds the table, one launch
    assert wp.table is not None and all(e[2] for e in wp.entries.values())
    kinds = sorted({k for _, k in wp.entries})
    assert kinds == [0, 1, 2, 3, 4, 5], kinds
    for e in wp.entries.values():                   # poison check: run() must have rewritten every workspace
        assert e[2]
    second = run_all(wp)                            # w_ready = 1 everywhere
    for a, b, c in zip(ref, first, second):
        assert torch.equal(a, b) and torch.equal(a, c)
    # stale detection in inference mode: an in-place update bumps the version counter -> run() re-lays
    with torch.no_grad():
        for w in ws:
            w.mul_(1.5)
    wp.run(False)
    third = run_all(wp)
    ref2 = run_all(None)
    for a, b in zip(ref2, third):
        assert torch.equal(a, b)
    assert not torch.equal(ref[0], ref2[0])
    # a training-mode run marks the cache dirty (the optimiser's update is invisible): next inference run re-lays
    wp.run(True)
    assert wp.dirty
    wp.run(False)
    assert not wp.dirty


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 5, 7, 9), (1, 2, 14, 14), (2, 4, 5, 12), (1, 1, 1, 1)])
def test_subsample2(ops, shape):
    """x[:, :, ::2, ::2] packed: even/odd planes, vector and scalar paths; bit-exact (a copy)."""
    x = t(98, "x", shape)
    assert torch.equal(ops.subsample2(g(x)).cpu(), x[:, :, ::2, ::2].contiguous())


def test_conv_bias_and_edge_batches(ops):
    for B in (1, 5):
        x = t(10, "x", (B, 20, 9, 9))
        w = t(11, "w", (130, 20, 1, 1), std=0.2)
        b = t(12, "b", (130,))
        y = F.conv2d(x.double(), w.double(), b.double())
        assert rel_err(ops.conv2d_fwd(g(x), g(w), 1, 0, bias=g(b)), y) < 2e-5


@pytest.mark.parametrize("M,N,K", [(2016, 1536, 784), (2016, 784, 512), (84, 588, 784), (84, 3, 147),
                                   (96, 1024, 2048), (2016, 196, 294), (7, 66, 1090), (300, 200, 100)])
def test_linear(ops, M, N, K):
    """(the largest shape, 2016 x 1536 x 784, runs on scat_gemm_split in the default product mode, the others on the
    fp32 engine: ops.GEMM_SPLIT_MIN)"""
    x = t(13, "x", (M, K)).requires_grad_(True)
    w = t(14, "w", (N, K), std=K ** -0.5).requires_grad_(True)
    b = t(15, "b", (N,))
    y = F.linear(x.double(), w.double(), b.double())
    dy = t(16, "dy", (M, N))
    dx_ref, dw_ref = torch.autograd.grad(y, (x, w), dy.double())
    assert rel_err(ops.linear_fwd(g(x.detach()), g(w.detach()), g(b)), y) < 2e-5
    assert rel_err(ops.linear_dgrad(g(dy), g(w.detach())), dx_ref) < 2e-5
    assert rel_err(ops.linear_wgrad(g(dy), g(x.detach())), dw_ref) < 2e-5
    assert rel_err(ops.colsum(g(dy)), dy.double().sum(0)) < 1e-5


@pytest.mark.parametrize("M,N,K", [(2016, 1536, 392), (2016, 196, 512), (2016, 294, 392), (300, 200, 147),
                                   (130, 70, 66), (2016, 1536, 196)])
def test_gemm_split(ops, M, N, K):
    """scat_gemm_split directly: contraction lengths that are not multiples of 16 or 32 (392, 196, 147, 66), ragged row
    and column tiles, transposed A, bias and accumulate — the ViT projection shapes of layers 1 and 2."""
    assert ops.get_math_mode() == 1
    a = t(600, "a", (M, K))
    b = t(601, "b", (K, N), std=K ** -0.5)
    bias = t(602, "bias", (N,))
    ref = a.double() @ b.double()
    c = ops.gemm_split(g(a), 0, g(b), torch.empty(M, N, device="cuda"), M, N, K, g(bias))
    assert "gemm_split" in ops.lib().scat_last_kernel().decode()
    assert rel_err(c, ref + bias.double()) < 2e-5
    at = g(a.t().contiguous())                                   # stored [K][M]
    base = g(t(603, "base", (M, N)))
    c2 = ops.gemm_split(at, 1, g(b), base.clone(), M, N, K, None, accumulate=True)
    assert rel_err(c2, ref + base.double().cpu()) < 2e-5


@pytest.mark.parametrize("B,C,H", [(4, 64, 56), (3, 256, 14), (5, 2048, 7), (2, 64, 112)])
def test_batchnorm(ops, B, C, H):
    x = (t(17, "x", (B, C, H, H)) * 1.7 + 0.4).requires_grad_(True)
    gamma = torch.from_numpy(synth.uniform(18, "g", (C,), 0.5, 1.5)).requires_grad_(True)
    beta = torch.from_numpy(synth.uniform(19, "b", (C,), -0.3, 0.3)).requires_grad_(True)
    rm = torch.from_numpy(synth.uniform(20, "rm", (C,), -0.2, 0.2))
    rv = torch.from_numpy(synth.uniform(21, "rv", (C,), 0.6, 1.4))
    res = t(22, "res", (B, C, H, H))
    rm_ref, rv_ref = rm.clone(), rv.clone()
    y = F.relu(F.batch_norm(x, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5) + res)
    dy = t(23, "dy", (B, C, H, H))
    dx_ref, dg_ref, db_ref = torch.autograd.grad(y, (x, gamma, beta), dy)
    xg, gg, bg, rmg, rvg = g(x.detach()), g(gamma.detach()), g(beta.detach()), g(rm), g(rv)
    mean, invstd, scale, shift = ops.bn_train_stats(xg, gg, bg, rmg, rvg)
    assert rel_err(rmg, rm_ref) < 1e-5 and rel_err(rvg, rv_ref) < 1e-5
    yg = ops.bn_apply(xg, scale, shift, g(res), relu=True)
    assert rel_err(yg, y) < 1e-5
    dres = torch.empty_like(xg)
    dxg, dgg, dbg = ops.bn_bwd(g(dy), xg, yg, True, scale, shift, mean, invstd, gg, dres=dres)
    assert rel_err(dxg, dx_ref) < 2e-5 and rel_err(dgg, dg_ref) < 2e-5 and rel_err(dbg, db_ref) < 2e-5
    assert rel_err(dres, dy * (y > 0)) < 1e-6
    # recomputed-mask form (no residual): y = relu(bn(x))
    y2 = F.relu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, 1e-5))
    dx2, dg2, db2 = torch.autograd.grad(y2, (x, gamma, beta), dy)
    dxg2, dgg2, dbg2 = ops.bn_bwd(g(dy), xg, None, True, scale, shift, mean, invstd, gg)
    assert rel_err(dxg2, dx2) < 2e-5 and rel_err(dgg2, dg2) < 2e-5 and rel_err(dbg2, db2) < 2e-5
    # eval fold
    sc_e, sh_e = ops.bn_eval_fold(gg, bg, rmg, rvg)
    ye = F.batch_norm(x.detach(), rm_ref, rv_ref, gamma.detach(), beta.detach(), False, 0.1, 1e-5)
    assert rel_err(ops.bn_apply(xg, sc_e, sh_e), ye) < 1e-5


@pytest.mark.timeout(900)
@pytest.mark.parametrize("C,H", [(256, 56), (512, 28)])
def test_batchnorm_backward_batch96(ops, C, H):
    """The BatchNorm-backward grids of a batch-96 step (VERDICT r03 "Next" item 2): bn_bwd and bn_bwd_pre on
    (96, 256, 56, 56) and (96, 512, 28, 28) — bn_bwd_reduce_g_kernel's largest launch is reached by no smaller test —
    against fp64 torch autograd of relu(batch_norm(x) + res): dx (materialised, and as formed from bn_bwd_pre's three
    per-channel constants), dgamma, dbeta, the masked residual gradient."""
    B = 96
    gen = torch.Generator().manual_seed(900 + C)
    x = torch.randn((B, C, H, H), generator=gen) * 1.7 + 0.4
    res = torch.randn((B, C, H, H), generator=gen)
    dy = torch.randn((B, C, H, H), generator=gen)
    gamma = torch.from_numpy(synth.uniform(18, "g", (C,), 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform(19, "b", (C,), -0.3, 0.3))
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.relu(F.batch_norm(xd, None, None, gd, bd, True, 0.1, 1e-5) + res.double())
    dx_ref, dg_ref, db_ref = torch.autograd.grad(y, (xd, gd, bd), dy.double())
    dres_ref = (dy.double() * (y > 0)).float()
    del y
    xg, gg, bg = g(x), g(gamma), g(beta)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd, scale, shift = ops.bn_train_stats(xg, gg, bg, rm, rv)
    yg, mask = ops.bn_apply(xg, scale, shift, g(res), True, want_mask=True)
    dres = torch.empty_like(xg)
    dxg, dgg, dbg = ops.bn_bwd(g(dy), xg, None, True, scale, shift, mean, invstd, gg, dres=dres, y_mask=mask)
    assert rel_err(dxg, dx_ref) < 2e-5 and rel_err(dgg, dg_ref) < 2e-5 and rel_err(dbg, db_ref) < 2e-5
    assert rel_err(dres, dres_ref) < 1e-6
    del dxg, dres
    gbuf = g(dy)
    coef3, dg2, db2 = ops.bn_bwd_pre(gbuf, xg, True, scale, shift, mean, invstd, gg, y_mask=mask)
    assert rel_err(gbuf, dres_ref) < 1e-6
    assert rel_err(dg2, dg_ref) < 2e-5 and rel_err(db2, db_ref) < 2e-5
    gbuf.mul_(coef3[0].view(1, -1, 1, 1)).addcmul_(xg, coef3[1].view(1, -1, 1, 1)).add_(coef3[2].view(1, -1, 1, 1))
    assert rel_err(gbuf, dx_ref) < 2e-5


@pytest.mark.parametrize("B,cin,cout,k,s,p,H,W", [(3, 64, 256, 1, 1, 0, 28, 28), (2, 128, 64, 1, 1, 0, 13, 9),
                                                   (3, 64, 64, 3, 1, 1, 20, 24), (2, 32, 32, 3, 1, 1, 11, 9),
                                                   (2, 128, 128, 3, 2, 1, 28, 28), (2, 3, 64, 7, 2, 3, 64, 96),
                                                   (5, 256, 96, 1, 1, 0, 7, 7), (2, 64, 128, 1, 2, 0, 14, 14)])
def test_conv_epilogue_batchnorm_statistics(ops, B, cin, cout, k, s, p, H, W):
    """conv2d_fwd(stats=True): the kernel leaves per-tile channel sums of its output behind and bn_train_stats finishes
    from them — same mean / invstd / scale / shift / running statistics as the pass over the output (and as torch),
    ragged last tiles and dead columns included."""
    x = t(61, "x", (B, cin, H, W)) * 1.3 + 0.2
    w = t(62, "w", (cout, cin, k, k), std=(2.0 / (cin * k * k)) ** 0.5)
    gamma = torch.from_numpy(synth.uniform(63, "g", (cout,), 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform(64, "b", (cout,), -0.3, 0.3))
    y_ref = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    rm_ref, rv_ref = torch.zeros(cout, dtype=torch.float64), torch.ones(cout, dtype=torch.float64)
    F.batch_norm(y_ref, rm_ref, rv_ref, gamma.double(), beta.double(), True, 0.1, 1e-5)
    mean_ref = y_ref.mean(dim=(0, 2, 3))
    invstd_ref = 1.0 / torch.sqrt(y_ref.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    y = ops.conv2d_fwd(g(x), g(w), s, p, stats=True)
    assert getattr(y, "scat_stats", None) is not None, ops.lib().scat_last_kernel()
    assert rel_err(y, y_ref) < 2e-5
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    mean, invstd, scale, shift = ops.bn_train_stats(y, g(gamma), g(beta), rm, rv)
    assert y.scat_stats is None                      # consumed
    rm2, rv2 = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    mean2, invstd2, scale2, shift2 = ops.bn_train_stats(y, g(gamma), g(beta), rm2, rv2)      # the pass over y
    for a, b, ref in ((mean, mean2, mean_ref), (invstd, invstd2, invstd_ref), (rm, rm2, rm_ref), (rv, rv2, rv_ref)):
        assert rel_err(a, ref) < 2e-5 and rel_err(a, b.cpu()) < 2e-6
    assert rel_err(scale, scale2.cpu()) < 2e-6 and rel_err(shift, shift2.cpu()) < 2e-5


@pytest.mark.parametrize("k,cin,cout,H", [(1, 64, 256, 28), (3, 64, 64, 28)])
def test_conv_epilogue_statistics_with_large_channel_offsets(ops, k, cin, cout, H):
    """the epilogue leaves fp32 sums of x and x^2 over 32..128 pixels; with |mean| ~ 100 sigma (an input
    with a DC level) the variance E[x^2] - mean^2 formed from them has lost four digits.  Taken about a per-channel
    reference (``stats_shift``: in the network the previous step's batch mean) the sums are of (x - c), (x - c)^2 and
    the statistics are as accurate as the fp64 pass over the output again."""
    B = 8
    gen = torch.Generator().manual_seed(77 + k)
    x = 1.0 + 0.01 * torch.randn((B, cin, H, H), generator=gen)
    w = torch.randn((cout, cin, k, k), generator=gen) * (1.0 / (cin * k * k)) ** 0.5
    y_ref = F.conv2d(x.double(), w.double(), padding=k // 2)
    inner = y_ref[:, :, 2:-2, 2:-2]                                   # (the offset/sigma ratio away from the zero padding)
    assert float((inner.mean(dim=(0, 2, 3)).abs() / inner.std(dim=(0, 2, 3))).median()) > 30
    mean_ref = y_ref.mean(dim=(0, 2, 3))
    invstd_ref = 1.0 / torch.sqrt(y_ref.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    ones, zeros = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)

    def run(shift):
        y = ops.conv2d_fwd(g(x), g(w), 1, k // 2, stats=True, stats_shift=shift)
        assert getattr(y, "scat_stats", None) is not None
        mean, invstd, _, _ = ops.bn_train_stats(y, ones, zeros, zeros.clone(), ones.clone())
        return rel_err(mean, mean_ref), rel_err(invstd, invstd_ref)

    e_plain = run(None)
    ref = g(mean_ref.float() * (1.0 + 1e-3))                          # "last step's mean": close to, not equal to, this one
    e_ref = run(ref)
    assert e_ref[0] < 2e-6 and e_ref[1] < 2e-5, (e_ref, e_plain)
    if k == 1:                                                         # (no padding: every pixel carries the offset)
        assert e_plain[1] > 10 * e_ref[1], (e_ref, e_plain)           # the reference is what makes the difference


# the small shapes of tests/test_gpu_guard.py conv_epilogue_stats: ragged last tiles on the pointwise and the halo kernel
EPI_PW, EPI_3X3 = (2, 128, 64, 1, 13, 9), (2, 32, 32, 3, 11, 9)


def _epi_conv(ops, shape, seed, bias=None, sentinel=-7.5):
    """one forward convolution at the C level with a ScatEpilogue over the test's own partials buffer
    -> (y, fp64 reference of the convolution without bias, the descriptor, the partials pre-filled with ``sentinel``)"""
    import ctypes

    L, P = ops.lib(), (lambda a: 0 if a is None else a.data_ptr())
    B, cin, cout, k, H, W = shape
    x = t(seed, "x", (B, cin, H, W)) * 1.3 + 0.2
    w = t(seed + 1, "w", (cout, cin, k, k), std=(2.0 / (cin * k * k)) ** 0.5)
    xg, wg, y = g(x), g(w), torch.empty((B, cout, H, W), device=DEV)
    part = torch.full((cout * ((B * H * W + 31) // 32 + 4) * 2,), sentinel, device=DEV)
    epi = ops._Epilogue(P(part), part.numel() * 4, 77)
    if k == 1:
        ws = torch.empty(L.scat_conv1x1_s1_ws(cout, cin), dtype=torch.uint8, device=DEV)
        L.scat_conv1x1_s1(P(xg), P(wg), P(y), B, cin, H * W, cout, 0, P(bias), 0, 0, 0, 0, P(ws), ws.numel(), 0,
                          ctypes.addressof(epi), ops._stream())
    else:
        ws = torch.empty(L.scat_conv3x3_s1_ws(cout, cin), dtype=torch.uint8, device=DEV)
        L.scat_conv3x3_s1(P(xg), P(wg), P(y), B, cin, H, W, cout, 0, 0, 0, 0, 0, P(ws), ws.numel(), 0,
                          ctypes.addressof(epi), ops._stream())
    return y, F.conv2d(x.double(), w.double(), padding=k // 2), epi, part


def test_an_epilogue_request_belongs_to_its_call(ops, math_mode):
    """Two convolutions, each with its own ScatEpilogue, then a contraction that offers none (scat_gemm_split: a
    non-accumulating, bias-less launch of the same kernel family), then the two sets of statistics finished in the
    reverse order: each request was served by its own call, and the contraction in between touched neither buffer."""
    math_mode(1)
    L, P = ops.lib(), (lambda a: a.data_ptr())
    ya, ra, ea, pa = _epi_conv(ops, EPI_PW, 81)
    yb, rb, eb, pb = _epi_conv(ops, EPI_3X3, 83)
    assert ea.groups > 0 and eb.groups > 0, (ea.groups, eb.groups)
    before = (pa.clone(), pb.clone())
    a, b, c = g(t(85, "a", (64, 64))), g(t(86, "b", (64, 64))), torch.empty((64, 64), device=DEV)
    ws = torch.empty(L.scat_gemm_split_ws(64, 64), dtype=torch.uint8, device=DEV)
    L.scat_gemm_split(P(a), 0, P(b), P(c), 64, 64, 64, 0, 0, P(ws), ws.numel(), ops._stream())
    assert rel_err(c, t(85, "a", (64, 64)).double() @ t(86, "b", (64, 64)).double()) < 2e-5
    assert torch.equal(pa, before[0]) and torch.equal(pb, before[1])
    for (B, _, cout, _, H, W), y, ref, epi, part in ((EPI_3X3, yb, rb, eb, pb), (EPI_PW, ya, ra, ea, pa)):
        assert rel_err(y, ref) < 2e-5
        gamma, beta, rm, rv = (torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV),
                               torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV))
        o = torch.empty((4, cout), device=DEV)
        L.scat_bn_train_stats_partials(P(part), epi.groups, B, cout, H * W, P(gamma), P(beta), P(rm), P(rv), 0.1, 1e-5,
                                       P(o[0]), P(o[1]), P(o[2]), P(o[3]), ops._stream())
        e_mean = rel_err(o[0], ref.mean(dim=(0, 2, 3)))
        e_invstd = rel_err(o[1], 1.0 / torch.sqrt(ref.var(dim=(0, 2, 3), unbiased=False) + 1e-5))
        print(f"epilogue request k{3 if H == 11 else 1}: groups {epi.groups} mean {e_mean:.2e} invstd {e_invstd:.2e}")
        assert e_mean < 2e-5 and e_invstd < 2e-5


def test_a_convolution_with_bias_leaves_an_epilogue_request_alone(ops, math_mode):
    """the sums would be those of y - bias: the call reports 0 groups and does not touch the partials"""
    math_mode(1)
    bias = t(88, "bias", (EPI_PW[2],))
    y, ref, epi, part = _epi_conv(ops, EPI_PW, 81, bias=g(bias), sentinel=-7.5)
    assert epi.groups == 0
    assert bool((part == -7.5).all())
    assert rel_err(y, ref + bias.double().view(1, -1, 1, 1)) < 2e-5


def test_batchnorm_sign_mask(ops):
    """bn_bwd from the 1-bit sign mask of the block output == bn_bwd from the output itself, bit for bit."""
    B, C, H = 3, 64, 28
    x, res, dy = (g(t(30 + i, n, (B, C, H, H))) for i, n in enumerate(("x", "res", "dy")))
    gamma = g(torch.from_numpy(synth.uniform(33, "g", (C,), 0.5, 1.5)))
    beta = g(t(34, "b", (C,), 0.1))
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd, scale, shift = ops.bn_train_stats(x, gamma, beta, rm, rv)
    y, mask = ops.bn_apply(x, scale, shift, res, True, want_mask=True)
    assert mask is not None and mask.dtype == torch.uint8 and mask.numel() == y.numel() // 4
    bits = ((mask.view(-1, 1) >> torch.arange(4, device=DEV, dtype=torch.uint8)) & 1).bool().view_as(y)
    assert torch.equal(bits, y > 0)
    a = ops.bn_bwd(dy, x, y, True, scale, shift, mean, invstd, gamma, dres=torch.empty_like(dy))
    dres_a = torch.empty_like(dy)
    a = ops.bn_bwd(dy, x, y, True, scale, shift, mean, invstd, gamma, dres=dres_a)
    dres_b = torch.empty_like(dy)
    b = ops.bn_bwd(dy, x, None, True, scale, shift, mean, invstd, gamma, dres=dres_b, y_mask=mask)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(dres_a, dres_b)


@pytest.mark.parametrize("B,cin,cout,H", [(3, 64, 256, 12), (2, 128, 512, 8), (5, 32, 48, 6)])
def test_batchnorm_backward_folded_into_conv(ops, B, cin, cout, H):
    """bn_bwd_pre + conv1x1_{dgrad,wgrad}_bnb (the BatchNorm backward's apply formed inside the conv's gradient
    kernels, dx never materialised) == bn_bwd followed by the plain gradient kernels."""
    assert ops.get_math_mode() == 1
    z, res, dy = (g(t(40 + i, n, (B, cout, H, H))) for i, n in enumerate(("z", "res", "dy")))   # z: conv3's raw output
    a2 = g(t(43, "a2", (B, cin, H, H)))                                                         # conv3's raw input
    w = g(t(44, "w", (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5))
    gamma = g(torch.from_numpy(synth.uniform(45, "g", (cout,), 0.5, 1.5)))
    beta = g(t(46, "b", (cout,), 0.1))
    sc2 = g(torch.from_numpy(synth.uniform(47, "sc", (cin,), 0.5, 1.5)))
    sh2 = g(torch.from_numpy(synth.uniform(48, "sh", (cin,), -0.5, 0.5)))
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    mean, invstd, scale, shift = ops.bn_train_stats(z, gamma, beta, rm, rv)
    y, mask = ops.bn_apply(z, scale, shift, res, True, want_mask=True)
    # reference composition
    dres_ref = torch.empty_like(dy)
    dz, dg_ref, db_ref = ops.bn_bwd(dy, z, y, True, scale, shift, mean, invstd, gamma, dres=dres_ref)
    dw_ref = ops.conv2d_wgrad(dz, a2, tuple(w.shape), 1, 0, sc2, sh2, True)
    da_ref = ops.conv2d_dgrad_w(dz, w, tuple(a2.shape), 1, 0)
    # folded
    gbuf = dy.clone()
    coef3, dg, db = ops.bn_bwd_pre(gbuf, z, True, scale, shift, mean, invstd, gamma, y_mask=mask)
    assert torch.equal(gbuf, dres_ref)                      # g in place == the masked / residual gradient
    assert rel_err(dg, dg_ref) < 1e-6 and rel_err(db, db_ref) < 1e-6
    dz_formed = coef3[0].view(1, -1, 1, 1) * gbuf + coef3[1].view(1, -1, 1, 1) * z + coef3[2].view(1, -1, 1, 1)
    assert rel_err(dz_formed, dz) < 2e-6
    dw = ops.conv1x1_wgrad_bnb(gbuf, z, coef3, a2, tuple(w.shape), sc2, sh2, True)
    assert "_bnb" in ops.lib().scat_last_kernel().decode()
    da = ops.conv1x1_dgrad_bnb(gbuf, z, coef3, w, tuple(a2.shape))
    assert rel_err(dw, dw_ref) < 2e-5 and rel_err(da, da_ref) < 2e-5
    base = g(t(49, "acc", tuple(a2.shape)))
    daa = ops.conv1x1_dgrad_bnb(gbuf, z, coef3, w, tuple(a2.shape), out=base.clone(), accumulate=True)
    assert rel_err(daa, da_ref + base) < 2e-5


def test_bn_apply_shortcut(ops):
    """block output with the shortcut's BatchNorm folded into the add: relu(bn3(c3) + bnd(cd)), vector and scalar
    paths, against the two-pass form (bit-exact: same operations in the same order)."""
    for n, shp in enumerate([(2, 24, 6, 6), (3, 8, 5, 3)]):
        c3, cd = g(t(400 + n, "c3", shp)), g(t(410 + n, "cd", shp))
        C = shp[1]
        s3, h3 = g(torch.from_numpy(synth.uniform(420, "s", (C,), 0.5, 1.5))), g(t(421, "h", (C,)))
        sd, hd = g(torch.from_numpy(synth.uniform(422, "s", (C,), 0.5, 1.5))), g(t(423, "h", (C,)))
        res = ops.bn_apply(cd, sd, hd, None, False)
        two = ops.bn_apply(c3, s3, h3, res, True)
        one = ops.bn_apply(c3, s3, h3, cd, True, res_scale=sd, res_shift=hd)
        assert torch.equal(one, two)
        ref = F.relu(c3 * s3.view(1, -1, 1, 1) + h3.view(1, -1, 1, 1) + cd * sd.view(1, -1, 1, 1) + hd.view(1, -1, 1, 1))
        assert rel_err(one, ref) < 1e-6


def test_pools(ops):
    B, C, H = 3, 16, 112
    x = t(24, "x", (B, C, H, H)).requires_grad_(True)
    sc = torch.from_numpy(synth.uniform(25, "sc", (C,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(26, "sh", (C,), -0.5, 0.5))
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    a.retain_grad()
    y = F.max_pool2d(a, 3, 2, 1)
    dy = t(27, "dy", tuple(y.shape))
    y.backward(dy)
    yg, idx = ops.maxpool_fwd(g(x.detach()), g(sc), g(sh), True)
    assert rel_err(yg, y) < 1e-6
    da = ops.maxpool_bwd(g(dy), idx, tuple(x.shape))
    # ties at exactly 0 after ReLU are killed by the ReLU mask downstream: compare on a>0
    m = (a > 0).double()
    assert rel_err(da.cpu().double() * m, a.grad.double() * m) < 1e-6
    # pair kernel (even H, W % 4 == 0): values bit-exact and arg-max taps equal to ATen's, rows shorter and longer than
    # a wavefront (left neighbour from the previous lane / from memory / padding)
    for n, shp in enumerate([(2, 3, 6, 8), (1, 2, 4, 260), (2, 2, 10, 132)]):
        xp = t(200 + n, "xp", shp)
        yt, it = F.max_pool2d(xp, 3, 2, 1, return_indices=True)
        yp, ip = ops.maxpool_fwd(g(xp))
        assert torch.equal(yp.cpu(), yt)
        OH, OW = yt.shape[2:]
        oy = torch.arange(OH).view(1, 1, OH, 1)
        ox = torch.arange(OW).view(1, 1, 1, OW)
        tap = ip.cpu().long()
        flat = (2 * oy - 1 + tap // 3) * shp[3] + (2 * ox - 1 + tap % 3)
        assert torch.equal(flat, it)
    # odd size, no fused transform
    x2 = t(28, "x2", (2, 5, 13, 13))
    y2g, _ = ops.maxpool_fwd(g(x2))
    assert rel_err(y2g, F.max_pool2d(x2, 3, 2, 1)) == 0.0
    # avg pool 7x7 + relu
    x4 = t(29, "x4", (4, 128, 7, 7)).requires_grad_(True)
    f = F.relu(F.avg_pool2d(x4, 7, 1).flatten(1))
    df = t(30, "df", (4, 128))
    f.backward(df)
    fg = ops.avgpool_fwd(g(x4.detach()))
    assert rel_err(fg, f) < 1e-6
    assert rel_err(ops.avgpool_bwd(g(df), fg, tuple(x4.shape)), x4.grad) < 1e-6


@pytest.mark.parametrize("rows,dim", [(84, 784), (2016, 392), (40, 196), (7, 50), (24001, 196)])   # (the last: sliced column sums)
def test_layernorm(ops, rows, dim):
    x = (t(31, "x", (rows, dim)) * 2 + 0.3).requires_grad_(True)
    gm = torch.from_numpy(synth.uniform(32, "g", (dim,), 0.7, 1.3)).requires_grad_(True)
    bt = torch.from_numpy(synth.uniform(33, "b", (dim,), -0.2, 0.2)).requires_grad_(True)
    y = F.layer_norm(x, (dim,), gm, bt, 1e-5)
    dy = t(34, "dy", (rows, dim))
    dx, dg, db = torch.autograd.grad(y, (x, gm, bt), dy)
    yg, mean, rstd = ops.layernorm_fwd(g(x.detach()), g(gm.detach()), g(bt.detach()))
    assert rel_err(yg, y) < 1e-5
    dxg, dgg, dbg = ops.layernorm_bwd(g(dy), g(x.detach()), g(gm.detach()), mean, rstd)
    assert rel_err(dxg, dx) < 1e-5 and rel_err(dgg, dg) < 1e-5 and rel_err(dbg, db) < 1e-5
    # the input gradient alone (the pose-length term's replay, hand_net.py:396): same bits, no parameter sums
    dx_only, none_g, none_b = ops.layernorm_bwd(g(dy), g(x.detach()), g(gm.detach()), mean, rstd, want_params=False)
    assert none_g is None and none_b is None and torch.equal(dx_only, dxg)


@pytest.mark.parametrize("B,n,heads", [(4, 21, 8), (2, 128, 8), (3, 65, 2), (2, 21, 16), (3, 64, 3), (2, 96, 5),
                                       (96, 128, 8)])
def test_attention_core(ops, B, n, heads):
    d = 64
    qkv = t(35, "qkv", (B, n, 3 * heads * d)).requires_grad_(True)
    scale = d ** -0.5
    q, k, v = (z.reshape(B, n, heads, d).permute(0, 2, 1, 3) for z in qkv.split(heads * d, dim=-1))
    attn = (q @ k.transpose(-1, -2) * scale).softmax(-1)
    out = (attn @ v).permute(0, 2, 1, 3).reshape(B, n, heads * d)
    do = t(36, "do", (B, n, heads * d))
    (dqkv,) = torch.autograd.grad(out, qkv, do)
    og, ag = ops.attention_fwd(g(qkv.detach()), heads, d, scale)
    assert rel_err(og, out) < 1e-5 and rel_err(ag, attn) < 1e-5
    assert rel_err(ops.attention_bwd(g(do), g(qkv.detach()), ag, heads, d, scale), dqkv) < 2e-5


@pytest.mark.parametrize("B,n,dim,heads", [(2, 21, 784, 8), (7, 21, 392, 8), (13, 21, 196, 8), (96, 21, 784, 8),
                                            (5, 16, 200, 2), (3, 32, 72, 16)])
def test_vit_qkv_attention_fused(ops, math_mode, B, n, dim, heads):
    """One launch per transformer layer for the qkv projection + softmax attention (models/vision_transformer.py:
    61-76): a workgroup = one head of a block of 128/n images, q/k/v stay in LDS.  Full blocks, a ragged last block,
    feature counts that are not multiples of 16 or 32, against fp64 torch and the unfused kernels."""
    math_mode(1)
    d = 64
    inner = heads * d
    h = t(110, "h", (B * n, dim))
    w = t(111, "w", (3 * inner, dim), std=dim ** -0.5)
    scale = d ** -0.5
    qkv_ref = h.double() @ w.double().t()
    q, k, v = (z.reshape(B, n, heads, d).permute(0, 2, 1, 3) for z in qkv_ref.split(inner, dim=-1))
    attn = (q @ k.transpose(-1, -2) * scale).softmax(-1)
    out = (attn @ v).permute(0, 2, 1, 3).reshape(B, n, inner)
    qg, og, ag = ops.qkv_attention_fwd(g(h), g(w), B, n, heads, scale)
    assert ops.lib().scat_last_kernel().decode().startswith("vit_qkv_attn_fused")
    assert rel_err(qg, qkv_ref) < 2e-5
    assert rel_err(ag, attn) < 2e-5 and rel_err(og, out) < 2e-5
    q0 = ops.linear_fwd(g(h), g(w))
    o0, a0 = ops.attention_fwd(q0.view(B, n, 3 * inner), heads, d, scale)
    assert rel_err(qg, q0.cpu()) < 2e-5 and rel_err(og, o0.cpu()) < 2e-5 and rel_err(ag, a0.cpu()) < 2e-5


def test_elementwise_tokens(ops):
    x = t(37, "x", (4, 21, 784)).requires_grad_(True)
    y = F.gelu(x)
    dy = t(38, "dy", (4, 21, 784))
    (dx,) = torch.autograd.grad(y, x, dy)
    assert rel_err(ops.gelu_fwd(g(x.detach())), y) < 1e-6
    assert rel_err(ops.gelu_bwd(g(dy), g(x.detach())), dx) < 1e-5
    assert rel_err(ops.axpy(g(x.detach()), g(dy), 0.5), x.detach() + 0.5 * dy) < 1e-6
    r = ops.relu_fwd(g(x.detach()))
    assert rel_err(r, F.relu(x)) == 0.0
    assert rel_err(ops.relu_bwd(g(dy), r), dy * (x > 0)) == 0.0
    pe = t(39, "pe", (21, 784))
    mt = t(40, "mt", (784,)).requires_grad_(True)
    masked = [5, 0, 17, 9]
    f = x + pe
    f2 = f.clone()
    f2[:, masked, :] = mt
    (dxr, dmr) = torch.autograd.grad(f2, (x, mt), dy)
    mi = torch.tensor(masked, dtype=torch.int32, device=DEV)
    assert rel_err(ops.tokens_fwd(g(x.detach()), g(pe), g(mt.detach()), mi), f2) < 1e-6
    dxg, dmg = ops.tokens_bwd(g(dy), mi)
    assert rel_err(dxg, dxr) < 1e-6 and rel_err(dmg, dmr) < 1e-5
    assert rel_err(ops.tokens_fwd(g(x.detach()), g(pe), None, None), f) < 1e-6


@pytest.mark.parametrize("iters", [0, 1, 3])
def test_regressor_and_loss(ops, iters):
    B, Fd, P = 6, 1024, 66
    feat = F.relu(t(41, "feat", (B, Fd))).requires_grad_(True)
    fo = t(42, "fo", (B, 63), std=0.05).requires_grad_(True)
    mean = torch.from_numpy(synth.mean_params(43))
    w = t(44, "w", (P, Fd + P), std=0.3 * (Fd + P) ** -0.5).requires_grad_(True)
    b = t(45, "b", (P,), std=0.05).requires_grad_(True)
    lab = torch.from_numpy(synth.labels(46, B))
    pred = mean.repeat(B, 1).clone()
    pred[:, 3:] = pred[:, 3:] + fo
    for _ in range(iters):
        pred = pred + F.linear(torch.cat((feat, pred), 1), w, b)
    j = pred[:, 3:].reshape(B, 21, 3)
    j = j - j[:, 1:2]
    out = torch.cat((pred[:, :3], j.reshape(B, 63)), 1)
    from oracle.scat_oracle import scat_loss

    loss, l3, l2, _ = scat_loss(out, lab)
    out.retain_grad()
    loss.backward()
    og, preds = ops.regressor_fwd(g(feat.detach()), g(fo.detach()), g(mean).view(-1), g(w.detach()), g(b.detach()),
                                  iters)
    assert rel_err(og, out) < 1e-5
    losses, dout = ops.loss_fwd_bwd(og, g(lab))
    assert rel_err(losses, torch.stack([loss, l3, l2]).detach()) < 1e-5
    assert rel_err(dout, out.grad) < 1e-4
    dfeat, dfo, dw, db = ops.regressor_bwd(g(out.grad), g(feat.detach()), preds, g(w.detach()), iters)
    assert rel_err(dfo, fo.grad) < 1e-5
    if iters:
        assert rel_err(dfeat, feat.grad) < 1e-5 and rel_err(dw, w.grad) < 1e-5 and rel_err(db, b.grad) < 1e-5


def test_adam(ops):
    n = 100003
    p = t(47, "p", (n,))
    gr = t(48, "g", (n,), std=1e-3)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=5e-4)
    pg, m, v = g(p), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in (1, 2, 3):
        ref.grad = gr * step
        opt.step()
        ops.adam(pg, g(gr * step), m, v, 5e-4, step)
    assert rel_err(pg, ref.detach()) < 1e-6


def test_errors_are_loud(ops):
    from scat_amd._lib import ScatError

    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ScatError):
        ops.conv2d_fwd(x, torch.zeros(4, 3, 3, 3), 1, 1)  # CPU tensor: no fallback
    with pytest.raises(ScatError):
        ops.conv2d_fwd(g(x), g(torch.zeros(4, 3, 5, 5)), 1, 2)  # unsupported kernel size


def test_preprocess_u8(ops):
    """input pipeline kernel vs torch: /127.5-1 then bilinear(align_corners=False), CHW and HWC sources"""
    u8 = torch.from_numpy(synth.randint_u8(60, "img", (3, 3, 256, 256)))
    ref = F.interpolate(u8.float() / 127.5 - 1.0, size=(224, 224), mode="bilinear", align_corners=False)
    assert rel_err(ops.preprocess_u8(u8.cuda()), ref) < 1e-5
    hwc = u8.permute(0, 2, 3, 1).contiguous()
    assert rel_err(ops.preprocess_u8(hwc.cuda(), hwc=True), ref) < 1e-5
    same = torch.from_numpy(synth.randint_u8(61, "img", (2, 3, 224, 224)))
    assert rel_err(ops.preprocess_u8(same.cuda()), same.float() / 127.5 - 1.0) < 1e-6
    small = torch.from_numpy(synth.randint_u8(62, "img", (2, 3, 64, 64)))   # BASELINE configs[0]: 64x64 source
    ref = F.interpolate(small.float() / 127.5 - 1.0, size=(224, 224), mode="bilinear", align_corners=False)
    assert rel_err(ops.preprocess_u8(small.cuda()), ref) < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# Batch 96: the instantiations the bench actually times (VERDICT r02 "Next" item 1).  Tile choices, split-K plans, the
# row-walking / producer-consumer / packed-shortcut / folded-BatchNorm kernels are picked from the shape AT BATCH 96, so
# the B = 2..3 cases above never reach them.  Every ResNet-50 geometry is run here the way the step runs it (the role
# column: which operand transform, which gradient form) against fp64 F.conv2d on the same seeded tensors.
#   role "in"  : the convolution reads a block input / packed shortcut input as it is      (conv1, downsample)
#   role "tf"  : it reads relu(bn(x)) formed in its operand load                           (conv2, conv3)
#   role "both": 64->256 @56 is conv3 of layer1 AND the shortcut of layer1.0
B96_ROLES = {
    (3, 64, 7, 2): "in", (64, 64, 1, 1): "in", (64, 64, 3, 1): "tf", (64, 256, 1, 1): "both", (256, 64, 1, 1): "in",
    (256, 128, 1, 1): "in", (128, 128, 3, 2): "tf", (128, 512, 1, 1): "tf", (256, 512, 1, 2): "in", (512, 128, 1, 1): "in",
    (128, 128, 3, 1): "tf", (512, 256, 1, 1): "in", (256, 256, 3, 2): "tf", (256, 1024, 1, 1): "tf", (512, 1024, 1, 2): "in",
    (1024, 256, 1, 1): "in", (256, 256, 3, 1): "tf", (1024, 512, 1, 1): "in", (512, 512, 3, 2): "tf", (512, 2048, 1, 1): "tf",
    (1024, 2048, 1, 2): "in", (2048, 512, 1, 1): "in", (512, 512, 3, 1): "tf", (512, 21, 1, 1): "in",
}
_B96_LABELS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "b96_kernel_labels.json")
_B96_SEEN = {}


def _label(ops):
    return ops.lib().scat_last_kernel().decode()


def _b96_note(key, label):
    """the kernel label each (shape, op) took — compared with the committed table (the same table tools/conv_bench.py
    prints into profiles/*_conv_shapes.txt), so a dispatch change that is not re-checked here shows up"""
    import json

    _B96_SEEN[key] = label
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "b96_kernel_labels.json"), "w") as f:
            json.dump(_B96_SEEN, f, indent=1, sort_keys=True)
    except OSError:
        pass
    if os.path.exists(_B96_LABELS_FILE):
        want = json.load(open(_B96_LABELS_FILE)).get(key)
        assert want is None or want == label, f"{key}: kernel {label}, committed table says {want}"


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cin,cout,k,s,p,H", CONVS)
def test_conv_batch96_instantiations(ops, cin, cout, k, s, p, H):
    B = 96
    role = B96_ROLES[(cin, cout, k, s)]
    name = f"{cin}->{cout} k{k} s{s} {H}x{H}"
    gen = torch.Generator().manual_seed(1000 + cin + 7 * cout + k)
    x = torch.randn((B, cin, H, H), generator=gen)
    w = torch.randn((cout, cin, k, k), generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    sc = torch.rand((cin,), generator=gen) + 0.5
    sh = torch.rand((cin,), generator=gen) - 0.5
    tf = role in ("tf", "both")
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if tf else x
    a64 = a.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y = F.conv2d(a64, w64, stride=s, padding=p)
    dy = torch.randn(tuple(y.shape), generator=gen)
    dx_ref, dw_ref = torch.autograd.grad(y, (a64, w64), dy.double())
    y = y.detach()
    xg, wg, dyg = g(x), g(w), g(dy)
    tfa = (g(sc), g(sh), True) if tf else (None, None, False)
    wp = ops.WeightPrep()          # prepared weights like the network's: first call registers, run() re-lays, then w_ready=1

    # ---- forward with the BatchNorm sums in its epilogue (what _block_forward launches), then the finish
    ops.conv2d_fwd(xg, wg, s, p, *tfa, wp=wp, stats=True)
    wp.run(True)
    yg = ops.conv2d_fwd(xg, wg, s, p, *tfa, wp=wp, stats=True)
    _b96_note(f"{name} fwd{'_tf' if tf else ''}", _label(ops))
    assert rel_err(yg, y) < 2e-5
    gamma, beta = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    had_partials = getattr(yg, "scat_stats", None) is not None
    mean, invstd, _, _ = ops.bn_train_stats(yg, gamma, beta, rm, rv)
    var = y.var(dim=(0, 2, 3), unbiased=False)
    assert rel_err(mean, y.mean(dim=(0, 2, 3))) < 2e-5, had_partials
    assert rel_err(invstd, (var + 1e-5).rsqrt()) < 2e-5, had_partials
    if role == "both":             # the shortcut of layer1.0 reads the block input as it is
        yp = ops.conv2d_fwd(xg, wg, s, p, wp=wp, stats=True)
        _b96_note(f"{name} fwd", _label(ops))
        assert rel_err(yp, F.conv2d(x.double(), w.double(), stride=s, padding=p)) < 2e-5

    # ---- weight gradient (the fused operand transform is the forward's)
    dwg = ops.conv2d_wgrad(dyg, xg, tuple(w.shape), s, p, *tfa)
    _b96_note(f"{name} wgrad{'_tf' if tf else ''}", _label(ops))
    assert rel_err(dwg, dw_ref) < 2e-5

    # ---- data gradient, plain and accumulating (conv1 adds onto the residual gradient)
    if k != 7:
        dxg = ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p, wp=wp)
        wp.run(True)
        dxg = ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p, wp=wp)
        _b96_note(f"{name} dgrad", _label(ops))
        assert rel_err(dxg, dx_ref) < 2e-5
        base = torch.randn(tuple(x.shape), generator=gen)
        dxa = ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p, out=g(base), accumulate=True, wp=wp)
        assert rel_err(dxa, dx_ref + base.double()) < 2e-5
        del dxa, base

    # ---- the 1x1/stride-2 shortcuts run packed: subsample once, then stride-1 kernels forward and for dW
    if k == 1 and s == 2:
        xs = ops.subsample2(xg)
        assert torch.equal(xs, xg[:, :, ::2, ::2])
        ys = ops.conv2d_fwd(xs, wg, 1, 0, wp=wp, stats=True)
        _b96_note(f"{name} fwd_packed", _label(ops))
        assert rel_err(ys, y) < 2e-5
        dws = ops.conv2d_wgrad(dyg, xs, tuple(w.shape), 1, 0)
        _b96_note(f"{name} wgrad_packed", _label(ops))
        assert rel_err(dws, dw_ref) < 2e-5

    # ---- conv3 on the 56x56 / 28x28 planes: bn3's backward apply is formed inside conv3's two gradient kernels
    if k == 1 and s == 1 and tf and H >= 28 and cout % 16 == 0 and ops.get_math_mode() == 1:
        z = yg                                                            # conv3's raw output
        coef = torch.rand((3, cout), generator=gen) - 0.5
        coef[0] += 1.0
        coef[2] *= 0.1
        dz = (coef[0].view(1, -1, 1, 1).double() * dy.double() + coef[1].view(1, -1, 1, 1).double() * y
              + coef[2].view(1, -1, 1, 1).double())
        da_ref, dwz_ref = torch.autograd.grad(F.conv2d(a64, w64), (a64, w64), dz)
        cg = g(coef)
        dwb = ops.conv1x1_wgrad_bnb(dyg, z, cg, xg, tuple(w.shape), *tfa)
        _b96_note(f"{name} wgrad_bnb", _label(ops))
        assert rel_err(dwb, dwz_ref) < 2e-5
        dab = ops.conv1x1_dgrad_bnb(dyg, z, cg, wg, tuple(x.shape), wp=wp)
        _b96_note(f"{name} dgrad_bnb", _label(ops))
        assert rel_err(dab, da_ref) < 2e-5


# the eight-consumer producer/consumer pointwise kernel (256 x 128 tiles): the default rule sends only the batch-96 layers
# with 257..329 tiles of 128 x 128 there (covered by test_conv_batch96_instantiations); forced onto small shapes here so
# that every epilogue / staging variant of BOTH shipped forms (SCAT_PC=6: 16-byte pixel quads; 5: scalar pixels, the
# fallback for HW % 4 != 0) is held to fp64: forward + bias, forward + fused input transform, data gradient, data
# gradient accumulating, ragged row and pixel tiles, 7x7 planes.  (SCAT_PC is read once per process, hence the child.)
PC_SHAPES = [(3, 64, 256, 14, 14), (5, 96, 384, 7, 7), (2, 160, 272, 9, 12), (1, 64, 1024, 5, 30), (4, 128, 256, 7, 9)]


def _pc_case(ops, B, cin, cout, H, W, expect):
    x = t(170, "x", (B, cin, H, W)).requires_grad_(True)
    w = t(171, "w", (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5).requires_grad_(True)
    bias = t(172, "b", (cout,))
    y = F.conv2d(x.double(), w.double(), bias.double())
    dy = t(173, "dy", tuple(y.shape))
    (dx_ref,) = torch.autograd.grad(y, x, dy.double())
    yg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 0, bias=g(bias))
    lab = ops.lib().scat_last_kernel().decode()
    assert lab.startswith(expect), (lab, expect)
    assert rel_err(yg, y) < 2e-5
    sc = torch.from_numpy(synth.uniform(175, "sc", (cin,), 0.5, 1.5))
    sh = torch.from_numpy(synth.uniform(176, "sh", (cin,), -0.5, 0.5))
    a = F.relu(x.detach() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    ytg = ops.conv2d_fwd(g(x.detach()), g(w.detach()), 1, 0, g(sc), g(sh), True)
    assert ops.lib().scat_last_kernel().decode().endswith("_tf")
    assert rel_err(ytg, F.conv2d(a.double(), w.detach().double())) < 2e-5
    # this convolution's data gradient has M = Cin < 256 rows: the plain kernel, same process, same switch
    dxg = ops.conv2d_dgrad_w(g(dy), g(w.detach()), tuple(x.shape), 1, 0)
    assert rel_err(dxg, dx_ref) < 2e-5
    # the transposed role at 256 rows: a convolution whose data gradient has M = Cin >= 256
    xt = t(177, "xt", (B, cout, H, W)).requires_grad_(True)
    wt = t(178, "wt", (cin, cout, 1, 1), std=(2.0 / cout) ** 0.5)
    yt = F.conv2d(xt.double(), wt.double())
    dyt = t(179, "dyt", tuple(yt.shape))
    (dxt_ref,) = torch.autograd.grad(yt, xt, dyt.double())
    dxt = ops.conv2d_dgrad_w(g(dyt), g(wt), tuple(xt.shape), 1, 0)
    lab = ops.lib().scat_last_kernel().decode()
    assert lab.startswith(expect), (lab, expect)
    assert rel_err(dxt, dxt_ref) < 2e-5
    base = g(t(180, "acct", tuple(xt.shape)))
    dxta = ops.conv2d_dgrad_w(g(dyt), g(wt), tuple(xt.shape), 1, 0, out=base.clone(), accumulate=True)
    assert rel_err(dxta, dxt_ref + base.cpu().double()) < 2e-5


PC_EXACT_SHAPES = [PC_SHAPES[0], PC_SHAPES[4]]        # full pixel quads; HW % 4 != 0 (scalar pixels in both forms)


def _pc_exact_case(ops, B, cin, cout, H, W, expect):
    """the same roles on exact-sum data (tests/test_gpu_exact_split.py): every result bit-for-bit the fp64 answer, so a
    lost or mis-paired term of the six shows in this form too"""
    import test_gpu_exact_split as X
    X.pc_exact_case(ops, B, cin, cout, H, W, expect)


@pytest.mark.parametrize("pc", [5, 6])
def test_conv1x1_producer_consumer_forms(pc):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_ops as T\nfrom scat_amd import ops\n"
            "for a in T.PC_SHAPES:\n"
            "    wide = %d == 6 and (a[3] * a[4]) %% 4 == 0\n"
            "    T._pc_case(ops, *a, 'conv1x1_split_pc4_256' if wide else 'conv1x1_split_pc8w_256')\n"
            "    if a in T.PC_EXACT_SHAPES:\n"
            "        T._pc_exact_case(ops, *a, 'conv1x1_split_pc4_256' if wide else 'conv1x1_split_pc8w_256')\n"
            "print('PC OK')\n") % (root, os.path.join(root, "tests"), pc)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SCAT_PC=str(pc)), capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert "PC OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# pointwise kernels on launches of >= 256 tiles of 128 pixels: few and many contraction stages per tile, ragged rows and
# pixel columns, 64-row tiles; forward (+ fused transform, + BatchNorm sums in the epilogue), data gradient
# (+ accumulate), the folded-BatchNorm data gradient.  Held to fp64 and to itself bit for bit.
PW_MANY_TILES = [(28, 256, 256, 28, 28), (7, 64, 256, 56, 56), (5, 96, 200, 63, 52), (10, 128, 64, 60, 60), (5, 512, 1024, 34, 33)]


@pytest.mark.parametrize("B,cin,cout,H,W", PW_MANY_TILES)
def test_conv1x1_many_tiles(ops, B, cin, cout, H, W):
    assert ops.get_math_mode() == 1
    gen = torch.Generator().manual_seed(B * 1000 + cin + cout)
    x = torch.randn((B, cin, H, W), generator=gen)
    w = torch.randn((cout, cin, 1, 1), generator=gen) * (2.0 / cin) ** 0.5
    sc, sh = torch.rand((cin,), generator=gen) + 0.5, torch.rand((cin,), generator=gen) - 0.5
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    xg, wg = g(x), g(w)

    def twice(fn):
        r1 = fn().clone()
        r2 = fn().clone()
        assert torch.equal(r1, r2), "result is not reproducible"
        return r1

    y = twice(lambda: ops.conv2d_fwd(xg, wg, 1, 0, g(sc), g(sh), True))
    yr = F.conv2d(a.double(), w.double())
    assert rel_err(y, yr) < 2e-5
    # BatchNorm sums from the epilogue
    ys = ops.conv2d_fwd(xg, wg, 1, 0, stats=True)
    assert getattr(ys, "scat_stats", None) is not None
    ones, zeros = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    mean, invstd, _, _ = ops.bn_train_stats(ys, ones, zeros, zeros.clone(), ones.clone())
    yp = F.conv2d(x.double(), w.double())
    assert rel_err(ys, yp) < 2e-5
    assert rel_err(mean, yp.mean(dim=(0, 2, 3))) < 2e-5
    assert rel_err(invstd, (yp.var(dim=(0, 2, 3), unbiased=False) + 1e-5).rsqrt()) < 2e-5
    # data gradient of the transposed role (M = cout rows here: a convolution cout <- cin seen from its output side)
    dy = torch.randn((B, cin, H, W), generator=gen)
    wt = torch.randn((cin, cout, 1, 1), generator=gen) * (2.0 / cout) ** 0.5
    base = torch.randn((B, cout, H, W), generator=gen)
    dxr = F.conv_transpose2d(dy.double(), wt.double())
    dx = twice(lambda: ops.conv2d_dgrad_w(g(dy), g(wt), (B, cout, H, W), 1, 0))
    assert rel_err(dx, dxr) < 2e-5
    dxa = ops.conv2d_dgrad_w(g(dy), g(wt), (B, cout, H, W), 1, 0, out=g(base), accumulate=True)
    assert rel_err(dxa, dxr + base.double()) < 2e-5
    # folded BatchNorm backward: operand ca*g + cb*z + cc formed in the load (dual source)
    if cin % 16 == 0 and (H * W) % 4 == 0:
        z = torch.randn((B, cin, H, W), generator=gen)
        coef = torch.rand((3, cin), generator=gen) - 0.5
        v = lambda i: coef[i].view(1, -1, 1, 1).double()
        dzr = F.conv_transpose2d(v(0) * dy.double() + v(1) * z.double() + v(2), wt.double())
        dzb = twice(lambda: ops.conv1x1_dgrad_bnb(g(dy), g(z), g(coef), g(wt), (B, cout, H, W)))
        assert rel_err(dzb, dzr) < 2e-5


@pytest.mark.parametrize("B,C,H,W", [(96, 21, 28, 28), (3, 5, 7, 9), (1, 21, 28, 28)])
def test_pose_length_term(ops, B, C, H, W):
    """train.py:178-183 as two launches (scat_pose_length_term) against the torch expression of the reference"""
    pl = t(300, "pl", (B, C, H, W), 0.01)
    lens = torch.sum(torch.square(pl.double()), dim=[2, 3]).mean(dim=[1]).sqrt()
    ref = torch.square(lens - 0.01 * torch.mean(lens)).mean()
    got = ops.pose_length_term(g(pl))
    assert got.shape == () and abs(got.item() - ref.item()) <= 1e-6 * abs(ref.item())
    got_view = ops.pose_length_term(g(pl).transpose(2, 3).contiguous().transpose(2, 3))    # non-contiguous input
    assert abs(got_view.item() - ref.item()) <= 1e-6 * abs(ref.item())


# second-generation pointwise weight gradient (csrc/conv_wgrad_pw.hip): every tile shape (256x128, 128x256, 128x128,
# 256x64, 64x256), partial tiles (channel counts that are multiples of 64 but not of the tile), planes whose size is not
# a multiple of 8 (last octet of an image half empty) or of 4 (7x7: pixel-by-pixel loads), split-K slices that end
# inside an image, the fused input transform on x, the folded BatchNorm backward on dy.
WGPW = [
    # B, Cin, Cout, H, W, tf
    (5, 128, 512, 14, 14, True), (3, 512, 128, 12, 10, False), (4, 256, 256, 7, 7, True), (6, 192, 320, 14, 14, False),
    (2, 64, 256, 28, 28, True), (3, 256, 64, 20, 22, False), (7, 1024, 256, 7, 7, False), (2, 128, 128, 14, 18, True),
    (3, 320, 192, 5, 5, True), (9, 2048, 512, 7, 7, False),
]


@pytest.mark.parametrize("B,cin,cout,H,W,tf", WGPW)
def test_wgrad1x1_pw(ops, B, cin, cout, H, W, tf):
    assert ops.get_math_mode() == 1
    gen = torch.Generator().manual_seed(B * 131 + cin + 3 * cout)
    x = torch.randn((B, cin, H, W), generator=gen)
    dy = torch.randn((B, cout, H, W), generator=gen)
    sc, sh = torch.rand((cin,), generator=gen) + 0.5, torch.rand((cin,), generator=gen) - 0.5
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if tf else x
    ref = torch.einsum("nop,nip->oi", dy.double().flatten(2), a.double().flatten(2)).view(cout, cin, 1, 1)
    tfa = (g(sc), g(sh), True) if tf else (None, None, False)
    dw = ops.conv2d_wgrad(g(dy), g(x), (cout, cin, 1, 1), 1, 0, *tfa)
    lab = ops.lib().scat_last_kernel().decode()
    assert lab.startswith("wgrad1x1_pw_"), lab
    assert ("_rag" in lab) == ((H * W) % 4 != 0)
    assert rel_err(dw, ref) < 2e-5
    assert torch.equal(dw, ops.conv2d_wgrad(g(dy), g(x), (cout, cin, 1, 1), 1, 0, *tfa))      # deterministic split-K
    if (H * W) % 4 == 0:       # folded BatchNorm backward: dy = ca*g + cb*z + cc formed in the load
        z = torch.randn((B, cout, H, W), generator=gen)
        coef = torch.rand((3, cout), generator=gen) - 0.5
        v = lambda i: coef[i].view(1, -1, 1, 1).double()
        dz = v(0) * dy.double() + v(1) * z.double() + v(2)
        refb = torch.einsum("nop,nip->oi", dz.flatten(2), a.double().flatten(2)).view(cout, cin, 1, 1)
        dwb = ops.conv1x1_wgrad_bnb(g(dy), g(z), g(coef), g(x), (cout, cin, 1, 1), *tfa)
        lab = ops.lib().scat_last_kernel().decode()
        assert lab.startswith("wgrad1x1_pw_") and "_bnb" in lab, lab
        assert rel_err(dwb, refb) < 2e-5


def test_gemm_group(ops):
    """scat_gemm_group: independent weight-gradient contractions in one launch == the same contractions one by one and
    fp64 (shapes of the token mixer at batch 96 and ragged ones; split-K inside the group)."""
    for M, dims in ((2016, [(1536, 784), (784, 512), (588, 784), (392, 588), (1536, 392), (3, 147), (147, 196)]),
                    (300, [(70, 33), (129, 64), (64, 200)])):
        gen = torch.Generator().manual_seed(M)
        pairs, refs = [], []
        for N, K in dims:
            dy, x = torch.randn((M, N), generator=gen), torch.randn((M, K), generator=gen)
            pairs.append((g(dy), g(x)))
            refs.append(dy.double().t() @ x.double())
        outs = ops.linear_wgrad_group(pairs)
        assert ops.lib().scat_last_kernel().decode().startswith("gemm_group")
        for (dy, x), o, r in zip(pairs, outs, refs):
            assert rel_err(o, r) < 2e-5
            assert rel_err(o, ops.linear_wgrad(dy, x)) < 5e-6


@pytest.mark.parametrize("B,C,H", [(96, 32, 28), (7, 64, 14), (96, 128, 7), (3, 16, 5), (33, 200, 9)])
def test_batchnorm_last_arriver_finalize(ops, B, C, H):
    """The per-channel reduce of the BatchNorm statistics / backward sums finishes in the workgroup that arrives last
    (csrc/norm.hip bn_publish) instead of in a second launch: same bits as the two-launch form (SCAT_BN_LASTBLOCK=0, a
    child process), every call finishes every channel EXACTLY once (the running statistics follow the recurrence over 40
    repeated calls), forward statistics, backward sums and the folded-backward constants."""
    import subprocess
    import sys
    x = t(201, "x", (B, C, H, H)) * 1.7 + 0.4
    dy = t(202, "dy", (B, C, H, H))
    gamma = torch.from_numpy(synth.uniform(203, "g", (C,), 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform(204, "b", (C,), -0.3, 0.3))
    xg, dyg, gg, bg = g(x), g(dy), g(gamma), g(beta)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    outs = []
    for it in range(40):
        mean, invstd, scale, shift = ops.bn_train_stats(xg, gg, bg, rm, rv)
        outs.append(torch.stack((mean, invstd, scale, shift)).clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    m64 = x.double().mean(dim=(0, 2, 3))
    v64 = x.double().var(dim=(0, 2, 3), unbiased=True)
    k = 1.0 - 0.9 ** 40
    assert rel_err(rm, k * m64) < 1e-5 and rel_err(rv, 0.9 ** 40 + k * v64) < 1e-5      # 40 updates, not 39 or 41
    assert rel_err(mean, m64) < 1e-6
    dxs = []
    for it in range(10):
        dxg, dgg, dbg = ops.bn_bwd(dyg.clone(), xg, None, True, scale, shift, mean, invstd, gg)
        dxs.append(torch.cat((dxg.flatten()[:4096], dgg, dbg)).clone())
    assert all(torch.equal(dxs[0], o) for o in dxs[1:])
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5))
    dx_ref, dg_ref, db_ref = torch.autograd.grad(yr, (xr, gr, br), dy.double())
    assert rel_err(dxg, dx_ref) < 2e-5 and rel_err(dgg, dg_ref) < 2e-5 and rel_err(dbg, db_ref) < 2e-5
    if (H * H) % 4 == 0:
        gbuf = dyg.clone()
        coef3, dg3, db3 = ops.bn_bwd_pre(gbuf, xg, True, scale, shift, mean, invstd, gg)
        formed = coef3[0].view(1, -1, 1, 1) * gbuf + coef3[1].view(1, -1, 1, 1) * xg + coef3[2].view(1, -1, 1, 1)
        assert rel_err(formed, dx_ref) < 2e-5 and rel_err(dg3, dg_ref) < 2e-5
    # the two-launch form gives the same bits
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_ops as T\nfrom scat_amd import ops, synth\n"
            "x = T.g(T.t(201, 'x', (%d, %d, %d, %d)) * 1.7 + 0.4)\n"
            "gm = T.g(torch.from_numpy(synth.uniform(203, 'g', (%d,), 0.5, 1.5))); bt = T.g(torch.from_numpy(synth.uniform(204, 'b', (%d,), -0.3, 0.3)))\n"
            "rm, rv = torch.zeros(%d, device='cuda'), torch.ones(%d, device='cuda')\n"
            "o = ops.bn_train_stats(x, gm, bt, rm, rv)\n"
            "torch.save(torch.stack(o).cpu(), sys.argv[1])\n") % (root, os.path.join(root, "tests"), B, C, H, H, C, C, C, C)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "two.pt")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, SCAT_BN_LASTBLOCK="0"), capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        two = torch.load(f)
    assert torch.equal(outs[0].cpu(), two)


@pytest.mark.parametrize("B,C,H,W", [(3, 32, 56, 56), (2, 64, 28, 28), (2, 16, 14, 14), (1, 8, 8, 12), (2, 8, 6, 10)])
def test_fuse_sum_exchange_output(ops, B, C, H, W):
    """scat_fuse_sum (models/hrnet.py:117-144, one output of an exchange unit): BatchNorm-normalised, nearest-upsampled
    terms added in the given order + ReLU in one pass == the reference's chain of BatchNorm / Upsample / add / ReLU."""
    v = lambda a: a.view(1, -1, 1, 1)
    x0 = t(301, "x0", (B, C, H, W))
    terms, ref = [(g(x0), None, None, 0)], x0.double()
    for n, k in enumerate((1, 2, 0)):
        if H % (1 << k) or W % (1 << k):
            continue                                      # (14 x 14 maps have no branch four times coarser)
        c = t(302 + n, "c", (B, C, H >> k, W >> k)) * (1.3 - 0.3 * n) + 0.2 * n
        sc = torch.from_numpy(synth.uniform(310 + n, "s", (C,), 0.5, 1.5))
        sh = torch.from_numpy(synth.uniform(320 + n, "h", (C,), -0.5, 0.5))
        term = c.double() * v(sc.double()) + v(sh.double())
        ref = ref + (F.interpolate(term, scale_factor=1 << k, mode="nearest") if k else term)
        terms.append((g(c), g(sc), g(sh), k))
    assert rel_err(ops.fuse_sum(terms, relu=True), F.relu(ref)) < 1e-6
    # an upsampled term first, no ReLU
    got = ops.fuse_sum([terms[1], terms[0]], relu=False)
    c, sc, sh, k = terms[1]
    ref2 = F.interpolate(c.cpu().double() * v(sc.cpu().double()) + v(sh.cpu().double()), scale_factor=2, mode="nearest") + x0.double()
    assert rel_err(got, ref2) < 1e-6


@pytest.mark.parametrize("rows,cols", [(24672, 196), (24001, 392), (70000, 61), (5000, 196)])
def test_colsum_tall(ops, rows, cols):
    """bias gradients of the token mixers at HRNet's token count (models/vit.py:40-47, 96 x 257 tokens): tall matrices are
    summed in row slices (scat_colsum_sliced), small ones by the one-launch form; also accumulating; same bits twice"""
    x = t(401, "x", (rows, cols)) + 0.25
    ref = x.double().sum(0)
    got = ops.colsum(g(x))
    assert rel_err(got, ref) < 2e-6
    assert torch.equal(got, ops.colsum(g(x)))
    acc = g(torch.ones(cols))
    ops.colsum(g(x), out=acc, accumulate=True)
    assert rel_err(acc, ref + 1.0) < 2e-6


def test_colsum_group(ops):
    """the bias gradients of a token mixer's backward as one launch (scat_colsum_group): bit for bit what one scat_colsum
    per matrix gives, for ragged shapes, more than 16 jobs, and a tall matrix in the list (which keeps its sliced form)"""
    shapes = [(2016, 392), (2016, 784), (2016, 3), (77, 1), (5, 1090), (2016, 196)] * 3 + [(24672, 196)]
    xs = [g(t(410 + i, "x", sh) + 0.1 * i) for i, sh in enumerate(shapes)]
    got = ops.colsum_group(xs)
    assert len(got) == len(xs)
    for x, o in zip(xs, got):
        assert o.shape == (x.shape[1],) and torch.equal(o, ops.colsum(x))
        assert rel_err(o, x.double().sum(0)) < 2e-6


@pytest.mark.parametrize("B,C,H", [(96, 256, 14), (96, 64, 7), (5, 128, 14), (3, 70, 9)])
def test_batchnorm_backward_one_pass(ops, B, C, H):
    """Small planes: the BatchNorm backward reduces and applies in one launch from registers (csrc/norm.hip
    bn_bwd_onepass_kernel) — against fp64 autograd, with the residual-gradient output, and bit for bit the two-launch
    form's result (SCAT_BN_ONEPASS=0 in a child process)."""
    import subprocess
    import sys
    import tempfile
    x = t(501, "x", (B, C, H, H)) * 1.4 - 0.3
    dy = t(502, "dy", (B, C, H, H))
    gamma = torch.from_numpy(synth.uniform(503, "g", (C,), 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform(504, "b", (C,), -0.3, 0.3))
    xg, dyg, gg, bg = g(x), g(dy), g(gamma), g(beta)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd, scale, shift = ops.bn_train_stats(xg, gg, bg, rm, rv)
    res = torch.full_like(dyg, 0.5)
    dxg, dgg, dbg = ops.bn_bwd(dyg, xg, None, True, scale, shift, mean, invstd, gg, dres=res)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5))
    dx_ref, dg_ref, db_ref = torch.autograd.grad(yr, (xr, gr, br), dy.double())
    assert rel_err(dxg, dx_ref) < 2e-5 and rel_err(dgg, dg_ref) < 2e-5 and rel_err(dbg, db_ref) < 2e-5
    assert rel_err(res, dy.double() * (yr > 0)) < 1e-6          # dres: the masked gradient itself
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_ops as T\nfrom scat_amd import ops, synth\n"
            "B, C, H = %d, %d, %d\n"
            "x = T.g(T.t(501, 'x', (B, C, H, H)) * 1.4 - 0.3); dy = T.g(T.t(502, 'dy', (B, C, H, H)))\n"
            "gm = T.g(torch.from_numpy(synth.uniform(503, 'g', (C,), 0.5, 1.5))); bt = T.g(torch.from_numpy(synth.uniform(504, 'b', (C,), -0.3, 0.3)))\n"
            "rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')\n"
            "mean, invstd, scale, shift = ops.bn_train_stats(x, gm, bt, rm, rv)\n"
            "dx, dg, db = ops.bn_bwd(dy, x, None, True, scale, shift, mean, invstd, gm)\n"
            "torch.save((dx.cpu(), dg.cpu(), db.cpu()), sys.argv[1])\n") % (root, os.path.join(root, "tests"), B, C, H)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "two.pt")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, SCAT_BN_ONEPASS="0"), capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        dx2, dg2, db2 = torch.load(f)
    dx1, dg1, db1 = ops.bn_bwd(dyg, xg, None, True, scale, shift, mean, invstd, gg)
    assert torch.equal(dx1.cpu(), dx2) and torch.equal(dg1.cpu(), dg2) and torch.equal(db1.cpu(), db2)


@pytest.mark.parametrize("B,C,H,W", [(4, 64, 112, 112), (3, 16, 8, 12), (2, 8, 6, 4), (5, 70, 10, 8)])
def test_batchnorm_backward_through_maxpool(ops, B, C, H, W):
    """scat_bn_bwd_maxpool (the stem, models/resnet.py:108-112): bn1's backward taken straight from the max-pool's output
    gradient and arg-max taps == max-pool backward followed by the BatchNorm backward (the library's own two-step path,
    and fp64 autograd of batch_norm -> relu -> max_pool2d)."""
    x = t(601, "x", (B, C, H, W)) * 1.2 + 0.1
    gamma = torch.from_numpy(synth.uniform(603, "g", (C,), 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform(604, "b", (C,), -0.3, 0.3))
    xg, gg, bg = g(x), g(gamma), g(beta)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd, scale, shift = ops.bn_train_stats(xg, gg, bg, rm, rv)
    y, idx = ops.maxpool_fwd(xg, scale, shift, True)
    dy = t(602, "dy", tuple(y.shape))
    dyg = g(dy)
    dx1, dg1, db1 = ops.bn_bwd_maxpool(dyg, idx, xg, True, scale, shift, mean, invstd, gg)
    da = ops.maxpool_bwd(dyg, idx, tuple(x.shape))
    dx2, dg2, db2 = ops.bn_bwd(da, xg, None, True, scale, shift, mean, invstd, gg)
    assert rel_err(dx1, dx2) < 1e-6 and rel_err(dg1, dg2) < 1e-6 and rel_err(db1, db2) < 1e-6
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = F.max_pool2d(F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5)), 3, 2, 1)
    dx_ref, dg_ref, db_ref = torch.autograd.grad(yr, (xr, gr, br), dy.double())
    assert rel_err(dx1, dx_ref) < 2e-5 and rel_err(dg1, dg_ref) < 2e-5 and rel_err(db1, db_ref) < 2e-5


def test_batchnorm_backward_through_maxpool_survives_garbage_taps(ops):
    """an arg-max buffer nobody filled (every byte value) must give wrong numbers, never an access outside x"""
    B, C, H, W = 2, 8, 12, 16
    x = g(t(611, "x", (B, C, H, W)))
    dy = g(t(612, "dy", (B, C, H // 2, W // 2)))
    idx = torch.arange(B * C * (H // 2) * (W // 2), device=DEV).to(torch.int8).view(B, C, H // 2, W // 2)   # -128 .. 127
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    dx, dg, db = ops.bn_bwd_maxpool(dy, idx, x, True, one, zero, zero, one, one)
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all() and torch.isfinite(dg).all()


# ---------------------------------------------------------------- activations as pre-split bf16 planes (csrc/planes.hip)

def test_planes_are_the_exact_fp32_values(ops):
    """scat_planes_from_f32: hi + mid + lo reproduces every fp32 value exactly (3 x 8 significand bits), with and
    without the fused BatchNorm + ReLU, on planes whose pixel count is / is not a multiple of 4."""
    for n, (B, C, H) in enumerate([(3, 32, 14), (2, 64, 7), (2, 8, 5), (1, 96, 28)]):
        x = g(t(700 + n, "x", (B, C, H, H)) * 3.0)
        assert torch.equal(ops.planes_from(x).to_f32(), x)
        sc, sh = g(t(710 + n, "sc", (C,))), g(t(720 + n, "sh", (C,)))
        ref = torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1)))     # one fma per element
        got = ops.planes_from(x, sc, sh, True).to_f32()
        assert rel_err(got.cpu(), torch.relu(x.cpu().double() * sc.cpu().double().view(1, -1, 1, 1)
                                             + sh.cpu().double().view(1, -1, 1, 1)).float()) < 2e-7
        assert float((got < 0).sum()) == 0
        ref2 = ops.planes_from(x, sc, sh, False).to_f32()
        assert rel_err(ref2.cpu(), (x.cpu().double() * sc.cpu().double().view(1, -1, 1, 1)
                                    + sh.cpu().double().view(1, -1, 1, 1)).float()) < 2e-7


@pytest.mark.parametrize("cin,cout,H,B", [(64, 256, 56, 2), (256, 64, 56, 2), (128, 512, 28, 3), (512, 128, 28, 3),
                                          (256, 1024, 14, 5), (1024, 256, 14, 5), (512, 2048, 7, 7), (2048, 512, 7, 7),
                                          (32, 64, 9, 3), (96, 224, 5, 2)])
def test_conv1x1_planes_bit_identical(ops, cin, cout, H, B):
    """scat_conv1x1_planes (activations as planes, LDS-DMA staging) against scat_conv1x1_s1 (in-kernel split): the MFMA
    stream is the same, so forward, data gradient, accumulate and the epilogue's BatchNorm sums must agree BIT FOR BIT;
    ragged tiles (pixel count not a multiple of 128, rows not a multiple of 32) included.  Both LDS ring depths."""
    assert ops.get_math_mode() == 1
    x = g(t(730, "x", (B, cin, H, H)))
    w = g(t(731, "w", (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5))
    dy = g(t(732, "dy", (B, cout, H, H)))
    sc, sh = g(t(733, "sc", (cin,)).abs() + 0.5), g(t(734, "sh", (cin,)))
    base = g(t(735, "base", (B, cin, H, H)))
    ref_f = ops.conv2d_fwd(x, w, 1, 0)
    ref_tf = ops.conv2d_fwd(x, w, 1, 0, sc, sh, True)
    ref_d = ops.conv2d_dgrad_w(dy, w, tuple(x.shape), 1, 0)
    ref_da = ops.conv2d_dgrad_w(dy, w, tuple(x.shape), 1, 0, out=base.clone(), accumulate=True)
    xp, xtp, dyp = ops.planes_from(x), ops.planes_from(x, sc, sh, True), ops.planes_from(dy)
    for nb in (0, 2, 3):
        assert torch.equal(ops.conv1x1_planes(xp, w, lds_stages=nb), ref_f)
        assert torch.equal(ops.conv1x1_planes(xtp, w, lds_stages=nb), ref_tf)
        assert torch.equal(ops.conv1x1_planes(dyp, w, transposed=True, lds_stages=nb), ref_d)
        assert torch.equal(ops.conv1x1_planes(dyp, w, transposed=True, out=base.clone(), accumulate=True,
                                              lds_stages=nb), ref_da)
    # against the torch op itself
    want = F.conv2d(x.cpu().double(), w.cpu().double()).float()
    assert rel_err(ops.conv1x1_planes(xp, w).cpu(), want) < 2e-5


@pytest.mark.timeout(900)
@pytest.mark.parametrize("B,C,K,H", [(5, 256, 64, 28), (3, 512, 128, 28), (2, 256, 64, 56),
                                     (5, 192, 64, 28), (3, 320, 128, 28),      # a partial last 128-row tile
                                     (96, 256, 64, 56)])                       # the benchmarked size (layer1 -> layer2)
def test_bn_backward_sums_in_the_data_gradient_epilogue(ops, B, C, K, H):
    """The gradient of a Bottleneck output is completed by the next block's conv1 data gradient, accumulated onto the
    shortcut's gradient (models/resnet.py:93-96).  Asked to (ScatEpilogue x / mask / mean), that kernel's epilogue applies the
    output's sign mask and leaves bn3's backward sums: the masked gradient must be bit for bit what the accumulate followed
    by scat_bn_bwd_pre writes, coef3 / d-gamma / d-beta the same to rounding (fp32 tile sums, then fp64).

    And against a reference that is not the library: the masked accumulated gradient, coef3, d-gamma and d-beta from fp64
    torch on the CPU (tests/test_gpu_guard.py bn3_reference), 2e-5 for the gradient (a contraction) and the 1e-5 this test
    holds the sums to.  The sign of the block output is taken from the library's mask after that mask has been checked
    against the fp64 output wherever the fp64 value is not within rounding of zero (there either sign is right, and a
    reference that chose the other one would differ by a whole gradient element, not by rounding)."""
    # (the hash-based generator of synth takes seconds per 77 M elements: torch's for the batch-96 case)
    mk = t if B < 96 else (lambda seed, name, shape: torch.randn(shape, generator=torch.Generator().manual_seed(seed)))
    c3_c, res_c = mk(701, "c3", (B, C, H, H)) * 1.3 + 0.2, mk(702, "res", (B, C, H, H))
    dc1_c, w1_c, g_old_c = mk(705, "dc1", (B, K, H, H)), t(706, "w1", (K, C, 1, 1)) * 0.1, mk(707, "gold", (B, C, H, H))
    c3 = g(c3_c)
    res = g(res_c)
    gamma = g(torch.from_numpy(synth.uniform(703, "g", (C,), 0.5, 1.5)))
    beta = g(torch.from_numpy(synth.uniform(704, "b", (C,), -0.3, 0.3)))
    rm, rv = g(torch.zeros(C)), g(torch.ones(C))
    mean, invstd, scale, shift = ops.bn_train_stats(c3, gamma, beta, rm, rv)
    out, mask = ops.bn_apply(c3, scale, shift, res, True, want_mask=True)
    assert mask is not None
    dc1 = g(dc1_c)
    w1 = g(w1_c)
    g_old = g(g_old_c)
    # reference: accumulate, then the reduction pass
    ref = ops.conv2d_dgrad_w(dc1, w1, (B, C, H, H), 1, 0, out=g_old.clone(), accumulate=True)
    coef_r, dg_r, db_r = ops.bn_bwd_pre(ref, c3, True, scale, shift, mean, invstd, gamma, y_mask=mask)
    # the same call with the request
    new = ops.conv2d_dgrad_w(dc1, w1, (B, C, H, H), 1, 0, out=g_old.clone(), accumulate=True, bnb=(c3, mask, mean))
    assert new.scat_bnb is not None, ops.lib().scat_last_kernel()
    part, groups = new.scat_bnb
    assert groups > 0 and ops.lib().scat_last_kernel().decode().endswith("_epibn"), ops.lib().scat_last_kernel()
    coef_n, dg_n, db_n = ops.bn_bwd_pre_partials(part, groups, (B, C, H, H), mean, invstd, gamma)
    assert torch.equal(new, ref)
    assert rel_err(dg_n, dg_r) < 1e-5 and rel_err(db_n, db_r) < 1e-5
    for k in range(3):
        assert rel_err(coef_n[k], coef_r[k]) < 1e-5
    # the request belonged to that call: the next one without it is the plain accumulate again
    again = ops.conv2d_dgrad_w(dc1, w1, (B, C, H, H), 1, 0, out=g_old.clone(), accumulate=True)
    assert getattr(again, "scat_bnb", None) is None and not ops.lib().scat_last_kernel().decode().endswith("_epibn")
    assert not torch.equal(again, ref)
    del again, ref, res, g_old, dc1
    # ---- fp64, independent of the library's own unfused pair
    from test_gpu_guard import bn3_reference

    v = lambda a: a.cpu().double().view(1, -1, 1, 1)
    a64, r64 = c3_c.double() * v(scale), res_c.double()
    y64 = a64 + v(shift) + r64
    sure = y64.abs() > 4e-7 * (a64.abs() + v(shift).abs() + r64.abs())      # (two fp32 roundings of the fused form)
    del a64, r64
    sign = ((mask.view(-1, 1) >> torch.arange(4, device=DEV, dtype=torch.uint8)) & 1).bool().view(B, C, H, H).cpu()
    assert float(sure.double().mean()) > 0.9999 and torch.equal(sign[sure], (y64 > 0)[sure])
    del y64, sure
    g64, coef64, dg64, db64 = bn3_reference(c3_c, sign, gamma.cpu(), mean.cpu(), invstd.cpu(), g_old_c, dc1_c, w1_c)
    e_g, e_dg, e_db = rel_err(new, g64), rel_err(dg_n, dg64), rel_err(db_n, db64)
    e_c = [rel_err(coef_n[k], coef64[k]) for k in range(3)]
    print(f"armed bn3 epilogue ({B},{C},{K},{H}) against fp64: g {e_g:.2e} d-gamma {e_dg:.2e} d-beta {e_db:.2e} coef3 "
          f"{e_c[0]:.2e} {e_c[1]:.2e} {e_c[2]:.2e}")
    assert e_g < 2e-5 and e_dg < 1e-5 and e_db < 1e-5 and max(e_c) < 1e-5
    # the unfused pair against the same reference
    assert rel_err(dg_r, dg64) < 1e-5 and rel_err(db_r, db64) < 1e-5
    assert all(rel_err(coef_r[k], coef64[k]) < 1e-5 for k in range(3))


# ---------------------------------------------------------------------------------------------------------------
# HRNet-W32 (c = 32, 224 x 224; BASELINE configs[3]) at the benchmarked batch 96: every convolution geometry of the
# backbone except layer1's four Bottlenecks (ResNet's block executor, in CONVS above), plus the wrapper's 3x3/2 512->128
# reduction on the 28x28 view (models/hand_net.py EncoderTransformerHRNet).  Each geometry runs the way the step runs it:
#   "cbr"  : hrnet._CbrFn — forward with the BatchNorm sums, taken about a stats_shift, in its epilogue; the BN finish; dW; dX
#   "block": hrnet._BasicBlockFn — conv1 forward; conv2 forward and dW with bn1 + ReLU in the operand load; dW plain;
#            dX plain (conv2) and accumulating onto the residual gradient (conv1)
#   "plain": snn.Conv2d — forward, dW, dX (the exchange's 1x1s, the last 3x3/2 of each strided chain, the wrapper's reduction)
#   "bias" : snn.Conv2d with a bias — final_layer (forward + bias, the bias gradient's column sum)
# tests/test_hrnet_geometry.py holds the table to the oracle's HRNet-W32: every geometry it runs is here or in CONVS.
HRNET_B96 = {
    # (Cin, Cout, k, stride, H = W of the input): roles
    (3, 64, 3, 2, 224): ("cbr",), (64, 64, 3, 2, 112): ("cbr",), (256, 32, 3, 1, 56): ("cbr",),
    (256, 64, 3, 2, 56): ("cbr",), (32, 32, 3, 2, 56): ("cbr",), (32, 32, 3, 2, 28): ("cbr",),
    (64, 64, 3, 2, 28): ("cbr",), (64, 128, 3, 2, 28): ("cbr", "plain"), (128, 256, 3, 2, 14): ("cbr", "plain"),
    (32, 32, 3, 1, 56): ("block",), (64, 64, 3, 1, 28): ("block",), (128, 128, 3, 1, 14): ("block",),
    (256, 256, 3, 1, 7): ("block",),
    (32, 64, 3, 2, 56): ("plain",), (32, 128, 3, 2, 28): ("plain",), (32, 256, 3, 2, 14): ("plain",),
    (64, 256, 3, 2, 14): ("plain",), (64, 32, 1, 1, 28): ("plain",), (128, 32, 1, 1, 14): ("plain",),
    (128, 64, 1, 1, 14): ("plain",), (256, 32, 1, 1, 7): ("plain",), (256, 64, 1, 1, 7): ("plain",),
    (256, 128, 1, 1, 7): ("plain",), (32, 128, 1, 1, 56): ("bias",),
    (512, 128, 3, 2, 28): ("plain",),      # the wrapper's conv1x1_channel_reduction (a 3x3/2 despite its name)
}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cin,cout,k,s,H", sorted(HRNET_B96))
def test_hrnet_conv_batch96_instantiations(ops, cin, cout, k, s, H):
    B, p = 96, k // 2
    roles = HRNET_B96[(cin, cout, k, s, H)]
    name = f"hrnet {cin}->{cout} k{k} s{s} {H}x{H}"
    gen = torch.Generator().manual_seed(3000 + cin + 7 * cout + 31 * k + 5 * s + H)
    z = torch.randn((B, cin, H, H), generator=gen)
    # what the step feeds it: the image (stem) or a ReLU output (every other plain read); "block" also reads z raw
    x = z * 0.5 + 0.1 if cin == 3 else F.relu(z)
    w = torch.randn((cout, cin, k, k), generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn((cout,), generator=gen) * 0.2
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y = F.conv2d(x64, w64, stride=s, padding=p)
    dy = torch.randn(tuple(y.shape), generator=gen)
    dx_ref, dw_ref = torch.autograd.grad(y, (x64, w64), dy.double())
    y = y.detach()
    xg, wg, dyg = g(x), g(w), g(dy)
    wp = ops.WeightPrep()          # prepared weights like the network's: first call registers, run() re-lays, then w_ready=1

    def prepared(fn):
        fn()
        wp.run(True)
        return fn()

    if "cbr" in roles:
        # the BatchNorm sums about the previous step's batch mean (resnet._BNState leaves it in bn._stat_ref)
        mean64, var64 = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
        shift = g((mean64 + 0.05 * var64.sqrt() * torch.randn((cout,), generator=gen).double()).float())
        yg = prepared(lambda: ops.conv2d_fwd(xg, wg, s, p, wp=wp, stats=True, stats_shift=shift))
        _b96_note(f"{name} fwd_stats", _label(ops))
        assert rel_err(yg, y) < 2e-5
        had_partials = getattr(yg, "scat_stats", None) is not None
        gamma, beta = g(torch.rand((cout,), generator=gen) + 0.5), g(torch.rand((cout,), generator=gen) - 0.5)
        rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
        mean, invstd, scale, bshift = ops.bn_train_stats(yg, gamma, beta, rm, rv)
        assert rel_err(mean, mean64) < 2e-5, had_partials
        assert rel_err(invstd, (var64 + 1e-5).rsqrt()) < 2e-5, had_partials
        assert rel_err(rv, 0.9 + 0.1 * y.var(dim=(0, 2, 3), unbiased=True)) < 2e-5, had_partials
        del yg
    if "plain" in roles or "block" in roles:
        yg = prepared(lambda: ops.conv2d_fwd(xg, wg, s, p, wp=wp))
        _b96_note(f"{name} fwd", _label(ops))
        assert rel_err(yg, y) < 2e-5
        del yg
    if "bias" in roles:
        yb = prepared(lambda: ops.conv2d_fwd(xg, wg, s, p, bias=g(bias), wp=wp))
        _b96_note(f"{name} fwd_bias", _label(ops))
        assert rel_err(yb, y + bias.double().view(1, -1, 1, 1)) < 2e-5
        del yb
        db = ops.colsum(dyg.permute(0, 2, 3, 1).reshape(-1, cout).contiguous())
        assert rel_err(db, dy.double().sum(dim=(0, 2, 3))) < 1e-5

    dwg = ops.conv2d_wgrad(dyg, xg, tuple(w.shape), s, p)
    _b96_note(f"{name} wgrad", _label(ops))
    assert rel_err(dwg, dw_ref) < 2e-5
    del dwg
    if cin != 3:                   # (the image needs no gradient)
        dxg = prepared(lambda: ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p, wp=wp))
        _b96_note(f"{name} dgrad", _label(ops))
        assert rel_err(dxg, dx_ref) < 2e-5
        del dxg

    if "block" in roles:
        # conv2 reads relu(bn1(c1)) formed in its operand load, forward and for dW
        sc = torch.rand((cin,), generator=gen) + 0.5
        sh = torch.rand((cin,), generator=gen) - 0.5
        a64 = F.relu(z.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        ya = F.conv2d(a64, w.double(), stride=s, padding=p)
        dwa_ref = torch.nn.grad.conv2d_weight(a64, tuple(w.shape), dy.double(), stride=s, padding=p)
        zg, tfa = g(z), (g(sc), g(sh), True)
        yt = prepared(lambda: ops.conv2d_fwd(zg, wg, s, p, *tfa, wp=wp))
        _b96_note(f"{name} fwd_tf", _label(ops))
        assert rel_err(yt, ya.detach()) < 2e-5
        del yt
        dwt = ops.conv2d_wgrad(dyg, zg, tuple(w.shape), s, p, *tfa)
        _b96_note(f"{name} wgrad_tf", _label(ops))
        assert rel_err(dwt, dwa_ref) < 2e-5
        del dwt
        # conv1's data gradient accumulates straight into the residual gradient
        base = torch.randn(tuple(x.shape), generator=gen)
        dxa = ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p, out=g(base), accumulate=True, wp=wp)
        _b96_note(f"{name} dgrad_acc", _label(ops))
        assert rel_err(dxa, dx_ref + base.double()) < 2e-5


# ---------------------------------------------------------------------------------------------------------------
# FAVOR+ core (csrc/performer.hip) against the fp64 formula of oracle.performer_block (prm_exp, D, kptv), forward, the
# saved tensors and the backward, at the performer config's shape (B = 96, T = 21 tokens, 16 heads of e = 49, m = 24) and
# at the kernels' edges: m = 64 / 65 / 128 (the lane loops and performer_bwd3_kernel's sh[4][2][128] LDS bound), e > 64,
# T = 1, and a B*H*T that is not a multiple of 4 (a dead wave in the last workgroup of bwd1 / bwd3 / out).
def _favor64(kqv, w):
    """kqv[B,T,H,3e] (k | q | v), w[m,e] -> y[B,T,H*e], kp, qp [B,H,T,m], kptv [B,H,e,m], ksum [B,H,m], D [B,H,T]"""
    B, T, H, e3 = kqv.shape
    e, m = e3 // 3, w.shape[0]
    k, q, v = (t.permute(0, 2, 1, 3) for t in kqv.split(e, dim=-1))        # [B,H,T,e]

    def prm_exp(t):
        return torch.exp(t @ w.t() - (t * t).sum(dim=-1, keepdim=True) / 2) / math.sqrt(m)

    kp, qp = prm_exp(k), prm_exp(q)
    ksum = kp.sum(dim=2)
    D = (qp * ksum.unsqueeze(2)).sum(dim=-1)
    kptv = torch.einsum("bhtn,bhtm->bhnm", v, kp)
    y = torch.einsum("bhtm,bhnm->bhtn", qp, kptv) / D.unsqueeze(-1)
    return y.permute(0, 2, 1, 3).reshape(B, T, H * e), kp, qp, kptv, ksum, D


@pytest.mark.parametrize("B,T,H,e,m", [(96, 21, 16, 49, 24), (3, 21, 16, 49, 64), (2, 21, 8, 49, 65), (2, 21, 4, 49, 128),
                                       (2, 9, 3, 100, 24), (3, 5, 2, 130, 65), (5, 1, 4, 49, 24), (3, 7, 5, 49, 24),
                                       (1, 3, 1, 70, 128)])
def test_performer_core(ops, B, T, H, e, m):
    gen = torch.Generator().manual_seed(4000 + B + 3 * T + 5 * H + 7 * e + 11 * m)
    kqv = torch.randn((B, T, H, 3 * e), generator=gen) * (1.5 / e ** 0.5)
    w = torch.randn((m, e), generator=gen)
    k64 = kqv.double().requires_grad_(True)
    y64, kp, qp, kptv, ksum, D = _favor64(k64, w.double())
    dy = torch.randn(tuple(y64.shape), generator=gen)
    (dk_ref,) = torch.autograd.grad(y64, (k64,), dy.double())
    yg, saved = ops.performer_fwd(g(kqv), g(w), H)
    assert rel_err(yg, y64) < 2e-5
    for got, ref in zip(saved, (kp, qp, kptv, ksum, D)):
        assert rel_err(got, ref) < 2e-5
    dkg = ops.performer_bwd(g(dy), g(kqv), g(w), yg, saved)
    for sl in range(3):            # k, q, v slices on their own: each has its own formula in performer_bwd3_kernel
        got, ref = dkg[..., sl * e:(sl + 1) * e], dk_ref[..., sl * e:(sl + 1) * e]
        if T == 1 and sl < 2:      # one token: y = v whatever k and q are, so dk = dq = 0 up to rounding (of dv's size)
            assert float((got.cpu().double() - ref).abs().max()) < 2e-5 * float(dk_ref.abs().max()), "kqv"[sl]
        else:
            assert rel_err(got, ref) < 2e-5, "kqv"[sl]


def test_performer_core_rejects_m_above_128(ops):
    from scat_amd._lib import ScatError

    kqv, w = torch.zeros((1, 2, 1, 3 * 8), device=DEV), torch.zeros((129, 8), device=DEV)
    with pytest.raises(ScatError, match="m <= 128"):
        ops.performer_fwd(kqv, w, 1)
    y, saved = ops.performer_fwd(kqv, w[:128].contiguous(), 1)
    with pytest.raises(ScatError, match="m <= 128"):
        ops.performer_bwd(torch.zeros_like(y), kqv, w, y, saved)


# ---------------------------------------------------------------------------------------------------------------
# The small ops of the HRNet exchange, the HRNet wrapper and the performer's train mode, on their own.
@pytest.mark.parametrize("B,C,H,W,f", [(2, 3, 7, 5, 2), (3, 4, 8, 6, 2), (2, 3, 7, 5, 4), (1, 5, 4, 6, 4), (2, 3, 3, 5, 8),
                                       (1, 2, 2, 2, 8), (1, 1, 1, 1, 2),
                                       # the HRNet-W32 exchange at batch 96: 2^(j-i) onto the 56 / 28 / 14 maps
                                       (96, 32, 28, 28, 2), (96, 32, 14, 14, 4), (96, 32, 7, 7, 8), (96, 64, 14, 14, 2),
                                       (96, 64, 7, 7, 4), (96, 128, 7, 7, 2)])
def test_upsample_nearest(ops, B, C, H, W, f):
    gen = torch.Generator().manual_seed(5000 + B + C + H * W + f)
    x = torch.randn((B, C, H, W), generator=gen)
    dy = torch.randn((B, C, H * f, W * f), generator=gen)
    y = ops.upsample_nearest_fwd(g(x), f)
    assert torch.equal(y.cpu(), F.interpolate(x, scale_factor=float(f), mode="nearest"))
    ref = dy.double().reshape(B, C, H, f, W, f).sum(dim=(3, 5))          # the f x f block sums
    assert rel_err(ops.upsample_nearest_bwd(g(dy), f), ref) < 1e-5


@pytest.mark.parametrize("B,T,D", [(96, 128, 196), (96, 22, 784), (3, 7, 5), (2, 1, 61), (5, 33, 1), (4, 129, 197)])
def test_token_mean(ops, B, T, D):
    gen = torch.Generator().manual_seed(5100 + B + T + D)
    x = torch.randn((B, T, D), generator=gen) + 0.5
    dy = torch.randn((B, D), generator=gen)
    assert rel_err(ops.token_mean_fwd(g(x)), x.double().mean(dim=1)) < 1e-5
    dx = ops.token_mean_bwd(g(dy), T)
    assert tuple(dx.shape) == (B, T, D)
    assert rel_err(dx, (dy.double() / T).unsqueeze(1).expand(B, T, D)) < 1e-6


@pytest.mark.parametrize("n,p", [(96 * 21 * 784, 0.1), (100003, 0.1), (1023, 0.5), (7, 0.1), (1, 0.3), (4099, 0.0),
                                 (96 * 21 * 3136, 0.1)])
def test_dropout(ops, n, p):
    """the keep mask is oracle.hash_dropout_mask element for element, kept values scale by 1/(1-p) (in fp32, as
    scat_dropout forms it), and snn.Dropout's backward applies the same mask"""
    import random

    from oracle.scat_oracle import hash_dropout_mask
    from scat_amd import nn as snn

    gen = torch.Generator().manual_seed(5200 + n)
    x = torch.randn((n,), generator=gen) + 0.01          # (no exact zeros: a zero output then means "dropped")
    dy = torch.randn((n,), generator=gen)
    seed = random.Random(n).getrandbits(63)
    keep = hash_dropout_mask(n, p, seed)
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    y = ops.dropout(g(x), p, seed).cpu()
    assert torch.equal((y != 0).double(), keep)
    assert torch.equal(y, x * keep.float() * scale)
    assert rel_err(y, x.double() * keep / (1.0 - p)) < 1e-6
    if 0 < p and n > 1000:
        assert abs(1.0 - keep.mean().item() - p) < 6 * (p * (1 - p) / n) ** 0.5
    # through the module: the seed is drawn from python random at forward, the backward regenerates the same mask
    mod = snn.Dropout(p).train()
    xg = g(x).requires_grad_(True)
    random.seed(n)
    yg = mod(xg)
    random.seed(n)
    keep2 = hash_dropout_mask(n, p, random.getrandbits(63)) if p > 0 else torch.ones(n, dtype=torch.float64)
    yg.backward(g(dy))
    assert torch.equal(yg.detach().cpu(), x * keep2.float() * scale)
    assert torch.equal(xg.grad.cpu(), dy * keep2.float() * scale)


# The HRNet wrapper's transformer at batch 96 runs on 96 x 128 = 12 288 tokens: the qkv projection (12 288 x 1 536 x 196)
# and its weight / data gradients cross GEMM_SPLIT_MIN and run on scat_gemm_split, the output and MLP projections stay on
# the fp32 engine — at a row count no other test uses.
@pytest.mark.parametrize("N,K,has_bias", [(1536, 196, False), (196, 512, True), (392, 196, True), (196, 392, True)])
def test_linear_hrnet_wrapper_tokens(ops, N, K, has_bias):
    M = 96 * 128
    gen = torch.Generator().manual_seed(5300 + N + K)
    x = torch.randn((M, K), generator=gen)
    w = torch.randn((N, K), generator=gen) * K ** -0.5
    b = torch.randn((N,), generator=gen) if has_bias else None
    dy = torch.randn((M, N), generator=gen)
    x64, w64 = x.double(), w.double()
    y = x64 @ w64.t() + (b.double() if has_bias else 0.0)

    def on_split(m, n, k):
        ok = ops._gemm_split_ok(m, n, k)
        assert ("gemm_split" in _label(ops)) == ok, (_label(ops), m, n, k)
        return ok

    assert rel_err(ops.linear_fwd(g(x), g(w), g(b) if has_bias else None), y) < 2e-5
    split = [on_split(M, N, K)]
    assert rel_err(ops.linear_dgrad(g(dy), g(w)), dy.double() @ w64) < 2e-5
    split.append(on_split(M, K, N))
    assert rel_err(ops.linear_wgrad(g(dy), g(x)), dy.double().t() @ x64) < 2e-5
    split.append(on_split(N, K, M))
    assert rel_err(ops.colsum(g(dy)), dy.double().sum(0)) < 1e-5
    # the qkv projection is the one that crosses the threshold (in the default product mode)
    assert all(split) == (N == 1536 and ops.get_math_mode() == 1 and ops.GEMM_SPLIT), split
