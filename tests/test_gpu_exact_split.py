"""Every bf16x3 split kernel (csrc/split.h) held to its six terms on exact-sum data, on a real MI355X.

The inputs (tests/_exact_split.py, designs A, B and C) make every order of fp32 accumulation exact, so the fp64 torch
operation is the bit-exact answer of any correct kernel, whatever its tiles, its split-K and the order inside the MFMA:
every assertion is torch.equal against fp64.  A lost, doubled or mis-paired term changes nearly every output of at
least one design (tests/test_exact_split.py).  Each case first checks its data on the CPU (the bound, and that at least
99 % of the outputs receive a non-zero product), then runs the fp32-MFMA twin of the kernel (product mode 0) where one
exists: if that is inexact the data is wrong, not the kernel.

Fused operands: relu(x*sc + sh) with sc in {1/2, 1, 2}, sh = 0 and ca*g + cb*z + cc with ca in {+-1, +-2}, cb = cc = 0
are exact, and the raw tensors are chosen so that the operand formed in the load is the design's.  BatchNorm sums from
the epilogues and everything downstream of a softmax are not exact-sum quantities and stay with the other tests."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_split as E  # noqa: E402

from scat_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


def _data(which, left_shape, right_shape, seed, terms, abs_sum, extra=0.0, reachable=None, right_weight=None):
    l, r, s = E.build(which, left_shape, right_shape, seed, terms, abs_sum, extra, right_weight=right_weight)
    share = E.fed_share(s, reachable)
    assert share >= 0.99, "only %.3f of the outputs receive a non-zero product" % share
    return l, r


def _check(ops, math_mode, run, ref, which, prefix, has=(), hasnot=(), twin=None):
    """twin() in product mode 0 (the control: the data), then run() in mode 1 (the kernel), both bit-for-bit fp64"""
    lib = ops.lib()
    if twin is not None:
        math_mode(0)
        got0 = twin()
        lab0 = lib.scat_last_kernel().decode()
        assert "_split_" not in lab0, lab0
        assert E.is_exact(got0, ref), "design %s: the fp32 twin %s is inexact - the data is wrong, not the kernel" % (which, lab0)
    math_mode(1)
    got = run()
    lab = lib.scat_last_kernel().decode()
    assert lab.startswith(prefix) and all(h in lab for h in has) and not any(h in lab for h in hasnot), (lab, prefix, has)
    assert E.is_exact(got, ref), "design %s: %s is not the fp64 answer on exact-sum data (%d of %d outputs differ)" % (
        which, lab, int((got.cpu().double() != ref).sum()), ref.numel())


def _relu_form(seed, a, C):
    """raw, scale, shift with relu(raw * scale + shift) == relu(a) exactly: scale in {1/2, 1, 2}, shift = 0"""
    sc = E.pow2_scale(seed, "sc", C)
    return a / sc.view(1, -1, 1, 1), sc, torch.zeros(C)


def conv_fwd(ops, math_mode, which, seed, B, cin, cout, H, W, k, s, prefix, has=(), bias=False, tf=False, twin=True):
    p = k // 2
    act = F.relu if tf else (lambda v: v)
    a, w = _data(which, (B, cin, H, W), (cout, cin, k, k), seed, cin * k * k / (2 if tf else 1),
                 lambda l, r: F.conv2d(act(l).double().abs(), r.double().abs(), stride=s, padding=p), 2.0 * bias)
    b = E.small_ints(seed, "bias", (cout,)) if bias else None
    ref = F.conv2d(act(a).double(), w.double(), b.double() if bias else None, stride=s, padding=p)
    x, tfa = a, ()
    if tf:
        x, sc, sh = _relu_form(seed, a, cin)
        tfa = (g(sc), g(sh), True)
    run = lambda: ops.conv2d_fwd(g(x), g(w), s, p, *tfa, bias=g(b) if bias else None)
    _check(ops, math_mode, run, ref, which, prefix, has + (("_tf",) if tf else ()), twin=run if twin else None)


def conv_dgrad(ops, math_mode, which, seed, B, cin, cout, H, W, k, s, prefix, has=(), accumulate=False, bnb=False):
    p = k // 2
    OH, OW = ops.conv_out_hw(H, W, k, s, p)
    opad = (H - ((OH - 1) * s - 2 * p + k), W - ((OW - 1) * s - 2 * p + k))
    T = lambda dy, w: F.conv_transpose2d(dy, w, stride=s, padding=p, output_padding=opad)
    taps = k * k if s == 1 else ((k + 1) // 2) ** 2                # of the parity class with the most taps
    reach = T(torch.ones(B, cout, OH, OW, dtype=torch.float64), torch.ones(cout, cin, k, k, dtype=torch.float64)) > 0
    # 3x3 / stride 2: a pixel's parity class takes the centre tap alone, two edge taps or the four corner taps
    rw = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]]).numpy() if (s, k) == (2, 3) else None
    dy, w = _data(which, (B, cout, OH, OW), (cout, cin, k, k), seed, cout * taps,
                  lambda l, r: T(l.double().abs(), r.double().abs()), 3.0 * accumulate, reach, rw)
    base = E.small_ints(seed, "base", (B, cin, H, W), 3) if accumulate else None
    ref = T(dy.double(), w.double()) + (base.double() if accumulate else 0.0)
    out = lambda: g(base) if accumulate else None                  # a fresh copy for every launch
    plain = lambda: ops.conv2d_dgrad_w(g(dy), g(w), (B, cin, H, W), s, p, out=out(), accumulate=accumulate)
    run = plain
    if bnb:     # operand ca*g + cb*z + cc formed in the load: g = dy / ca, z arbitrary, cb = cc = 0
        coef = E.bnb_coef(seed, "coef", cout)
        gs = dy / coef[0].view(1, -1, 1, 1)
        z = torch.from_numpy(synth.normal_like(seed, "z", (B, cout, OH, OW)))
        run = lambda: ops.conv1x1_dgrad_bnb(g(gs), g(z), g(coef), g(w), (B, cin, H, W), out=out(), accumulate=accumulate)
    _check(ops, math_mode, run, ref, which, prefix, has, twin=plain)


def conv_wgrad(ops, math_mode, which, seed, B, cin, cout, H, W, k, s, prefix, has=(), hasnot=(), tf=False, bnb=False,
               twin=True):
    p = k // 2
    OH, OW = ops.conv_out_hw(H, W, k, s, p)
    ws = (cout, cin, k, k)
    act = F.relu if tf else (lambda v: v)
    wg = lambda a, dy: torch.nn.grad.conv2d_weight(a, ws, dy, stride=s, padding=p)
    dy, a = _data(which, (B, cout, OH, OW), (B, cin, H, W), seed, B * OH * OW / (2 if tf else 1),
                  lambda l, r: wg(act(r).double().abs(), l.double().abs()))
    ref = wg(act(a).double(), dy.double())
    x, tfa = a, ()
    if tf:
        x, sc, sh = _relu_form(seed, a, cin)
        tfa = (g(sc), g(sh), True)
    plain = lambda: ops.conv2d_wgrad(g(dy), g(x), ws, s, p, *tfa)
    run = plain
    if bnb:
        coef = E.bnb_coef(seed, "coef", cout)
        gs = dy / coef[0].view(1, -1, 1, 1)
        z = torch.from_numpy(synth.normal_like(seed, "z", (B, cout, OH, OW)))
        run = lambda: ops.conv1x1_wgrad_bnb(g(gs), g(z), g(coef), g(x), ws, *tfa)
    _check(ops, math_mode, run, ref, which, prefix, has + (("_tf",) if tf else ()) + (("_bnb",) if bnb else ()), hasnot,
           twin=plain if twin else None)


DESIGNS = pytest.mark.parametrize("which", E.DESIGNS)


# ---------------------------------------------------------------- conv1x1.hip: pointwise, taps, stem, gemm_split

@DESIGNS
@pytest.mark.parametrize("B,cin,cout,H,W", [(2, 48, 80, 9, 13), (5, 256, 128, 14, 14)])
def test_conv1x1_split(ops, monkeypatch, math_mode, which, B, cin, cout, H, W):
    """scalar and vector pixel staging, ragged and full tiles: forward + bias, forward with the fused transform, data
    gradient, data gradient into a base, data gradient with the folded BatchNorm backward (alone and into a base)"""
    monkeypatch.setattr(ops, "PW_MIN_C", 0)          # (the fp32 twin is the pointwise kernel at these channel counts too)
    a = (ops, math_mode, which)
    conv_fwd(*a, 100, B, cin, cout, H, W, 1, 1, "conv1x1_split_", bias=True)
    conv_fwd(*a, 101, B, cin, cout, H, W, 1, 1, "conv1x1_split_", tf=True)
    conv_dgrad(*a, 102, B, cin, cout, H, W, 1, 1, "conv1x1_split_")
    conv_dgrad(*a, 103, B, cin, cout, H, W, 1, 1, "conv1x1_split_", accumulate=True)
    conv_dgrad(*a, 104, B, cin, cout, H, W, 1, 1, "conv1x1_split_", ("_bnb",), bnb=True)
    conv_dgrad(*a, 105, B, cin, cout, H, W, 1, 1, "conv1x1_split_", ("_bnb",), accumulate=True, bnb=True)


def pc_exact_case(ops, B, cin, cout, H, W, expect):
    """the roles of test_gpu_ops._pc_case on exact-sum data, for its child process (SCAT_PC is read once per process):
    forward + bias and forward with the fused transform at M = cout >= 256 rows, the data gradient and the data
    gradient into a base of the transposed role (M >= 256 input channels)"""
    saved = ops.get_math_mode()
    mode = lambda m: ops.set_math_mode(m)
    try:
        for which in E.DESIGNS:
            a = (ops, mode, which)
            conv_fwd(*a, 110, B, cin, cout, H, W, 1, 1, expect, bias=True)
            conv_fwd(*a, 111, B, cin, cout, H, W, 1, 1, expect, tf=True)
            conv_dgrad(*a, 112, B, cout, cin, H, W, 1, 1, expect)
            conv_dgrad(*a, 113, B, cout, cin, H, W, 1, 1, expect, accumulate=True)
    finally:
        ops.set_math_mode(saved)


@DESIGNS
@pytest.mark.parametrize("B,cin,cout,H,W,k", [(2, 32, 72, 9, 13, 3), (2, 64, 136, 30, 5, 1)])
def test_taps_stride2_forward(ops, math_mode, which, B, cin, cout, H, W, k):
    """scat_conv2d_fwd_split: the stride-2 3x3 and 1x1 forward, with bias and with the fused transform"""
    a = (ops, math_mode, which)
    conv_fwd(*a, 120, B, cin, cout, H, W, k, 2, "conv%dx%d_s2_split_" % (k, k), bias=True)
    conv_fwd(*a, 121, B, cin, cout, H, W, k, 2, "conv%dx%d_s2_split_" % (k, k), tf=True)


@DESIGNS
@pytest.mark.parametrize("H,W", [(13, 9), (8, 14)])
@pytest.mark.parametrize("k", [3, 1])
def test_taps_stride2_dgrad(ops, math_mode, which, H, W, k):
    """the parity classes of the stride-2 data gradient on the taps kernel (ragged class grids), alone and into a base;
    for 1x1 only the even pixels can receive a product (the share is taken over those), the others must be exactly 0"""
    a = (ops, math_mode, which)
    conv_dgrad(*a, 130, 2, 12, 48, H, W, k, 2, "dgrad_s2_class", ("_split_",))
    conv_dgrad(*a, 131, 2, 12, 48, H, W, k, 2, "dgrad_s2_class", ("_split_",), accumulate=True)


@DESIGNS
@pytest.mark.parametrize("B,cout,H,W", [(3, 64, 38, 54), (1, 96, 32, 18)])
def test_stem_forward(ops, math_mode, which, B, cout, H, W):
    conv_fwd(ops, math_mode, which, 140, B, 3, cout, H, W, 7, 2, "conv7x7_s2_split_")


@DESIGNS
@pytest.mark.parametrize("M,N,K", [(300, 200, 147), (2016, 196, 294)])
def test_gemm_split(ops, monkeypatch, math_mode, which, M, N, K):
    """scat_gemm_split directly (+ bias; transposed A into a base) and through linear_fwd / linear_dgrad /
    linear_wgrad above the split threshold (set to 0 here: by default only the largest projection is above it); the
    fp32 twin is the same call below the threshold, on the fp32 engine"""
    monkeypatch.setattr(ops, "GEMM_SPLIT_MIN", 0)
    absmm = lambda l, r: l.double().abs() @ r.double().abs()
    lab = lambda: ops.lib().scat_last_kernel().decode()
    a, b = _data(which, (M, K), (K, N), 150, K, absmm, 3.0)
    bias, base = E.small_ints(150, "bias", (N,), 3), E.small_ints(150, "base", (M, N), 3)
    ref = a.double() @ b.double()
    math_mode(0)
    assert E.is_exact(ops.linear_fwd(g(a), g(b.t()), g(bias)), ref + bias.double()), (which, "data", lab())
    math_mode(1)
    c = ops.gemm_split(g(a), 0, g(b), torch.empty(M, N, device=DEV), M, N, K, g(bias))
    assert lab().startswith("gemm_split_") and E.is_exact(c, ref + bias.double()), (which, lab())
    c = ops.gemm_split(g(a.t()), 1, g(b), g(base), M, N, K, None, accumulate=True)
    assert lab().startswith("gemm_split_") and E.is_exact(c, ref + base.double()), (which, lab())
    # the three roles of a projection y[M, N] = x[M, K] w[N, K]^T + bias
    x, w = _data(which, (M, K), (N, K), 151, K, lambda l, r: absmm(l, r.t()), 3.0)
    dy, w2 = _data(which, (M, N), (N, K), 152, N, absmm)
    dy3, x3 = _data(which, (M, N), (M, K), 153, M, lambda l, r: absmm(l.t(), r))
    roles = [(lambda: ops.linear_fwd(g(x), g(w), g(bias)), x.double() @ w.double().t() + bias.double()),
             (lambda: ops.linear_dgrad(g(dy), g(w2)), dy.double() @ w2.double()),
             (lambda: ops.linear_wgrad(g(dy3), g(x3)), dy3.double().t() @ x3.double())]
    for n, (run, ref) in enumerate(roles):
        math_mode(0)
        assert E.is_exact(run(), ref) and "gemm_split" not in lab(), (which, n, "data", lab())
        math_mode(1)
        got = run()
        assert lab().startswith("gemm_split_"), (n, lab())
        assert E.is_exact(got, ref), (which, n, lab())


# ---------------------------------------------------------------- conv3x3.hip

@DESIGNS
@pytest.mark.parametrize("B,cin,cout,H,W", [(2, 20, 72, 9, 13), (3, 36, 64, 7, 7)])
def test_conv3x3_split(ops, math_mode, which, B, cin, cout, H, W):
    """ragged channel counts, tiles that straddle images: forward, forward with the fused transform, data gradient
    (alone and into a base)"""
    a = (ops, math_mode, which)
    conv_fwd(*a, 200, B, cin, cout, H, W, 3, 1, "conv3x3_split_")
    conv_fwd(*a, 201, B, cin, cout, H, W, 3, 1, "conv3x3_split_", tf=True)
    conv_dgrad(*a, 202, B, cin, cout, H, W, 3, 1, "conv3x3_split_", ("_dgrad",))
    conv_dgrad(*a, 203, B, cin, cout, H, W, 3, 1, "conv3x3_split_", ("_dgrad",), accumulate=True)


# ---------------------------------------------------------------- weight gradients

@DESIGNS
@pytest.mark.parametrize("B,cin,cout,H,W,k,s", [(2, 20, 136, 9, 13, 3, 1), (2, 144, 136, 9, 13, 1, 1), (2, 20, 136, 9, 13, 3, 2)])
def test_wgrad_split(ops, math_mode, which, B, cin, cout, H, W, k, s):
    """conv_wgrad_split.hip: 3x3 and 1x1 at stride 1, 3x3 at stride 2, with and without the fused transform"""
    prefix = "wgrad%dx%d%s_split_" % (k, k, "_s2" if s == 2 else "")
    conv_wgrad(ops, math_mode, which, 300, B, cin, cout, H, W, k, s, prefix)
    conv_wgrad(ops, math_mode, which, 301, B, cin, cout, H, W, k, s, prefix, tf=True)


@DESIGNS
@pytest.mark.parametrize("B,cin,cout,H,W,prefix", [(2, 64, 64, 9, 44, "wgrad3x3_rows_32x288x16"),
                                                   (2, 128, 128, 9, 28, "wgrad3x3_rows_64x576x16")])
def test_wgrad_rows(ops, math_mode, which, B, cin, cout, H, W, prefix):
    """conv_wgrad_rows.hip, both block shapes, with and without the fused transform (no fp32 twin: in product mode 0
    the call goes to the fp32 engine, which is the control here)"""
    conv_wgrad(ops, math_mode, which, 310, B, cin, cout, H, W, 3, 1, prefix)
    conv_wgrad(ops, math_mode, which, 311, B, cin, cout, H, W, 3, 1, prefix, tf=True)


@DESIGNS
@pytest.mark.parametrize("B,cin,cout,H,W", [(4, 256, 256, 7, 7), (3, 256, 64, 20, 22)])
def test_wgrad_pw(ops, math_mode, which, B, cin, cout, H, W):
    """conv_wgrad_pw.hip: the pixel-by-pixel (_rag, 7x7 planes) and the vector loads, the fused transform on x, the
    folded BatchNorm backward on dy (vector loads only)"""
    rag = (H * W) % 4 != 0
    kw = dict(has=("_rag",)) if rag else dict(hasnot=("_rag",))
    conv_wgrad(ops, math_mode, which, 320, B, cin, cout, H, W, 1, 1, "wgrad1x1_pw_", **kw)
    conv_wgrad(ops, math_mode, which, 321, B, cin, cout, H, W, 1, 1, "wgrad1x1_pw_", tf=True, **kw)
    if not rag:
        conv_wgrad(ops, math_mode, which, 322, B, cin, cout, H, W, 1, 1, "wgrad1x1_pw_", bnb=True)
        conv_wgrad(ops, math_mode, which, 323, B, cin, cout, H, W, 1, 1, "wgrad1x1_pw_", tf=True, bnb=True)


@DESIGNS
def test_stem_wgrad(ops, math_mode, which):
    conv_wgrad(ops, math_mode, which, 330, 5, 3, 64, 22, 32, 7, 2, "wgrad7x7_s2_split_")


# ---------------------------------------------------------------- planes.hip, vit_fused.hip

@DESIGNS
@pytest.mark.parametrize("cin,cout,H,B", [(32, 64, 9, 3), (96, 224, 5, 2)])
def test_conv1x1_planes(ops, math_mode, which, cin, cout, H, B):
    """scat_conv1x1_planes: forward from pre-split planes (plain and with the transform fused into the split), and the
    data gradient from the planes of dy (alone and into a base); every LDS ring depth.  Control: the same data through
    the plain entry points in product mode 0."""
    absf = lambda l, r: F.conv2d(l.double().abs(), r.double().abs())
    lab = lambda: ops.lib().scat_last_kernel().decode()
    x, w = _data(which, (B, cin, H, H), (cout, cin, 1, 1), 400, cin, absf, 2.0)
    bias = E.small_ints(400, "bias", (cout,))
    ref = F.conv2d(x.double(), w.double(), bias.double())
    a, w1 = _data(which, (B, cin, H, H), (cout, cin, 1, 1), 401, cin / 2, lambda l, r: absf(F.relu(l), r))
    raw, sc, sh = _relu_form(401, a, cin)
    ref1 = F.conv2d(F.relu(a).double(), w1.double())
    dy, w2 = _data(which, (B, cout, H, H), (cout, cin, 1, 1), 402, cout,
                   lambda l, r: F.conv_transpose2d(l.double().abs(), r.double().abs()), 3.0)
    base = E.small_ints(402, "base", (B, cin, H, H), 3)
    ref2 = F.conv_transpose2d(dy.double(), w2.double())
    math_mode(0)
    assert E.is_exact(ops.conv2d_fwd(g(x), g(w), 1, 0, bias=g(bias)), ref), (which, "data")
    assert E.is_exact(ops.conv2d_fwd(g(raw), g(w1), 1, 0, g(sc), g(sh), True), ref1), (which, "data")
    assert E.is_exact(ops.conv2d_dgrad_w(g(dy), g(w2), (B, cin, H, H), 1, 0), ref2), (which, "data")
    math_mode(1)
    xp, ap, dyp = ops.planes_from(g(x)), ops.planes_from(g(raw), g(sc), g(sh), True), ops.planes_from(g(dy))
    assert torch.equal(xp.to_f32().cpu(), x) and torch.equal(ap.to_f32().cpu(), F.relu(a)) and torch.equal(dyp.to_f32().cpu(), dy)
    for nb in (0, 2, 3):
        assert E.is_exact(ops.conv1x1_planes(xp, g(w), bias=g(bias), lds_stages=nb), ref), (which, nb, lab())
        assert lab().startswith("conv1x1_planes_"), lab()
        assert E.is_exact(ops.conv1x1_planes(ap, g(w1), lds_stages=nb), ref1), (which, nb, lab())
        assert E.is_exact(ops.conv1x1_planes(dyp, g(w2), transposed=True, lds_stages=nb), ref2), (which, nb, lab())
        assert E.is_exact(ops.conv1x1_planes(dyp, g(w2), transposed=True, out=g(base), accumulate=True, lds_stages=nb),
                          ref2 + base.double()), (which, nb, lab())
        assert lab().startswith("conv1x1_planes_"), lab()


@DESIGNS
def test_vit_qkv_projection(ops, math_mode, which):
    """vit_fused.hip: the qkv tensor it returns (a ragged last block of images, a feature count that is no multiple of
    16); its softmax outputs are not exact-sum quantities.  Control: the fp32 engine on the same projection."""
    B, n, dim, heads = 5, 16, 200, 2
    h, w = _data(which, (B * n, dim), (3 * heads * 64, dim), 500, dim, lambda l, r: l.double().abs() @ r.double().abs().t())
    ref = h.double() @ w.double().t()
    math_mode(0)
    assert E.is_exact(ops.linear_fwd(g(h), g(w)), ref), (which, "data")
    math_mode(1)
    qkv, out, attn = ops.qkv_attention_fwd(g(h), g(w), B, n, heads, 64 ** -0.5)
    lab = ops.lib().scat_last_kernel().decode()
    assert lab.startswith("vit_qkv_attn_fused"), lab
    assert E.is_exact(qkv, ref), (which, lab)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(attn).all())
