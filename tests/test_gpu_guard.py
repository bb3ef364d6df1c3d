"""Every C-ABI kernel family inside a poisoned arena (tests/_guard.py), in three placements.

tests/test_gpu_ops.py holds the kernels to fp64 on freshly allocated, tightly sized, 512-byte aligned tensors and looks at
the returned tensor only.  Here every operand, every output the ``ops`` wrappers allocate and every workspace sits
between guard bands of a known NaN (or +1e30 under a fused ReLU, where fmaxf(NaN, 0) would hide an over-read):

  A  every operand aligned, guards only
  S  every operand skewed by one float (data_ptr() % 16 == 4); some families also by two and three
  O  inputs aligned, only the buffers the call writes skewed (catches dispatch that looks at its inputs only)

and in every placement (1) the result meets the gate the family's test in test_gpu_ops.py uses against an fp64 torch
reference computed once, (2) arena.check(): no guard byte changed, every output element written and finite, (3) the
placements agree with each other within the same gate.

What a skewed operand does is written down per case BEFORE any run, from the host code of the entry point: ``compute``
(a fallback kernel, or a kernel that never needed the alignment) or the SCAT_E_* code a specialised entry point rejects
with.  A call through a dispatching ``ops`` wrapper must compute; only ``direct`` cases (a specialised entry point, or a
wrapper that is nothing but that entry point) may reject.  Workspaces are allocator-aligned in the product
(ops.workspace, WeightPrep): here they are guarded, never skewed, and EXACTLY as large as the caller asked for — which is
what the scat_*_ws query returned — so a query that promises less than its launch writes, or a launch that ignores
ws_bytes, damages the guard behind the workspace.  (ops.workspace itself never hands out less than 1 MiB.)

CASES / EXEMPT / WS are read by tests/test_guard_harness.py (no GPU): every pointer-taking prototype of
include/scat_hip.h is in one of the first two, every prototype with a ws_bytes argument (both headers) has a row in WS.
In placement A each case also checks that the entry points it names were really called, and that each of them with a row
in WS was handed, at least once, a workspace of exactly its queried size with that size non-zero."""
import contextlib
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.util import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARENA_BYTES = 192 << 20
CODES = {"SCAT_E_SHAPE": -1, "SCAT_E_ARG": -2, "SCAT_E_WORKSPACE": -3}

# pointer-taking entry points no case calls, each with its one-line reason (kinds: tests/test_guard_harness.py)
EXEMPT = {}

CASES = []


class Case:
    def __init__(self, fn, name, syms, gate, expect, direct, fills, maths, skews):
        self.fn, self.name, self.syms, self.gate, self.direct = fn, name, tuple(syms), gate, direct
        self.expect = {"A": "compute", "S": "compute", "O": "compute"}
        self.expect.update(expect or {})
        self.fills, self.maths, self.skews = tuple(fills), tuple(maths), tuple(skews)


def case(name, syms, gate, expect=None, direct=False, fills=("nan",), maths=(None,), skews=()):
    """gate: the family's gate in tests/test_gpu_ops.py (an output may name another of those gates: Ctx.out).
    expect: placement -> "compute" | "SCAT_E_*", fixed from the code before any run.  maths: product modes to run in
    (None: the default).  skews: extra all-operand skews (2, 3 floats), expected to behave like S."""
    def deco(fn):
        CASES.append(Case(fn, name, syms, gate, expect, direct, fills, maths, skews))
        return fn
    return deco


def R(seed, shape, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g) * std + mean


def U(seed, shape, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(tuple(shape), generator=g) * (hi - lo) + lo


def v4(a):
    return a.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------ the workspace contract

class Ws:
    """What one entry point with a (ws, ws_bytes) pair promises about it, written down from its host code before any run.
    query / qargs: the scat_*_ws function that sizes ws and its arguments from the entry point's own (named) ones.
    align: bytes, the widest access the kernels make to ws (16: 16-byte stores of re-laid weights / 16-byte loads; 8:
    doubles and 64-bit atomics; 4: floats only).
    short: what ws_bytes = query - 1, or a null ws, does: "reject" (SCAT_E_WORKSPACE) or "single_pass" (scat_gemm).
    misaligned: the code for a ws that is not a multiple of ``align`` ("single_pass": scat_gemm again).
    shape -> nbytes: the smallest arguments of interest and the bytes the query returns there; shape2 -> nbytes2: the other
    side of the branch in the query's plan (``branch`` names it).
    unused: argument overrides ("null": pointers passed as null) under which ws is not looked at and (0, 0) is fine.
    math: the product mode the entry point insists on (the weight gradient: the mode in which its first candidate runs).
    build: shape -> the arguments that are host memory.  where: the module that tests the refusals, if not test_cabi."""

    def __init__(self, query, qargs, align, shape, nbytes, short="reject", misaligned="SCAT_E_WORKSPACE", shape2=None,
                 nbytes2=None, branch=None, unused=None, null=(), math=None, build=None, where="tests/test_cabi.py"):
        self.query, self.qargs, self.align, self.shape, self.nbytes = query, qargs, align, shape, nbytes
        self.short, self.misaligned, self.shape2, self.nbytes2, self.branch = short, misaligned, shape2, nbytes2, branch
        self.unused, self.null, self.math, self.build, self.where = unused, tuple(null), math, build, where


def _group_problems(shape):
    """scat_gemm_group's HOST array for the (M_q, N_q, K) of shape["problems"], operands laid out as a weight gradient"""
    from scat_amd.ops import _GemmProblem

    dims = shape["problems"]
    arr = (_GemmProblem * len(dims))()
    for q, (M, N, K) in enumerate(dims):
        arr[q] = _GemmProblem(0x100000 * (3 * q + 1), 1, M, 0x100000 * (3 * q + 2), N, 1, 0x100000 * (3 * q + 3), N, 1, M, N, K)
    return dict(problems=arr, n=len(dims))


def _wprep_host(shape):
    jobs, nj = ctypes.create_string_buffer(4 * 256), ctypes.c_int(0)
    return dict(jobs_out=jobs, njobs_out=ctypes.byref(nj), max_jobs=4)


def _wprep_query(a):
    """the query of the entry point that will be handed this buffer (include/scat_hip.h SCAT_WPREP_*)"""
    k = a["kind"]
    if k in (0, 1):
        return ("scat_conv1x1_s1_ws", (a["Cout"], a["Cin"]) if k == 0 else (a["Cin"], a["Cout"]))
    if k in (2, 3):
        return ("scat_conv3x3_s1_ws", (a["Cout"], a["Cin"]))
    if k == 4:
        return ("scat_conv2d_fwd_split_ws", (a["Cout"], a["Cin"], a["KH"], a["KW"]))
    return ("scat_conv2d_dgrad_s2_ws", (a["Cin"], a["Cout"], a["KH"], a["KW"]))


_BN_Q = lambda a: (a["B"], a["C"], a["HW"])
_BN_ROW = dict(shape=dict(B=4, C=32, HW=49), nbytes=4608, shape2=dict(B=12, C=200, HW=729), nbytes2=73600,
               branch="bn_splits: 4 slots per channel, limited by B | 11, limited by 2048 / C")
_GEMM_STRIDES = lambda M, N, K: dict(M=M, N=N, K=K, a_si=K, a_sk=1, b_sk=N, b_sj=1, c_si=N, c_sj=1)
_WG = lambda B, Cin, H, W, Cout, k, s: dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, KH=k, KW=k, stride=s, pad=k // 2)

# one row per prototype with a ws_bytes argument, include/scat_hip.h then include/scat_eval.h, in header order
WS = {
    "scat_conv2d_dgrad_s2": Ws("scat_conv2d_dgrad_s2_ws", lambda a: (a["Cin"], a["Cout"], a["KH"], a["KW"]), 16,
                               dict(B=2, Cin=32, H=13, W=9, Cout=72, KH=3, KW=3, pad=1), 138240),
    "scat_conv3x3_s1": Ws("scat_conv3x3_s1_ws", lambda a: (a["Cout"], a["Cin"]), 16,
                          dict(B=3, Cin=36, H=7, W=7, Cout=64), 165888),
    "scat_conv2d_fwd_split": Ws("scat_conv2d_fwd_split_ws", lambda a: (a["Cout"], a["Cin"], a["KH"], a["KW"]), 16,
                                dict(B=2, Cin=32, H=13, W=9, Cout=72, KH=3, KW=3, stride=2, pad=1), 124416, math=1),
    "scat_vit_qkv_attn_fwd": Ws("scat_vit_qkv_attn_fwd_ws", lambda a: (a["dim"], a["heads"]), 16,
                                dict(B=5, n=16, dim=200, heads=2), 479232, math=1),
    "scat_conv7x7_s2_fwd_split": Ws("scat_conv7x7_s2_fwd_split_ws", lambda a: (a["Cout"],), 16,
                                    dict(B=3, H=38, W=54, Cout=64), 73728, math=1),
    "scat_conv7x7_s2_wgrad_split": Ws("scat_conv7x7_s2_wgrad_split_ws", lambda a: (a["B"], a["H"], a["W"]), 16,
                                      dict(B=2, H=22, W=32, Cout=64), 225792, shape2=dict(B=4, H=1544, W=32, Cout=64),
                                      nbytes2=23256576, math=1,
                                      branch="stem_wg_rows_per_wg: 4 rows per workgroup (22 rows) | 5 (3088 rows > 4 * 768)"),
    # its one alignment test covers w, src and ws and answers SCAT_E_ARG
    "scat_conv1x1_s1": Ws("scat_conv1x1_s1_ws", lambda a: (a["M"], a["C"]), 16, dict(B=2, C=48, HW=117, M=80), 23040,
                          misaligned="SCAT_E_ARG"),
    "scat_conv1x1_planes": Ws("scat_conv1x1_s1_ws", lambda a: (a["M"], a["C"]), 16, dict(B=3, C=32, HW=81, M=64), 12288,
                              math=1),
    "scat_wprep_jobs": Ws(None, _wprep_query, 16, dict(kind=0, Cout=80, Cin=48, KH=1, KW=1, pad=0, blk0=0), 23040,
                          build=_wprep_host),
    # the engine is chosen per call from one candidate list and only its own slabs are asked for; the row's shape is one
    # whose first candidate in product mode 1 (the rows engine) is also the largest, so query - 1 is short for it
    "scat_conv2d_wgrad": Ws("scat_conv2d_wgrad_ws", lambda a: tuple(a[k] for k in ("B", "Cin", "H", "W", "Cout", "KH", "KW",
                                                                                   "stride", "pad")), 4,
                            _WG(5, 32, 7, 40, 64, 3, 1), 368640, unused=_WG(2, 48, 9, 13, 80, 1, 1), math=1),
    "scat_gemm": Ws("scat_gemm_ws", lambda a: (a["M"], a["N"], a["K"]), 4, _GEMM_STRIDES(84, 588, 784), 592704,
                    short="single_pass", misaligned="single_pass", shape2=_GEMM_STRIDES(84, 3, 147), nbytes2=0,
                    null=("bias",), branch="gemm_plan: 3 K-slices | 1 (K < 512: no slabs, no workspace)"),
    "scat_gemm_group": Ws("scat_gemm_group_ws", lambda a: (a["problems"], a["n"]), 16,
                          dict(problems=[(70, 33, 600), (3, 147, 600)]), 22008, build=_group_problems,
                          shape2=dict(problems=[(70, 33, 300), (3, 147, 300)]), nbytes2=0,
                          branch="group_splits: 2 K-slices | 1 (K < 512)"),
    "scat_gemm_split": Ws("scat_gemm_split_ws", lambda a: (a["M"], a["K"]), 16, dict(M=130, N=70, K=66), 62400, math=1,
                          null=("bias_n",)),
    "scat_bn_train_stats": Ws("scat_bn_ws", _BN_Q, 8, **_BN_ROW),
    "scat_bn_bwd": Ws("scat_bn_ws", _BN_Q, 8, null=("y_out", "y_mask"), **_BN_ROW),
    "scat_bn_bwd_maxpool": Ws("scat_bn_ws", lambda a: (a["B"], a["C"], a["H"] * a["W"]), 8, dict(B=5, C=70, H=10, W=8),
                              12320, shape2=dict(B=13, C=200, H=4, W=8), nbytes2=73600, branch=_BN_ROW["branch"]),
    "scat_bn_bwd_pre": Ws("scat_bn_ws", _BN_Q, 8, dict(B=3, C=48, HW=36), 5376, shape2=dict(B=13, C=200, HW=36),
                          nbytes2=73600, null=("y_out", "y_mask"), branch=_BN_ROW["branch"]),
    "scat_conv1x1_s1_bnb": Ws("scat_conv1x1_s1_ws", lambda a: (a["Cin"], a["Cout"]), 16, dict(B=3, Cin=64, HW=144, Cout=256),
                              98304, math=1),
    "scat_conv1x1_wgrad_bnb": Ws("scat_conv1x1_wgrad_bnb_ws", lambda a: (a["B"], a["Cin"], a["HW"], a["Cout"]), 4,
                                 dict(B=2, Cin=128, HW=252, Cout=128), 131072, unused=dict(B=3, Cin=64, HW=144, Cout=256),
                                 math=1),
    "scat_layernorm_bwd": Ws("scat_layernorm_bwd_ws", lambda a: (a["rows"], a["dim"]), 4, dict(rows=40, dim=196), 32928,
                             shape2=dict(rows=21400, dim=196), nbytes2=16901472, unused=dict(null=("dgamma", "dbeta")),
                             branch="colsum2_slices: 1 slice | 79 (rows * dim >= 1 << 22)"),
    "scat_performer_bwd": Ws("scat_performer_bwd_ws", lambda a: tuple(a[k] for k in ("B", "T", "heads", "e", "m")), 4,
                             dict(B=2, T=21, heads=8, e=49, m=65), 362560),
    "scat_colsum_sliced": Ws("scat_colsum_ws", lambda a: (a["rows"], a["cols"]), 4, dict(rows=24001, cols=196), 61936,
                             shape2=dict(rows=300, cols=61), nbytes2=0, unused=dict(rows=300, cols=61),
                             branch="colsum2_slices: 79 slices | 1 (rows * cols < 1 << 22: the call is scat_colsum)"),
    "scat_regressor_bwd": Ws("scat_regressor_bwd_ws", lambda a: (a["B"], a["F"], a["P"], a["iters"]), 4,
                             dict(B=5, F=196, P=61, iters=3), 4880),
    # include/scat_eval.h: a null or misaligned ws is SCAT_E_ARG there, a short one SCAT_E_WORKSPACE
    "scat_eval_frame_mask": Ws("scat_eval_frame_mask_ws", lambda a: (a["B"], a["n"]), 8, dict(B=3, n=150528), 456,
                               misaligned="SCAT_E_ARG", where="tests/test_eval.py"),
    "scat_eval_accumulate": Ws("scat_eval_accumulate_ws", lambda a: (a["B"], a["T"]), 8, dict(B=5, T=7, ld_gt=105), 232,
                               misaligned="SCAT_E_ARG", null=("keep", "per_sample", "aligned"), where="tests/test_eval.py"),
}


def ws_query(L, name, args):
    """the bytes row WS[name]'s query returns for the entry point's named arguments"""
    row = WS[name]
    q, qa = (row.query, row.qargs(args)) if row.query else row.qargs(args)
    return int(getattr(L, q)(*qa))


def ws_call_args(L, name, shape, ws, ws_bytes, null=()):
    """positional arguments of entry point ``name`` at ``shape`` for a call that is to stop in the host code (no GPU):
    distinct non-null 16-byte-aligned integers as pointers (null for row.null and ``null``), 0 for flags and the stream,
    and null for ``epi`` (HOST memory that the entry point reads and writes) unless ``shape`` brings a real one"""
    row = WS[name]
    vals = dict(shape)
    if row.build:
        vals.update(row.build(shape))
    out = []
    for n, (ty, an) in enumerate(L.protos[name][1]):
        if an in ("ws", "ws_bytes"):
            out.append(ws if an == "ws" else ws_bytes)
        elif an in vals:
            out.append(vals[an])
        elif ty is ctypes.c_void_p:
            out.append(0 if an in row.null or an in null or an in ("stream", "epi") else 0x100000 * (n + 1))
        else:
            out.append(0.125 if ty is ctypes.c_float else 0)
    return out


class _Recorder:
    """scat_amd._lib.lib() with the names of the entry points that were called and, for those with a row in WS, the
    (ws_bytes handed in, bytes the row's query returns for the call's own arguments) of every call"""

    def __init__(self, real):
        self._real, self.called, self.ws = real, set(), {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("scat_"):
            return fn
        names = [an for _, an in self._real.protos[name][1]] if name in WS else None

        def call(*a):
            self.called.add(name)
            if names is not None:
                args = dict(zip(names, a))
                self.ws.setdefault(name, []).append((int(args["ws_bytes"]), ws_query(self._real, name, args)))
            return fn(*a)
        return call


class Ctx:
    """what a case sees in one placement"""

    def __init__(self, ops, arena, lib, skew_in, skew_out, cache, placement, math, mp):
        self.ops, self.arena, self.lib, self.skew_in, self.skew_out = ops, arena, lib, skew_in, skew_out
        self.cache, self.placement, self.math, self.mp, self.outs = cache, placement, math, mp, []

    def once(self, key, fn):
        """inputs and fp64 references are made once per case, not once per placement"""
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def inp(self, t, name=None):
        return self.arena.place(t.contiguous(), self.skew_in, name=name or f"in{len(self.arena.slots)}")

    def acc(self, t, name):
        """a buffer the kernel accumulates into / updates in place: real values, written -> skewed with the outputs"""
        return self.arena.place(t.contiguous(), self.skew_out, name=name, out=True)

    def buf(self, shape, name, dtype=torch.float32):
        """an output the caller hands in (out=...): pre-filled with the guard NaN"""
        return self.arena.place(shape, self.skew_out, dtype, name=name, out=True)

    def out(self, name, got, ref, gate=None):
        """ref: fp64 tensor or a function that makes it (called once per case)"""
        r = self.once(("ref", name), ref) if callable(ref) else ref
        self.outs.append((name, got, r, gate))

    @property
    def aligned(self):
        return self.placement == "A"

    def label(self):
        return self.lib.scat_last_kernel().decode()

    def stream(self):
        return self.ops._stream()


def P(t):
    return 0 if t is None else t.data_ptr()


# ====================================================================================================== convolution

def _conv_ref(x, w, bias, s, p, sc=None, sh=None):
    a = x.double()
    if sc is not None:
        a = F.relu(a * v4(sc.double()) + v4(sh.double()))
    return F.conv2d(a, w.double(), None if bias is None else bias.double(), stride=s, padding=p)


def _conv_family(t, B, cin, cout, H, W, k, s, p, seed, bias=True, fwd_label=None, wg_label=None, wg_deep=None):
    """forward (+bias), forward with the fused relu(bn(x)) operand, data gradient plain and accumulating (from the original
    weights), weight gradient plain and with the fused operand.  wg_deep = (B, H, W): the weight gradient once more over
    enough pixels for scat_conv2d_wgrad_ws to be non-zero (the family's own plane needs no slabs)"""
    ops = t.ops
    x = t.once("x", lambda: R(seed, (B, cin, H, W)))
    w = t.once("w", lambda: R(seed + 1, (cout, cin, k, k), std=(2.0 / (cin * k * k)) ** 0.5))
    b = t.once("b", lambda: R(seed + 2, (cout,)))
    sc = t.once("sc", lambda: U(seed + 3, (cin,), 0.5, 1.5))
    sh = t.once("sh", lambda: U(seed + 4, (cin,), 0.1 if s == 2 else -0.5, 0.6 if s == 2 else 0.5))
    OH, OW = ops.conv_out_hw(H, W, k, s, p)
    dy = t.once("dy", lambda: R(seed + 5, (B, cout, OH, OW)))
    base = t.once("base", lambda: R(seed + 6, (B, cin, H, W)))
    xg, wg, dyg, scg, shg = t.inp(x, "x"), t.inp(w, "w"), t.inp(dy, "dy"), t.inp(sc, "scale"), t.inp(sh, "shift")
    bg = t.inp(b, "bias") if bias else None
    y = ops.conv2d_fwd(xg, wg, s, p, bias=bg)
    if fwd_label and t.aligned:
        assert t.label().startswith(fwd_label), t.label()
    t.out("y", y, lambda: _conv_ref(x, w, b if bias else None, s, p))
    if k != 7:          # (no fused operand and no data gradient for the 7x7 stem: it reads the image)
        t.out("y_tf", ops.conv2d_fwd(xg, wg, s, p, scg, shg, True), lambda: _conv_ref(x, w, None, s, p, sc, sh))

        def dx_ref():
            xx = x.double().requires_grad_(True)
            return torch.autograd.grad(F.conv2d(xx, w.double(), stride=s, padding=p), xx, dy.double())[0]
        t.out("dx", ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p), dx_ref)
        acc = t.acc(base, "dx_acc")
        ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, p, out=acc, accumulate=True)
        t.out("dx_acc", acc, lambda: t.once(("ref", "dx"), dx_ref) + base.double())
    dw = ops.conv2d_wgrad(dyg, xg, tuple(w.shape), s, p)
    if wg_label and t.aligned:
        assert t.label().startswith(wg_label), t.label()
    t.out("dw", dw, lambda: torch.nn.grad.conv2d_weight(x.double(), tuple(w.shape), dy.double(), stride=s, padding=p))
    if k != 7:
        a = lambda: F.relu(x.double() * v4(sc.double()) + v4(sh.double()))
        t.out("dw_tf", ops.conv2d_wgrad(dyg, xg, tuple(w.shape), s, p, scg, shg, True),
              lambda: torch.nn.grad.conv2d_weight(a(), tuple(w.shape), dy.double(), stride=s, padding=p))
    if wg_deep:
        _wgrad_deep(t, cin, cout, k, s, p, seed, *wg_deep)


def _wgrad_deep(t, cin, cout, k, s, p, seed, B, H, W):
    x = t.once("x_deep", lambda: R(seed + 7, (B, cin, H, W)))
    dy = t.once("dy_deep", lambda: R(seed + 8, (B, cout) + tuple(t.ops.conv_out_hw(H, W, k, s, p))))
    t.out("dw_deep", t.ops.conv2d_wgrad(t.inp(dy, "dy_deep"), t.inp(x, "x_deep"), (cout, cin, k, k), s, p),
          lambda: torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dy.double(), stride=s, padding=p))


def _pw(t, *shape, seed):
    t.mp.setattr(t.ops, "PW_MIN_C", 0)
    _conv_family(t, *shape, 1, 1, 0, seed, fwd_label="conv1x1_split" if t.math else "conv1x1_pw", wg_deep=(6, 13, 13))


# the pointwise (weights-in-registers) kernel: scalar and vector pixel staging, ragged row / pixel tiles, both product modes,
# both fills (the fused operand forms relu(x * scale + shift) in its load).  S: ops._pw_ok sends skewed x / w / scale /
# shift / out to the generic engine, which picks its scalar loaders (csrc/conv.hip av4 / bv4).  O: the entry point takes a
# skewed dst (its wide epilogue tests dst itself: w4ok).
@case("conv_pw_9x13", ("scat_conv1x1_s1", "scat_conv2d_wgrad"), 2e-5, fills=("nan", "big"), maths=(0, 1), skews=(2, 3))
def _c1(t):
    _pw(t, 2, 48, 80, 9, 13, seed=100)


@case("conv_pw_5x64", ("scat_conv1x1_s1", "scat_conv2d_wgrad"), 2e-5, maths=(0, 1))
def _c2(t):
    _pw(t, 1, 16, 208, 5, 64, seed=110)


@case("conv_pw_7x7", ("scat_conv1x1_s1", "scat_conv2d_wgrad"), 2e-5, fills=("nan", "big"), maths=(0, 1))
def _c3(t):
    _pw(t, 3, 32, 64, 7, 7, seed=120)


# the 3x3 LDS-halo kernel: every source element is a 4-byte buffer load, the weights come re-laid from the (aligned)
# workspace, the epilogue stores per element: no alignment need -> compute everywhere
@case("conv3x3_9x13", ("scat_conv3x3_s1", "scat_conv2d_wgrad"), 2e-5, fills=("nan", "big"), maths=(0, 1), skews=(2, 3))
def _c4(t):
    _conv_family(t, 2, 20, 72, 9, 13, 3, 1, 1, 130, bias=False, fwd_label="conv3x3_split" if t.math else "conv3x3_halo",
                 wg_deep=(6, 13, 13))


@case("conv3x3_7x7", ("scat_conv3x3_s1", "scat_conv2d_wgrad"), 2e-5, maths=(0, 1))
def _c5(t):
    _conv_family(t, 3, 36, 64, 7, 7, 3, 1, 1, 140, bias=False, fwd_label="conv3x3_split" if t.math else "conv3x3_halo",
                 wg_deep=(6, 13, 13))


# stride 2 on the split-operand taps kernel (forward) and the parity-class data gradient, odd planes
@case("conv_s2_3x3_13x9", ("scat_conv2d_fwd_split", "scat_conv2d_dgrad_s2", "scat_conv2d_wgrad"), 2e-5,
      fills=("nan", "big"), maths=(1,))
def _c6(t):
    _conv_family(t, 2, 32, 72, 13, 9, 3, 2, 1, 150)
    if t.aligned:
        assert "_s2_split_" in t.label(), t.label()
    _wgrad_deep(t, 32, 72, 3, 2, 1, 150, 4, 27, 27)


@case("conv_s2_1x1_7x7", ("scat_conv2d_fwd_split", "scat_conv2d_dgrad_s2", "scat_conv2d_wgrad"), 2e-5, maths=(1,))
def _c7(t):
    _conv_family(t, 3, 48, 64, 7, 7, 1, 2, 0, 160, wg_deep=(8, 28, 28))


@case("dgrad_s2_odd", ("scat_conv2d_dgrad_s2",), 2e-5, maths=(0, 1))
def _c8(t):
    """parity classes with ragged class grids; Cout = 20 -> the fp32 engine per class, 48 -> the split taps kernel"""
    for H, W in ((13, 9), (7, 7)):
        for cout in (20, 48):
            for k, p in ((3, 1), (1, 0)):
                key = f"{H}x{W}_{cout}_{k}"
                x = t.once("x" + key, lambda: R(170, (2, 12, H, W)))
                w = t.once("w" + key, lambda: R(171 + cout + k, (cout, 12, k, k), std=0.2))
                OH, OW = t.ops.conv_out_hw(H, W, k, 2, p)
                dy = t.once("dy" + key, lambda: R(172 + k, (2, cout, OH, OW)))
                base = t.once("b" + key, lambda: R(173, (2, 12, H, W)))

                def ref():
                    xx = x.double().requires_grad_(True)
                    return torch.autograd.grad(F.conv2d(xx, w.double(), stride=2, padding=p), xx, dy.double())[0]
                dyg, wg = t.inp(dy, "dy" + key), t.inp(w, "w" + key)
                t.out("dx" + key, t.ops.conv2d_dgrad_w(dyg, wg, (2, 12, H, W), 2, p), ref)
                acc = t.acc(base, "acc" + key)
                t.ops.conv2d_dgrad_w(dyg, wg, (2, 12, H, W), 2, p, out=acc, accumulate=True)
                t.out("dxa" + key, acc, lambda: t.once(("ref", "dx" + key), ref) + base.double())


# the 7x7 stem on split products: x by 4-byte buffer loads, weights from the workspace -> compute everywhere.  Its weight
# gradient (Cout 64, OW % 16 == 0) wants dy aligned: ops.conv2d_wgrad mirrors that test and falls through to the general
# engine for a skewed dy or x.
@case("stem_fwd_38x54", ("scat_conv7x7_s2_fwd_split", "scat_conv2d_wgrad"), 2e-5, maths=(1,))
def _c9(t):
    _conv_family(t, 3, 3, 64, 38, 54, 7, 2, 3, 180, bias=False, fwd_label="conv7x7_s2_split")


@case("stem_wgrad_30x64", ("scat_conv7x7_s2_fwd_split", "scat_conv7x7_s2_wgrad_split"), 2e-5, maths=(1,))
def _c10(t):
    _conv_family(t, 3, 3, 64, 30, 64, 7, 2, 3, 190, bias=False, fwd_label="conv7x7_s2_split", wg_label="wgrad7x7_s2_split")


# the specialised stem weight gradient called directly: dy (and the workspace) must be aligned -> SCAT_E_WORKSPACE is the
# code its one alignment test raises; x and dw are not looked at (4-byte loads, per-element stores) -> O computes
@case("stem_wgrad_direct", ("scat_conv7x7_s2_wgrad_split",), 2e-5, expect={"S": "SCAT_E_WORKSPACE"}, direct=True, maths=(1,))
def _c11(t):
    # 22 output rows: 4 rows per workgroup; 3088 rows: 5 (the other value of stem_wg_rows_per_wg, 618 slabs)
    for tag, (B, H, W) in (("", (2, 22, 32)), ("_tall", (4, 1544, 32))):
        x = t.once("x" + tag, lambda: R(200, (B, 3, H, W)))
        dy = t.once("dy" + tag, lambda: R(201, (B, 64, H // 2, W // 2)))
        xg, dyg = t.inp(x, "x" + tag), t.inp(dy, "dy" + tag)
        dw = t.buf((64, 3, 7, 7), "dw" + tag)
        ws = t.ops.workspace(t.lib.scat_conv7x7_s2_wgrad_split_ws(B, H, W), xg.device, "stem")
        t.lib.scat_conv7x7_s2_wgrad_split(P(dyg), P(xg), P(dw), B, H, W, 64, P(ws), ws.numel(), t.stream())
        t.out("dw" + tag, dw,
              lambda: torch.nn.grad.conv2d_weight(x.double(), (64, 3, 7, 7), dy.double(), stride=2, padding=3))


# row-walking 3x3 weight gradient (csrc/conv_wgrad_rows.hip): taken only for aligned dy and x (its host test), else the
# general weight-gradient engine
@case("wgrad3x3_rows", ("scat_conv2d_wgrad",), 2e-5, fills=("nan", "big"), maths=(1,))
def _c12(t):
    for B, cin, cout, H, W, tf in ((2, 64, 64, 9, 44, True), (5, 32, 64, 7, 40, True), (3, 32, 32, 20, 56, False)):
        key = f"{cin}_{cout}_{H}x{W}"
        x = t.once("x" + key, lambda: R(210 + H, (B, cin, H, W)))
        dy = t.once("dy" + key, lambda: R(211 + H, (B, cout, H, W)))
        sc = t.once("sc" + key, lambda: U(212, (cin,), 0.5, 1.5))
        sh = t.once("sh" + key, lambda: U(213, (cin,), -0.5, 0.5))
        args = (t.inp(sc, "scale"), t.inp(sh, "shift"), True) if tf else ()
        dw = t.ops.conv2d_wgrad(t.inp(dy, "dy" + key), t.inp(x, "x" + key), (cout, cin, 3, 3), 1, 1, *args)
        if t.aligned:
            assert t.label().startswith("wgrad3x3_rows"), t.label()
        a = (lambda: F.relu(x.double() * v4(sc.double()) + v4(sh.double()))) if tf else (lambda: x.double())
        t.out("dw" + key, dw, lambda: torch.nn.grad.conv2d_weight(a(), (cout, cin, 3, 3), dy.double(), padding=1))


# producer/consumer pointwise weight gradient (csrc/conv_wgrad_pw.hip): its plan is dropped for a skewed dy or x
@case("wgrad1x1_pw", ("scat_conv2d_wgrad",), 2e-5, fills=("nan", "big"), maths=(1,))
def _c13(t):
    for B, cin, cout, H, W, tf in ((3, 320, 192, 5, 5, True), (2, 128, 128, 14, 18, True), (3, 512, 128, 12, 10, False)):
        key = f"{cin}_{cout}_{H}x{W}"
        x = t.once("x" + key, lambda: R(220 + H, (B, cin, H, W)))
        dy = t.once("dy" + key, lambda: R(221 + H, (B, cout, H, W)))
        sc = t.once("sc" + key, lambda: U(222, (cin,), 0.5, 1.5))
        sh = t.once("sh" + key, lambda: U(223, (cin,), -0.5, 0.5))
        args = (t.inp(sc, "scale"), t.inp(sh, "shift"), True) if tf else ()
        dw = t.ops.conv2d_wgrad(t.inp(dy, "dy" + key), t.inp(x, "x" + key), (cout, cin, 1, 1), 1, 0, *args)
        if t.aligned:
            assert t.label().startswith("wgrad1x1_pw_"), t.label()
        a = (lambda: F.relu(x.double() * v4(sc.double()) + v4(sh.double()))) if tf else (lambda: x.double())
        t.out("dw" + key, dw, lambda: torch.einsum("nop,nip->oi", dy.double().flatten(2), a().flatten(2))
              .view(cout, cin, 1, 1))


# The weight-gradient entry points with a workspace of exactly the bytes their _ws query promises, inside the arena: the
# query and the launch take their engine from one plan (csrc/conv_wgrad.hip wgrad_candidates), and a launch that wrote one
# slab more than the query returned would land in the guard behind "ws".  One shape per engine, the smallest the tests of
# tests/test_gpu_ops.py choose it at; a skewed dy or x drops the rows and pointwise engines to the next candidate under
# the same query; product mode 0 takes the fp32 engine everywhere.  -> compute in every placement
_WG_EXACT = [
    # B, cin, cout, H, W, k, stride, label in product mode 1 when aligned
    (5, 32, 64, 7, 40, 3, 1, "wgrad3x3_rows_32x288x16"), (2, 128, 128, 9, 28, 3, 1, "wgrad3x3_rows_64x576x16"),
    (3, 320, 192, 5, 5, 1, 1, "wgrad1x1_pw_"), (2, 128, 128, 14, 18, 1, 1, "wgrad1x1_pw_"),
    (2, 20, 136, 9, 13, 3, 1, "wgrad3x3_split_"), (2, 20, 136, 9, 13, 3, 2, "wgrad3x3_s2_split_"),
    (2, 144, 136, 8, 14, 1, 2, "wgrad1x1_128x64x32"),
]


def _exact_ws(t, nbytes):
    """(pointer, bytes) of a guarded workspace of exactly nbytes (its contents are the kernel's business)"""
    if nbytes == 0:
        return 0, 0
    return P(t.arena.place(nbytes, 0, torch.uint8, name="ws", out=True, finite=False)), nbytes


@case("wgrad_exact_workspace", ("scat_conv2d_wgrad",), 2e-5, direct=True, maths=(0, 1))
def _c13b(t):
    for B, cin, cout, H, W, k, s, label in _WG_EXACT:
        key, p, w_shape = f"{cin}_{cout}_{H}x{W}k{k}s{s}", k // 2, (cout, cin, k, k)
        OH, OW = t.ops.conv_out_hw(H, W, k, s, p)
        x = t.once("x" + key, lambda: R(230 + H, (B, cin, H, W)))
        dy = t.once("dy" + key, lambda: R(231 + H, (B, cout, OH, OW)))
        sc = t.once("sc" + key, lambda: U(232, (cin,), 0.5, 1.5))
        sh = t.once("sh" + key, lambda: U(233, (cin,), 0.1, 0.6))
        dyg, xg, scg, shg = t.inp(dy, "dy" + key), t.inp(x, "x" + key), t.inp(sc, "scale"), t.inp(sh, "shift")
        need = t.lib.scat_conv2d_wgrad_ws(B, cin, H, W, cout, k, k, s, p)
        assert need >= 0
        for tf in (False, True):
            dw = t.buf(w_shape, "dw" + key)
            ws, nb = _exact_ws(t, need)
            t.lib.scat_conv2d_wgrad(P(dyg), P(xg), P(dw), B, cin, H, W, cout, k, k, s, p, P(scg) if tf else 0,
                                    P(shg) if tf else 0, int(tf), ws, nb, t.stream())
            if t.aligned:
                want = label if t.math == 1 else f"wgrad{k}x{k}_{64 if cout <= 64 else 128}x64x32"
                assert t.label().startswith(want), (t.label(), want)
            a = (lambda: F.relu(x.double() * v4(sc.double()) + v4(sh.double()))) if tf else (lambda: x.double())
            t.out(f"dw{key}tf{int(tf)}", dw,
                  lambda: torch.nn.grad.conv2d_weight(a(), w_shape, dy.double(), stride=s, padding=p))


@case("wgrad_bnb_exact_workspace", ("scat_conv1x1_wgrad_bnb",), 2e-5, direct=True, maths=(1,))
def _c13c(t):
    B, cin, cout, H, W = 2, 128, 128, 14, 18
    g = t.once("g", lambda: R(240, (B, cout, H, W)))
    z = t.once("z", lambda: R(241, (B, cout, H, W)))
    coef = t.once("coef", lambda: U(242, (3, cout), -0.5, 0.5))
    x = t.once("x", lambda: R(243, (B, cin, H, W)))
    gg, zg, cg, xg = t.inp(g, "g"), t.inp(z, "z"), t.inp(coef, "coef3"), t.inp(x, "x")
    dw = t.buf((cout, cin, 1, 1), "dw")
    ws, nb = _exact_ws(t, t.lib.scat_conv1x1_wgrad_bnb_ws(B, cin, H * W, cout))
    t.lib.scat_conv1x1_wgrad_bnb(P(gg), P(zg), P(cg), P(xg), P(dw), B, cin, H * W, cout, 0, 0, 0, ws, nb, t.stream())
    if t.aligned:
        assert t.label().startswith("wgrad1x1_pw_") and "_bnb" in t.label(), t.label()
    dz = lambda: v4(coef[0].double()) * g.double() + v4(coef[1].double()) * z.double() + v4(coef[2].double())
    t.out("dw", dw, lambda: torch.einsum("nop,nip->oi", dz().flatten(2), x.double().flatten(2)).view(cout, cin, 1, 1))


# the general engine itself (channel counts no specialised kernel takes), bias on a ragged channel count, and the
# transposed-weights data gradient
@case("conv_generic", ("scat_conv2d_fwd", "scat_conv2d_dgrad", "scat_conv2d_wt", "scat_conv2d_wgrad"), 2e-5,
      fills=("nan", "big"), maths=(0, 1))
def _c14(t):
    _conv_family(t, 5, 20, 130, 9, 9, 1, 1, 0, 230, wg_deep=(6, 13, 13))
    x = t.once("x3", lambda: R(236, (4, 3, 6, 5)))
    w = t.once("w3", lambda: R(237, (5, 3, 3, 3), std=0.3))
    dy = t.once("dy3", lambda: R(238, (4, 5, 6, 5)))
    base = t.once("b3", lambda: R(239, (4, 3, 6, 5)))
    wt = t.ops.conv2d_wt(t.inp(w, "w3"))
    t.out("wt", wt, w.double().permute(1, 0, 2, 3).reshape(3, 45), gate=0.0)

    def ref():
        xx = x.double().requires_grad_(True)
        return torch.autograd.grad(F.conv2d(xx, w.double(), padding=1), xx, dy.double())[0]
    dyg = t.inp(dy, "dy3")
    t.out("dx3", t.ops.conv2d_dgrad(dyg, wt, (4, 3, 6, 5), (5, 3, 3, 3), 1, 1), ref)
    acc = t.acc(base, "dx3_acc")
    t.ops.conv2d_dgrad(dyg, wt, (4, 3, 6, 5), (5, 3, 3, 3), 1, 1, out=acc, accumulate=True)
    t.out("dx3a", acc, lambda: t.once(("ref", "dx3"), ref) + base.double())


# BatchNorm sums in the forward epilogue.  S / O: the pointwise and halo kernels still run for the 3x3 and stride-2 cases;
# where the general engine takes over the call reports 0 groups and bn_train_stats takes its pass over y: same numbers.
@case("conv_epilogue_stats", ("scat_bn_train_stats_partials", "scat_bn_train_stats_partials_shifted", "scat_conv1x1_s1",
                              "scat_conv3x3_s1"), 2e-5, maths=(1,))
def _c15(t):
    for B, cin, cout, k, H, W in ((2, 128, 64, 1, 13, 9), (2, 32, 32, 3, 11, 9)):
        key = f"k{k}"
        x = t.once("x" + key, lambda: R(240 + k, (B, cin, H, W)) * 1.3 + 0.2)
        w = t.once("w" + key, lambda: R(241 + k, (cout, cin, k, k), std=(2.0 / (cin * k * k)) ** 0.5))
        gamma = t.once("g" + key, lambda: U(242, (cout,), 0.5, 1.5))
        beta = t.once("b" + key, lambda: U(243, (cout,), -0.3, 0.3))
        yr = lambda: t.once("yr" + key, lambda: F.conv2d(x.double(), w.double(), padding=k // 2))
        mean_r = lambda: yr().mean(dim=(0, 2, 3))
        invstd_r = lambda: 1.0 / torch.sqrt(yr().var(dim=(0, 2, 3), unbiased=False) + 1e-5)
        xg, wg, gg, bg = t.inp(x, "x" + key), t.inp(w, "w" + key), t.inp(gamma, "gamma"), t.inp(beta, "beta")
        for tag in ("", "_shift"):
            ss = t.inp(t.once("ss" + key, lambda: (mean_r() * 1.001).float()), "stats_shift") if tag else None
            y = t.ops.conv2d_fwd(xg, wg, 1, k // 2, stats=True, stats_shift=ss)
            if t.aligned:
                assert getattr(y, "scat_stats", None) is not None, t.label()
            rm, rv = t.acc(torch.zeros(cout), "rm"), t.acc(torch.ones(cout), "rv")
            mean, invstd, scale, shift = t.ops.bn_train_stats(y, gg, bg, rm, rv)
            t.out("y" + key + tag, y, yr)
            t.out("mean" + key + tag, mean, mean_r)
            t.out("invstd" + key + tag, invstd, invstd_r)
            t.out("scale" + key + tag, scale, lambda: gamma.double() * invstd_r())
            t.out("shift" + key + tag, shift, lambda: beta.double() - mean_r() * gamma.double() * invstd_r())
            t.out("rm" + key + tag, rm, lambda: 0.1 * mean_r())
            t.out("rv" + key + tag, rv, lambda: 0.9 + 0.1 * yr().var(dim=(0, 2, 3), unbiased=True))


# prepared weights: scat_wprep_jobs writes HOST records, scat_wprep_run re-lays every registered weight with one launch
# into the persistent (aligned, guarded) workspaces; all six kinds, then the w_ready = 1 calls
@case("prepared_weights", ("scat_wprep_jobs", "scat_wprep_run", "scat_conv1x1_s1", "scat_conv3x3_s1", "scat_conv2d_fwd_split",
                           "scat_conv2d_dgrad_s2"), 2e-5, maths=(1,))
def _c16(t):
    ops = t.ops
    wp = ops.WeightPrep()
    shapes = [(32, 48, 1, 1, 9), (48, 32, 3, 1, 10), (32, 64, 3, 2, 11), (64, 32, 1, 2, 12), (16, 80, 3, 2, 8)]
    ten = []
    for n, (cin, cout, k, s, H) in enumerate(shapes):
        OH, _ = ops.conv_out_hw(H, H, k, s, k // 2)
        w = t.once(f"w{n}", lambda: R(250 + n, (cout, cin, k, k), std=0.1))
        x = t.once(f"x{n}", lambda: R(260 + n, (2, cin, H, H)))
        dy = t.once(f"dy{n}", lambda: R(270 + n, (2, cout, OH, OH)))
        ten.append((w, x, dy, t.inp(w, f"w{n}"), t.inp(x, f"x{n}"), t.inp(dy, f"dy{n}")))

    def run_all():
        outs = []
        for (cin, cout, k, s, H), (w, x, dy, wg, xg, dyg) in zip(shapes, ten):
            outs.append(ops.conv2d_fwd(xg, wg, s, k // 2, wp=wp))
            outs.append(ops.conv2d_dgrad_w(dyg, wg, tuple(x.shape), s, k // 2, wp=wp))
        return outs

    run_all()                      # registers; every call still prepares for itself
    wp.run(False)                  # the table, one launch
    if t.aligned:
        assert sorted({k for _, k in wp.entries}) == [0, 1, 2, 3, 4, 5] and all(e[2] for e in wp.entries.values())
    outs = run_all()               # w_ready = 1 wherever a specialised kernel runs
    for n, ((cin, cout, k, s, H), (w, x, dy, *_)) in enumerate(zip(shapes, ten)):
        def dx_ref(x=x, w=w, dy=dy, s=s, k=k):
            xx = x.double().requires_grad_(True)
            return torch.autograd.grad(F.conv2d(xx, w.double(), stride=s, padding=k // 2), xx, dy.double())[0]
        t.out(f"y{n}", outs[2 * n], lambda x=x, w=w, s=s, k=k: F.conv2d(x.double(), w.double(), stride=s, padding=k // 2))
        t.out(f"dx{n}", outs[2 * n + 1], dx_ref)


# activations as bf16 planes: scat_planes_from_f32 requires src and planes 16-B aligned, scat_conv1x1_planes its planes
# (the LDS-DMA path) -> SCAT_E_ARG for a skewed source (S) and for skewed planes, which planes_from itself writes (O)
@case("planes", ("scat_planes_from_f32", "scat_conv1x1_planes"), 2e-5, expect={"S": "SCAT_E_ARG", "O": "SCAT_E_ARG"},
      direct=True, fills=("nan", "big"), maths=(1,))
def _c17(t):
    B, cin, cout, H = 3, 32, 64, 9
    x = t.once("x", lambda: R(280, (B, cin, H, H)))
    w = t.once("w", lambda: R(281, (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5))
    dy = t.once("dy", lambda: R(282, (B, cout, H, H)))
    sc, sh = t.once("sc", lambda: U(283, (cin,), 0.5, 1.5)), t.once("sh", lambda: U(284, (cin,), -0.5, 0.5))
    base = t.once("base", lambda: R(285, (B, cin, H, H)))
    xg, wg = t.inp(x, "x"), t.inp(w, "w")
    xp = t.ops.planes_from(xg)
    xtp = t.ops.planes_from(xg, t.inp(sc, "scale"), t.inp(sh, "shift"), True)
    dyp = t.ops.planes_from(t.inp(dy, "dy"))
    t.out("planes", xp.to_f32(), x.double(), gate=0.0)
    t.out("y", t.ops.conv1x1_planes(xp, wg), lambda: _conv_ref(x, w, None, 1, 0))
    t.out("y_tf", t.ops.conv1x1_planes(xtp, wg, lds_stages=3), lambda: _conv_ref(x, w, None, 1, 0, sc, sh))
    dx_ref = lambda: F.conv_transpose2d(dy.double(), w.double())
    t.out("dx", t.ops.conv1x1_planes(dyp, wg, transposed=True, lds_stages=2), dx_ref)
    acc = t.acc(base, "dx_acc")
    t.ops.conv1x1_planes(dyp, wg, transposed=True, out=acc, accumulate=True)
    t.out("dx_acc", acc, lambda: dx_ref() + base.double())


# ====================================================================================================== BatchNorm

def _bn_inputs(t, B, C, H, W, seed):
    x = t.once("x", lambda: R(seed, (B, C, H, W)) * 1.7 + 0.4)
    gamma = t.once("gamma", lambda: U(seed + 1, (C,), 0.5, 1.5))
    beta = t.once("beta", lambda: U(seed + 2, (C,), -0.3, 0.3))
    res = t.once("res", lambda: R(seed + 3, (B, C, H, W)))
    dy = t.once("dy", lambda: R(seed + 4, (B, C, H, W)))
    rm = t.once("rm", lambda: U(seed + 5, (C,), -0.2, 0.2))
    rv = t.once("rv", lambda: U(seed + 6, (C,), 0.6, 1.4))
    return x, gamma, beta, res, dy, rm, rv


def _bn_ref(t, x, gamma, beta, res, dy, rm, rv):
    """fp64: everything a train-mode BatchNorm + residual + ReLU block yields, forward and backward"""
    def make():
        xr, gr, br = (a.double().requires_grad_(True) for a in (x, gamma, beta))
        rmr, rvr = rm.double().clone(), rv.double().clone()
        bn = F.batch_norm(xr, rmr, rvr, gr, br, True, 0.1, 1e-5)
        y = F.relu(bn + res.double())
        dx, dg, db = torch.autograd.grad(y, (xr, gr, br), dy.double(), retain_graph=True)
        y2 = F.relu(bn)
        dx2, dg2, db2 = torch.autograd.grad(y2, (xr, gr, br), dy.double())
        mean = x.double().mean(dim=(0, 2, 3))
        invstd = 1.0 / torch.sqrt(x.double().var(dim=(0, 2, 3), unbiased=False) + 1e-5)
        return dict(y=y.detach(), dx=dx, dg=dg, db=db, dx2=dx2, dg2=dg2, db2=db2, mean=mean, invstd=invstd, rm=rmr, rv=rvr,
                    scale=gamma.double() * invstd, shift=beta.double() - mean * gamma.double() * invstd,
                    dres=dy.double() * (y.detach() > 0))
    return t.once("bnref", make)


def _bn_block(t, B, C, H, W, seed, with_mask=True):
    """bn_train_stats, bn_apply with residual (+ sign mask where the wrapper gives one: aligned x / y / residual and
    HW % 4 == 0; it returns None otherwise and the backward takes the output itself), bn_bwd with the masked-gradient
    output, the recomputed-mask form, bn_eval_fold"""
    ops = t.ops
    x, gamma, beta, res, dy, rm, rv = _bn_inputs(t, B, C, H, W, seed)
    r = lambda k: (lambda: _bn_ref(t, x, gamma, beta, res, dy, rm, rv)[k])
    xg, gg, bg, resg, dyg = t.inp(x, "x"), t.inp(gamma, "gamma"), t.inp(beta, "beta"), t.inp(res, "res"), t.inp(dy, "dy")
    rmg, rvg = t.acc(rm, "running_mean"), t.acc(rv, "running_var")
    mean, invstd, scale, shift = ops.bn_train_stats(xg, gg, bg, rmg, rvg)
    for k, got in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift), ("rm", rmg), ("rv", rvg)):
        t.out(k, got, r(k), gate=1e-5)
    y, mask = ops.bn_apply(xg, scale, shift, resg, relu=True, want_mask=True)
    t.out("y", y, r("y"), gate=1e-5)
    if t.aligned and with_mask and (H * W) % 4 == 0:
        assert mask is not None
        bits = ((mask.view(-1, 1) >> torch.arange(4, device=DEV, dtype=torch.uint8)) & 1).bool().view_as(y)
        assert torch.equal(bits, y > 0)
    if not t.aligned:
        assert mask is None       # ops.bn_apply: "None when the plane is not a multiple of 4" or a tensor is not aligned
    dres = t.buf(tuple(x.shape), "dres")
    dx, dg, db = ops.bn_bwd(dyg, xg, None if mask is not None else y, True, scale, shift, mean, invstd, gg, dres=dres,
                            y_mask=mask)
    t.out("dx", dx, r("dx"))
    t.out("dgamma", dg, r("dg"))
    t.out("dbeta", db, r("db"))
    t.out("dres", dres, r("dres"), gate=1e-6)
    dx2, dg2, db2 = ops.bn_bwd(dyg, xg, None, True, scale, shift, mean, invstd, gg)
    t.out("dx2", dx2, r("dx2"))
    t.out("dgamma2", dg2, r("dg2"))
    t.out("dbeta2", db2, r("db2"))
    sc_e, sh_e = ops.bn_eval_fold(gg, bg, rmg, rvg)
    t.out("y_eval", ops.bn_apply(xg, sc_e, sh_e),
          lambda: F.batch_norm(x.double(), r("rm")(), r("rv")(), gamma.double(), beta.double(), False, 0.1, 1e-5), gate=1e-5)


_BN_SYMS = ("scat_bn_train_stats", "scat_bn_apply", "scat_bn_bwd", "scat_bn_eval_fold")


# HW % 4 != 0 (scalar kernels in every placement), one-pass backward (C >= 64, small planes)
@case("bn_3x70x9x9", _BN_SYMS, 2e-5, skews=(2, 3))
def _b1(t):
    _bn_block(t, 3, 70, 9, 9, 300)


# HW % 4 == 0: vector kernels when aligned, <1> kernels when any tensor is skewed; one-pass backward
@case("bn_5x128x14x14", _BN_SYMS, 2e-5, skews=(2, 3))
def _b2(t):
    _bn_block(t, 5, 128, 14, 14, 310)


# C < 64: the two-pass backward (reduce + apply), last-arriver finalize
@case("bn_4x32x28x28", _BN_SYMS, 2e-5)
def _b3(t):
    _bn_block(t, 4, 32, 28, 28, 320)


# C >= 256: the statistics finish inside the reducing kernel (one workgroup per channel)
@case("bn_3x256x14x14", _BN_SYMS, 2e-5)
def _b4(t):
    _bn_block(t, 3, 256, 14, 14, 330)


# C = 200, B = 12: 2048 / C limits the slots per channel (11 < B; above, B does); HW % 4 != 0 and B * HW > 8192: scalar
# kernels, the two-pass backward with its slots and claim words
@case("bn_12x200x27x27", _BN_SYMS, 2e-5)
def _b4b(t):
    _bn_block(t, 12, 200, 27, 27, 335)


@case("bn_apply_shortcut", ("scat_bn_apply",), 1e-6)
def _b5(t):
    """relu(bn3(c3) + bnd(cd)): the shortcut's BatchNorm folded into the add, vector and scalar planes"""
    for n, shp in enumerate([(2, 24, 6, 6), (3, 8, 5, 3)]):
        C = shp[1]
        c3, cd = t.once(f"c3{n}", lambda: R(340 + n, shp)), t.once(f"cd{n}", lambda: R(342 + n, shp))
        s3, h3 = t.once(f"s3{n}", lambda: U(344, (C,), 0.5, 1.5)), t.once(f"h3{n}", lambda: R(345, (C,)))
        sd, hd = t.once(f"sd{n}", lambda: U(346, (C,), 0.5, 1.5)), t.once(f"hd{n}", lambda: R(347, (C,)))
        one = t.ops.bn_apply(t.inp(c3, "c3"), t.inp(s3, "s3"), t.inp(h3, "h3"), t.inp(cd, "cd"), True,
                             res_scale=t.inp(sd, "sd"), res_shift=t.inp(hd, "hd"))
        t.out(f"y{n}", one, lambda: F.relu(c3.double() * v4(s3.double()) + v4(h3.double()) + cd.double() * v4(sd.double())
                                           + v4(hd.double())))


# bn_bwd handed a sign mask needs the vector kernels: dy / x / dx / dres aligned.  Skewed inputs (S) or a skewed dx (O)
# are rejected with SCAT_E_SHAPE ("the sign mask needs HW % 4 == 0 and 16-B aligned tensors").
@case("bn_bwd_sign_mask_direct", ("scat_bn_bwd",), 2e-5, expect={"S": "SCAT_E_SHAPE", "O": "SCAT_E_SHAPE"}, direct=True)
def _b6(t):
    B, C, H, W = 3, 64, 6, 6
    x, gamma, beta, res, dy, rm, rv = _bn_inputs(t, B, C, H, W, 350)
    ref = lambda: _bn_ref(t, x, gamma, beta, res, dy, rm, rv)
    f32 = lambda k: t.once("f32" + k, lambda: ref()[k].float())

    def mask_bytes():
        b = (ref()["y"] > 0).reshape(-1, 4).to(torch.uint8)
        return (b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)).contiguous()
    mask = t.inp(t.once("mask", mask_bytes), "y_mask")
    dres = t.buf((B, C, H, W), "dres")
    dx, dg, db = t.ops.bn_bwd(t.inp(dy, "dy"), t.inp(x, "x"), None, True, t.inp(f32("scale"), "scale"),
                              t.inp(f32("shift"), "shift"), t.inp(f32("mean"), "mean"), t.inp(f32("invstd"), "invstd"),
                              t.inp(gamma, "gamma"), dres=dres, y_mask=mask)
    t.out("dx", dx, lambda: ref()["dx"])
    t.out("dgamma", dg, lambda: ref()["dg"])
    t.out("dbeta", db, lambda: ref()["db"])
    t.out("dres", dres, lambda: ref()["dres"], gate=1e-6)


# the folded backward's first half: "Needs HW % 4 == 0 and 16-B aligned tensors" (include/scat_hip.h) -> SCAT_E_SHAPE for a
# skewed dy_g / dy_add / x / y_out; dy_g is also what it writes, so O rejects too
@case("bn_bwd_pre", ("scat_bn_bwd_pre",), 2e-5, expect={"S": "SCAT_E_SHAPE", "O": "SCAT_E_SHAPE"}, direct=True)
def _b7(t):
    _bn_pre(t, 3, 48, 6, 6, 360)


# the same with 2048 / C limiting the slots per channel (C = 200, B = 13: 11 slots; above, B = 3 does)
@case("bn_bwd_pre_wide", ("scat_bn_bwd_pre",), 2e-5, expect={"S": "SCAT_E_SHAPE", "O": "SCAT_E_SHAPE"}, direct=True)
def _b7b(t):
    _bn_pre(t, 13, 200, 6, 6, 365)


def _bn_pre(t, B, C, H, W, seed):
    x, gamma, beta, res, dy, rm, rv = _bn_inputs(t, B, C, H, W, seed)
    add = t.once("add", lambda: R(seed + 7, (B, C, H, W)))
    ref = lambda: _bn_ref(t, x, gamma, beta, res, dy, rm, rv)
    f32 = lambda k: t.once("f32" + k, lambda: ref()[k].float())
    yout = t.inp(t.once("yout", lambda: ref()["y"].float()), "y_out")
    g, xg = t.acc(dy - add, "dy_g"), t.inp(x, "x")
    coef3, dg, db = t.ops.bn_bwd_pre(g, xg, True, t.inp(f32("scale"), "scale"), t.inp(f32("shift"), "shift"),
                                     t.inp(f32("mean"), "mean"), t.inp(f32("invstd"), "invstd"), t.inp(gamma, "gamma"),
                                     y_out=yout, dy_add=t.inp(add, "dy_add"))
    t.out("g", g, lambda: ref()["dres"], gate=1e-6)
    t.out("dgamma", dg, lambda: ref()["dg"])
    t.out("dbeta", db, lambda: ref()["db"])
    formed = v4(coef3[0]) * g + v4(coef3[1]) * xg + v4(coef3[2])     # (plain torch on the results)
    t.out("dx_formed", formed, lambda: ref()["dx"])


# BatchNorm backward straight from the max-pool's gradient: x and dx must be aligned (SCAT_E_SHAPE), dx is the
# wrapper's own allocation -> O rejects as well
@case("bn_bwd_maxpool", ("scat_bn_bwd_maxpool", "scat_maxpool3x3s2_fwd", "scat_bn_train_stats"), 2e-5,
      expect={"S": "SCAT_E_SHAPE", "O": "SCAT_E_SHAPE"}, direct=True, fills=("nan", "big"))
def _b8(t):
    _bn_maxpool(t, 5, 70, 10, 8, 370)


@case("bn_bwd_maxpool_wide", ("scat_bn_bwd_maxpool", "scat_maxpool3x3s2_fwd", "scat_bn_train_stats"), 2e-5,
      expect={"S": "SCAT_E_SHAPE", "O": "SCAT_E_SHAPE"}, direct=True)
def _b8b(t):
    _bn_maxpool(t, 13, 200, 4, 8, 375)


def _bn_maxpool(t, B, C, H, W, seed):
    x = t.once("x", lambda: R(seed, (B, C, H, W)) * 1.2 + 0.1)
    gamma, beta = t.once("gamma", lambda: U(seed + 1, (C,), 0.5, 1.5)), t.once("beta", lambda: U(seed + 2, (C,), -0.3, 0.3))
    dy = t.once("dy", lambda: R(seed + 3, (B, C, H // 2, W // 2)))
    xg, gg, bg = t.inp(x, "x"), t.inp(gamma, "gamma"), t.inp(beta, "beta")
    mean, invstd, scale, shift = t.ops.bn_train_stats(xg, gg, bg, t.acc(torch.zeros(C), "rm"), t.acc(torch.ones(C), "rv"))
    y, idx = t.ops.maxpool_fwd(xg, scale, shift, True)
    dx, dg, db = t.ops.bn_bwd_maxpool(t.inp(dy, "dy"), idx, xg, True, scale, shift, mean, invstd, gg)

    def ref():
        xr, gr, br = (a.double().requires_grad_(True) for a in (x, gamma, beta))
        yr = F.max_pool2d(F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5)), 3, 2, 1)
        return (yr.detach(),) + torch.autograd.grad(yr, (xr, gr, br), dy.double())
    rr = lambda i: (lambda: t.once("mpref", ref)[i])
    t.out("y", y, rr(0), gate=1e-6)
    t.out("dx", dx, rr(1))
    t.out("dgamma", dg, rr(2))
    t.out("dbeta", db, rr(3))


# the folded pair: the BatchNorm backward's apply formed in the operand load of the 1x1 data gradient (split taps kernel:
# g / z by 4-byte buffer loads, no alignment need) and of its weight gradient (the producer/consumer plan is dropped for
# skewed operands: csrc/conv_wgrad.hip) -> compute everywhere
@case("conv1x1_bnb_pair", ("scat_conv1x1_s1_bnb", "scat_conv1x1_wgrad_bnb"), 2e-5, direct=True, fills=("nan", "big"), maths=(1,))
def _b9(t):
    B, cin, cout, H = 3, 64, 256, 12
    g = t.once("g", lambda: R(380, (B, cout, H, H)))
    z = t.once("z", lambda: R(381, (B, cout, H, H)))
    coef = t.once("coef", lambda: U(382, (3, cout), -0.5, 0.5))
    w = t.once("w", lambda: R(383, (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5))
    a2 = t.once("a2", lambda: R(384, (B, cin, H, H)))
    sc, sh = t.once("sc", lambda: U(385, (cin,), 0.5, 1.5)), t.once("sh", lambda: U(386, (cin,), -0.5, 0.5))
    base = t.once("base", lambda: R(387, (B, cin, H, H)))
    dz = lambda: t.once("dz", lambda: v4(coef[0].double()) * g.double() + v4(coef[1].double()) * z.double() + v4(coef[2].double()))
    gg, zg, cg, wg = t.inp(g, "g"), t.inp(z, "z"), t.inp(coef, "coef3"), t.inp(w, "w")
    da_ref = lambda: F.conv_transpose2d(dz(), w.double())
    t.out("da", t.ops.conv1x1_dgrad_bnb(gg, zg, cg, wg, (B, cin, H, H)), da_ref)
    acc = t.acc(base, "da_acc")
    t.ops.conv1x1_dgrad_bnb(gg, zg, cg, wg, (B, cin, H, H), out=acc, accumulate=True)
    t.out("da_acc", acc, lambda: da_ref() + base.double())
    dw = t.ops.conv1x1_wgrad_bnb(gg, zg, cg, t.inp(a2, "a2"), (cout, cin, 1, 1), t.inp(sc, "scale"), t.inp(sh, "shift"), True)
    if t.aligned:
        assert "_bnb" in t.label(), t.label()
    t.out("dw", dw, lambda: torch.einsum("nop,nip->oi", dz().flatten(2), F.relu(a2.double() * v4(sc.double())
                                                                                 + v4(sh.double())).flatten(2)).view(cout, cin, 1, 1))
    # that weight gradient needs no slabs (its query is 0); 128 -> 128 over 2 x 252 pixels does (131 072 bytes)
    B, cin, cout, H, W = 2, 128, 128, 14, 18
    g2, z2 = t.once("g2", lambda: R(388, (B, cout, H, W))), t.once("z2", lambda: R(389, (B, cout, H, W)))
    c2, x2 = t.once("c2", lambda: U(378, (3, cout), -0.5, 0.5)), t.once("x2", lambda: R(379, (B, cin, H, W)))
    dw2 = t.ops.conv1x1_wgrad_bnb(t.inp(g2, "g2"), t.inp(z2, "z2"), t.inp(c2, "coef3_2"), t.inp(x2, "x2"), (cout, cin, 1, 1))
    dz2 = lambda: v4(c2[0].double()) * g2.double() + v4(c2[1].double()) * z2.double() + v4(c2[2].double())
    t.out("dw2", dw2, lambda: torch.einsum("nop,nip->oi", dz2().flatten(2), x2.double().flatten(2)).view(cout, cin, 1, 1))


def bn3_reference(c3, res_sign, gamma, mean, invstd, g_old, dc1, w1):
    """fp64: the masked accumulated gradient of a block output and bn3's backward constants.
    res_sign[B,C,H,W] bool: the sign of the block output (the caller decides where it comes from).
    -> (g, coef3[3,C], dgamma, dbeta) with dx = coef3[0] * g + coef3[1] * c3 + coef3[2]"""
    g = (g_old.double() + torch.einsum("bkhw,kc->bchw", dc1.double(), w1.double()[:, :, 0, 0])) * res_sign
    mu, is_ = v4(mean.double()), v4(invstd.double())
    xhat = (c3.double() - mu) * is_
    n = g.numel() // g.shape[1]
    db = g.sum(dim=(0, 2, 3))
    dg = (g * xhat).sum(dim=(0, 2, 3))
    ca = gamma.double() * invstd.double()
    cb = -ca * invstd.double() * (dg / n)
    cc = -ca * (db / n) - cb * mean.double()
    return g, torch.stack((ca, cb, cc)), dg, db


# the bn3 epilogue at a channel count with a partial 128-row tile.  A: the accumulating pointwise data gradient masks,
# stores and leaves the sums.  S / O: ops._pw_ok sends a skewed dy / w / out to the general engine, which takes no
# request (no groups), and the caller's fallback, scat_bn_bwd_pre, rejects the skewed gradient with SCAT_E_SHAPE.
@case("bn3_epilogue_ragged_c", ("scat_bn_bwd_pre_partials", "scat_conv1x1_s1"), 2e-5,
      expect={"S": "SCAT_E_SHAPE", "O": "SCAT_E_SHAPE"}, direct=True, maths=(1,))
def _b10(t):
    B, C, K, H = 3, 320, 64, 28
    ops = t.ops
    c3 = t.once("c3", lambda: R(390, (B, C, H, H)) * 1.3 + 0.2)
    res = t.once("res", lambda: R(391, (B, C, H, H)))
    gamma, beta = t.once("gamma", lambda: U(392, (C,), 0.5, 1.5)), t.once("beta", lambda: U(393, (C,), -0.3, 0.3))
    dc1 = t.once("dc1", lambda: R(394, (B, K, H, H)))
    w1 = t.once("w1", lambda: R(395, (K, C, 1, 1)) * 0.1)
    g_old = t.once("g_old", lambda: R(396, (B, C, H, H)))
    mean = t.once("mean", lambda: c3.double().mean(dim=(0, 2, 3)).float())
    invstd = t.once("invstd", lambda: (1.0 / torch.sqrt(c3.double().var(dim=(0, 2, 3), unbiased=False) + 1e-5)).float())
    scale = t.once("scale", lambda: gamma * invstd)
    shift = t.once("shift", lambda: beta - mean * scale)
    sign = t.once("sign", lambda: (c3.double() * v4(scale.double()) + v4(shift.double()) + res.double()) > 0)

    def mask_bytes():
        b = sign.reshape(-1, 4).to(torch.uint8)
        return (b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)).contiguous()
    ref = lambda i: (lambda: t.once("bn3ref", lambda: bn3_reference(c3, sign, gamma, mean, invstd, g_old, dc1, w1))[i])
    c3g, maskg, meang = t.inp(c3, "c3"), t.inp(t.once("mask", mask_bytes), "mask"), t.inp(mean, "mean")
    invg, gammag = t.inp(invstd, "invstd"), t.inp(gamma, "gamma")
    new = t.acc(g_old, "g")
    ops.conv2d_dgrad_w(t.inp(dc1, "dc1"), t.inp(w1, "w1"), (B, C, H, H), 1, 0, out=new, accumulate=True,
                       bnb=(c3g, maskg, meang))
    part, groups = new.scat_bnb or (None, 0)
    if t.aligned:
        assert groups > 0 and t.label().endswith("_epibn"), (groups, t.label())
    if groups > 0:
        coef3, dg, db = ops.bn_bwd_pre_partials(part, groups, (B, C, H, H), meang, invg, gammag)
    else:
        coef3, dg, db = ops.bn_bwd_pre(new, c3g, True, t.inp(scale, "scale"), t.inp(shift, "shift"), meang, invg, gammag,
                                       y_mask=maskg)
    t.out("g", new, ref(0))
    t.out("coef3", coef3, ref(1), gate=1e-5)
    t.out("dgamma", dg, ref(2), gate=1e-5)
    t.out("dbeta", db, ref(3), gate=1e-5)


# ====================================================================================================== pools, resampling

# pair kernel (even H, W % 4 == 0, aligned x / y / idx) and generic kernel (anything else), forward values bit-exact
@case("maxpool", ("scat_maxpool3x3s2_fwd", "scat_maxpool3x3s2_bwd"), 1e-6, fills=("nan", "big"), skews=(2, 3))
def _p1(t):
    for n, shp in enumerate([(2, 3, 6, 8), (2, 2, 10, 132), (2, 5, 13, 13), (3, 4, 7, 12)]):
        x = t.once(f"x{n}", lambda: R(400 + n, shp))
        yt = t.once(f"yt{n}", lambda: F.max_pool2d(x.double(), 3, 2, 1, return_indices=True))
        dy = t.once(f"dy{n}", lambda: R(410 + n, tuple(yt[0].shape)))
        y, idx = t.ops.maxpool_fwd(t.inp(x, f"x{n}"))
        t.out(f"y{n}", y, lambda: yt[0], gate=0.0)
        OH, OW = yt[0].shape[2:]
        tap = idx.cpu().long()
        flat = (2 * torch.arange(OH).view(1, 1, OH, 1) - 1 + tap // 3) * shp[3] + (2 * torch.arange(OW).view(1, 1, 1, OW) - 1 + tap % 3)
        assert torch.equal(flat, yt[1]), "arg-max taps differ from ATen's"

        def dx_ref():
            xx = x.double().requires_grad_(True)
            return torch.autograd.grad(F.max_pool2d(xx, 3, 2, 1), xx, dy.double())[0]
        t.out(f"dx{n}", t.ops.maxpool_bwd(t.inp(dy, f"dy{n}"), idx, shp), dx_ref)
    # the stem's fused relu(bn(x)) operand
    shp = (2, 6, 10, 12)
    x = t.once("xs", lambda: R(420, shp))
    sc, sh = t.once("sc", lambda: U(421, (6,), 0.5, 1.5)), t.once("sh", lambda: U(422, (6,), -0.5, 0.5))
    y, _ = t.ops.maxpool_fwd(t.inp(x, "xs"), t.inp(sc, "scale"), t.inp(sh, "shift"), True)
    t.out("y_tf", y, lambda: F.max_pool2d(F.relu(x.double() * v4(sc.double()) + v4(sh.double())), 3, 2, 1))


@case("avgpool", ("scat_avgpool_fwd", "scat_avgpool_bwd"), 1e-6)
def _p2(t):
    for n, shp in enumerate([(4, 128, 7, 7), (3, 5, 2, 3)]):
        x = t.once(f"x{n}", lambda: R(430 + n, shp))
        df = t.once(f"df{n}", lambda: R(432 + n, shp[:2]))
        base = t.once(f"b{n}", lambda: R(434 + n, shp))
        f_ref = lambda: F.relu(x.double().mean(dim=(2, 3)))
        dx_ref = lambda: (df.double() * (f_ref() > 0) / (shp[2] * shp[3])).view(*shp[:2], 1, 1).expand(shp).contiguous()
        f = t.ops.avgpool_fwd(t.inp(x, f"x{n}"))
        t.out(f"f{n}", f, f_ref)
        dfg = t.inp(df, f"df{n}")
        t.out(f"dx{n}", t.ops.avgpool_bwd(dfg, f, shp), dx_ref)
        acc = t.acc(base, f"acc{n}")
        t.ops.avgpool_bwd(dfg, f, shp, out=acc, accumulate=True)
        t.out(f"dxa{n}", acc, lambda: dx_ref() + base.double())


@case("subsample2", ("scat_subsample2",), 0.0, skews=(2, 3))
def _p3(t):
    for n, shp in enumerate([(2, 3, 8, 8), (3, 5, 7, 9), (2, 4, 5, 12), (1, 1, 1, 1)]):
        x = t.once(f"x{n}", lambda: R(440 + n, shp))
        t.out(f"y{n}", t.ops.subsample2(t.inp(x, f"x{n}")), lambda: x[:, :, ::2, ::2].double().contiguous())


@case("upsample_nearest", ("scat_upsample_nearest_fwd", "scat_upsample_nearest_bwd"), 1e-5)
def _p4(t):
    for n, (B, C, H, W, f) in enumerate([(2, 3, 7, 5, 2), (1, 5, 4, 6, 4), (2, 3, 3, 5, 8)]):
        x = t.once(f"x{n}", lambda: R(450 + n, (B, C, H, W)))
        dy = t.once(f"dy{n}", lambda: R(453 + n, (B, C, H * f, W * f)))
        t.out(f"y{n}", t.ops.upsample_nearest_fwd(t.inp(x, f"x{n}"), f),
              lambda: F.interpolate(x.double(), scale_factor=float(f), mode="nearest"), gate=0.0)
        t.out(f"dx{n}", t.ops.upsample_nearest_bwd(t.inp(dy, f"dy{n}"), f),
              lambda: dy.double().reshape(B, C, H, f, W, f).sum(dim=(3, 5)))


# vector form for W % 4 == 0 and aligned out / full-resolution inputs (csrc/misc.hip), scalar otherwise
@case("fuse_sum", ("scat_fuse_sum",), 1e-6, skews=(2, 3))
def _p5(t):
    for n, (B, C, H, W) in enumerate([(2, 16, 14, 14), (1, 8, 8, 12), (2, 8, 6, 10)]):
        x0 = t.once(f"x0{n}", lambda: R(460 + n, (B, C, H, W)))
        terms, parts = [(t.inp(x0, "x0"), None, None, 0)], [(x0, None, None, 0)]
        for j, k in enumerate((1, 2, 0)):
            if H % (1 << k) or W % (1 << k):
                continue
            c = t.once(f"c{n}{j}", lambda: R(463 + 3 * n + j, (B, C, H >> k, W >> k)) * (1.3 - 0.3 * j) + 0.2 * j)
            sc, sh = t.once(f"sc{n}{j}", lambda: U(470 + j, (C,), 0.5, 1.5)), t.once(f"sh{n}{j}", lambda: U(475 + j, (C,), -0.5, 0.5))
            terms.append((t.inp(c, "c"), t.inp(sc, "sc"), t.inp(sh, "sh"), k))
            parts.append((c, sc, sh, k))

        def ref(parts=parts, order=None, relu=True):
            tot = 0.0
            for c, sc, sh, k in (parts if order is None else [parts[i] for i in order]):
                term = c.double() if sc is None else c.double() * v4(sc.double()) + v4(sh.double())
                tot = tot + (F.interpolate(term, scale_factor=1 << k, mode="nearest") if k else term)
            return F.relu(tot) if relu else tot
        t.out(f"y{n}", t.ops.fuse_sum(terms, relu=True), ref)
        t.out(f"y2{n}", t.ops.fuse_sum([terms[1], terms[0]], relu=False), lambda: ref(order=(1, 0), relu=False))


@case("token_mean", ("scat_token_mean_fwd", "scat_token_mean_bwd"), 1e-5)
def _p6(t):
    for n, (B, T, D) in enumerate([(3, 7, 5), (2, 1, 61), (4, 129, 197)]):
        x = t.once(f"x{n}", lambda: R(480 + n, (B, T, D), mean=0.5))
        dy = t.once(f"dy{n}", lambda: R(483 + n, (B, D)))
        t.out(f"y{n}", t.ops.token_mean_fwd(t.inp(x, f"x{n}")), lambda: x.double().mean(dim=1))
        t.out(f"dx{n}", t.ops.token_mean_bwd(t.inp(dy, f"dy{n}"), T),
              lambda: (dy.double() / T).unsqueeze(1).expand(B, T, D).contiguous(), gate=1e-6)


# ====================================================================================================== token path

@case("layernorm", ("scat_layernorm_fwd", "scat_layernorm_bwd"), 1e-5, skews=(2, 3))
def _t1(t):
    # (21400 x 196 >= 1 << 22: the parameter sums in 79 row slices, their partials behind the rows * dim floats of ws)
    for rows, dim in ((7, 50), (40, 196), (21400, 196)):
        key = f"{rows}"
        x = t.once("x" + key, lambda: R(500 + rows, (rows, dim)) * 2 + 0.3)
        gm, bt = t.once("g" + key, lambda: U(501, (dim,), 0.7, 1.3)), t.once("b" + key, lambda: U(502, (dim,), -0.2, 0.2))
        dy = t.once("dy" + key, lambda: R(503 + rows, (rows, dim)))

        def ref():
            xr, gr, br = (a.double().requires_grad_(True) for a in (x, gm, bt))
            y = F.layer_norm(xr, (dim,), gr, br, 1e-5)
            return (y.detach(),) + torch.autograd.grad(y, (xr, gr, br), dy.double())
        rr = lambda i: (lambda: t.once("lnref" + key, ref)[i])
        xg, gg = t.inp(x, "x" + key), t.inp(gm, "gamma")
        y, mean, rstd = t.ops.layernorm_fwd(xg, gg, t.inp(bt, "beta"))
        t.out("y" + key, y, rr(0))
        t.out("mean" + key, mean, lambda: x.double().mean(dim=1))
        t.out("rstd" + key, rstd, lambda: 1.0 / torch.sqrt(x.double().var(dim=1, unbiased=False) + 1e-5))
        dyg = t.inp(dy, "dy" + key)
        dx, dg, db = t.ops.layernorm_bwd(dyg, xg, gg, mean, rstd)
        t.out("dx" + key, dx, rr(1))
        t.out("dg" + key, dg, rr(2))
        t.out("db" + key, db, rr(3))
        dx_only, _, _ = t.ops.layernorm_bwd(dyg, xg, gg, mean, rstd, want_params=False)
        t.out("dx_only" + key, dx_only, rr(1))


def _attention(t, B, n, heads, seed):
    d = 64
    qkv = t.once("qkv", lambda: R(seed, (B, n, 3 * heads * d)))
    do = t.once("do", lambda: R(seed + 1, (B, n, heads * d)))
    scale = d ** -0.5

    def ref():
        qr = qkv.double().requires_grad_(True)
        q, k, v = (z.reshape(B, n, heads, d).permute(0, 2, 1, 3) for z in qr.split(heads * d, dim=-1))
        attn = (q @ k.transpose(-1, -2) * scale).softmax(-1)
        out = (attn @ v).permute(0, 2, 1, 3).reshape(B, n, heads * d)
        return out.detach(), attn.detach(), torch.autograd.grad(out, qr, do.double())[0]
    rr = lambda i: (lambda: t.once("attref", ref)[i])
    qg = t.inp(qkv, "qkv")
    og, ag = t.ops.attention_fwd(qg, heads, d, scale)
    t.out("out", og, rr(0))
    t.out("attn", ag, rr(1))
    t.out("dqkv", t.ops.attention_bwd(t.inp(do, "dout"), qg, ag, heads, d, scale), rr(2), gate=2e-5)


_ATT = ("scat_attention_fwd", "scat_attention_bwd")


# n = 21, 65: the LDS kernels (per-element global accesses).  n = 64, 96: the matrix-pipe core for aligned qkv / attn /
# dout (16-byte loads of q, k, v rows), the LDS kernels otherwise.  In O the saved attn is an output of the forward:
# skewed, so the forward and the backward both leave the matrix-pipe core.
@case("attention_n21", _ATT, 1e-5)
def _t2(t):
    _attention(t, 3, 21, 4, 510)


@case("attention_n65", _ATT, 1e-5)
def _t3(t):
    _attention(t, 3, 65, 2, 520)


@case("attention_n64", _ATT, 1e-5, skews=(2, 3))
def _t4(t):
    _attention(t, 3, 64, 3, 530)


@case("attention_n96", _ATT, 1e-5)
def _t5(t):
    _attention(t, 2, 96, 5, 540)


# one launch for the qkv projection + attention: the token rows h are read with 16-byte buffer loads and must be aligned,
# tested together with the workspace -> SCAT_E_WORKSPACE for a skewed h; qkv / attn / ao are stored per element -> O computes
@case("vit_qkv_attn_fused", ("scat_vit_qkv_attn_fwd",), 2e-5, expect={"S": "SCAT_E_WORKSPACE"}, direct=True, maths=(1,))
def _t6(t):
    B, n, dim, heads, d = 5, 16, 200, 2, 64
    inner = heads * d
    h = t.once("h", lambda: R(550, (B * n, dim)))
    w = t.once("w", lambda: R(551, (3 * inner, dim), std=dim ** -0.5))
    scale = d ** -0.5

    def ref():
        qkv = h.double() @ w.double().t()
        q, k, v = (z.reshape(B, n, heads, d).permute(0, 2, 1, 3) for z in qkv.split(inner, dim=-1))
        attn = (q @ k.transpose(-1, -2) * scale).softmax(-1)
        return qkv, (attn @ v).permute(0, 2, 1, 3).reshape(B, n, inner), attn
    rr = lambda i: (lambda: t.once("vitref", ref)[i])
    qg, og, ag = t.ops.qkv_attention_fwd(t.inp(h, "h"), t.inp(w, "wqkv"), B, n, heads, scale)
    t.out("qkv", qg, rr(0))
    t.out("out", og, rr(1))
    t.out("attn", ag, rr(2))


def _favor64(kqv, w):
    B, T, H, e3 = kqv.shape
    e, m = e3 // 3, w.shape[0]
    k, q, v = (z.permute(0, 2, 1, 3) for z in kqv.split(e, dim=-1))

    def prm_exp(z):
        return torch.exp(z @ w.t() - (z * z).sum(dim=-1, keepdim=True) / 2) / math.sqrt(m)
    kp, qp = prm_exp(k), prm_exp(q)
    ksum = kp.sum(dim=2)
    D = (qp * ksum.unsqueeze(2)).sum(dim=-1)
    kptv = torch.einsum("bhtn,bhtm->bhnm", v, kp)
    y = torch.einsum("bhtm,bhnm->bhtn", qp, kptv) / D.unsqueeze(-1)
    return y.permute(0, 2, 1, 3).reshape(B, T, H * e), kp, qp, kptv, ksum, D


@case("performer", ("scat_performer_fwd", "scat_performer_bwd"), 2e-5)
def _t7(t):
    B, T, H, e, m = 2, 21, 8, 49, 65
    kqv = t.once("kqv", lambda: R(560, (B, T, H, 3 * e)) * (1.5 / e ** 0.5))
    w = t.once("w", lambda: R(561, (m, e)))
    dy = t.once("dy", lambda: R(562, (B, T, H * e)))

    def ref():
        k64 = kqv.double().requires_grad_(True)
        outs = _favor64(k64, w.double())
        (dk,) = torch.autograd.grad(outs[0], (k64,), dy.double())
        return tuple(o.detach() for o in outs) + (dk,)
    rr = lambda i: (lambda: t.once("pref", ref)[i])
    kg, wg = t.inp(kqv, "kqv"), t.inp(w, "w")
    y, saved = t.ops.performer_fwd(kg, wg, H)
    t.out("y", y, rr(0))
    for i, (nm, got) in enumerate(zip(("kp", "qp", "kptv", "ksum", "D"), saved)):
        t.out(nm, got, rr(1 + i))
    dk = t.ops.performer_bwd(t.inp(dy, "dy"), kg, wg, y, saved)
    for sl in range(3):
        t.out("d" + "kqv"[sl], dk[..., sl * e:(sl + 1) * e], lambda sl=sl: rr(6)()[..., sl * e:(sl + 1) * e])


# the fp32 GEMM engine picks 16-byte loaders per operand from its pointer and strides (csrc/linear.hip av / bv)
@case("linear_gemm", ("scat_gemm",), 2e-5, skews=(2, 3))
def _t8(t):
    # (K = 147: one pass.  7 x 66 x 1090: 4 K-slices forward.  84 x 588 x 784: 3 forward, 3 for the input gradient)
    for M, N, K in ((84, 3, 147), (300, 200, 147), (7, 66, 1090), (84, 588, 784)):
        key = f"{M}x{N}"
        x = t.once("x" + key, lambda: R(570 + M, (M, K)))
        w = t.once("w" + key, lambda: R(571 + M, (N, K), std=K ** -0.5))
        b = t.once("b" + key, lambda: R(572 + M, (N,)))
        dy = t.once("dy" + key, lambda: R(573 + M, (M, N)))
        base = t.once("base" + key, lambda: R(574 + M, (M, N)))
        xg, wg, dyg = t.inp(x, "x" + key), t.inp(w, "w" + key), t.inp(dy, "dy" + key)
        y_ref = lambda: x.double() @ w.double().t() + b.double()
        t.out("y" + key, t.ops.linear_fwd(xg, wg, t.inp(b, "bias")), y_ref)
        acc = t.acc(base, "y_acc" + key)
        t.ops.linear_fwd(xg, wg, None, out=acc, accumulate=True)
        t.out("ya" + key, acc, lambda: x.double() @ w.double().t() + base.double())
        t.out("dx" + key, t.ops.linear_dgrad(dyg, wg), lambda: dy.double() @ w.double())
        t.out("dw" + key, t.ops.linear_wgrad(dyg, xg), lambda: dy.double().t() @ x.double())


# scat_gemm does not reject a missing or short workspace: it drops its K-slices and runs one pass, whose epilogue applies
# bias and accumulate in the contraction kernel (the sliced form applies them in the reduce).  84 x 588 x 784: 3 slices,
# 592 704 bytes.  (0, 0) and a buffer one byte short end in _split1, the exact one in _split3; the short buffer is real
# and guarded, so a launch that believed the plan instead of ws_bytes would be seen.
@case("gemm_without_workspace", ("scat_gemm",), 2e-5, direct=True)
def _t8b(t):
    M, N, K = 84, 588, 784
    a = t.once("a", lambda: R(575, (M, K)))
    b = t.once("b", lambda: R(576, (K, N), std=K ** -0.5))
    bias = t.once("bias", lambda: R(577, (N,)))
    base = t.once("base", lambda: R(578, (M, N)))
    ag, bg, biasg = t.inp(a, "a"), t.inp(b, "b"), t.inp(bias, "bias")
    need = int(t.lib.scat_gemm_ws(M, N, K))
    assert need == 3 * M * N * 4
    ref = lambda: a.double() @ b.double()
    for tag, nbytes, want in (("none", 0, "_split1"), ("short", need - 1, "_split1"), ("exact", need, "_split3")):
        ws, nb = _exact_ws(t, nbytes)
        c = t.buf((M, N), "c_" + tag)
        t.lib.scat_gemm(P(ag), K, 1, P(bg), N, 1, P(c), N, 1, M, N, K, P(biasg), 2, 0, ws, nb, t.stream())
        assert t.label().endswith(want), (tag, t.label())
        t.out("c_" + tag, c, lambda: ref() + bias.double())
        acc = t.acc(base, "acc_" + tag)
        t.lib.scat_gemm(P(ag), K, 1, P(bg), N, 1, P(acc), N, 1, M, N, K, 0, 0, 1, ws, nb, t.stream())
        assert t.label().endswith(want), (tag, t.label())
        t.out("acc_" + tag, acc, lambda: ref() + base.double())


# the same contraction on the pointwise split kernel: b by 4-byte buffer loads, a re-laid into the workspace -> no
# alignment need on a / b / c; bias along columns, transposed a, accumulate
@case("gemm_split", ("scat_gemm_split",), 2e-5, direct=True, maths=(1,))
def _t9(t):
    for M, N, K in ((300, 200, 147), (130, 70, 66)):
        key = f"{M}"
        a = t.once("a" + key, lambda: R(580 + M, (M, K)))
        b = t.once("b" + key, lambda: R(581 + M, (K, N), std=K ** -0.5))
        bias = t.once("bias" + key, lambda: R(582 + M, (N,)))
        base = t.once("base" + key, lambda: R(583 + M, (M, N)))
        ref = lambda: a.double() @ b.double()
        bg = t.inp(b, "b" + key)
        c = t.ops.gemm_split(t.inp(a, "a" + key), 0, bg, t.buf((M, N), "c" + key), M, N, K, t.inp(bias, "bias"))
        if t.aligned:
            assert "gemm_split" in t.label()
        t.out("c" + key, c, lambda: ref() + bias.double())
        c2 = t.ops.gemm_split(t.inp(a.t().contiguous(), "at" + key), 1, bg, t.acc(base, "c2" + key), M, N, K, None, accumulate=True)
        t.out("c2" + key, c2, lambda: ref() + base.double())


@case("gemm_group", ("scat_gemm_group_ws", "scat_gemm_group"), 2e-5)
def _t10(t):
    # (M is the contraction length: 300 and 84 tokens run in one pass, 600 in 2 K-slices through the workspace)
    for M, dims in ((300, [(70, 33), (129, 64), (64, 200), (3, 147)]), (84, [(3, 147), (147, 196)]), (600, [(70, 33), (3, 147)])):
        pairs, cpu = [], []
        for j, (N, K) in enumerate(dims):
            dy = t.once(f"dy{M}_{j}", lambda: R(590 + M + j, (M, N)))
            x = t.once(f"x{M}_{j}", lambda: R(595 + M + j, (M, K)))
            pairs.append((t.inp(dy, f"dy{j}"), t.inp(x, f"x{j}")))
            cpu.append((dy, x))
        outs = t.ops.linear_wgrad_group(pairs)
        if t.aligned:
            assert t.label().startswith("gemm_group"), t.label()
        for j, ((dy, x), o) in enumerate(zip(cpu, outs)):
            t.out(f"dw{M}_{j}", o, lambda dy=dy, x=x: dy.double().t() @ x.double())


@case("transpose2d", ("scat_transpose2d",), 0.0, direct=True)
def _t11(t):
    for R_, C_ in ((147, 200), (33, 65), (1, 7)):
        src = t.once(f"s{R_}", lambda: R(600 + R_, (R_, C_)))
        dst = t.buf((C_, R_), f"dst{R_}")
        t.lib.scat_transpose2d(P(t.inp(src, "src")), P(dst), R_, C_, t.stream())
        t.out(f"t{R_}", dst, src.double().t().contiguous())


@case("colsum", ("scat_colsum", "scat_colsum_sliced", "scat_colsum_group"), 1e-5)
def _t12(t):
    # (the second: row slices — 4.3 M elements, above the 2^22 switch; the third: 79 ragged slices of 304 rows)
    for rows, cols in ((300, 61), (22000, 196), (24001, 196)):
        x = t.once(f"x{rows}", lambda: R(610 + cols, (rows, cols), mean=0.25))
        xg = t.inp(x, f"x{rows}")
        t.out(f"s{rows}", t.ops.colsum(xg), lambda: x.double().sum(0))
        acc = t.acc(torch.ones(cols), f"acc{rows}")
        t.ops.colsum(xg, out=acc, accumulate=True)
        t.out(f"sa{rows}", acc, lambda: x.double().sum(0) + 1.0)
    # one slice: the entry point is scat_colsum, its workspace unused (query 0) and absent
    x300, small = t.once("x300", lambda: R(610 + 61, (300, 61), mean=0.25)), t.buf((61,), "direct300")
    assert t.lib.scat_colsum_ws(300, 61) == 0
    t.lib.scat_colsum_sliced(P(t.inp(x300, "x300_direct")), P(small), 300, 61, 0, 0, 0, t.stream())
    t.out("direct300", small, lambda: x300.double().sum(0))
    xs = [t.once(f"g{j}", lambda: R(620 + j, shp, mean=0.1 * j)) for j, shp in enumerate([(77, 1), (5, 1090), (300, 3), (84, 196)])]
    for j, (x, o) in enumerate(zip(xs, t.ops.colsum_group([t.inp(x, f"g{j}") for j, x in enumerate(xs)]))):
        t.out(f"g{j}", o, lambda x=x: x.double().sum(0))


@case("elementwise", ("scat_gelu_fwd", "scat_gelu_bwd", "scat_relu_fwd", "scat_relu_bwd", "scat_axpy"), 1e-6, skews=(2, 3))
def _t13(t):
    for n in (4 * 21 * 61, 1023):
        x = t.once(f"x{n}", lambda: R(630 + n, (n,)))
        dy = t.once(f"dy{n}", lambda: R(631 + n, (n,)))
        xg, dyg = t.inp(x, "x"), t.inp(dy, "dy")

        def gelu_bwd():
            xr = x.double().requires_grad_(True)
            return torch.autograd.grad(F.gelu(xr), xr, dy.double())[0]
        t.out(f"gelu{n}", t.ops.gelu_fwd(xg), lambda: F.gelu(x.double()))
        t.out(f"dgelu{n}", t.ops.gelu_bwd(dyg, xg), gelu_bwd, gate=1e-5)
        t.out(f"axpy{n}", t.ops.axpy(xg, dyg, 0.5), lambda: x.double() + 0.5 * dy.double())
        r = t.ops.relu_fwd(xg)
        t.out(f"relu{n}", r, lambda: F.relu(x.double()), gate=0.0)
        t.out(f"drelu{n}", t.ops.relu_bwd(dyg, r), lambda: dy.double() * (x > 0), gate=0.0)


@case("dropout", ("scat_dropout",), 1e-6)
def _t14(t):
    from oracle.scat_oracle import hash_dropout_mask

    for n, p in ((100003, 0.1), (1023, 0.5), (7, 0.0)):
        x = t.once(f"x{n}", lambda: R(640 + n, (n,), mean=0.01))
        seed = 0x1234567 * n + 99
        y = t.ops.dropout(t.inp(x, f"x{n}"), p, seed)
        keep = t.once(f"keep{n}", lambda: hash_dropout_mask(n, p, seed))
        assert torch.equal((y.cpu() != 0).double(), keep)
        t.out(f"y{n}", y, lambda: x.double() * keep / (1.0 - p))


@case("tokens", ("scat_tokens_fwd", "scat_tokens_bwd"), 1e-6)
def _t15(t):
    B, T, D = 4, 21, 61
    x, pe, mt = t.once("x", lambda: R(650, (B, T, D))), t.once("pe", lambda: R(651, (T, D))), t.once("mt", lambda: R(652, (D,)))
    dy = t.once("dy", lambda: R(653, (B, T, D)))
    masked = [5, 0, 17, 9]

    def ref():
        xr, mr = x.double().requires_grad_(True), mt.double().requires_grad_(True)
        f2 = (xr + pe.double()).clone()
        f2[:, masked, :] = mr
        return (f2.detach(),) + torch.autograd.grad(f2, (xr, mr), dy.double())
    rr = lambda i: (lambda: t.once("tokref", ref)[i])
    mi = t.inp(torch.tensor(masked, dtype=torch.int32), "masked")
    xg, peg = t.inp(x, "x"), t.inp(pe, "pe")
    t.out("y", t.ops.tokens_fwd(xg, peg, t.inp(mt, "mask_token"), mi), rr(0))
    t.out("y_plain", t.ops.tokens_fwd(xg, peg, None, None), lambda: x.double() + pe.double())
    dx, dm = t.ops.tokens_bwd(t.inp(dy, "dy"), mi)
    t.out("dx", dx, rr(1))
    t.out("dmask", dm, rr(2), gate=1e-5)


# ====================================================================================================== head and step

def _regressor(t, B, Fd, Pn, iters, offsets, root, seed):
    from scat_amd import synth

    key = f"{Fd}_{iters}"
    feat = t.once("feat" + key, lambda: F.relu(R(seed, (B, Fd))))
    fo = t.once("fo" + key, lambda: R(seed + 1, (B, Pn - 3), std=0.05)) if offsets else None
    mean = t.once("mean" + key, lambda: torch.from_numpy(synth.mean_params(seed + 2, Pn)).view(-1))
    w = t.once("w" + key, lambda: R(seed + 3, (Pn, Fd + Pn), std=0.3 * (Fd + Pn) ** -0.5))
    b = t.once("b" + key, lambda: R(seed + 4, (Pn,), std=0.05))
    dout = t.once("dout" + key, lambda: R(seed + 5, (B, Pn)))

    def ref():
        fr, wr, br = (a.double().requires_grad_(True) for a in (feat, w, b))
        fo_r = fo.double().requires_grad_(True) if offsets else None
        pred = mean.double().repeat(B, 1).clone()
        if offsets:
            pred = torch.cat((pred[:, :3], pred[:, 3:] + fo_r), 1)
        preds = [pred]
        for _ in range(iters):
            pred = pred + F.linear(torch.cat((fr, pred), 1), wr, br)
            preds.append(pred)
        out = pred
        if root:
            j = pred[:, 3:].reshape(B, -1, 3)
            out = torch.cat((pred[:, :3], (j - j[:, 1:2]).reshape(B, -1)), 1)
        ins = [a for a in (fr, wr, br, fo_r) if a is not None]
        g = {}
        if out.requires_grad:      # (no iteration and no offsets: the output is the mean, nothing to differentiate)
            g = dict(zip(["feat", "w", "b", "fo"], torch.autograd.grad(out, ins, dout.double(), allow_unused=True)))
        return out.detach(), torch.stack([p.detach() for p in preds]), g
    rr = lambda: t.once("regref" + key, ref)
    featg, wg = t.inp(feat, "feat"), t.inp(w, "w")
    og, preds = t.ops.regressor_fwd(featg, t.inp(fo, "feat_out") if offsets else None, t.inp(mean, "mean"), wg,
                                    t.inp(b, "bias"), iters, root)
    t.out("out" + key, og, lambda: rr()[0])
    t.out("preds" + key, preds, lambda: rr()[1])
    dfeat, dfo, dw, db = t.ops.regressor_bwd(t.inp(dout, "dout"), featg, preds, wg, iters, root, want_dfeat_out=offsets)
    if offsets:
        t.out("dfo" + key, dfo, lambda: rr()[2]["fo"])
    if iters:
        t.out("dfeat" + key, dfeat, lambda: rr()[2]["feat"])
        t.out("dw" + key, dw, lambda: rr()[2]["w"])
        t.out("db" + key, db, lambda: rr()[2]["b"])
    else:       # no iteration: the loop's parameters get no gradient, the buffers are still written (zeros)
        t.out("dfeat" + key, dfeat, torch.zeros(B, Fd, dtype=torch.float64), gate=0.0)
        t.out("dw" + key, dw, torch.zeros(Pn, Fd + Pn, dtype=torch.float64), gate=0.0)
        t.out("db" + key, db, torch.zeros(Pn, dtype=torch.float64), gate=0.0)


@case("regressor_1024x66", ("scat_regressor_fwd", "scat_regressor_bwd"), 1e-5)
def _h1(t):
    _regressor(t, 5, 1024, 66, 3, True, True, 700)
    _regressor(t, 5, 1024, 66, 0, True, True, 710)


@case("regressor_196x61", ("scat_regressor_fwd", "scat_regressor_bwd"), 1e-5)
def _h2(t):
    _regressor(t, 5, 196, 61, 3, False, False, 720)
    _regressor(t, 5, 196, 61, 0, False, False, 730)


# gt3d / gt2d are interior pointers of the label rows (floats 0 / 63 of 105, 61 / 124 of 166): odd offsets already
@case("loss", ("scat_loss_fwd_bwd",), 1e-5)
def _h3(t):
    from oracle.scat_oracle import scat_loss
    from scat_amd import synth

    B = 5
    out = t.once("out", lambda: torch.cat((U(740, (B, 1), 4.0, 6.0), R(741, (B, 2), std=0.1), R(742, (B, 63), std=0.03)), 1))
    lab105 = t.once("lab105", lambda: torch.from_numpy(synth.labels(743, B)))
    lab166 = t.once("lab166", lambda: torch.cat((R(744, (B, 61)), lab105), 1).contiguous())
    og = t.inp(out, "out")
    for lab, tag in ((lab105, "105"), (lab166, "166")):
        def ref(lab=lab):
            o = out.double().requires_grad_(True)
            loss, l3, l2, _ = scat_loss(o, lab.double())
            return torch.stack([loss, l3, l2]).detach(), torch.autograd.grad(loss, o)[0]
        rr = lambda i, tag=tag, ref=ref: (lambda: t.once("lossref" + tag, ref)[i])
        losses, dout = t.ops.loss_fwd_bwd(og, t.inp(lab, "labels" + tag))
        t.out("losses" + tag, losses, rr(0))
        t.out("dout" + tag, dout, rr(1), gate=1e-4)      # (the bar test_regressor_and_loss holds this gradient to)


@case("pose_length_term", ("scat_pose_length_term",), 1e-6, skews=(2, 3))
def _h4(t):
    for n, shp in enumerate([(3, 5, 7, 9), (2, 21, 4, 4)]):      # C * HW % 4 != 0 / == 0: scalar / 16-byte loads per image
        pl = t.once(f"pl{n}", lambda: R(750 + n, shp, std=0.01))

        def ref():
            lens = pl.double().square().sum(dim=[2, 3]).mean(dim=[1]).sqrt()
            return (lens - 0.01 * lens.mean()).square().mean()
        t.out(f"l_pl{n}", t.ops.pose_length_term(t.inp(pl, f"pl{n}")), ref)


# in place: p, m, v carry real values between guards (g is read only); three steps.  The C ABI carries lr, beta1, beta2
# and eps as fp32 (include/scat_hip.h scat_adam), so the operation's hyper-parameters ARE the fp32 values: fl32(0.999) is
# 0.999 (1 + 1.3e-8) and 1 - fl32(0.999) is 0.001 (1 - 1.29e-5).  The fp64 reference is the same recurrence on the same
# inputs, hyper-parameters included; a reference run with the decimal 0.9 / 0.999 would be another operation's (off by
# 2.4e-7 in m and 1.3e-5 in v, whatever precision the kernel computes in).
@case("adam", ("scat_adam",), 1e-6, skews=(2, 3))
def _h5(t):
    n = 100003
    p0, gr = t.once("p", lambda: R(760, (n,))), t.once("g", lambda: R(761, (n,), std=1e-3))
    lr, b1, b2, eps = (float(np.float32(a)) for a in (5e-4, 0.9, 0.999, 1e-8))

    def ref():
        p, m, v = p0.double().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for step in (1, 2, 3):
            g = (gr * step).double()
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            p = p - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
        return p, m, v
    rr = lambda i: (lambda: t.once("adamref", ref)[i])
    p, m, v = t.acc(p0, "p"), t.acc(torch.zeros(n), "m"), t.acc(torch.zeros(n), "v")
    for step in (1, 2, 3):
        t.ops.adam(p, t.inp(gr * step, f"g{step}"), m, v, 5e-4, step)
    t.out("p", p, rr(0))
    t.out("m", m, rr(1))
    t.out("v", v, rr(2))


def _resize_ref(u8, OH, OW):
    """x / 127.5 - 1, then bilinear with align_corners=False, in fp64"""
    return F.interpolate(u8.double() / 127.5 - 1.0, size=(OH, OW), mode="bilinear", align_corners=False)


# source sizes whose ratio to 224 is a power of two: the kernel's fp32 source coordinate is then exact and the fp64
# formula is a fair reference at the 1e-5 of test_preprocess_u8 (tests/test_gpu_augment.py explains the 256 case)
@case("preprocess_u8", ("scat_preprocess_u8",), 1e-5, skews=(2, 3))
def _h6(t):
    for n, (SH, SW) in enumerate([(112, 448), (224, 224), (56, 112)]):
        g = torch.Generator().manual_seed(770 + n)
        u8 = t.once(f"u8{n}", lambda: torch.randint(0, 256, (2, 3, SH, SW), generator=g, dtype=torch.uint8))
        ref = lambda: _resize_ref(u8, 224, 224)
        t.out(f"chw{n}", t.ops.preprocess_u8(t.inp(u8, f"chw{n}")), ref)
        t.out(f"hwc{n}", t.ops.preprocess_u8(t.inp(u8.permute(0, 2, 3, 1), f"hwc{n}"), hwc=True), ref)


# the two augmentation launches: the plan must be 8-byte aligned (it holds fp64 values) and the image 16-byte aligned
# (16-byte stores): SCAT_E_ARG when the wrapper's own plan / image allocation is skewed (S and O alike)
@case("augment", ("scat_augment_plan", "scat_augment_warp_u8"), 1e-5, expect={"S": "SCAT_E_ARG", "O": "SCAT_E_ARG"}, direct=True)
def _h7(t):
    import _augment_oracle as AO

    W, H, B = 640, 480, 4

    def make():
        rng = np.random.default_rng(23)
        j2, j3 = AO.seeded_joints(rng, B, W, H)
        params = np.array([[0, 0, 0, 0], [1, 3, 1, 0], [0, 0, 0, 37], [1, 10, 0, 270]], dtype=np.int32)
        frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        labels, images = [], []
        for i in range(B):
            lab, plan = AO.labels_and_plan(j2[i], j3[i], W, H, params[i, 0], params[i, 3])
            assert AO.half_distance(plan) >= 1e-6
            labels.append(lab)
            images.append(AO.image(frames[i], params[i, 0], params[i, 1], params[i, 2], plan))
        return (torch.from_numpy(j2.astype(np.float32)), torch.from_numpy(j3.astype(np.float32)), torch.from_numpy(params),
                torch.from_numpy(frames), torch.from_numpy(np.stack(labels)), torch.from_numpy(np.stack(images)))
    j2, j3, params, frames, labels_ref, images_ref = t.once("aug", make)
    labels, plan = t.ops.augment_plan(t.inp(j2, "j2d"), t.inp(j3, "j3d"), t.inp(params, "params"), (W, H))
    t.out("labels3d", labels[:, :63], labels_ref[:, :63], gate=1e-6)
    t.out("labels2d", labels[:, 63:], labels_ref[:, 63:], gate=1e-6)
    t.out("plan", plan, None)            # (its integer part is what the image below is made from; here: written and finite)
    img = t.ops.augment_warp_u8(t.inp(frames, "frames_hwc"), plan, (224, 224), hwc=True)
    t.out("image_hwc", img, images_ref)
    img2 = t.ops.augment_warp_u8(t.inp(frames.permute(0, 3, 1, 2), "frames_chw"), plan, (224, 224), hwc=False)
    t.out("image_chw", img2, images_ref)


# ====================================================================================================== the runner

PARAMS = [pytest.param(c, m, f, id=c.name + ("" if m is None else f"-math{m}") + ("" if f == "nan" else f"-{f}"))
          for c in CASES for m in c.maths for f in c.fills]


@pytest.fixture(scope="module")
def ops():
    from scat_amd import ops as o
    from scat_amd._lib import lib

    lib().scat_check_device()
    return o


@pytest.fixture(scope="module")
def arena():
    return _guard.Arena(DEV, "nan", nbytes=ARENA_BYTES)


@contextlib.contextmanager
def _placed(ops, arena, mp, skew_out):
    """ops as the case sees it: torch -> the arena proxy, workspaces of exactly the requested size and prepared-weight
    slots carved as scratch, lib() -> the call recorder"""
    from scat_amd._lib import lib

    proxy = _guard.TorchProxy(arena, skew_out)
    rec = _Recorder(lib())
    real_slot = ops.WeightPrep.slot
    workspace = _guard.exact_workspace(proxy, ops._stream)

    def wp_slot(self, *a, **k):
        with proxy.scratch():
            return real_slot(self, *a, **k)

    with mp.context() as m:
        m.setattr(ops, "torch", proxy)
        m.setattr(ops, "workspace", workspace)
        m.setattr(ops.WeightPrep, "slot", wp_slot)
        m.setattr(ops, "lib", lambda: rec)
        yield rec, m


def _compare(name, got, ref, gate):
    if ref is None:
        return 0.0
    g = got.detach().cpu()
    if gate == 0.0:
        ok = torch.equal(g.double(), ref.double().reshape(g.shape))
        return 0.0 if ok else float("inf")
    return rel_err(g, ref.reshape(g.shape))


@pytest.mark.parametrize("case,math,fill", PARAMS)
def test_guarded_placements(case, math, fill, ops, arena, monkeypatch):
    from scat_amd._lib import ScatError

    saved_mode = ops.get_math_mode()
    if math is not None:
        ops.set_math_mode(math)
    cache, results = {}, {}
    placements = [("A", 0, 0), ("S", 1, 1), ("O", 0, 1)] + [(f"S{k}", k, k) for k in case.skews]
    try:
        for pl, skew_in, skew_out in placements:
            expect = case.expect["S" if pl.startswith("S") else pl]
            arena.reset(fill)
            with _placed(ops, arena, monkeypatch, skew_out) as (rec, mp):
                t = Ctx(ops, arena, rec, skew_in, skew_out, cache, pl, ops.get_math_mode(), mp)
                if expect != "compute":
                    with pytest.raises(ScatError, match=rf"failed \({CODES[expect]}\)"):
                        case.fn(t)
                    torch.cuda.synchronize()
                    damaged = [e for e in arena.problems() if e.startswith("guard")]
                    assert not damaged, f"{case.name} [{pl}] rejected, yet: {damaged}"
                    continue
                case.fn(t)
                torch.cuda.synchronize()
                if pl == "A":
                    missing = set(case.syms) - rec.called
                    assert not missing, f"{case.name}: never called {sorted(missing)} (called: {sorted(rec.called)})"
                    for sym in case.syms:
                        if sym in WS:
                            seen = sorted(set(rec.ws.get(sym, [])))
                            print(f"{case.name} [{pl}] {sym}: (ws_bytes, queried) {seen}")
                            assert any(q > 0 and b == q for b, q in seen), \
                                f"{case.name}: {sym} never ran with a workspace of exactly its non-zero queried size: {seen}"
                res = {}
                for name, got, ref, gate in t.outs:
                    gate = case.gate if gate is None else gate
                    err = _compare(name, got, ref, gate)
                    print(f"{case.name} [{pl}] {name}: rel-err {err:.2e} (gate {gate:g})")
                    assert err < gate or err == 0.0, f"{case.name} [{pl}] {name}: {err:.3e} against fp64, gate {gate:g}"
                    res[name] = (got.detach().cpu().clone(), gate)
                arena.check()
                results[pl] = res
        for pl, res in results.items():
            if pl == "A":
                continue
            for name, (got, gate) in res.items():
                a = results["A"][name][0]
                err = 0.0 if torch.equal(got, a) else (float("inf") if gate == 0.0 else rel_err(got, a))
                assert err < gate or err == 0.0, f"{case.name}: placement {pl} disagrees with A on {name}: {err:.3e}"
    finally:
        ops.set_math_mode(saved_mode)
