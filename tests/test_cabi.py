"""CPU-side checks of the C ABI: the header parses, the library loads and exports every declared symbol
with the declared arity, error codes come back as exceptions.  No kernel is launched (no GPU here)."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/test_gpu_guard.py (the WS table), tests/_guard.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


# the per-thread request protocol that ScatEpilogue replaced: declared and exported nowhere
ARM_STATE = ("scat_epilogue_stats_arm", "scat_epilogue_stats_arm_shift", "scat_epilogue_stats_groups",
             "scat_epilogue_bnb_arm", "scat_epilogue_bnb_groups")


def test_header_declares_the_path():
    from scat_amd._lib import parse_header

    protos = parse_header()
    need = {"scat_conv2d_fwd", "scat_conv2d_dgrad", "scat_conv2d_dgrad_s2", "scat_conv2d_wgrad", "scat_gemm",
            "scat_bn_train_stats", "scat_bn_apply", "scat_bn_bwd", "scat_maxpool3x3s2_fwd", "scat_maxpool3x3s2_bwd",
            "scat_avgpool_fwd", "scat_layernorm_fwd", "scat_layernorm_bwd", "scat_attention_fwd", "scat_attention_bwd",
            "scat_gelu_fwd", "scat_tokens_fwd", "scat_regressor_fwd", "scat_regressor_bwd", "scat_loss_fwd_bwd",
            "scat_adam", "scat_last_error", "scat_version"}
    assert need <= set(protos), need - set(protos)
    # every data-path entry point is stream-ordered: last argument is the stream
    for name, (rt, args) in protos.items():
        if rt is ctypes.c_int and name not in ("scat_version", "scat_check_device", "scat_get_math_mode",
                                                "scat_set_math_mode"):
            assert args[-1][1] == "stream", name
    src = open(os.path.join(ROOT, "include", "scat_hip.h")).read()
    # an epilogue request travels with its call (ScatEpilogue): no entry point keeps one for the next launch
    for name in ARM_STATE:
        assert name not in protos and name not in src, name
    # every prototype cites the reference file it replaces somewhere in the header
    assert len(re.findall(r"models/\w+\.py:\d+|train\.py:\d+|hand_net\.py:\d+", src)) >= 12


def test_library_exports_every_symbol(built):
    from scat_amd._lib import lib, parse_header

    L = lib()
    for name in parse_header():
        assert hasattr(L.cdll, name), name
        assert "streamk" not in name, name
    for name in ("scat_streamk_bytes", "scat_streamk_arm", "scat_streamk_error") + ARM_STATE:
        assert not hasattr(L.cdll, name), name
    assert L.scat_version() >= 100
    assert isinstance(L.scat_last_kernel(), bytes)


def test_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call, so it is testable on CPU"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    with pytest.raises(ScatError, match="kernel 5x5 unsupported"):
        L.scat_conv2d_fwd(1, 1, 0, 1, 1, 3, 8, 8, 4, 5, 5, 1, 2, 0, 0, 0, 0)
    with pytest.raises(ScatError, match="null pointer"):
        L.scat_conv2d_fwd(0, 0, 0, 0, 1, 3, 8, 8, 4, 3, 3, 1, 1, 0, 0, 0, 0)
    with pytest.raises(ScatError, match="dim_head must be 64"):
        L.scat_attention_fwd(1, 1, 1, 2, 21, 8, 32, 0.1, 0)
    assert L.scat_conv2d_wgrad_ws(96, 64, 56, 56, 64, 3, 3, 1, 1) > 0
    assert L.scat_gemm_ws(2016, 1536, 784) >= 0


def test_wgrad_workspace_queries_are_pinned(built):
    """scat_conv2d_wgrad_ws / scat_conv1x1_wgrad_bnb_ws return, byte for byte, what tests/golden/wgrad_ws.json recorded
    before the query and the launch were given one plan (key: "<query>:<its arguments>"): every geometry of CONVS and
    HRNET_B96 at batch 96 and 8 and the shapes of the weight-gradient tests.  The queries launch nothing."""
    import json

    from scat_amd._lib import lib
    from test_gpu_ops import CONVS, HRNET_B96

    L = lib()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "wgrad_ws.json")))
    for B in (96, 8):
        for cin, cout, k, s, p, H in CONVS + [(cin, cout, k, s, k // 2, H) for cin, cout, k, s, H in HRNET_B96]:
            assert f"conv2d_wgrad_ws:{B},{cin},{H},{H},{cout},{k},{k},{s},{p}" in gold
            if k == 1 and s == 1:
                assert f"conv1x1_wgrad_bnb_ws:{B},{cin},{H * H},{cout}" in gold
    for key, want in gold.items():
        fn, args = key.split(":")
        assert getattr(L, "scat_" + fn)(*map(int, args.split(","))) == want, key


def test_product_has_no_cpu_fallback():
    import torch

    from scat_amd import ops
    from scat_amd._lib import ScatError

    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.conv2d_fwd(torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 3, 3), 1, 1)
    # and nothing under scat_amd imports the oracle
    for root, _, files in os.walk(os.path.join(ROOT, "scat_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f


def test_module_api_mirrors_reference():
    """class names / ctor signatures / state_dict keys of the drop-in"""
    import inspect

    from scat_amd.models import hand_net, resnet, vision_transformer, vit

    assert list(inspect.signature(hand_net.EncoderTransformer.__init__).parameters) == ["self", "opt", "mean_params"]
    assert list(inspect.signature(vision_transformer.Transformer.__init__).parameters) == \
        ["self", "dim", "depth", "heads", "dim_head", "mlp_dim", "dropout"]
    assert list(inspect.signature(vit.Transformer.__init__).parameters) == \
        ["self", "dim", "depth", "heads", "dim_head", "mlp_dim", "dropout"]
    net = resnet.resnet50(pretrained=True, num_classes=512)
    from scat_amd import synth

    ref = synth.resnet_state(1)
    sd = net.state_dict()
    assert set(sd) == set(ref) and all(tuple(sd[k].shape) == tuple(ref[k].shape) for k in ref)
    t = vision_transformer.Transformer(784, 3, 8, 64, 392)
    assert set(t.state_dict()) == set(synth.vt_state(1, ""))
    v = vit.Transformer(196, 3, 8, 64, 392, 0.0)
    assert set(v.state_dict()) == set(synth.vit_state(1, ""))


def test_synth_is_deterministic():
    import numpy as np

    from scat_amd import synth

    a = synth.normal_like(3, "w", (5, 7))
    b = synth.normal_like(3, "w", (5, 7))
    assert np.array_equal(a, b) and a.dtype == np.float32
    assert not np.array_equal(a, synth.normal_like(4, "w", (5, 7)))
    assert abs(float(synth.normal_like(1, "big", (200000,)).std()) - 1.0) < 0.01
    u = synth.uniform(1, "u", (100000,), 2.0, 3.0)
    assert u.min() >= 2.0 and u.max() < 3.0


def test_bench_roofline_lookup_matches_profiles():
    """bench.py prices its roofline kernel's HBM traffic from profiles/r*_traffic.json (rocprofv3 --pmc passes over the
    bench command): the kernel labels the library reports must map onto the instantiation names that file is keyed by,
    or `roofline.traffic` silently becomes null."""
    import importlib.util
    import json

    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    traffic, name = bench.latest_traffic()
    assert name is not None and traffic, "no profiles/r*_traffic.json"
    for label in ("conv1x1_split_128x128x32", "conv1x1_split_128x128x32_tf", "conv3x3_split_64x128x16",
                  "wgrad1x1_pw_128x256x32_split124", "wgrad1x1_pw_256x128x32_tf_split32", "wgrad1x1_pw_128x128x32_tf_bnb_split64",
                  "wgrad3x3_rows_64x576x16_tf_r1_split64", "wgrad3x3_s2_split_pc128x128x16_tf_split86",
                  "conv7x7_s2_split_64x128x32"):
        inst = bench.instantiation_of(label, traffic)
        assert inst in traffic, (label, inst, sorted(traffic)[:8])
        assert traffic[inst]["hbm_bytes_per_launch"] > 0


# ------------------------------------------------------------------ the workspace contract (tests/test_gpu_guard.py WS)
#
# Argument validation runs before any HIP call, so a call that is REFUSED never touches a device and the pointers can be
# made-up integers: those tests run everywhere.  A call that passes validation goes on to launch; that outcome (-4 where no
# device is visible, after the label was set) is only looked at where no device is visible — with one, the launch would
# run on the made-up pointers.

WS_PTR = 0x7000000      # 16-byte aligned, non-null, never dereferenced


def _ws_rows():
    import test_gpu_guard as G

    return [n for n, r in G.WS.items() if r.where == "tests/test_cabi.py"]


class _Entry:
    """one row's entry point, called with made-up pointers; the product mode the row asks for is set around each call"""

    def __init__(self, name):
        import test_gpu_guard as G
        from scat_amd._lib import lib

        self.G, self.L, self.name, self.row = G, lib(), name, G.WS[name]
        self.fn = getattr(self.L.cdll, name)        # the raw entry point: the code comes back, no exception

    def need(self, shape=None):
        args = self.G.ws_call_args(self.L, self.name, shape or self.row.shape, 0, 0)
        return self.G.ws_query(self.L, self.name, dict(zip([an for _, an in self.L.protos[self.name][1]], args)))

    def __call__(self, ws, ws_bytes, shape=None, null=()):
        """-> (code, scat_last_error(), label before, label after)"""
        saved = self.L.scat_get_math_mode()
        if self.row.math is not None:
            self.L.scat_set_math_mode(self.row.math)
        try:
            before = self.L.scat_last_kernel()
            rc = int(self.fn(*self.G.ws_call_args(self.L, self.name, shape or self.row.shape, ws, ws_bytes, null)))
            return rc, self.L.scat_last_error().decode(errors="replace"), before, self.L.scat_last_kernel()
        finally:
            self.L.scat_set_math_mode(saved)


def _no_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a device is visible: a call that passes validation would launch on the made-up pointers")


@pytest.mark.parametrize("name", _ws_rows())
def test_short_absent_and_misaligned_workspaces_are_refused_on_the_host(name, built):
    e = _Entry(name)
    row, need = e.row, e.need()
    assert need == row.nbytes > 0
    refused = []
    if row.short == "reject":
        refused += [("one byte short", WS_PTR, need - 1, -3), ("absent", 0, need, -3)]
    for off in (2, 4, 8):
        if off % row.align and row.misaligned != "single_pass":
            refused.append((f"ws % 16 == {off}", WS_PTR + off, need, CODES[row.misaligned]))
    if row.short == "reject":
        assert len(refused) >= 3
    for what, ws, nbytes, code in refused:
        rc, err, before, after = e(ws, nbytes)
        assert rc == code, f"{name}, workspace {what}: {rc} ({err}), expected {code}"
        assert name in err, (name, what, err)
        assert before == after, f"{name}, workspace {what}: refused, yet the kernel label moved to {after}"


CODES = {"SCAT_E_ARG": -2, "SCAT_E_WORKSPACE": -3}


@pytest.mark.parametrize("name", _ws_rows())
def test_sufficient_and_unused_workspaces_pass_validation(name, built):
    """the other side of every refusal above: the exact size, every aligned offset and, where the row says the workspace
    is unused, (0, 0) get as far as the launch"""
    _no_device()
    e = _Entry(name)
    row, need = e.row, e.need()
    launched = (lambda rc: rc >= 0) if name == "scat_wprep_jobs" else (lambda rc: rc == -4)     # (host only: no launch)
    for off in (0, 4, 8, 16):
        if off % row.align == 0:
            rc, err, _, _ = e(WS_PTR + off, need)
            assert launched(rc), f"{name}, ws % 16 == {off}, {need} bytes: {rc} ({err})"
    if row.shape2 is not None and row.nbytes2:
        rc, err, _, _ = e(WS_PTR, row.nbytes2, row.shape2)
        assert launched(rc), (name, rc, err)
        rc, err, _, _ = e(WS_PTR, row.nbytes2 - 1, row.shape2)
        assert rc == (-4 if row.short == "single_pass" else -3), (name, rc, err)
    if row.unused is not None:
        over = dict(row.unused)
        null = over.pop("null", ())
        shape = dict(row.shape, **over)
        assert over == {} or e.need(shape) == 0
        rc, err, _, _ = e(0, 0, shape, null)
        assert launched(rc), f"{name}: an unused workspace may be absent, yet {rc} ({err})"
    if row.short == "single_pass":
        # scat_gemm: no workspace, a short one or one that cannot hold floats -> one pass over K, the exact one -> the plan
        for ws, nbytes, want in ((0, 0, "_split1"), (WS_PTR, need - 1, "_split1"), (0, need, "_split1"),
                                 (WS_PTR + 2, need, "_split1"), (WS_PTR, need, "_split3")):
            rc, err, _, label = e(ws, nbytes)
            assert rc == -4 and label.decode().endswith(want), (ws, nbytes, rc, err, label)


# ------------------------------------------------------------------ the epilogue request (include/scat_hip.h ScatEpilogue)

EPI_ENTRIES = ("scat_conv1x1_s1", "scat_conv3x3_s1", "scat_conv2d_fwd_split", "scat_conv7x7_s2_fwd_split")


def test_epilogue_descriptor_mirror_has_the_librarys_size(built):
    from scat_amd import ops
    from scat_amd._lib import lib

    assert ctypes.sizeof(ops._Epilogue) == lib().scat_epilogue_bytes() == 56


@pytest.mark.parametrize("name", EPI_ENTRIES)
def test_a_refused_call_reports_zero_groups(name, built):
    """groups is written before the first check: a caller that reads it after a refusal never sees a stale count"""
    from scat_amd import ops
    from scat_amd._lib import HostInOut

    e = _Entry(name)
    assert [an for _, an in e.L.protos[name][1]][-2:] == ["epi", "stream"]
    # host memory, dereferenced before the first check: bound as its own type, which ws_call_args leaves null
    assert [an for ty, an in e.L.protos[name][1] if ty is HostInOut] == ["epi"]
    assert e.G.ws_call_args(e.L, name, e.row.shape, 0, 0)[-2:] == [0, 0]
    epi = ops._Epilogue(0x5000000, 1 << 20, 77)
    rc, err, before, after = e(WS_PTR, e.need() - 1, dict(e.row.shape, epi=ctypes.addressof(epi)))
    assert rc == -3 and name in err, (rc, err)
    assert epi.groups == 0
    assert before == after, f"{name}: refused, yet the kernel label moved to {after}"


def test_the_request_is_decided_by_its_own_call(built):
    """scat_conv1x1_s1 forward, 64 rows x 234 pixels on 64 x 128 tiles of two column groups each: 4 groups.  The capacity
    rule (rows * groups * 8 <= part_bytes, else not done) and the bias rule, as far as the launch (-4: no device)"""
    _no_device()
    from scat_amd import ops

    e = _Entry("scat_conv1x1_s1")
    shape = dict(B=2, C=128, HW=117, M=64)
    need = e.need(shape)
    saved = e.L.scat_get_math_mode()
    e.L.scat_set_math_mode(1)
    try:
        def groups(part_bytes, null):
            epi = ops._Epilogue(0x5000000, part_bytes, 77)
            rc, err, _, label = e(WS_PTR, need, dict(shape, epi=ctypes.addressof(epi)), null)
            assert rc == -4 and label.startswith(b"conv1x1_split_64x128x32"), (rc, err, label)
            return epi.groups
        g = groups(1 << 20, ("bias",))
        assert g == 4
        assert groups(64 * g * 8, ("bias",)) == g
        assert groups(64 * g * 8 - 1, ("bias",)) == 0
        assert groups(1 << 20, ()) == 0                     # a bias: the statistics would not be the convolution's
    finally:
        e.L.scat_set_math_mode(saved)
