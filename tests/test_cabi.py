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
                                                "scat_set_math_mode",
                                                # host-side state of the NEXT launch of this thread, no device work
                                                "scat_epilogue_stats_arm", "scat_epilogue_stats_arm_shift", "scat_epilogue_stats_groups",
                                                "scat_epilogue_bnb_arm", "scat_epilogue_bnb_groups"):
            assert args[-1][1] == "stream", name
    # every prototype cites the reference file it replaces somewhere in the header
    src = open(os.path.join(ROOT, "include", "scat_hip.h")).read()
    assert len(re.findall(r"models/\w+\.py:\d+|train\.py:\d+|hand_net\.py:\d+", src)) >= 12


def test_library_exports_every_symbol(built):
    from scat_amd._lib import lib, parse_header

    L = lib()
    for name in parse_header():
        assert hasattr(L.cdll, name), name
        assert "streamk" not in name, name
    for name in ("scat_streamk_bytes", "scat_streamk_arm", "scat_streamk_error"):
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
