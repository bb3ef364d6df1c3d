"""CPU-only completeness check of the batch-96 HRNet table in tests/test_gpu_ops.py (HRNET_B96): the convolution
geometries the oracle's HRNet-W32 wrapper (oracle/scat_oracle.py encoder_transformer_hrnet_forward: the backbone and the
wrapper's reduction) runs at 224 x 224 are recorded from F.conv2d, and every one of them must be in the table — or, for
layer1's Bottlenecks, which run on ResNet's block executor, in CONVS — with nothing in the table that HRNet-W32 does not
run.  A change of the network that adds a geometry then fails here instead of going untested at batch 96."""
import torch
import torch.nn.functional as F

from oracle import scat_oracle as O
from scat_amd import synth


def test_hrnet_b96_table_is_every_hrnet_w32_conv_geometry(monkeypatch):
    from scat_amd.models import hrnet as H
    from test_gpu_ops import CONVS, HRNET_B96

    net = H.HRNet(c=32, nof_joints=128, bn_momentum=0.1)
    sd = {"main_encoder." + k: v for k, v in synth.to_torch(synth.fill_state(7, net.state_dict())).items()}
    sd.update(synth.to_torch(synth.vit_state(8, "transformer.")))
    sd["conv1x1_channel_reduction.weight"] = torch.randn(128, 512, 3, 3) * 0.01
    sd["positionalEncoding.pe"] = torch.from_numpy(synth.positional_encoding(196, 128)).view(1, 128, 196)
    sd["mask_token"] = torch.randn(1, 1, 196)
    sd["regressor.0.weight"] = torch.randn(61, 196 + 61) * 0.01
    sd["regressor.0.bias"] = torch.zeros(61)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    names = {id(v): k for k, v in sd.items()}
    seen = {}
    conv2d = F.conv2d

    def recording(x, w, bias=None, stride=1, padding=0, *a, **kw):
        s = stride if isinstance(stride, int) else stride[0]
        p = padding if isinstance(padding, int) else padding[0]
        assert x.shape[2] == x.shape[3]
        seen.setdefault((w.shape[1], w.shape[0], w.shape[2], s, p, x.shape[2]), set()).add(names[id(w)])
        return conv2d(x, w, bias, stride, padding, *a, **kw)

    monkeypatch.setattr(F, "conv2d", recording)
    with torch.no_grad():
        pred = O.encoder_transformer_hrnet_forward(sd, torch.zeros(1, 61, dtype=torch.float64),
                                                   torch.randn(1, 3, 224, 224, dtype=torch.float64), masked=[])
    assert tuple(pred.shape) == (1, 61)
    assert sum(len(v) for v in seen.values()) == 293 + 1          # HRNet-W32's convolutions + the wrapper's reduction

    table = {(cin, cout, k, s, k // 2, H) for cin, cout, k, s, H in HRNET_B96}
    layer1 = {geo for geo, keys in seen.items() if all(k.startswith("main_encoder.layer1.") for k in keys)}
    assert layer1 and layer1 <= set(CONVS), layer1 - set(CONVS)
    assert set(seen) - layer1 == table, (sorted(set(seen) - layer1 - table), sorted(table - set(seen)))
    # the roles: a geometry that some strided chain, transition or block runs is run that way in the table
    for (cin, cout, k, s, p, H), keys in seen.items():
        if (cin, cout, k, s, p, H) in layer1:
            continue
        roles = HRNET_B96[(cin, cout, k, s, H)]
        blocks = {key for key in keys if ".branches." in key}
        assert bool(blocks) == ("block" in roles), (keys, roles)
        assert any(key.endswith("final_layer.weight") for key in keys) == ("bias" in roles), (keys, roles)
