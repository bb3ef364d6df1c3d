"""fp64 torch restatement of rot_pose_beta_to_mesh (models/mano.py:280-391, semantics in include/scat_mano.h) with the
model's arrays as arguments; gradients come from autograd.  Test-only: imports neither scat_amd's kernels nor oracle/
(scat_amd.synth only, for the golden's seeded inputs).

Rodrigues is R = I + a S(r) + b S(r)^2 with a = sin(theta)/theta, b = 2 sin^2(theta/2)/theta^2, and below
theta^2 = 1e-8 the series in theta^2 (a = 1 - t/6 + t^2/120, b = 1/2 - t/24 + t^2/720; the next terms are below 1e-27):
value and gradient are exact to rounding at and near zero, where the reference's autograd gives NaN."""
import numpy as np
import torch

SERIES_T = 1e-8
MIN_ANGLE = 0.05      # the golden's angles are at least this: below it the reference's fp32 gradient is noise, eps / theta


def golden_inputs(seed, batch):
    """the inputs of tests/golden/mano.npz (tools/gen_mano_golden.py stores them; tests check the stored copy against this)"""
    from scat_amd import synth

    return (synth.normal_like(seed, "mano.golden.rots", (batch, 3), 0.8),
            synth.normal_like(seed, "mano.golden.poses", (batch, 45), 0.4),
            synth.normal_like(seed, "mano.golden.betas", (batch, 10), 1.0))


def golden_dout(seed, batch, V):
    """the cotangent of the golden's gradients: not stored, regenerated from the golden's seed"""
    from scat_amd import synth

    return synth.normal_like(seed, "mano.golden.dout", (batch, 21 + V, 3), 1.0)


def rodrigues(r):
    """r [N,3] fp64 -> R [N,3,3]"""
    t = (r * r).sum(-1)
    small = t < SERIES_T
    ts = torch.where(small, torch.ones_like(t), t)      # keeps the unused branch (and its gradient) finite
    th = ts.sqrt()
    a = torch.where(small, 1.0 - t / 6.0 + t * t / 120.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t / 24.0 + t * t / 720.0, 2.0 * torch.sin(0.5 * th) ** 2 / ts)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    o = torch.zeros_like(x)
    S = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=r.dtype).unsqueeze(0)
    S2 = r.unsqueeze(2) * r.unsqueeze(1) - t.reshape(-1, 1, 1) * eye
    return eye + a.reshape(-1, 1, 1) * S + b.reshape(-1, 1, 1) * S2


def _t64(a):
    return a.double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def forward(model, rots, poses, betas):
    """model: an object with v_template[V,3], shapedirs[V,3,10], posedirs[V,3,135], J_regressor[16,V], weights[V,16],
    hands_mean[45], parents[16], tips[5] (numpy); rots [B,3], poses [B,45], betas [B,10] fp64 tensors (may require grad)
    -> [B, 21 + V, 3] fp64"""
    vt, sd, pd = _t64(model.v_template), _t64(model.shapedirs), _t64(model.posedirs)
    Jr, W, hm = _t64(model.J_regressor), _t64(model.weights), _t64(model.hands_mean)
    parents, tips = list(model.parents), list(model.tips)
    B, V = rots.shape[0], vt.shape[0]
    pose = torch.cat([torch.zeros(B, 1, 3, dtype=torch.float64), (hm.reshape(1, 45) + poses).reshape(B, 15, 3)], dim=1)
    R = rodrigues(pose.reshape(-1, 3)).reshape(B, 16, 3, 3)
    v_shaped = vt.unsqueeze(0) + torch.einsum("vck,bk->bvc", sd, betas)
    J = torch.einsum("jv,bvc->bjc", Jr, v_shaped)
    pw = (R[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(B, 135)
    v_posed = v_shaped + torch.einsum("vck,bk->bvc", pd, pw)
    RG, t = [R[:, 0]], [J[:, 0]]
    for i in range(1, 16):
        p = parents[i]
        RG.append(RG[p] @ R[:, i])
        t.append((RG[p] @ (J[:, i] - J[:, p]).unsqueeze(2)).squeeze(2) + t[p])
    RG, t = torch.stack(RG, 1), torch.stack(t, 1)                          # [B,16,3,3], [B,16,3]
    a = t - (RG @ J.unsqueeze(3)).squeeze(3)
    TR = torch.einsum("vi,birc->bvrc", W, RG)
    Ta = torch.einsum("vi,bir->bvr", W, a)
    v = (TR @ v_posed.unsqueeze(3)).squeeze(3) + Ta                        # [B,V,3]
    joints = torch.cat([t, v[:, tips]], dim=1)                             # [B,21,3]
    Rg = rodrigues(rots)
    x = torch.cat([joints, v], dim=1) @ Rg.transpose(1, 2)
    return x - x[:, 1:2]


def forward_backward(model, rots, poses, betas, dout):
    """numpy in, numpy out (fp64): out, drots, dposes, dbetas for the cotangent dout"""
    r, p, b = (torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True) for a in (rots, poses, betas))
    out = forward(model, r, p, b)
    out.backward(torch.from_numpy(np.asarray(dout, dtype=np.float64)))
    return out.detach().numpy(), r.grad.numpy(), p.grad.numpy(), b.grad.numpy()


def rel(a, b):
    """max |a - b| / max |b|: the normalisation of every gate of the MANO tests"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())
