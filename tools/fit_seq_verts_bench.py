#!/usr/bin/env python
"""The on-device MANO fit to a track of point clouds against the kernels it is built from, V = 778, N = 2048 points on the
faces, point-to-plane, rounds x iters from a start 0.03 off the truth in every model unknown and 3 mm off in trans: device
events after warm-up, medians over alternated repeats, all columns in the same process.

  track       ManoFitter.fit_points_sequence: rounds x (1 + 2 iters + 2) + 1 launches
  (a) frames  ManoFitter.fit_points_plane on the same S T frames flattened, every frame on its own: 2 rounds + 1 launches
  (b) joints  ManoFitter.fit_sequence on the same tracks' 21 joints, rounds x iters iterations in its one launch: the
              measure of the walk along the frames inside one workgroup
  assign      scat_mano_cloud_assign_plane alone over the S T frames: a round's first launch
  solve       scat_mano_fit_seq_verts alone (plane metric, `iters` iterations, on the ordered meshes with their normals): the
              rest of a round, iters + 1 frame launches and iters + 1 track launches
  solve x2    the same with 2 iters iterations: (solve x2 - solve) / iters is one {track, frame} pair

The split of a solve between its two kernels needs the kernels' own durations: --profile S T runs the track ICP alone, to
be started under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/fit_seq_verts_bench.py --profile 1 256),
whose per-kernel table has the frame kernel (grid S T), the track kernel (grid S) and the assignment.  What would mean that
the split failed is the frame kernel's time growing with T at S = 1: compare the rows of --profile 1 16 and --profile 1 256.

The model is tests/_fit_plane_cases.smooth_model, as in tools/fit_plane_bench.py; the tracks are linear in the unknowns
(tests/_fit_seq_cases.track's velocities); meshes and clouds are made on the device.  --out also writes the table to a file
(profiles/fit_seq_verts_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SMOOTH = dict(rots=1e-2, poses=1e-2, betas=10.0, trans=3.0, scale=100.0)      # tests/_fit_seq_verts_cases.Q_SMOOTH
SMOOTH_JOINTS = dict(rots=1e-4, poses=1e-4, betas=1e-2, trans=1e-1, scale=1e-1)


def timed(cases, repeats, inner, warmup):
    """-> {name: sorted ms per call}: windows of `inner` calls between two events, the cases alternated in every repeat"""
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(repeats):
        for name, fn in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    return {k: sorted(v) for k, v in times.items()}


def inputs(fitter, faces_d, S, T, N, dev, seed):
    """-> the true P [S,T,62], the true meshes [S,T,V,3], their joints [S,T,21,3], clouds [S,T,N,3] on the faces, a start"""
    from scat_amd import synth
    from scat_amd.fit import SequenceFitResult, _groups

    base = np.concatenate([synth.normal_like(seed, n, (S, k), s) for n, k, s in
                           (("rots", 3, 0.8), ("poses", 45, 0.25), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.1))], axis=1)
    vel = np.zeros((S, 62))
    vel[:, 0:3] = synth.normal_like(seed, "vel.rots", (S, 3), 0.04)
    vel[:, 3:48] = synth.normal_like(seed, "vel.poses", (S, 45), 0.02)
    vel[:, 58:61] = synth.normal_like(seed, "vel.trans", (S, 3), 0.003)
    t = np.arange(T) - 0.5 * (T - 1)
    P = T_((base[:, None, :] + t[None, :, None] * vel[:, None, :]).astype(np.float32)).to(dev)
    res = SequenceFitResult(*_groups(P), None, None, P)
    joints, mesh = fitter.joints(res), fitter.mesh(res)
    g = torch.Generator(device=dev).manual_seed(seed)
    f = faces_d[torch.randint(0, faces_d.shape[0], (S, T, N), device=dev, generator=g)]      # [S,T,N,3]
    u = torch.rand((S, T, N, 2), device=dev, generator=g)
    u = torch.where((u.sum(-1) > 1.0).unsqueeze(-1), 1.0 - u, u)
    bary = torch.cat([1.0 - u.sum(-1, keepdim=True), u], -1)
    corners = torch.gather(mesh.unsqueeze(2).expand(S, T, 3, -1, 3), 3,
                           f.permute(0, 1, 3, 2).unsqueeze(-1).expand(S, T, 3, N, 3))      # [S,T,3,N,3]
    pts = (bary.permute(0, 1, 3, 2).unsqueeze(-1) * corners).sum(2).contiguous()
    P0 = P.clone()
    P0[..., :58] += 0.03 * torch.randn((S, T, 58), device=dev, generator=g)
    P0[..., 58:61] += 0.003 * torch.randn((S, T, 3), device=dev, generator=g)
    return P, mesh.contiguous(), joints.contiguous(), pts, P0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 16, 96, 16, 1024, 16, 1, 256], help="S T pairs")
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", type=int, nargs=2, default=None, metavar=("S", "T"), help="run the track ICP alone, three times")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import _fit_plane_cases as G
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter, mano_cloud_assign_plane, mano_fit_seq_verts, mesh_normals

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = G.smooth_model().to(dev)
    fitter = ManoFitter(model)
    faces = G.topology(778)[0]
    topo = fitter._topology("fit_seq_verts_bench", faces, dev)
    faces_d = topo.faces.long()
    N, sm5 = a.points, tuple(SMOOTH[k] for k in ("rots", "poses", "betas", "trans", "scale"))
    if a.profile:
        S, T = a.profile
        _, _, _, pts, P0 = inputs(fitter, faces_d, S, T, N, dev, 700 + S + T)
        for _ in range(3):
            fitter.fit_points_sequence(pts, P0, faces=faces, smooth=SMOOTH, rounds=a.rounds, iters=a.iters, w_tangent=a.tau)
        torch.cuda.synchronize()
        return
    lines = [f"V = {model.V}, F = {len(faces)}, N = {N} points on the faces, {a.rounds} rounds x {a.iters} LM iterations, w_tangent {a.tau}, "
             f"{a.warmup} warm-up calls of every case, cases alternated, repeats and calls per window as every row says (from 4096 "
             f"frames on: 3 repeats of 1 call); ms per call, device events around the window (host launch time included); "
             f"{torch.cuda.get_device_name(0)}"]
    for S, T in zip(a.sizes[::2], a.sizes[1::2]):
        P, mesh, joints, pts, P0 = inputs(fitter, faces_d, S, T, N, dev, 700 + S + T)
        B = S * T
        flat_pts, flat_P0 = pts.flatten(0, 1), P0.flatten(0, 1).contiguous()
        normals = mesh_normals(mesh.flatten(0, 1), topo).reshape(S, T, -1, 3)

        def solve(iters):
            p = P0.clone()
            mano_fit_seq_verts(model, mesh, None, normals, p, iters, 0, a.tau, fitter.lambda0, fitter.w_pose, fitter.w_beta, sm5)
            return p

        cases = [("track", lambda: fitter.fit_points_sequence(pts, P0, faces=faces, smooth=SMOOTH, rounds=a.rounds, iters=a.iters,
                                                              w_tangent=a.tau).p),
                 ("frames", lambda: fitter.fit_points_plane(flat_pts, flat_P0, faces, rounds=a.rounds, iters=a.iters, w_tangent=a.tau).p),
                 ("joints", lambda: fitter.fit_sequence(joints, smooth=SMOOTH_JOINTS, init=P0, iters=a.rounds * a.iters).p),
                 ("assign", lambda: mano_cloud_assign_plane(model, flat_P0, flat_pts, None, topo, float("inf"), a.tau)[0].idx),
                 ("solve", lambda: solve(a.iters)), ("solve x2", lambda: solve(2 * a.iters))]
        repeats, inner = (3, 1) if B >= 4096 else (a.repeats, a.inner)      # a call of 16384 frames takes seconds
        times = timed(cases, repeats, inner, a.warmup)
        from scat_amd.fit import SequenceFitResult, _groups

        def vrms(p):
            m = fitter.mesh(SequenceFitResult(*_groups(p), None, None, p))
            return float(((m - mesh) ** 2).sum(-1).mean(-1).sqrt().median()) * 1e3

        def accel(p):
            if T < 3:
                return float("nan")
            e = fitter.mesh(SequenceFitResult(*_groups(p), None, None, p)) - mesh
            return float((e[:, :-2] - 2 * e[:, 1:-1] + e[:, 2:]).norm(dim=-1).mean()) * 1e3

        tr, fr = cases[0][1](), cases[1][1]().reshape(S, T, 62)
        lines.append(f"S = {S}, T = {T} ({B} frames), {repeats} repeats, windows of {inner} calls: median vertex RMS / mean acceleration error against the true meshes in mm: start "
                     f"{vrms(P0):.3f} / {accel(P0):.3f}; track {vrms(tr):.3f} / {accel(tr):.3f}; frames {vrms(fr):.3f} / {accel(fr):.3f}")
        med = {}
        for name, _ in cases:
            t = times[name]
            med[name] = statistics.median(t)
            lines.append(f"  {name:9s} median {med[name]:11.4f} ms  min {t[0]:11.4f}  max {t[-1]:11.4f}")
        pair = (med["solve x2"] - med["solve"]) / a.iters
        lines.append(f"  a round: assign {med['assign']:.4f} ms + solve {med['solve']:.4f} ms; one {{track, frame}} pair "
                     f"{pair:.4f} ms; the cost of temporal coupling, track / frames: {med['track'] / med['frames']:.3f}; "
                     f"track / joints (the walk in one launch): {med['track'] / med['joints']:.3f}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
