#!/usr/bin/env python
"""A SHA-256 of every output tensor of every fit entry point, through scat_amd.fit, on the inputs of tests/_fit*_cases.py:
the bits that a change to the fit kernels which is to compute the same thing must keep.  Run it once with the library to
compare against (SCAT_LIBPATH) and once with this tree's, each in its own process, and diff the two outputs
(profiles/fit_family_refactor.txt is such a pair).

The smallest shapes: V = 37, and 778 once per entry point; 6 hands for the joints, keypoint and mesh fits, 2 sequences of 5
frames (joints, keypoints, meshes and clouds; at V = 37 also of 1 and of 2 frames, the block-tridiagonal walk's smallest), a
cloud of (3, 257, 37); 6 hands in 3 calibrated views and 2 tracks of 5 frames in 3 views (at V = 37 also of 1 and of 2
frames), which a library from before that entry point reports as absent.  5 iterations; the closed-form start and the caller's; one run with a frozen group and one with some
zero weights.  The plane metric (the mesh fit at three tau, the normals, the assignment, the loop) and the tracks of meshes
and clouds (a frame without weight, a frame in which nothing matches) come last per V."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ITERS = 5


def main():
    import _fit_kp_cases as KC
    import _fit_plane_cases as LC
    import _fit_points_cases as PC
    import _fit_seq_cases as SC
    import _fit_seq_kp_cases as QC
    import _fit_seq_verts_cases as GC
    import _fit_seq_views_cases as XC
    import _fit_verts_cases as VC
    import _fit_views_cases as WC
    from _fit_cases import JOINT_MAP, host_model
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import (Cameras, ManoFitter, Topology, free_mask, mano_cloud_assign_plane, mano_fit_verts_metric, mano_joints_jac,
                              mano_verts_jac, mesh_normals)

    lib().scat_check_device()
    dev = torch.device("cuda", 0)

    def show(name, res):
        fields = res._asdict().items() if hasattr(res, "_asdict") else enumerate(res)
        for k, t in fields:
            t = t.detach().cpu().contiguous()
            print(f"{name}.{k} {t.dtype} {list(t.shape)} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}")

    frozen = free_mask(betas=False, log_scale=False)
    for V in (37, 778):
        fitter = ManoFitter(host_model(V).to(dev), joint_map=JOINT_MAP, iters=ITERS)
        P, Tj, Tv = VC.seeded(V)
        P, Tj, Tv = P.float().to(dev), Tj.float().to(dev), Tv.to(dev)
        near = KC.near_start(V)[:, :62].float().to(dev)       # 0.05 off the truth in the 58 model unknowns
        wj = torch.ones(6, 21, device=dev)
        wj[:, ::4] = 0.0
        wj[:, 1] = 0.5
        wv = torch.ones(6, V, device=dev)
        wv[:, ::3] = 0.0
        wv[:, 1::3] = 0.25

        show(f"v{V}.joints_jac", mano_joints_jac(fitter.model, P[:, 0:3], P[:, 3:48], P[:, 48:58]))
        show(f"v{V}.fit", fitter.fit(Tj))
        show(f"v{V}.fit.init", fitter.fit(Tj, init=near))
        show(f"v{V}.fit.frozen", fitter.fit(Tj, init=near, free=frozen))
        show(f"v{V}.fit.weights", fitter.fit(Tj, weights=wj))

        _, T3, T2 = KC.truth(V)
        T3, T2 = T3.to(dev), T2.to(dev)
        near65 = KC.near_start(V).float().to(dev)
        w2 = torch.full((6, 21), KC.W2, device=dev)
        show(f"v{V}.kp.3d", fitter.fit_keypoints(joints3d=T3, free_cam=0))
        show(f"v{V}.kp.both", fitter.fit_keypoints(joints3d=T3, joints2d=T2, w2=w2))
        show(f"v{V}.kp.both.init", fitter.fit_keypoints(joints3d=T3, joints2d=T2, w2=w2, init=near65, sigma3=0.01, sigma2=10.0))
        show(f"v{V}.kp.2d", fitter.fit_keypoints(joints2d=T2))
        show(f"v{V}.kp.frozen", fitter.fit_keypoints(joints3d=T3, joints2d=T2, w2=w2, init=near65, free=frozen))
        show(f"v{V}.kp.weights", fitter.fit_keypoints(joints3d=T3, joints2d=T2, w3=wj, w2=w2 * wj))

        Ps, X = SC.track(25, 2, 5, V)
        X = X.to(dev)
        off = 0.05 * torch.from_numpy(np.array(synth.normal_like(23, "seq.off", (2, 5, 58), 1.0))).float()
        near_s = Ps.float().clone()
        near_s[:, :, :58] += off
        near_s = near_s.to(dev)
        ws = torch.ones(2, 5, 21, device=dev)
        ws[:, 2] = 0.0                                           # a frame without data, bridged by its neighbours
        ws[:, :, 3] = 0.0
        show(f"v{V}.seq", fitter.fit_sequence(X, smooth=SC.SMOOTH))
        show(f"v{V}.seq.decoupled", fitter.fit_sequence(X))
        show(f"v{V}.seq.init", fitter.fit_sequence(X, smooth=SC.SMOOTH, init=near_s))
        show(f"v{V}.seq.frozen", fitter.fit_sequence(X, smooth=SC.SMOOTH, init=near_s, free=frozen))
        show(f"v{V}.seq.weights", fitter.fit_sequence(X, weights=ws, smooth=SC.SMOOTH))

        _, Q3, Q2 = QC.truth(25, 2, 5, V)                        # the same tracks under a camera per sequence
        Q3, Q2 = Q3.to(dev), Q2.to(dev)
        near_q = QC.near_start(25, 2, 5, V).float().to(dev)
        q2 = torch.full((2, 5, 21), QC.W2, device=dev)
        wide = torch.full((45,), QC.WIDE_BOX)                    # active on a few angles at near_q
        both = dict(joints3d=Q3, joints2d=Q2, w2=q2)
        seqkp = fitter.fit_keypoints_sequence
        show(f"v{V}.seqkp.both", seqkp(**both, smooth=QC.SMOOTH))
        show(f"v{V}.seqkp.2d", seqkp(joints2d=Q2, smooth=QC.SMOOTH))
        show(f"v{V}.seqkp.init", seqkp(**both, smooth=QC.SMOOTH, init=near_q, sigma3=0.01, sigma2=10.0))
        show(f"v{V}.seqkp.limits", seqkp(**both, smooth=QC.SMOOTH, init=near_q, limits=(-wide, wide), w_limit=QC.W_LIMIT))
        show(f"v{V}.seqkp.frozen", seqkp(**both, smooth=QC.SMOOTH, init=near_q, free=frozen, free_cam=0))
        show(f"v{V}.seqkp.weights", seqkp(joints3d=Q3, joints2d=Q2, w3=ws, w2=q2 * ws, smooth=QC.SMOOTH))
        show(f"v{V}.seqkp.decoupled", seqkp(**both))
        if V == 37:      # the walk's smallest shapes: T = 1 eliminates nothing, T = 2 has one M_t and no middle frame
            for T in (1, 2):
                show(f"v{V}.seq.t{T}", fitter.fit_sequence(SC.track(25, 2, T, V)[1].to(dev), smooth=SC.SMOOTH))
                _, R3, R2 = QC.truth(25, 2, T, V)
                show(f"v{V}.seqkp.t{T}", seqkp(joints3d=R3.to(dev), joints2d=R2.to(dev), w2=q2[:, :T].contiguous(), smooth=QC.SMOOTH))

        # keypoints in calibrated views: a rig per hand, the triangulated start and the caller's; then tracks of them
        def rig(c):
            c = c.to(dev)
            return Cameras(c[:, :, :9].reshape(c.shape[0], -1, 3, 3).contiguous(), c[:, :, 9:12].contiguous(), c[:, :, 12:16].contiguous())

        vf = ManoFitter(fitter.model, joint_map=JOINT_MAP, iters=ITERS, w_pose=1e-2, w_beta=1e-2)
        U2, ucams = WC.truth(V, 6, 3, True)[2].to(dev), rig(WC.truth(V, 6, 3, True)[3])
        near_w = WC.near_start(V, 6, 3, True).float().to(dev)
        box = torch.full((45,), WC.BOX)
        wu = torch.ones(6, 3, 21, device=dev)
        wu[:, 0, ::4] = 0.0
        wu[:, 1, 1] = 0.5
        show(f"v{V}.triangulate", vf.triangulate(U2, ucams, w2=wu))
        show(f"v{V}.views", vf.fit_keypoints_views(U2, ucams))
        show(f"v{V}.views.init", vf.fit_keypoints_views(U2, ucams, init=near_w, sigma2=WC.SIGMA2, limits=(-box, box), w_limit=WC.W_LIMIT))
        show(f"v{V}.views.frozen", vf.fit_keypoints_views(U2, ucams, init=near_w, free=frozen))
        show(f"v{V}.views.weights", vf.fit_keypoints_views(U2, ucams, w2=wu, sigma2=WC.SIGMA2))
        try:
            sm = dict(zip(("rots", "poses", "betas", "trans", "scale"), XC.SMOOTH))
            seqw = vf.fit_keypoints_views_sequence
            for T in (1, 2, 5) if V == 37 else (5,):
                Y2, ycams = XC.truth(V, 2, T, 3)[2].to(dev), rig(XC.truth(V, 2, T, 3)[3])
                show(f"v{V}.seqviews.t{T}", seqw(Y2, ycams, smooth=sm))
            near_y = XC.near_start(V, 2, 5, 3).float().to(dev)
            wy = torch.ones(2, 5, 3, 21, device=dev)
            wy[:, 2, 1:] = 0.0                                       # a frame that one camera sees
            wy[0, 3] = 0.0                                           # and one that none sees
            show(f"v{V}.seqviews.init", seqw(Y2, ycams, smooth=sm, init=near_y, sigma2=XC.SIGMA2, limits=(-box, box), w_limit=XC.W_LIMIT))
            show(f"v{V}.seqviews.frozen", seqw(Y2, ycams, smooth=sm, init=near_y, free=frozen))
            show(f"v{V}.seqviews.weights", seqw(Y2, ycams, w2=wy, smooth=sm, sigma2=XC.SIGMA2))
            show(f"v{V}.seqviews.decoupled", seqw(Y2, ycams))
        except AttributeError as e:      # a library from before scat_mano_fit_seq_views
            print(f"v{V}.seqviews absent: {str(e).split(', which')[0].split('/')[-1]}")

        show(f"v{V}.verts_jac", mano_verts_jac(fitter.model, P[:, 0:3], P[:, 3:48], P[:, 48:58]))
        show(f"v{V}.verts", fitter.fit_vertices(Tv))
        show(f"v{V}.verts.init", fitter.fit_vertices(Tv, init=near))
        show(f"v{V}.verts.frozen", fitter.fit_vertices(Tv, init=near, free=frozen))
        show(f"v{V}.verts.weights", fitter.fit_vertices(Tv, weights=wv))

        if V == 37:      # the random cloud of the assignment tests; for the model's forms 257 points 3 mm off the hands' meshes
            verts, cloud, weights, cloud_dist, _ = PC.assign_case(3, 257, 37, True)
            verts, cloud, weights = (torch.from_numpy(np.array(t)).to(dev) for t in (verts, cloud, weights))
            noise = torch.from_numpy(np.array(synth.normal_like(29, "bits.noise", (3, 257, 3), 0.003))).float().to(dev)
            points = (Tv[:3, torch.arange(257, device=dev) * 7 % V] + noise).contiguous()
            max_dist, start = 0.02, near[:3].contiguous()      # the start is centimetres off: both sides of the trim are taken
        else:            # the hands' own meshes as unordered clouds
            points, weights, max_dist, start = torch.from_numpy(np.array(PC.cloud(V, "shuffled"))).to(dev), None, PC.TRIM, near
            verts, cloud, cloud_dist = Tv, points, max_dist
        show(f"v{V}.nearest.verts", fitter.nearest_vertices(verts, cloud, weights, cloud_dist))
        show(f"v{V}.nearest.p", fitter.nearest_vertices(start, points, weights, max_dist))
        show(f"v{V}.points", fitter.fit_points(points, start, rounds=3, iters=ITERS))
        show(f"v{V}.points.trim", fitter.fit_points(points, start, weights=weights, rounds=3, iters=ITERS, max_dist=max_dist))
        show(f"v{V}.points.frozen", fitter.fit_points(points, start, weights=weights, rounds=2, iters=ITERS, free=frozen))

        # the plane metric: the mesh fit on _fit_plane_cases.metric_case, then the cloud above against topology(V)
        Mv, mw, mn, M1 = (t.float().to(dev) for t in LC.metric_case(V))
        for tau in LC.TAUS:
            mp = M1.clone()
            show(f"v{V}.metric.tau{tau:g}", (mp, *mano_fit_verts_metric(fitter.model, Mv, mw, mn, mp, ITERS, tau, fitter.lambda0,
                                                                        fitter.w_pose, fitter.w_beta)))
        faces = LC.topology(V)[0]
        topo = Topology(*(torch.from_numpy(np.array(a)).to(dev) for a in LC.topology(V)))
        show(f"v{V}.normals", (mesh_normals(Tv, topo),))
        ca, cn, cm = mano_cloud_assign_plane(fitter.model, start, points, weights, topo, max_dist, LC.TAU, want_model_pts=True)
        show(f"v{V}.assign_plane", ca)
        show(f"v{V}.assign_plane.more", (cn, cm))
        show(f"v{V}.plane", fitter.fit_points_plane(points, start, faces, rounds=3, iters=ITERS))
        show(f"v{V}.plane.trim", fitter.fit_points_plane(points, start, faces, weights=weights, rounds=3, iters=ITERS, max_dist=max_dist))
        show(f"v{V}.plane.frozen", fitter.fit_points_plane(points, start, faces, weights=weights, rounds=2, iters=ITERS, free=frozen))

        # tracks of meshes: _fit_seq_verts_cases.track at S 2 T 5, a start 0.05 off, a frame without weight
        Pv, Xv = GC.track(25, 2, 5, V)
        Xv, near_v = Xv.to(dev), GC.off_start(Pv, 23).float().to(dev)
        wx = torch.ones(2, 5, V, device=dev)
        wx[:, 2] = 0.0
        wx[:, :, ::3] = 0.0
        seqv = fitter.fit_vertices_sequence
        show(f"v{V}.seqv", seqv(Xv, smooth=GC.SMOOTH))
        show(f"v{V}.seqv.init", seqv(Xv, smooth=GC.SMOOTH, init=near_v))
        show(f"v{V}.seqv.frozen", seqv(Xv, smooth=GC.SMOOTH, init=near_v, free=frozen))
        show(f"v{V}.seqv.weights", seqv(Xv, weights=wx, smooth=GC.SMOOTH))
        if V == 37:
            for T in (1, 2):
                show(f"v{V}.seqv.t{T}", seqv(GC.track(25, 2, T, V)[1].to(dev), smooth=GC.SMOOTH))
        # tracks of clouds: 257 points 3 mm off the meshes' vertices; in the last, frame 2 of sequence 0 sits 1 m away
        sn = torch.from_numpy(np.array(synth.normal_like(31, "bits.seq.noise", (2, 5, 257, 3), 0.003))).float().to(dev)
        cloud_s = (Xv[:, :, torch.arange(257, device=dev) * 7 % V] + sn).contiguous()
        gap = cloud_s.clone()
        gap[0, 2] += 1.0
        seqp = fitter.fit_points_sequence
        show(f"v{V}.seqp", seqp(cloud_s, near_v, smooth=GC.ICP_SMOOTH, rounds=2, iters=ITERS))
        show(f"v{V}.seqp.plane", seqp(cloud_s, near_v, faces=faces, smooth=GC.ICP_SMOOTH, rounds=2, iters=ITERS))
        show(f"v{V}.seqp.gap", seqp(gap, near_v, faces=faces, smooth=GC.ICP_SMOOTH, rounds=2, iters=ITERS, max_dist=GC.ICP_TRIM))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
