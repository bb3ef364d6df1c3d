// init = 1 of scat_mano_fit_seq_views (include_ext/scat_mano_fit_seq_views.h): every frame's own closed-form start, which
// is mano_fit_views.hip's (views_start of mano_fit_views_common.h: triangulation, then Procrustes), one workgroup per frame,
// into the first buffer of the sequence's unknowns in the workspace, and the flag "this frame has a start" into the
// frame's L_t slot.  The walk (mano_fit_seq_views.hip), launched after it on the same stream, ties the frames.
#include "mano_fit_seq_views.h"

namespace scat {

struct SeqViewsStartLds {
    float cam[kVMaxC][kVCam];
    float tgt[kVMaxC][kKRows2], w[kVMaxC][kFJoints];
    float h[kFRows], rho[kFJoints];
    float p[kFU];
    int few;
};

// init = 1, grid = S T, block = 256, launched before mano_fit_seq_views_kernel on the same stream.  A frame with fewer
// than three triangulated joints, or with an input that is not usable (its sequence is then not fitted at all), keeps
// zeros and the flag 0.  The frames are independent here; the scan that ties them is the main kernel's.
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_views_start_kernel(SeqViewsArgs a) {
    __shared__ JacLds m;
    __shared__ SeqViewsStartLds f;
    const int tid = threadIdx.x, T = a.T, C = a.C, t = blockIdx.x % T;
    const int64_t s = blockIdx.x / T, fr = s * T + t;
    const float* cams = a.cams + s * a.cam_stride;
    const float* tgt = a.targets2 + fr * C * kKRows2;
    const float* wts = a.weights2 ? a.weights2 + fr * C * kFJoints : nullptr;
    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
    } else if (tid >= 64 && tid < 64 + kFU) {
        f.p[tid - 64] = 0.f;
    }
    for (int i = tid; i < C * kVCam; i += kFThreads) f.cam[0][i] = cams[i];
    for (int i = tid; i < C * kKRows2; i += kFThreads) f.tgt[i / kKRows2][i % kKRows2] = tgt[i];
    for (int i = tid; i < C * kFJoints; i += kFThreads) f.w[i / kFJoints][i % kFJoints] = wts ? wts[i] : 1.f;
    if (tid == 0) f.few = 1;
    if (!__syncthreads_or(views_unusable(cams, tgt, wts, C, kFThreads))) {   // the same for every thread of the workgroup
        ManoArgs pc = a.m;
        pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
        jac_eval(m, pc, 0, false, 1.f, nullptr, 0);   // the zero pose
        views_start(m, f, C, a.z_near, f.p, &f.few);
    }
    if (tid < kFU) seq_ws_start<kFU>(a.ws, s, T, t)[tid] = f.p[tid];
    if (tid == 0) *seq_views_flag(a.ws, s, T, t) = f.few ? 0.f : 1.f;
}

void seq_views_launch_start(const SeqViewsArgs& a, int S, hipStream_t stream) {
    hipLaunchKernelGGL(mano_fit_seq_views_start_kernel, dim3((unsigned)(S * a.T)), dim3(kFThreads), 0, stream, a);
}

}  // namespace scat
