// init = 1 of scat_mano_fit_seq_kp (include/scat_mano_fit_seq_kp.h): every frame's own closed-form start, which is
// mano_fit_kp.hip's (kp_start of mano_fit_kp_common.h), one workgroup per frame, into the first buffer of the sequence's
// unknowns in the workspace.  The walk (mano_fit_seq_kp.hip), launched after it on the same stream, ties the frames.
#include "mano_fit_seq_kp.h"

namespace scat {

struct SeqKpStartLds {
    float tgt3[kFRows], tgt2[kKRows2], w3[kFJoints], w2[kFJoints];
    float p[kKU];
    int skip;
};

// init = 1, grid = S T, block = 256, launched before mano_fit_seq_kp_kernel on the same stream: mano_fit_kp.hip's
// closed-form start of frame t of sequence s into the first buffer of the sequence's unknowns in the workspace.  A frame
// without weight, or with an input that is not usable (its sequence is then not fitted at all), keeps zeros and the
// camera (1, 0, 0).  The frames are independent here; the scan that ties them is the main kernel's.
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_kp_start_kernel(SeqKpArgs a) {
    __shared__ JacLds m;
    __shared__ SeqKpStartLds f;
    const int tid = threadIdx.x, T = a.T, t = blockIdx.x % T;
    const int64_t s = blockIdx.x / T;
    const bool has3 = a.targets3 != nullptr, has2 = a.targets2 != nullptr;
    const int64_t fr = s * T + t;
    float* const q = seq_ws_start<kKU>(a.ws, s, T, t);
    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
        f.w3[tid] = has3 ? (a.weights3 ? a.weights3[fr * kFJoints + tid] : 1.f) : 0.f;
        f.w2[tid] = has2 ? (a.weights2 ? a.weights2[fr * kFJoints + tid] : 1.f) : 0.f;
    } else if (tid >= 64 && tid < 64 + kFRows) {
        f.tgt3[tid - 64] = has3 ? a.targets3[fr * kFRows + (tid - 64)] : 0.f;
    } else if (tid >= 128 && tid < 128 + kKU) {
        f.p[tid - 128] = tid - 128 == kKCam ? 1.f : 0.f;
    } else if (tid >= 193 && tid < 193 + kKRows2) {
        f.tgt2[tid - 193] = has2 ? a.targets2[fr * kKRows2 + (tid - 193)] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        int bad = 0;
        float W = 0.f;
        for (int i = 0; i < kFRows; ++i) bad |= !fit_finite(f.tgt3[i]);
        for (int i = 0; i < kKRows2; ++i) bad |= !fit_finite(f.tgt2[i]);
        for (int j = 0; j < kFJoints; ++j) {
            bad |= !(fit_finite(f.w3[j]) && f.w3[j] >= 0.f) || !(fit_finite(f.w2[j]) && f.w2[j] >= 0.f);
            W += f.w3[j];
        }
        for (int j = 0; j < kFJoints; ++j) W += f.w2[j];
        f.skip = bad || !(W > 0.f);
    }
    __syncthreads();
    if (!f.skip) {   // the same for every thread of the workgroup
        ManoArgs pc = a.m;
        pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
        jac_eval(m, pc, 0, false, 1.f, nullptr, 0);   // the zero pose: p's first 58 are zeros
        if (tid == 0) kp_start(m.x, f, a, f.p, has3, has2);
        __syncthreads();
    }
    if (tid < kKU) q[tid] = f.p[tid];
}

void seq_kp_launch_start(const SeqKpArgs& a, int S, hipStream_t stream) {
    hipLaunchKernelGGL(mano_fit_seq_kp_start_kernel, dim3((unsigned)(S * a.T)), dim3(kFThreads), 0, stream, a);
}

}  // namespace scat
