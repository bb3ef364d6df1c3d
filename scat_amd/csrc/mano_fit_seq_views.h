// What the two launches of scat_mano_fit_seq_views share (mano_fit_seq_views.hip: the walk; mano_fit_seq_views_start.hip:
// the frames' triangulated starts): the kernels' arguments, and where a frame's start flag travels; the workspace's layout
// is mano_fit_seq_common.h's at 62 unknowns.  Two translation units for the reason mano_fit_seq_kp.h gives.
#pragma once
#include "mano_fit_views_common.h"
#include "mano_fit_seq_common.h"

#include "../../include_ext/scat_mano_fit_seq_views.h"

namespace scat {

struct SeqViewsArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float* cams;
    const float *targets2, *weights2;
    const int* joint_map;
    const float *lo, *hi;
    float* p;
    float* cost;
    int* accepted;
    float* ws;
    int T, C, cam_stride, iters, init;   // cam_stride: C * 16 floats with a rig per sequence, 0 with one for all
    float lambda0, w_pose, w_beta, w_limit, sigma2, z_near;
    float s_rots, s_poses, s_betas, s_trans, s_scale;
    uint64_t free_mask;
};

// init = 1: "frame t has a start" (1.f or 0.f) travels in the first word of the frame's L_t slot, which nothing else
// touches before the first forward walk writes L_t
__device__ __forceinline__ float* seq_views_flag(float* ws, int64_t s, int T, int t) {
    return seq_ws_l<kFU>(ws, s, T) + (int64_t)t * kSeqL<kFU>;
}

// init = 1: the launch of the start kernel, S T workgroups; the caller checks hipGetLastError
void seq_views_launch_start(const SeqViewsArgs& a, int S, hipStream_t stream);

}  // namespace scat
