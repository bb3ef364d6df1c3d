// What the two launches of scat_mano_fit_seq_kp share (mano_fit_seq_kp.hip: the walk; mano_fit_seq_kp_start.hip: the frames'
// closed-form starts): the kernels' arguments; the workspace's layout is mano_fit_seq_common.h's at 65 unknowns.  The two
// kernels are two translation units on purpose: compiled in one, hipcc's inliner spends the walk's registers differently
// (mano_fit_seq_kp.hip has the figures).
#pragma once
#include "mano_fit_kp_common.h"
#include "mano_fit_seq_common.h"

#include "../../include/scat_mano_fit_seq_kp.h"

namespace scat {

struct SeqKpArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float *targets3, *weights3, *targets2, *weights2;
    const int* joint_map;
    const float *lo, *hi;
    float* p;
    float* cost;
    int* accepted;
    float* ws;
    int T, iters, init;
    float lambda0, w_pose, w_beta, w_limit, sigma3, sigma2, half[2];
    float s_rots, s_poses, s_betas, s_trans, s_scale, s_cs, s_ct;
    uint64_t free_mask;
    int free_cam;
};

// init = 1: the launch of the start kernel, S T workgroups; the caller checks hipGetLastError
void seq_kp_launch_start(const SeqKpArgs& a, int S, hipStream_t stream);

}  // namespace scat
