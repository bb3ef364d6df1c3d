// What the two launches of scat_mano_fit_seq_kp share (mano_fit_seq_kp.hip: the walk; mano_fit_seq_kp_start.hip: the frames'
// closed-form starts): the workspace's layout and the kernels' arguments.  The two kernels are two translation units on
// purpose: compiled in one, hipcc's inliner spends the walk's registers differently (mano_fit_seq_kp.hip has the figures).
#pragma once
#include "mano_fit_kp_common.h"

#include "../../include/scat_mano_fit_seq_kp.h"

namespace scat {

// per sequence: L_t and y_t for every frame, then M_t^T for every frame, then the unknowns, two buffers of [T][65]
constexpr int kQL = (kKU + 1) * kKU;            // 4290 floats: L_t, y_t as row 65
constexpr int kQM = kKU * kKU;                  // 4225 floats: M_t^T
constexpr int kQFrame = kQL + kQM + 2 * kKU;    // 8645 floats of workspace per frame
constexpr int kQMaxT = SCAT_FIT_SEQ_MAX_T;

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
