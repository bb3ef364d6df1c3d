// The track solve of mano_fit_seq_verts.hip as the library's own callers see it: scat_mano_fit_seq_verts is
// seq_verts_check, then seq_verts_launch, with stats = null and acc_add = 0; the ICP loop over a track of clouds
// (mano_fit_points.hip) checks once, launches once per round, passes the assignment's stats and lets the accepted counts
// add up over its rounds.
#pragma once
#include <stdint.h>

struct SeqVertsCall {
    const float *blend, *joint_t, *joint_s, *weights_t, *hands_mean;
    const float* targets;   // [S,T,V,3]
    const float* weights;   // [S,T,V] or null
    const float* normals;   // [S,T,V,3] or null: selects the plane metric
    const double* stats;    // [S T,4] of the assignment that made targets and weights, or null.  With it a frame whose
                            // stats[.][0] != 0 refuses its sequence and one with no matched weight is bridged
    float* p;               // [S,T,62]
    float* cost;            // [S]
    int* accepted;          // [S]
    void* ws;
    int64_t ws_bytes;
    int S, T, V;
    uint64_t parents;
    int iters, init;
    float w_tangent, lambda0, w_pose, w_beta;
    float smooth[5];        // s_rots, s_poses, s_betas, s_trans, s_scale
    uint64_t free_mask;
    int acc_add;            // accepted[s] += the count, instead of = the count
    void* stream;
};

// the names of smooth[] in the errors
static const char* const kSeqVertsSmooth[5] = {"s_rots", "s_poses", "s_betas", "s_trans", "s_scale"};

// the bytes of workspace the solve needs; 0 for sizes it refuses
int64_t seq_verts_ws_bytes(int S, int T, int V);

// every check.  fn: the entry point named in the errors; *levels: the depth of the joint tree, which the launches take
int seq_verts_check(const char* fn, const SeqVertsCall& c, int* levels);
// the 2 iters + 2 launches (two more with init), no check but the launches' own
int seq_verts_launch(const char* fn, const SeqVertsCall& c, int levels);
