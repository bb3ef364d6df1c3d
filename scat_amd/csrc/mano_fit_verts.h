// The mesh fit of mano_fit_verts.hip as the library's own callers see it: scat_mano_fit_verts and
// scat_mano_fit_verts_metric are fit_verts_check, then fit_verts_launch; the ICP loop over a cloud (mano_fit_points.hip)
// checks once and launches once per round.
#pragma once
#include <stdint.h>

struct VertsCall {
    const float *blend, *joint_t, *joint_s, *weights_t, *hands_mean;
    const float* targets;   // [B,V,3]
    const float* weights;   // [B,V] or null
    const float* normals;   // metric: [B,V,3]
    float* p;               // [B,62]
    float* cost;            // [B]
    int* accepted;          // [B]
    int B, V;
    uint64_t parents;
    int iters, init;
    int metric;             // the plane metric of the normals with w_tangent; its start is the caller's
    float w_tangent, lambda0, w_pose, w_beta;
    uint64_t free_mask;
    int tile;               // vertices per tile; 0: kVTile, the product's
    void* stream;
};

// every check but the tile's.  fn: the entry point named in the errors; *levels: the depth of the joint tree, which the
// launch takes
int fit_verts_check(const char* fn, const VertsCall& c, int* levels);
int fit_verts_launch(const char* fn, const VertsCall& c, int levels);

// tau of a plane metric, in 0..1: the one text of the mesh fit, the track solve and the assignment
int fit_check_tau(const char* fn, float w_tangent);
