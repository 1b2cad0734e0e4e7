// kp_pose_contacts.hpp -- the collision query of compute_physcis_metris (scripts/eval_pose_all.py:205-260: sim.forward() on a frame, then
// the walk of data.contact) on arbitrary poses, batched over frames and with no dynamics.
//
// One wavefront per row; a row is one frame: the 24 body poses (xpos / xquat, kp_sim_fk's wbpos / wbquat) and the frame's 35-float object
// block.  The pairs and narrow phases are those of collide<> (kp_step_collide.hpp): hull - floor (mjc_PlaneConvex) and hull - object geom
// (mjc_Convex, MPR in fp64, kp_collide.hpp), behind the same exact-safe culls.  What the metrics read is accumulated in registers instead of
// stored: the number of hull - (floor | object) contacts, the sum of their penetrations beyond pen_margin, and per object geom the set of
// hulls it touches.  No contact record is kept, so a row may hold any number of contacts (a lying pose sunk into the floor has 72).
//
// The kernel lives in its own translation unit (kp_pose_contacts.hip): compiled next to the step kernels in kp_sim.hip, it changed their code
// generation (same source, different register assignment in the object kernels), and the step kernels' code must not move.
#pragma once
#include <hip/hip_runtime.h>

#include "kp_device.hpp"

namespace kp {

constexpr int PC_MAXGEOM = 16;        // object geoms of a model the query accepts (the reference's scenes have 10); all may be active in one row

struct PoseContactArgs {
    DevTables T;
    Params P;                         // margin, pm_max, pm_tol
    int n_rows, n_og, n_obj;
    const float *xpos, *xquat;        // [R, 72], [R, 96]
    const float* obj_qpos;            // [R, 35] or null (floor only)
    const float* og;                  // body-frame object geoms [n_og][18] = object, type, size[3], pos[3], mat[9], mass
    float pen_margin;
    float* pen;                       // [R]
    int32_t* ncon;                    // [R]
    uint32_t* hits;                   // [R, n_og]
};

// enqueues k_pose_contacts on stream for A.n_rows > 0 rows (one workgroup of one wavefront per row)
hipError_t launch_pose_contacts(const PoseContactArgs& A, hipStream_t stream);

}  // namespace kp
