// kp_kin_tape.hpp -- the backward side of TrajARNet's kinematic roll-out in train form (kin_poly/models/traj_ar_smpl_net.py:346-383), one gradient kernel
// beside every forward kernel of kinpoly_amd/context.py's roll-out (include/kinpoly_sim.h: kp_kin_advance_backward, kp_sim_obs_ar_backward,
// kp_sim_fk_head_backward):
//
//   k_kin_advance_grad   (d k_kin_advance)^T: TrajARNet.step (:292-330) + get_qvel_fd_batch (kin_poly/utils/torch_utils.py:315-331)
//   k_obs_ar_grad        (d k_obs_ar / k_obs_ar_thread)^T with respect to qpos (local pose block), qvel (use_vel), the head position and the head's
//                        world quaternion (humanoid_ar_v1.py:133-214)
//   k_fk_head_grad       (d k_target_fk)^T for wbpos AND the head's world quaternion: k_fk_wbpos_grad's sums with the head quaternion's torque added on
//                        the head's root path (kin_poly/utils/torch_smpl_humanoid.py:125-202)
//
// fp32, rows independent, no atomics, no cross-row traffic: a row's gradient does not depend on its position in the batch.  The gradients are those of
// the forward kernels' own formulas (rotations normalise their quaternion, so a raw root quaternion receives no radial component).  The kernels live in
// their own translation unit (kp_kin_tape.hip) for the reason kp_pose_contacts.hpp gives: the step kernels' code generation must not move.
#pragma once
#include <hip/hip_runtime.h>

#include "kp_device.hpp"

namespace kp {

struct KinAdvanceGradArgs {
    int n;
    const float *qpos, *act;          // [n,76], [n,80]: the inputs of the forward call
    float dt;
    const float *g_next, *g_qvel;     // [n,76], [n,75] cotangents of next_qpos / qvel; either may be null (zero)
    float *g_qpos, *g_act;            // [n,76], [n,80]
};

struct ObsArGradArgs {
    int n, vel, head, width;          // the handle's layout; width = its row width (the one-hot's four columns carry no gradient)
    int T;                            // kp_ctx: frames, tables, frame of every row, optional row indirection
    const float *head_pose, *action_one_hot, *obj_qpos;
    const int *cur_t, *row;
    const float *qpos, *wbpos, *wbquat;      // [n,76] and the kp_sim_fk outputs of those rows
    const float *g_obs, *g_obj;              // [n,width]; optional [n,7] cotangent of the object block read as a feature (obj_2_head)
    float *g_qpos, *g_qvel, *g_hpos, *g_hquat;      // [n,76] (local pose block only), [n,75] (vel layouts), [n,3], [n,4]
};

struct FkHeadGradArgs {
    int n;
    const float *qpos, *wbpos, *wbquat;      // [n,76] and the kp_sim_fk outputs of those rows
    const float *g_wbpos, *g_hpos, *g_hquat; // [n,72], [n,3] (added to the head's slot of g_wbpos), [n,4]; each may be null (zero)
    const float* g_add;                      // optional [n,76] added to the result (k_obs_ar_grad's local part); may be g_qpos itself
    float* g_qpos;                           // [n,76]
    const int8_t* parent;
    const uint8_t* subtree;
};

hipError_t launch_kin_advance_grad(const KinAdvanceGradArgs& A, hipStream_t stream);
hipError_t launch_obs_ar_grad(const ObsArGradArgs& A, hipStream_t stream);
hipError_t launch_fk_head_grad(const FkHeadGradArgs& A, hipStream_t stream);

}  // namespace kp
