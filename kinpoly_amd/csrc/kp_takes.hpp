// kp_takes.hpp -- the UHC's take library and the fused tracking step (include/kinpoly_sim.h: kp_takes_*, kp_sim_uhc_track, kp_sim_uhc_assign).
//
//   k_take_tables   get_expert's derived features (uhc/utils/tools.py:20-85) for R concatenated rows, segmented by take
//   k_take_minima   height_lb / head_height_lb per take (tools.py:82-83)
//   k_uhc_track     the tail of HumanoidEnv.step after do_simulation (uhc/envs/humanoid_im.py:527-572): cur_t, calc_body_diff, termination,
//                   world_rfc_implicit_reward (uhc/core/reward_function.py:4-53), and the expert rows of the next observation / control step
//   k_uhc_track_r   k_uhc_track with another function of the reward registry (reward_function.py:453-460; kp_sim_uhc_track_r), one instantiation each
//   k_uhc_assign    reset_model / fail_safe (humanoid_im.py:574-623, 235-238): take, start and state of the masked envs
//   k_uhc_assign_obj  the same for a library that carries object poses (kp_takes_create_obj): reset_model's has_obj branch (:613-616) installs the env's
//                   object block from the library row the humanoid state comes from -- what kp_sim.hip's k_set_objects installs from a caller's rows
//
// One wavefront per row / take / env, lane = body; reductions are kp_collide.hpp's DPP butterflies, so there is no LDS, no atomic and every
// store is a plain vector store.  The kernels live in their own translation unit (kp_takes.hip) for the reason kp_pose_contacts.hpp gives: the step
// kernels' code generation must not move.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/kinpoly_sim.h"
#include "kp_device.hpp"

namespace kp {

// the tables, in the order of TakeTables::tab; the last two have one row per take
enum TakeTab { TT_QPOS, TT_QPOS_FK, TT_WBPOS, TT_WBQUAT, TT_BQUAT, TT_BODY_COM, TT_COM, TT_HEAD_POSE, TT_EE_WPOS, TT_EE_POS, TT_RQ_RMH, TT_QVEL,
               TT_RLINV, TT_RANGV, TT_RLINV_LOCAL, TT_BANGVEL, TT_HEIGHT_LB, TT_HEAD_HEIGHT_LB, TT_COUNT };
constexpr int TT_ROW_TABLES = TT_HEIGHT_LB;
constexpr int TAKE_TAB_WIDTH[TT_COUNT] = {76, 76, 72, 96, 96, 72, 3, 7, 15, 15, 4, 75, 3, 3, 3, 72, 1, 1};

struct TakeTables {
    float* tab[TT_COUNT];             // [R, width] ([K, 1] for the last two)
    const int32_t* take_off;          // [K + 1]
    const int32_t* row_take;          // [R] the take a row belongs to
    int R, K;
};

struct TakeBuildArgs {
    TakeTables L;
    const float* body_mass;           // [24]
    float inv_dt;                     // (float)(1 / dt) in fp64: the factor the torch path's `x / dt` multiplies by
};

struct UhcTrackArgs {
    TakeTables L;
    int n;
    kp_uhc_state st;
    kp_uhc_cfg cfg;
    float inv_dt;
    const float *qpos, *xpos, *xipos, *prev_bquat;             // sim state after the control step
    float *t_qpos, *t_wbpos, *t_wbquat, *t_bquat, *t_com;      // the stored target (kp_sim_set_target's buffers)
    const float *body_mass, *b_diffw, *jpos_diffw;             // [24] each
    const float* action;
    float *reward, *info, *body_diff, *percent;
    uint8_t *fail, *end, *done;
};

// what the other reward functions read beside UhcTrackArgs (k_uhc_track's arguments stay as they are)
struct UhcRewardExt {
    float w_rp, w_rv, k_rh, k_rq, k_rl, k_ra, w_wp, w_j, k_wp, k_j;
    const float* jw;                  // [24] reward_weights.jpos_diffw (v2 / v3)
    const float* prev_qpos;           // [N,76] the qpos before the control step (local_rfc_implicit)
    const float* xquat;               // sim state after the control step (v2 / v3)
};

struct UhcAssignArgs {
    TakeTables L;
    int n, keep_t, obs_v;
    kp_uhc_state st;
    const uint8_t* mask;
    const int32_t *take_ids, *start;  // device [N] or null
    const float* noise;               // [N, 69] or null
    const float* a_ref;
    float *qpos, *qpos_d, *qvel, *qvel_d, *warm;
    float *t_qpos, *t_wbpos, *t_wbquat, *t_bquat, *t_com;
};

// k_uhc_assign's arguments stay as they are; the object block rides beside them
struct UhcAssignObjArgs {
    UhcAssignArgs A;
    const float* obj_tab;             // [R,35] data.qpos[76:111] per library row (outside TakeTables::tab: the three kernels above never see it)
    float *obj_qpos, *obj_qvel, *obj_warm, *geoms;             // kp_sim's object rows [N,35], [N,30], [N,6 D_MAXOBJ], [N,D_MAXGEOM,17]
    int* ngeom;
    signed char* slot;                // [N,D_MAXOBJ]
    const float *og, *omass;          // the model's object geoms [n_og,18] and masses [n_obj]
    int n_og, n_obj, dynamic;         // n_og <= 64: one lane per geom
};

hipError_t launch_take_tables(const TakeBuildArgs& A, hipStream_t stream);
hipError_t launch_uhc_track(const UhcTrackArgs& A, hipStream_t stream);
hipError_t launch_uhc_track_r(int reward_id, const UhcTrackArgs& A, const UhcRewardExt& X, hipStream_t stream);      // reward_id: KP_UHC_*
hipError_t launch_uhc_assign(const UhcAssignArgs& A, hipStream_t stream);
hipError_t launch_uhc_assign_obj(const UhcAssignObjArgs& A, hipStream_t stream);

}  // namespace kp
