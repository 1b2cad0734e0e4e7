// kp_readout.hpp -- the kernels beside the control step that are built from its device functions (kp_step_device.hpp): impulse pushes (kp_push.hpp,
// DESIGN.md section 12), the contact-force read-out (kp_contact_force.hpp, section 14) inverse dynamics on motion rows (kp_inverse_dyn.hpp,
// section 15), body motion, momentum and energy on motion rows (kp_body_motion.hpp, section 16) and point Jacobians and pose fitting on motion rows
// (kp_fit_pose.hpp, section 17; kp_fit_points.hpp, section 20; kp_fit_scene.hpp, section 21; kp_fit_image.hpp, section 22) and contact forces estimated from kinematics on motion rows (kp_contact_estimate.hpp, section 18).  They live in their own translation unit (kp_readout.hip): however they specialise the shared device functions, the step kernels' unit
// does not see it, so the step kernels' code cannot move with them.  kp_sim.hip keeps the entry points' argument checks and calls the launchers below.
#pragma once
#include <hip/hip_runtime.h>

#include "kp_step_device.hpp"

namespace kp {

// every pointer optional (kp_contact_out of the C ABI)
struct ContactOut {
    int32_t* ncon;             // [N]
    float *contact;            // [N, 64, 12]
    float *wrench;             // [N, 26, 6] force, torque about the WORLD ORIGIN (world axes)
    float *qfrc_constraint;    // [N, 75]
    float *qacc;               // [N, 75]
    float *torque;             // [N, 75] qfrc_applied[0:6] ++ ctrl[69] as the solve used them
    float *obj_qacc;           // [N, 2, 6] object slots, joint coordinates
};

// every pointer optional (kp_invdyn_out of the C ABI)
struct InvDynOut {
    float *qfrc_inverse;       // [R, 75] qfrc_applied[0:6] ++ ctrl[69] coordinates
    float *qfrc_constraint;    // [R, 75] J^T f + the limit rows at the given qacc
    float *qfrc_bias;          // [R, 75] C(q, qd) + g
    float *contact;            // [R, 64, 12] the rows of kp_sim_contact_forces
    float *net_wrench;         // [R, 6] sum of the contact forces, their torque about the WORLD ORIGIN (world axes)
    int32_t* ncon;             // [R]
};

struct InvDynArgs {
    DevTables T;
    Params P;
    int n_rows, row0;          // a launch covers rows row0 .. n_rows - 1 (blockIdx.x + row0); row0 is the launcher's
    const float *qpos, *qvel, *qacc;     // [R, 76], [R, 75] or null (zero), [R, 75] or null (zero)
    const float* geoms;        // OBJ: [R, D_MAXGEOM, 17] world-frame static geoms of the rows
    const int* ngeom;          // OBJ: [R]
    InvDynOut O;
};

// every pointer optional (kp_motion_out of the C ABI)
struct BodyMotionOut {
    float *body_vel;           // [R, 24, 6] world angular velocity, world linear velocity of the body frame origin
    float *body_acc;           // [R, 24, 6] world angular acceleration, classical linear acceleration of the body frame origin
    float *body_com_vel;       // [R, 24, 3] linear velocity of the body's centre of mass
    float *centroid;           // [R, 18] com, com_vel, L_com, ke, pe, com_acc, Ldot_com, mass
};

struct BodyMotionArgs {
    DevTables T;
    Params P;
    int n_rows, row0;          // as InvDynArgs
    const float *qpos, *qvel, *qacc;     // [R, 76], [R, 75] or null (zero), [R, 75] or null (zero)
    BodyMotionOut O;
};

struct PointJacArgs {
    DevTables T;
    Params P;
    int n_rows, row0;          // as InvDynArgs
    const float* qpos;         // [R, 76]
    const int32_t* body;       // [R] 0..23; anything else: a zero row
    const float* offset;       // [R, 3] in the body frame, or null (the body origin)
    float* J;                  // [R, 6, 75]
};

// kp_fit_in, kp_fit_cfg and kp_fit_out of the C ABI in one block
struct FitPoseArgs {
    DevTables T;
    Params P;
    int n_rows, row0;          // as InvDynArgs
    const float *qpos0, *tgt_pos, *tgt_quat, *w_pos, *w_rot, *q_prior, *w_prior;      // [R, 76], [R, 24, 3], then optional: [R, 24, 4], [R, 24], [R, 24], [R, 69], [R, 69]
    int n_iters, clamp_limits;
    float mu0, mu_min, mu_max, mu_up, mu_down;
    float damp[D_NV];
    float *qpos, *info, *dq;   // [R, 76], [R, 8], [R, 75] or null
};

// kp_fit_points_in, kp_fit_points_cfg and kp_fit_points_out of the C ABI in one block, and the marker set as kp_sim_fit_points uploads it
struct FitPointsArgs {
    DevTables T;
    Params P;
    int n_rows, row0;          // as InvDynArgs
    const float *qpos0, *pt_tgt, *pt_w, *tgt_pos, *tgt_quat, *w_pos, *w_rot, *q_prior, *w_prior;      // [R, 76], [R, K, 3], then optional: [R, K], [R, 24, 3], [R, 24, 4], [R, 24], [R, 24], [R, 69], [R, 69]
    int n_points;              // K
    const float* pt_off;       // [K, 3] offsets in the body frame, ordered by body
    const int32_t *pt_perm, *pt_adr;     // [K] the caller's index of ordered point j; [25] body b owns ordered points adr[b] .. adr[b + 1]
    int n_iters, clamp_limits;
    float mu0, mu_min, mu_max, mu_up, mu_down;
    float damp[D_NV];
    float w_floor, floor_z;
    float *qpos, *info, *dq, *pt_err;    // [R, 76], [R, 12], [R, 75] or null, [R, K] or null (the caller's point order)
};

// kp_sim_fit_scene: kp_sim_fit_points' block, the rows' static geoms as place_static_rows leaves them and the object term's weight
struct FitSceneArgs : FitPointsArgs {      // info is [R, 16] here
    const float* geoms;        // [R, D_MAXGEOM, 17] world-frame static geoms of the rows, or null: every row is the floor scene
    const int* ngeom;          // [R]
    float w_obj;
};

// kp_sim_fit_image: kp_sim_fit_scene's block and the 2D observations of calibrated cameras (kp_fit_image_obs / kp_fit_image_cfg / kp_fit_image_out)
struct FitImageArgs : FitSceneArgs {      // info is [R, 20] here; pt_adr is a table of zeros when the call has no 3D targets (pt_tgt null)
    const int32_t* img_adr;    // [25] the marker set's own adr: the points the image walk covers
    int n_cams, camera_rows;   // C (0..8); 1 or R
    const float *cam, *uv, *uv_w;        // [camera_rows, C, 16] R_cw (row-major), t, fx, fy, cx, cy; [R, C, K, 2]; [R, C, K] or null (ones)
    float z_near;
    float* uv_err;             // [R, C, K] or null (the caller's order)
};

// every pointer optional (kp_estimate_out of the C ABI)
struct EstimateOut {
    float *qfrc_inverse;       // [R, 75] need - qfrc_contact; its root part is the residual
    float *qfrc_contact;       // [R, 75] J^T f of the estimated forces
    float *contact;            // [R, 64, 12] the rows of kp_sim_contact_forces: B = -1, the candidate's distance, the estimated force
    float *lambda;             // [R, 64, 4] pyramid-edge multipliers (N), edges n + mu t1, n - mu t1, n + mu t2, n - mu t2
    float *resid;              // [R, 6] e = r - G lambda: force, moment about the root position (world axes)
    float *net_wrench;         // [R, 6] sum of the estimated forces, their torque about the WORLD ORIGIN (world axes)
    int32_t* ncon;             // [R] candidates
    float *info;               // [R, 8] cost at lambda = 0, final cost, iterations, active columns, |F(e)| at exit, line searches, 0, status
};

struct EstimateArgs {
    DevTables T;
    Params P;                  // the model's with margin = reach and mu = the call's
    int n_rows, row0;          // as InvDynArgs
    const float *qpos, *qvel, *qacc;     // [R, 76], [R, 75] or null (zero), [R, 75] or null (zero)
    const float* geoms;        // OBJ: [R, D_MAXGEOM, 17] world-frame static geoms of the rows
    const int* ngeom;          // OBJ: [R]
    float sf, sm, rho_hat;     // sqrt(w_f), sqrt(w_m), rho / w_f
    int n_iters;
    EstimateOut O;
};

// Each enqueues on `stream` and returns; the caller reads the launch status (hipGetLastError).  One wavefront per env / row, full LDS layouts.
// A: the step kernels' argument pack (state rows, object rows); one block per env
void launch_apply_impulse(const StepArgs& A, const int32_t* entity, const float* offset, const float* impulse, const uint8_t* mask, float* dqvel, hipStream_t stream);
// obj: the handle simulates objects (EnvLdsObj); xc: the extended controller (X); one block per env
void launch_contact_forces(const StepArgs& A, const XcArgs& X, bool obj, bool xc, int actuation, const float* act, const uint8_t* mask, const ContactOut& O, hipStream_t stream);
// obj: the rows carry static geoms (A.geoms / A.ngeom); launches of at most 2^24 rows each
void launch_inverse_dynamics(InvDynArgs A, bool obj, hipStream_t stream);
// body motion, momentum and energy of rows (kp_body_motion.hpp, section 16): its own small LDS layout; launches of at most 2^24 rows each
void launch_body_motion(BodyMotionArgs A, hipStream_t stream);
// point Jacobians and pose fitting on rows (kp_fit_pose.hpp, section 17): the first on its own small LDS layout, the second on EnvLds; launches of at most 2^24 rows each
void launch_point_jacobian(PointJacArgs A, hipStream_t stream);
void launch_fit_pose(FitPoseArgs A, hipStream_t stream);
// pose fitting to points at body offsets with a floor term (kp_fit_points.hpp, section 20): on EnvLds; launches of at most 2^24 rows each
void launch_fit_points(FitPointsArgs A, hipStream_t stream);
// pose fitting that keeps the hulls out of the rows' static objects (kp_fit_scene.hpp, section 21): on EnvLds; launches of at most 2^24 rows each
void launch_fit_scene(FitSceneArgs A, hipStream_t stream);
// pose fitting to 2D key points seen by calibrated cameras (kp_fit_image.hpp, section 22): on EnvLds; launches of at most 2^24 rows each
void launch_fit_image(FitImageArgs A, hipStream_t stream);
// contact forces estimated from kinematics (kp_contact_estimate.hpp, section 18): obj as launch_inverse_dynamics; launches of at most 2^24 rows each
void launch_estimate_contacts(EstimateArgs A, bool obj, hipStream_t stream);

}  // namespace kp
