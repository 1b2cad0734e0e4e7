// kp_obs_ctx.hpp -- the kinematic model's observation row under `use_context` / `use_of` (config/statear/kin_only.yml, use_of.yml;
// kin_poly/models/traj_ar_smpl_net.py:226-230, 284-285; humanoid_ar_v1.py:151-155):
//
//   k_obs_ar_ctx         one launch writes [context block H | k_obs_ar's row W | of block F] at pitch H + W + F: the context GRU's hidden state at the
//                        row's frame, the base observation as obs_ar_row writes it (kp_obs_ar_row.hpp: k_obs_ar's text, the words are kp_sim_obs_ar's), the
//                        frame's image feature.  A null context table writes zeros (the reference's row before init_states)
//   k_obs_ctx_grad       the context block's cotangent: the first H columns of grad_obs as a contiguous [n, H] slab (the `of` block is data)
//   k_ctx_rows_write     the sampler's ring refill of the two wide context tables (kp_ctx_rows_write): m drawn clips' context sequence (time-major
//                        [T', m, H], what the GRU step writes) and image features ([m, T', F]) into row-major tables [R, T, .] at scattered rows, clips
//                        shorter than T padded with their last frame.  A pure copy: one block per (clip, frame), lanes along the feature axis,
//                        plain dwords (H and F need not be multiples of 4).  Duplicate rows are the caller's error (two clips would race for one
//                        row; ring_refill_plan never produces them); a row outside [0, R) is refused by the entry point and skipped by the kernel
//
// fp32, rows independent, no LDS, no cross-lane traffic, no atomics.  The kernels live in their own translation unit (kp_obs_ctx.hip) for the reason
// kp_pose_contacts.hpp gives: the step kernels' code generation must not move.  Inline device math is shared with kp_sim.hip's kernels through
// kp_quat.hpp and kp_obs_ar_row.hpp, which define no kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "kp_device.hpp"

namespace kp {

struct ObsArCtxArgs {
    int n, vel, head, action;          // rows and the handle's layout (kp::ObsArLayout)
    int T;                             // kp_ctx: frames, tables, frame of every row, optional row indirection
    const float *head_pose, *head_vels, *obj_rel, *action_one_hot, *obj_qpos;
    const int *cur_t, *row;
    int ctx_dim; const float* ctx_feat; long long ctx_stride_row, ctx_stride_t;      // kp_obs_ext; strides in floats, ctx_feat may be null (zeros)
    int of_dim; const float* of; long long of_stride_row, of_stride_t;
    const float *qpos, *qvel, *xpos, *xquat;      // the handle's state rows
    float* out;                        // [n, ctx_dim + W + of_dim]
};

hipError_t launch_obs_ar_ctx(const ObsArCtxArgs& A, hipStream_t stream);
// grad_ctx [n, H] <- grad_obs[:, :H] of rows `pitch` floats apart
hipError_t launch_obs_ctx_grad(int n, int H, const float* grad_obs, int pitch, float* grad_ctx, hipStream_t stream);

// ctx_table[rows[c], t, :] <- seq[min(t, Tp - 1), c, :], of_table[rows[c], t, :] <- of[c, min(t, Tp - 1), :] for c < m, t < T; either table may be null
// (its source is then not read).  rows: device int64 [m], every one in [0, R).  m >= 1, 1 <= Tp <= T, m * T < 2^31.
struct CtxRowsArgs {
    int m, R, T, Tp, H, F;
    const long long* rows;
    const float *seq, *of;
    float *ctx_table, *of_table;
};
hipError_t launch_ctx_rows_write(const CtxRowsArgs& A, hipStream_t stream);

}  // namespace kp
