// kp_readout.hip -- the kernels declared in kp_readout.hpp (see there) and their launchers.
#include <algorithm>

#include "kp_readout.hpp"
#include "kp_push.hpp"
#include "kp_contact_force.hpp"
#include "kp_inverse_dyn.hpp"
#include "kp_body_motion.hpp"
#include "kp_fit_pose.hpp"
#include "kp_contact_estimate.hpp"

namespace kp {

void launch_apply_impulse(const StepArgs& A, const int32_t* entity, const float* offset, const float* impulse, const uint8_t* mask, float* dqvel, hipStream_t stream) {
    hipLaunchKernelGGL(k_apply_impulse, dim3(A.n_envs), dim3(64), sizeof(EnvLds), stream, A, entity, offset, impulse, mask, dqvel);
}

void launch_contact_forces(const StepArgs& A, const XcArgs& X, bool obj, bool xc, int actuation, const float* act, const uint8_t* mask, const ContactOut& O, hipStream_t stream) {
    const dim3 grid(A.n_envs), block(64);
    if (obj) {
        if (xc) hipLaunchKernelGGL((k_contact_forces<true, true>), grid, block, sizeof(EnvLdsObj), stream, A, X, actuation, act, mask, O);
        else hipLaunchKernelGGL((k_contact_forces<true, false>), grid, block, sizeof(EnvLdsObj), stream, A, X, actuation, act, mask, O);
    } else {
        if (xc) hipLaunchKernelGGL((k_contact_forces<false, true>), grid, block, sizeof(EnvLds), stream, A, X, actuation, act, mask, O);
        else hipLaunchKernelGGL((k_contact_forces<false, false>), grid, block, sizeof(EnvLds), stream, A, X, actuation, act, mask, O);
    }
}

void launch_inverse_dynamics(InvDynArgs A, bool obj, hipStream_t stream) {
    // one wavefront per row; a launch holds at most 2^24 rows (grid x block stays below 2^32 threads)
    constexpr int CHUNK = 1 << 24;
    for (int r0 = 0; r0 < A.n_rows; r0 += CHUNK) {
        A.row0 = r0;
        const dim3 grid(std::min(CHUNK, A.n_rows - r0)), block(64);
        if (obj) hipLaunchKernelGGL((k_inverse_dynamics<true>), grid, block, sizeof(EnvLdsObj), stream, A);
        else hipLaunchKernelGGL((k_inverse_dynamics<false>), grid, block, sizeof(EnvLds), stream, A);
    }
}

void launch_body_motion(BodyMotionArgs A, hipStream_t stream) {
    constexpr int CHUNK = 1 << 24;                                      // as launch_inverse_dynamics
    for (int r0 = 0; r0 < A.n_rows; r0 += CHUNK) {
        A.row0 = r0;
        hipLaunchKernelGGL(k_body_motion, dim3(std::min(CHUNK, A.n_rows - r0)), dim3(64), sizeof(BodyMotionLds), stream, A);
    }
}

void launch_point_jacobian(PointJacArgs A, hipStream_t stream) {
    constexpr int CHUNK = 1 << 24;                                      // as launch_inverse_dynamics
    for (int r0 = 0; r0 < A.n_rows; r0 += CHUNK) {
        A.row0 = r0;
        hipLaunchKernelGGL(k_point_jacobian, dim3(std::min(CHUNK, A.n_rows - r0)), dim3(64), sizeof(PointJacLds), stream, A);
    }
}

void launch_fit_pose(FitPoseArgs A, hipStream_t stream) {
    constexpr int CHUNK = 1 << 24;                                      // as launch_inverse_dynamics
    for (int r0 = 0; r0 < A.n_rows; r0 += CHUNK) {
        A.row0 = r0;
        hipLaunchKernelGGL(k_fit_pose, dim3(std::min(CHUNK, A.n_rows - r0)), dim3(64), sizeof(EnvLds), stream, A);
    }
}

void launch_estimate_contacts(EstimateArgs A, bool obj, hipStream_t stream) {
    constexpr int CHUNK = 1 << 24;                                      // as launch_inverse_dynamics
    for (int r0 = 0; r0 < A.n_rows; r0 += CHUNK) {
        A.row0 = r0;
        const dim3 grid(std::min(CHUNK, A.n_rows - r0)), block(64);
        if (obj) hipLaunchKernelGGL((k_estimate_contacts<true>), grid, block, sizeof(EnvLdsObj), stream, A);
        else hipLaunchKernelGGL((k_estimate_contacts<false>), grid, block, sizeof(EnvLds), stream, A);
    }
}

}  // namespace kp
