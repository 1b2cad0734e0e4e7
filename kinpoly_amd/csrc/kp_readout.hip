// kp_readout.hip -- the kernels declared in kp_readout.hpp (see there) and their launchers.
#include <algorithm>
#include <cstdlib>

#include "kp_readout.hpp"
#include "kp_push.hpp"
#include "kp_contact_force.hpp"
#include "kp_inverse_dyn.hpp"
#include "kp_body_motion.hpp"
#include "kp_fit_pose.hpp"
#include "kp_fit_points.hpp"
#include "kp_fit_scene.hpp"
#include "kp_fit_image.hpp"
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

// The rows kernels: one wavefront per row; a launch holds at most 2^24 rows (grid x block stays below 2^32 threads), so a call is a loop of chunks and
// the kernel finds its row at blockIdx.x + row0.  KP_ROWS_CHUNK (an experiment variable; read per call, clamped to [64, 2^24],
// absent or invalid: 2^24) makes the chunks small enough that a test reaches row0 > 0.
static int rows_chunk() {
    constexpr long MAX = 1 << 24;
    const char* e = std::getenv("KP_ROWS_CHUNK");
    if (!e || !*e) return MAX;
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    if (*end || v <= 0) return MAX;
    return (int)std::clamp(v, 64L, MAX);
}

template <auto K, size_t LDS, class Args>
static void launch_rows(Args A, hipStream_t stream) {
    const int chunk = rows_chunk();
    for (int r0 = 0, n; r0 < A.n_rows; r0 += n) {
        n = std::min(chunk, A.n_rows - r0);
        A.row0 = r0;
        hipLaunchKernelGGL(K, dim3(n), dim3(64), LDS, stream, A);
    }
}

void launch_inverse_dynamics(InvDynArgs A, bool obj, hipStream_t stream) {
    if (obj) launch_rows<k_inverse_dynamics<true>, sizeof(EnvLdsObj)>(A, stream);
    else launch_rows<k_inverse_dynamics<false>, sizeof(EnvLds)>(A, stream);
}

void launch_body_motion(BodyMotionArgs A, hipStream_t stream) { launch_rows<k_body_motion, sizeof(BodyMotionLds)>(A, stream); }

void launch_point_jacobian(PointJacArgs A, hipStream_t stream) { launch_rows<k_point_jacobian, sizeof(PointJacLds)>(A, stream); }

void launch_fit_pose(FitPoseArgs A, hipStream_t stream) { launch_rows<k_fit_pose, sizeof(EnvLds)>(A, stream); }

void launch_fit_points(FitPointsArgs A, hipStream_t stream) { launch_rows<k_fit_points, sizeof(EnvLds)>(A, stream); }

void launch_fit_scene(FitSceneArgs A, hipStream_t stream) { launch_rows<k_fit_scene, sizeof(EnvLds)>(A, stream); }

void launch_fit_image(FitImageArgs A, hipStream_t stream) { launch_rows<k_fit_image, sizeof(EnvLds)>(A, stream); }

void launch_estimate_contacts(EstimateArgs A, bool obj, hipStream_t stream) {
    if (obj) launch_rows<k_estimate_contacts<true>, sizeof(EnvLdsObj)>(A, stream);
    else launch_rows<k_estimate_contacts<false>, sizeof(EnvLds)>(A, stream);
}

}  // namespace kp
