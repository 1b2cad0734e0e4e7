// kp_readout_device.hpp -- what the read-out kernels (kp_push.hpp, kp_contact_force.hpp, kp_inverse_dyn.hpp, kp_fit_pose.hpp, kp_fit_points.hpp, kp_fit_scene.hpp) share beyond the control step's own device
// functions: the env prologue and the projection of forces on the dofs.  Read-out unit only (kp_readout.hip): the step kernels' unit does not see how these
// specialise the step's functions.  Each helper holds what ALL its users did before it existed, no more: a store one kernel does not need costs the
// object instantiations scalar registers (profiles/readout_split/tool_benches.md).
#pragma once
#include "kp_step_device.hpp"

namespace kp {

// An env's LDS block before a kernel's own state rows: the per-lane model tables, no applied force (applied[6] ++ ctrl[72]), no rows yet.  The caller loads
// its state (OBJ: its geoms and slots) and syncs.  k_apply_impulse, k_contact_forces and k_fit_pose; k_inverse_dynamics has the same stores fused into its row loads.
template <class SL>
__device__ __forceinline__ void readout_prologue(SL& s, const DevTables& T, int tid) {
    for (int i = tid; i < D_NV; i += 64) { s.arm[i] = T.dof_armature[i]; s.dbody[i] = T.dof_body[i]; }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bsub[tid] = T.body_subtree[tid]; s.bdep[tid] = T.body_depth[tid]; }
    for (int i = tid; i < 78; i += 64) s.applied[i] = 0.f;
    if (tid == 0) { s.ncon = 0; s.nlim = 0; s.flag = 0; }
}

// What the articulated-body passes read besides: no extra armature, and the zero words / zero record of IAa / pAa for padded and absent operands.  The two
// kernels that run such a pass (k_apply_impulse, k_contact_forces, k_fit_pose).
template <class SL>
__device__ __forceinline__ void readout_aba_zeros(SL& s, int tid) {
    for (int i = tid; i < D_NV; i += 64) s.extra[i] = 0.f;
    if (tid < 25) s.IAa[22 * tid + 21] = 0.f;
    if (tid < 22) s.IAa[22 * 24 + tid] = 0.f;
    if (tid < 6) s.pAa[6 * 24 + tid] = 0.f;
}

// out[d] = cdof_d . (sum of the body wrenches s.sw over the subtree of d's body): the backward half of mj_rne on whatever wrenches the caller stored
template <class SL>
__device__ __forceinline__ void project_body_wrenches(SL& s, float* out, int tid) {
    KP_SYNC();
    subtree_sums<64>(s, tid);
    for (int d = tid; d < D_NV; d += 64) out[d] = dot6(lds6(s.cdof + 6 * d), lds6(s.sa + 6 * s.dbody[d]));
    KP_SYNC();
}

// out = J^T f as a PROJECTION of the forces (never M qacc - qfrc_smooth): the hulls' contact wrenches about o from the contacts' world forces fc [ncon][3],
// their subtree sums, the dot product with every dof's motion axis; the limit rows add sgn (-D jar) on their own dof (lim_D is the signed weight), inside
// the projection loop.  (wrench_project of the step kernels does the same with the opposite sign.)
// Preconditions: make_constraint and a row evaluation have run (con_start, con_pos, lim_jar, lim_D are current); fc[0 .. 3 ncon) is written and visible to
// every lane (a KP_SYNC behind its store).  out is visible on return.
template <class SL>
__device__ __forceinline__ void project_contact_forces(SL& s, const float* fc, float* out, int tid) {
    if (tid < D_NB) {
        const V3 o = ld3(s.xpos);
        S6 W = S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
        for (int c = s.con_start[tid]; c < s.con_start[tid + 1]; c++) {
            const V3 F = ld3(fc + 3 * c), p = ld3(s.con_pos + 3 * c) - o;
            W.a = W.a + cross(p, F); W.l = W.l + F;
        }
        sts6(s.sw + 6 * tid, W);
    }
    KP_SYNC();
    subtree_sums<64>(s, tid);
    for (int d = tid; d < D_NV; d += 64) {
        float v = dot6(lds6(s.cdof + 6 * d), lds6(s.sa + 6 * s.dbody[d]));
        if (d >= 6) { const float jr = s.lim_jar[d - 6]; if (jr < 0.f) v -= s.lim_D[d - 6] * jr; }
        out[d] = v;
    }
    KP_SYNC();
}

}  // namespace kp
