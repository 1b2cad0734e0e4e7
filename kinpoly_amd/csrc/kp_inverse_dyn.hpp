// kp_inverse_dyn.hpp -- inverse dynamics on motion rows (kp_sim_inverse_dynamics).
//
// What mj_inverse hands out in mujoco-py (data.qfrc_inverse), per ROW of a motion (qpos, qvel, qacc): the generalized force the model needs to perform
// it.  The reference has no counterpart (deviation list).  In the soft-constraint model the inverse is closed form: the row residuals
// at the GIVEN acceleration are jar = J qacc - aref, the row forces -D jar where jar < 0, and
//     qfrc_inverse = M qacc + qfrc_bias - J^T f,
// which is one evaluation of the Newton solver's gradient with no applied force -- no solve.  So the kernel is the front half of k_contact_forces
// (forward pass, collide, make_constraint) with the given qacc in the iterate's place, one row evaluation and the projections.
// A rows API like kp_sim_fk: it reads the model tables and the row inputs only, none of the handle's stored state and no warm start, and stores into
// its own output rows alone.  Always the full layouts (EnvLds / EnvLdsObj, 64 contact slots): no lean layout, so no overflow path.
// Objects are static obstacles at the row's pose (nobj = 0: no obj_forward, no Schur part); their world geoms come from a per-call scratch buffer that
// the placement kernel of kp_sim_set_objects filled.  A row without a placed geom runs the floor code, so a parked block and no block agree bit for bit.
// Compiled in the read-out unit (kp_readout.hip), which the step kernels' unit cannot see; the force projections are kp_readout_device.hpp's.  The load
// section is the kernel's own, like step_body's: it is readout_prologue's stores fused into the row loads, and calling the helper instead (two loops over
// the dofs where this is one) costs k_inverse_dynamics<true> 5 to 9 scalar-register spills and 1 % of its time.
#pragma once
#include "kp_contact_force.hpp"

namespace kp {

// one row on one wavefront; s: the row's LDS block with qpos, qvel, qacc and the per-lane tables loaded (OBJ: the static geoms too)
template <bool OBJ, class SL>
__device__ __forceinline__ void invdyn_row(SL& s, const InvDynArgs& A, size_t r, int tid) {
    const DevTables& T = A.T;
    const Params& P = A.P;
    const InvDynOut& O = A.O;
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<64>(s, T, P, depth, bpos, tid);                    // always the given pose: fresh kinematics
    collide<64, OBJ>(s, T, P, tid);
    const int ncon = s.ncon;                                            // <= 64: one contact per lane below
    const float my_dist = tid < ncon ? s.con_D[tid] : 0.f;              // con_D holds the distance until make_constraint
    make_constraint<64, OBJ>(s, T, P, tid);
    const bool rows = ncon != 0 || s.nlim != 0;
    // the given qacc in the iterate's place: body accelerations, then jar = J qacc - aref (exactly the solver's first row evaluation)
    float* sacc = s.Mv;                                                 // [24][6] over Mv + mres
    spatial_accumulate<64>(s, s.qacc, depth, tid, sacc);
    eval_rows<64, OBJ>(s, s.qacc, s.jar3, s.lim_jar, true, tid, sacc);

    // ---- M qacc + qfrc_bias -> s.qacc_s: body wrenches I_b a_b + fb_b, subtree sums, projection, armature
    if (tid < D_NB) sts6(s.sw + 6 * tid, inert_mul(s.cinert + 10 * tid, lds6(sacc + 6 * tid)) + lds6(s.fb + 6 * tid));
    project_body_wrenches(s, s.qacc_s, tid);
    for (int d = tid; d < D_NV; d += 64) s.qacc_s[d] += s.arm[d] * s.qacc[d];
    // ---- qfrc_bias alone -> s.search (only when asked for: no other output depends on it)
    if (O.qfrc_bias) {
        if (tid < D_NB) sts6(s.sw + 6 * tid, lds6(s.fb + 6 * tid));
        project_body_wrenches(s, s.search, tid);
    }
    // ---- J^T f -> s.x, as k_contact_forces forms it: the contacts' world forces, hull wrenches about o, subtree sums, projection, the limit rows
    float* fc = s.jv3;                                                  // [ncon][3] world force on A (aref is folded into jar3 by now)
    if (rows) {
        KP_SYNC();
        if (tid < ncon) st3(fc + 3 * tid, contact_force<OBJ>(s, P, tid));
        KP_SYNC();
        project_contact_forces(s, fc, s.x, tid);
    }
    KP_SYNC();

    // ---- outputs
    for (int i = tid; i < D_NV; i += 64) {
        const float fcon = rows ? s.x[i] : 0.f;
        if (O.qfrc_inverse) O.qfrc_inverse[r * D_NV + i] = s.qacc_s[i] - fcon;
        if (O.qfrc_constraint) O.qfrc_constraint[r * D_NV + i] = fcon;
        if (O.qfrc_bias) O.qfrc_bias[r * D_NV + i] = s.search[i];
    }
    if (O.ncon && tid == 0) O.ncon[r] = ncon;
    if (O.contact) {
        // k_contact_forces' row store with B = -1 (the floor or a static geom, always).  Written out in both kernels: as one function of the LDS block it
        // costs the object kernels 5 % code and 1.5 % time (profiles/readout_split/tool_benches.md)
        float* row = O.contact + (r * D_MAXCON + tid) * D_CF_ROW;
        if (tid < ncon) {
            V3 n = v3(0.f, 0.f, 1.f);
            if constexpr (OBJ) n = ld3(s.con_n + 3 * tid);
            const V3 f = ld3(fc + 3 * tid);
            row[0] = (float)s.con_body[tid]; row[1] = -1.f; row[2] = my_dist;
            st3(row + 3, ld3(s.con_pos + 3 * tid)); st3(row + 6, n); st3(row + 9, f);
        } else {
#pragma unroll
            for (int k = 0; k < D_CF_ROW; k++) row[k] = 0.f;
        }
    }
    if (O.net_wrench && tid == 0) {
        // every contact's vertex sits on a hull (no object entities): one lane, the contacts in stored order: one summation order, no atomics
        V3 F = v3(0.f, 0.f, 0.f), M = v3(0.f, 0.f, 0.f);
        for (int c = 0; c < ncon; c++) { const V3 f = ld3(fc + 3 * c); F = F + f; M = M + cross(ld3(s.con_pos + 3 * c), f); }
        st3(O.net_wrench + r * 6, F); st3(O.net_wrench + r * 6 + 3, M);
    }
}

// One wavefront per row.  OBJ: the rows carry static geoms (A.geoms / A.ngeom); a row with none of them runs the floor code on the same block.
template <bool OBJ>
__global__ __launch_bounds__(64) void k_inverse_dynamics(InvDynArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using SL = typename std::conditional<OBJ, EnvLdsObj, EnvLds>::type;
    SL& s = *reinterpret_cast<SL*>(smem_raw);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    for (int i = tid; i < D_NQ; i += 64) s.qpos[i] = A.qpos[r * D_NQ + i];
    for (int i = tid; i < D_NV; i += 64) {
        s.qvel[i] = A.qvel ? A.qvel[r * D_NV + i] : 0.f;
        s.qacc[i] = A.qacc ? A.qacc[r * D_NV + i] : 0.f;
        s.arm[i] = T.dof_armature[i]; s.dbody[i] = T.dof_body[i];
    }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bsub[tid] = T.body_subtree[tid]; s.bdep[tid] = T.body_depth[tid]; }
    for (int i = tid; i < 78; i += 64) s.applied[i] = 0.f;             // applied[6] ++ ctrl[72]: no force is applied
    if (tid == 0) { s.ncon = 0; s.nlim = 0; s.flag = 0; }
    int ngs = 0;
    if constexpr (OBJ) {
        ngs = min(max(A.ngeom[r], 0), D_MAXGEOM);                       // wave-uniform
        for (int i = tid; i < ngs * 17; i += 64) s.geom[i] = A.geoms[r * D_MAXGEOM * 17 + i];
        if (tid < D_MAXGEOM) s.gobj[tid] = -1;                          // every geom static: no dynamic slot
        if (tid == 0) { s.ngeom_static = ngs; s.ngeom = ngs; s.nobj = 0; }
    }
    KP_SYNC();
    if constexpr (OBJ) {
        if (ngs > 0) { invdyn_row<true>(s, A, r, tid); return; }
    }
    invdyn_row<false>(static_cast<EnvLds&>(s), A, r, tid);
}

}  // namespace kp
