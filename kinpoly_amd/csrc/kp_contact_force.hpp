// kp_contact_force.hpp -- contact-force read-out (kp_sim_contact_forces).
//
// What `sim.forward()` followed by mj_contactForce / data.efc_force, data.cfrc_ext, data.qfrc_constraint, data.qacc and data.qfrc_actuator hands
// out in mujoco-py, for the stored state of every env: the mj_forward of substep 0 of the control step kp_sim_step_ctrl would run next, WITHOUT the
// integration.  The reference reads none of these (deviation list); the engine solved the same problem fifteen times per control
// step and kept only qpos / qvel.  Nothing of the control step changes: the kernel is composed from the step kernel's device functions the way
// kp_push.hpp is, reads the stored rows (and the warm start, read only) and stores into its own output rows alone.
// Always the full layouts (EnvLds / EnvLdsObj, 64 contact slots): no lean layout, so no overflow path.
// Compiled in the read-out unit (kp_readout.hip), which the step kernels' unit cannot see.
#pragma once
#include "kp_readout.hpp"
#include "kp_readout_device.hpp"

namespace kp {

constexpr int D_CF_ENTITIES = D_NB + D_MAXOBJ;      // 0..23 humanoid bodies, 24 + k object slot k (the numbering of kp_sim_contacts)
constexpr int D_CF_ROW = 12;                        // floats of a contact row: A, B, dist, pos[3], normal[3], force[3]

// con_force (kp_step_obj.hpp) for both layouts: the world force of contact c at the residuals in jar3, acting on the entity that carries
// the vertex (A).  Row forces fe = -D jar where jar < 0, frame components (sum fe, mu (fe0 - fe1), mu (fe2 - fe3)).
template <bool OBJ, class SL>
__device__ __forceinline__ V3 contact_force(const SL& s, const Params& P, int c) {
    const float Dc = s.con_D[c], jn = s.jar3[3 * c], jt1 = s.jar3[3 * c + 1], jt2 = s.jar3[3 * c + 2];
    float fe[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { const float x = row_val(e, P.mu, jn, jt1, jt2); fe[e] = x < 0.f ? -Dc * x : 0.f; }
    return frame_world(contact_frame<OBJ>(s, c), v3(fe[0] + fe[1] + fe[2] + fe[3], P.mu * (fe[0] - fe[1]), P.mu * (fe[2] - fe[3])));
}

// One wavefront per env.  actuation: 0 none, 1 torque (act [N, 75] = qfrc_applied[0:6] ++ ctrl[69], as given), 2 controller (act = cc_action rows, the
// torque of the step kernel's first substep).  mask [N] or null: a masked-out env gets zero rows and ncon = 0.
template <bool OBJ, bool XC>
__global__ __launch_bounds__(64) void k_contact_forces(StepArgs A, XcArgs X, int actuation, const float* __restrict__ act, const uint8_t* __restrict__ mask, ContactOut O) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using SL = typename std::conditional<OBJ, EnvLdsObj, EnvLds>::type;
    SL& s = *reinterpret_cast<SL*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x, env = blockIdx.x;
    if (env >= A.n_envs) return;
    const DevTables& T = A.T;
    const Params& P = A.P;
    const size_t e = (size_t)env;
    if (mask && !mask[env]) {
        if (O.ncon && tid == 0) O.ncon[e] = 0;
        if (O.contact) for (int i = tid; i < D_MAXCON * D_CF_ROW; i += NT) O.contact[e * D_MAXCON * D_CF_ROW + i] = 0.f;
        if (O.wrench) for (int i = tid; i < D_CF_ENTITIES * 6; i += NT) O.wrench[e * D_CF_ENTITIES * 6 + i] = 0.f;
        for (int i = tid; i < D_NV; i += NT) {
            if (O.qfrc_constraint) O.qfrc_constraint[e * D_NV + i] = 0.f;
            if (O.qacc) O.qacc[e * D_NV + i] = 0.f;
            if (O.torque) O.torque[e * D_NV + i] = 0.f;
        }
        if (O.obj_qacc && tid < 6 * D_MAXOBJ) O.obj_qacc[e * 6 * D_MAXOBJ + tid] = 0.f;
        return;
    }
    // the controller (mode 2) runs only where the control step runs it (model option actuation); without it the step's torque is zero
    const bool ctrl_on = actuation == 2 && P.actuation;
    const bool stale_ctrl = ctrl_on && P.stale;         // the controller sees the kinematics of the derived state (the last forward pass)
    const int stride = actuation == 2 ? (XC ? X.stride : D_NV) : D_NV;
    const float* act_row = (actuation != 0 && act) ? act + e * stride : nullptr;
    const float* tq_row = A.target_qpos ? A.target_qpos + e * D_NQ : nullptr;

    // ---- load, as step_body does: derived state first when the stale controller needs it, else the stored state
    for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = (stale_ctrl ? A.qpos_d : A.qpos)[e * D_NQ + i];
    for (int i = tid; i < D_NV; i += NT) {
        s.qvel[i] = (stale_ctrl ? A.qvel_d : A.qvel)[e * D_NV + i];
        s.qacc[i] = A.warm[e * D_NV + i];                // the warm start, read only; no extrapolation (beta = 0): the minimiser does not depend on the start
    }
    readout_prologue(s, T, tid);
    readout_aba_zeros(s, tid);
    if constexpr (OBJ) {
        for (int i = tid; i < D_MAXGEOM * 17; i += NT) s.geom[i] = A.geoms[e * D_MAXGEOM * 17 + i];
        if (tid < D_MAXGEOM) s.gobj[tid] = -1;
        const int ngs = A.ngeom[env];
        int nobj = 0, ng = ngs;
        for (int k = 0; k < D_MAXOBJ; k++) {
            const int oi = A.obj_slot ? A.obj_slot[e * D_MAXOBJ + k] : -1;
            if (oi < 0 || oi >= T.n_obj) break;
            nobj = k + 1;
            if (tid < 7) s.oq[7 * k + tid] = A.obj_qpos[e * 35 + 7 * oi + tid];
            if (tid < 6) { s.ov[6 * k + tid] = A.obj_qvel[e * 30 + 6 * oi + tid]; s.oqa[6 * k + tid] = A.obj_warm[e * 6 * D_MAXOBJ + 6 * k + tid]; s.oqa_prev[6 * k + tid] = 0.f; }
            if (tid < 13) s.oc[13 * k + tid] = T.obj_inertial[13 * oi + tid];
            for (int gi = T.obj_geom_adr[oi]; gi < T.obj_geom_adr[oi + 1] && ng < D_MAXGEOM; gi++, ng++) {
                if (tid == 0) { s.gobj[ng] = (signed char)k; s.ggi[ng] = (unsigned char)gi; }
            }
        }
        if (tid == 0) { s.ngeom_static = ngs; s.ngeom = ng; s.nobj = nobj; }
    }
    if (actuation == 1 && act_row) for (int i = tid; i < D_NV; i += NT) s.applied[i] = act_row[i];      // as given, no clipping
    KP_SYNC();

    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    // Pass 0 (stale controller only) is step_body's entry pass: forward pass on the derived state, then the stored state and the stable-PD torque on those
    // kinematics.  Pass 1 is the forward pass of substep 0.  One loop: one inlined copy of the forward pass for every mode.
    for (int pass = stale_ctrl ? 0 : 1; pass < 2; pass++) {
        forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
        if (pass == 0) {
            for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = A.qpos[e * D_NQ + i];
            for (int i = tid; i < D_NV; i += NT) s.qvel[i] = A.qvel[e * D_NV + i];
            KP_SYNC();
            Lane8 La; La.init(tid, T.sched8);
            spd_torque_rfc<NT, OBJ, SL, XC>(s, T, P, La, tid, tq_row, act_row, &X, 0);
        }
    }
    if constexpr (OBJ) obj_forward(s, T, P, tid);
    collide<NT, OBJ>(s, T, P, tid);
    const int ncon = s.ncon;                                            // <= SL::MAXCON = 64: one contact per lane below
    const float my_dist = tid < ncon ? s.con_D[tid] : 0.f;              // con_D holds the distance until make_constraint
    make_constraint<NT, OBJ>(s, T, P, tid);
    if (ctrl_on && !P.stale) { Lane8 La; La.init(tid, T.sched8); spd_torque_rfc<NT, OBJ, SL, XC>(s, T, P, La, tid, tq_row, act_row, &X, 0); }
    for (int i = tid; i < D_NV; i += NT) s.extra[i] = 0.f;
    KP_SYNC();
    Lane8 L8; L8.init(tid, T.sched8);
    int nfact = 0, ncap = 0;
    if constexpr (OBJ) solve_constraints_obj<NT>(s, P, L8, depth, tid, nfact, ncap, s.arm);
    else solve_constraints_direct<NT>(s, P, L8, depth, tid, nfact, ncap, s.arm);
    KP_SYNC();

    // ---- force pass.  jar3 / lim_jar hold J qacc - aref of the FINAL iterate: the solvers evaluate them at the start (eval_rows with sub_aref on the warm
    // start) and keep them current with the same step as qacc (`s.jar3[k] += alpha * s.jv3[k]`, `s.lim_jar[j] += alpha * s.lim_jv[j]` right behind
    // `s.qacc[i] += alpha * s.search[i]`); every exit of the iteration lies before the update or behind both.  Without rows (ncon == 0 && nlim == 0) the
    // solvers return before any of it: all forces are zero there and qacc is the plain solve.
    const bool rows = ncon != 0 || s.nlim != 0;
    float* fc = s.jv3;                                                  // [ncon][3] world force on A (J search is dead behind the solve)
    if (rows) {
        if (tid < ncon) st3(fc + 3 * tid, contact_force<OBJ>(s, P, tid));
        KP_SYNC();
        project_contact_forces(s, fc, s.x, tid);                        // qfrc_constraint
    }
    if (O.ncon && tid == 0) O.ncon[e] = ncon;
    if (O.contact) {
        float* row = O.contact + (e * D_MAXCON + tid) * D_CF_ROW;
        if (tid < ncon) {
            int B = -1;
            V3 n = v3(0.f, 0.f, 1.f);
            if constexpr (OBJ) { const int b2 = s.con_b2[tid]; B = b2 < 0 ? -1 : b2; n = ld3(s.con_n + 3 * tid); }
            const V3 f = rows ? ld3(fc + 3 * tid) : v3(0.f, 0.f, 0.f);
            row[0] = (float)s.con_body[tid]; row[1] = (float)B; row[2] = my_dist;
            st3(row + 3, ld3(s.con_pos + 3 * tid)); st3(row + 6, n); st3(row + 9, f);
        } else {
#pragma unroll
            for (int k = 0; k < D_CF_ROW; k++) row[k] = 0.f;
        }
    }
    if (O.wrench && tid < D_CF_ENTITIES) {
        // lane = entity; the contacts in stored order: one summation order, no atomics.  + where the entity carries the vertex (A), - where it is the
        // object slot that carries the surface (B); floor and static geoms receive nothing
        V3 F = v3(0.f, 0.f, 0.f), M = v3(0.f, 0.f, 0.f);
        for (int c = 0; rows && c < ncon; c++) {
            float sg = (int)s.con_body[c] == tid ? 1.f : 0.f;
            if constexpr (OBJ) { if (tid >= D_NB && (int)s.con_b2[c] == tid) sg = -1.f; }
            if (sg == 0.f) continue;
            const V3 f = sg * ld3(fc + 3 * c);
            F = F + f; M = M + cross(ld3(s.con_pos + 3 * c), f);
        }
        float* w = O.wrench + (e * D_CF_ENTITIES + tid) * 6;
        st3(w, F); st3(w + 3, M);
    }
    for (int i = tid; i < D_NV; i += NT) {
        if (O.qfrc_constraint) O.qfrc_constraint[e * D_NV + i] = rows ? s.x[i] : 0.f;
        if (O.qacc) O.qacc[e * D_NV + i] = s.qacc[i];
        if (O.torque) O.torque[e * D_NV + i] = s.applied[i];
    }
    if (O.obj_qacc && tid < D_MAXOBJ) {
        float* q = O.obj_qacc + (e * D_MAXOBJ + tid) * 6;
        S6 out = S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
        if constexpr (OBJ) {
            if (tid < s.nobj) {                                         // spatial (about o) -> joint coordinates, as obj_integrate does
                const float* R = s.oR + 9 * tid;
                const S6 a = lds6(s.oa + 6 * tid);
                const V3 ra = ld3(s.oq + 7 * tid) - ld3(s.xpos);
                out.a = a.l + cross(a.a, ra);
                out.l = v3(R[0] * a.a.x + R[3] * a.a.y + R[6] * a.a.z, R[1] * a.a.x + R[4] * a.a.y + R[7] * a.a.z, R[2] * a.a.x + R[5] * a.a.y + R[8] * a.a.z);
            }
        }
        st3(q, out.a); st3(q + 3, out.l);
    }
}

}  // namespace kp
