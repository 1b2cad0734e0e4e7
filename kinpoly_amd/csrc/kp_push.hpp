// kp_push.hpp -- impulse pushes between control steps (kp_sim_apply_impulse).
//
// A push is a velocity jump at a control-step boundary, qvel += M(qpos)^-1 J_b(r)^T [p; l]: the linear impulse p (N s) acts at the
// point r of body b, the angular impulse l (N m s) on the body, both in world axes.  No reference counterpart (the reference has no
// perturbation path); it is what `data.qvel[:75] += dv` between two env.step calls does in mujoco-py, with dv worked out here.
// Nothing of the control step changes: the kernel reads and writes the stored rows (KP_QPOS, KP_QVEL, KP_OBJ_QPOS, KP_OBJ_QVEL) and
// is built from the step kernel's device functions -- forward_kin_bias for the kinematics at the CURRENT qpos (not the stale
// qpos_d the read-outs belong to) and the matrix-free aba_solve with the model's armature and no contact rows for M^-1.
// Compiled in the read-out unit (kp_readout.hip), which the step kernels' unit cannot see.
#pragma once
#include "kp_readout_device.hpp"

namespace kp {

constexpr int D_PUSH_ENTITIES = D_NB + D_MAXOBJ;     // 0..23 humanoid bodies, 24 + k object slot k (the numbering of kp_sim_contacts)

// M_obj^-1 g of one free object, one lane: M_obj as the oracle's kpo_obj_forward forms it (dofs = 3 world translations of the body
// origin, 3 rotations about the body axes; the free joint's armature on the diagonal), Cholesky, two triangular solves.
__device__ __forceinline__ void obj_impulse(const float* __restrict__ C, const float* __restrict__ q, V3 off, V3 p, V3 l, float* dv) {
    const Q4 qq = qnormalize(Q4{q[3], q[4], q[5], q[6]});
    float R[9];
    q2mat(qq, R);
    const float mass = C[0], arm = C[12];
    const V3 r = mulmat(R, ld3(C + 1));                      // com - body origin, world axes
    const float I3[9] = {C[4], C[7], C[8], C[7], C[5], C[9], C[8], C[9], C[6]};
    float Tm[9], W[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Tm[3 * i + j] = R[3 * i] * I3[j] + R[3 * i + 1] * I3[3 + j] + R[3 * i + 2] * I3[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) W[3 * i + j] = Tm[3 * i] * R[3 * j] + Tm[3 * i + 1] * R[3 * j + 1] + Tm[3 * i + 2] * R[3 * j + 2];
    // velocity Jacobians of (com velocity, angular velocity) w.r.t. the 6 dofs, and the generalised impulse g = J(r_push)^T [p; l]
    float Jv[3][6], Jw[3][6], g[6], M[6][6];
    const V3 rp = mulmat(R, off);                             // push point - body origin, world axes
    const V3 tq = l + cross(rp, p);                           // angular impulse about the body origin
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int j = 0; j < 6; j++) { Jv[a][j] = 0.f; Jw[a][j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Jv[j][j] = 1.f;
        const V3 ax = v3(R[j], R[3 + j], R[6 + j]), axr = cross(ax, r);
        Jv[0][3 + j] = axr.x; Jv[1][3 + j] = axr.y; Jv[2][3 + j] = axr.z;
        Jw[0][3 + j] = ax.x; Jw[1][3 + j] = ax.y; Jw[2][3 + j] = ax.z;
        g[3 + j] = dot(ax, tq);
    }
    g[0] = p.x; g[1] = p.y; g[2] = p.z;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            float v = 0.f;
#pragma unroll
            for (int a = 0; a < 3; a++) v += mass * Jv[a][i] * Jv[a][j];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) v += Jw[a][i] * W[3 * a + b] * Jw[b][j];
            M[i][j] = v + (i == j ? arm : 0.f);
        }
    // M = L L^T in place (lower triangle), then L y = g, L^T dv = y
#pragma unroll
    for (int j = 0; j < 6; j++) {
        float d = M[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= M[j][k] * M[j][k];
        const float Ljj = sqrtf(d), inv = 1.0f / Ljj;
        M[j][j] = Ljj;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            float v = M[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= M[i][k] * M[j][k];
            M[i][j] = v * inv;
        }
    }
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        float v = g[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= M[i][k] * y[k];
        y[i] = v / M[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        float v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= M[k][i] * dv[k];
        dv[i] = v / M[i][i];
    }
}

// One wavefront per env.  entity [N] (0..23 body, 24 + k object slot, anything else: no push), offset [N,3] or null (the entity's frame
// origin), impulse [N,6] = (p, l), mask [N] or null, dqvel [N,75] or null (the humanoid's velocity jump; zero rows for object pushes
// and envs without a push).  A.obj_slot is null on a handle whose objects are not simulated.  An env whose impulse is exactly zero
// stores nothing, so that its rows stay bit for bit.
__global__ __launch_bounds__(64) void k_apply_impulse(StepArgs A, const int32_t* __restrict__ entity, const float* __restrict__ offset, const float* __restrict__ impulse,
                                                      const uint8_t* __restrict__ mask, float* __restrict__ dqvel) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EnvLds& s = *reinterpret_cast<EnvLds*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x, env = blockIdx.x;
    if (env >= A.n_envs) return;
    const DevTables& T = A.T;
    const Params& P = A.P;
    // wave-uniform decisions: every lane reads the same words
    const int ent = entity[env];
    const V3 p = ld3(impulse + (size_t)env * 6), l = ld3(impulse + (size_t)env * 6 + 3);
    const V3 off = offset ? ld3(offset + (size_t)env * 3) : v3(0.f, 0.f, 0.f);
    const bool zero = p.x == 0.f && p.y == 0.f && p.z == 0.f && l.x == 0.f && l.y == 0.f && l.z == 0.f;
    const bool live = (!mask || mask[env]) && ent >= 0 && ent < D_PUSH_ENTITIES && !zero;
    const bool body = live && ent < D_NB;
    if (dqvel && !body) for (int d = tid; d < D_NV; d += NT) dqvel[(size_t)env * D_NV + d] = 0.f;
    if (!live) return;
    if (!body) {
        // object slot k: simulated only when slots 0..k of the env all hold an object of the model (the step kernel's own rule)
        const int k = ent - D_NB;
        if (!A.obj_slot || !T.obj_inertial) return;
        int oi = -1;
        for (int j = 0; j <= k; j++) {
            oi = A.obj_slot[(size_t)env * D_MAXOBJ + j];
            if (oi < 0 || oi >= T.n_obj || oi >= 5) return;
        }
        if (tid == 0) {
            float dv[6];
            obj_impulse(T.obj_inertial + 13 * oi, A.obj_qpos + (size_t)env * 35 + 7 * oi, off, p, l, dv);
            float* v = A.obj_qvel + (size_t)env * 30 + 6 * oi;
#pragma unroll
            for (int i = 0; i < 6; i++) v[i] += dv[i];
        }
        return;
    }
    // ---- humanoid body `ent`: kinematics at the current qpos
    const int depth = tid < D_NB ? T.body_depth[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = A.qpos[(size_t)env * D_NQ + i];
    for (int i = tid; i < D_NV; i += NT) s.qvel[i] = A.qvel[(size_t)env * D_NV + i];
    readout_prologue(s, T, tid);
    readout_aba_zeros(s, tid);
    KP_SYNC();
    forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
    // g = J_b(r)^T [p; l]: the impulse as a wrench about o (the root body origin, where every spatial quantity of the env is expressed),
    // projected on the motion axes of the dofs that carry body `ent`.  Bodies are in depth-first order, so body k carries it iff
    // k <= ent < k + subtree(k): one dot product per lane and dof, no reduction.
    const V3 r = ld3(s.xpos + 3 * ent) + qrot(Q4{s.xquat[4 * ent], s.xquat[4 * ent + 1], s.xquat[4 * ent + 2], s.xquat[4 * ent + 3]}, off);
    const S6 w = S6{l + cross(r - ld3(s.xpos), p), p};
    for (int d = tid; d < D_NV; d += NT) {
        const int k = s.dbody[d];
        s.x[d] = (k <= ent && ent < k + (int)s.bsub[k]) ? dot6(lds6(s.cdof + 6 * d), w) : 0.f;
    }
    KP_SYNC();
    // dv = M^-1 g: no contact rows, no extra armature, every tree level
    Lane8 L;
    L.init(tid, T.sched8);
    aba_solve<NT, false>(s, P, L, s.x, s.qacc_s, false, tid);
    for (int d = tid; d < D_NV; d += NT) {
        const float dv = s.qacc_s[d];
        A.qvel[(size_t)env * D_NV + d] = s.qvel[d] + dv;
        if (dqvel) dqvel[(size_t)env * D_NV + d] = dv;
    }
}

}  // namespace kp
