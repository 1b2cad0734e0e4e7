// kp_body_motion.hpp -- body velocities and accelerations, momentum and energy on motion rows (kp_sim_body_motion).
//
// What a mujoco-py user reads from data.body_xvelp / body_xvelr, mj_objectAcceleration, data.subtree_com / subtree_linvel / subtree_angmom of the root
// and mj_energyPos / mj_energyVel, per ROW of a motion (qpos, qvel, qacc).  The reference never reads them (deviation list).  All of it
// is in what forward_kin_bias leaves behind: the bodies' spatial velocities s.sv, the velocity-product accelerations s.sa (with the -g seed of the
// Newton-Euler trick), the inertias about the root s.cinert and the bias wrenches s.fb = I a + v x* I v.  So the kernel is the forward pass, one
// spatial_accumulate of the given qacc where an acceleration is asked for, and the read-out: no collide, no make_constraint, no solve, a smooth
// function of its inputs.  A rows API like kp_sim_fk: it reads the model tables and the row inputs only, and stores into its own output rows alone.
//
// Frames.  Every spatial vector is [ang; lin] in world axes about the point O that coincides with the root body's origin o at this instant and stays
// where it is (the root's seed sa_0.l = -g + v x w is what makes sa a derivative in that fixed frame although o itself moves).  With V = (w, v_O) and
// A = dV/dt = (alpha, a_O) of a body, a point p fixed on it, r = p - o:
//     velocity      v_p = v_O + w x r
//     acceleration  a_p = a_O + alpha x r + w x v_p            (mj_objectAcceleration's correction; a_O = (sa + sum_j qacc_j cdof_j).l + g)
// Momentum about O: H = sum_b I_b V_b (I_b: cinert), H.l = m com_vel, L_com = H.a - c x H.l with c = com - o = sum_b h_b / m.  Its rate in the fixed
// frame is sum_b (I_b A_b + V_b x* I_b V_b); with W = sum_b (fb_b + I_b (sum_j qacc_j cdof_j)_b), which lacks I_b (0, g) = (h_b x g, m_b g) per body,
//     com_acc = W.l / m + g,     Ldot_com = W.a - c x W.l                                 (gravity cancels in the second)
// With qacc = NULL (zeros) both are the acceleration-free part: what the velocity products and gravity's seed alone give.
// ke = 1/2 sum_b V_b . I_b V_b + 1/2 sum_d armature_d qvel_d^2 (mj_energyVel: 1/2 qvel^T M qvel); pe = -m g . com (mj_energyPos).
//
// Sums over the 24 bodies and the 75 dofs: lane = body (dofs: lane, lane + 64), then wave_sum's fixed DPP pattern; no atomics, so a row's result
// depends on the row alone.  Outputs are staged in LDS and stored with consecutive lanes.
// Compiled in the read-out unit (kp_readout.hip) only.  The load section has the per-lane table stores fused into the row loads, like
// k_inverse_dynamics and for the reason its header gives.
#pragma once
#include "kp_readout.hpp"

namespace kp {

// The row's LDS block: the fields forward_kin_bias and spatial_accumulate touch, the armature (ke), the staging area and nothing else (no subtree
// sizes and no dof -> body map: nothing here sums over subtrees or projects on the dofs; the sums are wave_sum's, which needs no LDS words).
// 10 080 B = 8 allocation granules of 1 280 B: 16 rows per CU (EnvLds: 8).
struct __attribute__((aligned(16))) BodyMotionLds {
    float qpos[76], qvel[76], qacc[76];
    float xpos[72], xquat[96];
    float cinert[240];
    float cdof[450];
    float sv[144], sa[144];
    float fb[144];
    float U[384];                         // forward_kin_bias' scratch: [0, 138) half-angle sin / cos, [144, 384) joint frames
    float arm[76];
    float sacc[144];                      // spatial_accumulate(qacc)
    float stage[384];                     // body_vel [144] | body_acc [144] | body_com_vel [72] | centroid [18]
    unsigned char bpar[D_NB], bdep[D_NB];
};
static_assert(offsetof(BodyMotionLds, U) % 8 == 0, "s.U must be 8-byte aligned");
static_assert(sizeof(BodyMotionLds) == 10080 && sizeof(BodyMotionLds) <= 8 * 1280, "16 rows per CU");

// One wavefront per row.
__global__ __launch_bounds__(64) void k_body_motion(BodyMotionArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    BodyMotionLds& s = *reinterpret_cast<BodyMotionLds*>(smem_raw);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    const Params& P = A.P;
    const BodyMotionOut& O = A.O;
    for (int i = tid; i < D_NQ; i += 64) s.qpos[i] = A.qpos[r * D_NQ + i];
    for (int i = tid; i < D_NV; i += 64) {
        s.qvel[i] = A.qvel ? A.qvel[r * D_NV + i] : 0.f;
        s.qacc[i] = A.qacc ? A.qacc[r * D_NV + i] : 0.f;
        s.arm[i] = T.dof_armature[i];
    }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bdep[tid] = T.body_depth[tid]; }
    KP_SYNC();
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<64>(s, T, P, depth, bpos, tid);
    const bool want_acc = O.body_acc || O.centroid;                     // wave-uniform
    if (want_acc) spatial_accumulate<64>(s, s.qacc, depth, tid, s.sacc);

    float* st_vel = s.stage; float* st_acc = s.stage + 144; float* st_cv = s.stage + 288; float* st_cen = s.stage + 360;
    const V3 g = v3(P.gx, P.gy, P.gz);
    const V3 o = ld3(s.xpos);
    // per body (lane = body; the other lanes carry zeros into the sums)
    float mass = 0.f, ke = 0.f;
    V3 h = v3(0.f, 0.f, 0.f);
    S6 H = S6{h, h}, W = H;
    if (tid < D_NB) {
        const int b = tid;
        const float* ci = s.cinert + 10 * b;
        const S6 cv = lds6(s.sv + 6 * b);
        const V3 rb = ld3(s.xpos + 3 * b) - o;
        const V3 vb = cv.l + cross(cv.a, rb);
        sts6(st_vel + 6 * b, S6{cv.a, vb});
        const Q4 q = Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]};
        st3(st_cv + 3 * b, cv.l + cross(cv.a, rb + qrot(q, ld3(T.body_ipos + 3 * b))));
        mass = ci[9]; h = ld3(ci + 6);
        H = inert_mul(ci, cv);
        ke = 0.5f * dot6(cv, H);
        if (want_acc) {
            const S6 qa = lds6(s.sacc + 6 * b);
            const S6 ca = lds6(s.sa + 6 * b) + qa;
            sts6(st_acc + 6 * b, S6{ca.a, ca.l + g + cross(ca.a, rb) + cross(cv.a, vb)});
            W = lds6(s.fb + 6 * b) + inert_mul(ci, qa);
        }
    }
    if (O.centroid) {                                                   // wave-uniform: every lane takes part in the sums
        for (int d = tid; d < D_NV; d += 64) ke += 0.5f * s.arm[d] * s.qvel[d] * s.qvel[d];
        const float m = wave_sum(mass);
        ke = wave_sum(ke);
        h = v3(wave_sum(h.x), wave_sum(h.y), wave_sum(h.z));
        H = S6{v3(wave_sum(H.a.x), wave_sum(H.a.y), wave_sum(H.a.z)), v3(wave_sum(H.l.x), wave_sum(H.l.y), wave_sum(H.l.z))};
        W = S6{v3(wave_sum(W.a.x), wave_sum(W.a.y), wave_sum(W.a.z)), v3(wave_sum(W.l.x), wave_sum(W.l.y), wave_sum(W.l.z))};
        if (tid == 0) {
            const float im = 1.0f / m;
            const V3 c = im * h, com = o + c;
            st3(st_cen, com); st3(st_cen + 3, im * H.l); st3(st_cen + 6, H.a - cross(c, H.l));
            st_cen[9] = ke; st_cen[10] = -m * dot(g, com);
            st3(st_cen + 11, im * W.l + g); st3(st_cen + 14, W.a - cross(c, W.l));
            st_cen[17] = m;
        }
    }
    KP_SYNC();
    // ---- outputs: consecutive lanes, consecutive words
    if (O.body_vel) for (int i = tid; i < 144; i += 64) O.body_vel[r * 144 + i] = st_vel[i];
    if (O.body_acc) for (int i = tid; i < 144; i += 64) O.body_acc[r * 144 + i] = st_acc[i];
    if (O.body_com_vel) for (int i = tid; i < 72; i += 64) O.body_com_vel[r * 72 + i] = st_cv[i];
    if (O.centroid && tid < 18) O.centroid[r * 18 + tid] = st_cen[tid];
}

}  // namespace kp
