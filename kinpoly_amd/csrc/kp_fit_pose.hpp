// kp_fit_pose.hpp -- point Jacobians and pose fitting on motion rows (kp_sim_point_jacobian, kp_sim_fit_pose).
//
// k_point_jacobian is mj_jac per ROW: the velocity of a point of a body and the body's angular velocity per unit dof velocity (qvel order: root
// translation in world axes, root rotation about the body axes, the 69 hinges).  It is the forward pass' motion axes read out: dof d moves body b iff
// d's body k carries b (bodies are in depth-first order: k <= b < k + subtree(k)), and then the column is [cdof_d.l + cdof_d.a x (r - o); cdof_d.a].
//
// k_fit_pose goes the other way, from body poses to qpos: damped Gauss-Newton (Levenberg-Marquardt) steps on
//     c(q) = 1/2 sum_b w_pos_b |x*_b - x_b|^2 + 1/2 sum_b w_rot_b |log(R*_b R_b^T)|^2 + 1/2 sum_d w_prior_d (q*_d - q_d)^2.
// No reference counterpart (the reference gets qpos from SMPL axis-angles offline).  The normal matrix J^T W J + diag(mu damp + w_prior) IS the
// joint-space inertia of the same tree when every body's inertia is a point mass w_pos_b at the body origin plus a spherical rotational inertia
// w_rot_b I_3 and the damping stands in for the armature.  So it has M's sparsity, and the step's matrix-free articulated-body pass solves it from
// s.cinert, s.cdof and s.extra: one iteration is one forward_kin_bias (at the trial point; an accepted trial's kinematics serve the next iteration),
// ten floats per body written into s.cinert, one project_body_wrenches for J^T W e, one aba_solve and one position update.  Built from the step's
// device functions like k_apply_impulse, compiled in the read-out unit (kp_readout.hip) only.
//
// Every loop has a trip count fixed by the arguments (n_iters, tree levels, 24, 75); no atomics, nothing shared between rows.  The accept decision is
// taken on wave_sum's result, which every lane holds alike (one v_readlane), so the branch is wave-uniform.  A row whose input or first cost is not
// finite runs no iteration and returns its input.
#pragma once
#include "kp_readout_device.hpp"

namespace kp {

// ------------------------------------------------------------------ k_point_jacobian
// The row's LDS block: the fields forward_kin_bias touches, the subtree sizes and the dof -> body map.  7 456 B = 6 allocation granules of 1 280 B.
struct __attribute__((aligned(16))) PointJacLds {
    float qpos[76], qvel[76];
    float xpos[72], xquat[96];
    float cinert[240];
    float cdof[450];
    float sv[144], sa[144];
    float fb[144];
    float U[384];                         // forward_kin_bias' scratch
    unsigned char bpar[D_NB], bdep[D_NB], bsub[D_NB], dbody[76];
};
static_assert(offsetof(PointJacLds, U) % 8 == 0, "s.U must be 8-byte aligned");
static_assert(sizeof(PointJacLds) == 7456 && sizeof(PointJacLds) <= 6 * 1280, "6 allocation granules");

// One wavefront per row: lane = dof (d, d + 64), six consecutive-lane stores per pass.
__global__ __launch_bounds__(64) void k_point_jacobian(PointJacArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    PointJacLds& s = *reinterpret_cast<PointJacLds*>(smem_raw);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    float* J = A.J + r * 6 * D_NV;
    const int b = A.body[r];                                             // wave-uniform
    if (b < 0 || b >= D_NB) {                                            // tested before it indexes anything
        for (int i = tid; i < 6 * D_NV; i += 64) J[i] = 0.f;
        return;
    }
    for (int i = tid; i < D_NQ; i += 64) s.qpos[i] = A.qpos[r * D_NQ + i];
    for (int i = tid; i < D_NV; i += 64) { s.qvel[i] = 0.f; s.dbody[i] = T.dof_body[i]; }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bdep[tid] = T.body_depth[tid]; s.bsub[tid] = T.body_subtree[tid]; }
    KP_SYNC();
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<64>(s, T, A.P, depth, bpos, tid);
    const V3 off = A.offset ? ld3(A.offset + r * 3) : v3(0.f, 0.f, 0.f);
    const V3 ro = ld3(s.xpos + 3 * b) + qrot(Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]}, off) - ld3(s.xpos);
    for (int d = tid; d < D_NV; d += 64) {
        const int k = s.dbody[d];
        const bool on = k <= b && b < k + (int)s.bsub[k];
        const S6 c = lds6(s.cdof + 6 * d);
        const V3 lin = c.l + cross(c.a, ro);
        J[d] = on ? lin.x : 0.f; J[D_NV + d] = on ? lin.y : 0.f; J[2 * D_NV + d] = on ? lin.z : 0.f;
        J[3 * D_NV + d] = on ? c.a.x : 0.f; J[4 * D_NV + d] = on ? c.a.y : 0.f; J[5 * D_NV + d] = on ? c.a.z : 0.f;
    }
}

// ------------------------------------------------------------------ k_fit_pose
// rotation vector of a unit quaternion with w >= 0 (the shortest arc): 2 atan2(|v|, w) v / |v|.  atan2 stays accurate up to pi (w -> 0), where an
// acos of w would not; below |v| = 1e-4 the factor 2 atan2(n, w) / n is its series 2 / w (1 - n^2 / (3 w^2)), exact to fp32 there.
__device__ __forceinline__ V3 quat_log(Q4 q) {
    const V3 v = v3(q.x, q.y, q.z);
    const float n2 = dot(v, v), n = sqrtf(n2);
    const float k = n < 1e-4f ? (2.0f / q.w) * (1.0f - n2 / (3.0f * q.w * q.w)) : 2.0f * atan2f(n, q.w) / n;
    return k * v;
}

// unit quaternion of a rotation vector (mju_quatIntegrate's increment); below 1e-4 rad the series of sin(a / 2) / a and cos(a / 2)
__device__ __forceinline__ Q4 quat_exp(V3 w) {
    const float a2 = dot(w, w), a = sqrtf(a2);
    float k, c;
    if (a < 1e-4f) { k = 0.5f - a2 * (1.0f / 48.0f); c = 1.0f - a2 * 0.125f; }
    else { float sn; sincosf(0.5f * a, &sn, &c); k = sn / a; }
    return Q4{c, k * w.x, k * w.y, k * w.z};
}

// Cost of the pose whose kinematics forward_kin_bias has just left in s, and the residuals of this lane's body (lane = body; zero elsewhere).
// The row's inputs sit in words of EnvLds that only a collision pass or a constraint would use: see k_fit_pose.
struct FitEval { float cost, epos, erot; V3 ep, er; };
__device__ __forceinline__ FitEval fit_eval(const EnvLds& s, const float* tpos, const float* tquat, const float* wpos, const float* wrot, const float* qpr, const float* wpr,
                                            bool prior, int tid) {
    FitEval E{0.f, 0.f, 0.f, v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
    float c = 0.f;
    if (tid < D_NB) {
        const int b = tid;
        const float wp = wpos[b], wr = wrot[b];
        E.ep = ld3(tpos + 3 * b) - ld3(s.xpos + 3 * b);
        // R* R_b^T as a quaternion: q* (x) conj(q_b), sign-fixed to the shortest arc
        const Q4 qt = Q4{tquat[4 * b], tquat[4 * b + 1], tquat[4 * b + 2], tquat[4 * b + 3]};
        Q4 qe = qmul(qt, Q4{s.xquat[4 * b], -s.xquat[4 * b + 1], -s.xquat[4 * b + 2], -s.xquat[4 * b + 3]});
        if (qe.w < 0.f) qe = Q4{-qe.w, -qe.x, -qe.y, -qe.z};
        E.er = quat_log(qe);
        const float p2 = dot(E.ep, E.ep), r2 = dot(E.er, E.er);
        c = 0.5f * wp * p2 + 0.5f * wr * r2;
        E.epos = wp > 0.f ? sqrtf(p2) : 0.f; E.erot = wr > 0.f ? sqrtf(r2) : 0.f;
    }
    if (prior)
        for (int j = tid; j < D_NU; j += 64) { const float e = qpr[j] - s.qpos[7 + j]; c += 0.5f * wpr[j] * e * e; }
    E.cost = wave_sum(c);
    E.epos = wave_max_f(E.epos); E.erot = wave_max_f(E.erot);
    return E;
}

// One wavefront per row, on EnvLds (8 rows per CU).
__global__ __launch_bounds__(64) void k_fit_pose(FitPoseArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EnvLds& s = *reinterpret_cast<EnvLds*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    const Params& P = A.P;
    // the row's inputs, in words no function called here touches (no collide, no make_constraint, no contact rows in the solve)
    float* tpos = s.con_pos;              // [72] target positions
    float* tquat = s.jar3;                // [96] target quaternions, normalised
    float* wpos = s.con_D;                // [24] position weights
    float* wrot = s.con_D + D_NB;         // [24] orientation weights
    float* qpr = s.lim_D;                 // [69] prior angles
    float* wpr = s.lim_jar;               // [69] prior weights
    float* damp = s.Mv;                   // [75] mu's scale per dof
    float* qcur = s.search;               // [76] the accepted pose (s.qpos: the pose forward_kin_bias last ran on)
    float* g = s.x;                       // [75] J^T W e + the prior's share
    float* dq = s.qacc_s;                 // [75] the step
    const bool prior = A.q_prior != nullptr;

    float bad = 0.f;
    for (int i = tid; i < D_NQ; i += NT) { const float v = A.qpos0[r * D_NQ + i]; s.qpos[i] = v; bad += isfinite(v) ? 0.f : 1.f; }
    for (int i = tid; i < D_NV; i += NT) { s.qvel[i] = 0.f; damp[i] = A.damp[i]; dq[i] = 0.f; }
    for (int i = tid; i < 3 * D_NB; i += NT) tpos[i] = A.tgt_pos[r * 72 + i];
    if (tid < D_NB) {
        const Q4 q = A.tgt_quat ? qnormalize(Q4{A.tgt_quat[r * 96 + 4 * tid], A.tgt_quat[r * 96 + 4 * tid + 1], A.tgt_quat[r * 96 + 4 * tid + 2], A.tgt_quat[r * 96 + 4 * tid + 3]})
                                : Q4{1.f, 0.f, 0.f, 0.f};
        tquat[4 * tid] = q.w; tquat[4 * tid + 1] = q.x; tquat[4 * tid + 2] = q.y; tquat[4 * tid + 3] = q.z;
        wpos[tid] = A.w_pos ? fmaxf(A.w_pos[r * D_NB + tid], 0.f) : 1.f;              // fmaxf(NaN, 0) = 0 would hide a NaN weight: counted below
        wrot[tid] = (A.w_rot && A.tgt_quat) ? fmaxf(A.w_rot[r * D_NB + tid], 0.f) : 0.f;
        if (A.w_pos && !isfinite(A.w_pos[r * D_NB + tid])) bad += 1.f;
        if (A.w_rot && A.tgt_quat && !isfinite(A.w_rot[r * D_NB + tid])) bad += 1.f;
    }
    for (int j = tid; j < D_NU; j += NT) {
        qpr[j] = prior ? A.q_prior[r * D_NU + j] : 0.f;
        wpr[j] = prior ? fmaxf(A.w_prior[r * D_NU + j], 0.f) : 0.f;
        if (prior && !isfinite(A.w_prior[r * D_NU + j])) bad += 1.f;
    }
    readout_prologue(s, T, tid);
    readout_aba_zeros(s, tid);
    for (int i = tid; i < D_NV; i += NT) s.arm[i] = 0.f;                 // the damping is the armature: all of it goes through s.extra
    KP_SYNC();
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
    for (int i = tid; i < D_NQ; i += NT) qcur[i] = s.qpos[i];            // root quaternion normalised by the forward pass
    FitEval E = fit_eval(s, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
    const float cost0 = E.cost;
    const bool ok = wave_sum(bad) == 0.f && isfinite(cost0);             // wave-uniform
    float mu = A.mu0, nacc = 0.f, dqmax = 0.f;
    const int n_iters = ok ? A.n_iters : 0;
#pragma nounroll
    for (int it = 0; it < n_iters; it++) {
        // J^T W e: body wrenches about o, subtree sums, projection on the motion axes; the pseudo-inertia of every body
        if (tid < D_NB) {
            const int b = tid;
            const float wp = wpos[b], wr = wrot[b];
            const V3 rr = ld3(s.xpos + 3 * b) - ld3(s.xpos);
            const V3 f = wp * E.ep;
            sts6(s.sw + 6 * b, S6{wr * E.er + cross(rr, f), f});
            const float r2 = dot(rr, rr);
            float* ci = s.cinert + 10 * b;
            ci[0] = wr + wp * (r2 - rr.x * rr.x); ci[1] = wr + wp * (r2 - rr.y * rr.y); ci[2] = wr + wp * (r2 - rr.z * rr.z);
            ci[3] = -wp * rr.x * rr.y; ci[4] = -wp * rr.x * rr.z; ci[5] = -wp * rr.y * rr.z;
            ci[6] = wp * rr.x; ci[7] = wp * rr.y; ci[8] = wp * rr.z; ci[9] = wp;
        }
        project_body_wrenches(s, g, tid);
        for (int d = tid; d < D_NV; d += NT) {
            float ex = mu * damp[d];
            if (d >= 6) { ex += wpr[d - 6]; g[d] += wpr[d - 6] * (qpr[d - 6] - s.qpos[1 + d]); }
            s.extra[d] = ex;
        }
        KP_SYNC();
        Lane8 L;
        L.init(tid, T.sched8);
        aba_solve<NT, false>(s, P, L, g, dq, false, tid);
        // trial q (+) dq: mj_integratePos with dt = 1
        float dm = 0.f;
        for (int d = tid; d < D_NV; d += NT) dm = fmaxf(dm, fabsf(dq[d]));
        dqmax = wave_max_f(dm);
        if (tid == 0) {
            st3(s.qpos, ld3(qcur) + ld3(dq));
            const Q4 qn = qmul(Q4{qcur[3], qcur[4], qcur[5], qcur[6]}, quat_exp(ld3(dq + 3)));
            s.qpos[3] = qn.w; s.qpos[4] = qn.x; s.qpos[5] = qn.y; s.qpos[6] = qn.z;
        }
        for (int j = tid; j < D_NU; j += NT) {
            float q = qcur[7 + j] + dq[6 + j];
            if (A.clamp_limits && T.jnt_limited[j]) q = fminf(fmaxf(q, T.jnt_lo[j]), T.jnt_hi[j]);
            s.qpos[7 + j] = q;
        }
        KP_SYNC();
        forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
        const FitEval Et = fit_eval(s, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
        if (isfinite(Et.cost) && Et.cost < E.cost) {                     // wave-uniform
            E = Et; nacc += 1.f;
            mu = fmaxf(mu * A.mu_down, A.mu_min);
            for (int i = tid; i < D_NQ; i += NT) qcur[i] = s.qpos[i];
            KP_SYNC();
        } else {
            mu = fminf(mu * A.mu_up, A.mu_max);
            for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = qcur[i];
            KP_SYNC();
            forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
        }
    }
    // a row that was refused returns its input as given
    for (int i = tid; i < D_NQ; i += NT) A.qpos[r * D_NQ + i] = ok ? qcur[i] : A.qpos0[r * D_NQ + i];
    if (A.dq) for (int d = tid; d < D_NV; d += NT) A.dq[r * D_NV + d] = dq[d];
    if (tid < 8) {
        const float v[8] = {cost0, E.cost, nacc, mu, E.epos, E.erot, dqmax, ok ? 0.f : 1.f};
        float o = v[0];
#pragma unroll
        for (int k = 1; k < 8; k++) o = tid == k ? v[k] : o;
        A.info[r * 8 + tid] = o;
    }
}

}  // namespace kp
