// kp_fit_points.hpp -- pose fitting to points at body offsets, with a floor that holds (kp_sim_fit_points).
//
// k_fit_points is k_fit_pose (kp_fit_pose.hpp, section 17) with two more sums in the cost:
//     c(q) = c_fit(q) + 1/2 sum_k w_k |t_k - (x_b(k) + R_b(k) o_k)|^2 + 1/2 w_floor sum_v min(0, z_v - floor_z)^2
// over K points rigidly attached to bodies (markers, key points, end-effector targets) and over every hull vertex v of every body.  A weighted point p of
// body b is a POINT MASS w at p: sum_k w_k J_k^T J_k is still the joint-space inertia of the same tree, and only the ten s.cinert floats of a body change
// (mass, first and second moment of its points about the root origin o).  A hull vertex below the floor is such a point as well, with its own projection
// on the plane as the target, re-projected at every evaluation; in the MATRIX it counts as an isotropic point mass w_floor (a majoriser of the
// point-to-plane block: w I >= w n n^T), in the GRADIENT exactly (e = (0, 0, floor_z - z_v)).  The accept test runs on the true cost, so descent stays
// monotone.  The iteration, q (+) dq, clamp_limits, the accept rule and the mu schedule are k_fit_pose's.
//
// The marker set is one table for all rows, validated and ordered by body on the host (kp_sim.hip): offsets [K, 3] in that order, the permutation back
// to the caller's order and adr[25], so lane b walks points adr[b] .. adr[b + 1] and no device value is ever used as an index unchecked.  Lane = body:
// the lane adds its body's origin term, its points in the table's order and its hull's vertices in the blob's order into registers (wrench about o,
// the ten inertia floats, cost) -- no atomics, an order that depends on the marker set alone.  A point with w <= 0 and a vertex above the floor are
// skipped by a branch, not by a zero factor: their targets are not read, and the sums hold the same bits as without them.  The per-row targets and
// weights stay in HBM and are re-read at every evaluation (K x 16 B); the row's other inputs sit where k_fit_pose keeps them.
//
// Every loop has a trip count fixed by the arguments (n_iters, K through adr, the vertex table, tree levels, 24, 75); the loops over points and vertices
// hold no barrier, so lanes may leave them apart.  Every branch around a barrier is taken on a wave_sum / wave_max result (wave-uniform).  Nothing is
// shared between rows.  A row whose input or first cost is not finite runs no iteration and returns its input.
#pragma once
#include "kp_fit_pose.hpp"

namespace kp {

// what a lane has summed for its body: the wrench about o, the pseudo-inertia (s.cinert's layout) and the lane's share of the cost
struct PtSum { S6 W; float ci[10]; float c; };

// a point mass w at rr (from o) with the residual e
__device__ __forceinline__ void pt_add(PtSum& A, V3 rr, V3 e, float w) {
    const V3 f = w * e;
    A.W.a = A.W.a + cross(rr, f); A.W.l = A.W.l + f;
    const float r2 = dot(rr, rr);
    A.ci[0] += w * (r2 - rr.x * rr.x); A.ci[1] += w * (r2 - rr.y * rr.y); A.ci[2] += w * (r2 - rr.z * rr.z);
    A.ci[3] -= w * rr.x * rr.y; A.ci[4] -= w * rr.x * rr.z; A.ci[5] -= w * rr.y * rr.z;
    A.ci[6] += w * rr.x; A.ci[7] += w * rr.y; A.ci[8] += w * rr.z; A.ci[9] += w;
    A.c += 0.5f * w * dot(e, e);
}

struct PtEval { float cost, epos, erot; PtSum S; };

// Cost of the pose whose kinematics forward_kin_bias has just left in s, and this lane's body sums (lane = body; zero elsewhere).
__device__ __forceinline__ PtEval fit_points_eval(const EnvLds& s, const FitPointsArgs& A, size_t r, const float* tpos, const float* tquat, const float* wpos, const float* wrot,
                                                  const float* qpr, const float* wpr, bool prior, int tid) {
    PtEval E;
    E.epos = 0.f; E.erot = 0.f;
    E.S.W = S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
#pragma unroll
    for (int i = 0; i < 10; i++) E.S.ci[i] = 0.f;
    E.S.c = 0.f;
    if (tid < D_NB) {
        const int b = tid;
        const V3 o = ld3(s.xpos), xb = ld3(s.xpos + 3 * b);
        const Q4 qb = Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]};
        // the body origin and orientation: k_fit_pose's terms
        const float wp = wpos[b], wr = wrot[b];
        const V3 ep = ld3(tpos + 3 * b) - xb;
        const Q4 qt = Q4{tquat[4 * b], tquat[4 * b + 1], tquat[4 * b + 2], tquat[4 * b + 3]};
        Q4 qe = qmul(qt, Q4{qb.w, -qb.x, -qb.y, -qb.z});
        if (qe.w < 0.f) qe = Q4{-qe.w, -qe.x, -qe.y, -qe.z};
        const V3 er = quat_log(qe);
        pt_add(E.S, xb - o, ep, wp);
        E.S.W.a = E.S.W.a + wr * er;
        E.S.ci[0] += wr; E.S.ci[1] += wr; E.S.ci[2] += wr;
        const float r2 = dot(er, er);
        E.S.c += 0.5f * wr * r2;
        E.epos = wp > 0.f ? sqrtf(dot(ep, ep)) : 0.f; E.erot = wr > 0.f ? sqrtf(r2) : 0.f;
        // the body's points, in the table's order
        const int j1 = A.pt_adr[b + 1];
        for (int j = A.pt_adr[b]; j < j1; j++) {
            const size_t k = r * (size_t)A.n_points + (size_t)A.pt_perm[j];
            const float w = A.pt_w ? A.pt_w[k] : 1.f;
            if (w > 0.f) {
                const V3 p = xb + qrot(qb, ld3(A.pt_off + 3 * j));
                pt_add(E.S, p - o, ld3(A.pt_tgt + 3 * k) - p, w);
            }
        }
        // the hull's vertices below the floor, each pulled to its own projection on the plane
        if (A.w_floor > 0.f) {
            const int v1 = A.T.vert_adr[b + 1];
            for (int v = A.T.vert_adr[b]; v < v1; v++) {
                const V3 p = xb + qrot(qb, ld3(A.T.verts + 3 * v));
                const float d = A.floor_z - p.z;
                if (d > 0.f) pt_add(E.S, p - o, v3(0.f, 0.f, d), A.w_floor);
            }
        }
    }
    float c = E.S.c;
    if (prior)
        for (int j = tid; j < D_NU; j += 64) { const float e = qpr[j] - s.qpos[7 + j]; c += 0.5f * wpr[j] * e * e; }
    E.cost = wave_sum(c);
    E.epos = wave_max_f(E.epos); E.erot = wave_max_f(E.erot);
    return E;
}

// One wavefront per row, on EnvLds (8 rows per CU).
__global__ __launch_bounds__(64) void k_fit_points(FitPointsArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EnvLds& s = *reinterpret_cast<EnvLds*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    const Params& P = A.P;
    const int K = A.n_points;
    // the row's inputs, in the words k_fit_pose keeps them in
    float* tpos = s.con_pos;              // [72] target positions of the body origins (zero without tgt_pos)
    float* tquat = s.jar3;                // [96] target quaternions, normalised
    float* wpos = s.con_D;                // [24] position weights (zero without tgt_pos)
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
    for (int i = tid; i < 3 * D_NB; i += NT) tpos[i] = A.tgt_pos ? A.tgt_pos[r * 72 + i] : 0.f;
    if (tid < D_NB) {
        const Q4 q = A.tgt_quat ? qnormalize(Q4{A.tgt_quat[r * 96 + 4 * tid], A.tgt_quat[r * 96 + 4 * tid + 1], A.tgt_quat[r * 96 + 4 * tid + 2], A.tgt_quat[r * 96 + 4 * tid + 3]})
                                : Q4{1.f, 0.f, 0.f, 0.f};
        tquat[4 * tid] = q.w; tquat[4 * tid + 1] = q.x; tquat[4 * tid + 2] = q.y; tquat[4 * tid + 3] = q.z;
        wpos[tid] = !A.tgt_pos ? 0.f : A.w_pos ? fmaxf(A.w_pos[r * D_NB + tid], 0.f) : 1.f;
        wrot[tid] = (A.w_rot && A.tgt_quat) ? fmaxf(A.w_rot[r * D_NB + tid], 0.f) : 0.f;
        if (A.tgt_pos && A.w_pos && !isfinite(A.w_pos[r * D_NB + tid])) bad += 1.f;
        if (A.w_rot && A.tgt_quat && !isfinite(A.w_rot[r * D_NB + tid])) bad += 1.f;
    }
    for (int j = tid; j < D_NU; j += NT) {
        qpr[j] = prior ? A.q_prior[r * D_NU + j] : 0.f;
        wpr[j] = prior ? fmaxf(A.w_prior[r * D_NU + j], 0.f) : 0.f;
        if (prior && !isfinite(A.w_prior[r * D_NU + j])) bad += 1.f;
    }
    // the row's points: a NaN weight, or a target that is not finite under a positive weight, refuses the row; a skipped point's target is not read
    for (int k = tid; k < K; k += NT) {
        const size_t i = r * (size_t)K + k;
        const float w = A.pt_w ? A.pt_w[i] : 1.f;
        if (w != w) bad += 1.f;
        if (w > 0.f) { const V3 t = ld3(A.pt_tgt + 3 * i); if (!isfinite(t.x) || !isfinite(t.y) || !isfinite(t.z)) bad += 1.f; }
    }
    readout_prologue(s, T, tid);
    readout_aba_zeros(s, tid);
    for (int i = tid; i < D_NV; i += NT) s.arm[i] = 0.f;                 // the damping is the armature: all of it goes through s.extra
    KP_SYNC();
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
    for (int i = tid; i < D_NQ; i += NT) qcur[i] = s.qpos[i];            // root quaternion normalised by the forward pass
    PtEval E = fit_points_eval(s, A, r, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
    const float cost0 = E.cost;
    const bool ok = wave_sum(bad) == 0.f && isfinite(cost0);             // wave-uniform
    float mu = A.mu0, nacc = 0.f, dqmax = 0.f;
    const int n_iters = ok ? A.n_iters : 0;
#pragma nounroll
    for (int it = 0; it < n_iters; it++) {
        // J^T W e: body wrenches about o, subtree sums, projection on the motion axes; the pseudo-inertia of every body
        if (tid < D_NB) {
            sts6(s.sw + 6 * tid, E.S.W);
            float* ci = s.cinert + 10 * tid;
#pragma unroll
            for (int i = 0; i < 10; i++) ci[i] = E.S.ci[i];
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
        const PtEval Et = fit_points_eval(s, A, r, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
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
    // The result's own figures: s holds the kinematics of the accepted pose here (an accepted trial's, or the forward pass after a rejected one).
    // Lane = body again, so the sums do not depend on which points were skipped; a refused row reports zeros.
    float emax = 0.f, e2 = 0.f, npt = 0.f, deep = 0.f, nbelow = 0.f;
    if (tid < D_NB) {
        const int b = tid;
        const V3 xb = ld3(s.xpos + 3 * b);
        const Q4 qb = Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]};
        const int j1 = A.pt_adr[b + 1];
        for (int j = A.pt_adr[b]; j < j1; j++) {
            const size_t k = r * (size_t)K + (size_t)A.pt_perm[j];
            const float w = A.pt_w ? A.pt_w[k] : 1.f;
            float en = 0.f;
            if (ok && w > 0.f) {
                const V3 e = ld3(A.pt_tgt + 3 * k) - (xb + qrot(qb, ld3(A.pt_off + 3 * j)));
                const float n2 = dot(e, e);
                en = sqrtf(n2); emax = fmaxf(emax, en); e2 += n2; npt += 1.f;
            }
            if (A.pt_err) A.pt_err[k] = en;
        }
        if (ok) {
            const int v1 = T.vert_adr[b + 1];
            for (int v = T.vert_adr[b]; v < v1; v++) {
                const float d = A.floor_z - (xb + qrot(qb, ld3(T.verts + 3 * v))).z;
                if (d > 0.f) { deep = fmaxf(deep, d); nbelow += 1.f; }
            }
        }
    }
    emax = wave_max_f(emax); e2 = wave_sum(e2); npt = wave_sum(npt); deep = wave_max_f(deep); nbelow = wave_sum(nbelow);
    // a row that was refused returns its input as given
    for (int i = tid; i < D_NQ; i += NT) A.qpos[r * D_NQ + i] = ok ? qcur[i] : A.qpos0[r * D_NQ + i];
    if (A.dq) for (int d = tid; d < D_NV; d += NT) A.dq[r * D_NV + d] = dq[d];
    if (tid < 12) {
        const float v[12] = {cost0, E.cost, nacc, mu, E.epos, E.erot, dqmax, ok ? 0.f : 1.f, emax, npt > 0.f ? sqrtf(e2 / npt) : 0.f, deep, nbelow};
        float o = v[0];
#pragma unroll
        for (int k = 1; k < 12; k++) o = tid == k ? v[k] : o;
        A.info[r * 12 + tid] = o;
    }
}

}  // namespace kp
