// kp_fit_image.hpp -- pose fitting to 2D key points seen by calibrated cameras (kp_sim_fit_image).
//
// k_fit_image is k_fit_scene (kp_fit_scene.hpp, section 21) with one more sum in the cost:
//     c(q) = c_scene(q) + 1/2 sum_c sum_k w_ck |uv_ck - pi_c(p_k)|^2,      p_k = x_b(k) + R_b(k) o_k  (the call's one marker set)
// over C <= 8 pinhole cameras, 16 floats each: R_cw (9, row-major), t (3), fx, fy, cx, cy; cam = R_cw p + t, the camera looks along +z,
// pi = (cx + fx cam_x / cam_z, cy + fy cam_y / cam_z).  With a = cam_x / cam_z, b = cam_y / cam_z the projection's Jacobian in the camera frame is
//     J_pi = [ fx/z  0  -fx a/z ;  0  fy/z  -fy b/z ]      (2 x 3; in the world frame J_pi R_cw)
// GRADIENT: exact, a force at the point: f = R_cw^T J_pi^T w (uv - pi), so J_p^T f joins the wrench sums.  MATRIX: the point counts as an isotropic
// mass m = w lambda, lambda the largest eigenvalue of the 2 x 2 J_pi J_pi^T in closed form,
//     lambda = (A11 + A22)/2 + sqrt(((A11 - A22)/2)^2 + A12^2),   A11 = (fx/z)^2 (1 + a^2), A22 = (fy/z)^2 (1 + b^2), A12 = fx fy a b / z^2
// (fx == fy == f: (f/z)^2 (1 + a^2 + b^2)).  m I >= w R_cw^T J_pi^T J_pi R_cw: a majoriser, as for the floor and the objects, so the normal matrix stays
// a joint-space inertia and aba_solve solves it.  The accept test runs on the true cost.
//
// Lane = body.  After fit_scene_eval's sums the lane walks its points in the table's order and, per point, the cameras in index order; the sums go
// into the same registers (pt_add_force), no atomics.  The camera records stay in HBM: their addresses are wave-uniform (row, camera).  uv and uv_w are
// re-read at every evaluation (C K x 12 B per row).  An observation with w <= 0 is skipped by a branch: its uv is never read (NaN: an undetected key
// point) and the sums hold the bits they would hold without it; with no camera, or every weight <= 0, they hold k_fit_scene's.
// BEHIND THE CAMERA: a weighted observation with cam_z < z_near raises a flag that travels through wave_max.  At the start it gives the row status 2
// (no iteration, the input back); in a trial pose it makes that trial's cost +inf, which the accept rule rejects -- the fit never lowers its cost by
// hiding a point.  A NaN weight, a uv that is not finite under a positive weight and a camera record that is not finite give status 1.
// Every loop has a trip count fixed by the arguments; the walks hold no barrier; every branch around a barrier is wave-uniform.
#pragma once
#include "kp_fit_scene.hpp"

namespace kp {

// pt_add with the three things given apart: the force f at rr (from o), the isotropic mass m and the cost c
__device__ __forceinline__ void pt_add_force(PtSum& A, V3 rr, V3 f, float m, float c) {
    A.W.a = A.W.a + cross(rr, f); A.W.l = A.W.l + f;
    const float r2 = dot(rr, rr);
    A.ci[0] += m * (r2 - rr.x * rr.x); A.ci[1] += m * (r2 - rr.y * rr.y); A.ci[2] += m * (r2 - rr.z * rr.z);
    A.ci[3] -= m * rr.x * rr.y; A.ci[4] -= m * rr.x * rr.z; A.ci[5] -= m * rr.y * rr.z;
    A.ci[6] += m * rr.x; A.ci[7] += m * rr.y; A.ci[8] += m * rr.z; A.ci[9] += m;
    A.c += c;
}

// camera coordinates of the world point p
__device__ __forceinline__ V3 cam_point(const float* C, V3 p) {
    return v3(C[0] * p.x + C[1] * p.y + C[2] * p.z + C[9], C[3] * p.x + C[4] * p.y + C[5] * p.z + C[10], C[6] * p.x + C[7] * p.y + C[8] * p.z + C[11]);
}

// fit_scene_eval with the image term: the lane sums of the weighted observations join E.S, the term's cost joins E.cost.  behind: some weighted
// observation of the row lies in front of z_near (wave-uniform); E.cost is +inf then.  cams: the row's C records.
__device__ __forceinline__ PtEval fit_image_eval(const EnvLds& s, const FitImageArgs& A, size_t r, const float* geoms, int ngeom, const float* cams, const float* tpos, const float* tquat,
                                                 const float* wpos, const float* wrot, const float* qpr, const float* wpr, bool prior, int tid, bool& behind) {
    PtEval E = fit_scene_eval(s, A, r, geoms, ngeom, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
    float c = 0.f, flag = 0.f;
    if (tid < D_NB && A.n_cams > 0) {
        const int b = tid, K = A.n_points, C = A.n_cams;
        const V3 o = ld3(s.xpos), xb = ld3(s.xpos + 3 * b);
        const Q4 qb = Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]};
        E.S.c = 0.f;                      // its earlier content is in E.cost already
        const int j1 = A.img_adr[b + 1];
        for (int j = A.img_adr[b]; j < j1; j++) {
            const V3 p = xb + qrot(qb, ld3(A.pt_off + 3 * j));
            const size_t k0 = r * (size_t)C * K + (size_t)A.pt_perm[j];
            for (int ci = 0; ci < C; ci++) {
                const size_t k = k0 + (size_t)ci * K;
                const float w = A.uv_w ? A.uv_w[k] : 1.f;
                if (w > 0.f) {
                    const float* Cm = cams + 16 * ci;
                    const V3 cp = cam_point(Cm, p);
                    if (cp.z < A.z_near) { flag = 1.f; continue; }
                    const float iz = 1.f / cp.z, ax = cp.x * iz, ay = cp.y * iz;
                    const float gx = Cm[12] * iz, gy = Cm[13] * iz;
                    const float eu = A.uv[2 * k] - (Cm[14] + Cm[12] * ax), ev = A.uv[2 * k + 1] - (Cm[15] + Cm[13] * ay);
                    const V3 fc = v3(w * gx * eu, w * gy * ev, -w * (gx * ax * eu + gy * ay * ev));
                    const V3 f = v3(Cm[0] * fc.x + Cm[3] * fc.y + Cm[6] * fc.z, Cm[1] * fc.x + Cm[4] * fc.y + Cm[7] * fc.z, Cm[2] * fc.x + Cm[5] * fc.y + Cm[8] * fc.z);
                    const float a11 = gx * gx * (1.f + ax * ax), a22 = gy * gy * (1.f + ay * ay), a12 = gx * gy * ax * ay;
                    const float h = 0.5f * (a11 - a22);
                    const float lam = 0.5f * (a11 + a22) + sqrtf(h * h + a12 * a12);
                    pt_add_force(E.S, p - o, f, w * lam, 0.5f * w * (eu * eu + ev * ev));
                }
            }
        }
        c = E.S.c;
    }
    E.cost += wave_sum(c);
    behind = wave_max_f(flag) > 0.f;
    if (behind) E.cost = __builtin_inff();
    return E;
}

// One wavefront per row, on EnvLds (8 rows per CU): k_fit_scene's loop on fit_image_eval.
__global__ __launch_bounds__(64) void k_fit_image(FitImageArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EnvLds& s = *reinterpret_cast<EnvLds*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    const Params& P = A.P;
    const int K = A.n_points, C = A.n_cams;
    // the row's inputs, in the words k_fit_points keeps them in
    float* tpos = s.con_pos;
    float* tquat = s.jar3;
    float* wpos = s.con_D;
    float* wrot = s.con_D + D_NB;
    float* qpr = s.lim_D;
    float* wpr = s.lim_jar;
    float* damp = s.Mv;
    float* qcur = s.search;
    float* g = s.x;
    float* dq = s.qacc_s;
    const bool prior = A.q_prior != nullptr;
    // the row's static geoms and camera records: wave-uniform addresses
    const int ngeom = A.geoms ? min(max(A.ngeom[r], 0), D_MAXGEOM) : 0;
    const float* geoms = A.geoms ? A.geoms + r * (size_t)(D_MAXGEOM * 17) : nullptr;
    const float* cams = C > 0 ? A.cam + (A.camera_rows == 1 ? (size_t)0 : r) * (size_t)(16 * C) : nullptr;

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
    // the 3D targets, when the call has some
    if (A.pt_tgt)
        for (int k = tid; k < K; k += NT) {
            const size_t i = r * (size_t)K + k;
            const float w = A.pt_w ? A.pt_w[i] : 1.f;
            if (w != w) bad += 1.f;
            if (w > 0.f) { const V3 t = ld3(A.pt_tgt + 3 * i); if (!isfinite(t.x) || !isfinite(t.y) || !isfinite(t.z)) bad += 1.f; }
        }
    for (int i = tid; i < ngeom * 17; i += NT) bad += isfinite(geoms[i]) ? 0.f : 1.f;
    // the observations: a NaN weight, or a uv that is not finite under a positive weight, refuses the row; a skipped observation's uv is not read
    for (int k = tid; k < C * K; k += NT) {
        const size_t i = r * (size_t)C * K + k;
        const float w = A.uv_w ? A.uv_w[i] : 1.f;
        if (w != w) bad += 1.f;
        if (w > 0.f && (!isfinite(A.uv[2 * i]) || !isfinite(A.uv[2 * i + 1]))) bad += 1.f;
    }
    for (int i = tid; i < 16 * C; i += NT) bad += isfinite(cams[i]) ? 0.f : 1.f;
    readout_prologue(s, T, tid);
    readout_aba_zeros(s, tid);
    for (int i = tid; i < D_NV; i += NT) s.arm[i] = 0.f;
    KP_SYNC();
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
    for (int i = tid; i < D_NQ; i += NT) qcur[i] = s.qpos[i];
    bool behind0;
    PtEval E = fit_image_eval(s, A, r, geoms, ngeom, cams, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid, behind0);
    const float cost0 = E.cost;
    const bool clean = wave_sum(bad) == 0.f;                             // wave-uniform, as behind0
    const bool ok = clean && !behind0 && isfinite(cost0);
    const float status = !clean ? 1.f : behind0 ? 2.f : ok ? 0.f : 1.f;
    float mu = A.mu0, nacc = 0.f, dqmax = 0.f;
    const int n_iters = ok ? A.n_iters : 0;
#pragma nounroll
    for (int it = 0; it < n_iters; it++) {
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
        bool bt;
        const PtEval Et = fit_image_eval(s, A, r, geoms, ngeom, cams, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid, bt);
        if (isfinite(Et.cost) && Et.cost < E.cost) {                     // wave-uniform; a trial with a point behind a camera costs +inf
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
    // The result's own figures, on the kinematics of the accepted pose; a refused row reports zeros.
    float emax = 0.f, e2 = 0.f, npt = 0.f, deep = 0.f, nbelow = 0.f;
    float umax = 0.f, u2 = 0.f, nuv = 0.f, zmin = 3.0e38f;
    SceneFig F{0.f, 0.f, 0.f, 0.f};
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
        // without 3D targets pt_adr is the table of zeros: the distances are zeros
        if (!A.pt_tgt && A.pt_err)
            for (int j = A.img_adr[b]; j < A.img_adr[b + 1]; j++) A.pt_err[r * (size_t)K + (size_t)A.pt_perm[j]] = 0.f;
        if (ok) {
            const int v1 = T.vert_adr[b + 1];
            for (int v = T.vert_adr[b]; v < v1; v++) {
                const float d = A.floor_z - (xb + qrot(qb, ld3(T.verts + 3 * v))).z;
                if (d > 0.f) { deep = fmaxf(deep, d); nbelow += 1.f; }
            }
            F = scene_walk<false>(T, geoms, ngeom, ld3(s.xpos), xb, qb, b, 1.f, E.S);
        }
        // the reprojection errors at the result, in pixels
        if (C > 0) {
            const int i1 = A.img_adr[b + 1];
            for (int j = A.img_adr[b]; j < i1; j++) {
                const V3 p = xb + qrot(qb, ld3(A.pt_off + 3 * j));
                const size_t k0 = r * (size_t)C * K + (size_t)A.pt_perm[j];
                for (int ci = 0; ci < C; ci++) {
                    const size_t k = k0 + (size_t)ci * K;
                    const float w = A.uv_w ? A.uv_w[k] : 1.f;
                    float en = 0.f;
                    if (ok && w > 0.f) {
                        const float* Cm = cams + 16 * ci;
                        const V3 cp = cam_point(Cm, p);
                        const float eu = A.uv[2 * k] - (Cm[14] + Cm[12] * cp.x / cp.z), ev = A.uv[2 * k + 1] - (Cm[15] + Cm[13] * cp.y / cp.z);
                        const float n2 = eu * eu + ev * ev;
                        en = sqrtf(n2); umax = fmaxf(umax, en); u2 += n2; nuv += 1.f; zmin = fminf(zmin, cp.z);
                    }
                    if (A.uv_err) A.uv_err[k] = en;
                }
            }
        }
    }
    emax = wave_max_f(emax); e2 = wave_sum(e2); npt = wave_sum(npt); deep = wave_max_f(deep); nbelow = wave_sum(nbelow);
    const float odeep = wave_max_f(F.deep), onv = wave_sum(F.nvert), onp = wave_sum(F.npair);
    umax = wave_max_f(umax); u2 = wave_sum(u2); nuv = wave_sum(nuv); zmin = -wave_max_f(-zmin);
    for (int i = tid; i < D_NQ; i += NT) A.qpos[r * D_NQ + i] = ok ? qcur[i] : A.qpos0[r * D_NQ + i];
    if (A.dq) for (int d = tid; d < D_NV; d += NT) A.dq[r * D_NV + d] = dq[d];
    if (tid < 20) {
        const float v[20] = {cost0, E.cost, nacc, mu, E.epos, E.erot, dqmax, status, emax, npt > 0.f ? sqrtf(e2 / npt) : 0.f, deep, nbelow, odeep, onv, onp, 0.f,
                             umax, nuv > 0.f ? sqrtf(u2 / nuv) : 0.f, nuv, nuv > 0.f ? zmin : 0.f};
        float o = v[0];
#pragma unroll
        for (int k = 1; k < 20; k++) o = tid == k ? v[k] : o;
        A.info[r * 20 + tid] = o;
    }
}

}  // namespace kp
