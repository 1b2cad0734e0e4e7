// kp_fit_scene.hpp -- pose fitting that keeps the hulls out of the scene's static objects (kp_sim_fit_scene).
//
// k_fit_scene is k_fit_points (kp_fit_points.hpp, section 20) with one more sum in the cost:
//     c(q) = c_points(q) + 1/2 w_obj sum_{pairs (b, g)} sum_{v in footprint of f*} max(0, d_f* - n_f* . x_v)^2
// over the hulls b and the row's static geoms g (boxes and z-axis cylinders, the 17-float world records kp_sim_inverse_dynamics places; at most 8).
// Per pair, after the exact-safe cull geom_sdf(g, xpos_b) - body_rbound[b] > 0 (collide's second cull, without its margin):
//   candidate planes  box: (+-a_i, n.c + h_i) in the order +x -x +y -y +z -z; cylinder: the caps +-a_3 and, when the radial part of xpos_b - c is
//                     longer than 1e-6, the tangent plane n = u, d = u.c + rho with u the unit radial direction towards the body origin (the plane
//                     collide's third cull tests);
//   hull depth        D_f = max_v (d_f - n_f . x_v) over ALL vertices of the hull.  Some D_f <= 0: a separating plane exists, the pair has no term.
//                     Otherwise f* is the first plane of least D_f;
//   footprint of f*   the primitive's extent in the directions other than n: |a_j.(x - c)| < h_j for the two other axes of a box, radial distance
//                     < rho for a cap, |a_3.(x - c)| < h and |(a_3 x u).(x - c)| < rho for the tangent plane;
//   cost              every footprint vertex behind the plane counts, however deep, and is pulled to its own projection on the plane, re-projected at
//                     every evaluation.  A vertex in two geoms' footprints counts in both.
// GRADIENT: J_v^T w_obj (d - n.x_v) n with n held fixed -- exact for box faces and caps (n is constant in the world); for the tangent plane it leaves
// out the turn of u with the body origin (u follows xpos_b, so the true gradient has a term in du/dq that is not here).  MATRIX: every counted vertex
// is an isotropic point mass w_obj (pt_add), a majoriser as for the floor, so the normal matrix stays a joint-space inertia and aba_solve solves it.
// The accept test runs on the true cost.
//
// Lane = body.  Per geom (index order), the lane culls, walks its hull's vertices once for the D_f (minima and maxima of the vertex coordinates in the
// geom's frame: registers), picks f*, and walks them again for the sums -- in registers, no atomics, an order fixed by geom index and the blob's vertex
// order.  No collide call: the fit's inputs occupy the collision words of EnvLds, and one contact per pair is too weak a signal.  The geom table
// [8, 17] stays in HBM: its addresses are wave-uniform (row and geom index), so the records arrive through scalar loads and cost no LDS; the block
// stays on EnvLds, 8 rows per CU like k_fit_points.  The loops over geoms and vertices hold no barrier; their trip counts are fixed by ngeom and the
// vertex table.  Every branch around a barrier is taken on a wave_sum / wave_max result.  Nothing is shared between rows.  A row whose input, geom
// records or first cost are not finite runs no iteration and returns its input.  With w_obj == 0, no geoms or every pair separated, the sums hold the
// bits k_fit_points' hold: the term is skipped by branches, not by zero factors, and its cost is added as + 0.
#pragma once
#include "kp_fit_points.hpp"

namespace kp {

struct SceneFig { float c, deep, nvert, npair; };      // a lane's share of the object cost (without the 1/2 w_obj ... see scene_walk), its deepest counted vertex, counted vertices, pairs with a term

// The object term of body b (lane = body) at the pose whose kinematics s holds.  SUM: add the counted vertices to S as point masses w (wrench about o
// and the ten inertia floats; S.c is left alone) -- otherwise only the figures.  F.c = 1/2 w sum depth^2.
template <bool SUM>
__device__ __forceinline__ SceneFig scene_walk(const DevTables& T, const float* geoms, int ngeom, V3 o, V3 xb, Q4 qb, int b, float w, PtSum& S) {
    SceneFig F{0.f, 0.f, 0.f, 0.f};
    const float rb = T.body_rbound[b];
    const int v0 = T.vert_adr[b], v1 = T.vert_adr[b + 1];
    const float keep = S.c;
    for (int gi = 0; gi < ngeom; gi++) {
        const float* g = geoms + 17 * gi;
        if (geom_sdf(g, xb) - rb > 0.f) continue;
        const float* R = g + 7;
        const V3 c = ld3(g + 4);
        const bool cyl = g[0] != 0.f;
        // the tangent plane's direction in the geom frame: the unit radial direction from the axis towards the body origin
        const V3 cb = xb - c;
        float ux = R[0] * cb.x + R[3] * cb.y + R[6] * cb.z, uy = R[1] * cb.x + R[4] * cb.y + R[7] * cb.z;
        const float un = sqrtf(ux * ux + uy * uy);
        const bool tang = cyl && un > 1e-6f;
        ux = tang ? ux / un : 0.f; uy = tang ? uy / un : 0.f;
        // pass 1: extent of the hull along the geom's axes and along u
        V3 mn = v3(3.0e38f, 3.0e38f, 3.0e38f), mx = v3(-3.0e38f, -3.0e38f, -3.0e38f);
        float tmn = 3.0e38f;
        for (int v = v0; v < v1; v++) {
            const V3 d = xb + qrot(qb, ld3(T.verts + 3 * v)) - c;
            const V3 l = v3(R[0] * d.x + R[3] * d.y + R[6] * d.z, R[1] * d.x + R[4] * d.y + R[7] * d.z, R[2] * d.x + R[5] * d.y + R[8] * d.z);
            mn = v3(fminf(mn.x, l.x), fminf(mn.y, l.y), fminf(mn.z, l.z));
            mx = v3(fmaxf(mx.x, l.x), fmaxf(mx.y, l.y), fmaxf(mx.z, l.z));
            tmn = fminf(tmn, l.x * ux + l.y * uy);
        }
        // the first plane of least depth; a depth <= 0 separates
        const float hz = cyl ? g[2] : g[3];
        float D = hz - mn.z; int f = 4;                       // +z (box) / +cap
        float sep = D;
        { const float d = hz + mx.z; sep = fminf(sep, d); if (d < D) { D = d; f = 5; } }
        if (cyl) {
            if (tang) { const float d = g[1] - tmn; sep = fminf(sep, d); if (d < D) { D = d; f = 6; } }
        } else {
            // +x -x +y -y come before +z -z: a tie goes to the earlier plane
            float d = g[2] + mx.y; sep = fminf(sep, d); if (d <= D) { D = d; f = 3; }
            d = g[2] - mn.y; sep = fminf(sep, d); if (d <= D) { D = d; f = 2; }
            d = g[1] + mx.x; sep = fminf(sep, d); if (d <= D) { D = d; f = 1; }
            d = g[1] - mn.x; sep = fminf(sep, d); if (d <= D) { D = d; f = 0; }
        }
        if (!(sep > 0.f)) continue;
        F.npair += 1.f;
        // the plane in the geom frame: depth = hn - nl . l; the footprint along t1, t2 (a cap: the radius)
        V3 nl, t1, t2; float hn, e1, e2;
        const bool cap = cyl && f != 6;
        if (f == 6) { nl = v3(ux, uy, 0.f); hn = g[1]; t1 = v3(0.f, 0.f, 1.f); e1 = g[2]; t2 = v3(-uy, ux, 0.f); e2 = g[1]; }
        else if (f >= 4) { nl = v3(0.f, 0.f, f == 4 ? 1.f : -1.f); hn = hz; t1 = v3(1.f, 0.f, 0.f); e1 = g[1]; t2 = v3(0.f, 1.f, 0.f); e2 = g[2]; }
        else if (f >= 2) { nl = v3(0.f, f == 2 ? 1.f : -1.f, 0.f); hn = g[2]; t1 = v3(1.f, 0.f, 0.f); e1 = g[1]; t2 = v3(0.f, 0.f, 1.f); e2 = g[3]; }
        else { nl = v3(f == 0 ? 1.f : -1.f, 0.f, 0.f); hn = g[1]; t1 = v3(0.f, 1.f, 0.f); e1 = g[2]; t2 = v3(0.f, 0.f, 1.f); e2 = g[3]; }
        const V3 n = mulmat(R, nl);
        // pass 2: the footprint's vertices behind the plane
        for (int v = v0; v < v1; v++) {
            const V3 p = xb + qrot(qb, ld3(T.verts + 3 * v));
            const V3 d = p - c;
            const V3 l = v3(R[0] * d.x + R[3] * d.y + R[6] * d.z, R[1] * d.x + R[4] * d.y + R[7] * d.z, R[2] * d.x + R[5] * d.y + R[8] * d.z);
            const float dep = hn - dot(nl, l);
            const bool in = cap ? sqrtf(l.x * l.x + l.y * l.y) < g[1] : (fabsf(dot(t1, l)) < e1 && fabsf(dot(t2, l)) < e2);
            if (in && dep > 0.f) {
                if (SUM) pt_add(S, p - o, dep * n, w);
                F.c += 0.5f * w * dep * dep;
                F.deep = fmaxf(F.deep, dep); F.nvert += 1.f;
            }
        }
    }
    S.c = keep;
    return F;
}

// fit_points_eval with the object term: the lane sums of the counted vertices join E.S, the term's cost joins E.cost
__device__ __forceinline__ PtEval fit_scene_eval(const EnvLds& s, const FitSceneArgs& A, size_t r, const float* geoms, int ngeom, const float* tpos, const float* tquat, const float* wpos,
                                                 const float* wrot, const float* qpr, const float* wpr, bool prior, int tid) {
    PtEval E = fit_points_eval(s, A, r, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
    float c = 0.f;
    if (tid < D_NB && A.w_obj > 0.f) {
        const Q4 qb = Q4{s.xquat[4 * tid], s.xquat[4 * tid + 1], s.xquat[4 * tid + 2], s.xquat[4 * tid + 3]};
        c = scene_walk<true>(A.T, geoms, ngeom, ld3(s.xpos), ld3(s.xpos + 3 * tid), qb, tid, A.w_obj, E.S).c;
    }
    E.cost += wave_sum(c);
    return E;
}

// One wavefront per row, on EnvLds (8 rows per CU): k_fit_points' loop on fit_scene_eval.
__global__ __launch_bounds__(64) void k_fit_scene(FitSceneArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EnvLds& s = *reinterpret_cast<EnvLds*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    const Params& P = A.P;
    const int K = A.n_points;
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
    // the row's static geoms: wave-uniform addresses
    const int ngeom = A.geoms ? min(max(A.ngeom[r], 0), D_MAXGEOM) : 0;
    const float* geoms = A.geoms ? A.geoms + r * (size_t)(D_MAXGEOM * 17) : nullptr;

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
    for (int k = tid; k < K; k += NT) {
        const size_t i = r * (size_t)K + k;
        const float w = A.pt_w ? A.pt_w[i] : 1.f;
        if (w != w) bad += 1.f;
        if (w > 0.f) { const V3 t = ld3(A.pt_tgt + 3 * i); if (!isfinite(t.x) || !isfinite(t.y) || !isfinite(t.z)) bad += 1.f; }
    }
    // a geom record that is not finite (an object pose that is not) refuses the row
    for (int i = tid; i < ngeom * 17; i += NT) bad += isfinite(geoms[i]) ? 0.f : 1.f;
    readout_prologue(s, T, tid);
    readout_aba_zeros(s, tid);
    for (int i = tid; i < D_NV; i += NT) s.arm[i] = 0.f;
    KP_SYNC();
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
    for (int i = tid; i < D_NQ; i += NT) qcur[i] = s.qpos[i];
    PtEval E = fit_scene_eval(s, A, r, geoms, ngeom, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
    const float cost0 = E.cost;
    const bool ok = wave_sum(bad) == 0.f && isfinite(cost0);             // wave-uniform
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
        const PtEval Et = fit_scene_eval(s, A, r, geoms, ngeom, tpos, tquat, wpos, wrot, qpr, wpr, prior, tid);
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
    // The result's own figures, on the kinematics of the accepted pose; a refused row reports zeros.
    float emax = 0.f, e2 = 0.f, npt = 0.f, deep = 0.f, nbelow = 0.f;
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
        if (ok) {
            const int v1 = T.vert_adr[b + 1];
            for (int v = T.vert_adr[b]; v < v1; v++) {
                const float d = A.floor_z - (xb + qrot(qb, ld3(T.verts + 3 * v))).z;
                if (d > 0.f) { deep = fmaxf(deep, d); nbelow += 1.f; }
            }
            F = scene_walk<false>(T, geoms, ngeom, ld3(s.xpos), xb, qb, b, 1.f, E.S);
        }
    }
    emax = wave_max_f(emax); e2 = wave_sum(e2); npt = wave_sum(npt); deep = wave_max_f(deep); nbelow = wave_sum(nbelow);
    const float odeep = wave_max_f(F.deep), onv = wave_sum(F.nvert), onp = wave_sum(F.npair);
    for (int i = tid; i < D_NQ; i += NT) A.qpos[r * D_NQ + i] = ok ? qcur[i] : A.qpos0[r * D_NQ + i];
    if (A.dq) for (int d = tid; d < D_NV; d += NT) A.dq[r * D_NV + d] = dq[d];
    if (tid < 16) {
        const float v[16] = {cost0, E.cost, nacc, mu, E.epos, E.erot, dqmax, ok ? 0.f : 1.f, emax, npt > 0.f ? sqrtf(e2 / npt) : 0.f, deep, nbelow, odeep, onv, onp, 0.f};
        float o = v[0];
#pragma unroll
        for (int k = 1; k < 16; k++) o = tid == k ? v[k] : o;
        A.info[r * 16 + tid] = o;
    }
}

}  // namespace kp
