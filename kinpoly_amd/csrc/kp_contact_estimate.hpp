// kp_contact_estimate.hpp -- contact forces estimated from kinematics on motion rows (kp_sim_estimate_contacts).
//
// Inverse dynamics (kp_inverse_dyn.hpp) charges a row the contact forces of the soft-constraint model, a function of how many millimetres a hull
// penetrates.  This kernel asks the other question: which forces inside the friction pyramids of the points NEAR a surface explain the row's root
// residual best.  Per row:
//   candidates  the contacts collide() finds at the row's pose with the margin set to `reach` (the launcher's copy of Params): p_c, unit normal n_c
//               into the hull, tangents t1_c, t2_c of contact_frame; pyramid edges d_ck = n_c +- mu t1_c, n_c +- mu t2_c (row_val's order)
//   demand      need = M qacc + qfrc_bias (+ armature), as k_inverse_dynamics forms it; no joint-limit row is evaluated;
//               r = [need[0:3]; R_root need[3:6]]: force and moment in world axes about the root position o
//   solve       lambda >= 0 [4 C] minimising 1/2 (r - G lambda)^T W (r - G lambda) + 1/2 rho |lambda|^2, g_ck = [d_ck; (p_c - o) x d_ck],
//               W = diag(w_f I, w_m I).  Strictly convex: the minimiser is unique.
// Method: semismooth Newton on the 6-vector e = r - G lambda.  The KKT conditions give lambda = max(0, G^T W e) / rho, so e is the root of
//     F(e) = e + (1 / rho) G max(0, G^T W e) - r,
// which is W^-1 grad phi of the strictly convex, piecewise quadratic phi(e) = 1/2 e^T W e + 1/(2 rho) |max(0, G^T W e)|^2 - r^T W e.  In scaled variables
// (e^ = W^1/2 e, lambda^ = sqrt(w_f) lambda: forces in body weights with the default weights, G^ = W^1/2 G / sqrt(w_f), rho^ = rho / w_f) the Jacobian is
// H = I + (1 / rho^) G^_A G^_A^T over the active columns A.  Lane = candidate; a lane owns its four columns as three 6-vectors (normal, t1, t2).  One
// iteration: H's 21 entries by wave_sum, a 6 x 6 Cholesky solved redundantly by every lane, then the step along d = -H^-1 F: the full step where phi's
// slope there is <= 0 (to 1e-3 of the slope at 0), otherwise the exact minimiser of phi along d (phi' is piecewise linear along a line: EST_LS_MAX steps
// of a bracketed Newton iteration, two wave_sums each).  Newton with an exact line search on a strictly convex piecewise quadratic terminates finitely;
// an Armijo halving does not serve here: where few columns are active H is close to I, the step activates many columns at once and the curvature along d
// is up to 1 / rho^ times the model's.  It stops when the active set repeats and the step is below e's resolution (|alpha d| <= 5e-7 |r^|) or a full
// step reaches |F| <= 1e-6 |r^|, when phi no longer descends within its rounding, or at n_iters.
// Every branch is taken on a wave_sum result, which every lane holds alike, so all branches are wave-uniform; every loop's trip count is bounded by the
// arguments; no atomics, nothing shared between rows.  A row with a non-finite input runs nothing (not even the collision pass), reports status 1 and
// writes zeros.  Then f_c = sum_k lambda_ck d_ck goes into s.jv3 and project_contact_forces (the one copy, kp_readout_device.hpp) gives qfrc_contact.
// A rows API like k_inverse_dynamics, whose load section and OBJ dispatch this follows: full layouts, static objects from the call's scratch, a row
// without a placed geom runs the floor code.  Compiled in the read-out unit (kp_readout.hip) only.
#pragma once
#include "kp_contact_force.hpp"

namespace kp {

constexpr int EST_LS_MAX = 12;            // steps of the line search's safeguarded Newton iteration
constexpr int EST_TRUNCATED = 2;          // status bit: all 64 slots are taken, collide() may have dropped candidates
constexpr int EST_NOT_CONVERGED = 4;      // status bit: n_iters ran out before the stopping rule held

// phi, F and the column products z = G^^T e^ at a point; every lane holds the same phi, F, fn and its own z
struct EstPoint { float phi, fn; float F[6]; float z[4]; };

__device__ __forceinline__ EstPoint est_eval(const float* gn, const float* g1, const float* g2, float mu, float inv_rho, const float* rh, const float* e) {
    EstPoint E;
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) { a = fmaf(gn[i], e[i], a); b = fmaf(g1[i], e[i], b); c = fmaf(g2[i], e[i], c); }
    E.z[0] = a + mu * b; E.z[1] = a - mu * b; E.z[2] = a + mu * c; E.z[3] = a - mu * c;
    float p[4], pp = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) { p[k] = fmaxf(E.z[k], 0.f); pp = fmaf(p[k], p[k], pp); }
    const float sn = (p[0] + p[1]) + (p[2] + p[3]), s1 = mu * (p[0] - p[1]), s2 = mu * (p[2] - p[3]);
    float ee = 0.f, re = 0.f, ff = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const float gi = wave_sum(sn * gn[i] + s1 * g1[i] + s2 * g2[i]);
        E.F[i] = (e[i] - rh[i]) + inv_rho * gi;
        ee = fmaf(e[i], e[i], ee); re = fmaf(rh[i], e[i], re); ff = fmaf(E.F[i], E.F[i], ff);
    }
    E.phi = 0.5f * ee - re + 0.5f * inv_rho * wave_sum(pp);
    E.fn = sqrtf(ff);
    return E;
}

// d = -H^-1 F by Cholesky; Hp: H packed by s6i.  H = I + a positive semidefinite matrix, so every pivot is >= 1 before rounding.
__device__ __forceinline__ void est_solve(const float* Hp, const float* F, float* d) {
    float L[6][6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        float djj = Hp[s6i(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) djj -= L[j][k] * L[j][k];
        const float ljj = sqrtf(fmaxf(djj, 1e-20f)), inv = 1.0f / ljj;
        L[j][j] = inv;                                                   // the diagonal is kept inverted
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            float v = Hp[s6i(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v * inv;
        }
    }
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        float v = -F[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
        y[i] = v * L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        float v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= L[k][i] * d[k];
        d[i] = v * L[i][i];
    }
}

// a refused row: zeros everywhere, status 1
__device__ __forceinline__ void estimate_refuse(const EstimateOut& O, size_t r, int tid) {
    for (int i = tid; i < D_NV; i += 64) {
        if (O.qfrc_inverse) O.qfrc_inverse[r * D_NV + i] = 0.f;
        if (O.qfrc_contact) O.qfrc_contact[r * D_NV + i] = 0.f;
    }
    if (O.contact) for (int i = tid; i < D_MAXCON * D_CF_ROW; i += 64) O.contact[r * D_MAXCON * D_CF_ROW + i] = 0.f;
    if (O.lambda) for (int i = tid; i < D_MAXCON * 4; i += 64) O.lambda[r * D_MAXCON * 4 + i] = 0.f;
    if (tid < 6) {
        if (O.resid) O.resid[r * 6 + tid] = 0.f;
        if (O.net_wrench) O.net_wrench[r * 6 + tid] = 0.f;
    }
    if (O.ncon && tid == 0) O.ncon[r] = 0;
    if (O.info && tid < 8) O.info[r * 8 + tid] = tid == 7 ? 1.f : 0.f;
}

// one row on one wavefront; s: the row's LDS block with qpos, qvel, qacc and the per-lane tables loaded (OBJ: the static geoms too)
template <bool OBJ, class SL>
__device__ __forceinline__ void estimate_row(SL& s, const EstimateArgs& A, size_t r, int tid) {
    const DevTables& T = A.T;
    const Params& P = A.P;                                               // the model's with margin = reach (and mu = cfg.mu where given)
    const EstimateOut& O = A.O;
    const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    forward_kin_bias<64>(s, T, P, depth, bpos, tid);
    collide<64, OBJ>(s, T, P, tid);
    const int ncon = s.ncon;                                            // <= 64: one candidate per lane below
    const bool mine = tid < ncon;
    const float my_dist = mine ? s.con_D[tid] : 0.f;                    // no make_constraint here: con_D keeps the distance
    // ---- need = M qacc + qfrc_bias -> s.qacc_s, as invdyn_row forms it
    float* sacc = s.Mv;                                                 // [24][6] over Mv + mres
    spatial_accumulate<64>(s, s.qacc, depth, tid, sacc);
    if (tid < D_NB) sts6(s.sw + 6 * tid, inert_mul(s.cinert + 10 * tid, lds6(sacc + 6 * tid)) + lds6(s.fb + 6 * tid));
    project_body_wrenches(s, s.qacc_s, tid);
    for (int d = tid; d < D_NV; d += 64) s.qacc_s[d] += s.arm[d] * s.qacc[d];
    for (int j = tid; j < 72; j += 64) s.lim_jar[j] = 0.f;              // no joint-limit row: project_contact_forces adds one only where lim_jar < 0
    KP_SYNC();

    // ---- the demand and this lane's columns, scaled
    const float sf = A.sf, sm = A.sm, kap = sm / sf, mu = P.mu, inv_rho = 1.0f / A.rho_hat;
    const V3 o = ld3(s.xpos);
    const V3 rf = ld3(s.qacc_s), rm = qrot(Q4{s.xquat[0], s.xquat[1], s.xquat[2], s.xquat[3]}, ld3(s.qacc_s + 3));
    const float rh[6] = {sf * rf.x, sf * rf.y, sf * rf.z, sm * rm.x, sm * rm.y, sm * rm.z};
    float gn[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, g1[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, g2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Frame fr = Frame{v3(0.f, 0.f, 1.f), v3(0.f, 1.f, 0.f), v3(-1.f, 0.f, 0.f)};
    if (mine) {
        fr = contact_frame<OBJ>(s, tid);
        const V3 p = ld3(s.con_pos + 3 * tid) - o;
        const V3 mn = kap * cross(p, fr.n), m1 = kap * cross(p, fr.t1), m2 = kap * cross(p, fr.t2);
        gn[0] = fr.n.x; gn[1] = fr.n.y; gn[2] = fr.n.z; gn[3] = mn.x; gn[4] = mn.y; gn[5] = mn.z;
        g1[0] = fr.t1.x; g1[1] = fr.t1.y; g1[2] = fr.t1.z; g1[3] = m1.x; g1[4] = m1.y; g1[5] = m1.z;
        g2[0] = fr.t2.x; g2[1] = fr.t2.y; g2[2] = fr.t2.z; g2[3] = m2.x; g2[4] = m2.y; g2[5] = m2.z;
    }

    // ---- semismooth Newton from e = r (lambda = 0)
    float e[6];
    float rr = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) { e[i] = rh[i]; rr = fmaf(rh[i], rh[i], rr); }
    EstPoint E = est_eval(gn, g1, g2, mu, inv_rho, rh, e);
    const float cost0 = 0.5f * rr, ftol = 1e-6f * sqrtf(rr), slack = 1e-6f * (0.5f * rr);
    float iters = 0.f, searches = 0.f;
    bool conv = ncon == 0;                                              // no candidate: lambda = none, e = r
    const int n_iters = ncon > 0 ? A.n_iters : 0;                       // wave-uniform
#pragma nounroll
    for (int it = 0; it < n_iters && !conv; it++) {
        float S[21];
#pragma unroll
        for (int i = 0; i < 21; i++) S[i] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float on = E.z[k] > 0.f ? 1.f : 0.f, sg = (k & 1) ? -mu : mu;
            float g[6];
#pragma unroll
            for (int i = 0; i < 6; i++) g[i] = gn[i] + sg * (k < 2 ? g1[i] : g2[i]);
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) S[s6i(a, b)] = fmaf(on * g[a], g[b], S[s6i(a, b)]);
        }
        float Hp[21];
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) Hp[s6i(a, b)] = (a == b ? 1.f : 0.f) + inv_rho * wave_sum(S[s6i(a, b)]);
        float d[6];
        est_solve(Hp, E.F, d);
        // along d the column products are linear, z_k + alpha w_k, so phi's slope and curvature there cost one dot product per column and two wave_sums:
        //     phi'(alpha) = (e + alpha d - r) . d + (1 / rho) sum_k max(0, z_k + alpha w_k) w_k,   phi''(alpha) = d . d + (1 / rho) sum_{z_k + alpha w_k > 0} w_k^2
        float Fd = 0.f, dd = 0.f, ed = 0.f, wa = 0.f, wb = 0.f, wc = 0.f;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            Fd = fmaf(E.F[i], d[i], Fd); dd = fmaf(d[i], d[i], dd); ed = fmaf(e[i] - rh[i], d[i], ed);
            wa = fmaf(gn[i], d[i], wa); wb = fmaf(g1[i], d[i], wb); wc = fmaf(g2[i], d[i], wc);
        }
        const float w[4] = {wa + mu * wb, wa - mu * wb, wa + mu * wc, wa - mu * wc};
        auto slope = [&](float a, float& g, float& h) {
            float sg = 0.f, sh = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) { const float za = fmaf(a, w[k], E.z[k]); const bool on = za > 0.f; sg += on ? za * w[k] : 0.f; sh += on ? w[k] * w[k] : 0.f; }
            g = ed + a * dd + inv_rho * wave_sum(sg); h = dd + inv_rho * wave_sum(sh);
        };
        float alpha = 1.f, g, h;
        slope(1.f, g, h);
        if (!(g <= 1e-3f * fabsf(Fd))) {                                  // wave-uniform: the full step overshoots the minimiser along d
            // the exact minimiser along d: safeguarded Newton on phi', which is increasing and piecewise linear, inside a bracket [lo, hi] with phi'(lo) <= 0 < phi'(hi)
            float lo = 0.f, hi = 1.f, a = 0.f;
            slope(0.f, g, h);
            g = Fd;
#pragma nounroll
            for (int ls = 0; ls < EST_LS_MAX; ls++) {
                float an = a - g / h;
                if (!(an > lo && an < hi)) an = 0.5f * (lo + hi);
                a = an;
                slope(a, g, h);
                if (g <= 0.f) lo = a; else hi = a;
            }
            alpha = fabsf(g) <= 1e-3f * fabsf(Fd) ? a : (lo > 0.f ? lo : a);
            searches += 1.f;
        }
        float et[6];
#pragma unroll
        for (int i = 0; i < 6; i++) et[i] = fmaf(alpha, d[i], e[i]);
        const EstPoint Et = est_eval(gn, g1, g2, mu, inv_rho, rh, et);
        iters += 1.f;
        if (!(Et.phi <= E.phi + slack)) { conv = E.fn <= 1e-4f * sqrtf(rr); break; }      // no descent within phi's rounding: e stays (wave-uniform)
        float diff = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) diff += (Et.z[k] > 0.f) != (E.z[k] > 0.f) ? 1.f : 0.f;
        const bool same = wave_sum(diff) == 0.f;
        conv = same && (alpha * sqrtf(dd) <= 5e-7f * sqrtf(rr) || (alpha == 1.f && Et.fn <= ftol));
#pragma unroll
        for (int i = 0; i < 6; i++) e[i] = et[i];
        E = Et;
    }

    // ---- lambda, f_c, the projection
    float lam[4], nact = 0.f, ll = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float lh = fmaxf(E.z[k], 0.f) * inv_rho;                  // lambda^ (body weights with the default weights)
        lam[k] = lh / sf; nact += E.z[k] > 0.f ? 1.f : 0.f; ll = fmaf(lh, lh, ll);
    }
    nact = wave_sum(nact); ll = wave_sum(ll);
    float ee = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) ee = fmaf(e[i], e[i], ee);
    const float cost = 0.5f * ee + 0.5f * A.rho_hat * ll;
    float* fc = s.jv3;                                                  // [ncon][3] world force on the hull
    const V3 f = frame_world(fr, v3((lam[0] + lam[1]) + (lam[2] + lam[3]), mu * (lam[0] - lam[1]), mu * (lam[2] - lam[3])));
    if (ncon != 0) {
        if (mine) st3(fc + 3 * tid, f);
        KP_SYNC();
        project_contact_forces(s, fc, s.x, tid);
    }
    KP_SYNC();

    // ---- outputs
    for (int i = tid; i < D_NV; i += 64) {
        const float fcon = ncon != 0 ? s.x[i] : 0.f;
        if (O.qfrc_inverse) O.qfrc_inverse[r * D_NV + i] = s.qacc_s[i] - fcon;
        if (O.qfrc_contact) O.qfrc_contact[r * D_NV + i] = fcon;
    }
    if (O.ncon && tid == 0) O.ncon[r] = ncon;
    if (O.contact) {
        // section 14's row with B = -1 (the floor or a static geom, always), the candidate's distance and the estimated force
        float* row = O.contact + (r * D_MAXCON + tid) * D_CF_ROW;
        if (mine) {
            row[0] = (float)s.con_body[tid]; row[1] = -1.f; row[2] = my_dist;
            st3(row + 3, ld3(s.con_pos + 3 * tid)); st3(row + 6, fr.n); st3(row + 9, f);
        } else {
#pragma unroll
            for (int k = 0; k < D_CF_ROW; k++) row[k] = 0.f;
        }
    }
    if (O.lambda) {
        float* row = O.lambda + (r * D_MAXCON + tid) * 4;
#pragma unroll
        for (int k = 0; k < 4; k++) row[k] = mine ? lam[k] : 0.f;
    }
    if (O.resid && tid == 0) {
        st3(O.resid + r * 6, v3(e[0] / sf, e[1] / sf, e[2] / sf)); st3(O.resid + r * 6 + 3, v3(e[3] / sm, e[4] / sm, e[5] / sm));
    }
    if (O.net_wrench && tid == 0) {
        // one lane, the candidates in stored order: one summation order, no atomics (as invdyn_row)
        V3 Fs = v3(0.f, 0.f, 0.f), Ms = v3(0.f, 0.f, 0.f);
        for (int c = 0; c < ncon; c++) { const V3 fi = ld3(fc + 3 * c); Fs = Fs + fi; Ms = Ms + cross(ld3(s.con_pos + 3 * c), fi); }
        st3(O.net_wrench + r * 6, Fs); st3(O.net_wrench + r * 6 + 3, Ms);
    }
    if (O.info && tid < 8) {
        const float status = (float)((ncon == D_MAXCON ? EST_TRUNCATED : 0) | (conv ? 0 : EST_NOT_CONVERGED));
        const float v[8] = {cost0, cost, iters, nact, E.fn, searches, 0.f, status};
        float out = v[0];
#pragma unroll
        for (int k = 1; k < 8; k++) out = tid == k ? v[k] : out;
        O.info[r * 8 + tid] = out;
    }
}

// One wavefront per row.  OBJ: the rows carry static geoms (A.geoms / A.ngeom); a row with none of them runs the floor code on the same block.
template <bool OBJ>
__global__ __launch_bounds__(64) void k_estimate_contacts(EstimateArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using SL = typename std::conditional<OBJ, EnvLdsObj, EnvLds>::type;
    SL& s = *reinterpret_cast<SL*>(smem_raw);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= A.n_rows - A.row0) return;
    const size_t r = (size_t)A.row0 + blockIdx.x;
    const DevTables& T = A.T;
    float bad = 0.f;
    for (int i = tid; i < D_NQ; i += 64) { const float v = A.qpos[r * D_NQ + i]; s.qpos[i] = v; bad += isfinite(v) ? 0.f : 1.f; }
    for (int i = tid; i < D_NV; i += 64) {
        const float v = A.qvel ? A.qvel[r * D_NV + i] : 0.f, a = A.qacc ? A.qacc[r * D_NV + i] : 0.f;
        s.qvel[i] = v; s.qacc[i] = a; bad += (isfinite(v) && isfinite(a)) ? 0.f : 1.f;
        s.arm[i] = T.dof_armature[i]; s.dbody[i] = T.dof_body[i];
    }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bsub[tid] = T.body_subtree[tid]; s.bdep[tid] = T.body_depth[tid]; }
    for (int i = tid; i < 78; i += 64) s.applied[i] = 0.f;             // applied[6] ++ ctrl[72]: no force is applied
    if (tid == 0) { s.ncon = 0; s.nlim = 0; s.flag = 0; }
    int ngs = 0;
    if constexpr (OBJ) {
        ngs = min(max(A.ngeom[r], 0), D_MAXGEOM);                       // wave-uniform
        for (int i = tid; i < ngs * 17; i += 64) { const float v = A.geoms[r * D_MAXGEOM * 17 + i]; s.geom[i] = v; bad += isfinite(v) ? 0.f : 1.f; }
        if (tid < D_MAXGEOM) s.gobj[tid] = -1;                          // every geom static: no dynamic slot
        if (tid == 0) { s.ngeom_static = ngs; s.ngeom = ngs; s.nobj = 0; }
    }
    if (wave_sum(bad) != 0.f) { estimate_refuse(A.O, r, tid); return; }  // wave-uniform; before the collision pass indexes anything with it
    KP_SYNC();
    if constexpr (OBJ) {
        if (ngs > 0) { estimate_row<true>(s, A, r, tid); return; }
    }
    estimate_row<false>(static_cast<EnvLds&>(s), A, r, tid);
}

}  // namespace kp
