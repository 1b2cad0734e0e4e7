// kp_step_solve.hpp -- constraint rows and the Newton solver of the control step (make_constraint ... solve_constraints_direct).  Part of kp_step_device.hpp.
#pragma once
#include "kp_step_aba.hpp"

namespace kp {

// efc_D and the reference acceleration of every constraint row.  aref (contact-frame 3-vector) goes to jv3.
template <int NT, bool OBJ, class SL>
__device__ __forceinline__ void make_constraint(SL& s, const DevTables& T, const Params& P, int tid) {
    const V3 o = ld3(s.xpos);
    for (int c = tid; c < s.ncon; c += NT) {
        int b = s.con_body[c];
        float r = s.con_D[c] - P.margin;                    // collide() left the distance here
        float imp = impedance(P, r);
        float iwA = T.body_invw[b < D_NB ? b : 0];
        if (OBJ && b >= D_NB) iwA = as_obj(s).oc[13 * (b - D_NB) + 10];
        float iwB = 0.f;
        if (OBJ) {                                         // invweight0 of the surface's entity: static geom / object slot / floor (0)
            const EnvLdsObj& so = as_obj(s);
            const int b2 = so.con_b2[c];
            if (b2 >= D_NB) iwB = so.oc[13 * (b2 - D_NB) + 10]; else if (b2 < -1) iwB = so.geom[17 * (-2 - b2) + 16];
        }
        float dA = (iwA + iwB) * (1.0f + P.mu * P.mu);
        float Rn = fmaxf(1e-15f, (1.0f - imp) * dA / imp);
        s.con_D[c] = 1.0f / (2.0f * P.mu * P.mu * Rn);
        S6 cv = lds6(s.sv + 6 * b);                         // sv still holds cvel from forward_kin_bias (objects: obj_forward)
        V3 vp = cv.l + cross(cv.a, ld3(s.con_pos + 3 * c) - o);
        if (OBJ) {
            const int b2 = as_obj(s).con_b2[c];
            if (b2 >= 0) { const S6 c2 = lds6(s.sv + 6 * b2); vp = vp - (c2.l + cross(c2.a, ld3(s.con_pos + 3 * c) - o)); }
        }
        V3 vf = frame_comp(contact_frame<OBJ>(s, c), vp);
        s.jv3[3 * c] = -P.B * vf.x - P.K * imp * r; s.jv3[3 * c + 1] = -P.B * vf.y; s.jv3[3 * c + 2] = -P.B * vf.z;
    }
    for (int j = tid; j < D_NU; j += NT) {
        float sgn = 0.f, aref = 0.f, Dl = 0.f;
        if (P.limits && T.jnt_limited[j]) {
            float q = s.qpos[7 + j], dlo = q - T.jnt_lo[j], dhi = T.jnt_hi[j] - q;
            float dist = 0.f;
            if (dlo < 0.f) { sgn = 1.f; dist = dlo; } else if (dhi < 0.f) { sgn = -1.f; dist = dhi; }
            if (sgn != 0.f) {
                float imp = impedance(P, dist);
                Dl = 1.0f / fmaxf(1e-15f, (1.0f - imp) * T.lim_invw[j] / imp);
                aref = -P.B * (sgn * s.qvel[6 + j]) - P.K * imp * dist;
                atomicAdd(&s.nlim, 1);
            }
        }
        s.lim_jv[j] = aref; s.lim_D[j] = sgn * Dl;          // signed weight; aref sits in lim_jv until the first J search product
    }
    KP_SYNC();
}

// contact-frame residuals of all rows for the body spatial accelerations in acc (default: sv) and the generalized vector vec [- vec_b]:
// out3 = frame^T (point accel) [- aref] [+ jar3];  sub_aref: subtract the reference acceleration (jv3 / lim_jv);  add_base: add the
// residuals already in jar3 / lim_jar (rows are linear: residual(q + dq) = residual(q) + J dq)
template <int NT, bool OBJ, class SL>
__device__ __forceinline__ void eval_rows(SL& s, const float* vec, float* out3, float* lim_rows, bool sub_aref, int tid, const float* acc = nullptr, const float* vec_b = nullptr, bool add_base = false) {
    const V3 o = ld3(s.xpos);
    if (!acc) acc = s.sv;
    for (int c = tid; c < s.ncon; c += NT) {
        S6 S = lds6(acc + 6 * s.con_body[c]);
        V3 ap = S.l + cross(S.a, ld3(s.con_pos + 3 * c) - o);
        if (OBJ) {
            const int b2 = as_obj(s).con_b2[c];
            if (b2 >= 0) { const S6 S2 = lds6(acc + 6 * b2); ap = ap - (S2.l + cross(S2.a, ld3(s.con_pos + 3 * c) - o)); }
        }
        V3 a = frame_comp(contact_frame<OBJ>(s, c), ap);
        if (sub_aref) { a.x -= s.jv3[3 * c]; a.y -= s.jv3[3 * c + 1]; a.z -= s.jv3[3 * c + 2]; }
        if (add_base) { a.x += s.jar3[3 * c]; a.y += s.jar3[3 * c + 1]; a.z += s.jar3[3 * c + 2]; }
        out3[3 * c] = a.x; out3[3 * c + 1] = a.y; out3[3 * c + 2] = a.z;
    }
    for (int j = tid; j < D_NU; j += NT) {
        const float Ds = s.lim_D[j], sg = Ds > 0.f ? 1.f : (Ds < 0.f ? -1.f : 0.f);
        lim_rows[j] = sg != 0.f ? sg * (vec[6 + j] - (vec_b ? vec_b[6 + j] : 0.f)) - (sub_aref ? s.lim_jv[j] : 0.f) + (add_base ? s.lim_jar[j] : 0.f) : 0.f;
    }
    KP_SYNC();
}

// sa[b] = sum of the body wrenches sw over the subtree of b (bodies are in depth-first order: the subtree is [b, b + bsub[b])), summed in
// ascending body order.  The trip count is wave-uniform (the largest subtree among the wave's items) and the LDS reads go out in
// batches of 8 before the first add: a per-lane loop over its own subtree pays one LDS round trip per element (24 for the root).
// Reads past the subtree (at most 7 records, still inside EnvLds) are discarded by the select.
template <int NT, class SL>
__device__ __forceinline__ void subtree_sums(SL& s, int tid) {
    for (int base = 0; base < D_NB * 6; base += NT) {
        const int it = base + tid;
        const bool ok = it < D_NB * 6;
        const int b = ok ? it / 6 : 0, c = ok ? it - 6 * b : 0, n = ok ? (int)s.bsub[b] : 0;
        const float* src = s.sw + 6 * b + c;
        float acc = 0.f;
        for (int k0 = 0; __builtin_amdgcn_ballot_w64(k0 < n) != 0ull; k0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = src[6 * (k0 + j)];
#pragma unroll
            for (int j = 0; j < 8; j++) acc += (k0 + j < n) ? v[j] : 0.f;
        }
        if (ok) s.sa[it] = acc;
    }
    KP_SYNC();
}

// out = M (va - vb) (with_inertia; acc6 [24][6] must hold the body spatial accelerations of va - vb) - J^T f(jar) (with_forces)
template <int NT, bool OBJ, class SL>
// forces (optional): the contacts' world forces at the current residuals, [ncon][3], already evaluated (object kernels: con_prepare, lane = contact)
// bias / rhs (optional): body wrenches [24][6] added to, and a generalized force [75] subtracted from, the result: with the bias wrenches fb and
// rhs = qfrc_applied + qfrc_actuator, out = M va - qfrc_smooth - J^T f, the gradient of the primal problem without a detour through qacc_smooth
__device__ __forceinline__ void wrench_project(SL& s, const Params& P, const float* acc6, const float* va, const float* vb, float* out, bool with_inertia, bool with_forces, int tid,
                                               const float* arm, const float* forces = nullptr, const float* bias = nullptr, const float* rhs = nullptr) {
    if (tid < D_NB) {
        const int b = tid;
        S6 W = with_inertia ? inert_mul(s.cinert + 10 * b, lds6(acc6 + 6 * b)) : S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
        if (bias) W = W + lds6(bias + 6 * b);
        if (with_forces) {
            const int c0 = s.con_start[b], c1 = s.con_start[b + 1];
            if (c1 > c0) {
                const V3 o = ld3(s.xpos);
                if (forces) {
                    V3 Fn = ld3(forces + 3 * c0), pn = ld3(s.con_pos + 3 * c0);
                    for (int c = c0; c < c1; c++) {
                        const V3 F = Fn, p = pn - o;
                        const int cn = min(c + 1, c1 - 1);
                        Fn = ld3(forces + 3 * cn); pn = ld3(s.con_pos + 3 * cn);
                        W.a = W.a - cross(p, F); W.l = W.l - F;
                    }
                } else {
                // the next contact's operands are requested before this one's arithmetic (one LDS round trip for the loop, not one per contact)
                float Dn = s.con_D[c0];
                V3 jn3 = ld3(s.jar3 + 3 * c0), pn = ld3(s.con_pos + 3 * c0);
                for (int c = c0; c < c1; c++) {
                    const float Dc = Dn, jn = jn3.x, jt1 = jn3.y, jt2 = jn3.z;
                    const V3 p = pn - o;
                    const int cn = min(c + 1, c1 - 1);
                    Dn = s.con_D[cn]; jn3 = ld3(s.jar3 + 3 * cn); pn = ld3(s.con_pos + 3 * cn);
                    float fe[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) { float x = row_val(e, P.mu, jn, jt1, jt2); fe[e] = x < 0.f ? -Dc * x : 0.f; }
                    // sum_e f_e (n +- mu t_k) in frame coordinates, then to world
                    const V3 F = frame_world(contact_frame<OBJ>(s, c), v3(fe[0] + fe[1] + fe[2] + fe[3], P.mu * (fe[0] - fe[1]), P.mu * (fe[2] - fe[3])));
                    W.a = W.a - cross(p, F); W.l = W.l - F;
                }
                }
            }
        }
        sts6(s.sw + 6 * b, W);
    }
    KP_SYNC();
    subtree_sums<NT>(s, tid);
    for (int d = tid; d < D_NV; d += NT) {
        float v = dot6(lds6(s.cdof + 6 * d), lds6(s.sa + 6 * s.dbody[d]));
        if (with_inertia) v += arm[d] * (va[d] - (vb ? vb[d] : 0.f));
        if (with_forces && d >= 6) { float jr = s.lim_jar[d - 6]; if (jr < 0.f) v += s.lim_D[d - 6] * jr; }      // - sign * (-D jar): lim_D is signed
        if (rhs) v -= rhs[d];
        out[d] = v;
    }
    KP_SYNC();
}

// 0.5 a^T I_b b summed over the bodies + 0.5 arm x y over the dofs: lane partial of  0.5 x^T M y  for the generalized vectors x, y
// whose body spatial accelerations are acca / accb (xa - xb and ya - yb give the dof vectors; xb / yb may be null)
template <int NT, class SL>
// arm: the dof armature (the layout's own copy, or the model table where the layout keeps none)
__device__ __forceinline__ float quad_form_M(const SL& s, const float* arm, const float* acca, const float* accb, const float* xa, const float* xb, const float* ya, const float* yb, int tid) {
    float c = 0.f;
    if (tid < D_NB) c += 0.5f * dot6(lds6(acca + 6 * tid), inert_mul(s.cinert + 10 * tid, lds6(accb + 6 * tid)));
    for (int i = tid; i < D_NV; i += NT) c += 0.5f * arm[i] * (xa[i] - (xb ? xb[i] : 0.f)) * (ya[i] - (yb ? yb[i] : 0.f));
    return c;
}

// spatial "acceleration" of every body induced by a generalized vector (what aba_solve leaves in sv).  Each body's own share
// da_b = sum_j vec_j cdof_j is formed body-parallel first, so the level-synchronous chain is one 6-vector add per level (as in the kinematics).
template <int NT, class SL>
__device__ __forceinline__ void spatial_accumulate(SL& s, const float* vec, int depth, int tid, float* out = nullptr) {
    if (!out) out = s.sv;
    S6 da = S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
    if (tid < D_NB) {
        const int b = tid, nd = b == 0 ? 6 : 3, d0 = b == 0 ? 0 : 6 + 3 * (b - 1);
        for (int j = 0; j < nd; j++) da = da + vec[d0 + j] * lds6(s.cdof + 6 * (d0 + j));
        if (b == 0) sts6(out, da);
    }
    KP_SYNC();
#pragma nounroll
    for (int lev = 1; lev < D_NLEV; lev++) {
        if (depth == lev) sts6(out + 6 * tid, lds6(out + 6 * s.bpar[tid]) + da);
        KP_SYNC();
    }
}

// records the active pyramid rows of every contact; returns 1 on the lanes that saw a change since the last call.  deep: running
// maximum of the tree level of the hulls that carry an active row (first_clean_level's contact half, from the same row values)
template <int NT, class SL>
__device__ __forceinline__ float active_set_changed(SL& s, const Params& P, int tid, float& deep) {
    float changed = 0.f;
    for (int c = tid; c < s.ncon; c += NT) {
        const float jn = s.jar3[3 * c], jt1 = s.jar3[3 * c + 1], jt2 = s.jar3[3 * c + 2];
        unsigned m = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) m |= (row_val(e, P.mu, jn, jt1, jt2) < 0.f ? 1u : 0u) << e;
        if (m != s.con_act[c]) changed = 1.f;
        s.con_act[c] = (unsigned char)m;
        const int b = s.con_body[c];
        if (m != 0u && b < D_NB) deep = fmaxf(deep, (float)s.bdep[b]);      // object-side contacts do not touch the humanoid tree
    }
    return changed;
}

// first tree level below every active constraint: 1 + the deepest level holding a body with an active contact row or a dof with
// an active joint limit (jar < 0); the root level always counts as dirty.  deep: per-lane maxima gathered by active_set_changed and
// the gradient loop
template <int NT, class SL>
__device__ __forceinline__ int first_clean_level(SL& s, float deep, int tid) {
    float m = -wave_min(-deep);
    if (NT > 64) {
        KP_SYNC();
        if ((tid & 63) == 0) s.red[tid >> 6] = m;
        KP_SYNC();
        m = s.red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; w++) m = fmaxf(m, s.red[w]);
        KP_SYNC();
    }
    return (int)m + 1;
}

// exact minimiser of the cost along the search direction: root of phi'(alpha) = g0 + alpha h0 + sum_rows D (jar + alpha jv)_- jv by
// safeguarded Newton steps on the piecewise-linear phi'.  Every lane keeps its rows in registers for the whole search -- one contact
// (four pyramid rows a + alpha b with a = row(jar), b = row(jv)) and ceil(69 / NT) joint-limit rows -- so an evaluation is a few
// FMAs per row and two wave sums, without LDS traffic.  rowcost: the rows' share of the cost at the returned alpha.
// ROWCOST = false leaves rowcost alone (rounds 1 - 2: the object kernel kept its full cost evaluation because three more live values across
// the search moved spills into its articulated-body loops; since the round-3 register discipline both solvers take the closed form)
template <int NT, bool ROWCOST = true, class SL>
// want_rc0: rc0 receives the rows' share of the cost at alpha = 0, i.e. at the iterate the search starts from (the solve's first iteration has no
// previous line search to take it from)
__device__ __forceinline__ float line_search(SL& s, const Params& P, float g0, float h0, int tid, float& rowcost, bool want_rc0, float& rc0) {
    static_assert(SL::MAXCON <= 64 && NT >= 64, "one contact per lane");
    float ra[4], rb[4], rD[4], Dc;
    {
        const bool ok = tid < s.ncon;
        const int k = ok ? tid : 0;
        Dc = ok ? s.con_D[k] : 0.f;
        const float jn = ok ? s.jar3[3 * k] : 0.f, jt1 = ok ? s.jar3[3 * k + 1] : 0.f, jt2 = ok ? s.jar3[3 * k + 2] : 0.f;
        const float vn = ok ? s.jv3[3 * k] : 0.f, vt1 = ok ? s.jv3[3 * k + 1] : 0.f, vt2 = ok ? s.jv3[3 * k + 2] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) { ra[e] = row_val(e, P.mu, jn, jt1, jt2); rb[e] = row_val(e, P.mu, vn, vt1, vt2); rD[e] = Dc * rb[e]; }
    }
    constexpr int LR = (D_NU + NT - 1) / NT;
    float la[LR], lb[LR], lD[LR], lW[LR];
#pragma unroll
    for (int n = 0; n < LR; n++) {
        const int j = tid + n * NT, jj = j < D_NU ? j : 0;
        const bool ok = j < D_NU && s.lim_D[jj] != 0.f;
        const float w = ok ? fabsf(s.lim_D[jj]) : 0.f;
        if (ROWCOST) lW[n] = w;
        la[n] = ok ? s.lim_jar[jj] : 0.f; lb[n] = ok ? s.lim_jv[jj] : 0.f; lD[n] = w * lb[n];
    }
    if (ROWCOST && want_rc0) {
        float rc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) if (ra[e] < 0.f) rc += 0.5f * Dc * ra[e] * ra[e];
#pragma unroll
        for (int n = 0; n < LR; n++) if (la[n] < 0.f) rc += 0.5f * lW[n] * la[n] * la[n];
        rc0 = block_sum<NT>(s, rc, tid);
    }
    // The search direction solves H search = -grad with the Hessian of the current active set, so phi'(0) = -phi''(0) and the Newton
    // step from alpha = 0 is 1: the first evaluation happens there, bracketed by lo = 0 (descent direction).
    float alpha = 1.f, lo = 0.f, hi = 3.0e38f;
    for (int ls = 0; ls < 20; ls++) {
        float d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) { const float x = fmaf(alpha, rb[e], ra[e]); if (x < 0.f) { d1 += x * rD[e]; d2 += rb[e] * rD[e]; } }
#pragma unroll
        for (int n = 0; n < LR; n++) { const float x = fmaf(alpha, lb[n], la[n]); if (x < 0.f) { d1 += x * lD[n]; d2 += lb[n] * lD[n]; } }
        d1 = block_sum<NT>(s, d1, tid); d2 = block_sum<NT>(s, d2, tid);
        const float dphi = g0 + alpha * h0 + d1, ddphi = h0 + d2;
        if (!(ddphi > 0.f)) { if (ls == 0) alpha = 0.f; break; }
        if (dphi < 0.f) lo = alpha; else hi = alpha;
        float an = alpha - dphi * rcp_nr(ddphi);
        if (!(an > lo && an < hi)) an = hi < 1.0e38f ? 0.5f * (lo + hi) : 2.0f * alpha + 1.0f;
        const float step = an - alpha;
        alpha = an;
        if (fabsf(step) <= 1e-6f * fabsf(alpha)) break;
    }
    if (ROWCOST) {   // constraint part of the cost at the step taken: sum over the rows of 0.5 D (a + alpha b)_-^2 (the caller adds the Gauss term in closed form)
        float rc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) { const float x = fmaf(alpha, rb[e], ra[e]); if (x < 0.f) rc += 0.5f * Dc * x * x; }
#pragma unroll
        for (int n = 0; n < LR; n++) { const float x = fmaf(alpha, lb[n], la[n]); if (x < 0.f) rc += 0.5f * lW[n] * x * x; }
        rowcost = block_sum<NT>(s, rc, tid);
    }
    return alpha;
}

// Constraint solve: Newton on the primal problem (mj_solNewton) with an exact line search, WITHOUT qacc_smooth.  Returns iterations.
// mj_fwdConstraint evaluates two starting points -- qacc_smooth and the warm start -- and iterates from the cheaper one (rounds 1 - 2 did the
// same); the primal problem is strictly convex, so its minimiser does not depend on the starting point, and its cost
//     0.5 (a - a_s)^T M (a - a_s) + s(J a - aref)  =  0.5 a^T M a - a^T qfrc_smooth + s(J a - aref) + const
// needs a_s = M^-1 qfrc_smooth neither for the gradient (M a - qfrc_smooth - J^T f, in body form: I_b sacc_b + fb_b - contact wrenches, projected)
// nor for the termination tests (|gradient| and the cost DIFFERENCE of consecutive iterates, exact in closed form along the search direction).
// So the solve starts from the warm start always, and the substep's "smooth" articulated-body factorisation + solve (a fifth of a substep) is not
// run at all: the FIRST Newton factorisation walks every tree level and so leaves M's own factors on the clean levels, which the later
// factorisations of the substep reuse exactly as they reused the smooth solve's.  Without constraint rows qacc = M^-1 qfrc_smooth is one plain solve.
// Results agree with the two-candidate form to the solver's tolerance; the iteration path is MuJoCo's whenever MuJoCo starts from its warm start.
// On entry: s.qacc = warm start, jv3 / lim_jv = aref, s.applied ++ s.ctrl = qfrc_applied + qfrc_actuator, s.fb = bias wrenches.
template <int NT, class SL>
__device__ __forceinline__ int solve_constraints_direct(SL& s, const Params& P, const Lane8& L8, int depth, int tid, int& nfact, int& ncap, const float* arm) {
    if (s.ncon == 0 && s.nlim == 0) {
        aba_solve<NT, false>(s, P, L8, s.applied, s.qacc, false, tid, D_NLEV, s.fb);
        return 0;
    }
    float* sacc;               // [24][6] spatial accelerations of the bodies induced by the iterate qacc: over Mv + mres; lean layout: over qpos | qvel (restored by step_body)
    if constexpr (SL::LEAN) sacc = s.qpos; else sacc = s.Mv;
    float* grad = s.qacc_s;    // the words qacc_smooth would occupy
    spatial_accumulate<NT>(s, s.qacc, depth, tid, sacc);
    eval_rows<NT, false>(s, s.qacc, s.jar3, s.lim_jar, true, tid, sacc);
    float rowcost = 0.f;       // the rows' share of the cost at the iterate (the first line search evaluates it at alpha = 0)
    int it = 0, lev_hist = 1;
    bool done = false;          // left the loop through one of mj_solNewton's termination tests (not the iteration cap)
    const unsigned conlev = contact_levels(s, L8);
    // active set of the iterate: pyramid rows (con_act) and joint limits (their D as extra armature); changed = it differs from the set of the last call
    float changed = 0.f, deep = 0.f;
    auto active_set = [&]() {
        changed = 0.f; deep = 0.f;
        for (int i = tid; i < D_NV; i += NT) {
            const float ex = (i >= 6 && s.lim_jar[i - 6] < 0.f) ? fabsf(s.lim_D[i - 6]) : 0.f;
            const float st = SL::LEAN ? arm[i] + ex : ex;          // lean layout: extra holds armature + extra, the sum aba_elim3 forms on the full layout
            if (st != s.extra[i]) changed = 1.f;
            s.extra[i] = st;
            if (ex != 0.f) deep = fmaxf(deep, (float)s.bdep[s.dbody[i]]);     // active joint limit: its body's level is dirty
        }
        changed += active_set_changed<NT>(s, P, tid, deep);
        changed = (NT == 64) ? (__ballot(changed > 0.f) != 0ull ? 1.f : 0.f) : block_sum<NT>(s, changed, tid);
        KP_SYNC();
    };
    active_set();
    for (; it < P.max_iter; it++) {
        wrench_project<NT, false>(s, P, sacc, s.qacc, nullptr, grad, true, true, tid, arm, nullptr, s.fb, s.applied);
        float g2 = 0.f;
        for (int i = tid; i < D_NV; i += NT) { const float g = grad[i]; g2 += g * g; s.x[i] = -g; }
        g2 = block_sum<NT>(s, g2, tid);
        KP_SYNC();
        if (P.scale * sqrtf(g2) < P.tol) { done = true; break; }
        if (it == 0 || changed > 0.f) {
            const int clean = first_clean_level<NT>(s, deep, tid);
            lev_hist = max(lev_hist, clean);
            // first factorisation of the substep: every level (its clean levels ARE M's factors from then on)
            aba_solve<NT, false>(s, P, L8, s.x, s.search, true, tid, it == 0 ? D_NLEV : lev_hist, nullptr, conlev);
            nfact++;
        }
        else aba_resolve(s, L8, s.x, nullptr, s.search);
        eval_rows<NT, false>(s, s.search, s.jv3, s.lim_jv, false, tid);           // aref (in jv3) is folded into jar3 by now
        // phi(alpha) = cost(qacc + alpha search): smooth part g0 = search^T (M qacc - qfrc_smooth), h0 = search^T M search, in body form
        float g0 = 2.0f * quad_form_M<NT>(s, arm, s.sv, sacc, s.search, nullptr, s.qacc, nullptr, tid);
        float h0 = 2.0f * quad_form_M<NT>(s, arm, s.sv, s.sv, s.search, nullptr, s.search, nullptr, tid);
        for (int i = tid; i < D_NB * 6; i += NT) g0 += s.sv[i] * s.fb[i];
        for (int i = tid; i < D_NV; i += NT) g0 -= s.search[i] * s.applied[i];
        g0 = block_sum<NT>(s, g0, tid); h0 = block_sum<NT>(s, h0, tid);
        float rownew, rc0 = 0.f;
        const float alpha = line_search<NT>(s, P, g0, h0, tid, rownew, it == 0, rc0);
        if (it == 0) rowcost = rc0;
        if (!(alpha > 0.f)) { done = true; break; }
        for (int i = tid; i < D_NV; i += NT) s.qacc[i] += alpha * s.search[i];
        for (int i = tid; i < D_NB * 6; i += NT) sacc[i] += alpha * s.sv[i];
        for (int k = tid; k < 3 * s.ncon; k += NT) s.jar3[k] += alpha * s.jv3[k];
        for (int j = tid; j < D_NU; j += NT) if (s.lim_D[j] != 0.f) s.lim_jar[j] += alpha * s.lim_jv[j];
        KP_SYNC();
        // cost(old) - cost(new): the smooth part is an exact quadratic along the search direction, the rows' share comes out of the line search
        const float improvement = P.scale * ((rowcost - rownew) - alpha * (g0 + 0.5f * alpha * h0));
        rowcost = rownew;
        if (improvement < P.tol) { it++; done = true; break; }
        // The Newton step of a model that was exact: the search direction solved H search = -gradient for the active set of the old iterate and the new
        // iterate has the same active set -- on a piecewise-quadratic cost its gradient is then (1 - alpha) x the old one, alpha = 1 up to the line
        // search's rounding.  When that bound already passes mj_solNewton's |gradient| < tolerance test, the pass that would evaluate the gradient at
        // the top of the next iteration (body wrenches, subtree sums, projection: a sixth of an iteration's work) is not run to confirm it.
        active_set();
        if (changed == 0.f && P.scale * fabsf(1.0f - alpha) * sqrtf(g2) < P.tol) { it++; done = true; break; }     // gradient(new) = (1 - alpha) gradient(old) on an unchanged active set
    }
    if (!done) ncap++;
    return it;
}

}  // namespace kp
