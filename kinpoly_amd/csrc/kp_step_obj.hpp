// kp_step_obj.hpp -- dynamic free objects in the control step (inert_entry ... solve_constraints_obj).  Part of kp_step_device.hpp.
#pragma once
#include "kp_step_solve.hpp"

namespace kp {

// ---------------------------------------------------------------- dynamic free objects (OBJ kernels; one wave per env)
// An object is one more rigid body whose unknown in the Newton solve is its spatial acceleration about o (a linear
// re-parametrisation of its six free-joint accelerations, under which Newton steps and the exact line search are invariant).
// Oracle counterpart: kpo_obj_forward + the object columns of kpo_make_constraint / kpo_solve_constraint.

// 6x6 entry of a 10-float spatial inertia [Ixx Iyy Izz Ixy Ixz Iyz | h | m]
__device__ __forceinline__ float inert_entry(const float* I, int r, int c) {
    if (r > c) { const int t = r; r = c; c = t; }
    if (c < 3) return r == c ? I[r] : I[2 + r + c];
    if (r >= 3) return r == c ? I[9] : 0.f;
    const int l = c - 3;
    if (r == l) return 0.f;
    return ((l == (r + 2) % 3) ? 1.f : -1.f) * I[6 + (3 - r - l)];
}
__device__ __forceinline__ S6 unit6(int j) { return S6{v3(j == 0, j == 1, j == 2), v3(j == 3, j == 4, j == 5)}; }

// D F G F^T a: the active pyramid rows of contact c applied to a point acceleration (world components)
__device__ __forceinline__ V3 con_DG(const EnvLdsObj& s, const Params& P, int c, V3 a) {
    const float mu = P.mu, mu2 = mu * mu, Dc = s.con_D[c], jn = s.jar3[3 * c], jt1 = s.jar3[3 * c + 1], jt2 = s.jar3[3 * c + 2];
    const float a0 = row_val(0, mu, jn, jt1, jt2) < 0.f, a1 = row_val(1, mu, jn, jt1, jt2) < 0.f;
    const float a2 = row_val(2, mu, jn, jt1, jt2) < 0.f, a3 = row_val(3, mu, jn, jt1, jt2) < 0.f;
    const float gnn = a0 + a1 + a2 + a3, g11 = mu2 * (a0 + a1), g22 = mu2 * (a2 + a3), gn1 = mu * (a0 - a1), gn2 = mu * (a2 - a3);
    const Frame fr = contact_frame<true>(s, c);
    const V3 pf = frame_comp(fr, a);
    return frame_world(fr, v3(Dc * (gnn * pf.x + gn1 * pf.y + gn2 * pf.z), Dc * (gn1 * pf.x + g11 * pf.y), Dc * (gn2 * pf.x + g22 * pf.z)));
}
// K_c acc: the wrench (about o) contact c's active rows put on a body accelerating with acc
__device__ __forceinline__ S6 con_K(const EnvLdsObj& s, const Params& P, int c, S6 acc, V3 o) {
    const V3 p = ld3(s.con_pos + 3 * c) - o;
    const V3 w = con_DG(s, P, c, acc.l + cross(acc.a, p));
    return S6{cross(p, w), w};
}
// contact force (world) of contact c at the current residuals, acting on the entity that carries the vertex
__device__ __forceinline__ V3 con_force(const EnvLdsObj& s, const Params& P, int c) {
    const float Dc = s.con_D[c], jn = s.jar3[3 * c], jt1 = s.jar3[3 * c + 1], jt2 = s.jar3[3 * c + 2];
    float fe[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { const float x = row_val(e, P.mu, jn, jt1, jt2); fe[e] = x < 0.f ? -Dc * x : 0.f; }
    return frame_world(contact_frame<true>(s, c), v3(fe[0] + fe[1] + fe[2] + fe[3], P.mu * (fe[0] - fe[1]), P.mu * (fe[2] - fe[3])));
}

// pose-dependent quantities of the objects (lane = slot), their world geoms (lane = geom); spatial velocity -> sv[24 + k]
__device__ __forceinline__ void obj_forward(EnvLdsObj& s, const DevTables& T, const Params& P, int tid) {
    const V3 o = ld3(s.xpos);
    if (tid < s.nobj) {
        const int k = tid;
        float* q = s.oq + 7 * k;
        const Q4 qq = qnormalize(Q4{q[3], q[4], q[5], q[6]});
        q[3] = qq.w; q[4] = qq.x; q[5] = qq.y; q[6] = qq.z;
        float R[9];
        q2mat(qq, R);
#pragma unroll
        for (int i = 0; i < 9; i++) s.oR[9 * k + i] = R[i];
        const float* C = s.oc + 13 * k;
        const float mass = C[0], arm = C[12];
        const V3 xp = ld3(q), com = xp + mulmat(R, ld3(C + 1));
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
        const V3 rr = com - o, ra = xp - o;
        const float r2 = dot(rr, rr), a2 = dot(ra, ra);
        float* ci = s.oI + 10 * k;
        ci[0] = W[0] + mass * (r2 - rr.x * rr.x); ci[1] = W[4] + mass * (r2 - rr.y * rr.y); ci[2] = W[8] + mass * (r2 - rr.z * rr.z);
        ci[3] = W[1] - mass * rr.x * rr.y; ci[4] = W[2] - mass * rr.x * rr.z; ci[5] = W[5] - mass * rr.y * rr.z;
        ci[6] = mass * rr.x; ci[7] = mass * rr.y; ci[8] = mass * rr.z; ci[9] = mass;
        // the free joint's armature (diagonal in joint coordinates) = a point mass at the body origin + an isotropic rotor
        float* ce = s.oIe + 10 * k;
        ce[0] = ci[0] + arm * (a2 - ra.x * ra.x) + arm; ce[1] = ci[1] + arm * (a2 - ra.y * ra.y) + arm; ce[2] = ci[2] + arm * (a2 - ra.z * ra.z) + arm;
        ce[3] = ci[3] - arm * ra.x * ra.y; ce[4] = ci[4] - arm * ra.x * ra.z; ce[5] = ci[5] - arm * ra.y * ra.z;
        ce[6] = ci[6] + arm * ra.x; ce[7] = ci[7] + arm * ra.y; ce[8] = ci[8] + arm * ra.z; ce[9] = ci[9] + arm;
        const V3 vl = ld3(s.ov + 6 * k), ww = mulmat(R, ld3(s.ov + 6 * k + 3));
        const S6 cv = S6{ww, vl - cross(ww, ra)};
        const S6 ca = S6{v3(0.f, 0.f, 0.f), v3(-P.gx, -P.gy, -P.gz) + cross(vl, ww)};
        sts6(s.ofb + 6 * k, inert_mul(ci, ca) + cross_force(cv, inert_mul(ci, cv)));
        sts6(s.sv + 6 * (D_NB + k), cv);
        // warm start: joint-space acceleration of the previous solve -> spatial acceleration in this pose
        const V3 al_q = ld3(s.oqa + 6 * k), aa = mulmat(R, ld3(s.oqa + 6 * k + 3));
        sts6(s.oa + 6 * k, S6{aa, al_q - cross(aa, ra)});
    }
    KP_SYNC();
    if (tid >= s.ngeom_static && tid < s.ngeom) {
        const int k = s.gobj[tid];
        const float* l = T.obj_geoms + 18 * s.ggi[tid] + 1;      // body-frame geom: type, size[3], pos[3], mat[9] (L2-resident table)
        const float* R = s.oR + 9 * k;
        float* g = s.geom + 17 * tid;
        g[0] = l[0]; g[1] = l[1]; g[2] = l[2]; g[3] = l[3];
        st3(g + 4, ld3(s.oq + 7 * k) + mulmat(R, ld3(l + 4)));
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) g[7 + 3 * i + j] = R[3 * i] * l[7 + j] + R[3 * i + 1] * l[10 + j] + R[3 * i + 2] * l[13 + j];
        g[16] = s.oc[13 * k + 10];
    }
    KP_SYNC();
}

// The <= 12 x 12 SPD object system, one row per lane, held in registers (row stride 13 in s.Sm, right-hand side in column n).
// Gaussian elimination with the pivot row broadcast by v_readlane; rows >= n are identity padding.  refactor = false reuses the
// multipliers / upper triangle a previous call stored back to s.Sm and only pushes a new right-hand side through them.
// NN = 6 or 12: compiled for one and for two simulated objects (the elimination is unrolled over NN columns; most scenes hold one object)
template <int NN>
__device__ __forceinline__ void dense_solve_n(EnvLdsObj& s, int n, int tid, bool refactor) {
    constexpr int ST = 6 * D_MAXOBJ + 1;
    float a[NN + 1];
    const bool rowok = tid < n;
#pragma unroll
    for (int c = 0; c < NN; c++) a[c] = (rowok && c < n) ? s.Sm[tid * ST + c] : (c == tid ? 1.f : 0.f);
    a[NN] = rowok ? s.Sm[tid * ST + n] : 0.f;
#pragma unroll
    for (int j = 0; j < NN; j++) {
        const float pinv = 1.0f / __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[j]), j));
        const bool lower = tid > j;
        const float l = refactor ? (lower ? a[j] * pinv : 0.f) : (lower ? a[j] : 0.f);
        if (refactor) {
#pragma unroll
            for (int c = j + 1; c < NN; c++) a[c] -= l * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[c]), j));
            if (lower) a[j] = l;
        }
        a[NN] -= l * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[NN]), j));
    }
#pragma unroll
    for (int j = NN - 1; j >= 0; j--) {
        const float xj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[NN] / a[j]), j));
        if (tid == j) a[NN] = xj;
        if (tid < j) a[NN] -= a[j] * xj;
    }
    if (rowok) {
        if (refactor) {
#pragma unroll
            for (int c = 0; c < NN; c++) if (c < n) s.Sm[tid * ST + c] = a[c];
        }
        s.Sm[tid * ST + n] = a[NN];
    }
    KP_SYNC();
}
__device__ __forceinline__ void dense_solve(EnvLdsObj& s, int n, int tid, bool refactor) {
    if (n <= 6) dense_solve_n<6>(s, n, tid, refactor); else dense_solve_n<6 * D_MAXOBJ>(s, n, tid, refactor);
}

// per contact (lane = contact): the active-row matrix D F G F^T and the contact force at the current residuals
template <int NT>
__device__ __forceinline__ void con_prepare(EnvLdsObj& s, const Params& P, int tid) {
    for (int c = tid; c < s.ncon; c += NT) {
        const V3 mx = con_DG(s, P, c, v3(1.f, 0.f, 0.f)), my = con_DG(s, P, c, v3(0.f, 1.f, 0.f)), mz = con_DG(s, P, c, v3(0.f, 0.f, 1.f));
        float* m = s.cM + 6 * c;
        m[0] = mx.x; m[1] = my.y; m[2] = mz.z; m[3] = mx.y; m[4] = mx.z; m[5] = my.z;
        st3(s.jv3 + 3 * c, con_force(s, P, c));    // contact forces live in jv3 (the previous search direction's rows: dead since the update) until this iteration's eval_rows
    }
    KP_SYNC();
}
// K_c acc from the prepared matrix
__device__ __forceinline__ S6 con_Kp(const EnvLdsObj& s, int c, S6 acc, V3 o) {
    const V3 p = ld3(s.con_pos + 3 * c) - o;
    const V3 a = acc.l + cross(acc.a, p);
    const float* m = s.cM + 6 * c;
    const V3 w = v3(m[0] * a.x + m[3] * a.y + m[4] * a.z, m[3] * a.x + m[1] * a.y + m[5] * a.z, m[4] * a.x + m[5] * a.y + m[2] * a.z);
    return S6{cross(p, w), w};
}
__device__ __forceinline__ S6 wave_sum6(S6 v) {
    return S6{v3(wave_sum(v.a.x), wave_sum(v.a.y), wave_sum(v.a.z)), v3(wave_sum(v.l.x), wave_sum(v.l.y), wave_sum(v.l.z))};
}

// sum of V per-lane values over the 64 lanes (lane = contact): four DPP exchanges inside each 16-lane row, the four row sums meet
// in LDS.  Deterministic order.  Lane v < V returns sum v.
__device__ __forceinline__ float row_sum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}
template <int V>
__device__ __forceinline__ float lanes_sum(EnvLdsObj& s, const float* vals, int tid) {
    static_assert(V <= 21, "red[] holds 4 x 21 partials");
#pragma unroll
    for (int v = 0; v < V; v++) {
        const float r = row_sum16(vals[v]);
        if ((tid & 15) == 0) s.red[(tid >> 4) * 21 + v] = r;
    }
    KP_SYNC();
    const float out = tid < V ? (s.red[tid] + s.red[21 + tid]) + (s.red[42 + tid] + s.red[63 + tid]) : 0.f;
    KP_SYNC();
    return out;                                                     // lane v < V holds sum v
}

// object rows of the Newton system: Sm = blockdiag(I_eff) + sum of the active contact matrices K_c = P M_c P^T over the contacts that
// touch an object (own block +K_c, object-object block -K_c); column n = sign * rhs.  Lane = contact: every lane forms the 21 unique
// entries of its K_c = [[X M X^T, X M], [M X^T, M]] (X = [p]x), then one wave-wide vector sum per block.
__device__ __forceinline__ void obj_hessian(EnvLdsObj& s, const Params& P, const float* rhs, float sign, int tid) {
    constexpr int ST = 6 * D_MAXOBJ + 1;
    const int nobj = s.nobj, n = 6 * nobj;
    const V3 o = ld3(s.xpos);
    const bool have = tid < s.ncon;
    const int c = have ? tid : 0;
    const int A = have ? s.con_body[c] : -1, B = have ? (int)s.con_b2[c] : -1;
    float K[21];
    {
        const V3 p = ld3(s.con_pos + 3 * c) - o;
        const float* m = s.cM + 6 * c;
        const V3 m0 = v3(m[0], m[3], m[4]), m1 = v3(m[3], m[1], m[5]), m2 = v3(m[4], m[5], m[2]);     // columns (= rows) of M
        const V3 b0 = cross(p, m0), b1 = cross(p, m1), b2 = cross(p, m2);                               // B = X M, column j = p x M[:, j]
        // rows of B: B_i = (b0[i], b1[i], b2[i]); A = X M X^T, row i = p x B_i
        const V3 a0 = cross(p, v3(b0.x, b1.x, b2.x)), a1 = cross(p, v3(b0.y, b1.y, b2.y)), a2 = cross(p, v3(b0.z, b1.z, b2.z));
        K[s6i(0, 0)] = a0.x; K[s6i(0, 1)] = a0.y; K[s6i(0, 2)] = a0.z; K[s6i(1, 1)] = a1.y; K[s6i(1, 2)] = a1.z; K[s6i(2, 2)] = a2.z;
        K[s6i(0, 3)] = b0.x; K[s6i(0, 4)] = b1.x; K[s6i(0, 5)] = b2.x;
        K[s6i(1, 3)] = b0.y; K[s6i(1, 4)] = b1.y; K[s6i(1, 5)] = b2.y;
        K[s6i(2, 3)] = b0.z; K[s6i(2, 4)] = b1.z; K[s6i(2, 5)] = b2.z;
        K[s6i(3, 3)] = m[0]; K[s6i(3, 4)] = m[3]; K[s6i(3, 5)] = m[4]; K[s6i(4, 4)] = m[1]; K[s6i(4, 5)] = m[5]; K[s6i(5, 5)] = m[2];
    }
    // lane v < 21 owns unique entry v: its (r, cc)
    int er = 0, ec = tid;
#pragma unroll
    for (int r = 0; r < 5; r++) if (ec >= 6 - er && er == r) { ec -= 6 - er; er++; }
    ec += er;
    for (int blk = 0; blk < (nobj == 2 ? 3 : 1); blk++) {           // blocks (0,0), (1,1), (0,1)
        const int k = blk == 1 ? 1 : 0;
        float w;
        if (blk < 2) w = (have && (A == D_NB + k || B == D_NB + k)) ? 1.f : 0.f;
        else w = (have && A >= D_NB && B >= D_NB) ? -1.f : 0.f;
        float vals[21];
#pragma unroll
        for (int v = 0; v < 21; v++) vals[v] = w * K[v];
        const float sum = lanes_sum<21>(s, vals, tid);
        if (tid < 21) {
            if (blk < 2) {
                const float v = sum + inert_entry(s.oIe + 10 * k, er, ec);
                s.Sm[(6 * k + er) * ST + 6 * k + ec] = v; s.Sm[(6 * k + ec) * ST + 6 * k + er] = v;
            } else {                                                 // K symmetric: block (0,1) = -K, block (1,0) = -K^T = -K
                s.Sm[er * ST + 6 + ec] = sum; s.Sm[ec * ST + 6 + er] = sum; s.Sm[(6 + ec) * ST + er] = sum; s.Sm[(6 + er) * ST + ec] = sum;
            }
        }
    }
    if (tid < n) s.Sm[tid * ST + n] = sign * rhs[tid];
    KP_SYNC();
}

// out[6k..] = sum over the hull contacts whose surface belongs to object k of K_c sv[hull]   (= -H_oh y for the y behind sv)
__device__ __forceinline__ void obj_coupling_u(EnvLdsObj& s, const Params& P, float* out, int tid) {
    const V3 o = ld3(s.xpos);
    const bool have = tid < s.con_start[D_NB];
    const int c = have ? tid : 0;
    const int B = have ? (int)s.con_b2[c] : -1;
    const S6 w = con_Kp(s, c, lds6(s.sv + 6 * s.con_body[c]), o);
    float vals[12];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float f = B == D_NB + k ? 1.f : 0.f;
        vals[6 * k] = f * w.a.x; vals[6 * k + 1] = f * w.a.y; vals[6 * k + 2] = f * w.a.z; vals[6 * k + 3] = f * w.l.x; vals[6 * k + 4] = f * w.l.y; vals[6 * k + 5] = f * w.l.z;
    }
    const float sum = lanes_sum<12>(s, vals, tid);
    if (tid < 6 * s.nobj) out[tid] = sum;
    KP_SYNC();
}
// sw[b] = sign * sum over hull b's contacts with an object surface (slot ksel, or any if ksel < 0) of K_c acc[slot]
__device__ __forceinline__ void hull_coupling_wrench(EnvLdsObj& s, const Params& P, int ksel, const float* acc, float sign, int tid) {
    if (tid < D_NB) {
        const V3 o = ld3(s.xpos);
        S6 W = S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
        for (int c = s.con_start[tid]; c < s.con_start[tid + 1]; c++) {
            const int B = s.con_b2[c];
            if (B >= D_NB && (ksel < 0 || B == D_NB + ksel)) W = W + con_Kp(s, c, lds6(acc + 6 * (B - D_NB)), o);
        }
        sts6(s.sw + 6 * tid, sign * W);
    }
    KP_SYNC();
}
// object part of the gradient: g_k = mres_k - sum_{vertex side = k} [p x F; F] + sum_{surface side = k} [p x F; F]
__device__ __forceinline__ void obj_gradient(EnvLdsObj& s, int tid) {
    const V3 o = ld3(s.xpos);
    const bool have = tid < s.ncon;
    const int c = have ? tid : 0;
    const int A = have ? s.con_body[c] : -1, B = have ? (int)s.con_b2[c] : -1;
    const V3 F = ld3(s.jv3 + 3 * c), p = ld3(s.con_pos + 3 * c) - o;
    const V3 t = cross(p, F);
    float vals[12];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float f = A == D_NB + k ? -1.f : (B == D_NB + k ? 1.f : 0.f);
        vals[6 * k] = f * t.x; vals[6 * k + 1] = f * t.y; vals[6 * k + 2] = f * t.z; vals[6 * k + 3] = f * F.x; vals[6 * k + 4] = f * F.y; vals[6 * k + 5] = f * F.z;
    }
    const float sum = lanes_sum<12>(s, vals, tid);
    if (tid < 6 * s.nobj) s.ogr[tid] = s.omres[tid] + sum;
    KP_SYNC();
}
// spatial -> joint-space acceleration of the objects, then the same semi-implicit Euler step as the humanoid root
__device__ __forceinline__ void obj_integrate(EnvLdsObj& s, const Params& P, int tid) {
    if (tid < s.nobj) {
        const int k = tid;
        const float* R = s.oR + 9 * k;
        const S6 a = lds6(s.oa + 6 * k);
        const V3 ra = ld3(s.oq + 7 * k) - ld3(s.xpos);
        const V3 ql = a.l + cross(a.a, ra);
        const V3 qa = v3(R[0] * a.a.x + R[3] * a.a.y + R[6] * a.a.z, R[1] * a.a.x + R[4] * a.a.y + R[7] * a.a.z, R[2] * a.a.x + R[5] * a.a.y + R[8] * a.a.z);
        sts6(s.oqa + 6 * k, S6{ql, qa});
        float* v = s.ov + 6 * k;
        float* q = s.oq + 7 * k;
        v[0] += P.h * ql.x; v[1] += P.h * ql.y; v[2] += P.h * ql.z; v[3] += P.h * qa.x; v[4] += P.h * qa.y; v[5] += P.h * qa.z;
        q[0] += P.h * v[0]; q[1] += P.h * v[1]; q[2] += P.h * v[2];
        const V3 w = ld3(v + 3);
        const float n = sqrtf(dot(w, w));
        Q4 qr = Q4{1.f, 0.f, 0.f, 0.f};
        if (n >= 1e-15f) { float sn, cs; sincosf(0.5f * P.h * n, &sn, &cs); const float kk = sn / n; qr = Q4{cs, w.x * kk, w.y * kk, w.z * kk}; }
        const Q4 qn = qmul(qnormalize(Q4{q[3], q[4], q[5], q[6]}), qr);
        q[3] = qn.w; q[4] = qn.x; q[5] = qn.y; q[6] = qn.z;
    }
}

// Schur-complement columns of the object block, all at once.  Column j of  S = H_oo - H_oh H_hh^-1 H_ho  needs z_j = H_hh^-1 (H_ho e_j):
// a bias-force-only pass through the articulated-body factorisation whose right-hand side is a set of body wrenches on the hulls that
// touch object k(j) (-K_c e_j), and of whose result only the spatial accelerations of the touching hulls are read (H_oh z_j = sum K_c a).
// So only the union of the touching hulls' paths to the root takes part, and the columns are independent: lane = (column, row of the
// 6-vector), 8 columns x 8 rows per round, the bodies of the path visited one after the other (leaves -> root in descending body order,
// root -> leaves ascending; bodies are in depth-first order, so a per-depth accumulator is all the hand-up needs).  Replaces 6 n_obj
// passes of aba_resolve + hull_coupling_wrench + obj_coupling_u (12 passes per factorisation in the push scene) by one or two rounds.
// Scratch: the 552 contiguous floats jv3 | lim_jv | sa | sw (dead between the gradient and the row evaluation): per-depth accumulators
// [9][nc][6] + the joint-space right-hand sides u of the path's dofs [npd][nc]; nc = columns per round is what fits.
constexpr int D_SCHUR_SCRATCH = D_MAXCON * 3 + 72 + 144 + 144;
__device__ __forceinline__ void schur_columns(EnvLdsObj& s, const Params& P, unsigned cmask, int tid) {
    static_assert(offsetof(EnvLds, lim_jv) == offsetof(EnvLds, jv3) + sizeof(float) * D_MAXCON * 3 && offsetof(EnvLds, sa) == offsetof(EnvLds, lim_jv) + sizeof(float) * 72 &&
                  offsetof(EnvLds, sw) == offsetof(EnvLds, sa) + sizeof(float) * 144, "jv3 | lim_jv | sa | sw must be contiguous");
    constexpr int ST = 6 * D_MAXOBJ + 1;
    const int jl = tid >> 3, r = tid & 7;
    const bool rowok = r < 6;
    const int rc = rowok ? r : 5;
    const float rmask = rowok ? 1.f : 0.f;
    const V3 o = ld3(s.xpos);
    // hulls that press on an object with an active row, and the union of their paths to the root (subtree of b = bodies [b, b + bsub[b]))
    bool mine = false;
    if (tid < D_NB)
        for (int c = s.con_start[tid]; c < s.con_start[tid + 1]; c++) { const int B = s.con_b2[c]; if (B >= D_NB && ((cmask >> (B - D_NB)) & 1u)) mine = true; }
    const unsigned touch = (unsigned)__ballot(mine);
    const unsigned subtree = tid < D_NB ? ((s.bsub[tid] >= 32 ? 0xFFFFFFFFu : ((1u << s.bsub[tid]) - 1u)) << tid) : 0u;
    const unsigned path = (unsigned)__ballot((touch & subtree) != 0u);
    if (path == 0u) return;
    const int npd = 3 * __popc(path) + 3;                       // dofs on the path (the root has six)
    const int ncols = 6 * __popc(cmask);
    // columns per round: the accumulators [9][nc][6] and the first s0 rows of the right-hand sides [npd][nc] share the 552 floats of jv3 | lim_jv | sa | sw,
    // the remaining rows go to sv[0, 144) (the hulls' spatial accelerations of y0: read by obj_coupling_u before this call, rewritten by the
    // back-substitution pass after it).  Round 4: with the 552 floats alone a humanoid lying on the table (14 - 20 bodies on the path) got 4 - 5
    // columns per round, i.e. three rounds for the push scene's twelve columns; now six, i.e. two.
    int ncmax = min(8, ncols);
    while (ncmax > 1 && (54 * ncmax > D_SCHUR_SCRATCH || (npd - (D_SCHUR_SCRATCH - 54 * ncmax) / ncmax) * ncmax > 144)) ncmax--;
    if (ncols > ncmax) ncmax = min(ncmax, (ncols + ((ncols + ncmax - 1) / ncmax) - 1) / ((ncols + ncmax - 1) / ncmax));      // same number of rounds, evenly filled
    float* ACC = s.jv3;                                          // [9 levels][ncmax][6]
    float* UUa = ACC + 54 * ncmax;                               // rows [0, s0) of [npd][ncmax]
    float* UUb = s.sv;                                           // rows [s0, npd)
    const int s0 = (D_SCHUR_SCRATCH - 54 * ncmax) / ncmax;
#define KP_UU(slot) ((slot) < s0 ? UUa + (slot) * ncmax : UUb + ((slot) - s0) * ncmax)
    const int nobj = s.nobj;
    struct Fac3 { float c[3], U[3], Di[3]; };                     // motion axis, U = IA s and 1 / D of a body's three dofs: this lane's row
    auto ldfac = [&](int d0) {
        Fac3 f;
#pragma unroll
        for (int j = 0; j < 3; j++) { f.c[j] = s.cdof[6 * (d0 + j) + rc]; f.U[j] = s.U[6 * (d0 + j) + rc]; f.Di[j] = s.Dinv[d0 + j]; }
        return f;
    };
    for (int c0 = 0; c0 < ncols; c0 += ncmax) {
        const int nc = min(ncmax, ncols - c0);
        const bool colok = jl < nc;
        const int jc = colok ? jl : 0;
        const int gcol = (cmask == 2u ? 6 : 0) + c0 + jc;        // column of the object system
        const int kcol = gcol / 6, icol = gcol - 6 * kcol;
        // ---- leaves -> root: bias forces.  The per-depth accumulators belong to lane (column, row) alone and live in its registers (accd[depth], indexed by
        // the wave-uniform depth of the body being visited): the walk is a serial chain over the path's bodies, and a read-modify-write of an LDS
        // accumulator per body put two LDS round trips on that chain (round 4: the walk was latency-bound; 176 k cycles per substep on the env that ends the
        // objects launch, whose path is the whole tree)
        float accd[D_NLEV];
#pragma unroll
        for (int k = 0; k < D_NLEV; k++) accd[k] = 0.f;
        // The walk is a serial chain over the path's bodies and every body needs nine factor words (cdof, U, 1 / D of its three dofs) + its depth from LDS:
        // loaded at the top of the body's own turn they put one LDS round trip per body on the chain (16 - 20 bodies x two directions x one or two rounds
        // x every factorisation on the envs the objects launch ends on).  They do not depend on the chain: the NEXT body's words are requested
        // before the current body's arithmetic and have arrived when its turn comes (same operations on the same values: results unchanged).
        unsigned todo = path;
        int b = 31 - __clz((int)todo);
        Fac3 cur = ldfac(b == 0 ? 3 : 6 + 3 * (b - 1));
        int dv = (int)s.bdep[b];
        while (true) {
            todo &= ~(1u << b);
            const int nb = todo ? 31 - __clz((int)todo) : 0;
            const Fac3 nxt = ldfac(nb == 0 ? 3 : 6 + 3 * (nb - 1));
            const int ndv = (int)s.bdep[nb];
            const int d = __builtin_amdgcn_readfirstlane(dv);
            float pA = accd[d];
            if ((touch >> b) & 1u) {                             // right-hand side: + (K_c e_icol)[r] for this hull's contacts on object kcol
                V3 Pi, Pr;                                       // rows of P = [[p]x ; 1]: K_c = P M P^T, entry (r, i) = P_r . (M P_i)
                for (int c = s.con_start[b]; c < s.con_start[b + 1]; c++) {
                    if ((int)s.con_b2[c] - D_NB != kcol) continue;
                    const V3 p = ld3(s.con_pos + 3 * c) - o;
                    if (icol == 0) Pi = v3(0.f, -p.z, p.y); else if (icol == 1) Pi = v3(p.z, 0.f, -p.x); else if (icol == 2) Pi = v3(-p.y, p.x, 0.f);
                    else Pi = v3(icol == 3 ? 1.f : 0.f, icol == 4 ? 1.f : 0.f, icol == 5 ? 1.f : 0.f);
                    if (r == 0) Pr = v3(0.f, -p.z, p.y); else if (r == 1) Pr = v3(p.z, 0.f, -p.x); else if (r == 2) Pr = v3(-p.y, p.x, 0.f);
                    else Pr = v3(r == 3 ? 1.f : 0.f, r == 4 ? 1.f : 0.f, r == 5 ? 1.f : 0.f);
                    const float* m = s.cM + 6 * c;
                    const V3 w = v3(m[0] * Pi.x + m[3] * Pi.y + m[4] * Pi.z, m[3] * Pi.x + m[1] * Pi.y + m[5] * Pi.z, m[4] * Pi.x + m[5] * Pi.y + m[2] * Pi.z);
                    pA += rmask * dot(Pr, w);
                }
            }
            const int slot0 = b == 0 ? 0 : 3 + 3 * __popc(path & ((1u << b) - 1u));
            for (int g = 0; g < (b == 0 ? 2 : 1); g++) {
                const int sl = b == 0 ? (g == 0 ? 3 : 0) : slot0;
                const Fac3 f = g == 0 ? cur : ldfac(0);          // the root's second group (its translations) is loaded in its turn
#pragma unroll
                for (int j = 2; j >= 0; j--) {
                    const float u = -sum8(rmask * f.c[j] * pA);
                    pA += rmask * f.U[j] * (u * f.Di[j]);
                    if (colok && r == 0) KP_UU(sl + j)[jc] = u;
                }
            }
            accd[d] = 0.f;
            if (b > 0) accd[d - 1] += (colok && rowok) ? pA : 0.f;
            if (!todo) break;
            b = nb; cur = nxt; dv = ndv;
        }
        KP_SYNC();
        // ---- root -> leaves: spatial accelerations (accd[depth] now holds the last visited body's at that depth: a body's parent is the last one
        // visited one level up, bodies being in depth-first order); at a touching hull, H_oh z accumulates per object
        float cpl0 = 0.f, cpl1 = 0.f;
        todo = path;
        b = __ffs((int)todo) - 1;
        auto ldrhs = [&](int bb, int g, float* uu) {                // the joint-space right-hand sides of a body's group, this lane's column
            const int sl = bb == 0 ? (g == 0 ? 0 : 3) : 3 + 3 * __popc(path & ((1u << bb) - 1u));
#pragma unroll
            for (int j = 0; j < 3; j++) uu[j] = KP_UU(sl + j)[jc];
        };
        cur = ldfac(b == 0 ? 0 : 6 + 3 * (b - 1));
        float cuu[3];
        ldrhs(b, 0, cuu);
        dv = (int)s.bdep[b];
        while (true) {
            todo &= todo - 1u;
            const int nb = todo ? __ffs((int)todo) - 1 : b;
            const Fac3 nxt = ldfac(nb == 0 ? 0 : 6 + 3 * (nb - 1));
            float nuu[3];
            ldrhs(nb, 0, nuu);
            const int ndv = (int)s.bdep[nb];
            const int d = __builtin_amdgcn_readfirstlane(dv);
            float a = (b > 0 && colok && rowok) ? accd[d - 1] : 0.f;
            for (int g = 0; g < (b == 0 ? 2 : 1); g++) {
                Fac3 f = cur;
                float uu[3] = {cuu[0], cuu[1], cuu[2]};
                if (g == 1) { f = ldfac(3); ldrhs(0, 1, uu); }
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float qdd = (uu[j] - sum8(rmask * f.U[j] * a)) * f.Di[j];
                    a += qdd * f.c[j];
                }
            }
            accd[d] = a;
            if ((touch >> b) & 1u) {
                KP_SYNC();
                if (colok && rowok) ACC[jc * 6 + r] = a;                    // the column's whole 6-vector is needed by every lane of the column: through LDS, for the touching hulls only
                KP_SYNC();
                const S6 ab = lds6(ACC + jc * 6);
                for (int c = s.con_start[b]; c < s.con_start[b + 1]; c++) {
                    const int B = s.con_b2[c];
                    if (B < D_NB) continue;
                    const S6 w = con_Kp(s, c, ab, o);
                    const float wr = r == 0 ? w.a.x : r == 1 ? w.a.y : r == 2 ? w.a.z : r == 3 ? w.l.x : r == 4 ? w.l.y : w.l.z;
                    if (B == D_NB) cpl0 += wr; else cpl1 += wr;
                }
            }
            if (!todo) break;
            b = nb; cur = nxt; dv = ndv;
            cuu[0] = nuu[0]; cuu[1] = nuu[1]; cuu[2] = nuu[2];
        }
        if (colok && rowok) {
            s.Sm[r * ST + gcol] += cpl0;
            if (nobj > 1) s.Sm[(6 + r) * ST + gcol] += cpl1;
        }
        KP_SYNC();
    }
#undef KP_UU
}

// the constraint solve with free objects in the scene: same Newton iteration as solve_constraints on the joint unknowns
// (q_humanoid, a_object...).  The Newton system is solved exactly by block elimination: the articulated-body pass factorises
// the humanoid block, 6 n_obj + 1 bias-only passes form the Schur complement on the objects when a hull touches one.
template <int NT>
__device__ __forceinline__ int solve_constraints_obj(EnvLdsObj& s, const Params& P, const Lane8& L8, int depth, int tid, int& nfact, int& ncap, const float* arm) {
    constexpr int ST = 6 * D_MAXOBJ + 1;
    const int nobj = s.nobj, no6 = 6 * nobj;
    // smooth acceleration of the objects: I_eff a = -bias wrench
    if (no6 > 0) {
        {
            const int n = no6;
            if (tid < n) {
                const int k = tid / 6, r = tid - 6 * k;
                float* row = s.Sm + ST * tid;
                for (int c = 0; c < n; c++) row[c] = (c / 6 == k) ? inert_entry(s.oIe + 10 * k, r, c - 6 * k) : 0.f;
                row[n] = -s.ofb[tid];
            }
            KP_SYNC();
        }
        dense_solve(s, no6, tid, true);
        if (tid < no6) s.oas[tid] = s.Sm[ST * tid + no6];
        KP_SYNC();
    }
    // The humanoid's share of the problem in the direct form of solve_constraints_direct: no qacc_smooth, no smooth articulated-body solve, the
    // start is the warm start, the first factorisation walks every level.  The objects keep their (cheap) smooth accelerations oas: their
    // share of the Gauss term stays 0.5 (oa - oas)^T I_eff (oa - oas), carried as omres = I_eff (oa - oas).
    if (s.ncon == 0 && s.nlim == 0) {
        aba_solve<NT, true>(s, P, L8, s.applied, s.qacc, false, tid, D_NLEV, s.fb);
        if (tid < no6) s.oa[tid] = s.oas[tid];
        KP_SYNC();
        return 0;
    }
    float* sacc = s.Mv;        // [24 + 2][6] over Mv + mres (+ x[0..3]): spatial accelerations induced by the iterate (hulls: of qacc; object slots: oa, for the first row evaluation)
    float* grad = s.qacc_s;    // the words qacc_smooth would occupy
    static_assert(offsetof(EnvLds, x) == offsetof(EnvLds, Mv) + 152 * sizeof(float), "sacc's object slots continue into x");
    spatial_accumulate<NT>(s, s.qacc, depth, tid, sacc);
    if (tid < no6) sacc[6 * D_NB + tid] = s.oa[tid];
    if (tid < nobj) sts6(s.omres + 6 * tid, inert_mul(s.oIe + 10 * tid, lds6(s.oa + 6 * tid) + (-1.0f) * lds6(s.oas + 6 * tid)));
    KP_SYNC();
    eval_rows<NT, true>(s, s.qacc, s.jar3, s.lim_jar, true, tid, sacc);
    float rowcost = 0.f;       // the rows' share of the cost at the iterate (the first line search evaluates it at alpha = 0)
    int it = 0, lev_hist = 1;
    bool done = false;          // left the loop through one of mj_solNewton's termination tests (not the iteration cap)
    const unsigned conlev = contact_levels(s, L8);
    // active set of the iterate (see solve_constraints_direct)
    float changed = 0.f, deep = 0.f;
    auto active_set = [&]() {
        changed = 0.f; deep = 0.f;
        for (int i = tid; i < D_NV; i += NT) {
            const float ex = (i >= 6 && s.lim_jar[i - 6] < 0.f) ? fabsf(s.lim_D[i - 6]) : 0.f;
            if (ex != s.extra[i]) changed = 1.f;
            s.extra[i] = ex;
            if (ex != 0.f) deep = fmaxf(deep, (float)s.bdep[s.dbody[i]]);     // active joint limit: its body's level is dirty
        }
        changed += active_set_changed<NT>(s, P, tid, deep);
        changed = (NT == 64) ? (__ballot(changed > 0.f) != 0ull ? 1.f : 0.f) : block_sum<NT>(s, changed, tid);     // one wave: a ballot is the whole reduction
        KP_SYNC();
    };
    active_set();
    for (; it < P.max_iter; it++) {
        // gradient: humanoid dofs (mres - J^T f) and object wrenches
        con_prepare<NT>(s, P, tid);                  // lane = contact: M_c at this iterate (object rows of the Hessian AND the hulls' contact inertia in aba_solve) and the contact force
        wrench_project<NT, true>(s, P, sacc, s.qacc, nullptr, grad, true, true, tid, arm, s.jv3, s.fb, s.applied);
        if (nobj > 0) obj_gradient(s, tid);
        float g2 = 0.f;
        for (int i = tid; i < D_NV; i += NT) { const float g = grad[i]; g2 += g * g; s.x[i] = -g; }
        if (tid < nobj) {   // gradient in joint coordinates: [g_l ; R^T (g_a + r x g_l)], r = o - body origin
            const S6 g = lds6(s.ogr + 6 * tid);
            const V3 t = g.a + cross(ld3(s.xpos) - ld3(s.oq + 7 * tid), g.l);
            g2 += dot(g.l, g.l) + dot(t, t);
        }
        g2 = block_sum<NT>(s, g2, tid);
        KP_SYNC();
        if (P.scale * sqrtf(g2) < P.tol) { done = true; break; }
        // search direction
        const bool refactor = it == 0 || changed > 0.f;
        nfact += refactor;
        int cslot = -1;                                   // object slot this lane's hull contact presses on with an active row
        for (int c = tid; c < s.con_start[D_NB]; c += NT) {
            if (s.con_b2[c] < D_NB) continue;
            const float jn = s.jar3[3 * c], jt1 = s.jar3[3 * c + 1], jt2 = s.jar3[3 * c + 2];
            bool act = false;
#pragma unroll
            for (int e = 0; e < 4; e++) act |= row_val(e, P.mu, jn, jt1, jt2) < 0.f;
            if (act) cslot = s.con_b2[c] - D_NB;
        }
        const unsigned cmask = (__ballot(cslot == 0) != 0ull ? 1u : 0u) | (__ballot(cslot == 1) != 0ull ? 2u : 0u);
        const bool couple = cmask != 0u;
        // H = [[H_hh, H_ho], [H_oh, H_oo]] by block elimination.  refactor: one articulated-body factorisation of H_hh (+ the object
        // rows), then -- when a hull presses on an object -- the Schur-complement columns (schur_columns); the dense object system; and
        // one more pass through the factorisation for the back-substitution
        if (refactor) {
            if (no6 > 0) obj_hessian(s, P, s.ogr, -1.0f, tid);
            lev_hist = max(lev_hist, first_clean_level<NT>(s, deep, tid));   // the clean range only shrinks within a substep
            // the substep's first factorisation walks every level: its clean levels hold M's own factors from then on
            aba_solve<NT, true>(s, P, L8, s.x, s.search, true, tid, it == 0 ? D_NLEV : lev_hist, nullptr, conlev);     // y0 = H_hh^-1 (-g_h); sv = its spatial accelerations
            if (couple) { obj_coupling_u(s, P, s.ot, tid); if (tid < no6) s.Sm[ST * tid + no6] += s.ot[tid]; KP_SYNC(); }     // rhs_o -= H_oh y0
        }
        if (refactor && couple) schur_columns(s, P, cmask, tid);          // S = H_oo - H_oh H_hh^-1 H_ho, all columns in one or two rounds
        if (!refactor) {                                                  // factors reused: y0 = H_hh^-1 (-g_h) through them, then the object right-hand side
            aba_resolve(s, L8, s.x, nullptr, s.search);
            if (no6 > 0) {
                if (tid < no6) s.Sm[ST * tid + no6] = -s.ogr[tid];
                KP_SYNC();
                if (couple) { obj_coupling_u(s, P, s.ot, tid); if (tid < no6) s.Sm[ST * tid + no6] += s.ot[tid]; KP_SYNC(); }
            }
        }
        if (no6 > 0) {
            dense_solve(s, no6, tid, refactor);
            if (tid < no6) s.osrch[tid] = s.Sm[ST * tid + no6];
            KP_SYNC();
            if (couple) {                                                 // back-substitution: search = H_hh^-1 (-g_h - H_ho da)
                hull_coupling_wrench(s, P, -1, s.osrch, 1.0f, tid);
                aba_resolve(s, L8, s.x, s.sw, s.search);
            }
        }
        if (tid < no6) s.sv[6 * D_NB + tid] = s.osrch[tid];
        KP_SYNC();
        eval_rows<NT, true>(s, s.search, s.jv3, s.lim_jv, false, tid);
        if (tid < nobj) sts6(s.oMv + 6 * tid, inert_mul(s.oIe + 10 * tid, lds6(s.osrch + 6 * tid)));
        KP_SYNC();
        float g0 = 2.0f * quad_form_M<NT>(s, arm, s.sv, sacc, s.search, nullptr, s.qacc, nullptr, tid);      // search^T (M qacc - qfrc_smooth) for the hulls ...
        float h0 = 2.0f * quad_form_M<NT>(s, arm, s.sv, s.sv, s.search, nullptr, s.search, nullptr, tid);
        for (int i = tid; i < D_NB * 6; i += NT) g0 += s.sv[i] * s.fb[i];
        for (int i = tid; i < D_NV; i += NT) g0 -= s.search[i] * s.applied[i];
        if (tid < no6) { g0 += s.osrch[tid] * s.omres[tid]; h0 += s.osrch[tid] * s.oMv[tid]; }                // ... and search^T I_eff (oa - oas) for the objects
        g0 = block_sum<NT>(s, g0, tid); h0 = block_sum<NT>(s, h0, tid);
        float rownew, rc0 = 0.f;
        const float alpha = line_search<NT>(s, P, g0, h0, tid, rownew, it == 0, rc0);
        if (it == 0) rowcost = rc0;
        if (!(alpha > 0.f)) { done = true; break; }
        for (int i = tid; i < D_NV; i += NT) s.qacc[i] += alpha * s.search[i];
        for (int i = tid; i < D_NB * 6; i += NT) sacc[i] += alpha * s.sv[i];
        if (tid < no6) { s.oa[tid] += alpha * s.osrch[tid]; s.omres[tid] += alpha * s.oMv[tid]; }
        for (int k = tid; k < 3 * s.ncon; k += NT) s.jar3[k] += alpha * s.jv3[k];
        for (int j = tid; j < D_NU; j += NT) if (s.lim_D[j] != 0.f) s.lim_jar[j] += alpha * s.lim_jv[j];
        KP_SYNC();
        // cost(old) - cost(new) in closed form: the Gauss term of hulls and objects is quadratic along the search direction (g0, h0 hold both
        // shares), the rows' share comes out of the line search's registers
        const float improvement = P.scale * ((rowcost - rownew) - alpha * (g0 + 0.5f * alpha * h0));
        rowcost = rownew;
        if (improvement < P.tol) { it++; done = true; break; }
        active_set();
        if (changed == 0.f && P.scale * fabsf(1.0f - alpha) * sqrtf(g2) < P.tol) { it++; done = true; break; }     // gradient(new) = (1 - alpha) gradient(old): see solve_constraints_direct
    }
    if (!done) ncap++;          // the solver stopped at opt.iterations: counted per env in diag (flags >> 8)
    return it;
}

}  // namespace kp
