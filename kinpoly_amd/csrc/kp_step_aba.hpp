// kp_step_aba.hpp -- the articulated-body passes of the control step, 8 lanes per body (DPP helpers, Lane8, aba_elim3 ... aba_resolve).  Part of kp_step_device.hpp.
#pragma once
#include "kp_step_args.hpp"

namespace kp {

// ---------------------------------------------------------------- articulated-body solve, 8 lanes per body
// Lane layout inside a tree level: tid = 8 * slot + r; slot = index of the body within the level (<= 5 bodies),
// r = row of the 6x6 articulated inertia (rows 6, 7 are zero padding).  A lane keeps its row in "XOR order":
// register k holds column r ^ KX[k], KX = {0,1,2,3,7,6,5,4}.  With that order the three DPP exchanges
// quad_perm[1,0,3,2] (xor 1), quad_perm[2,3,0,1] (xor 2) and row_half_mirror (xor 7) implement both the
// 8-lane sum and the 8-lane all-gather (7 moves) with results already aligned to the row registers, so the
// rank-1 updates  IA -= U U^T / D  need no LDS round trip.
__device__ __forceinline__ float dpp_x1(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)); }
__device__ __forceinline__ float dpp_x2(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)); }
__device__ __forceinline__ float dpp_x7(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)); }
__device__ __forceinline__ float sum8(float v) { v += dpp_x1(v); v += dpp_x2(v); v += dpp_x7(v); return v; }
__device__ __forceinline__ void gather8(float v, float* g) {
    g[0] = v; g[1] = dpp_x1(v); g[2] = dpp_x2(g[0]); g[3] = dpp_x2(g[1]);
    g[4] = dpp_x7(g[0]); g[5] = dpp_x7(g[1]); g[6] = dpp_x7(g[2]); g[7] = dpp_x7(g[3]);
}
__device__ __forceinline__ float rcp_nr(float d) { float r = __builtin_amdgcn_rcpf(d); return r * (2.0f - d * r); }

struct Lane8 {
    int slot, r;
    int col[8];      // column held by register k
    int ciidx[8];    // index into the 10-float body inertia giving IA[r][col[k]] (times cisgn)
    float cisgn[8];
    int idx21[8];    // index into the 21-float symmetric storage
    unsigned long long sb, sp, sc0, sc1, sc2;  // 5 bits per level: body, parent, children (31 = none) of this lane's slot
    unsigned multi;  // bit lev set: some body of that level has more than one child (wave-uniform; only levels 0 and 3 of the SMPL tree)
    // The per-lane schedule comes ready-made from the host (kp_sim.hip: build_lane8_table, 28 dwords per lane): seven 16-byte loads
    // and a few bit-field extracts, cheap enough to redo at the top of every solve instead of keeping 45 registers alive between them.
    //   words 0..9   sb, sp, sc0, sc1, sc2 (64 bit each: 5 bits per tree level = body / parent / children of this lane's slot;
    //                31 = no body at that level, absent child -> the zero record 24)
    //   word  10     multi (bit lev: some body of that level has more than one child; only levels 0 and 3 of the SMPL tree)
    //   words 12..19 per register k: col | ciidx << 4 | idx21 << 8     (column r ^ KX[k], index into the 10-float body inertia, index into the 21-float symmetric storage)
    //   words 20..27 per register k: cisgn as float
    __device__ __forceinline__ void init(int tid, const uint32_t* __restrict__ tab) {
        slot = tid >> 3; r = tid & 7;
        const uint4* q = reinterpret_cast<const uint4*>(tab + 28 * (tid & 63));
        const uint4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4], w5 = q[5], w6 = q[6];
        sb = (unsigned long long)w0.x | ((unsigned long long)w0.y << 32); sp = (unsigned long long)w0.z | ((unsigned long long)w0.w << 32);
        sc0 = (unsigned long long)w1.x | ((unsigned long long)w1.y << 32); sc1 = (unsigned long long)w1.z | ((unsigned long long)w1.w << 32);
        sc2 = (unsigned long long)w2.x | ((unsigned long long)w2.y << 32); multi = w2.z;
        if (tid >= 64) {            // threads_per_env = 128 / 256: only the first wavefront serves the tree passes (31 = no body, 24 = zero record)
            sb = sp = 0x1FFFFFFFFFFFull;
            sc0 = sc1 = sc2 = 0x18C6318C6318ull;      // 24 in every 5-bit field of the 9 levels
        }
        const unsigned pk[8] = {w3.x, w3.y, w3.z, w3.w, w4.x, w4.y, w4.z, w4.w};
        const unsigned sg[8] = {w5.x, w5.y, w5.z, w5.w, w6.x, w6.y, w6.z, w6.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            col[k] = (int)(pk[k] & 7u); ciidx[k] = (int)((pk[k] >> 4) & 15u); idx21[k] = (int)((pk[k] >> 8) & 31u);
            cisgn[k] = __builtin_bit_cast(float, sg[k]);
        }
    }
};

// out = (M + diag(s.extra) [+ J^T D_active J])^-1 rhs.  Leaves s.sv[b] = sum over ancestor dofs cdof_d out_d
// (the spatial "acceleration" of every body induced by out).  rhs/out are LDS vectors (may alias).
// eliminate the three dofs d0+2, d0+1, d0 of one body from its articulated inertia (row r in XOR order)
template <class SL>
__device__ __forceinline__ void aba_elim3(SL& s, const Lane8& L, const float* rhs, int d0, bool store_ok, float* IAx, float& pA) {
    const int r = L.r;
    const bool rowok = r < 6;
    float sxa[3][8], dsc[3], rh[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int d = d0 + j;
        gather8(rowok ? s.cdof[6 * d + r] : 0.f, sxa[j]);    // lane r fetches its own component, the 8-lane all-gather lands in XOR order
        if constexpr (SL::LEAN) dsc[j] = s.extra[d]; else dsc[j] = s.arm[d] + s.extra[d];      // lean layout: extra holds armature + extra (see step_body)
        rh[j] = rhs[d];
    }
    float Uo[3], Do[3], uo[3];
    // Round 5 (VERDICT r4 #5a): the two 8-term blocks of a joint elimination -- the row product U_r = sum_k IA[r][k] s[k] and the rank-1 update
    // IA[r][k] -= (U_r / D) U[k] -- as hand-placed packed fp32 operations (v_pk_mul_f32 / v_pk_fma_f32 on register pairs), everything else unchanged.
    // The blanket SLP vectoriser lost to register pairing on this kernel (build.py OPT_FLAGS); here the operands of a pair are adjacent by construction:
    // 576 scalar fp32 instructions become 324 packed ones, no extra v_mov, 208 -> 212 VGPRs (floor kernel), launch 2.665 -> 2.611 ms on the metric's
    // workload in three A/B pairs (profiles/r05/pk_elim_ab.log), objects 4.79 -> 4.78 ms.  The scalar form it replaced is gone (the pairwise row
    // product sums in another order: the two builds were not bit-identical; every parity test and sweep was re-run on this one).
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 IA2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) IA2[k] = f2{IAx[2 * k], IAx[2 * k + 1]};
#pragma unroll
    for (int j = 2; j >= 0; j--) {
        f2 acc = IA2[0] * f2{sxa[j][0], sxa[j][1]};
#pragma unroll
        for (int k = 1; k < 4; k++) acc = __builtin_elementwise_fma(IA2[k], f2{sxa[j][2 * k], sxa[j][2 * k + 1]}, acc);
        const float Ur = acc.x + acc.y;
        const float sr = sxa[j][0];
        const float dsum = sum8(sr * Ur), usum = sum8(sr * pA);
        const float D = dsc[j] + dsum, u = rh[j] - usum;
        const float Dinv = rcp_nr(D);
        float Ux[8];
        gather8(Ur, Ux);
        const float ur = -(Ur * Dinv);
        const f2 ur2 = f2{ur, ur};
#pragma unroll
        for (int k = 0; k < 4; k++) IA2[k] = __builtin_elementwise_fma(ur2, f2{Ux[2 * k], Ux[2 * k + 1]}, IA2[k]);
        pA += Ur * (u * Dinv);
        Uo[j] = Ur; Do[j] = Dinv; uo[j] = u;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { IAx[2 * k] = IA2[k].x; IAx[2 * k + 1] = IA2[k].y; }
    if (store_ok && rowok) {
#pragma unroll
        for (int j = 0; j < 3; j++) s.U[6 * (d0 + j) + r] = Uo[j];
    }
    if (store_ok && r == 0) {
#pragma unroll
        for (int j = 0; j < 3; j++) { s.Dinv[d0 + j] = Do[j]; s.uj[d0 + j] = uo[j]; }
    }
}

template <class SL>
__device__ __forceinline__ float aba_fwd3(SL& s, const Lane8& L, float* out, int d0, bool store_ok, float a) {
    const int r = L.r;
    const int rc = r < 6 ? r : 5;
    const float rmask = r < 6 ? 1.f : 0.f;
    float Ud[3], sd[3], ujd[3], Did[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int d = d0 + j;
        Ud[j] = rmask * s.U[6 * d + rc]; sd[j] = s.cdof[6 * d + rc];
        ujd[j] = s.uj[d]; Did[j] = s.Dinv[d];
    }
    float qo[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float qdd = (ujd[j] - sum8(Ud[j] * a)) * Did[j];
        qo[j] = qdd;
        a += qdd * sd[j];
    }
    if (store_ok && r == 0) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[d0 + j] = qo[j];
    }
    return a;
}

// root->leaves pass: joint accelerations from (U, 1/D, u) and the parent's spatial acceleration; leaves them in sv
template <class SL>
__device__ __forceinline__ void aba_forward(SL& s, const Lane8& L, float* out, int lev_max = D_NLEV - 1) {
    const int r = L.r;
    const bool rowok = r < 6;
#pragma nounroll
    for (int lev = 0; lev <= lev_max; lev++) {
        const int sh = 5 * lev;
        const int bq = (int)((L.sb >> sh) & 31ull), par = (int)((L.sp >> sh) & 31ull);
        const bool active = bq != 31;
        const int b = active ? bq : 0;
        float a = (rowok && par != 31) ? s.sv[6 * (par == 31 ? 0 : par) + r] : 0.f;
        if (lev == 0) {
            a = aba_fwd3(s, L, out, 0, active, a);
            a = aba_fwd3(s, L, out, 3, active, a);
        } else {
            a = aba_fwd3(s, L, out, b == 0 ? 6 : 6 + 3 * (b - 1), active, a);
        }
        if (active && rowok) s.sv[6 * b + r] = a;
        KP_SYNC();
    }
}

// bit lev set: the body this lane serves at tree level lev has contacts (con_start is fixed for the substep, so the Newton
// factorisations test a register instead of reading two LDS words per level)
template <class SL>
__device__ __forceinline__ unsigned contact_levels(const SL& s, const Lane8& L) {
    unsigned m = 0;
#pragma unroll
    for (int lev = 0; lev < D_NLEV; lev++) {
        const int bq = (int)((L.sb >> (5 * lev)) & 31ull), b = bq != 31 ? bq : 0;
        if (bq != 31 && s.con_start[b + 1] > s.con_start[b]) m |= 1u << lev;
    }
    return m;
}

template <int NT, bool OBJ, class SL>
// lev_clean: tree levels >= lev_clean carry no active contact row and no active joint limit, so their articulated inertias, U and
// 1/D are the ones the substep's first Newton factorisation (which walks every level; same M, no extra armature there) left in LDS:
// only the bias-force half runs there.
__device__ __forceinline__ void aba_solve(SL& s, const Params& P, const Lane8& L, const float* rhs, float* out, bool contact_inertia, int tid, int lev_clean = D_NLEV, const float* bwrench = nullptr,
                                          unsigned conlev = 0xFFFFFFFFu) {
    const int r = L.r;
    const bool rowok = r < 6;
    if constexpr (SL::LEAN) {              // pAa shares its words with J search there: the zero record absent children read is written anew for this solve
        if (tid < 6) s.pAa[6 * 24 + tid] = 0.f;
        KP_SYNC();
    }
#pragma nounroll
    for (int lev = D_NLEV - 1; lev >= 0; lev--) {
        const int sh = 5 * lev;
        const int bq = (int)((L.sb >> sh) & 31ull), c0 = (int)((L.sc0 >> sh) & 31ull), c1 = (int)((L.sc1 >> sh) & 31ull), c2 = (int)((L.sc2 >> sh) & 31ull);
        const bool active = bq != 31;
        const int b = active ? bq : 0;
        if (lev >= lev_clean) {                                    // lev_clean >= 1: the root level is never clean
            const float rmask = rowok ? 1.f : 0.f;
            const int rc = rowok ? r : 5, pr = 6 * 24;
            float pA = s.pAa[rowok ? 6 * c0 + r : pr];
            if ((L.multi >> lev) & 1u) pA += s.pAa[rowok ? 6 * c1 + r : pr] + s.pAa[rowok ? 6 * c2 + r : pr];
            const int d0 = 6 + 3 * (b == 0 ? 0 : b - 1);
            float uo[3];
#pragma unroll
            for (int j = 2; j >= 0; j--) {
                const int d = d0 + j;
                const float u = rhs[d] - sum8(rmask * s.cdof[6 * d + rc] * pA);
                pA += rmask * s.U[6 * d + rc] * (u * s.Dinv[d]);
                uo[j] = u;
            }
            if (active && r == 0) {
#pragma unroll
                for (int j = 0; j < 3; j++) s.uj[d0 + j] = uo[j];
            }
            if (active && rowok) s.pAa[6 * b + r] = pA;
            KP_SYNC();
            continue;
        }
        // ---- one LDS round: body inertia row + children rows (the per-dof operands are fetched by aba_elim3 in the same round)
        float IAx[8];
        float pA;
        {
            const float* ci = s.cinert + 10 * b;
            const float* r0 = s.IAa + 22 * c0;
            const int pr = rowok ? r : 6 * 24;                 // padding rows read the zero record
#pragma unroll
            for (int k = 0; k < 8; k++) IAx[k] = L.cisgn[k] * ci[L.ciidx[k]] + r0[L.idx21[k]];
            pA = s.pAa[rowok ? 6 * c0 + r : pr];
            if ((L.multi >> lev) & 1u) {                       // second / third child: only the levels where some body branches
                const float* r1 = s.IAa + 22 * c1; const float* r2 = s.IAa + 22 * c2;
#pragma unroll
                for (int k = 0; k < 8; k++) IAx[k] += r1[L.idx21[k]] + r2[L.idx21[k]];
                pA += s.pAa[rowok ? 6 * c1 + r : pr] + s.pAa[rowok ? 6 * c2 + r : pr];
            }
            if (bwrench) pA += (rowok ? 1.f : 0.f) * bwrench[6 * b + (rowok ? r : 5)];
        }
        if (contact_inertia && active && ((conlev >> lev) & 1u)) {     // conlev: this lane's body at this level carries contacts (contact_levels)
            // active pyramid rows come from con_act (active_set_changed ran on this iterate); the next contact's operands are
            // requested before this one's arithmetic, so the loop pays one LDS round trip, not one per contact
            const int c0 = s.con_start[b], c1 = s.con_start[b + 1];
            if (c1 > c0) {
                const V3 o = ld3(s.xpos);
                float Krow[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if constexpr (OBJ) {
                    // object kernels: M_c = D F G F^T of every contact's active rows is already in LDS for this iterate (con_prepare, lane = contact, which
                    // also feeds the object rows of the Hessian), so a row of K = P M_c P^T is one symmetric 3 x 3 product and a cross product -- no
                    // mju_makeFrame, no frame round trip per contact, body row and factorisation
                    const float* cM = as_obj(s).cM;
                    V3 pn = ld3(s.con_pos + 3 * c0);
                    float mn[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) mn[k] = cM[6 * c0 + k];
                    for (int c = c0; c < c1; c++) {
                        const V3 p = pn - o;
                        float m[6];
#pragma unroll
                        for (int k = 0; k < 6; k++) m[k] = mn[k];
                        const int cn = min(c + 1, c1 - 1);
                        pn = ld3(s.con_pos + 3 * cn);
#pragma unroll
                        for (int k = 0; k < 6; k++) mn[k] = cM[6 * cn + k];
                        V3 Pr;  // row r of P = [[p]x ; 1]:  row r of K = [p x q ; q] with q = M_c P_r
                        if (r == 0) Pr = v3(0.f, -p.z, p.y); else if (r == 1) Pr = v3(p.z, 0.f, -p.x); else if (r == 2) Pr = v3(-p.y, p.x, 0.f);
                        else Pr = v3(r == 3 ? 1.f : 0.f, r == 4 ? 1.f : 0.f, r == 5 ? 1.f : 0.f);
                        const V3 q = v3(m[0] * Pr.x + m[3] * Pr.y + m[4] * Pr.z, m[3] * Pr.x + m[1] * Pr.y + m[5] * Pr.z, m[4] * Pr.x + m[5] * Pr.y + m[2] * Pr.z);
                        const V3 pq = cross(p, q);
                        Krow[0] += pq.x; Krow[1] += pq.y; Krow[2] += pq.z; Krow[3] += q.x; Krow[4] += q.y; Krow[5] += q.z;
                    }
                } else {
                const float mu = P.mu, mu2 = P.mu * P.mu;
                V3 pn = ld3(s.con_pos + 3 * c0);
                float Dn = s.con_D[c0];
                unsigned an = s.con_act[c0];
                for (int c = c0; c < c1; c++) {
                    const V3 p = pn - o;
                    const float Dc = Dn;
                    const unsigned am = an;
                    const int cn = min(c + 1, c1 - 1);
                    pn = ld3(s.con_pos + 3 * cn); Dn = s.con_D[cn]; an = s.con_act[cn];
                    const float a0 = (am & 1u) ? 1.f : 0.f, a1 = (am & 2u) ? 1.f : 0.f, a2 = (am & 4u) ? 1.f : 0.f, a3 = (am & 8u) ? 1.f : 0.f;
                    // G = sum_e a_e dir_e dir_e^T with dir_e = n +- mu t1, n +- mu t2; in frame coordinates (n, t1, t2):
                    const float gnn = a0 + a1 + a2 + a3, g11 = mu2 * (a0 + a1), g22 = mu2 * (a2 + a3), gn1 = mu * (a0 - a1), gn2 = mu * (a2 - a3);
                    const Frame fr = contact_frame<OBJ>(s, c);
                    V3 Pr;  // row r of P = [[p]x ; 1]:  K = D P G P^T, row r = [p x q ; q] with q = D (P_r G)
                    if (r == 0) Pr = v3(0.f, -p.z, p.y); else if (r == 1) Pr = v3(p.z, 0.f, -p.x); else if (r == 2) Pr = v3(-p.y, p.x, 0.f);
                    else Pr = v3(r == 3 ? 1.f : 0.f, r == 4 ? 1.f : 0.f, r == 5 ? 1.f : 0.f);
                    const V3 pf = frame_comp(fr, Pr);
                    const V3 q = frame_world(fr, v3(Dc * (gnn * pf.x + gn1 * pf.y + gn2 * pf.z), Dc * (gn1 * pf.x + g11 * pf.y), Dc * (gn2 * pf.x + g22 * pf.z)));
                    const V3 pq = cross(p, q);
                    Krow[0] += pq.x; Krow[1] += pq.y; Krow[2] += pq.z; Krow[3] += q.x; Krow[4] += q.y; Krow[5] += q.z;
                }
                }
                // the column of register k from a laundered copy of r (col[k] = r ^ KX[k], see Lane8): the 40 lane masks of the selects below are invariant over
                // the level loop and the Newton loop, so the compiler formed them once per solve and kept them in 80 scalar registers -- all spilled, and read
                // back lane by lane here at every level that carries contacts.  Forty compares cost less than eighty spill reads.
                const int rl = kp_launder(r);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int c = rl ^ (k < 4 ? k : 11 - k);
                    float v = Krow[0];
                    v = c == 1 ? Krow[1] : v; v = c == 2 ? Krow[2] : v; v = c == 3 ? Krow[3] : v; v = c == 4 ? Krow[4] : v; v = c == 5 ? Krow[5] : v;
                    if (rowok && c < 6) IAx[k] += v;
                }
            }
        }
        if (lev == 0) {
            aba_elim3(s, L, rhs, 3, active, IAx, pA);
            aba_elim3(s, L, rhs, 0, active, IAx, pA);
        } else {
            aba_elim3(s, L, rhs, 6 + 3 * (b - 1) < 6 ? 6 : 6 + 3 * (b - 1), active, IAx, pA);
        }
        if (active && rowok) {
#pragma unroll
            for (int k = 0; k < 8; k++) {      // upper triangle only; the other lanes' copies go to a scrap word instead of eight exec-masked stores
                float* dst = (L.col[k] < 6 && r <= L.col[k]) ? s.IAa + 22 * b + L.idx21[k] : s.red + 7;
                *dst = IAx[k];
            }
            s.pAa[6 * b + r] = pA;
        }
        KP_SYNC();
    }
    aba_forward(s, L, out, D_NLEV - 1);
}

// out = H^-1 (rhs + J_body^T wrench) with the factorisation (U, 1/D) the last aba_solve left in LDS: the bias-force half of the
// leaves->root pass only (no inertia updates), then the usual root->leaves pass.  rhs / wrench ([24][6], about o) may be null.
// lev_max < D_NLEV - 1: the caller knows that rhs and wrench vanish on every body below tree level lev_max and only needs the
// accelerations (sv) / out entries down to that level: the deeper levels would carry exact zeros up and are skipped in both halves.
template <class SL>
__device__ __forceinline__ void aba_resolve(SL& s, const Lane8& L, const float* rhs, const float* wrench, float* out, int lev_max = D_NLEV - 1) {
    const int r = L.r;
    const bool rowok = r < 6;
    const int rc = rowok ? r : 5;
    const float rmask = rowok ? 1.f : 0.f;
    if constexpr (SL::LEAN) {              // see aba_solve
        if (threadIdx.x < 6) s.pAa[6 * 24 + threadIdx.x] = 0.f;
        KP_SYNC();
    }
    if (lev_max < D_NLEV - 1) {            // the skipped children hand up zero bias forces
        for (int i = threadIdx.x; i < 24 * 6; i += 64) s.pAa[i] = 0.f;
        KP_SYNC();
    }
#pragma nounroll
    for (int lev = lev_max; lev >= 0; lev--) {
        const int sh = 5 * lev;
        const int bq = (int)((L.sb >> sh) & 31ull), c0 = (int)((L.sc0 >> sh) & 31ull), c1 = (int)((L.sc1 >> sh) & 31ull), c2 = (int)((L.sc2 >> sh) & 31ull);
        const bool active = bq != 31;
        const int b = active ? bq : 0;
        const int pr = 6 * 24;
        float pA = s.pAa[rowok ? 6 * c0 + r : pr];
        if ((L.multi >> lev) & 1u) pA += s.pAa[rowok ? 6 * c1 + r : pr] + s.pAa[rowok ? 6 * c2 + r : pr];
        if (wrench) pA -= rmask * wrench[6 * b + rc];
        const int nrounds = lev == 0 ? 2 : 1;
        for (int rd = 0; rd < nrounds; rd++) {
            const int d0 = lev == 0 ? (rd == 0 ? 3 : 0) : 6 + 3 * (b == 0 ? 0 : b - 1);
            float uo[3];
#pragma unroll
            for (int j = 2; j >= 0; j--) {
                const int d = d0 + j;
                const float u = (rhs ? rhs[d] : 0.f) - sum8(rmask * s.cdof[6 * d + rc] * pA);
                pA += rmask * s.U[6 * d + rc] * (u * s.Dinv[d]);
                uo[j] = u;
            }
            if (active && r == 0) {
#pragma unroll
                for (int j = 0; j < 3; j++) s.uj[d0 + j] = uo[j];
            }
        }
        if (active && rowok) s.pAa[6 * b + r] = pA;
        KP_SYNC();
    }
    aba_forward(s, L, out, lev_max);
}

}  // namespace kp
