// kp_step_kin.hpp -- kinematics, velocities and bias wrenches of the control step (forward_kin_bias).  Part of kp_step_device.hpp.
#pragma once
#include "kp_step_args.hpp"

namespace kp {

// ---------------------------------------------------------------- kinematics + velocities + bias
// Phases, so that the level-serial chain stays short:
//   0. half-angle sin/cos of all 69 hinge angles, one lane per hinge (scratch: s.U, free outside the ABA passes), then per
//      body (parallel) the local rotation qz qy qx and the second / third hinge axis in the parent frame;
//   K. two short level-synchronous chains (lane = body) with a body-parallel block between them: world pose; then motion axes cdof
//      and each body's own velocity terms; then spatial velocity cvel and the velocity-product acceleration cacc
//      (mj_kinematics + mj_comVel + the forward half of mj_rne);
//   B. body-parallel (24 lanes at once): COM, world inertia about o, body wrench fb = I a + v x* I v.  qfrc_bias itself
//      (backward half of mj_rne: subtree sums + projection on the dofs) is never formed: the solves take fb as bias force.
template <int NT, class SL>
__device__ __forceinline__ void forward_kin_bias(SL& s, const DevTables& T, const Params& P, int depth, V3 bpos, int tid) {
    float* sc = s.U;              // scratch (free outside the ABA passes): [0, 138) half-angle sin/cos, [144, 384) per-body joint frames
    float* jf = s.U + 144;        // per body: local rotation qz (x) qy (x) qx (4), second axis R(qz) e_y (3), third axis R(qz qy) e_x (3)
    for (int i = tid; i < D_NU; i += NT) { float sn, cs; sincosf(0.5f * s.qpos[7 + i], &sn, &cs); sc[2 * i] = sn; sc[2 * i + 1] = cs; }
    KP_SYNC();
    if (tid >= 1 && tid < D_NB) {         // body-parallel: everything of the three hinges that does not depend on the parent
        const int j0 = 3 * (tid - 1);
        const Q4 qz = Q4{sc[2 * j0 + 1], 0.f, 0.f, sc[2 * j0]}, qy = Q4{sc[2 * j0 + 3], 0.f, sc[2 * j0 + 2], 0.f}, qx = Q4{sc[2 * j0 + 5], sc[2 * j0 + 4], 0.f, 0.f};
        const Q4 qzy = qmul(qz, qy);
        const Q4 ql = qmul(qzy, qx);
        const V3 a1 = qrot(qz, v3(0.f, 1.f, 0.f)), a2 = qrot(qzy, v3(1.f, 0.f, 0.f));
        float* f = jf + 10 * tid;
        f[0] = ql.w; f[1] = ql.x; f[2] = ql.y; f[3] = ql.z; st3(f + 4, a1); st3(f + 7, a2);
    }
    KP_SYNC();
    if (tid == 0) {                       // root (level 0): free joint
        const Q4 q = qnormalize(Q4{s.qpos[3], s.qpos[4], s.qpos[5], s.qpos[6]});
        s.qpos[3] = q.w; s.qpos[4] = q.x; s.qpos[5] = q.y; s.qpos[6] = q.z;
        const V3 pos = ld3(s.qpos);
        float R[9]; q2mat(q, R);
        const V3 vl = ld3(s.qvel), wb = ld3(s.qvel + 3);
        const V3 ww = mulmat(R, wb);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float* c = s.cdof + 6 * k;
            c[0] = c[1] = c[2] = 0.f; c[3] = k == 0; c[4] = k == 1; c[5] = k == 2;
            float* r = s.cdof + 6 * (3 + k);
            r[0] = R[k]; r[1] = R[3 + k]; r[2] = R[6 + k]; r[3] = r[4] = r[5] = 0.f;
        }
        st3(s.xpos, pos);
        s.xquat[0] = q.w; s.xquat[1] = q.x; s.xquat[2] = q.y; s.xquat[3] = q.z;
        sts6(s.sv, S6{ww, vl}); sts6(s.sa, S6{v3(0.f, 0.f, 0.f), v3(-P.gx, -P.gy, -P.gz) + cross(vl, ww)});
    }
    KP_SYNC();
    // K1. pose chain (level-synchronous, lane = body): world position and orientation only
#pragma nounroll
    for (int lev = 1; lev < D_NLEV; lev++) {
        if (depth == lev) {
            const int b = tid;
            const int p = s.bpar[b];
            const Q4 q = Q4{s.xquat[4 * p], s.xquat[4 * p + 1], s.xquat[4 * p + 2], s.xquat[4 * p + 3]};
            const V3 ppos = ld3(s.xpos + 3 * p);
            const float* f = jf + 10 * b;
            const Q4 ql = Q4{f[0], f[1], f[2], f[3]};
            const V3 pos = ppos + qrot(q, bpos);
            const Q4 qn = qnormalize(qmul(q, ql));
            st3(s.xpos + 3 * b, pos);
            s.xquat[4 * b] = qn.w; s.xquat[4 * b + 1] = qn.x; s.xquat[4 * b + 2] = qn.y; s.xquat[4 * b + 3] = qn.z;
        }
        KP_SYNC();
    }
    // K2. body-parallel: motion axes of the three hinges (about o) and the body's own share of the velocity chain.  With
    // run_j = sum_{i<j} qd_i cdof_i the level-serial recursion  cv += qd_j cdof_j,  ca += qd_j (cv x cdof_j)  splits into
    //   cv_b = cv_p + dv,   ca_b = ca_p + cv_p x dv + loc,   dv = run_3,   loc = sum_j qd_j (run_j x cdof_j)
    // (x = cross_motion, bilinear), so that only two 6-vector updates per body remain on the chain.
    S6 dv = S6{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)}, loc = dv;
    if (tid >= 1 && tid < D_NB) {
        const int b = tid;
        const int p = s.bpar[b];
        const int d0 = 6 + 3 * (b - 1);
        const V3 o = ld3(s.xpos);
        const Q4 q = Q4{s.xquat[4 * p], s.xquat[4 * p + 1], s.xquat[4 * p + 2], s.xquat[4 * p + 3]};
        const V3 r = o - ld3(s.xpos + 3 * b);
        const float qds[3] = {s.qvel[d0], s.qvel[d0 + 1], s.qvel[d0 + 2]};
        const float* f = jf + 10 * b;
        const V3 a1 = ld3(f + 4), a2 = ld3(f + 7);
        float R[9];
        q2mat(q, R);                                           // parent rotation: the three hinge axes are R e_z, R a1, R a2
        const V3 axes[3] = {v3(R[2], R[5], R[8]), mulmat(R, a1), mulmat(R, a2)};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const S6 cd = S6{axes[j], cross(axes[j], r)};
            sts6(s.cdof + 6 * (d0 + j), cd);
            if (j > 0) loc = loc + qds[j] * cross_motion(dv, cd);
            dv = dv + qds[j] * cd;
        }
    }
    KP_SYNC();
    // K3. velocity chain (level-synchronous): spatial velocity cvel and velocity-product acceleration cacc
#pragma nounroll
    for (int lev = 1; lev < D_NLEV; lev++) {
        if (depth == lev) {
            const int b = tid;
            const int p = s.bpar[b];
            const S6 cvp = lds6(s.sv + 6 * p), cap = lds6(s.sa + 6 * p);
            sts6(s.sv + 6 * b, cvp + dv);
            sts6(s.sa + 6 * b, cap + cross_motion(cvp, dv) + loc);
        }
        KP_SYNC();
    }
    if (tid < D_NB) {
        const int b = tid;
        const V3 o = ld3(s.xpos), pos = ld3(s.xpos + 3 * b);
        float R[9];
        q2mat(Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]}, R);
        const S6 cv = lds6(s.sv + 6 * b), ca = lds6(s.sa + 6 * b);
        const V3 xi = pos + mulmat(R, ld3(T.body_ipos + 3 * b));
        const float* Ib = T.body_inertia + 6 * b;
        float I3[9] = {Ib[0], Ib[3], Ib[4], Ib[3], Ib[1], Ib[5], Ib[4], Ib[5], Ib[2]};
        float Tm[9], W[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Tm[3 * i + j] = R[3 * i] * I3[j] + R[3 * i + 1] * I3[3 + j] + R[3 * i + 2] * I3[6 + j];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) W[3 * i + j] = Tm[3 * i] * R[3 * j] + Tm[3 * i + 1] * R[3 * j + 1] + Tm[3 * i + 2] * R[3 * j + 2];
        const V3 rr = xi - o;
        const float mass = T.body_mass[b], r2 = dot(rr, rr);
        float* ci = s.cinert + 10 * b;
        ci[0] = W[0] + mass * (r2 - rr.x * rr.x); ci[1] = W[4] + mass * (r2 - rr.y * rr.y); ci[2] = W[8] + mass * (r2 - rr.z * rr.z);
        ci[3] = W[1] - mass * rr.x * rr.y; ci[4] = W[2] - mass * rr.x * rr.z; ci[5] = W[5] - mass * rr.y * rr.z;
        ci[6] = mass * rr.x; ci[7] = mass * rr.y; ci[8] = mass * rr.z; ci[9] = mass;
        const S6 f = inert_mul(ci, ca) + cross_force(cv, inert_mul(ci, cv));
        sts6(s.fb + 6 * b, f);         // stays a body wrench: the articulated-body passes fold it into their bias force,
    }                                  // which is the backward half of mj_rne (subtree sums + projection) done for free
    KP_SYNC();
}

}  // namespace kp
