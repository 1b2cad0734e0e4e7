// kp_step_pd.hpp -- stable-PD torque and residual force of the control step (XcArgs, xc_gains, spd_torque_rfc).  Part of kp_step_device.hpp.
#pragma once
#include "kp_step_aba.hpp"

namespace kp {

// ---------------------------------------------------------------- stable-PD torque + residual force (reference controller)
// The extended controller (XC, a UHC config other than uhc.yml's; humanoid_im.py:433-480, 506-524): the action row is `stride` wide; action_v0: the PD base
// pose is the target row as it is (cfg.a_ref, which the caller installs), without the 2 pi unwrap; rfc = 0: no residual force (applied[0:6] = 0, vf_dim 0);
// meta = 1 (meta_pd): kp / kd of every joint x clip(m + 1, 0, 10) with m = the action's meta entries [i_iter] / [i_iter + 15]; meta = 2 (meta_pd_joint):
// by joint, [j] / [69 + j].  The meta block starts at 69 + 6 rfc.  The scaled gains enter everywhere the SPD uses them: the K_d h armature, x and tau.
struct XcArgs { int stride, action_v0, rfc, meta; };
template <bool XC>
__device__ __forceinline__ void xc_gains(const DevTables& T, const XcArgs* X, const float* __restrict__ act, int j, int i_iter, float& kp, float& kd) {
    kp = T.kp[j]; kd = T.kd[j];
    if constexpr (XC) {
        if (X->meta && act) {
            const int m0 = 69 + 6 * X->rfc;
            const float mp = X->meta == 1 ? act[m0 + i_iter] : act[m0 + j], md = X->meta == 1 ? act[m0 + i_iter + 15] : act[m0 + 69 + j];
            kp = kp * fminf(fmaxf(mp + 1.f, 0.f), 10.f);
            kd = kd * fminf(fmaxf(md + 1.f, 0.f), 10.f);
        }
    }
}
template <int NT, bool OBJ, class SL, bool XC = false>
// tq / act: this env's rows of the PD target and the action in HBM (null: zeros); read here once per substep instead of living in LDS.  i_iter: the substep's
// index within the control step (the extended controller's meta_pd)
__device__ __forceinline__ void spd_torque_rfc(SL& s, const DevTables& T, const Params& P, const Lane8& L8, int tid, const float* __restrict__ tq, const float* __restrict__ act,
                                               const XcArgs* X = nullptr, int i_iter = 0) {
    float* const epv = SL::LEAN ? s.lim_jar - 6 : s.search;      // the position error of dof i >= 6 (lean layout: search is the solve's own vector, lim_jar is dead here)
    for (int i = tid; i < D_NV; i += NT) {
        float ep = 0.f, kp = 0.f, kd = 0.f;
        if (i >= 6) {
            int j = i - 6;
            float q = s.qpos[i + 1], base = tq ? tq[i + 1] : 0.f;
            // the reference's 2 pi unwrap loops (humanoid_im.py:447-452) in closed form: no trip count that depends on the data, so a
            // non-finite or absurd target cannot spin the wavefront (it yields a non-finite state, which diag flags)
            const float dq = base - q;
            if (!XC || !X->action_v0) {
                if (dq > 3.14159265358979f) base -= 6.28318530717959f * ceilf((dq - 3.14159265358979f) * 0.159154943091895f);
                else if (dq < -3.14159265358979f) base += 6.28318530717959f * ceilf((-dq - 3.14159265358979f) * 0.159154943091895f);
            }
            float target = base + (act ? act[j] : 0.f) * T.ascale[j];
            xc_gains<XC>(T, X, act, j, i_iter, kp, kd);
            ep = q + s.qvel[i] * P.h - target;
        }
        float kdh = kd * P.h;                         // (M + K_d dt): K_d dt is extra joint armature
        if constexpr (SL::LEAN) { asm volatile("" : "+v"(kdh)); kdh = T.dof_armature[i] + kdh; }      // the rounded product, then the sum aba_elim3 forms on the full layout (no fused multiply-add across the two)
        s.extra[i] = kdh;
        if (!SL::LEAN || i >= 6) epv[i] = ep;
        s.x[i] = -kp * ep - kd * s.qvel[i];
    }
    KP_SYNC();
    aba_solve<NT, OBJ>(s, P, L8, s.x, s.x, false, tid, D_NLEV, s.fb);
    for (int j = tid; j < D_NU; j += NT) {
        int i = j + 6;
        float kp, kd;
        xc_gains<XC>(T, X, act, j, i_iter, kp, kd);
        float tau = -kp * epv[i] - kd * (s.qvel[i] + s.x[i] * P.h);
        float lim = T.tlim[j];
        s.ctrl[j] = fminf(fmaxf(tau, -lim), lim);
    }
    if (tid == 0) {  // rfc_implicit
        Q4 cq = qmul(Q4{s.qpos[3], s.qpos[4], s.qpos[5], s.qpos[6]}, Q4{P.br_inv[0], P.br_inv[1], P.br_inv[2], P.br_inv[3]});
        float hn = sqrtf(cq.w * cq.w + cq.z * cq.z);
        Q4 hq = Q4{cq.w / hn, 0.f, 0.f, cq.z / hn};
        float ar[6];
#pragma unroll
        for (int k = 0; k < 6; k++) ar[k] = (act && (!XC || X->rfc)) ? act[69 + k] : 0.f;      // residual_force off: vf = 0 -> applied = 0
        V3 f = qrot(hq, v3(ar[0] * P.rfc_scale, ar[1] * P.rfc_scale, ar[2] * P.rfc_scale));
        float vf[6] = {f.x, f.y, f.z, ar[3] * P.rfc_scale, ar[4] * P.rfc_scale, ar[5] * P.rfc_scale};
#pragma unroll
        for (int k = 0; k < 6; k++) s.applied[k] = fminf(fmaxf(vf[k], -P.rfc_lim), P.rfc_lim);
    }
    KP_SYNC();
}

}  // namespace kp
