// kp_obs_ar_row.hpp -- one text for a row of HumanoidAREnv.get_ar_obs_v1 (kin_poly/envs/humanoid_ar_v1.py:133-214): the context view, the layout and
// the row itself as an inline function template.  k_obs_ar (kp_rollout_kernels.hpp) and k_obs_ar_ctx (kp_obs_ctx.hip) are both a row pointer plus
// obs_ar_row, so the base block of the wide row is the plain row bit for bit by construction.  No kernel is defined here: any unit may include it.
#pragma once
#include "kp_quat.hpp"

namespace kp {

struct CtxDev {  // mirrors kp_ctx in include/kinpoly_sim.h
    int T;
    const float *head_pose, *head_vels, *obj_rel, *action_one_hot, *gt_bquat, *gt_wbpos, *obj_qpos;
    const int* cur_t;
    const int* row;      // optional: env e reads context row row[e] of the [R, T, .] arrays (null: row e)
    __device__ __forceinline__ size_t r(int e) const { return row ? (size_t)row[e] : (size_t)e; }
};

// transform_vec(v, q, 'heading') of the observation row: q_tmul_vec(q_heading(q), v) with its contraction written out.  Each component is a sum of
// three products, which the compiler contracts into one product and two fused multiply-adds; which product stays the plain one is its choice per
// kernel, and the observation kernels must agree to the bit.  So the row pins it: x keeps m3 vy, y keeps m1 vx, z keeps m2 vx.  Only the observation
// row rotates with this; q_tmul_vec keeps its plain text for everybody else.
__device__ __forceinline__ V3 tv_heading(V3 v, Q4 q) {
    float m[9]; q_matrix(q_heading(q), m);
    return V3{fmaf(m[6], v.z, fmaf(m[0], v.x, m[3] * v.y)), fmaf(m[7], v.z, fmaf(m[4], v.y, m[1] * v.x)), fmaf(m[8], v.z, fmaf(m[5], v.y, m[2] * v.x))};
}

// The observation's switches (humanoid_ar_v1.py:183-201; a statear yml's use_vel / use_head / use_action).  Blocks in the reference's order:
//   [0, 74) height, de-headed root quaternion, joint angles | VEL: 75 qvel (data.qvel[:75], :184-185) | HEAD: diff_hpos 3, diff_hrot 4 (:187-189) |
//   predicted object relative to head 7 (:191-192) | HEAD: t_havel 3, t_hlvel 3, t_obj_relative_head 7 (:194-198) | ACTION: one-hot 4 (:200-201)
// D is the row width: 105 / 101 for <false, true, .> (kin_poly.yml / kin_poly_wo_action.yml), 180 / 176 with VEL, 85 / 81 without HEAD, 160 / 156 with VEL and without HEAD.
template <bool VEL, bool HEAD, bool ACTION>
struct ObsArLayout {
    static constexpr int O_VEL = 74, O_DIFF = O_VEL + (VEL ? 75 : 0), O_OBJ = O_DIFF + (HEAD ? 7 : 0), O_TGT = O_OBJ + 7, O_ACT = O_TGT + (HEAD ? 13 : 0),
                         D = O_ACT + (ACTION ? 4 : 0);
};

// Row e of the observation into o, by lane l of the 32 lanes an env has: the 69 joint angles and the 75 velocities are copied lane-strided, the five
// short blocks go to lanes 0 .. 4, each with the same expressions in every layout (a block two layouts share is equal bit for bit).  No LDS, no
// cross-lane traffic.  The state arrays are the kernel's __restrict__ parameters, passed on with the qualifier.
template <bool VEL, bool HEAD, bool ACTION>
__device__ __forceinline__ void obs_ar_row(const CtxDev& C, int e, int l, const float* __restrict__ qpos, const float* __restrict__ qvel,
                                           const float* __restrict__ xpos, const float* __restrict__ xquat, float* __restrict__ o) {
    using L = ObsArLayout<VEL, HEAD, ACTION>;
    const float* q = qpos + (size_t)e * D_NQ;
    for (int j = l; j < D_NU; j += 32) o[5 + j] = q[7 + j];
    if (VEL) {
        const float* v = qvel + (size_t)e * D_NV;
        for (int j = l; j < D_NV; j += 32) o[L::O_VEL + j] = v[j];
    }
    if (l > 4) return;
    if (l == 0) {
        Q4 rq = Q4{q[3], q[4], q[5], q[6]};
        Q4 dh = qmul(q_inverse(q_heading(rq)), rq);  // de_heading(qpos[3:7]) (:140-141)
        o[0] = q[2]; o[1] = dh.w; o[2] = dh.x; o[3] = dh.y; o[4] = dh.z;
        return;
    }
    int t = C.cur_t[e];
    t = t < 0 ? 0 : (t >= C.T ? C.T - 1 : t);
    const float* oh = C.action_one_hot + C.r(e) * 4;
    if (l == 4) {
        if (ACTION) for (int k = 0; k < 4; k++) o[L::O_ACT + k] = oh[k];
        return;
    }
    if (l == 3) {
        if (HEAD) {
            const float* hv = C.head_vels + (C.r(e) * C.T + t) * 6;
            const float* orl = C.obj_rel + (C.r(e) * C.T + t) * 7;
            float* g = o + L::O_TGT;
            g[0] = hv[3]; g[1] = hv[4]; g[2] = hv[5];
            g[3] = hv[0]; g[4] = hv[1]; g[5] = hv[2];
            for (int k = 0; k < 7; k++) g[6 + k] = orl[k];
        }
        return;
    }
    const int hb = 13;
    V3 hpos = ld3(xpos + (size_t)e * 72 + 3 * hb);
    const float* hq4 = xquat + (size_t)e * 96 + 4 * hb;
    Q4 hrot = Q4{hq4[0], hq4[1], hq4[2], hq4[3]};
    if (l == 1) {
        if (HEAD) {
            const float* hp = C.head_pose + (C.r(e) * C.T + t) * 7;
            st3(o + L::O_DIFF, tv_heading(ld3(hp) - hpos, hrot));
            Q4 dr = qmul(q_inverse(Q4{hp[3], hp[4], hp[5], hp[6]}), hrot);
            float* g = o + L::O_DIFF + 3;
            g[0] = dr.w; g[1] = dr.x; g[2] = dr.y; g[3] = dr.z;
        }
        return;
    }
    float ohs = oh[0] + oh[1] + oh[2] + oh[3];
    V3 opos = v3(0.f, 0.f, 0.f); Q4 orot = Q4{1.f, 0.f, 0.f, 0.f};   // get_obj_qpos: [0,0,0,1,0,0,0] when no action (:465-466)
    if (ohs != 0.f && C.obj_qpos) { const float* ob = C.obj_qpos + (size_t)e * 7; opos = ld3(ob); orot = Q4{ob[3], ob[4], ob[5], ob[6]}; }
    st3(o + L::O_OBJ, tv_heading(opos - hpos, hrot));
    Q4 ol = qmul(q_inverse(q_heading(hrot)), orot);
    float* g = o + L::O_OBJ + 3;
    g[0] = ol.w; g[1] = ol.x; g[2] = ol.y; g[3] = ol.z;
}

}  // namespace kp
