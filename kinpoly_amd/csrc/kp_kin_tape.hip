// kp_kin_tape.hip -- the kernels declared in kp_kin_tape.hpp (see there).  Every forward quantity a gradient needs is recomputed from the forward
// call's inputs with the forward kernel's own expressions (kp_obs_kernels.hpp: k_kin_advance; kp_obs_ar_row.hpp: obs_ar_row) and the helpers those
// kernels use (kp_quat.hpp), so the tape holds tensors the roll-out keeps anyway and no kernel-private state.
//
// Two identities carry every rotation gradient:
//   * R(r / |r|) with r -> r + dr turns its image by the world rotation vector dphi, (0, dphi) = 2 (du (x) u^-1), u = r / |r|.  A cotangent that meets dphi as
//     dphi . tau (a torque) is therefore the quaternion gradient 2 (0, tau) (x) u / |r| -- orthogonal to u: no radial component (k_fk_wbpos_grad's root rule);
//   * p = a (x) b: cotangent g gives g (x) conj(b) for a and conj(a) (x) g for b.
#include "kp_kin_tape.hpp"
#include "kp_quat.hpp"

namespace kp {

namespace {

constexpr int KT_HEAD = 13;                                                  // body "Head" of the SMPL tree

__device__ __forceinline__ Q4 operator+(Q4 a, Q4 b) { return Q4{a.w + b.w, a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Q4 operator*(float s, Q4 a) { return Q4{s * a.w, s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float kt_dot4(Q4 a, Q4 b) { return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 kt_vec(Q4 q) { return v3(q.x, q.y, q.z); }
// the quaternion gradient of a torque on R(r / |r|): u = r / |r|, inv_n = 1 / |r|
__device__ __forceinline__ Q4 kt_torque_grad(V3 tau, Q4 u, float inv_n) { return inv_n * qmul(Q4{0.f, 2.0f * tau.x, 2.0f * tau.y, 2.0f * tau.z}, u); }
// get_heading_q of q as a turn about z by theta = 2 atan2(z, w): cos, sin, and d theta / d (w, z)
struct KtHeading { float c, s, dw, dz; };
__device__ __forceinline__ KtHeading kt_heading(Q4 q) {
    const float inv = 1.0f / (q.w * q.w + q.z * q.z);
    return KtHeading{(q.w * q.w - q.z * q.z) * inv, 2.0f * q.w * q.z * inv, -2.0f * q.z * inv, 2.0f * q.w * inv};
}
// gradient of inverse(get_heading_q(q)) = (c, 0, 0, -s), (c, s) = (w, z) / |(w, z)|, from the cotangent ga of that quaternion: -> d / d (w, z)
__device__ __forceinline__ void kt_inv_heading_grad(Q4 q, Q4 ga, float& gw, float& gz) {
    const float n = sqrtf(q.w * q.w + q.z * q.z), c = q.w / n, s = q.z / n;
    const float gc = ga.w, gs = -ga.z, rad = c * gc + s * gs;
    gw = (gc - c * rad) / n; gz = (gs - s * rad) / n;
}

}  // namespace

// ---------------------------------------------------------------- (d k_kin_advance)^T, one thread per row
__global__ __launch_bounds__(128) void k_kin_advance_grad(KinAdvanceGradArgs A) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.n) return;
    const float* q = A.qpos + (size_t)e * D_NQ;
    const float* a = A.act + (size_t)e * 80;
    const float* gn = A.g_next ? A.g_next + (size_t)e * D_NQ : nullptr;
    const float* gv = A.g_qvel ? A.g_qvel + (size_t)e * D_NV : nullptr;
    float* oq = A.g_qpos + (size_t)e * D_NQ;
    float* oa = A.g_act + (size_t)e * 80;
    const float dt = A.dt, idt = 1.0f / dt;
#define KT_GN(i) (gn ? gn[i] : 0.f)
#define KT_GV(i) (gv ? gv[i] : 0.f)
    const Q4 rot = ldq(q + 3);
    // ---- linear part: next.xy = q.xy + dt Rz(heading) a[74:76], v.xy = (next.xy - q.xy) / dt; next.z = a[0], v.z = (a[0] - q.z) / dt
    const KtHeading H = kt_heading(rot);
    const float glx = (KT_GN(0) + KT_GV(0) * idt) * dt, gly = (KT_GN(1) + KT_GV(1) * idt) * dt;
    oa[74] = H.c * glx + H.s * gly; oa[75] = -H.s * glx + H.c * gly; oa[76] = 0.f;
    const float gth = glx * (-H.s * a[74] - H.c * a[75]) + gly * (H.c * a[74] - H.s * a[75]);
    Q4 grot = Q4{gth * H.dw, 0.f, 0.f, gth * H.dz};
    oq[0] = KT_GN(0); oq[1] = KT_GN(1);                 // d v.xy / d q.xy = (1 - 1) / dt
    oq[2] = -KT_GV(2) * idt;
    oa[0] = KT_GN(2) + KT_GV(2) * idt; oa[1] = oa[2] = oa[3] = oa[4] = 0.f;
    for (int j = 0; j < D_NU; j++) { const float g = KT_GV(6 + j) * idt; oa[5 + j] = KT_GN(7 + j) + g; oq[7 + j] = -g; }
    // ---- angular part, forward (k_kin_advance's expressions)
    float m[9];
    q_matrix(rot, m);
    const V3 angv = mulmat(m, v3(a[77], a[78], a[79]));
    const V3 ev = dt * angv;
    const float ang = sqrtf(dot(ev, ev));
    const bool guard = ang < 1e-12f;                                  // q_from_expmap's constant axis: no gradient through the expmap
    float hs, hc; sincosf(0.5f * ang, &hs, &hc);
    const V3 nh = guard ? v3(1.f, 0.f, 0.f) : (1.0f / ang) * ev;
    const Q4 ex = Q4{hc, nh.x * hs, nh.y * hs, nh.z * hs};
    const Q4 nraw = qmul(ex, rot);
    const float nn = sqrtf(kt_dot4(nraw, nraw));
    const Q4 nr = (1.0f / nn) * nraw;
    const float c2 = kt_dot4(rot, rot), cn = sqrtf(c2);
    const Q4 rinv = (1.0f / c2) * qconj(rot);
    const Q4 qrel = qmul(nr, rinv);
    const Q4 u = (1.0f / cn) * rot;
    const float sn = sqrtf(qrel.x * qrel.x + qrel.y * qrel.y + qrel.z * qrel.z);
    const bool small = !(sn > 0.0f) || (ev.x == 0.0f && ev.y == 0.0f && ev.z == 0.0f);
    // ---- angular part, backward
    Q4 gnr = Q4{KT_GN(3), KT_GN(4), KT_GN(5), KT_GN(6)};
    if (!small) {                                                      // the `small` rows' angular velocity is the constant 0 (torch.where's gradient)
        const V3 g_rv = qrot(u, v3(KT_GV(3), KT_GV(4), KT_GV(5)));     // wv = R(u)^T rv
        const V3 axis = (1.0f / sn) * kt_vec(qrel);
        float angle = 2.0f * atan2f(sn, qrel.w);
        if (angle > KP_PI) angle -= KP_2PI;
        if (angle < -KP_PI) angle += KP_2PI;
        const V3 rv = (angle * idt) * axis;
        grot = grot + kt_torque_grad(cross(g_rv, rv), u, 1.0f / cn);
        const float g_angle = idt * dot(axis, g_rv);
        const V3 g_axis = (angle * idt) * g_rv;
        const float d = sn * sn + qrel.w * qrel.w;                     // atan2(sn, w): d / d sn = w / d, d / d w = -sn / d
        const V3 g_xyz = (1.0f / sn) * (g_axis - dot(axis, g_axis) * axis) + (g_angle * 2.0f * qrel.w / d) * axis;
        const Q4 g_qrel = Q4{-g_angle * 2.0f * sn / d, g_xyz.x, g_xyz.y, g_xyz.z};
        gnr = gnr + qmul(g_qrel, qconj(rinv));
        const Q4 h = qmul(qconj(nr), g_qrel);                          // cotangent of rinv = conj(rot) / |rot|^2
        grot = grot + (1.0f / c2) * qconj(h) + (-2.0f * kt_dot4(h, rinv) / c2) * rot;
    }
    const Q4 graw = (1.0f / nn) * (gnr + (-kt_dot4(nr, gnr)) * nr);   // next = nraw / |nraw|
    const Q4 gex = qmul(graw, qconj(rot));
    grot = grot + qmul(qconj(ex), graw);
    V3 g_angv = v3(0.f, 0.f, 0.f);
    if (!guard) {
        // ex = (cos(ang / 2), f ev), f = sin(ang / 2) / ang; f' next to 0 from its series (the closed form cancels)
        const float f = hs / ang;
        const float fp = ang < 0.05f ? ang * (-1.0f / 24.0f + ang * ang * (1.0f / 960.0f)) : (0.5f * hc * ang - hs) / (ang * ang);
        const V3 gx = kt_vec(gex);
        g_angv = dt * (f * gx + (-0.5f * hs * gex.w + fp * dot(ev, gx)) * nh);
    }
    st3(oa + 77, tmulmat(m, g_angv));
    grot = grot + kt_torque_grad(cross(angv, g_angv), u, 1.0f / cn);
    stq(oq + 3, grot);
#undef KT_GN
#undef KT_GV
}

// ---------------------------------------------------------------- (d k_obs_ar)^T, one thread per row
// Blocks as kp::ObsArLayout: [0, 74) local pose | VEL 75 | HEAD: diff_hpos 3, diff_hrot 4 | object relative to head 7 | HEAD: 13 targets | one-hot.
template <bool VEL, bool HEAD>
__global__ __launch_bounds__(64) void k_obs_ar_grad(ObsArGradArgs A) {
    constexpr int O_DIFF = 74 + (VEL ? 75 : 0), O_OBJ = O_DIFF + (HEAD ? 7 : 0);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.n) return;
    const float* g = A.g_obs + (size_t)e * A.width;
    const float* q = A.qpos + (size_t)e * D_NQ;
    float* oq = A.g_qpos + (size_t)e * D_NQ;
    // local pose: height, de_heading(root) = inverse(heading(root)) (x) root, joint angles
    const Q4 rq = ldq(q + 3);
    const Q4 gd = ldq(g + 1);
    float gw, gz;
    kt_inv_heading_grad(rq, qmul(gd, qconj(rq)), gw, gz);
    const float rn = sqrtf(rq.w * rq.w + rq.z * rq.z);
    Q4 gr = qmul(Q4{rq.w / rn, 0.f, 0.f, rq.z / rn}, gd);
    gr.w += gw; gr.z += gz;
    oq[0] = 0.f; oq[1] = 0.f; oq[2] = g[0];
    stq(oq + 3, gr);
    for (int j = 0; j < D_NU; j++) oq[7 + j] = g[5 + j];
    if (VEL) {
        float* ov = A.g_qvel + (size_t)e * D_NV;
        for (int j = 0; j < D_NV; j++) ov[j] = g[74 + j];
    }
    // the head's position and world quaternion
    const V3 hpos = ld3(A.wbpos + (size_t)e * 72 + 3 * KT_HEAD);
    const Q4 hrot = ldq(A.wbquat + (size_t)e * 96 + 4 * KT_HEAD);
    const KtHeading H = kt_heading(hrot);
    V3 ghp = v3(0.f, 0.f, 0.f);
    Q4 ghq = Q4{0.f, 0.f, 0.f, 0.f};
    // out = transform_vec(D, hrot, 'heading') = Rz(-theta) D with D = target - hpos: cotangent gb
    auto pos_block = [&](V3 D, V3 gb) {
        const V3 out = v3(H.c * D.x + H.s * D.y, -H.s * D.x + H.c * D.y, D.z);
        ghp = ghp - v3(H.c * gb.x - H.s * gb.y, H.s * gb.x + H.c * gb.y, gb.z);
        const float gth = gb.x * out.y - gb.y * out.x;
        ghq.w += gth * H.dw; ghq.z += gth * H.dz;
    };
    const size_t r = A.row ? (size_t)A.row[e] : (size_t)e;
    if (HEAD) {
        int t = A.cur_t[e];
        t = t < 0 ? 0 : (t >= A.T ? A.T - 1 : t);
        const float* hp = A.head_pose + (r * A.T + t) * 7;
        pos_block(ld3(hp) - hpos, ld3(g + O_DIFF));
        const Q4 th = ldq(hp + 3);                                     // diff_hrot = inverse(t_hrot) (x) hrot, inverse = conj / dot
        ghq = ghq + qmul((1.0f / kt_dot4(th, th)) * th, ldq(g + O_DIFF + 3));
    }
    float gob[7];
    for (int k = 0; k < 7; k++) gob[k] = g[O_OBJ + k] + (A.g_obj ? A.g_obj[(size_t)e * 7 + k] : 0.f);
    const float* oh = A.action_one_hot + r * 4;
    const float ohs = oh[0] + oh[1] + oh[2] + oh[3];
    V3 opos = v3(0.f, 0.f, 0.f); Q4 orot = Q4{1.f, 0.f, 0.f, 0.f};
    if (ohs != 0.f && A.obj_qpos) { const float* ob = A.obj_qpos + (size_t)e * 7; opos = ld3(ob); orot = ldq(ob + 3); }
    pos_block(opos - hpos, v3(gob[0], gob[1], gob[2]));
    kt_inv_heading_grad(hrot, qmul(Q4{gob[3], gob[4], gob[5], gob[6]}, qconj(orot)), gw, gz);      // inverse(heading(hrot)) (x) orot
    ghq.w += gw; ghq.z += gz;
    st3(A.g_hpos + (size_t)e * 3, ghp);
    stq(A.g_hquat + (size_t)e * 4, ghq);
}

// ---------------------------------------------------------------- (d k_target_fk)^T for wbpos and the head's world quaternion
// k_fk_wbpos_grad's scheme (one wave per row, lane = body; F_b, M_b over the strict descendants of b) with two additions: the head position's cotangent
// joins the head's slot of grad_wbpos, and the head quaternion's cotangent g acts as the torque T = vec(g (x) conj(hquat)) / 2 on every hinge of
// the head's root path, the head's own included (a hinge turning about the world axis a by d theta changes hquat by (0, a d theta) (x) hquat / 2).
__global__ __launch_bounds__(256) void k_fk_head_grad(FkHeadGradArgs A) {
    __shared__ float sp[4][D_NB * 3], sg[4][D_NB * 3];
    const int w = threadIdx.x >> 6, b = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + w;
    const bool live = e < A.n;
    if (live && b < D_NB) {
        st3(sp[w] + 3 * b, ld3(A.wbpos + (size_t)e * 72 + 3 * b));
        V3 g = A.g_wbpos ? ld3(A.g_wbpos + (size_t)e * 72 + 3 * b) : v3(0.f, 0.f, 0.f);
        if (b == KT_HEAD && A.g_hpos) g = g + ld3(A.g_hpos + (size_t)e * 3);
        st3(sg[w] + 3 * b, g);
    }
    __syncthreads();
    if (!live || b >= D_NB) return;
    const V3 pb = ld3(sp[w] + 3 * b);
    V3 F = v3(0.f, 0.f, 0.f), M = v3(0.f, 0.f, 0.f);
    const int nb = A.subtree[b];
    for (int j = b + 1; j < b + nb && j < D_NB; j++) {
        const V3 g = ld3(sg[w] + 3 * j);
        F = F + g; M = M + cross(ld3(sp[w] + 3 * j) - pb, g);
    }
    if (A.g_hquat && b <= KT_HEAD && KT_HEAD < b + nb) {
        const Q4 t = qmul(ldq(A.g_hquat + (size_t)e * 4), qconj(ldq(A.wbquat + (size_t)e * 96 + 4 * KT_HEAD)));
        M = M + 0.5f * kt_vec(t);
    }
    const float* q = A.qpos + (size_t)e * D_NQ;
    const float* add = A.g_add ? A.g_add + (size_t)e * D_NQ : nullptr;
    float* o = A.g_qpos + (size_t)e * D_NQ;
    if (b == 0) {
        const V3 f0 = F + ld3(sg[w]);
        const float qn = sqrtf(q[3] * q[3] + q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
        const Q4 G = kt_torque_grad(M, ldq(A.wbquat + (size_t)e * 96), 1.0f / qn);
        const float r[7] = {f0.x, f0.y, f0.z, G.w, G.x, G.y, G.z};
        for (int i = 0; i < 7; i++) o[i] = r[i] + (add ? add[i] : 0.f);
    } else {
        const int p = A.parent[b];
        float R[9];
        q_matrix(ldq(A.wbquat + (size_t)e * 96 + 4 * p), R);
        const int c = 7 + 3 * (b - 1);
        const float tz = q[c], ty = q[c + 1];
        float sz, cz, sy, cy;
        sincosf(tz, &sz, &cz); sincosf(ty, &sy, &cy);
        const V3 az = mulmat(R, v3(0.f, 0.f, 1.f));
        const V3 ay = mulmat(R, v3(-sz, cz, 0.f));                  // Rz e_y
        const V3 ax = mulmat(R, v3(cz * cy, sz * cy, -sy));         // Rz Ry e_x
        const float r[3] = {dot(az, M), dot(ay, M), dot(ax, M)};
        for (int i = 0; i < 3; i++) o[c + i] = r[i] + (add ? add[c + i] : 0.f);
    }
}

hipError_t launch_kin_advance_grad(const KinAdvanceGradArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(k_kin_advance_grad, dim3((A.n + 127) / 128), dim3(128), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_obs_ar_grad(const ObsArGradArgs& A, hipStream_t stream) {
    const dim3 grid((A.n + 63) / 64), block(64);
    if (A.vel && A.head) hipLaunchKernelGGL((k_obs_ar_grad<true, true>), grid, block, 0, stream, A);
    else if (A.vel) hipLaunchKernelGGL((k_obs_ar_grad<true, false>), grid, block, 0, stream, A);
    else if (A.head) hipLaunchKernelGGL((k_obs_ar_grad<false, true>), grid, block, 0, stream, A);
    else hipLaunchKernelGGL((k_obs_ar_grad<false, false>), grid, block, 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_fk_head_grad(const FkHeadGradArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(k_fk_head_grad, dim3((A.n + 3) / 4), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace kp
