// kp_quat.hpp -- inline device math every translation unit may share: the reference's quaternion helpers (uhc/khrylib/utils/math.py:102-198 and
// transformation.py, Gohlke), the quaternion load / store / conjugate, the sigmoid of the GRU gates and the wrap constants.  Only
// __device__ __forceinline__ functions and constants: no kernel is defined here, so including it moves no other kernel's code generation.
#pragma once
#include "kp_device.hpp"

namespace kp {

constexpr float KP_PI = 3.14159265358979f, KP_2PI = 6.28318530717959f;      // the constants an angle is wrapped into (-pi, pi] with (k_kin_advance and its gradient)

__device__ __forceinline__ Q4 ldq(const float* p) { return Q4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void stq(float* p, Q4 q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }
__device__ __forceinline__ Q4 qconj(Q4 q) { return Q4{q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ float kp_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

// ---- reference quaternion helpers (w,x,y,z); these do NOT assume unit quaternions where the reference does not
__device__ __forceinline__ Q4 q_inverse(Q4 q) {  // quaternion_inverse: conj / dot
    float n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    return Q4{q.w / n, -q.x / n, -q.y / n, -q.z / n};
}
__device__ __forceinline__ void q_matrix(Q4 q, float* m) {  // quaternion_matrix: normalises by dot, identity if ~0
    float n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    if (n < 8.881784197001252e-16f) { m[0] = m[4] = m[8] = 1.f; m[1] = m[2] = m[3] = m[5] = m[6] = m[7] = 0.f; return; }
    float s = sqrtf(2.0f / n);
    float w = q.w * s, x = q.x * s, y = q.y * s, z = q.z * s;
    m[0] = 1.f - y * y - z * z; m[1] = x * y - z * w; m[2] = x * z + y * w;
    m[3] = x * y + z * w; m[4] = 1.f - x * x - z * z; m[5] = y * z - x * w;
    m[6] = x * z - y * w; m[7] = y * z + x * w; m[8] = 1.f - x * x - y * y;
}
__device__ __forceinline__ V3 tmulmat(const float* m, V3 v) {                                                       // m^T v (mulmat of kp_device.hpp is m v)
    return V3{m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z, m[2] * v.x + m[5] * v.y + m[8] * v.z};
}
__device__ __forceinline__ V3 q_mul_vec(Q4 q, V3 v) { float m[9]; q_matrix(q, m); return mulmat(m, v); }            // quat_mul_vec
__device__ __forceinline__ V3 q_tmul_vec(Q4 q, V3 v) { float m[9]; q_matrix(q, m); return tmulmat(m, v); }          // transform_vec(.., 'root')
__device__ __forceinline__ Q4 q_heading(Q4 q) {  // get_heading_q
    float n = sqrtf(q.w * q.w + q.z * q.z);
    return Q4{q.w / n, 0.f, 0.f, q.z / n};
}
__device__ __forceinline__ float heading_angle(Q4 q) {  // get_heading
    float w = q.w, z = q.z;
    if (z < 0.f) { w = -w; z = -z; }
    // 2 acos(w / |(w, z)|) with z >= 0, as the angle of the point (w, z): acos next to 1 would turn the 6e-8 of an fp32 cosine into 1e-4 rad
    // for a heading of 1e-3 rad (the reference works in fp64)
    return 2.0f * atan2f(fabsf(z), w);
}
__device__ __forceinline__ Q4 q_from_expmap(V3 e) {  // quat_from_expmap + quaternion_about_axis
    float angle = sqrtf(dot(e, e));
    V3 axis = angle < 1e-12f ? v3(1.f, 0.f, 0.f) : (1.0f / angle) * e;
    float sn, cs; sincosf(0.5f * angle, &sn, &cs);
    float ql = sqrtf(dot(axis, axis));
    float k = ql > 8.881784197001252e-16f ? sn / ql : 1.0f;
    return Q4{cs, axis.x * k, axis.y * k, axis.z * k};
}
// local hinge rotation: Gohlke quaternion_from_euler(tz, ty, tx, 'rzyx') = qz (x) qy (x) qx
__device__ __forceinline__ Q4 q_euler_rzyx(float tz, float ty, float tx) {
    float sz, cz, sy, cy, sx, cx;
    sincosf(0.5f * tz, &sz, &cz); sincosf(0.5f * ty, &sy, &cy); sincosf(0.5f * tx, &sx, &cx);
    return qmul(qmul(Q4{cz, 0.f, 0.f, sz}, Q4{cy, 0.f, sy, 0.f}), Q4{cx, sx, 0.f, 0.f});
}
// the reference's "bquat" quirk: quaternion_from_euler(a0, a1, a2) with default 'sxyz' on (tz, ty, tx)
__device__ __forceinline__ Q4 q_euler_sxyz(float ai, float aj, float ak) {
    float si, ci, sj, cj, sk, ck;
    sincosf(0.5f * ai, &si, &ci); sincosf(0.5f * aj, &sj, &cj); sincosf(0.5f * ak, &sk, &ck);
    float cc = ci * ck, cs = ci * sk, sc = si * ck, ss = si * sk;
    return Q4{cj * cc + sj * ss, cj * sc - sj * cs, cj * ss + sj * cc, cj * cs - sj * sc};
}

}  // namespace kp
