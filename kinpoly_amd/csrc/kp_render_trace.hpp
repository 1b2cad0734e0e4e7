// kp_render_trace.hpp -- the one copy of the renderers' intersection code: the per-row set-up of a body and of an object geom in LDS, the hit loop over
// floor, hulls, boxes and cylinders, and the colour of a hit.  Included by kp_render.hip (k_render) and kp_render_ego.hip (k_render_ego); what one
// pixel is: kp_render.hpp.  Everything is __forceinline__, so each kernel carries its own inlined code and neither translation unit moves the other.
#pragma once
#include <cmath>

#include "kp_device.hpp"
#include "kp_render.hpp"

namespace kp {

constexpr int RK_OBJECT = 4, RK_FLOOR = 5, RK_SKY = 7;      // rows of the colour table (floor: 5 + parity)
constexpr int RD_BODY_LDS = RD_MAXFIG * D_NB * 16;          // per body: R^T [9], camera in the body frame [3], body origin - camera [3], culling radius^2
constexpr int RD_GEOM_LDS = RD_MAXGEOM * 16;                // per object geom: type (-1: not there), size [3], R^T [9], camera in the geom frame [3]

struct RayHit { float best, shade; int geom, kind; };

// one half-space n.x <= d of a convex clip: den = n.dir, dist = d - n.origin
__device__ __forceinline__ void clip(float den, float dist, float& t_in, float& t_out, float& den_in) {
    const float t = dist * __builtin_amdgcn_rcpf(den);
    const bool enter = den < 0.f && t > t_in;             // selects, not branches: the lanes of a tile disagree on every plane
    t_in = enter ? t : t_in;
    den_in = enter ? den : den_in;
    t_out = den > 0.f ? fminf(t_out, t) : (den == 0.f && dist < 0.f) ? -INFINITY : t_out;
}

__device__ __forceinline__ V3 mulmat_t(const float* m, V3 v) {      // m^T v
    return V3{m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z, m[2] * v.x + m[5] * v.y + m[8] * v.z};
}

// the colour table of a row: figure 0..3, objects, floor cell 0 / 1, sky
__device__ __forceinline__ void rd_colours(float* col, const RenderStyle& st) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < RD_MAXFIG; k++) col[3 * k + i] = st.figure[k][i];
        col[3 * RK_OBJECT + i] = st.object[i];
        col[3 * RK_FLOOR + i] = st.floor[0][i];
        col[3 * (RK_FLOOR + 1) + i] = st.floor[1][i];
        col[3 * RK_SKY + i] = st.sky[i];
    }
}

// one body's 16 floats B for a camera at o: xq its world quaternion, x its origin, rb its hull's bounding radius
__device__ __forceinline__ void rd_body_setup(float* B, const float* xq, V3 x, V3 o, float rb) {
    const V3 oc = x - o;
    q2mat(Q4{xq[0], xq[1], xq[2], xq[3]}, B);
    float Rt[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rt[3 * i + j] = B[3 * j + i];
    for (int i = 0; i < 9; i++) B[i] = Rt[i];
    st3(B + 9, mulmat(Rt, o - x));
    st3(B + 12, oc);
    B[15] = rb * rb * 1.001f + 1e-5f * (1.f + dot(oc, oc));      // the cull is conservative: fp32 slack on the sphere test
}

// the world pose (Rg, pos) of object geom g [18] of a row whose object block is obj_qpos [35], placed as k_pose_contacts / k_set_objects do:
// pos = p + R(q) g_pos, R = R(q) R_g (zero quaternion: identity); false when the geom is not there (an object parked more than 50 m from the
// origin has no geoms, nor has one outside the block)
__device__ __forceinline__ bool rd_geom_pose(const float* g, const float* obj_qpos, int n_obj, float* Rg, V3& pos) {
    const int oi = (int)g[0];
    if (!(oi < n_obj && oi < 5)) return false;
    const float* pose = obj_qpos + 7 * oi;
    if (sqrtf(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]) > 50.0f) return false;
    float R[9];
    q2mat(qnormalize(Q4{pose[3], pose[4], pose[5], pose[6]}), R);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rg[3 * i + j] = R[3 * i] * g[8 + j] + R[3 * i + 1] * g[11 + j] + R[3 * i + 2] * g[14 + j];
    pos = ld3(pose) + mulmat(R, ld3(g + 5));
    return true;
}

// one object geom's 16 floats G for a camera at o (G[0] = -1: not there); obj_qpos: the row's block or null
__device__ __forceinline__ void rd_geom_setup(float* G, const float* g, const float* obj_qpos, int n_obj, V3 o) {
    G[0] = -1.f;
    float Rg[9];
    V3 pos;
    if (obj_qpos && rd_geom_pose(g, obj_qpos, n_obj, Rg, pos)) {
        G[0] = g[1]; G[1] = g[2]; G[2] = g[3]; G[3] = g[4];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) G[4 + 3 * i + j] = Rg[3 * j + i];
        st3(G + 13, mulmat_t(Rg, o - pos));
    }
}

// the nearest hit of the ray (o, d) of a lane: body / geoms = the row's LDS blocks; hide: a body of figure 0 that is not drawn, or -1
__device__ __forceinline__ RayHit rd_trace(const float* body, const float* geoms, int n_fig, const float4* planes, const int32_t* plane_adr, float zfar,
                                           V3 o, V3 d, bool valid, int hide) {
    float best = INFINITY, shade = 0.f;
    int geom = -1, kind = RK_SKY;
    if (d.z < 0.f) {
        const float t = -o.z / d.z;
        if (t > 0.f && t <= zfar) { best = t; shade = -d.z; geom = 0; kind = RK_FLOOR; }
    }
    // the figures' hulls: a per-lane bounding-sphere cull, then a wave-uniform loop over the body's planes (uniform index: the 16-byte planes come
    // in through the scalar cache), left as soon as no lane of the tile can still hit
    for (int k = 0; k < n_fig; k++)
        for (int b = 0; b < D_NB; b++) {
            if (k == 0 && b == hide) continue;
            const float* B = body + 16 * (k * D_NB + b);
            const V3 oc = ld3(B + 12);
            const float tca = dot(oc, d), oc2 = dot(oc, oc), r2 = B[15];
            const bool pass = valid && oc2 - tca * tca <= r2 && (tca > 0.f || oc2 <= r2);
            if (__ballot(pass) == 0ull) continue;
            const V3 dl = mulmat(B, d), ol = ld3(B + 9);
            float t_in = -INFINITY, t_out = INFINITY, den_in = 0.f;
            const int p1 = plane_adr[b + 1];
            for (int p = plane_adr[b]; p < p1; p++) {
                const float4 pl = planes[p];
                clip(pl.x * dl.x + pl.y * dl.y + pl.z * dl.z, pl.w - (pl.x * ol.x + pl.y * ol.y + pl.z * ol.z), t_in, t_out, den_in);
                if (__ballot(pass && t_in <= t_out) == 0ull) break;
            }
            if (pass && t_in <= t_out && t_in > 0.f && t_in < best) { best = t_in; shade = -den_in; geom = 100 * k + 1 + b; kind = k; }
        }
    for (int gi = 0; gi < RD_MAXGEOM; gi++) {
        const float* G = geoms + 16 * gi;
        const float type = G[0];
        if (type < 0.f) continue;
        const V3 dl = mulmat(G + 4, d), ol = ld3(G + 13);
        float t_in = -INFINITY, t_out = INFINITY, den_in = 0.f;
        if (type == 0.f) {                                   // 0 box, 1 cylinder: kp_sim_render refuses a model with any other object geom type
            clip(dl.x, G[1] - ol.x, t_in, t_out, den_in); clip(-dl.x, G[1] + ol.x, t_in, t_out, den_in);
            clip(dl.y, G[2] - ol.y, t_in, t_out, den_in); clip(-dl.y, G[2] + ol.y, t_in, t_out, den_in);
            clip(dl.z, G[3] - ol.z, t_in, t_out, den_in); clip(-dl.z, G[3] + ol.z, t_in, t_out, den_in);
        } else {
            clip(dl.z, G[2] - ol.z, t_in, t_out, den_in); clip(-dl.z, G[2] + ol.z, t_in, t_out, den_in);
            const float a = dl.x * dl.x + dl.y * dl.y, hb = ol.x * dl.x + ol.y * dl.y, c = ol.x * ol.x + ol.y * ol.y - G[1] * G[1];
            if (a > 0.f) {
                const float disc = hb * hb - a * c;
                if (disc < 0.f) t_out = -INFINITY;
                else {
                    const float sq = sqrtf(disc), ia = __builtin_amdgcn_rcpf(a), t0 = (-hb - sq) * ia;
                    t_out = fminf(t_out, (-hb + sq) * ia);
                    if (t0 > t_in) { t_in = t0; den_in = ((ol.x + t0 * dl.x) * dl.x + (ol.y + t0 * dl.y) * dl.y) / G[1]; }
                }
            } else if (c > 0.f) t_out = -INFINITY;
        }
        if (valid && t_in <= t_out && t_in > 0.f && t_in < best) { best = t_in; shade = -den_in; geom = 25 + gi; kind = RK_OBJECT; }
    }
    return RayHit{best, shade, geom, kind};
}

// the stored colour of a hit (kind already carries the floor cell's parity): base x (0.35 + 0.65 max(0, shade)), rounded to nearest; alpha 255
__device__ __forceinline__ unsigned rd_rgba(const float* col, RayHit h) {
    const float lvl = h.geom < 0 ? 1.f : 0.35f + 0.65f * fmaxf(0.f, h.shade);
    const float* c = col + 3 * h.kind;
    unsigned w = 255u << 24;
    for (int i = 0; i < 3; i++) w |= (unsigned)__float2int_rn(255.f * fminf(fmaxf(c[i] * lvl, 0.f), 1.f)) << (8 * i);
    return w;
}

}  // namespace kp
