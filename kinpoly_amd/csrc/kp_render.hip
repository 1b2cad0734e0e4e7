// kp_render.hip -- k_render, the batched ray-caster declared in kp_render.hpp (what one pixel is: see there), and the host-side face-plane builder.
#include "kp_render.hpp"

#include <cmath>

#include "kp_device.hpp"

namespace kp {

// ------------------------------------------------------------------ host: face planes of the hulls
// Every vertex triple's plane is kept when all of the hull's vertices lie on one side of it (within 1e-9), oriented outward (n.x <= d inside) and
// merged with a plane already kept whose four components agree within 1e-7.  64 vertices are 41 664 triples: instant.
int hull_planes(const HostModel& m, std::vector<float>& planes4, std::vector<int32_t>& adr) {
    planes4.clear();
    adr.assign(m.nb + 1, 0);
    std::vector<double> kept;
    for (int b = 0; b < m.nb; b++) {
        const double* V = m.verts.data() + 3 * m.vert_adr[b];
        const int nv = m.vert_adr[b + 1] - m.vert_adr[b];
        kept.clear();
        for (int i = 0; i < nv; i++)
            for (int j = i + 1; j < nv; j++)
                for (int k = j + 1; k < nv; k++) {
                    const double *a = V + 3 * i, *p = V + 3 * j, *q = V + 3 * k;
                    const double e1[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]}, e2[3] = {q[0] - a[0], q[1] - a[1], q[2] - a[2]};
                    double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                    const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                    if (!(len > 1e-14)) continue;
                    n[0] /= len; n[1] /= len; n[2] /= len;
                    double d = n[0] * a[0] + n[1] * a[1] + n[2] * a[2], lo = 0.0, hi = 0.0;
                    for (int v = 0; v < nv; v++) {
                        const double sd = n[0] * V[3 * v] + n[1] * V[3 * v + 1] + n[2] * V[3 * v + 2] - d;
                        lo = std::min(lo, sd); hi = std::max(hi, sd);
                    }
                    if (hi > 1e-9 && lo < -1e-9) continue;
                    if (hi > 1e-9) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; d = -d; }
                    bool dup = false;
                    for (size_t c = 0; c < kept.size() && !dup; c += 4)
                        dup = std::fabs(kept[c] - n[0]) <= 1e-7 && std::fabs(kept[c + 1] - n[1]) <= 1e-7 && std::fabs(kept[c + 2] - n[2]) <= 1e-7 && std::fabs(kept[c + 3] - d) <= 1e-7;
                    if (!dup) kept.insert(kept.end(), {n[0], n[1], n[2], d});
                }
        for (double x : kept) planes4.push_back((float)x);
        adr[b + 1] = (int32_t)(planes4.size() / 4);
    }
    return (int)(planes4.size() / 4);
}

// ------------------------------------------------------------------ device
struct __attribute__((aligned(16))) RenderLds {
    float cam[12];                               // position, forward, right tan(fovy / 2) W / H, up tan(fovy / 2)
    float col[8 * 3];                            // base colours: figure 0..3, objects, floor cell 0 / 1, sky
    float body[RD_MAXFIG * D_NB * 16];           // per body: R^T [9], camera in the body frame [3], body origin - camera [3], culling radius^2
    float geom[RD_MAXGEOM * 16];                 // per object geom: type (-1: not there), size [3], R^T [9], camera in the geom frame [3]
};

constexpr int RK_OBJECT = 4, RK_FLOOR = 5, RK_SKY = 7;      // rows of RenderLds::col (floor: 5 + parity)

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

// grid = n_rows * blocks_per_row workgroups of RD_TILES wavefronts; a wavefront owns one 8 x 8 pixel tile of its workgroup's row
__global__ __launch_bounds__(64 * RD_TILES) void k_render(RenderArgs A) {
    __shared__ RenderLds s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = blockIdx.x / A.blocks_per_row, blk = blockIdx.x - row * A.blocks_per_row;
    if (tid == 0) {
        const float* c = A.camera + 7 * (A.cam_rows > 1 ? row : 0);
        const float rad = 0.017453292519943295f;
        const float ca = cosf(c[4] * rad), sa = sinf(c[4] * rad), ce = cosf(c[5] * rad), se = sinf(c[5] * rad), th = tanf(0.5f * c[6] * rad);
        const V3 f = v3(ce * ca, ce * sa, se), r = v3(sa, -ca, 0.f), u = cross(r, f);      // normalize(f x z) = (sin az, -cos az, 0)
        st3(s.cam, ld3(c) - c[3] * f);
        st3(s.cam + 3, f);
        st3(s.cam + 6, (th * (float)A.width / (float)A.height) * r);
        st3(s.cam + 9, th * u);
        const RenderStyle& st = A.style;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int k = 0; k < RD_MAXFIG; k++) s.col[3 * k + i] = st.figure[k][i];
            s.col[3 * RK_OBJECT + i] = st.object[i];
            s.col[3 * RK_FLOOR + i] = st.floor[0][i];
            s.col[3 * (RK_FLOOR + 1) + i] = st.floor[1][i];
            s.col[3 * RK_SKY + i] = st.sky[i];
        }
    }
    __syncthreads();
    const V3 o = ld3(s.cam);
    const int nb = A.n_fig * D_NB;
    if (tid < nb) {
        const size_t fig = (size_t)row * A.n_fig + tid / D_NB;
        const int b = tid % D_NB;
        const float* xq = A.xquat + fig * 96 + 4 * b;
        const V3 x = ld3(A.xpos + fig * 72 + 3 * b), oc = x - o;
        float* B = s.body + 16 * tid;
        q2mat(Q4{xq[0], xq[1], xq[2], xq[3]}, B);
        float Rt[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rt[3 * i + j] = B[3 * j + i];
        for (int i = 0; i < 9; i++) B[i] = Rt[i];
        st3(B + 9, mulmat(Rt, o - x));
        st3(B + 12, oc);
        const float rb = A.rbound[b];
        B[15] = rb * rb * 1.001f + 1e-5f * (1.f + dot(oc, oc));      // the cull is conservative: fp32 slack on the sphere test
    } else if (tid >= 128 && tid < 128 + RD_MAXGEOM) {
        // the row's object geoms, placed as k_pose_contacts / k_set_objects do: pos = p + R(q) g_pos, R = R(q) R_g (zero quaternion: identity);
        // an object parked more than 50 m from the origin has no geoms
        const int gi = tid - 128;
        float* G = s.geom + 16 * gi;
        G[0] = -1.f;
        if (A.obj_qpos && gi < A.n_og) {
            const float* g = A.og + 18 * gi;
            const int oi = (int)g[0];
            if (oi < A.n_obj && oi < 5) {
                const float* pose = A.obj_qpos + (size_t)row * 35 + 7 * oi;
                if (!(sqrtf(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]) > 50.0f)) {
                    float R[9], Rg[9];
                    q2mat(qnormalize(Q4{pose[3], pose[4], pose[5], pose[6]}), R);
                    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rg[3 * i + j] = R[3 * i] * g[8 + j] + R[3 * i + 1] * g[11 + j] + R[3 * i + 2] * g[14 + j];
                    const V3 pos = ld3(pose) + mulmat(R, ld3(g + 5));
                    G[0] = g[1]; G[1] = g[2]; G[2] = g[3]; G[3] = g[4];
                    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) G[4 + 3 * i + j] = Rg[3 * j + i];
                    st3(G + 13, mulmat_t(Rg, o - pos));
                }
            }
        }
    }
    __syncthreads();
    const int tile = blk * RD_TILES + __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tile >= A.tiles) return;
    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    const int px = 8 * tx + (lane & 7), py = 8 * ty + (lane >> 3);
    const bool valid = px < A.width && py < A.height;
    const float sx = (float)(2 * px + 1 - A.width) / (float)A.width, sy = (float)(A.height - 2 * py - 1) / (float)A.height;
    V3 d = ld3(s.cam + 3) + sx * ld3(s.cam + 6) + sy * ld3(s.cam + 9);
    d = (1.0f / sqrtf(dot(d, d))) * d;

    float best = INFINITY, shade = 0.f;
    int geom = -1, kind = RK_SKY;
    if (d.z < 0.f) {
        const float t = -o.z / d.z;
        if (t > 0.f && t <= A.style.zfar) { best = t; shade = -d.z; geom = 0; kind = RK_FLOOR; }
    }
    // the figures' hulls: a per-lane bounding-sphere cull, then a wave-uniform loop over the body's planes (uniform index: the 16-byte planes come
    // in through the scalar cache), left as soon as no lane of the tile can still hit
    for (int k = 0; k < A.n_fig; k++)
        for (int b = 0; b < D_NB; b++) {
            const float* B = s.body + 16 * (k * D_NB + b);
            const V3 oc = ld3(B + 12);
            const float tca = dot(oc, d), oc2 = dot(oc, oc), r2 = B[15];
            const bool pass = valid && oc2 - tca * tca <= r2 && (tca > 0.f || oc2 <= r2);
            if (__ballot(pass) == 0ull) continue;
            const V3 dl = mulmat(B, d), ol = ld3(B + 9);
            float t_in = -INFINITY, t_out = INFINITY, den_in = 0.f;
            const int p1 = A.plane_adr[b + 1];
            for (int p = A.plane_adr[b]; p < p1; p++) {
                const float4 pl = A.planes[p];
                clip(pl.x * dl.x + pl.y * dl.y + pl.z * dl.z, pl.w - (pl.x * ol.x + pl.y * ol.y + pl.z * ol.z), t_in, t_out, den_in);
                if (__ballot(pass && t_in <= t_out) == 0ull) break;
            }
            if (pass && t_in <= t_out && t_in > 0.f && t_in < best) { best = t_in; shade = -den_in; geom = 100 * k + 1 + b; kind = k; }
        }
    for (int gi = 0; gi < RD_MAXGEOM; gi++) {
        const float* G = s.geom + 16 * gi;
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
    if (!valid) return;
    if (kind == RK_FLOOR) kind += ((int)floorf(o.x + best * d.x) + (int)floorf(o.y + best * d.y)) & 1;
    const size_t at = ((size_t)row * A.height + py) * A.width + px;
    if (A.geom) A.geom[at] = geom;
    if (A.depth) A.depth[at] = best;
    if (A.rgba) {
        const float lvl = geom < 0 ? 1.f : 0.35f + 0.65f * fmaxf(0.f, shade);
        const float* c = s.col + 3 * kind;
        unsigned w = 255u << 24;
        for (int i = 0; i < 3; i++) w |= (unsigned)__float2int_rn(255.f * fminf(fmaxf(c[i] * lvl, 0.f), 1.f)) << (8 * i);
        A.rgba[at] = w;
    }
}

hipError_t launch_render(RenderArgs A, hipStream_t stream) {
    A.tiles_x = (A.width + 7) / 8;
    A.tiles = A.tiles_x * ((A.height + 7) / 8);
    A.blocks_per_row = (A.tiles + RD_TILES - 1) / RD_TILES;
    hipLaunchKernelGGL(k_render, dim3((unsigned)(A.n_rows * A.blocks_per_row)), dim3(64 * RD_TILES), 0, stream, A);
    return hipGetLastError();
}

}  // namespace kp
