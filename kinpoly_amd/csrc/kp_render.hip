// kp_render.hip -- k_render, the batched ray-caster declared in kp_render.hpp (what one pixel is: see there), and the host-side face-plane builder.
#include "kp_render.hpp"

#include <cmath>

#include "kp_device.hpp"
#include "kp_render_trace.hpp"

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
    float body[RD_BODY_LDS];                     // per body and per object geom: see kp_render_trace.hpp
    float geom[RD_GEOM_LDS];
};

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
        rd_colours(s.col, A.style);
    }
    __syncthreads();
    const V3 o = ld3(s.cam);
    const int nb = A.n_fig * D_NB;
    if (tid < nb) {
        const size_t fig = (size_t)row * A.n_fig + tid / D_NB;
        const int b = tid % D_NB;
        rd_body_setup(s.body + 16 * tid, A.xquat + fig * 96 + 4 * b, ld3(A.xpos + fig * 72 + 3 * b), o, A.rbound[b]);
    } else if (tid >= 128 && tid < 128 + RD_MAXGEOM) {
        const int gi = tid - 128;
        rd_geom_setup(s.geom + 16 * gi, A.og + 18 * gi, A.obj_qpos && gi < A.n_og ? A.obj_qpos + (size_t)row * 35 : nullptr, A.n_obj, o);
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

    RayHit h = rd_trace(s.body, s.geom, A.n_fig, A.planes, A.plane_adr, A.style.zfar, o, d, valid, -1);
    if (!valid) return;
    if (h.kind == RK_FLOOR) h.kind += ((int)floorf(o.x + h.best * d.x) + (int)floorf(o.y + h.best * d.y)) & 1;
    const size_t at = ((size_t)row * A.height + py) * A.width + px;
    if (A.geom) A.geom[at] = h.geom;
    if (A.depth) A.depth[at] = h.best;
    if (A.rgba) A.rgba[at] = rd_rgba(s.col, h);
}

hipError_t launch_render(RenderArgs A, hipStream_t stream) {
    A.tiles_x = (A.width + 7) / 8;
    A.tiles = A.tiles_x * ((A.height + 7) / 8);
    A.blocks_per_row = (A.tiles + RD_TILES - 1) / RD_TILES;
    hipLaunchKernelGGL(k_render, dim3((unsigned)(A.n_rows * A.blocks_per_row)), dim3(64 * RD_TILES), 0, stream, A);
    return hipGetLastError();
}

}  // namespace kp
