// kp_render_ego.hip -- k_render_ego and k_flow_cells, the egocentric renderer declared in kp_render_ego.hpp (what one pixel is: see there).
#include "kp_render_ego.hpp"

#include <cmath>

#include "kp_device.hpp"
#include "kp_render_trace.hpp"

namespace kp {

constexpr int EGO_NENT = RD_MAXFIG * D_NB + RD_MAXGEOM;      // entities that move: the bodies of every figure, then the object geoms

struct __attribute__((aligned(16))) EgoLds {
    float cam[12];                               // camera A: eye, forward, right tan(fovy / 2) W / H, up tan(fovy / 2)
    float col[8 * 3];                            // base colours, as k_render
    float body[RD_BODY_LDS];                     // per body and per object geom, for camera A: see kp_render_trace.hpp
    float geom[RD_GEOM_LDS];
    float camb[13];                              // camera B: eye, right, up, forward, focal length in pixels H / (2 tan(fovy_B / 2))
    float mot[EGO_NENT * 12];                    // per entity: R_B R_A^T [9], x_B - R_B R_A^T x_A [3]
    float live_b[RD_MAXGEOM];                    // 1: the geom is there in frame B
};

// eye, forward, right, up of a pose-camera row [8]; returns tan(fovy / 2)
__device__ __forceinline__ float pose_camera(const float* c, V3& f, V3& r, V3& u) {
    float R[9];
    q2mat(qnormalize(Q4{c[3], c[4], c[5], c[6]}), R);
    f = v3(R[2], R[5], R[8]);
    u = v3(R[1], R[4], R[7]);
    r = v3(-R[0], -R[3], -R[6]);
    return tanf(0.5f * c[7] * 0.017453292519943295f);
}

// (R_B R_A^T, x_B - R_B R_A^T x_A) of an entity whose world pose is (Ra, xa) in frame A and (Rb, xb) in frame B
__device__ __forceinline__ void rigid_motion(float* M, const float* Ra, V3 xa, const float* Rb, V3 xb) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
    st3(M + 9, xb - mulmat(M, xa));
}

// v + (v of the lane the DPP control names); every lane of the wavefront is active where this is called
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// the sum of v over the 64 lanes, the same bits in every lane: a butterfly inside each row of 16 lanes (quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror: after each stage both partners hold the same sum), then the four rows added in row order
__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add<0xB1>(v);
    v = dpp_add<0x4E>(v);
    v = dpp_add<0x141>(v);
    v = dpp_add<0x140>(v);
    const int w = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(w, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(w, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(w, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(w, 48));
    return ((r0 + r1) + r2) + r3;
}

// grid = n_rows * blocks_per_row workgroups of RD_TILES wavefronts; a wavefront owns one 8 x 8 pixel tile of its workgroup's row
__global__ __launch_bounds__(64 * RD_TILES) void k_render_ego(RenderEgoArgs A) {
    __shared__ EgoLds s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = blockIdx.x / A.blocks_per_row, blk = blockIdx.x - row * A.blocks_per_row;
    const bool pair = A.camera_b != nullptr;
    if (tid == 0) {
        V3 f, r, u;
        const float* c = A.camera + 8 * (A.cam_rows > 1 ? row : 0);
        const float th = pose_camera(c, f, r, u);
        st3(s.cam, ld3(c));
        st3(s.cam + 3, f);
        st3(s.cam + 6, (th * (float)A.width / (float)A.height) * r);
        st3(s.cam + 9, th * u);
        rd_colours(s.col, A.style);
        if (pair) {
            const float* cb = A.camera_b + 8 * (A.cam_rows > 1 ? row : 0);
            const float thb = pose_camera(cb, f, r, u);
            st3(s.camb, ld3(cb));
            st3(s.camb + 3, r);
            st3(s.camb + 6, u);
            st3(s.camb + 9, f);
            s.camb[12] = 0.5f * (float)A.height / thb;
        }
    }
    __syncthreads();
    const V3 o = ld3(s.cam);
    const int nb = A.n_fig * D_NB;
    if (tid < nb) {
        const size_t fig = (size_t)row * A.n_fig + tid / D_NB;
        const int b = tid % D_NB;
        const float* xq = A.xquat + fig * 96 + 4 * b;
        const V3 x = ld3(A.xpos + fig * 72 + 3 * b);
        rd_body_setup(s.body + 16 * tid, xq, x, o, A.rbound[b]);
        if (pair) {
            const float* xqb = A.xquat_b + fig * 96 + 4 * b;
            float Ra[9], Rb[9];
            q2mat(qnormalize(Q4{xq[0], xq[1], xq[2], xq[3]}), Ra);      // normalised here: identical frames must give R_B R_A^T = 1
            q2mat(qnormalize(Q4{xqb[0], xqb[1], xqb[2], xqb[3]}), Rb);
            rigid_motion(s.mot + 12 * tid, Ra, x, Rb, ld3(A.xpos_b + fig * 72 + 3 * b));
        }
    } else if (tid >= 128 && tid < 128 + RD_MAXGEOM) {
        const int gi = tid - 128;
        const bool there = A.obj_qpos && gi < A.n_og;
        rd_geom_setup(s.geom + 16 * gi, A.og + 18 * gi, there ? A.obj_qpos + (size_t)row * 35 : nullptr, A.n_obj, o);
        if (pair) {
            float Ra[9], Rb[9];
            V3 xa, xb;
            bool live = false;
            if (there && A.obj_qpos_b && rd_geom_pose(A.og + 18 * gi, A.obj_qpos + (size_t)row * 35, A.n_obj, Ra, xa) &&
                rd_geom_pose(A.og + 18 * gi, A.obj_qpos_b + (size_t)row * 35, A.n_obj, Rb, xb)) {
                rigid_motion(s.mot + 12 * (RD_MAXFIG * D_NB + gi), Ra, xa, Rb, xb);
                live = true;
            }
            s.live_b[gi] = live ? 1.f : 0.f;
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

    RayHit h = rd_trace(s.body, s.geom, A.n_fig, A.planes, A.plane_adr, A.style.zfar, o, d, valid, A.hide_body);

    // the pair: carry the hit point to frame B with the motion of what was hit, project it through camera B
    float fu = 0.f, fv = 0.f;
    bool okp = false;
    if (pair) {
        V3 v = d;
        bool live = true;
        if (h.kind != RK_SKY) {
            V3 p = o + h.best * d;
            if (h.kind != RK_FLOOR) {
                const int e = h.kind == RK_OBJECT ? RD_MAXFIG * D_NB + (h.geom - 25) : h.kind * D_NB + (h.geom - 100 * h.kind - 1);
                const float* M = s.mot + 12 * e;
                p = mulmat(M, p) + ld3(M + 9);
                if (h.kind == RK_OBJECT) live = s.live_b[h.geom - 25] != 0.f;
            }
            v = p - ld3(s.camb);
        }
        const float cz = dot(ld3(s.camb + 9), v);
        okp = valid && live && cz > EGO_MIN_Z;
        if (okp) {
            const float k = s.camb[12] * __builtin_amdgcn_rcpf(cz);
            fu = (0.5f * (float)A.width - ((float)px + 0.5f)) + k * dot(ld3(s.camb + 3), v);
            fv = (0.5f * (float)A.height - ((float)py + 0.5f)) - k * dot(ld3(s.camb + 6), v);
        }
    }
    if (valid) {
        if (h.kind == RK_FLOOR) h.kind += ((int)floorf(o.x + h.best * d.x) + (int)floorf(o.y + h.best * d.y)) & 1;
        const size_t at = ((size_t)row * A.height + py) * A.width + px;
        if (A.geom) A.geom[at] = h.geom;
        if (A.depth) A.depth[at] = h.best;
        if (A.rgba) A.rgba[at] = rd_rgba(s.col, h);
        if (A.flow) { A.flow[2 * at] = fu; A.flow[2 * at + 1] = fv; }
        if (A.ok) A.ok[at] = okp ? 1 : 0;
    }
    if (A.partial) {                             // wave-uniform; the lanes have converged again: the sums below are taken over all 64
        const float su = wave_sum(fu), sv = wave_sum(fv), cnt = wave_sum(okp ? 1.f : 0.f);
        if (lane == 0) {
            float* P = A.partial + 3 * ((size_t)row * A.tiles + tile);
            P[0] = su; P[1] = sv; P[2] = cnt;
        }
    }
}

// one thread per cell: the a x b partials of the cell added row by row, then the mean
__global__ __launch_bounds__(256) void k_flow_cells(int n_cells, int grid_x, int grid_y, int tiles_x, int tiles, const float* partial, float* cells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    const int per = grid_x * grid_y, row = i / per, c = i - row * per, cy = c / grid_x, cx = c - cy * grid_x;
    const int a = tiles_x / grid_x, b = (tiles / tiles_x) / grid_y;
    float su = 0.f, sv = 0.f, cnt = 0.f;
    for (int j = 0; j < b; j++)
        for (int k = 0; k < a; k++) {
            const float* P = partial + 3 * ((size_t)row * tiles + (size_t)(cy * b + j) * tiles_x + cx * a + k);
            su += P[0]; sv += P[1]; cnt += P[2];
        }
    cells[2 * (size_t)i] = cnt > 0.f ? su / cnt : 0.f;
    cells[2 * (size_t)i + 1] = cnt > 0.f ? sv / cnt : 0.f;
}

hipError_t launch_render_ego(RenderEgoArgs A, hipStream_t stream) {
    A.tiles_x = (A.width + 7) / 8;
    A.tiles = A.tiles_x * ((A.height + 7) / 8);
    A.blocks_per_row = (A.tiles + RD_TILES - 1) / RD_TILES;
    if (!A.cells) A.partial = nullptr;
    hipLaunchKernelGGL(k_render_ego, dim3((unsigned)(A.n_rows * A.blocks_per_row)), dim3(64 * RD_TILES), 0, stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !A.cells) return e;
    const int n_cells = A.n_rows * A.grid_x * A.grid_y;
    hipLaunchKernelGGL(k_flow_cells, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, stream, n_cells, A.grid_x, A.grid_y, A.tiles_x, A.tiles, A.partial, A.cells);
    return hipGetLastError();
}

}  // namespace kp
