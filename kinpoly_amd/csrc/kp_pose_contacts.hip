// kp_pose_contacts.hip -- k_pose_contacts, the batched pose-contact query declared in kp_pose_contacts.hpp (see there).
// Narrow phases: kp_collide.hpp; the culls and the floor rule are those of collide<> (kp_step_collide.hpp).
#include "kp_pose_contacts.hpp"
#include "kp_collide.hpp"

namespace kp {

struct __attribute__((aligned(16))) PoseLds {
    double pm[30];                    // MPR witnesses (convex_pair)
    float geom[PC_MAXGEOM * 17];      // world-frame object geoms of the row: type, size[3], pos[3], mat[9], (unused)
    float hrec[16];                   // hull record of the support functor (hull_support_store)
};

// Twin of the floor branch of collide<> (kp_step_collide.hpp), kept as a separate copy so that the step kernels' code is untouched: mjc_PlaneConvex
// on hull b, whose world vertices xw sit on the lanes below the hull's vertex count (z = 3e38 on the others).  The deepest vertex (first on ties)
// makes the first contact; then its hull-graph neighbours in graph order, up to maxplanemesh contacts in all, each within the margin and not
// closer than tolplanemesh * rbound to the first contact's position.  Adds the contacts to ncon and their penetration to pen (wave-uniform).
__device__ __forceinline__ void pose_floor(const DevTables& T, const Params& P, int b, int vadr, V3 xw, float pen_margin, int tid, int& ncon, float& pen) {
    const float dmin = wave_min(xw.z);
    if (dmin > P.margin) return;
    const int idx = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(xw.z == dmin)) - 1);
    const int n0 = T.vert_nbr_adr[vadr + idx], n1 = T.vert_nbr_adr[vadr + idx + 1];
    const int deg = n1 - n0;
    const int j = tid < deg ? (int)T.vert_nbr[n0 + tid] : 0;
    const V3 xj = v3(__shfl(xw.x, j, 64), __shfl(xw.y, j, 64), __shfl(xw.z, j, 64));
    const V3 x0 = v3(bcast_lane(xw.x, idx), bcast_lane(xw.y, idx), bcast_lane(xw.z, idx));
    const V3 dj = xj - v3(x0.x, x0.y, x0.z - 0.5f * x0.z);
    const float tolr = P.pm_tol * T.mesh_rbound[b];
    const bool ok = tid < deg && !(xj.z > P.margin) && !(dot(dj, dj) < tolr * tolr);
    const unsigned long long m = __ballot(ok);
    const int rank = __popcll(m & ((1ull << tid) - 1ull));
    const int extra = P.pm_max - 1;
    ncon += 1 + min(__popcll(m), extra);
    pen += fmaxf(0.f, -dmin - pen_margin) + wave_sum(ok && rank < extra ? fmaxf(0.f, -xj.z - pen_margin) : 0.f);
}

// collide<>'s third cull before the MPR query: every vertex of the hull (lanes with has) lies beyond one face plane of the box -- or beyond a
// cap plane / the tangent plane facing the body origin xb of the cylinder -- by more than the margin (+ 0.1 mm of slack for the fp32 test).
__device__ __forceinline__ bool pose_separated(const float* g, V3 xw, V3 xb, bool has, float margin) {
    const float* Rg = g + 7;
    const V3 dv = xw - ld3(g + 4);
    const float px = Rg[0] * dv.x + Rg[3] * dv.y + Rg[6] * dv.z, py = Rg[1] * dv.x + Rg[4] * dv.y + Rg[7] * dv.z, pz = Rg[2] * dv.x + Rg[5] * dv.y + Rg[8] * dv.z;
    const float lim = margin + 1e-4f;
    if (g[0] == 0.f) {
        const float hx = g[1] + lim, hy = g[2] + lim, hz = g[3] + lim;
        return __ballot(has && !(px > hx)) == 0ull || __ballot(has && !(px < -hx)) == 0ull || __ballot(has && !(py > hy)) == 0ull ||
               __ballot(has && !(py < -hy)) == 0ull || __ballot(has && !(pz > hz)) == 0ull || __ballot(has && !(pz < -hz)) == 0ull;
    }
    const float hz = g[2] + lim;
    if (__ballot(has && !(pz > hz)) == 0ull || __ballot(has && !(pz < -hz)) == 0ull) return true;
    const V3 cb = xb - ld3(g + 4);
    const float ux = Rg[0] * cb.x + Rg[3] * cb.y + Rg[6] * cb.z, uy = Rg[1] * cb.x + Rg[4] * cb.y + Rg[7] * cb.z;
    const float un = sqrtf(ux * ux + uy * uy);
    return un > 1e-6f && __ballot(has && !((px * ux + py * uy) > (g[1] + lim) * un)) == 0ull;
}

// grid = n_rows workgroups of one wavefront
__global__ __launch_bounds__(64) void k_pose_contacts(PoseContactArgs A) {
    __shared__ PoseLds s;
    const int row = blockIdx.x, tid = threadIdx.x;
    const DevTables& T = A.T;
    const Params& P = A.P;
    // the row's object geoms, lane = model geom, placed as k_set_objects does: pos = p + R(q) g_pos, R = R(q) R_g (zero quaternion: identity);
    // an object parked more than 50 m from the origin has no geoms
    bool live = false;
    if (A.obj_qpos && tid < A.n_og) {
        const float* g = A.og + 18 * tid;
        const int oi = (int)g[0];
        if (oi < A.n_obj && oi < 5) {
            const float* pose = A.obj_qpos + (size_t)row * 35 + 7 * oi;
            if (!(sqrtf(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]) > 50.0f)) {
                float R[9], Rg[9];
                q2mat(qnormalize(Q4{pose[3], pose[4], pose[5], pose[6]}), R);
                for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rg[3 * i + j] = R[3 * i] * g[8 + j] + R[3 * i + 1] * g[11 + j] + R[3 * i + 2] * g[14 + j];
                const V3 p = mulmat(R, ld3(g + 5));
                float* o = s.geom + 17 * tid;
                o[0] = g[1]; o[1] = g[2]; o[2] = g[3]; o[3] = g[4];
                o[4] = pose[0] + p.x; o[5] = pose[1] + p.y; o[6] = pose[2] + p.z;
                for (int k = 0; k < 9; k++) o[7 + k] = Rg[k];
                o[16] = 0.f;
                live = true;
            }
        }
    }
    const unsigned gmask = (unsigned)__ballot(live);
    __syncthreads();
    const float* xp = A.xpos + (size_t)row * 72;
    const float* xq = A.xquat + (size_t)row * 96;
    // mid phase, lane = hull body: bit 0 = floor, bit 1 + g = object geom g (bounding spheres, then the signed-distance cull of collide<>)
    unsigned mybits = 0;
    if (tid < D_NB) {
        const V3 xb = ld3(xp + 3 * tid);
        const float rb = T.body_rbound[tid];
        if (!(xb.z - rb > P.margin)) mybits = 1u;
        for (unsigned gm = gmask; gm; gm &= gm - 1u) {
            const int gi = __ffs((int)gm) - 1;
            const float* g = s.geom + 17 * gi;
            const V3 dx = xb - ld3(g + 4);
            if (sqrtf(dot(dx, dx)) - rb - geom_rbound(g) > P.margin) continue;
            if (geom_sdf(g, xb) - rb > P.margin + 1e-4f) continue;
            mybits |= 2u << gi;
        }
    }
    int ncon = 0;
    float pen = 0.f;
    unsigned myhits = 0;                                   // lane g: bit b = hull b touches object geom g
    unsigned long long bodies = __ballot(mybits != 0u);
    while (bodies) {
        const int b = __ffsll((long long)bodies) - 1;
        bodies &= bodies - 1ull;
        unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)mybits, b);
        const int vadr = T.vert_adr[b], nvb = T.vert_adr[b + 1] - vadr;
        const V3 xb = ld3(xp + 3 * b);
        float R[9];
        q2mat(Q4{xq[4 * b], xq[4 * b + 1], xq[4 * b + 2], xq[4 * b + 3]}, R);
        V3 v = v3(0.f, 0.f, 0.f), xw = v3(0.f, 0.f, 3.0e38f);
        if (tid < nvb) { v = ld3(T.verts + 3 * (vadr + tid)); xw = xb + mulmat(R, v); }
        while (bits) {
            const int gi = __ffs((int)bits) - 2;           // -1 = floor
            bits &= bits - 1u;
            if (gi < 0) { pose_floor(T, P, b, vadr, xw, A.pen_margin, tid, ncon, pen); continue; }
            const float* g = s.geom + 17 * gi;
            if (pose_separated(g, xw, xb, tid < nvb, P.margin)) continue;
            // mjc_Convex: geom 1 = the box / cylinder, geom 2 = the hull (centre = the body's COM)
            const GeomSupport ga(g);
            hull_support_store(s.hrec, xb, xb + mulmat(R, ld3(T.body_ipos + 3 * b)), R);
            const HullSupport hb(s.hrec, v, tid < nvb);
            Contact c;
            if (convex_pair(ga, hb, P.margin, c, s.pm)) {
                ncon++;
                pen += fmaxf(0.f, -c.dist - A.pen_margin);
                if (tid == gi) myhits |= 1u << b;
            }
        }
    }
    if (tid == 0) { A.pen[row] = pen; A.ncon[row] = ncon; }
    if (tid < A.n_og) A.hits[(size_t)row * A.n_og + tid] = myhits;
}

hipError_t launch_pose_contacts(const PoseContactArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(k_pose_contacts, dim3(A.n_rows), dim3(64), 0, stream, A);
    return hipGetLastError();
}

}  // namespace kp
