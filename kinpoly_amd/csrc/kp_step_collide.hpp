// kp_step_collide.hpp -- the collision pass of the control step (put_contact, mpr_scratch, collide); narrow phases: kp_collide.hpp.  Part of kp_step_device.hpp.
#pragma once
#include "kp_collide.hpp"
#include "kp_step_args.hpp"

namespace kp {

// ---------------------------------------------------------------- collision (first wavefront)

// one lane appends a contact: vertex-side entity A (0..23 hull, 24 + k object slot), surface-side entity B (-1 world / static geom),
// normal pointing from B's geom into A's
template <bool OBJ, class SL>
// B: entity carrying the surface (-1 floor, -2 - g static geom g, 24 + k object slot k); its invweight0 is looked up by make_constraint
__device__ __forceinline__ void put_contact(SL& s, int c, V3 pos, float dist, V3 nrm, int A, int B) {
    st3(s.con_pos + 3 * c, pos);
    s.con_D[c] = dist; s.con_body[c] = (unsigned char)A;          // con_D holds the distance until make_constraint
    if constexpr (OBJ) {
        EnvLdsObj& so = as_obj(s);
        st3(so.con_n + 3 * c, nrm); so.con_b2[c] = (signed char)B;
    }
}

// LDS scratch of the MPR query (witnesses of the portal vertices, 30 doubles) inside s.U, which is free outside the ABA passes:
// U[0, 96) box-box polygon, U[96, 152) contact records of a pair, U[160, 220) this, U[232, 247) hull record of the support functor
template <class SL>
__device__ __forceinline__ double* mpr_scratch(SL& s) {
    static_assert(offsetof(SL, U) % 8 == 0, "s.U must be 8-byte aligned for the fp64 MPR scratch");
    return reinterpret_cast<double*>(s.U + 160);
}

// mj_collision of the scene.  Mid phase in parallel: lane = hull body (then lane = object geom) tests all its targets (bit 0 = floor,
// bit j = geom j - 1) with bounding spheres; the serial part visits only the pairs that passed, in the oracle's order (entity-major,
// floor first), so contact indices and the con_start[] grouping are the oracle's.  Narrow phases: kp_collide.hpp.
template <int NT, bool OBJ, class SL>
__device__ __forceinline__ void collide(SL& s, const DevTables& T, const Params& P, int tid) {
    if (tid < 64) {
        int ncon = 0, next_b = 0;
        bool over = false;           // wave-uniform: a pair found more contacts than the layout has room for (the lean layout reports it: ncon = MAXCON + 1)
        const int ngeom = OBJ ? as_obj(s).ngeom : 0;
        unsigned mybits = 0;
        if (tid < D_NB && P.contact) {
            const V3 xb = ld3(s.xpos + 3 * tid);
            const float rb = T.body_rbound[tid];
            if (!(xb.z - rb > P.margin)) mybits = 1u;
            if constexpr (OBJ) {
                for (int gi = 0; gi < ngeom; gi++) {
                    const float* g = as_obj(s).geom + 17 * gi;
                    const V3 dx = xb - ld3(g + 4);
                    if (sqrtf(dot(dx, dx)) - rb - geom_rbound(g) > P.margin) continue;
                    // second, exact-safe cull: the hull lies inside the sphere (body origin, rbound) and a signed distance is 1-Lipschitz, so
                    // no point of it is closer to the primitive than sdf(origin) - rbound; only pairs that cannot touch are dropped (the
                    // 0.1 mm slack keeps fp32 rounding of this test away from the margin).  Saves the MPR query for most near misses.
                    if (geom_sdf(g, xb) - rb > P.margin + 1e-4f) continue;
                    mybits |= 2u << gi;
                }
            }
        }
        unsigned long long bodies = __ballot(mybits != 0u);
        while (bodies) {
            const int b = __ffsll((long long)bodies) - 1;
            bodies &= bodies - 1ull;
            unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)mybits, b);
            if (tid == 0) for (int bb = next_b; bb <= b; bb++) s.con_start[bb] = ncon;
            next_b = b + 1;
            const int vadr = T.vert_adr[b], nvb = T.vert_adr[b + 1] - vadr;
            const V3 xb = ld3(s.xpos + 3 * b);
            float R[9];
            q2mat(Q4{s.xquat[4 * b], s.xquat[4 * b + 1], s.xquat[4 * b + 2], s.xquat[4 * b + 3]}, R);
            V3 v = v3(0.f, 0.f, 0.f), xw = v3(0.f, 0.f, 3.0e38f);
            if (tid < nvb) { v = ld3(T.verts + 3 * (vadr + tid)); xw = xb + mulmat(R, v); }
            while (bits) {
                const int gi = __ffs((int)bits) - 2;           // -1 = floor
                bits &= bits - 1u;
                if (gi < 0) {
                    // mjc_PlaneConvex: the support vertex of -normal (deepest, first on ties) makes the first contact; then its hull-graph
                    // neighbours in graph order, while fewer than maxplanemesh (3) contacts exist, each within the margin and not closer
                    // than tolplanemesh * geom_rbound (0.3 rbound) to the first contact's position (addplanemesh)
                    const float dmin = wave_min(xw.z);
                    if (dmin > P.margin) continue;
                    const int idx = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(xw.z == dmin)) - 1);
                    const int n0 = T.vert_nbr_adr[vadr + idx], n1 = T.vert_nbr_adr[vadr + idx + 1];
                    // lane k < deg takes neighbour k of the support vertex (one coalesced load of the list), fetches that vertex from the
                    // lane that holds it, and ranks itself among the qualifying neighbours in list order with a ballot
                    const int deg = n1 - n0;
                    const int j = tid < deg ? (int)T.vert_nbr[n0 + tid] : 0;
                    const V3 xj = v3(__shfl(xw.x, j, 64), __shfl(xw.y, j, 64), __shfl(xw.z, j, 64));
                    const V3 x0 = v3(bcast_lane(xw.x, idx), bcast_lane(xw.y, idx), bcast_lane(xw.z, idx));
                    const V3 dj = xj - v3(x0.x, x0.y, x0.z - 0.5f * x0.z);           // vertex against the first contact's position
                    const float tolr = P.pm_tol * T.mesh_rbound[b];
                    const bool ok = tid < deg && !(xj.z > P.margin) && !(dot(dj, dj) < tolr * tolr);
                    const unsigned long long m = __ballot(ok);
                    const int rank = __popcll(m & ((1ull << tid) - 1ull));
                    const int extra = P.pm_max - 1;
                    const int cnt = 1 + min(__popcll(m), extra);
                    const int room = SL::MAXCON - ncon;
                    over |= cnt > room;
                    if (tid == idx && room > 0) put_contact<OBJ>(s, ncon, v3(xw.x, xw.y, xw.z - 0.5f * xw.z), xw.z, v3(0.f, 0.f, 1.f), b, -1);
                    if (ok && rank < extra && 1 + rank < room) put_contact<OBJ>(s, ncon + 1 + rank, v3(xj.x, xj.y, xj.z - 0.5f * xj.z), xj.z, v3(0.f, 0.f, 1.f), b, -1);
                    ncon += min(cnt, max(room, 0));
                } else if constexpr (OBJ) {
                    // mjc_Convex (libccd MPR): geom 1 = the box / cylinder, geom 2 = the hull; one contact, normal into the hull
                    EnvLdsObj& so = as_obj(s);
                    const float* g = so.geom + 17 * gi;
                    // Third, exact-safe cull before the MPR query (round 4: on the envs that end the `objects` launch 13 of 15 queries per substep
                    // found nothing and cost 5 - 6 k cycles each): a separating PLANE.  lane = hull vertex (xw, already in registers); if every
                    // vertex lies beyond one face plane of the box -- or beyond a cap plane / a tangent plane of the cylinder -- by more than the
                    // margin, the hull is farther than the margin from the primitive and libccd would return "no intersection" for the shapes
                    // inflated by margin / 2 each.  The 0.1 mm slack keeps the fp32 evaluation of the test away from the margin (the query itself
                    // runs in fp64 on the same fp32 poses); a pair that is not separated by one of these planes goes to the query as before.
                    {
                        const float* Rg = g + 7;
                        const V3 dv = xw - ld3(g + 4);
                        const float px = Rg[0] * dv.x + Rg[3] * dv.y + Rg[6] * dv.z, py = Rg[1] * dv.x + Rg[4] * dv.y + Rg[7] * dv.z, pz = Rg[2] * dv.x + Rg[5] * dv.y + Rg[8] * dv.z;
                        const bool has = tid < nvb;
                        const float lim = P.margin + 1e-4f;
                        bool sep;
                        if (g[0] == 0.f) {
                            const float hx = g[1] + lim, hy = g[2] + lim, hz = g[3] + lim;
                            sep = __ballot(has && !(px > hx)) == 0ull || __ballot(has && !(px < -hx)) == 0ull || __ballot(has && !(py > hy)) == 0ull ||
                                  __ballot(has && !(py < -hy)) == 0ull || __ballot(has && !(pz > hz)) == 0ull || __ballot(has && !(pz < -hz)) == 0ull;
                        } else {
                            const float hz = g[2] + lim;
                            sep = __ballot(has && !(pz > hz)) == 0ull || __ballot(has && !(pz < -hz)) == 0ull;
                            if (!sep) {          // tangent plane facing the hull: the unit radial direction u from the cylinder's axis towards the body origin
                                const V3 cb = xb - ld3(g + 4);
                                const float ux = Rg[0] * cb.x + Rg[3] * cb.y + Rg[6] * cb.z, uy = Rg[1] * cb.x + Rg[4] * cb.y + Rg[7] * cb.z;
                                const float un = sqrtf(ux * ux + uy * uy);
                                if (un > 1e-6f) sep = __ballot(has && !((px * ux + py * uy) > (g[1] + lim) * un)) == 0ull;
                            }
                        }
                        if (sep) continue;
                    }
                    const GeomSupport ga(g);
                    float* hrec = s.U + 232;                              // hull record of the support functor (LDS scratch: s.U is free outside the ABA passes)
                    hull_support_store(hrec, xb, xb + mulmat(R, ld3(T.body_ipos + 3 * b)), R);       // centre = the body's COM (xipos)
                    const HullSupport hb(hrec, v, tid < nvb);
                    Contact c;
                    if (convex_pair(ga, hb, P.margin, c, mpr_scratch(s)) && ncon < SL::MAXCON) {
                        if (tid == 0) put_contact<OBJ>(s, ncon, c.pos, c.dist, c.n, b, so.gobj[gi] < 0 ? -2 - gi : D_NB + so.gobj[gi]);
                        ncon++;
                    }
                }
            }
        }
        if (tid == 0) for (int bb = next_b; bb <= D_NB; bb++) s.con_start[bb] = ncon;
        if constexpr (OBJ) {
            // dynamic objects in slot order: every geom against the floor, then against the geoms of the objects in higher slots
            EnvLdsObj& so = as_obj(s);
            float* rec = s.U + 96;                             // contact records of one pair; s.U is free outside the ABA passes
            int slot_done = 0;
            unsigned gbits = 0;
            if (tid >= so.ngeom_static && tid < ngeom && P.contact) {
                const float* g = so.geom + 17 * tid;
                const V3 gp = ld3(g + 4);
                const float gra = geom_rbound(g);
                const int ka = so.gobj[tid];
                if (!(gp.z - gra > P.margin)) gbits = 1u;
                for (int gb = 0; gb < ngeom; gb++) {
                    const float* h = so.geom + 17 * gb;
                    if (so.gobj[gb] < 0 || so.gobj[gb] <= ka) continue;
                    const V3 dx = gp - ld3(h + 4);
                    if (sqrtf(dot(dx, dx)) - gra - geom_rbound(h) > P.margin) continue;
                    gbits |= 2u << gb;
                }
            }
            unsigned long long geoms = __ballot(gbits != 0u);
            while (geoms) {
                const int ga = __ffsll((long long)geoms) - 1;
                geoms &= geoms - 1ull;
                unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)gbits, ga);
                const float* g = so.geom + 17 * ga;
                const int ka = so.gobj[ga];
                while (slot_done < ka) { slot_done++; if (tid == 0) s.con_start[D_NB + slot_done] = ncon; }
                while (bits) {
                    const int gb = __ffs((int)bits) - 2;
                    bits &= bits - 1u;
                    const float* h = gb < 0 ? nullptr : so.geom + 17 * gb;
                    int n = 0, entB = -1; float sgn = 1.f;
                    if (gb < 0) {
                        if (g[0] == 0.f) {
                            // mjc_PlaneBox: lane = corner (bit 0 / 1 / 2 = +x / +y / +z); corners that point up or lie beyond the margin
                            // are skipped, the first four of the rest (in index order) make contacts
                            const int i = tid & 7;
                            const V3 corner = mulmat(g + 7, v3((i & 1) ? g[1] : -g[1], (i & 2) ? g[2] : -g[2], (i & 4) ? g[3] : -g[3]));
                            const float dist = g[6], ldist = corner.z;
                            const bool ok = tid < 8 && !(dist + ldist > P.margin || ldist > 0.f);
                            const unsigned long long m = __ballot(ok);
                            const int rank = __popcll(m & ((1ull << tid) - 1ull));
                            n = min(__popcll(m), 4);
                            if (ok && rank < 4) put_rec(rec, rank, dist + ldist, corner + ld3(g + 4) - (0.5f * (dist + ldist)) * v3(0.f, 0.f, 1.f), v3(0.f, 0.f, 1.f));
                        } else n = plane_cylinder(g, P.margin, rec, tid == 0);
                    } else {
                        // geom 1 = the lower geom type (cylinder < box), then the lower geom id (ga); the stored normal runs from gb into ga
                        const bool a_first = !(g[0] == 0.f && h[0] != 0.f);
                        entB = D_NB + so.gobj[gb]; sgn = a_first ? -1.f : 1.f;
                        if (g[0] == 0.f && h[0] == 0.f) {
                            if (tid == 0) n = box_box(g, h, P.margin, rec, s.U);
                            n = __builtin_amdgcn_readfirstlane(n);
                        } else {
                            const GeomSupport s1(a_first ? g : h), s2(a_first ? h : g);
                            Contact c;
                            n = convex_pair(s1, s2, P.margin, c, mpr_scratch(s));
                            if (n && tid == 0) put_rec(rec, 0, c.dist, c.pos, c.n);
                        }
                    }
                    n = min(n, SL::MAXCON - ncon);
                    if (tid < n) put_contact<OBJ>(s, ncon + tid, ld3(rec + 7 * tid + 1), rec[7 * tid], sgn * ld3(rec + 7 * tid + 4), D_NB + ka, entB);
                    ncon += n;
                }
            }
            while (slot_done < D_MAXOBJ) { slot_done++; if (tid == 0) s.con_start[D_NB + slot_done] = ncon; }
        }
        if (tid == 0) { s.ncon = (SL::LEAN && over) ? SL::MAXCON + 1 : ncon; s.nlim = 0; }
    }
    KP_SYNC();
}

}  // namespace kp
