// kp_render.hpp -- the offscreen renderer: what the reference shows through MuJoCo's GL viewer (Visualizer.render / save_screen_shots,
// scripts/eval_uhc.py:85-131, scripts/eval_pose_all.py:468-531), as a batched ray-caster over the collision geometry the engine already holds:
// the 24 convex hulls of every figure, the scene's object geoms (boxes, cylinders) and the floor.
//
// A hull is ray-cast as the intersection of its face half-spaces.  The blob holds hull vertices and a neighbour graph, not faces, so the face
// planes are built once per model on the host (hull_planes) and uploaded as one float4 table [n, 4] = (unit outward normal, d), n.x <= d inside,
// with per-body offsets [NB + 1].
//
// One pixel, exactly (tests/render_oracle.py restates this in fp64):
//   camera   (lookat[3], distance, azimuth, elevation, fovy), angles in degrees; forward f = (cos el cos az, cos el sin az, sin el), position
//            lookat - distance f, right = normalize(f x z), up = right x f; the ray goes through the pixel centre ((x + .5) / W, (y + .5) / H),
//            row 0 at the top: dir = normalize(f + (2u - 1) tan(fovy / 2) (W / H) right + (1 - 2v) tan(fovy / 2) up)
//   hits     nearest wins (the first on a tie, in the order floor, figures' bodies, object geoms), t > 0 only: the floor z = 0 when dir.z < 0,
//            up to zfar; every hull of every figure; every live object geom (placed as k_pose_contacts places them)
//   hull     the ray in the body frame clipped against the body's planes: t_in = max over planes with n.dir < 0, t_out = min over n.dir > 0, a
//            ray parallel to a plane and outside it misses; a hit when t_in <= t_out and t_in > 0 (a camera inside a hull does not see it)
//   box      six planes; cylinder: two cap planes along local z, then the quadratic of the side (size = radius, half height)
//   colour   base x (0.35 + 0.65 max(0, -n.dir)), n the hit face's normal (cylinder side: the analytic one), rounded to nearest; alpha 255
//   floor    1 m checker, parity (floor(x) + floor(y)) & 1 of the hit point
//
// The kernel lives in its own translation unit for the reason given in kp_pose_contacts.hpp: the step kernels' code must not move.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kp_model.hpp"

namespace kp {

constexpr int RD_MAXFIG = 4;          // figures of a row (simulated, expert, ...)
constexpr int RD_MAXGEOM = 16;        // object geoms of a model the renderer accepts (the reference's scenes have 10)
constexpr int RD_MAXDIM = 4096;       // width / height limit
constexpr int RD_TILES = 4;           // 8 x 8 pixel tiles (= wavefronts) of a workgroup

struct RenderStyle { float figure[RD_MAXFIG][3], object[3], floor[2][3], sky[3], zfar; };      // = kp_render_style (include/kinpoly_sim.h)

struct RenderArgs {
    int n_rows, n_fig, width, height, cam_rows, n_og, n_obj;
    int tiles_x, tiles, blocks_per_row;   // 8 x 8 tiles across, tiles of an image, workgroups of a row (filled in by launch_render)
    const float *xpos, *xquat;        // [R, n_fig, 72], [R, n_fig, 96]
    const float* obj_qpos;            // [R, 35] or null
    const float* camera;              // [cam_rows, 7], cam_rows = R or 1
    const float* og;                  // body-frame object geoms [n_og][18] (as PoseContactArgs::og)
    const float* rbound;              // [NB] bounding-sphere radius of every hull about its body origin
    const float4* planes;             // [n, 4]
    const int32_t* plane_adr;         // [NB + 1]
    RenderStyle style;
    int32_t* geom;                    // [R, H, W] or null
    float* depth;                     // [R, H, W] or null
    uint32_t* rgba;                   // [R, H, W] (r | g << 8 | b << 16 | 255 << 24) or null
};

// host: the face planes of the model's hulls, planes4 [n, 4] and adr [nb + 1]; returns n
int hull_planes(const HostModel& m, std::vector<float>& planes4, std::vector<int32_t>& adr);

// enqueues k_render on stream; the caller has checked the arguments
hipError_t launch_render(RenderArgs A, hipStream_t stream);

}  // namespace kp
