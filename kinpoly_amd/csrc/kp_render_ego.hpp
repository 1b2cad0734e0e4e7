// kp_render_ego.hpp -- the egocentric renderer: k_render's ray-caster (kp_render.hpp, kp_render_trace.hpp) behind a camera given as a pose -- one that
// can sit on a body and roll with it, which the viewer's free camera cannot -- and, for a pair of frames A and B, the exact optical flow of every pixel
// of A: the motion field that the rigid motion of what the pixel shows, and of the camera, produce between the two frames.  The reference's video
// features are PWC-Net flow over the wearer's video fed to a CNN; this is the signal that flow estimates, computed rather than estimated.
//
// One pixel, exactly (tests/ego_oracle.py restates this in fp64):
//   camera   one row [8] = eye[3], quaternion[4] (w, x, y, z; world from camera; normalised here), fovy in degrees.  The axes follow the head body's
//            convention (+z forward, +y up, +x to the left): with R = R(q), forward f = R e_z, up u = R e_y, right r = -R e_x, so a head quaternion
//            passes straight through.  dir = normalize(f + sx th (W / H) r + sy th u), th = tan(fovy / 2), sx = (2 px + 1 - W) / W,
//            sy = (H - 2 py - 1) / H: the pixel centres, row 0 at the top, as k_render
//   hits     as k_render (floor up to zfar, every hull of every figure, every live object geom, nearest wins with the same tie order), except
//            that body hide_body of figure 0 is not drawn (-1: none); for an eye mounted outside the head hull
//   pair     with a B side, the hit point p_A = eye_A + t dir is carried to frame B by the rigid motion of what was hit:
//            floor p_B = p_A; body b of figure k p_B = x_B + R_B R_A^T (p_A - x_A), R of the body's normalised quaternion (identical frames then
//            give exactly no rotation; the hits keep k_render's unnormalised one); object geom: the same with the geom's world pose in A and B (a
//            geom live in A but parked in B: ok = 0); sky: the direction dir as a point at infinity
//   project  c = R_camB^T (p_B - eye_B) (sky: c = R_camB^T dir); u' = (W / 2) (1 + (-c_x / c_z) / (th_B W / H)), v' = (H / 2) (1 - (c_y / c_z) / th_B);
//            flow = (u' - (px + .5), v' - (py + .5)) in pixels; ok = c_z > 0.01 (metres; sky: the unit direction's z component); ok = 0: flow (0, 0)
//   no visibility test in frame B: this is the motion field of the points visible in A
//   cells    the mean flow over the ok pixels of each cell of a Gy x Gx grid (a cell with no ok pixel: 0); the image is 8 a Gx wide and 8 b Gy high,
//            so a cell is a x b whole tiles.  Every wavefront reduces its tile to (sum u, sum v, count) across its lanes in a fixed butterfly
//            and writes one partial; k_flow_cells adds a cell's a b partials row by row and divides.  No atomics: equal inputs give equal bits.
//
// Lane mapping and launch shape are k_render's: one wavefront per 8 x 8 tile, RD_TILES tiles per workgroup, the row's set-up in LDS -- the
// per-body and per-geom blocks of k_render, and beside them one rigid motion (R_B R_A^T [9], x_B - R_B R_A^T x_A [3]) per body and per geom.
// Its own translation unit for the reason kp_render.hip has one: the step kernels' code must not move.
#pragma once
#include "kp_render.hpp"

namespace kp {

constexpr float EGO_MIN_Z = 0.01f;     // a carried point nearer than this to camera B's plane (or behind it) has no flow

struct RenderEgoArgs {
    int n_rows, n_fig, width, height, cam_rows, n_og, n_obj, hide_body;
    int grid_x, grid_y;               // cells: the grid (0: no cells)
    int tiles_x, tiles, blocks_per_row;   // filled in by launch_render_ego
    const float *xpos, *xquat, *obj_qpos, *camera;              // frame A: [R, n_fig, 72], [R, n_fig, 96], [R, 35] or null, [cam_rows, 8]
    const float *xpos_b, *xquat_b, *obj_qpos_b, *camera_b;      // frame B, or all null
    const float* og;                  // as RenderArgs
    const float* rbound;
    const float4* planes;
    const int32_t* plane_adr;
    RenderStyle style;
    int32_t* geom;                    // [R, H, W] or null
    float* depth;                     // [R, H, W] or null
    uint32_t* rgba;                   // [R, H, W] or null
    float* flow;                      // [R, H, W, 2] or null
    uint8_t* ok;                      // [R, H, W] or null
    float* cells;                     // [R, Gy, Gx, 2] or null
    float* partial;                   // [R, tiles, 3] scratch of the cells (sum u, sum v, count), or null without cells
};

// enqueues k_render_ego, and k_flow_cells when cells are wanted, on stream; the caller has checked the arguments
hipError_t launch_render_ego(RenderEgoArgs A, hipStream_t stream);

}  // namespace kp
