// kp_step_device.hpp -- the device functions of the fused control step: n_substeps x { stable-PD torque, residual
// force, mj_step-equivalent forward dynamics with soft contact (hulls, floor, free objects), semi-implicit Euler }.
//
// Replaces HOT LOOP C of the reference: HumanoidEnv.do_simulation (uhc/envs/humanoid_im.py:506-533)
//   compute_torque / compute_desired_accel   uhc/envs/humanoid_im.py:418-480
//   rfc_implicit                              uhc/envs/humanoid_im.py:497-504
//   sim.step()  (MuJoCo mj_step)              uhc/envs/humanoid_im.py:527         [MJ-ext]
// The arithmetic follows oracle/kp_oracle.c (fp64) in fp32, organised MATRIX-FREE for a wavefront:
//   * every spatial quantity is expressed in ONE world-aligned frame at the root body origin, so tree
//     recursions need no coordinate transforms: parents and children simply add;
//   * kinematics, velocities and bias forces (RNE) come out of one level-synchronous pass (9 levels);
//   * every linear solve -- (M + K_d h) for the stable-PD controller, M + J^T D J for the Newton steps of the
//     contact solver (M alone when no constraint row exists; qacc_smooth is never formed otherwise, see
//     solve_constraints_direct) -- is an articulated-body (ABA) pass:
//     leaves->root articulated inertia + bias, root->leaves accelerations.  K_d h and joint-limit terms
//     enter as extra joint armature, active contact rows as a per-body 6x6 "contact inertia" D w w^T.
//     The joint-space mass matrix is never formed or factorised (the reference materialises a dense
//     105x105 M and a Cholesky factor per substep);
//   * J v is read off the spatial accelerations the ABA forward pass leaves behind, J^T f and M v are a
//     body-wrench subtree sum projected on the dofs; the solver's Gauss term lives in body form (spatial
//     accelerations), so one projection per Newton iteration suffices;
//   * the first Newton factorisation of a substep walks every tree level; the later ones reuse its factors on the levels no active constraint reaches;
//   * the RNE bias forces are never projected on the dofs: they stay body wrenches and enter the passes as articulated bias force.
// Launch forms (kp_step_kernel.hpp): kp_step_kernel (one workgroup = one wavefront per env and control step), kp_forward_kernel (sim.forward() only) and
// kp_step_queue_kernel (the same step_body run by resident wavefronts that pull (env, few substeps) jobs from a FIFO in HBM, used
// when there are more envs than wavefront slots; bit-identical results; the finishing job hands its successor the next stable-PD torque, and a wave
// keeps an env it finds heavy or that started late).  The functions are templates over the LDS layout (kp_device.hpp): floor scenes' queue launches run on
// EnvLdsLean (12 envs per CU) and hand a job with more contacts than it holds to kp_step_overflow_kernel (full layout); same arithmetic, same bits.
//
// One header per phase, in the order of a substep.  Every function in them is a template or __forceinline__ and none is __global__, so any translation
// unit may include this header: the step unit does through kp_step_kernel.hpp, the read-out unit (kp_readout.hip) through kp_readout.hpp.
#pragma once
#include "kp_step_args.hpp"
#include "kp_step_kin.hpp"
#include "kp_step_aba.hpp"
#include "kp_step_pd.hpp"
#include "kp_step_collide.hpp"
#include "kp_step_solve.hpp"
#include "kp_step_obj.hpp"
