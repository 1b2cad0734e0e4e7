// kp_step_device.hpp -- the device functions of the control step without its kernels: the part of kp_step_kernel.hpp above its "the kernel" rule (KP_SYNC,
// StepArgs, kp_kernarg, XcArgs, forward_kin_bias, the articulated-body passes, spd_torque_rfc, collide, make_constraint, both Newton solvers, the object
// code).  Every function there is a template or __forceinline__, so any translation unit may include this header; the read-out unit (kp_readout.hip) does.
// The two halves of kp_step_kernel.hpp have an include guard each, so this header and that one may be included in either order (kp_sim.hip has both).
// The text stays in one file; moving it here is a move only.
#pragma once
#define KP_STEP_DEVICE_ONLY
#include "kp_step_kernel.hpp"
#undef KP_STEP_DEVICE_ONLY
