// kp_step_args.hpp -- the argument block of the control step and the small helpers every phase shares (KP_SYNC, kp_launder, StepArgs, kp_kernarg, block_sum, the contact frame).  Part of kp_step_device.hpp.
#pragma once
#include "kp_device.hpp"
#include "kp_collide.hpp"      // wave_sum

namespace kp {

#define KP_SYNC() __syncthreads()

// An opaque copy of a lane index.  Everything the compiler derives from threadIdx.x alone (per-lane table addresses, the Lane8 schedule)
// is invariant over the substep loop and over the job loop of the queue kernel, so LLVM hoists it all to the kernel entry and then has
// ~150 such values live across the whole kernel: with the narrow phases' own demand that is far beyond the 256 VGPRs two waves per SIMD
// leave each wave, and the allocator parks them in scratch and reloads them at every use (839 scratch instructions in the object kernel,
// tools/micro/spill_report.py).  Re-deriving them from a laundered index per substep / per solve costs a few address adds and keeps
// their live ranges inside the phase that uses them.
__device__ __forceinline__ int kp_launder(int x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ int kp_launder_uniform(int x) { asm volatile("" : "+s"(x)); return x; }      // the same for a wave-uniform value (stays in an SGPR)

// the object extension of an env's LDS block.  Only reached under OBJ (a compile-time constant), where SL is EnvLdsObj itself; the other layouts never execute it
template <class SL> __device__ __forceinline__ EnvLdsObj& as_obj(SL& s) { return reinterpret_cast<EnvLdsObj&>(s); }
template <class SL> __device__ __forceinline__ const EnvLdsObj& as_obj(const SL& s) { return reinterpret_cast<const EnvLdsObj&>(s); }

struct StepArgs {
    DevTables T;
    Params P;
    int n_envs, n_substeps;
    // per-env state (HBM, row-major [N, dim])
    float *qpos, *qvel, *qpos_d, *qvel_d, *warm;
    float *warm3;              // [N][75] lean layout: the same vector between the solves of one job (step_body)
    float *warm2;              // [N][75] hand-over of the previous-but-one solution between the jobs of a control step (warm_extrap)
    float warm_extrap;         // beta of the extrapolated Newton start a_{k-1} + beta (a_{k-1} - a_{k-2}); 0 = MuJoCo's plain warm start
    const float *target_qpos, *action;
    const uint8_t* env_mask;  // optional: envs with mask==0 are skipped
    // outputs: kinematics of the last forward pass (x_14 in stale mode)
    float *xpos, *xquat, *xipos;
    int* diag;  // [N,4]: ncon (last substep), newton iterations (sum), flags | substeps whose Newton solve ended at the iteration cap << 8, max ncon | factorisations << 8
    unsigned long long* prof;  // optional [N,8] shader-clock cycles per phase (kp_sim_phase_cycles)
    float* dbg_contacts;       // optional [N, 1 + 64 * 9]: contacts of the last substep's collision pass (kp_sim_contacts; tests)
    const float* geoms;        // OBJ kernels: [N, D_MAXGEOM, 17] world-frame static geoms
    const int* ngeom;          // OBJ kernels: [N]
    // OBJ kernels, dynamic free objects: slot -> object index of the scene (-1 = empty), free-joint state of all objects
    const signed char* obj_slot;   // [N, D_MAXOBJ]
    float *obj_qpos, *obj_qvel, *obj_warm;   // [N, 35], [N, 30], [N, 6 * D_MAXOBJ]
    float *obj_warm2;                         // [N, 6 * D_MAXOBJ] the objects' a_{k-2} between the jobs of a control step (warm_extrap)
    // launch order (longest-processing-time first): workgroup i simulates env order[i]; cost[env] = shader-clock cycles >> 10 this
    // launch spent on env.  Both optional.  The result of an env does not depend on the workgroup that computes it.
    const int* order;
    unsigned* cost;
    // job-queue launch (kp_step_queue_kernel): a control step of an env = n_parts jobs of part_sub[] substeps handed from wave to
    // wave through HBM.  jobq [n_envs * n_parts] entries (env | part << 24, 0xFFFFFFFF = not yet published), jobctr = {head, tail, stalled}
    unsigned* jobq;
    unsigned* jobctr;
    int lean_cap;              // contacts a lean job accepts before it hands the env over (<= EnvLdsLean::MAXCON; model option lean_max_contacts)
    unsigned* ovfq;            // [n_envs] lean queue kernel: (env | part << 24) of the jobs whose contacts did not fit its layout; jobctr[64] = count, [65] = claimed (kp_step_overflow_kernel)
    float* spd_next;           // [N, 80]: qfrc_applied ++ qfrc_actuator (78 floats) of an env's NEXT substep, computed by the job that ran the substep before it
    int n_parts;
    int queue_heavy;           // > 0: a wave that finds its env heavy (this job's cycles per substep > queue_heavy % of the launch's running mean) runs the env's next job itself
    int queue_fence;           // 1: the hand-over is a release (publish) / acquire (consume) pair at agent scope instead of relaxed sc1 accesses + s_waitcnt
    int queue_late;            // 1: a wave whose env's FIRST job came from beyond the resident slots (it started late) runs that env's later jobs itself, at once
    int queue_prio;            // issue priority (s_setprio) of a wave: 0 none; 1 envs known to be heavy; 2 by the env's remaining jobs; 3 by its remaining substeps, re-set at every substep
    int order_valid;           // the first jobs were queued longest-env-first
    unsigned long long part_sub_lo, part_sub_hi;   // substeps of job 0 .. 15, one byte each (sum = n_substeps); packed so that no lookup indexes the kernel argument
};


// The argument block as it lies in the kernarg segment, behind a laundered scalar pointer.  Every kernel that runs step_body takes its StepArgs by value as
// its FIRST parameter, i.e. at offset 0 of the segment.  Read through the by-value parameter, all ~110 dwords of the block are loaded at the kernel's entry (in
// tuples of up to 16) and then parked in spill lanes for the whole job, to be restored tuple-wise inside the loops that use one field of them; read through
// this reference, a field is one scalar load from the constant cache at the site that uses it.  Same memory, same values.
__device__ __forceinline__ const StepArgs& kp_kernarg() {
    auto p = (const __attribute__((address_space(4))) StepArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const StepArgs*)p;
}

template <int NT, class SL>
__device__ __forceinline__ float block_sum(SL& s, float v, int tid) {
    v = wave_sum(v);
    if (NT > 64) {
        KP_SYNC();
        if ((tid & 63) == 0) s.red[tid >> 6] = v;
        KP_SYNC();
        v = 0.f;
#pragma unroll
        for (int w = 0; w < NT / 64; w++) v += s.red[w];
    }
    return v;
}

__device__ __forceinline__ constexpr int s6i(int r, int c) { return r <= c ? (r * (13 - r)) / 2 + (c - r) : (c * (13 - c)) / 2 + (r - c); }

// contact row e (0..3) of the pyramid in the plane frame n=(0,0,1), t1=(0,1,0), t2=(-1,0,0): dir = n +- mu t
__device__ __forceinline__ V3 row_dir(int e, float mu) {
    float sg = (e & 1) ? -mu : mu;
    return (e < 2) ? v3(0.f, sg, 1.f) : v3(-sg, 0.f, 1.f);
}
// row value from contact-frame components (n, t1, t2)
__device__ __forceinline__ float row_val(int e, float mu, float jn, float jt1, float jt2) {
    float sg = (e & 1) ? -mu : mu;
    return jn + sg * (e < 2 ? jt1 : jt2);
}
__device__ __forceinline__ V3 to_frame(V3 v) { return v3(v.z, v.y, -v.x); }  // (n, t1, t2) components of a world vector

// contact frame (n, t1, t2).  Floor-only kernels: the constant plane frame; OBJ kernels: mju_makeFrame of the stored normal.
struct Frame { V3 n, t1, t2; };
template <bool OBJ, class SL>
__device__ __forceinline__ Frame contact_frame(const SL& s, int c) {
    if (!OBJ) return Frame{v3(0.f, 0.f, 1.f), v3(0.f, 1.f, 0.f), v3(-1.f, 0.f, 0.f)};
    const float* cn = as_obj(s).con_n + 3 * c;
    const V3 n = ld3(cn);
    V3 y = fabsf(n.y) < 0.5f ? v3(0.f, 1.f, 0.f) : v3(0.f, 0.f, 1.f);
    y = y - dot(n, y) * n;
    y = (1.0f / sqrtf(dot(y, y))) * y;
    return Frame{n, y, cross(n, y)};
}
__device__ __forceinline__ V3 frame_comp(const Frame& f, V3 v) { return v3(dot(f.n, v), dot(f.t1, v), dot(f.t2, v)); }
__device__ __forceinline__ V3 frame_world(const Frame& f, V3 c) { return c.x * f.n + c.y * f.t1 + c.z * f.t2; }

}  // namespace kp
