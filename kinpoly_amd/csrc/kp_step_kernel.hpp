// kp_step_kernel.hpp -- the kernels of the fused control step: step_body (one job = a few substeps of one env, built from the phases of kp_step_device.hpp,
// where the method is described) and the __global__ functions that run it, kp_mass_kernel, k_lpt_order and k_queue_init.  Non-template kernels among
// them: kp_sim.hip only.
#pragma once
#include <type_traits>

#include "kp_step_device.hpp"

namespace kp {

// the phase profiler's state (step_body<..., PROF = true>): shader-clock cycles per phase of the substep loop, [7] = the whole loop
struct PhaseClock {
    unsigned long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0 = 0, tstart = 0;
    __device__ __forceinline__ void lap(int i) { const unsigned long long t1 = __builtin_readcyclecounter(); pc[i] += t1 - t0; t0 = t1; }
};
// FWD = true compiles the forward-only launch (sim.forward(): derived quantities at a new state, no substeps) as its own
// small kernel, so that the control-step kernel's launches are the only ones under its name in a profile.
// Global accesses to state that one job of kp_step_queue_kernel writes and a later job (another wave, maybe another XCD with its own
// L2) reads.  Relaxed agent-scope atomics are plain loads / stores with the sc1 bit: they go through to the memory side instead of
// living in an XCD's L2, so the hand-over needs no L2 write-back / invalidate fence.  Outside the queue kernel: ordinary accesses.
template <bool Q, typename V> __device__ __forceinline__ V gld(const V* p) {
    if constexpr (Q) return __hip_atomic_load(const_cast<V*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool Q, typename V> __device__ __forceinline__ void gst(V* p, V v) {
    if constexpr (Q) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// LEAN: the floor scenes' job-queue layout (EnvLdsLean).  Returns 1 when the lean layout could not hold a substep's contacts: the job has written nothing to HBM at
// that point and is re-run on the full layout (kp_step_overflow_kernel); 0 otherwise.
// PROF: the phase profiler (kp_sim_phase_cycles) is a compile-time property.  Its eight counters and three time stamps are live through the whole job; as a
// run-time flag they cost every step kernel a quarter of its scalar-register spills and the lean queue kernel two vector spills.  The product
// instantiations carry none of it; the one-workgroup-per-env kernels exist a second time with it, and a profiled handle launches those.
template <int NT, bool OBJ, bool FWD, bool Q = false, bool LEAN = false, bool XC = false, bool PROF = false>
__device__ __forceinline__ int step_body(const int env_in, const int part, const XcArgs* X = nullptr) {
    static_assert(!LEAN || (Q && !OBJ && !FWD && NT == 64), "the lean layout serves the floor scenes' job queue only");
    static_assert(!PROF || (!Q && !FWD), "the phase profiler runs on the one-workgroup-per-env step kernels");
    // A is the kernel's read-only argument block where it lies in memory (kp_kernarg), taken anew at the top of every pass of the substep loop
    const StepArgs& A = kp_kernarg();
    // this job's share of the control step
    const int n_substeps = FWD ? 0 : (part >= 0 ? (int)(((part < 8 ? A.part_sub_lo >> (8 * part) : A.part_sub_hi >> (8 * (part - 8)))) & 255ull) : A.n_substeps);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using SL = typename std::conditional<OBJ, EnvLdsObj, typename std::conditional<LEAN, EnvLdsLean, EnvLds>::type>::type;
    SL& s = *reinterpret_cast<SL*>(smem_raw);
    const int tid0 = threadIdx.x;
    // laundered per job: the per-lane table addresses of the load section below are invariant over the queue kernel's job loop, so LLVM formed them all at
    // kernel entry and kept ~20 of them (64-bit, per lane) in scratch for the whole launch, reloading them in every job.  With the store section's
    // addresses (below) that made the object queue kernel's scratch 464 B per lane = 6.6 MB per XCD on 224 resident waves, more than the 4 MB of L2
    // behind them: every job's spills and reloads went to HBM (298 MB per launch, 22 x the algorithmic bytes; one workgroup per env: 176 B per lane,
    // 45 MB).  Now 176 B per lane and 101 MB per launch (profiles/r04/traffic_with_and_without_queue.log).
    const int tid = kp_launder(tid0);
    const int env = env_in;
    if (env >= A.n_envs) return 0;
    if (A.env_mask && !A.env_mask[env]) return 0;
    const unsigned long long t_launch = __builtin_readcyclecounter();
    const DevTables& T = A.T;
    const Params& P = A.P;

    // ---- load: derived state first (the state the last forward pass ran on), then the real state
    const float* tq_row = A.target_qpos ? A.target_qpos + (size_t)env * D_NQ : nullptr;
    const float* act_row = A.action ? A.action + (size_t)env * (XC ? X->stride : D_NV) : nullptr;
    int sub_base = 0;             // the extended controller's substep index: this job's first substep within the control step
    if constexpr (XC && Q) for (int p = 0; p < part; p++) sub_base += (int)(((p < 8 ? A.part_sub_lo >> (8 * p) : A.part_sub_hi >> (8 * (p - 8)))) & 255ull);
    // Torque hand-over between the jobs of a control step (stale mode): the stable-PD torque of substep k is a function of the kinematics of
    // substep k - 1, which sit in the LDS of the job that ran k - 1.  That job therefore also computes the torque of k (it is the same
    // solve its successor would start with) and hands over 78 floats; the successor then needs neither the derived state nor the forward
    // pass on it (17.7 k cycles of a 49 k hand-over).  The first job of a control step still starts from the derived state the previous
    // control step left.  Same code site, same operands: results do not depend on how the control step is cut.
    const bool torque_in = Q && P.stale && P.actuation && part > 0 && A.spd_next != nullptr;
    const bool torque_out = Q && P.stale && P.actuation && part >= 0 && part + 1 < A.n_parts && A.spd_next != nullptr;
    for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = gld<Q>((torque_in ? A.qpos : A.qpos_d) + (size_t)env * D_NQ + (unsigned)(i));
    for (int i = tid; i < D_NV; i += NT) {
        s.qvel[i] = gld<Q>((torque_in ? A.qvel : A.qvel_d) + (size_t)env * D_NV + (unsigned)(i));
        if constexpr (LEAN) s.extra[i] = T.dof_armature[i]; else { s.arm[i] = T.dof_armature[i]; s.extra[i] = 0.f; }
        s.dbody[i] = T.dof_body[i]; s.qacc[i] = gld<Q>(A.warm + (size_t)env * D_NV + (unsigned)(i));
    }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bsub[tid] = T.body_subtree[tid]; s.bdep[tid] = T.body_depth[tid]; }
    if (tid < 6) s.applied[tid] = 0.f;
    if (torque_in) for (int i = tid; i < 78; i += NT) s.applied[i] = gld<Q>(A.spd_next + (size_t)env * 80 + (unsigned)(i));
    if (tid < 25) s.IAa[22 * tid + 21] = 0.f;
    if (tid < 22) s.IAa[22 * 24 + tid] = 0.f;
    if (tid < 6) s.pAa[6 * 24 + tid] = 0.f;
    if (tid == 0) { s.ncon = 0; s.nlim = 0; s.flag = 0; }
    if constexpr (OBJ) {
        static_assert(NT == 64, "the object kernel runs one wavefront per environment");
        for (int i = tid; i < D_MAXGEOM * 17; i += NT) s.geom[i] = A.geoms[(size_t)env * D_MAXGEOM * 17 + (unsigned)(i)];
        const int ngs = A.ngeom[env];
        int nobj = 0, ng = ngs;
        if (tid < D_MAXGEOM) s.gobj[tid] = -1;
        for (int k = 0; k < D_MAXOBJ; k++) {
            const int oi = A.obj_slot ? A.obj_slot[(size_t)env * D_MAXOBJ + k] : -1;
            if (oi < 0 || oi >= T.n_obj) break;
            nobj = k + 1;
            if (tid < 7) s.oq[7 * k + tid] = gld<Q>(A.obj_qpos + (size_t)env * 35 + (unsigned)(7 * oi + tid));
            if (tid < 6) { s.ov[6 * k + tid] = gld<Q>(A.obj_qvel + (size_t)env * 30 + (unsigned)(6 * oi + tid)); s.oqa[6 * k + tid] = gld<Q>(A.obj_warm + (size_t)env * 6 * D_MAXOBJ + (unsigned)(6 * k + tid));
                           s.oqa_prev[6 * k + tid] = (A.warm_extrap != 0.f && Q && part > 0 && A.obj_warm2) ? gld<Q>(A.obj_warm2 + (size_t)env * 6 * D_MAXOBJ + (unsigned)(6 * k + tid)) : 0.f; }
            if (tid < 13) s.oc[13 * k + tid] = T.obj_inertial[13 * oi + tid];
            for (int gi = T.obj_geom_adr[oi]; gi < T.obj_geom_adr[oi + 1] && ng < D_MAXGEOM; gi++, ng++) {
                if (tid == 0) { s.gobj[ng] = (signed char)k; s.ggi[ng] = (unsigned char)gi; }
            }
        }
        if (tid == 0) { s.ngeom_static = ngs; s.ngeom = ng; s.nobj = nobj; }
    }
    KP_SYNC();
    float qd_save_q[(D_NQ + NT - 1) / NT], qd_save_v[(D_NV + NT - 1) / NT];
    int niter_total = 0, maxcon = 0, nfact_total = 0, ncap_total = 0;
    // Extrapolated start of the Newton solve (model option warm_extrap; round 5): see the solve's call site below.  The previous-but-one solution is
    // available from the control step's second substep on -- within a job in the words of qacc_s, across jobs through A.warm2 -- so whether a
    // substep extrapolates depends on its index in the control step only, never on how the control step is cut into jobs.
    const float beta = A.warm_extrap;
    bool have_prev = false;
    // lean layout (qacc_s is the solve's own vector there): a_{k-2} rides in a second HBM row of the env (A.warm3) between the solves of a job; the hand-over row
    // A.warm2 is read at the job's start and written at its end only, so that a job cut short by a contact overflow leaves no trace
    if (beta != 0.f && Q && part > 0 && A.warm2) {
        for (int i = tid; i < D_NV; i += NT) {
            const float v = gld<Q>(A.warm2 + (size_t)env * D_NV + (unsigned)(i));
            if constexpr (LEAN) gst<Q>(A.warm3 + (size_t)env * D_NV + (unsigned)(i), v); else s.qacc_s[i] = v;
        }
        have_prev = true;
    }
    const float* armv;            // dof armature as the solve reads it: the layout's copy, or the model table (lean layout: folded into extra for the eliminations)
    if constexpr (LEAN) armv = T.dof_armature; else armv = s.arm;
    auto store_readouts = [&](int lane, int e) {
        for (int i = lane; i < 72; i += NT) A.xpos[(size_t)e * 72 + (unsigned)(i)] = s.xpos[i];
        if (lane < D_NB) {                   // xipos = xpos + R ipos of the same forward pass
            const V3 xi = ld3(s.xpos + 3 * lane) + qrot(Q4{s.xquat[4 * lane], s.xquat[4 * lane + 1], s.xquat[4 * lane + 2], s.xquat[4 * lane + 3]}, ld3(T.body_ipos + 3 * lane));
            st3(A.xipos + (size_t)e * 72 + (unsigned)(3 * lane), xi);
        }
        for (int i = lane; i < 96; i += NT) A.xquat[(size_t)e * 96 + (unsigned)(i)] = s.xquat[i];
    };
    struct NoClock {};
    typename std::conditional<PROF, PhaseClock, NoClock>::type pk;
#define KP_T(i) if constexpr (PROF) pk.lap(i);
    // One loop, one inlined copy of every phase.  Pass -1 is the entry pass: the forward pass on the derived state the job was handed
    // (qpos_d / qvel_d), after which the real state is loaded; passes 0 .. n - 1 are the substeps; in fresh mode (stale_kinematics = 0)
    // pass n is the forward pass on the final state.  Running the entry pass through the SAME code as a substep's forward pass is what
    // makes a control step cut into jobs bit-identical to an uncut one (two inlined copies need not contract their FMAs alike), and it
    // keeps the kernel's code a third shorter.
    int rem_after = 0;          // substeps of the control step's later jobs (queue_prio = 3)
    if constexpr (Q) for (int p = part + 1; p < A.n_parts; p++) rem_after += (int)(((p < 8 ? A.part_sub_lo >> (8 * p) : A.part_sub_hi >> (8 * (p - 8)))) & 255ull);
    const int last_pass = (n_substeps > 0 && (!P.stale || torque_out)) ? n_substeps : n_substeps - 1;
    for (int sub = torque_in ? 0 : -1; sub <= last_pass; sub++) {
        // per-lane invariants are re-derived from a laundered lane index every pass (see kp_launder): table addresses, the body's tree
        // level and offset, and -- at the top of each solve -- the Lane8 schedule
        const int tid = kp_launder(tid0);
        const StepArgs& A = kp_kernarg();
        const DevTables& T = A.T;
        const Params& P = A.P;
        const int depth = tid < D_NB ? (int)s.bdep[tid] : -1;
        const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
        const bool substep = sub >= 0 && sub < n_substeps;
        if constexpr (Q) {
            // queue_prio = 3: issue priority by the env's distance from the end of its control step, set anew at every substep -- the waves of a SIMD then progress
            // together: an env that started late or runs heavy (and so has more substeps left than its neighbours) is preferred until it has caught up
            if (A.queue_prio == 3 && substep) {
                const int lvl = (4 * (rem_after + n_substeps - sub) - 1) / A.n_substeps;
                if (lvl >= 3) __builtin_amdgcn_s_setprio(3); else if (lvl == 2) __builtin_amdgcn_s_setprio(2); else if (lvl == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
            }
        }
        if constexpr (PROF) { if (sub == 0) pk.tstart = __builtin_readcyclecounter(); pk.t0 = __builtin_readcyclecounter(); }
        // stale mode: the controller sees M / bias of the previous forward pass (cinert, cdof, bias still in LDS)
        const bool spd_pass = torque_out && sub == n_substeps;           // the extra pass of a job that is not the control step's last: the successor's first torque
        // (the spd pass computes the torque of the control step's substep sub_base + n_substeps, the successor job's first)
        if ((substep || spd_pass) && P.stale && P.actuation && !(torque_in && sub == 0)) { Lane8 La; La.init(kp_launder(tid), T.sched8); spd_torque_rfc<NT, OBJ, SL, XC>(s, T, P, La, tid, tq_row, act_row, X, sub_base + sub); }
        if (spd_pass) {
            for (int i = tid; i < 78; i += NT) gst<Q>(A.spd_next + (size_t)env * 80 + (unsigned)(i), s.applied[i]);
            break;
        }
        if (substep && !P.actuation) {              // model option "actuation" = 0: ctrl = qfrc_applied = 0 (torque-free motion; tests)
            for (int i = tid; i < 78; i += NT) s.applied[i] = 0.f;          // applied[6] ++ ctrl[72]
            KP_SYNC();
        }
        KP_T(0)
        // ---- mj_forward at the current state
        if (sub >= 0) {
#pragma unroll
            for (int n = 0; n < (D_NQ + NT - 1) / NT; n++) { int i = tid + n * NT; if (i < D_NQ) qd_save_q[n] = s.qpos[i]; }
#pragma unroll
            for (int n = 0; n < (D_NV + NT - 1) / NT; n++) { int i = tid + n * NT; if (i < D_NV) qd_save_v[n] = s.qvel[i]; }
        }
        forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
        if (sub < 0) {          // entry pass: the derived state is what the forward pass just ran on (quaternion normalised); now the real state
#pragma unroll
            for (int n = 0; n < (D_NQ + NT - 1) / NT; n++) { int i = tid + n * NT; qd_save_q[n] = i < D_NQ ? s.qpos[i] : 0.f; }
#pragma unroll
            for (int n = 0; n < (D_NV + NT - 1) / NT; n++) { int i = tid + n * NT; qd_save_v[n] = i < D_NV ? s.qvel[i] : 0.f; }
            KP_SYNC();
            if (n_substeps > 0) {
                for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = gld<Q>(A.qpos + (size_t)env * D_NQ + (unsigned)(i));
                for (int i = tid; i < D_NV; i += NT) s.qvel[i] = gld<Q>(A.qvel + (size_t)env * D_NV + (unsigned)(i));
                KP_SYNC();
            }
            continue;
        }
        if (!substep) continue;         // fresh mode's exit pass: outputs are the kinematics of the final state
        if constexpr (OBJ) {
            if (beta != 0.f) {          // the objects' share of the extrapolated start, in their joint coordinates (obj_forward turns oqa into the spatial start oa)
                if (tid < 6 * s.nobj) { const float cur = s.oqa[tid]; if (have_prev) s.oqa[tid] = cur + beta * (cur - s.oqa_prev[tid]); s.oqa_prev[tid] = cur; }
                KP_SYNC();
            }
            obj_forward(s, T, P, tid);
        }
        KP_T(1)
        collide<NT, OBJ>(s, T, P, tid);
        if constexpr (LEAN) {
            if (s.ncon > min(SL::MAXCON, A.lean_cap)) return 1;      // wave-uniform; nothing of this job has been stored yet (lean_cap: model option, tests lower it to exercise the hand-over)
            // stale kinematics: the control step's read-outs are those of its last substep's forward pass; the solve below re-uses the words of xquat
            if (P.stale && sub == n_substeps - 1 && part == A.n_parts - 1) store_readouts(tid, env);
        }
        if (A.dbg_contacts && sub == n_substeps - 1) {      // test hook: the contact set of the last collision pass (con_D still holds the distance)
            float* o = A.dbg_contacts + (size_t)env * (1 + D_MAXCON * 9);
            if (tid == 0) o[0] = (float)s.ncon;
            for (int c = tid; c < s.ncon; c += NT) {
                float* r = o + 1 + 9 * c;
                r[0] = (float)s.con_body[c]; r[2] = s.con_D[c]; r[3] = s.con_pos[3 * c]; r[4] = s.con_pos[3 * c + 1]; r[5] = s.con_pos[3 * c + 2];
                if constexpr (OBJ) { const EnvLdsObj& so = as_obj(s); r[1] = so.con_b2[c] < 0 ? -1.f : (float)so.con_b2[c]; r[6] = so.con_n[3 * c]; r[7] = so.con_n[3 * c + 1]; r[8] = so.con_n[3 * c + 2]; }
                else { r[1] = -1.f; r[6] = 0.f; r[7] = 0.f; r[8] = 1.f; }
            }
        }
        KP_T(2)
        make_constraint<NT, OBJ>(s, T, P, tid);                 // needs sv = cvel: before any aba_solve
        KP_T(3)
        if (!P.stale && P.actuation) { Lane8 La; La.init(kp_launder(tid), T.sched8); spd_torque_rfc<NT, OBJ, SL, XC>(s, T, P, La, tid, tq_row, act_row, X, sub_base + sub); }
        for (int i = tid; i < D_NV; i += NT) s.extra[i] = LEAN ? T.dof_armature[i] : 0.f;
        KP_SYNC();
        Lane8 L8; L8.init(kp_launder(tid), T.sched8);          // lives through the Newton solve
        // Start of the Newton solve.  MuJoCo starts from the previous substep's solution a_{k-1} (qacc_warmstart); with warm_extrap = beta != 0 the start is
        // a_{k-1} + beta (a_{k-1} - a_{k-2}).  The problem is strictly convex: the minimiser and the termination tests do not depend on the starting point, only
        // the path does (INTEGRATION deviation 6 already starts from the warm start where MuJoCo might pick qacc_smooth).  Where accelerations change
        // smoothly from substep to substep -- falls, impacts, a humanoid going down on the table -- the extrapolated point is closer to the solution and has its
        // active set more often; on quiet standing states the change is contact chatter and extrapolating it gains nothing or costs.  Measured (MI355X, 60 timed
        // steps, profiles/r05/warm_extrap_*.log), launch ms / Newton iterations per substep at beta = 0 | 0.5 | 0.75 | 1: objects 4.77 / 1.95 | 4.61 / 1.87 |
        // 4.52 / 1.87 | 4.62 / 1.94; random_init 3.17 / 2.96 | 2.75 / 2.30 | 2.51 / 1.88 | 2.75 / 2.27; tracked (the metric) 2.616 / 2.06 | 2.621 / 2.02 | 2.636 / 2.05 |
        // 2.697 / 2.14; wild_eval + 2 ... 4 % at 0.5 - 0.75.  Extrapolating only across large changes (a threshold on max |a_{k-1} - a_{k-2}|) is worse than either:
        // the large changes are the contact events, where the extrapolation is wrong.  Defaults: 0.75 when the scene's free objects are simulated, 0 (MuJoCo's
        // start) for floor scenes -- a caller whose envs are mostly falling (a policy at random init) sets 0.75.  a_{k-2} rides in the words of qacc_s between
        // solves (dead outside the
        // solve, where they hold the gradient); a_{k-1} is kept in two registers across the solve.  The objects' accelerations likewise (oqa / oqa_prev, in their joint coordinates).
        float keep0 = 0.f, keep1 = 0.f;
        if (beta != 0.f) {
            const int i0 = tid, i1 = tid + NT;
            auto prev = [&](int i) { if constexpr (LEAN) return gld<Q>(A.warm3 + (size_t)env * D_NV + (unsigned)(i)); else return s.qacc_s[i]; };
            if (i0 < D_NV) { keep0 = s.qacc[i0]; if (have_prev) s.qacc[i0] = keep0 + beta * (keep0 - prev(i0)); }
            if (NT < D_NV && i1 < D_NV) { keep1 = s.qacc[i1]; if (have_prev) s.qacc[i1] = keep1 + beta * (keep1 - prev(i1)); }
            KP_SYNC();
        }
        if constexpr (OBJ) {
            KP_T(4)                                            // no smooth solve: the Newton solve starts from the warm start (solve_constraints_direct)
            niter_total += solve_constraints_obj<NT>(s, P, L8, depth, tid, nfact_total, ncap_total, s.arm);
        } else {
            KP_T(4)
            niter_total += solve_constraints_direct<NT>(s, P, L8, depth, tid, nfact_total, ncap_total, armv);
            if constexpr (LEAN) {
                // the solve's body accelerations lived in the words of qpos | qvel: both come back from the registers that hold this substep's forward-pass state,
                // the root quaternion normalised as forward_kin_bias left it
#pragma unroll
                for (int n = 0; n < (D_NQ + NT - 1) / NT; n++) { int i = tid + n * NT; if (i < D_NQ) s.qpos[i] = qd_save_q[n]; }
#pragma unroll
                for (int n = 0; n < (D_NV + NT - 1) / NT; n++) { int i = tid + n * NT; if (i < D_NV) s.qvel[i] = qd_save_v[n]; }
                KP_SYNC();
                if (tid == 0) { const Q4 q = qnormalize(Q4{s.qpos[3], s.qpos[4], s.qpos[5], s.qpos[6]}); s.qpos[3] = q.w; s.qpos[4] = q.x; s.qpos[5] = q.y; s.qpos[6] = q.z; }
                KP_SYNC();
            }
        }
        if (beta != 0.f) {
            const int i0 = tid, i1 = tid + NT;
            if constexpr (LEAN) {
                if (i0 < D_NV) gst<Q>(A.warm3 + (size_t)env * D_NV + (unsigned)(i0), keep0);
                if (NT < D_NV && i1 < D_NV) gst<Q>(A.warm3 + (size_t)env * D_NV + (unsigned)(i1), keep1);
            } else {
                if (i0 < D_NV) s.qacc_s[i0] = keep0;
                if (NT < D_NV && i1 < D_NV) s.qacc_s[i1] = keep1;
            }
            have_prev = true;
            KP_SYNC();
        }
        KP_T(5)
        maxcon = max(maxcon, s.ncon);
        // ---- semi-implicit Euler (mj_Euler, no damping)
        if constexpr (OBJ) obj_integrate(s, P, tid);       // reads xpos[0] (o) of this substep's forward pass
        for (int i = tid; i < D_NV; i += NT) s.qvel[i] += P.h * s.qacc[i];
        KP_SYNC();
        for (int j = tid; j < D_NU; j += NT) s.qpos[7 + j] += P.h * s.qvel[6 + j];
        if (tid == 0) {
            s.qpos[0] += P.h * s.qvel[0]; s.qpos[1] += P.h * s.qvel[1]; s.qpos[2] += P.h * s.qvel[2];
            V3 w = ld3(s.qvel + 3);
            float n = sqrtf(dot(w, w));
            Q4 qr = Q4{1.f, 0.f, 0.f, 0.f};
            if (n >= 1e-15f) { float sn, cs; sincosf(0.5f * P.h * n, &sn, &cs); float k = sn / n; qr = Q4{cs, w.x * k, w.y * k, w.z * k}; }
            Q4 q = qmul(qnormalize(Q4{s.qpos[3], s.qpos[4], s.qpos[5], s.qpos[6]}), qr);
            s.qpos[3] = q.w; s.qpos[4] = q.x; s.qpos[5] = q.y; s.qpos[6] = q.z;
        }
        KP_SYNC();
        KP_T(6)
    }
    if constexpr (PROF) {
        if (tid == 0 && n_substeps > 0) {
            pk.pc[7] = __builtin_readcyclecounter() - pk.tstart;
            for (int k = 0; k < 8; k++) A.prof[8 * (size_t)env + k] = pk.pc[k];
        }
    }
    // ---- store.  The row addresses are re-derived from laundered copies of the env and lane indices: the ones the load section formed at the top of the job
    // would otherwise stay live through the whole job (37 spilled 64-bit addresses per lane in the object queue kernel)
    const int tidS = kp_launder(tid0);
    const int envS = kp_launder_uniform(env);
    bool bad = false;
    for (int i = tidS; i < D_NQ; i += NT) { float v = s.qpos[i]; bad |= !(fabsf(v) < 1e10f); if (n_substeps > 0) gst<Q>(A.qpos + (size_t)envS * D_NQ + (unsigned)(i), v); }
    for (int i = tidS; i < D_NV; i += NT) { float v = s.qvel[i]; bad |= !(fabsf(v) < 1e10f); if (n_substeps > 0) { gst<Q>(A.qvel + (size_t)envS * D_NV + (unsigned)(i), v); gst<Q>(A.warm + (size_t)envS * D_NV + (unsigned)(i), s.qacc[i]); if (Q && beta != 0.f && A.warm2 && part >= 0 && part + 1 < A.n_parts) { float pv; if constexpr (LEAN) pv = gld<Q>(A.warm3 + (size_t)envS * D_NV + (unsigned)(i)); else pv = s.qacc_s[i]; gst<Q>(A.warm2 + (size_t)envS * D_NV + (unsigned)(i), pv); } } }
    if (!torque_out) {       // the derived state is read by the control step's NEXT first job only (a job that hands its torque over has no reader for it)
#pragma unroll
        for (int n = 0; n < (D_NQ + NT - 1) / NT; n++) { int i = tidS + n * NT; if (i < D_NQ) gst<Q>(A.qpos_d + (size_t)envS * D_NQ + (unsigned)(i), qd_save_q[n]); }
#pragma unroll
        for (int n = 0; n < (D_NV + NT - 1) / NT; n++) { int i = tidS + n * NT; if (i < D_NV) gst<Q>(A.qvel_d + (size_t)envS * D_NV + (unsigned)(i), qd_save_v[n]); }
    }
    // read-outs: the last job of the control step only (earlier jobs' copies could land later from another L2); lean layout in stale mode: already stored (above)
    if ((!Q || part == A.n_parts - 1) && !(LEAN && P.stale && n_substeps > 0)) store_readouts(tidS, envS);
    if constexpr (OBJ) {
        if (n_substeps > 0) {
            for (int k = 0; k < s.nobj; k++) {
                const int oi = A.obj_slot[(size_t)envS * D_MAXOBJ + k];
                if (tidS < 7) { const float v = s.oq[7 * k + tidS]; bad |= !(fabsf(v) < 1e10f); gst<Q>(A.obj_qpos + (size_t)envS * 35 + (unsigned)(7 * oi + tidS), v); }
                if (tidS < 6) { gst<Q>(A.obj_qvel + (size_t)envS * 30 + (unsigned)(6 * oi + tidS), s.ov[6 * k + tidS]); gst<Q>(A.obj_warm + (size_t)envS * 6 * D_MAXOBJ + (unsigned)(6 * k + tidS), s.oqa[6 * k + tidS]);
                                if (Q && A.warm_extrap != 0.f && A.obj_warm2 && part >= 0 && part + 1 < A.n_parts) gst<Q>(A.obj_warm2 + (size_t)envS * 6 * D_MAXOBJ + (unsigned)(6 * k + tidS), s.oqa_prev[6 * k + tidS]); }
            }
        }
    }
    if (bad) atomicOr(&s.flag, 1);
    KP_SYNC();
    if (tidS == 0 && A.diag && n_substeps > 0) {
        int* dg = A.diag + 4 * (size_t)envS;
        if (part > 0) {      // later job of the same control step: accumulate
            const int d3 = gld<Q>(dg + 3), d2 = gld<Q>(dg + 2);
            niter_total += gld<Q>(dg + 1); s.flag |= d2 & 255; ncap_total += d2 >> 8;
            maxcon = max(maxcon, d3 & 255); nfact_total += d3 >> 8;
        }
        gst<Q>(dg + 0, s.ncon); gst<Q>(dg + 1, niter_total); gst<Q>(dg + 2, (s.flag & 255) | (ncap_total << 8)); gst<Q>(dg + 3, maxcon | (nfact_total << 8));
    }
    if (tidS == 0 && A.cost && n_substeps > 0)
        gst<Q>(A.cost + envS, (part > 0 ? gld<Q>(A.cost + envS) : 0u) + (unsigned)((__builtin_readcyclecounter() - t_launch) >> 10));
    return 0;
}

// mj_fullM(model, M, data.qM)[:75, :75] and data.qfrc_bias[:75] as the reference's compute_desired_accel reads them
// (uhc/envs/humanoid_im.py:422-426): the dense joint-space inertia matrix (armature included) and the bias force of the state the
// derived quantities belong to (qpos_d / qvel_d: what mujoco-py's data holds between sim.step() calls).  The simulator itself
// never forms either (every solve is an articulated-body pass); this read-out builds column j of M as the projection of the body
// wrenches I_b a_b(e_j) summed over subtrees (a composite-rigid-body product M e_j), and qfrc_bias as the same projection of the
// RNE body wrenches.  Off the hot path: 76 projections per env.
__global__ __launch_bounds__(64) void kp_mass_kernel(StepArgs A, float* __restrict__ Mout, float* __restrict__ bias_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    EnvLds& s = *reinterpret_cast<EnvLds*>(smem_raw);
    constexpr int NT = 64;
    const int tid = threadIdx.x, env = blockIdx.x;
    if (env >= A.n_envs) return;
    const DevTables& T = A.T;
    const Params& P = A.P;
    const int depth = tid < D_NB ? T.body_depth[tid] : -1;
    const V3 bpos = tid < D_NB ? ld3(T.body_pos + 3 * tid) : v3(0.f, 0.f, 0.f);
    for (int i = tid; i < D_NQ; i += NT) s.qpos[i] = A.qpos_d[(size_t)env * D_NQ + i];
    for (int i = tid; i < D_NV; i += NT) { s.qvel[i] = A.qvel_d[(size_t)env * D_NV + i]; s.arm[i] = T.dof_armature[i]; s.dbody[i] = T.dof_body[i]; }
    if (tid < D_NB) { s.bpar[tid] = (unsigned char)(T.body_parent[tid] < 0 ? 0 : T.body_parent[tid]); s.bsub[tid] = T.body_subtree[tid]; s.bdep[tid] = T.body_depth[tid]; }
    KP_SYNC();
    forward_kin_bias<NT>(s, T, P, depth, bpos, tid);
    // qfrc_bias: subtree sums of the RNE body wrenches projected on the motion axes (backward half of mj_rne)
    for (int it = tid; it < D_NB * 6; it += NT) {
        const int b = it / 6, c = it - 6 * b, n = s.bsub[b];
        float acc = 0.f;
        for (int k = b; k < b + n; k++) acc += s.fb[6 * k + c];
        s.sa[it] = acc;
    }
    KP_SYNC();
    if (bias_out) for (int d = tid; d < D_NV; d += NT) bias_out[(size_t)env * D_NV + d] = dot6(lds6(s.cdof + 6 * d), lds6(s.sa + 6 * s.dbody[d]));
    KP_SYNC();
    if (!Mout) return;
    for (int j = 0; j < D_NV; j++) {
        for (int i = tid; i < D_NV; i += NT) s.x[i] = i == j ? 1.f : 0.f;
        KP_SYNC();
        spatial_accumulate<NT>(s, s.x, depth, tid);
        wrench_project<NT, false>(s, P, s.sv, s.x, nullptr, s.qacc_s, true, false, tid, s.arm);
        for (int d = tid; d < D_NV; d += NT) Mout[((size_t)env * D_NV + d) * D_NV + j] = s.qacc_s[d];
        KP_SYNC();
    }
}

// Launch order for the next control step: envs sorted by the cycles they took in the last one, longest first (counting sort on
// 256 bins scaled to the maximum, one workgroup).  With N envs on 8 x 256 wave slots the launch otherwise ends on whichever
// long env (many contacts, many Newton iterations) happened to start in the second round.
__global__ __launch_bounds__(1024) void k_lpt_order(int n, const unsigned* __restrict__ cost, int* __restrict__ order) {
    __shared__ unsigned hist[256], base[256], cmax;
    const int tid = threadIdx.x;
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) cmax = 1;
    __syncthreads();
    unsigned m = 0;
    for (int i = tid; i < n; i += 1024) m = max(m, cost[i]);
    atomicMax(&cmax, m);
    __syncthreads();
    const float sc = 255.f / (float)cmax;
    for (int i = tid; i < n; i += 1024) atomicAdd(&hist[255 - (int)((float)cost[i] * sc)], 1u);
    __syncthreads();
    if (tid == 0) { unsigned a = 0; for (int b = 0; b < 256; b++) { base[b] = a; a += hist[b]; } }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) order[atomicAdd(&base[255 - (int)((float)cost[i] * sc)], 1u)] = i;
}

template <int NT, bool OBJ, bool PROF = false>
__global__ __launch_bounds__(NT, (NT == 64 ? 2 : 1)) void kp_step_kernel(StepArgs A) {
    step_body<NT, OBJ, false, false, false, false, PROF>(A.order ? A.order[blockIdx.x] : (int)blockIdx.x, -1);
}
// the extended controller (XcArgs), one workgroup per env
template <int NT, bool OBJ, bool PROF = false>
__global__ __launch_bounds__(NT, (NT == 64 ? 2 : 1)) void kp_step_kernel_xc(StepArgs A, XcArgs X) {
    step_body<NT, OBJ, false, false, false, true, PROF>(A.order ? A.order[blockIdx.x] : (int)blockIdx.x, -1, &X);
}
template <int NT, bool OBJ>
__global__ __launch_bounds__(NT, (NT == 64 ? 2 : 1)) void kp_forward_kernel(StepArgs A) { step_body<NT, OBJ, true>((int)blockIdx.x, -1); }

// Same control step, scheduled in finer grains.  4096 envs on 8 x 256 wave slots are two rounds of whole-control-step jobs whose
// lengths spread 2.9 M .. 5.4 M cycles, so a third of a kp_step_kernel launch is its tail (tools/launch_balance.py).  Here one
// resident wavefront per slot pulls jobs (env, part) from a FIFO in HBM: a job is a few substeps of one env, and finishing it
// publishes the env's next part at the tail.  An env therefore migrates between waves (its state already round-trips through HBM at
// job boundaries exactly as it does between launches), the makespan becomes sum / slots + about one job, and the arithmetic is
// that of kp_step_kernel bit for bit.  Progress: indices are claimed in order, so a wave that waits for entry idx waits for a publish by
// a wave that is running a job; if nothing is running every entry below n_envs * n_parts has been published.  A bounded wait (2 s) turns
// any violation of that argument into an error flag (jobctr[2]) instead of a hung queue.
// Memory ordering of the hand-over, two variants (model option "queue_fence"):
//   1 (default)  the state arrays a later job reads are written / read as relaxed agent-scope atomics (sc1 write-through accesses), and the
//                publish is bracketed by __builtin_amdgcn_fence(release, agent) on the producing wave and fence(acquire, agent) after the
//                consuming load: a release / acquire pair, correct by the HIP memory model.
//   0            the round-1 form without the two fences: s_waitcnt vmcnt(0) alone orders the sc1 stores before the publish.  Correct on
//                gfx950 by what sc1 means in hardware only.
// Both are bit-identical in results (test_job_queue_schedule_is_bit_identical).  Measured on MI355X, 4096 envs standing + contact
// (tools/queue_fence_bench.py, profiles/r02/queue_fence_bench.log): 3.818 ms (0) vs 3.837 ms (1) per launch -- the fences cost 0.5 %, so
// the variant that is correct by construction is the default.
// LEAN (floor scenes): the EnvLdsLean layout and a register budget for three waves per SIMD; a job whose contacts do not fit the layout is handed, with the env's
// remaining jobs, to kp_step_overflow_kernel (launched right behind this kernel, same stream).
template <bool OBJ, bool LEAN, bool XC>
__device__ __forceinline__ void step_queue_body(const StepArgs& A, const XcArgs* X) {
    // jobctr: [0] head (claimed), [1] tail (published), [2] stalled flag; on cache lines of their own, away from the head / tail every claim and publish hits:
    //         [16] jobs that were never queued because the finishing wave ran them itself; [32] time (40 ns units) and [33] substeps of the jobs finished so
    //         far in this launch; [48], [49] the same sums of the previous launch (the mean behind "heavy": constant during the launch, read once per wave)
    const unsigned total = (unsigned)A.n_envs * (unsigned)A.n_parts;
    const unsigned prev_tot = A.jobctr[48], prev_cnt = A.jobctr[49];
    for (;;) {
        unsigned idx = 0;
        if (threadIdx.x == 0) idx = atomicAdd(&A.jobctr[0], 1u);
        idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
        if (idx >= total) return;
        unsigned e, spins = 0;
        unsigned long long t_wait = 0;
        while ((e = __hip_atomic_load(&A.jobq[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0xFFFFFFFFu) {
            // Back-off: the first polls come 0.9 us apart (a job published mid-launch is picked up at once); a wave that has waited longer is in the
            // launch's tail, where the work left is the costliest envs' chains that their own waves keep (queue_heavy) -- it polls every 3.4 ... 27 us.
            // Every poll is a read that goes through to memory (agent-scope atomic) on behalf of a wave that has nothing to do.
            if (spins < 16u) __builtin_amdgcn_s_sleep(32);
            else for (unsigned k = 0; k <= min((spins - 16u) >> 3, 7u); k++) __builtin_amdgcn_s_sleep(127);
            // entries at and beyond total - jobctr[16] will never be published (the counter only grows): nothing left for this wave
            if (idx >= total - __hip_atomic_load(&A.jobctr[16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
            // a bounded wait (2 s of the 100 MHz clock) turns any violation of the progress argument into an error flag instead of a hung queue
            if (++spins == 1u) t_wait = __builtin_amdgcn_s_memrealtime();
            else if ((spins & 63u) == 0u && __builtin_amdgcn_s_memrealtime() - t_wait > 200000000ull) { if (threadIdx.x == 0) atomicExch(&A.jobctr[2], 1u); return; }
        }
        asm volatile("" ::: "memory");                        // the job's (sc1) state loads stay behind the load that saw the entry
        if (A.queue_fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // memory-model variant: acquire side of the publish below
        e = (unsigned)__builtin_amdgcn_readfirstlane((int)e);
        const int env = (int)(e & 0xFFFFFFu);
        int part = (int)(e >> 24);
        // With more envs than slots the launch ends on the envs whose first job had to wait for a slot: their chain starts one job late, and every pass through
        // the FIFO (behind the early envs' later jobs) delays it further.  queue_late: such an env is never queued again.
        const bool late = A.queue_late && part == 0 && idx >= gridDim.x;
        // (running a late env's whole control step as ONE job, without the hand-overs between its parts, was measured and dropped: 2.216 vs 2.194 ms,
        // profiles/r06/lean_schedule_knobs5.log)
        // Issue priority: the launch ends on its costliest envs' serial chains, and a wave shares its SIMD's issue slots with one other wave.  A wave that
        // runs a job of an env known to be heavy -- one of the first queue entries when the first jobs were queued longest-env-first (k_lpt_order), or an
        // env it kept because its last job ran long (below) -- raises its own priority, so the SIMD's arbiter prefers it over its neighbour
        // (s_setprio: scheduling only, results do not depend on it); every other job runs at the default priority.
        if (A.queue_prio == 1) { if (A.order_valid && part == 0 && idx < (unsigned)A.n_envs / 16u) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(0); }
        // queue_prio = 2: most remaining work first.  With more envs than slots the envs whose first job starts late are the ones the launch ends on; a wave on an
        // env's first job outranks its SIMD neighbours on second jobs, those outrank last jobs (at the launch's start every wave is on a first job: no preference)
        if (A.queue_prio == 2) { if (part == 0) __builtin_amdgcn_s_setprio(2); else if (part + 1 < A.n_parts) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        for (;;) {
            const unsigned long long tj = __builtin_amdgcn_s_memrealtime();          // 100 MHz ticks: only ratios of job times are used
            const int overflow = step_body<64, OBJ, false, true, LEAN, XC>(env, part, X);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // every lane's write-through state store has been acknowledged ...
            if (A.queue_fence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // memory-model variant: release all of this wave's stores at agent scope
            if (LEAN && overflow) {
                // more contacts than the lean layout holds: this job (which has stored nothing) and the env's later jobs go to the overflow list; none of them
                // will be published to this queue, which the waiting waves learn from jobctr[16] like they do for jobs a wave kept
                if (threadIdx.x == 0) {
                    A.ovfq[atomicAdd(&A.jobctr[64], 1u)] = (unsigned)env | ((unsigned)part << 24);
                    atomicAdd(&A.jobctr[16], (unsigned)(A.n_parts - 1 - part));
                }
                break;
            }
            if (part + 1 >= A.n_parts) break;
            // An env whose jobs run long is the one the launch will end on: with two envs per slot every hand-over through the FIFO costs it about one
            // job's length of waiting.  The wave that finds its env heavy -- cycles per substep above queue_heavy % of the launch's running mean --
            // keeps it: it runs the next job itself, at once, and the queue gets one entry fewer (jobctr[3]).  Who runs a job never changes its result.
            int keep = 0;
            if (A.queue_heavy > 0 && threadIdx.x == 0) {
                const unsigned nsub = (unsigned)(((part < 8 ? A.part_sub_lo >> (8 * part) : A.part_sub_hi >> (8 * (part - 8)))) & 255ull);
                const unsigned dt = (unsigned)((__builtin_amdgcn_s_memrealtime() - tj) >> 2);      // 40 ns units: the launch's sum stays far below 2^32
                atomicAdd(&A.jobctr[32], dt); atomicAdd(&A.jobctr[33], nsub);
                // the yardstick is the PREVIOUS launch's mean (k_queue_init moves it to jobctr[48..49]): this launch's own running mean is made of the jobs
                // that finished first, i.e. of the light ones.  Jobs of fewer than four substeps are too noisy a sample of their env (one extra Newton
                // iteration in one substep is + 25 %)
                keep = prev_cnt >= 512u && nsub >= 4u && (unsigned long long)dt * prev_cnt * 100ull > (unsigned long long)prev_tot * nsub * (unsigned)A.queue_heavy;
            }
            keep = __builtin_amdgcn_readfirstlane(keep) | (int)late;
            if (!keep) {
                if (threadIdx.x == 0) {                                    // ... before the env's next job becomes visible
                    const unsigned pos = atomicAdd(&A.jobctr[1], 1u);
                    __hip_atomic_store(&A.jobq[pos], (unsigned)env | ((unsigned)(part + 1) << 24), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                break;
            }
            if (threadIdx.x == 0) atomicAdd(&A.jobctr[16], 1u);
            if (A.queue_prio == 1) __builtin_amdgcn_s_setprio(3);
            part++;
            if (A.queue_prio == 2) { if (part + 1 < A.n_parts) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(1); }      // a kept (heavy) env stays one rank above its part
        }
    }
}

template <bool OBJ, bool LEAN = false>
__global__ __launch_bounds__(64, (LEAN ? 3 : 2)) void kp_step_queue_kernel(StepArgs A) { step_queue_body<OBJ, LEAN, false>(A, nullptr); }
// the extended controller (XcArgs) on the full / object layout (never the lean one)
template <bool OBJ>
__global__ __launch_bounds__(64, 2) void kp_step_queue_kernel_xc(StepArgs A, XcArgs X) { step_queue_body<OBJ, false, true>(A, &X); }

// The jobs the lean queue kernel could not hold (more than EnvLdsLean::MAXCON contacts in a substep), run on the full layout: a wave claims an entry and runs that
// job and the env's remaining jobs itself.  Launched behind every lean queue launch; with an empty list (the rule: floor scenes hold 7 - 10 contacts) every wave
// leaves at its first read.  The arithmetic is step_body's: which kernel ran a job changes nothing but the contact capacity.
__global__ __launch_bounds__(64, 2) void kp_step_overflow_kernel(StepArgs A) {
    for (;;) {
        unsigned idx = 0;
        if (threadIdx.x == 0) idx = atomicAdd(&A.jobctr[65], 1u);
        idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
        if (idx >= __hip_atomic_load(&A.jobctr[64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&A.ovfq[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const int env = (int)(e & 0xFFFFFFu);
        for (int part = (int)(e >> 24); part < A.n_parts; part++) {
            step_body<64, false, false, true, false>(env, part);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            if (A.queue_fence) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
        }
    }
}

// order (optional): the envs' first jobs enter the FIFO longest-env-first (k_lpt_order on the previous control step's cycles) instead of in
// env order, so that the env whose three jobs take longest does not also start last
__global__ void k_queue_init(int n_envs, unsigned total, unsigned* __restrict__ jobq, unsigned* __restrict__ jobctr, const int* __restrict__ order) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) jobq[i] = i < (unsigned)n_envs ? (order ? (unsigned)order[i] : i) : 0xFFFFFFFFu;
    if (i == 0) { jobctr[0] = 0u; jobctr[1] = (unsigned)n_envs; jobctr[16] = 0u; jobctr[64] = 0u; jobctr[65] = 0u; jobctr[48] = jobctr[32]; jobctr[49] = jobctr[33]; jobctr[32] = 0u; jobctr[33] = 0u; }
}

}  // namespace kp
