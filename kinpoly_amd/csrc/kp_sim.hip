// kp_sim.hip -- host side of libkinpoly_sim.so: model upload, per-env state buffers, kernel launches,
// and the extern "C" entry points declared in include/kinpoly_sim.h.  No torch types anywhere.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <unistd.h>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kinpoly_sim.h"
#include "kp_model.hpp"
#include "kp_obs_kernels.hpp"
#include "kp_rollout_kernels.hpp"
#include "kp_policy_kernels.hpp"
#include "kp_step_kernel.hpp"
#include "kp_readout.hpp"
#include "kp_pose_contacts.hpp"
#include "kp_render.hpp"
#include "kp_render_ego.hpp"
#include "kp_takes.hpp"
#include "kp_kin_tape.hpp"
#include "kp_obs_ctx.hpp"

namespace {
thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }
#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define HIP_OK_NULL(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fail(std::string(#expr) + ": " + hipGetErrorString(e_)); return nullptr; } } while (0)
int launched() { HIP_OK(hipGetLastError()); return 0; }      // the status of the launches an entry point has just enqueued
}  // namespace

struct kp_model {
    kp::HostModel h;
    int contact = 1, limits = 1, stale = 1, solver_iter = 100, threads = 64, dynamic_objects = 1, lpt_order = -1, substeps_per_job = 4, queue_slots = 0, job_taper = 1, queue_fence = 1, queue_heavy = 160, queue_prio = -1, queue_late = -1, job_auto = 1, lean_queue = 1, lean_adaptive = 1, lds_pad = 0, lean_cap = kp::EnvLdsLean::MAXCON;
    double warm_extrap = -1.0;     // a float's value; < 0: automatic (0.75 when the scene's free objects are simulated, 0 otherwise); see kp_step_kernel.hpp
    int planemesh_max = 3; double planemesh_tol = 0.3;   // mjc_PlaneConvex's maxplanemesh / tolplanemesh (the blob's `planemesh`)
    int ar_obs_action = 1;        // 0: kp_sim_obs_ar writes the 101-d observation without the action one-hot (use_action: false, humanoid_ar_v1.py:200-201)
    int ar_obs_vel = 0, ar_obs_head = 1;   // use_vel: the 75 qvel after the pose block (:184-185); use_head: false drops the head-tracking blocks (:157-169, 187-198)
    // the UHC controller's observation (kp_sim_obs_cc_ex): obs_v 0 / 1 / 2, obs_vel 'root', and obs_v 0's obs_heading / root_deheading / obs_phase
    int cc_obs_v = 1, cc_obs_vel_root = 0, cc_obs_heading = 0, cc_obs_deheading = 0, cc_obs_phase = 0;
    // the UHC controller (kp_sim_step_ctrl): action_v 0 / 1, residual force off / on, meta-PD 0 none / 1 by substep / 2 by joint (humanoid_im.py:433-524)
    int cc_action_v = 1, cc_rfc = 1, cc_meta_pd = 0;
    int actuation = 1;            // 0: no stable-PD torque, no residual force (ctrl = qfrc_applied = 0): torque-free flight for the energy test
    double solver_tol = 1e-8, gravity_z = -9.81, gravity_x = 0.0, gravity_y = 0.0;   // solver_iter / solver_tol: mjOption.iterations / tolerance of the reference model (kp_model_load)
};

// kp_sim's device rows, one group per concern; kp_sim_create allocates them group by group, kp_sim::allocs owns them all
struct StateRows {        // the simulated state, its derived kinematics and the solver's warm starts
    float *qpos = nullptr, *qvel = nullptr, *qpos_d = nullptr, *qvel_d = nullptr, *warm = nullptr, *warm2 = nullptr, *warm3 = nullptr;
    float *xpos = nullptr, *xquat = nullptr, *xipos = nullptr, *prev_bquat = nullptr, *prev_hpos = nullptr;
    int* diag = nullptr;
};
struct JobQueue {         // the control-step launch: LPT order, the job FIFO of kp_step_queue_kernel, the lean layout's overflow list
    int* order = nullptr; unsigned* cost = nullptr;   // launch order of the control-step kernel (k_lpt_order)
    unsigned *jobq = nullptr, *jobctr = nullptr, *ovfq = nullptr;      // ovfq: jobs handed from the lean queue kernel to kp_step_overflow_kernel
    float* spd_next = nullptr;                        // [N, 80] torque hand-over between the jobs of a control step
    int wave_slots = 2048;
    int nsub = -1, layout = -1;                       // what the queue's "heavy job" yardstick (jobctr[32..33] -> [48..49]) was measured on
};
// how many envs the lean layout handed to the overflow kernel, read back WITHOUT waiting: every lean launch copies its count to pinned memory and records an
// event; a later launch whose predecessor's event has completed looks at the number.  When more than 1 / 64 of the envs overflow (a policy at random init resets
// every env onto a garbage pose, half buried, with 30 - 70 contacts) the overflow kernel's second pass over them costs more than the lean layout saves: the
// next 64 launches use the full layout, then the lean one is tried again.  Results do not depend on the layout.
struct OverflowReadback {
    unsigned* host = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; bool pending[2] = {false, false};
    long lean_off_until = -1; int fallbacks = 0;
    unsigned last = 0;            // the most recent count that has arrived: sizes the overflow kernel's grid (an empty 2048-workgroup launch costs 34 us)
};
struct ObjectRows {
    float *qpos = nullptr, *geoms = nullptr;          // [N,35], [N,8,17]
    float *qvel = nullptr, *warm = nullptr, *warm2 = nullptr;   // [N,30], [N,12], [N,12]
    signed char* slot = nullptr;                      // [N,2]
    int* ngeom = nullptr;
    const float* d_geoms = nullptr; const float* d_mass = nullptr; int n_geoms = 0, n_obj = 0;      // the model's object geoms / masses on the device
    bool on = false;                                  // kp_sim_set_objects / kp_sim_reset_rows installed objects: the control step runs the object kernels
};
struct Timing {
    hipEvent_t ev0 = nullptr, ev1 = nullptr, last0 = nullptr, last1 = nullptr;      // the handle's own pair; the pair of the last timed launch
    std::vector<hipEvent_t> ring;                     // event pairs of the recorded launches (kp_sim_timing_reset)
    int ring_used = 0;
    bool ring_on = false, timed = false;
};

struct RenderTables {     // the hulls' face planes (kp::hull_planes), uploaded by the first kp_sim_render / kp_sim_render_ego
    const float* planes = nullptr; const int32_t* adr = nullptr;
    float* partial = nullptr; size_t partial_n = 0;       // kp_sim_render_ego's per-tile flow sums (floats held); grows on demand
};

struct InvDynScratch {    // kp_sim_inverse_dynamics with objects: what the placement kernel (k_set_objects) writes for the call's rows; grows on demand
    float* buf = nullptr; size_t rows = 0;
};

struct MarkerScratch {    // kp_sim_fit_points: the marker set ordered by body as the kernel reads it (offsets [K,3] | perm [K] | adr [25], 4-byte words); allocated once
    static constexpr int MAXK = 1024, ZEROS = 4 * MAXK + 25, WORDS = ZEROS + 25;      // the last 25 words stay zero: the adr of a call without 3D targets (kp_sim_fit_image)
    void* buf = nullptr;
    std::vector<uint32_t> host;       // what buf holds: a call with the same marker set uploads nothing
};

struct kp_sim {
    const kp_model* model = nullptr;
    int n = 0, device = 0;
    int ar_obs_vel = 0, ar_obs_head = 1, ar_obs_action = 1;   // the model's three ar_obs_* switches when the handle was created
    int ar_obs_dim = KP_AR_OBS_DIM;                   // ar_obs_width of the three: one of the eight widths of KP_AR_OBS_WIDTHS
    int cc_obs_v = 1, cc_obs_vel_root = 0, cc_obs_heading = 0, cc_obs_deheading = 0, cc_obs_phase = 0, cc_obs_dim = KP_CC_OBS_DIM;   // the model's cc_obs_* at creation
    kp::XcArgs xc{KP_CC_ACTION_DIM, 0, 1, 0};        // the model's controller at creation; xc_on: not uhc.yml's (the extended-controller kernels, full layout)
    bool xc_on = false;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    kp::DevTables T{};
    kp::Params P{};
    float* diffw = nullptr;                           // the model's body_diffw
    StateRows st;
    kp::TargetBufs tgt{};                             // the target dict {qpos, wbpos, wbquat, bquat, body_com}
    JobQueue q;
    OverflowReadback ovf;
    ObjectRows obj;
    RenderTables rd;
    InvDynScratch idyn;
    MarkerScratch mk;
    Timing tm;
    long launch_index = 0;
    int last_nsub = 15;                               // substeps of the last control step (kp_sim_lean_state)
    unsigned long long* prof = nullptr;
    bool prof_noted = false;      // launch_step has said that profiling keeps this handle off the job queue
    float* dbg_contacts = nullptr;
    int32_t* uhc_stage = nullptr;                     // [2, N] kp_sim_uhc_assign's take ids and starts on their way to the device
};

// the take library (include/kinpoly_sim.h): tables on `device`, built with the tables of `model`
struct kp_takes {
    const kp_model* model = nullptr;
    int device = 0;
    kp::TakeTables L{};
    float* obj = nullptr;                             // [R,35] the rows' object block (kp_takes_create_obj), or null: a library without objects
    std::vector<int32_t> off;
    std::vector<void*> allocs;
};

namespace {

template <typename T, typename S>
const T* upload(kp_sim* s, const std::vector<S>& src, bool* ok) {
    std::vector<T> tmp(src.size());
    for (size_t i = 0; i < src.size(); i++) tmp[i] = (T)src[i];
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(sizeof(T) * tmp.size(), 16)) != hipSuccess) { *ok = false; return nullptr; }
    s->allocs.push_back(d);
    if (hipMemcpy(d, tmp.data(), sizeof(T) * tmp.size(), hipMemcpyHostToDevice) != hipSuccess) { *ok = false; return nullptr; }
    return (const T*)d;
}

float* dalloc(kp_sim* s, size_t count, bool* ok) {
    void* d = nullptr;
    if (hipMalloc(&d, sizeof(float) * count) != hipSuccess) { *ok = false; return nullptr; }
    s->allocs.push_back(d);
    hipMemset(d, 0, sizeof(float) * count);
    return (float*)d;
}

bool build_tables(kp_sim* s) {
    const kp::HostModel& m = s->model->h;
    using namespace kp;
    bool ok = true;
    auto& T = s->T;
    T.body_pos = upload<float>(s, m.body_pos, &ok); T.body_ipos = upload<float>(s, m.body_ipos, &ok);
    T.body_mass = upload<float>(s, m.body_mass, &ok); T.body_inertia = upload<float>(s, m.body_inertia, &ok);
    T.body_rbound = upload<float>(s, m.body_rbound, &ok); T.mesh_rbound = upload<float>(s, m.mesh_rbound, &ok);
    std::vector<double> invw(NB), liminvw(NU), lo(NU), hi(NU);
    for (int b = 0; b < NB; b++) invw[b] = m.body_invweight0[2 * b];
    for (int j = 0; j < NU; j++) { liminvw[j] = m.dof_invweight0[6 + j]; lo[j] = m.jnt_range[2 * j]; hi[j] = m.jnt_range[2 * j + 1]; }
    T.body_invw = upload<float>(s, invw, &ok); T.lim_invw = upload<float>(s, liminvw, &ok);
    T.jnt_lo = upload<float>(s, lo, &ok); T.jnt_hi = upload<float>(s, hi, &ok);
    T.dof_armature = upload<float>(s, m.dof_armature, &ok);
    T.kp = upload<float>(s, m.kp, &ok); T.kd = upload<float>(s, m.kd, &ok); T.tlim = upload<float>(s, m.torque_lim, &ok);
    T.ascale = upload<float>(s, m.a_scale, &ok);
    s->diffw = const_cast<float*>(upload<float>(s, m.body_diffw, &ok));
    T.verts = upload<float>(s, m.verts, &ok);
    T.vert_adr = upload<uint16_t>(s, m.vert_adr, &ok);
    T.vert_nbr_adr = upload<uint16_t>(s, m.vert_nbr_adr, &ok); T.vert_nbr = upload<uint8_t>(s, m.vert_nbr, &ok);
    T.dof_body = upload<uint8_t>(s, m.dof_body, &ok);
    T.body_parent = upload<int8_t>(s, m.body_parent, &ok); T.body_depth = upload<uint8_t>(s, m.body_depth, &ok);
    T.body_subtree = upload<uint8_t>(s, m.body_subtree, &ok); T.jnt_limited = upload<uint8_t>(s, m.jnt_limited, &ok);
    // layout assumptions of the kernels: bodies in DFS order (subtree(b) = [b, b + size)), body b > 0 owns dofs 6+3(b-1)..+2
    for (int b = 1; b < NB; b++) {
        if (m.body_parent[b] >= b) return false;
        for (int j = 0; j < 3; j++) if (m.dof_body[6 + 3 * (b - 1) + j] != b) return false;
    }
    for (int b = 0; b < NB; b++)
        for (int k = b + 1; k < NB; k++) {
            bool desc = false;
            for (int p = m.body_parent[k]; p >= 0; p = m.body_parent[p]) if (p == b) desc = true;
            if (desc != (k < b + m.body_subtree[b])) return false;
        }
    std::vector<int> lev_start(D_NLEV + 2, 0), lev_body;
    for (int lev = 0; lev <= D_NLEV; lev++) {
        lev_start[lev] = (int)lev_body.size();
        for (int b = 0; b < NB; b++) if (m.body_depth[b] == lev) lev_body.push_back(b);
    }
    lev_start[D_NLEV + 1] = (int)lev_body.size();
    if ((int)lev_body.size() != NB || lev_start[D_NLEV] != NB) return false;  // tree deeper than D_NLEV levels
    T.lev_start = upload<uint8_t>(s, lev_start, &ok); T.lev_body = upload<uint8_t>(s, lev_body, &ok);
    // static schedule of the 8-lanes-per-body tree passes (Lane8, kp_step_aba.hpp): lane = 8 * slot + row, 28 words per lane, built
    // here once so that the kernels load it instead of deriving it (they re-read it at the top of every solve to keep it out of the
    // registers in between)
    std::vector<unsigned> tab(64 * 28, 0u);
    unsigned multi = 0;
    for (int lev = 0; lev < D_NLEV; lev++)
        for (int i = lev_start[lev]; i < lev_start[lev + 1]; i++) {
            int nc = 0;
            for (int k = lev_body[i] + 1; k < NB; k++) if (m.body_parent[k] == lev_body[i]) nc++;
            if (nc > 3) return false;
            if (nc > 1) multi |= 1u << lev;
        }
    for (int tid = 0; tid < 64; tid++) {
        const int slot = tid >> 3, r = tid & 7;
        unsigned long long sb = 0, sp = 0, sc[3] = {0, 0, 0};
        for (int lev = 0; lev < D_NLEV; lev++) {
            const int nb = lev_start[lev + 1] - lev_start[lev];
            if (nb > 8) return false;
            unsigned long long b = 31, par = 31, ch[3] = {24, 24, 24};      // no body in this slot: 31; absent child: the zero record 24
            if (slot < nb) {
                const int body = lev_body[lev_start[lev] + slot];
                b = (unsigned)body; par = m.body_parent[body] < 0 ? 31u : (unsigned)m.body_parent[body];
                int nc = 0;
                for (int k = body + 1; k < NB; k++) if (m.body_parent[k] == body) ch[nc++] = (unsigned)k;
            }
            sb |= b << (5 * lev); sp |= par << (5 * lev);
            for (int c = 0; c < 3; c++) sc[c] |= ch[c] << (5 * lev);
        }
        unsigned* w = tab.data() + 28 * tid;
        w[0] = (unsigned)sb; w[1] = (unsigned)(sb >> 32); w[2] = (unsigned)sp; w[3] = (unsigned)(sp >> 32);
        for (int c = 0; c < 3; c++) { w[4 + 2 * c] = (unsigned)sc[c]; w[5 + 2 * c] = (unsigned)(sc[c] >> 32); }
        w[10] = multi;
        for (int k = 0; k < 8; k++) {
            const int kx = k < 4 ? k : 11 - k;          // XOR order {0,1,2,3,7,6,5,4}: register k holds column r ^ kx
            const int c = r ^ kx;
            int idx = 0; float sg = 0.f;
            if (r < 6 && c < 6) {                       // entry (r, c) of the 6x6 spatial inertia from the 10 floats [Ixx Iyy Izz Ixy Ixz Iyz | h | m]
                if (r < 3 && c < 3) { idx = (r == c) ? r : r + c + 2; sg = 1.f; }
                else if (r >= 3 && c >= 3) { idx = 9; sg = (r == c) ? 1.f : 0.f; }
                else {
                    const int a = r < 3 ? r : c, l = (r < 3 ? c : r) - 3;   // [h]x(a, l)
                    if (a != l) { idx = 6 + (3 - a - l); sg = (l == (a + 2) % 3) ? 1.f : -1.f; }
                }
            }
            const int rr = r < c ? r : c, cc = r < c ? c : r;
            const int idx21 = (r < 6 && c < 6) ? (rr * (13 - rr)) / 2 + (cc - rr) : 21;   // 21 = the always-zero slot of a record
            w[12 + k] = (unsigned)c | ((unsigned)idx << 4) | ((unsigned)idx21 << 8);
            std::memcpy(&w[20 + k], &sg, 4);
        }
    }
    T.sched8 = upload<uint32_t>(s, tab, &ok);
    T.obj_inertial = nullptr; T.obj_geoms = nullptr; T.obj_geom_adr = nullptr; T.n_obj = 0;
    if (!m.obj_geoms.empty() && m.obj_inertial.size() == 13 * m.obj_mass.size()) {
        T.obj_inertial = upload<float>(s, m.obj_inertial, &ok); T.obj_geoms = upload<float>(s, m.obj_geoms, &ok);
        T.obj_geom_adr = upload<int>(s, m.obj_geom_adr, &ok); T.n_obj = (int)m.obj_mass.size();
    }
    // scalar parameters
    auto& P = s->P;
    const auto& o = m.opt;
    auto clampimp = [](double v) { return std::min(0.9999, std::max(0.0001, v)); };
    P.h = (float)o[OPT_TIMESTEP]; P.gx = (float)s->model->gravity_x; P.gy = (float)s->model->gravity_y; P.gz = (float)s->model->gravity_z;
    double tc = std::max(o[OPT_SOLREF_TC], 2 * o[OPT_TIMESTEP]), dr = o[OPT_SOLREF_DR], dmax = clampimp(o[OPT_IMP_DW]);
    P.K = (float)(1.0 / (dmax * dmax * tc * tc * dr * dr)); P.B = (float)(2.0 / (dmax * tc));
    P.imp_d0 = (float)clampimp(o[OPT_IMP_D0]); P.imp_dw = (float)dmax; P.imp_w = (float)o[OPT_IMP_W];
    P.imp_mid = (float)clampimp(o[OPT_IMP_MID]); P.imp_pow = (float)std::max(1.0, o[OPT_IMP_POW]);
    P.mu = (float)o[OPT_FRIC]; P.margin = (float)o[OPT_MARGIN];
    P.pm_max = s->model->planemesh_max; P.pm_tol = (float)s->model->planemesh_tol;
    // mj_solNewton's termination scale: mean inertia and dof count of the WHOLE reference scene (objects included)
    P.scale = (float)(1.0 / (o[OPT_MEANINERTIA] * (o.size() > OPT_NV_FULL ? o[OPT_NV_FULL] : NV)));
    P.rfc_scale = (float)o[OPT_RFC_SCALE]; P.rfc_lim = (float)o[OPT_RFC_LIM];
    double bn = o[OPT_BR_W] * o[OPT_BR_W] + o[OPT_BR_X] * o[OPT_BR_X] + o[OPT_BR_Y] * o[OPT_BR_Y] + o[OPT_BR_Z] * o[OPT_BR_Z];
    P.br_inv[0] = (float)(o[OPT_BR_W] / bn); P.br_inv[1] = (float)(-o[OPT_BR_X] / bn);
    P.br_inv[2] = (float)(-o[OPT_BR_Y] / bn); P.br_inv[3] = (float)(-o[OPT_BR_Z] / bn);
    P.tol = (float)s->model->solver_tol; P.max_iter = s->model->solver_iter;
    P.contact = s->model->contact; P.limits = s->model->limits; P.stale = s->model->stale; P.actuation = s->model->actuation;
    return ok;
}

// Job sizes of kp_step_queue_kernel for a control step of nsub substeps: `spj` substeps for the last job and `taper` more for each job
// before it -- the FIFO runs all envs' first jobs, then all second jobs ...: long jobs first keep the hand-overs few, short jobs
// last keep the end of the launch short -- what is left over becomes the first job (or joins it if shorter than spj); at most 16 jobs.
// Default (spj 4, taper 1): 15 = 6 + 5 + 4.
int job_schedule(int nsub, int spj, int taper, int* sizes) {
    int parts = 0, rem = nsub, size = spj;
    while (rem > 0 && parts < 16) {
        int take = parts == 15 ? rem : std::min(rem, size);
        if (rem - take > 0 && rem - take < spj) take = rem;
        sizes[parts++] = take; rem -= take;
        size += taper;
    }
    std::reverse(sizes, sizes + parts);
    return parts;
}

// The lean layout (EnvLdsLean) serves floor scenes in stale mode only: its pAa shares words with jv3 | lim_jv, which in fresh mode (stale_kinematics = 0)
// hold make_constraint's aref while the substep's aba_solve writes pAa (kp_device.hpp).  P.stale: the value the kernel receives.
// (the extended controller has no lean-layout instantiation: plan_step sends it to the full layout)
bool lean_eligible(const kp_sim& s) { return !s.obj.on && s.model->lean_queue && s.model->threads == 64 && s.P.stale && !s.xc_on; }

// resident envs per CU: LDS is allocated in 1 280-byte granules, 128 per CU (tools/micro/lds_granule_probe.hip); the register budgets allow 8 waves per CU
// (full layout, <= 256 VGPRs) and 12 (lean layout, 168 VGPRs)
int envs_per_cu(size_t lds_bytes, int reg_cap) { return std::min(reg_cap, 128 / (int)((lds_bytes + 1279) / 1280)); }

// the adaptive lean / full fallback (OverflowReadback): take the overflow counts that have arrived; a failed query ends the slot's wait and fails the step
int poll_overflow(kp_sim* s) {
    for (int k = 0; k < 2; k++) {
        if (!s->ovf.pending[k]) continue;
        const hipError_t e = hipEventQuery(s->ovf.ev[k]);
        if (e == hipErrorNotReady) continue;
        s->ovf.pending[k] = false;
        if (e != hipSuccess) return fail(std::string("hipEventQuery(ovf_ev): ") + hipGetErrorString(e));
        s->ovf.last = s->ovf.host[k];
        if ((size_t)s->ovf.host[k] * 64 > (size_t)s->n) { s->ovf.lean_off_until = s->launch_index + 64; s->ovf.fallbacks++; }
    }
    return 0;
}

enum Layout { FULL = 0, OBJECTS = 1, LEAN = 2 };      // EnvLds, EnvLdsObj, EnvLdsLean
// What one launch_step runs, from the handle's options and state alone (no HIP calls, no writes): launch_step launches it, kp_sim_lean_state reports it.
struct StepPlan {
    bool queue, lpt;      // the job queue (kp_step_queue_kernel on `slots` resident waves) instead of one workgroup per env; k_lpt_order first
    bool prof_per_env;    // the job queue would run, but the handle is profiled (KP_PROFILE=1) and the phase profiler exists in the one-workgroup-per-env kernels only
    Layout layout;        // the queue's LDS layout (one workgroup per env runs on FULL or OBJECTS)
    int threads, slots, parts, sizes[16], queue_prio, queue_late, ovf_grid;      // ovf_grid: workgroups of kp_step_overflow_kernel
    size_t lds;           // dynamic LDS bytes of the step kernel
};

StepPlan plan_step(const kp_sim& s, int nsub, bool capturing) {
    const kp_model& m = *s.model;
    StepPlan p{};
    // floor scenes: the job queue runs on the lean layout (EnvLdsLean) with a register budget for three waves per SIMD, except during a fallback (poll_overflow);
    // model option lean_queue = 0 keeps the full layout (two waves per SIMD; A / B measurements)
    bool lean = lean_eligible(s);
    if (lean && nsub > 0 && s.ovf.host && !capturing && m.lean_adaptive && s.launch_index < s.ovf.lean_off_until) lean = false;
    p.layout = s.obj.on ? OBJECTS : lean ? LEAN : FULL;
    p.threads = m.threads;
    // lpt_order: 1 on, 0 off, -1 (default) on when the scene's objects are simulated: an env whose hulls press on objects stays the launch's
    // longest for many control steps, so starting it first shortens the launch (objects workload 7.21 -> 6.62 ms); floor-only costs are not
    // predictable from step to step (correlation 0.25 .. 0.55) and gain nothing
    p.lpt = nsub > 0 && (m.lpt_order > 0 || (m.lpt_order < 0 && s.obj.on));
    // lds_pad: allocate at least that many bytes per env (experiments: fewer envs per CU with the same binary)
    const size_t lds = s.obj.on ? sizeof(kp::EnvLdsObj) : sizeof(kp::EnvLds);
    size_t lds_q = lean ? sizeof(kp::EnvLdsLean) : lds;
    if (m.lds_pad > 0) lds_q = std::max(lds_q, (size_t)m.lds_pad);
    p.slots = m.queue_slots > 0 ? m.queue_slots : s.q.wave_slots / 8 * envs_per_cu(lds_q, lean ? 12 : 8);
    // Schedule defaults.  Full layout (objects; floor with lean_queue = 0): 6 + 5 + 4 substeps, FIFO, no issue priorities (rounds 2 - 5).  Lean layout: 3072 slots hold
    // three quarters of BASELINE's 4096 envs, so a quarter of the envs start one job late and the launch ends on them (sum of env cycles / slots 1.83 ms, launch
    // 2.44 ms).  Three measures take the launch to 2.19 ms (profiles/r06/lean_schedule_knobs*.log): equal jobs 5 + 5 + 5 (the late envs start earlier), a late
    // env is never queued again (queue_late), and every wave's issue priority follows its env's distance from the end of the control step (queue_prio = 3).
    // Options the caller sets (substeps_per_job / job_taper, queue_prio, queue_late) are obeyed.
    const bool lean_auto = lean && m.job_auto;
    const int spj = lean_auto ? 5 : m.substeps_per_job, taper = lean_auto ? 0 : m.job_taper;
    if (spj > 0 && nsub > 0) {
        p.parts = job_schedule(nsub, spj, taper, p.sizes);
        if (const char* e = std::getenv("KP_JOB_SCHEDULE")) {      // experiments: explicit comma-separated job sizes
            int tmp[16], np = 0, sum = 0;
            for (const char* c = e; *c && np < 16;) { tmp[np] = std::atoi(c); sum += tmp[np++]; while (*c && *c != ',') c++; if (*c) c++; }
            if (sum == nsub) { p.parts = np; std::copy(tmp, tmp + np, p.sizes); }
        }
    }
    // more envs than resident wave slots: schedule the control step as jobs pulled from a FIFO by one resident wave per slot instead of one workgroup per env,
    // which ends on a long tail.  The queue pays from the env count on that one-workgroup-per-env launches (full layout) cannot hold resident at once; the lean
    // queue then runs with every env resident up to its own slot count and in rounds beyond it.  Env ids take 24 bits of a queue entry.
    const int resident_full = s.q.wave_slots / 8 * envs_per_cu(lds, 8);
    const bool queue = nsub > 0 && p.parts > 1 && m.threads == 64 && s.n > std::min(p.slots, resident_full) && s.n <= 0xFFFFFF;
    p.queue = queue && !s.prof; p.prof_per_env = queue && s.prof;
    p.lds = p.queue ? lds_q : lds;
    p.queue_prio = m.queue_prio >= 0 ? m.queue_prio : (lean ? 3 : 0);
    p.queue_late = m.queue_late >= 0 ? m.queue_late : (lean ? 1 : 0);
    // overflow kernel: twice the overflow count last seen (the scenes that overflow keep doing so for a while), at least 128 workgroups -- an unexpected burst
    // is slow once and sized right from the next-but-one launch on; launching full residency every time costs 34 us per control step for nothing
    p.ovf_grid = std::min(std::min(s.n, resident_full), std::max(128, 2 * (int)std::min<unsigned>(s.ovf.last, 1u << 20)));
    return p;
}

// one workgroup of NT threads per env: the control step, or (nsub = 0) the forward pass alone
template <int NT, bool OBJ>
void launch_per_env(const kp_sim* s, const kp::StepArgs& A, int nsub, size_t lds) {
    // a profiled handle (KP_PROFILE=1) runs the instantiations that carry the phase profiler; plan_step keeps it on this launch form
    if (nsub > 0 && s->prof && s->xc_on) hipLaunchKernelGGL((kp::kp_step_kernel_xc<NT, OBJ, true>), dim3(s->n), dim3(NT), lds, s->stream, A, s->xc);
    else if (nsub > 0 && s->prof) hipLaunchKernelGGL((kp::kp_step_kernel<NT, OBJ, true>), dim3(s->n), dim3(NT), lds, s->stream, A);
    else if (nsub > 0 && s->xc_on) hipLaunchKernelGGL((kp::kp_step_kernel_xc<NT, OBJ>), dim3(s->n), dim3(NT), lds, s->stream, A, s->xc);
    else if (nsub > 0) hipLaunchKernelGGL((kp::kp_step_kernel<NT, OBJ>), dim3(s->n), dim3(NT), lds, s->stream, A);
    else hipLaunchKernelGGL((kp::kp_forward_kernel<NT, OBJ>), dim3(s->n), dim3(NT), lds, s->stream, A);
}

// the timed bracket of a launch: the handle's event pair, or the next pair of the ring while kp_sim_timing_reset's recording is on
int timing_begin(kp_sim* s, hipEvent_t* e0, hipEvent_t* e1) {
    Timing& t = s->tm;
    *e0 = t.ev0; *e1 = t.ev1;
    if (t.ring_on && t.ring_used < 4096) {
        if ((int)t.ring.size() < 2 * (t.ring_used + 1)) {
            hipEvent_t a, b;
            HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
            t.ring.push_back(a); t.ring.push_back(b);
        }
        *e0 = t.ring[2 * t.ring_used]; *e1 = t.ring[2 * t.ring_used + 1];
        t.ring_used++;
    }
    HIP_OK(hipEventRecord(*e0, s->stream));
    return 0;
}
int timing_end(kp_sim* s, hipEvent_t e0, hipEvent_t e1) {
    HIP_OK(hipEventRecord(e1, s->stream));
    s->tm.last0 = e0; s->tm.last1 = e1; s->tm.timed = true;
    return 0;
}

// the step kernels' argument pack for plan p; base_qpos (optional): compute_torque's base pose for this launch instead of the stored target
kp::StepArgs step_args(const kp_sim* s, const StepPlan& p, int nsub, const float* action, const uint8_t* mask, const float* base_qpos) {
    const kp_model& m = *s->model;
    const StateRows& st = s->st; const ObjectRows& o = s->obj; const JobQueue& q = s->q;
    kp::StepArgs A{};
    A.T = s->T; A.P = s->P; A.n_envs = s->n; A.n_substeps = nsub;
    A.qpos = st.qpos; A.qvel = st.qvel; A.qpos_d = st.qpos_d; A.qvel_d = st.qvel_d; A.warm = st.warm; A.warm2 = st.warm2; A.warm3 = st.warm3;
    A.target_qpos = base_qpos ? base_qpos : s->tgt.qpos; A.action = action; A.env_mask = mask;
    A.xpos = st.xpos; A.xquat = st.xquat; A.xipos = st.xipos; A.diag = st.diag; A.prof = s->prof; A.dbg_contacts = s->dbg_contacts;
    A.geoms = o.geoms; A.ngeom = o.ngeom; A.obj_slot = o.slot; A.obj_qpos = o.qpos; A.obj_qvel = o.qvel; A.obj_warm = o.warm; A.obj_warm2 = o.warm2;
    A.warm_extrap = m.warm_extrap < 0 ? (o.on ? 0.75f : 0.f) : (float)m.warm_extrap;      // the Newton solve's starting point (kp_step_kernel.hpp)
    A.order = p.lpt ? q.order : nullptr; A.order_valid = p.lpt; A.cost = q.cost;
    A.jobq = q.jobq; A.jobctr = q.jobctr; A.ovfq = q.ovfq; A.spd_next = q.spd_next; A.lean_cap = m.lean_cap;
    A.n_parts = p.queue ? p.parts : 1; A.queue_fence = m.queue_fence; A.queue_heavy = m.queue_heavy; A.queue_prio = p.queue_prio; A.queue_late = p.queue_late;
    for (int k = 0; p.queue && k < p.parts; k++) (k < 8 ? A.part_sub_lo : A.part_sub_hi) |= (unsigned long long)(p.sizes[k] & 255) << (8 * (k & 7));
    return A;
}

// the control step as jobs pulled from a FIFO by resident waves (plan p.queue)
int launch_queue(kp_sim* s, const StepPlan& p, kp::StepArgs& A, int nsub, bool capturing) {
    JobQueue& q = s->q;
    // the yardstick of queue_heavy is the previous launch's mean job time per substep: it only means something for the same kernel on the same
    // schedule, so a change of the substep count or of the kernel instantiation starts it from nothing (that launch keeps no env)
    if (nsub != q.nsub || (int)p.layout != q.layout) {
        HIP_OK(hipMemsetAsync(q.jobctr + 32, 0, 2 * sizeof(unsigned), s->stream));
        q.nsub = nsub; q.layout = (int)p.layout;
    }
    const unsigned total = (unsigned)s->n * (unsigned)p.parts;
    hipLaunchKernelGGL(kp::k_queue_init, dim3((total + 255) / 256), dim3(256), 0, s->stream, s->n, total, q.jobq, q.jobctr, A.order);   // inside the timed bracket
    A.order = nullptr;                                              // the queue kernel addresses envs by their queue entry
    if (s->xc_on && p.layout == OBJECTS) hipLaunchKernelGGL((kp::kp_step_queue_kernel_xc<true>), dim3(p.slots), dim3(64), p.lds, s->stream, A, s->xc);
    else if (s->xc_on) hipLaunchKernelGGL((kp::kp_step_queue_kernel_xc<false>), dim3(p.slots), dim3(64), p.lds, s->stream, A, s->xc);
    else if (p.layout == OBJECTS) hipLaunchKernelGGL((kp::kp_step_queue_kernel<true>), dim3(p.slots), dim3(64), p.lds, s->stream, A);
    else if (p.layout == FULL) hipLaunchKernelGGL((kp::kp_step_queue_kernel<false>), dim3(p.slots), dim3(64), p.lds, s->stream, A);
    else {
        hipLaunchKernelGGL((kp::kp_step_queue_kernel<false, true>), dim3(p.slots), dim3(64), p.lds, s->stream, A);
        // the jobs whose contacts did not fit the lean layout (normally none: every wave leaves at its first read)
        hipLaunchKernelGGL(kp::kp_step_overflow_kernel, dim3(p.ovf_grid), dim3(64), sizeof(kp::EnvLds), s->stream, A);
        const int k = (int)(s->launch_index & 1);
        if (s->ovf.host && !capturing && !s->ovf.pending[k]) {
            HIP_OK(hipMemcpyAsync(s->ovf.host + k, q.jobctr + 64, sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
            HIP_OK(hipEventRecord(s->ovf.ev[k], s->stream));
            s->ovf.pending[k] = true;
        }
    }
    return 0;
}

// one control step (nsub > 0) or the forward pass alone (nsub = 0) of the masked envs: timing bracket, plan, argument pack, launch
int launch_step(kp_sim* s, const float* action, int nsub, const uint8_t* mask, bool time_it, const float* base_qpos = nullptr) {
    const int threads = s->model->threads;
    if (s->obj.on && threads != 64) return fail("object contact needs threads_per_env = 64");
    if (threads != 64 && threads != 128 && threads != 256) return fail("threads_per_env must be 64, 128 or 256");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    time_it = time_it && !capturing;      // a launch that is being captured into a hipGraph carries no timing events (they could not be read back)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (time_it && timing_begin(s, &e0, &e1)) return -1;
    if (nsub > 0 && s->ovf.host && !capturing && lean_eligible(*s) && poll_overflow(s)) return -1;
    const StepPlan p = plan_step(*s, nsub, capturing);
    if (nsub > 0) { s->launch_index++; s->last_nsub = nsub; }
    if (p.prof_per_env && !s->prof_noted) {      // said once per handle: the figures of kp_sim_phase_cycles are those of another launch form than the unprofiled handle's
        std::fprintf(stderr, "kp_sim: KP_PROFILE=1: the job-queue kernels carry no phase profiler; this handle's control steps run one workgroup per env "
                             "(kp_step_kernel), whose profiling instantiation fills kp_sim_phase_cycles\n");
        s->prof_noted = true;
    }
    kp::StepArgs A = step_args(s, p, nsub, action, mask, base_qpos);
    // longest env first (inside the timed bracket): order the workgroups / the queue's first jobs by the cycles of the previous control step
    if (p.lpt) hipLaunchKernelGGL(kp::k_lpt_order, dim3(1), dim3(1024), 0, s->stream, s->n, s->q.cost, s->q.order);
    if (p.queue) { if (launch_queue(s, p, A, nsub, capturing)) return -1; }
    else if (s->obj.on) launch_per_env<64, true>(s, A, nsub, p.lds);
    else if (p.threads == 64) launch_per_env<64, false>(s, A, nsub, p.lds);
    else if (p.threads == 128) launch_per_env<128, false>(s, A, nsub, p.lds);
    else launch_per_env<256, false>(s, A, nsub, p.lds);
    HIP_OK(hipGetLastError());
    return time_it ? timing_end(s, e0, e1) : 0;
}

// the target dict's forward kinematics of n rows of tq into B; K (optional): the head of the env step in the same launch (kp_sim_step_head)
void launch_target_fk(const kp_sim* s, int n, const float* tq, const uint8_t* mask, const kp::TargetBufs& B,
                      const kp::KinStep& K = kp::KinStep{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f}) {
    hipLaunchKernelGGL(kp::k_target_fk, dim3((n + 3) / 4), dim3(256), 0, s->stream, n, tq, mask, B, s->T.body_pos, s->T.body_ipos, s->T.body_parent, s->T.body_depth, K);
}

}  // namespace

extern "C" {

const char* kp_last_error(void) { return g_err.c_str(); }
const char* kp_version(void) { return "kinpoly_sim 0.1 (gfx950)"; }

kp_model* kp_model_load(const char* path) {
    kp_model* m = new kp_model();
    if (!kp::load_kpm(path, m->h)) { fail("kp_model_load: " + m->h.error); delete m; return nullptr; }
    m->gravity_z = m->h.opt[kp::OPT_GZ]; m->gravity_x = m->h.opt[kp::OPT_GX]; m->gravity_y = m->h.opt[kp::OPT_GY];
    m->solver_tol = m->h.opt[kp::OPT_SOLVER_TOL];
    m->solver_iter = (int)m->h.opt[kp::OPT_SOLVER_ITER];      // 100: MuJoCo's default, which the reference never overrides
    if (m->solver_iter < 1) m->solver_iter = 100;
    m->planemesh_max = (int)m->h.planemesh[0]; m->planemesh_tol = m->h.planemesh[1];
    return m;
}
void kp_model_free(kp_model* m) { delete m; }

// width of the action row kp_sim_step_ctrl reads for these controller options (HumanoidEnv.set_spaces, humanoid_im.py:68-89)
static int cc_action_width(int rfc, int meta) { return 69 + 6 * rfc + (meta == 1 ? 30 : meta == 2 ? 138 : 0); }

// width of the observation kp_sim_obs_cc_ex writes for these switches (kp::ObsCcLayout)
static int cc_obs_width(int v, int vel_root, int heading, int phase) {
    const int lv = vel_root ? 6 : 75;
    return v == 0 ? heading + 74 + lv + 69 + phase : 229 + lv + (v == 1 ? 4 : 2) * 72 + 2 * 96;
}

// width of the observation kp_sim_obs_ar writes for these switches (kp::ObsArLayout; the table next to KP_AR_OBS_DIM in include/kinpoly_sim.h)
static int ar_obs_width(int vel, int head, int action) { return 74 + 75 * vel + 7 * head + 7 + 13 * head + 4 * action; }
static bool ar_obs_width_known(int d) {
    for (int k = 0; k < 8; k++) if (d == ar_obs_width(k & 1, (k >> 1) & 1, (k >> 2) & 1)) return true;
    return false;
}
#define KP_AR_OBS_WIDTHS "105, 101, 180, 176, 85, 81, 160 or 156"

// ---- model options: ONE table behind kp_model_set_option and kp_model_get_option (include/kinpoly_sim.h describes what each option does).
// A settable option lives in an int or a double member of kp_model; how a value is accepted:
// O_BOOL: v != 0;  O_TRI: -1 (v < 0: automatic) / 0 / 1;  O_INT: (int)v and O_REAL: v, unchecked;  O_REAL32: v rounded to float;  O_ENUM: one of the integers
// 0 .. hi or refused;  O_RANGE: lo <= v <= hi or refused (an int member stores (int)v);  O_CLAMP: (int)v clamped to lo .. hi;  O_THREADS: 64, 128 or 256;
// O_READ_ONLY: derived, `get` computes it and set does not know the name.
enum OptRule { O_BOOL, O_TRI, O_INT, O_REAL, O_REAL32, O_ENUM, O_RANGE, O_CLAMP, O_THREADS, O_READ_ONLY };
struct Opt {
    const char* name;
    OptRule rule;
    int kp_model::*i; double kp_model::*d;
    double lo, hi;
    const char* must;                    // the refusal reads "<name> must be <must>"; null: "0 or 1" (O_ENUM), "<lo> .. <hi>" (O_RANGE)
    bool clears_job_auto;                // the caller's own job sizes switch the layout's default schedule off (plan_step)
    double (*get)(const kp_model&);      // O_READ_ONLY
};
constexpr double INF = HUGE_VAL;
#define OPT_I(name, rule, member, ...) Opt{name, rule, &kp_model::member, nullptr, __VA_ARGS__}
#define OPT_D(name, rule, member, ...) Opt{name, rule, nullptr, &kp_model::member, __VA_ARGS__}
#define OPT_RO(name, expr) Opt{name, O_READ_ONLY, nullptr, nullptr, 0, 0, nullptr, false, [](const kp_model& m) -> double { return expr; }}
static const Opt OPTIONS[] = {
    OPT_I("contact", O_BOOL, contact), OPT_I("limits", O_BOOL, limits), OPT_I("actuation", O_BOOL, actuation), OPT_I("stale_kinematics", O_BOOL, stale),
    OPT_D("gravity_z", O_REAL, gravity_z), OPT_D("gravity_x", O_REAL, gravity_x), OPT_D("gravity_y", O_REAL, gravity_y),
    OPT_I("solver_iter", O_INT, solver_iter), OPT_D("solver_tol", O_REAL, solver_tol), OPT_I("dynamic_objects", O_BOOL, dynamic_objects),
    OPT_I("planemesh_max", O_RANGE, planemesh_max, 1, 8), OPT_D("planemesh_tol", O_RANGE, planemesh_tol, 0, INF, ">= 0"),
    OPT_I("threads_per_env", O_THREADS, threads, 0, 0, "64, 128 or 256"),
    OPT_D("warm_extrap", O_REAL32, warm_extrap),
    // the kinematic policy's and the UHC's observation and controller (fixed in a kp_sim when it is created)
    OPT_I("ar_obs_action", O_ENUM, ar_obs_action, 0, 1, "1 (105-d observation with the action one-hot) or 0 (101-d, use_action: false)"),
    OPT_I("ar_obs_vel", O_ENUM, ar_obs_vel, 0, 1, "0 (no velocities) or 1 (use_vel: the 75 qvel follow the pose block)"),
    OPT_I("ar_obs_head", O_ENUM, ar_obs_head, 0, 1, "1 (with the head-tracking blocks) or 0 (use_head: false)"),
    OPT_RO("ar_obs_dim", ar_obs_width(m.ar_obs_vel, m.ar_obs_head, m.ar_obs_action)),
    OPT_I("cc_obs_v", O_ENUM, cc_obs_v, 0, 2, "0 (get_full_obs), 1 (get_full_obs_v1) or 2 (get_full_obs_v2)"),
    OPT_I("cc_obs_vel_root", O_ENUM, cc_obs_vel_root, 0, 1), OPT_I("cc_obs_heading", O_ENUM, cc_obs_heading, 0, 1),
    OPT_I("cc_obs_deheading", O_ENUM, cc_obs_deheading, 0, 1), OPT_I("cc_obs_phase", O_ENUM, cc_obs_phase, 0, 1),
    OPT_RO("cc_obs_dim", m.cc_obs_v == 0 ? cc_obs_width(0, m.cc_obs_vel_root, m.cc_obs_heading, m.cc_obs_phase) : cc_obs_width(m.cc_obs_v, m.cc_obs_vel_root, 0, 0)),
    OPT_I("cc_action_v", O_ENUM, cc_action_v, 0, 1), OPT_I("cc_rfc", O_ENUM, cc_rfc, 0, 1),
    OPT_I("cc_meta_pd", O_ENUM, cc_meta_pd, 0, 2, "0 (none), 1 (meta_pd: by substep) or 2 (meta_pd_joint: by joint)"),
    OPT_RO("cc_action_dim", cc_action_width(m.cc_rfc, m.cc_meta_pd)),
    OPT_RO("n_obj_geoms", (double)(m.h.obj_geoms.size() / 18)),     // columns of kp_sim_pose_contacts' hits
    OPT_RO("timestep", m.h.opt[kp::OPT_TIMESTEP]),
    // scheduling of the control-step launch (results do not depend on it)
    OPT_I("lpt_order", O_TRI, lpt_order),
    OPT_I("substeps_per_job", O_RANGE, substeps_per_job, 0, 255, "0 (whole control step per workgroup) .. 255", true),
    OPT_I("job_taper", O_CLAMP, job_taper, 0, 8, nullptr, true),
    OPT_RO("job_auto", m.job_auto),       // 1: the job sizes are the layout's defaults (lean queue: 5 + 5 + 5; otherwise substeps_per_job / job_taper = 6 + 5 + 4)
    OPT_I("queue_slots", O_RANGE, queue_slots, 0, INF, ">= 0 (0 = resident wave slots of the device)"),
    OPT_I("queue_fence", O_BOOL, queue_fence), OPT_I("queue_heavy", O_CLAMP, queue_heavy, 0, INT_MAX),
    OPT_I("queue_late", O_TRI, queue_late), OPT_I("queue_prio", O_CLAMP, queue_prio, -1, 3),
    OPT_I("lean_queue", O_BOOL, lean_queue), OPT_I("lean_adaptive", O_BOOL, lean_adaptive),
    OPT_I("lean_max_contacts", O_RANGE, lean_cap, 0, kp::EnvLdsLean::MAXCON),
    OPT_I("lds_pad", O_RANGE, lds_pad, 0, 65536, "0 .. 65536 bytes"),
    OPT_RO("lds_bytes_per_env", (double)sizeof(kp::EnvLds)), OPT_RO("lds_bytes_per_env_objects", (double)sizeof(kp::EnvLdsObj)),
    OPT_RO("lds_bytes_per_env_lean", (double)sizeof(kp::EnvLdsLean)),
};
#undef OPT_I
#undef OPT_D
#undef OPT_RO
static const Opt* find_option(const char* name) {
    for (const Opt& o : OPTIONS) if (name && !std::strcmp(name, o.name)) return &o;
    return nullptr;
}

int kp_model_set_option(kp_model* m, const char* name, double v) {
    if (!m || !name) return fail("kp_model_set_option: null argument");
    const Opt* o = find_option(name);
    if (!o || o->rule == O_READ_ONLY) return fail(std::string("kp_model_set_option: unknown option ") + name);
    bool ok = true;
    double x = v;
    switch (o->rule) {
        case O_BOOL: x = v != 0; break;
        case O_TRI: x = v < 0 ? -1 : (v != 0); break;
        case O_REAL32: x = (float)v; break;
        case O_ENUM: ok = false; for (int k = 0; k <= (int)o->hi; k++) ok = ok || v == k; break;
        case O_RANGE: ok = !(v < o->lo || v > o->hi); break;
        case O_CLAMP: x = std::max((int)o->lo, std::min((int)o->hi, (int)v)); break;
        case O_THREADS: ok = v == 64 || v == 128 || v == 256; break;
        default: break;
    }
    if (!ok) {
        const std::string must = o->must ? o->must : o->rule == O_ENUM ? "0 or 1" : std::to_string((int)o->lo) + " .. " + std::to_string((int)o->hi);
        return fail(std::string(name) + " must be " + must);
    }
    if (o->i) m->*(o->i) = (int)x; else m->*(o->d) = x;
    if (o->clears_job_auto) m->job_auto = 0;
    return 0;
}
double kp_model_get_option(const kp_model* m, const char* name) {
    const Opt* o = find_option(name);
    if (!m || !o) return NAN;
    return o->get ? o->get(*m) : o->i ? (double)(m->*(o->i)) : m->*(o->d);
}

kp_sim* kp_sim_create(const kp_model* m, int n_envs, int device_id, void* stream) {
    if (!m || n_envs <= 0) { fail("kp_sim_create: bad arguments"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("kp_sim_create: no HIP device available (the simulator has no CPU fallback)"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(device_id));
    kp_sim* s = new kp_sim();
    s->model = m; s->n = n_envs; s->device = device_id; s->stream = (hipStream_t)stream;
    s->ar_obs_vel = m->ar_obs_vel; s->ar_obs_head = m->ar_obs_head; s->ar_obs_action = m->ar_obs_action;
    s->ar_obs_dim = ar_obs_width(s->ar_obs_vel, s->ar_obs_head, s->ar_obs_action);
    s->cc_obs_v = m->cc_obs_v; s->cc_obs_vel_root = m->cc_obs_vel_root;
    s->cc_obs_heading = m->cc_obs_v == 0 && m->cc_obs_heading; s->cc_obs_deheading = m->cc_obs_v == 0 && m->cc_obs_deheading; s->cc_obs_phase = m->cc_obs_v == 0 && m->cc_obs_phase;
    s->cc_obs_dim = cc_obs_width(s->cc_obs_v, s->cc_obs_vel_root, s->cc_obs_heading, s->cc_obs_phase);
    s->xc = kp::XcArgs{cc_action_width(m->cc_rfc, m->cc_meta_pd), m->cc_action_v == 0, m->cc_rfc, m->cc_meta_pd};
    s->xc_on = m->cc_action_v != 1 || m->cc_rfc != 1 || m->cc_meta_pd != 0;
    bool ok = build_tables(s);
    const size_t N = n_envs;
    StateRows& st = s->st;
    st.qpos = dalloc(s, N * 76, &ok); st.qvel = dalloc(s, N * 75, &ok); st.qpos_d = dalloc(s, N * 76, &ok); st.qvel_d = dalloc(s, N * 75, &ok);
    st.warm = dalloc(s, N * 75, &ok); st.warm2 = dalloc(s, N * 75, &ok); st.warm3 = dalloc(s, N * 75, &ok);
    st.xpos = dalloc(s, N * 72, &ok); st.xquat = dalloc(s, N * 96, &ok); st.xipos = dalloc(s, N * 72, &ok);
    st.prev_bquat = dalloc(s, N * 96, &ok); st.prev_hpos = dalloc(s, N * 7, &ok); st.diag = (int*)dalloc(s, N * 4, &ok);
    s->tgt = kp::TargetBufs{dalloc(s, N * 76, &ok), dalloc(s, N * 72, &ok), dalloc(s, N * 96, &ok), dalloc(s, N * 96, &ok), dalloc(s, N * 72, &ok)};
    JobQueue& q = s->q;
    q.order = (int*)dalloc(s, N, &ok); q.cost = (unsigned*)dalloc(s, N, &ok);
    q.jobq = (unsigned*)dalloc(s, N * 16, &ok); q.jobctr = (unsigned*)dalloc(s, 128, &ok); q.ovfq = (unsigned*)dalloc(s, N, &ok);
    q.spd_next = dalloc(s, N * 80, &ok);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->device) == hipSuccess && prop.multiProcessorCount > 0) q.wave_slots = prop.multiProcessorCount * 8;
    ObjectRows& o = s->obj;
    o.qpos = dalloc(s, N * 35, &ok); o.qvel = dalloc(s, N * 30, &ok); o.geoms = dalloc(s, N * kp::D_MAXGEOM * 17, &ok); o.ngeom = (int*)dalloc(s, N, &ok);
    o.warm = dalloc(s, N * 6 * kp::D_MAXOBJ, &ok); o.warm2 = dalloc(s, N * 6 * kp::D_MAXOBJ, &ok); o.slot = (signed char*)dalloc(s, (N * kp::D_MAXOBJ + 3) / 4 + 1, &ok);
    if (!m->h.obj_geoms.empty()) {
        o.d_geoms = upload<float>(s, m->h.obj_geoms, &ok); o.d_mass = upload<float>(s, m->h.obj_mass, &ok);
        o.n_geoms = (int)(m->h.obj_geoms.size() / 18); o.n_obj = (int)m->h.obj_mass.size();
    }
    if (const char* e = std::getenv("KP_PROFILE")) if (e[0] == '1') s->prof = (unsigned long long*)dalloc(s, N * 16, &ok);
    OverflowReadback& v = s->ovf;      // optional: without the pinned word or its events the lean layout runs without the adaptive fallback
    if (hipHostMalloc((void**)&v.host, 2 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) v.host = nullptr;
    else {
        v.host[0] = v.host[1] = 0u;
        if (hipEventCreateWithFlags(&v.ev[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&v.ev[1], hipEventDisableTiming) != hipSuccess) { hipHostFree(v.host); v.host = nullptr; }
    }
    if (!ok || hipEventCreate(&s->tm.ev0) != hipSuccess || hipEventCreate(&s->tm.ev1) != hipSuccess) {
        fail("kp_sim_create: device allocation / table build failed");
        kp_sim_destroy(s);
        return nullptr;
    }
    return s;
}

void kp_sim_destroy(kp_sim* s) {
    if (!s) return;
    hipSetDevice(s->device);
    hipStreamSynchronize(s->stream);
    for (void* p : s->allocs) hipFree(p);
    if (s->rd.partial) hipFree(s->rd.partial);
    if (s->idyn.buf) hipFree(s->idyn.buf);
    if (s->mk.buf) hipFree(s->mk.buf);
    for (hipEvent_t e : s->tm.ring) hipEventDestroy(e);
    if (s->ovf.host) { hipHostFree(s->ovf.host); for (hipEvent_t e : s->ovf.ev) if (e) hipEventDestroy(e); }
    if (s->tm.ev0) hipEventDestroy(s->tm.ev0);
    if (s->tm.ev1) hipEventDestroy(s->tm.ev1);
    delete s;
}
int kp_sim_n_envs(const kp_sim* s) { return s ? s->n : -1; }

int kp_sim_set_stream(kp_sim* s, void* stream) {
    if (!s) return fail("kp_sim_set_stream: null argument");
    s->stream = (hipStream_t)stream;
    return 0;
}

const uint32_t* kp_sim_status_device(kp_sim* s) { return s ? s->q.jobctr : nullptr; }

int kp_sim_contacts(kp_sim* s, float* out_host) {
    if (!s) return fail("kp_sim_contacts: null argument");
    HIP_OK(hipSetDevice(s->device));
    const size_t count = (size_t)s->n * (1 + kp::D_MAXCON * 9);
    if (!s->dbg_contacts) {           // first call arms the recording: later kp_sim_step_ctrl launches store their last contact set
        bool ok = true;
        s->dbg_contacts = dalloc(s, count, &ok);
        if (!ok) return fail("kp_sim_contacts: allocation failed");
        if (out_host) std::memset(out_host, 0, sizeof(float) * count);
        return 0;
    }
    if (!out_host) return 0;
    HIP_OK(hipStreamSynchronize(s->stream));
    HIP_OK(hipMemcpy(out_host, s->dbg_contacts, sizeof(float) * count, hipMemcpyDeviceToHost));
    return 0;
}

int kp_sim_mass_matrix(kp_sim* s, float* M, float* bias) {
    if (!s || (!M && !bias)) return fail("kp_sim_mass_matrix: null argument");
    HIP_OK(hipSetDevice(s->device));
    kp::StepArgs A{};
    A.T = s->T; A.P = s->P; A.n_envs = s->n; A.n_substeps = 0;
    A.qpos_d = s->st.qpos_d; A.qvel_d = s->st.qvel_d;
    hipLaunchKernelGGL(kp::kp_mass_kernel, dim3(s->n), dim3(64), sizeof(kp::EnvLds), s->stream, A, M, bias);
    return launched();
}

// masked row copy kernel (set_state writes only the masked envs)
__global__ void k_copy_rows(int n, int dim, const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ dst2,
                            const uint8_t* __restrict__ mask) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * dim) return;
    int e = (int)(t / dim);
    if (mask && !mask[e]) return;
    float v = src ? src[t] : 0.f;
    dst[t] = v;
    if (dst2) dst2[t] = v;
}
// dst (and dst2) <- src, or zero without src, in the masked envs' rows of width dim
static void copy_rows(const kp_sim* s, int dim, const float* src, float* dst, float* dst2, const uint8_t* mask) {
    hipLaunchKernelGGL(k_copy_rows, dim3((s->n * dim + 255) / 256), dim3(256), 0, s->stream, s->n, dim, src, dst, dst2, mask);
}

int kp_sim_set_state(kp_sim* s, const float* qpos, const float* qvel, const uint8_t* mask) {
    if (!s || !qpos || !qvel) return fail("kp_sim_set_state: null argument");
    HIP_OK(hipSetDevice(s->device));
    copy_rows(s, 76, qpos, s->st.qpos, s->st.qpos_d, mask);
    copy_rows(s, 75, qvel, s->st.qvel, s->st.qvel_d, mask);
    copy_rows(s, 75, nullptr, s->st.warm, nullptr, mask);
    HIP_OK(hipGetLastError());
    return launch_step(s, nullptr, 0, mask, false);  // sim.forward(): derived quantities at the new state
}

int kp_sim_set_target(kp_sim* s, const float* tq, const uint8_t* mask) {
    if (!s || !tq) return fail("kp_sim_set_target: null argument");
    HIP_OK(hipSetDevice(s->device));
    launch_target_fk(s, s->n, tq, mask, s->tgt);
    return launched();
}

// objects that are not parked (convert_obj_qpos parks the inactive ones 100+ m away): dynamic mode -> they become the env's
// free bodies (slots in object order, velocities zeroed as reset_model does); static mode -> their world-frame geoms are frozen
// row (optional): env e takes row row[e] of obj_qpos_in (a table of context rows, kp_sim_reset_rows) instead of row e; obj7 / one_hot (optional):
// obj7[e] <- get_obj_qpos(action_one_hot) of the fresh block, i.e. the 7 floats at the action's slot, untouched when the row has no action
__global__ void k_set_objects(int n, const float* __restrict__ obj_qpos_all, const uint8_t* __restrict__ mask, float* __restrict__ obj_qpos,
                              float* __restrict__ geoms, int* __restrict__ ngeom, const float* __restrict__ og, const float* __restrict__ omass,
                              int n_og, int n_obj, int dynamic, signed char* __restrict__ slot, float* __restrict__ obj_qvel, float* __restrict__ obj_warm,
                              const int* __restrict__ row, const float* __restrict__ one_hot, float* __restrict__ obj7) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (mask && !mask[e]) return;
    int ng = 0, ns = 0;
    const size_t r = row ? (size_t)row[e] : (size_t)e;
    const float* src = obj_qpos_all + r * 35;
    if (obj7) {
        const int st = kp::obj_action_start(one_hot ? one_hot + r * 4 : nullptr);
        if (st >= 0) for (int i = 0; i < 7; i++) obj7[(size_t)e * 7 + i] = obj_qpos_all[r * 35 + st + i];
        else { for (int i = 0; i < 7; i++) obj7[(size_t)e * 7 + i] = 0.f; obj7[(size_t)e * 7 + 3] = 1.f; }
    }
    for (int i = 0; i < 35; i++) obj_qpos[(size_t)e * 35 + i] = src[i];
    for (int i = 0; i < 30; i++) obj_qvel[(size_t)e * 30 + i] = 0.f;
    for (int i = 0; i < 6 * kp::D_MAXOBJ; i++) obj_warm[(size_t)e * 6 * kp::D_MAXOBJ + i] = 0.f;
    for (int k = 0; k < kp::D_MAXOBJ; k++) slot[(size_t)e * kp::D_MAXOBJ + k] = -1;
    if (dynamic) {
        for (int oi = 0; oi < n_obj && oi < 5 && ns < kp::D_MAXOBJ; oi++) {
            const float* pose = src + 7 * oi;
            if (sqrtf(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]) > 50.0f) continue;
            slot[(size_t)e * kp::D_MAXOBJ + ns++] = (signed char)oi;
        }
        ngeom[e] = 0;
        return;
    }
    for (int gi = 0; gi < n_og && ng < kp::D_MAXGEOM; gi++) {
        const float* g = og + 18 * gi;
        const int oi = (int)g[0];
        if (oi >= n_obj || oi >= 5) continue;
        const float* pose = src + 7 * oi;
        if (sqrtf(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]) > 50.0f) continue;
        kp::Q4 q = kp::qnormalize(kp::Q4{pose[3], pose[4], pose[5], pose[6]});
        float R[9], Rg[9];
        kp::q2mat(q, R);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rg[3 * i + j] = R[3 * i] * g[8 + j] + R[3 * i + 1] * g[11 + j] + R[3 * i + 2] * g[14 + j];
        kp::V3 p = kp::mulmat(R, kp::ld3(g + 5));
        float* o = geoms + ((size_t)e * kp::D_MAXGEOM + ng) * 17;
        o[0] = g[1]; o[1] = g[2]; o[2] = g[3]; o[3] = g[4];
        o[4] = pose[0] + p.x; o[5] = pose[1] + p.y; o[6] = pose[2] + p.z;
        for (int k = 0; k < 9; k++) o[7 + k] = Rg[k];
        o[16] = 1.0f / omass[oi];
        ng++;
    }
    ngeom[e] = ng;
}

// install the object block of the masked envs (k_set_objects); from now on the control step runs the object kernels
static int launch_set_objects(kp_sim* s, const char* who, const float* obj_qpos, const uint8_t* mask, const int* row, const float* one_hot, float* obj7) {
    ObjectRows& o = s->obj;
    if (!o.d_geoms) return fail(std::string(who) + ": the model blob has no object geoms");
    const int dynamic = s->model->dynamic_objects && s->T.obj_inertial != nullptr;
    hipLaunchKernelGGL(k_set_objects, dim3((s->n + 63) / 64), dim3(64), 0, s->stream, s->n, obj_qpos, mask, o.qpos, o.geoms, o.ngeom,
                       o.d_geoms, o.d_mass, o.n_geoms, o.n_obj, dynamic, o.slot, o.qvel, o.warm, row, one_hot, obj7);
    HIP_OK(hipGetLastError());
    o.on = true;
    return 0;
}

int kp_sim_set_objects(kp_sim* s, const float* obj_qpos, const uint8_t* mask) {
    if (!s || !obj_qpos) return fail("kp_sim_set_objects: null argument");
    HIP_OK(hipSetDevice(s->device));
    return launch_set_objects(s, "kp_sim_set_objects", obj_qpos, mask, nullptr, nullptr, nullptr);
}

int kp_sim_fk(kp_sim* s, int n_rows, const float* qpos, float* qpos_out, float* wbpos, float* wbquat, float* bquat, float* com) {
    if (!s || !qpos || n_rows <= 0) return fail("kp_sim_fk: bad arguments");
    HIP_OK(hipSetDevice(s->device));
    launch_target_fk(s, n_rows, qpos, nullptr, kp::TargetBufs{qpos_out, wbpos, wbquat, bquat, com});
    return launched();
}

int kp_sim_pose_contacts(kp_sim* s, int n_rows, const float* xpos, const float* xquat, const float* obj_qpos, float pen_margin,
                         float* pen, int32_t* ncon, uint32_t* hits) {
    if (!s) return fail("kp_sim_pose_contacts: null sim");
    if (n_rows < 0) return fail("kp_sim_pose_contacts: n_rows < 0");
    if (!xpos || !xquat) return fail("kp_sim_pose_contacts: null xpos / xquat");
    if (!pen || !ncon || !hits) return fail("kp_sim_pose_contacts: null output");
    if (obj_qpos && !s->obj.d_geoms) return fail("kp_sim_pose_contacts: obj_qpos given but the model blob has no object geoms");
    if (s->obj.n_geoms > kp::PC_MAXGEOM) return fail("kp_sim_pose_contacts: the model has more object geoms than the query holds (16)");
    if (n_rows == 0) return 0;
    HIP_OK(hipSetDevice(s->device));
    kp::PoseContactArgs A{};
    A.T = s->T; A.P = s->P; A.n_rows = n_rows; A.n_og = s->obj.n_geoms; A.n_obj = s->obj.n_obj;
    A.xpos = xpos; A.xquat = xquat; A.obj_qpos = obj_qpos; A.og = s->obj.d_geoms; A.pen_margin = pen_margin;
    A.pen = pen; A.ncon = ncon; A.hits = hits;
    HIP_OK(kp::launch_pose_contacts(A, s->stream));
    return 0;
}

int kp_model_hull_planes(const kp_model* m, float* planes4, int32_t* adr) {
    if (!m) return fail("kp_model_hull_planes: null model");
    std::vector<float> pl; std::vector<int32_t> ad;
    const int n = kp::hull_planes(m->h, pl, ad);
    if (planes4) std::memcpy(planes4, pl.data(), sizeof(float) * pl.size());
    if (adr) std::memcpy(adr, ad.data(), sizeof(int32_t) * ad.size());
    return n;
}

void kp_render_style_default(kp_render_style* st) {
    if (!st) return;
    const kp_render_style d = {{{0.8f, 0.8f, 0.8f}, {0.7f, 0.f, 0.f}, {0.1f, 0.5f, 0.1f}, {0.1f, 0.2f, 0.7f}}, {0.75f, 0.6f, 0.35f},
                               {{0.45f, 0.45f, 0.45f}, {0.6f, 0.6f, 0.6f}}, {0.75f, 0.85f, 1.0f}, 100.0f};
    *st = d;
}

namespace {
// what both renderers refuse, as the message of `who` ("" when the arguments are fine); n_out: outputs that are not null
std::string render_refusal(const char* who, const kp_sim* s, int n_rows, int n_fig, const float* xpos, const float* xquat, const float* obj_qpos, const float* camera,
                           int camera_rows, int width, int height, const kp_render_style* style, int n_out, const char* outputs) {
    const std::string w = std::string(who) + ": ";
    if (!s) return w + "null sim";
    if (n_rows < 0) return w + "n_rows < 0";
    if (n_fig < 1 || n_fig > kp::RD_MAXFIG) return w + "n_fig outside 1..4";
    if (width < 1 || width > kp::RD_MAXDIM || height < 1 || height > kp::RD_MAXDIM) return w + "width / height outside 1..4096";
    if (!xpos || !xquat) return w + "null xpos / xquat";
    if (!camera) return w + "null camera";
    if (camera_rows != 1 && camera_rows != n_rows) return w + "camera_rows is neither 1 nor n_rows";
    if (n_out == 0) return w + "null output (" + outputs + " are all null)";
    if (obj_qpos && !s->obj.d_geoms) return w + "obj_qpos given but the model blob has no object geoms";
    if (s->obj.n_geoms > kp::RD_MAXGEOM) return w + "the model has more object geoms than the renderer holds (16)";
    if (obj_qpos)
        for (int g = 0; g < s->obj.n_geoms; g++) {      // what the kernel draws: boxes and cylinders of the five objects of the 35-float block
            const double* og = s->model->h.obj_geoms.data() + 18 * g;
            if (og[1] != 0.0 && og[1] != 1.0) return w + "the model has an object geom that is neither a box (0) nor a cylinder (1)";
            if (og[0] < 0.0 || og[0] >= 5.0 || og[0] >= (double)s->obj.n_obj) return w + "the model has an object geom of an object outside the 35-float object block";
        }
    if (style && !(style->zfar > 0.f)) return w + "style.zfar must be positive";
    const long tiles = (long)((width + 7) / 8) * ((height + 7) / 8), blocks = (tiles + kp::RD_TILES - 1) / kp::RD_TILES * (long)n_rows;
    if (blocks > INT_MAX) return w + "n_rows x image tiles exceed one launch (render fewer rows per call)";
    return "";
}

// the hull planes on the device, uploaded by the first render
bool render_tables(kp_sim* s) {
    if (s->rd.planes) return true;
    std::vector<float> pl; std::vector<int32_t> ad;
    kp::hull_planes(s->model->h, pl, ad);
    bool ok = true;
    const float* dp = upload<float>(s, pl, &ok);
    const int32_t* da = upload<int32_t>(s, ad, &ok);
    if (ok) { s->rd.planes = dp; s->rd.adr = da; }
    return ok;
}
}  // namespace

int kp_sim_render(kp_sim* s, int n_rows, int n_fig, const float* xpos, const float* xquat, const float* obj_qpos, const float* camera, int camera_rows,
                  int width, int height, const kp_render_style* style, int32_t* geom, float* depth, uint8_t* rgba) {
    static_assert(sizeof(kp_render_style) == sizeof(kp::RenderStyle), "kp_render_style and kp::RenderStyle are one layout");
    const std::string no = render_refusal("kp_sim_render", s, n_rows, n_fig, xpos, xquat, obj_qpos, camera, camera_rows, width, height, style,
                                          (geom != nullptr) + (depth != nullptr) + (rgba != nullptr), "geom, depth and rgba");
    if (!no.empty()) return fail(no);
    if (n_rows == 0) return 0;
    HIP_OK(hipSetDevice(s->device));
    if (!render_tables(s)) return fail("kp_sim_render: uploading the hull planes failed");
    kp::RenderArgs A{};
    A.n_rows = n_rows; A.n_fig = n_fig; A.width = width; A.height = height; A.cam_rows = camera_rows; A.n_og = s->obj.n_geoms; A.n_obj = s->obj.n_obj;
    A.xpos = xpos; A.xquat = xquat; A.obj_qpos = obj_qpos; A.camera = camera; A.og = s->obj.d_geoms; A.rbound = s->T.body_rbound;
    A.planes = (const float4*)s->rd.planes; A.plane_adr = s->rd.adr;
    kp_render_style st;
    if (style) st = *style; else kp_render_style_default(&st);
    std::memcpy(&A.style, &st, sizeof(st));
    A.geom = geom; A.depth = depth; A.rgba = (uint32_t*)rgba;
    HIP_OK(kp::launch_render(A, s->stream));
    return 0;
}

int kp_sim_render_ego(kp_sim* s, int n_rows, int n_fig, const float* xpos, const float* xquat, const float* obj_qpos, const float* camera,
                      const float* xpos_b, const float* xquat_b, const float* obj_qpos_b, const float* camera_b, int camera_rows, int width, int height,
                      int hide_body, const kp_render_style* style, int grid_x, int grid_y,
                      int32_t* geom, float* depth, uint8_t* rgba, float* flow, uint8_t* ok, float* cells) {
    const char* who = "kp_sim_render_ego";
    const int n_out = (geom != nullptr) + (depth != nullptr) + (rgba != nullptr) + (flow != nullptr) + (ok != nullptr) + (cells != nullptr);
    const std::string no = render_refusal(who, s, n_rows, n_fig, xpos, xquat, obj_qpos, camera, camera_rows, width, height, style, n_out,
                                          "geom, depth, rgba, flow, ok and cells");
    if (!no.empty()) return fail(no);
    const bool pair = xpos_b && xquat_b && camera_b;
    if (!pair && (xpos_b || xquat_b || camera_b || obj_qpos_b))
        return fail("kp_sim_render_ego: the B side is given only in part (xpos_b, xquat_b and camera_b go together; obj_qpos_b needs them)");
    if (pair && (obj_qpos_b != nullptr) != (obj_qpos != nullptr))
        return fail("kp_sim_render_ego: the B side is given only in part (obj_qpos_b must be given exactly when obj_qpos is)");
    if (!pair && (flow || ok || cells)) return fail("kp_sim_render_ego: flow / ok / cells need a B side (xpos_b, xquat_b, camera_b)");
    if (hide_body < -1 || hide_body > 23) return fail("kp_sim_render_ego: hide_body outside -1..23");
    if (cells && (grid_x < 1 || grid_y < 1 || width % (8 * grid_x) != 0 || height % (8 * grid_y) != 0))
        return fail("kp_sim_render_ego: the cells grid does not divide the image into whole 8 x 8 tiles (width = 8 a grid_x, height = 8 b grid_y)");
    if (n_rows == 0) return 0;
    HIP_OK(hipSetDevice(s->device));
    if (!render_tables(s)) return fail("kp_sim_render_ego: uploading the hull planes failed");
    kp::RenderEgoArgs A{};
    if (cells) {                                 // the per-tile partial sums: a scratch of the handle that only grows
        const size_t need = (size_t)n_rows * ((width + 7) / 8) * ((height + 7) / 8) * 3;
        if (need > s->rd.partial_n) {
            if (s->rd.partial) { HIP_OK(hipStreamSynchronize(s->stream)); HIP_OK(hipFree(s->rd.partial)); s->rd.partial = nullptr; s->rd.partial_n = 0; }
            HIP_OK(hipMalloc((void**)&s->rd.partial, sizeof(float) * need));
            s->rd.partial_n = need;
        }
        A.partial = s->rd.partial; A.grid_x = grid_x; A.grid_y = grid_y;
    }
    A.n_rows = n_rows; A.n_fig = n_fig; A.width = width; A.height = height; A.cam_rows = camera_rows; A.n_og = s->obj.n_geoms; A.n_obj = s->obj.n_obj;
    A.hide_body = hide_body;
    A.xpos = xpos; A.xquat = xquat; A.obj_qpos = obj_qpos; A.camera = camera;
    if (pair) { A.xpos_b = xpos_b; A.xquat_b = xquat_b; A.obj_qpos_b = obj_qpos_b; A.camera_b = camera_b; }
    A.og = s->obj.d_geoms; A.rbound = s->T.body_rbound;
    A.planes = (const float4*)s->rd.planes; A.plane_adr = s->rd.adr;
    kp_render_style st;
    if (style) st = *style; else kp_render_style_default(&st);
    std::memcpy(&A.style, &st, sizeof(st));
    A.geom = geom; A.depth = depth; A.rgba = (uint32_t*)rgba; A.flow = flow; A.ok = ok; A.cells = cells;
    HIP_OK(kp::launch_render_ego(A, s->stream));
    return 0;
}

int kp_sim_fk_backward(kp_sim* s, int n_rows, const float* qpos, const float* wbpos, const float* wbquat, const float* grad_wbpos, float* grad_qpos) {
    if (!s || !qpos || !wbpos || !wbquat || !grad_wbpos || !grad_qpos || n_rows <= 0) return fail("kp_sim_fk_backward: bad arguments");
    HIP_OK(hipSetDevice(s->device));
    hipLaunchKernelGGL(kp::k_fk_wbpos_grad, dim3((n_rows + 3) / 4), dim3(256), 0, s->stream, n_rows, qpos, wbpos, wbquat, grad_wbpos, grad_qpos,
                       s->T.body_parent, s->T.body_subtree);
    return launched();
}

static int check_step_ctrl(const char* who, const kp_sim* s, const float* action, int nsub) {
    if (!s || !action || nsub <= 0) return fail(std::string(who) + ": bad arguments");
    if (s->xc.meta == 1 && nsub > 15)       // the reference's 30-entry meta_pd block holds kp / kd scales of 15 substeps (meta_pds[i_iter + 15], humanoid_im.py:456-458)
        return fail(std::string(who) + ": cc_meta_pd = 1 (meta_pd) scales the gains of at most 15 substeps per control step, got " + std::to_string(nsub));
    return 0;
}

int kp_sim_step_ctrl(kp_sim* s, const float* action, int nsub, const uint8_t* mask) {
    if (check_step_ctrl("kp_sim_step_ctrl", s, action, nsub)) return -1;
    HIP_OK(hipSetDevice(s->device));
    return launch_step(s, action, nsub, mask, true);
}

int kp_sim_step_ctrl_base(kp_sim* s, const float* action, int nsub, const uint8_t* mask, const float* base_qpos) {
    if (!base_qpos) return fail("kp_sim_step_ctrl_base: null base_qpos");
    if (check_step_ctrl("kp_sim_step_ctrl_base", s, action, nsub)) return -1;
    HIP_OK(hipSetDevice(s->device));
    return launch_step(s, action, nsub, mask, true, base_qpos);
}

// kp_takes_create (obj_rows null) and kp_takes_create_obj
static kp_takes* takes_create(const std::string& w, kp_sim* s, const float* qpos_rows, const float* obj_rows, int rows_on_device, const int32_t* take_off, int K, double dt) {
    if (!s || !qpos_rows || !take_off) { fail(w + ": null argument"); return nullptr; }
    if (K < 1) { fail(w + ": n_takes must be at least 1, got " + std::to_string(K)); return nullptr; }
    if (!(dt > 0.0)) { fail(w + ": dt must be positive"); return nullptr; }
    if (take_off[0] != 0) { fail(w + ": take_off[0] must be 0, got " + std::to_string(take_off[0])); return nullptr; }
    for (int k = 0; k < K; k++) {
        if (take_off[k + 1] <= take_off[k]) { fail(w + ": take_off must be increasing (take " + std::to_string(k) + ")"); return nullptr; }
        if (take_off[k + 1] - take_off[k] < 2) { fail(w + ": take " + std::to_string(k) + " has one row; a take needs at least 2"); return nullptr; }
    }
    if (obj_rows && !s->obj.d_geoms) { fail(w + ": obj_rows given but the model blob has no object geoms"); return nullptr; }
    if (obj_rows && s->obj.n_geoms > 64) { fail(w + ": the model has more object geoms than the reset kernel has lanes (64)"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(s->device));
    if (obj_rows) {                                   // one flag describes both arrays: obj_rows must live where it says qpos_rows does
        hipPointerAttribute_t at{};
        const bool on_dev = hipPointerGetAttributes(&at, obj_rows) == hipSuccess && at.type == hipMemoryTypeDevice;
        (void)hipGetLastError();                      // a plain host pointer is "invalid value" to some runtimes: not an error here
        if (on_dev != (rows_on_device != 0)) {
            fail(w + ": obj_rows is " + (on_dev ? "device" : "host") + " memory but rows_on_device = " + std::to_string(rows_on_device) + " (qpos_rows and obj_rows must be on the same side)");
            return nullptr;
        }
    }
    kp_takes* t = new kp_takes();
    t->model = s->model; t->device = s->device; t->off.assign(take_off, take_off + K + 1);
    const int R = take_off[K];
    t->L.R = R; t->L.K = K;
    bool ok = true;
    auto alloc = [&](size_t bytes) -> void* {
        void* d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(bytes, 16)) != hipSuccess) { ok = false; return nullptr; }
        t->allocs.push_back(d);
        return d;
    };
    for (int i = 0; i < kp::TT_COUNT; i++)
        t->L.tab[i] = (float*)alloc(sizeof(float) * (size_t)(i < kp::TT_ROW_TABLES ? R : K) * kp::TAKE_TAB_WIDTH[i]);
    std::vector<int32_t> row_take((size_t)R);
    for (int k = 0; k < K; k++) for (int r = take_off[k]; r < take_off[k + 1]; r++) row_take[r] = k;
    int32_t* d_off = (int32_t*)alloc(sizeof(int32_t) * (K + 1));
    int32_t* d_rt = (int32_t*)alloc(sizeof(int32_t) * (size_t)R);
    t->L.take_off = d_off; t->L.row_take = d_rt;
    if (obj_rows) t->obj = (float*)alloc(sizeof(float) * (size_t)R * 35);
    auto bail = [&](const std::string& m) -> kp_takes* { fail(w + m); kp_takes_destroy(t); return nullptr; };
    if (!ok) return bail(": device allocation failed");
    if (hipMemcpy(d_off, take_off, sizeof(int32_t) * (K + 1), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_rt, row_take.data(), sizeof(int32_t) * (size_t)R, hipMemcpyHostToDevice) != hipSuccess)
        return bail(": upload of the take offsets failed");
    if (hipMemcpyAsync(t->L.tab[kp::TT_QPOS], qpos_rows, sizeof(float) * (size_t)R * 76, rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream) != hipSuccess)
        return bail(": copy of qpos_rows failed");
    if (obj_rows && hipMemcpyAsync(t->obj, obj_rows, sizeof(float) * (size_t)R * 35, rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream) != hipSuccess)
        return bail(": copy of obj_rows failed");
    launch_target_fk(s, R, t->L.tab[kp::TT_QPOS], nullptr,
                     kp::TargetBufs{t->L.tab[kp::TT_QPOS_FK], t->L.tab[kp::TT_WBPOS], t->L.tab[kp::TT_WBQUAT], t->L.tab[kp::TT_BQUAT], t->L.tab[kp::TT_BODY_COM]});
    kp::TakeBuildArgs A{t->L, s->T.body_mass, (float)(1.0 / dt)};
    if (hipGetLastError() != hipSuccess || kp::launch_take_tables(A, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)
        return bail(": building the tables failed");
    return t;
}

kp_takes* kp_takes_create(kp_sim* s, const float* qpos_rows, int rows_on_device, const int32_t* take_off, int K, double dt) {
    return takes_create("kp_takes_create", s, qpos_rows, nullptr, rows_on_device, take_off, K, dt);
}

kp_takes* kp_takes_create_obj(kp_sim* s, const float* qpos_rows, const float* obj_rows, int rows_on_device, const int32_t* take_off, int K, double dt) {
    return takes_create("kp_takes_create_obj", s, qpos_rows, obj_rows, rows_on_device, take_off, K, dt);
}

int kp_takes_has_objects(const kp_takes* t) { return t && t->obj ? 1 : 0; }

void kp_takes_destroy(kp_takes* t) {
    if (!t) return;
    hipSetDevice(t->device);
    hipDeviceSynchronize();
    for (void* p : t->allocs) hipFree(p);
    delete t;
}

int kp_takes_table(const kp_takes* t, const char* name, const float** ptr, int* rows, int* width) {
    static const char* names[kp::TT_COUNT] = {"qpos", "qpos_fk", "wbpos", "wbquat", "bquat", "body_com", "com", "head_pose", "ee_wpos", "ee_pos", "rq_rmh", "qvel",
                                              "rlinv", "rangv", "rlinv_local", "bangvel", "height_lb", "head_height_lb"};
    if (!t || !name) return fail("kp_takes_table: null argument");
    for (int i = 0; i < kp::TT_COUNT; i++)
        if (!std::strcmp(name, names[i])) {
            if (ptr) *ptr = t->L.tab[i];
            if (rows) *rows = i < kp::TT_ROW_TABLES ? t->L.R : t->L.K;
            if (width) *width = kp::TAKE_TAB_WIDTH[i];
            return 0;
        }
    if (!std::strcmp(name, "obj_pose")) {             // kept beside the table set: only a library built by kp_takes_create_obj with obj_rows has it
        if (!t->obj) return fail("kp_takes_table: 'obj_pose' asked of a library without objects");
        if (ptr) *ptr = t->obj;
        if (rows) *rows = t->L.R;
        if (width) *width = 35;
        return 0;
    }
    return fail(std::string("kp_takes_table: no table named '") + name + "'");
}

int kp_takes_info(const kp_takes* t, int* n_takes, int* n_rows, int32_t* lens) {
    if (!t) return fail("kp_takes_info: null argument");
    if (n_takes) *n_takes = t->L.K;
    if (n_rows) *n_rows = t->L.R;
    for (int k = 0; lens && k < t->L.K; k++) lens[k] = t->off[k + 1] - t->off[k];
    return 0;
}

static int uhc_check(const char* who, const kp_sim* s, const kp_takes* t, const kp_uhc_state* st, const kp_uhc_cfg* c) {
    const std::string w(who);
    if (!s || !t || !st || !c) return fail(w + ": null argument");
    if (!st->take_id || !st->start_ind || !st->cur_t || !st->base_qpos) return fail(w + ": null pointer in kp_uhc_state");
    if (t->model != s->model) return fail(w + ": the take library was built for another model");
    if (t->device != s->device) return fail(w + ": the take library lives on device " + std::to_string(t->device) + ", the handle on " + std::to_string(s->device));
    if (!c->b_diffw) return fail(w + ": null b_diffw in kp_uhc_cfg");
    if (!(c->dt > 0.0)) return fail(w + ": kp_uhc_cfg.dt must be positive");
    if (c->action_dim != s->xc.stride) return fail(w + ": kp_uhc_cfg.action_dim " + std::to_string(c->action_dim) + " is not the handle's " + std::to_string(s->xc.stride));
    if (c->vf_dim < 0 || c->vf_dim > c->action_dim) return fail(w + ": vf_dim out of range");
    if ((c->a_ref != nullptr) != (s->xc.action_v0 != 0)) return fail(w + ": a_ref must be given exactly for an action_v 0 controller");
    return 0;
}

static kp::UhcTrackArgs uhc_track_args(kp_sim* s, const kp_takes* t, const kp_uhc_state* st, const kp_uhc_cfg* c, const float* action,
                                       float* reward, float* info, float* body_diff, uint8_t* failp, uint8_t* endp, uint8_t* donep, float* percent) {
    kp::UhcTrackArgs A{};
    A.L = t->L; A.n = s->n; A.st = *st; A.cfg = *c; A.inv_dt = (float)(1.0 / c->dt);
    A.qpos = s->st.qpos; A.xpos = s->st.xpos; A.xipos = s->st.xipos; A.prev_bquat = s->st.prev_bquat;
    A.t_qpos = s->tgt.qpos; A.t_wbpos = s->tgt.wbpos; A.t_wbquat = s->tgt.wbquat; A.t_bquat = s->tgt.bquat; A.t_com = s->tgt.com;
    A.body_mass = s->T.body_mass; A.b_diffw = c->b_diffw; A.jpos_diffw = s->diffw; A.action = action;
    A.reward = reward; A.info = info; A.body_diff = body_diff; A.percent = percent; A.fail = failp; A.end = endp; A.done = donep;
    return A;
}

int kp_sim_uhc_track(kp_sim* s, const kp_takes* t, const kp_uhc_state* st, const kp_uhc_cfg* c, const float* action,
                     float* reward, float* info, float* body_diff, uint8_t* failp, uint8_t* endp, uint8_t* donep, float* percent) {
    if (uhc_check("kp_sim_uhc_track", s, t, st, c)) return -1;
    if (!action || !reward || !info || !body_diff || !failp || !endp || !donep || !percent) return fail("kp_sim_uhc_track: null argument");
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(kp::launch_uhc_track(uhc_track_args(s, t, st, c, action, reward, info, body_diff, failp, endp, donep, percent), s->stream));
    return 0;
}

int kp_uhc_reward_info_dim(int reward_id) {
    if (reward_id < 0 || reward_id >= KP_UHC_REWARD_COUNT) return -1;
    return reward_id == KP_UHC_WORLD_RFC_IMPLICIT || reward_id == KP_UHC_WORLD_RFC_IMPLICIT_V1_MUL ? 5 : 6;
}

int kp_sim_uhc_track_r(kp_sim* s, const kp_takes* t, const kp_uhc_state* st, const kp_uhc_cfg_r* c, const float* action,
                       float* reward, float* info, float* body_diff, uint8_t* failp, uint8_t* endp, uint8_t* donep, float* percent) {
    if (!c) return fail("kp_sim_uhc_track_r: null argument");
    if (uhc_check("kp_sim_uhc_track_r", s, t, st, &c->base)) return -1;
    if (!action || !reward || !info || !body_diff || !failp || !endp || !donep || !percent) return fail("kp_sim_uhc_track_r: null argument");
    const int id = c->reward_id;
    if (kp_uhc_reward_info_dim(id) < 0) return fail("kp_sim_uhc_track_r: unknown reward_id " + std::to_string(id));
    if ((id == KP_UHC_WORLD_RFC_IMPLICIT_V2 || id == KP_UHC_WORLD_RFC_IMPLICIT_V3) && !c->jpos_diffw)
        return fail("kp_sim_uhc_track_r: world_rfc_implicit_v2 / _v3 need kp_uhc_cfg_r.jpos_diffw");
    if (id == KP_UHC_LOCAL_RFC_IMPLICIT && !c->prev_qpos) return fail("kp_sim_uhc_track_r: local_rfc_implicit needs kp_uhc_cfg_r.prev_qpos");
    HIP_OK(hipSetDevice(s->device));
    const kp::UhcRewardExt X{c->w_rp, c->w_rv, c->k_rh, c->k_rq, c->k_rl, c->k_ra, c->w_wp, c->w_j, c->k_wp, c->k_j, c->jpos_diffw, c->prev_qpos, s->st.xquat};
    HIP_OK(kp::launch_uhc_track_r(id, uhc_track_args(s, t, st, &c->base, action, reward, info, body_diff, failp, endp, donep, percent), X, s->stream));
    return 0;
}

int kp_sim_uhc_assign(kp_sim* s, const kp_takes* t, const kp_uhc_state* st, const kp_uhc_cfg* c, const uint8_t* mask,
                      const int32_t* take_ids, const int32_t* start, int keep_t, const float* noise) {
    if (uhc_check("kp_sim_uhc_assign", s, t, st, c)) return -1;
    if (start && !take_ids) return fail("kp_sim_uhc_assign: start_host needs take_ids_host (a start is checked against its take's length)");
    for (int e = 0; take_ids && e < s->n; e++) {
        if (take_ids[e] < 0 || take_ids[e] >= t->L.K)
            return fail("kp_sim_uhc_assign: take_id " + std::to_string(take_ids[e]) + " of env " + std::to_string(e) + " is out of range (the library holds " + std::to_string(t->L.K) + " takes)");
        if (start && (start[e] < 0 || start[e] >= t->off[take_ids[e] + 1] - t->off[take_ids[e]]))
            return fail("kp_sim_uhc_assign: start " + std::to_string(start[e]) + " of env " + std::to_string(e) + " is outside its take");
    }
    if (t->obj && !s->obj.d_geoms) return fail("kp_sim_uhc_assign: the take library carries objects but the model blob has no object geoms");
    if (t->obj && s->model->threads != 64) return fail("kp_sim_uhc_assign: a take library with objects needs threads_per_env = 64");
    HIP_OK(hipSetDevice(s->device));
    if (take_ids && !s->uhc_stage) {
        bool ok = true;
        s->uhc_stage = (int32_t*)dalloc(s, 2 * (size_t)s->n, &ok);
        if (!ok) { s->uhc_stage = nullptr; return fail("kp_sim_uhc_assign: allocation failed"); }
    }
    kp::UhcAssignArgs A{};
    if (take_ids) {
        HIP_OK(hipMemcpyAsync(s->uhc_stage, take_ids, sizeof(int32_t) * s->n, hipMemcpyHostToDevice, s->stream));
        A.take_ids = s->uhc_stage;
        if (start) { HIP_OK(hipMemcpyAsync(s->uhc_stage + s->n, start, sizeof(int32_t) * s->n, hipMemcpyHostToDevice, s->stream)); A.start = s->uhc_stage + s->n; }
    }
    A.L = t->L; A.n = s->n; A.keep_t = keep_t; A.obs_v = c->obs_v; A.st = *st; A.mask = mask; A.noise = noise; A.a_ref = c->a_ref;
    A.qpos = s->st.qpos; A.qpos_d = s->st.qpos_d; A.qvel = s->st.qvel; A.qvel_d = s->st.qvel_d; A.warm = s->st.warm;
    A.t_qpos = s->tgt.qpos; A.t_wbpos = s->tgt.wbpos; A.t_wbquat = s->tgt.wbquat; A.t_bquat = s->tgt.bquat; A.t_com = s->tgt.com;
    if (t->obj) {                                        // reset_model's has_obj branch: the object block comes from the same library row (k_uhc_assign_obj)
        ObjectRows& o = s->obj;
        kp::UhcAssignObjArgs B{};
        B.A = A; B.obj_tab = t->obj; B.obj_qpos = o.qpos; B.obj_qvel = o.qvel; B.obj_warm = o.warm; B.geoms = o.geoms; B.ngeom = o.ngeom; B.slot = o.slot;
        B.og = o.d_geoms; B.omass = o.d_mass; B.n_og = o.n_geoms; B.n_obj = o.n_obj;
        B.dynamic = s->model->dynamic_objects && s->T.obj_inertial != nullptr;
        HIP_OK(kp::launch_uhc_assign_obj(B, s->stream));
        o.on = true;                                     // from now on the control step and the forward pass below run the object kernels
    } else
        HIP_OK(kp::launch_uhc_assign(A, s->stream));
    return launch_step(s, nullptr, 0, mask, false);      // sim.forward(): derived quantities at the new state
}

int kp_sim_step_head(kp_sim* s, const float* act) {
    if (!s || !act) return fail("kp_sim_step_head: null argument");
    HIP_OK(hipSetDevice(s->device));
    launch_target_fk(s, s->n, s->st.qpos, nullptr, s->tgt, kp::KinStep{act, s->st.xpos, s->st.xquat, s->st.prev_bquat, s->st.prev_hpos, 1.0f / 30.0f});
    return launched();
}

int kp_sim_step_kin(kp_sim* s, const float* act, float* next_qpos) {
    if (!s || !act || !next_qpos) return fail("kp_sim_step_kin: null argument");
    HIP_OK(hipSetDevice(s->device));
    hipLaunchKernelGGL(kp::k_step_kin, dim3((s->n + 63) / 64), dim3(64), 0, s->stream, s->n, s->st.qpos, act, next_qpos, 1.0f / 30.0f);
    return launched();
}

static kp::ObsCcArgs obs_cc_args(const kp_sim* s, float* out, const float* zf_mean, const float* zf_std, float clip) {
    kp::ObsCcArgs A;
    A.n = s->n; A.qpos = s->st.qpos; A.qvel = s->st.qvel; A.xpos = s->st.xpos; A.xquat = s->st.xquat; A.xipos = s->st.xipos;
    A.t_qpos = s->tgt.qpos; A.t_wbpos = s->tgt.wbpos; A.t_wbquat = s->tgt.wbquat; A.t_com = s->tgt.com;
    for (int k = 0; k < 4; k++) A.br_inv[k] = s->P.br_inv[k];
    A.zf_mean = zf_mean; A.zf_std = zf_std; A.clip = clip; A.out = out;
    return A;
}

// ---- the UHC observation: ONE table of the 20 layouts, the 16 of obs_v 0 first (index vel_root | heading << 1 | deheading << 2 | phase << 3),
// then obs_v 1 and 2, which have the obs_vel switch only (a handle of theirs holds the other three as 0)
extern "C++" {   // the launcher is a template
using ObsCcLaunch = void (*)(kp_sim*, const kp::ObsCcArgs&, const float*);
template <int V, int I>
static void launch_obs_cc(kp_sim* s, const kp::ObsCcArgs& A, const float* phase) {
    if constexpr (V == 1 && I == 0) hipLaunchKernelGGL(kp::k_obs_cc_uhc, dim3(s->n), dim3(64), 0, s->stream, A);      // uhc.yml's: no phase argument
    else hipLaunchKernelGGL((kp::k_obs_cc<V, (I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0>), dim3(s->n), dim3(64), 0, s->stream, A, phase);
}
template <int... I>
static constexpr std::array<ObsCcLaunch, 20> obs_cc_table(std::integer_sequence<int, I...>) {
    return {launch_obs_cc<0, I>..., launch_obs_cc<1, 0>, launch_obs_cc<1, 1>, launch_obs_cc<2, 0>, launch_obs_cc<2, 1>};
}
static constexpr auto OBS_CC = obs_cc_table(std::make_integer_sequence<int, 16>{});
static constexpr int OBS_CC_V1 = 16;      // get_full_obs_v1 with the full velocities: uhc.yml's 784-wide row
}

int kp_sim_obs_cc(kp_sim* s, float* out, const float* zf_mean, const float* zf_std, float clip) {
    if (!s || !out) return fail("kp_sim_obs_cc: null argument");
    if ((zf_mean == nullptr) != (zf_std == nullptr)) return fail("kp_sim_obs_cc: pass both zf_mean and zf_std or neither");
    HIP_OK(hipSetDevice(s->device));
    OBS_CC[OBS_CC_V1](s, obs_cc_args(s, out, zf_mean, zf_std, clip), nullptr);      // whatever the handle's layout
    return launched();
}

int kp_sim_obs_cc_ex(kp_sim* s, float* out, const float* zf_mean, const float* zf_std, float clip, const float* phase) {
    if (!s || !out) return fail("kp_sim_obs_cc_ex: null argument");
    if ((zf_mean == nullptr) != (zf_std == nullptr)) return fail("kp_sim_obs_cc_ex: pass both zf_mean and zf_std or neither");
    if (s->cc_obs_phase && !phase) return fail("kp_sim_obs_cc_ex: this handle's observation ends with the phase (cc_obs_phase = 1): pass phase [N]");
    if (!s->cc_obs_phase && phase) return fail("kp_sim_obs_cc_ex: phase given, but this handle's observation has no phase slot (cc_obs_phase = 0 or cc_obs_v != 0)");
    HIP_OK(hipSetDevice(s->device));
    const int i = s->cc_obs_v == 0 ? s->cc_obs_vel_root | s->cc_obs_heading << 1 | s->cc_obs_deheading << 2 | s->cc_obs_phase << 3
                                   : OBS_CC_V1 + 2 * (s->cc_obs_v - 1) + s->cc_obs_vel_root;
    OBS_CC[i](s, obs_cc_args(s, out, zf_mean, zf_std, clip), phase);
    return launched();
}
int kp_sim_cc_obs_dim(const kp_sim* s) { return s ? s->cc_obs_dim : -1; }

// ---- state fields: ONE table behind kp_field_dim, kp_sim_field_device and kp_sim_get, indexed by kp_field.  row: where a stored field lives (null: a
// derived read-out, computed by kp_sim_get); view: kp_sim_field_device hands the row out (not the target read-outs and the prev_* records).
struct Field { int dim; bool view; float* (*row)(const kp_sim&); };
#define ROW(member) [](const kp_sim& s) -> float* { return s.member; }
static const Field FIELDS[] = {
    /* KP_QPOS */ {76, true, ROW(st.qpos)}, /* KP_QVEL */ {75, true, ROW(st.qvel)}, /* KP_XPOS */ {72, true, ROW(st.xpos)}, /* KP_XQUAT */ {96, true, ROW(st.xquat)},
    /* KP_XIPOS */ {72, true, ROW(st.xipos)}, /* KP_BQUAT */ {96, false, nullptr}, /* KP_HEAD */ {7, false, nullptr},
    /* KP_TARGET_QPOS */ {76, true, ROW(tgt.qpos)}, /* KP_TARGET_WBPOS */ {72, false, ROW(tgt.wbpos)}, /* KP_TARGET_WBQUAT */ {96, false, ROW(tgt.wbquat)},
    /* KP_TARGET_BQUAT */ {96, false, ROW(tgt.bquat)}, /* KP_TARGET_COM */ {72, false, ROW(tgt.com)},
    /* KP_QPOS_D */ {76, true, ROW(st.qpos_d)}, /* KP_QVEL_D */ {75, true, ROW(st.qvel_d)},
    /* KP_PREV_BQUAT */ {96, false, ROW(st.prev_bquat)}, /* KP_PREV_HPOS */ {7, false, ROW(st.prev_hpos)},
    /* KP_OBJ_QPOS */ {35, true, ROW(obj.qpos)}, /* KP_OBJ_QVEL */ {30, true, ROW(obj.qvel)}, /* KP_M */ {75 * 75, false, nullptr}, /* KP_BIAS */ {75, false, nullptr},
};
#undef ROW
static_assert(sizeof(FIELDS) / sizeof(FIELDS[0]) == KP_BIAS + 1, "one row per kp_field");
static const Field* find_field(int f) { return f >= 0 && f <= KP_BIAS ? &FIELDS[f] : nullptr; }

int kp_field_dim(int f) { const Field* d = find_field(f); return d ? d->dim : -1; }

__global__ void k_head(int n, const float* __restrict__ xpos, const float* __restrict__ xquat, float* __restrict__ out) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int hb = 13;  // Head (model._body_name2id['Head'] - 1)
    for (int k = 0; k < 3; k++) out[(size_t)e * 7 + k] = xpos[(size_t)e * 72 + 3 * hb + k];
    for (int k = 0; k < 4; k++) out[(size_t)e * 7 + 3 + k] = xquat[(size_t)e * 96 + 4 * hb + k];
}

const float* kp_sim_field_device(kp_sim* s, int field) {
    const Field* d = find_field(field);
    return s && d && d->view ? d->row(*s) : nullptr;
}

int kp_sim_get(kp_sim* s, int field, float* out) {
    if (!s || !out) return fail("kp_sim_get: null argument");
    HIP_OK(hipSetDevice(s->device));
    const Field* d = find_field(field);
    if (!d) return fail("kp_sim_get: unknown field");
    if (d->row) {
        HIP_OK(hipMemcpyAsync(out, d->row(*s), sizeof(float) * (size_t)s->n * d->dim, hipMemcpyDeviceToDevice, s->stream));
        return 0;
    }
    if (field == KP_M) return kp_sim_mass_matrix(s, out, nullptr);
    if (field == KP_BIAS) return kp_sim_mass_matrix(s, nullptr, out);
    if (field == KP_BQUAT) hipLaunchKernelGGL(kp::k_bquat, dim3((s->n * 24 + 255) / 256), dim3(256), 0, s->stream, s->n, s->st.qpos, out);
    else hipLaunchKernelGGL(k_head, dim3((s->n + 255) / 256), dim3(256), 0, s->stream, s->n, s->st.xpos, s->st.xquat, out);      // KP_HEAD
    return launched();
}

static kp::CtxDev to_dev(const kp_ctx* c) {
    kp::CtxDev d;
    d.T = c->T; d.head_pose = c->head_pose; d.head_vels = c->head_vels; d.obj_rel = c->obj_head_relative_poses;
    d.action_one_hot = c->action_one_hot; d.gt_bquat = c->gt_bquat; d.gt_wbpos = c->gt_wbpos; d.obj_qpos = c->obj_qpos; d.cur_t = c->cur_t; d.row = c->row;
    return d;
}

int kp_sim_step_begin(kp_sim* s) {
    if (!s) return fail("kp_sim_step_begin: null argument");
    HIP_OK(hipSetDevice(s->device));
    hipLaunchKernelGGL(kp::k_snapshot, dim3((s->n * 24 + 255) / 256), dim3(256), 0, s->stream, s->n, s->st.qpos, s->st.xpos, s->st.xquat, s->st.prev_bquat, s->st.prev_hpos);
    return launched();
}

extern "C++" {   // the launcher is a template
template <int I>      // I = vel | head << 1 | action << 2
static void launch_obs_ar(kp_sim* s, const kp_ctx* c, float* out) {
    constexpr bool VEL = (I & 1) != 0, HEAD = (I & 2) != 0, ACTION = (I & 4) != 0;
    static_assert(kp::ObsArLayout<VEL, HEAD, ACTION>::D == 74 + 75 * VEL + 7 * HEAD + 7 + 13 * HEAD + 4 * ACTION, "ar_obs_width is the kernel's row width");
    if constexpr (!VEL && HEAD)      // 105 / 101: the one-thread-per-env kernel, 2 us faster than k_obs_ar<false, true, .> at 4096 envs; the same words
        hipLaunchKernelGGL(kp::k_obs_ar_thread<ACTION>, dim3((s->n + 63) / 64), dim3(64), 0, s->stream, s->n, to_dev(c), s->st.qpos, s->st.xpos, s->st.xquat, out);
    else
        hipLaunchKernelGGL((kp::k_obs_ar<VEL, HEAD, ACTION>), dim3((s->n + 7) / 8), dim3(256), 0, s->stream, s->n, to_dev(c), s->st.qpos, s->st.qvel, s->st.xpos, s->st.xquat, out);
}
}
static void (*const OBS_AR[8])(kp_sim*, const kp_ctx*, float*) = {launch_obs_ar<0>, launch_obs_ar<1>, launch_obs_ar<2>, launch_obs_ar<3>,
                                                                  launch_obs_ar<4>, launch_obs_ar<5>, launch_obs_ar<6>, launch_obs_ar<7>};

// the arguments kp_sim_obs_ar and kp_sim_obs_ar_ex share: the handle, the row's context tables, the destination
static int check_obs_ar_args(const char* who, const kp_sim* s, const kp_ctx* c, const float* out) {
    if (!s || !c || !out || !c->head_pose || !c->head_vels || !c->obj_head_relative_poses || !c->action_one_hot || !c->cur_t || c->T < 1)
        return fail(std::string(who) + ": bad arguments");
    return 0;
}

int kp_sim_obs_ar(kp_sim* s, const kp_ctx* c, float* out) {
    if (check_obs_ar_args("kp_sim_obs_ar", s, c, out)) return -1;
    HIP_OK(hipSetDevice(s->device));
    OBS_AR[s->ar_obs_vel | s->ar_obs_head << 1 | s->ar_obs_action << 2](s, c, out);
    return launched();
}

static kp::RewardW reward_w(const kp_reward_cfg* w) {
    return kp::RewardW{w->w_hp, w->w_hq, w->w_p, w->w_jp, w->w_act_p, w->w_act_v, w->k_hp, w->k_hq, w->k_p, w->k_jp, w->k_act_p, w->k_act_v,
                       w->dt, w->body_diff_thresh, w->body_diff_gt_thresh, w->use_gt_term};
}
// termination + reward of the env step; post (optional): with the tail of HumanoidAREnv.step in the same launch (kp_sim_post_step)
static int launch_term_reward(kp_sim* s, const kp_ctx* c, const kp_reward_cfg* w, float* reward, float* info, uint8_t* failp, float* diffs, const kp::PostStep* post) {
    const StateRows& st = s->st;
    if (!post) hipLaunchKernelGGL(kp::k_term_reward<false>, dim3((s->n + 7) / 8), dim3(256), 0, s->stream, s->n, to_dev(c), reward_w(w), st.qpos, st.xpos, st.xquat,
                                  s->tgt.wbpos, s->tgt.bquat, st.prev_bquat, st.prev_hpos, s->diffw, reward, info, failp, diffs, kp::PostStep{});
    else hipLaunchKernelGGL(kp::k_term_reward<true>, dim3((s->n + 7) / 8), dim3(256), 0, s->stream, s->n, to_dev(c), reward_w(w), st.qpos, st.xpos, st.xquat,
                            s->tgt.wbpos, s->tgt.bquat, st.prev_bquat, st.prev_hpos, s->diffw, reward, info, failp, diffs, *post);
    return launched();
}

int kp_sim_term_reward(kp_sim* s, const kp_ctx* c, const kp_reward_cfg* w, float* reward, float* info, uint8_t* failp, float* diffs) {
    if (!s || !c || !w || !reward || !info || !failp || !diffs || !c->head_pose || !c->gt_bquat || !c->gt_wbpos || !c->cur_t || c->T < 2)
        return fail("kp_sim_term_reward: bad arguments");
    HIP_OK(hipSetDevice(s->device));
    return launch_term_reward(s, c, w, reward, info, failp, diffs, nullptr);
}

int kp_sim_post_step(kp_sim* s, const kp_ctx* c, const kp_reward_cfg* w, int32_t* cur_t, const int32_t* row_len, int env_episode_len,
                     float* reward, float* info, uint8_t* failp, float* diffs, uint8_t* done, uint8_t* end, float* percent, int32_t* done_count, float* obj7) {
    if (!s || !c || !w || !cur_t || !row_len || !reward || !info || !failp || !diffs || !done || !end || !percent || !c->head_pose || !c->gt_bquat || !c->gt_wbpos || c->T < 2)
        return fail("kp_sim_post_step: bad arguments");
    if (c->cur_t != cur_t) return fail("kp_sim_post_step: cur_t must be the buffer the context reads (kp_ctx.cur_t)");
    if (obj7 && !c->action_one_hot) return fail("kp_sim_post_step: obj7 needs the context's action_one_hot");
    HIP_OK(hipSetDevice(s->device));
    const kp::PostStep PS{cur_t, row_len, env_episode_len, done, end, percent, done_count, obj7, obj7 ? s->obj.qpos : nullptr};
    return launch_term_reward(s, c, w, reward, info, failp, diffs, &PS);
}

// dynamic_supervision_v2: the same two entries on k_term_reward<POST, 2, RewardW2>
static int launch_term_reward_v2(kp_sim* s, const kp_ctx* c, const kp_reward_cfg_v2* w, float* reward, float* info, uint8_t* failp, float* diffs, const kp::PostStep* post) {
    const StateRows& st = s->st;
    const kp::RewardW2 W{w->w_hp, w->w_hq, w->w_p, w->w_v, w->w_e, w->k_hp, w->k_hq, w->k_p, w->k_v, w->k_e, w->dt, w->body_diff_thresh, w->body_diff_gt_thresh,
                         w->use_gt_term, w->b_diffw};
    if (!post) hipLaunchKernelGGL((kp::k_term_reward<false, 2, kp::RewardW2>), dim3((s->n + 7) / 8), dim3(256), 0, s->stream, s->n, to_dev(c), W, st.qpos, st.xpos, st.xquat,
                                  s->tgt.wbpos, s->tgt.bquat, st.prev_bquat, st.prev_hpos, s->diffw, reward, info, failp, diffs, kp::PostStep{});
    else hipLaunchKernelGGL((kp::k_term_reward<true, 2, kp::RewardW2>), dim3((s->n + 7) / 8), dim3(256), 0, s->stream, s->n, to_dev(c), W, st.qpos, st.xpos, st.xquat,
                            s->tgt.wbpos, s->tgt.bquat, st.prev_bquat, st.prev_hpos, s->diffw, reward, info, failp, diffs, *post);
    return launched();
}

int kp_sim_term_reward_v2(kp_sim* s, const kp_ctx* c, const kp_reward_cfg_v2* w, float* reward, float* info, uint8_t* failp, float* diffs) {
    if (!s || !c || !w || !w->b_diffw || !reward || !info || !failp || !diffs || !c->head_pose || !c->gt_bquat || !c->gt_wbpos || !c->cur_t || c->T < 2)
        return fail("kp_sim_term_reward_v2: bad arguments");
    HIP_OK(hipSetDevice(s->device));
    return launch_term_reward_v2(s, c, w, reward, info, failp, diffs, nullptr);
}

int kp_sim_post_step_v2(kp_sim* s, const kp_ctx* c, const kp_reward_cfg_v2* w, int32_t* cur_t, const int32_t* row_len, int env_episode_len,
                        float* reward, float* info, uint8_t* failp, float* diffs, uint8_t* done, uint8_t* end, float* percent, int32_t* done_count, float* obj7) {
    if (!s || !c || !w || !w->b_diffw || !cur_t || !row_len || !reward || !info || !failp || !diffs || !done || !end || !percent || !c->head_pose || !c->gt_bquat ||
        !c->gt_wbpos || c->T < 2)
        return fail("kp_sim_post_step_v2: bad arguments");
    if (c->cur_t != cur_t) return fail("kp_sim_post_step_v2: cur_t must be the buffer the context reads (kp_ctx.cur_t)");
    if (obj7 && !c->action_one_hot) return fail("kp_sim_post_step_v2: obj7 needs the context's action_one_hot");
    HIP_OK(hipSetDevice(s->device));
    const kp::PostStep PS{cur_t, row_len, env_episode_len, done, end, percent, done_count, obj7, obj7 ? s->obj.qpos : nullptr};
    return launch_term_reward_v2(s, c, w, reward, info, failp, diffs, &PS);
}

int kp_sim_reset_rows(kp_sim* s, const float* init_qpos, const float* init_qvel, const int32_t* row, const uint8_t* mask, int32_t* cur_t, int set_target,
                      float* aux_rows, int aux_cols, const float* row_obj_qpos, const float* row_action_one_hot, float* obj7) {
    if (!s || !init_qpos || !init_qvel || (aux_rows && aux_cols <= 0)) return fail("kp_sim_reset_rows: null argument");
    if (obj7 && !row_obj_qpos) return fail("kp_sim_reset_rows: obj7 needs row_obj_qpos");
    HIP_OK(hipSetDevice(s->device));
    // the object block of reset_model (humanoid_ar_v1.py:377-382) from the env's context row, before sim.forward()
    if (row_obj_qpos && launch_set_objects(s, "kp_sim_reset_rows", row_obj_qpos, mask, row, row_action_one_hot, obj7)) return -1;
    hipLaunchKernelGGL(kp::k_reset_rows, dim3(s->n), dim3(128), 0, s->stream, s->n, init_qpos, init_qvel, row, mask, cur_t, s->st.qpos, s->st.qvel, s->st.qpos_d, s->st.qvel_d,
                       s->st.warm, aux_rows, aux_rows ? aux_cols : 0);
    HIP_OK(hipGetLastError());
    if (int rc = launch_step(s, nullptr, 0, mask, false)) return rc;      // sim.forward(): derived quantities at the new state
    if (set_target) {                                                     // target = smpl_humanoid.qpos_fk(init_qpos) (humanoid_ar_v1.py:384-386): the state just written
        launch_target_fk(s, s->n, s->st.qpos, mask, s->tgt);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int kp_gae_bootstrap(int n, int T, const float* rewards, const float* masks, const float* values, const float* last_values, float gamma, float tau,
                     float* adv, float* ret, void* stream) {
    if (n <= 0 || T <= 0 || !rewards || !masks || !values || !adv || !ret) return fail("kp_gae: bad arguments");
    hipLaunchKernelGGL(kp::k_gae, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, T, rewards, masks, values, last_values, gamma, tau, adv, ret);
    return launched();
}
int kp_gae(int n, int T, const float* rewards, const float* masks, const float* values, float gamma, float tau, float* adv, float* ret, void* stream) {
    return kp_gae_bootstrap(n, T, rewards, masks, values, nullptr, gamma, tau, adv, ret, stream);
}

int kp_pool_advance(int n, int n_slots, const uint8_t* done, int32_t* head, int32_t* ahead, int32_t* row, void* stream) {
    if (n <= 0 || n_slots <= 0 || !done || !head || !ahead || !row) return fail("kp_pool_advance: bad arguments");
    hipLaunchKernelGGL(kp::k_pool_advance, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, n_slots, done, head, ahead, row);
    return launched();
}

int kp_sim_ar_obs_dim(const kp_sim* s) { return s ? s->ar_obs_dim : -1; }

// The sampler's records, one path per half-step: the source / destination checks and the launch.  The row width is the kernel's argument; every
// entry point checks its own width first (`who` is the name its errors carry).
static int record_pre(const char* who, const kp_record_pre* r, int obs_dim, void* stream) {
    if ((r->states && !r->obs) || (r->episode_start && !r->fresh) || (r->curr_qpos && !r->qpos) || (r->meta && !r->row_meta) ||
        (r->gt_target_qpos && (!r->ctx_qpos || !r->cur_t || !r->row_len || r->ctx_T <= 0)))
        return fail(std::string(who) + ": a destination without its source");
    kp::RecordPre R{r->n, r->T, r->t, r->ctx_T, obs_dim, r->obs, r->fresh, r->qpos, r->ctx_qpos, r->row, r->cur_t, r->row_len, r->row_meta,
                    r->states, r->episode_start, r->curr_qpos, r->gt_target_qpos, r->meta};
    hipLaunchKernelGGL(kp::k_record_pre, dim3(r->n), dim3(128), 0, (hipStream_t)stream, R);
    return launched();
}
static int record_post(const char* who, const kp_record_post* r, int obs_dim, void* stream) {
    if ((r->actions && !r->action) || (r->rewards && !r->reward) || (r->fails && !r->fail) || (r->dones && !r->done) || (r->percents && !r->percent) ||
        (r->c_infos && !r->c_info) || (r->next_states && !r->obs) || (r->res_qpos && !r->qpos) || (r->cc_actions && !r->cc_action) ||
        (r->cc_states && !r->cc_state) || (r->v_metas && !r->meta))
        return fail(std::string(who) + ": a destination without its source");
    kp::RecordPost R{r->n, r->T, r->t, obs_dim, r->fr_num, r->action, r->reward, r->fail, r->done, r->percent, r->c_info, r->obs, r->qpos, r->cc_action, r->cc_state, r->meta,
                     r->actions, r->rewards, r->fails, r->dones, r->percents, r->c_infos, r->next_states, r->res_qpos, r->cc_actions, r->cc_states, r->v_metas};
    hipLaunchKernelGGL(kp::k_record_post, dim3(r->n), dim3(128), 0, (hipStream_t)stream, R);
    return launched();
}

int kp_rollout_record_pre_w(const kp_record_pre* r, int obs_dim, void* stream) {
    if (!r || r->n <= 0 || r->T <= 0 || r->t < 0 || r->t >= r->T) return fail("kp_rollout_record_pre: bad arguments");
    if (!ar_obs_width_known(obs_dim)) return fail("kp_rollout_record_pre: obs_dim must be " KP_AR_OBS_WIDTHS ", got " + std::to_string(obs_dim));
    return record_pre("kp_rollout_record_pre", r, obs_dim, stream);
}
int kp_rollout_record_pre(const kp_record_pre* r, void* stream) { return kp_rollout_record_pre_w(r, KP_AR_OBS_DIM, stream); }

int kp_rollout_record_post_w(const kp_record_post* r, int obs_dim, void* stream) {
    if (!r || r->n <= 0 || r->T <= 0 || r->t < 0 || r->t >= r->T) return fail("kp_rollout_record_post: bad arguments");
    if (!ar_obs_width_known(obs_dim)) return fail("kp_rollout_record_post: obs_dim must be " KP_AR_OBS_WIDTHS ", got " + std::to_string(obs_dim));
    return record_post("kp_rollout_record_post", r, obs_dim, stream);
}
int kp_rollout_record_post(const kp_record_post* r, void* stream) { return kp_rollout_record_post_w(r, KP_AR_OBS_DIM, stream); }

int kp_mcp_compose(int n, int K, int A, const float* logits, const float* prim, const float* noise, int noise_stride, const float* stdv, float* out, void* stream) {
    if (n <= 0 || K <= 0 || K > 64 || A <= 0 || !logits || !prim || !out || (noise && !stdv)) return fail("kp_mcp_compose: bad arguments");
    if (noise && noise_stride < A) return fail("kp_mcp_compose: noise_stride " + std::to_string(noise_stride) + " is smaller than the row width A = " + std::to_string(A));
    const size_t tot = (size_t)n * A;
    hipLaunchKernelGGL(kp::k_mcp_compose, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, K, A, logits, prim, noise, noise_stride, stdv, out);
    return launched();
}

int kp_kin_advance(int n, const float* qpos, const float* kin_action, float dt, float* next_qpos, float* qvel_fd, void* stream) {
    if (n <= 0 || !qpos || !kin_action || !next_qpos || !qvel_fd || !(dt > 0.f)) return fail("kp_kin_advance: bad arguments");
    hipLaunchKernelGGL(kp::k_kin_advance, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, n, qpos, kin_action, dt, next_qpos, qvel_fd);
    return launched();
}

int kp_mcp_tail(int n, int K, int J, int A, const float* h2, const float* b2, const float* w3, int ldw, const float* b3, const float* logits, const float* noise,
                int noise_stride, const float* stdv, float* out, void* stream) {
    if (n <= 0 || K <= 0 || K > 16 || J <= 0 || J % kp::MCP_CHUNK || A <= 0 || A > 80 || ldw < A || !h2 || !b2 || !w3 || !b3 || !logits || !out || (noise && !stdv))
        return fail("kp_mcp_tail: bad arguments (K <= 16 primitives, hidden width a multiple of 64, A <= 80 actions, ldw >= A)");
    const dim3 grid((unsigned)((n + 15) / 16)), block(64 * kp::MCP_WAVES);
    hipStream_t st = (hipStream_t)stream;
#define KP_TAIL(NT, V) hipLaunchKernelGGL((kp::k_mcp_tail<NT, V>), grid, block, 0, st, n, K, J, A, h2, b2, w3, ldw, b3, logits, noise, noise_stride, stdv, out)
    if (A <= 16) KP_TAIL(1, false);
    else if (A <= 48) KP_TAIL(3, false);
    else if (ldw >= 80 && ldw % 4 == 0 && ((uintptr_t)w3 & 15) == 0) KP_TAIL(5, true);      // rows padded to 80 columns: 16-byte operand loads
    else KP_TAIL(5, false);
#undef KP_TAIL
    return launched();
}

int kp_gru_cell_step(int n, int H, int D, const float* gi, const float* gh, const float* b_ih, const float* b_hh, const float* h_in, const float* state,
                     float* h_out, float* xcat, void* stream) {
    if (n <= 0 || H <= 0 || !gi || !gh || !b_ih || !b_hh || !h_in || !h_out || (xcat && (!state || D <= 0)))
        return fail("kp_gru_cell_step: bad arguments (the [state | h] row needs state and D > 0)");
    const size_t tot = (size_t)n * H;
    hipLaunchKernelGGL(kp::k_gru_cell_step, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, H, D, gi, gh, b_ih, b_hh, h_in, state, h_out, xcat);
    return launched();
}

int kp_gru_gates_forward(int n, int H, const float* gi, const float* gh, const float* hm_prev, const float* next_keep, float* h_out, float* hm_next, void* stream) {
    if (n <= 0 || H <= 0 || !gi || !gh || !hm_prev || !h_out) return fail("kp_gru_gates_forward: bad arguments");
    const size_t tot = (size_t)n * H;
    hipLaunchKernelGGL(kp::k_gru_gates_fwd, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, H, gi, gh, hm_prev, next_keep, h_out, hm_next);
    return launched();
}
int kp_gru_gates_backward(int n, int H, const float* gi, const float* gh, const float* hm_prev, const float* dh_out, const float* carry, const float* carry_keep,
                          float* dgi, float* dgh, float* dhz, void* stream) {
    if (n <= 0 || H <= 0 || !gi || !gh || !hm_prev || !dgi || !dgh || !dhz) return fail("kp_gru_gates_backward: bad arguments");
    const size_t tot = (size_t)n * H;
    hipLaunchKernelGGL(kp::k_gru_gates_bwd, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, H, gi, gh, hm_prev, dh_out, carry, carry_keep, dgi, dgh, dhz);
    return launched();
}

int kp_sim_set_full_state(kp_sim* s, const float* qpos, const float* qvel, const float* qpos_d, const float* qvel_d, const uint8_t* mask) {
    if (!s || !qpos || !qvel || !qpos_d || !qvel_d) return fail("kp_sim_set_full_state: null argument");
    HIP_OK(hipSetDevice(s->device));
    copy_rows(s, 76, qpos, s->st.qpos, nullptr, mask);
    copy_rows(s, 75, qvel, s->st.qvel, nullptr, mask);
    copy_rows(s, 76, qpos_d, s->st.qpos_d, nullptr, mask);
    copy_rows(s, 75, qvel_d, s->st.qvel_d, nullptr, mask);
    HIP_OK(hipGetLastError());
    return launch_step(s, nullptr, 0, mask, false);
}

int kp_sim_set_obj_state(kp_sim* s, const float* obj_qpos, const float* obj_qvel, const uint8_t* mask) {
    if (!s || !obj_qpos || !obj_qvel) return fail("kp_sim_set_obj_state: null argument");
    if (!s->obj.on) return fail("kp_sim_set_obj_state: call kp_sim_set_objects first (it decides which objects are simulated)");
    HIP_OK(hipSetDevice(s->device));
    copy_rows(s, 35, obj_qpos, s->obj.qpos, nullptr, mask);
    copy_rows(s, 30, obj_qvel, s->obj.qvel, nullptr, mask);
    return launched();
}

int kp_sim_apply_impulse(kp_sim* s, const int32_t* entity, const float* offset, const float* impulse, const uint8_t* mask, float* dqvel) {
    if (!s || !entity || !impulse) return fail("kp_sim_apply_impulse: null argument");
    HIP_OK(hipSetDevice(s->device));
    kp::StepArgs A{};
    A.T = s->T; A.P = s->P; A.n_envs = s->n; A.n_substeps = 0;
    A.qpos = s->st.qpos; A.qvel = s->st.qvel;
    // the object slots mean something once kp_sim_set_objects / kp_sim_reset_rows have installed a block (zero-filled before that)
    const ObjectRows& o = s->obj;
    if (o.on && s->T.obj_inertial) { A.obj_slot = o.slot; A.obj_qpos = o.qpos; A.obj_qvel = o.qvel; }
    kp::launch_apply_impulse(A, entity, offset, impulse, mask, dqvel, s->stream);
    return launched();
}

int kp_sim_diag(kp_sim* s, int32_t* out_host) {
    if (!s || !out_host) return fail("kp_sim_diag: null argument");
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipStreamSynchronize(s->stream));
    HIP_OK(hipMemcpy(out_host, s->st.diag, sizeof(int) * 4 * (size_t)s->n, hipMemcpyDeviceToHost));
    unsigned ctr[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpy(ctr, s->q.jobctr, sizeof(ctr), hipMemcpyDeviceToHost));
    if (ctr[2]) {
        hipMemset(s->q.jobctr + 2, 0, sizeof(unsigned));     // reported once
        return fail("kp_step_queue_kernel: a wavefront gave up waiting for a job to be published (job queue stalled); states are incomplete");
    }
    return 0;
}

int kp_job_schedule(int n_substeps, int substeps_per_job, int taper, int* sizes16) {
    if (!sizes16 || n_substeps <= 0 || substeps_per_job <= 0 || n_substeps > 255) return fail("kp_job_schedule: need sizes16, 0 < n_substeps <= 255, substeps_per_job > 0");
    return job_schedule(n_substeps, substeps_per_job, taper, sizes16);
}

int kp_sim_lean_state(kp_sim* s, int32_t* out3) {
    if (!s || !out3) return fail("kp_sim_lean_state: null argument");
    const StepPlan p = plan_step(*s, s->last_nsub, false);
    out3[0] = p.queue && p.layout == LEAN;
    out3[1] = s->ovf.fallbacks; out3[2] = (int32_t)s->launch_index;
    return 0;
}

int kp_sim_launch_cost(kp_sim* s, uint32_t* out_host) {
    if (!s || !out_host) return fail("kp_sim_launch_cost: null argument");
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipStreamSynchronize(s->stream));
    HIP_OK(hipMemcpy(out_host, s->q.cost, sizeof(unsigned) * (size_t)s->n, hipMemcpyDeviceToHost));
    return 0;
}

double kp_sim_last_step_seconds(kp_sim* s) {
    if (!s || !s->tm.timed) return -1.0;
    if (hipEventSynchronize(s->tm.last1) != hipSuccess) return -1.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->tm.last0, s->tm.last1) != hipSuccess) return -1.0;
    return ms * 1e-3;
}

// the per-env phase cycles of the last control step (KP_PROFILE=1) on the host: [N, 8]
static int read_profile(const char* who, kp_sim* s, const double* out, std::vector<unsigned long long>& h) {
    if (!s || !out) return fail(std::string(who) + ": null argument");
    if (!s->prof) return fail(std::string(who) + ": create the simulator with KP_PROFILE=1");
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipStreamSynchronize(s->stream));
    h.resize((size_t)s->n * 8);
    HIP_OK(hipMemcpy(h.data(), s->prof, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    return 0;
}

int kp_sim_phase_cycles(kp_sim* s, double* out) {
    std::vector<unsigned long long> h;
    if (read_profile("kp_sim_phase_cycles", s, out, h)) return -1;
    for (int k = 0; k < 8; k++) { double acc = 0; for (int e = 0; e < s->n; e++) acc += (double)h[(size_t)e * 8 + k]; out[k] = acc / s->n; }
    return 0;
}

int kp_sim_phase_cycles_env(kp_sim* s, double* out) {
    std::vector<unsigned long long> h;
    if (read_profile("kp_sim_phase_cycles_env", s, out, h)) return -1;
    for (size_t i = 0; i < h.size(); i++) out[i] = (double)h[i];
    return 0;
}

int kp_sim_timing_reset(kp_sim* s) {
    if (!s) return fail("kp_sim_timing_reset: null argument");
    s->tm.ring_used = 0; s->tm.ring_on = true;
    return 0;
}

double kp_sim_timing_mean_seconds(kp_sim* s, int* n_launches) {
    if (n_launches) *n_launches = 0;
    if (!s || s->tm.ring_used == 0) return -1.0;
    const Timing& tm = s->tm;
    if (hipStreamSynchronize(s->stream) != hipSuccess) return -1.0;
    double tot = 0.0;
    for (int i = 0; i < tm.ring_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tm.ring[2 * i], tm.ring[2 * i + 1]) != hipSuccess) return -1.0;
        tot += ms;
    }
    if (n_launches) *n_launches = tm.ring_used;
    return tot * 1e-3 / tm.ring_used;
}

// ---- the backward side of the kinematic roll-out (kp_kin_tape.hip): every refusal comes before any launch
int kp_kin_advance_backward(int n, const float* qpos, const float* kin_action, float dt, const float* grad_next_qpos, const float* grad_qvel,
                            float* grad_qpos, float* grad_action, void* stream) {
    if (n < 0) return fail("kp_kin_advance_backward: n < 0");
    if (!qpos || !kin_action) return fail("kp_kin_advance_backward: null qpos / kin_action");
    if (!grad_qpos || !grad_action) return fail("kp_kin_advance_backward: null output");
    if (!(dt > 0.f)) return fail("kp_kin_advance_backward: dt must be positive");
    if (n == 0) return 0;
    HIP_OK(kp::launch_kin_advance_grad(kp::KinAdvanceGradArgs{n, qpos, kin_action, dt, grad_next_qpos, grad_qvel, grad_qpos, grad_action}, (hipStream_t)stream));
    return 0;
}

// (d obs_ar)^T for both row forms.  The handle and the layout first (`who`: the entry point's name in every message) ...
static int check_obs_ar_grad(const char* who, const kp_sim* s) {
    const std::string w(who);
    if (!s) return fail(w + ": null sim");
    if (!s->ar_obs_head && !s->ar_obs_action)
        return fail(w + ": the " + std::to_string(s->ar_obs_dim) + "-d layout (use_head and use_action both off) has no gradient kernel");
    return 0;
}
static int check_obs_ar_grad_rows(const char* who, const kp_sim* s, int n_rows) {
    if (n_rows < 0 || n_rows > s->n) return fail(std::string(who) + ": n_rows must be in [0, " + std::to_string(s->n) + "], got " + std::to_string(n_rows));
    return 0;
}
// ... then, once the entry point has checked its row width, the backward of the base block: it sits at column `offset` of grad_obs rows `pitch` floats
// apart (the plain row: 0 and its own width).  The columns before it are the context block, whose cotangent goes to grad_ctx (kp_obs_ctx.hip).
static int obs_ar_base_backward(const char* who, kp_sim* s, const kp_ctx* c, int n_rows, int pitch, int offset, const float* qpos, const float* wbpos,
                                const float* wbquat, const float* grad_obs, const float* grad_obj_2_head, float* grad_qpos, float* grad_qvel,
                                float* grad_hpos, float* grad_hquat, float* grad_ctx) {
    const std::string w(who);
    if (!c || !c->action_one_hot || !c->cur_t || c->T < 1 || (s->ar_obs_head && !c->head_pose)) return fail(w + ": null or empty context");
    if (!qpos || !wbpos || !wbquat || !grad_obs) return fail(w + ": null qpos / wbpos / wbquat / grad_obs");
    if (!grad_qpos || !grad_hpos || !grad_hquat || (s->ar_obs_vel && !grad_qvel) || (offset > 0 && !grad_ctx)) return fail(w + ": null output");
    if (n_rows == 0) return 0;
    HIP_OK(hipSetDevice(s->device));
    kp::ObsArGradArgs A{};
    A.n = n_rows; A.vel = s->ar_obs_vel; A.head = s->ar_obs_head; A.width = pitch;
    A.T = c->T; A.head_pose = c->head_pose; A.action_one_hot = c->action_one_hot; A.obj_qpos = c->obj_qpos; A.cur_t = c->cur_t; A.row = c->row;
    A.qpos = qpos; A.wbpos = wbpos; A.wbquat = wbquat; A.g_obs = grad_obs + offset; A.g_obj = grad_obj_2_head;
    A.g_qpos = grad_qpos; A.g_qvel = grad_qvel; A.g_hpos = grad_hpos; A.g_hquat = grad_hquat;
    HIP_OK(kp::launch_obs_ar_grad(A, s->stream));
    if (offset > 0) HIP_OK(kp::launch_obs_ctx_grad(n_rows, offset, grad_obs, pitch, grad_ctx, s->stream));
    return 0;
}

int kp_sim_obs_ar_backward(kp_sim* s, const kp_ctx* c, int n_rows, int grad_width, const float* qpos, const float* wbpos, const float* wbquat,
                           const float* grad_obs, const float* grad_obj_2_head, float* grad_qpos, float* grad_qvel, float* grad_hpos, float* grad_hquat) {
    const char* who = "kp_sim_obs_ar_backward";
    if (check_obs_ar_grad(who, s) || check_obs_ar_grad_rows(who, s, n_rows)) return -1;
    if (grad_width != s->ar_obs_dim)
        return fail("kp_sim_obs_ar_backward: grad_obs is " + std::to_string(grad_width) + " wide, the handle's observation " + std::to_string(s->ar_obs_dim));
    return obs_ar_base_backward(who, s, c, n_rows, s->ar_obs_dim, 0, qpos, wbpos, wbquat, grad_obs, grad_obj_2_head, grad_qpos, grad_qvel, grad_hpos, grad_hquat, nullptr);
}

int kp_sim_fk_head_backward(kp_sim* s, int n_rows, const float* qpos, const float* wbpos, const float* wbquat, const float* grad_wbpos,
                            const float* grad_hpos, const float* grad_hquat, const float* grad_qpos_add, float* grad_qpos) {
    if (!s) return fail("kp_sim_fk_head_backward: null sim");
    if (n_rows < 0) return fail("kp_sim_fk_head_backward: n_rows < 0");
    if (!qpos || !wbpos || !wbquat) return fail("kp_sim_fk_head_backward: null qpos / wbpos / wbquat");
    if (!grad_qpos) return fail("kp_sim_fk_head_backward: null output");
    if (n_rows == 0) return 0;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(kp::launch_fk_head_grad(kp::FkHeadGradArgs{n_rows, qpos, wbpos, wbquat, grad_wbpos, grad_hpos, grad_hquat, grad_qpos_add, grad_qpos,
                                                      s->T.body_parent, s->T.body_subtree}, s->stream));
    return 0;
}

// ---- the observation with a context / `of` block (kp_obs_ctx.hip)
static int check_obs_ext(const char* who, const kp_obs_ext* x) {
    const std::string w(who);
    if (!x) return fail(w + ": null kp_obs_ext");
    if (x->ctx_dim < 0 || x->of_dim < 0) return fail(w + ": negative ctx_dim / of_dim");
    if (x->of_dim > 0 && !x->of) return fail(w + ": of_dim > 0 with a null `of` table");
    if (x->ctx_dim > 0 && x->ctx_feat && (x->ctx_stride_row < 1 || x->ctx_stride_t < 1)) return fail(w + ": ctx_feat needs strides >= 1 (in floats)");
    if (x->of_dim > 0 && (x->of_stride_row < 1 || x->of_stride_t < 1)) return fail(w + ": `of` needs strides >= 1 (in floats)");
    return 0;
}

int kp_sim_obs_ar_ex(kp_sim* s, const kp_ctx* c, const kp_obs_ext* x, float* out) {
    if (check_obs_ar_args("kp_sim_obs_ar_ex", s, c, out)) return -1;
    if (check_obs_ext("kp_sim_obs_ar_ex", x)) return -1;
    HIP_OK(hipSetDevice(s->device));
    kp::ObsArCtxArgs A{};
    A.n = s->n; A.vel = s->ar_obs_vel; A.head = s->ar_obs_head; A.action = s->ar_obs_action;
    A.T = c->T; A.head_pose = c->head_pose; A.head_vels = c->head_vels; A.obj_rel = c->obj_head_relative_poses; A.action_one_hot = c->action_one_hot;
    A.obj_qpos = c->obj_qpos; A.cur_t = c->cur_t; A.row = c->row;
    A.ctx_dim = x->ctx_dim; A.ctx_feat = x->ctx_dim > 0 ? x->ctx_feat : nullptr; A.ctx_stride_row = x->ctx_stride_row; A.ctx_stride_t = x->ctx_stride_t;
    A.of_dim = x->of_dim; A.of = x->of_dim > 0 ? x->of : nullptr; A.of_stride_row = x->of_stride_row; A.of_stride_t = x->of_stride_t;
    A.qpos = s->st.qpos; A.qvel = s->st.qvel; A.xpos = s->st.xpos; A.xquat = s->st.xquat; A.out = out;
    HIP_OK(kp::launch_obs_ar_ctx(A, s->stream));
    return 0;
}

int kp_sim_obs_ar_ex_backward(kp_sim* s, const kp_ctx* c, const kp_obs_ext* x, int n_rows, int grad_width, const float* qpos, const float* wbpos,
                              const float* wbquat, const float* grad_obs, const float* grad_obj_2_head, float* grad_qpos, float* grad_qvel,
                              float* grad_hpos, float* grad_hquat, float* grad_ctx) {
    const char* who = "kp_sim_obs_ar_ex_backward";
    if (check_obs_ar_grad(who, s) || check_obs_ext(who, x) || check_obs_ar_grad_rows(who, s, n_rows)) return -1;
    const int pitch = x->ctx_dim + s->ar_obs_dim + x->of_dim;
    if (grad_width != pitch)
        return fail("kp_sim_obs_ar_ex_backward: grad_obs is " + std::to_string(grad_width) + " wide, the row " + std::to_string(pitch) + " (" +
                    std::to_string(x->ctx_dim) + " + " + std::to_string(s->ar_obs_dim) + " + " + std::to_string(x->of_dim) + ")");
    return obs_ar_base_backward(who, s, c, n_rows, pitch, x->ctx_dim, qpos, wbpos, wbquat, grad_obs, grad_obj_2_head, grad_qpos, grad_qvel, grad_hpos, grad_hquat,
                                grad_ctx);
}

// ---- the sampler's records at a row with a context / `of` block: the same kernels (the width is their argument), obs_dim = ctx_dim + base + of_dim
static int check_wide_width(const char* who, int obs_dim, int ctx_dim, int of_dim) {
    if (ctx_dim < 0 || of_dim < 0 || !ar_obs_width_known(obs_dim - ctx_dim - of_dim))
        return fail(std::string(who) + ": obs_dim must be ctx_dim + one of " KP_AR_OBS_WIDTHS " + of_dim, got " + std::to_string(obs_dim) + " with ctx_dim " +
                    std::to_string(ctx_dim) + ", of_dim " + std::to_string(of_dim));
    return 0;
}

int kp_rollout_record_pre_x(const kp_record_pre* r, int obs_dim, int ctx_dim, int of_dim, void* stream) {
    if (!r || r->n <= 0 || r->T <= 0 || r->t < 0 || r->t >= r->T) return fail("kp_rollout_record_pre_x: bad arguments");
    if (check_wide_width("kp_rollout_record_pre_x", obs_dim, ctx_dim, of_dim)) return -1;
    return record_pre("kp_rollout_record_pre_x", r, obs_dim, stream);
}

int kp_rollout_record_post_x(const kp_record_post* r, int obs_dim, int ctx_dim, int of_dim, void* stream) {
    if (!r || r->n <= 0 || r->T <= 0 || r->t < 0 || r->t >= r->T) return fail("kp_rollout_record_post_x: bad arguments");
    if (check_wide_width("kp_rollout_record_post_x", obs_dim, ctx_dim, of_dim)) return -1;
    return record_post("kp_rollout_record_post_x", r, obs_dim, stream);
}

// ---- the ring refill of the wide context tables (k_ctx_rows_write, kp_obs_ctx.hip)
static bool on_device(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }      // plain host memory: not registered with the runtime
    return at.type == hipMemoryTypeDevice;
}

int kp_ctx_rows_write(int m, int R, int T, int Tp, int ctx_dim, int of_dim, const int64_t* rows, const int64_t* rows_host, const float* seq, const float* of,
                      float* ctx_table, float* of_table, void* stream) {
    const std::string w("kp_ctx_rows_write: ");
    if (m < 0 || R < 1 || T < 1 || ctx_dim < 0 || of_dim < 0) return fail(w + "bad sizes");
    if (Tp < 1 || Tp > T) return fail(w + "clips of " + std::to_string(Tp) + " frames do not fit tables of " + std::to_string(T) + " (1 <= T' <= T)");
    if (ctx_dim > 0 && !ctx_table) return fail(w + "ctx_dim " + std::to_string(ctx_dim) + " with a null context table");
    if (of_dim > 0 && !of_table) return fail(w + "of_dim " + std::to_string(of_dim) + " with a null `of` table");
    if (ctx_dim == 0) ctx_table = nullptr;
    if (of_dim == 0) of_table = nullptr;
    if (m == 0 || (!ctx_table && !of_table)) return 0;
    if (!rows || !rows_host) return fail(w + "null rows (the device array and its host copy)");
    if ((ctx_table && !seq) || (of_table && !of)) return fail(w + "a table without its source");
    if ((long long)m * T > INT_MAX) return fail(w + "m * T exceeds 2^31 - 1 blocks");
    for (int c = 0; c < m; c++)
        if (rows_host[c] < 0 || rows_host[c] >= R) return fail(w + "row " + std::to_string((long long)rows_host[c]) + " of clip " + std::to_string(c) + " is outside [0, " + std::to_string(R) + ")");
    for (const void* p : {(const void*)rows, (const void*)(ctx_table ? seq : nullptr), (const void*)(of_table ? of : nullptr), (const void*)ctx_table, (const void*)of_table})
        if (p && !on_device(p)) return fail(w + "rows, sources and tables must be device memory (a host pointer was given)");
    HIP_OK(kp::launch_ctx_rows_write(kp::CtxRowsArgs{m, R, T, Tp, ctx_dim, of_dim, (const long long*)rows, seq, of, ctx_table, of_table}, (hipStream_t)stream));
    return 0;
}

int kp_sim_contact_forces(kp_sim* s, int actuation, const float* act, const uint8_t* mask, const kp_contact_out* out) {
    if (!s) return fail("kp_sim_contact_forces: null handle");
    if (!out) return fail("kp_sim_contact_forces: null out");
    if (!out->ncon && !out->contact && !out->wrench && !out->qfrc_constraint && !out->qacc && !out->torque && !out->obj_qacc)
        return fail("kp_sim_contact_forces: every output of out is null");
    if (actuation < 0 || actuation > 2) return fail("kp_sim_contact_forces: actuation must be 0 (none), 1 (torque) or 2 (controller)");
    if (actuation != 0 && !act) return fail("kp_sim_contact_forces: act is null with actuation 1 or 2");
    if (s->model->threads != 64) return fail("kp_sim_contact_forces: needs a handle with threads_per_env = 64");
    HIP_OK(hipSetDevice(s->device));
    // the step kernels' argument pack without substeps and without a job queue; the kernel reads the state rows and the warm start only
    StepPlan p{};
    kp::StepArgs A = step_args(s, p, 0, nullptr, mask, nullptr);
    A.warm_extrap = 0.f; A.prof = nullptr; A.dbg_contacts = nullptr; A.order = nullptr;
    const kp::ContactOut O{out->ncon, out->contact, out->wrench, out->qfrc_constraint, out->qacc, out->torque, out->obj_qacc};
    kp::launch_contact_forces(A, s->xc, s->obj.on, s->xc_on, actuation, act, mask, O, s->stream);
    return launched();
}

// ---- the rows tools: read-only kernels on motion rows the caller passes, one wavefront per row.  rows_begin is the preamble of
// their entry points: the handle and n_rows, then own() -- the entry point's checks of its own arguments, 0 or fail's -1 -- then what the handle must
// offer; every refusal comes before the first HIP call.  Returns -1: refused; 0: no rows, nothing to do; 1: go -- the device is set and A.T / A.P /
// A.n_rows are filled.  obj_given: the call carries obj_qpos.  (A generic lambda: this part of the file has C linkage, which a template cannot have.)
static const auto rows_begin = [](const char* who, kp_sim* s, int n_rows, bool obj_given, auto& A, auto own) -> int {
    const auto no = [who](const char* what) { return fail(std::string(who) + ": " + what); };
    if (!s) return no("null handle");
    if (n_rows < 0) return no("n_rows < 0");
    if (own()) return -1;
    if (s->model->threads != 64) return no("needs a handle with threads_per_env = 64");
    if (obj_given && !s->obj.d_geoms) return no("obj_qpos given but the model blob has no object geoms");
    if (n_rows == 0) return 0;
    HIP_OK(hipSetDevice(s->device));
    A.T = s->T; A.P = s->P; A.n_rows = n_rows;
    return 1;
};

// the first null among named arguments: "<who>: null <name>"
static int refuse_null(const char* who, std::initializer_list<std::pair<const char*, const void*>> args) {
    for (const auto& a : args)
        if (!a.second) return fail(std::string(who) + ": null " + a.first);
    return 0;
}

// named floats that must be > 0 (!(x > 0) also refuses a NaN) and, where `finite`, not +inf either
static int refuse_not_positive(const char* who, std::initializer_list<std::pair<const char*, float>> fields, bool finite) {
    for (const auto& f : fields)
        if (!(f.second > 0.f) || (finite && !std::isfinite(f.second)))
            return fail(std::string(who) + ": " + f.first + " must be > 0" + (finite ? " and finite" : ""));
    return 0;
}

// The static geoms of motion rows (kp_sim_inverse_dynamics, kp_sim_estimate_contacts), placed by the kernel kp_sim_set_objects uses (static mode) into the
// call's scratch: per row the geoms [8,17], then what that kernel stores besides (object block [35], velocities [30], warm start [12], geom count, slots),
// none of which the callers read.  Stream-ordered: the next call's placement waits for this call's kernel.
static int place_static_rows(kp_sim* s, int n_rows, const float* obj_qpos, const float** geoms_out, const int** ngeom_out) {
    constexpr size_t GW = kp::D_MAXGEOM * 17, PER_ROW = GW + 35 + 30 + 6 * kp::D_MAXOBJ + 1 + 1;
    InvDynScratch& sc = s->idyn;
    if ((size_t)n_rows > sc.rows) {
        if (sc.buf) { HIP_OK(hipStreamSynchronize(s->stream)); HIP_OK(hipFree(sc.buf)); sc.buf = nullptr; sc.rows = 0; }
        HIP_OK(hipMalloc((void**)&sc.buf, sizeof(float) * PER_ROW * (size_t)n_rows));
        sc.rows = (size_t)n_rows;
    }
    const size_t R = (size_t)n_rows;
    float* geoms = sc.buf; float* oq = geoms + R * GW; float* ov = oq + R * 35; float* ow = ov + R * 30;
    int* ngeom = (int*)(ow + R * 6 * kp::D_MAXOBJ);
    signed char* slot = (signed char*)(ngeom + R);
    static_assert(kp::D_MAXOBJ <= 4, "the slot bytes of a row fit the one word the scratch keeps for them");
    hipLaunchKernelGGL(k_set_objects, dim3((n_rows + 63) / 64), dim3(64), 0, s->stream, n_rows, obj_qpos, (const uint8_t*)nullptr, oq, geoms, ngeom,
                       s->obj.d_geoms, s->obj.d_mass, s->obj.n_geoms, s->obj.n_obj, 0, slot, ov, ow, (const int*)nullptr, (const float*)nullptr, (float*)nullptr);
    HIP_OK(hipGetLastError());
    *geoms_out = geoms; *ngeom_out = ngeom;
    return 0;
}

int kp_sim_inverse_dynamics(kp_sim* s, int n_rows, const float* qpos, const float* qvel, const float* qacc, const float* obj_qpos, const kp_invdyn_out* out) {
    const char* who = "kp_sim_inverse_dynamics";
    kp::InvDynArgs A{};
    const int go = rows_begin(who, s, n_rows, obj_qpos != nullptr, A, [&] {
        if (refuse_null(who, {{"qpos", qpos}, {"out", out}})) return -1;
        if (!out->qfrc_inverse && !out->qfrc_constraint && !out->qfrc_bias && !out->contact && !out->net_wrench && !out->ncon)
            return fail("kp_sim_inverse_dynamics: every output of out is null");
        return 0;
    });
    if (go <= 0) return go;
    A.qpos = qpos; A.qvel = qvel; A.qacc = qacc;
    A.O = kp::InvDynOut{out->qfrc_inverse, out->qfrc_constraint, out->qfrc_bias, out->contact, out->net_wrench, out->ncon};
    if (obj_qpos && place_static_rows(s, n_rows, obj_qpos, &A.geoms, &A.ngeom)) return -1;
    kp::launch_inverse_dynamics(A, obj_qpos != nullptr, s->stream);
    return launched();
}

void kp_estimate_cfg_default(const kp_model* m, kp_estimate_cfg* c) {
    if (!c) return;
    double mass = 0.0, g = 9.81;
    if (m) {
        for (double b : m->h.body_mass) mass += b;
        g = std::sqrt(m->gravity_x * m->gravity_x + m->gravity_y * m->gravity_y + m->gravity_z * m->gravity_z);
    }
    const double bw = mass * g;                     // body weight; without a model (or without gravity) the weights come out non-finite and the call refuses them
    c->reach = 0.03f;
    c->w_f = (float)(1.0 / (bw * bw)); c->w_m = (float)(1.0 / (bw * bw));       // 1 / (m g)^2 and 1 / (m g x 1 m)^2
    c->rho = (float)(1e-3 / (bw * bw));
    c->mu = 0.f;
    c->n_iters = 20;
}

int kp_sim_estimate_contacts(kp_sim* s, int n_rows, const float* qpos, const float* qvel, const float* qacc, const float* obj_qpos, const kp_estimate_cfg* cfg,
                             const kp_estimate_out* out) {
    const char* who = "kp_sim_estimate_contacts";
    kp::EstimateArgs A{};
    const int go = rows_begin(who, s, n_rows, obj_qpos != nullptr, A, [&] {
        if (refuse_null(who, {{"qpos", qpos}, {"cfg", cfg}, {"out", out}})) return -1;
        if (!out->qfrc_inverse && !out->qfrc_contact && !out->contact && !out->lambda && !out->resid && !out->net_wrench && !out->ncon && !out->info)
            return fail("kp_sim_estimate_contacts: every output of out is null");
        if (refuse_not_positive(who, {{"reach", cfg->reach}, {"w_f", cfg->w_f}, {"w_m", cfg->w_m}, {"rho", cfg->rho}}, true)) return -1;
        if (!(cfg->mu >= 0.f) || !std::isfinite(cfg->mu)) return fail("kp_sim_estimate_contacts: mu must be >= 0 and finite (0: the model's)");
        if (cfg->n_iters < 0) return fail("kp_sim_estimate_contacts: n_iters < 0");
        return 0;
    });
    if (go <= 0) return go;
    A.P.margin = cfg->reach;                        // the detection distance of the collision pass; everything else is the model's
    if (cfg->mu > 0.f) A.P.mu = cfg->mu;
    A.qpos = qpos; A.qvel = qvel; A.qacc = qacc;
    A.sf = (float)std::sqrt((double)cfg->w_f); A.sm = (float)std::sqrt((double)cfg->w_m); A.rho_hat = (float)((double)cfg->rho / (double)cfg->w_f);
    A.n_iters = cfg->n_iters;
    A.O = kp::EstimateOut{out->qfrc_inverse, out->qfrc_contact, out->contact, out->lambda, out->resid, out->net_wrench, out->ncon, out->info};
    if (obj_qpos && place_static_rows(s, n_rows, obj_qpos, &A.geoms, &A.ngeom)) return -1;
    kp::launch_estimate_contacts(A, obj_qpos != nullptr, s->stream);
    return launched();
}

int kp_sim_body_motion(kp_sim* s, int n_rows, const float* qpos, const float* qvel, const float* qacc, const kp_motion_out* out) {
    const char* who = "kp_sim_body_motion";
    kp::BodyMotionArgs A{};
    const int go = rows_begin(who, s, n_rows, false, A, [&] {
        if (refuse_null(who, {{"qpos", qpos}, {"out", out}})) return -1;
        if (!out->body_vel && !out->body_acc && !out->body_com_vel && !out->centroid) return fail("kp_sim_body_motion: every output of out is null");
        return 0;
    });
    if (go <= 0) return go;
    A.qpos = qpos; A.qvel = qvel; A.qacc = qacc;
    A.O = kp::BodyMotionOut{out->body_vel, out->body_acc, out->body_com_vel, out->centroid};
    kp::launch_body_motion(A, s->stream);
    return launched();
}

int kp_sim_point_jacobian(kp_sim* s, int n_rows, const float* qpos, const int32_t* body, const float* offset, float* J) {
    const char* who = "kp_sim_point_jacobian";
    kp::PointJacArgs A{};
    const int go = rows_begin(who, s, n_rows, false, A, [&] { return refuse_null(who, {{"qpos", qpos}, {"body", body}, {"J", J}}); });
    if (go <= 0) return go;
    A.qpos = qpos; A.body = body; A.offset = offset; A.J = J;
    kp::launch_point_jacobian(A, s->stream);
    return launched();
}

void kp_fit_cfg_default(kp_fit_cfg* c) {
    if (!c) return;
    c->n_iters = 30;
    c->mu0 = 1e-2f; c->mu_min = 1e-7f; c->mu_max = 1e6f; c->mu_up = 8.f; c->mu_down = 0.3f;
    for (int d = 0; d < kp::D_NV; d++) c->damp[d] = 1.f;
    c->clamp_limits = 0;
}

int kp_sim_fit_pose(kp_sim* s, int n_rows, const kp_fit_in* in, const kp_fit_cfg* cfg, const kp_fit_out* out) {
    const char* who = "kp_sim_fit_pose";
    kp::FitPoseArgs A{};
    const int go = rows_begin(who, s, n_rows, false, A, [&] {
        if (refuse_null(who, {{"in", in}, {"cfg", cfg}, {"out", out}}) || refuse_null(who, {{"qpos0", in->qpos0}, {"tgt_pos", in->tgt_pos}})) return -1;
        if (!in->q_prior != !in->w_prior) return fail("kp_sim_fit_pose: q_prior and w_prior go together (one of them is null)");
        if (refuse_null(who, {{"out qpos", out->qpos}, {"out info", out->info}})) return -1;
        if (cfg->n_iters < 0) return fail("kp_sim_fit_pose: n_iters < 0");
        // +inf passes here, where kp_sim_estimate_contacts refuses it
        if (refuse_not_positive(who, {{"mu0", cfg->mu0}, {"mu_min", cfg->mu_min}, {"mu_max", cfg->mu_max}, {"mu_up", cfg->mu_up}, {"mu_down", cfg->mu_down}}, false)) return -1;
        for (int d = 0; d < kp::D_NV; d++)
            if (!(cfg->damp[d] > 0.f)) return fail("kp_sim_fit_pose: damp[" + std::to_string(d) + "] must be > 0");
        return 0;
    });
    if (go <= 0) return go;
    A.qpos0 = in->qpos0; A.tgt_pos = in->tgt_pos; A.tgt_quat = in->tgt_quat; A.w_pos = in->w_pos; A.w_rot = in->w_rot; A.q_prior = in->q_prior; A.w_prior = in->w_prior;
    A.n_iters = cfg->n_iters; A.clamp_limits = cfg->clamp_limits;
    A.mu0 = cfg->mu0; A.mu_min = cfg->mu_min; A.mu_max = cfg->mu_max; A.mu_up = cfg->mu_up; A.mu_down = cfg->mu_down;
    for (int d = 0; d < kp::D_NV; d++) A.damp[d] = cfg->damp[d];
    A.qpos = out->qpos; A.info = out->info; A.dq = out->dq;
    kp::launch_fit_pose(A, s->stream);
    return launched();
}

void kp_fit_points_cfg_default(kp_fit_points_cfg* c) {
    if (!c) return;
    kp_fit_cfg_default(&c->fit);
    c->w_floor = 0.f; c->floor_z = 0.f;
}

// what kp_sim_fit_points and kp_sim_fit_scene check of the arguments they share: 0, or fail's -1
// image: kp_sim_fit_image's rule for what must be present (pt_tgt may be null there; the caller checks the rest)
static int fit_points_refuse(const char* who, const kp_marker_set* markers, const kp_fit_points_in* in, const kp_fit_points_cfg* cfg, const kp_fit_points_out* out, bool image = false) {
    const std::string w = std::string(who) + ": ";
    if (refuse_null(who, {{"markers", markers}, {"in", in}, {"cfg", cfg}, {"out", out}})) return -1;
    const int K = markers->n_points;
    if (K < 0 || K > MarkerScratch::MAXK) return fail(w + "n_points must be 0 .. " + std::to_string(MarkerScratch::MAXK));
    if (K > 0 && refuse_null(who, {{"pt_body", markers->pt_body}, {"pt_offset", markers->pt_offset}})) return -1;
    for (int k = 0; k < K; k++) {
        if (markers->pt_body[k] < 0 || markers->pt_body[k] >= kp::D_NB) return fail(w + "pt_body[" + std::to_string(k) + "] must be 0 .. 23");
        for (int i = 0; i < 3; i++)
            if (!std::isfinite(markers->pt_offset[3 * k + i])) return fail(w + "pt_offset[" + std::to_string(k) + "] must be finite");
    }
    if (refuse_null(who, {{"qpos0", in->qpos0}})) return -1;
    if (!image && K > 0 && refuse_null(who, {{"pt_tgt", in->pt_tgt}})) return -1;
    if (!image && K == 0 && !in->tgt_pos) return fail(w + "nothing to fit (n_points == 0 and null tgt_pos)");
    if (!in->q_prior != !in->w_prior) return fail(w + "q_prior and w_prior go together (one of them is null)");
    if (refuse_null(who, {{"out qpos", out->qpos}, {"out info", out->info}})) return -1;
    const kp_fit_cfg& f = cfg->fit;
    if (f.n_iters < 0) return fail(w + "n_iters < 0");
    if (refuse_not_positive(who, {{"mu0", f.mu0}, {"mu_min", f.mu_min}, {"mu_max", f.mu_max}, {"mu_up", f.mu_up}, {"mu_down", f.mu_down}}, false)) return -1;      // as kp_sim_fit_pose
    for (int d = 0; d < kp::D_NV; d++)
        if (!(f.damp[d] > 0.f)) return fail(w + "damp[" + std::to_string(d) + "] must be > 0");
    if (!(cfg->w_floor >= 0.f) || !std::isfinite(cfg->w_floor)) return fail(w + "w_floor must be >= 0 and finite");
    if (!std::isfinite(cfg->floor_z)) return fail(w + "floor_z must be finite");
    return 0;
}

// the marker set ordered by body into the handle's scratch, and the argument block of the two kernels filled from the C structs
static int fit_points_fill(kp_sim* s, kp::FitPointsArgs& A, const kp_marker_set* markers, const kp_fit_points_in* in, const kp_fit_points_cfg* cfg, const kp_fit_points_out* out) {
    // the marker set ordered by body (stable: a body's points keep the caller's order): offsets [K,3] | perm [K] | adr [25]
    const int K = markers->n_points;
    std::vector<uint32_t> tab((size_t)4 * K + 25);
    {
        float* off = (float*)tab.data();
        int32_t* perm = (int32_t*)tab.data() + 3 * K;
        int32_t* adr = perm + K;
        int j = 0;
        for (int b = 0; b < kp::D_NB; b++) {
            adr[b] = j;
            for (int k = 0; k < K; k++)
                if (markers->pt_body[k] == b) { perm[j] = k; for (int i = 0; i < 3; i++) off[3 * j + i] = markers->pt_offset[3 * k + i]; j++; }
        }
        adr[kp::D_NB] = j;
    }
    MarkerScratch& mk = s->mk;
    if (!mk.buf) {
        HIP_OK(hipMalloc(&mk.buf, sizeof(uint32_t) * MarkerScratch::WORDS));
        HIP_OK(hipMemset((uint32_t*)mk.buf + MarkerScratch::ZEROS, 0, sizeof(uint32_t) * 25));
    }
    if (tab != mk.host) {      // another marker set: the kernels of earlier calls may still read the old one
        HIP_OK(hipStreamSynchronize(s->stream));
        mk.host.clear();
        HIP_OK(hipMemcpy(mk.buf, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
        mk.host = tab;
    }
    A.n_points = K;
    A.pt_off = (const float*)mk.buf; A.pt_perm = (const int32_t*)mk.buf + 3 * K; A.pt_adr = A.pt_perm + K;
    A.qpos0 = in->qpos0; A.pt_tgt = in->pt_tgt; A.pt_w = in->pt_w; A.tgt_pos = in->tgt_pos; A.tgt_quat = in->tgt_quat; A.w_pos = in->w_pos; A.w_rot = in->w_rot;
    A.q_prior = in->q_prior; A.w_prior = in->w_prior;
    const kp_fit_cfg& f = cfg->fit;
    A.n_iters = f.n_iters; A.clamp_limits = f.clamp_limits;
    A.mu0 = f.mu0; A.mu_min = f.mu_min; A.mu_max = f.mu_max; A.mu_up = f.mu_up; A.mu_down = f.mu_down;
    for (int d = 0; d < kp::D_NV; d++) A.damp[d] = f.damp[d];
    A.w_floor = cfg->w_floor; A.floor_z = cfg->floor_z;
    A.qpos = out->qpos; A.info = out->info; A.dq = out->dq; A.pt_err = out->pt_err;
    return 0;
}

int kp_sim_fit_points(kp_sim* s, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const kp_fit_points_cfg* cfg, const kp_fit_points_out* out) {
    const char* who = "kp_sim_fit_points";
    kp::FitPointsArgs A{};
    const int go = rows_begin(who, s, n_rows, false, A, [&] { return fit_points_refuse(who, markers, in, cfg, out); });
    if (go <= 0) return go;
    if (fit_points_fill(s, A, markers, in, cfg, out)) return -1;
    kp::launch_fit_points(A, s->stream);
    return launched();
}

void kp_fit_scene_cfg_default(kp_fit_scene_cfg* c) {
    if (!c) return;
    kp_fit_points_cfg_default(&c->pts);
    c->w_obj = 0.f;
}

int kp_sim_fit_scene(kp_sim* s, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const float* obj_qpos, const kp_fit_scene_cfg* cfg, const kp_fit_scene_out* out) {
    const char* who = "kp_sim_fit_scene";
    kp::FitSceneArgs A{};
    const int go = rows_begin(who, s, n_rows, obj_qpos != nullptr, A, [&] {
        if (refuse_null(who, {{"cfg", cfg}})) return -1;
        if (fit_points_refuse(who, markers, in, &cfg->pts, out)) return -1;
        if (!(cfg->w_obj >= 0.f) || !std::isfinite(cfg->w_obj)) return fail("kp_sim_fit_scene: w_obj must be >= 0 and finite");
        return 0;
    });
    if (go <= 0) return go;
    if (fit_points_fill(s, A, markers, in, &cfg->pts, out)) return -1;
    A.w_obj = cfg->w_obj;
    if (obj_qpos && place_static_rows(s, n_rows, obj_qpos, &A.geoms, &A.ngeom)) return -1;
    kp::launch_fit_scene(A, s->stream);
    return launched();
}

void kp_fit_image_cfg_default(kp_fit_image_cfg* c) {
    if (!c) return;
    kp_fit_scene_cfg_default(&c->scene);
    c->z_near = 0.05f;
}

int kp_sim_fit_image(kp_sim* s, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const float* obj_qpos, const kp_fit_image_obs* obs, const kp_fit_image_cfg* cfg,
                     const kp_fit_image_out* out) {
    const char* who = "kp_sim_fit_image";
    kp::FitImageArgs A{};
    const int C = obs ? obs->n_cams : 0;
    const int go = rows_begin(who, s, n_rows, obj_qpos != nullptr, A, [&] {
        if (refuse_null(who, {{"cfg", cfg}, {"out", out}})) return -1;
        const kp_fit_points_out pout{out->qpos, out->info, out->dq, out->pt_err};
        if (fit_points_refuse(who, markers, in, &cfg->scene.pts, &pout, true)) return -1;
        if (!(cfg->scene.w_obj >= 0.f) || !std::isfinite(cfg->scene.w_obj)) return fail("kp_sim_fit_image: w_obj must be >= 0 and finite");
        if (!(cfg->z_near > 0.f) || !std::isfinite(cfg->z_near)) return fail("kp_sim_fit_image: z_near must be > 0 and finite");
        if (C < 0 || C > 8) return fail("kp_sim_fit_image: n_cams must be 0 .. 8");
        if (C > 0 && obs->camera_rows != 1 && obs->camera_rows != n_rows) return fail("kp_sim_fit_image: camera_rows must be 1 or n_rows");
        if (C > 0 && refuse_null(who, {{"cam", obs->cam}, {"uv", obs->uv}})) return -1;
        const int K = markers->n_points;
        if (!(K > 0 && in->pt_tgt) && !in->tgt_pos && !(K > 0 && C > 0)) return fail("kp_sim_fit_image: nothing to fit (no 3D targets, null tgt_pos and no observations)");
        return 0;
    });
    if (go <= 0) return go;
    const kp_fit_points_out pout{out->qpos, out->info, out->dq, out->pt_err};
    if (fit_points_fill(s, A, markers, in, &cfg->scene.pts, &pout)) return -1;
    A.img_adr = A.pt_adr;
    if (!in->pt_tgt) A.pt_adr = (const int32_t*)s->mk.buf + MarkerScratch::ZEROS;      // no 3D term: the shared walks find no point
    A.w_obj = cfg->scene.w_obj;
    A.n_cams = C; A.camera_rows = C > 0 ? obs->camera_rows : 1;
    A.cam = C > 0 ? obs->cam : nullptr; A.uv = C > 0 ? obs->uv : nullptr; A.uv_w = C > 0 ? obs->uv_w : nullptr;
    A.z_near = cfg->z_near;
    A.uv_err = C > 0 ? out->uv_err : nullptr;
    if (obj_qpos && place_static_rows(s, n_rows, obj_qpos, &A.geoms, &A.ngeom)) return -1;
    kp::launch_fit_image(A, s->stream);
    return launched();
}

}  // extern "C"

// ---- model compiler behind the ABI (host only).  Included last: its `#pragma clang fp contract(off)` (bit-reproducible double arithmetic,
// shared rule for rule with kinpoly_amd/model_compiler.py) must not reach the kernels above.
#include "kp_compile.hpp"

extern "C" {

int kp_model_compile(const char* xml_path, const char* uhc_yml_path, const char* out_kpm_path) {
    if (!xml_path || !out_kpm_path) return fail("kp_model_compile: null argument");
    std::string err;
    if (kpc::compile(xml_path, uhc_yml_path, out_kpm_path, err) != 0) return fail("kp_model_compile: " + err);
    return 0;
}

kp_model* kp_model_load_xml(const char* xml_path, const char* uhc_yml_path) {
    if (!xml_path) { fail("kp_model_load_xml: null argument"); return nullptr; }
    char tmpl[] = "/tmp/kp_model_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0) { fail("kp_model_load_xml: cannot create a temporary file"); return nullptr; }
    close(fd);
    kp_model* m = nullptr;
    if (kp_model_compile(xml_path, uhc_yml_path, tmpl) == 0) m = kp_model_load(tmpl);
    std::remove(tmpl);
    return m;
}

}  // extern "C"

