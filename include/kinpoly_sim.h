/* kinpoly_sim.h -- C ABI of libkinpoly_sim.so: the batched MI355X-native replacement of the
 * MuJoCo rollout path of KinPoly (one call = N environments).
 *
 * The reference has no FFI for this path; the two Python surfaces it replaces are
 *   B1  HumanoidAREnv            kin_poly/envs/humanoid_ar_v1.py:28-516  (+ uhc/envs/humanoid_im.py)
 *   B2  the mujoco-py object API uhc/khrylib/rl/envs/common/mujoco_env.py:23-24,87,99-103,
 *                                 uhc/envs/humanoid_im.py:193,203,217,423,426,504,516,527
 * Each entry point cites the reference interface it stands in for.  INTEGRATION.md shows the ctypes
 * binding a reference maintainer adds.
 *
 * Conventions
 *   - every array argument is a DEVICE pointer (hipMalloc / torch tensor .data_ptr()) to a dense
 *     row-major float32 array [n_envs, dim]; `env_mask` is uint8 [n_envs] (1 = apply) or NULL = all;
 *   - all work is enqueued on the HIP stream given to kp_sim_create (no implicit sync), except
 *     kp_sim_diag() which synchronises that stream;
 *   - return value 0 = ok, negative = error (kp_last_error() gives the text, thread-local);
 *   - handles are opaque; one kp_sim is used by one host thread at a time.
 *
 * Several handles in one process
 *   Any number of kp_sim handles (of the same or of different models) may live in a process and run at the same time on different
 *   HIP streams (kp_sim_create's stream / kp_sim_set_stream): a handle owns every array its kernels write -- state, job queue and its
 *   counters, status words, timing events -- and the library keeps no process-wide device state (no __constant__ / __device__ symbols),
 *   so launches of different handles do not interact except by sharing the machine.  The persistent job-queue kernel of the control step
 *   (kp_step_queue_kernel) waits only for jobs that a RUNNING wavefront of the same launch is about to publish, never for a wavefront that
 *   has yet to become resident, so co-scheduled launches cannot starve each other into a deadlock; a wait that exceeds 2 s raises the
 *   handle's stall flag (kp_sim_status_device word 2 -> the next host-synchronising call fails) instead of hanging.
 *   Measured on MI355X (tests/test_gpu_round5.py::test_concurrent_handles_...; tools/micro/concurrent_handles.py, profiles/r05): two and
 *   three handles of 4096 envs each -- floor scenes and scenes with free objects, in any mix -- stepped 50 control steps on their own
 *   streams with no host synchronisation end in the same states, bit for bit, as when they run one after the other, with clean status
 *   words; the round of launches is 5 ... 20 % shorter than the serial one (the launches' tails overlap).  (The device hang that rounds
 *   3 / 4 saw with THREE sub-batched env-steps on three streams is reproduced by the policies' library GEMMs ALONE at 1365 = 4096 / 3 rows on
 *   three streams -- no kernel of this library in the loop -- and not at 1024 rows: profiles/r05/gemm_streams_probe.log)
 *   What is NOT supported: two host threads in one handle at once; one handle on two streams at once (kp_sim_set_stream moves it, the
 *   caller orders the old stream's work before the new stream's).
 */
#ifndef KINPOLY_SIM_H
#define KINPOLY_SIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct kp_model kp_model;
typedef struct kp_sim kp_sim;

/* layout constants of the SMPL humanoid (reference humanoid_im.py:30-49 qpos_lim/qvel_lim/body_lim) */
#define KP_NQ 76
#define KP_NV 75
#define KP_NU 69
#define KP_NBODY 24
#define KP_CC_OBS_DIM 784   /* get_full_obs_v1, humanoid_im.py:144-233 */
#define KP_AR_OBS_DIM 105   /* get_ar_obs_v1, humanoid_ar_v1.py:133-214 (kin_poly.yml flags): the action one-hot is the last block, [101..104] */
#define KP_AR_OBS_DIM_NO_ACTION 101   /* the same without the one-hot (use_action: false, kin_poly_wo_action.yml; humanoid_ar_v1.py:200-201): the
                                         first 101 entries of the 105-d layout.  Model option "ar_obs_action" = 0 selects it (kp_model_set_option) */
/* The observation's blocks in the reference's order (humanoid_ar_v1.py:183-201) and the model option that switches each (kp_model_set_option):
 *     height, de-headed root quaternion, joint angles    74   always
 *     qvel of the simulated humanoid (data.qvel[:75])     75   "ar_obs_vel" = 1      (use_vel, :184-185)
 *     diff_hpos, diff_hrot                                 7   "ar_obs_head" = 1     (use_head, :187-189)
 *     predicted object relative to head                    7   always                (:191-192)
 *     t_havel, t_hlvel, t_obj_relative_head               13   "ar_obs_head" = 1     (:194-198)
 *     action one-hot                                       4   "ar_obs_action" = 1   (use_action, :200-201)
 * Row widths by (head, vel, action): (1,0,1) 105, (1,0,0) 101, (1,1,1) 180, (1,1,0) 176, (0,0,1) 85, (0,0,0) 81, (0,1,1) 160, (0,1,0) 156. */
#define KP_KIN_ACTION_DIM 80
#define KP_CC_ACTION_DIM 75

/* ---- model --------------------------------------------------------------------------------------
 * replaces mujoco_py.load_model_from_path(xml) (mujoco_env.py:23): `kpm_path` is the blob
 * kinpoly_amd/model_compiler.py compiles from the same XML + STL hulls + uhc.yml gains. */
kp_model* kp_model_load(const char* kpm_path);
/* mujoco_py.load_model_from_path(xml) itself (mujoco_env.py:23), no Python: compile the reference's scene XML -- with the binary STL meshes it
 * names (resolved relative to the XML), `coordinate="global"`, mesh-hull humanoid bodies with a free root + z / y / x hinges, box / cylinder
 * free objects -- and the PD-gain table of config/uhc/uhc.yml (may be NULL: zero gains) into the blob, then load it.  kp_model_compile writes
 * the blob to a file (same bytes as kinpoly_amd/model_compiler.py up to floating-point rounding of the fields that go through a matrix
 * inverse / eigenvectors; integer tables identical). */
int kp_model_compile(const char* xml_path, const char* uhc_yml_path, const char* out_kpm_path);
kp_model* kp_model_load_xml(const char* xml_path, const char* uhc_yml_path);
void kp_model_free(kp_model*);
/* options: "contact" (0/1), "limits" (0/1), "gravity_z" ("gravity_x", "gravity_y": mjOption.gravity, 0 in the reference's XML; tilted-plane tests),
 * "actuation" (0/1, default 1; 0: ctrl = qfrc_applied = 0, i.e. do_simulation without compute_torque / rfc: torque-free motion for tests), "stale_kinematics" (0/1, default 1: SPD and
 * read-outs see the one-substep-stale derived quantities mujoco-py exposes), "solver_iter" (default: the blob's
 * mjOption.iterations = 100; cap hits are counted in kp_sim_diag), "solver_tol", "threads_per_env" (64/128/256), "dynamic_objects" (0/1);
 * scheduling only (results do not depend on them): "substeps_per_job" (default 4; 0 = one workgroup per env and control step):
 * with more envs than resident wavefront slots a control step is cut into jobs of that many substeps (the last job; each earlier job is
 * "job_taper" substeps longer, default 1: 15 = 6 + 5 + 4; 0 = uniform) which resident waves pull from a FIFO, so that the
 * launch does not end on the tail of its longest envs; "queue_slots" (0 = CUs x 8, x 6 with objects); "queue_fence" (0/1, default 1: the job hand-over is an agent-scope
 * release / acquire fence pair around relaxed write-through accesses, correct by the HIP memory model; 0 = without the fences, +0.5 %);
 * "queue_heavy" (default 160; 0 = off): a wave whose job ran at more than that percentage of the launch's mean time per substep keeps its env and runs the
 * env's next job itself instead of queueing it -- the costliest envs are the ones a launch ends on, and with two envs per slot every trip through the
 * FIFO costs them about one job's length of waiting (objects workload 6.49 -> 5.78 ms per launch; bit-identical results);
 * "lean_queue" (0/1, default 1): floor scenes' queue launches run on the lean LDS layout (12 784 B per env: 12 envs per CU = three waves per SIMD instead of
 * 8 = two; same results bit for bit), in stale mode only: with "stale_kinematics" = 0 a substep's constraint reference sits in words the lean layout gives to the
 * bias forces of the same substep, so those scenes run the full layout.  Its defaults, unless the caller sets the option: jobs of 5 + 5 + 5 substeps,
 * "queue_late" (default -1 = automatic: on with the lean layout): an env whose first job had to wait for a slot is never queued again, its wave runs its later
 * jobs itself; "queue_prio" (default -1 = automatic: 3 with the lean layout, else 0): a wave's issue priority (s_setprio) -- 1 envs known to be heavy, 2 by the
 * env's remaining jobs, 3 by its remaining substeps, re-set at every substep.  "lean_max_contacts" (<= 24): a lean job that finds more contacts in a substep
 * hands the env (before it has stored anything) to a second kernel on the full layout; "lean_adaptive" (0/1, default 1): when more than 1 / 64 of the envs did
 * so, the next 64 control steps run on the full layout (kp_sim_lean_state).
 * "lds_pad" (bytes): allocate at least that much LDS per env (experiments: fewer envs per CU with the same binary);
 * "lpt_order" (1 / 0 / -1 = default: on when free objects are simulated): longest-env-first order of the workgroups (plain launch) or of the
 * envs' first jobs in the FIFO, from the previous control step's per-env cycles;
 * "warm_extrap" (beta; default -1 = automatic: 0.75 when the scene's free objects are simulated, 0 otherwise): starting point of the constraint solve.  0 is
 * MuJoCo's: the previous substep's solution a_{k-1} (mjData.qacc_warmstart).  beta != 0 starts from a_{k-1} + beta (a_{k-1} - a_{k-2}) from the second substep
 * of a kp_sim_step_ctrl call on (every call begins with the plain warm start).  Same strictly convex problem, same minimiser, same termination tests: only the
 * iteration path changes (fewer Newton iterations where accelerations change smoothly -- falls, impacts; more on quiet standing states); results do not
 * depend on how a control step is cut into jobs.
 * "ar_obs_action" (1 / 0, default 1; anything else fails): the kinematic observation of a kp_sim created afterwards from this model -- 1: KP_AR_OBS_DIM
 * floats with the action one-hot (use_action), 0: the first KP_AR_OBS_DIM_NO_ACTION of them (use_action: false, humanoid_ar_v1.py:200-201).
 * "ar_obs_vel" (0 / 1, default 0; anything else fails): 1 puts the 75 generalised velocities the step leaves in the state rows (KP_QVEL) after the
 * pose block of that observation (use_vel).  "ar_obs_head" (1 / 0, default 1; anything else fails): 0 removes the two head-tracking blocks
 * (use_head: false).  Both are fixed in a kp_sim when it is created, like "ar_obs_action"; the layout is next to KP_AR_OBS_DIM.
 * kp_model_get_option also answers "ar_obs_dim": the row width of the three switches (105 by default).
 * The UHC config's observation (kp_sim_obs_cc_ex of a kp_sim created afterwards; humanoid_im.py:105-318), each 0 / 1 unless said otherwise, anything
 * else fails: "cc_obs_v" (0 get_full_obs, 1 get_full_obs_v1 = default, 2 get_full_obs_v2), "cc_obs_vel_root" (obs_vel 'root': qvel[:6] instead of the
 * 75 of 'full'), and obs_v 0's "cc_obs_heading", "cc_obs_deheading", "cc_obs_phase" (obs_heading, root_deheading, obs_phase; ignored by obs_v 1 / 2).
 * kp_model_get_option also answers "cc_obs_dim" (784 / 715 for obs_v 1 full / root, 640 / 571 for obs_v 2, heading + 74 + (75 | 6) + 69 + phase for
 * obs_v 0) and "cc_action_dim".
 * The UHC controller (kp_sim_step_ctrl of a kp_sim created afterwards; humanoid_im.py:433-524): "cc_action_v" (1 default: PD base pose = the target row
 * unwrapped to within pi of qpos; 0: the target row as it is, the caller installs cfg.a_ref), "cc_rfc" (1 default: implicit residual force from action
 * [69:75]; 0: none), "cc_meta_pd" (0 default; 1 meta_pd: kp / kd x clip(m + 1, 0, 10) with m = action[m0 + substep] / [m0 + substep + 15], at most 15
 * substeps per call; 2 meta_pd_joint: by joint, [m0 + j] / [m0 + 69 + j]; m0 = 69 + 6 cc_rfc).  cc_action_dim = 69 + 6 cc_rfc + (30 | 138 | 0); any
 * other value fails.  A non-default controller runs on the full layout (no lean job-queue form).
 * Every name, where its value lives and how a set value is checked or clamped is one row of the OPTIONS table in kinpoly_amd/csrc/kp_sim.hip; a refusal
 * reads "<name> must be ...", an unknown name fails to set and reads NaN. */
int kp_model_set_option(kp_model*, const char* name, double value);
double kp_model_get_option(const kp_model*, const char* name);

/* ---- simulator ------------------------------------------------------------------------------------
 * replaces MjSim(model) x N (mujoco_env.py:24) */
kp_sim* kp_sim_create(const kp_model*, int n_envs, int device_id, void* hip_stream);
void kp_sim_destroy(kp_sim*);
int kp_sim_n_envs(const kp_sim*);

/* Rebind the HIP stream all later calls enqueue on (kp_sim_create's stream otherwise).  The caller orders the two streams
 * (e.g. an event) if work is still in flight on the old one. */
int kp_sim_set_stream(kp_sim*, void* hip_stream);

/* Device pointer to uint32[4] the control-step launches maintain: [2] != 0 means a kp_step_queue_kernel launch stalled (a wave gave
 * up waiting for a job; sticky until the next kp_sim_diag reports it) -- a rollout loop can fold it into its own device-side
 * checks without a host sync.  [0], [1] are the queue's head / tail counters of the last launch. */
const uint32_t* kp_sim_status_device(kp_sim*);

/* Test / debugging read-out of data.contact: the contact set of the LAST collision pass of the last kp_sim_step_ctrl launch
 * (i.e. of the state before its final substep).  The first call arms the recording (costs a few KB of stores per env and launch
 * afterwards), later calls copy float32 [N, 1 + 64 * 9] to the HOST pointer: [0] = number of contacts, then per contact
 * {entity carrying the first geom's counterpart (0..23 hull body, 24 + k object slot), other entity (-1 world), dist, pos[3],
 * normal[3] (pointing into the first entity)}.  Synchronises. */
int kp_sim_contacts(kp_sim*, float* out_host);

/* mjf.mj_fullM(model, M, data.qM) and data.qfrc_bias as compute_desired_accel reads them (uhc/envs/humanoid_im.py:422-426):
 * M [N,75,75] (dense, symmetric, armature on the diagonal), bias [N,75]; either may be NULL.  The simulator never forms them
 * on the hot path (matrix-free solves); this read-out is for callers of the reference surface.  Same data as KP_M / KP_BIAS. */
int kp_sim_mass_matrix(kp_sim*, float* M, float* bias);

/* sim.reset() + set_state(qpos, qvel) + sim.forward()   (mujoco_env.py:86-103) for the masked envs.
 * qpos [N,76], qvel [N,75]. */
int kp_sim_set_state(kp_sim*, const float* qpos, const float* qvel, const uint8_t* env_mask);

/* self.target = smpl_humanoid.qpos_fk(target_qpos)   (humanoid_ar_v1.py:256, numpy_smpl_humanoid.py:180)
 * target_qpos [N,76] is copied; the target dict {qpos, wbpos, wbquat, bquat, body_com} is kept on device. */
int kp_sim_set_target(kp_sim*, const float* target_qpos, const uint8_t* env_mask);

/* object block of set_state: obj_qpos [N,35] = data.qpos[76:111] as reset_model builds it with convert_obj_qpos
 * (humanoid_ar_v1.py:377-381, 479-496: inactive objects parked at [(i+1)*100, 100, 0]), object velocities zero (:382).
 * Objects within 50 m of the origin (at most two: push = box + table) become free rigid bodies of the env: their
 * boxes / cylinders (XML :190-214) collide with the humanoid hulls, the floor and each other, and they are integrated
 * by the same soft-constraint solve as the humanoid.  Model option "dynamic_objects" = 0 freezes them as static obstacles.
 * Parked objects are not simulated (in the reference they only bounce on the floor 100 m away). */
int kp_sim_set_objects(kp_sim*, const float* obj_qpos, const uint8_t* env_mask);

/* Humanoid.qpos_fk_batch(qpos) (numpy_smpl_humanoid.py:124-178) on n_rows arbitrary rows, used by
 * load_context for the GT clip (humanoid_ar_v1.py:87): qpos [n_rows,76] -> qpos_out [n_rows,76] (root quat
 * normalised), wbpos [n_rows,72], wbquat [n_rows,96], bquat [n_rows,96], body_com [n_rows,72]; outputs may be NULL. */
int kp_sim_fk(kp_sim*, int n_rows, const float* qpos, float* qpos_out, float* wbpos, float* wbquat, float* bquat, float* body_com);

/* compute_physcis_metris' sim.forward() + data.contact walk (scripts/eval_pose_all.py:205-260) on n_rows arbitrary frames:
 * xpos [R,72] / xquat [R,96] body poses (kp_sim_fk's wbpos / wbquat of the rows' qpos), obj_qpos [R,35] or NULL (floor only);
 * out: pen [R] = sum over hull-vs-(floor|object) contacts of max(0, -dist - pen_margin), ncon [R] (int32), hits [R, n_obj_geom] (uint32,
 * bit b = hull b touches object geom g; reference geom id = 25 + g; n_obj_geom = the model option "n_obj_geoms").  Enqueued on the sim's
 * stream; no contact-count limit.  n_rows == 0 does nothing. */
int kp_sim_pose_contacts(kp_sim*, int n_rows, const float* xpos, const float* xquat, const float* obj_qpos, float pen_margin,
                         float* pen, int32_t* ncon, uint32_t* hits);

/* The face planes of the model's 24 convex hulls, built from the blob's hull vertices (the blob holds vertices and a neighbour graph, not faces):
 * planes4 [n,4] = (unit outward normal, d) in the body frame, n.x <= d inside; adr [nb + 1] = first plane of every body.  Either array may be NULL;
 * returns n (2302 for the shipped blobs), -1 on a null model.  Host only: works without a device.  This is the geometry kp_sim_render draws where the
 * reference's viewer (Visualizer.render, uhc/khrylib/rl/utils/visualizer.py; scripts/eval_uhc.py:85-131) draws the mesh geoms MuJoCo compiled. */
int kp_model_hull_planes(const kp_model*, float* planes4, int32_t* adr);

/* colours (r, g, b in 0..1) and far plane of kp_sim_render: one base colour per figure, one for the object geoms, the two greys of the floor's
 * 1 m checker (parity (floor(x) + floor(y)) & 1), the sky; floor hits beyond zfar metres along the ray are sky */
typedef struct { float figure[4][3], object[3], floor[2][3], sky[3], zfar; } kp_render_style;
/* light grey for figure 0, the reference's expert red (0.7, 0, 0) for figure 1, zfar = 100 */
void kp_render_style_default(kp_render_style*);

/* Offscreen frames: replaces Visualizer.render / save_screen_shots of the reference's MuJoCo GL viewer as scripts/eval_uhc.py:85-131 (--mode vis,
 * --record, --preview) and scripts/eval_pose_all.py:468-531 (--mode vis) drive it, with a ray-caster over the collision geometry: per row n_fig
 * figures (1..4, e.g. simulated and expert) given as body poses xpos [R,n_fig,72] / xquat [R,n_fig,96] (kp_sim_fk's wbpos / wbquat), the row's object
 * block obj_qpos [R,35] or NULL (floor and figures only; objects are placed as kp_sim_pose_contacts places them) and the floor z = 0.
 * camera [camera_rows,7] on the device, camera_rows = 1 or R: lookat[3], distance, azimuth, elevation, fovy (degrees), the viewer's free camera;
 * one ray per pixel centre, row 0 at the top.  style: NULL = kp_render_style_default.  Outputs [R,height,width], each may be NULL but not all:
 * geom (int32: -1 nothing, 0 floor, 100 k + 1 + b body b of figure k, 25 + g object geom g -- for figure 0 and the objects the reference's
 * geom ids), depth (float, distance along the normalised ray, +inf where nothing is hit), rgba (4 x uint8, base colour x (0.35 + 0.65 max(0,
 * -n.dir)), alpha 255).  Refused before anything is launched: n_fig outside 1..4, width or height outside 1..4096, null inputs, all outputs null,
 * obj_qpos on a blob without object geoms, more than 16 object geoms, obj_qpos on a blob with an object geom that is neither box nor cylinder or
 * that belongs to no object of the block.  Enqueued on the sim's stream; the first call uploads the plane table. */
int kp_sim_render(kp_sim*, int n_rows, int n_fig, const float* xpos, const float* xquat, const float* obj_qpos, const float* camera, int camera_rows,
                  int width, int height, const kp_render_style* style, int32_t* geom, float* depth, uint8_t* rgba);

/* The egocentric renderer: kp_sim_render's ray-caster behind a camera given as a pose (one that sits on a body and rolls with it, which the viewer's
 * free camera cannot), and for a pair of frames A and B the exact optical flow of every pixel of A.  Rows, figures, object block, style and the
 * outputs geom / depth / rgba are kp_sim_render's.  camera [camera_rows,8] on the device, camera_rows = 1 or R: eye[3], quaternion[4] (w, x, y, z,
 * world from camera, normalised by the kernel), fovy (degrees).  The camera's axes are the head body's: forward = R e_z, up = R e_y, right = -R e_x,
 * so the head's world quaternion is a camera looking where the head looks; dir = normalize(forward + sx th (W/H) right + sy th up), th = tan(fovy/2),
 * (sx, sy) the pixel centre in -1..1, row 0 at the top.  hide_body: -1, or a body 0..23 of figure 0 that is not drawn (an eye outside the head hull).
 * The B side -- xpos_b, xquat_b, camera_b, and obj_qpos_b exactly when obj_qpos is given; or all four NULL -- is the same rows one frame later.  With
 * it, the point a pixel of A shows is carried to B by the rigid motion of what was hit (floor: stays; body b of figure k: x_B + R_B R_A^T (p - x_A);
 * object geom: the same with the geom's world poses, a geom parked in B gives ok = 0; sky: the ray direction, a point at infinity) and projected
 * through camera B: c = R_camB^T (p_B - eye_B), u' = (W/2)(1 + (-c_x/c_z)/(th_B W/H)), v' = (H/2)(1 - (c_y/c_z)/th_B).  There is no visibility test in
 * B: this is the motion field of the points visible in A.  Further outputs, each may be NULL: flow float [R,H,W,2] = (u' - (px + .5), v' - (py + .5))
 * in pixels; ok uint8 [R,H,W] = c_z > 0.01 (flow is (0, 0) where ok = 0); cells float [R,grid_y,grid_x,2] = the mean flow over the ok pixels of each
 * grid cell (0 for a cell without one), which needs width = 8 a grid_x and height = 8 b grid_y with whole a, b >= 1 and is summed in a fixed order
 * without atomics: equal inputs give equal bits.  With cells alone no per-pixel array is written.  Refused before anything is launched: everything
 * kp_sim_render refuses; a B side given only in part; flow / ok / cells without a B side; a cells grid that does not divide the image into whole
 * 8 x 8 tiles; hide_body outside -1..23; camera_rows neither 1 nor R; all six outputs NULL.  Enqueued on the sim's stream. */
int kp_sim_render_ego(kp_sim*, int n_rows, int n_fig, const float* xpos, const float* xquat, const float* obj_qpos, const float* camera,
                      const float* xpos_b, const float* xquat_b, const float* obj_qpos_b, const float* camera_b, int camera_rows, int width, int height,
                      int hide_body, const kp_render_style* style, int grid_x, int grid_y,
                      int32_t* geom, float* depth, uint8_t* rgba, float* flow, uint8_t* ok, float* cells);

/* backward of qpos -> wbpos of the same rows (the autograd path through Humanoid.qpos_fk that TrajARNet.compute_loss_lite's
 * end-effector term takes, traj_ar_smpl_net.py:459-497, torch_smpl_humanoid.py:125-202): grad_qpos [n_rows,76] =
 * (d wbpos / d qpos)^T grad_wbpos [n_rows,72]; wbpos / wbquat are the outputs of the kp_sim_fk call on those rows. */
int kp_sim_fk_backward(kp_sim*, int n_rows, const float* qpos, const float* wbpos, const float* wbquat, const float* grad_wbpos, float* grad_qpos);

/* HumanoidEnv.do_simulation(cc_action, n_substeps)   (humanoid_im.py:506-533): per substep stable-PD
 * torque (compute_torque :433-480), clip, rfc_implicit (:497-504), sim.step() (:527).  cc_action [N, cc_action_dim] (75 for a default model; the
 * width of the model's cc_rfc / cc_meta_pd when the handle was created). */
int kp_sim_step_ctrl(kp_sim*, const float* cc_action, int n_substeps, const uint8_t* env_mask);

/* HumanoidAREnv.step_ar(a)   (humanoid_ar_v1.py:216-241): kin_action [N,80] -> next_qpos [N,76] */
int kp_sim_step_kin(kp_sim*, const float* kin_action, float* next_qpos);

/* The head of HumanoidAREnv.step in one launch (humanoid_ar_v1.py:246-256): kp_sim_step_begin + kp_sim_step_kin + kp_sim_set_target with the
 * kinematic step's result -- prev_bquat / prev_hpos recorded, target = qpos_fk(step_ar(kin_action)).  kin_action [N,80]. */
int kp_sim_step_head(kp_sim*, const float* kin_action);

/* get_full_obs_v1() [N,784]   (humanoid_im.py:144-233), optional ZFilter(update=False) + clip
 * (zfilter.py:58-67): pass mean/std [784] device pointers or NULL, clip <= 0 disables clipping. */
int kp_sim_obs_cc(kp_sim*, float* out, const float* zf_mean, const float* zf_std, float clip);

/* The observation the handle's cc_obs_* options select (kp_model_set_option; fixed when the handle is created), [N, kp_sim_cc_obs_dim] with the same
 * optional ZFilter + clip (zf_mean / zf_std of that width).  obs_v 1 / 2 read the target as kp_sim_obs_cc does (the caller installs expert frame t + 1);
 * obs_v 0 reads only the target's joint angles, as get_expert_kin_pose(delta_t=0) (:679): the caller installs expert frame t.  phase: device float [N]
 * = cur_t / expert len, required when the handle has cc_obs_phase (obs_v 0), and must be NULL otherwise.  A default handle writes exactly what
 * kp_sim_obs_cc writes (the same kernel).  kp_sim_obs_cc itself always writes the 784-d uhc.yml layout. */
int kp_sim_obs_cc_ex(kp_sim*, float* out, const float* zf_mean, const float* zf_std, float clip, const float* phase);
/* the handle's width of kp_sim_obs_cc_ex (-1 for NULL) */
int kp_sim_cc_obs_dim(const kp_sim*);

/* per-episode context rows the env reads each step (ar_context, humanoid_ar_v1.py:84-88).
 * Arrays are [R, T, dim] device pointers (action_one_hot [R, 4]), R >= N context rows; env e reads row `row[e]` (int32 [N], or
 * NULL: row e, R = N).  The indirection lets a sampler keep the NEXT episodes' contexts resident next to the current ones and
 * switch an env to its new clip on `done` without copying (agent_ar.py:519-537 draws a new clip per episode).  cur_t is
 * int32 [N] (env.cur_t).  obj_qpos [N,7] (per env, not per row) may be NULL (then get_obj_qpos() == [0,0,0,1,0,0,0], :465-466).
 * What the host can and cannot check: T and the null pointers are checked by every call that takes this struct: -1 and a kp_last_error text; cur_t [N] and
 * row [N] live on the device, so their VALUES are not: cur_t is clamped into the clip by the kernels (any int32 is safe), but row[e] must lie in
 * [0, R) -- a row outside the table is read out of bounds.  The same holds for the row / row_len arrays of kp_sim_reset_rows, kp_sim_post_step and of
 * the kp_record_pre struct: row_len[r] must be < ctx_T, and cur_t[e] >= -1 there (gt_target_qpos reads frame min(cur_t + 1, row_len), unclamped from below). */
typedef struct {
    int T;
    const float* head_pose;               /* [N,T,7]  ar_context['head_pose'] */
    const float* head_vels;               /* [N,T,6]  ar_context['head_vels'] */
    const float* obj_head_relative_poses; /* [N,T,7]  */
    const float* action_one_hot;          /* [N,4]    ar_context['action_one_hot'][0] */
    const float* gt_bquat;                /* [N,T,96] ar_context['bquat'] (GT clip) */
    const float* gt_wbpos;                /* [N,T,72] gt_targets['wbpos'] */
    const float* obj_qpos;                /* [N,7] or NULL */
    const int32_t* cur_t;                 /* [N] */
    const int32_t* row;                   /* [N] context row of every env, or NULL */
} kp_ctx;

/* records prev_bquat / prev_hpos at the top of HumanoidAREnv.step (humanoid_ar_v1.py:246-249) */
int kp_sim_step_begin(kp_sim*);

/* get_ar_obs_v1() [N,105]   (humanoid_ar_v1.py:133-214; use_head, use_action, use_obj on; use_vel/of/context off).  A handle created from a model
 * whose option "ar_obs_action" is 0 writes [N,101] instead: no action one-hot (use_action: false, :200-201); the one-hot still selects the object
 * of the "predicted object relative to head" block (:146-147, 466-476).  "ar_obs_vel" = 1 and "ar_obs_head" = 0 give the other layouts listed next
 * to KP_AR_OBS_DIM (use_vel / use_head: false); the velocity block is a copy of KP_QVEL.  kp_sim_ar_obs_dim: the handle's row width (-1 for NULL). */
int kp_sim_obs_ar(kp_sim*, const kp_ctx* ctx, float* out);
int kp_sim_ar_obs_dim(const kp_sim*);

/* termination (calc_body_diff / calc_body_gt_diff, :435-458, thresholds :53-54) and the reward
 * dynamic_supervision_v1 (kin_poly/core/reward_function.py:931-995) for the state after do_simulation,
 * with ctx->cur_t already incremented.  reward [N], info [N,6], fail uint8 [N], diffs [N,2]. */
typedef struct {
    float w_hp, w_hq, w_p, w_jp, w_act_p, w_act_v;
    float k_hp, k_hq, k_p, k_jp, k_act_p, k_act_v;
    float dt;                  /* env.dt = 1/30 */
    float body_diff_thresh;    /* 10  */
    float body_diff_gt_thresh; /* 12  */
    int use_gt_term;           /* mode == "train" and not wild (:303-306) */
} kp_reward_cfg;
int kp_sim_term_reward(kp_sim*, const kp_ctx* ctx, const kp_reward_cfg* cfg, float* reward, float* info, uint8_t* fail, float* diffs);

/* The tail of HumanoidAREnv.step in one launch (humanoid_ar_v1.py:288-316): cur_t += 1 (in place; cur_t must be ctx->cur_t), termination and
 * reward as kp_sim_term_reward with the incremented cur_t, then end = cur_t >= min(env_episode_len, ar_context['len']), done = fail || end,
 * percent = cur_t / ar_context['len'].  row_len: int32 [R] = ar_context['len'] of every context row (env e reads row_len[ctx->row[e]]).
 * done / end: uint8 [N]; percent: float [N]; done_count (optional, may be NULL): int32 device counter incremented by the number of done envs.
 * obj7 (optional, may be NULL): float [N,7] <- get_obj_qpos(ar_context['action_one_hot'][0]) of the state after the step (humanoid_ar_v1.py:171-172,
 * 466-477): the simulated pose of the action's first object, data.qpos[76 + action_index_map[a] : +7]; rows whose clip has no action are left
 * alone.  It is the buffer kp_ctx.obj_qpos points to, so the next kp_sim_obs_ar reads the objects where the physics left them.  obj7 needs
 * ctx->action_one_hot (refused with -1 otherwise); ctx->T < 2 is refused: the reward reads ground-truth frame t - 1 with t clamped into [1, T - 1]. */
int kp_sim_post_step(kp_sim*, const kp_ctx* ctx, const kp_reward_cfg* cfg, int32_t* cur_t, const int32_t* row_len, int env_episode_len,
                     float* reward, float* info, uint8_t* fail, float* diffs, uint8_t* done, uint8_t* end, float* percent, int32_t* done_count, float* obj7);

/* kp_sim_term_reward / kp_sim_post_step with dynamic_supervision_v2 (kin_poly/core/reward_function.py:999-1050), the "ground truth, no dynamics
 * regulation" reward: the head position and orientation terms of v1, then against ar_context frame cur_t (clamped into [1, T - 1] as for v1)
 *   pose  exp(-k_p |multi_quat_norm(bquat (x) gt_bquat^-1) * (1, b_diffw)|^2)        vel  exp(-k_v |get_angvel_fd(prev_bquat, bquat) - get_angvel_fd(gt_bquat[t - 1], gt_bquat[t])|^2)
 *   ee    exp(-k_e |wbpos - gt_wbpos|^2) over all 24 bodies
 * and reward = w_hp hp + w_hq hq + w_p pose + w_v vel + w_e ee (not normalised).  multi_quat_norm is kin_poly's (kin_poly/utils/math_utils.py:105-109:
 * acos(w), no absolute value, so a body quaternion of the opposite sign counts as a turn of 2 pi - angle) and get_angvel_fd's rotation_from_quaternion
 * kin_poly's too (kin_poly/utils/transformation.py:362-372: zero if |1 - w| < 1e-6 or |1 + w| < 1e-6).  info stays [N,6] so that records keep their shape: (hp, hq, pose,
 * vel, ee, 0).  Termination, end / done / percent and the obj7 write-back are v1's, bit for bit; every other argument and refusal is the v1 entry's,
 * plus a NULL b_diffw. */
typedef struct {
    float w_hp, w_hq, w_p, w_v, w_e;
    float k_hp, k_hq, k_p, k_v, k_e;
    float dt, body_diff_thresh, body_diff_gt_thresh;
    int use_gt_term;
    const float* b_diffw;      /* device [24]: root 1, then cc_cfg.b_diffw (the blob's uhc_b_diffw) */
} kp_reward_cfg_v2;
int kp_sim_term_reward_v2(kp_sim*, const kp_ctx* ctx, const kp_reward_cfg_v2* cfg, float* reward, float* info, uint8_t* fail, float* diffs);
int kp_sim_post_step_v2(kp_sim*, const kp_ctx* ctx, const kp_reward_cfg_v2* cfg, int32_t* cur_t, const int32_t* row_len, int env_episode_len,
                        float* reward, float* info, uint8_t* fail, float* diffs, uint8_t* done, uint8_t* end, float* percent, int32_t* done_count, float* obj7);

/* Masked reset in one gather + sim.forward() (mujoco_env.py:86-103, humanoid_ar_v1.py:334-387): for the envs with env_mask != 0 (NULL: all)
 * qpos / qvel <- init_qpos / init_qvel [R, 76] / [R, 75] of context row row[e] (NULL: row e), cur_t[e] = 0 (cur_t may be NULL), warm start
 * zeroed, derived quantities recomputed; set_target != 0: target = qpos_fk(init_qpos) for those envs as reset_model does (:384-386).
 * aux_rows (optional, may be NULL): caller-owned float [N, aux_cols] device rows zeroed for the same envs -- per-episode state that lives
 * outside the simulator, i.e. the kinematic policy's GRU hidden state (PolicyAR.reset / action_rnn.initialize at every episode start,
 * kin_poly/models/policy_ar.py:124-131).
 * row_obj_qpos (optional, may be NULL): float [R,35] = convert_obj_qpos(action_one_hot, obj_pose[0]) of every context row (humanoid_ar_v1.py:377,
 * 479-496); the masked envs' object block is set from their row exactly as kp_sim_set_objects sets it (velocities zero, :382) before sim.forward().
 * row_action_one_hot [R,4] + obj7 [N,7] (optional, both or neither): obj7 <- get_obj_qpos(action_one_hot) of the fresh block for those envs
 * ([0,0,0,1,0,0,0] for a clip without action, :465-466). */
int kp_sim_reset_rows(kp_sim*, const float* init_qpos, const float* init_qvel, const int32_t* row, const uint8_t* env_mask, int32_t* cur_t, int set_target,
                      float* aux_rows, int aux_cols, const float* row_obj_qpos, const float* row_action_one_hot, float* obj7);

/* Episode turnover of a sampler that keeps the NEXT clips of every env resident (the per-episode sample_seq -> init_context -> load_context of
 * sample_worker, kin_poly/core/agent_ar.py:518-535, made ahead of time and batched): the context table holds n_slots rows per env, row = slot * n + env;
 * for every env with done != 0: head <- (head + 1) mod n_slots, ahead <- ahead - 1 (clips still queued behind the current one), row <- head * n + env
 * (the int32 [n] buffer kp_ctx.row points to).  A pure function of its device arrays (no simulator handle); follow with kp_sim_reset_rows(done). */
int kp_pool_advance(int n, int n_slots, const uint8_t* done, int32_t* head, int32_t* ahead, int32_t* row, void* hip_stream);

/* The sampler's per-step record: Memory.push of sample_worker (kin_poly/core/agent_ar.py:582-597; TrajBatchEgo's twelve fields,
 * kin_poly/core/trajbatch_ego.py:5-14) for all n envs in one launch per half-step, into env-major [n, T, .] device buffers at time index t.
 * Every destination may be NULL (field not recorded); a destination needs its source.  bool-like arrays are uint8.
 *   pre  (before the env step): states <- obs [n,105]; episode_start <- fresh [n]; curr_qpos <- qpos [n,76] (get_humanoid_qpos, :571);
 *        gt_target_qpos <- ctx_qpos[row[e], min(cur_t[e] + 1, row_len[row[e]])] (ar_context['qpos'][cur_t + 1], :572; ctx_qpos is [R, ctx_T, 76]);
 *        meta [n,T,2] <- row_meta[row[e]] = (take_ind, fr_start) of the clip the env is on (:627-631).  row may be NULL (row = env).
 *   post (after the env step, before the episode turnover): actions, rewards, fails, dones, percents, c_infos [n,T,6] and, for the full record,
 *        next_states <- obs, res_qpos <- qpos, cc_actions [75], cc_states [784], v_metas [n,T,3] <- (meta[.., t, :], fr_num). */
typedef struct {
    int n, T, t, ctx_T;
    const float* obs; const uint8_t* fresh; const float* qpos; const float* ctx_qpos; const int32_t* row; const int32_t* cur_t; const int32_t* row_len; const float* row_meta;
    float* states; uint8_t* episode_start; float* curr_qpos; float* gt_target_qpos; float* meta;
} kp_record_pre;
typedef struct {
    int n, T, t; float fr_num;
    const float* action; const float* reward; const uint8_t* fail; const uint8_t* done; const float* percent; const float* c_info;
    const float* obs; const float* qpos; const float* cc_action; const float* cc_state; const float* meta;     /* meta: the [n,T,2] buffer `pre` wrote */
    float* actions; float* rewards; uint8_t* fails; uint8_t* dones; float* percents; float* c_infos;
    float* next_states; float* res_qpos; float* cc_actions; float* cc_states; float* v_metas;
} kp_record_post;
int kp_rollout_record_pre(const kp_record_pre*, void* hip_stream);
int kp_rollout_record_post(const kp_record_post*, void* hip_stream);
/* the same with the observation width of obs / states / next_states: KP_AR_OBS_DIM (what the two above use), KP_AR_OBS_DIM_NO_ACTION or one of the six
 * other widths of the layout next to KP_AR_OBS_DIM (180, 176, 85, 81, 160, 156); any other width fails and nothing is launched */
int kp_rollout_record_pre_w(const kp_record_pre*, int obs_dim, void* hip_stream);
int kp_rollout_record_post_w(const kp_record_post*, int obs_dim, void* hip_stream);

/* estimate_advantages before normalisation (uhc/khrylib/rl/core/common.py:5-20) on an env-major
 * [N,T] layout (each env's T rows contiguous, time increasing).  All pointers device, float32. */
int kp_gae(int n_envs, int T, const float* rewards, const float* masks, const float* values, float gamma, float tau,
           float* advantages, float* returns, void* hip_stream);
/* same with a bootstrap: last_values [N] = V(state after env e's last row), used where that row's mask is 1 (an episode the fixed
 * horizon of the lock-step sampler cut; the reference's workers always finish their episodes, so its recursion starts from 0).
 * last_values may be NULL (= kp_gae). */
int kp_gae_bootstrap(int n_envs, int T, const float* rewards, const float* masks, const float* values, const float* last_values,
                     float gamma, float tau, float* advantages, float* returns, void* hip_stream);

/* PolicyMCP.forward / select_action after the primitives' and the composer's GEMMs (uhc/core/policy_mcp.py:30-38, uhc/khrylib/rl/core/policy.py:12-15):
 * out [n, A] = sum_k softmax(logits [n, K])_k * prim [K, n, A]  (+ stdv [A] * noise [n, A], rows noise_stride floats apart, when noise != NULL).
 * All device float32; logits are the composer MLP's output BEFORE its softmax.  noise_stride < A (rows of the noise window overlapping, the last one read
 * past the buffer) and K > 64 are refused (-1). */
int kp_mcp_compose(int n, int K, int A, const float* logits, const float* prim, const float* noise, int noise_stride, const float* stdv, float* out, void* hip_stream);

/* One frame of the kinematic roll-out behind PolicyAR.init_context (TrajARNet.step, kin_poly/models/traj_ar_smpl_net.py:292-330): next_qpos [n,76] =
 * step_ar(qpos, kin_action [n,80]) with the root quaternion normalised, qvel_fd [n,75] = get_qvel_fd_batch(qpos, next_qpos, dt)
 * (kin_poly/utils/torch_utils.py:315-331).  A pure function of its device rows (no simulator handle). */
int kp_kin_advance(int n, const float* qpos, const float* kin_action, float dt, float* next_qpos, float* qvel_fd, void* hip_stream);

/* PolicyMCP's last layer AND its mixing stage in one fp32 MFMA kernel (same reference lines): with h2 [K, n, J] the raw output of the second
 * batched GEMM (no bias, no activation), b2 [K, J], w3 [K, J, ldw >= A] (= nets[k][1].weight^T stacked, rows ldw floats apart; with ldw >= 80,
 * ldw % 4 == 0 and a 16-byte aligned base the kernel reads it with 16-byte loads: pad the rows to 80), b3 [K, A]:
 *   out [n, A] = sum_k softmax(logits [n, K])_k * (b3[k] + relu(h2[k] + b2[k]) w3[k])   (+ stdv [A] * noise [n, A] as above)
 * K <= 16, J a multiple of 64, A <= 80.  All device float32, contiguous except noise (row stride noise_stride). */
int kp_mcp_tail(int n, int K, int J, int A, const float* h2, const float* b2, const float* w3, int ldw, const float* b3, const float* logits, const float* noise,
                int noise_stride, const float* stdv, float* out, void* hip_stream);

/* One roll-out step of torch.nn.GRUCell after its two gate GEMMs (TrajARNet.get_action, kin_poly/models/traj_ar_smpl_net.py:333-343;
 * RNN.forward in step mode, uhc/khrylib/models/rnn.py:24-36): gi [n, 3H] = x W_ih^T and gh [n, 3H] = h_in W_hh^T WITHOUT biases, b_ih / b_hh [3H]
 * -> h_out [n, H] (may alias h_in); xcat (optional) [n, D + H] <- [state | h_out], the row `torch.cat((state, hx), dim=1)` builds for
 * the action MLP (state [n, D]; a state wider than the hidden state, D > H -- 357 against 256 under kin_only.yml -- takes the kernel of
 * kp_obs_ctx.hip whose copy loops over the columns: the same gate math, the same h_out). */
int kp_gru_cell_step(int n, int H, int D, const float* gi, const float* gh, const float* b_ih, const float* b_hh, const float* h_in, const float* state,
                     float* h_out, float* xcat, void* hip_stream);

/* GRU re-unroll of the PPO / supervised updates (policy_ar.py:104-122, 216-240), one time step of torch.nn.GRUCell
 * semantics over n rows, all arrays contiguous float32 device pointers:
 *   forward : gi [n,3H] = x_t W_ih^T + b_ih, gh [n,3H] = hm_prev W_hh^T + b_hh (the caller's GEMMs), hm_prev [n,H] = previous hidden state
 *             already zeroed at episode starts -> h_out [n,H]; hm_next [n,H] (optional) = h_out * next_keep[row] (next_keep [n] = 1 - episode
 *             start flag of step t + 1, or NULL), the next step's GEMM input.
 *   backward: dh_out [n,H] (gradient reaching h_t from outside the recurrence, may be NULL), carry [n,H] * carry_keep [n] (gradient from
 *             step t + 1, may be NULL) -> dgi [n,3H], dgh [n,3H] (the caller forms carry' = dgh W_hh + dhz and dW_hh += dgh^T hm_prev), dhz [n,H]. */
int kp_gru_gates_forward(int n, int H, const float* gi, const float* gh, const float* hm_prev, const float* next_keep, float* h_out, float* hm_next,
                         void* hip_stream);
int kp_gru_gates_backward(int n, int H, const float* gi, const float* gh, const float* hm_prev, const float* dh_out, const float* carry,
                          const float* carry_keep, float* dgi, float* dgh, float* dhz, void* hip_stream);

/* restore a complete simulator state (what MjSimState + the derived arrays would hold): qpos/qvel and the
 * state (qpos_d/qvel_d) the stale derived quantities belong to; runs the forward pass on the latter. */
int kp_sim_set_full_state(kp_sim*, const float* qpos, const float* qvel, const float* qpos_d, const float* qvel_d, const uint8_t* env_mask);

/* object block of MjSimState save / restore: overwrite data.qpos[76:111] / data.qvel[75:105] of the simulated objects
 * (read them back with KP_OBJ_QPOS / KP_OBJ_QVEL).  Which objects are simulated stays as kp_sim_set_objects decided. */
int kp_sim_set_obj_state(kp_sim*, const float* obj_qpos, const float* obj_qvel, const uint8_t* env_mask);

/* An impulse push between two control steps; no reference counterpart (the reference never disturbs the character).  It is what a mujoco-py user
 * gets from `data.qvel[:75] += dv` between two env.step calls, with dv = M(qpos)^-1 J_b(r)^T [p; l] worked out on the device: momentum-exact, and
 * the same as kp_sim_set_full_state(qpos, qvel + dv, qpos_d, qvel_d) with the solver's warm start kept.  Per env:
 *   entity  int32 [N] device: 0..23 the humanoid's bodies, 24 + k simulated object slot k (the numbering of kp_sim_contacts); -1 and every other
 *           value = no push for this env (the values live on the device: the kernel checks them before it indexes with them);
 *   offset  [N,3] or NULL (= the origin): the point the impulse acts at, in the entity's own frame, metres from its frame origin;
 *   impulse [N,6]: p (linear, N s) and l (angular, N m s), world axes;
 *   dqvel   [N,75] or NULL: receives dv of the humanoid; zero rows for object pushes and for envs without a push.
 * Humanoid body b: r = xpos_b + R_b offset from kinematics computed anew at the CURRENT KP_QPOS (not the stale KP_QPOS_D of the read-outs),
 * M = the joint-space inertia there, armature included (mj_fullM), solved matrix-free; KP_QVEL += dv.  Object slot k (a no-op unless that slot is
 * simulated in the env): KP_OBJ_QVEL of the slot's object += M_obj^-1 g with the 6 x 6 free-joint inertia (armature included; 3 world translations
 * of the body origin, 3 rotations about the body axes); the humanoid is untouched.  Everything else in the handle stays bit for bit: qpos,
 * KP_QPOS_D / KP_QVEL_D and the derived arrays that belong to them, warm starts, targets, prev_*, the other entity's velocities, masked-out envs.
 * An impulse of exact zeros stores nothing; two pushes in a row add.  The jump is applied with no constraint active: contacts and joint limits answer
 * from the next substep on.  Works on every handle (floor / objects, any threads_per_env, lean or full launch form): it touches the stored rows only.
 * Enqueued on the handle's stream, no sync.  Refused (-1, kp_last_error) before anything is launched: null handle, null entity, null impulse. */
int kp_sim_apply_impulse(kp_sim*, const int32_t* entity, const float* offset, const float* impulse, const uint8_t* env_mask, float* dqvel);

/* Contact-force read-out of the STORED state.  Replaces what a mujoco-py user reads after `sim.forward()`: mj_contactForce / data.efc_force,
 * data.cfrc_ext, data.qfrc_constraint, data.qacc and data.qfrc_actuator.  The reference reads none of them (deviation 38).
 * The kernel runs the mj_forward of substep 0 of the control step kp_sim_step_ctrl would run next -- forward kinematics, collision, constraint rows,
 * the Newton solve from the stored warm start -- and stops before the integration.  It stores into the output rows alone: every row of the handle
 * (state, derived state, warm starts, diag) stays bit for bit, and a call between two control steps does not change them.
 *   actuation  0 none (qfrc_applied = ctrl = 0);
 *              1 torque: act [N,75] = qfrc_applied[0:6] ++ ctrl[69], used as given (no clipping);
 *              2 controller: act [N, cc_action_dim] is a cc_action row; the torque is the one the control step's FIRST substep forms from it (stable
 *                PD + residual force, on the kinematics of the derived state with stale_kinematics = 1, of the stored state otherwise; the
 *                extended controller of a handle that has one, at i_iter = 0).  Zero where the model option actuation is 0.
 *   act        device; required for actuation 1 and 2, ignored for 0.
 *   env_mask   [N] or NULL: a masked-out env gets zero rows and ncon = 0.
 *   out        device arrays, each may be NULL but not all:
 *     ncon            int32 [N]        contacts of the collision pass
 *     contact         float [N,64,12]  A, B, dist, pos[3], normal[3], force[3].  A = entity carrying the vertex (0..23 body, 24 + k object slot, the
 *                                      numbering of kp_sim_contacts), B = entity carrying the surface (-1 world: floor or static geom; 24 + k), normal
 *                                      pointing into A, force acting on A (N, world axes).  Rows >= ncon are zero.
 *     wrench          float [N,26,6]   per entity the net contact force[3] and torque[3] ABOUT THE WORLD ORIGIN (world axes): + f on A, - f on an
 *                                      object-slot B; floor and static geoms receive nothing.  Differs from data.cfrc_ext in the reference point only
 *                                      (cfrc_ext: the subtree COM); kinpoly_amd.contact.shift_wrench moves it.
 *     qfrc_constraint float [N,75]     J^T f of the contact rows + the joint-limit row forces
 *     qacc            float [N,75]     the solve's minimiser
 *     torque          float [N,75]     qfrc_applied[0:6] ++ ctrl[69] as the solve used them (mode 2: after the torque clip)
 *     obj_qacc        float [N,2,6]    accelerations of the simulated object slots in their free-joint coordinates; zero without simulated objects
 * Runs on the object layout exactly when the control step does (kp_sim_set_objects has installed a block).  Enqueued on the handle's stream, no sync.
 * Refused (-1, kp_last_error names the argument) before anything is launched: null handle, null out, all outputs null, actuation outside 0..2,
 * act NULL with actuation 1 or 2, a handle whose threads_per_env is not 64. */
typedef struct { int32_t* ncon; float *contact, *wrench, *qfrc_constraint, *qacc, *torque, *obj_qacc; } kp_contact_out;
int kp_sim_contact_forces(kp_sim*, int actuation, const float* act, const uint8_t* env_mask, const kp_contact_out* out);

/* Inverse dynamics on motion ROWS.  Replaces what a mujoco-py user reads after `mj_inverse`: data.qfrc_inverse, the generalized force the model
 * needs to perform a given motion (qpos, qvel, qacc).  The reference never calls it (deviation 39).  In the soft-constraint model
 * the inverse is closed form, no solve: jar = J qacc - aref, row forces -D jar where jar < 0, qfrc_inverse = M qacc + qfrc_bias - J^T f.  Its first
 * six entries are the residual wrench no contact and no joint supplies (force on the root in world axes, torque about the root position in the
 * root's own axes: kinpoly_amd.dynamics.root_residual); the other 69 are the joint torques a controller would have to deliver.
 * A rows API like kp_sim_fk: n_rows is independent of the handle's envs; the kernel reads the model tables (options contact / limits honoured) and
 * the row inputs, none of the handle's stored state and no warm start, and stores into the output rows alone.  Kinematics are always those of the
 * given pose.  One launch for all rows (one wavefront per row).
 *   qpos      [R,76] device, required.
 *   qvel      [R,75] or NULL: zero velocities.
 *   qacc      [R,75] or NULL: zero accelerations (gravity compensation: the static torque of a pose).
 *   obj_qpos  [R,35] or NULL: the five objects' free-joint poses; those within 50 m of the origin are STATIC obstacles at that pose (zero velocity,
 *             zero acceleration: what dynamic_objects = 0 means in the control step), the humanoid's hulls collide with their boxes and cylinders.
 *             NULL, or a row with every object parked, is the floor scene (bit for bit the same result).
 *   out       device arrays, each may be NULL but not all:
 *     qfrc_inverse    float [R,75]     in the coordinates of qfrc_applied[0:6] ++ ctrl[69] (kp_sim_contact_forces' torque)
 *     qfrc_constraint float [R,75]     J^T f of the contact rows + the joint-limit row forces, at the GIVEN qacc
 *     qfrc_bias       float [R,75]     C(q, qvel) + g of the forward pass (kp_sim_mass_matrix' bias)
 *     contact         float [R,64,12]  the rows of kp_sim_contact_forces; B = -1 for the floor and for a static geom
 *     net_wrench      float [R,6]      sum of the contact forces on the humanoid and their torque ABOUT THE WORLD ORIGIN (world axes)
 *     ncon            int32 [R]        contacts of the collision pass
 * Enqueued on the handle's stream, no sync (the first call with obj_qpos, and one with more rows than any before, grows a scratch buffer and waits
 * for the stream once).  n_rows == 0 does nothing.  Refused (-1, kp_last_error names the argument) before anything is launched: null handle, null
 * qpos, null out, all outputs null, n_rows < 0, a handle whose threads_per_env is not 64, obj_qpos on a blob without object geoms. */
typedef struct { float *qfrc_inverse, *qfrc_constraint, *qfrc_bias, *contact, *net_wrench; int32_t* ncon; } kp_invdyn_out;
int kp_sim_inverse_dynamics(kp_sim*, int n_rows, const float* qpos, const float* qvel, const float* qacc, const float* obj_qpos, const kp_invdyn_out* out);

/* Body velocities and accelerations, momentum and energy on motion ROWS.  Replaces what a mujoco-py user reads from data.body_xvelr / body_xvelp,
 * mj_objectAcceleration, the root's data.subtree_com / subtree_linvel / subtree_angmom and mj_energyPos / mj_energyVel (data.energy).  The reference
 * never reads them (deviation 40).  The forward pass of the control step (kinematics, spatial velocities, velocity-product
 * accelerations, inertias, bias wrenches) on the given rows and a read-out of what it leaves behind: no collision pass, no constraint, no solve; a
 * smooth function of its inputs.  A rows API like kp_sim_fk: n_rows is independent of the handle's envs; the kernel reads the model tables (masses,
 * inertias, armature, gravity) and the row inputs, none of the handle's stored state, and stores into the output rows alone.  The root quaternion is
 * normalised first, as everywhere.  One launch for all rows (one wavefront per row); a row's result does not depend on the other rows.
 *   qpos      [R,76] device, required.
 *   qvel      [R,75] or NULL: zero velocities.
 *   qacc      [R,75] or NULL: zero accelerations.
 *   out       device arrays, each may be NULL but not all; world axes throughout:
 *     body_vel     float [R,24,6]  angular velocity[3] (body_xvelr), linear velocity[3] of the body frame origin xpos (body_xvelp)
 *     body_acc     float [R,24,6]  angular acceleration[3], classical (coordinate) linear acceleration[3] of the body frame origin: the second time
 *                                  derivative of xpos, gravity not included (mj_objectAcceleration reports it with +(-g); subtract g to compare)
 *     body_com_vel float [R,24,3]  linear velocity of each body's centre of mass xipos
 *     centroid     float [R,18]    com[3], com_vel[3], L_com[3] (angular momentum about the centre of mass), ke (1/2 qvel^T M qvel, armature
 *                                  included: mj_energyVel), pe (-m g . com: mj_energyPos), com_acc[3], Ldot_com[3] (rate of L_com), mass.
 *                                  With qacc = NULL, com_acc and Ldot_com are the acceleration-free part (what the velocity products give at qacc = 0).
 * Enqueued on the handle's stream, does not synchronise.  n_rows == 0 does nothing.  Refused (-1, kp_last_error names the argument) before anything is
 * launched: null handle, n_rows < 0, null qpos, null out, all outputs null, a handle whose threads_per_env is not 64. */
typedef struct { float *body_vel, *body_acc, *body_com_vel, *centroid; } kp_motion_out;
int kp_sim_body_motion(kp_sim*, int n_rows, const float* qpos, const float* qvel, const float* qacc, const kp_motion_out* out);

/* Point Jacobians on motion ROWS.  Stands in for mj_jac (mj_jacBody with offset NULL): per row the Jacobian of one point of one body.  The reference
 * never calls it (deviation 41).  The forward pass' motion axes read out, no solve.  A rows API like kp_sim_body_motion: any n_rows,
 * the kernel reads the model tables and the row inputs, none of the handle's stored state, and stores into J alone.
 *   qpos    [R,76] device, required (root quaternion normalised first).
 *   body    int32 [R] device, required: 0..23; any other value gives a zero row.
 *   offset  [R,3] or NULL: the point in the body's frame (NULL: the body origin xpos).
 *   J       float [R,6,75]: rows 0..2 the world velocity of the point r = xpos_b + R_b offset, rows 3..5 the body's world angular velocity, per unit
 *           dof velocity.  Columns in qvel order: root translation (world axes), root rotation (about the root's own axes), the 69 hinges.
 * Enqueued on the handle's stream, does not synchronise.  n_rows == 0 does nothing.  Refused (-1, kp_last_error names the argument) before anything is
 * launched: null handle, n_rows < 0, null qpos / body / J, a handle whose threads_per_env is not 64. */
int kp_sim_point_jacobian(kp_sim*, int n_rows, const float* qpos, const int32_t* body, const float* offset, float* J);

/* Pose fitting on ROWS: from body poses to qpos.  No reference counterpart (the reference converts SMPL axis-angles offline, uhc/data_process); it
 * is the IK loop a mujoco-py user would write on mj_jacBody (deviation 41).  Per row, n_iters Levenberg-Marquardt iterations on
 *     c(q) = 1/2 sum_b w_pos_b |x*_b - x_b|^2 + 1/2 sum_b w_rot_b |log(R*_b R_b^T)|^2 + 1/2 sum_d w_prior_d (q*_d - q_d)^2
 * over the 24 body origins.  One iteration: residuals e at q; g = J^T W e (+ the prior's share); dq = (J^T W J + diag(mu damp + w_prior))^-1 g by the
 * control step's matrix-free articulated-body pass (the normal matrix is the joint-space inertia of the tree with point masses w_pos and spherical
 * inertias w_rot); trial q' = q (+) dq as mj_integratePos with dt = 1 (hinges clamped to jnt_range with clamp_limits); accepted
 * iff c(q') is finite and < c(q): mu <- max(mu mu_down, mu_min), else q stays and mu <- min(mu mu_up, mu_max).
 *   in   qpos0 [R,76] and tgt_pos [R,24,3] required; tgt_quat [R,24,4] or NULL (no orientation term; normalised, either sign); w_pos [R,24] or NULL
 *        (ones); w_rot [R,24] or NULL (zeros); q_prior / w_prior [R,69], both or neither.  Weights below zero count as zero.
 *   cfg  kp_fit_cfg_default: n_iters 30, mu0 1e-2, mu_min 1e-7, mu_max 1e6, mu_up 8, mu_down 0.3, damp 1 on every dof, clamp_limits 0.
 *   out  qpos [R,76] (root quaternion normalised) and info [R,8] required: first cost, final cost, accepted steps, final mu, max |e_pos| (m) and
 *        max |e_rot| (rad) over the bodies with a positive weight, |dq|_inf of the last solve, status (0 ok; 1: a non-finite input or first cost, the
 *        row ran no iteration and qpos is the input as given).  dq [R,75] or NULL: the last solve's step.
 * n_iters == 0 returns the input with its quaternion normalised and both costs filled.  A row's result depends on that row alone.  Enqueued on the
 * handle's stream, does not synchronise; nothing the handle stores is read or written.  n_rows == 0 does nothing.  Refused (-1, kp_last_error names
 * the argument) before anything is launched: null handle / in / cfg / out, n_rows < 0, a null required array, a prior without its weights or the
 * reverse, n_iters < 0, any of mu0, mu_min, mu_max, mu_up, mu_down, damp[d] not > 0 (NaN included), a handle whose threads_per_env is not 64. */
typedef struct { const float *qpos0, *tgt_pos, *tgt_quat, *w_pos, *w_rot, *q_prior, *w_prior; } kp_fit_in;
typedef struct { int n_iters; float mu0, mu_min, mu_max, mu_up, mu_down; float damp[75]; int clamp_limits; } kp_fit_cfg;
typedef struct { float *qpos, *info, *dq; } kp_fit_out;
void kp_fit_cfg_default(kp_fit_cfg* cfg);
int kp_sim_fit_pose(kp_sim*, int n_rows, const kp_fit_in* in, const kp_fit_cfg* cfg, const kp_fit_out* out);

/* Pose fitting on ROWS to POINTS AT BODY OFFSETS, with a floor that holds: mocap markers on the surface, 3D key points (nose, ears, toes, heels,
 * finger tips), end-effector targets; occluded points; hull vertices kept out of the ground.  No reference counterpart (deviation 43;
 * DESIGN.md section 20).  Per row, n_iters Levenberg-Marquardt iterations on
 *     c(q) = c_fit(q)                                              kp_sim_fit_pose's three terms (tgt_pos is optional here)
 *          + 1/2 sum_k w_k |t_k - (x_b(k) + R_b(k) o_k)|^2          points: body b(k), offset o_k in the body frame, world target t_k
 *          + 1/2 w_floor sum_v min(0, z_v - floor_z)^2             every hull vertex v of every body (the model blob's verts / vert_adr)
 * The iteration, q (+) dq, clamp_limits, the accept rule (cost finite and strictly smaller) and the mu schedule are kp_sim_fit_pose's.  The GRADIENT is
 * exact: J_p^T w e per point, with e = (0, 0, floor_z - z_v) on the vertices with z_v < floor_z.  The MATRIX is J^T W J + diag(mu damp + w_prior) with
 * every point and every vertex below the floor counted as an ISOTROPIC point mass (w_k, w_floor) at its place: a weighted point rigidly attached to a
 * body is a point mass, so the matrix is still the joint-space inertia of the same tree and the articulated-body pass solves it.  For the points that
 * is Gauss-Newton itself; for the floor it is a majoriser of the point-to-plane term (w I >= w n n^T), not its Gauss-Newton block.  The accept test
 * runs on the true cost, so descent stays monotone.
 *   markers  the marker set, shared by all rows, on the HOST: n_points K (0 .. 1024), pt_body int32 [K] (0..23), pt_offset float [K,3] (finite).  The
 *            call checks it, orders the points by body (stable) and keeps the ordered table in a scratch buffer of the handle; a call with another
 *            marker set than the one before waits for the stream once.
 *   in       device rows: qpos0 [R,76] required; pt_tgt [R,K,3] required when K > 0; pt_w [R,K] or NULL (ones); tgt_pos [R,24,3] or NULL (no origin
 *            term); tgt_quat, w_pos, w_rot, q_prior, w_prior as in kp_fit_in: w_rot needs tgt_quat.  At least one of K > 0 and tgt_pos.
 *            A point with w <= 0 is skipped and its target is not read into anything: it may be NaN (an occluded marker).  A NaN weight, or a target
 *            that is not finite under a positive weight, gives the row status 1.
 *   cfg      kp_fit_points_cfg_default: kp_fit_cfg_default's values, w_floor 0 (>= 0 and finite; 0 switches the term off), floor_z 0 (finite).
 *   out      qpos [R,76] and info [R,12] required.  info 0..7 as kp_sim_fit_pose; 8: max |e_k| and 9: rms |e_k| over the points with a positive
 *            weight (m); 10: the deepest hull vertex below floor_z at the result (m, >= 0) and 11: the number of hull vertices below it, both
 *            computed whether or not w_floor > 0.  dq [R,75] or NULL.  pt_err [R,K] or NULL: the distance at the result in the caller's point
 *            order, 0 for skipped points.  A row with status 1 ran no iteration, returns its input and zeros in info 8..11 and pt_err.
 * A row's result depends on that row alone.  Enqueued on the handle's stream; nothing else the handle stores is read or written.  n_rows == 0 does
 * nothing.  Refused (-1, kp_last_error names the argument) before the first HIP call: what kp_sim_fit_pose refuses (tgt_pos may be null), null markers,
 * n_points outside 0 .. 1024, null pt_body / pt_offset with K > 0, a body outside 0..23, an offset that is not finite, null pt_tgt with K > 0, K == 0
 * without tgt_pos, w_floor < 0 or not finite, floor_z not finite. */
typedef struct { int n_points; const int32_t* pt_body; const float* pt_offset; } kp_marker_set;
typedef struct { const float *qpos0, *pt_tgt, *pt_w, *tgt_pos, *tgt_quat, *w_pos, *w_rot, *q_prior, *w_prior; } kp_fit_points_in;
typedef struct { kp_fit_cfg fit; float w_floor, floor_z; } kp_fit_points_cfg;
typedef struct { float *qpos, *info, *dq, *pt_err; } kp_fit_points_out;
void kp_fit_points_cfg_default(kp_fit_points_cfg* cfg);
int kp_sim_fit_points(kp_sim*, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const kp_fit_points_cfg* cfg, const kp_fit_points_out* out);

/* Pose fitting on ROWS that keeps the hulls out of the scene's STATIC OBJECTS: kp_sim_fit_points with one more term.  No reference counterpart
 * (deviation 44).  obj_qpos [R,35] are the rows' object poses; the objects within 50 m are static boxes and
 * z-axis cylinders, placed exactly as for kp_sim_inverse_dynamics (at most 8 geoms per row).  Per row
 *     c(q) = kp_sim_fit_points' cost + 1/2 w_obj sum over pairs (hull b, geom g) sum_{v in footprint of f*} max(0, d_f* - n_f* . x_v)^2
 * A pair is skipped when sdf_g(xpos_b) - body_rbound[b] > 0.  Candidate planes (n, d): a box's faces (+-a_i, n.c + h_i) in the order +x -x +y -y +z -z;
 * a cylinder's caps +-a_3 and, when the radial part of xpos_b - c is longer than 1e-6, the tangent plane n = u, d = u.c + rho, u the unit radial
 * direction towards the body origin.  D_f = max_v (d_f - n_f . x_v) over ALL vertices of the hull; some D_f <= 0: the pair has no term; otherwise f* is
 * the first plane of least D_f.  The footprint of f* is the primitive's extent in the directions other than n (box: |a_j.(x - c)| < h_j on the two
 * other axes; cap: radial distance < rho; tangent plane: |a_3.(x - c)| < h and |(a_3 x u).(x - c)| < rho).  Every footprint vertex behind the plane
 * counts, however deep, pulled to its own projection on the plane, re-projected at every evaluation; a vertex in two geoms' footprints counts in both.
 * GRADIENT: J_v^T w_obj (d - n.x_v) n with n held fixed: exact for faces and caps, without the turn of u with the body origin for the tangent plane.
 * MATRIX: every counted vertex is an isotropic point mass w_obj (a majoriser, as for the floor).  The accept test runs on the true cost.  The fit is
 * local: a hull far through a thin slab leaves through the nearer face of its deepest extent, which need not be the side it came from.
 *   markers, in   as kp_sim_fit_points.
 *   obj_qpos  device [R,35] or NULL: every row is the floor scene.  A row whose placed geom records are not finite (a NaN pose) gets status 1.
 *   cfg       kp_fit_scene_cfg_default: kp_fit_points_cfg_default's values, w_obj 0 (>= 0 and finite; 0 switches the term off).
 *   out       kp_fit_points_out with info [R,16]: 0..11 as kp_sim_fit_points; 12: the deepest counted vertex at the result (m); 13: the number of
 *             counted vertices; 14: the number of pairs with a term (no separating candidate plane); 15: 0.  12..14 are computed whether or not
 *             w_obj > 0.  A row with status 1 ran no iteration, returns its input and zeros in info 8..14 and pt_err.
 * With NULL obj_qpos, every object parked, w_obj == 0 or every pair separated, qpos, info 0..11, dq and pt_err are kp_sim_fit_points' bit for bit.
 * A row's result depends on that row alone.  Enqueued on the handle's stream; nothing else the handle stores is read or written.  Refused (-1)
 * before the first HIP call: what kp_sim_fit_points refuses, w_obj < 0 or not finite, obj_qpos on a blob without object geoms, a handle whose
 * threads_per_env is not 64. */
typedef struct { kp_fit_points_cfg pts; float w_obj; } kp_fit_scene_cfg;
typedef kp_fit_points_out kp_fit_scene_out;
void kp_fit_scene_cfg_default(kp_fit_scene_cfg* cfg);
int kp_sim_fit_scene(kp_sim*, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const float* obj_qpos, const kp_fit_scene_cfg* cfg, const kp_fit_scene_out* out);

/* Pose fitting on ROWS to 2D KEY POINTS seen by CALIBRATED CAMERAS: kp_sim_fit_scene with one more term.  No reference counterpart (INTEGRATION.md,
 * deviation 45).  Detections in video from one or several cameras need no triangulation first: a point seen by a single camera
 * counts, and the floor, object and prior terms resolve depth.  Per row
 *     c(q) = kp_sim_fit_scene's cost + 1/2 sum_c sum_k w_ck |uv_ck - pi_c(p_k)|^2,    p_k = x_b(k) + R_b(k) o_k  (the call's one marker set)
 * A camera record is 16 floats: R_cw (9, row-major), t (3), fx, fy, cx, cy; cam = R_cw p + t, the camera looks along +z,
 * pi = (cx + fx cam_x / cam_z, cy + fy cam_y / cam_z) in pixels.  GRADIENT: exact, J_p^T (w J_pi^T (uv - pi)), a force at the point.  MATRIX: the point
 * counts as an isotropic mass m = w lambda, lambda the largest eigenvalue of the 2 x 2 J_pi J_pi^T in closed form (fx == fy == f: (f / cam_z)^2 (1 + a^2
 * + b^2), a = cam_x / cam_z, b = cam_y / cam_z): m I >= w J_pi^T J_pi, a majoriser as for the floor and the objects, so the matrix is still a joint-space
 * inertia.  The accept test runs on the true cost.
 *   markers, in, obj_qpos   as kp_sim_fit_scene, but in->pt_tgt may be NULL with K > 0: no 3D term (pt_w is not read then, pt_err is zeros).  At least
 *             one of 3D targets (K > 0 and pt_tgt), tgt_pos and observations (K > 0 and n_cams > 0).
 *   obs       NULL or n_cams == 0: no image term.  n_cams C 0 .. 8; device arrays cam [camera_rows,C,16] with camera_rows 1 or R, uv [R,C,K,2] in
 *             the caller's point order, uv_w [R,C,K] or NULL (ones).  An observation with w <= 0 is skipped and its uv is not read into anything: it
 *             may be NaN (an undetected key point).  A NaN weight, a uv that is not finite under a positive weight or a camera record that is not
 *             finite gives the row status 1.
 *   cfg       kp_fit_image_cfg_default: kp_fit_scene_cfg_default's values, z_near 0.05 m (> 0 and finite).  BEHIND THE CAMERA: a weighted
 *             observation with cam_z < z_near at the start gives the row status 2: it runs no iteration and returns its input.  The same condition in
 *             a trial pose makes that trial's cost +inf, which the accept rule rejects: the fit never lowers its cost by hiding a point.
 *   out       qpos [R,76] and info [R,20] required.  info 0..15 as kp_sim_fit_scene (7: status 0, 1 or 2; both costs of a status 2 row are +inf);
 *             over the weighted observations at the result: 16 the max and 17 the rms reprojection error (pixels), 18 their number, 19 the smallest
 *             cam_z among them (m; 0 without any).  dq [R,75], pt_err [R,K], uv_err [R,C,K] or NULL: uv_err is the reprojection error in the caller's
 *             order, 0 for skipped observations.  A row with status 1 or 2 returns zeros in info 8..19, pt_err and uv_err.
 * With n_cams == 0, NULL obs or every uv_w <= 0, qpos, info 0..15, dq and pt_err are kp_sim_fit_scene's bit for bit.  A row's result depends on that
 * row alone.  Enqueued on the handle's stream; nothing else the handle stores is read or written.  n_rows == 0 does nothing.  Refused (-1) before the
 * first HIP call: what kp_sim_fit_scene refuses (pt_tgt may be null), n_cams outside 0 .. 8, camera_rows neither 1 nor R, null cam or uv with
 * n_cams > 0, z_near not > 0 or not finite, nothing to fit. */
typedef struct { kp_fit_scene_cfg scene; float z_near; } kp_fit_image_cfg;
typedef struct { int n_cams, camera_rows; const float *cam, *uv, *uv_w; } kp_fit_image_obs;
typedef struct { float *qpos, *info, *dq, *pt_err, *uv_err; } kp_fit_image_out;
void kp_fit_image_cfg_default(kp_fit_image_cfg* cfg);
int kp_sim_fit_image(kp_sim*, int n_rows, const kp_marker_set* markers, const kp_fit_points_in* in, const float* obj_qpos, const kp_fit_image_obs* obs,
                     const kp_fit_image_cfg* cfg, const kp_fit_image_out* out);

/* Contact forces ESTIMATED from kinematics on motion ROWS: the ground reaction a motion would need.  No reference counterpart and no mujoco-py one
 * (deviation 42); it is the support-force estimate of physics-based pose estimation and biomechanics.  kp_sim_inverse_dynamics charges
 * a row the forces of the soft-constraint model, a function of how many millimetres a hull penetrates; this call asks which forces inside the friction
 * pyramids of the points NEAR a surface explain the row's root residual best.  Per row:
 *   candidates  the contacts the control step's collision pass finds at the row's pose with its margin set to cfg->reach (everything else the model's):
 *               up to planemesh_max per hull on the floor, one per hull and box / cylinder, 64 slots in the stored order.  Candidate c has the point
 *               p_c, the unit normal n_c into the hull, the tangents t1_c, t2_c of the step's contact frame and the four pyramid edges
 *               d_ck = n_c + mu t1_c, n_c - mu t1_c, n_c + mu t2_c, n_c - mu t2_c (mu = cfg->mu if > 0, else the model's).
 *   demand      need = M qacc + qfrc_bias (+ armature) exactly as kp_sim_inverse_dynamics forms it; no joint-limit row is evaluated.
 *               r = [need[0:3]; R_root need[3:6]]: force and moment in world axes about the root position x_root.
 *   solve       lambda >= 0 in R^(4C) minimising 1/2 (r - G lambda)^T W (r - G lambda) + 1/2 rho |lambda|^2, g_ck = [d_ck; (p_c - x_root) x d_ck],
 *               W = diag(w_f I3, w_m I3).  Strictly convex: the minimiser is unique and does not depend on the method (a semismooth Newton iteration with an
 *               exact line search on the 6-vector e = r - G lambda, at most n_iters steps).
 * The score is a LOWER bound on the residual: every nearby point may push.  Objects are static obstacles as in kp_sim_inverse_dynamics.
 *   qpos, qvel, qacc, obj_qpos   as kp_sim_inverse_dynamics (NULL qvel / qacc: zeros; NULL obj_qpos or every object parked: the floor scene, bit for bit).
 *   cfg  kp_estimate_cfg_default(model, cfg), with m the model's total mass and g its gravity: reach 0.03 m, w_f = 1 / (m g)^2, w_m = 1 / (m g x 1 m)^2,
 *        rho = 1e-3 w_f, mu 0 (the model's), n_iters 20.  Conventions, not measurements.
 *   out  device arrays, each may be NULL but not all:
 *     qfrc_inverse float [R,75]     need - qfrc_contact; its first six entries are the residual in kp_sim_inverse_dynamics' root convention
 *     qfrc_contact float [R,75]     J^T f of the estimated forces
 *     contact      float [R,64,12]  the rows of kp_sim_contact_forces: A, B = -1, the candidate's distance, pos[3], normal[3], force f_c = sum_k lambda_ck d_ck
 *     lambda       float [R,64,4]   the multipliers (N) in the edge order above; zero rows past ncon
 *     resid        float [R,6]      e = r - G lambda: force, moment about the root position, world axes
 *     net_wrench   float [R,6]      sum of the estimated forces and their torque ABOUT THE WORLD ORIGIN (world axes)
 *     ncon         int32 [R]        candidates
 *     info         float [R,8]      cost at lambda = 0, final cost (both in the scaled units: 1/2 r^T W r), Newton iterations, active columns,
 *                                   |F(e)| at exit (scaled), iterations that needed a line search, 0, status
 *   status  0 ok; 1: a non-finite input, the row ran nothing and every output row is zero; bit 2: all 64 slots are taken, candidates may have been
 *           dropped; bit 4: n_iters ran out before the stopping rule held.
 * A row's result depends on that row alone.  Enqueued on the handle's stream, does not synchronise (the first call with obj_qpos, and one with more rows
 * than any before, grows the scratch buffer kp_sim_inverse_dynamics uses and waits for the stream once); nothing else the handle stores is read or
 * written.  n_rows == 0 does nothing.  Refused (-1, kp_last_error names the argument) before anything is launched: null handle / qpos / cfg / out, all
 * outputs null, n_rows < 0, reach not > 0, w_f, w_m or rho not > 0 or not finite (NaN included), mu < 0, n_iters < 0, a handle whose threads_per_env
 * is not 64, obj_qpos on a blob without object geoms. */
typedef struct { float reach, w_f, w_m, rho, mu; int n_iters; } kp_estimate_cfg;
typedef struct { float *qfrc_inverse, *qfrc_contact, *contact, *lambda, *resid, *net_wrench; int32_t* ncon; float* info; } kp_estimate_out;
void kp_estimate_cfg_default(const kp_model* model, kp_estimate_cfg* cfg);
int kp_sim_estimate_contacts(kp_sim*, int n_rows, const float* qpos, const float* qvel, const float* qacc, const float* obj_qpos, const kp_estimate_cfg* cfg, const kp_estimate_out* out);

/* read-outs of the mujoco-py data fields the env uses (humanoid_im.py:342-416, humanoid_ar_v1.py:460-512) */
typedef enum {
    KP_QPOS = 0,        /* data.qpos[:76]                    [N,76]  */
    KP_QVEL = 1,        /* data.qvel[:75]                    [N,75]  */
    KP_XPOS = 2,        /* data.body_xpos[1:25]              [N,72]  (stale by one substep, like mujoco-py) */
    KP_XQUAT = 3,       /* data.body_xquat[1:25]             [N,96]  */
    KP_XIPOS = 4,       /* data.xipos[1:25]                  [N,72]  */
    KP_BQUAT = 5,       /* get_body_quat()                   [N,96]  (humanoid_im.py:342-354, from fresh qpos) */
    KP_HEAD = 6,        /* get_head()                        [N,7]   */
    KP_TARGET_QPOS = 7, /* target['qpos']                    [N,76]  */
    KP_TARGET_WBPOS = 8,   /* target['wbpos']                [N,72]  */
    KP_TARGET_WBQUAT = 9,  /* target['wbquat']               [N,96]  */
    KP_TARGET_BQUAT = 10,  /* target['bquat']                [N,96]  */
    KP_TARGET_COM = 11,    /* target['body_com']             [N,72]  */
    KP_QPOS_D = 12,     /* state the derived quantities were computed at (x_14 after a control step) */
    KP_QVEL_D = 13,
    KP_PREV_BQUAT = 14, /* env.prev_bquat                    [N,96] */
    KP_PREV_HPOS = 15,  /* env.prev_hpos                     [N,7]  */
    KP_OBJ_QPOS = 16,   /* get_obj_qpos() = data.qpos[76:111] [N,35]  (simulated poses of the active objects) */
    KP_OBJ_QVEL = 17,   /* get_obj_qvel() = data.qvel[75:105] [N,30] */
    KP_M = 18,          /* mj_fullM(model, M, data.qM)[:75,:75]   [N,75*75] row-major, armature included (humanoid_im.py:422-425);
                           of the state the derived quantities belong to (KP_QPOS_D), like mujoco-py's data.qM between steps */
    KP_BIAS = 19        /* data.qfrc_bias[:75]               [N,75]  (humanoid_im.py:426), same state */
} kp_field;
int kp_field_dim(int field);
int kp_sim_get(kp_sim*, int field, float* out);
/* Device address of a STORED per-env field ([N, kp_field_dim(field)] float32 rows: KP_QPOS, KP_QVEL, KP_XPOS, KP_XQUAT, KP_XIPOS, KP_TARGET_QPOS,
 * KP_QPOS_D, KP_QVEL_D, KP_OBJ_QPOS, KP_OBJ_QVEL), NULL for derived read-outs.  The zero-copy counterpart of kp_sim_get (`data.qpos` as a view,
 * humanoid_im.py:193): valid for the life of the handle, contents ordered by the handle's stream, overwritten by the next step. */
const float* kp_sim_field_device(kp_sim*, int field);

/* per-env diagnostics of the last kp_sim_step_ctrl: int32 [N,4] = {contacts in last substep,
 * Newton iterations (sum over substeps), flags (bit 0 = non-finite state) | number of substeps whose Newton solve stopped at the
 * iteration cap ("solver_iter", default mjOption.iterations = 100) instead of a termination test << 8,
 * max contacts | Hessian factorisations << 8}.  HOST pointer;
 * synchronises the stream.  Fails if the job queue of the last launch stalled (never observed; see kp_step_queue_kernel). */
int kp_sim_diag(kp_sim*, int32_t* out_host);

/* shader-clock cycles >> 10 every env took inside the last kp_sim_step_ctrl launch, uint32 [N], HOST pointer; synchronises.
 * With model option "lpt_order" on (default: when free objects are simulated) the next launch starts the envs longest-first from these
 * (launch / queue order only: results do not depend on it). */
int kp_sim_launch_cost(kp_sim*, uint32_t* out_host);

/* Floor scenes' job queue: which LDS layout the control-step launches run on.  out3[0] = 1 when the next control step, with the substep count of the last one
 * (15 before any), would launch the job queue on the lean layout (12 envs per CU, 24 contact slots; model option "lean_queue"): 0 with one workgroup per env
 * (no more envs than slots), in fresh mode ("stale_kinematics" = 0) and during a fallback; out3[1] = how many times so far the handle has fallen back to the
 * full layout for 64 launches because more than 1 / 64 of the envs needed more contact slots than the lean layout has (their jobs are re-run by a second
 * kernel: cheaper to run everything on the full layout then; model option "lean_adaptive" = 0 keeps the lean layout regardless), out3[2] = control-step
 * launches so far.  Host arithmetic only; no reference counterpart (launch policy: results do not depend on the layout). */
int kp_sim_lean_state(kp_sim*, int32_t* out3);

/* the job sizes kp_sim_step_ctrl uses for a control step of n_substeps when it schedules through the job queue (host arithmetic, no
 * device): sizes16[0 .. return value) sum to n_substeps, the last is substeps_per_job (or absorbs a smaller remainder), every earlier
 * one is `taper` substeps longer than the one after it (the first takes what is left).  Returns the number of jobs (<= 16) or a negative error. */
int kp_job_schedule(int n_substeps, int substeps_per_job, int taper, int* sizes16);

/* seconds the last kp_sim_step_ctrl launch took, measured with HIP events on the sim's stream
 * (synchronises); -1 if none recorded. */
double kp_sim_last_step_seconds(kp_sim*);

/* Launch-duration statistics of kp_sim_step_ctrl: every launch after kp_sim_timing_reset() is bracketed
 * by a HIP event pair on the sim's stream (up to 4096 launches, no host sync while recording).
 * kp_sim_timing_mean_seconds() synchronises once and returns the mean duration (count in *n_launches). */
int kp_sim_timing_reset(kp_sim*);
double kp_sim_timing_mean_seconds(kp_sim*, int* n_launches);

/* Diagnostic: mean shader-clock cycles per environment the last kp_sim_step_ctrl spent in each phase
 * {stable-PD, kinematics+bias, collision, constraint set-up, smooth solve, contact solve, integrate, total}.
 * Collected only if the environment variable KP_PROFILE=1 was set at kp_sim_create.  The profiler is compiled into the one-workgroup-per-env
 * step kernels only: such a handle runs every control step in that launch form (never the job queue) and says so once on stderr.  Synchronises. */
int kp_sim_phase_cycles(kp_sim*, double* out8_host);
/* the same per environment: out_host [N, 8] (the tail of a launch is a few environments, not the mean). */
int kp_sim_phase_cycles_env(kp_sim*, double* out_host);

/* ---- the UHC's take library and fused tracking step (kinpoly_amd/csrc/kp_takes.hip) ----
 *
 * kp_takes: the expert tables of K takes of different lengths, concatenated row-wise (R rows in all; take k owns rows
 * take_off[k] .. take_off[k + 1] - 1), resident on the device of the handle that built them and independent of its number of envs.  It is
 * what get_expert (uhc/utils/tools.py:20-85) produces per take and DatasetAMASSSingle keeps per take (uhc/data_loaders/dataset_amass_single.py:
 * 24-241): per row qpos [76] (as given), qpos_fk [76] (root quaternion normalised: the row kp_sim_set_target stores), wbpos [72], wbquat [96],
 * bquat [96] (root = the raw root quaternion, get_body_quat), body_com [72], com [3], head_pose [7], ee_wpos [15], ee_pos [15], rq_rmh [4],
 * qvel [75] (get_qvel_fd_new of rows i - 1, i over dt, clamped to +-10; the first row of every take repeats its second row's, tools.py:57-66),
 * rlinv [3], rangv [3], rlinv_local [3], bangvel [72]; per take height_lb [1], head_height_lb [1].  A finite difference never crosses a take
 * boundary.  Forward kinematics is kp_sim_fk's kernel; the rest is one kernel, one wavefront per row, plus one wavefront per take for the minima.
 *
 * kp_takes_create: qpos_rows [R,76] on the host (rows_on_device = 0) or on the handle's device; take_off_host: K + 1 increasing offsets on
 * the host, take_off_host[0] == 0, take_off_host[K] == R, every take at least 2 rows, K >= 1; dt = env.dt (1 / 30; a finite difference is multiplied by (float)(1 / dt)).  Returns NULL and sets
 * kp_last_error on a bad argument (nothing is launched).  The library keeps no reference to qpos_rows.  Synchronises the handle's stream once.
 *
 * kp_takes_create_obj: the same with obj_rows [R,35], the object block data.qpos[76:111] of every row as DatasetSMPLObj.convert_obj_qpos builds it
 * (uhc/data_loaders/dataset_smpl_obj.py:230-243: five objects, the inactive ones parked 100+ m away), on the same side as qpos_rows (one
 * rows_on_device for both).  The library keeps a copy as the table "obj_pose" [R,35], beside the tables above, and kp_sim_uhc_assign places the
 * objects from it.  obj_rows == NULL is kp_takes_create.  Refused, besides kp_takes_create's errors, before anything is launched: a model blob
 * without object geoms (or with more than 64), obj_rows in host memory with rows_on_device = 1 or in device memory with rows_on_device = 0.
 * What is still refused elsewhere: the UHC observation and reward read nothing of the objects (the reference's have no such term). */
typedef struct kp_takes kp_takes;
kp_takes* kp_takes_create(kp_sim*, const float* qpos_rows, int rows_on_device, const int32_t* take_off_host, int n_takes, double dt);
kp_takes* kp_takes_create_obj(kp_sim*, const float* qpos_rows, const float* obj_rows, int rows_on_device, const int32_t* take_off_host, int n_takes, double dt);
void kp_takes_destroy(kp_takes*);
/* 1: the library was built with obj_rows (it answers "obj_pose"); 0: without, or a NULL library */
int kp_takes_has_objects(const kp_takes*);
/* device pointer, row count (R, or K for the per-take tables) and width of a table by its name above, or "obj_pose" [R,35] of a library with
 * objects; -1 for an unknown name and for "obj_pose" on a library without objects */
int kp_takes_table(const kp_takes*, const char* name, const float** ptr, int* rows, int* width);
/* K, R and (lens_host != NULL) the K take lengths */
int kp_takes_info(const kp_takes*, int* n_takes, int* n_rows, int32_t* lens_host);

/* Per-env tracking state, owned by the caller (device): which take an env imitates, where in it the episode started, and env.cur_t.
 * base_qpos [N,76] receives compute_torque's base pose for the next control step (humanoid_im.py:441, 451-452, 678). */
typedef struct {
    int32_t* take_id;      /* [N] */
    int32_t* start_ind;    /* [N] env.start_ind */
    int32_t* cur_t;        /* [N] env.cur_t */
    float* base_qpos;      /* [N,76] */
} kp_uhc_state;

/* world_rfc_implicit_reward's weights (uhc/core/reward_function.py:4-53; uhc.yml:37-48) and HumanoidEnv.step's episode constants */
typedef struct {
    float w_p, w_v, w_e, w_c, w_vf, k_p, k_v, k_e, k_c, k_vf;
    double dt;                 /* env.dt; velocities are differences times (float)(1 / dt), as the torch path evaluates `x / dt` */
    float body_diff_thresh;    /* 0.5 (humanoid_im.py:557) */
    int term_body;             /* 1: env_term_body 'body' (fail = body_diff > thresh); 0: 'head' and the rest of the chain never fail (:554-561) */
    int env_episode_len, trail;/* end = cur_t >= env_episode_len || cur_t + start_ind >= len + env_expert_trail_steps (:564) */
    int obs_v;                 /* 0: the observation's target is expert frame t; 1 / 2: frame t + 1 (:132, 158, 245) */
    int vf_dim;                /* the w_vf term reads action[-vf_dim:]; 0: the whole action (reward_function.py:44-46) */
    int action_dim;
    const float* a_ref;        /* device [69] for action_v 0 (the base pose's joint angles, :451-452), else NULL */
    const float* b_diffw;      /* device [24]: the pose term's body weights (root 1, then cfg.b_diffw; the blob's uhc_b_diffw) */
} kp_uhc_cfg;

/* kp_sim_step_ctrl with compute_torque's base pose read from base_qpos [N,76] instead of the stored target (which then stays the observation's) */
int kp_sim_step_ctrl_base(kp_sim*, const float* cc_action, int n_substeps, const uint8_t* env_mask, const float* base_qpos);

/* The tail of HumanoidEnv.step after do_simulation (uhc/envs/humanoid_im.py:527-572) in one launch, one wavefront per env: cur_t += 1;
 * row = take_off[take_id] + min(start_ind + cur_t, len - 1) (get_expert_index, :648-650); calc_body_diff (mean form, :719-726) -> body_diff [N];
 * fail / end / done uint8 [N]; percent = cur_t / len (:570); world_rfc_implicit_reward -> reward [N], info [N,5] (pose, vel, ee, com, vf terms;
 * prev_bquat is the record kp_sim_step_begin took); then the stored target <- the expert row the next observation looks at and
 * st->base_qpos <- the next control step's base pose.  Errors (nothing launched): null argument, a library of another model or device. */
int kp_sim_uhc_track(kp_sim*, const kp_takes*, const kp_uhc_state* st, const kp_uhc_cfg* cfg, const float* cc_action,
                     float* reward, float* info, float* body_diff, uint8_t* fail, uint8_t* end, uint8_t* done, float* percent);

/* reset_model (humanoid_im.py:574-623) / fail_safe (:235-238) for the envs of env_mask (uint8 [N] device, NULL = all): take_ids_host /
 * start_host (host int32 [N], may be NULL: keep) are checked (0 <= take_id < K, 0 <= start < len; nothing is launched on an error) and
 * assigned; keep_t == 0 zeroes cur_t; then qpos <- the take's raw row at min(start_ind + cur_t, len - 1) (+ noise [N,69] on the joint angles,
 * device, may be NULL), qvel <- that row's qvel, sim.forward(), and target / base pose as kp_sim_uhc_track leaves them.  keep_t = 1 with
 * NULL ids is fail_safe().
 * A library with objects (kp_takes_create_obj): with keep_t == 0 the same launch installs the env's object block from the library row the humanoid
 * state comes from (reset_model's has_obj branch, :613-616) -- pose, zero velocities and warm start, and the slot list (dynamic_objects) or the
 * frozen world-frame geoms, exactly what kp_sim_set_objects installs from that row -- and the handle runs the object layout from then on, as after
 * kp_sim_set_objects.  keep_t == 1 leaves the object block alone (fail_safe overwrites qpos[:76] / qvel[:75] only, :235-238); envs outside the mask
 * are untouched.  Needs threads_per_env = 64 (-1, nothing launched).  A library without objects never touches the object block. */
int kp_sim_uhc_assign(kp_sim*, const kp_takes*, const kp_uhc_state* st, const kp_uhc_cfg* cfg, const uint8_t* env_mask,
                      const int32_t* take_ids_host, const int32_t* start_host, int keep_t, const float* noise);

/* ---- the UHC's other tracking rewards (uhc/core/reward_function.py:453-460, the registry) ----
 *
 * kp_sim_uhc_track computes world_rfc_implicit_reward; kp_sim_uhc_track_r is the same launch with the reward function chosen by reward_id:
 *   KP_UHC_WORLD_RFC_IMPLICIT         :4-53     what kp_sim_uhc_track computes, by the same kernel: every output is bit-identical; info [N,5]
 *   KP_UHC_WORLD_RFC_IMPLICIT_V1_MUL  :56-102   the five terms of the above multiplied, the vf term always on (w_* unused); info [N,5]
 *   KP_UHC_LOCAL_RFC_IMPLICIT         :172-231  pose and velocity without the root, end effectors in root coordinates against the table ee_pos, root
 *                                               pose (height, de-headed root quaternion against rq_rmh), root velocity (get_qvel_fd_new(prev_qpos, qpos,
 *                                               dt, 'root')[:6] against rlinv_local / rangv), vf if w_vf > 0; weighted sum over the sum of the weights;
 *                                               info [N,6] = pose, vel, ee, root pose, root vel, vf
 *   KP_UHC_WORLD_RFC_IMPLICIT_V2      :301-372  pose, world pose (xquat against wbquat), per-body COM (xipos against body_com), joint positions (xpos
 *                                               against wbpos), velocity, vf: every distance a MEAN of squares, the terms multiplied;
 *                                               info [N,6] = pose, wpose, com, jpos, vel, vf
 *   KP_UHC_WORLD_RFC_IMPLICIT_V3      :376-450  v2's terms in a weighted sum that is NOT normalised; info [N,6] as v2
 * The termination outputs, cur_t, the stored target and base_qpos do not depend on reward_id. */
enum { KP_UHC_WORLD_RFC_IMPLICIT = 0, KP_UHC_WORLD_RFC_IMPLICIT_V1_MUL = 1, KP_UHC_LOCAL_RFC_IMPLICIT = 2, KP_UHC_WORLD_RFC_IMPLICIT_V2 = 3,
       KP_UHC_WORLD_RFC_IMPLICIT_V3 = 4, KP_UHC_REWARD_COUNT = 5 };

/* kp_uhc_cfg -- the weights the five functions share by name, and the episode constants -- plus the union of the others' `ws.get` keys.  A weight
 * a function does not read is ignored. */
typedef struct {
    kp_uhc_cfg base;           /* w_p w_v w_e w_c w_vf k_p k_v k_e k_c k_vf: each function's own keys of these names */
    int reward_id;             /* KP_UHC_* */
    float w_rp, w_rv;          /* local_rfc_implicit: root pose, root velocity (:176) */
    float k_rh, k_rq, k_rl, k_ra;      /* local_rfc_implicit: root height, root quaternion, root linear / angular velocity (:178) */
    float w_wp, w_j;           /* v3: world pose, joint positions (:380-381) */
    float k_wp, k_j;           /* v2 / v3 (:305-306, 383-384) */
    const float* jpos_diffw;   /* device [24]: reward_weights.jpos_diffw of v2 / v3 (:307; NOT the env's cfg.jpos_diffw); NULL for the other ids */
    const float* prev_qpos;    /* device [N,76]: env.prev_qpos, the qpos before the control step (humanoid_im.py:538), read by local_rfc_implicit;
                                  NULL for the other ids */
} kp_uhc_cfg_r;

/* the width of kp_sim_uhc_track_r's info row: 5 or 6; -1 for an unknown reward_id */
int kp_uhc_reward_info_dim(int reward_id);

/* kp_sim_uhc_track with cfg->reward_id's reward (the table above): the tail of HumanoidEnv.step (humanoid_im.py:527-572) and
 * reward_func[cfg.reward_id] (reward_function.py:453-460) in one launch, one wavefront per env.  info [N, kp_uhc_reward_info_dim(reward_id)]; the
 * other arguments are kp_sim_uhc_track's.  Errors (nothing launched): kp_sim_uhc_track's, an unknown reward_id, NULL jpos_diffw for v2 / v3, NULL
 * prev_qpos for local_rfc_implicit. */
int kp_sim_uhc_track_r(kp_sim*, const kp_takes*, const kp_uhc_state* st, const kp_uhc_cfg_r* cfg, const float* cc_action,
                       float* reward, float* info, float* body_diff, uint8_t* fail, uint8_t* end, uint8_t* done, float* percent);

const char* kp_last_error(void);
const char* kp_version(void);

/* ---- the backward side of the kinematic roll-out in train form (kinpoly_amd/csrc/kp_kin_tape.hip) ----
 *
 * TrajARNet.forward with a tape (kin_poly/models/traj_ar_smpl_net.py:346-383): the three gradients autograd takes through get_obs (:203-290), step
 * (:292-330) and get_qvel_fd_batch (kin_poly/utils/torch_utils.py:315-331), as one kernel beside each forward kernel.  fp32, rows independent, no
 * atomics.  They are the derivatives of the forward KERNELS' formulas: a rotation normalises its quaternion there, so a raw root quaternion gets no
 * radial gradient.  Every entry refuses (-1, kp_last_error, nothing launched) a null required pointer and a negative row count; zero rows do nothing.
 *
 * kp_kin_advance_backward: (d kp_kin_advance)^T.  qpos [n,76], kin_action [n,80], dt: the forward call's inputs; grad_next_qpos [n,76] and
 * grad_qvel [n,75]: cotangents of its outputs, either may be NULL (zero); -> grad_qpos [n,76], grad_action [n,80].  Rows of the forward kernel's
 * `no rotation` branch (dt * angv exactly zero, or |xyz| of next (x) cur^-1 exactly zero) get a zero angular-velocity gradient, as torch.where
 * gives in get_qvel_fd_batch; rows with 0 < |dt * angv| < 1e-12 (quat_from_expmap's guard) are outside the domain. */
int kp_kin_advance_backward(int n, const float* qpos, const float* kin_action, float dt, const float* grad_next_qpos, const float* grad_qvel,
                            float* grad_qpos, float* grad_action, void* hip_stream);

/* (d kp_sim_obs_ar)^T for the first n_rows (<= N) rows of the handle's layout (get_ar_obs_v1, humanoid_ar_v1.py:133-214; TrajARNet.get_obs,
 * traj_ar_smpl_net.py:203-290): grad_obs [n_rows, grad_width], grad_width = kp_sim_ar_obs_dim (refused otherwise); grad_obj_2_head [n_rows,7]
 * (may be NULL) is added to the object block's cotangent (the loss reads that block as a feature, :281-287).  qpos [n_rows,76] are the rows the
 * observation was taken of, wbpos / wbquat their kp_sim_fk outputs; ctx as for kp_sim_obs_ar (head_pose, action_one_hot, obj_qpos, cur_t, row).
 * -> grad_qpos [n_rows,76]: the local pose block's part only; grad_qvel [n_rows,75]: the velocity block's cotangent (use_vel layouts, else
 * ignored and may be NULL); grad_hpos [n_rows,3], grad_hquat [n_rows,4]: cotangents of the head's position and world quaternion, for
 * kp_sim_fk_head_backward.  The 81 / 156 layouts (use_head and use_action both off, which Config refuses) are refused. */
int kp_sim_obs_ar_backward(kp_sim*, const kp_ctx* ctx, int n_rows, int grad_width, const float* qpos, const float* wbpos, const float* wbquat,
                           const float* grad_obs, const float* grad_obj_2_head, float* grad_qpos, float* grad_qvel, float* grad_hpos, float* grad_hquat);

/* kp_sim_fk_backward plus the head's world quaternion (Humanoid.qpos_fk, kin_poly/utils/torch_smpl_humanoid.py:125-202, as get_obs reads it,
 * traj_ar_smpl_net.py:222-230): grad_qpos [n_rows,76] = (d wbpos / d qpos)^T (grad_wbpos [n_rows,72] with grad_hpos [n_rows,3] added to the head's
 * slot) + (d head quaternion / d qpos)^T grad_hquat [n_rows,4] + grad_qpos_add [n_rows,76].  The four cotangents may each be NULL (zero);
 * grad_qpos_add may be grad_qpos itself. */
int kp_sim_fk_head_backward(kp_sim*, int n_rows, const float* qpos, const float* wbpos, const float* wbquat, const float* grad_wbpos,
                            const float* grad_hpos, const float* grad_hquat, const float* grad_qpos_add, float* grad_qpos);

/* The kinematic model's observation under `use_context` / `use_of` (config/statear/kin_only.yml, use_of.yml; TrajARNet.get_obs,
 * traj_ar_smpl_net.py:226-230, 284-285): one launch writes out [N, ctx_dim + kp_sim_ar_obs_dim + of_dim] = [context GRU's hidden state at the row's
 * frame | kp_sim_obs_ar's row, the same words | the frame's image feature].  Both tables are read at the frame and row kp_sim_obs_ar reads
 * (ctx->cur_t clamped into [0, T - 1], ctx->row): element (row r, frame t, column c) of a table is at r * stride_row + t * stride_t + c, strides in
 * floats, so [R, T, .] and [T, R, .] storage both serve.  ctx_feat NULL with ctx_dim > 0 writes zeros (the row before init_states, :229-230).
 * Refused with -1 before any launch: a negative dim, of_dim > 0 with of NULL, a stride < 1 of a non-NULL table, and what kp_sim_obs_ar refuses. */
typedef struct { int ctx_dim; const float* ctx_feat; long ctx_stride_row, ctx_stride_t;   /* strides in floats: env-major or time-major */
                 int of_dim;  const float* of;       long of_stride_row,  of_stride_t; } kp_obs_ext;
int kp_sim_obs_ar_ex(kp_sim*, const kp_ctx* ctx, const kp_obs_ext* ext, float* out);
/* (d kp_sim_obs_ar_ex)^T: kp_sim_obs_ar_backward on the base block of grad_obs [n_rows, grad_width], grad_width = ext->ctx_dim + kp_sim_ar_obs_dim
 * + ext->of_dim (refused otherwise), and grad_ctx [n_rows, ctx_dim] <- the context block's cotangent, grad_obs's first ctx_dim columns (may be NULL
 * when ctx_dim is 0).  The `of` block is data.  The other arguments, outputs and refusals (the 81 / 156 layouts among them) are
 * kp_sim_obs_ar_backward's. */
int kp_sim_obs_ar_ex_backward(kp_sim*, const kp_ctx* ctx, const kp_obs_ext* ext, int n_rows, int grad_width, const float* qpos, const float* wbpos,
                              const float* wbquat, const float* grad_obs, const float* grad_obj_2_head, float* grad_qpos, float* grad_qvel,
                              float* grad_hpos, float* grad_hquat, float* grad_ctx);

/* kp_rollout_record_pre_w / _post_w for the rows of an env whose observation carries a context / `of` block (kp_sim_obs_ar_ex): obs_dim = ctx_dim +
 * base + of_dim with base one of the eight layout widths; anything else fails and nothing is launched.  The kernels are the ones above (the width is
 * their argument). */
int kp_rollout_record_pre_x(const kp_record_pre*, int obs_dim, int ctx_dim, int of_dim, void* hip_stream);
int kp_rollout_record_post_x(const kp_record_post*, int obs_dim, int ctx_dim, int of_dim, void* hip_stream);

/* The ring refill of the two wide context tables (the tables kp_obs_ext points to, row-major [R, T, .]), one launch: for clip c < m, frame t < T
 *   ctx_table[rows[c], t, :ctx_dim] = seq[min(t, Tp - 1), c, :]     seq: time-major [Tp, m, ctx_dim], the context GRU's hidden states as its step writes them
 *   of_table [rows[c], t, :of_dim]  = of [c, min(t, Tp - 1), :]     of:  [m, Tp, of_dim], the data set's image features
 * (a clip shorter than the tables is padded with its last frame).  A table whose width is 0 is not written and its source not read.  rows: device
 * int64 [m]; rows_host: the same values in host memory, checked here.  Refused with -1 before any launch: a row outside [0, R), Tp < 1 or Tp > T, a
 * NULL table with a non-zero width, a table without its source, rows / sources / tables that are not device memory.  m == 0 returns 0 without a
 * launch.  Duplicate rows are the caller's error: two clips would race for one row (the sampler's refill plan never names a row twice). */
int kp_ctx_rows_write(int m, int R, int T, int Tp, int ctx_dim, int of_dim, const int64_t* rows, const int64_t* rows_host, const float* seq, const float* of,
                      float* ctx_table, float* of_table, void* hip_stream);


#ifdef __cplusplus
}
#endif
#endif
