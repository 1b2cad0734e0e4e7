// kp_obs_ctx.hip -- the kernels declared in kp_obs_ctx.hpp (see there).  The base block and the gate math restate the expressions of k_obs_ar
// (kp_rollout_kernels.hpp, with the quaternion helpers of kp_obs_kernels.hpp) and k_gru_cell_step (kp_policy_kernels.hpp) operator for operator: those
// headers define non-template kernels and belong to kp_sim.hip alone, and the words written here must be theirs bit for bit
// (tests/test_gpu_context_obs.py holds both to it).
#include "kp_obs_ctx.hpp"

namespace kp {

namespace {

__device__ __forceinline__ Q4 oc_inverse(Q4 q) {  // q_inverse
    float n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    return Q4{q.w / n, -q.x / n, -q.y / n, -q.z / n};
}
__device__ __forceinline__ void oc_matrix(Q4 q, float* m) {  // q_matrix
    float n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    if (n < 8.881784197001252e-16f) { m[0] = m[4] = m[8] = 1.f; m[1] = m[2] = m[3] = m[5] = m[6] = m[7] = 0.f; return; }
    float s = sqrtf(2.0f / n);
    float w = q.w * s, x = q.x * s, y = q.y * s, z = q.z * s;
    m[0] = 1.f - y * y - z * z; m[1] = x * y - z * w; m[2] = x * z + y * w;
    m[3] = x * y + z * w; m[4] = 1.f - x * x - z * z; m[5] = y * z - x * w;
    m[6] = x * z - y * w; m[7] = y * z + x * w; m[8] = 1.f - x * x - y * y;
}
// q_tmul_vec.  Each component is a sum of three products, which the compiler contracts into one product and two fused multiply-adds; which product stays
// the plain one is its choice, and in this unit it chose another one for y than in k_obs_ar / k_obs_ar_thread (one ulp in that column).  The
// contraction those two kernels were compiled to is therefore written out: x keeps m3 vy, y keeps m1 vx, z keeps m2 vx.
__device__ __forceinline__ V3 oc_tmul_vec(Q4 q, V3 v) {
    float m[9]; oc_matrix(q, m);
    return V3{fmaf(m[6], v.z, fmaf(m[0], v.x, m[3] * v.y)), fmaf(m[7], v.z, fmaf(m[4], v.y, m[1] * v.x)), fmaf(m[8], v.z, fmaf(m[5], v.y, m[2] * v.x))};
}
__device__ __forceinline__ Q4 oc_heading(Q4 q) {  // q_heading
    float n = sqrtf(q.w * q.w + q.z * q.z);
    return Q4{q.w / n, 0.f, 0.f, q.z / n};
}
__device__ __forceinline__ V3 oc_tv_heading(V3 v, Q4 q) { return oc_tmul_vec(oc_heading(q), v); }  // tv_heading
__device__ __forceinline__ float oc_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }        // kp_sigmoid

}  // namespace

// ---------------------------------------------------------------- [ctx H | base W | of F], k_obs_ar's mapping: 32 lanes per env, 8 envs per 256-thread block
// The two wide blocks are copied lane-strided like the velocity block (a wavefront moves runs of 32 consecutive floats of two consecutive rows); a row
// of 357 floats is not 16-byte aligned, so the accesses are plain dwords.  The base block follows with k_obs_ar's statements at column H.
// The base block's part is k_obs_ar's text with its parameter list (the same __restrict__ qualifiers: what the compiler may keep in registers across the stores
// decides how it contracts the heading rotation); CtxLike mirrors kp::CtxDev, WideBlocks carries kp_obs_ext.
struct CtxLike {
    int T;
    const float *head_pose, *head_vels, *obj_rel, *action_one_hot, *gt_bquat, *gt_wbpos, *obj_qpos;
    const int* cur_t;
    const int* row;
    __device__ __forceinline__ size_t r(int e) const { return row ? (size_t)row[e] : (size_t)e; }
};
struct WideBlocks { int ctx_dim; const float* ctx_feat; long long ctx_stride_row, ctx_stride_t; int of_dim; const float* of; long long of_stride_row, of_stride_t; };

template <bool VEL, bool HEAD, bool ACTION>
__global__ __launch_bounds__(256) void k_obs_ar_ctx(int n, CtxLike C, const float* __restrict__ qpos, const float* __restrict__ qvel,
                                                     const float* __restrict__ xpos, const float* __restrict__ xquat, float* __restrict__ out, WideBlocks X) {
    constexpr int O_VEL = 74, O_DIFF = O_VEL + (VEL ? 75 : 0), O_OBJ = O_DIFF + (HEAD ? 7 : 0), O_TGT = O_OBJ + 7, O_ACT = O_TGT + (HEAD ? 13 : 0),
                  D = O_ACT + (ACTION ? 4 : 0);      // kp::ObsArLayout
    const int l = threadIdx.x & 31, e = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (e >= n) return;
    const int H = X.ctx_dim, F = X.of_dim;
    float* wide = out + (size_t)e * (size_t)(H + D + F);
    {
        int tw = C.cur_t[e];
        tw = tw < 0 ? 0 : (tw >= C.T ? C.T - 1 : tw);
        const long long rw = (long long)C.r(e);
        if (X.ctx_feat) {
            const float* __restrict__ c = X.ctx_feat + rw * X.ctx_stride_row + (long long)tw * X.ctx_stride_t;
            for (int j = l; j < H; j += 32) wide[j] = c[j];
        } else {
            for (int j = l; j < H; j += 32) wide[j] = 0.f;      // no sequence yet (traj_ar_smpl_net.py:229-230)
        }
        if (F > 0) {
            const float* __restrict__ f = X.of + rw * X.of_stride_row + (long long)tw * X.of_stride_t;
            for (int j = l; j < F; j += 32) wide[H + D + j] = f[j];
        }
    }
    // ---- k_obs_ar from here on, o at column H of the wide row
    const float* q = qpos + (size_t)e * D_NQ;
    float* o = wide + H;
    for (int j = l; j < D_NU; j += 32) o[5 + j] = q[7 + j];
    if (VEL) {
        const float* v = qvel + (size_t)e * D_NV;
        for (int j = l; j < D_NV; j += 32) o[O_VEL + j] = v[j];
    }
    if (l > 4) return;
    if (l == 0) {
        Q4 rq = Q4{q[3], q[4], q[5], q[6]};
        Q4 dh = qmul(oc_inverse(oc_heading(rq)), rq);  // de_heading(qpos[3:7]) (:140-141)
        o[0] = q[2]; o[1] = dh.w; o[2] = dh.x; o[3] = dh.y; o[4] = dh.z;
        return;
    }
    int t = C.cur_t[e];
    t = t < 0 ? 0 : (t >= C.T ? C.T - 1 : t);
    const float* oh = C.action_one_hot + C.r(e) * 4;
    if (l == 4) {
        if (ACTION) for (int k = 0; k < 4; k++) o[O_ACT + k] = oh[k];
        return;
    }
    if (l == 3) {
        if (HEAD) {
            const float* hv = C.head_vels + (C.r(e) * C.T + t) * 6;
            const float* orl = C.obj_rel + (C.r(e) * C.T + t) * 7;
            float* g = o + O_TGT;
            g[0] = hv[3]; g[1] = hv[4]; g[2] = hv[5];
            g[3] = hv[0]; g[4] = hv[1]; g[5] = hv[2];
            for (int k = 0; k < 7; k++) g[6 + k] = orl[k];
        }
        return;
    }
    const int hb = 13;
    V3 hpos = ld3(xpos + (size_t)e * 72 + 3 * hb);
    const float* hq4 = xquat + (size_t)e * 96 + 4 * hb;
    Q4 hrot = Q4{hq4[0], hq4[1], hq4[2], hq4[3]};
    if (l == 1) {
        if (HEAD) {
            const float* hp = C.head_pose + (C.r(e) * C.T + t) * 7;
            st3(o + O_DIFF, oc_tv_heading(ld3(hp) - hpos, hrot));
            Q4 dr = qmul(oc_inverse(Q4{hp[3], hp[4], hp[5], hp[6]}), hrot);
            float* g = o + O_DIFF + 3;
            g[0] = dr.w; g[1] = dr.x; g[2] = dr.y; g[3] = dr.z;
        }
        return;
    }
    float ohs = oh[0] + oh[1] + oh[2] + oh[3];
    V3 opos = v3(0.f, 0.f, 0.f); Q4 orot = Q4{1.f, 0.f, 0.f, 0.f};   // get_obj_qpos: [0,0,0,1,0,0,0] when no action (:465-466)
    if (ohs != 0.f && C.obj_qpos) { const float* ob = C.obj_qpos + (size_t)e * 7; opos = ld3(ob); orot = Q4{ob[3], ob[4], ob[5], ob[6]}; }
    st3(o + O_OBJ, oc_tv_heading(opos - hpos, hrot));
    Q4 ol = qmul(oc_inverse(oc_heading(hrot)), orot);
    float* g = o + O_OBJ + 3;
    g[0] = ol.w; g[1] = ol.x; g[2] = ol.y; g[3] = ol.z;
}

// ---------------------------------------------------------------- k_gru_cell_step with a state wider than the hidden state: thread (e, j) copies columns j, j + H, ...
__global__ void k_gru_cell_step_wide(int n, int H, int D, const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ b_ih,
                                     const float* __restrict__ b_hh, const float* h_in, const float* __restrict__ state, float* h_out, float* __restrict__ xcat) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * H) return;
    const int e = (int)(idx / H), j = (int)(idx - (size_t)e * H);
    const float* a = gi + (size_t)e * 3 * H; const float* b = gh + (size_t)e * 3 * H;
    const float r = oc_sigmoid(a[j] + b_ih[j] + b[j] + b_hh[j]);
    const float z = oc_sigmoid(a[H + j] + b_ih[H + j] + b[H + j] + b_hh[H + j]);
    const float nn = tanhf(a[2 * H + j] + b_ih[2 * H + j] + r * (b[2 * H + j] + b_hh[2 * H + j]));
    const float h = (1.0f - z) * nn + z * h_in[idx];
    h_out[idx] = h;
    float* xr = xcat + (size_t)e * (D + H);
    xr[D + j] = h;
    const float* s = state + (size_t)e * D;
    for (int c = j; c < D; c += H) xr[c] = s[c];
}

__global__ void k_obs_ctx_grad(int n, int H, const float* __restrict__ g_obs, int pitch, float* __restrict__ g_ctx) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * H) return;
    const size_t e = idx / H;
    g_ctx[idx] = g_obs[e * (size_t)pitch + (idx - e * H)];
}

// ---------------------------------------------------------------- ring refill of the wide context tables: block = (clip, frame), lanes along the features
__global__ __launch_bounds__(256) void k_ctx_rows_write(CtxRowsArgs A) {
    const int c = blockIdx.x / A.T, t = blockIdx.x - c * A.T;
    if (c >= A.m) return;
    const long long r = A.rows[c];
    if (r < 0 || r >= (long long)A.R) return;                       // refused by the entry point; never written through
    const int ts = t < A.Tp ? t : A.Tp - 1;                        // last-frame padding of a clip shorter than the tables
    const size_t dst = (size_t)r * A.T + t;
    if (A.ctx_table) {
        const float* __restrict__ s = A.seq + ((size_t)ts * A.m + c) * A.H;
        float* __restrict__ d = A.ctx_table + dst * A.H;
        for (int j = threadIdx.x; j < A.H; j += 256) d[j] = s[j];
    }
    if (A.of_table) {
        const float* __restrict__ s = A.of + ((size_t)c * A.Tp + ts) * A.F;
        float* __restrict__ d = A.of_table + dst * A.F;
        for (int j = threadIdx.x; j < A.F; j += 256) d[j] = s[j];
    }
}

hipError_t launch_obs_ar_ctx(const ObsArCtxArgs& A, hipStream_t stream) {
    const dim3 grid((A.n + 7) / 8), block(256);
    CtxLike C;
    C.T = A.T; C.head_pose = A.head_pose; C.head_vels = A.head_vels; C.obj_rel = A.obj_rel; C.action_one_hot = A.action_one_hot; C.gt_bquat = nullptr; C.gt_wbpos = nullptr;
    C.obj_qpos = A.obj_qpos; C.cur_t = A.cur_t; C.row = A.row;
    const WideBlocks X{A.ctx_dim, A.ctx_feat, A.ctx_stride_row, A.ctx_stride_t, A.of_dim, A.of, A.of_stride_row, A.of_stride_t};
#define KP_OBS_CTX(V, H, AC) hipLaunchKernelGGL((k_obs_ar_ctx<V, H, AC>), grid, block, 0, stream, A.n, C, A.qpos, A.qvel, A.xpos, A.xquat, A.out, X)
    switch ((A.vel ? 1 : 0) | (A.head ? 2 : 0) | (A.action ? 4 : 0)) {
        case 0: KP_OBS_CTX(false, false, false); break;
        case 1: KP_OBS_CTX(true, false, false); break;
        case 2: KP_OBS_CTX(false, true, false); break;
        case 3: KP_OBS_CTX(true, true, false); break;
        case 4: KP_OBS_CTX(false, false, true); break;
        case 5: KP_OBS_CTX(true, false, true); break;
        case 6: KP_OBS_CTX(false, true, true); break;
        default: KP_OBS_CTX(true, true, true); break;
    }
#undef KP_OBS_CTX
    return hipGetLastError();
}

hipError_t launch_gru_cell_step_wide(int n, int H, int D, const float* gi, const float* gh, const float* b_ih, const float* b_hh, const float* h_in, const float* state,
                                     float* h_out, float* xcat, hipStream_t stream) {
    const size_t tot = (size_t)n * H;
    hipLaunchKernelGGL(k_gru_cell_step_wide, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, n, H, D, gi, gh, b_ih, b_hh, h_in, state, h_out, xcat);
    return hipGetLastError();
}

hipError_t launch_obs_ctx_grad(int n, int H, const float* grad_obs, int pitch, float* grad_ctx, hipStream_t stream) {
    const size_t tot = (size_t)n * H;
    hipLaunchKernelGGL(k_obs_ctx_grad, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, n, H, grad_obs, pitch, grad_ctx);
    return hipGetLastError();
}

hipError_t launch_ctx_rows_write(const CtxRowsArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(k_ctx_rows_write, dim3((unsigned)((size_t)A.m * A.T)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace kp
