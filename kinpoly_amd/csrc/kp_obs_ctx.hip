// kp_obs_ctx.hip -- the kernels declared in kp_obs_ctx.hpp (see there).  The base block is obs_ar_row (kp_obs_ar_row.hpp), the text k_obs_ar itself
// is made of, so its words are kp_sim_obs_ar's by construction (tests/test_gpu_context_obs.py checks it).
#include "kp_obs_ctx.hpp"
#include "kp_obs_ar_row.hpp"

namespace kp {

// ---------------------------------------------------------------- [ctx H | base W | of F], k_obs_ar's mapping: 32 lanes per env, 8 envs per 256-thread block
// The two wide blocks are copied lane-strided like the velocity block (a wavefront moves runs of 32 consecutive floats of two consecutive rows); a row
// of 357 floats is not 16-byte aligned, so the accesses are plain dwords.  The base block follows at column H; WideBlocks carries kp_obs_ext.
struct WideBlocks { int ctx_dim; const float* ctx_feat; long long ctx_stride_row, ctx_stride_t; int of_dim; const float* of; long long of_stride_row, of_stride_t; };

template <bool VEL, bool HEAD, bool ACTION>
__global__ __launch_bounds__(256) void k_obs_ar_ctx(int n, CtxDev C, const float* __restrict__ qpos, const float* __restrict__ qvel,
                                                     const float* __restrict__ xpos, const float* __restrict__ xquat, float* __restrict__ out, WideBlocks X) {
    constexpr int D = ObsArLayout<VEL, HEAD, ACTION>::D;
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
    obs_ar_row<VEL, HEAD, ACTION>(C, e, l, qpos, qvel, xpos, xquat, wide + H);
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
    const CtxDev C{A.T, A.head_pose, A.head_vels, A.obj_rel, A.action_one_hot, nullptr, nullptr, A.obj_qpos, A.cur_t, A.row};      // the row reads no gt_* table
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
