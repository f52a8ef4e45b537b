// Optimiser tail on the device: gradient-norm clipping and the AdamW update of every parameter of a step in
// three launches, over the same kind of tables vrd_ema_update takes (device arrays of device pointers, a chunk map of 4,096
// elements per workgroup).  train.py:187-190 runs torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW.step there: a Python
// walk over ~520 parameters and chunked _foreach_* launches.
//
//  vrd_grad_sumsq        partial[c] = sum of g^2 over chunk c, in double (g^2 is exact there), no atomics
//  vrd_grad_norm_finish  one workgroup adds the partials in a fixed tree: out = {total_norm, clip_coef}
//  vrd_adamw_step        torch's AdamW update (non-capturable single-tensor form, torch/optim/adam.py) on g * clip_coef
//  vrd_scale_tensors     g *= clip_coef in place (the standalone clip)
//
// Element -> thread mapping: thread t of a chunk's workgroup owns the four elements 4 * (t + 256 * k) .. + 3 of the chunk, k =
// 0 .. 3, whether the tensor takes the float4 form (all of its pointers 16-byte aligned: vec[t] != 0) or the scalar form.  Sums
// therefore run in the same order in both forms: a result depends on values and shapes, never on where a tensor was allocated.
// The arithmetic is compiled without FMA contraction: every product and sum is rounded to f32 like the separate tensor
// operations of torch's update, and g * clip_coef is the same number whether this launch forms it or vrd_scale_tensors
// stored it (the folded clip equals clip-then-step bit for bit).
#include "vrd_common.h"

namespace {

constexpr int OPT_CHUNK = 4096, OPT_THREADS = 256, OPT_TRIPS = OPT_CHUNK / (4 * OPT_THREADS);
constexpr int FINISH_THREADS = 1024;
constexpr int GROUP_FLOATS = VRD_ADAMW_GROUP_FLOATS;

__device__ __forceinline__ float4 load4(const float* p, int64_t i, int64_t n, bool vec) {
    if (vec && i + 3 < n) return *reinterpret_cast<const float4*>(p + i);
    float4 v;
    v.x = i < n ? p[i] : 0.f;
    v.y = i + 1 < n ? p[i + 1] : 0.f;
    v.z = i + 2 < n ? p[i + 2] : 0.f;
    v.w = i + 3 < n ? p[i + 3] : 0.f;
    return v;
}

__device__ __forceinline__ void store4(float* p, int64_t i, int64_t n, bool vec, float4 v) {
    if (vec && i + 3 < n) {
        *reinterpret_cast<float4*>(p + i) = v;
        return;
    }
    if (i < n) p[i] = v.x;
    if (i + 1 < n) p[i + 1] = v.y;
    if (i + 2 < n) p[i + 2] = v.z;
    if (i + 3 < n) p[i + 3] = v.w;
}

// sum over the workgroup in a fixed tree (xor shuffles inside a wave, then the waves' sums in index order); valid in thread 0
template <int THREADS>
__device__ __forceinline__ double block_sum(double s) {
    __shared__ double wave_sum[THREADS / 64];
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / 64; ++w) total += wave_sum[w];
    return total;
}

__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(const float* const* __restrict__ grad, const int64_t* __restrict__ numel,
                                                                 const int32_t* __restrict__ vec, const int32_t* __restrict__ chunk_tensor,
                                                                 const int32_t* __restrict__ chunk_index, double* __restrict__ partial) {
    const int t = chunk_tensor[blockIdx.x];
    const int64_t base = (int64_t)chunk_index[blockIdx.x] * OPT_CHUNK, n = numel[t];
    const float* const g = grad[t];
    const bool v4 = vec[t] != 0;
    float4 v[OPT_TRIPS];
#pragma unroll
    for (int k = 0; k < OPT_TRIPS; ++k) v[k] = load4(g, base + 4 * (threadIdx.x + OPT_THREADS * k), n, v4);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_TRIPS; ++k) {
        s += (double)v[k].x * (double)v[k].x;
        s += (double)v[k].y * (double)v[k].y;
        s += (double)v[k].z * (double)v[k].z;
        s += (double)v[k].w * (double)v[k].w;
    }
    s = block_sum<OPT_THREADS>(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(FINISH_THREADS) void grad_norm_finish_kernel(const double* __restrict__ partial, int n, float max_norm,
                                                                          float* __restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += FINISH_THREADS) s += partial[i];          // thread t: partials t, t + 1024, ... in order
    s = block_sum<FINISH_THREADS>(s);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(s);
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0); a NaN norm stays a NaN coefficient
    double coef = 1.0;
    if (max_norm > 0.f) {
        const double c = (double)max_norm / (norm + 1e-6);
        coef = c < 1.0 ? c : (c != c ? c : 1.0);
    }
    out[0] = (float)norm;
    out[1] = (float)coef;
}

__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float coef, float keep, float beta2, float one_minus_beta1,
                                              float one_minus_beta2, float eps, float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
    g = g * coef;
    p = p * keep;                                          // param.mul_(1 - lr * weight_decay)
    m = m + one_minus_beta1 * (g - m);                     // exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + one_minus_beta2 * g * g;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(float* const* __restrict__ param, const float* const* __restrict__ grad,
                                                            float* const* __restrict__ exp_avg, float* const* __restrict__ exp_avg_sq,
                                                            const int64_t* __restrict__ numel, const int32_t* __restrict__ group,
                                                            const int32_t* __restrict__ vec, const float* __restrict__ groups,
                                                            const int32_t* __restrict__ chunk_tensor, const int32_t* __restrict__ chunk_index,
                                                            const float* __restrict__ clip_coef) {
#pragma clang fp contract(off)
    const int t = chunk_tensor[blockIdx.x];
    const int64_t base = (int64_t)chunk_index[blockIdx.x] * OPT_CHUNK, n = numel[t];
    float* const p = param[t];
    const float* const g = grad[t];
    float* const m = exp_avg[t];
    float* const v = exp_avg_sq[t];
    const bool v4 = vec[t] != 0;
    const float* const h = groups + (int64_t)group[t] * GROUP_FLOATS;
    const float keep = 1.f - h[0], beta2 = h[2], eps = h[3], step_size = h[4], bc2_sqrt = h[5], omb1 = h[6], omb2 = h[7];
    const float coef = clip_coef ? clip_coef[0] : 1.f;
    float4 pv[OPT_TRIPS], gv[OPT_TRIPS], mv[OPT_TRIPS], vv[OPT_TRIPS];
#pragma unroll
    for (int k = 0; k < OPT_TRIPS; ++k) {
        const int64_t i = base + 4 * (threadIdx.x + OPT_THREADS * k);
        pv[k] = load4(p, i, n, v4);
        gv[k] = load4(g, i, n, v4);
        mv[k] = load4(m, i, n, v4);
        vv[k] = load4(v, i, n, v4);
    }
#pragma unroll
    for (int k = 0; k < OPT_TRIPS; ++k) {
        const int64_t i = base + 4 * (threadIdx.x + OPT_THREADS * k);
        if (i >= n) break;
        adamw_element(pv[k].x, gv[k].x, mv[k].x, vv[k].x, coef, keep, beta2, omb1, omb2, eps, step_size, bc2_sqrt);
        adamw_element(pv[k].y, gv[k].y, mv[k].y, vv[k].y, coef, keep, beta2, omb1, omb2, eps, step_size, bc2_sqrt);
        adamw_element(pv[k].z, gv[k].z, mv[k].z, vv[k].z, coef, keep, beta2, omb1, omb2, eps, step_size, bc2_sqrt);
        adamw_element(pv[k].w, gv[k].w, mv[k].w, vv[k].w, coef, keep, beta2, omb1, omb2, eps, step_size, bc2_sqrt);
        store4(p, i, n, v4, pv[k]);
        store4(m, i, n, v4, mv[k]);
        store4(v, i, n, v4, vv[k]);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void scale_tensors_kernel(float* const* __restrict__ grad, const int64_t* __restrict__ numel,
                                                                    const int32_t* __restrict__ vec, const int32_t* __restrict__ chunk_tensor,
                                                                    const int32_t* __restrict__ chunk_index, const float* __restrict__ clip_coef) {
#pragma clang fp contract(off)
    const int t = chunk_tensor[blockIdx.x];
    const int64_t base = (int64_t)chunk_index[blockIdx.x] * OPT_CHUNK, n = numel[t];
    float* const g = grad[t];
    const bool v4 = vec[t] != 0;
    const float coef = clip_coef[0];
#pragma unroll
    for (int k = 0; k < OPT_TRIPS; ++k) {
        const int64_t i = base + 4 * (threadIdx.x + OPT_THREADS * k);
        if (i >= n) break;
        float4 x = load4(g, i, n, v4);
        x.x = x.x * coef, x.y = x.y * coef, x.z = x.z * coef, x.w = x.w * coef;
        store4(g, i, n, v4, x);
    }
}

}  // namespace

extern "C" {

int vrd_grad_sumsq(const float* const* grad, const int64_t* numel, const int32_t* vec, const int32_t* chunk_tensor,
                   const int32_t* chunk_index, int n_chunks, double* partial, void* stream) {
    VRD_CHECK_ARG(grad && numel && vec && chunk_tensor && chunk_index && partial && n_chunks > 0, "vrd_grad_sumsq: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)n_chunks * OPT_CHUNK);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, s, grad, numel, vec, chunk_tensor, chunk_index, partial);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_grad_norm_finish(const double* partial, int n_chunks, float max_norm, float* out, void* stream) {
    VRD_CHECK_ARG(partial && out && n_chunks > 0, "vrd_grad_norm_finish: bad arguments");
    VRD_CHECK_ARG(max_norm == max_norm, "vrd_grad_norm_finish: max_norm is NaN");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 8.0 * (double)n_chunks);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(FINISH_THREADS), 0, s, partial, n_chunks, max_norm, out);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_adamw_step(float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                   const int32_t* group, const int32_t* vec, const float* groups, int n_groups, const int32_t* chunk_tensor,
                   const int32_t* chunk_index, int n_chunks, const float* clip_coef, void* stream) {
    VRD_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && numel && group && vec && groups && chunk_tensor && chunk_index,
                  "vrd_adamw_step: null table");
    VRD_CHECK_ARG(n_groups > 0 && n_chunks > 0, "vrd_adamw_step: n_groups (%d) and n_chunks (%d) must be positive", n_groups, n_chunks);
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 28.0 * (double)n_chunks * OPT_CHUNK);
    hipLaunchKernelGGL(adamw_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, s, param, grad, exp_avg, exp_avg_sq, numel, group, vec, groups,
                       chunk_tensor, chunk_index, clip_coef);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_scale_tensors(float* const* grad, const int64_t* numel, const int32_t* vec, const int32_t* chunk_tensor, const int32_t* chunk_index,
                      int n_chunks, const float* clip_coef, void* stream) {
    VRD_CHECK_ARG(grad && numel && vec && chunk_tensor && chunk_index && clip_coef && n_chunks > 0, "vrd_scale_tensors: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 8.0 * (double)n_chunks * OPT_CHUNK);
    hipLaunchKernelGGL(scale_tensors_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, s, grad, numel, vec, chunk_tensor, chunk_index, clip_coef);
    VRD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
