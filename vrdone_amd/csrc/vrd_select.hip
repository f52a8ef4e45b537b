// Segmented triplet selection: the candidate filter and the per-video top-n_max_pair of MaskVRD.forward_test
// (models/maskvrd.py, reference maskvrd.py:247-300) for many videos in ONE launch, one workgroup per video.
//
// A video's candidates are its (pair, query, class rank) triples in flat order i = (pair * Q + query) * k + rank.  A candidate
// is kept when the query's segment is not empty and spans at least pred_min_frames frames; its score is the mean of the
// subject's, the predicate's and the object's score, bit for bit as torch computes `torch.stack(...).mean(-1)` on the GPU
// (see torch_mean3).  The selection is the first n_max_pair kept candidates in descending score order, ties to the lower flat
// index: torch.argsort(descending=True, stable=True) over nonzero(keep).
//
// Each candidate gets a 64-bit key [order-preserving score bits | 0xffffffff - i]; keys are unique, so the n-th largest key
// splits the kept candidates exactly.  The workgroup finds it with a radix select (8 passes of 8 bits over its segment,
// recomputing the keys from the candidate records: a video of 2070 pairs has ~150 k candidates, more than LDS holds), gathers
// the n keys at or above it into LDS and sorts them there (bitonic).
#include "vrd_common.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_MAX_KEEP = 4096;           // n_max_pair bound: the survivors are sorted in LDS (32 KiB)

// torch's mean over the last dim of an (N, 3) float tensor on the GPU (ATen Reduce.cuh, MeanOps): the reduction is split over
// a block width of last_pow2(3) = 2 threads, thread 0 accumulating elements 0 and 2 in two of its four accumulators, thread 1
// element 1; the accumulators start at 0 and are combined in order, then the two threads' values (shuffle down), then the sum
// is scaled by factor = float(N) / (3N).  The additions of 0 are kept: they turn -0 into +0 as torch's do.
__device__ __forceinline__ float torch_mean3(float s, float p, float o, float factor) {
    const float t0 = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(0.f, s), __fadd_rn(0.f, o)), 0.f), 0.f);
    const float t1 = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(0.f, p), 0.f), 0.f), 0.f);
    return __fmul_rn(__fadd_rn(t0, t1), factor);
}

// descending score, then ascending index; -0 sorts as +0
__device__ __forceinline__ uint64_t sel_key(float score, uint32_t i) {
    uint32_t u = __float_as_uint(score);
    if (u == 0x80000000u) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - i);
}

__device__ __forceinline__ float key_score(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// candidate i of the video whose pairs start at p0: 0 = dropped, 1 = kept, 3 = kept but outside its pair's shared frames
__device__ __forceinline__ int sel_eval(const vrd_select_args& a, int p0, int i, float factor, uint64_t& key) {
    const int Qk = a.Q * a.k;
    const int pl = i / Qk, rem = i - pl * Qk;
    const int q = rem / a.k, r = rem - q * a.k;
    const int p = p0 + pl;
    const float* rec = a.cand + ((int64_t)p * a.Q + q) * (2 * a.k + 2);
    const int first = __float_as_int(rec[2 * a.k]), last = __float_as_int(rec[2 * a.k + 1]);
    if (last < 0) return 0;
    const int64_t off = a.so_offset[p];
    const int64_t start = (int64_t)first * a.feat_stride + off, end = (int64_t)last * a.feat_stride + off + 1;
    if (end - start < a.pred_min_frames) return 0;
    key = sel_key(torch_mean3(a.s_score[p], rec[r], a.o_score[p], factor), (uint32_t)i);
    return (start >= 0 && end <= (int64_t)a.so_end[p] - a.so_start[p]) ? 1 : 3;
}

__global__ __launch_bounds__(SEL_THREADS) void select_triplets_kernel(vrd_select_args a) {
    __shared__ uint64_t keys[SEL_MAX_KEEP];
    __shared__ int hist[256];
    __shared__ int s_kept, s_bad, s_fill, s_remaining;
    __shared__ uint64_t s_prefix;
    const int v = blockIdx.x;
    const int tid = threadIdx.x;
    const int p0 = a.video_pairs[v], p1 = a.video_pairs[v + 1];
    const int n = (p1 - p0) * a.Q * a.k;
    // torch: static_cast<float>(num_output_elements) / numel, the int64 numel converted to float
    const float factor = (float)n / (float)(3 * (int64_t)n);
    if (tid == 0) s_kept = 0, s_bad = 0, s_fill = 0, s_prefix = 0;
    __syncthreads();
    int kept = 0, bad = 0;
    for (int i = tid; i < n; i += SEL_THREADS) {
        uint64_t key;
        const int e = sel_eval(a, p0, i, factor, key);
        kept += e & 1;
        bad += e >> 1;
    }
    atomicAdd(&s_kept, kept);
    if (bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    const int need = min(s_kept, a.n_max_pair);
    if (tid == 0) s_remaining = need;
    // radix select of the need-th largest key, 8 bits at a time from the top
    uint64_t mask = 0;
    for (int shift = 56; shift >= 0 && need > 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        const uint64_t prefix = s_prefix;
        for (int i = tid; i < n; i += SEL_THREADS) {
            uint64_t key;
            if ((sel_eval(a, p0, i, factor, key) & 1) && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int above = 0;
            for (int b = 255; b >= 0; --b) {
                if (above + hist[b] >= s_remaining) {
                    s_prefix = prefix | ((uint64_t)b << shift);
                    s_remaining -= above;
                    break;
                }
                above += hist[b];
            }
        }
        mask |= (uint64_t)255 << shift;
        __syncthreads();
    }
    const uint64_t threshold = s_prefix;
    if (need > 0) {
        for (int i = tid; i < n; i += SEL_THREADS) {
            uint64_t key;
            if ((sel_eval(a, p0, i, factor, key) & 1) && key >= threshold) {
                const int slot = atomicAdd(&s_fill, 1);
                if (slot < SEL_MAX_KEEP) keys[slot] = key;
            }
        }
    }
    int m = 1;
    while (m < need) m <<= 1;
    __syncthreads();
    for (int j = need + tid; j < m; j += SEL_THREADS) keys[j] = 0;        // (below every real key: its index part is > 0)
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < m / 2; t += SEL_THREADS) {
                const int lo = 2 * stride * (t / stride) + (t % stride), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t x = keys[lo], y = keys[hi];
                if ((x < y) == desc) keys[lo] = y, keys[hi] = x;
            }
            __syncthreads();
        }
    }
    int32_t* idx = a.out_index + (int64_t)v * a.n_max_pair;
    float* score = a.out_score ? a.out_score + (int64_t)v * a.n_max_pair : nullptr;
    for (int j = tid; j < a.n_max_pair; j += SEL_THREADS) {
        const bool live = j < need;
        idx[j] = live ? (int32_t)(0xffffffffu - (uint32_t)keys[j]) : -1;
        if (score) score[j] = live ? key_score(keys[j]) : 0.f;
    }
    if (tid == 0) {
        a.out_count[2 * v] = s_fill == need ? need : -1;            // (-1: the keys were not unique -- cannot happen)
        a.out_count[2 * v + 1] = s_bad;
    }
}

}  // namespace

extern "C" int vrd_select_triplets(const vrd_select_args* a, void* stream) {
    VRD_CHECK_ARG(a && a->cand && a->s_score && a->o_score && a->so_offset && a->so_start && a->so_end && a->video_pairs &&
                  a->out_count && a->out_index, "vrd_select_triplets: null pointer");
    VRD_CHECK_ARG(a->n_videos > 0 && a->Q > 0 && a->k > 0 && a->feat_stride > 0, "vrd_select_triplets: bad sizes");
    VRD_CHECK_ARG(a->n_max_pair >= 1 && a->n_max_pair <= SEL_MAX_KEEP, "vrd_select_triplets: n_max_pair must be 1..%d (got %d)",
                  SEL_MAX_KEEP, a->n_max_pair);
    VRD_CHECK_ARG((int64_t)a->max_video_pairs * a->Q * a->k < ((int64_t)1 << 31) - 1,
                  "vrd_select_triplets: %d pairs x %d queries x %d ranks do not fit 32-bit candidate indices", a->max_video_pairs,
                  a->Q, a->k);
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(select_triplets_kernel, dim3((unsigned)a->n_videos), dim3(SEL_THREADS), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}
