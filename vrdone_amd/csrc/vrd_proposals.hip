// Eval proposals on the device (vrdone_amd/proposals.py prepare_test_videos; the reference dataloader's `_test_getitem`,
// dataloaders/vidvrd.py:552-715, up to the point where it starts copying features): box clamp, vIoU de-dup of the tracklets,
// and the pair tables of every video of a call.  Four launches over flat tables that span all videos (vrd_proposal_args):
//
// proposal_clamp_kernel   one wave per tracklet, lanes striding over its rows: the boxes clamped to the frame in place, and one
//                         byte per tracklet that says whether a box came out empty (or is not a number).
// proposal_shadow_kernel  one wave per unordered tracklet pair i < j of one video (the upper triangle, row-major, from the per-video
//                         offsets tri_first).  Same category and a shared frame: the lanes stride over the shared frames and form
//                         the reference's three sums -- per-frame terms in f32, every operation rounded on its own like the host's
//                         torch ops, accumulated in f64 and finished by a fixed-order butterfly, so a repeat gives the same bits.
//                         One byte per pair: bit 0 "i shadows j", bit 1 "j shadows i".
// proposal_walk_kernel    one wave per video reproduces the reference's greedy double loop over those bytes: rows i in order, a
//                         row's j in chunks of 64 lanes (see the kernel).  Also folds the tracklets' error bytes into the video's flag.
// proposal_pairs_kernel   one workgroup per video over its candidate (subject, object) pairs in their order: the kept ones
//                         compacted to the front of the video's slice by a ballot / LDS scan, the rest of the slice cleared.
//
// Every table offset is clamped or checked before it is used, so a broken table reads and writes nothing outside the buffers.
#include "vrd_common.h"

// every f32 operation below is rounded on its own, as the host's torch ops are: a fused multiply-add would keep a product unrounded
#pragma clang fp contract(off)

namespace {

constexpr int PROP_WAVES = 4;                // tracklets (clamp) / tracklet pairs (shadow) per workgroup
constexpr int PAIR_THREADS = 256;            // candidates per scan step

// butterfly sum over the 64 lanes: every lane ends with the same value, formed in the same order at every call
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ bool track_inside(int64_t row, int64_t frames, int64_t rows) {
    return row >= 0 && frames >= 0 && row <= rows && frames <= rows - row;
}

struct Tracklet {
    int64_t row, t0, n, cat, video;
};
__device__ __forceinline__ Tracklet load_tracklet(const int64_t* trk, int64_t k) {
    const int64_t* t = trk + 5 * k;
    return Tracklet{t[0], t[1], t[2], t[3], t[4]};
}

// tracklets [lo, hi) of video v, clamped to the table
__device__ __forceinline__ void video_tracklets(const vrd_proposal_args& a, int v, int& lo, int& hi) {
    lo = min(max(a.trk_first[v], 0), a.n_trk);
    hi = min(max(a.trk_first[v + 1], lo), a.n_trk);
}

__device__ __forceinline__ int64_t triangle(int64_t n) { return n * (n - 1) / 2; }
// entries of the row-major upper triangle of n tracklets in front of row i
__device__ __forceinline__ int64_t triangle_row(int64_t i, int64_t n) { return i * (2 * n - i - 1) / 2; }

__global__ __launch_bounds__(PROP_WAVES * 64) void proposal_clamp_kernel(vrd_proposal_args a) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * PROP_WAVES + (threadIdx.x >> 6);
    if (k >= a.n_trk) return;
    const Tracklet t = load_tracklet(a.trk, k);
    if (!track_inside(t.row, t.n, a.rows) || t.video < 0 || t.video >= a.n_videos) {      // a broken table touches no box
        if (lane == 0) a.trk_err[k] = 2;
        return;
    }
    const float x_max = a.video_max[2 * t.video], y_max = a.video_max[2 * t.video + 1];
    bool bad = false;
    for (int64_t r = lane; r < t.n; r += 64) {
        float* p = a.boxes + (t.row + r) * 4;
        float4 b = vrd::gload4(p);
        // (selects, not fmaxf / fminf: torch.clamp keeps a NaN, and the test below then reports it)
        b.x = b.x < 0.f ? 0.f : b.x;
        b.y = b.y < 0.f ? 0.f : b.y;
        b.z = b.z > x_max ? x_max : b.z;
        b.w = b.w > y_max ? y_max : b.w;
        bad |= !(b.z > b.x) || !(b.w > b.y);
        vrd::gstore4(p, b);
    }
    const bool any_bad = __any(bad) != 0;
    if (lane == 0) a.trk_err[k] = any_bad ? 1 : 0;
}

__global__ __launch_bounds__(PROP_WAVES * 64) void proposal_shadow_kernel(vrd_proposal_args a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * PROP_WAVES + (threadIdx.x >> 6);
    if (g >= a.n_tri) return;
    int v = 0, v_hi = a.n_videos;                                        // the last video whose triangle starts at or before g
    while (v_hi - v > 1) {
        const int mid = (v + v_hi) >> 1;
        if (a.tri_first[mid] <= g) v = mid; else v_hi = mid;
    }
    int t_lo, t_hi;
    video_tracklets(a, v, t_lo, t_hi);
    const int64_t n = t_hi - t_lo, k = g - a.tri_first[v];
    unsigned out = 0;
    if (n >= 2 && k >= 0 && k < triangle(n) && a.tri_first[v + 1] - a.tri_first[v] == triangle(n)) {
        // row i of entry k: the root of triangle_row(i) = k, then set right by whole numbers
        const double m = 2.0 * (double)n - 1.0;
        int64_t i = (int64_t)((m - sqrt(fmax(m * m - 8.0 * (double)k, 0.0))) * 0.5);
        i = min(max(i, (int64_t)0), n - 2);
        while (i > 0 && triangle_row(i, n) > k) --i;
        while (i < n - 2 && triangle_row(i + 1, n) <= k) ++i;
        const int64_t j = i + 1 + (k - triangle_row(i, n));
        const Tracklet ti = load_tracklet(a.trk, t_lo + i), tj = load_tracklet(a.trk, t_lo + j);
        if (ti.cat == tj.cat && track_inside(ti.row, ti.n, a.rows) && track_inside(tj.row, tj.n, a.rows)) {
            const int64_t i_end = ti.t0 + ti.n, j_end = tj.t0 + tj.n;
            const int64_t lo = max(ti.t0, tj.t0), hi = min(i_end, j_end);
            if (hi > lo) {
                double inter = 0.0, area_i = 0.0, area_j = 0.0;
                for (int64_t t = lo + lane; t < hi; t += 64) {
                    const float4 bi = vrd::gload4(a.boxes + (ti.row + t - ti.t0) * 4), bj = vrd::gload4(a.boxes + (tj.row + t - tj.t0) * 4);
                    const float w = fmaxf(fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x) + 1.0f, 0.0f);
                    const float h = fmaxf(fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y) + 1.0f, 0.0f);
                    inter = inter + (double)(w * h);
                    area_i = area_i + (double)((bi.z - bi.x + 1.0f) * (bi.w - bi.y + 1.0f));
                    area_j = area_j + (double)((bj.z - bj.x + 1.0f) * (bj.w - bj.y + 1.0f));
                }
                inter = wave_sum_f64(inter), area_i = wave_sum_f64(area_i), area_j = wave_sum_f64(area_j);
                if (inter / area_j > a.threshold && ti.t0 <= tj.t0 && i_end >= j_end) out |= 1u;
                if (inter / area_i > a.threshold && tj.t0 <= ti.t0 && j_end >= i_end) out |= 2u;
            }
        }
    }
    if (lane == 0) a.shadow[g] = (uint8_t)out;
}

// The reference loop (`for i: for j > i: ...`) with its three properties: a dropped i still examines its row; a dropped j is
// skipped for both rules; the mirrored rule drops i and ends row i.  A row only ever changes dropped[j] at the j it examines, so
// every j of a row sees the state from the row's start and the row may run in parallel: the wave finds the first live j whose
// byte says "j shadows i" without "i shadows j" (the `elif`), drops every live j in front of it that i shadows, then drops i.
// The dropped bytes live in global memory and belong to this wave alone; the barrier orders a row's stores before the next
// row's loads.
__global__ __launch_bounds__(64) void proposal_walk_kernel(vrd_proposal_args a) {
    const int lane = threadIdx.x;
    const int v = blockIdx.x;
    int t_lo, t_hi;
    video_tracklets(a, v, t_lo, t_hi);
    const int64_t n = t_hi - t_lo;
    bool bad = false;
    for (int k = t_lo + lane; k < t_hi; k += 64) {
        bad |= a.trk_err[k] != 0;
        a.dropped[k] = 0;
    }
    const bool any_bad = __any(bad) != 0;
    const int64_t tri0 = a.tri_first[v], tri1 = a.tri_first[v + 1];
    const bool tables_ok = n < 2 || (tri0 >= 0 && tri1 <= a.n_tri && tri1 - tri0 == triangle(n));
    if (lane == 0) a.video_err[v] = any_bad ? 1 : (tables_ok ? 0 : 2);
    __syncthreads();
    if (!tables_ok || n < 2) return;
    uint8_t* dropped = a.dropped + t_lo;
    int64_t row = tri0;                                                 // first byte of row i
    for (int64_t i = 0; i + 1 < n; ++i) {
        const int64_t m = n - 1 - i;                                    // the row's entries: j = i + 1 + x
        for (int64_t x0 = 0; x0 < m; x0 += 64) {
            const int64_t x = x0 + lane;
            const bool in = x < m;
            const unsigned f = in ? a.shadow[row + x] : 0u;
            const bool live = in && dropped[i + 1 + x] == 0;
            const unsigned long long stop = __ballot(live && (f & 2u) && !(f & 1u));
            const int first = stop ? __ffsll((long long)stop) - 1 : 64;
            if (live && (f & 1u) && lane < first) dropped[i + 1 + x] = 1;
            if (stop) {                                                 // (wave-uniform)
                if (lane == 0) dropped[i] = 1;
                break;
            }
        }
        row += m;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PAIR_THREADS) void proposal_pairs_kernel(vrd_proposal_args a) {
    __shared__ int wave_kept[PAIR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = blockIdx.x;
    int t_lo, t_hi;
    video_tracklets(a, v, t_lo, t_hi);
    const int64_t n = t_hi - t_lo;
    const int64_t c_lo = min(max(a.cand_first[v], (int64_t)0), a.n_cand), c_hi = min(max(a.cand_first[v + 1], c_lo), a.n_cand);
    const int64_t row0 = n > 0 ? a.trk[5 * (int64_t)t_lo] : 0;         // rows are counted from the video's own first row
    const int64_t offset = a.stride_offset[v], stride = a.feat_stride;
    int64_t base = 0;                                                   // kept so far (the same in every thread)
    for (int64_t c0 = c_lo; c0 < c_hi; c0 += PAIR_THREADS) {
        const int64_t c = c0 + tid;
        bool keep = false;
        int s = -1, o = -1, steps = 0;
        int64_t s_row = 0, o_row = 0;
        if (c < c_hi) {
            s = a.cand_s[c], o = a.cand_o[c];
            if (s >= 0 && s < n && o >= 0 && o < n && a.dropped[t_lo + s] == 0 && a.dropped[t_lo + o] == 0) {
                const Tracklet ts = load_tracklet(a.trk, t_lo + s), to = load_tracklet(a.trk, t_lo + o);
                const int64_t lo = max(ts.t0, to.t0), shared = min(ts.t0 + ts.n, to.t0 + to.n) - lo;
                const int64_t len = shared > offset ? (shared - offset + stride - 1) / stride : 0;      // len(range(offset, shared, stride))
                keep = shared >= a.min_frames && len >= 2 && len <= 0x7fffffff;
                steps = (int)len;
                s_row = ts.row - row0 + lo - ts.t0 + offset;
                o_row = to.row - row0 + lo - to.t0 + offset;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PAIR_THREADS / 64; ++w) {
            const int cnt = wave_kept[w];
            before += w < wave ? cnt : 0;
            total += cnt;
        }
        if (keep) {
            const int64_t at = c_lo + base + before + __popcll(mask & ((1ull << lane) - 1ull));
            a.s_row[at] = s_row, a.o_row[at] = o_row, a.lens[at] = steps, a.kept_s[at] = s, a.kept_o[at] = o;
        }
        base += total;
        __syncthreads();                                                // wave_kept is rewritten by the next step
    }
    for (int64_t c = c_lo + base + tid; c < c_hi; c += PAIR_THREADS)    // the rest of the slice: the same bytes at every call
        a.s_row[c] = 0, a.o_row[c] = 0, a.lens[c] = 0, a.kept_s[c] = -1, a.kept_o[c] = -1;
    if (tid == 0) a.count[v] = (int)base;
}

int check_args(const vrd_proposal_args* a, const char* what) {
    VRD_CHECK_ARG(a, "%s: null argument struct", what);
    VRD_CHECK_ARG(a->n_videos >= 0 && a->n_trk >= 0 && a->n_tri >= 0 && a->n_cand >= 0 && a->rows >= 0,
                  "%s: negative count (%d videos, %d tracklets, %lld tracklet pairs, %lld candidates, %lld box rows)", what, a->n_videos,
                  a->n_trk, (long long)a->n_tri, (long long)a->n_cand, (long long)a->rows);
    VRD_CHECK_ARG((a->trk_first && a->tri_first && a->cand_first && a->video_max && a->stride_offset && a->count && a->video_err) ||
                  a->n_videos == 0, "%s: null per-video table", what);
    VRD_CHECK_ARG((a->trk && a->trk_err && a->dropped) || a->n_trk == 0, "%s: null tracklet table", what);
    VRD_CHECK_ARG(a->shadow || a->n_tri == 0, "%s: null tracklet-pair scratch", what);
    VRD_CHECK_ARG((a->cand_s && a->cand_o && a->s_row && a->o_row && a->lens && a->kept_s && a->kept_o) || a->n_cand == 0,
                  "%s: null candidate table", what);
    VRD_CHECK_ARG(a->boxes || a->rows == 0, "%s: null box array", what);
    VRD_CHECK_ARG((uintptr_t)a->boxes % 16 == 0, "%s: the box array must be 16-byte aligned", what);
    VRD_CHECK_ARG(a->feat_stride >= 1, "%s: feat_stride %d < 1", what, a->feat_stride);
    VRD_CHECK_ARG(a->threshold == a->threshold, "%s: the threshold is not a number", what);
    return 0;
}

// workgroups of PROP_WAVES waves for `waves` waves, or -1 when the grid has no room for them
int64_t wave_blocks(int64_t waves) {
    const int64_t blocks = (waves + PROP_WAVES - 1) / PROP_WAVES;
    return blocks <= 0x7fffffff ? blocks : -1;
}

}  // namespace

extern "C" int vrd_proposal_clamp(const vrd_proposal_args* a, void* stream) {
    if (int rc = check_args(a, "vrd_proposal_clamp")) return rc;
    if (a->n_trk == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(proposal_clamp_kernel, dim3((unsigned)wave_blocks(a->n_trk)), dim3(PROP_WAVES * 64), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vrd_proposal_shadow(const vrd_proposal_args* a, void* stream) {
    if (int rc = check_args(a, "vrd_proposal_shadow")) return rc;
    if (a->n_tri == 0 || a->n_videos == 0) return 0;
    const int64_t blocks = wave_blocks(a->n_tri);
    VRD_CHECK_ARG(blocks > 0, "vrd_proposal_shadow: %lld tracklet pairs are more than one launch takes: split the call", (long long)a->n_tri);
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(proposal_shadow_kernel, dim3((unsigned)blocks), dim3(PROP_WAVES * 64), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vrd_proposal_walk(const vrd_proposal_args* a, void* stream) {
    if (int rc = check_args(a, "vrd_proposal_walk")) return rc;
    if (a->n_videos == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(proposal_walk_kernel, dim3((unsigned)a->n_videos), dim3(64), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vrd_proposal_pairs(const vrd_proposal_args* a, void* stream) {
    if (int rc = check_args(a, "vrd_proposal_pairs")) return rc;
    if (a->n_videos == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(proposal_pairs_kernel, dim3((unsigned)a->n_videos), dim3(PAIR_THREADS), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}
