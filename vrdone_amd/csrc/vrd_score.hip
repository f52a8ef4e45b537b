// Relation scoring on the device (vrdone_amd/evaluate.py, the scoring VidVRD-helper's visual_relation_detection.py does on the
// host): the trajectory vIoU of (prediction, ground truth) candidates and the greedy matching of eval_detection_scores.
//
// relation_viou_kernel: one wave per candidate.  A track is `frames` consecutive rows of a flat (rows, 4) f32 box array; the
// lanes stride over frames, every difference, product and sum is formed in f64 with separately rounded operations (no fused
// multiply-add: evaluate.viou rounds the product before it adds), and a butterfly over the 64 lanes in a fixed order finishes
// each sum, so a repeat gives the same bits.  Quarter-pixel boxes below 2048 make every value exact, whatever the order.
//
// match_relations_kernel: one wave per video, walking the video's predictions in their scoring order.  The lanes stride over
// the prediction's candidates, the wave agrees on the best one (largest ov, ties to the lower ground-truth index -- the host
// loop's strict `>` over ascending ground truths), lane 0 marks it.  The detected flags are bytes in global memory that only
// this wave touches; a workgroup barrier orders lane 0's store before the next prediction's loads (one vector L1 per CU).
#include "vrd_common.h"

// every f64 operation below is rounded on its own, as numpy's are: a fused multiply-add would keep the product unrounded
#pragma clang fp contract(off)

namespace {

constexpr int VIOU_WAVES = 4;                // candidates per workgroup

// butterfly sum over the 64 lanes: every lane ends with the same value, formed in the same order at every call
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double box_area(float4 b) {
    return ((double)b.z - (double)b.x + 1.0) * ((double)b.w - (double)b.y + 1.0);
}

// sum over the frames of a track of (x1 - x0 + 1) * (y1 - y0 + 1), this lane's share
__device__ __forceinline__ double track_volume(const float* boxes, int64_t row, int64_t frames, int lane) {
    double acc = 0.0;
    for (int64_t t = lane; t < frames; t += 64) acc = acc + box_area(vrd::gload4(boxes + (row + t) * 4));
    return acc;
}

// this lane's share of the intersection volume over the shared frames [lo, hi) of track a (first frame a0) and b (first frame b0)
__device__ __forceinline__ double track_overlap(const float* boxes_a, int64_t row_a, int64_t a0, const float* boxes_b, int64_t row_b,
                                                int64_t b0, int64_t lo, int64_t hi, int lane) {
    double acc = 0.0;
    for (int64_t t = lo + lane; t < hi; t += 64) {
        const float4 a = vrd::gload4(boxes_a + (row_a + t - a0) * 4), b = vrd::gload4(boxes_b + (row_b + t - b0) * 4);
        const double w = (double)fminf(a.z, b.z) - (double)fmaxf(a.x, b.x) + 1.0;
        const double h = (double)fminf(a.w, b.w) - (double)fmaxf(a.y, b.y) + 1.0;
        acc = acc + fmax(w, 0.0) * fmax(h, 0.0);
    }
    return acc;
}

__device__ __forceinline__ bool track_inside(int64_t row, int64_t frames, int64_t rows) {
    return row >= 0 && frames >= 0 && row <= rows && frames <= rows - row;
}

__global__ __launch_bounds__(VIOU_WAVES * 64) void relation_viou_kernel(vrd_viou_args a) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * VIOU_WAVES + (threadIdx.x >> 6);
    if (c >= a.n_cand) return;
    const int p = a.cand[2 * c], g = a.cand[2 * c + 1];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (p < 0 || p >= a.n_pred || g < 0 || g >= a.n_gt) {                 // a broken table reads nothing and shows in the output
        if (lane == 0) a.ov[c] = nan;
        return;
    }
    const int64_t* pr = a.pred + 4 * (int64_t)p;
    const int64_t* gr = a.gt + 4 * (int64_t)g;
    const int64_t p0 = pr[2], pn = pr[3], g0 = gr[2], gn = gr[3];
    if (!track_inside(pr[0], pn, a.pred_rows) || !track_inside(pr[1], pn, a.pred_rows) || !track_inside(gr[0], gn, a.gt_rows) ||
        !track_inside(gr[1], gn, a.gt_rows)) {
        if (lane == 0) a.ov[c] = nan;
        return;
    }
    const int64_t lo = max(p0, g0), hi = min(p0 + pn, g0 + gn);
    double ov = 0.0;
    if (hi > lo) {
#pragma unroll
        for (int role = 0; role < 2; ++role) {                            // subject, object
            const double overlap = wave_sum_f64(track_overlap(a.pred_boxes, pr[role], p0, a.gt_boxes, gr[role], g0, lo, hi, lane));
            const double vol_p = wave_sum_f64(track_volume(a.pred_boxes, pr[role], pn, lane));
            const double vol_g = wave_sum_f64(track_volume(a.gt_boxes, gr[role], gn, lane));
            const double v = overlap / (vol_p + vol_g - overlap);
            ov = role == 0 ? v : (v < ov ? v : ov);                       // Python's min(subject, object)
        }
    }
    if (lane == 0) a.ov[c] = ov;
}

__global__ __launch_bounds__(64) void match_relations_kernel(vrd_match_args a) {
    const int lane = threadIdx.x;
    const int v = blockIdx.x;
    // (offsets clamped to the tables: a broken table reads nothing outside them)
    const int p_lo = max(a.pred_first[v], 0), p_hi = min(a.pred_first[v + 1], a.n_pred);
    if (p_hi <= p_lo) return;
    // this video's flags: the ground truths its candidates name
    const int c_lo = max(a.cand_first[p_lo], 0), c_hi = min(a.cand_first[p_hi], a.n_cand);
    for (int c = c_lo + lane; c < c_hi; c += 64) {
        const int g = a.cand[2 * c + 1];
        if (g >= 0 && g < a.n_gt) a.detected[g] = 0;
    }
    __syncthreads();
    const double none = -__longlong_as_double(0x7ff0000000000000ll);      // -inf
    for (int p = p_lo; p < p_hi; ++p) {
        const int c0 = max(a.cand_first[p], 0), c1 = min(a.cand_first[p + 1], a.n_cand);
        double best = none;
        int best_g = -1;
        for (int c = c0 + lane; c < c1; c += 64) {
            const int g = a.cand[2 * c + 1];
            if (g < 0 || g >= a.n_gt || a.detected[g]) continue;
            const double ov = a.ov[c];
            if (ov >= a.threshold && (ov > best || (ov == best && g < best_g))) best = ov, best_g = g;
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const double o_best = __shfl_xor(best, m, 64);
            const int o_g = __shfl_xor(best_g, m, 64);
            if (o_g >= 0 && (best_g < 0 || o_best > best || (o_best == best && o_g < best_g))) best = o_best, best_g = o_g;
        }
        if (lane == 0) {
            a.hit[p] = best_g;
            if (best_g >= 0) a.detected[best_g] = 1;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int vrd_relation_viou(const vrd_viou_args* a, void* stream) {
    VRD_CHECK_ARG(a, "vrd_relation_viou: null argument struct");
    VRD_CHECK_ARG(a->n_pred >= 0 && a->n_gt >= 0 && a->n_cand >= 0 && a->pred_rows >= 0 && a->gt_rows >= 0,
                  "vrd_relation_viou: negative count (%d predictions, %d ground truths, %d candidates, %lld / %lld box rows)", a->n_pred,
                  a->n_gt, a->n_cand, (long long)a->pred_rows, (long long)a->gt_rows);
    VRD_CHECK_ARG((a->pred || a->n_pred == 0) && (a->gt || a->n_gt == 0) && ((a->cand && a->ov) || a->n_cand == 0) &&
                  (a->pred_boxes || a->pred_rows == 0) && (a->gt_boxes || a->gt_rows == 0),
                  "vrd_relation_viou: null table with a non-zero count");
    VRD_CHECK_ARG(((uintptr_t)a->pred_boxes | (uintptr_t)a->gt_boxes) % 16 == 0, "vrd_relation_viou: box arrays must be 16-byte aligned");
    if (a->n_cand == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(relation_viou_kernel, dim3((unsigned)((a->n_cand + VIOU_WAVES - 1) / VIOU_WAVES)), dim3(VIOU_WAVES * 64), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vrd_match_relations(const vrd_match_args* a, void* stream) {
    VRD_CHECK_ARG(a, "vrd_match_relations: null argument struct");
    VRD_CHECK_ARG(a->n_videos >= 0 && a->n_pred >= 0 && a->n_cand >= 0 && a->n_gt >= 0,
                  "vrd_match_relations: negative count (%d videos, %d predictions, %d candidates, %d ground truths)", a->n_videos,
                  a->n_pred, a->n_cand, a->n_gt);
    VRD_CHECK_ARG((a->pred_first || a->n_videos == 0) && ((a->cand_first && a->hit) || a->n_pred == 0) &&
                  ((a->cand && a->ov) || a->n_cand == 0) && (a->detected || a->n_gt == 0),
                  "vrd_match_relations: null table with a non-zero count");
    VRD_CHECK_ARG(a->threshold == a->threshold, "vrd_match_relations: the threshold is not a number");
    if (a->n_videos == 0 || a->n_pred == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_POSTPROC, s, 0.0, 0.0);
    hipLaunchKernelGGL(match_relations_kernel, dim3((unsigned)a->n_videos), dim3(64), 0, s, *a);
    VRD_LAUNCH_CHECK();
    return 0;
}
