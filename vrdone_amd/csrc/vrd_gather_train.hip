// Training batches built on the device (vrd_gather_train): the counterpart of vrd_gather_pairs for the reference's training
// dataloader (`_train_getitem`, dataloaders/vidvrd.py:324-457).  A video's ground-truth trajectories live on the device once --
// vis (sum L, V), clip, boxes (sum L, 4, clamped) --; the host decides which relation keys survive, their sub-sampling offset
// and their crop (proposals.train_tables: index arithmetic only) and one launch writes
//   (a) the backbone's channels-last operand buffers at max_seq_len, zero rows behind each sequence, and its validity mask;
//   (b) the 0/1 target masks of all relations.
// The kernel is pure HBM streaming: the wide rows (2 x V (+ 2 x Cc) floats per frame) are copied with 16-byte loads and stores,
// one workgroup per (sequence, GT_FRAMES frames), a wave per frame, the subject's and the object's loads of a frame in flight
// together; no LDS, no atomics (but the f16 range flag).  Rows that are float4-shaped but not 16-byte aligned are read as
// four scalar loads (ROWS_UNALIGNED; the ldv4<false> convention of vrd_colsum.hip); widths that are no multiple of 4 take the
// scalar form throughout.
#include "vrd_common.h"
#include "vrd_box_feats.h"

namespace {

constexpr int GT_FRAMES = 8;
enum RowMode { ROWS_SCALAR = 0, ROWS_UNALIGNED = 1, ROWS_ALIGNED = 2 };

using vrd::aligned16;

template <bool A16>
__device__ __forceinline__ float4 ldv4(const float* p) {
    if (A16) return vrd::gload4(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// the subject's and the object's row of one frame: src_* -> dst_* (`width` floats each; zeros when !live)
template <int MODE>
__device__ __forceinline__ void copy_rows(const float* src_s, const float* src_o, bool live, float* dst_s, float* dst_o, int width,
                                          int lane, int pair, vrd::RangeTrack* rt) {
    if (MODE == ROWS_SCALAR) {
        for (int c = lane; c < width; c += 64) {
            const float vs = live ? src_s[c] : 0.f, vo = live ? src_o[c] : 0.f;
            if (pair) vrd::store_pair1(dst_s, c, width, vs, pair, rt), vrd::store_pair1(dst_o, c, width, vo, pair, rt);
            else dst_s[c] = vs, dst_o[c] = vo;
        }
        return;
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const int n4 = width >> 2;
    for (int c0 = lane; c0 < n4; c0 += 256) {           // four float4 per lane and side in flight
        float4 vs[4], vo[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 64 * u;
            const bool ok = live && c < n4;
            vs[u] = ok ? ldv4<MODE == ROWS_ALIGNED>(src_s + 4 * c) : zero;
            vo[u] = ok ? ldv4<MODE == ROWS_ALIGNED>(src_o + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 64 * u;
            if (c >= n4) break;
            if (pair) {
                vrd::store_pair4(dst_s, 4 * c, width, vs[u], pair, rt);
                vrd::store_pair4(dst_o, 4 * c, width, vo[u], pair, rt);
            } else {
                vrd::gstore4(dst_s + 4 * c, vs[u]);
                vrd::gstore4(dst_o + 4 * c, vo[u]);
            }
        }
    }
}

// grid: x = block of GT_FRAMES frames, y = sequence p < P; the rows y >= P of the grid write the target masks
template <int MODE, bool BOX16>
__global__ __launch_bounds__(256) void gather_train_kernel(vrd_gather_train_args a, unsigned* rflag) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.y >= a.P) {           // (b) targets[g, t] = seg_lo[g] <= t < seg_hi[g]
        const int64_t i = ((int64_t)(blockIdx.y - a.P) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (i < (int64_t)a.G * a.T) {
            const int g = (int)(i / a.T), t = (int)(i - (int64_t)g * a.T);
            a.out_targets[i] = (t >= a.seg_lo[g] && t < a.seg_hi[g]) ? 1.f : 0.f;
        }
        return;
    }
    vrd::RangeTrack rt;
    const int p = blockIdx.y;
    const int n = a.lens[p];
    const int64_t s0 = a.s_row[p], o0 = a.o_row[p];
    const int64_t half = (int64_t)a.P * a.T;
    for (int k = wave; k < GT_FRAMES; k += 4) {
        const int t = blockIdx.x * GT_FRAMES + k;
        if (t >= a.T) break;
        const bool live = t < n;
        const int64_t row = (int64_t)p * a.T + t;
        const int64_t rs = live ? s0 + (int64_t)t * a.stride : 0, ro = live ? o0 + (int64_t)t * a.stride : 0;
        copy_rows<MODE>(a.vis + rs * a.V, a.vis + ro * a.V, live, a.out_vis + row * a.V, a.out_vis + (half + row) * a.V, a.V, lane,
                        a.pair_wide, &rt);
        if (a.Cc)
            copy_rows<MODE>(a.clip + rs * a.Cc, a.clip + ro * a.Cc, live, a.out_clip + row * a.Cc, a.out_clip + (half + row) * a.Cc,
                            a.Cc, lane, a.pair_wide, &rt);
        // box features: lanes 0 (subject-object), 1 (subject), 2 (object) compute, everybody stores zeros for padded frames
        float* const so = a.out_so_box + row * 5;
        float* const es = a.out_ent + row * 8;
        float* const eo = a.out_ent + (half + row) * 8;
        if (lane == 0) a.out_mask[row] = live ? 1 : 0;
        if (!live) {
            if (lane < 5) so[lane] = 0.f;
            if (lane < 8) es[lane] = 0.f, eo[lane] = 0.f;
            continue;
        }
        if (lane == 0) {
            float f[5];
            vrd::so_box_feats(vrd::load_box<BOX16>(a.boxes, rs), vrd::load_box<BOX16>(a.boxes, ro), f);
#pragma unroll
            for (int i = 0; i < 5; ++i) so[i] = f[i];
        } else if (lane == 1 || lane == 2) {
            // The reference differentiates the boxes along the sub-sampled frames BEFORE it crops (dataloaders/vidvrd.py:405-431):
            // frame 0 of a sequence whose crop starts at a later frame (lead > 0) takes the ordinary difference to the frame in
            // front of it, not the extrapolated one -- the same frame t + 1 of the sequence that starts one step earlier
            const int back = a.lead[p] > 0 ? 1 : 0;
            float f[8];
            vrd::entity_feats<BOX16>(a.boxes, (lane == 1 ? s0 : o0) - (int64_t)back * a.stride, a.stride, t + back, n + back,
                                     a.seq_wh[2 * (int64_t)p], a.seq_wh[2 * (int64_t)p + 1], f);
            float* const dst = lane == 1 ? es : eo;
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i] = f[i];
        }
    }
    rt.report(rflag, vrd::RANGE_INPUT);
}

}  // namespace

extern "C" int vrd_gather_train(const vrd_gather_train_args* a, void* stream) {
    VRD_CHECK_ARG(a && a->vis && a->boxes && a->s_row && a->o_row && a->lens && a->lead && a->seq_wh && a->out_vis && a->out_so_box &&
                      a->out_ent && a->out_mask,
                  "vrd_gather_train: null pointer");
    VRD_CHECK_ARG(a->P > 0 && a->T > 0 && a->V > 0 && a->Cc >= 0 && a->G >= 0 && a->stride >= 1, "vrd_gather_train: bad sizes");
    VRD_CHECK_ARG(a->Cc == 0 || (a->clip && a->out_clip), "vrd_gather_train: clip buffers missing");
    VRD_CHECK_ARG(a->G == 0 || (a->seg_lo && a->seg_hi && a->out_targets), "vrd_gather_train: target tables missing");
    VRD_CHECK_ARG(a->pair_wide == VRD_PAIR_NONE || a->pair_wide == VRD_PAIR_BF16 || a->pair_wide == VRD_PAIR_F16,
                  "vrd_gather_train: unknown pair format %d", a->pair_wide);
    VRD_CHECK_ARG(!a->pair_wide || (a->V % 32 == 0 && a->Cc % 32 == 0), "vrd_gather_train: pair rows need widths %% 32 == 0");
    const bool shaped = a->V % 4 == 0 && a->Cc % 4 == 0;
    VRD_CHECK_ARG(!shaped || (aligned16(a->out_vis) && (!a->Cc || aligned16(a->out_clip))),
                  "vrd_gather_train: the output buffers must be 16-byte aligned");
    const int64_t fblocks = (a->T + GT_FRAMES - 1) / GT_FRAMES;
    const int64_t tblocks = ((int64_t)a->G * a->T + 255) / 256;
    const int64_t ty = (tblocks + fblocks - 1) / fblocks;
    VRD_CHECK_ARG(a->P + ty <= 65535, "vrd_gather_train: too many sequences (%d) / relations (%d) for one launch", a->P, a->G);
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_TRANSPOSE, s, 0.0,
                        8.0 * (2.0 * a->V + 2.0 * a->Cc + 21.0) * a->P * a->T + 4.0 * a->G * a->T);
    const dim3 grid((unsigned)fblocks, (unsigned)(a->P + ty)), block(256);
    unsigned* rflag = a->pair_wide == VRD_PAIR_F16 ? vrd::range_flag() : nullptr;
    const int mode = !shaped ? ROWS_SCALAR : (aligned16(a->vis) && (!a->Cc || aligned16(a->clip))) ? ROWS_ALIGNED : ROWS_UNALIGNED;
    const bool box16 = aligned16(a->boxes);
#define VRD_GT_LAUNCH(M)                                                                          \
    do {                                                                                          \
        if (box16) hipLaunchKernelGGL((gather_train_kernel<M, true>), grid, block, 0, s, *a, rflag);  \
        else hipLaunchKernelGGL((gather_train_kernel<M, false>), grid, block, 0, s, *a, rflag);       \
    } while (0)
    if (mode == ROWS_ALIGNED) VRD_GT_LAUNCH(ROWS_ALIGNED);
    else if (mode == ROWS_UNALIGNED) VRD_GT_LAUNCH(ROWS_UNALIGNED);
    else VRD_GT_LAUNCH(ROWS_SCALAR);
#undef VRD_GT_LAUNCH
    VRD_LAUNCH_CHECK();
    return 0;
}
