// Banded (local-window) attention of the stem / branch blocks, forward: the strip kernels and the entry points.  (The per-row
// kernel local_attn_kernel: vrd_local_attn_row.hip; training forward with attn_drop and the backward: vrd_local_attn_bwd.hip; the
// envelope of shapes and the dispatch helpers: vrd_local_attn.h.)
//
//  * local_attn_strip_kernel / local_attn_kernel
//                        O(T*w) work and HBM-bound: one wavefront per strip of 16 query rows (K / V window rows in a
//                        register ring) or per query row, covering all heads; window scores in
//                        registers, head-wise dot products reduced over the 8 or 16 lanes of a head.
//                        Any odd window from 3 to 19.  C = 512 (8 channels a lane): above window 9
//                        local_attn_strip_half_kernel, two waves per strip, 4 channels a lane.  C = 256: that kernel
//                        with one wave per strip (4 channels a lane are the whole row) at every window.
//                        head_dim 32, 64 or 128: 4 ... 32 lanes per head.
#include "vrd_local_attn.h"
#include <cmath>
#include <cstdlib>

namespace {

using vrd::aligned16;
using vrd::ld4;
using vrd::st4;
using vrd::dot4;

// ------------------------------------------------------------------------------------------
// banded attention.  C = 512: lane l owns channels [8l, 8l+8); GROUP = head_dim / 8 lanes per head (4, 8 or 16).
// C = 256: lane l owns channels [4l, 4l+4); GROUP = head_dim / 4 (8, 16 or 32) -- the row addressing stays wave-uniform
// ------------------------------------------------------------------------------------------
// REL: the learnable per-(head, window slot) bias `rel_pe` (n_head x W) is added to the scaled scores before the key mask
// (blocks.py:957-958); a separate instantiation, so that the default path carries no extra instruction

// Strip variant of the banded attention: one wave walks RW consecutive query rows of one sequence and keeps the K and V
// rows of the moving window in registers (a ring of W + 1 slots, the row entering the window next already requested),
// so every K / V row is read W + 1 -> (RW + W - 1) / RW times from the L1 instead of W times.  The ring is indexed with
// compile-time slots: the row loop runs in rounds of R = W + 1 unrolled phases.
template <int W, int GROUP, int RW, bool REL>
__global__ __launch_bounds__(256) void local_attn_strip_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                               const float* __restrict__ v, int64_t ld,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ rel,
                                                               int B, int T_u, int strips_per_seq,
                                                               float scale, float* __restrict__ out, int64_t ldo, int pair,
                                                               unsigned* rflag, vrd::SegTable sg) {
    constexpr int HW = W / 2, R = W + 1;
    vrd::RangeTrack rt;
    const int lane = threadIdx.x & 63;
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, qq = nwg >> 3, rem = nwg & 7;
    const int lid = (xcd < rem ? xcd * (qq + 1) : rem * (qq + 1) + (xcd - rem) * qq) + (bid >> 3);
    const int64_t ws = (int64_t)lid * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int T, t0;
    int64_t row_b;
    if (sg.count) {                                  // ragged row space: groups of sequences of different lengths
        int g, b, strip;
        if (!vrd::seg_find(sg, ws, g, b, strip)) return;
        T = sg.T[g], t0 = strip * RW, row_b = sg.row[g] + (int64_t)b * T;
    } else {
        const int b = (int)(ws / strips_per_seq);
        if (b >= B) return;
        T = T_u, t0 = (int)(ws - (int64_t)b * strips_per_seq) * RW, row_b = (int64_t)b * T;
    }
    const int t1 = min(t0 + RW, T);
    // validity of rows t0 - HW .. t0 + RW + HW - 1 as one bit each (bit i = row t0 - HW + i; outside [0, T) = 0)
    const int tm = t0 - HW + lane;
    const unsigned long long live = __ballot(lane < RW + 2 * HW && tm >= 0 && tm < T && mask[row_b + (tm >= 0 && tm < T ? tm : 0)] != 0);
    if (((live >> HW) & ((1ull << (t1 - t0)) - 1ull)) == 0ull) {      // every query row of the strip is padding
        for (int t = t0; t < t1; ++t) {
            float* o = out + (row_b + t) * ldo + lane * 8;
            st4(o, make_float4(0.f, 0.f, 0.f, 0.f));
            st4(o + 4, make_float4(0.f, 0.f, 0.f, 0.f));
        }
        return;
    }
    struct Row {
        float4 a, b;
    };
    auto load_row = [&](const float* base, int t) {
        Row r;
        r.a = r.b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < T) {
            const float* p = base + (row_b + t) * ld + lane * 8;
            r.a = ld4(p), r.b = ld4(p + 4);
        }
        return r;
    };
    float rb[W];
#pragma unroll
    for (int j = 0; j < W; ++j) rb[j] = REL ? rel[(lane / GROUP) * W + j] : 0.f;
    Row kr[R], vr[R];
#pragma unroll
    for (int i = 0; i < W; ++i) {          // window of the first query row: rows t0 - HW .. t0 + HW in slots 0 .. W-1
        kr[i] = load_row(k, t0 - HW + i);
        vr[i] = load_row(v, t0 - HW + i);
    }
    for (int base = 0; base < RW; base += R) {
#pragma unroll
        for (int ph = 0; ph < R; ++ph) {
            const int t = t0 + base + ph;
            if (t >= t1) break;
            // the row that enters the window with the next query row goes into the slot the window does not cover
            kr[(ph + W) % R] = load_row(k, t + HW + 1);
            vr[(ph + W) % R] = load_row(v, t + HW + 1);
            float* o = out + (row_b + t) * ldo + lane * 8;
            const int bit0 = base + ph;                       // bit of window row j is bit0 + j (row t - HW + j)
            if (!((live >> (bit0 + HW)) & 1ull)) {            // masked query rows are zeroed after the softmax
                st4(o, make_float4(0.f, 0.f, 0.f, 0.f));
                st4(o + 4, make_float4(0.f, 0.f, 0.f, 0.f));
                continue;
            }
            float4 q0 = ld4(q + (row_b + t) * ld + lane * 8), q1 = ld4(q + (row_b + t) * ld + lane * 8 + 4);
            q0.x *= scale; q0.y *= scale; q0.z *= scale; q0.w *= scale;
            q1.x *= scale; q1.y *= scale; q1.z *= scale; q1.w *= scale;
            float sc[W];
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int tj = t + j - HW;
                if (tj < 0 || tj >= T) { sc[j] = -INFINITY; continue; }
                const Row& kk = kr[(ph + j) % R];
                float d = dot4(q0, kk.a) + dot4(q1, kk.b);
                d = vrd::group_sum<GROUP>(d);
                if (REL) d += rb[j];
                sc[j] = d + (((live >> (bit0 + j)) & 1ull) ? 0.f : -1e4f);
                m = fmaxf(m, sc[j]);
            }
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < W; ++j) { sc[j] = __expf(sc[j] - m); den += sc[j]; }
            const float inv = 1.0f / den;
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int tj = t + j - HW;
                if (tj < 0 || tj >= T) continue;
                const Row& vv = vr[(ph + j) % R];
                const float pj = sc[j] * inv;
                a0.x += pj * vv.a.x; a0.y += pj * vv.a.y; a0.z += pj * vv.a.z; a0.w += pj * vv.a.w;
                a1.x += pj * vv.b.x; a1.y += pj * vv.b.y; a1.z += pj * vv.b.z; a1.w += pj * vv.b.w;
            }
            if (pair) {
                vrd::store_pair4(out + (row_b + t) * ldo, lane * 8, 512, a0, pair, &rt);
                vrd::store_pair4(out + (row_b + t) * ldo, lane * 8 + 4, 512, a1, pair, &rt);
            } else {
                st4(o, a0);
                st4(o + 4, a1);
            }
        }
    }
    rt.report(rflag, vrd::RANGE_ATTN_OUT);
}

// Half-row strip variant for the windows above 9.  The ring of the kernel above costs 16 (W + 1) VGPRs -- 320 at W = 19,
// more than a wave has -- and its W + 1 unrolled phases of W window slots each outgrow what the compiler will unroll (the
// ring then lands in scratch).  So here two waves share a strip: wave `half` owns channels [256 half, 256 half + 256),
// lane l four of them, which halves the registers of a row; and the row loop runs in rounds of U = 2 unrolled phases over
// W + U slots (phase p: window in slots p .. p + W - 1, the row entering next goes to slot p + W), after which the W live
// rows move down U slots: W register moves per two query rows.  Heads never straddle the two halves (head_dim 64 or
// 128, or 32 with 16 heads), so the waves do not talk to each other; GROUP = head_dim / 4 lanes per head.
// HALVES = 1 is the same kernel at C = 256: one wave per strip, its 64 lanes x 4 channels being the whole row, and there
// for every window (a row costs the ring half the registers it costs at C = 512, so no window needs a second form).
template <int W, int GROUP, int RW, bool REL, int HALVES = 2>
__global__ __launch_bounds__(256) void local_attn_strip_half_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                    const float* __restrict__ v, int64_t ld,
                                                                    const uint8_t* __restrict__ mask, const float* __restrict__ rel,
                                                                    int B, int T_u, int strips_per_seq,
                                                                    float scale, float* __restrict__ out, int64_t ldo, int pair,
                                                                    unsigned* rflag, vrd::SegTable sg) {
    static_assert(GROUP == 8 || GROUP == 16 || GROUP == 32, "lanes per head at four channels a lane");
    static_assert(HALVES == 1 || HALVES == 2, "C = 256 or 512");
    static_assert(RW + 2 * (W / 2) <= 64, "one validity bit per row of the strip and its halo");
    constexpr int HW = W / 2, U = 2;
    static_assert(RW % U == 0, "whole rounds");
    vrd::RangeTrack rt;
    const int lane = threadIdx.x & 63;
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, qq = nwg >> 3, rem = nwg & 7;
    const int lid = (xcd < rem ? xcd * (qq + 1) : rem * (qq + 1) + (xcd - rem) * qq) + (bid >> 3);
    const int64_t wv = (int64_t)lid * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ws = HALVES == 2 ? wv >> 1 : wv;    // strip; at HALVES = 2 its two waves sit in one workgroup
    const int half = HALVES == 2 ? (int)(wv & 1) : 0;
    const int c0 = half * 256 + lane * 4;             // first channel of this lane
    int T, t0;
    int64_t row_b;
    if (sg.count) {
        int g, b, strip;
        if (!vrd::seg_find(sg, ws, g, b, strip)) return;
        T = sg.T[g], t0 = strip * RW, row_b = sg.row[g] + (int64_t)b * T;
    } else {
        const int b = (int)(ws / strips_per_seq);
        if (b >= B) return;
        T = T_u, t0 = (int)(ws - (int64_t)b * strips_per_seq) * RW, row_b = (int64_t)b * T;
    }
    const int t1 = min(t0 + RW, T);
    // validity of rows t0 - HW .. t0 + RW + HW - 1 as one bit each (bit i = row t0 - HW + i; outside [0, T) = 0)
    const int tm = t0 - HW + lane;
    const unsigned long long live = __ballot(lane < RW + 2 * HW && tm >= 0 && tm < T && mask[row_b + (tm >= 0 && tm < T ? tm : 0)] != 0);
    if (((live >> HW) & ((1ull << (t1 - t0)) - 1ull)) == 0ull) {      // every query row of the strip is padding
        for (int t = t0; t < t1; ++t) st4(out + (row_b + t) * ldo + c0, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    auto load_row = [&](const float* base, int t) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < T) r = ld4(base + (row_b + t) * ld + c0);
        return r;
    };
    float rb[W];
#pragma unroll
    for (int j = 0; j < W; ++j) rb[j] = REL ? rel[((half * 64 + lane) / GROUP) * W + j] : 0.f;
    float4 kr[W + U], vr[W + U];
#pragma unroll
    for (int i = 0; i < W; ++i) {          // window of the first query row: rows t0 - HW .. t0 + HW in slots 0 .. W-1
        kr[i] = load_row(k, t0 - HW + i);
        vr[i] = load_row(v, t0 - HW + i);
    }
    for (int base = 0; t0 + base < t1; base += U) {
        if (base) {
#pragma unroll
            for (int i = 0; i < W; ++i) kr[i] = kr[i + U], vr[i] = vr[i + U];
        }
#pragma unroll
        for (int ph = 0; ph < U; ++ph) {
            const int t = t0 + base + ph;
            if (t >= t1) break;
            kr[ph + W] = load_row(k, t + HW + 1);
            vr[ph + W] = load_row(v, t + HW + 1);
            float* o = out + (row_b + t) * ldo + c0;
            const int bit0 = base + ph;                       // bit of window row j is bit0 + j (row t - HW + j)
            if (!((live >> (bit0 + HW)) & 1ull)) {            // masked query rows are zeroed after the softmax
                st4(o, make_float4(0.f, 0.f, 0.f, 0.f));
                continue;
            }
            float4 q0 = ld4(q + (row_b + t) * ld + c0);
            q0.x *= scale; q0.y *= scale; q0.z *= scale; q0.w *= scale;
            float sc[W];
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int tj = t + j - HW;
                if (tj < 0 || tj >= T) { sc[j] = -INFINITY; continue; }
                float d = dot4(q0, kr[ph + j]);
                d = vrd::group_sum<GROUP>(d);
                if (REL) d += rb[j];
                sc[j] = d + (((live >> (bit0 + j)) & 1ull) ? 0.f : -1e4f);
                m = fmaxf(m, sc[j]);
            }
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < W; ++j) { sc[j] = __expf(sc[j] - m); den += sc[j]; }
            const float inv = 1.0f / den;
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int tj = t + j - HW;
                if (tj < 0 || tj >= T) continue;
                const float4 vv = vr[ph + j];
                const float pj = sc[j] * inv;
                a0.x += pj * vv.x; a0.y += pj * vv.y; a0.z += pj * vv.z; a0.w += pj * vv.w;
            }
            if (pair)
                vrd::store_pair4(out + (row_b + t) * ldo, c0, HALVES * 256, a0, pair, &rt);
            else
                st4(o, a0);
        }
    }
    rt.report(rflag, vrd::RANGE_ATTN_OUT);
}

// uniform (B, T) or, segs != NULL, the row groups of a ragged row space; both entry points report as vrd_local_attn
int local_attn_launch(const float* q, const float* k, const float* v, int64_t ld, const uint8_t* mask, const float* rel_pe,
                      int B, int T, const vrd_row_segs* segs, int C, int n_head, int half_win, float* out, int64_t ldo,
                      int out_pair, void* stream) {
    VRD_CHECK_ARG(q && k && v && mask && out, "vrd_local_attn: null pointer");
    vrd::LaShape sh;
    if (int rc = vrd::la_shape("vrd_local_attn", C, n_head, half_win, &sh)) return rc;
    VRD_CHECK_ARG(ld >= C && ldo >= C && ld % 4 == 0 && ldo % 4 == 0 && aligned16(q) && aligned16(k) &&
                      aligned16(v) && aligned16(out), "vrd_local_attn: bad layout");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::SegTable sg;
    sg.count = 0;
    int64_t rows = (int64_t)B * T, seg_strips = 0;
    if (segs) {
        seg_strips = vrd::seg_table(sg, segs, 1, 16);
        VRD_CHECK_ARG(seg_strips >= 0, "vrd_local_attn_segs: bad row groups (1..%d groups)", VRD_MAX_SEGS);
        rows = 0;
        for (int g = 0; g < sg.count; ++g) rows += (int64_t)sg.n[g] * sg.T[g];
    }
    vrd::ProfScope prof(VRD_K_LOCAL_ATTN, s, 4.0 * (double)rows * sh.W * C, 16.0 * (double)rows * C);
    const float scale = 1.0f / sqrtf((float)sh.hd);
    unsigned* const rflag = out_pair == VRD_PAIR_F16 ? vrd::range_flag() : nullptr;
    const dim3 block(256);
    // strips of 16 query rows per wave (default; 32 measured the same) or, VRD_LOCAL_STRIP=0, one wave per query row
    // (6.1 vs 5.6 ms per step at the benchmark shape)
    static const int strip_env = [] { const char* e = getenv("VRD_LOCAL_STRIP"); return e ? atoi(e) : 1; }();
    if (strip_env || segs) {
        constexpr int RW = 16;
        const int strips = (T + RW - 1) / RW;
        const int64_t n_strips = segs ? seg_strips : (int64_t)B * strips;
        // four channels a lane: HV = 2 waves per strip at C = 512, one wave (its 64 lanes x 4 channels the whole row) at C = 256
        auto half_rows = [&](auto wins, auto HV) {
            constexpr int HVn = decltype(HV)::value;
            const dim3 grid((unsigned)((HVn * n_strips + 3) / 4));
            vrd::pick_of(wins, sh.W, [&](auto Wc) {
                vrd::la_pick_group<4>(sh.hd, [&](auto G) {
                    vrd::pick_bool(rel_pe != nullptr, [&](auto REL) {
                        hipLaunchKernelGGL((local_attn_strip_half_kernel<decltype(Wc)::value, decltype(G)::value, RW, decltype(REL)::value, HVn>),
                                           grid, block, 0, s, q, k, v, ld, mask, rel_pe, B, T, strips, scale, out, ldo, out_pair, rflag, sg);
                    });
                });
            });
        };
        // C = 512, windows up to 9: one wave per strip, whole rows in the ring; above: two waves per strip, half a row
        // each.  C = 256: the four-channels-a-lane kernel, one wave per strip, at every window
        if (C == 512 && sh.W <= vrd::LA_WRT) {
            const dim3 grid((unsigned)((n_strips + 3) / 4));
            vrd::pick_of(vrd::LaWinsLow{}, sh.W, [&](auto Wc) {
                vrd::la_pick_group<8>(sh.hd, [&](auto G) {
                    vrd::pick_bool(rel_pe != nullptr, [&](auto REL) {
                        hipLaunchKernelGGL((local_attn_strip_kernel<decltype(Wc)::value, decltype(G)::value, RW, decltype(REL)::value>),
                                           grid, block, 0, s, q, k, v, ld, mask, rel_pe, B, T, strips, scale, out, ldo, out_pair, rflag, sg);
                    });
                });
            });
        } else if (C == 512) {
            half_rows(vrd::LaWinsHigh{}, std::integral_constant<int, 2>{});
        } else {
            half_rows(vrd::LaWinsAll{}, std::integral_constant<int, 1>{});
        }
        VRD_LAUNCH_CHECK();
        return 0;
    }
    return vrd::local_attn_rows(sh, q, k, v, ld, mask, rel_pe, B, T, scale, out, ldo, out_pair, rflag, s);
}

}  // namespace

extern "C" {

int vrd_local_attn(const float* q, const float* k, const float* v, int64_t ld, const uint8_t* mask, const float* rel_pe,
                   int B, int T, int C, int n_head, int half_win, float* out, int64_t ldo, int out_pair, void* stream) {
    VRD_CHECK_ARG(B > 0 && T > 0, "vrd_local_attn: bad B / T");
    return local_attn_launch(q, k, v, ld, mask, rel_pe, B, T, nullptr, C, n_head, half_win, out, ldo, out_pair, stream);
}

int vrd_local_attn_segs(const float* q, const float* k, const float* v, int64_t ld, const uint8_t* mask, const float* rel_pe,
                        const vrd_row_segs* segs, int C, int n_head, int half_win, float* out, int64_t ldo, int out_pair,
                        void* stream) {
    VRD_CHECK_ARG(segs, "vrd_local_attn_segs: null row groups");
    return local_attn_launch(q, k, v, ld, mask, rel_pe, 0, 0, segs, C, n_head, half_win, out, ldo, out_pair, stream);
}

}  // extern "C"
