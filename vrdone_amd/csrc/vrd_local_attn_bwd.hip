// Banded (local-window) attention in training: the forward with attn_drop and the backward.  (The inference forward, which is
// also the training forward at p = 0: vrd_local_attn.hip; the envelope of shapes and the dispatch helpers: vrd_local_attn.h.)
//
//  vrd_local_attn_bwd                banded attention: dq, dk, dv
//  vrd_local_attn_bwd_segs           the same over a ragged row space (vrd_row_segs), one launch per pass
//  vrd_local_attn_drop / _drop_bwd   the same with attn_drop on the window probabilities (training forward and backward)
#include "vrd_local_attn.h"
#include "vrd_philox.h"
#include <cmath>

namespace {

using vrd::aligned16;
using vrd::ld4;
using vrd::st4;

// ------------------------------------------------------------------------------------------------------------------
// banded attention backward.  C = 512: lane l owns channels [8l, 8l+8), GROUP = head_dim / 8 lanes per head (4, 8, 16);
// C = 256 (CPL = 4): lane l owns channels [4l, 4l+4), GROUP = head_dim / 4 (8, 16, 32), the second float4 of every row
// dropped at compile time.  Either way 64 / GROUP heads, and the scratch is rows x heads x W.
// Pass 1, one wave per query row t: recompute the window probabilities P[t, j] (models/blocks.py:950-986: masked keys
// -1e4, out-of-range -inf, masked query rows all zero), dP = dO . v, dS = P * (dP - sum_j P dP); dq = scale * sum_j dS k;
// P and dS of the row go to scratch (rows x heads x W).  Pass 2, one wave per key row j: dk_j = scale * sum_t dS[t, j] q_t,
// dv_j = sum_t P[t, j] dO_t over the (at most W) queries whose window holds j.
// DROP (attn_drop, blocks.py:975-979, behind the masked-query zeroing): slot j of (row, head) has the factor f_j = keep / (1 - p)
// of element id ((row0 + row) * heads + head) * W + j (vrd_philox.h; every lane of a head's group computes the same decision).
// out = sum_j f_j P_j v_j, so dP_j = f_j dO . v_j, dS_j = P_j (dP_j - sum_k P_k dP_k), and the scratch's P holds f_j P_j, which
// is what dv sums over; pass 2 does not change.
// ------------------------------------------------------------------------------------------------------------------
template <int GROUP>
__device__ __forceinline__ float head_sum(float d) { return vrd::group_sum<GROUP>(d); }
__device__ __forceinline__ float dot8(const float4& a0, const float4& a1, const float4& b0, const float4& b1) {
    return (a0.x * b0.x + a0.y * b0.y + a0.z * b0.z + a0.w * b0.w) + (a1.x * b1.x + a1.y * b1.y + a1.z * b1.z + a1.w * b1.w);
}
__device__ __forceinline__ float la_dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// a lane's CPL channels of a row: .a alone at CPL = 4
struct LaRow {
    float4 a, b;
};
template <int CPL>
__device__ __forceinline__ LaRow la_load(const float* p) {
    LaRow r;
    r.a = ld4(p);
    r.b = CPL == 8 ? ld4(p + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    return r;
}
template <int CPL>
__device__ __forceinline__ float la_dot(const LaRow& x, const LaRow& y) {
    return CPL == 8 ? dot8(x.a, x.b, y.a, y.b) : la_dot4(x.a, y.a);
}
// WT: the window as a compile-time constant (11 .. 19: the loops unroll and s[] / dp[] stay in registers), or 0 for the
// run-time windows up to LA_WRT, whose nine-entry arrays the compiler already keeps in registers
using vrd::LA_WRT;
// SEGS (vrd_local_attn_bwd_segs): wave w works on frame w of the groups' frames counted through `sg` in order; its q / k / v / dO /
// mask / dq row is the frame's row in the row space, its scratch row is w -- the scratch has no gaps, so that the sum of dS over
// all its rows (d rel_pe) stays one reduction.  B is unused, T is the group's.
template <int GROUP, int WT, int CPL = 8, bool DROP = false, bool SEGS = false>
__global__ __launch_bounds__(256) void local_attn_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                               const float* __restrict__ v, int64_t ld,
                                                               const float* __restrict__ dO, int64_t lddo,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ rel,
                                                               int B, int T, int W_rt, float scale,
                                                               float* __restrict__ dq, int64_t lddq, float* __restrict__ P,
                                                               float* __restrict__ dS, vrd::DropSite drop, uint64_t row0,
                                                               const vrd::RowSegArg<SEGS> sg) {
    const int W = WT ? WT : W_rt;
    const int HW = W / 2;
    const int lane = threadIdx.x & 63;
    const int64_t srow = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // the wave's scratch row
    int64_t row = srow;
    int t;
    if constexpr (SEGS) {
        int g, b;
        if (!vrd::seg_find(sg, vrd::wave_uniform(srow), g, b, t)) return;
        T = sg.T[g];
        row = sg.row[g] + (int64_t)b * T + t;
    } else {
        if (row >= (int64_t)B * T) return;
        t = (int)(row % T);
    }
    constexpr int H = 64 / GROUP;
    const int head = lane / GROUP;
    float* const Pr = P + (srow * H + head) * W;
    float* const dSr = dS + (srow * H + head) * W;
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
    if (!mask[row]) {
        if (lane % GROUP == 0)
            for (int j = 0; j < W; ++j) Pr[j] = 0.f, dSr[j] = 0.f;
        st4(dq + row * lddq + lane * CPL, g0);
        if (CPL == 8) st4(dq + row * lddq + lane * CPL + 4, g0);
        return;
    }
    const LaRow qv = la_load<CPL>(q + row * ld + lane * CPL), ov = la_load<CPL>(dO + row * lddo + lane * CPL);
    float s[WT ? WT : LA_WRT], dp[WT ? WT : LA_WRT];
    float m = -INFINITY;
    for (int j = 0; j < W; ++j) {
        const int tj = t + j - HW;
        s[j] = -INFINITY;
        dp[j] = 0.f;
        if (tj < 0 || tj >= T) continue;
        const float* kr = k + (row + j - HW) * ld + lane * CPL;
        const float* vr = v + (row + j - HW) * ld + lane * CPL;
        const float d = head_sum<GROUP>(la_dot<CPL>(qv, la_load<CPL>(kr))) * scale;
        dp[j] = head_sum<GROUP>(la_dot<CPL>(ov, la_load<CPL>(vr)));
        s[j] = (rel ? d + rel[head * W + j] : d) + (mask[row + j - HW] ? 0.f : -1e4f);
        m = fmaxf(m, s[j]);
    }
    float den = 0.f;
    for (int j = 0; j < W; ++j) { s[j] = __expf(s[j] - m); den += s[j]; }
    const float inv = 1.0f / den;
    float fac[DROP ? (WT ? WT : LA_WRT) : 1];
    if (DROP) {
        const uint64_t seed = vrd::uniform_load(drop.seed), id0 = ((row0 + (uint64_t)row) * H + head) * W;
        for (int j = 0; j < W; ++j) {
            fac[j] = vrd::drop_factor(seed, drop, id0 + j);
            dp[j] *= fac[j];
        }
    }
    float dsum = 0.f;
    for (int j = 0; j < W; ++j) { s[j] *= inv; dsum = fmaf(s[j], dp[j], dsum); }
    for (int j = 0; j < W; ++j) {
        const float ds = s[j] * (dp[j] - dsum);
        if (lane % GROUP == 0) Pr[j] = DROP ? s[j] * fac[j] : s[j], dSr[j] = ds;
        const int tj = t + j - HW;
        if (tj < 0 || tj >= T) continue;
        const float* kr = k + (row + j - HW) * ld + lane * CPL;
        const float4 k0 = ld4(kr);
        const float f = ds * scale;
        g0.x = fmaf(f, k0.x, g0.x); g0.y = fmaf(f, k0.y, g0.y); g0.z = fmaf(f, k0.z, g0.z); g0.w = fmaf(f, k0.w, g0.w);
        if (CPL == 8) {
            const float4 k1 = ld4(kr + 4);
            g1.x = fmaf(f, k1.x, g1.x); g1.y = fmaf(f, k1.y, g1.y); g1.z = fmaf(f, k1.z, g1.z); g1.w = fmaf(f, k1.w, g1.w);
        }
    }
    st4(dq + row * lddq + lane * CPL, g0);
    if (CPL == 8) st4(dq + row * lddq + lane * CPL + 4, g1);
}
// The training forward with attn_drop, in the shape of pass 1: one wave per query row, the window in registers.  (The strip
// kernels of vrd_local_attn.hip keep the inference path and the p = 0 training forward; this one re-reads every K / V row W times.)
template <int GROUP, int WT, int CPL = 8>
__global__ __launch_bounds__(256) void local_attn_drop_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int64_t ld,
                                                                  const uint8_t* __restrict__ mask, const float* __restrict__ rel,
                                                                  int B, int T, int W_rt, float scale, vrd::DropSite drop, uint64_t row0,
                                                                  float* __restrict__ out, int64_t ldo) {
    const int W = WT ? WT : W_rt;
    const int HW = W / 2;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B * T) return;
    const int t = (int)(row % T);
    constexpr int H = 64 / GROUP;
    const int head = lane / GROUP;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    if (!mask[row]) {
        st4(out + row * ldo + lane * CPL, a0);
        if (CPL == 8) st4(out + row * ldo + lane * CPL + 4, a0);
        return;
    }
    const LaRow qv = la_load<CPL>(q + row * ld + lane * CPL);
    float s[WT ? WT : LA_WRT];
    float m = -INFINITY;
    for (int j = 0; j < W; ++j) {
        const int tj = t + j - HW;
        s[j] = -INFINITY;
        if (tj < 0 || tj >= T) continue;
        const float d = head_sum<GROUP>(la_dot<CPL>(qv, la_load<CPL>(k + (row + j - HW) * ld + lane * CPL))) * scale;
        s[j] = (rel ? d + rel[head * W + j] : d) + (mask[row + j - HW] ? 0.f : -1e4f);
        m = fmaxf(m, s[j]);
    }
    float den = 0.f;
    for (int j = 0; j < W; ++j) { s[j] = __expf(s[j] - m); den += s[j]; }
    const float inv = 1.0f / den;
    const uint64_t seed = vrd::uniform_load(drop.seed), id0 = ((row0 + (uint64_t)row) * H + head) * W;
    for (int j = 0; j < W; ++j) {
        const int tj = t + j - HW;
        if (tj < 0 || tj >= T) continue;
        const float f = s[j] * inv * vrd::drop_factor(seed, drop, id0 + j);
        const LaRow vv = la_load<CPL>(v + (row + j - HW) * ld + lane * CPL);
        a0.x = fmaf(f, vv.a.x, a0.x); a0.y = fmaf(f, vv.a.y, a0.y); a0.z = fmaf(f, vv.a.z, a0.z); a0.w = fmaf(f, vv.a.w, a0.w);
        if (CPL == 8) { a1.x = fmaf(f, vv.b.x, a1.x); a1.y = fmaf(f, vv.b.y, a1.y); a1.z = fmaf(f, vv.b.z, a1.z); a1.w = fmaf(f, vv.b.w, a1.w); }
    }
    st4(out + row * ldo + lane * CPL, a0);
    if (CPL == 8) st4(out + row * ldo + lane * CPL + 4, a1);
}
template <int GROUP, int CPL = 8, bool SEGS = false>
__global__ __launch_bounds__(256) void local_attn_bwd_kv_kernel(const float* __restrict__ q, int64_t ld,
                                                                const float* __restrict__ dO, int64_t lddo, int B, int T, int W,
                                                                float scale, const float* __restrict__ P,
                                                                const float* __restrict__ dS, float* __restrict__ dk,
                                                                float* __restrict__ dv, int64_t lddkv,
                                                                const vrd::RowSegArg<SEGS> sg) {
    const int HW = W / 2;
    const int lane = threadIdx.x & 63;
    const int64_t srow = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // key row j in the scratch's count (SEGS: see pass 1)
    int64_t row = srow;                                                      // ... and in the operands
    int tj;
    if constexpr (SEGS) {
        int g, b;
        if (!vrd::seg_find(sg, vrd::wave_uniform(srow), g, b, tj)) return;
        T = sg.T[g];
        row = sg.row[g] + (int64_t)b * T + tj;
    } else {
        if (row >= (int64_t)B * T) return;
        tj = (int)(row % T);
    }
    constexpr int H = 64 / GROUP;
    const int head = lane / GROUP;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, c0 = a0, c1 = a0;
    for (int i = 0; i < W; ++i) {           // query t = tj + HW - i sees key tj at window position i
        const int t = tj + HW - i;
        if (t < 0 || t >= T) continue;
        const int64_t qr = row + HW - i, sr = srow + HW - i;       // (a sequence's rows are consecutive in both counts)
        const float p = P[(sr * H + head) * W + i], ds = dS[(sr * H + head) * W + i] * scale;
        const float4 q0 = ld4(q + qr * ld + lane * CPL), o0 = ld4(dO + qr * lddo + lane * CPL);
        a0.x = fmaf(ds, q0.x, a0.x); a0.y = fmaf(ds, q0.y, a0.y); a0.z = fmaf(ds, q0.z, a0.z); a0.w = fmaf(ds, q0.w, a0.w);
        c0.x = fmaf(p, o0.x, c0.x); c0.y = fmaf(p, o0.y, c0.y); c0.z = fmaf(p, o0.z, c0.z); c0.w = fmaf(p, o0.w, c0.w);
        if (CPL == 8) {
            const float4 q1 = ld4(q + qr * ld + lane * CPL + 4), o1 = ld4(dO + qr * lddo + lane * CPL + 4);
            a1.x = fmaf(ds, q1.x, a1.x); a1.y = fmaf(ds, q1.y, a1.y); a1.z = fmaf(ds, q1.z, a1.z); a1.w = fmaf(ds, q1.w, a1.w);
            c1.x = fmaf(p, o1.x, c1.x); c1.y = fmaf(p, o1.y, c1.y); c1.z = fmaf(p, o1.z, c1.z); c1.w = fmaf(p, o1.w, c1.w);
        }
    }
    st4(dk + row * lddkv + lane * CPL, a0);
    if (CPL == 8) st4(dk + row * lddkv + lane * CPL + 4, a1);
    st4(dv + row * lddkv + lane * CPL, c0);
    if (CPL == 8) st4(dv + row * lddkv + lane * CPL + 4, c1);
}

// drop: NULL (vrd_local_attn_bwd, and vrd_local_attn_drop_bwd at p = 0: the same kernels, the same bits), or the attn_drop site
// segs: NULL, or the row groups of vrd_local_attn_bwd_segs (B, T unused; no drop)
int local_attn_bwd_launch(const float* q, const float* k, const float* v, int64_t ld, const float* dO, int64_t lddo,
                          const uint8_t* mask, const float* rel_pe, int B, int T, int C, int n_head, int half_win,
                          const vrd::DropSite* drop, int64_t row0, float* dq, float* dk, float* dv, int64_t ldd, float* scratch,
                          void* stream, const vrd_row_segs* segs = nullptr) {
    VRD_CHECK_ARG(q && k && v && dO && mask && dq && dk && dv && scratch, "vrd_local_attn_bwd: null pointer");
    vrd::LaShape sh;
    if (int rc = vrd::la_shape(segs ? "vrd_local_attn_bwd_segs" : "vrd_local_attn_bwd", C, n_head, half_win, &sh)) return rc;
    VRD_CHECK_ARG(ld >= C && lddo >= C && ldd >= C, "vrd_local_attn_bwd: leading dimension too small");
    VRD_CHECK_ARG(ld % 4 == 0 && lddo % 4 == 0 && ldd % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(dO) &&
                      aligned16(dq) && aligned16(dk) && aligned16(dv),
                  "vrd_local_attn_bwd: rows must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int W = sh.W;
    const float scale = 1.0f / sqrtf((float)sh.hd);
    if (segs) {
        // the frames of all groups, counted through the groups: the scratch rows.  P lies at the scratch's start, dS behind the
        // P rows of a scratch sized for every row the groups span (the caller sizes it without walking the table)
        vrd::SegTable sg;
        const int64_t rows = vrd::seg_table(sg, segs, 1, 1);
        VRD_CHECK_ARG(rows > 0 && !drop, "vrd_local_attn_bwd_segs: bad row groups (1..%d groups)", VRD_MAX_SEGS);
        int64_t lo = segs->row[0], hi = 0;
        for (int g = 0; g < segs->count; ++g) {
            const int64_t end = segs->row[g] + (int64_t)segs->n[g] * segs->T[g];
            lo = segs->row[g] < lo ? segs->row[g] : lo;
            hi = end > hi ? end : hi;
        }
        float* P = scratch;
        float* dS = scratch + (hi - lo) * n_head * W;
        vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)rows * C * 8);
        const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
        const vrd::DropSite site{nullptr, 0u, 0u, 1.0f};
        vrd::pick_of(vrd::LaWinsTrain{}, W <= LA_WRT ? 0 : W, [&](auto WT) {
            vrd::la_pick_lanes(sh, [&](auto G, auto CPL) {
                hipLaunchKernelGGL((local_attn_bwd_q_kernel<decltype(G)::value, decltype(WT)::value, decltype(CPL)::value, false, true>), grid, block,
                                   0, s, q, k, v, ld, dO, lddo, mask, rel_pe, 0, 0, W, scale, dq, ldd, P, dS, site, (uint64_t)0, sg);
            });
        });
        vrd::la_pick_lanes(sh, [&](auto G, auto CPL) {
            hipLaunchKernelGGL((local_attn_bwd_kv_kernel<decltype(G)::value, decltype(CPL)::value, true>), grid, block, 0, s, q, ld, dO, lddo, 0, 0,
                               W, scale, P, dS, dk, dv, ldd, sg);
        });
        VRD_LAUNCH_CHECK();
        return 0;
    }
    const int64_t rows = (int64_t)B * T;
    float* P = scratch;
    float* dS = scratch + rows * n_head * W;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)rows * C * 8);
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const vrd::DropSite site = drop ? *drop : vrd::DropSite{nullptr, 0u, 0u, 1.0f};
    vrd::pick_of(vrd::LaWinsTrain{}, W <= LA_WRT ? 0 : W, [&](auto WT) {
        vrd::la_pick_lanes(sh, [&](auto G, auto CPL) {
            vrd::pick_bool(drop != nullptr, [&](auto DROP) {
                hipLaunchKernelGGL((local_attn_bwd_q_kernel<decltype(G)::value, decltype(WT)::value, decltype(CPL)::value, decltype(DROP)::value>),
                                   grid, block, 0, s, q, k, v, ld, dO, lddo, mask, rel_pe, B, T, W, scale, dq, ldd, P, dS, site, (uint64_t)row0,
                                   vrd::NoRowSegs{});
            });
        });
    });
    vrd::la_pick_lanes(sh, [&](auto G, auto CPL) {
        hipLaunchKernelGGL((local_attn_bwd_kv_kernel<decltype(G)::value, decltype(CPL)::value>), grid, block, 0, s, q, ld, dO, lddo, B, T, W,
                           scale, P, dS, dk, dv, ldd, vrd::NoRowSegs{});
    });
    VRD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int vrd_local_attn_bwd(const float* q, const float* k, const float* v, int64_t ld, const float* dO, int64_t lddo,
                       const uint8_t* mask, const float* rel_pe, int B, int T, int C, int n_head, int half_win,
                       float* dq, float* dk, float* dv, int64_t ldd, float* scratch, void* stream) {
    return local_attn_bwd_launch(q, k, v, ld, dO, lddo, mask, rel_pe, B, T, C, n_head, half_win, nullptr, 0, dq, dk, dv, ldd, scratch, stream);
}

int vrd_local_attn_bwd_segs(const float* q, const float* k, const float* v, int64_t ld, const float* dO, int64_t lddo,
                            const uint8_t* mask, const float* rel_pe, const vrd_row_segs* segs, int C, int n_head, int half_win,
                            float* dq, float* dk, float* dv, int64_t ldd, float* scratch, void* stream) {
    VRD_CHECK_ARG(segs, "vrd_local_attn_bwd_segs: null row groups");
    return local_attn_bwd_launch(q, k, v, ld, dO, lddo, mask, rel_pe, 0, 0, C, n_head, half_win, nullptr, 0, dq, dk, dv, ldd, scratch, stream, segs);
}

int vrd_local_attn_drop_bwd(const float* q, const float* k, const float* v, int64_t ld, const float* dO, int64_t lddo,
                            const uint8_t* mask, const float* rel_pe, int B, int T, int C, int n_head, int half_win,
                            const uint64_t* seed, unsigned site, int64_t row0, float p, float* dq, float* dk, float* dv, int64_t ldd,
                            float* scratch, void* stream) {
    VRD_CHECK_ARG(p >= 0.f && p < 1.f && row0 >= 0, "vrd_local_attn_drop_bwd: the rate lies in [0, 1) (got %g), row0 >= 0", (double)p);
    VRD_CHECK_ARG(seed || p == 0.f, "vrd_local_attn_drop_bwd: null seed");
    const vrd::DropSite d = vrd::drop_site(seed, site, p);
    return local_attn_bwd_launch(q, k, v, ld, dO, lddo, mask, rel_pe, B, T, C, n_head, half_win, p == 0.f ? nullptr : &d, row0, dq, dk, dv, ldd,
                                 scratch, stream);
}

int vrd_local_attn_drop(const float* q, const float* k, const float* v, int64_t ld, const uint8_t* mask, const float* rel_pe, int B,
                        int T, int C, int n_head, int half_win, const uint64_t* seed, unsigned site, int64_t row0, float p, float* out,
                        int64_t ldo, void* stream) {
    VRD_CHECK_ARG(p >= 0.f && p < 1.f && row0 >= 0, "vrd_local_attn_drop: the rate lies in [0, 1) (got %g), row0 >= 0", (double)p);
    // p = 0: the forward everything else runs (f32 rows out), the same bits
    if (p == 0.f) return vrd_local_attn(q, k, v, ld, mask, rel_pe, B, T, C, n_head, half_win, out, ldo, VRD_PAIR_NONE, stream);
    VRD_CHECK_ARG(q && k && v && mask && out && seed, "vrd_local_attn_drop: null pointer");
    VRD_CHECK_ARG(B > 0 && T > 0, "vrd_local_attn_drop: bad B / T");
    vrd::LaShape sh;
    if (int rc = vrd::la_shape("vrd_local_attn_drop", C, n_head, half_win, &sh)) return rc;
    VRD_CHECK_ARG(ld >= C && ldo >= C && ld % 4 == 0 && ldo % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out),
                  "vrd_local_attn_drop: rows must be 16-byte aligned with leading dimensions >= C");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows = (int64_t)B * T;
    const int W = sh.W;
    const float scale = 1.0f / sqrtf((float)sh.hd);
    const vrd::DropSite d = vrd::drop_site(seed, site, p);
    vrd::ProfScope prof(VRD_K_LOCAL_ATTN, s, 4.0 * (double)rows * W * C, 16.0 * (double)rows * C);
    const dim3 grid((unsigned)((rows + 3) / 4));
    vrd::pick_of(vrd::LaWinsTrain{}, W <= LA_WRT ? 0 : W, [&](auto WT) {
        vrd::la_pick_lanes(sh, [&](auto G, auto CPL) {
            hipLaunchKernelGGL((local_attn_drop_fwd_kernel<decltype(G)::value, decltype(WT)::value, decltype(CPL)::value>), grid, dim3(256), 0, s,
                               q, k, v, ld, mask, rel_pe, B, T, W, scale, d, (uint64_t)row0, out, ldo);
        });
    });
    VRD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
