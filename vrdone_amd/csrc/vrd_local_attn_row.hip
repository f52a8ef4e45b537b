// Banded (local-window) attention, forward: the per-row kernel, one wave per query row.  vrd_local_attn runs it under
// VRD_LOCAL_STRIP=0 without row groups (vrd_local_attn.hip, which holds the strip kernels and the entry points); its 108
// instantiations are a translation unit of their own because they take half of the forward's compile time.
#include "vrd_local_attn.h"
#include <cmath>

namespace {

using vrd::dot4;
using vrd::ld4;
using vrd::st4;

// C = 512: lane l owns channels [8l, 8l+8); GROUP = head_dim / 8 lanes per head (4, 8 or 16).
// C = 256: lane l owns channels [4l, 4l+4); GROUP = head_dim / 4 (8, 16 or 32) -- the row addressing stays wave-uniform
// REL: the learnable per-(head, window slot) bias `rel_pe` (n_head x W) is added to the scaled scores before the key mask
// (blocks.py:957-958); a separate instantiation, so that the default path carries no extra instruction
// CPL: channels per lane, 8 (C = 512) or 4 (C = 256, the second float4 of every row dropped at compile time)
template <int W, int GROUP, bool REL, int CPL = 8>
__global__ __launch_bounds__(256) void local_attn_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                         const float* __restrict__ v, int64_t ld,
                                                         const uint8_t* __restrict__ mask, const float* __restrict__ rel,
                                                         int B, int T, float scale,
                                                         float* __restrict__ out, int64_t ldo, int pair, unsigned* rflag) {
    constexpr int HW = W / 2;
    const int lane = threadIdx.x & 63;
    // XCD-aware renumbering (as in the GEMM / flash kernels): consecutive workgroups are dealt round-robin to the
    // eight XCDs, and a row's K / V neighbours are re-read by the workgroups next to it -- a contiguous range of rows
    // per XCD keeps those re-reads in one L2 instead of fetching them from HBM once per XCD
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, qq = nwg >> 3, rem = nwg & 7;
    const int lid = (xcd < rem ? xcd * (qq + 1) : rem * (qq + 1) + (xcd - rem) * qq) + (bid >> 3);
    const int64_t row = (int64_t)lid * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: addresses on the scalar unit
    if (row >= (int64_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
    static_assert(CPL == 4 || CPL == 8, "C = 256 or 512");
    float* o = out + row * ldo + lane * CPL;
    if (!mask[row]) {      // masked query rows are zeroed after the softmax (blocks.py:977-978); 0 is 0 in pair rows too
        st4(o, make_float4(0.f, 0.f, 0.f, 0.f));
        if (CPL == 8) st4(o + 4, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    float4 q0 = ld4(q + row * ld + lane * CPL), q1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (CPL == 8) q1 = ld4(q + row * ld + lane * CPL + 4);
    q0.x *= scale; q0.y *= scale; q0.z *= scale; q0.w *= scale;
    q1.x *= scale; q1.y *= scale; q1.z *= scale; q1.w *= scale;
    float s[W];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int tj = t + j - HW;
        if (tj < 0 || tj >= T) { s[j] = -INFINITY; continue; }
        const float* kr = k + (row + j - HW) * ld + lane * CPL;
        float d = dot4(q0, ld4(kr));
        if (CPL == 8) d += dot4(q1, ld4(kr + 4));
        d = vrd::group_sum<GROUP>(d);
        if (REL) d += rel[(lane / GROUP) * W + j];
        s[j] = d + (mask[row + j - HW] ? 0.f : -1e4f);
        m = fmaxf(m, s[j]);
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < W; ++j) { s[j] = __expf(s[j] - m); den += s[j]; }
    const float inv = 1.0f / den;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int tj = t + j - HW;
        if (tj < 0 || tj >= T) continue;
        const float* vr = v + (row + j - HW) * ld + lane * CPL;
        const float4 v0 = ld4(vr);
        const float pj = s[j] * inv;
        a0.x += pj * v0.x; a0.y += pj * v0.y; a0.z += pj * v0.z; a0.w += pj * v0.w;
        if (CPL == 8) {
            const float4 v1 = ld4(vr + 4);
            a1.x += pj * v1.x; a1.y += pj * v1.y; a1.z += pj * v1.z; a1.w += pj * v1.w;
        }
    }
    if (pair) {
        vrd::RangeTrack rt;           // (q, k, v are f32 rows here: nothing upstream has checked their range)
        vrd::store_pair4(out + row * ldo, lane * CPL, 64 * CPL, a0, pair, &rt);
        if (CPL == 8) vrd::store_pair4(out + row * ldo, lane * CPL + 4, 64 * CPL, a1, pair, &rt);
        rt.report(rflag, vrd::RANGE_ATTN_OUT);
    } else {
        st4(o, a0);
        if (CPL == 8) st4(o + 4, a1);
    }
}

}  // namespace

int vrd::local_attn_rows(const LaShape& sh, const float* q, const float* k, const float* v, int64_t ld, const uint8_t* mask,
                         const float* rel_pe, int B, int T, float scale, float* out, int64_t ldo, int out_pair, unsigned* rflag,
                         hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)B * T + 3) / 4)), block(256);
    pick_of(LaWinsAll{}, sh.W, [&](auto Wc) {
        la_pick_lanes(sh, [&](auto G, auto CPL) {
            pick_bool(rel_pe != nullptr, [&](auto REL) {
                hipLaunchKernelGGL((local_attn_kernel<decltype(Wc)::value, decltype(G)::value, decltype(REL)::value, decltype(CPL)::value>),
                                   grid, block, 0, s, q, k, v, ld, mask, rel_pe, B, T, scale, out, ldo, out_pair, rflag);
            });
        });
    });
    VRD_LAUNCH_CHECK();
    return 0;
}

