// The 5 + 8 + 8 box-feature channels of a (subject, object) pair sequence (reference utils/misc.py:158-217), shared by the
// eval gather (vrd_gather_pairs, vrd_rowops.hip) and the training gather (vrd_gather_train, vrd_gather_train.hip).
// Box arithmetic is written operation by operation with the round-to-nearest intrinsics (no FMA contraction), in the
// reference's order, so everything but the three logarithms is the reference's f32 value bit for bit.
#pragma once
#include "vrd_common.h"
#include <cmath>

namespace vrd {

struct Box4 {
    float x0, y0, x1, y1;
};
// A16 = false: the boxes array is not 16-byte aligned -- the same four floats as four loads
template <bool A16 = true>
__device__ __forceinline__ Box4 load_box(const float* boxes, int64_t row) {
    const float* p = boxes + row * 4;
    if (A16) {
        const float4 b = *reinterpret_cast<const float4*>(p);
        return Box4{b.x, b.y, b.z, b.w};
    }
    return Box4{p[0], p[1], p[2], p[3]};
}
// normalised (cx, cy, w, h) of utils/misc.py:184-192
__device__ __forceinline__ void entity_geom(const Box4& b, float w, float h, float (&g)[4]) {
    const float x0 = __fdiv_rn(b.x0, w), x1 = __fdiv_rn(b.x1, w), y0 = __fdiv_rn(b.y0, h), y1 = __fdiv_rn(b.y1, h);
    g[0] = __fdiv_rn(__fadd_rn(x1, x0), 2.0f);
    g[1] = __fdiv_rn(__fadd_rn(y1, y0), 2.0f);
    g[2] = __fsub_rn(x1, x0);
    g[3] = __fsub_rn(y1, y0);
}
// [cx, dcx, cy, dcy, w, dw, h, dh] of frame t of an n-frame strided box sequence starting at row0 (utils/misc.py:194-217)
template <bool A16 = true>
__device__ __forceinline__ void entity_feats(const float* boxes, int64_t row0, int stride, int t, int n, float w, float h,
                                             float (&f)[8]) {
    float g[4], a[4], b[4];
    entity_geom(load_box<A16>(boxes, row0 + (int64_t)t * stride), w, h, g);
    float d[4];
    if (t > 0) {
        entity_geom(load_box<A16>(boxes, row0 + (int64_t)(t - 1) * stride), w, h, a);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = __fsub_rn(g[i], a[i]);
    } else if (n < 2) {     // a one-frame pair has no difference (the dataloader never emits one; never read past the pair)
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = 0.f;
    } else {            // first frame: d0 - (d1 - d0) with d0 = v1 - v0, d1 = v2 - v1; just d0 when there are two frames
        entity_geom(load_box<A16>(boxes, row0 + stride), w, h, a);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = __fsub_rn(a[i], g[i]);
        if (n > 2) {
            entity_geom(load_box<A16>(boxes, row0 + 2 * (int64_t)stride), w, h, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = __fsub_rn(d[i], __fsub_rn(__fsub_rn(b[i], a[i]), d[i]));
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) f[2 * i] = g[i], f[2 * i + 1] = d[i];
}
// the 5 subject-object channels of one frame (utils/misc.py:158-178)
__device__ __forceinline__ void so_box_feats(const Box4& s, const Box4& o, float (&f)[5]) {
    const float s_cx = __fdiv_rn(__fadd_rn(s.x1, s.x0), 2.0f), s_cy = __fdiv_rn(__fadd_rn(s.y1, s.y0), 2.0f);
    const float o_cx = __fdiv_rn(__fadd_rn(o.x1, o.x0), 2.0f), o_cy = __fdiv_rn(__fadd_rn(o.y1, o.y0), 2.0f);
    const float s_w = __fsub_rn(s.x1, s.x0), s_h = __fsub_rn(s.y1, s.y0), o_w = __fsub_rn(o.x1, o.x0), o_h = __fsub_rn(o.y1, o.y0);
    f[0] = __fdiv_rn(__fsub_rn(s_cx, o_cx), o_cx);
    f[1] = __fdiv_rn(__fsub_rn(s_cy, o_cy), o_cy);
    f[2] = logf(__fdiv_rn(s_w, o_w));
    f[3] = logf(__fdiv_rn(s_h, o_h));
    f[4] = logf(__fdiv_rn(__fmul_rn(s_w, s_h), __fmul_rn(o_w, o_h)));
}

}  // namespace vrd
