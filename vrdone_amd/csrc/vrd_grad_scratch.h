// What the parameter-gradient entry points (vrd_wgrad.hip, vrd_colsum.hip, vrd_layernorm_bwd in vrd_backward.hip) share: the
// caller's scratch buffer -- its check in the deterministic mode, the place of rows of partial sums in it -- and the launches of
// vrd_colsum.hip that the other two files need.  Host functions only: every kernel is compiled in exactly one file.
//
// An entry point works out a plan from its shapes, leading dimensions and mode before its first launch: the kernel form, the
// grid, and where in the scratch each region starts.  The deterministic mode's check compares the caller's scratch with the plan's
// total_floats and every launch takes its pointer as scratch + an offset of the plan, so what is asked for and what is written
// cannot drift apart.
#pragma once
#include "vrd_common.h"

namespace vrd {

// default mode: partial sums go through the scratch only when it holds them
inline bool scratch_holds(const float* scratch, int64_t scratch_floats, int64_t need) {
    return scratch && aligned16(scratch) && scratch_floats >= need;
}

// deterministic mode: a call whose scratch is missing, misaligned or smaller than `need` floats fails before any launch
// (VRD_ERR_SCRATCH; vrd_scratch_required() then reports `need`).  0 when the scratch will do.
int check_det_scratch(const char* what, const float* scratch, int64_t scratch_floats, int64_t need);

// Deterministic mode: floats the chain of colpartial_reduce_kernel<true> launches needs behind `parts` partial rows of `cols` columns
inline int64_t det_reduce_extra(int64_t parts, int64_t cols) {
    int64_t extra = 0;
    while (parts > 32) {
        parts = (parts + 31) / 32;
        extra += parts * cols;
    }
    return extra;
}

// `parts` rows of `cols` partial sums (one row per row block or row chunk) in the scratch, as float offsets: the rows, the levels
// of the deterministic mode's tree behind them (deterministic mode only), and the first float behind both
struct PartialRows {
    int64_t parts;
    int cols;
    int64_t rows_off, levels_off, end;
};
inline PartialRows place_partial_rows(int64_t base, int64_t parts, int64_t cols, bool det) {
    PartialRows p;
    p.parts = parts, p.cols = (int)cols;
    p.rows_off = base;
    p.levels_off = base + parts * cols;
    p.end = p.levels_off + (det ? det_reduce_extra(parts, cols) : 0);
    return p;
}

// out0[c] (c < split) / out1[c - split] += sum_p rows[p * cols + c].  det: in a fixed tree, 32 partial rows per
// block, level by level, the levels' rows at levels_off; default mode: one launch, one atomic per column and 32 rows
int reduce_partial_rows(float* scratch, const PartialRows& p, float* out0, float* out1, int split, bool det, hipStream_t s);

// One launch of a column-sum kernel over `rows` rows (vrd_colsum, vrd_dwconv_wgrad, the bias of a weight gradient)
struct ColsumPlan {
    bool vec;                   // four channels per lane (float4-shaped rows), else one
    int col_blocks, rpb;        // grid.y; rows per block
    unsigned row_blocks;        // grid.x
    bool partials;              // the row blocks' sums go to pr.rows_off and are reduced from there; else one atomic per block
    PartialRows pr;
    int64_t total_floats() const { return partials ? pr.end : pr.rows_off; }       // the scratch ends here for this launch
};

// dbias[n] += sum_r G[r, n] * mask[r] as a launch of its own (the wave kernel of vrd_gemm_wgrad_x3 has no bias path).  The plan
// puts its partial rows (deterministic mode) at `base`; bias_colsum launches the kernel and, in that mode, their reduction.
ColsumPlan plan_bias_colsum(int64_t M, int N, bool det, int64_t base);
int bias_colsum(const ColsumPlan& plan, const float* G, int64_t ldg, const uint8_t* row_mask, int64_t M, int N, float* dbias, float* scratch,
                bool det, hipStream_t s);

}  // namespace vrd

#define VRD_CHECK_FLAGS(what) VRD_CHECK_ARG((flags & ~VRD_DETERMINISTIC) == 0, "%s: unknown flags 0x%x", what, (unsigned)flags)
