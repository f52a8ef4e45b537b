// What the translation units of the banded (local-window) attention share -- vrd_local_attn.hip (forward: strip kernels, entry
// points), vrd_local_attn_row.hip (forward: per-row kernel) and vrd_local_attn_bwd.hip (training forward with attn_drop,
// backward): the envelope of accepted shapes, written once, and the helpers that turn a resolved shape into the template
// arguments of a kernel.  Host code but for dot4: every kernel, and every device helper only one file uses, lives in the file
// that compiles it.
#pragma once
#include "vrd_common.h"

namespace vrd {

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// Windows up to LA_WRT run the per-row training kernels with a run-time window (WT = 0), the wider ones up to LA_WMAX as
// compile-time constants; the strip kernels of the forward take every window as a constant.
constexpr int LA_WRT = 9, LA_WMAX = 19;

// The lists a wrapper picks its compile-time window from (pick_of): a kernel is instantiated for the windows of the list its
// wrapper names and for no other.
using LaWinsLow = IntList<3, 5, 7, 9>;
using LaWinsHigh = IntList<11, 13, 15, 17, 19>;
using LaWinsAll = IntList<3, 5, 7, 9, 11, 13, 15, 17, 19>;
using LaWinsTrain = IntList<0, 11, 13, 15, 17, 19>;       // 0: the run-time window, W <= LA_WRT

// A shape of the envelope.  CPL channels per lane of the per-row kernels (C / 64), GROUP = hd / CPL lanes per head.
struct LaShape {
    int C, hd, W, CPL, GROUP;
};

// The envelope: C = 256 or 512, head_dim 32, 64 or 128, window odd, 3 .. LA_WMAX.  0 and *sh filled, or -1 with the error set
// under the entry point's name `who`.
inline int la_shape(const char* who, int C, int n_head, int half_win, LaShape* sh) {
    VRD_CHECK_ARG((C == 256 || C == 512) && n_head > 0 && C % n_head == 0 &&
                      (C / n_head == 32 || C / n_head == 64 || C / n_head == 128),
                  "%s: built for C = 256 or 512 with head_dim = C / n_head of 32, 64 or 128 (got C = %d, n_head = %d)", who, C, n_head);
    VRD_CHECK_ARG(half_win >= 1 && half_win <= LA_WMAX / 2, "%s: window must be odd, 3..%d (got %d)", who, LA_WMAX, 2 * half_win + 1);
    sh->C = C, sh->hd = C / n_head, sh->W = 2 * half_win + 1, sh->CPL = C / 64, sh->GROUP = sh->hd / sh->CPL;
    return 0;
}

// f(GROUP) for the lanes per head of head_dim `hd` at CPL channels a lane: three cases
template <int CPL, class F>
void la_pick_group(int hd, F&& f) {
    pick_of(IntList<128 / CPL, 64 / CPL, 32 / CPL>{}, hd / CPL, f);
}
// f(GROUP, CPL) of a shape for the per-row kernels: the six pairs (4, 8, 16 | 8) and (8, 16, 32 | 4)
template <class F>
void la_pick_lanes(const LaShape& sh, F&& f) {
    if (sh.CPL == 8) la_pick_group<8>(sh.hd, [&](auto G) { f(G, std::integral_constant<int, 8>{}); });
    else la_pick_group<4>(sh.hd, [&](auto G) { f(G, std::integral_constant<int, 4>{}); });
}

// vrd_local_attn_row.hip: the per-row forward kernel over B x T rows of a resolved shape (0, or -2 with the error set)
int local_attn_rows(const LaShape& sh, const float* q, const float* k, const float* v, int64_t ld, const uint8_t* mask,
                    const float* rel_pe, int B, int T, float scale, float* out, int64_t ldo, int out_pair, unsigned* rflag,
                    hipStream_t s);

}  // namespace vrd
