// Training dropout on f32 rows (reference models/blocks.py:988,1057,1059: proj_drop and the two MLP dropouts of a
// TransformerBlock).  No mask is stored: forward and backward compute the keep decisions from (seed, site, element id)
// (vrd_philox.h; host mirror vrdone_amd/dropout.py).  The banded attention's attn_drop lives with its kernels (vrd_local_attn_bwd.hip).
//
//  vrd_dropout_mask   the keep decisions of n consecutive ids as bytes: what the tests pin against the host mirror
//  vrd_dropout_rows   out[r, c] = x[r, c] * keep(id) / (1 - p), id = (row0 + r) * C + c: the forward, and on dy the backward.
//                     HBM-bound: a lane owns a float4, whose four ids share one generator call
#include "vrd_philox.h"

namespace {

using vrd::aligned16;

__global__ __launch_bounds__(256) void dropout_mask_kernel(vrd::DropSite d, uint64_t first_id, int64_t n, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = vrd::drop_factor(vrd::uniform_load(d.seed), d, first_id + (uint64_t)i) != 0.f ? 1 : 0;
}

// (x and out may be the same rows: every lane reads its float4 before it writes it)
__global__ __launch_bounds__(256) void dropout_rows_kernel(const float* x, int64_t ldx, int64_t rows, int C4, vrd::DropSite d,
                                                           uint64_t row0, float* out, int64_t ldo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C4) return;
    const int64_t r = idx / C4;
    const int c4 = (int)(idx - r * C4);
    // id = (row0 + r) * C + 4 c4 is a multiple of 4 (C % 4 == 0): the lane's channels are the four words of block id / 4
    const vrd::PhiloxWords w = vrd::drop_words(vrd::uniform_load(d.seed), d.site, (row0 + (uint64_t)r) * (uint64_t)C4 + (uint64_t)c4);
    float4 v = vrd::gload4(x + r * ldx + 4 * c4);
    v.x *= w.w[0] >= d.threshold ? d.scale : 0.f;
    v.y *= w.w[1] >= d.threshold ? d.scale : 0.f;
    v.z *= w.w[2] >= d.threshold ? d.scale : 0.f;
    v.w *= w.w[3] >= d.threshold ? d.scale : 0.f;
    vrd::gstore4(out + r * ldo + 4 * c4, v);
}

}  // namespace

extern "C" {

int vrd_dropout_mask(const uint64_t* seed, unsigned site, int64_t first_id, int64_t n, float p, uint8_t* keep, void* stream) {
    VRD_CHECK_ARG(seed && keep && n > 0 && n <= ((int64_t)1 << 38) && first_id >= 0, "vrd_dropout_mask: bad arguments");
    VRD_CHECK_ARG(p >= 0.f && p < 1.f, "vrd_dropout_mask: the rate lies in [0, 1) (got %g)", (double)p);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, vrd::drop_site(seed, site, p),
                       (uint64_t)first_id, n, keep);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_dropout_rows(const float* x, int64_t ldx, int64_t rows, int C, const uint64_t* seed, unsigned site, int64_t row0, float p,
                     float* out, int64_t ldo, void* stream) {
    VRD_CHECK_ARG(x && out && seed && rows > 0 && C > 0 && C % 4 == 0 && row0 >= 0, "vrd_dropout_rows: bad arguments (C %% 4 == 0 required)");
    VRD_CHECK_ARG(p >= 0.f && p < 1.f, "vrd_dropout_rows: the rate lies in [0, 1) (got %g)", (double)p);
    VRD_CHECK_ARG(ldx >= C && ldo >= C && ldx % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(out),
                  "vrd_dropout_rows: rows must be 16-byte aligned");
    const int64_t n = rows * (C / 4);
    VRD_CHECK_ARG(n <= ((int64_t)1 << 38), "vrd_dropout_rows: too many elements for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 8.0 * (double)rows * C);
    hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, rows, C / 4,
                       vrd::drop_site(seed, site, p), (uint64_t)row0, out, ldo);
    VRD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
