// Backward kernels of the relation-encoding path (training step, BASELINE config 3).
//
// The reference differentiates its ATen graph with autograd (train.py:186); here every forward kernel family gets
// the hand-written kernel(s) that compute its input / parameter gradients, bound through the same C ABI and wrapped
// as torch.autograd.Function in vrdone_amd/autograd.py.  Training batches are small (24 pairs x 96 frames = 2,304
// rows for vidvrd.yaml; 48 x 512 for vidor), so these kernels are written for correctness and sane memory access
// (coalesced rows, one wave per row, f32 MFMA for the one real contraction), not tuned like the forward path.
// Everything is f32.  This file holds the input gradients and the LayerNorm backward; the weight gradients of the dense
// convolutions are in vrd_wgrad.hip, the column sums (bias, drop-path-scale, depthwise-conv-weight gradients) in vrd_colsum.hip.
// LayerNorm's parameter gradients are ACCUMULATED (+=) into caller-zeroed buffers, with float atomics or through rows of
// partial sums in the caller's scratch; with VRD_DETERMINISTIC always the latter, added up in index order (vrd_grad_scratch.h).
//
//  vrd_rowcol_scale    out = v * colscale[c] * rowscale[r] * mask[r] + res * (mask) + res2: the affine drop-path
//                      residual of blocks.py:1074-1076,1148 in training form, and its input gradient
//  vrd_act / _bwd      GELU (erf) / ReLU and their derivative
//  vrd_layernorm_bwd   dx, dgamma, dbeta of the channel LayerNorm (+ReLU)
//  vrd_dwconv_bwd      input gradient of the depthwise conv (k 1/3, stride 1/2, 1 or 2 inputs per group, up to 3 sets,
//                      optional nearest-x2-upsample-add input)
//  vrd_attn_bwd_probs  global attention: probabilities P and score gradients dS, row by row
//  vrd_bmm             strided batched matmul (dq = dS K, dk = dS^T Q, dv = P^T dO; mask head)
//  vrd_maxpool_bwd     MaxPool1d(3,2,1) * mask
//  vrd_dwconv_bwd_segs / vrd_maxpool_bwd_segs   the two over a ragged row space (vrd_row_segs), one launch for all groups
// (the banded attention's backward and its training forward with attn_drop: vrd_local_attn_bwd.hip)
#include "vrd_grad_scratch.h"
#include <cstdlib>
#include <cmath>

namespace {

using vrd::aligned16;
constexpr float LN_EPS = 1e-5f;

using vrd::ld4;
using vrd::st4;

// out[r,c] = v[r,c] * cs[c] * rs[r] * m[r] + res[r,c] * (res_masked ? m[r] : 1) + res2[r,c]
__global__ __launch_bounds__(256) void rowcol_scale_kernel(const float* __restrict__ v, int64_t ldv, int64_t rows, int C4,
                                                           const float* __restrict__ cs, const float* __restrict__ rs,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ res,
                                                           int64_t ldres, int res_masked, const float* __restrict__ res2,
                                                           int64_t ldres2, float* __restrict__ out, int64_t ldo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C4) return;
    const int64_t r = idx / C4;
    const int c = (int)(idx - r * C4) * 4;
    const float m = mask ? (float)mask[r] : 1.f;
    const float f = (rs ? rs[r] : 1.f) * m;
    float4 x = ld4(v + r * ldv + c);
    float4 k = cs ? ld4(cs + c) : make_float4(1.f, 1.f, 1.f, 1.f);
    x.x *= k.x * f; x.y *= k.y * f; x.z *= k.z * f; x.w *= k.w * f;
    if (res) {
        const float4 q = ld4(res + r * ldres + c);
        const float rm = res_masked ? m : 1.f;
        x.x += q.x * rm; x.y += q.y * rm; x.z += q.z * rm; x.w += q.w * rm;
    }
    if (res2) {
        const float4 q = ld4(res2 + r * ldres2 + c);
        x.x += q.x; x.y += q.y; x.z += q.z; x.w += q.w;
    }
    st4(out + r * ldo + c, x);
}

// y = act(x), or dx = dy * act'(x)  (act: 1 ReLU, 2 GELU(erf)); n4 float4 groups of a dense (rows x C) matrix with
// leading dimensions
__device__ __forceinline__ float act_fwd(float x, int act) { return act == VRD_ACT_RELU ? fmaxf(x, 0.f) : vrd::gelu_erf(x); }
__device__ __forceinline__ float act_grad(float x, int act) {
    if (act == VRD_ACT_RELU) return x > 0.f ? 1.f : 0.f;
    // d/dx [x * Phi(x)] = Phi(x) + x * phi(x)
    const float phi = 0.3989422804014327f * __expf(-0.5f * x * x);
    return 0.5f * (1.f + vrd::erf_f32(x * 0.70710678118654752440f)) + x * phi;
}
__global__ __launch_bounds__(256) void act_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ dy,
                                                  int64_t lddy, int64_t rows, int C4, int act, float* __restrict__ out, int64_t ldo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C4) return;
    const int64_t r = idx / C4;
    const int c = (int)(idx - r * C4) * 4;
    const float4 a = ld4(x + r * ldx + c);
    float4 o;
    if (dy) {
        const float4 g = ld4(dy + r * lddy + c);
        o = make_float4(g.x * act_grad(a.x, act), g.y * act_grad(a.y, act), g.z * act_grad(a.z, act), g.w * act_grad(a.w, act));
    } else {
        o = make_float4(act_fwd(a.x, act), act_fwd(a.y, act), act_fwd(a.z, act), act_fwd(a.w, act));
    }
    st4(out + r * ldo + c, o);
}

// ------------------------------------------------------------------------------------------------------------------
// LayerNorm backward.  One wave per row, several rows per wave; y = xhat * gamma + beta (ReLU optional):
//   g = dy * (relu ? y > 0 : 1) * gamma;  dx = rstd * (g - mean(g) - xhat * mean(g * xhat))
//   dgamma += sum_r dy' * xhat,  dbeta += sum_r dy'     (per-lane partial sums, one atomic per channel and wave)
// ------------------------------------------------------------------------------------------------------------------
constexpr int LNB_ROWS = 8;        // rows per wave at least (the host asks for more on long inputs: every block ends in 2 C
                                   // atomics on the same 2 C addresses, and atomics on one address queue up in L2)
template <int NV>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ dy,
                                                            int64_t lddy, int64_t rows, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int relu, float* __restrict__ dx,
                                                            int64_t lddx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            int rpw, float* __restrict__ partial) {
    constexpr float inv_c = 1.0f / (256.0f * NV);
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r0 = w * rpw;             // (a wave beyond the last row adds zeros)
    float4 g4[NV], b4[NV], dg[NV], db[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g4[i] = ld4(gamma + i * 256 + lane * 4);
        b4[i] = ld4(beta + i * 256 + lane * 4);
        dg[i] = db[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the rows of this wave in groups of four, a group's loads requested together (one row at a time ran at the latency of
    // its loads)
    for (int h = 0; h < rpw / 4; ++h) {
    const int64_t rh = r0 + 4 * h;
    if (rh >= rows) break;
    float4 vr[4][NV], dr[4][NV];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = rh + q < rows ? rh + q : rows - 1;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            vr[q][i] = ld4(x + r * ldx + i * 256 + lane * 4);
            dr[q][i] = ld4(dy + r * lddy + i * 256 + lane * 4);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = rh + q;
        if (r >= rows) break;
        float4 v[NV], d[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = vr[q][i];
            d[i] = dr[q][i];
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
        const float mean = vrd::wave_sum(s) * inv_c;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
            ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
        const float rstd = 1.0f / sqrtf(vrd::wave_sum(ss) * inv_c + LN_EPS);
        float sg = 0.f, sgx = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float* xh = reinterpret_cast<float*>(&v[i]);
            float* dd = reinterpret_cast<float*>(&d[i]);
            const float* gg = reinterpret_cast<const float*>(&g4[i]);
            const float* bb = reinterpret_cast<const float*>(&b4[i]);
            float* pdg = reinterpret_cast<float*>(&dg[i]);
            float* pdb = reinterpret_cast<float*>(&db[i]);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                xh[c] *= rstd;
                if (relu && fmaf(xh[c], gg[c], bb[c]) <= 0.f) dd[c] = 0.f;
                pdg[c] = fmaf(dd[c], xh[c], pdg[c]);
                pdb[c] += dd[c];
                dd[c] *= gg[c];
                sg += dd[c];
                sgx = fmaf(dd[c], xh[c], sgx);
            }
        }
        const float mg = vrd::wave_sum(sg) * inv_c, mgx = vrd::wave_sum(sgx) * inv_c;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4 o;
            o.x = rstd * (d[i].x - mg - v[i].x * mgx);
            o.y = rstd * (d[i].y - mg - v[i].y * mgx);
            o.z = rstd * (d[i].z - mg - v[i].z * mgx);
            o.w = rstd * (d[i].w - mg - v[i].w * mgx);
            st4(dx + r * lddx + i * 256 + lane * 4, o);
        }
    }
    }       // groups of four rows
    // the four waves of the block add their partial sums in LDS; one atomic per channel and BLOCK (the atomics on the 2 C
    // addresses were what the kernel spent its time on)
    __shared__ float4 red[2][3][NV][64];
    const int wv = threadIdx.x >> 6;
    if (wv > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[0][wv - 1][i][lane] = dg[i], red[1][wv - 1][i][lane] = db[i];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4 g = dg[i], b = db[i];
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const float4 pg = red[0][o][i][lane], pb = red[1][o][i][lane];
                g.x += pg.x, g.y += pg.y, g.z += pg.z, g.w += pg.w;
                b.x += pb.x, b.y += pb.y, b.z += pb.z, b.w += pb.w;
            }
            if (partial) {       // the block's row of the (blocks, 2 C) partial sums: colpartial_reduce_kernel adds them up
                float* pp = partial + (int64_t)blockIdx.x * (2 * 256 * NV) + i * 256 + lane * 4;
                st4(pp, g);
                st4(pp + 256 * NV, b);
                continue;
            }
            float* dgp = dgamma + i * 256 + lane * 4;
            float* dbp = dbeta + i * 256 + lane * 4;
            atomicAdd(dgp + 0, g.x), atomicAdd(dgp + 1, g.y), atomicAdd(dgp + 2, g.z), atomicAdd(dgp + 3, g.w);
            atomicAdd(dbp + 0, b.x), atomicAdd(dbp + 1, b.y), atomicAdd(dbp + 2, b.z), atomicAdd(dbp + 3, b.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// depthwise conv, input gradient.  Forward: D_o[b, to, c] = mask[b, to] * (bias + sum_{g,k} w_o[c,g,k] *
// xin[b, s*to + k - ks/2, gin*c + g]),  xin = x (+ x_up[b, t/2]).  Hence
//   dxin[b, ti, gin*c+g] = sum_o sum_k [to = (ti - k + ks/2) / s integral, in range] mask[b,to] dD_o[b,to,c] w_o[c,g,k]
// thread = one input element (b, ti, cin); with dx_up the thread owns the input pair (2 tu, 2 tu + 1) and also writes
// their sum (gradient of the nearest x2 upsample).
// ------------------------------------------------------------------------------------------------------------------
struct DwBwdArgs {
    const float* dD[3];
    int64_t lddd[3];
    const float* w[3];
    int n_out, B, Tin, C, ksize, stride, gin;
    const uint8_t* mask_out;
    float* dx;
    int64_t lddx;
    float* dx_up;
    int64_t lddx_up;
};
// out0: the first output row of the element's sequence, Tin: its input frames
__device__ __forceinline__ float dw_bwd_elem(const DwBwdArgs& p, int64_t out0, int Tin, int ti, int cin) {
    const int c = cin / p.gin, g = cin - c * p.gin;
    const int Tout = Tin / p.stride;
    float s = 0.f;
    for (int k = 0; k < p.ksize; ++k) {
        const int tn = ti - k + p.ksize / 2;
        if (tn < 0 || tn % p.stride) continue;
        const int to = tn / p.stride;
        if (to >= Tout) continue;
        const int64_t row = out0 + to;
        if (p.mask_out && !p.mask_out[row]) continue;
        for (int o = 0; o < p.n_out; ++o) s = fmaf(p.dD[o][row * p.lddd[o] + c], p.w[o][(c * p.gin + g) * p.ksize + k], s);
    }
    return s;
}
// The common case -- k = 3, stride 1, one input per group, no upsample branch, C % 4 == 0 -- with four channels per thread:
// dx[b, ti, c] = sum_o sum_k m[b, ti + 1 - k] dD_o[b, ti + 1 - k, c] w_o[c, k]: three rows x n_out float4 of dD and 3 n_out float4
// of weights (a channel's taps are contiguous: 12 floats for 4 channels) per 4 outputs.  The element-per-thread form below spends
// ~100 instructions per element on index arithmetic and scalar loads and ran at 3.2 TB/s of its traffic.
// SEGS (vrd_dwconv_bwd_segs, both kernels): the threads count the input frames (with dx_up: the frame pairs) of the groups of `sg`
// in order; a frame's rows are those of its group (input rows from row[g] on, output rows from row[g] / stride, x_up rows from
// row[g] / 2), and nothing else is read or written.  B and Tin of `p` are unused.
template <int NOUT, bool SEGS = false>
__global__ __launch_bounds__(256) void dwconv_bwd_vec_kernel(DwBwdArgs p, const vrd::RowSegArg<SEGS> sg) {
    const int C4 = p.C / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t r = idx / C4;
    const int c = (int)(idx - r * C4) * 4;
    int ti;
    if constexpr (SEGS) {
        int g, b;
        if (C4 % 64 == 0) r = vrd::wave_uniform(r);          // (a wave's 64 threads then lie in one row)
        if (!vrd::seg_find(sg, r, g, b, ti)) return;
        p.Tin = sg.T[g];
        r = sg.row[g] + (int64_t)b * p.Tin + ti;
    } else {
        if (idx >= (int64_t)p.B * p.Tin * C4) return;
        ti = (int)(r % p.Tin);
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 w[NOUT][3];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int q = 0; q < 3; ++q) w[o][q] = ld4(p.w[o] + (int64_t)c * 3 + 4 * q);       // w[c .. c+3][0 .. 2], row-major
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int to = ti + 1 - k;
        if (to < 0 || to >= p.Tin) continue;
        const int64_t row = r + 1 - k;
        if (p.mask_out && !p.mask_out[row]) continue;
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            const float4 d = ld4(p.dD[o] + row * p.lddd[o] + c);
            const float* wf = reinterpret_cast<const float*>(&w[o][0]);          // wf[3 * ch + k]
            acc.x = fmaf(d.x, wf[k], acc.x);
            acc.y = fmaf(d.y, wf[3 + k], acc.y);
            acc.z = fmaf(d.z, wf[6 + k], acc.z);
            acc.w = fmaf(d.w, wf[9 + k], acc.w);
        }
    }
    st4(p.dx + r * p.lddx + c, acc);
}

template <bool SEGS = false>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(DwBwdArgs p, const vrd::RowSegArg<SEGS> sg) {
    const int Cin = p.C * p.gin;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cin = (int)(idx % Cin);
    if (p.dx_up) {
        int64_t ru = idx / Cin;                   // the frame pair: its x_up row
        int64_t in0, out0;                        // first input / output row of its sequence
        int tu;
        if constexpr (SEGS) {
            int g, b;
            if (Cin % 64 == 0) ru = vrd::wave_uniform(ru);
            if (!vrd::seg_find(sg, ru, g, b, tu)) return;            // (the table counts T / 2 frame pairs per sequence)
            p.Tin = sg.T[g];
            in0 = sg.row[g] + (int64_t)b * p.Tin;
            out0 = sg.row[g] / p.stride + (int64_t)b * (p.Tin / p.stride);
            ru = sg.row[g] / 2 + (int64_t)b * (p.Tin / 2) + tu;
        } else {
            if (idx >= (int64_t)p.B * (p.Tin / 2) * Cin) return;
            const int b = (int)(ru / (p.Tin / 2));
            tu = (int)(ru - (int64_t)b * (p.Tin / 2));
            in0 = (int64_t)b * p.Tin, out0 = (int64_t)b * (p.Tin / p.stride);
        }
        const float g0 = dw_bwd_elem(p, out0, p.Tin, 2 * tu, cin), g1 = dw_bwd_elem(p, out0, p.Tin, 2 * tu + 1, cin);
        p.dx[(in0 + 2 * tu) * p.lddx + cin] = g0;
        p.dx[(in0 + 2 * tu + 1) * p.lddx + cin] = g1;
        p.dx_up[ru * p.lddx_up + cin] = g0 + g1;
        return;
    }
    int64_t r = idx / Cin, out0;
    int ti;
    if constexpr (SEGS) {
        int g, b;
        if (Cin % 64 == 0) r = vrd::wave_uniform(r);
        if (!vrd::seg_find(sg, r, g, b, ti)) return;
        p.Tin = sg.T[g];
        r = sg.row[g] + (int64_t)b * p.Tin + ti;
        out0 = sg.row[g] / p.stride + (int64_t)b * (p.Tin / p.stride);
    } else {
        if (idx >= (int64_t)p.B * p.Tin * Cin) return;
        const int b = (int)(r / p.Tin);
        ti = (int)(r - (int64_t)b * p.Tin);
        out0 = (int64_t)b * (p.Tin / p.stride);
    }
    p.dx[r * p.lddx + cin] = dw_bwd_elem(p, out0, p.Tin, ti, cin);
}

// ------------------------------------------------------------------------------------------------------------------
// global attention backward, scores: one wave per (b, h, tq).  P = softmax_j(scale q.k_j | kv_mask (masked: -inf)),
// dP_j = dO . v_j, dS = P * (dP - sum P dP).  Lane j handles keys j, j + 64, ...; q and dO rows sit in LDS.
// (models/local_transformer.py:163-183; the predictor's 9-query attention :44-63 runs through the same kernel)
// ------------------------------------------------------------------------------------------------------------------
constexpr int AB_HD_MAX = 128, AB_TK_MAX = 1024;
__global__ __launch_bounds__(256) void attn_bwd_probs_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                             const float* __restrict__ v, int64_t ldkv,
                                                             const float* __restrict__ dO, int64_t lddo,
                                                             const uint8_t* __restrict__ kv_mask, int B, int Tq, int Tk, int H,
                                                             int hd, float scale, float* __restrict__ P, float* __restrict__ dS) {
    __shared__ float qs[4][AB_HD_MAX], os[4][AB_HD_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;          // (b, h, tq)
    const bool live = w < (int64_t)B * H * Tq;
    const int tq = live ? (int)(w % Tq) : 0;
    const int h = live ? (int)((w / Tq) % H) : 0;
    const int b = live ? (int)(w / ((int64_t)Tq * H)) : 0;
    if (live)
        for (int d = lane; d < hd; d += 64) {
            qs[wave][d] = q[((int64_t)b * Tq + tq) * ldq + h * hd + d] * scale;
            os[wave][d] = dO[((int64_t)b * Tq + tq) * lddo + h * hd + d];
        }
    __syncthreads();
    if (!live) return;
    constexpr int NJ = AB_TK_MAX / 64;
    float s[NJ], dp[NJ];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = lane + 64 * i;
        s[i] = -INFINITY;
        dp[i] = 0.f;
        if (j >= Tk) continue;
        if (kv_mask && !kv_mask[(int64_t)b * Tk + j]) continue;
        const float* kr = k + ((int64_t)b * Tk + j) * ldkv + h * hd;
        const float* vr = v + ((int64_t)b * Tk + j) * ldkv + h * hd;
        float a = 0.f, c = 0.f;
        for (int d = 0; d < hd; d += 4) {
            const float4 kk = ld4(kr + d), vv = ld4(vr + d);
            a += qs[wave][d] * kk.x + qs[wave][d + 1] * kk.y + qs[wave][d + 2] * kk.z + qs[wave][d + 3] * kk.w;
            c += os[wave][d] * vv.x + os[wave][d + 1] * vv.y + os[wave][d + 2] * vv.z + os[wave][d + 3] * vv.w;
        }
        s[i] = a;
        dp[i] = c;
        m = fmaxf(m, a);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float den = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        s[i] = (m == -INFINITY || s[i] == -INFINITY) ? 0.f : __expf(s[i] - m);
        den += s[i];
    }
    den = vrd::wave_sum(den);
    const float inv = den > 0.f ? 1.0f / den : 0.f;
    float dsum = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) { s[i] *= inv; dsum = fmaf(s[i], dp[i], dsum); }
    dsum = vrd::wave_sum(dsum);
    float* const Pr = P + w * Tk;
    float* const dSr = dS + w * Tk;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = lane + 64 * i;
        if (j < Tk) { Pr[j] = s[i]; dSr[j] = s[i] * (dp[i] - dsum); }
    }
}

// C[z][i][n] (= or +=) alpha * sum_k A[z][i][k] * B[z][k][n];  z = (z0, z1) with z1 < Z1; every operand addressed by
// (offset of z0, offset of z1, stride of the row index, stride of the column index), in floats.  thread = (i, n), n
// fastest: choose the operand roles so that B and C are contiguous along n.  K loop in registers, no staging.
struct BmmArgs {
    const float *A, *B;
    float* C;
    int64_t a0, a1, ai, ak;
    int64_t b0, b1, bk, bn;
    int64_t c0, c1, ci, cn;
    int Z0, Z1, M, N, K;
    float alpha;
    int accumulate;
};
__global__ __launch_bounds__(256) void bmm_kernel(BmmArgs p) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int z = blockIdx.z;
    if (n >= p.N || i >= p.M) return;
    const int z0 = z / p.Z1, z1 = z - z0 * p.Z1;
    const float* a = p.A + z0 * p.a0 + z1 * p.a1 + i * p.ai;
    const float* b = p.B + z0 * p.b0 + z1 * p.b1 + n * p.bn;
    float s = 0.f;
    // eight k at a time with their loads requested together (same summation order; one k per iteration ran at the latency
    // of its two loads)
    int k = 0;
    for (; k + 8 <= p.K; k += 8) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            av[u] = a[(k + u) * p.ak];
            bv[u] = b[(k + u) * p.bk];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(av[u], bv[u], s);
    }
    for (; k < p.K; ++k) s = fmaf(a[k * p.ak], b[k * p.bk], s);
    float* c = p.C + z0 * p.c0 + z1 * p.c1 + i * p.ci + n * p.cn;
    *c = p.accumulate ? *c + p.alpha * s : p.alpha * s;
}

// The same product on the matrix cores, exact f32 (v_mfma_f32_32x32x2_f32: an fmaf chain per output, k ascending) -- round 3:
// at vidor.yaml's training sizes (48 pairs x 512 frames x 8 heads) the three products of the attention backward were
// 40 ms of a 150 ms step on the kernel above (one thread per output, every operand element re-read per thread).
// Workgroup = 4 waves = a 64 x 64 tile of C, one 32 x 32 accumulator per wave; K steps of 16 through k-major LDS tiles
// (a lane's operand of one MFMA is A[k][row] / B[k][col]: 32 consecutive floats per half-wave, conflict free).  An operand is
// read along whichever of its two indices has stride 1 (four elements per thread and K step, 16-byte loads when the launch's
// pointers and strides allow); anything goes through the scalar gather.  The next K step's elements are in registers while
// the current one multiplies.
typedef __attribute__((ext_vector_type(16))) float bmm_f32x16;
constexpr int BM_T = 64, BM_K = 16, BM_LD = BM_T + 4;
template <bool VEC>
__global__ __launch_bounds__(256) void bmm_mfma_kernel(BmmArgs p) {
    __shared__ float As[BM_K][BM_LD], Bs[BM_K][BM_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int z = blockIdx.z, z0 = z / p.Z1, z1 = z - z0 * p.Z1;
    const int i0 = blockIdx.y * BM_T, n0 = blockIdx.x * BM_T;
    const float* A = p.A + z0 * p.a0 + z1 * p.a1;
    const float* Bm = p.B + z0 * p.b0 + z1 * p.b1;
    // staging roles: "along k" = thread (row t / 4, four consecutive k), "along the row" = thread (k t / 16, four consecutive rows)
    const bool a_k = p.ak == 1, b_n = p.bn == 1;
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
        if (a_k) {                    // A[i][k], k contiguous
            const int r = tid >> 2, kq = (tid & 3) * 4;
            const float* src = A + (int64_t)(i0 + r) * p.ai + (k0 + kq);
            if (VEC && i0 + r < p.M && k0 + kq + 3 < p.K) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                ra[0] = t.x, ra[1] = t.y, ra[2] = t.z, ra[3] = t.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) ra[u] = (i0 + r < p.M && k0 + kq + u < p.K) ? src[u] : 0.f;
            }
        } else {                      // rows contiguous (or a general stride): thread (k, four rows)
            const int k = tid >> 4, rq = (tid & 15) * 4;
            const float* src = A + (int64_t)(k0 + k) * p.ak + (int64_t)(i0 + rq) * p.ai;
            if (VEC && p.ai == 1 && k0 + k < p.K && i0 + rq + 3 < p.M) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                ra[0] = t.x, ra[1] = t.y, ra[2] = t.z, ra[3] = t.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) ra[u] = (k0 + k < p.K && i0 + rq + u < p.M) ? src[u * p.ai] : 0.f;
            }
        }
        if (b_n) {                    // B[k][n], n contiguous: thread (k, four columns)
            const int k = tid >> 4, cq = (tid & 15) * 4;
            const float* src = Bm + (int64_t)(k0 + k) * p.bk + (n0 + cq);
            if (VEC && k0 + k < p.K && n0 + cq + 3 < p.N) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                rb[0] = t.x, rb[1] = t.y, rb[2] = t.z, rb[3] = t.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) rb[u] = (k0 + k < p.K && n0 + cq + u < p.N) ? src[u] : 0.f;
            }
        } else {                      // k contiguous (B given transposed) or general: thread (column, four k)
            const int c = tid >> 2, kq = (tid & 3) * 4;
            const float* src = Bm + (int64_t)(n0 + c) * p.bn + (int64_t)(k0 + kq) * p.bk;
            if (VEC && p.bk == 1 && n0 + c < p.N && k0 + kq + 3 < p.K) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                rb[0] = t.x, rb[1] = t.y, rb[2] = t.z, rb[3] = t.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) rb[u] = (n0 + c < p.N && k0 + kq + u < p.K) ? src[u * p.bk] : 0.f;
            }
        }
    };
    auto stage = [&]() {
        if (a_k) {
            const int r = tid >> 2, kq = (tid & 3) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) As[kq + u][r] = ra[u];
        } else {
            const int k = tid >> 4, rq = (tid & 15) * 4;
            *reinterpret_cast<float4*>(&As[k][rq]) = make_float4(ra[0], ra[1], ra[2], ra[3]);
        }
        if (b_n) {
            const int k = tid >> 4, cq = (tid & 15) * 4;
            *reinterpret_cast<float4*>(&Bs[k][cq]) = make_float4(rb[0], rb[1], rb[2], rb[3]);
        } else {
            const int c = tid >> 2, kq = (tid & 3) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) Bs[kq + u][c] = rb[u];
        }
    };
    bmm_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < p.K; k0 += BM_K) {
        __syncthreads();                              // everybody is done reading the previous tiles
        stage();
        __syncthreads();
        if (k0 + BM_K < p.K) fetch(k0 + BM_K);
#pragma unroll
        for (int kk = 0; kk < BM_K / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * kk + lh][wm * 32 + li], Bs[2 * kk + lh][wn * 32 + li], acc, 0, 0, 0);
    }
    // accumulator register e of lane (li, lh): row (e & 3) + 8 * (e >> 2) + 4 * lh, column li
    float* C = p.C + z0 * p.c0 + z1 * p.c1;
    const int n = n0 + wn * 32 + li;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = i0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (i < p.M && n < p.N) {
            float* c = C + (int64_t)i * p.ci + (int64_t)n * p.cn;
            *c = p.accumulate ? *c + p.alpha * acc[e] : p.alpha * acc[e];
        }
    }
}

// Global attention backward on matrices (round 3): S = scale * Q K^T and dP = dO V^T come from two vrd_bmm products; this
// kernel turns a row of each into P = softmax_j(S | kv_mask (masked: 0)) and dS = P * (dP - sum_j P dP), in place.
// One wave per (b, h, tq) row, lanes over the keys (Tk <= 1024: 16 per lane in registers).
__global__ __launch_bounds__(256) void attn_bwd_softmax_kernel(float* __restrict__ P, float* __restrict__ dS, const uint8_t* __restrict__ kv_mask,
                                                               int64_t rows, int Tq, int Tk, int H) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= rows) return;
    const int b = (int)(w / ((int64_t)Tq * H));
    constexpr int NJ = AB_TK_MAX / 64;
    float s[NJ], dp[NJ];
    float* const Pr = P + w * Tk;
    float* const dSr = dS + w * Tk;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = lane + 64 * i;
        s[i] = -INFINITY;
        dp[i] = 0.f;
        if (j >= Tk || (kv_mask && !kv_mask[(int64_t)b * Tk + j])) continue;
        s[i] = Pr[j];
        dp[i] = dSr[j];
        m = fmaxf(m, s[i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float den = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        s[i] = (m == -INFINITY || s[i] == -INFINITY) ? 0.f : __expf(s[i] - m);
        den += s[i];
    }
    den = vrd::wave_sum(den);
    const float inv = den > 0.f ? 1.0f / den : 0.f;
    float dsum = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) { s[i] *= inv; dsum = fmaf(s[i], dp[i], dsum); }
    dsum = vrd::wave_sum(dsum);
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = lane + 64 * i;
        if (j < Tk) { Pr[j] = s[i]; dSr[j] = s[i] * (dp[i] - dsum); }
    }
}

// MaxPool1d(3, 2, 1)(x) * mask[::2] backward: dx[b, ti, c] = sum over the (1 or 2) windows holding ti in which ti is the
// FIRST maximum (ATen's tie rule) of mask[2 to] * dy[b, to, c]
// SEGS (vrd_maxpool_bwd_segs): the threads count the input frames of the groups of `sg` in order; group g's x / mask / dx rows start
// at row[g], its dy rows at row[g] / 2.  B and Tin are unused.
template <bool SEGS = false>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ dy,
                                                          int64_t lddy, int B, int Tin, int C, const uint8_t* __restrict__ mask_in,
                                                          float* __restrict__ dx, int64_t lddx, const vrd::RowSegArg<SEGS> sg) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(idx % C);
    int64_t r = idx / C, in0, out0;               // the frame's row; first input / output row of its sequence
    int ti;
    if constexpr (SEGS) {
        int g, b;
        if (C % 64 == 0) r = vrd::wave_uniform(r);
        if (!vrd::seg_find(sg, r, g, b, ti)) return;
        Tin = sg.T[g];
        in0 = sg.row[g] + (int64_t)b * Tin;
        out0 = sg.row[g] / 2 + (int64_t)b * (Tin / 2);
        r = in0 + ti;
    } else {
        if (idx >= (int64_t)B * Tin * C) return;
        const int b = (int)(r / Tin);
        ti = (int)(r - (int64_t)b * Tin);
        in0 = (int64_t)b * Tin, out0 = (int64_t)b * (Tin / 2);
    }
    const int Tout = Tin / 2;
    const float xv = x[r * ldx + c];
    float g = 0.f;
    // windows: to with 2 to - 1 <= ti <= 2 to + 1
    for (int to = (ti + 1) / 2 - ((ti & 1) ? 1 : 0); to <= (ti + 1) / 2; ++to) {
        if (to < 0 || to >= Tout) continue;
        if (!mask_in[in0 + 2 * to]) continue;
        bool first_max = true;
        for (int tt = 2 * to - 1; tt <= 2 * to + 1; ++tt) {
            if (tt < 0 || tt >= Tin || tt == ti) continue;
            const float o = x[(in0 + tt) * ldx + c];
            if (o > xv || (o == xv && tt < ti)) first_max = false;
        }
        if (first_max) g += dy[(out0 + to) * lddy + c];
    }
    dx[r * lddx + c] = g;
}

}  // namespace

extern "C" {

int vrd_rowcol_scale(const float* v, int64_t ldv, int64_t rows, int C, const float* col_scale, const float* row_scale,
                     const uint8_t* row_mask, const float* res, int64_t ldres, int res_masked, const float* res2, int64_t ldres2,
                     float* out, int64_t ldo, void* stream) {
    VRD_CHECK_ARG(v && out && rows > 0 && C > 0 && C % 4 == 0, "vrd_rowcol_scale: bad arguments (C %% 4 == 0 required)");
    VRD_CHECK_ARG(ldv >= C && ldo >= C && ldv % 4 == 0 && ldo % 4 == 0 && aligned16(v) && aligned16(out) && aligned16(col_scale),
                  "vrd_rowcol_scale: rows must be 16-byte aligned");
    VRD_CHECK_ARG(!res || (ldres >= C && ldres % 4 == 0 && aligned16(res)), "vrd_rowcol_scale: bad res layout");
    VRD_CHECK_ARG(!res2 || (ldres2 >= C && ldres2 % 4 == 0 && aligned16(res2)), "vrd_rowcol_scale: bad res2 layout");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)rows * C * (2 + (res ? 1 : 0) + (res2 ? 1 : 0)));
    const int64_t n = rows * (C / 4);
    hipLaunchKernelGGL(rowcol_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, ldv, rows, C / 4, col_scale, row_scale,
                       row_mask, res, ldres, res_masked, res2, ldres2, out, ldo);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_activation(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t rows, int C, int act, float* out, int64_t ldo,
            void* stream) {
    VRD_CHECK_ARG(x && out && rows > 0 && C > 0 && C % 4 == 0, "vrd_activation: bad arguments (C %% 4 == 0 required)");
    VRD_CHECK_ARG(act == VRD_ACT_RELU || act == VRD_ACT_GELU, "vrd_activation: activation must be ReLU or GELU");
    VRD_CHECK_ARG(ldx >= C && ldo >= C && ldx % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(out), "vrd_activation: bad layout");
    VRD_CHECK_ARG(!dy || (lddy >= C && lddy % 4 == 0 && aligned16(dy)), "vrd_activation: bad dy layout");
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)rows * C * (dy ? 3 : 2));
    const int64_t n = rows * (C / 4);
    hipLaunchKernelGGL(act_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, dy, lddy, rows, C / 4, act, out, ldo);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_layernorm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t rows, int C, const float* gamma,
                      const float* beta, int relu, float* dx, int64_t lddx, float* dgamma, float* dbeta, float* scratch,
                      int64_t scratch_floats, void* stream, int flags) {
    VRD_CHECK_ARG(x && dy && gamma && beta && dx && dgamma && dbeta, "vrd_layernorm_bwd: null pointer");
    VRD_CHECK_ARG(C == 256 || C == 512, "vrd_layernorm_bwd: C must be 256 or 512 (got %d)", C);
    VRD_CHECK_ARG(ldx >= C && lddy >= C && lddx >= C && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && aligned16(x) && aligned16(dy) &&
                      aligned16(dx) && aligned16(gamma) && aligned16(beta),
                  "vrd_layernorm_bwd: rows must be 16-byte aligned");
    VRD_CHECK_FLAGS("vrd_layernorm_bwd");
    const bool det = flags & VRD_DETERMINISTIC;
    if (rows <= 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t rpw = (rows / (4 * 512) + 3) / 4 * 4;            // ~512 blocks on long inputs; a multiple of 4 rows, 8 .. 64
    if (rpw < LNB_ROWS) rpw = LNB_ROWS;
    if (rpw > 64) rpw = 64;
    const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)));
    // the blocks' column sums as (blocks, 2 C) rows of partial sums, then their reduction: always in the deterministic mode; in
    // the default mode with more than 32 blocks when the scratch holds them (else one atomic per channel and block)
    const vrd::PartialRows pr = vrd::place_partial_rows(0, grid.x, 2 * C, det);
    const bool partials = det || (grid.x > 32 && vrd::scratch_holds(scratch, scratch_floats, pr.end));
    if (det)
        if (int rc = vrd::check_det_scratch("vrd_layernorm_bwd", scratch, scratch_floats, pr.end)) return rc;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 12.0 * (double)rows * C);
    float* partial = partials ? scratch + pr.rows_off : nullptr;
    auto kern = C == 256 ? layernorm_bwd_kernel<1> : layernorm_bwd_kernel<2>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, x, ldx, dy, lddy, rows, gamma, beta, relu, dx, lddx, dgamma, dbeta, (int)rpw, partial);
    VRD_LAUNCH_CHECK();
    return partials ? vrd::reduce_partial_rows(scratch, pr, dgamma, dbeta, C, det, s) : 0;
}

// segs: NULL, or the row groups of vrd_dwconv_bwd_segs (a->B and a->Tin are then unused)
static int dwconv_bwd_launch(const vrd_dwconv_bwd_args* a, const vrd_row_segs* segs, void* stream) {
    VRD_CHECK_ARG(a && a->dx, "vrd_dwconv_bwd: null args");
    VRD_CHECK_ARG(a->n_out >= 1 && a->n_out <= 3 && a->C > 0 && (segs || (a->B > 0 && a->Tin > 0)), "vrd_dwconv_bwd: bad sizes");
    VRD_CHECK_ARG((a->ksize == 1 || a->ksize == 3) && (a->stride == 1 || a->stride == 2) && (a->group_in == 1 || a->group_in == 2) &&
                      (segs || a->Tin % a->stride == 0),
                  "vrd_dwconv_bwd: ksize 1/3, stride 1/2, group_in 1/2, Tin %% stride == 0");
    VRD_CHECK_ARG(!a->dx_up || ((segs || a->Tin % 2 == 0) && a->lddx_up >= (int64_t)a->C * a->group_in), "vrd_dwconv_bwd: bad dx_up");
    VRD_CHECK_ARG(a->lddx >= (int64_t)a->C * a->group_in, "vrd_dwconv_bwd: lddx too small");
    // the rules of vrd_dwconv_ln_args.segs: T[i] % stride == 0, row[i] even when x_up or stride 2 is used.  The table counts what a
    // thread owns: input frames, or with dx_up pairs of them
    vrd::SegTable sg;
    int64_t units = 0;
    if (segs) {
        const int even = (a->dx_up || a->stride == 2) ? 2 : 1;
        units = vrd::seg_table(sg, segs, a->dx_up ? 2 : 1, 1);
        VRD_CHECK_ARG(units > 0, "vrd_dwconv_bwd_segs: bad row groups (1..%d groups, T %% %d == 0)", VRD_MAX_SEGS, even);
        for (int g = 0; g < segs->count; ++g)
            VRD_CHECK_ARG(segs->T[g] % even == 0 && segs->row[g] % even == 0, "vrd_dwconv_bwd_segs: group %d: T and row must be even", g);
    }
    DwBwdArgs p{};
    for (int o = 0; o < a->n_out; ++o) {
        VRD_CHECK_ARG(a->dD[o] && a->w[o] && a->lddd[o] >= a->C, "vrd_dwconv_bwd: bad set %d", o);
        p.dD[o] = a->dD[o], p.lddd[o] = a->lddd[o], p.w[o] = a->w[o];
    }
    p.n_out = a->n_out, p.B = a->B, p.Tin = a->Tin, p.C = a->C, p.ksize = a->ksize, p.stride = a->stride, p.gin = a->group_in;
    p.mask_out = a->mask_out, p.dx = a->dx, p.lddx = a->lddx, p.dx_up = a->dx_up, p.lddx_up = a->lddx_up;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (segs ? units : (int64_t)a->B * (a->dx_up ? a->Tin / 2 : a->Tin)) * a->C * a->group_in;
    const double in_rows = segs ? (double)units * (a->dx_up ? 2 : 1) : (double)a->B * a->Tin;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * in_rows * a->C * (a->group_in + a->n_out));
    bool vec = a->ksize == 3 && a->stride == 1 && a->group_in == 1 && !a->dx_up && a->C % 4 == 0 && a->lddx % 4 == 0 && aligned16(a->dx);
    for (int o = 0; o < a->n_out; ++o) vec = vec && a->lddd[o] % 4 == 0 && aligned16(a->dD[o]) && aligned16(a->w[o]);
    if (vec) {
        const dim3 grid((unsigned)((n / 4 + 255) / 256));
        vrd::pick_of(vrd::IntList<1, 2, 3>{}, a->n_out, [&](auto NOUT) {
            if (segs) hipLaunchKernelGGL((dwconv_bwd_vec_kernel<decltype(NOUT)::value, true>), grid, dim3(256), 0, s, p, sg);
            else hipLaunchKernelGGL((dwconv_bwd_vec_kernel<decltype(NOUT)::value>), grid, dim3(256), 0, s, p, vrd::NoRowSegs{});
        });
    } else if (segs) {
        hipLaunchKernelGGL(dwconv_bwd_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, sg);
    } else {
        hipLaunchKernelGGL(dwconv_bwd_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, vrd::NoRowSegs{});
    }
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_dwconv_bwd(const vrd_dwconv_bwd_args* a, void* stream) { return dwconv_bwd_launch(a, nullptr, stream); }

int vrd_dwconv_bwd_segs(const vrd_dwconv_bwd_args* a, const vrd_row_segs* segs, void* stream) {
    VRD_CHECK_ARG(segs, "vrd_dwconv_bwd_segs: null row groups");
    return dwconv_bwd_launch(a, segs, stream);
}

int vrd_attn_bwd_probs(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* dO, int64_t lddo,
                       const uint8_t* kv_mask, int B, int Tq, int Tk, int n_head, int head_dim, float* P, float* dS, void* stream) {
    VRD_CHECK_ARG(q && k && v && dO && P && dS, "vrd_attn_bwd_probs: null pointer");
    VRD_CHECK_ARG(B > 0 && Tq > 0 && Tk > 0 && Tk <= AB_TK_MAX && n_head > 0 && head_dim > 0 && head_dim <= AB_HD_MAX && head_dim % 4 == 0,
                  "vrd_attn_bwd_probs: Tk <= %d, head_dim <= %d and %% 4 == 0 (got Tk %d, head_dim %d)", AB_TK_MAX, AB_HD_MAX, Tk, head_dim);
    VRD_CHECK_ARG(ldkv % 4 == 0 && aligned16(k) && aligned16(v), "vrd_attn_bwd_probs: k / v rows must be 16-byte aligned");
    VRD_CHECK_ARG(ldq >= (int64_t)n_head * head_dim && ldkv >= (int64_t)n_head * head_dim && lddo >= (int64_t)n_head * head_dim,
                  "vrd_attn_bwd_probs: leading dimension too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * n_head * Tq;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 4.0 * (double)n * Tk * head_dim, 8.0 * (double)n * Tk);
    hipLaunchKernelGGL(attn_bwd_probs_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, q, ldq, k, v, ldkv, dO, lddo, kv_mask, B, Tq, Tk,
                       n_head, head_dim, 1.0f / sqrtf((float)head_dim), P, dS);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_bmm(const vrd_bmm_args* a, void* stream) {
    VRD_CHECK_ARG(a && a->A && a->B && a->C, "vrd_bmm: null pointer");
    VRD_CHECK_ARG(a->Z0 > 0 && a->Z1 > 0 && a->M > 0 && a->N > 0 && a->K > 0 && (int64_t)a->Z0 * a->Z1 <= 65535 && (a->M + 3) / 4 <= 65535,
                  "vrd_bmm: bad sizes");
    BmmArgs p;
    p.A = a->A, p.B = a->B, p.C = a->C;
    p.a0 = a->a_z0, p.a1 = a->a_z1, p.ai = a->a_row, p.ak = a->a_col;
    p.b0 = a->b_z0, p.b1 = a->b_z1, p.bk = a->b_row, p.bn = a->b_col;
    p.c0 = a->c_z0, p.c1 = a->c_z1, p.ci = a->c_row, p.cn = a->c_col;
    p.Z0 = a->Z0, p.Z1 = a->Z1, p.M = a->M, p.N = a->N, p.K = a->K, p.alpha = a->alpha, p.accumulate = a->accumulate;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 2.0 * a->Z0 * a->Z1 * (double)a->M * a->N * a->K, 0.0);
    // matrix-core tiles once a 64 x 64 tile is at least a quarter full and K fills an LDS step (the predictor's 9-query
    // attention and the mask head's Q-row products stay on the one-thread-per-output kernel: a tile would be mostly padding)
    static const int mfma_env = [] { const char* e = getenv("VRD_BMM_MFMA"); return e ? atoi(e) : 1; }();
    if (mfma_env && a->M >= 32 && a->N >= 32 && a->K >= 16 && (a->M + 63) / 64 <= 65535) {
        auto al = [](const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; };
        auto m4 = [](int64_t v) { return v % 4 == 0; };
        // 16-byte loads: bases aligned and every stride that is not the unit one a multiple of 4 floats
        const bool vec = al(a->A) && al(a->B) && m4(a->a_z0) && m4(a->a_z1) && m4(a->b_z0) && m4(a->b_z1) &&
                         (a->a_col == 1 ? m4(a->a_row) : a->a_row == 1 && m4(a->a_col)) &&
                         (a->b_col == 1 ? m4(a->b_row) : a->b_row == 1 && m4(a->b_col));
        const dim3 grid((a->N + 63) / 64, (a->M + 63) / 64, a->Z0 * a->Z1);
        if (vec) hipLaunchKernelGGL(bmm_mfma_kernel<true>, grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL(bmm_mfma_kernel<false>, grid, dim3(256), 0, s, p);
    } else {
        hipLaunchKernelGGL(bmm_kernel, dim3((a->N + 63) / 64, (a->M + 3) / 4, a->Z0 * a->Z1), dim3(256), 0, s, p);
    }
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_attn_bwd_softmax(float* P, float* dS, const uint8_t* kv_mask, int B, int Tq, int Tk, int n_head, void* stream) {
    VRD_CHECK_ARG(P && dS && B > 0 && Tq > 0 && Tk > 0 && Tk <= AB_TK_MAX && n_head > 0, "vrd_attn_bwd_softmax: bad arguments (Tk <= %d)", AB_TK_MAX);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * n_head * Tq;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 16.0 * (double)n * Tk);
    hipLaunchKernelGGL(attn_bwd_softmax_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, P, dS, kv_mask, n, Tq, Tk, n_head);
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_maxpool_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, int B, int Tin, int C, const uint8_t* mask_in, float* dx,
                    int64_t lddx, void* stream) {
    VRD_CHECK_ARG(x && dy && mask_in && dx && B > 0 && Tin > 0 && Tin % 2 == 0 && C > 0, "vrd_maxpool_bwd: bad arguments");
    VRD_CHECK_ARG(ldx >= C && lddy >= C && lddx >= C, "vrd_maxpool_bwd: leading dimension too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * Tin * C;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)n * 2.5);
    hipLaunchKernelGGL(maxpool_bwd_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, dy, lddy, B, Tin, C, mask_in, dx,
                       lddx, vrd::NoRowSegs{});
    VRD_LAUNCH_CHECK();
    return 0;
}

int vrd_maxpool_bwd_segs(const float* x, int64_t ldx, const float* dy, int64_t lddy, const vrd_row_segs* segs, int C, const uint8_t* mask_in,
                         float* dx, int64_t lddx, void* stream) {
    VRD_CHECK_ARG(x && dy && mask_in && dx && segs && C > 0, "vrd_maxpool_bwd_segs: bad arguments");
    VRD_CHECK_ARG(ldx >= C && lddy >= C && lddx >= C, "vrd_maxpool_bwd_segs: leading dimension too small");
    vrd::SegTable sg;
    const int64_t rows = vrd::seg_table(sg, segs, 1, 1);
    VRD_CHECK_ARG(rows > 0, "vrd_maxpool_bwd_segs: bad row groups (1..%d groups)", VRD_MAX_SEGS);
    for (int g = 0; g < segs->count; ++g)
        VRD_CHECK_ARG(segs->T[g] % 2 == 0 && segs->row[g] % 2 == 0, "vrd_maxpool_bwd_segs: group %d: T and row must be even", g);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = rows * C;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)n * 2.5);
    hipLaunchKernelGGL(maxpool_bwd_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, dy, lddy, 0, 0, C, mask_in, dx, lddx,
                       sg);
    VRD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
