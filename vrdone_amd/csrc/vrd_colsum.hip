// Column sums over the rows of the training step's activations: the bias, drop-path-scale and depthwise-conv-weight gradients,
// and the reduction of per-block partial sums that every parameter-gradient kernel shares (vrd_grad_scratch.h).  f32 throughout;
// sums are ACCUMULATED (+=) into caller-zeroed buffers.  Default mode: one float atomic per column and block, or -- with a
// scratch buffer and enough row blocks -- rows of partial sums and one reducing launch.  VRD_DETERMINISTIC: always rows of
// partial sums, added up in index order by a fixed tree (reduce_partial_rows); the form is chosen by the shapes alone (DET / A16
// template arguments below; the atomics that remain sit in the !DET branches).
//
//  vrd_colsum            out[c] += sum_r a[r,c] * b[s*r+shift, c*bc+bo] * mask[r] * rscale[r]
//  vrd_dwconv_wgrad      weight and bias gradient of a depthwise conv in one pass over dD
//  vrd_dwconv_wgrad_segs the same with the rows as groups of sequences (vrd_row_segs): the sums run over all groups
//  vrd_scratch_required  floats of scratch the last refused deterministic call of this thread asked for
#include "vrd_grad_scratch.h"

namespace {

using vrd::aligned16;
using vrd::ld4;
using vrd::st4;

// out[c] += sum_p partial[p * cols + c]: the per-block column sums of a kernel whose blocks would otherwise each end in one
// atomic per column (atomics on one address are worked off one after the other, ~50 ns each: 512 blocks = 25 us).  Block =
// 64 columns x 32 partial rows (a wave takes eight of them), one atomic per column and block: parts / 32 per address.
// DET: no atomics -- with one row of blocks the sum is added to out, otherwise it becomes row blockIdx.y of `next`, which the
// next launch of the chain reduces the same way (reduce_partial_rows): the tree is fixed by `parts` alone.
template <bool DET>
__global__ __launch_bounds__(256) void colpartial_reduce_kernel(const float* __restrict__ partial, int parts, int cols,
                                                                float* __restrict__ out0, float* __restrict__ out1, int split,
                                                                float* __restrict__ next) {
    __shared__ float red[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int p0 = blockIdx.y * 32 + wave * 8;
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (c < cols && p0 + q < parts) ? partial[(int64_t)(p0 + q) * cols + c] : 0.f;
    float s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    if (wave > 0) red[wave - 1][lane] = s;
    __syncthreads();
    if (wave == 0 && c < cols) {
        s += red[0][lane] + red[1][lane] + red[2][lane];
        if (!DET) atomicAdd(c < split ? out0 + c : out1 + (c - split), s);
        else if (gridDim.y == 1) *(c < split ? out0 + c : out1 + (c - split)) += s;
        else next[(int64_t)blockIdx.y * cols + c] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// out[c] += sum_r a[r, c] * (b ? b[brow(r), c * bc + bo] : 1) * (mask ? mask[r] : 1) * (rscale ? rscale[r] : 1)
// brow(r): r = s * T + t  ->  s * (bs * T) + bs * t + shift, contributing only if 0 <= bs * t + shift < bs * T.
// block = rpb rows x 64 columns, a quarter of the rows per wave, one atomic per column and block: atomics on one address queue up
// behind each other in L2 (~50 ns each), and with 32 rows per atomic a 49 k-row input put 1,536 of them on every output element.
// ------------------------------------------------------------------------------------------------------------------
// DET: the block's sums become row blockIdx.x of `partial` (gridDim.x x C) instead, for reduce_partial_rows.
constexpr int CS_ROWS = 32;      // smallest rows-per-block
template <bool DET>
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                     int64_t ldb, int bc, int bo, int bs, int shift, int T,
                                                     const uint8_t* __restrict__ mask, const float* __restrict__ rscale,
                                                     int64_t rows, int C, int rpb, float* __restrict__ out, float* __restrict__ partial) {
    __shared__ float red[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool col_ok = c < C;
    const int wrows = rpb / 4;                   // (rpb is a multiple of 32)
    const int64_t r0 = (int64_t)blockIdx.x * rpb + (int64_t)wave * wrows;
    const int64_t r1 = r0 + wrows < rows ? r0 + wrows : rows;
    // eight rows per iteration with their loads requested together (one row per iteration ran at the latency of its loads);
    // the row's (sequence, position) pair is carried along instead of a 64-bit division per row
    int64_t seq = b ? r0 / T : 0;
    int tpos = b ? (int)(r0 - seq * T) : 0;
    float s = 0.f;
    for (int64_t rb = r0; rb < r1; rb += 8) {
        float av[8], bv[8], fv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t r = rb + u;
            bool live = col_ok && r < r1 && (!mask || mask[r]);
            av[u] = 0.f, bv[u] = 1.f, fv[u] = 1.f;
            if (b) {
                int tq = tpos + u;
                int64_t sq = seq;
                while (tq >= T) tq -= T, ++sq;
                const int tb = bs * tq + shift;
                live = live && tb >= 0 && tb < bs * T;
                if (live) bv[u] = b[(sq * (int64_t)bs * T + tb) * ldb + (int64_t)c * bc + bo];
            }
            if (live) {
                av[u] = a[r * lda + c];
                if (rscale) fv[u] = rscale[r];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(av[u] * fv[u], bv[u], s);
        if (b) {
            tpos += 8;
            while (tpos >= T) tpos -= T, ++seq;
        }
    }
    // the four waves (four row ranges of the same 64 columns) add up in LDS: one atomic per column and block
    if (wave > 0) red[wave - 1][lane] = s;
    __syncthreads();
    if (wave == 0 && col_ok) {
        if (DET) partial[(int64_t)blockIdx.x * C + c] = s + red[0][lane] + red[1][lane] + red[2][lane];
        else atomicAdd(out + c, s + red[0][lane] + red[1][lane] + red[2][lane]);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Weight and bias gradient of a depthwise conv (k = 1 / 3, stride bs, gin inputs per group) in ONE pass over dD:
//   dw[c, g, kk] += sum_r dD[r, c] * m[r] * x[brow(r, kk), c * gin + g],   dbias[c] += sum_r dD[r, c] * m[r]
// (dw in the parameter's own (C, gin, k) layout)
// (vrd_colsum computes one (g, kk) per launch: twelve launches and twelve passes over dD per q / k / v convolution triple).
// block = rpb rows x 64 columns, a quarter of the rows per wave (as vrd_colsum); one atomic per column, output and block.
// DET: row blockIdx.x of `partial` (gridDim.x x (C * GIN * KS [+ C])) instead: dw's layout, then the bias.
// ------------------------------------------------------------------------------------------------------------------
// SEGS (vrd_dwconv_wgrad_segs, both kernels): `rows` counts the OUTPUT frames of the groups of `sg` in order (the table is built
// over T[g] / bs frames per sequence); a frame's dD / mask row and its input rows are those of its group (output rows from
// row[g] / bs on, input rows from row[g]), and the sequence ends that bound the taps are the group's.  T is unused.
// seg_rows: the dD / mask row and the sequence's first input row and input frames at the cursor c.
__device__ __forceinline__ void seg_rows(const vrd::SegTable& sg, const vrd::SegCursor& c, int bs, int64_t& out_row, int64_t& in0, int& Tin) {
    const int g = c.g < sg.count ? c.g : sg.count - 1;        // (behind the last frame: a row nobody reads)
    Tin = sg.T[g];
    in0 = sg.row[g] + (int64_t)c.b * Tin;
    out_row = sg.row[g] / bs + (int64_t)c.b * sg.sps[g] + c.t;
}
template <int KS, int GIN, bool DET, bool SEGS = false>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ x,
                                                           int64_t ldx, int bs, int T, const uint8_t* __restrict__ mask,
                                                           int64_t rows, int C, int rpb, float* __restrict__ dw,
                                                           float* __restrict__ dbias, float* __restrict__ partial,
                                                           const vrd::RowSegArg<SEGS> sg) {
    __shared__ float red[3][GIN * KS + 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool col_ok = c < C;
    const int wrows = rpb / 4;
    const int64_t r0 = (int64_t)blockIdx.x * rpb + (int64_t)wave * wrows;
    const int64_t r1 = r0 + wrows < rows ? r0 + wrows : rows;
    int64_t seq = 0;
    int tpos = 0;
    vrd::SegCursor cur{0, 0, 0};
    if constexpr (SEGS) {
        if (r0 < r1) vrd::seg_find(sg, vrd::wave_uniform(r0), cur.g, cur.b, cur.t);          // (r0 is the wave's)
    } else {
        seq = r0 / T;
        tpos = (int)(r0 - seq * T);
    }
    float sw[GIN][KS], sb = 0.f;
#pragma unroll
    for (int g = 0; g < GIN; ++g)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) sw[g][kk] = 0.f;
    for (int64_t rb = r0; rb < r1; rb += 4) {
        float av[4], xv[4][GIN][KS];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int64_t r = rb + u, in0;
            int tq, Tin;
            if constexpr (SEGS) {
                vrd::SegCursor cu = cur;
                vrd::seg_step(sg, cu, u);
                const bool in_range = r < r1;
                seg_rows(sg, cu, bs, r, in0, Tin);
                tq = cu.t;
                if (!in_range) r = -1;
            } else {
                tq = tpos + u;
                int64_t sq = seq;
                while (tq >= T) tq -= T, ++sq;
                in0 = sq * (int64_t)bs * T, Tin = bs * T;
                if (r >= r1) r = -1;
            }
            const bool live = col_ok && r >= 0 && (!mask || mask[r]);
            av[u] = live ? a[r * lda + c] : 0.f;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int tb = bs * tq + kk - KS / 2;
                const bool ok = live && tb >= 0 && tb < Tin;
#pragma unroll
                for (int g = 0; g < GIN; ++g) xv[u][g][kk] = ok ? x[(in0 + tb) * ldx + (int64_t)c * GIN + g] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sb += av[u];
#pragma unroll
            for (int g = 0; g < GIN; ++g)
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) sw[g][kk] = fmaf(av[u], xv[u][g][kk], sw[g][kk]);
        }
        if constexpr (SEGS) {
            vrd::seg_step(sg, cur, 4);
        } else {
            tpos += 4;
            while (tpos >= T) tpos -= T, ++seq;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int g = 0; g < GIN; ++g)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) red[wave - 1][g * KS + kk][lane] = sw[g][kk];
        red[wave - 1][GIN * KS][lane] = sb;
    }
    __syncthreads();
    if (wave > 0 || !col_ok) return;
    if (DET) {
        float* pw = partial + (int64_t)blockIdx.x * ((int64_t)C * (GIN * KS) + (dbias ? C : 0));
#pragma unroll
        for (int g = 0; g < GIN; ++g)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk)
                pw[(int64_t)c * (GIN * KS) + g * KS + kk] = sw[g][kk] + red[0][g * KS + kk][lane] + red[1][g * KS + kk][lane] + red[2][g * KS + kk][lane];
        if (dbias) pw[(int64_t)C * (GIN * KS) + c] = sb + red[0][GIN * KS][lane] + red[1][GIN * KS][lane] + red[2][GIN * KS][lane];
        return;
    }
#pragma unroll
    for (int g = 0; g < GIN; ++g)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
            atomicAdd(dw + (int64_t)c * (GIN * KS) + g * KS + kk, sw[g][kk] + red[0][g * KS + kk][lane] + red[1][g * KS + kk][lane] + red[2][g * KS + kk][lane]);
    if (dbias) atomicAdd(dbias + c, sb + red[0][GIN * KS][lane] + red[1][GIN * KS][lane] + red[2][GIN * KS][lane]);
}

// ------------------------------------------------------------------------------------------------------------------
// The two column-sum kernels above with four channels per lane (float4 rows: 1 KiB per wave and row instead of 256 B) for their
// common cases, and the row blocks' sums as rows of `partial` for colpartial_reduce_kernel (nullable: then one atomic per column
// and block as above).  Block = rpb rows x 256 columns, a quarter of the rows per wave, four rows' loads in flight.
//   colsum_vec_kernel:        out[c] += sum_r a[r, c] * (b ? b[r, c] : 1) * m[r] * rs[r]        (b on the rows of a)
//   dwconv_wgrad_vec_kernel:  k = 3, one input per group: dw[c, kk] += sum_r dD[r, c] m[r] x[in_row(r, kk), c]; dbias[c] += ...
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fma4(float4& s, const float4& a, const float4& b) {
    s.x = fmaf(a.x, b.x, s.x), s.y = fmaf(a.y, b.y, s.y), s.z = fmaf(a.z, b.z, s.z), s.w = fmaf(a.w, b.w, s.w);
}
__device__ __forceinline__ void add4(float4& s, const float4& a) { s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w; }
// A16 = false (deterministic mode, rows that are float4-shaped but not 16-byte aligned): the same four floats as four loads, so
// the form -- and its summation tree -- depends on the shapes alone
template <bool A16>
__device__ __forceinline__ float4 ldv4(const float* p) {
    if (A16) return ld4(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

template <bool A16>
__global__ __launch_bounds__(256) void colsum_vec_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                                                         const uint8_t* __restrict__ mask, const float* __restrict__ rscale,
                                                         int64_t rows, int C, int rpb, float* __restrict__ out,
                                                         float* __restrict__ partial) {
    __shared__ float4 red[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 256 + lane * 4;
    const bool col_ok = c < C;
    const int wrows = rpb / 4;                   // (rpb is a multiple of 16)
    const int64_t r0 = (int64_t)blockIdx.x * rpb + (int64_t)wave * wrows;
    const int64_t r1 = r0 + wrows < rows ? r0 + wrows : rows;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f), one = make_float4(1.f, 1.f, 1.f, 1.f);
    float4 s = zero;
    for (int64_t rb = r0; rb < r1; rb += 4) {
        float4 av[4], bv[4];
        float fv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = rb + u;
            const bool live = col_ok && r < r1 && (!mask || mask[r]);
            av[u] = live ? ldv4<A16>(a + r * lda + c) : zero;
            bv[u] = live && b ? ldv4<A16>(b + r * ldb + c) : one;
            fv[u] = live && rscale ? rscale[r] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            av[u].x *= fv[u], av[u].y *= fv[u], av[u].z *= fv[u], av[u].w *= fv[u];
            fma4(s, av[u], bv[u]);
        }
    }
    if (wave > 0) red[wave - 1][lane] = s;
    __syncthreads();
    if (wave == 0 && col_ok) {
        add4(s, red[0][lane]), add4(s, red[1][lane]), add4(s, red[2][lane]);
        if (partial) st4(partial + (int64_t)blockIdx.x * C + c, s);
        else atomicAdd(out + c, s.x), atomicAdd(out + c + 1, s.y), atomicAdd(out + c + 2, s.z), atomicAdd(out + c + 3, s.w);
    }
}

template <bool A16, bool SEGS = false>
__global__ __launch_bounds__(256) void dwconv_wgrad_vec_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ x,
                                                               int64_t ldx, int bs, int T, const uint8_t* __restrict__ mask,
                                                               int64_t rows, int C, int rpb, float* __restrict__ dw,
                                                               float* __restrict__ dbias, float* __restrict__ partial,
                                                               const vrd::RowSegArg<SEGS> sg) {
    __shared__ float4 red[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 256 + lane * 4;
    const bool col_ok = c < C;
    const int wrows = rpb / 4;
    const int64_t r0 = (int64_t)blockIdx.x * rpb + (int64_t)wave * wrows;
    const int64_t r1 = r0 + wrows < rows ? r0 + wrows : rows;
    int64_t seq = 0;
    int tpos = 0;
    vrd::SegCursor cur{0, 0, 0};
    if constexpr (SEGS) {
        if (r0 < r1) vrd::seg_find(sg, vrd::wave_uniform(r0), cur.g, cur.b, cur.t);          // (r0 is the wave's)
    } else {
        seq = r0 / T;
        tpos = (int)(r0 - seq * T);
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 sw[3] = {zero, zero, zero}, sb = zero;         // sw[kk] = the four channels' sums of tap kk
    for (int64_t rb = r0; rb < r1; rb += 4) {
        float4 av[4], xv[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int64_t r = rb + u, in0;
            int tq, Tin;
            if constexpr (SEGS) {
                vrd::SegCursor cu = cur;
                vrd::seg_step(sg, cu, u);
                const bool in_range = r < r1;
                seg_rows(sg, cu, bs, r, in0, Tin);
                tq = cu.t;
                if (!in_range) r = -1;
            } else {
                tq = tpos + u;
                int64_t sq = seq;
                while (tq >= T) tq -= T, ++sq;
                in0 = sq * (int64_t)bs * T, Tin = bs * T;
                if (r >= r1) r = -1;
            }
            const bool live = col_ok && r >= 0 && (!mask || mask[r]);
            av[u] = live ? ldv4<A16>(a + r * lda + c) : zero;
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const int tb = bs * tq + kk - 1;
                const bool ok = live && tb >= 0 && tb < Tin;
                xv[u][kk] = ok ? ldv4<A16>(x + (in0 + tb) * ldx + c) : zero;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            add4(sb, av[u]);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) fma4(sw[kk], av[u], xv[u][kk]);
        }
        if constexpr (SEGS) {
            vrd::seg_step(sg, cur, 4);
        } else {
            tpos += 4;
            while (tpos >= T) tpos -= T, ++seq;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) red[wave - 1][kk][lane] = sw[kk];
        red[wave - 1][3][lane] = sb;
    }
    __syncthreads();
    if (wave > 0 || !col_ok) return;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) add4(sw[kk], red[o][kk][lane]);
        add4(sb, red[o][3][lane]);
    }
    // dw is (C, 1, 3): the lane's four channels are twelve consecutive floats, channel-major
    const float o12[12] = {sw[0].x, sw[1].x, sw[2].x, sw[0].y, sw[1].y, sw[2].y, sw[0].z, sw[1].z, sw[2].z, sw[0].w, sw[1].w, sw[2].w};
    if (partial) {
        float* pw = partial + (int64_t)blockIdx.x * ((int64_t)C * 3 + (dbias ? C : 0));
#pragma unroll
        for (int q = 0; q < 3; ++q) st4(pw + (int64_t)c * 3 + 4 * q, make_float4(o12[4 * q], o12[4 * q + 1], o12[4 * q + 2], o12[4 * q + 3]));
        if (dbias) st4(pw + (int64_t)C * 3 + c, sb);
    } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) atomicAdd(dw + (int64_t)c * 3 + q, o12[q]);
        if (dbias) atomicAdd(dbias + c, sb.x), atomicAdd(dbias + c + 1, sb.y), atomicAdd(dbias + c + 2, sb.z), atomicAdd(dbias + c + 3, sb.w);
    }
}

}  // namespace

// rows per block of the column-sum kernels: ~1024 blocks on long inputs, a multiple of 32 (a quarter per wave, eight rows per
// iteration), 32 .. 2048
static int64_t colsum_rows_per_block(int64_t rows, int col_blocks) {
    int64_t rpb = rows * col_blocks / 1024;
    rpb = (rpb + 31) / 32 * 32;
    if (rpb < CS_ROWS) rpb = CS_ROWS;
    if (rpb > 2048) rpb = 2048;
    return rpb;
}

// rows per block of the four-channels-per-lane column-sum kernels: ~4 blocks per CU (16 waves: the loop is bound by the latency of
// its loads; 2 per CU: 1.67 ms per training step in dwconv_wgrad_vec_kernel, 4: 1.11, 8: 1.24), a multiple of 16 rows
static int64_t colsum_vec_rows_per_block(int64_t rows, int col_blocks) {
    int64_t row_blocks = 1024 / col_blocks;
    if (row_blocks < 1) row_blocks = 1;
    int64_t rpb = (rows + row_blocks - 1) / row_blocks;
    rpb = (rpb + 15) / 16 * 16;
    return rpb < 16 ? 16 : rpb;
}

// The plan of one column-sum launch.  vec: the float4 form -- the caller lets the operands' alignment have a say in the default
// mode and goes by the shapes alone in the deterministic mode; pcols: the columns of a row of partial sums; base: the first float
// of the scratch the launch may use.  Rows of partial sums: always in the deterministic mode; in the default mode from the
// float4 form with more than 8 row blocks, when the scratch holds them.
static vrd::ColsumPlan plan_colsum(int64_t rows, int C, int64_t pcols, bool vec, bool det, int64_t base, const float* scratch,
                                   int64_t scratch_floats) {
    vrd::ColsumPlan p;
    p.vec = vec;
    p.col_blocks = vec ? (C + 255) / 256 : (C + 63) / 64;
    p.rpb = (int)(vec ? colsum_vec_rows_per_block(rows, p.col_blocks) : colsum_rows_per_block(rows, p.col_blocks));
    p.row_blocks = (unsigned)((rows + p.rpb - 1) / p.rpb);
    p.pr = vrd::place_partial_rows(base, p.row_blocks, pcols, det);
    p.partials = det || (vec && p.row_blocks > 8 && vrd::scratch_holds(scratch, scratch_floats, p.pr.end));
    return p;
}

// the column-sum kernel of the plan and the reduction of its partial rows (a16: the operands of the float4 form are 16-byte aligned)
static int launch_colsum(const vrd::ColsumPlan& p, const float* a, int64_t lda, const float* b, int64_t ldb, int bc, int bo, int bs, int shift,
                         int T, const uint8_t* mask, const float* rscale, int64_t rows, int C, float* out, float* scratch, bool a16, bool det,
                         hipStream_t s) {
    const dim3 grid(p.row_blocks, p.col_blocks);
    float* partial = p.partials ? scratch + p.pr.rows_off : nullptr;
    if (p.vec) {
        auto kern = a16 ? colsum_vec_kernel<true> : colsum_vec_kernel<false>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, a, lda, b, ldb, mask, rscale, rows, C, p.rpb, out, partial);
    } else {
        auto kern = det ? colsum_kernel<true> : colsum_kernel<false>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, a, lda, b, ldb, bc, bo, bs, shift, T, mask, rscale, rows, C, p.rpb, out, partial);
    }
    VRD_LAUNCH_CHECK();
    return p.partials ? vrd::reduce_partial_rows(scratch, p.pr, out, nullptr, C, det, s) : 0;
}

template <bool DET, bool SEGS = false>
static auto dwconv_wgrad_for(int ksize, int group_in) -> decltype(&dwconv_wgrad_kernel<3, 1, DET, SEGS>) {
    if (ksize == 3) return group_in == 1 ? dwconv_wgrad_kernel<3, 1, DET, SEGS> : dwconv_wgrad_kernel<3, 2, DET, SEGS>;
    return group_in == 1 ? dwconv_wgrad_kernel<1, 1, DET, SEGS> : dwconv_wgrad_kernel<1, 2, DET, SEGS>;
}

static thread_local int64_t g_scratch_need = 0;

namespace vrd {

int check_det_scratch(const char* what, const float* scratch, int64_t scratch_floats, int64_t need) {
    if (need <= 0 || scratch_holds(scratch, scratch_floats, need)) return 0;
    g_scratch_need = need;
    set_error("%s: the deterministic mode needs %lld floats of 16-byte aligned scratch (got %lld)", what, (long long)need,
              (long long)(scratch ? scratch_floats : 0));
    return VRD_ERR_SCRATCH;
}

int reduce_partial_rows(float* scratch, const PartialRows& p, float* out0, float* out1, int split, bool det, hipStream_t s) {
    float* src = scratch + p.rows_off;
    float* dst = scratch + p.levels_off;
    auto kern = det ? colpartial_reduce_kernel<true> : colpartial_reduce_kernel<false>;
    for (int64_t parts = p.parts;;) {
        const int64_t gy = (parts + 31) / 32;
        hipLaunchKernelGGL(kern, dim3((unsigned)((p.cols + 63) / 64), (unsigned)gy), dim3(256), 0, s, src, (int)parts, p.cols, out0, out1, split, dst);
        VRD_LAUNCH_CHECK();
        if (gy == 1 || !det) return 0;   // (default mode: every block adds its sums atomically, `dst` is not written)
        src = dst;
        dst += gy * p.cols;              // (the next level: det_reduce_extra counts the same rows)
        parts = gy;
    }
}

// (the one-channel-per-lane kernel whatever the shape, and no partial rows in the default mode)
ColsumPlan plan_bias_colsum(int64_t M, int N, bool det, int64_t base) { return plan_colsum(M, N, N, false, det, base, nullptr, 0); }

int bias_colsum(const ColsumPlan& plan, const float* G, int64_t ldg, const uint8_t* row_mask, int64_t M, int N, float* dbias, float* scratch,
                bool det, hipStream_t s) {
    return launch_colsum(plan, G, ldg, nullptr, 0, 1, 0, 1, 0, 1, row_mask, nullptr, M, N, dbias, scratch, false, det, s);
}

}  // namespace vrd

extern "C" {

int vrd_scratch_required(int64_t* floats) {
    VRD_CHECK_ARG(floats, "vrd_scratch_required: null pointer");
    *floats = g_scratch_need;
    return 0;
}

// segs: NULL, or the INPUT rows' groups of vrd_dwconv_wgrad_segs (T and rows are then taken from the table)
static int dwconv_wgrad_launch(const float* dD, int64_t lddd, const float* x, int64_t ldx, int ksize, int stride, int group_in, int T,
                               const uint8_t* row_mask, int64_t rows, int C, float* dw, float* dbias, float* scratch,
                               int64_t scratch_floats, void* stream, int flags, const vrd_row_segs* segs) {
    vrd::SegTable sg;
    if (segs) {
        VRD_CHECK_ARG(stride >= 1, "vrd_dwconv_wgrad_segs: bad stride %d", stride);
        rows = vrd::seg_table(sg, segs, stride, 1);          // (output frames: T[g] / stride per sequence)
        VRD_CHECK_ARG(rows > 0, "vrd_dwconv_wgrad_segs: bad row groups (1..%d groups, T %% %d == 0)", VRD_MAX_SEGS, stride);
        for (int g = 0; g < segs->count; ++g)
            VRD_CHECK_ARG(segs->row[g] % stride == 0, "vrd_dwconv_wgrad_segs: group %d: row %% stride != 0", g);
        T = 1;
    }
    VRD_CHECK_ARG(dD && x && dw && rows > 0 && C > 0 && lddd >= C, "vrd_dwconv_wgrad: bad arguments");
    VRD_CHECK_ARG((ksize == 1 || ksize == 3) && (group_in == 1 || group_in == 2) && stride >= 1 && T > 0 && rows % T == 0,
                  "vrd_dwconv_wgrad: unsupported k=%d group_in=%d stride=%d T=%d rows=%lld", ksize, group_in, stride, T, (long long)rows);
    VRD_CHECK_FLAGS("vrd_dwconv_wgrad");
    const bool det = flags & VRD_DETERMINISTIC;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec_shape = ksize == 3 && group_in == 1 && C % 4 == 0 && lddd % 4 == 0 && ldx % 4 == 0;
    const bool a16 = aligned16(dD) && aligned16(x);
    // a row of partial sums: dw's layout, then the bias
    const int64_t wcols = (int64_t)C * group_in * ksize, pcols = wcols + (dbias ? C : 0);
    const vrd::ColsumPlan plan = plan_colsum(rows, C, pcols, vec_shape && (det || a16), det, 0, scratch, scratch_floats);
    if (det)
        if (int rc = vrd::check_det_scratch("vrd_dwconv_wgrad", scratch, scratch_floats, plan.total_floats())) return rc;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)rows * C * (1 + group_in * stride));
    const dim3 grid(plan.row_blocks, plan.col_blocks);
    float* partial = plan.partials ? scratch + plan.pr.rows_off : nullptr;
    if (segs) {
        auto kern = plan.vec ? (a16 ? dwconv_wgrad_vec_kernel<true, true> : dwconv_wgrad_vec_kernel<false, true>)
                             : (det ? dwconv_wgrad_for<true, true>(ksize, group_in) : dwconv_wgrad_for<false, true>(ksize, group_in));
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, dD, lddd, x, ldx, stride, T, row_mask, rows, C, plan.rpb, dw, dbias, partial, sg);
    } else {
        auto kern = plan.vec ? (a16 ? dwconv_wgrad_vec_kernel<true> : dwconv_wgrad_vec_kernel<false>)
                             : (det ? dwconv_wgrad_for<true>(ksize, group_in) : dwconv_wgrad_for<false>(ksize, group_in));
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, dD, lddd, x, ldx, stride, T, row_mask, rows, C, plan.rpb, dw, dbias, partial,
                           vrd::NoRowSegs{});
    }
    VRD_LAUNCH_CHECK();
    return plan.partials ? vrd::reduce_partial_rows(scratch, plan.pr, dw, dbias, (int)wcols, det, s) : 0;
}

int vrd_dwconv_wgrad(const float* dD, int64_t lddd, const float* x, int64_t ldx, int ksize, int stride, int group_in, int T,
                     const uint8_t* row_mask, int64_t rows, int C, float* dw, float* dbias, float* scratch, int64_t scratch_floats,
                     void* stream, int flags) {
    return dwconv_wgrad_launch(dD, lddd, x, ldx, ksize, stride, group_in, T, row_mask, rows, C, dw, dbias, scratch, scratch_floats, stream,
                               flags, nullptr);
}

int vrd_dwconv_wgrad_segs(const float* dD, int64_t lddd, const float* x, int64_t ldx, int ksize, int stride, int group_in,
                          const vrd_row_segs* segs, const uint8_t* row_mask, int C, float* dw, float* dbias, float* scratch,
                          int64_t scratch_floats, void* stream, int flags) {
    VRD_CHECK_ARG(segs, "vrd_dwconv_wgrad_segs: null row groups");
    return dwconv_wgrad_launch(dD, lddd, x, ldx, ksize, stride, group_in, 0, row_mask, 0, C, dw, dbias, scratch, scratch_floats, stream, flags,
                               segs);
}

int vrd_colsum(const float* a, int64_t lda, const float* b, int64_t ldb, int b_cstride, int b_coffset, int b_rstride, int shift,
               int T, const uint8_t* row_mask, const float* row_scale, int64_t rows, int C, float* out, float* scratch,
               int64_t scratch_floats, void* stream, int flags) {
    VRD_CHECK_ARG(a && out && rows > 0 && C > 0 && lda >= C, "vrd_colsum: bad arguments");
    VRD_CHECK_ARG(!b || (T > 0 && rows % T == 0 && b_cstride >= 1 && b_rstride >= 1 && b_coffset >= 0 && b_coffset < b_cstride),
                  "vrd_colsum: bad second operand (T=%d rows=%lld)", T, (long long)rows);
    VRD_CHECK_FLAGS("vrd_colsum");
    const bool det = flags & VRD_DETERMINISTIC;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool same_rows = !b || (b_cstride == 1 && b_coffset == 0 && b_rstride == 1 && shift == 0);
    const bool vec_shape = same_rows && C % 4 == 0 && lda % 4 == 0 && (!b || (ldb % 4 == 0 && ldb >= C));
    const bool a16 = aligned16(a) && (!b || aligned16(b));
    const vrd::ColsumPlan plan = plan_colsum(rows, C, C, vec_shape && (det || a16), det, 0, scratch, scratch_floats);
    if (det)
        if (int rc = vrd::check_det_scratch("vrd_colsum", scratch, scratch_floats, plan.total_floats())) return rc;
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 0.0, 4.0 * (double)rows * C * (b ? 2 : 1));
    return launch_colsum(plan, a, lda, b, ldb, b ? b_cstride : 1, b ? b_coffset : 0, b ? b_rstride : 1, shift, b ? T : 1, row_mask, row_scale,
                         rows, C, out, scratch, a16, det, s);
}

}  // extern "C"
