// Weight gradients of the dense convolutions (k = 1 / 3) of the relation-encoding path:
//   dW[n, tap*Cin+ci] += sum_r G[r,n] X[r+tap-1, ci]
// f32 accumulate, ACCUMULATED (+=) into caller-zeroed buffers.  The rows are split into chunks; default mode: the chunks' tiles
// are added with float atomics or -- with a scratch buffer -- stored as partial tiles and summed by a second launch.
// VRD_DETERMINISTIC: always partial tiles summed in chunk order, the chunking assumes a fixed DET_CUS compute units and no form
// is chosen by pointer alignment (DET template arguments below; the atomics that remain sit in the !DET branches).
//
//  vrd_gemm_wgrad      exact f32 products (f32 MFMA)
//  vrd_gemm_wgrad_x3   the forward path's split precision (bf16x3 / f16 planes), optionally with the bias gradient
#include "vrd_grad_scratch.h"
#include <cstdlib>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using vrd::aligned16;

using vrd::ld4;

// ------------------------------------------------------------------------------------------------------------------
// dW[n, j] += sum_{r in chunk} G[r, n] * X[r + tap(j) - taps/2, ci(j)],  j = tap*Cin + ci, rows outside the length-T
// sequence of r contribute 0.  One wave per 64 x 64 tile of dW and per chunk of rows: v_mfma_f32_32x32x2_f32 takes
// the two operands of two rows straight from global memory (a lane holds G[r0 + (lane >> 5)][n0 + (lane & 31)] and
// X[r0 + (lane >> 5) + shift][ci]: 128-byte row segments), accumulates in f32 and adds its partial tile atomically.
// ------------------------------------------------------------------------------------------------------------------
constexpr int WG_CHUNK = 128;      // rows per wave
constexpr int DET_CUS = 256;       // deterministic mode: the CU count every chunking assumes (a function of the shapes only)

// DET: with several row chunks dW is the (chunks, N, K) array of the blocks' partial tiles (summed by wgrad_reduce_kernel)
template <bool DET>
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ G, int64_t ldg, const float* __restrict__ X,
                                                    int64_t ldx, const uint8_t* __restrict__ row_mask, int64_t M, int N,
                                                    int Cin, int taps, int T, int tiles_k, float* __restrict__ dW) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = Cin * taps;
    const int tile = blockIdx.x;
    // a wave owns a 64 x 64 tile of dW as 2 x 2 accumulators: two G values and two X values per row feed four MFMAs (with
    // one 32 x 32 tile per wave every MFMA needed its own two loads and the kernel ran at the rate of its L2 traffic)
    const int n0 = (tile / tiles_k) * 64, j0 = (tile % tiles_k) * 64;
    const int li = lane & 31, lh = lane >> 5;
    int shift[2];
    const float* xp[2];
    const float* gp[2];
    bool a_col[2], b_col[2];
    const int64_t r_begin = ((int64_t)blockIdx.y * 4 + wave) * WG_CHUNK;
    const int64_t r_end = r_begin + WG_CHUNK < M ? r_begin + WG_CHUNK : M;        // (empty for a wave beyond the last row)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = n0 + 32 * h + li, j = j0 + 32 * h + li;
        const int tap = j < K ? j / Cin : 0;
        const int ci = j < K ? j - tap * Cin : 0;
        shift[h] = tap - taps / 2;
        a_col[h] = n < N, b_col[h] = j < K;
        gp[h] = G + (r_begin + lh) * ldg + n;
        xp[h] = X + (r_begin + lh + shift[h]) * ldx + ci;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int hn = 0; hn < 2; ++hn)
#pragma unroll
        for (int hj = 0; hj < 2; ++hj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[hn][hj][e] = 0.f;
    // eight rows (four row pairs) per iteration, all sixteen loads requested before the first MFMA: with one row pair per
    // iteration the loop ran at the latency of its loads (~900 cycles per MFMA on a 4.6 k-row training batch).
    // The position t of a row in its sequence (k = 3: zero padding at the sequence ends) is carried along instead of a
    // 64-bit modulo per row.
    int t = taps == 3 ? (int)((r_begin + lh) % T) : 0;          // position of row r0 + lh
    const uint8_t* mp = row_mask ? row_mask + r_begin + lh : nullptr;
    // (the loads of iteration i + 1 are requested before the MFMAs of iteration i: a small batch leaves ~1 wave per SIMD,
    // nothing else would cover their latency)
    auto fetch = [&](int64_t r0, float (&a)[4][2], float (&b)[4][2]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = r0 + 2 * u + lh < r_end;
            const bool live = in && (!mp || mp[2 * u]);
            int tt = 0;
            if (taps == 3) {
                tt = t + 2 * u;
                while (tt >= T) tt -= T;                        // (at most a few wraps: 8 rows, T >= 1)
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                a[u][h] = live && a_col[h] ? gp[h][(int64_t)(2 * u) * ldg] : 0.f;
                const bool ok = in && b_col[h] && (taps == 1 || (tt + shift[h] >= 0 && tt + shift[h] < T));
                b[u][h] = ok ? xp[h][(int64_t)(2 * u) * ldx] : 0.f;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) gp[h] += 8 * ldg, xp[h] += 8 * ldx;
        if (mp) mp += 8;
        if (taps == 3) {
            t += 8;
            while (t >= T) t -= T;
        }
    };
    float a0[4][2], b0[4][2], a1[4][2], b1[4][2];
    if (r_begin < r_end) fetch(r_begin, a0, b0);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += 16) {
        fetch(r0 + 8, a1, b1);                                  // (past r_end: zeros, no loads)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int hn = 0; hn < 2; ++hn)
#pragma unroll
                for (int hj = 0; hj < 2; ++hj) acc[hn][hj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u][hn], b0[u][hj], acc[hn][hj], 0, 0, 0);
        fetch(r0 + 16, a0, b0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int hn = 0; hn < 2; ++hn)
#pragma unroll
                for (int hj = 0; hj < 2; ++hj) acc[hn][hj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u][hn], b1[u][hj], acc[hn][hj], 0, 0, 0);
    }
    // the four waves of the block (four row chunks of the same tile) add up in LDS: one atomic per element and BLOCK, a
    // plain update when the block covers all rows
    __shared__ f32x16 red[3][4][64];
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][lane] = acc[q >> 1][q & 1];
    }
    __syncthreads();
    if (wave > 0) return;
    const bool single = gridDim.y == 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x16 v = acc[q >> 1][q & 1];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const f32x16 part = red[o][q][lane];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] += part[e];
        }
        // element e of lane (li, lh): row (e & 3) + 8 * (e >> 2) + 4 * lh (n index), column li (j index)
        const int j = j0 + 32 * (q & 1) + li;
        if (j >= K) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int nn = n0 + 32 * (q >> 1) + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (nn < N) {
                if (single) dW[(int64_t)nn * K + j] += v[e];         // (dW holds the caller's initial value: zeros)
                else if (DET) dW[((int64_t)blockIdx.y * N + nn) * K + j] = v[e];
                else atomicAdd(dW + (int64_t)nn * K + j, v[e]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The same contraction in the forward path's split precision (bf16x3): every product as g_lo x_hi + g_hi x_lo + g_hi x_hi on
// v_mfma_f32_32x32x16_bf16 (16 rows per MFMA instead of 2, at 8x the f32 MFMA rate: ~5x for three products), f32
// accumulate.  Same decomposition: a wave owns a 64 x 64 tile of dW for a chunk of rows and takes its operands straight
// from global memory in MFMA layout -- lane (m = lane & 31, half = lane >> 5) holds rows r0 + 8 half .. + 7 of column m:
// eight dword loads, each a 128-byte row segment per half-wave -- splits them into bf16 hi / lo in registers (24 vector
// instructions per eight values; four fragments feed twelve MFMAs) and accumulates.  The four waves of a block reduce in
// LDS as above.  Used in the bf16x3 mode only (vrd_gemm_wgrad_x3); gradients then carry ~2^-17 relative product error like
// the forward pass, the f32 mode keeps exact products.
// ------------------------------------------------------------------------------------------------------------------
// F16 (the f16x3 mode's backward): both operands as f16 planes of power-of-two multiples -- the gradient rows times gscale[0]
// (vrd_absmax_scale: max |g| lands in [2^13, 2^14)), the activation rows times 2^VRD_F16_ACT_EXP as in the forward pass (they went
// through a forward GEMM's range check) -- and the accumulators times gscale[1] * 2^-VRD_F16_ACT_EXP on the way out: ~22-bit
// products at the cost of the bf16 split's ~17.
using bf16x8 = vrd::bf16x8_t;
template <bool F16>
struct WFragT { typename vrd::SplitFmt<F16>::x8 h, l; };
template <bool F16>
__device__ __forceinline__ WFragT<F16> wsplit8(const float (&v)[8], float mul) {
    typedef typename vrd::SplitFmt<F16>::elem E;
    WFragT<F16> f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float y = F16 ? v[i] * mul : v[i];
        const E h = (E)y;
        f.h[i] = h;
        f.l[i] = (E)(y - (float)h);
    }
    return f;
}

template <bool F16, bool DET>
__global__ __launch_bounds__(256) void wgrad_x3_kernel(const float* __restrict__ G, int64_t ldg, const float* __restrict__ X,
                                                       int64_t ldx, const uint8_t* __restrict__ row_mask, int64_t M, int N,
                                                       int Cin, int taps, int T, int tiles_k, int chunk, float* __restrict__ dW,
                                                       const float* __restrict__ gscale) {
    const float gmul = F16 ? vrd::uniform_load(gscale) : 1.f;
    const float unscale = F16 ? vrd::uniform_load(gscale + 1) * vrd::F16_ACT_INV : 1.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = Cin * taps;
    const int tile = blockIdx.x;
    const int n0 = (tile / tiles_k) * 64, j0 = (tile % tiles_k) * 64;
    const int li = lane & 31, lh = lane >> 5;
    int shift[2];
    const float* xp[2];
    const float* gp[2];
    bool a_col[2], b_col[2];
    const int64_t r_begin = ((int64_t)blockIdx.y * 4 + wave) * chunk;
    const int64_t r_end = r_begin + chunk < M ? r_begin + chunk : M;              // (empty for a wave beyond the last row)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = n0 + 32 * h + li, j = j0 + 32 * h + li;
        const int tap = j < K ? j / Cin : 0;
        const int ci = j < K ? j - tap * Cin : 0;
        shift[h] = tap - taps / 2;
        a_col[h] = n < N, b_col[h] = j < K;
        gp[h] = G + (r_begin + 8 * lh) * ldg + n;
        xp[h] = X + (r_begin + 8 * lh + shift[h]) * ldx + ci;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int hn = 0; hn < 2; ++hn)
#pragma unroll
        for (int hj = 0; hj < 2; ++hj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[hn][hj][e] = 0.f;
    int t = taps == 3 ? (int)((r_begin + 8 * lh) % T) : 0;      // position of this lane's first row in its sequence
    const uint8_t* mp = row_mask ? row_mask + r_begin + 8 * lh : nullptr;
    // sixteen rows per step; the 32 loads of step i + 1 are requested before the MFMAs of step i
    auto fetch = [&](int64_t r0, float (&a)[2][8], float (&b)[2][8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool in = r0 + 8 * lh + i < r_end;
            const bool live = in && (!mp || mp[i]);
            int tt = 0;
            if (taps == 3) {
                tt = t + i;
                while (tt >= T) tt -= T;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                a[h][i] = live && a_col[h] ? gp[h][(int64_t)i * ldg] : 0.f;
                const bool ok = in && b_col[h] && (taps == 1 || (tt + shift[h] >= 0 && tt + shift[h] < T));
                b[h][i] = ok ? xp[h][(int64_t)i * ldx] : 0.f;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) gp[h] += 16 * ldg, xp[h] += 16 * ldx;
        if (mp) mp += 16;
        if (taps == 3) {
            t += 16;
            while (t >= T) t -= T;
        }
    };
    auto mac = [&](const float (&a)[2][8], const float (&b)[2][8]) {
        const WFragT<F16> fa0 = wsplit8<F16>(a[0], gmul), fa1 = wsplit8<F16>(a[1], gmul);
        const WFragT<F16> fb0 = wsplit8<F16>(b[0], vrd::F16_ACT_SCALE), fb1 = wsplit8<F16>(b[1], vrd::F16_ACT_SCALE);
#pragma unroll
        for (int hn = 0; hn < 2; ++hn)
#pragma unroll
            for (int hj = 0; hj < 2; ++hj) {
                const WFragT<F16>& fa = hn ? fa1 : fa0;
                const WFragT<F16>& fb = hj ? fb1 : fb0;
                acc[hn][hj] = vrd::mfma32(fa.l, fb.h, acc[hn][hj]);
                acc[hn][hj] = vrd::mfma32(fa.h, fb.l, acc[hn][hj]);
                acc[hn][hj] = vrd::mfma32(fa.h, fb.h, acc[hn][hj]);
            }
    };
    float a0[2][8], b0[2][8], a1[2][8], b1[2][8];
    if (r_begin < r_end) fetch(r_begin, a0, b0);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
        fetch(r0 + 16, a1, b1);                                 // (past r_end: zeros, no loads)
        mac(a0, b0);
        fetch(r0 + 32, a0, b0);
        mac(a1, b1);
    }
    __shared__ f32x16 red[3][4][64];
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][lane] = acc[q >> 1][q & 1];
    }
    __syncthreads();
    if (wave > 0) return;
    const bool single = gridDim.y == 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x16 v = acc[q >> 1][q & 1];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const f32x16 part = red[o][q][lane];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] += part[e];
        }
        const int j = j0 + 32 * (q & 1) + li;
        if (j >= K) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int nn = n0 + 32 * (q >> 1) + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (nn < N) {
                if (single) dW[(int64_t)nn * K + j] += v[e] * unscale;
                else if (DET) dW[((int64_t)blockIdx.y * N + nn) * K + j] = v[e] * unscale;      // (as in wgrad_kernel)
                else atomicAdd(dW + (int64_t)nn * K + j, v[e] * unscale);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The split-precision weight gradient with operand reuse: the wave-per-tile kernel above moves 8 KiB from L2 per twelve
// MFMAs (16 FLOP per byte: measured 150 TFLOP/s, the rate of its L2 traffic).  Here a block owns a TILE x TILE tile of dW for
// a chunk of rows; per step of 32 rows its threads load the 32 x TILE slabs of G and X once (four float4 each), split them
// into bf16 hi / lo and write four row-major planes into LDS (two stages, one barrier per step); each wave then forms its
// 64 x SJ sub-tile, taking the transposed fragments the MFMA wants -- eight consecutive ROWS of one column per lane --
// with ds_read_b64_tr_b16 (the read the attention kernels use for V^T; 16-byte chunks swizzled by row & 3).
//   BIG = 0: TILE 128, 4 waves x (64 x 64), two blocks per CU -- every input of >= 256 rows
//   BIG = 1: TILE 256, 8 waves x (64 x 128), one block per CU -- inputs with enough rows per chunk.  The kernel is bound by
//            its vector instructions, not by its MFMAs: the split costs ~3 instructions per element and wave, ~150 per wave
//            and step whatever the tile, against 24 MFMAs per wave and step at TILE 128 and 48 at TILE 256.
// float4 loads when N, Cin, ldg, ldx are multiples of 4 and the operands 16-byte aligned (a group of four columns then never
// straddles a tap), scalar loads otherwise; the wave kernel above serves inputs of fewer than 256 rows.
// ------------------------------------------------------------------------------------------------------------------
constexpr int WL_ROWS = 32;                 // rows per step

template <int BIG>
struct WlGeo {
    static constexpr int TILE = BIG ? 256 : 128;
    static constexpr int NTHR = BIG ? 512 : 256;
    static constexpr int CGS = TILE / 4;                // column groups (four floats) per slab row; NTHR / CGS = 8 rows per pass
    static constexpr int ROWB = TILE * 2;               // bytes per plane row
    static constexpr int PLANE = WL_ROWS * ROWB;
    static constexpr int STAGE = 4 * PLANE;             // g_hi | g_lo | x_hi | x_lo: 32 / 64 KiB
    static constexpr int SJ = BIG ? 128 : 64;           // a wave's sub-tile: 64 (n) x SJ (j)
};

typedef __attribute__((ext_vector_type(4))) short wl_s16x4;
typedef __attribute__((address_space(3))) wl_s16x4* wl_lds_s16x4_ptr;
typedef __attribute__((ext_vector_type(8))) short wl_s16x8;

// DET: `partial` is set whenever there are several chunks; the bias sums of several chunks then follow its chunks x N x K
// partial tiles as chunks x N rows
template <int BIG, bool VEC, int TAPS, bool F16, bool DET>
__global__ __launch_bounds__(WlGeo<BIG>::NTHR, BIG ? 1 : 2) void wgrad_x3_lds_kernel(
    const float* __restrict__ G, int64_t ldg, const float* __restrict__ X, int64_t ldx, const uint8_t* __restrict__ row_mask, int64_t M,
    int N, int Cin, int T, int tiles_k, int chunk, float* __restrict__ dW, float* __restrict__ dbias, float* __restrict__ partial,
    const float* __restrict__ gscale) {
    using Geo = WlGeo<BIG>;
    typedef typename vrd::SplitFmt<F16>::x4 e16x4;
    typedef typename vrd::SplitFmt<F16>::elem e16;
    const float gmul = F16 ? vrd::uniform_load(gscale) : 1.f;                                        // (see wgrad_x3_kernel)
    const float unscale = F16 ? vrd::uniform_load(gscale + 1) * vrd::F16_ACT_INV : 1.f;
    constexpr int TILE = Geo::TILE, ROWB = Geo::ROWB, PLANE = Geo::PLANE, STAGE = Geo::STAGE, SJ = Geo::SJ, NJ = SJ / 32;
    extern __shared__ __attribute__((aligned(16))) char lds[];          // 2 * STAGE
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = Cin * TAPS;
    // XCD-aware renumbering (as in the GEMM kernels): workgroups are dealt round-robin to the eight XCDs; a contiguous range of
    // (chunk, tile) ids per XCD keeps all tiles of a chunk -- which share its G and X slabs -- on one L2
    const int tiles = (int)gridDim.x, nwg = tiles * (int)gridDim.y, bid = (int)blockIdx.x + tiles * (int)blockIdx.y;
    const int xcd = bid & 7, xq = nwg >> 3, xrem = nwg & 7;
    const int lid = (xcd < xrem ? xcd * (xq + 1) : xrem * (xq + 1) + (xcd - xrem) * xq) + (bid >> 3);
    const int tile = lid % tiles, chunk_id = lid / tiles;
    const int n0 = (tile / tiles_k) * TILE, j0 = (tile % tiles_k) * TILE;
    const int64_t r_begin = (int64_t)chunk_id * chunk;
    const int64_t r_end = r_begin + chunk < M ? r_begin + chunk : M;
    // ---- loader: thread -> column group cg (4 columns) of both slabs, rows lr, lr + 8, lr + 16, lr + 24 of the step (BIG: a
    // wave is one slab row, so the row arithmetic is scalar).
    // VEC: float4 loads; otherwise four scalar loads per group, each column with its own tap.
    // Every fetch issues the same loads whatever the step looks like: rows past the end of the input and taps outside the
    // row's sequence read a valid address and are zeroed when the slab is written to LDS, and the row mask bytes come with the
    // slab instead of deciding its loads.  (The compiler counts vmcnt per path: with a path without loads, or a mask byte that
    // had to arrive before the row's load was issued, every wait was a vmcnt(0).)
    const int cg = tid % Geo::CGS;
    const int lr = BIG ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid / Geo::CGS;
    const int gn = n0 + 4 * cg, xj = j0 + 4 * cg;
    int g_ok[4], x_ok[4], shift[4], gcol[4];
    int64_t xoff[4];                             // element offset of column e's source inside row r of X: shift * ldx + ci
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        g_ok[e] = gn + e < N;
        x_ok[e] = xj + e < K;
        gcol[e] = g_ok[e] ? gn + e : 0;
        const int tap = x_ok[e] ? (xj + e) / Cin : 0;
        const int ci = x_ok[e] ? (xj + e) - tap * Cin : 0;
        shift[e] = tap - TAPS / 2;
        xoff[e] = (int64_t)shift[e] * ldx + ci;
    }
    const int step_t = WL_ROWS % T;              // what 32 rows add to a row's position in its sequence (k = 3)
    int tt[4] = {0, 0, 0, 0};                    // positions of the thread's four rows of the next fetch
    if (TAPS == 3) {
#pragma unroll
        for (int i = 0; i < 4; ++i) tt[i] = (int)((r_begin + lr + 8 * i) % T);
    }
    struct Slab {
        float4 g[4], x[4];
        int mk[4];               // row mask bytes
        int sq;                  // k = 3, bit 4 i + e: column e's tap of row i lies inside the row's sequence
    };
    const uint8_t* mbytes = row_mask ? row_mask : reinterpret_cast<const uint8_t*>(G);      // (any M readable bytes)
    const int64_t last = M - 1;
    int64_t frow = r_begin + lr;                 // the thread's first row of the next fetch
    // bias gradient on the way (the blocks of the first tile column only): column sums of the masked G slab this thread loads
    const bool do_bias = dbias != nullptr && tile % tiles_k == 0;                     // (block-uniform)
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](Slab& sl) {
        sl.sq = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t rr = frow + 8 * i;
            const int64_t rc = rr < last ? rr : last;
            sl.mk[i] = mbytes[rc];
            const float* gr = G + rc * ldg;
            const float* xr = X + rc * ldx;
            int sq[4] = {1, 1, 1, 1};
            if (TAPS == 3) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sq[e] = (unsigned)(tt[i] + shift[e]) < (unsigned)T && rr <= last;      // (a row past the input has no taps:
                                                                                           // row `last` + 1 is not memory)
                    sl.sq |= sq[e] << (4 * i + e);
                }
                const int nt = tt[i] + step_t;
                tt[i] = nt >= T ? nt - T : nt;
            }
            if (VEC) {
                sl.g[i] = ld4(gr + gcol[0]);
                sl.x[i] = ld4(xr + (x_ok[0] & sq[0] ? xoff[0] : 0));
            } else {
                sl.g[i].x = gr[gcol[0]];
                sl.g[i].y = gr[gcol[1]];
                sl.g[i].z = gr[gcol[2]];
                sl.g[i].w = gr[gcol[3]];
                sl.x[i].x = xr[x_ok[0] & sq[0] ? xoff[0] : 0];
                sl.x[i].y = xr[x_ok[1] & sq[1] ? xoff[1] : 0];
                sl.x[i].z = xr[x_ok[2] & sq[2] ? xoff[2] : 0];
                sl.x[i].w = xr[x_ok[3] & sq[3] ? xoff[3] : 0];
            }
        }
        frow += WL_ROWS;
    };
    auto put = [&](char* plane_hi, int row, float4 v, float mul) {
        if (F16) v.x *= mul, v.y *= mul, v.z *= mul, v.w *= mul;
        const e16x4 h = {(e16)v.x, (e16)v.y, (e16)v.z, (e16)v.w};
        const e16x4 l = {(e16)(v.x - (float)h[0]), (e16)(v.y - (float)h[1]), (e16)(v.z - (float)h[2]), (e16)(v.w - (float)h[3])};
        const int off = row * ROWB + (((cg >> 1) ^ ((row & 3) << 2)) * 16) + (cg & 1) * 8;
        *reinterpret_cast<e16x4*>(plane_hi + off) = h;
        *reinterpret_cast<e16x4*>(plane_hi + PLANE + off) = l;
    };
    // (a row contributes G[r, n] X[r', j]: zeroing G's row takes care of masked rows and of rows past the chunk -- their X values
    // are real rows of the input --, and columns of X at or beyond K only reach entries of dW that are never stored; what X
    // needs is the zero of a tap outside the row's sequence, and without float4 groups the zero of a column beyond K next to
    // valid ones is cheap enough to keep)
    auto store = [&](char* st, const Slab& sl, int64_t r0) {       // r0: the slab's first row
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int in = r0 + lr + 8 * i < r_end;
            const int live = in & (row_mask ? sl.mk[i] != 0 : 1);
            float4 g = sl.g[i], x = sl.x[i];
            g.x = live & g_ok[0] ? g.x : 0.f;
            g.y = live & g_ok[VEC ? 0 : 1] ? g.y : 0.f;
            g.z = live & g_ok[VEC ? 0 : 2] ? g.z : 0.f;
            g.w = live & g_ok[VEC ? 0 : 3] ? g.w : 0.f;
            if (TAPS == 3 || !VEC) {
                const int sq = TAPS == 3 ? sl.sq >> (4 * i) : 15;
                x.x = x_ok[0] & sq ? x.x : 0.f;
                x.y = x_ok[VEC ? 0 : 1] & (sq >> (VEC ? 0 : 1)) ? x.y : 0.f;
                x.z = x_ok[VEC ? 0 : 2] & (sq >> (VEC ? 0 : 2)) ? x.z : 0.f;
                x.w = x_ok[VEC ? 0 : 3] & (sq >> (VEC ? 0 : 3)) ? x.w : 0.f;
            }
            put(st, lr + 8 * i, g, gmul);
            put(st + 2 * PLANE, lr + 8 * i, x, vrd::F16_ACT_SCALE);
            if (do_bias) bsum.x += g.x, bsum.y += g.y, bsum.z += g.z, bsum.w += g.w;
        }
    };
    // ---- compute: wave (wn, wj) owns the 64 x SJ sub-tile at (64 wn, SJ wj) as 2 x NJ accumulators
    const int wn = wave >> 1, wj = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int vq = (lane >> 2) & 3, vp = lane & 3, vcol0 = 16 * ((lane >> 4) & 1) + 4 * vp;
    f32x16 acc[2][NJ];
#pragma unroll
    for (int hn = 0; hn < 2; ++hn)
#pragma unroll
        for (int hj = 0; hj < NJ; ++hj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[hn][hj][e] = 0.f;
    // fragment (k16 step s, 32 columns from colbase) of the plane pair at `pl`: lane (column lane & 31, half) <- rows 16 s + 8 half .. + 7
    auto frag = [&](const char* pl, int s, int colbase) {
        WFragT<F16> f;
        wl_s16x8 rh, rl;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const int row = 16 * s + 8 * part + 4 * lh + vq;
            const int col = colbase + vcol0;
            const int off = row * ROWB + ((((col * 2) >> 4) ^ ((row & 3) << 2)) * 16) + ((col * 2) & 15);
            const wl_s16x4 th = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wl_lds_s16x4_ptr)(pl + off));
            const wl_s16x4 tl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wl_lds_s16x4_ptr)(pl + PLANE + off));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rh[4 * part + q] = th[q];
                rl[4 * part + q] = tl[q];
            }
        }
        f.h = __builtin_bit_cast(typename vrd::SplitFmt<F16>::x8, rh);
        f.l = __builtin_bit_cast(typename vrd::SplitFmt<F16>::x8, rl);
        return f;
    };
    auto compute = [&](const char* st) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            WFragT<F16> fa[2], fb[NJ];
#pragma unroll
            for (int hn = 0; hn < 2; ++hn) fa[hn] = frag(st, s, 64 * wn + 32 * hn);
#pragma unroll
            for (int hj = 0; hj < NJ; ++hj) fb[hj] = frag(st + 2 * PLANE, s, SJ * wj + 32 * hj);
#pragma unroll
            for (int hn = 0; hn < 2; ++hn)
#pragma unroll
                for (int hj = 0; hj < NJ; ++hj) {
                    acc[hn][hj] = vrd::mfma32(fa[hn].l, fb[hj].h, acc[hn][hj]);
                    acc[hn][hj] = vrd::mfma32(fa[hn].h, fb[hj].l, acc[hn][hj]);
                    acc[hn][hj] = vrd::mfma32(fa[hn].h, fb[hj].h, acc[hn][hj]);
                }
        }
    };
    // ---- rows: the loads of the next step(s) are in flight under the MFMAs of step i; one barrier per step (a stage is rewritten
    // only after every wave has passed the barrier behind its last read)
    // (two steps in flight where the registers allow it: 64 accumulators, float4 loads, no tap bookkeeping)
    constexpr int DEPTH = (!BIG && VEC && TAPS == 1) ? 2 : 1;
    if (DEPTH == 2) {
        // (even steps live in stage 0 and slab `sa`, odd ones in stage 1 and `sb`; a fetch past the chunk's end loads rows of the
        // input again and is never stored)
        Slab sa, sb;
        fetch(sa);
        fetch(sb);
        store(lds, sa, r_begin);
        __syncthreads();
        for (int64_t r0 = r_begin; r0 < r_end; r0 += 2 * WL_ROWS) {
            fetch(sa);                                   // step r0 + 64
            compute(lds);
            if (r0 + WL_ROWS < r_end) store(lds + STAGE, sb, r0 + WL_ROWS);
            __syncthreads();
            if (r0 + WL_ROWS >= r_end) break;
            fetch(sb);                                   // step r0 + 96
            compute(lds + STAGE);
            if (r0 + 2 * WL_ROWS < r_end) store(lds, sa, r0 + 2 * WL_ROWS);
            __syncthreads();
        }
    } else {
        // One slab: written to the other stage during the step before its own, and fetched again right behind that.  The MFMAs of
        // a step and the split of the next step's slab do not depend on each other, and measured alone each is about as long as
        // the other (and as the loads): run one after the other by every wave -- the barrier puts all waves of a block into the
        // same phase -- the step cost their sum.  BIG: waves w and w + 4 share a SIMD; the first four take compute -> split,
        // the other four split -> compute, so that a SIMD has one wave on the MFMA pipe and one on the vector ALU all along.
        Slab sa;
        fetch(sa);
        store(lds, sa, r_begin);
        fetch(sa);                                       // step 1
        __syncthreads();
        const bool split_first = BIG && wave >= 4;
        int cur = 0;
        for (int64_t r0 = r_begin; r0 < r_end; r0 += WL_ROWS) {
            const bool more = r0 + WL_ROWS < r_end;
            if (split_first) {
                if (more) {
                    store(lds + (cur ^ 1) * STAGE, sa, r0 + WL_ROWS);
                    fetch(sa);                           // step r0 + 64
                }
                compute(lds + cur * STAGE);
            } else {
                compute(lds + cur * STAGE);
                if (more) {
                    store(lds + (cur ^ 1) * STAGE, sa, r0 + WL_ROWS);
                    fetch(sa);
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    if (do_bias) {       // the eight row threads of a column add up in LDS (free behind the loop's last barrier): one atomic per
                         // column and block -- same-address atomics queue up one behind the other in L2
        float* red = reinterpret_cast<float*>(lds);
        *reinterpret_cast<float4*>(red + lr * TILE + 4 * cg) = bsum;
        __syncthreads();
        if (tid < TILE && n0 + tid < N) {     // (columns beyond N carry zeros)
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) t += red[q * TILE + tid];
            if (!DET) atomicAdd(dbias + n0 + tid, t);
            else if (gridDim.y == 1) dbias[n0 + tid] += t;
            else partial[((int64_t)gridDim.y * K + chunk_id) * N + n0 + tid] = t;
        }
    }
    // the chunk's share of the tile: straight into dW when there is one chunk; otherwise as plain stores into the chunk's slice of
    // `partial` (summed by wgrad_reduce_kernel: every (chunk, n, j) is written by exactly one block), or -- without a scratch
    // buffer -- as atomics.  L2 works float atomics off at about one element per clock and channel: the 16 k atomics of each of
    // ~512 blocks were 12-17 us of a 70 us launch at M = 24,576, N = K = 512, whatever the number of rows.
    const bool single = gridDim.y == 1;
    float* dst = single ? dW : partial ? partial + (int64_t)chunk_id * N * K : dW;
#pragma unroll
    for (int q = 0; q < 2 * NJ; ++q) {
        const int hn = q / NJ, hj = q % NJ;
        const int j = j0 + SJ * wj + 32 * hj + li;
        if (j >= K) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int nn = n0 + 64 * wn + 32 * hn + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (nn < N) {
                if (single) dst[(int64_t)nn * K + j] += acc[hn][hj][e] * unscale;
                else if (DET || partial) dst[(int64_t)nn * K + j] = acc[hn][hj][e] * unscale;
                else atomicAdd(dst + (int64_t)nn * K + j, acc[hn][hj][e] * unscale);
            }
        }
    }
}

// dW[i] += sum_c partial[c * NK + i]: the row chunks' partial tiles of wgrad_x3_lds_kernel, in chunk order (so the sum does not
// depend on the order the blocks ran in, as the atomics' did).  float4 per thread when NK % 4 == 0 (and V4: both buffers
// 16-byte aligned); the scalar form adds in the same order.
template <bool V4>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int chunks, int64_t NK,
                                                           float* __restrict__ dW) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= NK) return;
    if (V4 && (NK & 3) == 0) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        int c = 0;
        for (; c + 4 <= chunks; c += 4) {       // four loads in flight
            const float4 a = ld4(partial + (int64_t)c * NK + i), b = ld4(partial + (int64_t)(c + 1) * NK + i);
            const float4 d = ld4(partial + (int64_t)(c + 2) * NK + i), e = ld4(partial + (int64_t)(c + 3) * NK + i);
            s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
            s.x += b.x, s.y += b.y, s.z += b.z, s.w += b.w;
            s.x += d.x, s.y += d.y, s.z += d.z, s.w += d.w;
            s.x += e.x, s.y += e.y, s.z += e.z, s.w += e.w;
        }
        for (; c < chunks; ++c) {
            const float4 a = ld4(partial + (int64_t)c * NK + i);
            s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
        }
        float4 o = ld4(dW + i);
        o.x += s.x, o.y += s.y, o.z += s.z, o.w += s.w;
        *reinterpret_cast<float4*>(dW + i) = o;
    } else {
        for (int64_t k = i; k < i + 4 && k < NK; ++k) {
            float s = 0.f;
            for (int c = 0; c < chunks; ++c) s += partial[(int64_t)c * NK + k];
            dW[k] += s;
        }
    }
}

constexpr int WL_BIG_ROWS = 256;     // rows per block from which the 256 x 256 tiles pay

// Row chunks of wgrad_x3_lds_kernel<BIG>: as few as still give 2 (BIG: 1) blocks per CU
template <int BIG>
int64_t wgrad_lds_chunk(int64_t M, int N, int K, int n_cu) {
    using Geo = WlGeo<BIG>;
    const int64_t tiles = (int64_t)((N + Geo::TILE - 1) / Geo::TILE) * ((K + Geo::TILE - 1) / Geo::TILE);
    int64_t want = ((BIG ? 1 : 2) * (int64_t)n_cu + tiles - 1) / tiles;
    if (want < 1) want = 1;
    int64_t chunk = (M + want - 1) / want;
    chunk = (chunk + WL_ROWS - 1) / WL_ROWS * WL_ROWS;
    if (chunk < 4 * WL_ROWS) chunk = 4 * WL_ROWS;
    return chunk;
}

// The plan of a weight-gradient call: kernel, grid, and what goes where in the scratch.
//   [tiles_off: chunks x N x K partial tiles (tile_partials)][bias.pr: rows of bias sums + the levels of their reduction]
enum WgradForm { WG_WAVE, WG_LDS128, WG_LDS256 };       // a wave per 64 x 64 tile; wgrad_x3_lds_kernel<0>; <1>
struct WgradPlan {
    WgradForm form;
    bool vec;                   // LDS forms: float4 loads
    int tiles_k;
    int64_t tiles, chunk, chunks;   // grid.x; rows per chunk (wave form: per wave, four waves to a block); grid.y
    bool tile_partials;         // the chunks' tiles are stored at tiles_off and summed by wgrad_reduce_kernel, else added into dW
    int64_t tiles_off;          // 0: the partial tiles lead the scratch, rows of bias sums follow them
    vrd::ColsumPlan bias;       // wave form with dbias: its column-sum launch.  LDS forms: only .partials and .pr -- the kernel sums
                                // the bias itself and, deterministic with several chunks, stores chunks x N rows behind its tiles
    int64_t total_floats;
};

template <int BIG>
void plan_wgrad_lds(WgradPlan& p, int64_t M, int N, int K, int n_cu) {
    using Geo = WlGeo<BIG>;
    p.form = BIG ? WG_LDS256 : WG_LDS128;
    p.tiles_k = (K + Geo::TILE - 1) / Geo::TILE;
    p.tiles = (int64_t)((N + Geo::TILE - 1) / Geo::TILE) * p.tiles_k;
    p.chunk = wgrad_lds_chunk<BIG>(M, N, K, n_cu);
    p.chunks = (M + p.chunk - 1) / p.chunk;
}

// 0, or -1 (error set) when the rows do not fit a grid
int plan_wgrad_x3(WgradPlan& p, const float* G, int64_t ldg, const float* X, int64_t ldx, int64_t M, int N, int Cin, int taps, const float* dW,
                  bool has_bias, const float* scratch, int64_t scratch_floats, bool det) {
    const int K = Cin * taps;
    const int64_t NK = (int64_t)N * K;
    // (deterministic mode: a fixed CU figure and no lab switches -- the kernel form and the chunks follow from the shapes)
    const int n_cu = det ? DET_CUS : vrd::device_cu_count();
    static const bool use_lds = [] { const char* e = getenv("VRD_WGRAD_LDS"); return !(e && e[0] == '0'); }();
    // VRD_WGRAD_BIG: 0 = 128 x 128 tiles only, 2 = 256 x 256 tiles whenever the shape allows (lab); default: by rows per chunk
    static const int big_mode = [] { const char* e = getenv("VRD_WGRAD_BIG"); return e ? atoi(e) : 1; }();
    p = WgradPlan{};
    if ((det || use_lds) && M >= 256) {
        const bool vec_shape = N % 4 == 0 && Cin % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0;
        p.vec = vec_shape && aligned16(G) && aligned16(X);
        // 256 x 256 tiles, one block per CU, when a block then still walks >= WL_BIG_ROWS rows (its start, its 64 k partial sums
        // and their share of the reduction are paid per block); 128 x 128 tiles, two blocks per CU, otherwise
        // (deterministic mode: by the shapes, whatever the alignment -- the scalar-load form adds in the same order)
        const int64_t big_tiles = (int64_t)((N + 255) / 256) * ((K + 255) / 256);
        const bool big = det ? vec_shape && N >= 256 && K >= 256 && M * big_tiles >= (int64_t)WL_BIG_ROWS * n_cu
                             : big_mode != 0 && p.vec && N >= 256 && K >= 256 && (big_mode == 2 || M * big_tiles >= (int64_t)WL_BIG_ROWS * n_cu);
        if (big) plan_wgrad_lds<1>(p, M, N, K, n_cu);
        else plan_wgrad_lds<0>(p, M, N, K, n_cu);
        VRD_CHECK_ARG(p.chunks <= 65535 && p.chunk < (1ll << 30) && p.tiles < (1 << 20), "vrd_gemm_wgrad_x3: too many rows (%lld)", (long long)M);
        // default mode: through the scratch when it holds the partial tiles and dW takes float4 stores; else atomics
        p.tile_partials = p.chunks > 1 && (det || (vrd::scratch_holds(scratch, scratch_floats, p.chunks * NK) && aligned16(dW)));
        p.total_floats = p.tile_partials ? p.chunks * NK : 0;
        if (det && p.tile_partials && has_bias) {
            p.bias.partials = true;
            p.bias.pr = vrd::place_partial_rows(p.total_floats, p.chunks, N, true);     // (where the kernel puts them)
            p.total_floats = p.bias.pr.end;
        }
        return 0;
    }
    p.form = WG_WAVE;
    p.tiles_k = (K + 63) / 64;
    p.tiles = (int64_t)((N + 63) / 64) * p.tiles_k;
    // rows per wave: as few row chunks as still fill the chip (every block ends in 4096 atomics), multiples of 32 rows
    int64_t want_blocks = (2 * (int64_t)n_cu + p.tiles - 1) / p.tiles;              // row chunks for ~2 blocks per CU
    if (want_blocks < 1) want_blocks = 1;
    int64_t chunk = (M + 4 * want_blocks - 1) / (4 * want_blocks);
    chunk = (chunk + 31) / 32 * 32;
    if (chunk < 64) chunk = 64;
    if (chunk > 1024) chunk = 1024;
    p.chunk = chunk;
    p.chunks = (M + 4 * chunk - 1) / (4 * chunk);
    VRD_CHECK_ARG(p.chunks <= 65535, "vrd_gemm_wgrad_x3: too many rows (%lld)", (long long)M);
    p.tile_partials = det && p.chunks > 1;
    p.total_floats = p.tile_partials ? p.chunks * NK : 0;
    if (has_bias) {                              // the wave kernel has no bias path: a column-sum launch of its own
        p.bias = vrd::plan_bias_colsum(M, N, det, p.total_floats);
        p.total_floats = p.bias.total_floats();
    }
    return 0;
}

// dW[i] += sum_c partial[c * NK + i], in chunk order (dW may sit anywhere: the scalar form adds in the same order)
int launch_wgrad_reduce(const float* partial, int64_t chunks, int64_t NK, float* dW, hipStream_t s) {
    auto kern = aligned16(dW) ? wgrad_reduce_kernel<true> : wgrad_reduce_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((NK + 1023) / 1024)), dim3(256), 0, s, partial, (int)chunks, NK, dW);
    VRD_LAUNCH_CHECK();
    return 0;
}

template <int BIG, bool DET>
auto wgrad_lds_for(bool vec, int taps, bool f16) -> decltype(&wgrad_x3_lds_kernel<BIG, true, 1, true, DET>) {
    if (f16) {
        if (vec) return taps == 1 ? wgrad_x3_lds_kernel<BIG, true, 1, true, DET> : wgrad_x3_lds_kernel<BIG, true, 3, true, DET>;
        return taps == 1 ? wgrad_x3_lds_kernel<BIG, false, 1, true, DET> : wgrad_x3_lds_kernel<BIG, false, 3, true, DET>;
    }
    if (vec) return taps == 1 ? wgrad_x3_lds_kernel<BIG, true, 1, false, DET> : wgrad_x3_lds_kernel<BIG, true, 3, false, DET>;
    return taps == 1 ? wgrad_x3_lds_kernel<BIG, false, 1, false, DET> : wgrad_x3_lds_kernel<BIG, false, 3, false, DET>;
}

// one launch of wgrad_x3_lds_kernel<BIG, ...>, the reduction of its partial tiles and (deterministic mode) of its bias rows
template <int BIG>
int launch_wgrad_lds(const WgradPlan& p, const float* G, int64_t ldg, const float* X, int64_t ldx, const uint8_t* row_mask, int64_t M, int N,
                     int Cin, int taps, int T, float* dW, float* dbias, float* scratch, hipStream_t s, const float* gscale, bool det) {
    using Geo = WlGeo<BIG>;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.chunks);
    float* partial = p.tile_partials ? scratch + p.tiles_off : nullptr;
    constexpr size_t lds = 2 * Geo::STAGE;
    auto kern = det ? wgrad_lds_for<BIG, true>(p.vec, taps, gscale != nullptr) : wgrad_lds_for<BIG, false>(p.vec, taps, gscale != nullptr);
    if (int rc = vrd::reserve_lds(reinterpret_cast<const void*>(kern), lds, "vrd_gemm_wgrad_x3")) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(Geo::NTHR), lds, s, G, ldg, X, ldx, row_mask, M, N, Cin, T, p.tiles_k, (int)p.chunk, dW, dbias, partial,
                       gscale);
    VRD_LAUNCH_CHECK();
    if (p.tile_partials)
        if (int rc = launch_wgrad_reduce(partial, p.chunks, (int64_t)N * Cin * taps, dW, s)) return rc;
    if (p.bias.partials) return vrd::reduce_partial_rows(scratch, p.bias.pr, dbias, nullptr, N, true, s);
    return 0;
}

}  // namespace

extern "C" {

int vrd_gemm_wgrad(const float* G, int64_t ldg, const float* X, int64_t ldx, const uint8_t* row_mask, int64_t M, int N, int Cin,
                   int taps, int T, float* dW, float* scratch, int64_t scratch_floats, void* stream, int flags) {
    VRD_CHECK_ARG(G && X && dW, "vrd_gemm_wgrad: null pointer");
    VRD_CHECK_ARG(M > 0 && N > 0 && Cin > 0 && (taps == 1 || taps == 3), "vrd_gemm_wgrad: bad sizes M=%lld N=%d Cin=%d taps=%d", (long long)M, N, Cin, taps);
    VRD_CHECK_ARG(ldg >= N && ldx >= Cin, "vrd_gemm_wgrad: leading dimension too small");
    VRD_CHECK_ARG(T > 0 && M % T == 0, "vrd_gemm_wgrad: M (%lld) must be a multiple of T (%d)", (long long)M, T);
    VRD_CHECK_FLAGS("vrd_gemm_wgrad");
    const bool det = flags & VRD_DETERMINISTIC;
    const int K = Cin * taps;
    const int64_t NK = (int64_t)N * K;
    WgradPlan plan{};
    plan.form = WG_WAVE;
    plan.tiles_k = (K + 63) / 64;
    plan.tiles = (int64_t)((N + 63) / 64) * plan.tiles_k;
    plan.chunk = WG_CHUNK;
    plan.chunks = (M + 4 * WG_CHUNK - 1) / (4 * WG_CHUNK);
    VRD_CHECK_ARG(plan.chunks <= 65535, "vrd_gemm_wgrad: too many rows (%lld)", (long long)M);
    // deterministic mode: the row chunks' partial tiles, then their sum in chunk order (one chunk: straight into dW)
    plan.tile_partials = det && plan.chunks > 1;
    plan.total_floats = plan.tile_partials ? plan.chunks * NK : 0;
    if (det)
        if (int rc = vrd::check_det_scratch("vrd_gemm_wgrad", scratch, scratch_floats, plan.total_floats)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 2.0 * (double)M * N * K, 4.0 * ((double)M * (N + Cin) + (double)N * K));
    float* dst = plan.tile_partials ? scratch + plan.tiles_off : dW;
    auto kern = det ? wgrad_kernel<true> : wgrad_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)plan.tiles, (unsigned)plan.chunks), dim3(256), 0, s, G, ldg, X, ldx, row_mask, M, N, Cin, taps, T,
                       plan.tiles_k, dst);
    VRD_LAUNCH_CHECK();
    return plan.tile_partials ? launch_wgrad_reduce(dst, plan.chunks, NK, dW, s) : 0;
}

// The plan vrd_gemm_wgrad_x3 takes for these arguments (plan_wgrad_x3, the function the call itself asks), as numbers: host code only
int vrd_gemm_wgrad_x3_plan(const float* G, int64_t ldg, const float* X, int64_t ldx, int64_t M, int N, int Cin, int taps, const float* dW,
                           int has_bias, const float* scratch, int64_t scratch_floats, int flags, int64_t* plan) {
    VRD_CHECK_ARG(G && X && dW && plan, "vrd_gemm_wgrad_x3_plan: null pointer");
    VRD_CHECK_ARG(M > 0 && N > 0 && Cin > 0 && (taps == 1 || taps == 3), "vrd_gemm_wgrad_x3_plan: bad sizes M=%lld N=%d Cin=%d taps=%d", (long long)M, N, Cin, taps);
    VRD_CHECK_ARG(ldg >= N && ldx >= Cin, "vrd_gemm_wgrad_x3_plan: leading dimension too small");
    VRD_CHECK_FLAGS("vrd_gemm_wgrad_x3_plan");
    WgradPlan p;
    if (int rc = plan_wgrad_x3(p, G, ldg, X, ldx, M, N, Cin, taps, dW, has_bias != 0, scratch, scratch_floats, (flags & VRD_DETERMINISTIC) != 0)) return rc;
    plan[0] = p.form == WG_LDS256 ? VRD_WGRAD_LDS256 : p.form == WG_LDS128 ? VRD_WGRAD_LDS128 : VRD_WGRAD_WAVE;
    plan[1] = p.vec ? 1 : 0;
    plan[2] = p.tiles;
    plan[3] = p.chunk;
    plan[4] = p.chunks;
    plan[5] = p.tile_partials ? 1 : 0;
    plan[6] = p.total_floats;
    return 0;
}

int vrd_gemm_wgrad_x3(const float* G, int64_t ldg, const float* X, int64_t ldx, const uint8_t* row_mask, int64_t M, int N, int Cin,
                      int taps, int T, float* dW, float* dbias, float* scratch, int64_t scratch_floats, const float* g_scale,
                      void* stream, int flags) {
    VRD_CHECK_ARG(G && X && dW, "vrd_gemm_wgrad_x3: null pointer");
    VRD_CHECK_ARG(M > 0 && N > 0 && Cin > 0 && (taps == 1 || taps == 3), "vrd_gemm_wgrad_x3: bad sizes M=%lld N=%d Cin=%d taps=%d", (long long)M, N, Cin, taps);
    VRD_CHECK_ARG(ldg >= N && ldx >= Cin, "vrd_gemm_wgrad_x3: leading dimension too small");
    VRD_CHECK_ARG(T > 0 && M % T == 0, "vrd_gemm_wgrad_x3: M (%lld) must be a multiple of T (%d)", (long long)M, T);
    VRD_CHECK_FLAGS("vrd_gemm_wgrad_x3");
    const bool det = flags & VRD_DETERMINISTIC;
    const int K = Cin * taps;
    WgradPlan plan;
    if (int rc = plan_wgrad_x3(plan, G, ldg, X, ldx, M, N, Cin, taps, dW, dbias != nullptr, scratch, scratch_floats, det)) return rc;
    if (det)
        if (int rc = vrd::check_det_scratch("vrd_gemm_wgrad_x3", scratch, scratch_floats, plan.total_floats)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 2.0 * (double)M * N * K, 4.0 * ((double)M * (N + Cin) + (double)N * K));
    if (plan.form == WG_LDS256) return launch_wgrad_lds<1>(plan, G, ldg, X, ldx, row_mask, M, N, Cin, taps, T, dW, dbias, scratch, s, g_scale, det);
    if (plan.form == WG_LDS128) return launch_wgrad_lds<0>(plan, G, ldg, X, ldx, row_mask, M, N, Cin, taps, T, dW, dbias, scratch, s, g_scale, det);
    if (dbias)
        if (int rc = vrd::bias_colsum(plan.bias, G, ldg, row_mask, M, N, dbias, scratch, det, s)) return rc;
    float* dst = plan.tile_partials ? scratch + plan.tiles_off : dW;
    auto kern = g_scale ? (det ? wgrad_x3_kernel<true, true> : wgrad_x3_kernel<true, false>)
                        : (det ? wgrad_x3_kernel<false, true> : wgrad_x3_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)plan.tiles, (unsigned)plan.chunks), dim3(256), 0, s, G, ldg, X, ldx, row_mask, M, N, Cin, taps, T,
                       plan.tiles_k, (int)plan.chunk, dst, g_scale);
    VRD_LAUNCH_CHECK();
    return plan.tile_partials ? launch_wgrad_reduce(dst, plan.chunks, (int64_t)N * K, dW, s) : 0;
}

}  // extern "C"
