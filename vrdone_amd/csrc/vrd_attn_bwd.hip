// Global masked attention, backward, without the (B, H, Tq, Tk) matrices (round 4).
//
// Autograd of models/local_transformer.py:163-183 (same math as :44-63).  The five-product form in vrd_backward.hip
// (S = Q K^T and dP = dO V^T by vrd_bmm, softmax / dS row by row, then dQ, dK, dV by three more vrd_bmm) writes and reads two
// (B, H, Tq, Tk) matrices -- 805 MB each at vidor.yaml's 48 pairs x 8 heads x 512 x 512 -- and is bound by them.  Here the
// scores are recomputed tile by tile, flash style, in the split precision of the other backward GEMMs (x = bf16 hi + bf16 lo,
// three MFMA products per product, f32 accumulate: vrd_gemm_x3.hip), in two kernels that mirror the two products of the
// forward kernel (vrd_attn_x3.hip):
//
//   attn_bwd_dq_kernel    a wave owns 32 queries (query = lane).  Pass 1 over the key tiles: S^T = K Q^T -> log-sum-exp of
//                         every query (the forward does not keep it).  Pass 2: S^T again, P^T = exp(S^T - lse),
//                         dP^T = V dO^T, dS^T = P^T o (dP^T - delta) * scale, dQ^T += K^T dS^T (K^T fragments by transposed
//                         LDS reads, dS^T straight from the accumulator registers).  delta_i = sum_d dO_id O_id.
//                         Writes dq, and lse / delta for the second kernel.
//   attn_bwd_dkv_kernel   a wave owns 32 keys (key = lane).  Over the query tiles: S = Q K^T, P = exp(S - lse), dP = dO V^T,
//                         dS = P o (dP - delta) * scale, dV^T += dO^T P, dK^T += Q^T dS.
//
// Operands arrive as f32 rows (the training path keeps every activation f32) and are split into bf16 hi / lo planes while a
// tile is staged into LDS; a tile that is read both as MFMA rows and through transposed reads is stored twice, once per
// swizzle.  The three kernels are templates on the head dimension (geometry: BG<HD>), instantiated at 64 (vidor.yaml, vidor_x.yaml:
// 8 heads of 64) and 32 (`fuse_head: 16` at width 512, 8 heads at width 256), each in a bf16 and an f16 form; head_dim 128 and
// the exact-f32 mode keep the five-product form.
//
// Layout at head_dim 32.  A plane row is 64 bytes (CPR = 4 chunks of 16 bytes), a plane 2 KiB, a tile 32 rows x 8 float4 = one
// float4 per thread, and four tile rows share one 256-byte bank row.  The swizzles of the 128-byte rows do not carry over:
// `row % CPR` would put the row reads into a 4-way conflict, and the transposed-read swizzle XORs in a 4, which at CPR = 4 is a
// chunk of the NEXT row (wrong data, not a slow read).  What is used instead, derived on paper from the lane-group and bank rules
// of the LDS (the header of vrd_attn_x3.hip has the first two for the pair-row kernel) -- NOT measured, no bank-conflict
// counter was read:
//   row reads (ds_read_b128, 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; bank = (a / 4) mod 64, so
//     the 16-byte slot 4 (row & 3) + (chunk ^ swz) alone decides): in a group the chunk is the same for all lanes and every
//     residue row & 3 occurs in the four rows with row >> 2 = {0, 3, 5, 6} or {1, 2, 4, 7}; swz = (row >> 2) & 3 is {0, 3, 1, 2} /
//     {1, 2, 0, 3} on them: 16 lanes on 16 distinct slots.
//   transposed reads (ds_read_b64_tr_b16, two halves of 32 lanes; bank = (a / 4) mod 64): a half addresses rows r0 .. r0 + 3 with
//     r0 a multiple of 4 -- one bank row -- 8 lanes per row on its 8 different 8-byte pieces: 32 distinct pieces under any
//     permutation of a row's chunks, so the tr images are not swizzled.
//   writes (commit_tile, ds_write_b64: 4 groups of 16 contiguous lanes, bank = (a / 4) mod 32, i.e. a 128-byte window): thread p
//     stores the 8 bytes of float4 p & 7 of row p >> 3, so a group is the 8 pieces of an even row and the 8 of the odd row
//     behind it.  A row's 8 pieces cover its 64 bytes under any permutation of its chunks, and rows 2n and 2n + 1 lie at
//     byte offsets 0 and 64 modulo 128: 16 lanes on the 16 distinct 8-byte pieces of the window, for both images.
// For either head dimension and either image a static_assert holds (row, chunk) -> byte offset to a permutation of the plane's
// 16-byte slots: a swizzle that leaves its row does not build.
#include "vrd_common.h"
#include <cmath>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef vrd::bf16x8_t bf16x8;
typedef vrd::bf16x4_t bf16x4;
template <bool F16> using e16x8 = typename vrd::SplitFmt<F16>::x8;
template <bool F16> using e16x4 = typename vrd::SplitFmt<F16>::x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

constexpr int NW = 4;                        // waves per workgroup

// Tile geometry of one head dimension (AG<HD> of vrd_attn_x3.hip is the model)
template <int HD>
struct BG {
    static_assert(HD == 32 || HD == 64, "the flash training kernels exist for head_dim 32 and 64");
    static constexpr int KS = HD / 16;                  // k16 steps over head_dim
    static constexpr int DT = HD / 32;                  // 32-row d tiles
    static constexpr int ROWB = HD * 2;                 // bytes per tile row of one 16-bit plane (128 or 64)
    static constexpr int CPR = ROWB / 16;               // 16-byte chunks per row (8 or 4)
    static constexpr int PLANE = 32 * ROWB;             // 4 KiB or 2 KiB
    static constexpr int F4R = HD / 4, F4R_LOG2 = HD == 64 ? 4 : 3;         // float4 per f32 tile row (16 or 8)
    static constexpr int F4T = HD / 32;                 // float4 per thread and tile (256 threads: 2 or 1)
    static constexpr size_t DQ_LDS = 2 * 6 * PLANE + 2 * 32 * 4, DKV_LDS = 2 * 8 * PLANE + 2 * 64 * 4, FWD_LDS = 2 * 4 * PLANE + 2 * 32 * 4;
    // chunk swizzles: rswz for planes read row-wise (one 16-byte chunk per lane, lanes = rows), tswz for planes read through
    // ds_read_b64_tr_b16 (4 rows x 16 columns per 16-lane group).  128-byte rows: both conflict free as they were.  64-byte rows
    // (CPR = 4, four tile rows per 256-byte bank row): see "Layout at head_dim 32" in the header
    __host__ __device__ static constexpr int rswz(int row) { return CPR == 4 ? (row >> 2) & 3 : row % CPR; }
    __host__ __device__ static constexpr int tswz(int row) { return CPR == 4 ? 0 : (((row & 3) << 2) % CPR) ^ (((row >> 1) & 1) << 2); }
    // byte offset of 16-byte chunk `chunk` of tile row `row` in the row image (tr = false) or the transposed-read image
    __host__ __device__ static constexpr int chunk_off(bool tr, int row, int chunk) {
        return row * ROWB + ((chunk ^ (tr ? tswz(row) : rswz(row))) * 16);
    }
    // (row, chunk) -> byte offset hits every 16-byte slot of the plane exactly once and nothing outside it: a swizzle that
    // leaves its row (an XOR with a bit >= CPR) fails the build here, not a test
    static constexpr bool image_is_permutation(bool tr) {
        bool seen[PLANE / 16] = {};
        for (int row = 0; row < 32; ++row)
            for (int chunk = 0; chunk < CPR; ++chunk) {
                const int off = chunk_off(tr, row, chunk);
                if (off < 0 || off + 16 > PLANE || off % 16 != 0 || seen[off / 16]) return false;
                seen[off / 16] = true;
            }
        for (int i = 0; i < PLANE / 16; ++i)
            if (!seen[i]) return false;
        return true;
    }
};
static_assert(BG<64>::image_is_permutation(false) && BG<64>::image_is_permutation(true), "head_dim 64: an LDS image is no permutation of its plane");
static_assert(BG<32>::image_is_permutation(false) && BG<32>::image_is_permutation(true), "head_dim 32: an LDS image is no permutation of its plane");
static_assert(BG<32>::FWD_LDS == 16 * 1024 + 256 && BG<32>::DQ_LDS == 24 * 1024 + 256 && BG<32>::DKV_LDS == 32 * 1024 + 512, "LDS sizes at head_dim 32");

// 32 rows x HD channels of head h, rows t0 .. t0+31 of a (B, T, ld) f32 matrix -> 16-bit hi / lo planes.  ROW / TR: which
// swizzled copies are written (bytes: hi at `row_hi`, lo PLANE behind it; likewise tr).  Rows >= T: zeros.  256 threads.
// The two halves of staging a tile: the global loads (issued a tile ahead, so that they fly under the current tile's MFMAs) ...
template <int HD>
struct TileRegs {
    float4 v[BG<HD>::F4T];
};
template <int HD>
__device__ __forceinline__ TileRegs<HD> fetch_tile(const float* __restrict__ src, int64_t ld, int t0, int T) {
    using G = BG<HD>;
    TileRegs<HD> t;
#pragma unroll
    for (int i = 0; i < G::F4T; ++i) {
        const int p = threadIdx.x + 256 * i;
        const int r = p >> G::F4R_LOG2, c = (p & (G::F4R - 1)) * 4;
        t.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + r < T) t.v[i] = *reinterpret_cast<const float4*>(src + (int64_t)(t0 + r) * ld + c);
    }
    return t;
}
// ... and the hi / lo split into the swizzled planes: 8 bytes per lane and plane (ds_write_b64)
// (mul: the factor of the f16 format's planes when it is not the activations' fixed 2^VRD_F16_ACT_EXP: gradient operands)
template <int HD, bool ROW, bool TR, bool F16 = false>
__device__ __forceinline__ void commit_tile(const TileRegs<HD>& t, char* row_hi, char* tr_hi, vrd::RangeTrack* rt = nullptr,
                                            float mul = vrd::F16_ACT_SCALE) {
    using G = BG<HD>;
#pragma unroll
    for (int i = 0; i < G::F4T; ++i) {
        const int p = threadIdx.x + 256 * i;
        const int r = p >> G::F4R_LOG2, c = (p & (G::F4R - 1)) * 4;
        const float4 v = t.v[i];
        const float x[4] = {v.x, v.y, v.z, v.w};
        e16x4<F16> h, l;
        vrd::split_n_scaled<F16>(x, mul, h, l, rt);
        const int within = (c & 7) * 2;
        if (ROW) {
            const int off = G::chunk_off(false, r, c >> 3) + within;
            *reinterpret_cast<e16x4<F16>*>(row_hi + off) = h;
            *reinterpret_cast<e16x4<F16>*>(row_hi + G::PLANE + off) = l;
        }
        if (TR) {
            const int off = G::chunk_off(true, r, c >> 3) + within;
            *reinterpret_cast<e16x4<F16>*>(tr_hi + off) = h;
            *reinterpret_cast<e16x4<F16>*>(tr_hi + G::PLANE + off) = l;
        }
    }
}

// fragment (rows = lanes li, k = 16 s + 8 lh + 0..7) of a row plane
template <int HD, bool F16 = false>
__device__ __forceinline__ e16x8<F16> row_frag(const char* plane, int li, int lh, int s) {
    return *reinterpret_cast<const e16x8<F16>*>(plane + li * BG<HD>::ROWB + (((2 * s + lh) ^ BG<HD>::rswz(li)) * 16));      // (= chunk_off)
}

// transposed fragment of a tr plane: A[row = column 32 d + li of the tile][k = tile rows in the accumulator order
// 16 s + 8 (j >> 2) + 4 lh + (j & 3)] -- the order in which registers 8s .. 8s+7 of a 32 x 32 accumulator hold its rows
template <int HD, bool F16 = false>
__device__ __forceinline__ e16x8<F16> tr_frag(const char* plane, int lane, int s, int d) {
    const int lh = lane >> 5, vq = (lane >> 2) & 3, vp = lane & 3;
    const int col = 32 * d + 16 * ((lane >> 4) & 1) + 4 * vp;
    s16x8 r;
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        const int row = 16 * s + 8 * part + 4 * lh + vq;
        const int off = BG<HD>::chunk_off(true, row, (col * 2) >> 4) + ((col * 2) & 15);
        const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(plane + off));
#pragma unroll
        for (int j = 0; j < 4; ++j) r[4 * part + j] = t[j];
    }
    return __builtin_bit_cast(e16x8<F16>, r);
}

// lane (li, lh): elements d = 16 s + 8 lh + 0..7 of row `row` of head h (f32) as hi / lo fragments (the B operand of a product
// whose columns are this wave's 32 rows)
template <bool F16 = false, int KS>
__device__ __forceinline__ void load_col_frags(const float* __restrict__ rowp, int lh, bool ok, e16x8<F16> (&hi)[KS], e16x8<F16> (&lo)[KS],
                                               vrd::RangeTrack* rt = nullptr, float mul = vrd::F16_ACT_SCALE) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const float4 a = *reinterpret_cast<const float4*>(rowp + 16 * s + 8 * lh);
            const float4 b = *reinterpret_cast<const float4*>(rowp + 16 * s + 8 * lh + 4);
            x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
        }
        vrd::split_n_scaled<F16>(x, mul, hi[s], lo[s], rt);
    }
}

// acc += A . B in split precision
template <typename V>
__device__ __forceinline__ f32x16 mfma3(V ah, V al, V bh, V bl, f32x16 acc) {
    acc = vrd::mfma32(al, bh, acc);
    acc = vrd::mfma32(ah, bl, acc);
    return vrd::mfma32(ah, bh, acc);
}

// registers 8 s .. 8 s + 7 of a 32 x 32 accumulator as the hi / lo B fragment of k16 step s
template <bool F16 = false>
__device__ __forceinline__ void split_acc(const f32x16& a, int s, e16x8<F16>& hi, e16x8<F16>& lo, float mul = vrd::F16_ACT_SCALE) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = a[8 * s + j];
    vrd::split_n_scaled<F16>(x, mul, hi, lo);
}

__device__ __forceinline__ int acc_row(int e, int lh) { return (e & 3) + 8 * (e >> 2) + 4 * lh; }

// ---------------------------------------------------------------------------------------------------------------------
// Forward of a training step on the same building blocks (f32 rows in, split products, f32 rows + log-sum-exp out): what
// attn_flash_x3_kernel does on pair rows.  F16: the f16x3 mode's planes (values times 2^VRD_F16_ACT_EXP: the scores come out
// 2^(2e) too large, P is split as P 2^e, and O / l carries 2^(2e) once).
template <int HD, bool F16>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_rows_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int64_t ldkv,
                                                                  const uint8_t* __restrict__ kv_mask, int Tq, int Tk, int n_head,
                                                                  float scale, float* __restrict__ out, int64_t ldo,
                                                                  float* __restrict__ lse_out, unsigned* rflag) {
    constexpr int KS = BG<HD>::KS, DT = BG<HD>::DT, PLANE = BG<HD>::PLANE;
    extern __shared__ __attribute__((aligned(16))) char lds[];        // 2 stages x (k row h/l, v tr h/l) + key bias: FWD_LDS
    vrd::RangeTrack rt;                                               // q / k / v are f32 rows, split here (vrd_common.h)
    float* const kbias = reinterpret_cast<float*>(lds + 2 * 4 * PLANE);
    const int qblk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int tq = (qblk * NW + wave) * 32 + li;
    const bool q_ok = tq < Tq;
    const float* const kb = k + (int64_t)b * Tk * ldkv + h * HD;
    const float* const vb = v + (int64_t)b * Tk * ldkv + h * HD;
    const uint8_t* const mk = kv_mask ? kv_mask + (int64_t)b * Tk : nullptr;
    constexpr float s_in = F16 ? vrd::F16_ACT_INV * vrd::F16_ACT_INV : 1.0f;          // undoes the operand scaling of a product
    e16x8<F16> qh[KS], ql[KS];
    load_col_frags<F16>(q + ((int64_t)b * Tq + (q_ok ? tq : 0)) * ldq + h * HD, lh, q_ok, qh, ql, &rt);
    f32x16 oacc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    TileRegs<HD> rk, rv;
    float rbias = 0.f;
    const int nkt = (Tk + 31) / 32;
    auto fetch = [&](int kt) {
        rk = fetch_tile<HD>(kb, ldkv, kt * 32, Tk);
        rv = fetch_tile<HD>(vb, ldkv, kt * 32, Tk);
        if (threadIdx.x < 32) {
            const int key = kt * 32 + threadIdx.x;
            rbias = (key < Tk && (!mk || mk[key])) ? 0.f : -INFINITY;
        }
    };
    auto commit = [&](int buf) {
        char* st = lds + buf * 4 * PLANE;
        commit_tile<HD, true, false, F16>(rk, st, nullptr, &rt);
        commit_tile<HD, false, true, F16>(rv, nullptr, st + 2 * PLANE, &rt);
        if (threadIdx.x < 32) kbias[buf * 32 + threadIdx.x] = rbias;
    };
    fetch(0);
    commit(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) fetch(kt + 1);
        const char* st = lds + (kt & 1) * 4 * PLANE;
        const float* kbs = kbias + (kt & 1) * 32;
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int t = 0; t < KS; ++t) s = mfma3(row_frag<HD, F16>(st, li, lh, t), row_frag<HD, F16>(st + PLANE, li, lh, t), qh[t], ql[t], s);
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] = s[e] * (scale * s_in) + kbs[acc_row(e, lh)];
            mx = fmaxf(mx, s[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __expf(m_run - m_use);
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] = __expf(s[e] - m_use);
            ps += s[e];
        }
        ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            e16x8<F16> ph, pl;
            split_acc<F16>(s, s2, ph, pl);
#pragma unroll
            for (int d = 0; d < DT; ++d)
                oacc[d] = mfma3(tr_frag<HD, F16>(st + 2 * PLANE, lane, s2, d), tr_frag<HD, F16>(st + 3 * PLANE, lane, s2, d), ph, pl, oacc[d]);
        }
        if (kt + 1 < nkt) commit((kt + 1) & 1);
        __syncthreads();
    }
    if (q_ok) {
        const float inv = s_in / l_run;
        float* const orow = out + ((int64_t)b * Tq + tq) * ldo + h * HD;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(orow + 32 * d + 8 * g + 4 * lh) =
                    make_float4(oacc[d][4 * g] * inv, oacc[d][4 * g + 1] * inv, oacc[d][4 * g + 2] * inv, oacc[d][4 * g + 3] * inv);
        if (lh == 0) lse_out[((int64_t)b * n_head + h) * Tq + tq] = l_run > 0.f ? m_run + __logf(l_run) : 0.f;
    }
    if (F16) rt.report(rflag, vrd::RANGE_GEMM_IN);
}

// ---------------------------------------------------------------------------------------------------------------------
// lse_in: the forward's log-sum-exp (attn_fwd_rows_kernel), or NULL: pass 1 recomputes it
// F16 (the f16x3 mode): every operand as f16 planes of a power-of-two multiple -- q, k, v, P at the activations' 2^VRD_F16_ACT_EXP
// (they went through the forward's range check), dO at s_o = o_scale[0] (vrd_absmax_scale of dO), dS at s_s = s_o s_v 2^-17 with
// s_v = v_scale[0] (vrd_absmax_scale of V): |dS| <= (|dP| + |delta|) / 8 <= 16 max|dO| max|V| < 2^32 / (s_o s_v), so dS s_s stays
// below 2^15.  The planes keep 2^-25 ABSOLUTE precision down to their subnormals, i.e. 2^-25 / s_s on dS, and both factors come from
// the whole tensor: an entry dS carries the relative error 2^-25 / (s_s |dS|) once dS s_s < 2^-2.  What the bound gives away is not
// free: on flat rows of unit-scale randn operands dS s_s is about 2^-1 at 77 keys (P ~ 1 / Tk), so dS already sits at the 2^-24 of
// the subnormal lo plane, and a sequence whose dO is 2^-k of the batch maximum keeps 2^(k-24).  Measured per (sequence, head) block
// against float64 (tests/test_gpu_attn_hard.py, error over the block's largest entry, dq / dk): 0.9e-6 at 2^0, 1.4e-6 at 2^-6,
// 1.5e-4 at 2^-12 -- the per-tensor 2e-5 of the other tests holds per block down to about 2^-8 of the batch maximum, below that the
// bf16 planes (relative: 1-4e-5 at every spread) are the more precise ones.  dv and out do not go through dS and keep 1e-6.
// The accumulators are rescaled where they leave the kernel.
// rflag: q, k and v are split here again, and the caller need not have run attn_fwd_rows_kernel on them (lse_in NULL): the split of
// this wave's query rows and of every k / v tile of pass 2 feeds a tracker (RANGE_GEMM_IN), so the call reports on its own.
template <int HD, bool F16>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_dq_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                                const float* __restrict__ v, int64_t ldkv, const float* __restrict__ o,
                                                                const float* __restrict__ dO, int64_t ldo,
                                                                const uint8_t* __restrict__ kv_mask, int Tq, int Tk, int n_head,
                                                                float scale, float* __restrict__ dq, const float* __restrict__ lse_in,
                                                                float* __restrict__ lse_out, float* __restrict__ delta_out,
                                                                const float* __restrict__ o_scale, const float* __restrict__ v_scale,
                                                                unsigned* rflag) {
    constexpr int KS = BG<HD>::KS, DT = BG<HD>::DT, PLANE = BG<HD>::PLANE;
    typedef e16x8<F16> bf16x8;                                         // (this instantiation's eight 16-bit elements)
    vrd::RangeTrack rt;
    constexpr float a_inv = F16 ? vrd::F16_ACT_INV : 1.0f;
    const float s_o = F16 ? vrd::uniform_load(o_scale) : 1.f, s_o_inv = F16 ? vrd::uniform_load(o_scale + 1) : 1.f;
    const float s_s = F16 ? s_o * vrd::uniform_load(v_scale) * 0x1p-17f : 1.f;
    const float s_s_inv = F16 ? s_o_inv * vrd::uniform_load(v_scale + 1) * 0x1p17f : 1.f;
    extern __shared__ __attribute__((aligned(16))) char lds[];        // 2 stages x (k row h/l, k tr h/l, v row h/l) + key bias: DQ_LDS
    float* const kbias = reinterpret_cast<float*>(lds + 2 * 6 * PLANE);               // [2][32]
    const int qblk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int tq = (qblk * NW + wave) * 32 + li;
    const bool q_ok = tq < Tq;
    const float* const qrow = q + ((int64_t)b * Tq + (q_ok ? tq : 0)) * ldq + h * HD;
    const float* const orow = o + ((int64_t)b * Tq + (q_ok ? tq : 0)) * ldo + h * HD;
    const float* const drow = dO + ((int64_t)b * Tq + (q_ok ? tq : 0)) * ldo + h * HD;
    const float* const kb = k + (int64_t)b * Tk * ldkv + h * HD;
    const float* const vb = v + (int64_t)b * Tk * ldkv + h * HD;
    const uint8_t* const mk = kv_mask ? kv_mask + (int64_t)b * Tk : nullptr;

    bf16x8 qh[KS], ql[KS], gh[KS], gl[KS];
    load_col_frags<F16>(qrow, lh, q_ok, qh, ql, &rt);
    load_col_frags<F16>(drow, lh, q_ok, gh, gl, nullptr, s_o);
    // delta = sum_d dO O over the query's row: this lane holds half of the d's
    float delta = 0.f;
    if (q_ok) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) delta += drow[16 * s + 8 * lh + j] * orow[16 * s + 8 * lh + j];
    }
    delta += __shfl_xor(delta, 32, 64);

    const int nkt = (Tk + 31) / 32;
    TileRegs<HD> rk, rv;
    float rbias = 0.f;
    auto fetch = [&](int kt, bool second) {
        rk = fetch_tile<HD>(kb, ldkv, kt * 32, Tk);
        if (second) rv = fetch_tile<HD>(vb, ldkv, kt * 32, Tk);
        if (threadIdx.x < 32) {
            const int key = kt * 32 + threadIdx.x;
            rbias = (key < Tk && (!mk || mk[key])) ? 0.f : -INFINITY;
        }
    };
    auto commit = [&](int buf, bool second) {
        char* st = lds + buf * 6 * PLANE;
        if (second) {
            commit_tile<HD, true, true, F16>(rk, st, st + 2 * PLANE, &rt);
            commit_tile<HD, true, false, F16>(rv, st + 4 * PLANE, nullptr, &rt);
        } else {
            commit_tile<HD, true, false, F16>(rk, st, nullptr);
        }
        if (threadIdx.x < 32) kbias[buf * 32 + threadIdx.x] = rbias;
    };
    auto scores = [&](const char* st, const float* kbs) {
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int t = 0; t < KS; ++t) s = mfma3(row_frag<HD, F16>(st, li, lh, t), row_frag<HD, F16>(st + PLANE, li, lh, t), qh[t], ql[t], s);
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = s[e] * (scale * a_inv * a_inv) + kbs[acc_row(e, lh)];
        return s;
    };

    // ---- pass 1: log-sum-exp of every query over the valid keys (unless the forward kept it)
    float m_run = -INFINITY, l_run = 0.f;
    if (!lse_in) {
    fetch(0, false);
    commit(0, false);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) fetch(kt + 1, false);
        const f32x16 s = scores(lds + (kt & 1) * 6 * PLANE, kbias + (kt & 1) * 32);
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[e]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) ps += __expf(s[e] - m_use);
        ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * __expf(m_run - m_use) + ps;
        m_run = m_new;
        if (kt + 1 < nkt) commit((kt + 1) & 1, false);          // (the other buffer: last read before the previous barrier)
        __syncthreads();
    }
    }
    // (a query that sees no valid key: every p below is exp(-inf - 0) = 0)
    const float lse = lse_in ? (q_ok ? lse_in[((int64_t)b * n_head + h) * Tq + tq] : 0.f) : (l_run > 0.f ? m_run + __logf(l_run) : 0.f);

    // ---- pass 2: dQ^T += K^T . dS^T
    f32x16 dqa[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) dqa[d][e] = 0.f;
    fetch(0, true);
    commit(0, true);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) fetch(kt + 1, true);
        const char* st = lds + (kt & 1) * 6 * PLANE;
        f32x16 s = scores(st, kbias + (kt & 1) * 32);
        f32x16 dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) dp[e] = 0.f;
#pragma unroll
        for (int t = 0; t < KS; ++t)
            dp = mfma3(row_frag<HD, F16>(st + 4 * PLANE, li, lh, t), row_frag<HD, F16>(st + 5 * PLANE, li, lh, t), gh[t], gl[t], dp);
        const float dp_unscale = a_inv * s_o_inv;              // (dP came out of V 2^a times dO s_o)
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = __expf(s[e] - lse) * (dp[e] * dp_unscale - delta) * scale;            // dS^T (scaled)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 dh, dl;
            split_acc<F16>(s, s2, dh, dl, s_s);
#pragma unroll
            for (int d = 0; d < DT; ++d)
                dqa[d] = mfma3(tr_frag<HD, F16>(st + 2 * PLANE, lane, s2, d), tr_frag<HD, F16>(st + 3 * PLANE, lane, s2, d), dh, dl, dqa[d]);
        }
        if (kt + 1 < nkt) commit((kt + 1) & 1, true);
        __syncthreads();
    }
    if (q_ok) {
        float* const out = dq + ((int64_t)b * Tq + tq) * ldq + h * HD;
        const float u = a_inv * s_s_inv;         // (K 2^a times dS s_s)
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g)          // registers 4g .. 4g+3 are d = 32 d + 8 g + 4 lh + 0..3
                *reinterpret_cast<float4*>(out + 32 * d + 8 * g + 4 * lh) =
                    make_float4(dqa[d][4 * g] * u, dqa[d][4 * g + 1] * u, dqa[d][4 * g + 2] * u, dqa[d][4 * g + 3] * u);
        if (lh == 0) {
            lse_out[((int64_t)b * n_head + h) * Tq + tq] = lse;
            delta_out[((int64_t)b * n_head + h) * Tq + tq] = delta;
        }
    }
    if (F16) rt.report(rflag, vrd::RANGE_GEMM_IN);
}

// ---------------------------------------------------------------------------------------------------------------------
template <int HD, bool F16>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_dkv_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                                 const float* __restrict__ v, int64_t ldkv, const float* __restrict__ dO,
                                                                 int64_t ldo, const uint8_t* __restrict__ kv_mask, int Tq, int Tk,
                                                                 int n_head, float scale, const float* __restrict__ lse_in,
                                                                 const float* __restrict__ delta_in, float* __restrict__ dk,
                                                                 float* __restrict__ dv, const float* __restrict__ o_scale,
                                                                 const float* __restrict__ v_scale) {
    constexpr int KS = BG<HD>::KS, DT = BG<HD>::DT, PLANE = BG<HD>::PLANE;
    typedef e16x8<F16> bf16x8;
    constexpr float a_inv = F16 ? vrd::F16_ACT_INV : 1.0f;                       // (scales: see attn_bwd_dq_kernel)
    const float s_o = F16 ? vrd::uniform_load(o_scale) : 1.f, s_o_inv = F16 ? vrd::uniform_load(o_scale + 1) : 1.f;
    const float s_s = F16 ? s_o * vrd::uniform_load(v_scale) * 0x1p-17f : 1.f;
    const float s_s_inv = F16 ? s_o_inv * vrd::uniform_load(v_scale + 1) * 0x1p17f : 1.f;
    // 2 stages x (q row h/l, q tr h/l, dO row h/l, dO tr h/l) + lse / delta of the tile's 32 queries: DKV_LDS
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* const stat = reinterpret_cast<float*>(lds + 2 * 8 * PLANE);                // [2][lse 32 | delta 32]
    const int kblk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int tk = (kblk * NW + wave) * 32 + li;
    const bool k_in = tk < Tk;
    const bool k_ok = k_in && (!kv_mask || kv_mask[(int64_t)b * Tk + tk]);
    const float* const krow = k + ((int64_t)b * Tk + (k_in ? tk : 0)) * ldkv + h * HD;
    const float* const vrow = v + ((int64_t)b * Tk + (k_in ? tk : 0)) * ldkv + h * HD;
    const float* const qb = q + (int64_t)b * Tq * ldq + h * HD;
    const float* const gb = dO + (int64_t)b * Tq * ldo + h * HD;
    const float* const lse_b = lse_in + ((int64_t)b * n_head + h) * Tq;
    const float* const del_b = delta_in + ((int64_t)b * n_head + h) * Tq;

    bf16x8 kh[KS], kl[KS], vh[KS], vl[KS];
    load_col_frags<F16>(krow, lh, k_in, kh, kl);
    load_col_frags<F16>(vrow, lh, k_in, vh, vl);
    f32x16 dka[DT], dva[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) dka[d][e] = dva[d][e] = 0.f;

    const int nqt = (Tq + 31) / 32;
    TileRegs<HD> rq, rg;
    float rl = 0.f, rd = 0.f;
    auto fetch = [&](int qt) {
        rq = fetch_tile<HD>(qb, ldq, qt * 32, Tq);
        rg = fetch_tile<HD>(gb, ldo, qt * 32, Tq);
        if (threadIdx.x < 32) {
            const int t = qt * 32 + threadIdx.x;
            rl = t < Tq ? lse_b[t] : INFINITY;              // a query past Tq: p = exp(-inf) = 0
            rd = t < Tq ? del_b[t] : 0.f;
        }
    };
    auto commit = [&](int buf) {
        char* st = lds + buf * 8 * PLANE;
        commit_tile<HD, true, true, F16>(rq, st, st + 2 * PLANE);
        commit_tile<HD, true, true, F16>(rg, st + 4 * PLANE, st + 6 * PLANE, nullptr, s_o);
        if (threadIdx.x < 32) {
            stat[buf * 64 + threadIdx.x] = rl;
            stat[buf * 64 + 32 + threadIdx.x] = rd;
        }
    };
    fetch(0);
    commit(0);
    __syncthreads();
    for (int qt = 0; qt < nqt; ++qt) {
        if (qt + 1 < nqt) fetch(qt + 1);
        const char* st = lds + (qt & 1) * 8 * PLANE;
        const float* sl = stat + (qt & 1) * 64;
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            s = mfma3(row_frag<HD, F16>(st, li, lh, t), row_frag<HD, F16>(st + PLANE, li, lh, t), kh[t], kl[t], s);                          // S = Q K^T
            dp = mfma3(row_frag<HD, F16>(st + 4 * PLANE, li, lh, t), row_frag<HD, F16>(st + 5 * PLANE, li, lh, t), vh[t], vl[t], dp);        // dP = dO V^T
        }
        f32x16 p;
        const float s_unscale = scale * a_inv * a_inv, dp_unscale = a_inv * s_o_inv;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = acc_row(e, lh);
            p[e] = k_ok ? __expf(s[e] * s_unscale - sl[r]) : 0.f;
            s[e] = p[e] * (dp[e] * dp_unscale - sl[32 + r]) * scale;                                                  // dS (scaled)
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 ph, pl, dh, dl;
            split_acc<F16>(p, s2, ph, pl);
            split_acc<F16>(s, s2, dh, dl, s_s);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                dva[d] = mfma3(tr_frag<HD, F16>(st + 6 * PLANE, lane, s2, d), tr_frag<HD, F16>(st + 7 * PLANE, lane, s2, d), ph, pl, dva[d]);      // dV^T += dO^T P
                dka[d] = mfma3(tr_frag<HD, F16>(st + 2 * PLANE, lane, s2, d), tr_frag<HD, F16>(st + 3 * PLANE, lane, s2, d), dh, dl, dka[d]);      // dK^T += Q^T dS
            }
        }
        if (qt + 1 < nqt) commit((qt + 1) & 1);
        __syncthreads();
    }
    if (k_in) {
        float* const ok_ = dk + ((int64_t)b * Tk + tk) * ldkv + h * HD;
        float* const ov = dv + ((int64_t)b * Tk + tk) * ldkv + h * HD;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = 32 * d + 8 * g + 4 * lh;
                const float uk = a_inv * s_s_inv, uv = a_inv * s_o_inv;       // (Q 2^a times dS s_s; P 2^a times dO s_o)
                *reinterpret_cast<float4*>(ok_ + c) = make_float4(dka[d][4 * g] * uk, dka[d][4 * g + 1] * uk, dka[d][4 * g + 2] * uk, dka[d][4 * g + 3] * uk);
                *reinterpret_cast<float4*>(ov + c) = make_float4(dva[d][4 * g] * uv, dva[d][4 * g + 1] * uv, dva[d][4 * g + 2] * uv, dva[d][4 * g + 3] * uv);
            }
    }
}

using vrd::aligned16;

template <int HD, bool F16>
int launch_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* out, const float* dO, int64_t ldo,
               const uint8_t* kv_mask, int B, int Tq, int Tk, int n_head, float scale, float* dq, float* dk, float* dv, const float* lse,
               float* lse_own, float* delta, const float* o_scale, const float* v_scale, hipStream_t s) {
    using G = BG<HD>;
    const dim3 gq((Tq + NW * 32 - 1) / (NW * 32), n_head, B), gk((Tk + NW * 32 - 1) / (NW * 32), n_head, B);
    if (int rc = vrd::reserve_lds(reinterpret_cast<const void*>(attn_bwd_dq_kernel<HD, F16>), G::DQ_LDS, "vrd_attention_bwd(dq)")) return rc;
    if (int rc = vrd::reserve_lds(reinterpret_cast<const void*>(attn_bwd_dkv_kernel<HD, F16>), G::DKV_LDS, "vrd_attention_bwd(dk, dv)")) return rc;
    hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, F16>), gq, dim3(NW * 64), G::DQ_LDS, s, q, ldq, k, v, ldkv, out, dO, ldo, kv_mask, Tq, Tk, n_head, scale,
                       dq, lse, lse_own, delta, o_scale, v_scale, F16 ? vrd::range_flag() : (unsigned*)nullptr);
    VRD_LAUNCH_CHECK();
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<HD, F16>), gk, dim3(NW * 64), G::DKV_LDS, s, q, ldq, k, v, ldkv, dO, ldo, kv_mask, Tq, Tk, n_head, scale,
                       lse ? lse : lse_own, delta, dk, dv, o_scale, v_scale);
    VRD_LAUNCH_CHECK();
    return 0;
}

template <int HD, bool F16>
int launch_rows(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const uint8_t* kv_mask, int B, int Tq, int Tk,
                int n_head, float scale, float* out, int64_t ldo, float* lse, hipStream_t s) {
    using G = BG<HD>;
    const dim3 grid((Tq + NW * 32 - 1) / (NW * 32), n_head, B);
    if (int rc = vrd::reserve_lds(reinterpret_cast<const void*>(attn_fwd_rows_kernel<HD, F16>), G::FWD_LDS, "vrd_attention_rows")) return rc;
    hipLaunchKernelGGL((attn_fwd_rows_kernel<HD, F16>), grid, dim3(NW * 64), G::FWD_LDS, s, q, ldq, k, v, ldkv, kv_mask, Tq, Tk, n_head, scale, out,
                       ldo, lse, F16 ? vrd::range_flag() : (unsigned*)nullptr);
    VRD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int vrd_attention_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* out,
                                 const float* dO, int64_t ldo, const uint8_t* kv_mask, int B, int Tq, int Tk, int n_head, int head_dim,
                                 float* dq, float* dk, float* dv, const float* lse, float* scratch, const float* o_scale,
                                 const float* v_scale, void* stream) {
    VRD_CHECK_ARG(q && k && v && out && dO && dq && dk && dv && scratch, "vrd_attention_bwd: null pointer");
    VRD_CHECK_ARG(head_dim == 32 || head_dim == 64, "vrd_attention_bwd: head_dim must be 32 or 64 (got %d)", head_dim);
    VRD_CHECK_ARG((o_scale == nullptr) == (v_scale == nullptr), "vrd_attention_bwd: o_scale and v_scale go together");
    VRD_CHECK_ARG(B > 0 && B <= 65535 && n_head > 0 && n_head <= 65535 && Tq > 0 && Tk > 0, "vrd_attention_bwd: bad sizes");
    const int width = n_head * head_dim;
    VRD_CHECK_ARG(ldq >= width && ldkv >= width && ldo >= width && ldq % 4 == 0 && ldkv % 4 == 0 && ldo % 4 == 0 && aligned16(q) &&
                      aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dO) && aligned16(dq) && aligned16(dk) && aligned16(dv),
                  "vrd_attention_bwd: rows must be 16-byte aligned with leading dimensions >= n_head * head_dim");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)head_dim);
    // (dq: two passes over the keys, three + two products; dk / dv: four products)
    vrd::ProfScope prof(VRD_K_BACKWARD, s, 2.0 * 9.0 * B * (double)n_head * Tq * Tk * head_dim, 0.0);
    float* lse_own = scratch;
    float* delta = scratch + (int64_t)B * n_head * Tq;
    auto go = [&](auto fn) { return fn(q, ldq, k, v, ldkv, out, dO, ldo, kv_mask, B, Tq, Tk, n_head, scale, dq, dk, dv, lse, lse_own, delta, o_scale, v_scale, s); };
    if (head_dim == 32) return o_scale ? go(launch_bwd<32, true>) : go(launch_bwd<32, false>);
    return o_scale ? go(launch_bwd<64, true>) : go(launch_bwd<64, false>);
}

extern "C" int vrd_attention_rows(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const uint8_t* kv_mask, int B,
                                  int Tq, int Tk, int n_head, int head_dim, int fmt, float* out, int64_t ldo, float* lse, void* stream) {
    VRD_CHECK_ARG(q && k && v && out && lse, "vrd_attention_rows: null pointer");
    VRD_CHECK_ARG(head_dim == 32 || head_dim == 64, "vrd_attention_rows: head_dim must be 32 or 64 (got %d)", head_dim);
    VRD_CHECK_ARG(fmt == VRD_PAIR_BF16 || fmt == VRD_PAIR_F16, "vrd_attention_rows: fmt must be VRD_PAIR_BF16 or VRD_PAIR_F16");
    VRD_CHECK_ARG(B > 0 && B <= 65535 && n_head > 0 && n_head <= 65535 && Tq > 0 && Tk > 0, "vrd_attention_rows: bad sizes");
    const int width = n_head * head_dim;
    VRD_CHECK_ARG(ldq >= width && ldkv >= width && ldo >= width && ldq % 4 == 0 && ldkv % 4 == 0 && ldo % 4 == 0 && aligned16(q) &&
                      aligned16(k) && aligned16(v) && aligned16(out),
                  "vrd_attention_rows: rows must be 16-byte aligned with leading dimensions >= n_head * head_dim");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)head_dim);
    vrd::ProfScope prof(VRD_K_ATTN_FLASH, s, 4.0 * B * (double)n_head * Tq * Tk * head_dim, 4.0 * B * (double)width * (2.0 * Tq + 2.0 * Tk));
    const bool f16 = fmt == VRD_PAIR_F16;
    auto go = [&](auto fn) { return fn(q, ldq, k, v, ldkv, kv_mask, B, Tq, Tk, n_head, scale, out, ldo, lse, s); };
    if (head_dim == 32) return f16 ? go(launch_rows<32, true>) : go(launch_rows<32, false>);
    return f16 ? go(launch_rows<64, true>) : go(launch_rows<64, false>);
}
