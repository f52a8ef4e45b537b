"""Small-shape cases for the backward GEMM kernels (tests/test_bwd_gemm_cases_cpu.py, tests/test_gpu_bwd_gemm_tiles.py).

The weight-gradient kernels of csrc/vrd_wgrad.hip (the exact-f32 wave kernel, the split-precision wave kernel and the 32
instantiations of the LDS kernel, their partial-tile reduction and bias sums) and the input-gradient GEMM (ops.conv_dgrad: f32
rows of dy through the register-staged split kernels of csrc/vrd_gemm_x3.hip) are chosen by shape, CU count, alignment and two
switches that are read once per process.  This module holds the case table with the plan every weight-gradient case expects,
the seeded inputs in poisoned windows, the float64 reference of every element of dW, db and dx, the derived bounds, the checker,
a mirror of the plan, and an f32 emulation of the three-product arithmetic in chunk order that shows the reference alone stays
inside the bounds (and carries the Python stand-ins of the faults the GPU test exists to catch).  Nothing here needs a GPU.

Bounds (per element, derived -- not measured on the kernels).

dW, with mag = sum_r |g| |x| over the contraction (masked rows and taps outside a sequence contribute nothing):

    |got - ref| <= (u + R * 2^-24) * mag + 2^-23 * (|ref| + |dW_0|)

  u      the split's own error: g x ~= g_lo x_hi + g_hi x_lo + g_hi x_hi drops g_lo x_lo.  The reference is computed from the
         operands AS SPLIT (hi + lo of each format, f16: of g * 2^e and x * 2^4), so the rounding of an operand to hi + lo is not
         counted against the kernel and the dropped product is the whole of it.  bf16 planes have 8 significand bits: |lo| <=
         2^-8 |hi + lo|, the dropped product at most 2^-16 of |g x|, u = 2^-16.  (3 * 2^-18, the figure of
         tests/gemm_tile_cases.py, takes |lo| <= 2^-9: half an ulp of 1.0 where it is half an ulp of 2.0.  A contraction over
         one row shows it -- case wave_m1 holds an element whose dropped product is 2.95 * 2^-18 of |g x|, g = 1.0120 = 1.0156 -
         0.92 * 2^-8.)  f16 planes have 11 bits: the dropped product is at most 2^-22, u = 3 * 2^-22 is kept; 0 for the
         exact-f32 kernel;
  R      the f32 roundings on the path of one element, each at most 2^-24 of mag: one per MFMA issued on its accumulator
         (LDS forms: six per 32-row step of its chunk; split wave kernel: six per 32 rows of each of the four waves of a
         workgroup; exact-f32 wave kernel: an MFMA adds two rows' products one after the other, two roundings, eight MFMAs per 16
         rows), three per workgroup for the wave forms' sum over four waves, one per partial tile or atomic added, plus the
         unscale and the final add (+ 2): rounding_count();
  2^-23  the final `+=` onto dW_0 and the result's own rounding.  dW_0 and db_0 are seeded at the scale of the products
         (|g| |x|): a start value far above the sum would hide the sum in its last bits.

db, the exact-f32 column sums of the masked gradient:   |got - ref| <= (rows + chunks) * 2^-24 * sum_r |g| + chunks * 2^-23 * |db_0|
  (one rounding per row added and per chunk's partial sum, relative to at most sum |g|; the second term is for the adds onto the
  non-zero start value db_0 -- one per chunk that adds to it, each rounding relative to a running value that db_0 is part of,
  granted at 2^-23 like dW's final add.  With db_0 = 0 it vanishes.)

dx (ops.conv_dgrad), the forward module's bound with K = N * k and lip = the row mask:
    |got - ref| <= (u + (K/32 + 2) * 2^-24) * mag * lip + 2^-23 * |ref|

The emulation must stay inside every bound with only HALF of its rounding terms granted (slack = 0.5:  u * mag + half of
the rest) on every case (tests/test_bwd_gemm_cases_cpu.py).  The split's term is granted whole: the dropped product is a function
of the inputs alone, the same in the emulation and in every correct kernel, and over a contraction of one row it comes within a few
per cent of its worst case; what differs between a kernel and the emulation is the order and number of the f32 roundings."""
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

import f16x1_emulation as E
import gemm_tile_cases as GT
import window_cases as W

ACT_EXP = E.ACT_EXP
U = {"bf16": 2.0 ** -16, "f16": 3 * 2.0 ** -22, "f32": 0.0}
X3 = ("bf16", "f16")
GROUP_ENV = {
    "wave": {"VRD_WGRAD_LDS": "0"},
    "lds128": {"VRD_WGRAD_BIG": "0"},
    "lds256": {"VRD_WGRAD_BIG": "2"},
    "default": {},
    "dgrad128": {"VRD_X3_DMA": "0", "VRD_X3_SMALL": "0"},
    "dgrad64": {"VRD_X3_DMA": "0"},
}
WGRAD_GROUPS = ("wave", "lds128", "lds256", "default")
DET_CUS = 256          # csrc/vrd_wgrad.hip: the CU figure every deterministic chunking assumes (and the MI355X's own count)

# kind: "x3" (vrd_gemm_wgrad_x3), "f32" (vrd_gemm_wgrad), "dgrad" (ops.conv_dgrad)
# mask: None | "rand" (0.8) | "ends" (first and last row of every sequence) | "all" (every row masked) | ("rows", a, b): rows a .. b - 1
# align: "ok" | "ldg_odd" | "ldx_odd" | "shift" (G and X start one float past a 16-byte line) | "dw_shift" (dW does) | "ldc_odd" (dgrad)
# plan: (form, vec, multi, tile_partials) -- form "wave" / "lds128" / "lds256", multi: chunks >= 2 (else chunks == 1)
# data: the seed name -- cases that share it share their inputs (the deterministic aligned / shifted pairs)
Case = namedtuple("Case", "name kind group M T N Cin k modes det mask bias scratch align gmul xmax plan data tags")


def _table():
    cases = []

    def add(name, kind, group, M, T, N, Cin, k, modes=None, det=False, mask="rand", bias=True, scratch=True, align="ok", gmul=1.0,
            xmax=None, plan=None, data=None, tags=()):
        assert M % T == 0, name
        modes = (("f32",) if kind == "f32" else X3) if modes is None else modes
        cases.append(Case(name, kind, group, M, T, N, Cin, k, tuple(modes), det, mask, bias, scratch, align, gmul, xmax, plan,
                          data or name, tuple(tags)))

    ROWS_D = (0, 1, 31, 32, 33, 64, 65, 96, 97)
    K3_T = ((1, 257), (2, 258), (3, 258), (5, 260), (7, 259), (9, 261), (31, 279), (32, 288), (33, 264), (36, 288), (48, 288), (100, 300))
    # ------------------------------------------------------------------------------------------------- lds128 (VRD_WGRAD_BIG=0)
    # With 256 CUs and a handful of tiles the chunk is the minimum of 128 rows: M = 256 + d gives chunks of 128, 128 and d rows.
    V, S = ("lds128", True, True, True), ("lds128", False, True, True)          # float4 / scalar loads, through the scratch
    for d in ROWS_D:          # last chunk of one to four steps, full and partial; both parities of the two-slab loop (vec, k = 1)
        add(f"l128_rows_d{d}_vec", "x3", "lds128", 256 + d, 1, 128, 128, 1, plan=V, tags=("rows",))
        add(f"l128_rows_d{d}_scalar", "x3", "lds128", 256 + d, 1, 127, 129, 1, plan=S, tags=("rows", "tail"))
    for T, M in K3_T:         # k = 3 sequence ends; scalar loads with a four-column group straddling a tap (Cin = 21, 63)
        add(f"l128_k3_t{T}_vec", "x3", "lds128", M, T, 128, 44, 3, mask="ends" if T in (5, 36) else "rand", plan=V, tags=("k3",))
        add(f"l128_k3_t{T}_scalar", "x3", "lds128", M, T, 132, 21 if T % 2 else 63, 3, plan=S, tags=("k3", "straddle"))
    add("l128_k3_t3_c63", "x3", "lds128", 258, 3, 132, 63, 3, plan=S, tags=("k3", "straddle"))
    add("l128_k3_t32_c21", "x3", "lds128", 288, 32, 132, 21, 3, plan=S, tags=("k3", "straddle"))
    for N, K in ((127, 127), (127, 129), (129, 127), (129, 129)):          # tile tails, one short and one past
        add(f"l128_tail_n{N}_k{K}", "x3", "lds128", 289, 1, N, K, 1, plan=S, tags=("tail",))
    for N, K in ((124, 132), (132, 124)):
        add(f"l128_tail_n{N}_k{K}_vec", "x3", "lds128", 289, 1, N, K, 1, plan=V, tags=("tail",))
    add("l128_tail_k3_c43", "x3", "lds128", 288, 36, 129, 43, 3, plan=S, tags=("tail", "k3"))          # K = 129
    # scalar loads three ways (N % 4: the tails above), and what decides the way out of a block
    add("l128_scalar_cin", "x3", "lds128", 289, 1, 128, 126, 1, plan=S, tags=("scalar_cin",))
    add("l128_scalar_ldg_odd", "x3", "lds128", 289, 1, 128, 128, 1, align="ldg_odd", plan=S, tags=("scalar_ld",))
    add("l128_scalar_ldx_odd_k3", "x3", "lds128", 288, 36, 128, 44, 3, align="ldx_odd", plan=S, tags=("scalar_ld", "k3"))
    add("l128_scalar_shift", "x3", "lds128", 289, 1, 128, 128, 1, align="shift", plan=S, tags=("scalar_shift",))
    for k, T, M, Cin in ((1, 1, 289, 128), (3, 36, 288, 44)):
        add(f"l128_atomics_k{k}_vec", "x3", "lds128", M, T, 128, Cin, k, scratch=False, plan=("lds128", True, True, False), tags=("atomics",))
        add(f"l128_atomics_k{k}_scalar", "x3", "lds128", M, T, 130, Cin + 1, k, scratch=False, plan=("lds128", False, True, False), tags=("atomics",))
    add("l128_atomics_dw_unaligned", "x3", "lds128", 289, 1, 128, 128, 1, align="dw_shift", plan=("lds128", True, True, False), tags=("atomics",))
    # exactly one chunk, `+=` into a non-zero dW: an LDS form takes one chunk only from 2 * 256 tiles on (N = 2048, K = 4096)
    add("l128_one_chunk", "x3", "lds128", 256, 1, 2048, 4096, 1, modes=("bf16",), plan=("lds128", True, False, False), tags=("one_chunk",))
    # masks: none, sequence ends, a whole 32-row step, a whole chunk (its partial tile must hold zeros), every row
    for mname, mask, T in (("none", None, 1), ("ends", "ends", 17), ("step", ("rows", 160, 192), 1), ("chunk", ("rows", 128, 256), 1), ("all", "all", 1)):
        add(f"l128_mask_{mname}", "x3", "lds128", 289, T, 128, 128, 1, mask=mask, plan=V, tags=("mask_" + mname,))
        add(f"l128_mask_{mname}_k3", "x3", "lds128", 289, 17, 132, 21, 3, mask=mask, plan=S, tags=("mask_" + mname, "k3"))
    add("l128_mask_chunk_atomics", "x3", "lds128", 289, 1, 128, 128, 1, mask=("rows", 128, 256), scratch=False, plan=("lds128", True, True, False),
        tags=("mask_chunk",))
    add("l128_nobias", "x3", "lds128", 289, 1, 128, 128, 1, bias=False, plan=V, tags=("nobias",))
    add("l128_nobias_k3", "x3", "lds128", 288, 36, 132, 21, 3, bias=False, plan=S, tags=("nobias", "k3"))
    for gname, gmul in (("1e-9", 1e-9), ("1e6", 1e6)):          # f16 planes at the gradient's own power of two (vrd_absmax_scale)
        add(f"l128_gscale_{gname}", "x3", "lds128", 289, 1, 128, 128, 1, modes=("f16",), gmul=gmul, plan=V, tags=("gscale",))
    add("l128_x4000", "x3", "lds128", 289, 1, 128, 128, 1, modes=("f16",), xmax=4000.0, plan=V, tags=("x4000",))
    # ------------------------------------------------------------------------------------------------- lds256 (VRD_WGRAD_BIG=2)
    B = ("lds256", True, True, True)
    for d in ROWS_D:
        add(f"l256_rows_d{d}", "x3", "lds256", 256 + d, 1, 256, 256, 1, plan=B, tags=("rows",))
    for T, M in K3_T:          # the 256 tile with k = 3 at sequence lengths that are no multiple of the 32-row step
        add(f"l256_k3_t{T}", "x3", "lds256", M, T, 256, 88, 3, mask="ends" if T in (5, 36) else "rand", plan=B, tags=("k3",))
    add("l256_k3_t18_rows_d1", "x3", "lds256", 306, 18, 260, 92, 3, plan=B, tags=("k3", "tail"))          # max_seq_len 144 / 8
    for T in (72, 144):          # ... / 2 and the level itself
        add(f"l256_k3_t{T}", "x3", "lds256", 288, T, 256, 88, 3, plan=B, tags=("k3",))
    for N, Cin in ((260, 256), (256, 260), (260, 260), (512, 256), (256, 516)):          # one column group past a tile; two tiles
        add(f"l256_tail_n{N}_k{Cin}", "x3", "lds256", 289, 1, N, Cin, 1, plan=B, tags=("tail",))
    # where the shape refuses the 256 tile: one short or one past in single columns (no float4 groups), or below 256
    for N, Cin, vec in ((255, 256, False), (257, 256, False), (256, 255, False), (256, 257, False), (252, 256, True), (256, 252, True)):
        add(f"l256_refused_n{N}_k{Cin}", "x3", "lds256", 289, 1, N, Cin, 1, plan=("lds128", vec, True, True), tags=("refused",))
    add("l256_refused_ldx_odd", "x3", "lds256", 289, 1, 256, 256, 1, align="ldx_odd", plan=("lds128", False, True, True), tags=("refused",))
    add("l256_refused_shift", "x3", "lds256", 289, 1, 256, 256, 1, align="shift", plan=("lds128", False, True, True), tags=("refused",))
    for k, T, M, Cin in ((1, 1, 289, 256), (3, 36, 288, 88)):
        add(f"l256_atomics_k{k}", "x3", "lds256", M, T, 256, Cin, k, scratch=False, plan=("lds256", True, True, False), tags=("atomics",))
    for mname, mask, T in (("none", None, 1), ("ends", "ends", 17), ("step", ("rows", 160, 192), 1), ("chunk", ("rows", 128, 256), 1), ("all", "all", 1)):
        add(f"l256_mask_{mname}", "x3", "lds256", 289, T, 256, 256, 1, mask=mask, plan=B, tags=("mask_" + mname,))
        add(f"l256_mask_{mname}_k3", "x3", "lds256", 289, 17, 256, 88, 3, mask=mask, plan=B, tags=("mask_" + mname, "k3"))
    add("l256_nobias", "x3", "lds256", 289, 1, 256, 256, 1, bias=False, plan=B, tags=("nobias",))
    for gname, gmul in (("1e-9", 1e-9), ("1e6", 1e6)):
        add(f"l256_gscale_{gname}", "x3", "lds256", 289, 1, 256, 256, 1, modes=("f16",), gmul=gmul, plan=B, tags=("gscale",))
    add("l256_x4000", "x3", "lds256", 288, 36, 256, 88, 3, modes=("f16",), xmax=4000.0, plan=B, tags=("x4000",))
    # --------------------------------------------------------------------------------------------------- wave (VRD_WGRAD_LDS=0)
    # split wave kernel (bias: a column-sum launch of its own) and the exact-f32 kernel.  Up to 256 rows are one workgroup (`+=`);
    # beyond, workgroups of 4 x 64 rows (split) / 4 x 128 rows (exact f32) add with atomics.
    one, many = ("wave", False, False, False), ("wave", False, True, False)
    for M in (1, 63, 64, 129):
        add(f"wave_m{M}", "x3", "wave", M, 1, 63, 65, 1, plan=one, tags=("rows", "tail", "one_chunk"))
        add(f"f32_m{M}", "f32", "wave", M, 1, 63, 65, 1, tags=("rows", "tail", "one_chunk"))
    for N, K in ((65, 63), (64, 64), (130, 5)):
        add(f"wave_tail_n{N}_k{K}", "x3", "wave", 129, 1, N, K, 1, plan=one, tags=("tail",))
        add(f"f32_tail_n{N}_k{K}", "f32", "wave", 129, 1, N, K, 1, tags=("tail",))
    for T, M in K3_T:
        Ms = M if T >= 31 else T * (130 // T)          # below 256 rows where the sequences are short, beyond otherwise
        add(f"wave_k3_t{T}", "x3", "wave", Ms, T, 65, 21, 3, mask="ends" if T in (5, 36) else "rand", plan=many if Ms > 256 else one, tags=("k3",))
        add(f"f32_k3_t{T}_c5", "f32", "wave", Ms, T, 65, 5, 3, mask="ends" if T in (5, 36) else "rand", tags=("k3", "few_channels"))
        add(f"f32_k3_t{T}_c8", "f32", "wave", Ms, T, 64, 8, 3, tags=("k3", "few_channels"))
    add("wave_k3_c5", "x3", "wave", 129, 43, 64, 5, 3, plan=one, tags=("k3", "few_channels"))
    add("wave_chunks_inside_a_sequence", "x3", "wave", 301, 43, 65, 21, 3, plan=many, tags=("k3", "boundary"))
    add("f32_chunks_inside_a_sequence", "f32", "wave", 559, 43, 65, 5, 3, tags=("k3", "boundary", "atomics"))
    add("f32_chunks_det", "f32", "wave", 559, 43, 65, 5, 3, det=True, data="f32_chunks_inside_a_sequence", tags=("k3", "det", "partials"))
    add("f32_chunks_det_dw_unaligned", "f32", "wave", 559, 43, 65, 8, 3, det=True, align="dw_shift", tags=("k3", "det", "partials"))
    for M in (1, 129):
        add(f"f32_det_m{M}", "f32", "wave", M, 1, 63, 65, 1, det=True, tags=("det",))
    for mname, mask, T in (("none", None, 1), ("ends", "ends", 17), ("step", ("rows", 160, 192), 1), ("chunk", ("rows", 0, 256), 1), ("all", "all", 1)):
        add(f"wave_mask_{mname}", "x3", "wave", 289, T, 65, 63, 1, mask=mask, plan=many, tags=("mask_" + mname,))
        add(f"wave_mask_{mname}_k3", "x3", "wave", 289, 17, 65, 21, 3, mask=mask, plan=many, tags=("mask_" + mname, "k3"))
        fm = ("rows", 0, 512) if mname == "chunk" else mask
        add(f"f32_mask_{mname}_k3", "f32", "wave", 561, 17 if T == 1 else T, 65, 5, 3, mask=fm, tags=("mask_" + mname, "k3"))
    add("wave_nobias", "x3", "wave", 129, 1, 63, 65, 1, bias=False, plan=one, tags=("nobias",))
    add("wave_noscratch", "x3", "wave", 289, 1, 63, 65, 1, scratch=False, plan=many, tags=("atomics",))
    for gname, gmul in (("1e-9", 1e-9), ("1e6", 1e6)):
        add(f"wave_gscale_{gname}", "x3", "wave", 129, 1, 64, 64, 1, modes=("f16",), gmul=gmul, plan=one, tags=("gscale",))
    add("wave_x4000", "x3", "wave", 129, 43, 64, 21, 3, modes=("f16",), xmax=4000.0, plan=one, tags=("x4000",))
    # ----------------------------------------------------------------------------------------------------- default (nothing set)
    # selection by shape ...
    add("def_wave_m255", "x3", "default", 255, 1, 128, 128, 1, plan=one, tags=("select",))
    add("def_lds128_m256", "x3", "default", 256, 1, 128, 128, 1, plan=V, tags=("select",))
    add("def_lds128_small_m", "x3", "default", 289, 1, 256, 256, 1, plan=V, tags=("select",))          # 256 wide, too few rows
    add("def_lds256_by_rows", "x3", "default", 4097, 1, 1024, 1024, 1, modes=("bf16",), mask=None, plan=("lds256", True, True, True),
        data="det_l256_k1", tags=("select", "heavy"))
    # ... and the deterministic mode, which ignores both switches and the alignment: every reachable DET instantiation, ragged N
    # and K with the bias rows behind the partial tiles, and each shape once aligned and once one float off (the same bits)
    DV, DS = ("lds128", True, True, True), ("lds128", False, True, True)
    for k, T, M, Cin in ((1, 1, 289, 128), (3, 36, 288, 44)):
        add(f"det_l128_k{k}", "x3", "default", M, T, 128, Cin, k, det=True, plan=DV, tags=("det", "pair_a"))
        add(f"det_l128_k{k}_shift", "x3", "default", M, T, 128, Cin, k, det=True, align="shift", plan=DS, data=f"det_l128_k{k}", tags=("det", "pair_b"))
    for N, Cin, k, T, M in ((127, 129, 1, 1, 289), (129, 43, 3, 36, 288), (130, 21, 3, 3, 258), (65, 63, 3, 100, 300)):
        add(f"det_l128_ragged_n{N}_c{Cin}_k{k}", "x3", "default", M, T, N, Cin, k, det=True, plan=DS, tags=("det", "ragged"))
    add("det_l128_ragged_vec", "x3", "default", 289, 1, 132, 124, 1, det=True, plan=DV, tags=("det", "ragged"))
    add("det_l128_nobias", "x3", "default", 289, 1, 127, 129, 1, det=True, bias=False, plan=DS, tags=("det", "nobias"))
    add("det_l128_dw_unaligned", "x3", "default", 289, 1, 127, 129, 1, det=True, align="dw_shift", plan=DS, tags=("det",))
    add("det_l128_mask_chunk", "x3", "default", 289, 1, 127, 129, 1, det=True, mask=("rows", 128, 256), plan=DS, tags=("det", "mask_chunk"))
    add("det_l128_mask_all", "x3", "default", 289, 1, 132, 124, 1, det=True, mask="all", plan=DV, tags=("det", "mask_all"))
    for M in (1, 129, 255):
        add(f"det_wave_m{M}", "x3", "default", M, 1, 63, 65, 1, det=True, plan=one, tags=("det",))
    add("det_wave_k3", "x3", "default", 129, 43, 65, 21, 3, det=True, plan=one, tags=("det", "k3"))
    # deterministic 256 tiles need M * ceil(N/256) * ceil(K/256) >= 65536
    DB, DBS = ("lds256", True, True, True), ("lds256", False, True, True)
    add("det_l256_k1", "x3", "default", 4097, 1, 1024, 1024, 1, det=True, mask=None, plan=DB, tags=("det", "heavy", "pair_a"))
    add("det_l256_k1_shift", "x3", "default", 4097, 1, 1024, 1024, 1, det=True, mask=None, align="shift", plan=DBS, data="det_l256_k1",
        tags=("det", "heavy", "pair_b"))
    add("det_l256_k3", "x3", "default", 5472, 36, 512, 512, 3, det=True, plan=DB, tags=("det", "heavy", "pair_a", "k3"))
    add("det_l256_k3_shift", "x3", "default", 5472, 36, 512, 512, 3, det=True, align="shift", plan=DBS, data="det_l256_k3",
        tags=("det", "heavy", "pair_b", "k3"))
    # -------------------------------------------------------------------------------------------------------------------- dgrad
    # dx (M, Cin) = dy (M, N) against the transposed, tap-flipped operand: K = N * k, the output width Cin at the tile tails, the
    # smallest admissible N (N * k % 32 == 0, N % 4 == 0), dy in a wider buffer.  k = 1 with a row mask; k = 3 over sequence ends.
    for group, tile in (("dgrad128", 128), ("dgrad64", 64)):
        for Cin in (tile - 1, tile, tile + 1, 5):
            add(f"{group}_k1_c{Cin}", "dgrad", group, 200, 1, 32, Cin, 1, tags=("tail",))
        add(f"{group}_k1_m1", "dgrad", group, 1, 1, 32, tile + 1, 1, mask=None, tags=("rows",))
        add(f"{group}_k1_m{tile + 1}_n64", "dgrad", group, tile + 1, 1, 64, tile - 1, 1, mask="all", tags=("rows",))
        add(f"{group}_k1_n36", "dgrad", group, 130, 1, 36 * 8, 8, 1, tags=("tail",))
        add(f"{group}_k1_ldc_odd", "dgrad", group, 130, 1, 32, tile + 1, 1, align="ldc_odd", tags=("unstaged",))
        for T, M in ((1, 130), (2, 130), (3, 129), (7, 133), (33, 132), (36, 144)):
            add(f"{group}_k3_t{T}", "dgrad", group, M, T, 32, tile + 1 if T % 2 else tile - 1, 3, mask=None, tags=("k3",))
        add(f"{group}_k3_n64_c5", "dgrad", group, 144, 36, 64, 5, 3, mask=None, tags=("k3", "few_channels"))
        for gname, gmul in (("1e-9", 1e-9), ("1e6", 1e6)):
            add(f"{group}_gscale_{gname}", "dgrad", group, 130, 1, 32, tile + 1, 1, modes=("f16",), gmul=gmul, tags=("gscale",))
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _table()
BY_NAME = {c.name: c for c in CASES}


def cases_of(group):
    return [c for c in CASES if c.group == group]


# --------------------------------------------------------------------------------------------------------------- layout
def _up4(n):
    return (n + 3) // 4 * 4


def layout(case):
    """leading dimensions and first columns of the case's windows, and dW's offset in floats from a 16-byte line: what the plan
    reads besides the shapes (one source for make_inputs and plan_of)"""
    lds = W.LdSeq()
    ldg, ldx, ldc = lds(_up4(case.N)), lds(_up4(case.Cin)), lds(_up4(case.Cin))
    cg = cx = W.C0
    if case.align == "ldg_odd":
        ldg += 1
    if case.align == "ldx_odd":
        ldx += 1
    if case.align == "ldc_odd":
        ldc += 1
    if case.align == "shift":
        cg, cx = W.C0 + 1, W.C0 + 1
    return {"ldg": ldg, "ldx": ldx, "ldc": ldc, "cg": cg, "cx": cx, "dw_off": 1 if case.align == "dw_shift" else 0}


# ----------------------------------------------------------------------------------------------------------------- plan
Plan = namedtuple("Plan", "form vec tiles chunk chunks tile_partials")


def plan_of(case, n_cu=DET_CUS):
    """Mirror of plan_wgrad_x3 / vrd_gemm_wgrad (csrc/vrd_wgrad.hip) for the case's group, layout and a device of n_cu compute
    units -- what the emulation takes its chunk order from and what the CPU test holds the table's named plans against; the GPU
    test asks the library itself (vrd_gemm_wgrad_x3_plan)."""
    M, N, K = case.M, case.N, case.Cin * case.k
    if case.kind == "f32":
        chunks = (M + 511) // 512
        return Plan("wave", False, ((N + 63) // 64) * ((K + 63) // 64), 128, chunks, case.det and chunks > 1)
    lay = layout(case)
    cu = DET_CUS if case.det else n_cu
    use_lds = case.group != "wave"
    big_mode = {"lds128": 0, "lds256": 2}.get(case.group, 1)
    if (case.det or use_lds) and M >= 256:
        vec_shape = N % 4 == 0 and case.Cin % 4 == 0 and lay["ldg"] % 4 == 0 and lay["ldx"] % 4 == 0
        vec = vec_shape and lay["cg"] % 4 == 0 and lay["cx"] % 4 == 0
        big_tiles = ((N + 255) // 256) * ((K + 255) // 256)
        enough = M * big_tiles >= 256 * cu
        if case.det:
            big = vec_shape and N >= 256 and K >= 256 and enough
        else:
            big = big_mode != 0 and vec and N >= 256 and K >= 256 and (big_mode == 2 or enough)
        tile = 256 if big else 128
        tiles = ((N + tile - 1) // tile) * ((K + tile - 1) // tile)
        want = max(1, ((1 if big else 2) * cu + tiles - 1) // tiles)
        chunk = max(128, ((M + want - 1) // want + 31) // 32 * 32)
        chunks = (M + chunk - 1) // chunk
        partials = chunks > 1 and (case.det or (case.scratch and lay["dw_off"] == 0))
        return Plan("lds256" if big else "lds128", vec, tiles, chunk, chunks, partials)
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    want = max(1, (2 * cu + tiles - 1) // tiles)
    chunk = min(1024, max(64, ((M + 4 * want - 1) // (4 * want) + 31) // 32 * 32))
    chunks = (M + 4 * chunk - 1) // (4 * chunk)
    return Plan("wave", False, tiles, chunk, chunks, case.det and chunks > 1)


def block_rows(case, plan):
    """rows per workgroup (one partial tile / one atomic per element each)"""
    return plan.chunk * (4 if plan.form == "wave" else 1)


def rounding_count(case, plan):
    """R of the module docstring for a plan (form, chunk, chunks)"""
    M = case.M
    if plan.form == "wave":
        per, r = (16, 16) if case.kind == "f32" else (6, 32)          # roundings per r rows of a wave (f32: 8 MFMAs x 2 per 16 rows)
        waves = -(-M // plan.chunk)
        mfma = sum(per * -(-min(plan.chunk, M - w * plan.chunk) // r) for w in range(waves))
        return mfma + 3 * plan.chunks + plan.chunks + 2
    steps = sum(-(-min(plan.chunk, M - c * plan.chunk) // 32) for c in range(plan.chunks))
    return 6 * steps + plan.chunks + 2


# --------------------------------------------------------------------------------------------------------------- inputs
class Flat:
    """a flat f32 region of `n` floats between two guard bands of sentinel NaNs, `off` floats past a 16-byte line"""

    def __init__(self, n, device, name, off=0, guard=64, fill=None):
        self.n, self.start, self.name = n, guard + off, name
        bits = torch.full((n + 2 * guard + off,), W.SENTINEL_BITS, dtype=torch.int32, device=device)
        self.buf = bits.view(torch.float32)
        self.view = self.buf[self.start:self.start + n]
        if fill is not None:
            self.view.copy_(fill.reshape(-1))
        self.before = bits.clone()

    def guards_intact(self):
        now = self.buf.view(torch.int32)
        same = now == self.before
        same[self.start:self.start + self.n] = True
        assert bool(same.all()), f"guard elements of '{self.name}' were written: {int((~same).sum())}, first at float {int(torch.nonzero(~same)[0]) - self.start}"

    def unchanged(self):
        assert bool((self.buf.view(torch.int32) == self.before).all()), f"'{self.name}' was written"


class Inputs:
    pass


def absmax_exp(t):
    """e of vrd_absmax_scale: max |t| * 2^e in [2^13, 2^14) (0 for an all-zero matrix)"""
    m = float(t.abs().max())
    if m == 0.0 or not math.isfinite(m):
        return 0
    return max(-100, min(100, 14 - math.frexp(m)[1]))


def make_mask(case):
    M, T = case.M, case.T
    if case.mask is None:
        return None
    if case.mask == "rand":
        gen = torch.Generator().manual_seed(zlib.crc32(("mask " + case.data).encode()))
        return torch.rand(M, generator=gen) < 0.8
    if case.mask == "ends":
        t = torch.arange(M) % T
        return (t != 0) & (t != T - 1)
    if case.mask == "all":
        return torch.zeros(M, dtype=torch.bool)
    kind, a, b = case.mask
    m = torch.ones(M, dtype=torch.bool)
    m[a:b] = False
    return m


def make_inputs(case, mode, device="cpu"):
    """Seeded operands of `case` (by case.data) in poisoned windows of their own leading dimensions; outputs start from seeded
    non-zero values (dW, db) or the sentinel (dx), the scratch -- made by the caller -- from NaN."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.data.encode()))
    M, T, N, Cin, k = case.M, case.T, case.N, case.Cin, case.k
    lay = layout(case)
    inp = Inputs()
    inp.case, inp.mode, inp.device = case, mode, device
    g = torch.randn(M, N, generator=gen) * case.gmul
    if case.kind == "dgrad":
        w = torch.randn(N, Cin, k, generator=gen) / (N * k) ** 0.5
        inp.w = w
        inp.mask = make_mask(case)
        inp.hG = GT._embed3(g.reshape(M // T, T, N).to(device), ld=lay["ldg"], c0=lay["cg"], name="dy")
        inp.hX = None
        inp.hC = GT._embed3(torch.empty(M // T, T, Cin, device=device), out=True, ld=lay["ldc"], name="dx")
        inp.gexp = absmax_exp(g)
        return inp
    x = torch.randn(M, Cin, generator=gen)
    xs = 1.0
    if case.xmax is not None:          # |x| up to xmax: inside the f16 operand range (|x| * 2^4 < 65504), no flag involved
        x = (torch.rand(M, Cin, generator=gen) * 2 - 1) * case.xmax
        x[0, 0] = case.xmax
        xs = case.xmax / 2
    scale = case.gmul * xs
    inp.dw0 = torch.randn(N, Cin * k, generator=gen) * scale
    inp.db0 = torch.randn(N, generator=gen) * case.gmul
    inp.mask = make_mask(case)
    inp.hG = W.embed(g.to(device), ld=lay["ldg"], c0=lay["cg"], name="G")
    inp.hX = W.embed(x.to(device), ld=lay["ldx"], c0=lay["cx"], name="X")
    inp.fW = Flat(N * Cin * k, device, "dW", off=lay["dw_off"], fill=inp.dw0.to(device))
    inp.fB = Flat(N, device, "db", fill=inp.db0.to(device)) if case.bias and case.kind == "x3" else None
    inp.gexp = absmax_exp(g)
    return inp


# ------------------------------------------------------------------------------------------------------------ reference
def planes(t, mode, exp):
    """(hi, lo) f32 tensors: the 16-bit planes of t (f16: of t * 2^exp), or (t, None) in the f32 mode"""
    if mode == "f32":
        return t, None
    dt = torch.float16 if mode == "f16" else torch.bfloat16
    y = t * 2.0 ** exp if mode == "f16" else t
    hi = y.to(dt).float()
    return hi, (y - hi).to(dt).float()


def as_split(t, mode, exp):
    """float64: the operand as the kernel splits it, hi + lo (unscaled again)"""
    hi, lo = planes(t, mode, exp)
    if lo is None:
        return hi.double()
    v = hi.double() + lo.double()
    return v * 2.0 ** -exp if mode == "f16" else v


def _im2col(t, T, k, ends=True):
    """(M, C) -> (M, k * C) tap-major: column tap * C + c of row r holds t[r + tap - 1, c], zero outside r's length-T sequence
    (ends=False: the neighbouring sequence's row instead -- a fault stand-in)"""
    if k == 1:
        return t
    M, C = t.shape
    z = torch.zeros_like(t[:1])
    prev, nxt = torch.cat([z, t[:-1]]), torch.cat([t[1:], z])
    if ends:
        pos = torch.arange(M) % T
        prev = prev * (pos != 0).to(t.dtype)[:, None]
        nxt = nxt * (pos != T - 1).to(t.dtype)[:, None]
    return torch.cat([prev, t, nxt], 1)


_products = {}          # the last contractions, by data and shape: the aligned / shifted pairs share theirs


def _wgrad_products(inp):
    """float64 (G_masked^T X_col, |G_masked|^T |X_col|, column sums of the masked f32 G, of |G|) of a case's inputs"""
    case, mode = inp.case, inp.mode
    key = (case.data, mode, case.M, case.T, case.N, case.Cin, case.k, case.mask, case.xmax, case.gmul)
    if key not in _products:
        while len(_products) >= 2:
            _products.pop(next(iter(_products)))
        g, x = inp.hG.view.cpu(), inp.hX.view.cpu()
        mk = inp.mask.double()[:, None] if inp.mask is not None else 1.0
        gs = as_split(g, mode, inp.gexp if mode == "f16" else 0) * mk
        xc = _im2col(as_split(x, mode, ACT_EXP), case.T, case.k)
        gm = g.double() * mk
        _products[key] = (gs.T @ xc, gs.abs().T @ xc.abs(), gm.sum(0), gm.abs().sum(0))
    return _products[key]


def reference(inp):
    """wgrad: float64 (dW_ref, mag, db_ref, sum |g|); dgrad: (dx_ref, mag, lip) -- from the operands as split"""
    case, mode = inp.case, inp.mode
    if case.kind != "dgrad":
        prod, mag, gsum, gabs = _wgrad_products(inp)
        return inp.dw0.double() + prod, mag, inp.db0.double() + gsum, gabs
    B, T = case.M // case.T, case.T
    dy = as_split(inp.hG.view.cpu().reshape(case.M, case.N), mode, inp.gexp if mode == "f16" else 0).reshape(B, T, case.N)
    wt = inp.w.double().permute(1, 0, 2).flip(2)          # (Cin, N, k): dx[r] = sum_tap dy[r + 1 - tap] W[:, :, tap]
    conv = lambda a, b: F.conv1d(a.transpose(1, 2), b, None, padding=case.k // 2).transpose(1, 2)          # noqa: E731
    lip = inp.mask.double().reshape(B, T, 1) if inp.mask is not None else torch.ones(B, T, 1, dtype=torch.float64)
    ref, mag = conv(dy, wt) * lip, conv(dy.abs(), wt.abs())
    return ref, mag, lip.expand_as(ref)


# `slack`: the share of the rounding terms granted (1: the bound; 0.5: what the emulation has to meet, see the module docstring)
def bound_dw(case, mode, plan, ref, mag, dw0, slack=1.0):
    return U[mode] * mag + slack * (rounding_count(case, plan) * 2.0 ** -24 * mag + 2.0 ** -23 * (ref.abs() + dw0.double().abs()))


def bound_db(case, plan, gabs, db0, slack=1.0):
    return slack * ((case.M + plan.chunks) * 2.0 ** -24 * gabs + plan.chunks * 2.0 ** -23 * db0.double().abs())


def bound_dx(case, mode, ref, mag, lip, slack=1.0):
    return U[mode] * mag * lip + slack * ((case.N * case.k / 32 + 2) * 2.0 ** -24 * mag * lip + 2.0 ** -23 * ref.abs())


# -------------------------------------------------------------------------------------------------------------- checker
def _check(case, mode, what, got, ref, bnd, where):
    """every element of got within bnd of ref; returns the largest error-to-bound ratio (0 / 0 counts as 0)"""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bnd)                      # (a NaN in got is bad)
    if bool(bad.any()):
        idx = torch.nonzero(bad.reshape(ref.shape[0], -1) if ref.dim() > 1 else bad.reshape(-1, 1))
        flat = lambda t: t.reshape(ref.shape[0], -1) if ref.dim() > 1 else t.reshape(-1, 1)          # noqa: E731
        lines = [f"{where(r, c)}: got {float(flat(got)[r, c])!r}, want {float(flat(ref)[r, c])!r}, |diff| {float(flat(err)[r, c]):.3e} > bound {float(flat(bnd)[r, c]):.3e}"
                 for r, c in idx[:6].tolist()]
        raise AssertionError(f"case {case.name} [{mode}] {what}: {len(idx)} of {got.numel()} elements outside the bound, rows "
                             f"{int(idx[:, 0].min())}..{int(idx[:, 0].max())}, columns {int(idx[:, 1].min())}..{int(idx[:, 1].max())}\n  " + "\n  ".join(lines))
    ok = bnd > 0
    return float((err[ok] / bnd[ok]).max()) if bool(ok.any()) else 0.0


def verify(inp, plan, scratch=None, slack=1.0):
    """The checks of one case after the op (or its emulation) ran: guards intact, inputs unchanged, every output element finite
    (an element of dx never written is still the sentinel) and within its bound.  Returns {what: largest error-to-bound ratio}."""
    case, mode = inp.case, inp.mode
    tag = f"case {case.name} [{mode}]: "
    try:
        for h in (inp.hG, inp.hX):
            if h is not None:
                W.assert_unchanged(h)
        if case.kind == "dgrad":
            W.check([inp.hC])
        else:
            for f in (inp.fW, inp.fB, scratch):
                if f is not None:
                    f.guards_intact()
    except AssertionError as e:
        raise AssertionError(tag + str(e)) from None
    if case.kind == "dgrad":
        ref, mag, lip = reference(inp)
        where = lambda r, c: f"row {r} (frame {r % case.T} of {case.T}) channel {c}"          # noqa: E731
        got = inp.hC.result().cpu().reshape(case.M, case.Cin)
        return {"dx": _check(case, mode, "dx", got, ref.reshape(case.M, case.Cin), bound_dx(case, mode, ref, mag, lip, slack).reshape(case.M, case.Cin), where)}
    ref, mag, dbref, gabs = reference(inp)
    K = case.Cin * case.k
    got = inp.fW.view.cpu().reshape(case.N, K)
    assert bool(torch.isfinite(got).all()), tag + f"dW holds {int((~torch.isfinite(got)).sum())} elements that are not finite (stale scratch, or computed from a guard)"
    tile = {"wave": 64, "lds128": 128, "lds256": 256}[plan.form]
    where = lambda n, j: f"dW[{n}, {j}] ({tile} x {tile} tile ({n // tile}, {j // tile}), tap {j // case.Cin} channel {j % case.Cin})"          # noqa: E731
    out = {"dW": _check(case, mode, "dW", got, ref, bound_dw(case, mode, plan, ref, mag, inp.dw0, slack), where)}
    if inp.fB is not None:
        gb = inp.fB.view.cpu()
        assert bool(torch.isfinite(gb).all()), tag + "db holds elements that are not finite"
        out["db"] = _check(case, mode, "db", gb, dbref, bound_db(case, plan, gabs, inp.db0, slack), lambda n, _: f"db[{n}]")
    return out


# ------------------------------------------------------------------------------------------------------------ emulation
FAULTS = ("row_dropped_at_chunk_boundary", "tap_across_sequence_end", "rows_past_m_contracted", "lo_hi_product_left_out",
          "k_tail_from_neighbouring_tap", "mask_byte_of_neighbouring_row", "partial_tile_missing", "dw_overwritten", "bias_from_unmasked_rows")


def emulate(inp, plan, fault=None):
    """The arithmetic of the kernels in f32 on the CPU: the three products of the planes formed and accumulated in f32, workgroup
    by workgroup in chunk order (partial tiles: summed first, then added to dW; otherwise added to dW one after the other), the
    bias as f32 column sums of the masked rows; dgrad: K step by K step as tests/gemm_tile_cases.py does.  `fault`: one of FAULTS,
    the Python stand-in of a kernel fault."""
    case, mode = inp.case, inp.mode
    M, T, N, Cin, k = case.M, case.T, case.N, case.Cin, case.k
    g = inp.hG.view.cpu().reshape(M, N)
    if case.kind == "dgrad":
        assert fault is None
        gexp = inp.gexp if mode == "f16" else 0
        ah, al = planes(g, mode, gexp)
        ah, al = _im2col(ah, T, k), _im2col(al, T, k)
        wt = inp.w.permute(1, 0, 2).flip(2).permute(0, 2, 1).reshape(Cin, k * N)          # (Cin, tap-major K)
        wexp = E.weight_exp(inp.w) if mode == "f16" else 0
        wh, wl = planes(wt, mode, wexp)
        acc = torch.zeros(M, Cin)
        for s in range(N * k // 32):
            sl = slice(32 * s, 32 * s + 32)
            acc = acc + al[:, sl] @ wh[:, sl].T
            acc = acc + ah[:, sl] @ wl[:, sl].T
            acc = acc + ah[:, sl] @ wh[:, sl].T
        v = acc * (2.0 ** -(gexp + wexp) if mode == "f16" else 1.0)
        if inp.mask is not None:
            v = v * inp.mask.float()[:, None]
        inp.hC.buf[inp.hC.row0:inp.hC.row0 + M, inp.hC.c0:inp.hC.c0 + Cin] = v
        return inp
    x = inp.hX.view.cpu()
    mask = inp.mask if inp.mask is not None else torch.ones(M, dtype=torch.bool)
    if fault == "mask_byte_of_neighbouring_row":
        mask = torch.cat([mask[1:], mask[-1:]])
    gm = g * mask.float()[:, None]
    if fault == "rows_past_m_contracted":          # the last step contracts up to its 32nd row: the row behind M is the last row again
        assert M % 32 and k == 1
        gm, x = torch.cat([gm, g[-1:]]), torch.cat([x, x[-1:]])
    rows = block_rows(case, plan)
    if fault == "row_dropped_at_chunk_boundary":
        assert plan.chunks > 1
        gm = gm.clone()
        gm[rows] = 0.0
    gexp = inp.gexp if mode == "f16" else 0
    gh, gl = planes(gm, mode, gexp)
    xh, xl = planes(x, mode, ACT_EXP)
    cols = lambda p: _im2col(p, T, k, ends=fault != "tap_across_sequence_end")          # noqa: E731
    xh, xl = cols(xh), (cols(xl) if xl is not None else None)
    if fault == "k_tail_from_neighbouring_tap":
        assert k == 3
        xh, xl = xh.clone(), xl.clone()
        xh[:, -1], xl[:, -1] = xh[:, -1 - Cin], xl[:, -1 - Cin]
    unscale = 2.0 ** -(gexp + ACT_EXP) if mode == "f16" else 1.0
    parts = []
    for c in range(plan.chunks):
        sl = slice(c * rows, (c + 1) * rows)
        if gl is None:
            acc = gh[sl].T @ xh[sl]
        else:
            acc = torch.zeros(N, Cin * k)
            if fault != "lo_hi_product_left_out":
                acc = acc + gl[sl].T @ xh[sl]
            acc = acc + gh[sl].T @ xl[sl]
            acc = acc + gh[sl].T @ xh[sl]
        parts.append(acc * unscale)
    if fault == "partial_tile_missing":
        assert plan.tile_partials
        del parts[1]
    dw = torch.zeros_like(inp.dw0) if fault == "dw_overwritten" else inp.dw0.clone()
    if plan.tile_partials:
        s = parts[0]
        for p in parts[1:]:
            s = s + p
        dw = dw + s
    else:
        for p in parts:
            dw = dw + p
    inp.fW.view.copy_(dw.reshape(-1))
    if inp.fB is not None:
        src = g if fault == "bias_from_unmasked_rows" else g * mask.float()[:, None]
        db = inp.db0.clone()
        for c in range(plan.chunks):
            db = db + src[c * rows:(c + 1) * rows].sum(0)
        inp.fB.view.copy_(db)
    return inp
