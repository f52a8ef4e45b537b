"""Small-shape cases for the split-precision GEMM kernels (tests/test_gemm_tile_cases_cpu.py, tests/test_gpu_gemm_tiles.py).

The 256 x 256 and 128 x 256 LDS-DMA kernels serve only problems of 512 tiles or more by default, where a float64 reference of
every output element is out of reach.  The kernel-selection switches of csrc/ force them onto problems of a few hundred rows;
this module holds the case table, the pair-row encoding, the float64 reference of the whole output, the derived tolerance, the
checker, and an f32 emulation of the three-product arithmetic that shows the reference alone stays inside the tolerance (and
that carries Python stand-ins of the faults the GPU tests exist to catch).  Nothing here needs a GPU.

Tolerance (per element, derived -- not measured on the kernels).  With K = Cin * k, mag = sum |a| |w| over the contraction:

    |got - ref| <= (u + (K/32 + 2) * 2^-24) * mag * lip  +  2^-23 * |ref|

  u      the split's own error: a w ~= a_hi w_hi + a_hi w_lo + a_lo w_hi drops a_lo w_lo (2^-9 * 2^-9 = 2^-18 of |a w| for
         bf16 planes of 8 significand bits, 2^-22 for f16 planes of 11) and the two lo planes are themselves rounded (2^-9 *
         2^-9 resp. 2^-11 * 2^-11 each): u = 3 * 2^-18 (bf16x3), 3 * 2^-22 (f16x3).  The reference is computed from the DECODED
         pair rows, so the rounding of the input to hi + lo is not counted against the kernel;
  K/32+2 f32 roundings of the accumulator, 2^-24 each relative to at most mag: the MFMA adds a 32-wide product block per
         instruction -- three per K step, bounded here as one rounding per step of the exact three-product sum plus two for the
         split of a step into its products (the emulation below confirms the count is generous);
  lip    what the epilogue multiplies an accumulator error by, never above 1: row_mask (0 or 1) * min(1, |scale|).  The
         activations have slope <= 1 except GELU's 1.13 near x = 1.4, which is NOT granted: the bound is the one above;
  2^-23  the epilogue's own f32 steps (bias, mask * scale, residual sums), two roundings relative to the result.

Pair output: the decoded value lies within 2^-15 relative of the f32 output of the same call (|x| floored at 1e-3).
f16x1 cases: the float64 emulation of the mode's operand rounding (tests/f16x1_emulation.py) must be 100 x closer to the
result than the three-product result of the same call is (`err * 100 < gap`)."""
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

import f16x1_emulation as E
import window_cases as W

ACT_EXP = E.ACT_EXP                    # VRD_F16_ACT_EXP: f16 planes hold x * 2^4
X3 = ("bf16x3", "f16x3")
U = {"bf16x3": 3 * 2.0 ** -18, "f16x3": 3 * 2.0 ** -22}
BIG_GROUPS = ("big", "big_one_tile", "big_grid2", "big_grid3")
ALL6 = ("big", "big_one_tile", "big_grid2", "dma", "x3_128", "x3_64")          # the groups of the agreement claim
GROUP_ENV = {
    "big": {"VRD_X3_BIG_MIN_TILES": "1", "VRD_X3_DMA_MIN_TILES": "1"},
    "big_one_tile": {"VRD_X3_BIG_MIN_TILES": "1", "VRD_X3_DMA_MIN_TILES": "1", "VRD_BIG_PERSIST": "0"},
    "big_grid2": {"VRD_X3_BIG_MIN_TILES": "1", "VRD_X3_DMA_MIN_TILES": "1", "VRD_BIG_GRID": "2"},
    "big_grid3": {"VRD_X3_BIG_MIN_TILES": "1", "VRD_X3_DMA_MIN_TILES": "1", "VRD_BIG_GRID": "3"},
    "dma": {"VRD_X3_BIG_MIN_TILES": "100000000", "VRD_X3_DMA_MIN_TILES": "1"},
    "x3_128": {"VRD_X3_DMA": "0", "VRD_X3_SMALL": "0"},
    "x3_64": {"VRD_X3_DMA": "0"},
}
GROUP_FAMILY = {"big": "K_GEMM_X3_BIG", "big_one_tile": "K_GEMM_X3_BIG", "big_grid2": "K_GEMM_X3_BIG", "big_grid3": "K_GEMM_X3_BIG",
                "dma": "K_GEMM_X3_DMA", "x3_128": "K_GEMM_X3", "x3_64": "K_GEMM_X3"}

# epi: the epilogue terms present, out of bias / relu / gelu / mask / scale / res (unmasked) / res_masked / res2
# layout: "plain"; "pad_map" (row_mask and the padding map made from it); "pad_skip" (the padding map without row_mask: skipped
#         rows hold filler); "batch3" (three problems through conv_gemm_batch)
# agree: "bits" -- a bias-only case every split kernel accepts, whose f32 output must be the same bits on ALL6; "other" --
#        another epilogue on such a shape, compared across ALL6 as well (see tests/test_gpu_gemm_tiles.py); None
Case = namedtuple("Case", "name B T Cin N k epi layout pair_out groups modes agree")


def _table():
    cases = []

    def add(name, B, T, Cin, N, k, epi=("bias",), layout="plain", pair_out=False, groups=(), modes=X3, agree=None):
        cases.append(Case(name, B, T, Cin, N, k, tuple(epi), layout, pair_out, tuple(groups), tuple(modes), agree))

    one = ("big", "big_one_tile")
    # ---- 256 x 256 kernel: K steps 3 .. 9 (M = 512, N = 512), bias only (persistent under `big`) and with row_mask (one-tile form)
    for Cin in (96, 128, 160, 192, 224, 256, 288):
        add(f"big_ksteps_c{Cin}", 2, 256, Cin, 512, 1, groups=one)
        add(f"big_ksteps_c{Cin}_mask", 2, 256, Cin, 512, 1, epi=("bias", "mask"), groups=one)
    for Cin in (192, 256, 320, 448):             # f16x1: K steps of 64, 3 .. 7
        add(f"big_ksteps_x1_c{Cin}", 2, 256, Cin, 512, 1, groups=one, modes=("f16x1",))
    # ---- ring carry: 14 tiles (M = 1792, N = 512) on two workgroups, seven tiles each; on three, chains of 5, 5, 4
    for Cin in (96, 160, 192, 224):
        add(f"big_ring_c{Cin}", 7, 256, Cin, 512, 1, groups=("big_grid2",) + (("big_grid3",) if Cin == 160 else ()))
    add("big_ring_c160_gelu", 7, 256, 160, 512, 1, epi=("bias", "gelu"), groups=("big_grid2",))
    add("big_ring_c160_pair", 7, 256, 160, 512, 1, pair_out=True, groups=("big_grid2",))
    add("big_ring_c160_batch3", 7, 256, 160, 512, 1, layout="batch3", groups=("big_grid2", "big_grid3"))
    add("big_ring_c160_pad_skip", 7, 256, 160, 512, 1, layout="pad_skip", groups=("big_grid2",))
    add("big_ring_x1_c320", 7, 256, 320, 512, 1, groups=("big_grid2",), modes=("f16x1",))
    # ---- tile tails of 64, 128 and 192 rows / columns, f32 and pair output
    for M in (320, 384, 448, 576):
        for N in (256, 320, 384, 448):
            add(f"big_tail_m{M}_n{N}", M // 64, 64, 128, N, 1, groups=("big",))
            add(f"big_tail_m{M}_n{N}_pair", M // 64, 64, 128, N, 1, pair_out=True, groups=("big",))
    # ---- k = 3: sequence ends at every offset inside the 8-row DMA pieces; at Cin = 32 the tap changes at every K step
    for T, B in ((32, 10), (36, 16), (40, 8), (50, 32), (288, 2)):
        for Cin in (32, 64, 96):
            add(f"big_k3_t{T}_c{Cin}", B, T, Cin, 256, 3, epi=("bias", "mask"), groups=("big",))
            if T in (36, 50):
                add(f"big_k3_t{T}_c{Cin}_pad_map", B, T, Cin, 256, 3, epi=("bias", "mask"), layout="pad_map", groups=("big",))
    # ---- every epilogue form the lean epilogue admits (M = 512, N = 320, Cin = 128), f32 and pair output, on every kernel
    forms = {"nobias": (), "bias": ("bias",), "gelu": ("bias", "gelu"), "mask": ("bias", "mask"), "scale": ("bias", "scale"),
             "resm": ("bias", "mask", "res_masked"), "res": ("bias", "res"), "res2": ("bias", "res2"),
             "all": ("bias", "mask", "scale", "res_masked", "res2")}
    for k in (1, 3):
        for fname, epi in forms.items():
            for pair in (False, True):
                add(f"epi_k{k}_{fname}" + ("_pair" if pair else ""), 8, 64, 128, 320, k, epi=epi, pair_out=pair, groups=ALL6,
                    agree=None if (fname == "bias" and not pair) else "other")
    # ---- 128 x 256 kernel (and, pair-row A, the register-staged 128 x 128 / 64 x 64 kernels)
    small = ("dma", "x3_128", "x3_64")
    for Cin in (32, 64, 96, 128, 160, 224):          # K steps 1 .. 7: fewer steps than ring stages at 1 and 2
        add(f"dma_ksteps_c{Cin}", 8, 32, Cin, 256, 1, groups=small)
    add("dma_ksteps_k3_c32", 8, 32, 32, 256, 3, groups=small)
    # row and column tails (clamped to the last row / column), both extremes of each
    for M, N in ((1, 192), (1, 508), (257, 192), (257, 508), (7, 196), (127, 197), (129, 256), (130, 260), (200, 300),
                 (257, 197), (7, 508), (127, 300), (130, 197)):
        add(f"dma_tail_m{M}_n{N}", 1, M, 64, N, 1, groups=small)
    for T, B in ((1, 130), (2, 100), (3, 50), (7, 37), (24, 9), (33, 5)):
        for Cin in (32, 64):
            g = small if T <= 7 else ("dma",)
            add(f"dma_k3_t{T}_c{Cin}", B, T, Cin, 256 if Cin == 64 else 192, 3, groups=g)
            add(f"dma_k3_t{T}_c{Cin}_mask", B, T, Cin, 256 if Cin == 64 else 192, 3, epi=("bias", "mask"), groups=g)
    for act in ("relu", "gelu"):
        for pair in (False, True):
            add(f"dma_epi_{act}_all" + ("_pair" if pair else ""), 3, 67, 64, 320, 1,
                epi=("bias", act, "mask", "scale", "res_masked", "res2"), pair_out=pair, groups=("dma",))
        add(f"dma_epi_{act}_res", 3, 67, 64, 300, 3, epi=("bias", act, "scale", "res", "res2"), groups=("dma",))
    # ---- the agreement subset: every bias-only f32-output case that all split kernels accept runs on each of ALL6
    out = []
    for c in cases:
        M, K = c.B * c.T, c.Cin * c.k
        if (c.epi == ("bias",) and c.layout == "plain" and not c.pair_out and c.modes == X3 and M % 64 == 0 and c.N % 64 == 0
                and c.N >= 256 and K >= 96 and (c.k == 1 or c.T >= 32)):
            c = c._replace(groups=tuple(dict.fromkeys(c.groups + ALL6)), agree="bits")
        out.append(c)
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}


def cases_of(group):
    return [c for c in CASES if group in c.groups]


# ------------------------------------------------------------------------------------------------------------ pair rows
def encode_pair(t, f16):
    """f32 (..., C) -> the pair-row bytes as an f32-typed tensor of the same shape: per block of 32 channels [32 hi | 32 lo],
    bf16 planes of x or (f16) f16 planes of x * 2^ACT_EXP.  Mirrors vrd::store_pair4."""
    dt = torch.float16 if f16 else torch.bfloat16
    t = t * 2.0 ** ACT_EXP if f16 else t
    hi = t.to(dt)
    lo = (t - hi.float()).to(dt)
    C = t.shape[-1]
    raw = torch.stack([hi.reshape(*t.shape[:-1], C // 32, 32), lo.reshape(*t.shape[:-1], C // 32, 32)], dim=-2)
    return raw.reshape(*t.shape[:-1], 2 * C).contiguous().view(torch.float32)          # 4C bytes per row


def pair_planes(raw, f16):
    """pair-row bytes -> (hi, lo) planes as f32 tensors of the plane values (f16: still scaled by 2^ACT_EXP)"""
    v = raw.contiguous().view(torch.float16 if f16 else torch.bfloat16)
    blocks = v.reshape(*v.shape[:-1], -1, 2, 32).float()
    return blocks[..., 0, :].reshape(*raw.shape), blocks[..., 1, :].reshape(*raw.shape)


def decode_pair(raw, f16):
    """pair-row bytes -> float64 values hi + lo"""
    hi, lo = pair_planes(raw, f16)
    val = hi.double() + lo.double()
    return val * 2.0 ** -ACT_EXP if f16 else val


# --------------------------------------------------------------------------------------------------------------- inputs
class Problem:
    """one GEMM of a case: x, w, bias on the CPU; hA the pair-row window, hC / hP the f32 / pair output windows"""


class Inputs:
    """a case's operands: `problems` (one, or three for batch3) and the shared row inputs"""


def _lengths(case, gen):
    B, T = case.B, case.T
    if case.layout == "pad_skip":
        # five of the 56 32-row blocks hold a valid frame.  vrd_row_blocks deals the valid blocks over the segments in proportion
        # (here seven segments of one 256-row tile each: segment_counts below), so tiles 0 and 3 get none and skip their
        # contraction: of two workgroups one walks skip, 3 x contract, skip, 2 x contract, the other contract, skip, 3 x contract,
        # skip, contract
        assert (B, T) == (7, 256)
        return torch.tensor([100, 0, 0, 0, 0, 0, 17])
    lens = torch.randint(0, T + 1, (B,), generator=gen)
    lens[0] = T
    if B >= 3:
        lens[1] = 1
    if B >= 4:
        lens[-1] = 0
    if case.layout == "pad_map":           # a run of empty sequences: whole 32-row blocks without a valid row
        lens[B // 2:B // 2 + 3] = 0
    return lens


def _embed3(t, out=False, **kw):
    """W.embed / W.embed_out of a (B, T, C) tensor whose view keeps the row pitch as its frame stride at T = 1 too (a size-1
    dimension's stride is otherwise arbitrary, and ops reads the leading dimension from it)"""
    B, T, C = t.shape
    h = W.embed_out((B * T, C), t.device, **kw) if out else W.embed(t.reshape(B * T, C), **kw)
    h.view = h.view.as_strided((B, T, C), (T * h.ld, h.ld, 1))
    return h


def make_inputs(case, mode, device="cpu"):
    """Deterministic operands of `case` (seeded by its name), A as pair rows of `mode`'s format and every activation in a
    poisoned window of its own leading dimension."""
    f16 = mode != "bf16x3"
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    B, T, Cin, N, k = case.B, case.T, case.Cin, case.N, case.k
    inp = Inputs()
    inp.case, inp.mode, inp.f16, inp.device = case, mode, f16, device
    inp.problems = []
    lds = W.LdSeq()
    N32 = (N + 31) // 32 * 32          # leading dimensions are multiples of 32 floats whatever N is (N = 197: float4 rows through ld alone)
    lda, ldc, ldp = lds(Cin), lds(N32), lds(N32)          # the same for the problems of a batch (vrd_gemm_batch asks for that)
    for i in range(3 if case.layout == "batch3" else 1):
        p = Problem()
        p.x = torch.randn(B, T, Cin, generator=gen)          # padded frames hold data too
        p.w = torch.randn(N, Cin, k, generator=gen) / (Cin * k) ** 0.5
        p.bias = torch.randn(N, generator=gen) if "bias" in case.epi else None
        p.hA = _embed3(encode_pair(p.x, f16).to(device), ld=lda, name=f"A{i}")
        shape = torch.empty(B, T, N, device=device)
        p.hC = _embed3(shape, out=True, ld=ldc, name=f"C{i}")
        p.hP = _embed3(shape, out=True, ld=ldp, name=f"C{i} (pair)") if case.pair_out else None
        inp.problems.append(p)
    inp.lens = _lengths(case, gen)
    inp.mask = (torch.arange(T)[None, :] < inp.lens[:, None]).contiguous() if ("mask" in case.epi or case.layout == "pad_skip") else None
    inp.scale = torch.rand(N, generator=gen) + 0.5 if "scale" in case.epi else None
    inp.res = inp.res2 = inp.hR = inp.hR2 = None
    if "res" in case.epi or "res_masked" in case.epi:
        inp.res = torch.randn(B, T, N, generator=gen)
        inp.hR = _embed3(inp.res.to(device), ld=lds(N32), name="res")
    if "res2" in case.epi:
        inp.res2 = torch.randn(B, T, N, generator=gen)
        inp.hR2 = _embed3(inp.res2.to(device), ld=lds(N32), name="res2")
    return inp


# ------------------------------------------------------------------------------------------------------------ reference
def _conv64(x, w, k):
    return F.conv1d(x.transpose(1, 2), w, None, padding=k // 2).transpose(1, 2)


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def reference(inp, p):
    """float64 (ref, mag, lip), each (B, T, N), of the whole epilogue of vrd_gemm from the DECODED pair rows in p.hA:
    v = acc + bias; v = act(v); v *= row_mask; v *= scale; v += res * (res_masked ? row_mask : 1); v += res2."""
    case = inp.case
    xd = decode_pair(p.hA.view.cpu(), inp.f16)
    w = p.w.double()
    v = _conv64(xd, w, case.k)
    mag = _conv64(xd.abs(), w.abs(), case.k)
    if p.bias is not None:
        v = v + p.bias.double()
    if "gelu" in case.epi:
        v = _gelu64(v)
    elif "relu" in case.epi:
        v = v.clamp_min(0.0)
    mk = inp.mask.double()[..., None] if "mask" in case.epi else torch.ones(case.B, case.T, 1, dtype=torch.float64)
    sc = inp.scale.double() if inp.scale is not None else torch.ones(case.N, dtype=torch.float64)
    v = v * mk * sc
    if inp.res is not None:
        v = v + inp.res.double() * (mk if "res_masked" in case.epi else 1.0)
    if inp.res2 is not None:
        v = v + inp.res2.double()
    lip = mk * sc.abs().clamp_max(1.0)
    return v, mag, lip.expand_as(v)


def bound(case, mode, ref, mag, lip):
    K = case.Cin * case.k
    return (U[mode] + (K / 32 + 2) * 2.0 ** -24) * mag * lip + 2.0 ** -23 * ref.abs()


# -------------------------------------------------------------------------------------------------------------- checker
def _where(case, r, c):
    b, t = divmod(r, case.T)
    return (f"row {r} column {c} (256x256 tile ({r // 256}, {c // 256}), 128x256 tile ({r // 128}, {c // 256}), "
            f"frame {t} of {case.T} in sequence {b})")


def check_values(case, mode, got, ref, mag, lip, rows=None, what="f32 output"):
    """Every element of `got` (B, T, N) within the bound of `ref` (on the rows `rows` (B, T) bool selects, default all).
    Returns the largest error-to-bound ratio; raises AssertionError naming the case and the first wrong elements."""
    N = case.N
    got, ref = got.reshape(-1, N).double(), ref.reshape(-1, N)
    bnd = bound(case, mode, ref, mag.reshape(-1, N), lip.reshape(-1, N))
    err = (got - ref).abs()
    bad = ~(err <= bnd)                        # (a NaN in got is bad)
    if rows is not None:
        bad &= rows.reshape(-1, 1)
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        lines = [f"{_where(case, r, c)}: got {float(got[r, c])!r}, want {float(ref[r, c])!r}, |diff| {float(err[r, c]):.3e} > bound {float(bnd[r, c]):.3e}"
                 for r, c in idx[:6].tolist()]
        rws, cls = idx[:, 0], idx[:, 1]
        raise AssertionError(f"case {case.name} [{mode}] {what}: {len(idx)} of {got.numel()} elements outside the bound, in rows "
                             f"{int(rws.min())}..{int(rws.max())}, columns {int(cls.min())}..{int(cls.max())}\n  " + "\n  ".join(lines))
    ok = bnd > 0
    if rows is not None:
        ok &= rows.reshape(-1, 1)
    return float((err[ok] / bnd[ok]).max()) if bool(ok.any()) else 0.0


def check_pair(case, mode, got_pair, got):
    """the decoded pair output within 2^-15 relative of the f32 output of the same call"""
    rel = (got_pair.double() - got.double()).abs() / got.double().abs().clamp_min(1e-3)
    bad = ~(rel < 2.0 ** -15)
    if bool(bad.any()):
        idx = torch.nonzero(bad.reshape(-1, case.N))
        r, c = idx[0].tolist()
        raise AssertionError(f"case {case.name} [{mode}] pair output: {len(idx)} elements further than 2^-15 from the f32 output, first at "
                             f"{_where(case, r, c)}: pair {float(got_pair.reshape(-1, case.N)[r, c])!r}, f32 {float(got.reshape(-1, case.N)[r, c])!r}")


def segment_counts(mask):
    """valid 32-row blocks per segment of the padding map of a (B, T) mask, as vrd_row_blocks deals them (ops.row_blocks,
    tests/test_gpu_ops.py::test_row_blocks_padding_map): segment s of seg_len blocks gets n * end(s) // nblk - n * start(s) // nblk"""
    flags = mask.reshape(-1, 32).any(1)
    nblk, n = len(flags), int(flags.sum())
    seg_len = 8 * (((nblk + 7) // 8 + 7) // 8)
    start = [min(s * seg_len, nblk) for s in range((nblk + seg_len - 1) // seg_len + 1)]
    return [n * start[s + 1] // nblk - n * start[s] // nblk for s in range(len(start) - 1)], seg_len


def valid_block_rows(inp):
    """(B, T) bool: rows of 32-row blocks that hold a valid frame (the rows a padding map without row_mask still computes)"""
    m = inp.mask.reshape(-1, 32).any(1).repeat_interleave(32)
    return m.reshape(inp.case.B, inp.case.T)


def verify(inp, rows=None):
    """The checks of one case on its windows after the op (or its emulation) ran: guards intact, inputs unchanged, every output
    element written, and within the bound of the float64 reference -- on the rows `rows` (B, T) selects; default: all, or for
    pad_skip the rows of blocks that hold a valid frame.  Returns the largest error-to-bound ratio."""
    case, mode = inp.case, inp.mode
    outs = [h for p in inp.problems for h in (p.hC, p.hP) if h is not None]
    ins = [p.hA for p in inp.problems] + [h for h in (inp.hR, inp.hR2) if h is not None]
    try:
        W.check(outs, ins)
    except AssertionError as e:
        raise AssertionError(f"case {case.name} [{mode}]: {e}") from None
    worst = 0.0
    for i, p in enumerate(inp.problems):
        got = p.hC.result().cpu()
        if mode == "f16x1":
            want = E.conv1d(p.x, p.w, p.bias)
            err, gap = float((got.double() - want).abs().max()), float((got - p.got3).abs().max())
            assert err * 100 < gap, f"case {case.name} [f16x1] problem {i}: |got - emulation| {err:.3e} is not 100 x below |f16x1 - f16x3| {gap:.3e}"
            worst = max(worst, err * 100 / gap)
            continue
        ref, mag, lip = reference(inp, p)
        sel = rows if rows is not None else (valid_block_rows(inp) if case.layout == "pad_skip" else None)
        worst = max(worst, check_values(case, mode, got, ref, mag, lip, sel, what=f"f32 output of problem {i}"))
        if p.hP is not None:
            check_pair(case, mode, decode_pair(p.hP.result().cpu(), inp.f16), got)
    return worst


# ------------------------------------------------------------------------------------------------------------ emulation
def _im2col(t, k):
    """(B, T, C) -> (B * T, k * C), tap-major, zero rows beyond the sequence ends"""
    if k == 1:
        return t.reshape(-1, t.shape[-1])
    z = torch.zeros_like(t[:, :1])
    return torch.cat([torch.cat([z, t[:, :-1]], 1), t, torch.cat([t[:, 1:], z], 1)], -1).reshape(-1, 3 * t.shape[-1])


def _weight_planes(w, f16):
    """(hi, lo, alpha): planes of the tap-major (N, K) operand as f32 values, and the accumulator factor"""
    N, Cin, k = w.shape
    wp = w.permute(0, 2, 1).reshape(N, k * Cin)
    if f16:
        e = E.weight_exp(w)
        s = wp * 2.0 ** e
        hi = s.to(torch.float16)
        lo = (s - hi.float()).to(torch.float16)
        return hi.float(), lo.float(), 2.0 ** -(e + ACT_EXP)
    hi = wp.to(torch.bfloat16)
    lo = (wp - hi.float()).to(torch.bfloat16)
    return hi.float(), lo.float(), 1.0


FAULTS = ("dropped_product", "stale_first_step", "blocks_exchanged", "tile_unwritten", "tap_reads_neighbour_first",
          "tap_reads_neighbour_last", "column_tail_overrun")


def emulate(inp, fault=None, products=3):
    """The three-product arithmetic in f32 on the CPU, K step by K step in the kernels' order (lo x hi, hi x lo, hi x hi), with the
    epilogue in f32, written into the output windows the way a kernel writes them.  `fault`: one of FAULTS, the Python stand-in
    of a kernel fault (256 x 256 tiles)."""
    case, f16 = inp.case, inp.f16
    B, T, N, k = case.B, case.T, case.N, case.k
    M, K = B * T, case.Cin * k
    tm_f, tn_f = (M - 1) // 256, (N - 1) // 256                    # the tile the tile faults hit: the last one
    for p in inp.problems:
        ah, al = pair_planes(p.hA.view.cpu(), f16)
        if fault in ("tap_reads_neighbour_first", "tap_reads_neighbour_last"):
            assert k == 3 and B >= 2
            cols = []
            for pl in (ah, al):
                flat = pl.reshape(M, -1)
                prev = torch.cat([torch.zeros_like(flat[:1]), flat[:-1]])          # the row before / behind in the row space: the
                nxt = torch.cat([flat[1:], torch.zeros_like(flat[:1])])            # neighbouring sequence's at a sequence end
                good = _im2col(pl, 3)
                bad = torch.cat([prev, flat, nxt], -1)
                cols.append(torch.cat([bad[:, :case.Cin], good[:, case.Cin:]], -1) if fault.endswith("first")
                            else torch.cat([good[:, :2 * case.Cin], bad[:, 2 * case.Cin:]], -1))
            ah, al = cols
        else:
            ah, al = _im2col(ah, k), _im2col(al, k)
        wh, wl, alpha = _weight_planes(p.w, f16)
        acc = torch.zeros(M, N)
        for s in range(K // 32):
            sl = slice(32 * s, 32 * s + 32)
            a_h, a_l = ah[:, sl], al[:, sl]
            if fault == "stale_first_step" and s == 0:          # the tile's first K step from the previous row tile's ring slot
                a_h, a_l = a_h.clone(), a_l.clone()
                r0 = tm_f * 256
                a_h[r0:r0 + 256], a_l[r0:r0 + 256] = ah[r0 - 256:r0, sl][:M - r0], al[r0 - 256:r0, sl][:M - r0]
            if products == 3:
                lo_hi = a_l @ wh[:, sl].T
                if fault == "dropped_product" and s == min(1, K // 32 - 1):
                    lo_hi[tm_f * 256:, tn_f * 256:] = 0.0
                acc = acc + lo_hi
                acc = acc + a_h @ wl[:, sl].T
            acc = acc + a_h @ wh[:, sl].T
        v = acc * alpha
        if p.bias is not None:
            v = v + p.bias
        if "gelu" in case.epi:
            v = F.gelu(v)
        elif "relu" in case.epi:
            v = v.clamp_min(0.0)
        v = v.reshape(B, T, N)
        mk = inp.mask.float()[..., None] if "mask" in case.epi else None
        if mk is not None or inp.scale is not None:
            v = v * ((mk if mk is not None else 1.0) * (inp.scale if inp.scale is not None else 1.0))
        if inp.res is not None:
            v = v + inp.res * (mk if "res_masked" in case.epi else 1.0)
        if inp.res2 is not None:
            v = v + inp.res2
        v = v.reshape(M, N).clone()
        if fault == "blocks_exchanged":
            r0 = tm_f * 256
            v[r0:r0 + 32], v[r0 + 32:r0 + 64] = v[r0 + 32:r0 + 64].clone(), v[r0:r0 + 32].clone()
        for h, val in ((p.hC, v), (p.hP, encode_pair(v, f16) if p.hP is not None else None)):
            if h is None:
                continue
            dst = h.buf[h.row0:h.row0 + M, h.c0:h.c0 + N]
            if fault == "tile_unwritten":
                keep = torch.ones(M, N, dtype=torch.bool)
                keep[tm_f * 256:, tn_f * 256:] = False
                dst.view(torch.int32)[keep] = val.view(torch.int32)[keep]
            else:
                dst.view(torch.int32).copy_(val.view(torch.int32))
            if fault == "column_tail_overrun" and h is p.hC:
                # the tail tile computed on the clamped last weight row and stored one column too far
                assert N % 256
                for r in range(tm_f * 256, M):
                    h.flat[h.offset + r * h.ld + N] = val[r, N - 1]
    return inp
