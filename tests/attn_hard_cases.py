"""Hard inputs for the training attention kernels (global: vrd_attention_rows / vrd_attention_bwd, vrd_attn_bwd_softmax + vrd_bmm,
vrd_attn_bwd_probs; banded: vrd_local_attn_bwd and its _segs / _drop forms): sharp rows, dominant masked keys, exact ties, exactly
uniform rows, gradients that differ by 2^12 between sequences -- the conditions a trained model produces and `randn` never does.

Every case is built from a seed, computes its own float64 reference (autograd of oracle.vrd_oracle.full_attention /
banded_attention) and its own error bounds.  The bounds are a first-order propagation, in float64, of the errors the kernels'
headers state, through score -> P -> dS -> dq / dk / dv (`propagate`); nothing in them comes from what a kernel gave.  An output is
judged per (sequence, head) block: the largest absolute error of the block over the largest bound of the block.
tests/test_attn_hard_cases_cpu.py proves cases and bounds on an f32 emulation; tests/test_gpu_attn_hard.py runs the kernels."""
import math
import zlib
from collections import namedtuple

import torch

from oracle import vrd_oracle as O

B, H = 3, 2
TARGET = 24.0                    # the score of a dominant valid key
MASKED_EXTRA = 120.0             # a dominant masked key scores TARGET + this: beyond head_cases.SURE_UNDERFLOW (-110) of the valid ones
F16_LIMIT = 4094.0               # vrd_common.h: |x| 2^VRD_F16_ACT_EXP must stay below 65504
ACT_EXP = 4                      # VRD_F16_ACT_EXP
ARITH = ("f32", "bf16", "f16")   # the arithmetic of a route: exact f32, bf16 hi / lo planes, scaled f16 hi / lo planes

Case = namedtuple("Case", "name hd Tq Tk kind lens holes spread pow2 vmul")


SPREAD = (0, -6, -12)            # dO of sequence b times 2^SPREAD[b]; reversed: the full-length sequence holds the smallest gradient


def _case(name, hd, Tq, Tk, kind, holes=False, spread=None, pow2=0, vmul=1.0):
    return Case(name, hd, Tq, Tk, kind, [Tk, Tk // 2 + 3, 1], holes, spread, pow2, vmul)


FLASH_SHAPES = [(64, 130, 77), (32, 130, 77), (64, 40, 200), (32, 40, 200)]
SMALL = (64, 9, 12)              # below 32 queries / keys: vrd_attn_bwd_probs in every mode
KINDS = ("late_dominant", "masked_dominant", "tie", "flat_exact", "flat")

CASES = []
for _hd, _tq, _tk in FLASH_SHAPES + [SMALL]:
    _s = f"hd{_hd}_{_tq}x{_tk}"
    CASES += [_case(f"late_dominant_{_s}", _hd, _tq, _tk, "late_dominant"),
              _case(f"masked_dominant_{_s}", _hd, _tq, _tk, "masked_dominant"),
              # (v times 2^6: dS reaches the range the factor s_s exists for)
              _case(f"tie_{_s}", _hd, _tq, _tk, "tie", vmul=64.0),
              _case(f"flat_exact_{_s}", _hd, _tq, _tk, "flat_exact"),
              _case(f"grad_spread_{_s}", _hd, _tq, _tk, "flat", spread=SPREAD),
              _case(f"grad_spread_sharp_{_s}", _hd, _tq, _tk, "late_dominant", spread=SPREAD)]
for _hd, _tq, _tk in [(64, 130, 77), (32, 40, 200)]:
    # (the one-key sequence has dq = dk = 0: here the smallest gradient meets the longest sequence)
    _s = f"hd{_hd}_{_tq}x{_tk}"
    CASES += [_case(f"grad_spread_rev_{_s}", _hd, _tq, _tk, "flat", spread=SPREAD[::-1]),
              _case(f"grad_spread_rev_sharp_{_s}", _hd, _tq, _tk, "late_dominant", spread=SPREAD[::-1])]
CASES += [_case("late_dominant_hd128_96x96", 128, 96, 96, "late_dominant"),           # the five-product form in the split modes
          _case("masked_dominant_hd128_96x96", 128, 96, 96, "masked_dominant"),
          _case("holes_hd64_130x77", 64, 130, 77, "masked_dominant", holes=True),
          _case("holes_hd32_130x77", 32, 130, 77, "late_dominant", holes=True)]
POW2_BASES = ["grad_spread_hd64_130x77", "grad_spread_hd32_130x77", "grad_spread_hd64_9x12", "late_dominant_hd128_96x96"]
POW2 = (-30, 12)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def with_pow2(case, k):
    """the same case with the whole dO times 2^k (homogeneity: dq, dk, dv must come out times 2^k bit for bit)"""
    return case._replace(name=f"{case.name}_pow2_{k}", pow2=k)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.split("_pow2_")[0].encode()))


def key_mask(case):
    m = torch.arange(case.Tk)[None] < torch.tensor(case.lens)[:, None]
    if case.holes:
        assert case.Tk == 77
        m[1, :32] = False                    # the whole first key tile of sequence 1 (its valid keys: 32 .. 40)
        m[0, 40:45] = False                  # a hole in the middle tile of sequence 0
        m[0, 60] = False
    return m


def _dominant(qrow, score, hd):
    """the key whose scaled score against `qrow` is `score`"""
    return qrow * (score * math.sqrt(hd) / float(qrow.double().pow(2).sum()))


def rows_of(case):
    """(a query of wave 0, the last query, a third one): the rows that get dominant keys"""
    return 5, case.Tq - 1, case.Tq // 2


Inputs = namedtuple("Inputs", "case q k v dO km marks")


def make_inputs(case):
    """q, k, v, dO as f32 (B, T, H * hd) rows, the (B, Tk) key mask, and marks: what the case claims, for the CPU file to verify --
    ("dominant", b, h, query, key), ("tie", b, h, query, key, key), ("masked", b, h, query, key), ("uniform", b)"""
    g = _gen(case.name)
    hd, Tq, Tk = case.hd, case.Tq, case.Tk
    Cw = H * hd
    q, dO = torch.randn(B, Tq, Cw, generator=g), torch.randn(B, Tq, Cw, generator=g)
    k, v = torch.randn(B, Tk, Cw, generator=g), torch.randn(B, Tk, Cw, generator=g)
    v = v * case.vmul
    km = key_mask(case)
    marks = []
    r0, r1, r2 = rows_of(case)
    h0, h1 = slice(0, hd), slice(hd, 2 * hd)
    for b in range(B):
        valid = torch.nonzero(km[b])[:, 0].tolist()
        first, last = valid[0], valid[-1]
        if case.kind in ("late_dominant", "masked_dominant"):
            # head 0: the last valid key dominates row r0 and the last row (they share a query vector), the first valid key row r2
            q[b, r1, h0] = q[b, r0, h0]
            k[b, last, h0] = _dominant(q[b, r0, h0], TARGET, hd)
            marks += [("dominant", b, 0, r0, last), ("dominant", b, 0, r1, last)]
            if first != last:
                k[b, first, h0] = _dominant(q[b, r2, h0], TARGET, hd)
                marks.append(("dominant", b, 0, r2, first))
        if case.kind == "masked_dominant":
            # head 1: the first valid key dominates rows r0 and r1; the first masked key behind a valid one beats it by MASKED_EXTRA
            q[b, r1, h1] = q[b, r0, h1]
            k[b, first, h1] = _dominant(q[b, r0, h1], TARGET, hd)
            marks += [("dominant", b, 1, r0, first), ("dominant", b, 1, r1, first)]
            masked = [j for j in range(Tk) if not km[b, j] and j > first]
            if masked:
                k[b, masked[0], h1] = _dominant(q[b, r0, h1], TARGET + MASKED_EXTRA, hd)
                marks += [("masked", b, 1, r0, masked[0]), ("masked", b, 1, r1, masked[0])]
            if case.holes and not km[b, 0]:               # and one in the masked first tile
                k[b, 3, h1] = _dominant(q[b, r0, h1], TARGET + MASKED_EXTRA, hd)
                marks.append(("masked", b, 1, r0, 3))
        if case.kind == "tie" and len(valid) >= 2:
            j0, j1 = valid[1], last                       # different key tiles wherever the sequence has more than 32 keys
            q[b, r1, h0] = q[b, r0, h0]
            k[b, j0, h0] = k[b, j1, h0] = _dominant(q[b, r0, h0], TARGET, hd)
            marks += [("tie", b, 0, r0, j0, j1), ("tie", b, 0, r1, j0, j1)]
        if case.kind == "flat_exact":
            k[b] = k[b, first]                            # every key the same vector, masked ones included
            marks.append(("uniform", b))
    if case.spread:
        dO = dO * torch.tensor([2.0 ** e for e in case.spread])[:, None, None]
    dO = dO * 2.0 ** case.pow2
    for t in (q, k, v):
        assert float(t.abs().max()) < F16_LIMIT / 8, (case.name, "an operand near the f16 operand limit")
    assert float(k.abs().max()) < 128.0, case.name           # (a dominant masked key: |k| = 144 sqrt(hd) / |q|, entries of some tens)
    assert all(bool(torch.isfinite(t).all()) for t in (q, k, v, dO))
    return Inputs(case, q, k, v, dO, km, marks)


def heads(t, n_head=H):
    """(B, T, H * hd) -> (B, H, T, hd)"""
    return t.reshape(t.shape[0], t.shape[1], n_head, -1).transpose(1, 2)


def rows(t):
    """(B, H, T, hd) -> (B, T, H * hd)"""
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)


def _bct(t):
    return t.transpose(1, 2).contiguous()


_refs = {}


def reference(inp):
    """float64 autograd of the oracle: dict of out, dq, dk, dv as (B, T, H * hd) rows; computed once per case and left unchanged"""
    name = inp.case.name
    if name not in _refs:
        with torch.enable_grad():
            qr, kr, vr = (t.double().requires_grad_(True) for t in (inp.q, inp.k, inp.v))
            out = O.full_attention(_bct(qr), _bct(kr), _bct(vr), inp.km[:, None], H)
            out.backward(_bct(inp.dO.double()))
        _refs[name] = dict(out=_bct(out.detach()), dq=qr.grad, dk=kr.grad, dv=vr.grad)
        # the backward is linear in dO and nothing in it comes near an f32 denormal: the homogeneity check's premise
        tiny = min(float(t[t != 0].abs().min()) for t in (_refs[name]["dq"], _refs[name]["dk"], _refs[name]["dv"], inp.dO.double()))
        assert tiny > 2.0 ** -100 or inp.case.pow2 == 0, (name, tiny)
    return _refs[name]


def pow2_scale(x):
    """vrd_absmax_scale: the power of two 2^e with max |x| 2^e in [2^13, 2^14)"""
    return 2.0 ** (13 - math.floor(math.log2(float(x.abs().max()))))


# ------------------------------------------------------------------------------------------------------------------ bounds
U = 2.0 ** -23                   # one f32 operation (rounding to nearest is 2^-24; the matrix cores' accumulation is granted 2^-23)
PROD = {"f32": 0.0,
        # vrd_common.h:213: |x - hi - lo| <= 2^-17 |x| per operand, and the lo x lo product that is left out (<= 2^-18 |x y|):
        # three terms of at most 2^-17 each
        "bf16": 3 * 2.0 ** -17,
        # :214-217: 2^-22 |y| per operand while lo is normal, and lo x lo <= 2^-22 |x y|; below that the planes are absolute, 2^-25
        "f16": 3 * 2.0 ** -22}
PLANE_ABS = 2.0 ** -25


def _masked_sum(x, m, dim):
    return (x * m).sum(dim)


def propagate(q, k, v, dO, S, P, arith, slack=1.0, s_o=None, s_v=None, dS_extra=None):
    """First-order bounds on |out|, |dq|, |dk|, |dv| errors (and on the unscaled dS), all float64, shapes (B, H, T, hd):
    q, k, v, dO per head; S the scaled scores with the biases in (-inf where P is exactly 0), P the reference probabilities.
    arith: see ARITH.  slack multiplies the f32 rounding terms (the split and plane terms always count in full).
    s_o, s_v: the f16 planes' run-time factors of dO and of dS = s_o s_v 2^-17 (vrd_attn_bwd.hip:319-323)."""
    e, u = PROD[arith], U * slack
    f16 = arith == "f16"
    fa = PLANE_ABS / 2.0 ** ACT_EXP if f16 else 0.0                       # planes at the activations' 2^4: q, k, v, P
    fo = PLANE_ABS / s_o if f16 else 0.0                                  # dO planes
    fs = PLANE_ABS / (s_o * s_v * 2.0 ** -17) if f16 else 0.0             # dS planes
    hd, Tq, Tk = q.shape[-1], q.shape[-2], k.shape[-2]
    scale = hd ** -0.5
    live = (P > 0).double()                                               # (B, H, Tq, Tk): pairs that contribute at all
    aq, ak, av, ag = q.abs(), k.abs(), v.abs(), dO.abs()
    T = lambda x: x.transpose(-2, -1)                                     # noqa: E731
    Sf = torch.where(live > 0, S, torch.zeros_like(S))
    lse = torch.logsumexp(S, -1, keepdim=True)
    lse = torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))
    # scores: split products over hd terms, f32 accumulation, the scaling and the bias add
    ES = (scale * ((e + hd * u) * (aq @ T(ak)) + fa * (aq.sum(-1, keepdim=True) + T(ak.sum(-1, keepdim=True)))) + 2 * u * Sf.abs()) * live
    # log-sum-exp: a P-weighted mean of the score errors, the sum's accumulation, __logf and the add of the running maximum
    Else = (P * ES).sum(-1, keepdim=True) + (Tk + lse.abs() + 4) * u
    # P = __expf(S - lse): exp2 of a product with log2(e) rounded in f32 carries |x| 2^-24 relative, the instruction one ulp; the
    # flash forward's exp(S - m) / l has |x| larger by log l <= log Tk < 8
    x = (Sf - lse).abs() * live
    EP = P * (ES + Else + (x + 12) * u)
    out = P @ v
    Eout = EP @ av + (e + Tk * u) * (P @ av) + fa * (live @ av + 1.0) + u * out.abs()
    dP = dO @ T(v)
    EdP = (e + hd * u) * (ag @ T(av)) + fo * T(av.sum(-1, keepdim=True)) + fa * ag.sum(-1, keepdim=True)
    delta = (P * dP).sum(-1, keepdim=True)
    # delta: sum_d dO O of the computed output (flash) or sum_j P dP (the five-product form): either is granted
    Ed_flash = (ag * Eout).sum(-1, keepdim=True) + hd * u * (ag * out.abs()).sum(-1, keepdim=True)
    Ed_rows = (EP * dP.abs() + P * EdP).sum(-1, keepdim=True) + Tk * u * (P * dP.abs()).sum(-1, keepdim=True)
    Edelta = torch.maximum(Ed_flash, Ed_rows)
    dSu = P * (dP - delta)                                                # w.r.t. the scaled scores
    EdS = EP * (dP - delta).abs() + P * (EdP + Edelta) + 4 * u * dSu.abs()
    if dS_extra is not None:
        EdS = EdS + dS_extra
    adS = dSu.abs()
    # dq = scale dS K, dk = scale dS^T Q (flash: dS scale goes into the planes at s_s), dv = P^T dO
    Edq = scale * (EdS @ ak + (e + Tk * u) * (adS @ ak)) + fs * (live @ ak) + scale * fa * adS.sum(-1, keepdim=True)
    Edk = scale * (T(EdS) @ aq + (e + Tq * u) * (T(adS) @ aq)) + fs * (T(live) @ aq) + scale * fa * T(adS).sum(-1, keepdim=True)
    Edv = T(EP) @ ag + (e + Tq * u) * (T(P) @ ag) + fa * (T(live) @ ag) + fo * T(P).sum(-1, keepdim=True)
    key_live = (live.sum(-2) > 0).double()[..., None]                     # a key no query sees: exactly zero dk / dv
    return dict(out=Eout, dq=Edq, dk=Edk * key_live, dv=Edv * key_live, dS=EdS)


_bounds = {}


def bounds(inp, arith, slack=1.0):
    """per-block bounds (B, H) of out, dq, dk, dv for a global case, and the element bounds they are the block maxima of"""
    key = (inp.case.name, arith, slack)
    if key not in _bounds:
        q, k, v, dO = (heads(t.double()) for t in (inp.q, inp.k, inp.v, inp.dO))
        S = (q * inp.case.hd ** -0.5) @ k.transpose(-2, -1)
        S = S.masked_fill(~inp.km[:, None, None, :], float("-inf"))
        P = torch.softmax(S, -1)
        el = propagate(q, k, v, dO, S, P, arith, slack, s_o=pow2_scale(inp.dO), s_v=pow2_scale(inp.v))
        _bounds[key] = {n: el[n].amax((-2, -1)) for n in ("out", "dq", "dk", "dv")}
    return _bounds[key]


NAMES = ("out", "dq", "dk", "dv")


def ratios(got, inp, arith, slack=1.0, names=NAMES):
    """{output: (B, H) error / bound per block}; a non-finite output counts as infinitely wrong"""
    ref, bnd = reference(inp), bounds(inp, arith, slack)
    res = {}
    for n in names:
        g = got[n].detach().double().cpu()
        err = heads((g - ref[n]).abs()).amax((-2, -1))
        err = torch.where(torch.isfinite(heads(g)).all(-1).all(-1), err, torch.full_like(err, float("inf")))
        res[n] = err / bnd[n]
    return res


def block_rel(got, inp, names=("dq", "dk", "dv")):
    """{output: (B,) the largest block error of a sequence over the largest reference entry of that block; nan where that is zero}"""
    ref, res = reference(inp), {}
    for n in names:
        err = heads((got[n].detach().double().cpu() - ref[n]).abs()).amax((-2, -1))
        top = heads(ref[n].abs()).amax((-2, -1))
        res[n] = torch.where(top > 0, err / top.clamp_min(1e-300), torch.full_like(err, float("nan")))
        res[n] = torch.where(torch.isnan(res[n]).all(1), res[n][:, 0], torch.nan_to_num(res[n], nan=0.0).amax(1))
    return res


def masked_keys_are_zero(got, inp):
    """dk / dv at masked keys: exactly zero"""
    dead = ~inp.km
    return all(not bool(got[n].detach().cpu()[dead].ne(0).any()) and not bool(torch.isnan(got[n].detach().cpu()[dead]).any()) for n in ("dk", "dv"))


def worst(res):
    return {n: float(r.max()) for n, r in res.items()}


# ------------------------------------------------------------------------------------------------------------------ banded
WINDOWS = (3, 9, 19)
BAND_C, BAND_T, BAND_LENS = 256, 40, [40, 13, 2]         # width 256 at two heads: head_dim 128
BAND_SEGS = [(0, 2, 24), (48, 1, 40)]                    # the row groups used elsewhere: two sequences of 24 frames, one of 40 at row 48
BandCase = namedtuple("BandCase", "name W T lens")
BAND_CASES = [BandCase(f"band_w{W}", W, BAND_T, BAND_LENS) for W in WINDOWS]
BAND_GROUPS = {W: [BandCase(f"band_w{W}_g0", W, 24, [24, 7]), BandCase(f"band_w{W}_g1", W, 40, [33])] for W in WINDOWS}
BandInputs = namedtuple("BandInputs", "case q k v dO mask rel_pe marks")


def rel_pe_of(W):
    """one bias per (head, window slot) for all cases of a window (a row space shares it between its groups): entries reach +-20"""
    g = torch.Generator().manual_seed(7000 + W)
    rel = torch.randn(1, 1, H, W, generator=g) * 4.0
    rel[0, 0, 0, 0], rel[0, 0, 1, W - 1] = 20.0, -20.0
    return rel


def make_band_inputs(case):
    g = _gen(case.name)
    W, T, nb = case.W, case.T, len(case.lens)
    w, hd = W // 2, BAND_C // H
    q, k, v, dO = (torch.randn(nb, T, BAND_C, generator=g) for _ in range(4))
    mask = torch.arange(T)[None] < torch.tensor(case.lens)[:, None]
    marks = []
    h0, h1 = slice(0, hd), slice(hd, 2 * hd)
    for b, n in enumerate(case.lens):
        if n > 2 * w + 2:
            t = n // 2
            # both window edges of query t dominate and tie (the bias of their slots is not in this score: P is checked with it)
            k[b, t - w, h0] = k[b, t + w, h0] = _dominant(q[b, t, h0], TARGET, hd)
            marks.append(("edges", b, 0, t, t - w, t + w))
        if n < T:
            # a dominant masked key inside the window of the last valid query
            k[b, n, h1] = _dominant(q[b, n - 1, h1], TARGET + MASKED_EXTRA, hd)
            marks.append(("masked", b, 1, n - 1, n))
    assert float(k.abs().max()) < 160.0
    return BandInputs(case, q, k, v, dO, mask, rel_pe_of(W), marks)


BAND_NAMES = ("out", "dq", "dk", "dv", "drel")


def band_scores(inp):
    """(S, P) float64 (B, H, T, T): the banded attention as a dense one -- rel_pe and the -1e4 of masked keys in S, -inf outside the
    window; rows of masked queries have P = 0"""
    W, T = inp.case.W, inp.case.T
    w = W // 2
    q, k = heads(inp.q.double()), heads(inp.k.double())
    S = (q * q.shape[-1] ** -0.5) @ k.transpose(-2, -1)
    off = torch.arange(T)[None, :] - torch.arange(T)[:, None]                        # key - query
    band = off.abs() <= w
    S = S + inp.rel_pe.double().reshape(1, H, W)[:, :, (off + w).clamp(0, W - 1)]
    S = S + torch.where(inp.mask, 0.0, O.MASKED_KEY_BIAS)[:, None, None, :]
    S = S.masked_fill(~band[None, None], float("-inf"))
    P = torch.softmax(S, -1) * inp.mask[:, None, :, None]
    return S.masked_fill(P == 0, float("-inf")), P, off


def band_reference(inp):
    name = inp.case.name
    if name not in _refs:
        with torch.enable_grad():
            qr, kr, vr = (t.double().requires_grad_(True) for t in (inp.q, inp.k, inp.v))
            rel = inp.rel_pe.double().requires_grad_(True)
            out = O.banded_attention(_bct(qr), _bct(kr), _bct(vr), inp.mask[:, None], H, inp.case.W // 2, rel_pe=rel)
            out.backward(_bct(inp.dO.double()))
        _refs[name] = dict(out=_bct(out.detach()), dq=qr.grad, dk=kr.grad, dv=vr.grad, drel=rel.grad)
    return _refs[name]


def band_bounds(inp, slack=1.0):
    """per-block bounds of out, dq, dk, dv (B, H) and the element bound of d rel_pe (1, 1, H, W): exact f32 arithmetic"""
    key = (inp.case.name, "band", slack)
    if key not in _bounds:
        S, P, off = band_scores(inp)
        q, k, v, dO = (heads(t.double()) for t in (inp.q, inp.k, inp.v, inp.dO))
        # (the bias and the mask constant are two more f32 adds on a score; masked keys have P = 0 and no error)
        el = propagate(q, k, v, dO, S, P, "f32", slack)
        W, w = inp.case.W, inp.case.W // 2
        dP = dO @ v.transpose(-2, -1)
        dSu = P * (dP - (P * dP).sum(-1, keepdim=True))
        n_rows = P.shape[0] * P.shape[2]
        drel = torch.zeros(1, 1, H, W, dtype=torch.float64)
        for s in range(W):
            sel = (off == s - w)[None, None].double()
            drel[0, 0, :, s] = (el["dS"] * sel).sum((0, 2, 3)) + n_rows * U * slack * (dSu.abs() * sel).sum((0, 2, 3))
        res = {n: el[n].amax((-2, -1)) for n in NAMES}
        res["drel"] = drel
        _bounds[key] = res
    return _bounds[key]


def band_ratios(got, inp, slack=1.0):
    ref, bnd = band_reference(inp), band_bounds(inp, slack)
    res = {}
    for n in BAND_NAMES:
        g = got[n].detach().double().cpu()
        if n == "drel":
            err = (g - ref[n]).abs()
            err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
            res[n] = (err / bnd[n]).reshape(H, -1)
        else:
            err = heads((g - ref[n]).abs()).amax((-2, -1))
            err = torch.where(torch.isfinite(heads(g)).all(-1).all(-1), err, torch.full_like(err, float("inf")))
            res[n] = err / bnd[n].clamp_min(1e-300)
            res[n] = torch.where((bnd[n] == 0) & (err == 0), torch.zeros_like(err), res[n])
    return res
