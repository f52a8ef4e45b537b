"""`predictor.num_queries` above 16 (to the cap of 64) on the MI355X: the mask head in groups of 16 queries, the wave-per-pair
assignment (vrd_assign_wave), the criterion kernels, the predictor's attention shapes, and the model in eval and training against
goldens of the real reference at 24, 33 and 64 queries (scripts/make_golden_queries.py, cases in tests/queries_cases.py).

Every bound here is the one the existing test of the same kernel uses at 9 or 10 queries; each is named where it is used."""
import json
import os

import numpy as np
import pytest
import torch

import head_cases as H
import queries_cases as QC
import window_cases as W
from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["f32", "bf16x3", "f16x3"]


@pytest.fixture(params=MODES)
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def close(got, want, atol, what=""):
    """tests/test_gpu_ops.py `close`: absolute"""
    got = got.detach().double().cpu() if isinstance(got, torch.Tensor) else torch.as_tensor(got, dtype=torch.float64)
    want = want.detach().double().cpu() if isinstance(want, torch.Tensor) else torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) if got.numel() else 0.0
    assert err <= atol, f"{what}: max abs error {err:.3e} (tolerance {atol:.1e})"


def rel_close(got, want, rtol, what=""):
    """tests/test_gpu_backward.py `rel_close`: relative to the largest entry of the reference"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    assert err <= rtol, f"{what}: max error {err:.3e} of the largest entry (tolerance {rtol:.1e})"


def lens_mask(T, lens):
    return torch.arange(T)[None] < torch.tensor(lens)[:, None]


# ============================================================================================================ mask head
def mask_head_inputs(Q, T):
    g = torch.Generator().manual_seed(1000 * Q + T)
    B = 3
    m = lens_mask(T, [T, max(T // 2, 1), min(3, T)])
    emb, feat = torch.randn(B, Q, 256, generator=g), torch.randn(B, T, 256, generator=g) * m[..., None]
    return B, m, emb, feat


@pytest.mark.parametrize("T", [1, 33, 96])
@pytest.mark.parametrize("Q", [17, 32, 33, 64])
def test_mask_head_above_16_queries(Q, T):
    """Against the f32 einsum at test_gpu_ops.test_mask_head_kernel's 5e-5; then, as test_gpu_windows.test_mask_head_windows, on
    strided windows with NaN guard bands: the same bits, nothing outside the windows touched."""
    from vrdone_amd import _hip, ops
    B, m, emb, feat = mask_head_inputs(Q, T)
    want = torch.einsum("bqc,btc->bqt", emb, feat).masked_fill(~m[:, None], -10.0)
    md = m.to(DEV)
    plain = ops.mask_head(emb.to(DEV), feat.to(DEV), md)
    close(plain, want, 5e-5, "seg")
    lds = W.LdSeq()
    he = W.embed(emb.to(DEV), ld=lds(256), name="emb")
    hf = W.embed(feat.to(DEV).view(B * T, 256), ld=lds(256), name="feat")          # (as rows: at T = 1 a 3-d view has no pitch of its own)
    feat_view = torch.as_strided(hf.view, (B, T, 256), (T * hf.ld, hf.ld, 1), hf.view.storage_offset())
    hs =W.embed_out((B * Q, T), DEV, ld=T, c0=0, rows_before=8, rows_after=8, name="seg")       # (B, Q, T) contiguous by contract
    _hip.check(_hip.lib.vrd_mask_head(he.view.data_ptr(), he.ld, hf.view.data_ptr(), hf.ld, md.data_ptr(), B, Q, T, 256, -10.0,
                                      hs.view.data_ptr(), ops._stream()), "vrd_mask_head")
    got = ops.mask_head(he.view, feat_view, md)
    torch.cuda.synchronize()
    W.check([hs], [he, hf])
    assert W.bits_equal(hs.view, plain.view(B * Q, T)) and W.bits_equal(got, plain)


@pytest.mark.parametrize("Q", [1, 9, 16])
def test_mask_head_up_to_16_queries_keeps_its_bits_inside_a_64_query_buffer(Q):
    """The first Q queries of a 64-query embedding buffer give the bits of the dense Q-query call, and the 64-query call gives
    them too: one fmaf chain per output, whichever kernel runs it.  (A (B, Q, D) slice of a (B, 64, D) buffer is not a row
    matrix of one pitch -- the entry point takes pointer + leading dimension --, so the slice goes pair by pair.)"""
    from vrdone_amd import ops
    T = 96
    B, m, emb64, feat = mask_head_inputs(64, T)
    buf, fd, md = emb64.to(DEV), feat.to(DEV), m.to(DEV)
    dense = ops.mask_head(buf[:, :Q].contiguous(), fd, md)
    sliced = torch.cat([ops.mask_head(buf[b:b + 1, :Q], fd[b:b + 1], md[b:b + 1]) for b in range(B)])
    assert not buf[:, :Q].is_contiguous() or Q == 64
    assert W.bits_equal(sliced, dense)
    assert W.bits_equal(ops.mask_head(buf, fd, md)[:, :Q], dense)


@pytest.mark.parametrize("Q", [17, 33, 64])
def test_mask_head_backward_above_16_queries(Q):
    """autograd.MaskHead (vrd_bmm) against float64 autograd, at test_gpu_backward.test_maxpool_and_mask_head_backward's 2e-5."""
    from vrdone_amd import ops
    g = torch.Generator().manual_seed(Q)
    B, T, Dp = 3, 16, 256
    m = lens_mask(T, [16, 9, 2])
    emb, feat = torch.randn(B, Q, Dp, generator=g), torch.randn(B, T, Dp, generator=g)
    dseg = torch.randn(B, Q, T, generator=g)
    with torch.enable_grad():
        er, fr = emb.double().requires_grad_(True), feat.double().requires_grad_(True)
        sr = torch.einsum("bqc,btc->bqt", er, fr).masked_fill(~m[:, None], -10.0)
        sr.backward(dseg.double())
        ed, fd = emb.to(DEV).requires_grad_(True), feat.to(DEV).requires_grad_(True)
        seg = ops.mask_head(ed, fd, m.to(DEV), -10.0)
        seg.backward(dseg.to(DEV))
    rel_close(seg, sr, 2e-5, "seg")
    rel_close(ed.grad, er.grad, 2e-5, "demb")
    rel_close(fd.grad, fr.grad, 2e-5, "dfeat")


# ============================================================================================================ assignment
def padded(cost):
    """the cost block on the device at its own leading dimension, NaN behind the queries"""
    G, Q = cost.shape
    buf = torch.full((G, cost.stride(0)), float("nan"), device=DEV)
    buf[:, :Q] = cost.to(DEV)
    return buf[:, :Q]


WAVE_CASES = [(kind, Q) for kind in H.ASSIGN_KINDS for Q in (17, 32, 33, 63, 64)]


@pytest.mark.parametrize("kind,Q", WAVE_CASES, ids=[f"{k}-Q{q}" for k, q in WAVE_CASES])
def test_assignment_above_16_queries(kind, Q):
    """ops.assign (vrd_assign forwards to the wave kernel) on tied, quantised, extreme and infinite costs against scipy: the body
    of test_gpu_head_edges.test_assignment_on_tied_quantised_extreme_and_infinite_costs.  A repeat gives the same bits."""
    from vrdone_amd import ops
    cost, sizes = H.assign_inputs(kind, Q)
    expect = H.assign_expect(cost, sizes)
    G, ld = cost.shape[0], cost.stride(0)
    buf = padded(cost)
    got = ops.assign(buf, sizes)
    again = ops.assign(buf, sizes)
    torch.cuda.synchronize()
    assert (ld > Q) == (kind == "ld") and got.dtype == torch.int32 and got.shape == (G,)
    H.check_assignment(got.cpu().numpy(), cost, sizes, expect, exact_sum=(kind == "int"))
    assert torch.equal(got, again)


@pytest.mark.parametrize("kind,Q", H.ASSIGN_CASES, ids=[f"{k}-Q{q}" for k, q in H.ASSIGN_CASES])
def test_wave_assignment_equals_the_one_thread_kernel(kind, Q):
    """vrd_assign_wave at 1, 2, 9 and 16 queries against vrd_assign, element for element, ties and refusals included: one
    pivoting rule, the same float64 operations in the same order."""
    from vrdone_amd import ops
    cost, sizes = H.assign_inputs(kind, Q)
    buf = padded(cost)
    serial, wave = ops.assign(buf, sizes), ops.assign(buf, sizes, wave=True)
    torch.cuda.synchronize()
    assert torch.equal(serial, wave), (serial != wave).nonzero()[:8].tolist()
    H.check_assignment(wave.cpu().numpy(), cost, sizes, H.assign_expect(cost, sizes), exact_sum=(kind == "int"))


@pytest.mark.parametrize("Q", [9, 33, 64])
@pytest.mark.parametrize("poison", [float("nan"), float("-inf")])
def test_wave_assignment_refuses_a_poisoned_block_between_two_solvable_ones(Q, poison):
    """A NaN / -inf entry anywhere in a pair's block, even one the search would never visit: -1 for the whole pair (scipy
    raises), its neighbours solved as scipy solves them.  More relations than queries: -1 as well."""
    from vrdone_amd import _hip, ops
    g = torch.Generator().manual_seed(Q)
    n = max(Q // 2, 1)
    sizes = [n, n, n]
    cost = torch.randn(3 * n, Q, generator=g)
    cost[n + n - 1, Q - 1] = poison
    got = ops.assign(cost.to(DEV), sizes, wave=True).cpu()
    clean = H.solve_pairs(cost[:n], [n]), H.solve_pairs(cost[2 * n:], [n])
    assert bool((got[n:2 * n] == -1).all())
    assert torch.equal(got[:n].long(), clean[0]) and torch.equal(got[2 * n:].long(), clean[1])
    if Q < 64:          # count > Q, through the entry point (ops.assign asserts N <= Q): a block of Q + 1 rows, then a solvable one
        cost = torch.randn(Q + 1 + n, Q, generator=g).to(DEV)
        first, count = ops.assign_tables([Q + 1, n], DEV)
        out = torch.full((Q + 1 + n,), -7, dtype=torch.int32, device=DEV)
        _hip.check(_hip.lib.vrd_assign_wave(cost.data_ptr(), Q, first.data_ptr(), count.data_ptr(), 2, Q, out.data_ptr(), ops._stream()),
                   "vrd_assign_wave")
        assert bool((out[:Q + 1] == -1).all()) and torch.equal(out[Q + 1:].cpu().long(), H.solve_pairs(cost[Q + 1:].cpu(), [n]))


# ============================================================================================================= criterion
CRITERION_Q = [H._case(f"q{Q}_l{L}", 3, Q, 133, 96, L, [Q, 0, 1], [96, 61, 2], weights="eos") for Q in (17, 64) for L in (1, 4)]
CRITERION_Q = [dict(c, fuzzy=fz) for c in CRITERION_Q for fz in (False, True)]
_criterion = {}


def criterion_case(i):
    if i not in _criterion:
        inp = H.criterion_inputs(CRITERION_Q[i])
        _criterion[i] = (inp, H.criterion_form(inp, torch.float64))
    return _criterion[i]


@pytest.mark.parametrize("i", range(len(CRITERION_Q)), ids=[H.case_id(c) for c in CRITERION_Q])
def test_criterion_kernels_above_16_queries(i):
    """Costs, assignment, losses and both gradients per element against float64 within head_cases.criterion_bound() (8 E over
    the existing case table), as test_gpu_head_edges.test_criterion_kernels_against_float64; then the fused path against the
    tensor form of models/losses.py on the device at test_gpu_train.test_fused_criterion_equals_the_tensor_form's bounds."""
    import torch.nn.functional as F
    from test_gpu_head_edges import device_costs, device_criterion
    from vrdone_amd.models import losses
    inp, ref = criterion_case(i)
    got = device_criterion(inp)
    got["cost"] = device_costs(inp)
    H.check_criterion(got, ref, inp, H.criterion_bound(), label="QUERIES criterion " + H.case_id(CRITERION_Q[i]))
    # ---- the tensor form on the device, with the fused path's own assignment
    L, B, Q, G = inp["L"], inp["B"], inp["Q"], inp["G"]
    d = lambda t: t.to(DEV)                                  # noqa: E731
    valid, owner, ids, tgt = d(inp["valid"]), d(inp["owner"]), d(inp["ids"]), d(inp["tgt"])
    seg_d = d(inp["segs"]) if inp["fuzzy"] else None
    for l in range(L):
        with torch.enable_grad():
            lg, mk = d(inp["logits"][l]).requires_grad_(True), d(inp["masks"][l]).requires_grad_(True)
            with torch.no_grad():
                cc, cm, cd = losses.pair_costs(lg, mk, valid, ids, tgt, owner, seg_d, inp["scale_range"])
                cost = (inp["cost_w"][0] * cc + inp["cost_w"][1] * cm + inp["cost_w"][2] * cd).cpu()
            assert torch.equal(got["q_of"][l].long(), H.solve_pairs(cost, inp["sizes"])), l       # scipy on the tensor costs
            q = d(got["q_of"][l].long())
            target = torch.zeros(B, Q, dtype=torch.int64, device=DEV)
            target[owner, q] = ids
            ce = F.cross_entropy(lg.transpose(1, 2), target, d(inp["weight"]))
            focal, dice = losses.matched_losses(mk[owner, q], tgt, float(G), valid[owner], seg_d, inp["scale_range"])
            want = torch.stack([ce, focal, dice])
            (want * d(inp["coef"][l])).sum().backward()
        assert float((d(got["loss"][l]) - want).detach().abs().max()) < 2e-6 * max(1.0, float(want.detach().abs().max())), (l, got["loss"][l], want)
        for a, b in ((got["glogit"][l], lg.grad), (got["gmask"][l], mk.grad)):
            assert float((d(a) - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max())) + 1e-7, l


# ============================================================================================================= attention
ATTN_SHAPES = [(H_, hd, Tq, Tk) for H_, hd in ((8, 32), (4, 64)) for Tq in (17, 33, 64) for Tk in (1, 12, 36, 64)]
_attn = {}


def attn_case(n_head, hd, Tq, Tk):
    """inputs as (B, T, C) rows, key mask with one sequence of a single valid key, and float64 (out, dq, dk, dv): once per shape"""
    key = (n_head, hd, Tq, Tk)
    if key not in _attn:
        g = torch.Generator().manual_seed(hd * 10000 + Tq * 100 + Tk)
        B, C = 3, n_head * hd
        q, dO = torch.randn(B, Tq, C, generator=g) * 2.0, torch.randn(B, Tq, C, generator=g)
        k, v = torch.randn(B, Tk, C, generator=g), torch.randn(B, Tk, C, generator=g)
        km = lens_mask(Tk, [Tk, max(1, Tk // 2 + 1), 1])
        with torch.enable_grad():
            qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
            out = O.full_attention(qr.transpose(1, 2), kr.transpose(1, 2), vr.transpose(1, 2), km[:, None], n_head).transpose(1, 2)
            out.backward(dO.double())
        _attn[key] = (q, k, v, dO, km, (out.detach(), qr.grad, kr.grad, vr.grad))
    return _attn[key]


@pytest.mark.parametrize("n_head,hd,Tq,Tk", ATTN_SHAPES)
def test_predictor_attention_shapes_forward(n_head, hd, Tq, Tk):
    """ops.attention on f32 rows with Tq = the query count (self-attention Tk = Tq, cross-attention Tk = the coarsest level's
    frames): above 16 queries the generic kernel at head_dim 32, the flash kernel at 64; test_gpu_ops' 3e-5."""
    from vrdone_amd import ops
    q, k, v, _, km, ref = attn_case(n_head, hd, Tq, Tk)
    with torch.no_grad():
        close(ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), km.to(DEV), n_head), ref[0], 3e-5, "out")
        if hd == 64:
            close(ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), km.to(DEV), n_head, algo=1), ref[0], 3e-5, "out (generic kernel)")


@pytest.mark.parametrize("n_head,hd,Tq,Tk", ATTN_SHAPES)
def test_predictor_attention_shapes_backward(n_head, hd, Tq, Tk, precision):
    """autograd.Attention at those shapes against float64.  From 32 queries and 32 keys on the split modes take the flash pair
    (vrd_attention_rows / vrd_attention_bwd) -- here at Tq = 33, a partial second query tile --, held to
    test_global_attention_backward_fused's bounds (bf16x3 1e-4, f16x3 2e-5); every other case runs the generic forward and the
    five-product backward at tests/test_gpu_backward.py's 2e-5 (2e-4 in the bf16x3 mode, that file's bound for its products)."""
    from vrdone_amd import autograd, ops
    q, k, v, dO, km, ref = attn_case(n_head, hd, Tq, Tk)
    flash = autograd._flash_attention_route(ops.split_backward(), hd, Tq, Tk)
    assert flash == (precision != "f32" and Tq >= 32 and Tk >= 32)
    with torch.enable_grad():
        qd, kd, vd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, v))
        out = ops.attention(qd, kd, vd, km.to(DEV), n_head)
        out.backward(dO.to(DEV))
    tol = 2e-5 if precision != "bf16x3" else (1e-4 if flash else 2e-4)
    for name, a, r in zip(("out", "dq", "dk", "dv"), (out, qd.grad, kd.grad, vd.grad), ref):
        rel_close(a, r, tol, name)
    assert not bool(kd.grad[2, 1:].any()) and not bool(vd.grad[2, 1:].any())          # masked keys: exactly zero dk / dv


# ================================================================================================================= model
LOGIT_TOL, MASK_TOL = 2e-4, 2e-3           # tests/test_gpu_model.py
BF16X3_TIE = {"bf16x3": 5e-6}              # tests/test_gpu_model.py
_models = {}


def build_model(base, Q, train=False):
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, ic, keys = load_case(base)
    mc = QC.model_config(mc, Q)
    model = MaskVRD(mc, device=DEV)
    model.load_state_dict(O.synth_state_dict(QC.state_keys(keys, mc), eos_coef=mc["loss_coeff_dict"]["eos_coef"]), strict=True)
    model = model.to(DEV)
    return (model.train() if train else model.eval()), mc, ic


def get_model(base, Q):
    if (base, Q) not in _models:
        model, mc, ic = build_model(base, Q)
        model._config_eval(ic)
        _models[base, Q] = (model, mc, ic)
    return _models[base, Q]


def case_inputs(case):
    spec = QC.MODEL_CASES[case]
    model, mc, ic = get_model(spec["base"], spec["Q"])
    x, m = O.synth_pairs(len(spec["lens"]), QC.c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
    return model, x.to(DEV), m.to(DEV)


@pytest.fixture(scope="module")
def golden():
    return QC.load_npz("queries_model")


class rows_form:
    """_mask_vrd in the ragged row space: buckets as fine as tight padding allows, however few their rows"""

    def __init__(self, model, on=True):
        self.model, self.on = model, on

    def __enter__(self):
        if self.on:
            self.model.ROWS_MIN_ROWS = 0

    def __exit__(self, *exc):
        if self.on:
            del self.model.ROWS_MIN_ROWS


@pytest.mark.parametrize("form", ["batch", "rows"])
@pytest.mark.parametrize("case", list(QC.MODEL_CASES))
def test_mask_vrd_matches_reference_golden(case, form, precision, golden):
    """_mask_vrd at 24, 64 and 33 queries against the reference, all heads, at tests/test_gpu_model.py's 2e-4 / 2e-3, in the
    batch form and in the ragged row space."""
    model, x, m = case_inputs(case)
    with torch.no_grad(), rows_form(model, form == "rows"):
        plan = model._tight_plan(m, m.reshape(m.shape[0], -1))
        assert (plan is not None and plan["rows"] and len(plan["buckets"]) >= 3) if form == "rows" else plan is None
        out = model._mask_vrd(x, m)
        fast = model._mask_vrd(x, m, with_aux=False)
    assert len(out["aux_outputs"]) == 3 and "aux_outputs" not in fast
    for pre, lg, mk in QC.heads(out):
        if pre:
            lg, mk = lg[..., ::QC.CLASS_STRIDE], mk[..., ::QC.MASK_T_STRIDE]
        close(lg, golden[f"{case}/{pre}pred_logits"], LOGIT_TOL, pre + "pred_logits")
        close(mk, golden[f"{case}/{pre}pred_masks"], MASK_TOL, pre + "pred_masks")
    assert torch.equal(fast["pred_logits"], out["pred_logits"]) and torch.equal(fast["pred_masks"], out["pred_masks"])


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("case", list(QC.MODEL_CASES))
def test_reference_grade_against_float64(case, mode, golden):
    """tests/test_gpu_model.py::test_reference_grade_against_float64 at the new query counts: within 2 x (f32: 4 x on the worst
    element) the reference's own float32 distance from its float64 run, worst element and rms."""
    from vrdone_amd import ops
    model, x, m = case_inputs(case)
    with torch.no_grad(), ops.use_precision(mode):
        out = model._mask_vrd(x, m, with_aux=False)
    for k in ("pred_logits", "pred_masks"):
        ref32 = golden[f"{case}/{k}"].astype(np.float64)
        e32 = np.abs(golden[f"{case}/f64m32_{k}"].astype(np.float64))
        e = np.abs(out[k].double().cpu().numpy() - (ref32 + golden[f"{case}/f64m32_{k}"].astype(np.float64)))
        r_max, r_rms = float(e.max() / e32.max()), float(np.sqrt((e ** 2).mean() / (e32 ** 2).mean()))
        print(f"[{case}/{mode}] {k}: max {e.max():.3e} vs ref32 {e32.max():.3e} (x{r_max:.2f}), rms x{r_rms:.2f}")
        assert r_max <= (2.0 if mode == "f16x3" else 4.0) and r_rms <= 2.0, (case, mode, k, r_max, r_rms)


@pytest.mark.parametrize("case", list(QC.MODEL_CASES))
def test_mask_vrd_f16x1_against_reference_golden(case, golden):
    """The one-product mode at its own stated tolerance (tests/test_gpu_f16x1.py: 1e-2 / 1e-1), and really another kernel path."""
    from vrdone_amd import ops
    model, x, m = case_inputs(case)
    with torch.no_grad():
        with ops.use_precision("f16x1"):
            ops.f16_range_flag().zero_()
            out = model._mask_vrd(x, m, with_aux=False)
            assert ops.f16_range_exceeded() == 0
        with ops.use_precision("f16x3"):
            ref3 = model._mask_vrd(x, m, with_aux=False)
    dl = float(np.abs(out["pred_logits"].cpu().numpy() - golden[f"{case}/pred_logits"]).max())
    dm = float(np.abs(out["pred_masks"].cpu().numpy() - golden[f"{case}/pred_masks"]).max())
    print(f"f16x1 {case}: max |dlogit| {dl:.2e}, max |dmask| {dm:.2e}")
    assert dl <= 1e-2 and dm <= 1e-1, (dl, dm)
    assert not torch.equal(ref3["pred_logits"], out["pred_logits"])


@pytest.mark.parametrize("case", list(QC.MODEL_CASES))
def test_row_space_form_gives_the_same_outputs(case, precision):
    """tests/test_gpu_model.py::test_row_space_form_gives_the_same_outputs: the batch's buckets in one row space against the
    batch at its own padded length, at that test's tolerances, the reference's -10 behind every pair's frames."""
    model, x, m = case_inputs(case)
    try:
        with torch.no_grad(), rows_form(model):
            rows = model._mask_vrd(x, m)
            model.tight_padding = False
            full = model._mask_vrd(x, m.clone())
    finally:
        model.tight_padding = True
    tol = 2e-4 if precision == "bf16x3" else 2e-5
    for (pre, a_l, a_m), (_, b_l, b_m) in zip(QC.heads(rows), QC.heads(full)):
        close(a_l, b_l, tol, pre + "pred_logits")
        close(a_m, b_m, 10 * tol, pre + "pred_masks")
    pad = ~m[:, 0][:, None, :].expand(-1, rows["pred_masks"].shape[1], -1)
    assert bool((rows["pred_masks"][pad] == -10.0).all())


def on_device(data):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}


def test_forward_test_24_queries_matches_reference_golden(precision):
    """forward_test records at 24 queries on the proposal of forward_test_vidvrd.json, as
    tests/test_gpu_model.py::test_forward_test_matches_reference_golden; bucket by bucket and in one row space."""
    from golden_cases import compare_forward_test
    model, mc, ic = get_model("vidvrd", 24)
    with open(os.path.join(GOLDEN, "forward_test_vidvrd_q24.json")) as f:
        ref = json.load(f)
    data = on_device(synth_proposal(c_in=QC.c_in(mc), **QC.FORWARD_TEST_Q24))
    with torch.no_grad():
        res = model(data)
        try:
            model.ROWS_MIN_PAIRS = 1
            rows = model(data)
        finally:
            del model.ROWS_MIN_PAIRS
    assert len(res["triplets"]) == len(ref["triplets"]) == ic["n_max_pair"]
    for got in (res, rows):
        compare_forward_test(got, ref, ic["n_max_pair"], 5e-6, slack=0, tie_tol=BF16X3_TIE.get(precision, 0.0))


@pytest.mark.parametrize("base,Q", [("vidvrd", 24), ("vidvrd", 64), ("vidor_x", 33)])
def test_forward_test_videos_equals_one_call_per_video(base, Q, precision):
    """Three videos in one call (the candidate buffers and the 32-bit candidate index scale with the query count) against
    forward_test video by video: the same records, scores as tests/test_gpu_batched_eval.py compares them."""
    model, mc, ic = get_model(base, Q)
    stride = ic["feat_stride"]
    lo, hi = (20, 90) if stride == 1 else (150, 500)
    videos = [on_device(synth_proposal(n, QC.c_in(mc), lo, hi, seed=50 + i, feat_stride=stride, random_offset=stride > 1))
              for i, n in enumerate((5, 7, 4))]
    with torch.no_grad():
        want = [model.forward_test(v) for v in videos]
        got = model.forward_test_videos(videos)
    assert len(got) == 3 and all(w is not None for w in want)
    for g, w in zip(got, want):
        for key in ("triplets", "so_tids", "pred_durations", "so_trajs"):
            assert g[key] == w[key], key
        for key in ("triple_scores", "triple_scores_avg"):
            np.testing.assert_allclose(np.array(g[key]), np.array(w[key]), atol=1e-5, rtol=0)


# ============================================================================================================== training
POOL_FREE = r"(backbone\.branch\.[12]\.|neck\.|predictor\.)"        # tests/test_gpu_train.py


def train_setup():
    from vrdone_amd.models.blocks import AffineDropPath
    model, mc, _ = build_model("vidvrd", 24, train=True)
    with open(os.path.join(GOLDEN, "train_step_vidvrd_q24.json")) as f:
        meta = json.load(f)
    lens, _, _, data = QC.train_batch(mc, device=DEV)
    assert lens == meta["lengths"] and [len(p) for p in data["preds_list"]] == meta["sizes"]
    for mod in model.modules():
        if isinstance(mod, AffineDropPath):
            mod.drop_prob = 0.0
    return model, meta, data


def loss_tol(precision):
    return 1e-5 if precision == "f32" else 2e-4


@pytest.mark.parametrize("graphs", [False, True])
def test_training_step_24_queries_matches_reference_gradients(graphs, precision):
    """model.train()(batch) -> total_loss.backward() at 24 queries with 1 .. 24 relations a pair against the reference's own
    training step (stochastic depth off, the reference's matching replayed), eager and replayed as HIP graphs: the body and the
    bounds of tests/test_gpu_local_heads.py::test_training_step_width_256_matches_reference_gradients."""
    from golden_cases import compare_grads, replay_matching
    from vrdone_amd import train_graph
    model, meta, data = train_setup()
    gt = QC.load_npz("train_step_vidvrd_q24")
    model.enable_training_graphs(graphs)
    try:
        with torch.enable_grad():
            for step in range(2 if graphs else 1):          # (the second step replays what the first recorded)
                if step:
                    del model.bipartite_match               # the recorded assignments cover one step: start them again
                differing = replay_matching(model, meta["cases"]["nodrop"]["indices"])
                model.zero_grad(set_to_none=True)
                loss = model(data)
                loss["total_loss"].backward()
        assert not graphs or len(train_graph.recordings(model)) == 1
    finally:
        model.enable_training_graphs(False)
        train_graph.forget(model)
    want = meta["cases"]["nodrop"]["losses"]
    assert set(loss) == set(want)
    for k, v in want.items():
        print(f"[q24/{precision}/graphs={graphs}] {k}: {float(loss[k].detach()):.7f} (reference {v:.7f})")
    for k, v in want.items():
        assert abs(float(loss[k].detach()) - v) <= loss_tol(precision) * max(1.0, abs(v)), (k, float(loss[k]), v)
    assert all(len(call) <= 6 for call in differing), differing
    worst, median = compare_grads(((n, p.grad) for n, p in model.named_parameters()), gt, meta, "nodrop",
                                  rtol=3e-2, atol_frac=1e-4, median_tol=2e-5 if precision == "f32" else 5e-4, outlier_tol=1e-3,
                                  max_outliers=3, outlier_scope=None if precision != "bf16x3" else POOL_FREE)
    print(f"[q24/{precision}/graphs={graphs}] relative gradient error: worst {worst:.2e}, median {median:.2e}")


def test_training_step_24_queries_fused_criterion_matches_reference_losses(precision, monkeypatch):
    """The same step with the model's own matching: the fused device criterion (costs -> vrd_assign, here the wave kernel ->
    losses) gives the reference's loss dict at the loss tolerance of the test above, and its assignments are the reference's
    recorded ones on all but at most that test's 6 pairs per matcher call."""
    from vrdone_amd.models import losses
    model, meta, data = train_setup()
    calls = []
    real = losses.device_criterion

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append(out[1])
        return out
    monkeypatch.setattr(losses, "device_criterion", spy)
    with torch.enable_grad():
        loss = model(data)
        loss["total_loss"].backward()
    assert len(calls) == 1 and calls[0].shape[0] == 4           # one fused call for the four heads
    want = meta["cases"]["nodrop"]["losses"]
    assert set(loss) == set(want)
    for k, v in want.items():
        print(f"[q24 fused/{precision}] {k}: {float(loss[k].detach()):.7f} (reference {v:.7f})")
    for k, v in want.items():
        assert abs(float(loss[k].detach()) - v) <= loss_tol(precision) * max(1.0, abs(v)), (k, float(loss[k]), v)
    sizes = meta["sizes"]
    q_of = calls[0].cpu()
    for l, call in enumerate(meta["cases"]["nodrop"]["indices"]):
        differing = []
        for n, (block, (qi, ri)) in enumerate(zip(q_of[l].split(sizes), call)):
            ref_q = torch.empty(len(ri), dtype=torch.int64)
            ref_q[torch.tensor(ri, dtype=torch.int64)] = torch.tensor(qi, dtype=torch.int64)
            if not torch.equal(block.long(), ref_q):
                differing.append(n)
        assert len(differing) <= 6, (l, differing)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
