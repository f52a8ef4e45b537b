"""Banded attention at any odd window from 3 to 19 on the MI355X: vrd_local_attn / _segs / _bwd and the modules above them
against goldens of the real reference at windows 5, 11 and 19 (scripts/make_golden_window.py, cases in
tests/local_window_cases.py) and against the float64 oracle at every window, 3 included (the reference's own code fails
at window 3, see local_window_cases.REF_WINDOWS).

Windows 3 .. 9 run the whole-row strip kernel, 11 .. 19 the half-row one (csrc/vrd_local_attn.hip); the cases cover both with
4 and 8 heads, with and without rel_pe: two full strips of 16 rows and a partial one, a sequence of half a window, a
fully masked sequence.  Tolerances are those of the existing tests of the same op and mode (tests/test_gpu_ops.py,
test_gpu_backward.py, test_gpu_train.py, test_gpu_model.py): the banded kernels compute in f32 on the vector units in
every precision mode."""
import json
import os

import numpy as np
import pytest
import torch

import local_window_cases as LW
from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL, MASK_TOL = 2e-4, 2e-3           # tests/test_gpu_model.py


@pytest.fixture(params=["f32", "f16x3", "bf16x3"])
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(GOLDEN, "local_window.npz")) as z:
        return {k: z[k] for k in z.files}


_oracle = {}


def oracle_core(W, H, rel):
    """float64 oracle of a core case, computed once: out, dq, dk, dv (B, T, C) and d rel_pe."""
    key = (W, H, rel)
    if key not in _oracle:
        q, k, v, dO, rel_pe = LW.core_inputs(W, H, rel)
        leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
        bias = rel_pe.double().requires_grad_(True) if rel else None
        with torch.enable_grad():
            out = O.banded_attention(*leaves, LW.mask(W), H, W // 2, rel_pe=bias)
            out.backward(dO.double())
        _oracle[key] = tuple(cl(t.detach()) for t in (out, *(l.grad for l in leaves))) + (bias.grad if rel else None,)
    return _oracle[key]


def cl(x):          # (B, C, T) -> (B, T, C)
    return x.transpose(1, 2).contiguous()


def sub(t):
    """(B, T, C) on the device -> the stored (B, C / 17, T) sample"""
    return t.detach().float().cpu().transpose(1, 2)[:, ::LW.CH_STRIDE].numpy()


def close(got, want, atol):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().double().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, atol=atol, rtol=0)


def rel_close(got, want, rtol, what=""):
    """tests/test_gpu_backward.py: largest error over the largest entry"""
    got = got.detach().double().cpu() if isinstance(got, torch.Tensor) else torch.as_tensor(got, dtype=torch.float64)
    want = want.detach().double().cpu() if isinstance(want, torch.Tensor) else torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    assert err <= rtol, f"{what}: max error {err:.3e} of the largest entry (tolerance {rtol:.1e})"


def c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


def raw(t):
    from vrdone_amd import ops
    return t.t if isinstance(t, ops.Pair) else t


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("W,H,rel", LW.ALL_OP_CASES)
def test_forward_plain_pair_and_row_groups(g, W, H, rel, precision):
    """ops.local_attention on the core cases: f32 rows against the float64 oracle (every channel) and the reference's
    stored output (windows 5, 11, 19); pair rows decode to the f32 rows within the format's error; the same sequences and
    a second group of another length as ONE row-group launch give the bits of the launches per group."""
    from vrdone_amd import ops
    q, k, v, _, rel_pe = LW.core_inputs(W, H, rel)
    T, hw = LW.seq_len(W), W // 2
    qd, kd, vd = (cl(t).to(DEV) for t in (q, k, v))
    m = LW.mask(W)[:, 0].to(DEV)
    reld = rel_pe.to(DEV) if rel else None
    with torch.no_grad():
        got = ops.local_attention(qd, kd, vd, m, H, hw, rel_pe=reld)
        close(got, oracle_core(W, H, rel)[0], 2e-5)
        if W in LW.REF_WINDOWS:
            close(sub(got), g[f"core/{LW.tag(W, H, rel)}/out"], 2e-5)
        assert float(got[2].abs().max()) == 0.0 and float(got[1, hw:].abs().max()) == 0.0          # masked query rows: exact zeros
        pair = ops.local_attention(qd, kd, vd, m, H, hw, pair=True, rel_pe=reld)
        assert isinstance(pair, ops.Pair) == (precision != "f32")
        assert float((pair.float() - got).abs().max()) <= 2 ** -15 * float(got.abs().max())      # (tests/test_gpu_ops.py)
        # row groups: all three sequences at T frames, then the first two cut to T2 = 21 frames (a partial second strip)
        T2 = 21
        rows = lambda t: torch.cat([t.reshape(-1, *t.shape[2:]), t[:2, :T2].reshape(-1, *t.shape[2:])])[None]      # noqa: E731
        segs = [(0, 3, T), (3 * T, 2, T2)]
        for as_pair in (False, True):
            one = raw(ops.local_attention(rows(qd), rows(kd), rows(vd), rows(m), H, hw, pair=as_pair, rel_pe=reld, segs=segs))
            a = raw(ops.local_attention(qd, kd, vd, m, H, hw, pair=as_pair, rel_pe=reld))
            cut = lambda t: t[:2, :T2].contiguous()      # noqa: E731
            b = raw(ops.local_attention(cut(qd), cut(kd), cut(vd), cut(m), H, hw, pair=as_pair, rel_pe=reld))
            assert torch.equal(one[0, :3 * T].view(3, T, -1), a) and torch.equal(one[0, 3 * T:].view(2, T2, -1), b)


@pytest.mark.parametrize("W", [3, 9, 13, 19])
def test_forward_odd_shapes_against_oracle(W):
    """Every window form on shapes the goldens do not have: sequences shorter than half a window + 1, validity with holes, a
    strip that is all padding inside a live sequence, one valid frame at the very end, T = 50 (three strips and 2 rows), a
    number of strips that does not fill the last workgroup; windows 15 and 17 (no golden) on the plain case."""
    from vrdone_amd import ops
    gen = torch.Generator().manual_seed(W)
    for H in (4, 8):
        for B, T in ((5, 50), (3, W // 2), (2, 1)):
            q, k, v = (torch.randn(B, T, 512, generator=gen) for _ in range(3))
            mask = torch.rand(B, T, generator=gen) > 0.3
            if T == 50:
                mask[1, 16:32] = False
                mask[2] = False
                mask[2, 49] = True
                mask[3] = False
            rel = torch.randn(1, 1, H, W, generator=gen)
            for bias in (None, rel):
                want = O.banded_attention(q.transpose(1, 2).double(), k.transpose(1, 2).double(), v.transpose(1, 2).double(),
                                          mask[:, None], H, W // 2, rel_pe=None if bias is None else bias.double()).transpose(1, 2)
                got = ops.local_attention(q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, W // 2,
                                          rel_pe=None if bias is None else bias.to(DEV))
                close(got, want, 2e-5)
    for W2 in (15, 17):
        q, k, v = (torch.randn(2, 40, 512, generator=gen) for _ in range(3))
        mask = torch.arange(40)[None] < torch.tensor([40, 23])[:, None]
        want = O.banded_attention(q.transpose(1, 2).double(), k.transpose(1, 2).double(), v.transpose(1, 2).double(), mask[:, None], 4,
                                  W2 // 2).transpose(1, 2)
        close(ops.local_attention(q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), 4, W2 // 2), want, 2e-5)


@pytest.mark.parametrize("window", [1, 21])
def test_argument_errors(window):
    from vrdone_amd import ops
    q = torch.zeros(1, 16, 512, device=DEV)
    with pytest.raises(ValueError, match="odd, from 3 to 19"):
        ops.local_attention(q, q, q, torch.ones(1, 16, dtype=torch.bool, device=DEV), 4, window // 2)


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("W,H,rel", LW.ALL_OP_CASES)
def test_backward(g, W, H, rel):
    """autograd.LocalAttention: dq, dk, dv and d rel_pe against float64 autograd of the oracle (every element) and against the
    reference's stored gradients; in deterministic mode two runs give the same bits."""
    from vrdone_amd import ops
    q, k, v, dO, rel_pe = LW.core_inputs(W, H, rel)
    m = LW.mask(W)[:, 0].to(DEV)
    want = oracle_core(W, H, rel)
    runs = []
    for det in (None, True, True):
        ops.set_deterministic(det)
        try:
            leaves = [cl(t).to(DEV).requires_grad_(True) for t in (q, k, v)]
            bias = rel_pe.clone().to(DEV).requires_grad_(True) if rel else None
            with torch.enable_grad():
                out = ops.local_attention(*leaves, m, H, W // 2, rel_pe=bias)
            out.backward(cl(dO).to(DEV))
        finally:
            ops.set_deterministic(None)
        grads = [out.detach()] + [t.grad for t in leaves] + ([bias.grad] if rel else [])
        for name, a, r in zip(("out", "dq", "dk", "dv"), grads, want):
            rel_close(a, r, 2e-5, name)
        if rel:
            rel_close(bias.grad, want[4], 2e-5, "d rel_pe")
        if W in LW.REF_WINDOWS:
            p = f"core/{LW.tag(W, H, rel)}/"
            for name, a in zip(("out", "dq", "dk", "dv"), grads):
                rel_close(sub(a), g[p + name], 2e-5, name + " vs reference")
            if rel:
                rel_close(bias.grad.cpu(), g[p + "drel"], 2e-5, "d rel_pe vs reference")
        runs.append(grads)
    assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[2])), "deterministic mode: two runs differ"


def _rel(got, want, floor=0.0):
    """tests/test_gpu_train.py: l2 error relative to the l2 norm of `want` (+ floor for gradients that are mathematically zero)"""
    got = got.detach().double().cpu() if isinstance(got, torch.Tensor) else torch.as_tensor(got, dtype=torch.float64)
    want = want.detach().double().cpu() if isinstance(want, torch.Tensor) else torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    return float((got - want).norm()) / (float(want.norm()) + floor + 1e-12)


@pytest.mark.parametrize("W,H,rel", LW.OP_CASES)
def test_local_mhca_module_forward_backward(g, W, H, rel, precision):
    """blocks.LocalMaskedMHCA with the reference's weights: output, input gradient and every parameter's gradient (projection
    weights, rel_pe) against the reference's; bounds of tests/test_gpu_train.py's module tests (5e-5 in f32, 5e-4 in the split modes)."""
    from vrdone_amd.models.blocks import LocalMaskedMHCA
    x, dy = LW.mhca_inputs(W, H, rel)
    pre = LW.mhca_prefix(W, H, rel)
    mod = LocalMaskedMHCA(512, H, window_size=W, use_rel_pe=rel)
    sd = O.synth_state_dict([(f"{pre}.{k}", tuple(t.shape)) for k, t in mod.state_dict().items()])
    mod.load_state_dict({k[len(pre) + 1:]: t for k, t in sd.items()}, strict=True)
    mod = mod.to(DEV).eval()
    xd = x.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        out, _ = mod(xd, LW.mask(W).to(DEV))
    out.backward(dy.to(DEV))
    tol = 5e-5 if precision == "f32" else 5e-4
    p = f"mhca/{LW.tag(W, H, rel)}/"
    pick = lambda t: t.detach().cpu()[:, ::LW.CH_STRIDE]      # noqa: E731
    assert _rel(pick(out), g[p + "out"]) < tol and _rel(pick(xd.grad), g[p + "dx"]) < tol
    names = [n for n, _ in mod.named_parameters()]
    assert ("rel_pe" in names) == rel
    floor = 1e-3 * max(float(g[p + "norm/" + n]) for n in names)
    for n, prm in mod.named_parameters():
        assert prm.grad is not None, n
        assert _rel(LW.sample(prm.grad).cpu(), g[p + "d/" + n], floor) < tol, n


@pytest.mark.parametrize("W", LW.SOS_WINDOWS)
def test_sos_local_decoder_layer_forward_backward(g, W, precision):
    """local_transformer.LocalMaskedMHCA_QKV inside the vidor_local decoder layer at windows 5 and 19."""
    from vrdone_amd.models.local_transformer import MaskedConvTransformerDecoderLayer
    x, y, dy, m = LW.sos_inputs(W)
    pre = f"op.sos_local_w{W}"
    layer = MaskedConvTransformerDecoderLayer(512, 8, path_pdrop=0.1, n_qx_stride=1, n_kv_stride=1, with_ffn=False, use_local=True, win_size=W)
    sd = O.synth_state_dict([(f"{pre}.{k}", tuple(t.shape)) for k, t in layer.state_dict().items()])
    layer.load_state_dict({k[len(pre) + 1:]: t for k, t in sd.items()}, strict=True)
    layer = layer.to(DEV).eval()
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        out, _ = layer(xd, yd, m.to(DEV), m.to(DEV))
    out.backward(dy.to(DEV))
    tol = 5e-5 if precision == "f32" else 5e-4
    p = f"sos/w{W}/"
    pick = lambda t: t.detach().cpu()[:, ::LW.CH_STRIDE]      # noqa: E731
    assert _rel(pick(out), g[p + "out"]) < tol
    assert _rel(pick(xd.grad), g[p + "dx"]) < tol and _rel(pick(yd.grad), g[p + "dy"]) < tol


# ------------------------------------------------------------------------------------------------------ f16 range flag
@pytest.mark.parametrize("n_head", [4, 8])
@pytest.mark.parametrize("segs,b,c", [(False, 2, 511), (True, 0, 259)])
def test_f16_range_flag_at_window_19(n_head, segs, b, c):
    """The half-row kernel as a producer of f16 planes (tests/test_gpu_f16_range.py, tag 32): an output beyond the f16 operand
    range sets the flag, in-range values and the other modes do not.  A row's probabilities sum to 1 within (W + 2) roundings
    of 2^-24 = 1.3e-6 at W = 19: inside that file's bound of 2e-6."""
    from test_gpu_f16_range import ABIG, AOK, LOCAL_REL, _local_case, check_producer
    with torch.no_grad():
        check_producer(_local_case(n_head, 9, segs, b, c), 32, big=ABIG, ok=AOK, rel=LOCAL_REL, consumer=(c == 511))


# --------------------------------------------------------------------------------------------------------------- model
_models = {}


def get_model(case):
    if case not in _models:
        from vrdone_amd.models.maskvrd import MaskVRD
        mc, ic, keys = load_case(LW.MODEL_CASES[case]["base"])
        sd = O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"])
        mc = LW.model_config(mc, case)
        model = MaskVRD(mc, device=DEV)
        model.load_state_dict(sd, strict=True)
        model = model.to(DEV).eval()
        model._config_eval(ic)
        _models[case] = (model, mc, ic)
    return _models[case]


@pytest.mark.parametrize("case", list(LW.MODEL_CASES))
def test_mask_vrd_matches_reference_golden(case, precision):
    """_mask_vrd with tight padding on (pairs computed at lengths that are no multiple of the window's chunk) against the
    reference at its own padded length."""
    model, mc, _ = get_model(case)
    spec = LW.MODEL_CASES[case]
    gm = np.load(os.path.join(GOLDEN, "local_window_model.npz"))
    x, m = O.synth_pairs(len(spec["lens"]), c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
    assert model.tight_padding and any(model.tight_len(L, spec["T"]) < spec["T"] for L in spec["lens"])
    with torch.no_grad():
        out = model._mask_vrd(x.to(DEV), m.to(DEV), with_aux=False)
    close(out["pred_logits"], gm[f"{case}/pred_logits"], LOGIT_TOL)
    close(out["pred_masks"], gm[f"{case}/pred_masks"], MASK_TOL)


BF16X3_TIE = {"bf16x3": 5e-6}       # tests/test_gpu_model.py


def test_forward_test_window_19_matches_reference_golden(precision):
    from golden_cases import compare_forward_test
    model, mc, ic = get_model("vidvrd_w19")
    with open(os.path.join(GOLDEN, "forward_test_vidvrd_w19.json")) as f:
        ref = json.load(f)
    data = synth_proposal(c_in=c_in(mc), **LW.FORWARD_TEST_W19)
    dev_data = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}
    with torch.no_grad():
        res = model(dev_data)
    compare_forward_test(res, ref, ic["n_max_pair"], 5e-6, slack=0, tie_tol=BF16X3_TIE.get(precision, 0.0))


POOL_FREE = r"(backbone\.branch\.[12]\.|neck\.|predictor\.)"        # tests/test_gpu_train.py


@pytest.mark.parametrize("graphs", [False, True])
def test_training_step_window_5_matches_reference_gradients(graphs, precision):
    """model.train()(batch) -> total_loss.backward() at window 5 against the reference's own training step (stochastic depth
    off), eager and with the forward / backward replayed as HIP graphs; bounds of
    tests/test_gpu_train.py::test_training_step_matches_reference_gradients[nodrop]."""
    from golden_cases import compare_grads, replay_matching, train_batch
    from vrdone_amd import train_graph
    from vrdone_amd.models.blocks import AffineDropPath
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, keys = load_case("vidvrd")
    sd = O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"])
    mc = LW.model_config(mc, "vidvrd_w5")
    model = MaskVRD(mc, device=DEV)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).train()
    with open(os.path.join(GOLDEN, "train_step_vidvrd_w5.json")) as f:
        meta = json.load(f)
    gt = LW.load_npz_parts(os.path.join(GOLDEN, "train_step_vidvrd_w5"))
    lens, _, _, data = train_batch(mc, c_in(mc), device=DEV, spec=LW.TRAIN_W5)
    assert lens == meta["lengths"]
    for mod in model.modules():
        if isinstance(mod, AffineDropPath):
            mod.drop_prob = 0.0
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
        assert abs(float(loss[k].detach()) - v) <= (1e-5 if precision == "f32" else 2e-4) * max(1.0, abs(v)), (k, float(loss[k]), v)
    assert all(len(call) <= 6 for call in differing), differing
    worst, median = compare_grads(((n, p.grad) for n, p in model.named_parameters()), gt, meta, "nodrop",
                                  rtol=3e-2, atol_frac=1e-4, median_tol=2e-5 if precision == "f32" else 5e-4, outlier_tol=1e-3,
                                  max_outliers=3, outlier_scope=None if precision != "bf16x3" else POOL_FREE)
    print(f"[w5/{precision}/graphs={graphs}] relative gradient error: worst {worst:.2e}, median {median:.2e}")
