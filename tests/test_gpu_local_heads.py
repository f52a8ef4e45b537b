"""Banded attention at width 256 (8, 4, 2 heads: head_dim 32, 64, 128) and at width 512 with 16 heads (head_dim 32) on the
MI355X: vrd_local_attn / _segs / _bwd and the modules above them against goldens of the real reference at windows 5, 11 and
19 (scripts/make_golden_heads.py, cases in tests/local_heads_cases.py) and against the float64 oracle at every odd window
from 3 to 19.

Width 512 with 16 heads runs the whole-row strip kernel at windows 3 .. 9 (4 lanes a head) and the half-row one at 11 .. 19
(8 lanes a head): goldens at 5 | 11, 19 hold both forms.  Width 256 runs one kernel at every window (four channels a lane, one
wave per strip; 8, 16 or 32 lanes a head).  The sequences are those of tests/test_gpu_local_window.py: two full strips of 16
rows and a partial one, a sequence of half a window, a fully masked sequence.  Tolerances are that file's, which are those of
the existing tests of the same op and mode: the banded kernels compute in f32 on the vector units in every precision mode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import local_heads_cases as LH
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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
    with np.load(os.path.join(GOLDEN, "local_heads.npz")) as z:
        return {k: z[k] for k in z.files}


def cl(x):          # (B, C, T) -> (B, T, C)
    return x.transpose(1, 2).contiguous()


def sub(t):
    """(B, T, C) on the device -> the stored (B, C / 17, T) sample"""
    return t.detach().float().cpu().transpose(1, 2)[:, ::LH.CH_STRIDE].numpy()


def close(got, want, atol):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().double().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= atol, f"max error {err:.3e} (tolerance {atol:.1e})"


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


_oracle = {}


def oracle_core(C, H, W, rel):
    """float64 oracle of a core case, computed once: out, dq, dk, dv (B, T, C) and d rel_pe."""
    key = (C, H, W, rel)
    if key not in _oracle:
        q, k, v, dO, rel_pe = LH.core_inputs(C, H, W, rel)
        leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
        bias = rel_pe.double().requires_grad_(True) if rel else None
        with torch.enable_grad():
            out = O.banded_attention(*leaves, LH.mask(W), H, W // 2, rel_pe=bias)
            out.backward(dO.double())
        _oracle[key] = tuple(cl(t.detach()) for t in (out, *(l.grad for l in leaves))) + (bias.grad if rel else None,)
    return _oracle[key]


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("C,H,W,rel", LH.ALL_OP_CASES)
def test_forward_plain_pair_and_row_groups(g, C, H, W, rel, precision):
    """ops.local_attention on the core cases: f32 rows against the float64 oracle (every channel) and the reference's stored
    output (windows 5, 11, 19); masked query rows are exact zeros; pair rows decode to the f32 rows within the format's
    error; the same sequences and a second group of another length as ONE row-group launch give the bits of the launches per
    group."""
    from vrdone_amd import ops
    q, k, v, _, rel_pe = LH.core_inputs(C, H, W, rel)
    T, hw = LH.seq_len(W), W // 2
    qd, kd, vd = (cl(t).to(DEV) for t in (q, k, v))
    m = LH.mask(W)[:, 0].to(DEV)
    reld = rel_pe.to(DEV) if rel else None
    with torch.no_grad():
        got = ops.local_attention(qd, kd, vd, m, H, hw, rel_pe=reld)
        close(got, oracle_core(C, H, W, rel)[0], 2e-5)
        if W in LH.REF_WINDOWS:
            close(sub(got), g[f"core/{LH.tag(C, H, W, rel)}/out"], 2e-5)
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


def odd_shape_cases(W, C, H, gen):
    """(q, k, v, mask, bias) of shapes the goldens do not have: T = 50 (three strips and 2 rows; B = 5: 15 strips, which leave
    the last workgroup of four waves partly empty) with holes in the validity, a strip that is all padding inside a live
    sequence, one valid frame at the very end and a fully masked sequence; sequences of half a window; a single frame."""
    for B, T in ((5, 50), (3, W // 2), (2, 1)):
        q, k, v = (torch.randn(B, T, C, generator=gen) for _ in range(3))
        mask = torch.rand(B, T, generator=gen) > 0.3
        if T == 50:
            mask[1, 16:32] = False
            mask[2] = False
            mask[2, 49] = True
            mask[3] = False
        rel = torch.randn(1, 1, H, W, generator=gen)
        for bias in (None, rel):
            yield q, k, v, mask, bias


def check_against_oracle(q, k, v, mask, bias, H, W):
    from vrdone_amd import ops
    want = O.banded_attention(q.transpose(1, 2).double(), k.transpose(1, 2).double(), v.transpose(1, 2).double(),
                              mask[:, None], H, W // 2, rel_pe=None if bias is None else bias.double()).transpose(1, 2)
    got = ops.local_attention(q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, W // 2, rel_pe=None if bias is None else bias.to(DEV))
    close(got, want, 2e-5)


@pytest.mark.parametrize("C,H", LH.SHAPES)
@pytest.mark.parametrize("W", [3, 9, 13, 19])
def test_forward_odd_shapes_against_oracle(C, H, W):
    gen = torch.Generator().manual_seed(1000 * W + C + H)
    with torch.no_grad():
        for case in odd_shape_cases(W, C, H, gen):
            check_against_oracle(*case, H, W)


@pytest.mark.parametrize("width,n_head", [(384, 6), (512, 3), (256, 16)])
def test_argument_errors(width, n_head):
    from vrdone_amd import ops
    q = torch.zeros(1, 16, width, device=DEV)
    with pytest.raises(ValueError, match="width 256 or 512"):
        ops.local_attention(q, q, q, torch.ones(1, 16, dtype=torch.bool, device=DEV), n_head, 2)


def test_library_names_the_envelope():
    """The C entry points' own check (callers that do not go through ops): the error text names the accepted set and the values."""
    from vrdone_amd import _hip
    q = torch.zeros(1, 16, 384, device=DEV)
    m = torch.ones(1, 16, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(q)
    rc = _hip.lib.vrd_local_attn(q.data_ptr(), q.data_ptr(), q.data_ptr(), 384, m.data_ptr(), None, 1, 16, 384, 6, 2, out.data_ptr(), 384, 0,
                                 torch.cuda.current_stream().cuda_stream)
    with pytest.raises(Exception, match=r"C = 256 or 512 .*32, 64 or 128 .*C = 384, n_head = 6"):
        _hip.check(rc, "vrd_local_attn")
    scratch = torch.empty(2 * 16 * 6 * 5, device=DEV)
    rc = _hip.lib.vrd_local_attn_bwd(q.data_ptr(), q.data_ptr(), q.data_ptr(), 384, q.data_ptr(), 384, m.data_ptr(), None, 1, 16, 384, 6, 2,
                                     out.data_ptr(), out.data_ptr(), out.data_ptr(), 384, scratch.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    with pytest.raises(Exception, match=r"C = 256 or 512 .*32, 64 or 128 .*C = 384, n_head = 6"):
        _hip.check(rc, "vrd_local_attn_bwd")


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("C,H,W,rel", LH.ALL_OP_CASES)
def test_backward(g, C, H, W, rel):
    """autograd.LocalAttention: dq, dk, dv and d rel_pe against float64 autograd of the oracle (every element) and against the
    reference's stored gradients; in deterministic mode two runs give the same bits."""
    from vrdone_amd import ops
    q, k, v, dO, rel_pe = LH.core_inputs(C, H, W, rel)
    m = LH.mask(W)[:, 0].to(DEV)
    want = oracle_core(C, H, W, rel)
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
        if W in LH.REF_WINDOWS:
            p = f"core/{LH.tag(C, H, W, rel)}/"
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


def seeded(mod, pre):
    sd = O.synth_state_dict([(f"{pre}.{k}", tuple(t.shape)) for k, t in mod.state_dict().items()])
    mod.load_state_dict({k[len(pre) + 1:]: t for k, t in sd.items()}, strict=True)
    return mod.to(DEV).eval()


@pytest.mark.parametrize("C,H,W,rel", LH.MHCA_CASES)
def test_local_mhca_module_forward_backward(g, C, H, W, rel, precision):
    """blocks.LocalMaskedMHCA with the reference's weights: output, input gradient and every parameter's gradient (projection
    weights, rel_pe) against the reference's; bounds of tests/test_gpu_train.py's module tests (5e-5 in f32, 5e-4 in the split modes)."""
    from vrdone_amd.models.blocks import LocalMaskedMHCA
    x, dy = LH.mhca_inputs(C, H, W, rel)
    mod = seeded(LocalMaskedMHCA(C, H, window_size=W, use_rel_pe=rel), LH.mhca_prefix(C, H, W, rel))
    xd = x.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        out, _ = mod(xd, LH.mask(W).to(DEV))
    out.backward(dy.to(DEV))
    tol = 5e-5 if precision == "f32" else 5e-4
    p = f"mhca/{LH.tag(C, H, W, rel)}/"
    pick = lambda t: t.detach().cpu()[:, ::LH.CH_STRIDE]      # noqa: E731
    e_out, e_dx = _rel(pick(out), g[p + "out"]), _rel(pick(xd.grad), g[p + "dx"])
    print(f"[mhca {LH.tag(C, H, W, rel)}/{precision}] out {e_out:.2e} dx {e_dx:.2e}")
    assert e_out < tol and e_dx < tol
    names = [n for n, _ in mod.named_parameters()]
    assert ("rel_pe" in names) == rel
    floor = 1e-3 * max(float(g[p + "norm/" + n]) for n in names)
    for n, prm in mod.named_parameters():
        assert prm.grad is not None, n
        assert _rel(LH.sample(prm.grad).cpu(), g[p + "d/" + n], floor) < tol, n


def test_sos_local_decoder_layer_forward_backward(g, precision):
    """local_transformer.LocalMaskedMHCA_QKV inside the vidor_local decoder layer at width 256 with 8 heads."""
    from vrdone_amd.models.local_transformer import MaskedConvTransformerDecoderLayer
    s = LH.SOS_CASE
    x, y, dy, m = LH.sos_inputs()
    layer = seeded(MaskedConvTransformerDecoderLayer(s["C"], s["H"], path_pdrop=0.1, n_qx_stride=1, n_kv_stride=1, with_ffn=False,
                                                     use_local=True, win_size=s["W"]), LH.SOS_PREFIX)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        out, _ = layer(xd, yd, m.to(DEV), m.to(DEV))
    out.backward(dy.to(DEV))
    tol = 5e-5 if precision == "f32" else 5e-4
    pick = lambda t: t.detach().cpu()[:, ::LH.CH_STRIDE]      # noqa: E731
    assert _rel(pick(out), g["sos/out"]) < tol
    assert _rel(pick(xd.grad), g["sos/dx"]) < tol and _rel(pick(yd.grad), g["sos/dy"]) < tol


# ------------------------------------------------------------------------------------------------------ f16 range flag
def range_case(Cw, n_head, half_win, segs, b, c):
    """tests/test_gpu_f16_range.py's _local_case at width Cw: v is constant along t in channel c of one sequence, so every output
    row of that sequence is value * sum(p) = value (1 +- 1.3e-6)"""
    from test_gpu_f16_range import rnd
    from vrdone_amd import ops
    if segs:
        shape, rows = (1, 88, Cw), slice(48, 88)                     # [(0, 2, 24), (48, 1, 40)]: the last group
    else:
        shape, rows = (3, 40, Cw), None                              # strips of 16 rows: the third of a sequence is partial
    q, k = rnd(*shape, seed=1, scale=0.5), rnd(*shape, seed=2, scale=0.5)
    mask = torch.ones(shape[:2], dtype=torch.bool, device=DEV)

    def run(value):
        v = torch.zeros(*shape, device=DEV)
        want = torch.zeros(*shape, device=DEV, dtype=torch.float64)
        if segs:
            v[0, rows, c] = value
            want[0, rows, c] = value
        else:
            v[b, :, c] = value
            want[b, :, c] = value
        return ops.local_attention(q, k, v, mask, n_head, half_win, pair=True, segs=[(0, 2, 24), (48, 1, 40)] if segs else None), want
    return run


@pytest.mark.parametrize("Cw,n_head", [(256, 8), (512, 16)])
@pytest.mark.parametrize("half_win", [4, 9])
@pytest.mark.parametrize("segs,b,last", [(False, 2, True), (True, 0, False)])
def test_f16_range_flag(Cw, n_head, half_win, segs, b, last):
    """The new pair-row instantiations as producers of f16 planes (tests/test_gpu_f16_range.py, tag 32): an output beyond the f16
    operand range sets the flag, in-range values and the other modes do not.  Windows 9 and 19: at width 512 the whole-row and
    the half-row kernel.  The value sits in the last channel of the row (batch form: the last lane, and the consumer GEMM sees
    it) or in channel Cw / 2 + 3 (row groups).  A row's probabilities sum to 1 within (W + 2) roundings of 2^-24 = 1.3e-6 at
    W = 19: inside that file's bound of 2e-6."""
    from test_gpu_f16_range import ABIG, AOK, LOCAL_REL, check_producer
    from vrdone_amd import ops
    c = Cw - 1 if last else Cw // 2 + 3
    old = ops.get_precision()
    try:
        with torch.no_grad():
            ops.f16_range_flag().zero_()
            check_producer(range_case(Cw, n_head, half_win, segs, b, c), 32, big=ABIG, ok=AOK, rel=LOCAL_REL, consumer=last)
    finally:
        ops.f16_range_flag().zero_()
        ops.set_precision(old)


def _per_row_child():
    """runs in a fresh process with VRD_LOCAL_STRIP=0 (the library reads the switch once): the one-wave-per-row kernel at the new
    shapes, against the oracle (window 9 and 19, odd shapes included) and as a producer of f16 planes"""
    assert os.environ.get("VRD_LOCAL_STRIP") == "0" and "vrdone_amd" not in sys.modules
    from test_gpu_f16_range import ABIG, AOK, LOCAL_REL, check_producer
    from vrdone_amd import ops
    with torch.no_grad():
        for C, H in LH.SHAPES:
            for W in (9, 19):
                gen = torch.Generator().manual_seed(W + C + H)
                for case in odd_shape_cases(W, C, H, gen):
                    check_against_oracle(*case, H, W)
        ops.set_precision("f16x3")
        for Cw, n_head in ((256, 8), (512, 16)):
            check_producer(range_case(Cw, n_head, 4, False, 2, Cw - 1), 32, big=ABIG, ok=AOK, rel=LOCAL_REL, consumer=True)
    print("per-row kernel: ok")


def test_per_row_kernel_at_the_new_shapes():
    """The per-row banded kernel runs only under VRD_LOCAL_STRIP=0, which the library reads once per process: a child process
    (as tests/test_gpu_f16_range.py::test_local_attention_per_row_kernel)."""
    env = dict(os.environ, VRD_LOCAL_STRIP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "per-row"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "per-row kernel: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# --------------------------------------------------------------------------------------------------------------- model
_models = {}


def build_model(case, train=False):
    from conftest import load_case
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, ic, _ = load_case(LH.MODEL_CASES[case]["base"])
    mc = LH.model_config(mc, case)
    model = MaskVRD(mc, device=DEV)
    keys = [(k, list(v.shape)) for k, v in model.state_dict().items()]       # (held to the reference's list by test_local_heads_cpu)
    model.load_state_dict(O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]), strict=True)
    model = model.to(DEV)
    return (model.train() if train else model.eval()), mc, ic


def get_model(case):
    if case not in _models:
        model, mc, ic = build_model(case)
        model._config_eval(ic)
        _models[case] = (model, mc, ic)
    return _models[case]


@pytest.mark.parametrize("case", list(LH.MODEL_CASES))
def test_mask_vrd_matches_reference_golden(case, precision):
    """_mask_vrd with tight padding on (the row-space path: row-group launches of the banded kernels) against the reference at
    its own padded length."""
    model, mc, _ = get_model(case)
    spec = LH.MODEL_CASES[case]
    gm = np.load(os.path.join(GOLDEN, "local_heads_model.npz"))
    x, m = O.synth_pairs(len(spec["lens"]), c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
    assert model.tight_padding and any(model.tight_len(L, spec["T"]) < spec["T"] for L in spec["lens"])
    with torch.no_grad():
        out = model._mask_vrd(x.to(DEV), m.to(DEV), with_aux=False)
    dl = float((out["pred_logits"].cpu() - torch.as_tensor(gm[f"{case}/pred_logits"])).abs().max())
    dm = float((out["pred_masks"].cpu() - torch.as_tensor(gm[f"{case}/pred_masks"])).abs().max())
    print(f"[{case}/{precision}] max |dlogits| {dl:.2e}, max |dmasks| {dm:.2e}")
    close(out["pred_logits"], gm[f"{case}/pred_logits"], LOGIT_TOL)
    close(out["pred_masks"], gm[f"{case}/pred_masks"], MASK_TOL)


BF16X3_TIE = {"bf16x3": 5e-6}       # tests/test_gpu_model.py


def test_forward_test_width_256_matches_reference_golden(precision):
    """forward_test records of vidvrd at width 256, with the settings of the window-19 test."""
    from golden_cases import compare_forward_test
    model, mc, ic = get_model("vidvrd_c256")
    with open(os.path.join(GOLDEN, "forward_test_vidvrd_c256.json")) as f:
        ref = json.load(f)
    data = synth_proposal(c_in=c_in(mc), **LH.FORWARD_TEST_C256)
    dev_data = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}
    with torch.no_grad():
        res = model(dev_data)
    compare_forward_test(res, ref, ic["n_max_pair"], 5e-6, slack=0, tie_tol=BF16X3_TIE.get(precision, 0.0))


POOL_FREE = r"(backbone\.branch\.[12]\.|neck\.|predictor\.)"        # tests/test_gpu_train.py


@pytest.mark.parametrize("graphs", [False, True])
def test_training_step_width_256_matches_reference_gradients(graphs, precision):
    """model.train()(batch) -> total_loss.backward() of vidvrd at width 256 against the reference's own training step (stochastic
    depth off, the reference's matching replayed), eager and with the forward / backward replayed as HIP graphs; the bounds of
    tests/test_gpu_local_window.py::test_training_step_window_5_matches_reference_gradients."""
    from golden_cases import compare_grads, replay_matching, train_batch
    from vrdone_amd import train_graph
    from vrdone_amd.models.blocks import AffineDropPath
    model, mc, _ = build_model("vidvrd_c256", train=True)
    with open(os.path.join(GOLDEN, "train_step_vidvrd_c256.json")) as f:
        meta = json.load(f)
    gt = LH.load_npz_parts(os.path.join(GOLDEN, "train_step_vidvrd_c256"))
    lens, _, _, data = train_batch(mc, c_in(mc), device=DEV, spec=LH.TRAIN_C256)
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
        print(f"[c256/{precision}/graphs={graphs}] {k}: {float(loss[k].detach()):.7f} (reference {v:.7f})")
    for k, v in want.items():
        assert abs(float(loss[k].detach()) - v) <= (1e-5 if precision == "f32" else 2e-4) * max(1.0, abs(v)), (k, float(loss[k]), v)
    assert all(len(call) <= 6 for call in differing), differing
    worst, median = compare_grads(((n, p.grad) for n, p in model.named_parameters()), gt, meta, "nodrop",
                                  rtol=3e-2, atol_frac=1e-4, median_tol=2e-5 if precision == "f32" else 5e-4, outlier_tol=1e-3,
                                  max_outliers=3, outlier_scope=None if precision != "bf16x3" else POOL_FREE)
    print(f"[c256/{precision}/graphs={graphs}] relative gradient error: worst {worst:.2e}, median {median:.2e}")


if __name__ == "__main__" and sys.argv[1:] == ["per-row"]:
    _per_row_child()
