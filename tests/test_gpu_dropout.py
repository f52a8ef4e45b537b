"""Training dropout on the GPU (`dropattn`, `dropout`): the device's keep decisions against the host mirror bit for bit, the row
kernel and the banded attention with dropout against float64 references that apply the mirror's masks, a TransformerBlock against a
float64 composite of the oracle's pieces, and a whole training step against the REAL reference's autograd through those masks
(tests/golden/train_step_vidvrd_dropout.npz + _b.npz, scripts/make_golden_dropout.py).

Tolerances are those of the tests of the same code without dropout: 2e-5 of the largest entry for the attention kernels
(tests/test_gpu_backward.py::test_local_attention_backward), 5e-5 / 5e-4 for the block (tests/test_gpu_train.py::
test_transformer_block_forward_backward_vs_oracle), and the bounds of test_training_step_matches_reference_gradients for the step.
A keep decision that differed from the mirror's would show as an error of order 1 in any of them."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import window_cases as W
from conftest import GOLDEN, load_case
from golden_cases import compare_grads, replay_matching, train_batch
from oracle import vrd_oracle as O
from vrdone_amd import dropout as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0xC0FFEE1234567890                    # (beyond 2^63: stored as a negative int64)


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


@pytest.fixture(params=["f32", "bf16x3", "f16x3"])
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def seed_tensor(seed=SEED):
    v = seed & 0xFFFFFFFFFFFFFFFF
    return torch.full((1,), v - (1 << 64) if v >> 63 else v, dtype=torch.int64, device=DEV)


def stream():
    from vrdone_amd import ops
    return ops._stream()


def ok(rc, what):
    from vrdone_amd import _hip
    _hip.check(rc, what)


def p_(t):
    return None if t is None else t.data_ptr()


def rel_close(got, want, rtol, what=""):
    """relative to the largest entry of the float64 reference (tests/test_gpu_backward.py)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    print(f"{what}: max error {err:.3e} of the largest entry")
    assert err <= rtol, f"{what}: max error {err:.3e} of the largest entry (tolerance {rtol:.1e})"


def device_mask(seed_t, site, first_id, n, p):
    from vrdone_amd import _hip
    keep = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)
    ok(_hip.lib.vrd_dropout_mask(p_(seed_t), site, first_id, n, p, p_(keep), stream()), "vrd_dropout_mask")
    assert bool((keep[n:] == 7).all()), "vrd_dropout_mask wrote behind its n decisions"
    return keep[:n]


# ------------------------------------------------------------------------------------------------------ mask and row kernel
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("first_id", [0, 2 ** 32 - 5, 2 ** 40 + 3])
def test_dropout_mask_equals_the_mirror(first_id, p):
    n, site = 4099, D.site_id("backbone.branch.1.mlp.2")          # 17 workgroups, the last one partial; unaligned first ids
    got = device_mask(seed_tensor(), site, first_id, n, p).cpu().numpy()
    assert np.array_equal(got, D.keep_mask(SEED, site, first_id, n, p))
    # another seed, another site: other decisions
    assert not np.array_equal(got, device_mask(seed_tensor(SEED ^ 1), site, first_id, n, p).cpu().numpy())
    assert not np.array_equal(got, device_mask(seed_tensor(), site ^ 1, first_id, n, p).cpu().numpy())


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("rows,C", [(70, 256), (33, 2048)])
def test_dropout_rows(rows, C, inplace):
    """vrd_dropout_rows = x * mask / (1 - p) formed by torch from the dumped mask, bit for bit, on strided windows with NaN guard
    bands and on dense rows; row0 != 0 puts the ids beyond 2^32."""
    from vrdone_amd import _hip
    p, site, row0 = 0.1, D.site_id("backbone.stem.1.attn.proj_drop"), 2 ** 24 + 3
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, C, generator=g)
    st = seed_tensor()
    mask = device_mask(st, site, row0 * C, rows * C, p)
    assert np.array_equal(mask.cpu().numpy(), D.row_mask(SEED, site, row0, rows, C, p).reshape(-1))
    scale = torch.tensor(float(D.keep_scale(p)), dtype=torch.float32, device=DEV)
    want = x.to(DEV) * (mask.view(rows, C).to(torch.float32) * scale)
    lds = W.LdSeq()
    hx = W.embed(x.to(DEV), ld=lds(C), name="x")
    if inplace:
        ok(_hip.lib.vrd_dropout_rows(p_(hx.view), hx.ld, rows, C, p_(st), site, row0, p, p_(hx.view), hx.ld, stream()), "vrd_dropout_rows")
        W.assert_guards_intact(hx)
        got = hx.view
    else:
        ho = W.embed_out((rows, C), DEV, ld=lds(C), name="out")
        ok(_hip.lib.vrd_dropout_rows(p_(hx.view), hx.ld, rows, C, p_(st), site, row0, p, p_(ho.view), ho.ld, stream()), "vrd_dropout_rows")
        W.check([ho], [hx])
        got = ho.view
    assert W.bits_equal(got, want), "window call"
    xd, plain = x.to(DEV), torch.empty(rows, C, device=DEV)
    ok(_hip.lib.vrd_dropout_rows(p_(xd), C, rows, C, p_(st), site, row0, p, p_(xd if inplace else plain), C, stream()), "vrd_dropout_rows")
    assert W.bits_equal(xd if inplace else plain, want), "dense call"


def test_dropout_function_forward_and_on_dy():
    """autograd.Dropout: the forward and, on dy, the backward are the same masked scaling -- nothing stored in between"""
    from vrdone_amd import autograd
    from vrdone_amd.models.blocks import Drop
    B, T, C, p, site, row0 = 3, 11, 256, 0.5, 12345, 77
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(B, T, C, generator=g).to(DEV).requires_grad_(True), torch.randn(B, T, C, generator=g).to(DEV)
    y = autograd.Dropout.apply(x, Drop(seed_tensor(), site, row0, p))
    y.backward(dy)
    f = torch.from_numpy(D.row_mask(SEED, site, row0, B * T, C, p).astype(np.float32) * D.keep_scale(p)).view(B, T, C).to(DEV)
    assert W.bits_equal(y.detach(), x.detach() * f) and W.bits_equal(x.grad, dy * f)


# ---------------------------------------------------------------------------------------------------------- banded attention
def banded_ref(q, k, v, m, n_head, w, rel, factor):
    """float64 dense masked-window attention (oracle.banded_attention's math) with the factors `factor` (B, T, H, 2w+1) =
    keep / (1 - p) on the probabilities behind the masked-query zeroing."""
    B, C, T = q.shape
    hd = C // n_head
    sp = lambda t: t.view(B, n_head, hd, T).transpose(2, 3)          # noqa: E731  (B, H, T, hd)
    qh, kh, vh = sp(q) * (1.0 / math.sqrt(hd)), sp(k), sp(v)
    kp = F.pad(kh, (0, 0, w, w)).unfold(2, 2 * w + 1, 1)
    vp = F.pad(vh, (0, 0, w, w)).unfold(2, 2 * w + 1, 1)
    s = torch.einsum("bhtd,bhtdw->bhtw", qh, kp)
    if rel is not None:
        s = s + rel.reshape(1, n_head, 1, 2 * w + 1)
    pos = torch.arange(T)[:, None] + torch.arange(-w, w + 1)[None, :]
    inside = (pos >= 0) & (pos < T)
    key_ok = m[:, pos.clamp(0, T - 1)]
    s = s + torch.where(key_ok, 0.0, -1e4)[:, None]
    s = s.masked_fill(~inside[None, None], float("-inf"))
    pr = torch.softmax(s, dim=-1).masked_fill(~m[:, None, :, None], 0.0)
    pr = pr * factor.permute(0, 2, 1, 3)
    out = torch.einsum("bhtw,bhtdw->bhtd", pr, vp)
    return out.transpose(2, 3).reshape(B, C, T)


def attn_factor(site, row0, B, T, n_head, window, p):
    keep = D.attn_mask(SEED, site, row0, B * T, n_head, window, p).reshape(B, T, n_head, window)
    return torch.from_numpy(keep.astype(np.float64) * float(D.keep_scale(p)))


ATTN_B, ATTN_T, ATTN_LENS = 3, 24, (24, 13, 2)


def attn_inputs(C, n_head, window, with_rel):
    g = torch.Generator().manual_seed(C + n_head + window)
    m = torch.arange(ATTN_T)[None] < torch.tensor(ATTN_LENS)[:, None]
    q, k, v, dO = (torch.randn(ATTN_B, C, ATTN_T, generator=g) for _ in range(4))
    rel = torch.randn(1, 1, n_head, window, generator=g) if with_rel else None
    return m, q, k, v, dO, rel


def cl(x):
    return x.transpose(1, 2).contiguous()


@pytest.mark.parametrize("with_rel", [False, True])
@pytest.mark.parametrize("window", [3, 7, 9, 11, 19])
@pytest.mark.parametrize("C,n_head", [(512, 4), (512, 16), (256, 8), (256, 2)])
def test_local_attention_dropout(C, n_head, window, with_rel):
    """Forward, dq / dk / dv / d rel_pe of ops.local_attention(drop=...) against float64 autograd of the dense reference with the
    mirror's mask.  p = 0.1 without the bias, 0.5 with it; the call's first row is number 1000 of its site."""
    from vrdone_amd import ops
    from vrdone_amd.models.blocks import Drop
    hw, p, row0 = window // 2, 0.5 if with_rel else 0.1, 1000
    site = D.site_id("backbone.stem.0.attn.attn_drop")
    m, q, k, v, dO, rel = attn_inputs(C, n_head, window, with_rel)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    relr = rel.double().requires_grad_(True) if with_rel else None
    outr = banded_ref(qr, kr, vr, m, n_head, hw, relr, attn_factor(site, row0, ATTN_B, ATTN_T, n_head, window, p))
    outr.backward(dO.double())
    qd, kd, vd = (cl(t).to(DEV).requires_grad_(True) for t in (q, k, v))
    reld = rel.to(DEV).requires_grad_(True) if with_rel else None
    out = ops.local_attention(qd, kd, vd, m.to(DEV), n_head, hw, rel_pe=reld, drop=Drop(seed_tensor(), site, row0, p))
    out.backward(cl(dO).to(DEV))
    rel_close(out, cl(outr), 2e-5, "out")
    for name, a, r in (("dq", qd.grad, qr.grad), ("dk", kd.grad, kr.grad), ("dv", vd.grad, vr.grad)):
        rel_close(a, cl(r), 2e-5, name)
    if with_rel:
        rel_close(reld.grad, relr.grad, 2e-5, "d rel_pe")
    md = m.to(DEV)
    for name, t in (("out", out.detach()), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert bool((t[~md] == 0).all()), f"{name}: rows of masked queries / keys must be exactly zero"
    # (and dropout did act: the result differs from the p = 0 attention)
    with torch.no_grad():
        plain = ops.local_attention(qd.detach(), kd.detach(), vd.detach(), md, n_head, hw, rel_pe=None if reld is None else reld.detach())
    assert float((plain - out.detach()).abs().max()) > 1e-2


@pytest.mark.parametrize("C,n_head,window,with_rel", [(512, 4, 7, False), (512, 16, 19, True), (256, 8, 11, True), (256, 2, 9, False)])
def test_rate_zero_through_the_new_entry_points_is_the_existing_attention(C, n_head, window, with_rel):
    """vrd_local_attn_drop / _drop_bwd at p = 0 against vrd_local_attn / vrd_local_attn_bwd: the same bits in every output and in
    the scratch (P | dS)."""
    from vrdone_amd import _hip
    hw = window // 2
    m, q, k, v, dO, rel = attn_inputs(C, n_head, window, with_rel)
    md, qd, kd, vd, dOd = m.to(DEV).contiguous(), cl(q).to(DEV), cl(k).to(DEV), cl(v).to(DEV), cl(dO).to(DEV)
    reld = rel.to(DEV).contiguous() if with_rel else None
    B, T = ATTN_B, ATTN_T
    st = seed_tensor()
    outs = []
    for drop in (False, True):
        out, dq, dk, dv = (torch.full((B, T, C), float("nan"), device=DEV) for _ in range(4))
        scratch = torch.full((2 * B * T * n_head * window,), float("nan"), device=DEV)
        if drop:
            ok(_hip.lib.vrd_local_attn_drop(p_(qd), p_(kd), p_(vd), C, p_(md), p_(reld), B, T, C, n_head, hw, p_(st), 99, 5, 0.0, p_(out), C,
                                            stream()), "vrd_local_attn_drop")
            ok(_hip.lib.vrd_local_attn_drop_bwd(p_(qd), p_(kd), p_(vd), C, p_(dOd), C, p_(md), p_(reld), B, T, C, n_head, hw, p_(st), 99, 5, 0.0,
                                                p_(dq), p_(dk), p_(dv), C, p_(scratch), stream()), "vrd_local_attn_drop_bwd")
        else:
            ok(_hip.lib.vrd_local_attn(p_(qd), p_(kd), p_(vd), C, p_(md), p_(reld), B, T, C, n_head, hw, p_(out), C, 0, stream()), "vrd_local_attn")
            ok(_hip.lib.vrd_local_attn_bwd(p_(qd), p_(kd), p_(vd), C, p_(dOd), C, p_(md), p_(reld), B, T, C, n_head, hw, p_(dq), p_(dk), p_(dv), C,
                                           p_(scratch), stream()), "vrd_local_attn_bwd")
        outs.append((out, dq, dk, dv, scratch))
    for name, a, b in zip(("out", "dq", "dk", "dv", "scratch"), *outs):
        assert bool(torch.isfinite(a).all()) and W.bits_equal(a, b), name


# --------------------------------------------------------------------------------------------------------- TransformerBlock
def block_ref(sd, pre, x, mask, n_head, win, stride, factors, path):
    """oracle.transformer_block's composition in training form: the four dropout sites as factors (f64 tensors in the reference's
    layouts: att (B, T', H, 2w+1), rows (B, C, T')) and stochastic depth as per-sample factors `path` (B,)."""
    h = O.channel_ln(x, sd[f"{pre}.ln1.weight"], sd[f"{pre}.ln1.bias"])
    ap = f"{pre}.attn"
    q, qm = O._qkv_branch(sd, ap, "query", h, mask, stride)
    k, km = O._qkv_branch(sd, ap, "key", h, mask, stride)
    v, _ = O._qkv_branch(sd, ap, "value", h, mask, stride)
    if win > 1:
        o = banded_ref(q, k, v, km[:, 0], n_head, win // 2, sd.get(f"{ap}.rel_pe"), factors["attn.attn_drop"])
    else:
        o = O.full_attention(q, k, v, km, n_head)
    o = F.conv1d(o, sd[f"{ap}.proj.weight"], sd[f"{ap}.proj.bias"]) * factors["attn.proj_drop"] * qm.to(x.dtype)
    mf = qm.to(x.dtype)
    skip = x if stride == 1 else F.max_pool1d(x, stride + 1, stride, (stride + 1) // 2)
    y = skip * mf + sd[f"{pre}.drop_path_attn.scale"] * o * path[:, None, None]
    h = O.channel_ln(y, sd[f"{pre}.ln2.weight"], sd[f"{pre}.ln2.bias"])
    h = F.gelu(F.conv1d(h, sd[f"{pre}.mlp.0.weight"], sd[f"{pre}.mlp.0.bias"])) * factors["mlp.2"]
    h = F.conv1d(h, sd[f"{pre}.mlp.3.weight"], sd[f"{pre}.mlp.3.bias"]) * factors["mlp.4"]
    return y + sd[f"{pre}.drop_path_mlp.scale"] * (h * mf) * path[:, None, None], qm


def block_factors(pre, sample0, B, Tq, C, n_head, win, p_attn, p_proj):
    def rows(name, width):
        keep = D.row_mask(SEED, D.site_id(f"{pre}.{name}"), sample0 * Tq, B * Tq, width, p_proj).reshape(B, Tq, width)
        return torch.from_numpy(keep.astype(np.float64) * float(D.keep_scale(p_proj))).transpose(1, 2)
    f = {"attn.proj_drop": rows("attn.proj_drop", C), "mlp.2": rows("mlp.2", 4 * C), "mlp.4": rows("mlp.4", C)}
    if win > 1:
        keep = D.attn_mask(SEED, D.site_id(f"{pre}.attn.attn_drop"), sample0 * Tq, B * Tq, n_head, win, p_attn).reshape(B, Tq, n_head, win)
        f["attn.attn_drop"] = torch.from_numpy(keep.astype(np.float64) * float(D.keep_scale(p_attn)))
    return f


def rel_l2(got, want, floor=0.0):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    return float((got - want).norm()) / (float(want.norm()) + floor + 1e-12)


@pytest.mark.parametrize("stride,win", [(1, 7), (2, 7), (2, -1)])
def test_transformer_block_with_dropout_vs_float64(stride, win, precision):
    """One TransformerBlock in training mode, forward and backward, with all its dropout sites at 0.1 (window 7: four sites;
    window -1, global attention: proj_drop and the two MLP sites) and pinned stochastic depth, TWICE in one step -- the second call
    continues the first one's rows -- against float64 autograd of the oracle's pieces with the mirror's masks applied."""
    from vrdone_amd.models import blocks
    torch.manual_seed(0)
    C, H, B, T = 512, 4, 3, 48
    p_attn = 0.1 if win > 1 else 0.0
    blk = blocks.TransformerBlock(C, H, n_ds_strides=(stride, stride), attn_pdrop=p_attn, proj_pdrop=0.1, path_pdrop=0.1, mha_win_size=win)
    keys = [(f"blk.{k}", list(v.shape)) for k, v in blk.state_dict().items()]
    sd = O.synth_state_dict(keys)
    blk.load_state_dict({k[4:]: v for k, v in sd.items()})
    blk = blk.to(DEV).train()
    blk.set_dropout_names("blk")
    keep = torch.tensor([1.0, 0.0, 1.0])
    blk.drop_path_attn.keep = blk.drop_path_mlp.keep = keep
    lens = torch.tensor([48, 31, 6])
    m = (torch.arange(T)[None] < lens[:, None])[:, None]
    g = torch.Generator().manual_seed(1)
    tol = 5e-5 if precision == "f32" else 5e-4
    blocks.begin_dropout_step(blk, DEV, seed=SEED)
    for call in range(2):
        x = torch.randn(B, C, T, generator=g) * m
        dy = torch.randn(B, C, T // stride, generator=g)
        sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        x64 = x.double().requires_grad_(True)
        factors = block_factors("blk", call * B, B, T // stride, C, H, win, p_attn, 0.1)
        yr, _ = block_ref(sd64, "blk", x64, m, H, win, stride, factors, keep.double() / 0.9)
        yr.backward(dy.double())
        blk.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        y, _ = blk(xd, m.to(DEV))
        y.backward(dy.to(DEV))
        assert blk._drop_samples == (call + 1) * B and blk.attn._drop_samples == (call + 1) * B
        errs = {"y": rel_l2(y, yr), "dx": rel_l2(xd.grad, x64.grad)}
        floor = 1e-3 * max(float(v.grad.norm()) for v in sd64.values())
        for name, prm in blk.named_parameters():
            assert prm.grad is not None, name
            errs[name] = rel_l2(prm.grad, sd64["blk." + name].grad, floor)
        print(f"[stride {stride}, window {win}, {precision}, call {call}] worst {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
        assert max(errs.values()) < tol, {k: v for k, v in errs.items() if v >= tol}
    # eval: the same module without any dropout -- the p = 0 block's bits
    plain = blocks.TransformerBlock(C, H, n_ds_strides=(stride, stride), path_pdrop=0.1, mha_win_size=win)
    plain.load_state_dict(blk.state_dict())
    plain, blk = plain.to(DEV).eval(), blk.eval()
    with torch.no_grad():
        a, b = blk(x.to(DEV), m.to(DEV))[0], plain(x.to(DEV), m.to(DEV))[0]
    assert W.bits_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ the fixture step
def c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


def fixture():
    a, b = (np.load(os.path.join(GOLDEN, f)) for f in ("train_step_vidvrd_dropout.npz", "train_step_vidvrd_dropout_b.npz"))
    arrs = {k: z[k] for z in (a, b) for k in z.files}
    return arrs, json.loads(str(arrs["meta"]))


def build(meta=None, rates=None, pin=True):
    """the vidvrd model on synthetic weights; meta: the fixture's rates, pinned stochastic depth and (pin) its seed"""
    from vrdone_amd.models.blocks import AffineDropPath
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, ic, keys = load_case("vidvrd")
    sd = O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"])
    if meta is not None:
        rates = (meta["dropattn"], meta["dropout"])
    if rates is not None:
        mc = dict(mc, dropattn=rates[0], dropout=rates[1])
    model = MaskVRD(mc, device=DEV)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).train()
    if meta is not None:
        for name, mod in model.named_modules():
            if isinstance(mod, AffineDropPath):
                mod.keep = torch.tensor(meta["keep"][name], dtype=torch.float32, device=DEV)       # (on the device: read inside a recording)
        if pin:
            model.dropout_seed = meta["seed"]
    return model, mc, ic


def step(model, data):
    model.zero_grad(set_to_none=True)
    loss = model(data)
    loss["total_loss"].backward()
    return {k: float(v.detach()) for k, v in loss.items()}, {k: p.grad.detach().clone() for k, p in model.named_parameters()}


POOL_FREE = r"(backbone\.branch\.[12]\.|neck\.|predictor\.)"          # tests/test_gpu_train.py: why the outlier count is scoped


def test_training_step_with_dropout_matches_reference_gradients(precision):
    """The fixture step -- the reference's forward_training + autograd with the mirror's masks in place of its nn.Dropout draws --
    eager and as HIP graphs (recording step, then a pure replay), at the bounds of test_training_step_matches_reference_gradients;
    with the seed pinned a replay equals the eager step (bounds of test_training_graphs_take_the_same_steps)."""
    from vrdone_amd import train_graph
    arrs, meta = fixture()
    model, mc, _ = build(meta)
    lens, _, _, data = train_batch(mc, c_in(mc), device=DEV)
    assert lens == meta["lengths"]
    want = meta["cases"]["dropout"]["losses"]
    results = {}
    try:
        for how in ("eager", "recorded", "replayed"):
            model.enable_training_graphs(how != "eager")
            differing = replay_matching(model, meta["cases"]["dropout"]["indices"])
            loss, grads = step(model, data)
            del model.bipartite_match
            assert set(loss) == set(want)
            for k, v in want.items():
                assert abs(loss[k] - v) <= (1e-5 if precision == "f32" else 2e-4) * max(1.0, abs(v)), (how, k, loss[k], v)
            assert all(len(call) <= 6 for call in differing), differing
            worst, median = compare_grads(grads.items(), arrs, meta, "dropout", rtol=3e-2, atol_frac=1e-4,
                                          median_tol=2e-5 if precision == "f32" else 5e-4, outlier_tol=1e-3, max_outliers=3,
                                          outlier_scope=POOL_FREE)
            print(f"[dropout/{precision}/{how}] total_loss {loss['total_loss']:.6f} (reference {want['total_loss']:.6f}); relative "
                  f"gradient error: worst {worst:.2e}, median {median:.2e}")
            results[how] = (loss, grads)
        assert len(train_graph.recordings(model)) == 1
        (le, ge), (lr, gr) = results["eager"], results["replayed"]
        assert abs(le["total_loss"] - lr["total_loss"]) <= 2e-5 * abs(le["total_loss"])
        floor = 1e-6 * max(float(g.abs().max()) for g in ge.values())
        for k, g in ge.items():
            assert float((gr[k] - g).abs().max()) <= 2e-4 * float(g.abs().max()) + floor, k
        # the pinned seed is part of the recording's key: another value records anew
        model.dropout_seed = meta["seed"] + 1
        other, _ = step(model, data)
        assert len(train_graph.recordings(model)) == 2 and other["total_loss"] != lr["total_loss"]
    finally:
        train_graph.forget(model)


def test_free_seed_gives_every_replay_its_own_masks():
    from vrdone_amd import train_graph
    _, meta = fixture()
    model, mc, _ = build(meta, pin=False)
    _, _, _, data = train_batch(mc, c_in(mc), device=DEV)
    model.enable_training_graphs(True)
    try:
        losses = [step(model, data)[0]["total_loss"] for _ in range(3)]           # the recording step, then two pure replays
        assert len(train_graph.recordings(model)) == 1
        assert losses[1] != losses[2] and all(np.isfinite(losses)), losses
        model.enable_training_graphs(False)
        eager = [step(model, data)[0]["total_loss"] for _ in range(2)]
        assert eager[0] != eager[1]
    finally:
        train_graph.forget(model)


def test_deterministic_mode_repeats_a_seeded_step_bit_for_bit():
    """Same torch.manual_seed -> the same step seed, the same stochastic depth, the same bits; eager and as a replay."""
    from vrdone_amd import ops, train_graph
    from vrdone_amd.models.blocks import AffineDropPath
    _, meta = fixture()
    model, mc, _ = build(rates=(0.1, 0.1))
    assert all(mod.keep is None for mod in model.modules() if isinstance(mod, AffineDropPath)) and model.dropout_seed is None
    _, _, _, data = train_batch(mc, c_in(mc), device=DEV)
    try:
        with ops.use_deterministic(True):
            for graphs in (False, True):
                model.enable_training_graphs(graphs)
                runs = []
                for seed in (5, 5, 6):
                    torch.manual_seed(seed)
                    runs.append(step(model, data))
                (la, ga), (lb, gb), (lc, _) = runs
                assert la == lb and la["total_loss"] != lc["total_loss"], (graphs, la, lb, lc)
                for k in ga:
                    assert W.bits_equal(ga[k], gb[k]), (graphs, k)
    finally:
        train_graph.forget(model)


def test_eval_of_the_dropout_model_is_the_rate_zero_model():
    """model.eval(): forward_test of the model built with both keys at 0.1 equals the p = 0 model with the same weights, bit for
    bit; so does a validation pass under no_grad in training mode (dropout acts only when training AND autograd records)."""
    from oracle.synth import synth_proposal
    drop, mc, ic = build(rates=(0.1, 0.1))
    plain, _, _ = build()
    data = synth_proposal(4, c_in(mc), 20, 60, seed=99)
    dev = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}
    res = []
    for model in (drop, plain):
        model.eval()
        model._config_eval(ic)
        with torch.no_grad():
            res.append(model(dev))

    def same(a, b, path="result"):
        assert type(a) is type(b), path
        if isinstance(a, dict):
            assert a.keys() == b.keys(), path
            for k in a:
                same(a[k], b[k], f"{path}[{k!r}]")
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), path
            for i, (u, v) in enumerate(zip(a, b)):
                same(u, v, f"{path}[{i}]")
        elif torch.is_tensor(a):
            assert a.dtype == b.dtype and (W.bits_equal(a, b) if a.dtype == torch.float32 else torch.equal(a, b)), path
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b), path
        else:
            assert a == b, path
    assert res[0] is not None
    same(res[0], res[1])
    _, _, _, batch = train_batch(mc, c_in(mc), device=DEV)
    vals = []
    for model in (drop, plain):
        model.train()
        with torch.no_grad():
            vals.append({k: float(v) for k, v in model(batch).items()})
    assert vals[0] == vals[1]
