"""The f16x1 precision mode on the MI355X: the one-product split GEMM kernels (256 x 256, 128 x 256, 128 x 128) and flash
attention kernels against the float64 emulation of their operand rounding (tests/f16x1_emulation.py), the kernels' agreement
bit for bit, and the model end to end against the reference goldens at the mode's stated tolerances (not reference-grade:
logits <= 1e-2, mask logits <= 1e-1; the same forward_test records)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16x1_emulation as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def no_grad():
    with torch.no_grad():
        yield


def _to_pair(t):
    """f32 (B, T, C) -> f16-format pair rows (test helper; mirrors vrd::store_pair4)"""
    from gemm_tile_cases import encode_pair
    from vrdone_amd import _hip, ops
    return ops.Pair(encode_pair(t, True), t.shape[-1], _hip.PAIR_F16)


def _gemm(x, w, bias, mode, **kw):
    from vrdone_amd import ops
    with ops.use_precision(mode):
        xin = _to_pair(x) if kw.pop("pair", True) else x
        return ops.conv_gemm(xin, w, bias, **kw)


# (B, T, Cin, N, k, pair input, kernel served): 576 tiles of 256 x 256 -> the 256 x 256 kernel (persistent for k = 1);
# 128 sequences -> 576 tiles of 128 x 256 but 288 of 256 x 256 -> the 128 x 256 kernel (Cin 256 with k = 3: so is the larger
# problem, the 256 x 256 kernel's one-product K steps of 64 need Cin % 64 == 0 -- 256 is, so 576 tiles of 256 x 256 take it);
# f32 rows: 288 tiles of 128 x 128 -> the 128 x 128 kernel (A split into its hi plane while staged), fewer than 256 -> its
# 64 x 64 form (SMALL)
SHAPES = [(256, 288, 512, 512, 1, True, "256x256"), (256, 288, 512, 512, 3, True, "256x256"), (256, 288, 256, 512, 3, True, "256x256"),
          (128, 288, 512, 512, 1, True, "128x256"), (128, 288, 256, 512, 3, True, "128x256"),
          (64, 96, 512, 768, 1, False, "128x128"), (64, 96, 256, 768, 3, False, "128x128"),
          (8, 96, 512, 256, 1, False, "64x64"), (8, 96, 256, 512, 3, False, "64x64"), (24, 96, 512, 512, 1, True, "64x64")]


@pytest.mark.parametrize("B,T,Cin,N,k,pair,kernel", SHAPES)
def test_one_product_gemm_against_emulation(B, T, Cin, N, k, pair, kernel):
    from vrdone_amd import ops
    gen = torch.Generator().manual_seed(B + T + Cin + N + k)
    x = torch.randn(B, T, Cin, generator=gen)
    w = torch.randn(N, Cin, k, generator=gen) / (Cin * k) ** 0.5
    bias = torch.randn(N, generator=gen)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    got1 = _gemm(xd, wd, bd, "f16x1", pair=pair)
    got3 = _gemm(xd, wd, bd, "f16x3", pair=pair)
    sample = [0, 1, B // 2, B - 1]
    want = E.conv1d(x[sample], w, bias)
    err = float((got1[sample].double().cpu() - want).abs().max())
    gap = float((got1[sample] - got3[sample]).abs().max())
    # exactly one product of the hi planes: the emulation of that is 100x closer than the three-product result
    assert err * 100 < gap, (kernel, err, gap)
    # pair output: the same result in hi + lo planes (16 significand bits)
    got_pair = _gemm(xd, wd, bd, "f16x1", pair=pair, out_pair=True)
    assert float(((got_pair.float() - got1).abs() / got1.abs().clamp_min(1e-3)).max()) < 2 ** -15
    with ops.use_precision("f16x1"):
        assert torch.equal(ops.conv_gemm(_to_pair(xd) if pair else xd, wd, bd), got1)      # deterministic


def test_one_product_gemm_padding_skip_and_batch():
    """A row mask with padded sequences (the 256 x 256 kernel's padding map) and a q / k / v batch (vrd_gemm_batch) in f16x1."""
    from vrdone_amd import ops
    gen = torch.Generator().manual_seed(5)
    B, T, Cin, N = 256, 288, 512, 512
    x = torch.randn(B, T, Cin, generator=gen)
    lens = torch.randint(1, T + 1, (B,), generator=gen)
    mask = torch.arange(T)[None] < lens[:, None]
    x = x * mask[..., None]
    ws = [torch.randn(N, Cin, 1, generator=gen) / Cin ** 0.5 for _ in range(3)]
    bs = [torch.randn(N, generator=gen) for _ in range(3)]
    md = mask.to(DEV)
    with ops.use_precision("f16x1"):
        xp = _to_pair(x.to(DEV))
        one = [ops.conv_gemm(xp, w.to(DEV), b.to(DEV), row_mask=md) for w, b in zip(ws, bs)]
        batch = ops.conv_gemm_batch([((xp, w.to(DEV), b.to(DEV)), dict(row_mask=md)) for w, b in zip(ws, bs)])
    for a, b in zip(one, batch):
        assert torch.equal(a, b)
    sample = [0, 7, B - 1]
    for w, b, got in zip(ws, bs, one):
        want = E.conv1d(x[sample], w, b) * mask[sample].double()[..., None]
        assert float((got[sample].double().cpu() - want).abs().max()) < 1e-4


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[2])
from vrdone_amd import ops
from test_gpu_f16x1 import _to_pair
gen = torch.Generator().manual_seed(77)
B, T, Cin, N, k = 256, 288, 512, 512, int(sys.argv[3])
x = torch.randn(B, T, Cin, generator=gen)
w = torch.randn(N, Cin, k, generator=gen) / (Cin * k) ** 0.5
b = torch.randn(N, generator=gen)
with torch.no_grad(), ops.use_precision("f16x1"):
    y = ops.conv_gemm(_to_pair(x.cuda()), w.cuda(), b.cuda())
torch.save(y.cpu(), sys.argv[1])
"""


@pytest.mark.parametrize("k", [1, 3])
def test_one_product_gemm_kernels_agree_bit_for_bit(k, tmp_path):
    """The same problem on each split kernel (fresh child processes: the choice is read once per process), one at a time."""
    forced = [("256x256", {}), ("128x256", {"VRD_X3_BIG_MIN_TILES": "100000000"}),
              ("128x128", {"VRD_X3_DMA": "0", "VRD_X3_SMALL": "0"})]
    outs = []
    for name, env in forced:
        path = str(tmp_path / f"{name}.pt")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _CHILD, path, os.path.dirname(os.path.abspath(__file__)), str(k)],
                           cwd=REPO, env=dict(os.environ, **env), capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        outs.append((name, torch.load(path)))
    for name, y in outs[1:]:
        assert torch.equal(y, outs[0][1]), name


ATTN_SHAPES = [(4, 128, 288, 288), (8, 64, 144, 144), (4, 128, 96, 77), (8, 64, 288, 288)]


@pytest.mark.parametrize("w64", ["0", "1"])
@pytest.mark.parametrize("H,hd,Tq,Tk", ATTN_SHAPES)
def test_one_product_flash_attention_against_emulation(w64, H, hd, Tq, Tk, monkeypatch):
    from vrdone_amd import ops
    monkeypatch.setenv("VRD_FLASH_W64", w64)
    gen = torch.Generator().manual_seed(H + hd + Tq + Tk)
    B, C = 3, H * hd
    # every query's largest score lies on key 0 (the first tile, where both kernels set the reference point of their
    # exponentials), 3-5 above the rest, so the f16 rounding of P happens relative to the row maximum as in the emulation,
    # while the probability mass stays spread over all keys
    u = torch.ones(hd) / hd ** 0.5
    q = 0.1 * torch.randn(B, Tq, C, generator=gen) + u.repeat(H)
    k = 0.3 * torch.randn(B, Tk, C, generator=gen)
    k[:, 0] = (4 * hd ** 0.5 * u).repeat(H)
    v = torch.randn(B, Tk, C, generator=gen)
    lens = torch.tensor([Tk, max(1, Tk // 3), 1])
    mask = torch.arange(Tk)[None] < lens[:, None]
    qp, kp, vp = (_to_pair(t.to(DEV)) for t in (q, k, v))
    with ops.use_precision("f16x1"):
        got1 = ops.attention(qp, kp, vp, mask.to(DEV), H)
        qlens = torch.tensor([Tq, min(Tq, 33), 1])
        qm = torch.arange(Tq)[None] < qlens[:, None]
        got_qm = ops.attention(qp, kp, vp, mask.to(DEV), H, q_mask=qm.to(DEV))
    with ops.use_precision("f16x3"):
        got3 = ops.attention(qp, kp, vp, mask.to(DEV), H)
    want = E.attention(q, k, v, mask, H)
    err = float((got1.double().cpu() - want).abs().max())
    gap = float((got1 - got3).abs().max())
    print(f"f16x1 attention w64={w64} H{H} hd{hd} Tq{Tq} Tk{Tk}: |got - emulation| {err:.2e}, |f16x1 - f16x3| {gap:.2e}")
    assert err * 20 < gap, (err, gap)
    assert gap < 2e-2
    # q_mask: rows of a 32-query tile that holds a valid query are the call without it
    for b in range(B):
        n = int(((int(qlens[b]) + 31) // 32) * 32)
        assert torch.equal(got_qm[b, :min(n, Tq)], got1[b, :min(n, Tq)])


def test_one_product_flash_attention_three_waves_per_workgroup():
    """attn_flash_x3_kernel's NW = 3 instantiations (VRD_FLASH_NW is read once per process: a child, under its own
    time limit)."""
    ids = [f"{os.path.abspath(__file__)}::test_one_product_flash_attention_against_emulation[{H}-{hd}-{Tq}-{Tk}-0]"
           for H, hd, Tq, Tk in ATTN_SHAPES]
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider"] + ids,
                       cwd=REPO, env=dict(os.environ, VRD_FLASH_NW="3"), capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(ATTN_SHAPES)} passed" in r.stdout


def _model(name):
    from test_gpu_model import get_model
    return get_model(name)


@pytest.mark.parametrize("name,T", [("vidvrd", 96), ("vidvrd", 144), ("vidvrd", 288),
                                    ("vidor_x", 512), ("vidor_local", 512), ("vidor", 512)])
def test_mask_vrd_f16x1_against_reference_golden(name, T):
    from test_gpu_model import c_in
    from vrdone_amd import ops
    model, mc, _, _ = _model(name)
    g = np.load(os.path.join(GOLDEN, f"mask_vrd_{name}.npz"))
    lens = g[f"T{T}_lengths"].tolist()
    x, m = O.synth_pairs(len(lens), c_in(mc), T, lens, seed=1234 + T)
    with ops.use_precision("f16x1"):
        ops.f16_range_flag().zero_()
        out = model._mask_vrd(x.to(DEV), m.to(DEV), with_aux=False)
        assert ops.f16_range_exceeded() == 0
    dl = float(np.abs(out["pred_logits"].cpu().numpy() - g[f"T{T}_pred_logits"]).max())
    dm = float(np.abs(out["pred_masks"].cpu().numpy() - g[f"T{T}_pred_masks"]).max())
    print(f"f16x1 {name} T{T}: max |dlogit| {dl:.2e}, max |dmask| {dm:.2e}")
    assert dl <= 1e-2 and dm <= 1e-1, (dl, dm)
    with ops.use_precision("f16x3"):
        ref3 = model._mask_vrd(x.to(DEV), m.to(DEV), with_aux=False)
    assert not torch.equal(ref3["pred_logits"], out["pred_logits"])          # the mode really runs other kernels
    # the kernels round where the emulation does (tests/f16x1_emulation.py: the oracle with the mode's rounding): the result is
    # closer to the emulation than to the reference -- a GEMM left at three products, or P rounded at another scale, is not
    _, _, _, sd = _model(name)
    with E.oracle_f16x1() as Oe:
        emu = Oe.mask_vrd(sd, mc, x, m, with_aux=False)
    el = float((out["pred_logits"].cpu() - emu["pred_logits"]).abs().max())
    em = float((out["pred_masks"].cpu() - emu["pred_masks"]).abs().max())
    print(f"f16x1 {name} T{T}: to the emulation max |dlogit| {el:.2e}, max |dmask| {em:.2e}")
    assert el < dl and em < dm, (el, dl, em, dm)


def _forward_test_cases():
    from golden_cases import FORWARD_TEST_VARIANTS, SLICES, VIDOR_X
    return {"vidvrd": ("forward_test_vidvrd.json", lambda c: synth_proposal(6, c, 20, 130, seed=4321)),
            "vidvrd_slices": ("forward_test_vidvrd_slices.json", lambda c: synth_proposal(c_in=c, **SLICES)),
            "vidor_x": ("forward_test_vidor_x.json", lambda c: synth_proposal(c_in=c, **VIDOR_X)),
            "vidor": ("forward_test_vidor.json", lambda c: synth_proposal(c_in=c, **FORWARD_TEST_VARIANTS["vidor"])),
            "vidor_local": ("forward_test_vidor_local.json", lambda c: synth_proposal(c_in=c, **FORWARD_TEST_VARIANTS["vidor_local"]))}


def _on_device(data):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}


@pytest.mark.parametrize("case", ["vidvrd", "vidvrd_slices", "vidor_x", "vidor", "vidor_local"])
def test_forward_test_f16x1_keeps_the_golden_records(case):
    from golden_cases import compare_forward_test
    from test_gpu_model import c_in
    from vrdone_amd import ops
    golden, make = _forward_test_cases()[case]
    model, mc, ic, _ = _model(case.replace("_slices", ""))
    with open(os.path.join(GOLDEN, golden)) as f:
        ref = json.load(f)
    data = _on_device(make(c_in(mc)))
    with ops.use_precision("f16x1"):
        res = model(data)
        # many videos in one call: per video the same result
        other = _on_device(synth_proposal(5, c_in(mc), 20, 90, seed=11, feat_stride=ic["feat_stride"],
                                          random_offset=ic["feat_stride"] > 1))
        both = model.forward_test_videos([other, data])
        alone = model.forward_test(other)
    compare_forward_test(res, ref, ic["n_max_pair"], 2e-4, slack=0, tie_tol=2e-4)
    for got, want in ((both[1], res), (both[0], alone)):
        assert (got is None) == (want is None)
        if got is not None:
            assert got["triplets"] == want["triplets"] and got["triple_scores_avg"] == want["triple_scores_avg"]


def test_f16x1_internal_overflow_is_reported_and_repeated_in_f32():
    """The up-projection x 4000 edit of test_gpu_model: f16x1 reports flag bit 8 and forward_test returns the f32 result."""
    import warnings
    from test_gpu_model import _model_with, c_in
    from vrdone_amd import ops

    def edit(sd):
        sd["backbone.stem.0.mlp.0.weight"] *= 4000.0
        sd["backbone.stem.0.mlp.0.bias"] *= 4000.0
        sd["backbone.stem.0.mlp.3.weight"] /= 4000.0
    model, mc, _ = _model_with(edit)
    data = _on_device(synth_proposal(4, c_in(mc), 20, 60, seed=98))
    with ops.use_precision("f32"):
        want = model(data)
    with ops.use_precision("f16x1"):
        inputs, masks, _ = model.preprocessing(data["so_features_list"])
        ops.f16_range_flag().zero_()
        model._mask_vrd(inputs[0], masks[0], with_aux=False)
        assert ops.f16_range_exceeded() & 8
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = model(data)
    assert any("f16x1" in str(x.message) for x in w)
    assert got["triplets"] == want["triplets"] and got["triple_scores_avg"] == want["triple_scores_avg"]


def test_f16x1_training_step_raises():
    from vrdone_amd import configs, ops
    from vrdone_amd.models.maskvrd import MaskVRD
    from vrdone_amd import synth
    cfg = configs.model_config("vidvrd")
    model = synth.load_synthetic_weights(MaskVRD(cfg, device=DEV)).to(DEV)
    model.train()
    x, m = synth.synth_pairs(2, configs.input_channels(cfg), 96, [96, 40], seed=3)
    with ops.use_precision("f16x1"), torch.enable_grad():
        with pytest.raises(ValueError, match="f16x1"):
            model._mask_vrd(x.to(DEV), m.to(DEV), with_aux=False)
