"""The f16x1 precision mode (one f16 MFMA product per GEMM and global attention) without a GPU: the mode switch, the ABI of
the one-product form and its host-side argument checks, the forward-only guard, and the emulation helper's rounding."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN, load_case
from oracle.synth import synth_proposal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16x1_emulation as E  # noqa: E402
from torch.nn import functional as F  # noqa: E402


def test_set_precision_and_use_precision_accept_f16x1():
    from vrdone_amd import _hip, ops
    old = ops.get_precision()
    try:
        ops.set_precision("f16x1")
        assert ops.get_precision() == "f16x1"
        assert ops.pair_fmt() == _hip.PAIR_F16 and ops.products() == 1 and ops.f16_planes()
        with torch.no_grad():
            assert ops.pair_mode()
        with ops.use_precision("f16x3"):
            assert ops.products() == 0 and ops.f16_planes()
        assert ops.get_precision() == "f16x1"
        with ops.use_precision("bf16x3"):
            assert not ops.f16_planes() and ops.products() == 0
    finally:
        ops.set_precision(old)
    with pytest.raises(ValueError):
        ops.set_precision("f16x2")
    with pytest.raises(ValueError):
        ops.set_precision("bf16x1")


def test_environment_variable_selects_f16x1_in_a_fresh_interpreter():
    code = "from vrdone_amd import ops; print(ops.get_precision(), ops.products())"
    env = dict(os.environ, VRDONE_PRECISION="f16x1")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["f16x1", "1"]
    env["VRDONE_PRECISION"] = "f16x9"
    bad = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "VRDONE_PRECISION" in bad.stderr


def test_abi_version_and_products_field():
    from vrdone_amd import _hip
    assert _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    assert _hip.GemmArgs._fields_[-1] == ("products", ctypes.c_int32)
    header = open(os.path.join(REPO, "include", "vrdone_hip.h")).read()
    assert "#define VRD_ABI_VERSION 37" in header
    body = re.search(r"typedef struct \{([^}]*)\} vrd_gemm_args", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert body.strip().rstrip(";").split()[-1] == "products"
    proto = re.search(r"int vrd_attention_pair\(([^)]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    assert proto.split(",")[-1].split() == ["int", "products"]
    _, argtypes = _hip._SIGNATURES["vrd_attention_pair"]
    assert argtypes[-1] is ctypes.c_int and argtypes[-2] is ctypes.c_void_p


def _gemm_args(split_fmt, products):
    from vrdone_amd import _hip
    a = _hip.GemmArgs()
    # host-side validation happens before any device access: dummy (aligned, non-null) addresses suffice
    a.A, a.W, a.C, a.W_split, a.w_scale = 256, 256, 256, 256, 256
    a.lda, a.ldc, a.M, a.N, a.Cin, a.taps, a.T = 64, 64, 64, 64, 64, 1, 64
    a.split_fmt, a.products = split_fmt, products
    return a


@pytest.mark.parametrize("split_fmt,products", [(1, 1), (0, 1), (2, 2), (2, -1), (2, 4)])
def test_gemm_rejects_one_product_outside_the_f16_format(split_fmt, products):
    from vrdone_amd import _hip
    a = _gemm_args(split_fmt, products)
    rc = _hip.lib.vrd_gemm(ctypes.byref(a), None)
    assert rc < 0 and b"products" in _hip.lib.vrd_last_error()


def test_gemm_one_product_needs_w_split():
    from vrdone_amd import _hip
    a = _gemm_args(2, 1)
    a.W_split = None
    assert _hip.lib.vrd_gemm(ctypes.byref(a), None) < 0 and b"products" in _hip.lib.vrd_last_error()


def test_gemm_batch_requires_the_same_products_in_every_entry():
    from vrdone_amd import _hip
    arr = (_hip.GemmArgs * 2)(_gemm_args(2, 1), _gemm_args(2, 3))
    assert _hip.lib.vrd_gemm_batch(arr, 2, None) < 0 and b"vrd_gemm_batch" in _hip.lib.vrd_last_error()


@pytest.mark.parametrize("pair_fmt,products", [(1, 1), (2, 2), (2, 5)])
def test_attention_pair_rejects_bad_products(pair_fmt, products):
    from vrdone_amd import _hip
    rc = _hip.lib.vrd_attention_pair(256, 512, 256, 256, 512, None, None, 2, 64, 64, 4, 128, 256, 512, 0, pair_fmt, None, products)
    assert rc < 0 and b"products" in _hip.lib.vrd_last_error()


def test_recording_autograd_in_f16x1_raises():
    from vrdone_amd import autograd, ops
    x = torch.randn(2, 8, 32, requires_grad=True)
    w = torch.randn(16, 32, 1, requires_grad=True)
    with ops.use_precision("f16x1"):
        with torch.enable_grad():
            with pytest.raises(ValueError, match="f16x1"):
                ops.conv_gemm(x, w, None)
            with pytest.raises(ValueError, match="f16x1"):
                autograd.Linear.apply(x, w, None, None)
            with pytest.raises(ValueError, match="f16x1"):
                autograd.Activation.apply(x, ops.ACT_RELU)


def test_forward_training_with_grad_raises_in_f16x1():
    from vrdone_amd import configs, ops, synth
    from vrdone_amd.models.maskvrd import MaskVRD
    cfg = configs.model_config("vidvrd")
    model = synth.load_synthetic_weights(MaskVRD(cfg, device="cpu"))
    model.train()
    with ops.use_precision("f16x1"), torch.enable_grad():
        with pytest.raises(ValueError, match="forward-only"):
            model.forward_training({"so_features_list": []})


def test_emulation_rounding():
    # activations: f16 of x * 16 -- 11 significant bits, subnormals kept below 2^-14 / 16
    x = torch.tensor([1.0 + 2.0 ** -12, 1.0 + 2.0 ** -10, 2.0 ** -19, 3000.0], dtype=torch.float64)
    got = E.round_act(x)
    assert got[0] == 1.0 and got[1] == 1.0 + 2.0 ** -10 and got[2] == 2.0 ** -19 and got[3] == 3000.0
    # weights: a per-tensor power of two with max |w| * 2^e in [2^14, 2^15)
    w = torch.tensor([0.75, -0.001, 1e-9], dtype=torch.float64)
    e = E.weight_exp(w)
    assert 2.0 ** 14 <= 0.75 * 2.0 ** e < 2.0 ** 15
    assert E.round_weight(w)[0] == 0.75
    # the attention emulation is a softmax average: rows sum to one in the rounded P up to its rounding
    q, k, v = torch.randn(1, 5, 64), torch.randn(1, 7, 64), torch.ones(1, 7, 64)
    out = E.attention(q, k, v, None, 1)
    assert float((out - 1.0).abs().max()) < 2.0 ** -9


def _c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


def test_emulation_wraps_the_oracle():
    """Inside oracle_f16x1 the oracle's split-GEMM convs and flash-size global attention round; outside they do not."""
    from oracle import vrd_oracle as O
    gen = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 64, 40, generator=gen), torch.randn(32, 64, 3, generator=gen) / 14
    q, k, v = (torch.randn(2, 128, 40, generator=gen) for _ in range(3))
    mask = torch.ones(2, 1, 40, dtype=torch.bool)
    exact_c, exact_a = O.F.conv1d(x, w, padding=1), O.full_attention(q, k, v, mask, 2)
    with E.oracle_f16x1() as Oe:
        got_c, got_a = Oe.F.conv1d(x, w, padding=1), Oe.full_attention(q, k, v, mask, 2)
        dw = torch.randn(64, 1, 3, generator=gen)
        assert torch.equal(Oe.F.conv1d(x, dw, padding=1, groups=64), F.conv1d(x, dw, padding=1, groups=64))
    want_c = torch.nn.functional.conv1d(E.round_act(x), E.round_weight(w), padding=1).float()
    assert torch.equal(got_c, want_c) and not torch.equal(got_c, exact_c)
    assert 1e-5 < float((got_a - exact_a).abs().max()) < 5e-3
    assert O.F is torch.nn.functional and torch.equal(O.full_attention(q, k, v, mask, 2), exact_a)


def _forward_test_cases():
    from golden_cases import FORWARD_TEST_VARIANTS, SLICES, VIDOR_X
    return {"vidvrd": ("vidvrd", "forward_test_vidvrd.json", lambda c: synth_proposal(6, c, 20, 130, seed=4321)),
            "vidvrd_slices": ("vidvrd", "forward_test_vidvrd_slices.json", lambda c: synth_proposal(c_in=c, **SLICES)),
            "vidor_x": ("vidor_x", "forward_test_vidor_x.json", lambda c: synth_proposal(c_in=c, **VIDOR_X)),
            "vidor": ("vidor", "forward_test_vidor.json", lambda c: synth_proposal(c_in=c, **FORWARD_TEST_VARIANTS["vidor"])),
            "vidor_local": ("vidor_local", "forward_test_vidor_local.json",
                            lambda c: synth_proposal(c_in=c, **FORWARD_TEST_VARIANTS["vidor_local"]))}


@pytest.mark.parametrize("case", ["vidvrd", "vidvrd_slices", "vidor_x", "vidor", "vidor_local"])
def test_emulated_f16x1_forward_test_keeps_the_golden_records(case):
    """The accuracy claim of the mode without a GPU: the oracle with the f16x1 rounding returns the reference's records (same
    triplets, tracklets and durations; scores within 2e-4, ranks permuted only inside near-ties)."""
    from golden_cases import compare_forward_test
    from oracle import vrd_oracle as O
    name, golden, make = _forward_test_cases()[case]
    mc, ic, keys = load_case(name)
    sd = O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"])
    with open(os.path.join(GOLDEN, golden)) as f:
        ref = json.load(f)
    data = make(_c_in(mc))
    with torch.no_grad(), E.oracle_f16x1() as Oe:
        res = Oe.forward_test(sd, mc, ic, data)
    compare_forward_test(res, ref, ic["n_max_pair"], 2e-4, slack=0, tie_tol=2e-4)
    # ... and the rounding is really applied: scores move by more than the f32 oracle's own ~1e-6
    got = sorted(res["triple_scores_avg"])[::-1]
    want = sorted(ref["triple_scores_avg"])[::-1]
    assert max(abs(a - b) for a, b in zip(got, want)) > 5e-6
