"""Banded attention at width 256 (8, 4, 2 heads) and at width 512 with 16 heads, CPU side: the oracle against goldens of the
real reference (scripts/make_golden_heads.py; cases in tests/local_heads_cases.py), the envelope check of
ops.local_attention, and the width-256 model's parameter list.

Tolerances are those tests/test_local_window_cpu.py applies to the same functions at width 512 with 4 / 8 heads."""
import json
import os

import numpy as np
import pytest
import torch

import local_heads_cases as LH
from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal
from test_local_window_cpu import LOGIT_TOL, MASK_TOL, c_in, grad_close, sub


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(GOLDEN, "local_heads.npz")) as z:
        return {k: z[k] for k in z.files}


def model_keys(mc):
    """state_dict keys and shapes of the model at this config (test_width_256_model_has_the_reference_parameters holds them to
    the reference's list)."""
    from vrdone_amd.models.maskvrd import MaskVRD
    return [(k, list(v.shape)) for k, v in MaskVRD(mc, device="cpu").state_dict().items()]


def test_stored_channels_visit_every_lane_slot_and_head():
    """Every 17th channel: at either width the sample holds every channel slot of a lane (8 a lane at width 512, 4 at 256) and at
    least one channel of every head."""
    for C, H in LH.SHAPES:
        ch = np.arange(0, C, LH.CH_STRIDE)
        cpl = 8 if C == 512 else 4
        assert set(ch % cpl) == set(range(cpl)), (C, H)
        assert set(ch // (C // H)) == set(range(H)), (C, H)
    assert {C // H for C, H in LH.SHAPES} == {32, 64, 128}


@pytest.mark.parametrize("C,H,W,rel", LH.OP_CASES)
def test_banded_attention_matches_reference_core(g, C, H, W, rel):
    q, k, v, dO, rel_pe = LH.core_inputs(C, H, W, rel)
    m = LH.mask(W)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    bias = rel_pe.clone().requires_grad_(True) if rel else None
    with torch.enable_grad():
        out = O.banded_attention(*leaves, m, H, W // 2, rel_pe=bias)
        out.backward(dO)
    p = f"core/{LH.tag(C, H, W, rel)}/"
    np.testing.assert_allclose(sub(out), g[p + "out"], atol=2e-5, rtol=0)
    assert float(out[2].detach().abs().max()) == 0.0 and float(out[1, :, W // 2:].detach().abs().max()) == 0.0        # masked query rows
    for n, t in zip(("dq", "dk", "dv"), leaves):
        grad_close(sub(t.grad), g[p + n], 2e-5, n)
    if rel:
        grad_close(bias.grad.numpy(), g[p + "drel"], 2e-5, "d rel_pe")


@pytest.mark.parametrize("C,H,W,rel", LH.MHCA_CASES)
def test_local_mhca_matches_reference(g, C, H, W, rel):
    x, dy = LH.mhca_inputs(C, H, W, rel)
    pre = LH.mhca_prefix(C, H, W, rel)
    p = f"mhca/{LH.tag(C, H, W, rel)}/"
    names = [k[len(p) + 2:] for k in g if k.startswith(p + "d/")]
    assert ("rel_pe" in names) == rel
    shapes = {"rel_pe": (1, 1, H, W)}
    for n in ("query", "key", "value"):
        shapes.update({f"{n}_conv.conv.weight": (C, 1, 3), f"{n}_norm.weight": (1, C, 1), f"{n}_norm.bias": (1, C, 1)})
    for n in ("query", "key", "value", "proj"):
        shapes.update({f"{n}.weight": (C, C, 1), f"{n}.bias": (C,)})
    assert set(names) == set(shapes) - (set() if rel else {"rel_pe"})
    sd = {k: v.requires_grad_(True) for k, v in O.synth_state_dict([(f"{pre}.{n}", shapes[n]) for n in names]).items()}
    x = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out, _ = O.local_mhca(sd, pre, x, LH.mask(W), H, W, 1)
        out.backward(dy)
    np.testing.assert_allclose(sub(out), g[p + "out"], atol=2e-5, rtol=0)
    grad_close(sub(x.grad), g[p + "dx"], 2e-5, "dx")
    floor = 1e-3 * max(float(g[p + "norm/" + n]) for n in names)          # (test_local_window_cpu.test_local_mhca_matches_reference)
    for n in names:
        got, want = LH.sample(sd[f"{pre}.{n}"].grad).numpy().astype(np.float64), g[p + "d/" + n].astype(np.float64)
        assert got.shape == want.shape
        assert np.linalg.norm(got - want) / (np.linalg.norm(want) + floor) <= 1e-3, n


def test_sos_local_decoder_layer_matches_reference(g):
    from vrdone_amd.models.local_transformer import MaskedConvTransformerDecoderLayer
    s = LH.SOS_CASE
    x, y, dy, m = LH.sos_inputs()
    layer = MaskedConvTransformerDecoderLayer(s["C"], s["H"], path_pdrop=0.1, n_qx_stride=1, n_kv_stride=1, with_ffn=False, use_local=True,
                                              win_size=s["W"])
    sd = O.synth_state_dict([(f"{LH.SOS_PREFIX}.{k}", tuple(v.shape)) for k, v in layer.state_dict().items()])
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    with torch.enable_grad():
        out, _ = O.decoder_layer(sd, LH.SOS_PREFIX, x, y, m, m, s["H"], half_win=s["W"] // 2)
        out.backward(dy)
    np.testing.assert_allclose(sub(out), g["sos/out"], atol=5e-5, rtol=0)
    grad_close(sub(x.grad), g["sos/dx"], 2e-5, "dx")
    grad_close(sub(y.grad), g["sos/dy"], 2e-5, "dy")


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(case):
        if case not in cache:
            mc, ic, _ = load_case(LH.MODEL_CASES[case]["base"])
            mc = LH.model_config(mc, case)
            cache[case] = (mc, ic, O.synth_state_dict(model_keys(mc), eos_coef=mc["loss_coeff_dict"]["eos_coef"]))
        return cache[case]
    return get


def test_width_256_model_has_the_reference_parameters():
    """MaskVRD builds at width 256, with the state_dict keys and shapes of the reference's model (listed in the golden JSON)."""
    mc, _, _ = load_case("vidvrd")
    with open(os.path.join(GOLDEN, "train_step_vidvrd_c256.json")) as f:
        want = json.load(f)["state_keys"]
    got = model_keys(LH.model_config(mc, "vidvrd_c256"))
    assert [(k, list(s)) for k, s in want] == got
    assert any(s and s[0] == 256 for _, s in got) and not any(k.startswith("backbone.stem") and 512 in s for k, s in got)


@pytest.mark.parametrize("case", list(LH.MODEL_CASES))
def test_mask_vrd_matches_reference(models, case):
    mc, _, sd = models(case)
    spec = LH.MODEL_CASES[case]
    gm = np.load(os.path.join(GOLDEN, "local_heads_model.npz"))
    x, m = O.synth_pairs(len(spec["lens"]), c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
    with torch.no_grad():
        out = O.mask_vrd(sd, mc, x, m, with_aux=False)
    np.testing.assert_allclose(out["pred_logits"].numpy(), gm[f"{case}/pred_logits"], atol=LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(out["pred_masks"].numpy(), gm[f"{case}/pred_masks"], atol=MASK_TOL, rtol=0)


def test_forward_test_width_256_matches_reference(models):
    mc, ic, sd = models("vidvrd_c256")
    with open(os.path.join(GOLDEN, "forward_test_vidvrd_c256.json")) as f:
        ref = json.load(f)
    data = synth_proposal(c_in=c_in(mc), **LH.FORWARD_TEST_C256)
    assert [int(f.shape[1]) for f in data["so_features_list"]] == ref["pair_lengths"]
    with torch.no_grad():
        res = O.forward_test(sd, mc, ic, data)
    from golden_cases import compare_forward_test
    np.testing.assert_allclose(res["triple_scores"], ref["triple_scores"], atol=1e-5, rtol=0)
    compare_forward_test(res, ref, ic["n_max_pair"], 1e-5, slack=0)


def test_training_step_width_256_matches_reference(models):
    """As test_local_window_cpu.test_training_step_window_5_matches_reference, at width 256."""
    from golden_cases import compare_grads, replay_matching, train_batch
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, sd = models("vidvrd_c256")
    with open(os.path.join(GOLDEN, "train_step_vidvrd_c256.json")) as f:
        meta = json.load(f)
    gt = LH.load_npz_parts(os.path.join(GOLDEN, "train_step_vidvrd_c256"))
    lens, x, m, data = train_batch(mc, c_in(mc), spec=LH.TRAIN_C256)
    assert lens == meta["lengths"]
    model = MaskVRD(mc, device="cpu").train()
    differing = replay_matching(model, meta["cases"]["nodrop"]["indices"])
    names = [n for n, _ in model.named_parameters()]
    leaves = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    with torch.enable_grad():
        pred = O.mask_vrd(leaves, mc, x, m, with_aux=True)
        loss = model.criterion(pred, data)
        loss["total_loss"].backward()
    want = meta["cases"]["nodrop"]["losses"]
    assert set(loss) == set(want)
    for k, v in want.items():
        assert abs(float(loss[k]) - v) <= 1e-4 * max(1.0, abs(v)), k
    assert all(lens[n] < 16 for call in differing for n in call), differing       # only near-ties of very short pairs
    # The bound of the test this mirrors (atol_frac at its default 1e-6) on every parameter but the key branches' biases: a bias on
    # the keys shifts every score of a query equally, the softmax does not see it, so its gradient is mathematically zero and holds
    # rounding noise on both sides (key_norm.bias of branch.0 is 1.25e-3 of its own stored norm apart at width 256).  Those are
    # held to what they are instead: nothing, to 1e-5 of the model's largest gradient norm, here and in the reference.
    import re
    zero = [n for n in names if re.search(r"\.key(_norm)?\.bias$", n)]
    assert zero and len(zero) < len(names) // 8
    compare_grads([(n, leaves[n].grad) for n in names if n not in zero], gt, meta, "nodrop", rtol=1e-3, median_tol=2e-5)
    stats = meta["cases"]["nodrop"]["grad_stats"]
    biggest = max(v[2] for v in stats.values())
    for n in zero:
        assert float(leaves[n].grad.double().norm()) <= 1e-5 * biggest and stats[n][2] <= 1e-5 * biggest, n


# ------------------------------------------------------------------------------------------------------------ envelope
@pytest.mark.parametrize("width,n_head", [(384, 6), (512, 3), (256, 16)])
def test_local_attention_rejects_shapes_outside_the_envelope(width, n_head):
    """Width 384, width 512 with 3 heads, width 256 with 16 heads (head_dim 16): a ValueError that names the envelope and the
    offending values, before any device check or launch (CPU tensors never reach one)."""
    from vrdone_amd import ops
    q = torch.zeros(1, 8, width)
    with pytest.raises(ValueError, match=r"width 256 or 512 .* 32, 64 or 128 .*got width %d, n_head %d" % (width, n_head)):
        ops.local_attention(q, q, q, torch.ones(1, 8, dtype=torch.bool), n_head, 2)


@pytest.mark.parametrize("width,n_head", [(512, 16), (512, 8), (512, 4), (256, 8), (256, 4), (256, 2)])
def test_local_attention_takes_the_accepted_shapes_past_the_envelope_check(width, n_head):
    """The accepted sets do not raise that error: on CPU tensors the call gets as far as the device check."""
    from vrdone_amd import ops
    q = torch.zeros(1, 8, width)
    with pytest.raises(RuntimeError, match="HIP tensors"):
        ops.local_attention(q, q, q, torch.ones(1, 8, dtype=torch.bool), n_head, 2)
