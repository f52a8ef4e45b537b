"""Banded attention at windows other than the shipped 7 / 9 (any odd window from 3 to 19), CPU side: the oracle against
goldens of the real reference (scripts/make_golden_window.py; cases in tests/local_window_cases.py), the premise of tight
padding at the smallest and the largest window, and the argument check of ops.local_attention.

Tolerances are those tests/test_oracle_golden.py applies to the same functions at windows 7 / 9."""
import json
import os

import numpy as np
import pytest
import torch

import local_window_cases as LW
from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

LOGIT_TOL, MASK_TOL = 2e-5, 2e-4


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(GOLDEN, "local_window.npz")) as z:
        return {k: z[k] for k in z.files}


def sub(t):
    return t.detach()[:, ::LW.CH_STRIDE].numpy()


def c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


def grad_close(got, want, tol, what):
    """l2 error relative to the stored entries' l2 norm (the measure of golden_cases.compare_grads)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-12)
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.1e}"


def test_case_shapes():
    """What the cases are chosen for: two strips of 16 rows and a partial one, whole chunks of the reference, a sequence of
    half a window, a length that is no multiple of 16, a fully masked sequence."""
    for W in LW.WINDOWS:
        T, lens = LW.seq_len(W), LW.lengths(W)
        assert 34 <= T < 34 + 2 * (W // 2) and T % (2 * (W // 2)) == 0 and T % 16
        assert lens[0] % 16 and lens[1] == W // 2 and lens[2] == 0


@pytest.mark.parametrize("W,H,rel", LW.OP_CASES)
def test_banded_attention_matches_reference_core(g, W, H, rel):
    q, k, v, dO, rel_pe = LW.core_inputs(W, H, rel)
    m = LW.mask(W)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    bias = rel_pe.clone().requires_grad_(True) if rel else None
    with torch.enable_grad():
        out = O.banded_attention(*leaves, m, H, W // 2, rel_pe=bias)
        out.backward(dO)
    p = f"core/{LW.tag(W, H, rel)}/"
    np.testing.assert_allclose(sub(out), g[p + "out"], atol=2e-5, rtol=0)
    assert float(out[2].detach().abs().max()) == 0.0 and float(out[1, :, W // 2:].detach().abs().max()) == 0.0        # masked query rows
    for n, t in zip(("dq", "dk", "dv"), leaves):
        grad_close(sub(t.grad), g[p + n], 2e-5, n)
    if rel:
        grad_close(bias.grad.numpy(), g[p + "drel"], 2e-5, "d rel_pe")


@pytest.mark.parametrize("W,H,rel", LW.OP_CASES)
def test_local_mhca_matches_reference(g, W, H, rel):
    x, dy = LW.mhca_inputs(W, H, rel)
    pre = LW.mhca_prefix(W, H, rel)
    p = f"mhca/{LW.tag(W, H, rel)}/"
    names = [k[len(p) + 2:] for k in g if k.startswith(p + "d/")]
    assert ("rel_pe" in names) == rel
    shapes = {"rel_pe": (1, 1, H, W)}
    for n in ("query", "key", "value"):
        shapes.update({f"{n}_conv.conv.weight": (LW.C, 1, 3), f"{n}_norm.weight": (1, LW.C, 1), f"{n}_norm.bias": (1, LW.C, 1)})
    for n in ("query", "key", "value", "proj"):
        shapes.update({f"{n}.weight": (LW.C, LW.C, 1), f"{n}.bias": (LW.C,)})
    assert set(names) == set(shapes) - (set() if rel else {"rel_pe"})
    sd = {k: v.requires_grad_(True) for k, v in O.synth_state_dict([(f"{pre}.{n}", shapes[n]) for n in names]).items()}
    x = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out, _ = O.local_mhca(sd, pre, x, LW.mask(W), H, W, 1)
        out.backward(dy)
    np.testing.assert_allclose(sub(out), g[p + "out"], atol=2e-5, rtol=0)
    grad_close(sub(x.grad), g[p + "dx"], 2e-5, "dx")
    # the measure of tests/test_gpu_train.py's check_param_grads: l2 error over the l2 norm of the stored entries plus a floor of
    # 1e-3 of the largest whole-gradient norm (a key branch's biases shift every score of a query equally: their gradient is mathematically
    # zero and holds rounding noise on both sides), held to the 1e-3 test_oracle_golden asks of parameter gradients
    floor = 1e-3 * max(float(g[p + "norm/" + n]) for n in names)
    for n in names:
        got, want = LW.sample(sd[f"{pre}.{n}"].grad).numpy().astype(np.float64), g[p + "d/" + n].astype(np.float64)
        assert got.shape == want.shape
        assert np.linalg.norm(got - want) / (np.linalg.norm(want) + floor) <= 1e-3, n


@pytest.mark.parametrize("W", LW.SOS_WINDOWS)
def test_sos_local_decoder_layer_matches_reference(g, W):
    from vrdone_amd.models.local_transformer import MaskedConvTransformerDecoderLayer
    x, y, dy, m = LW.sos_inputs(W)
    pre = f"op.sos_local_w{W}"
    layer = MaskedConvTransformerDecoderLayer(LW.C, 8, path_pdrop=0.1, n_qx_stride=1, n_kv_stride=1, with_ffn=False, use_local=True,
                                              win_size=W)
    sd = O.synth_state_dict([(f"{pre}.{k}", tuple(v.shape)) for k, v in layer.state_dict().items()])
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    with torch.enable_grad():
        out, _ = O.decoder_layer(sd, pre, x, y, m, m, 8, half_win=W // 2)
        out.backward(dy)
    p = f"sos/w{W}/"
    np.testing.assert_allclose(sub(out), g[p + "out"], atol=5e-5, rtol=0)
    grad_close(sub(x.grad), g[p + "dx"], 2e-5, "dx")
    grad_close(sub(y.grad), g[p + "dy"], 2e-5, "dy")


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(case):
        if case not in cache:
            mc, ic, keys = load_case(LW.MODEL_CASES[case]["base"])
            cache[case] = (LW.model_config(mc, case), ic, O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]))
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(LW.MODEL_CASES))
def test_mask_vrd_matches_reference(models, case):
    mc, _, sd = models(case)
    spec = LW.MODEL_CASES[case]
    gm = np.load(os.path.join(GOLDEN, "local_window_model.npz"))
    x, m = O.synth_pairs(len(spec["lens"]), c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
    with torch.no_grad():
        out = O.mask_vrd(sd, mc, x, m, with_aux=False)
    np.testing.assert_allclose(out["pred_logits"].numpy(), gm[f"{case}/pred_logits"], atol=LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(out["pred_masks"].numpy(), gm[f"{case}/pred_masks"], atol=MASK_TOL, rtol=0)


def test_forward_test_window_19_matches_reference(models):
    mc, ic, sd = models("vidvrd_w19")
    with open(os.path.join(GOLDEN, "forward_test_vidvrd_w19.json")) as f:
        ref = json.load(f)
    data = synth_proposal(c_in=c_in(mc), **LW.FORWARD_TEST_W19)
    assert [int(f.shape[1]) for f in data["so_features_list"]] == ref["pair_lengths"]
    with torch.no_grad():
        res = O.forward_test(sd, mc, ic, data)
    from golden_cases import compare_forward_test
    np.testing.assert_allclose(res["triple_scores"], ref["triple_scores"], atol=1e-5, rtol=0)
    compare_forward_test(res, ref, ic["n_max_pair"], 1e-5, slack=0)


def test_training_step_window_5_matches_reference(models):
    """As test_oracle_golden.test_training_step_gradients_match_reference, at window 5."""
    from golden_cases import compare_grads, replay_matching, train_batch
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, sd = models("vidvrd_w5")
    with open(os.path.join(GOLDEN, "train_step_vidvrd_w5.json")) as f:
        meta = json.load(f)
    gt = LW.load_npz_parts(os.path.join(GOLDEN, "train_step_vidvrd_w5"))
    lens, x, m, data = train_batch(mc, c_in(mc), spec=LW.TRAIN_W5)
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
    compare_grads([(n, leaves[n].grad) for n in names], gt, meta, "nodrop", rtol=1e-3, median_tol=2e-5)


@pytest.mark.parametrize("win,T_ref", [(3, 96), (19, 144)])
def test_result_is_independent_of_the_padded_length_at_the_extreme_windows(win, T_ref):
    """The premise of MaskVRD.tight_len (see test_oracle_golden.test_result_is_independent_of_the_padded_length_above_the_tight_one)
    does not depend on the window: a masked key inside the window and a key beyond the sequence's end both weigh exactly
    nothing, so a valid frame cannot tell how far the padding goes.  The oracle in float64, windows 3 and 19: any padded
    length from 8 * (ceil(L / 8) + 1) on gives the outputs of the reference's own padded length to 1e-12 -- lengths that are no
    multiple of the window's chunk included, which the kernels (unlike the reference's chunked form) accept."""
    mc, _, keys = load_case("vidvrd")
    mc = dict(mc, n_mha_win_size=win, max_seq_len=T_ref)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]).items()}
    for L in (41, 7):
        feat = torch.randn(1, c_in(mc), L, generator=torch.Generator().manual_seed(L + win), dtype=torch.float64)

        def run(T):
            x = torch.zeros(1, c_in(mc), T, dtype=torch.float64)
            x[..., :L] = feat
            with torch.no_grad():
                o = O.mask_vrd(sd, mc, x, (torch.arange(T) < L)[None, None], with_aux=False)
            return o["pred_logits"], o["pred_masks"][..., :L]
        want = run(T_ref)
        tight = 8 * (-(-L // 8) + 1)
        for T in (tight, tight + 8):
            got = run(T)
            assert float((got[0] - want[0]).abs().max()) < 1e-12 and float((got[1] - want[1]).abs().max()) < 1e-12, (win, L, T)
        if L > 8:
            below = run(tight - 8)
            assert float((below[1] - want[1]).abs().max()) > 1e-3, (win, L, tight - 8)


@pytest.mark.parametrize("window", [1, 4, 21])
def test_local_attention_rejects_windows_outside_the_envelope(window):
    """Even or out-of-range windows: a ValueError that names the range, before any launch (CPU tensors never reach one).
    Callers pass half_win = window // 2 of an odd window; an even window has no integer half window ((window - 1) / 2)."""
    from vrdone_amd import ops
    half = (window - 1) // 2 if window % 2 else (window - 1) / 2
    q = torch.zeros(1, 8, 512)
    with pytest.raises(ValueError, match="odd, from 3 to 19"):
        ops.local_attention(q, q, q, torch.ones(1, 8, dtype=torch.bool), 4, half)


@pytest.mark.parametrize("window", [4, 1])
def test_modules_reject_even_and_unit_windows(window):
    from vrdone_amd.models.blocks import LocalMaskedMHCA
    with pytest.raises(AssertionError):
        LocalMaskedMHCA(512, 4, window_size=window)
