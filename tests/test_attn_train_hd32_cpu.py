"""The training fixture at 16 heads (head_dim 32 in the global attention of the SOS layers), on the CPU.

tests/golden/train_step_vidvrd_h16.json + _a.npz, _b.npz, ... hold one training step of the real reference at case `vidvrd_h16`
of tests/local_heads_cases.py (scripts/make_golden_h16_train.py).  Here the fixture is held to the model's parameter list and
to the CPU oracle, with the bounds tests/test_local_heads_cpu.py uses for the width-256 training fixture, before any GPU test
(tests/test_gpu_attn_train_hd32.py) relies on it."""
import glob
import json
import os
import re

import numpy as np
import torch

import local_heads_cases as LH
from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from test_local_heads_cpu import model_keys
from test_local_window_cpu import c_in

CASE = "vidvrd_h16"
STEM = os.path.join(GOLDEN, "train_step_" + CASE)
PART_LIMIT = max(os.path.getsize(os.path.join(GOLDEN, f"train_step_vidvrd_w5_{p}.npz")) for p in "ab")


def load_fixture():
    """(meta, sampled gradients of every part)"""
    with open(STEM + ".json") as f:
        meta = json.load(f)
    arrs = {}
    for path in sorted(glob.glob(STEM + "_?.npz")):
        with np.load(path) as z:
            assert not set(z.files) & set(arrs), path
            arrs.update({k: z[k] for k in z.files})
    return meta, arrs


def config():
    mc, _, _ = load_case(LH.MODEL_CASES[CASE]["base"])
    return LH.model_config(mc, CASE)


def test_fixture_parts_are_complete_and_small():
    meta, arrs = load_fixture()
    parts = sorted(glob.glob(STEM + "_?.npz"))
    assert len(parts) >= 2 and [os.path.basename(p)[-5] for p in parts] == [chr(ord("a") + i) for i in range(len(parts))]
    assert all(os.path.getsize(p) <= PART_LIMIT for p in parts), [os.path.getsize(p) for p in parts]
    assert {"nodrop/" + n for n in meta["cases"]["nodrop"]["grad_stats"]} == set(arrs)
    assert meta["sample_stride"] == LH.LW.GRAD_STRIDE and meta["B"] == LH.TRAIN_C256["B"] and meta["T"] == LH.TRAIN_C256["T"]


def test_16_head_model_has_the_reference_parameters():
    mc = config()
    assert mc["n_head"] == 16 and mc["fuse_head"] == 16 and mc["embd_dim"] // mc["n_head"] == 32
    meta, _ = load_fixture()
    assert [(k, list(s)) for k, s in meta["state_keys"]] == model_keys(mc)


def test_training_step_16_heads_matches_reference():
    """As test_local_heads_cpu.test_training_step_width_256_matches_reference, at width 512 with 16 heads."""
    from golden_cases import compare_grads, replay_matching, train_batch
    from vrdone_amd.models.maskvrd import MaskVRD
    mc = config()
    sd = O.synth_state_dict(model_keys(mc), eos_coef=mc["loss_coeff_dict"]["eos_coef"])
    meta, gt = load_fixture()
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
    # (the key branches' biases: mathematically zero gradients, see the test this mirrors)
    zero = [n for n in names if re.search(r"\.key(_norm)?\.bias$", n)]
    assert zero and len(zero) < len(names) // 8
    compare_grads([(n, leaves[n].grad) for n in names if n not in zero], gt, meta, "nodrop", rtol=1e-3, median_tol=2e-5)
    stats = meta["cases"]["nodrop"]["grad_stats"]
    biggest = max(v[2] for v in stats.values())
    for n in zero:
        assert float(leaves[n].grad.double().norm()) <= 1e-5 * biggest and stats[n][2] <= 1e-5 * biggest, n
