"""Training in the row space, the parts that need no GPU: the new entry points are declared, bound and exported under the unchanged
ABI version; the training plan of the four golden length lists gives the bucket tables of the issue; a layout maps its sequences
back to batch positions (stochastic depth), both halves."""
import json
import os
import re
import subprocess

import pytest
import torch

from conftest import GOLDEN, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["vrd_local_attn_bwd_segs", "vrd_dwconv_bwd_segs", "vrd_dwconv_wgrad_segs", "vrd_maxpool_bwd_segs"]


def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "vrdone_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define VRD_ABI_VERSION 37\b", header)
    from vrdone_amd import _hip
    assert _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    exported = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/vrdone_hip.h"
        assert name in _hip._SIGNATURES and getattr(_hip.lib, name).argtypes == _hip._SIGNATURES[name][1]
        assert re.search(r" T " + name + r"$", exported, re.M), f"{name} is not exported"
    # the row groups travel as a pointer to the host-side table, like the forward entry points'
    for name in ENTRY_POINTS:
        assert any(a is _hip.C.POINTER(_hip.RowSegs) for a in _hip._SIGNATURES[name][1])
    # the existing struct kept its fields: the row groups are an argument of their own
    assert [f[0] for f in _hip.DwconvBwdArgs._fields_] == ["dD", "lddd", "w", "n_out", "B", "Tin", "C", "ksize", "stride", "group_in", "mask_out",
                                                            "dx", "lddx", "dx_up", "lddx_up"]


def model_of(name):
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, _ = load_case(name)
    return MaskVRD(mc, device="cpu")


@pytest.mark.parametrize("name,table", [
    ("vidvrd", [(6, 32), (8, 64), (10, 96)]),
    ("vidor", [(2, 96), (1, 128), (1, 256), (1, 288), (1, 448)]),
    ("vidor_x", [(1, 224), (1, 288), (1, 480), (1, 512)]),
    ("vidor_local", [(1, 352), (1, 448), (1, 480), (1, 512)]),
])
def test_training_plan_of_the_golden_batches(name, table):
    model = model_of(name)
    assert model.train_rows is False and model.train_form == "batch"
    assert model.TRAIN_ROWS_MIN_ROWS == 4096                         # (the measured default: profiles/train_rows_bench.json)
    with open(os.path.join(GOLDEN, f"train_step_{name}.json")) as f:
        lens = json.load(f)["lengths"]
    model.TRAIN_ROWS_MIN_ROWS = 0
    plan = model.train_rows_plan(lens)
    assert [(len(ids), t) for t, ids, _ in plan] == table
    assert sum(len(ids) * t for t, ids, _ in plan) == {"vidvrd": 1664, "vidor": 1312, "vidor_x": 1504, "vidor_local": 1792}[name]
    assert sorted(i for _, ids, _ in plan for i in ids) == list(range(len(lens)))
    down = model.scale_factor ** model.backbone_arch[-1]
    for t, ids, flat in plan:
        assert t % down == 0 and flat == all(lens[i] <= t - 2 for i in ids)
        assert all(lens[i] <= t and (t == model.max_seq_len or t // down > -(-lens[i] // down)) for i in ids)
    # a threshold hands the small buckets' pairs to the next longer bucket: in the end the longest tight length takes them all
    model.TRAIN_ROWS_MIN_ROWS = 1 << 30
    merged = model.train_rows_plan(lens)
    assert [(len(ids), t) for t, ids, _ in merged] == [(len(lens), table[-1][1])]


def test_plan_puts_pairs_without_two_padded_frames_behind_the_flat_buckets():
    model = model_of("vidvrd")
    model.TRAIN_ROWS_MIN_ROWS = 0
    plan = model.train_rows_plan([96, 10, 95, 94, 40])
    assert [(t, ids, flat) for t, ids, flat in plan] == [(32, [1], True), (64, [4], True), (96, [3], True), (96, [0, 2], False)]


def test_layout_maps_every_sequence_to_its_batch_position():
    from vrdone_amd.models import ragged
    from vrdone_amd.models.blocks import AffineDropPath
    order = [3, 0, 4, 1, 2]                                   # buckets: pairs (3, 0) at 32 frames, 4 at 64, (1, 2) at 96
    lay = ragged.Layout([(2, 32, True), (1, 64, True), (2, 96, True)]).with_order(order)
    frames = [32, 32, 64, 96, 96]
    n, rows = lay.sample_rows("cpu")
    assert n == 5 and rows.tolist() == [p for p, T in zip(order, frames) for _ in range(T)]
    # stacked halves: the batch form stacks [all subjects | all objects], object i is sample B + i
    n2, rows2 = lay.stacked().sample_rows("cpu")
    assert n2 == 10 and rows2.tolist() == rows.tolist() + [5 + p for p in rows.tolist()]
    # every pyramid level and the predictor's queries keep the positions at their own frame counts
    n8, rows8 = lay.stacked().strided(8).sample_rows("cpu")
    assert n8 == 10 and rows8.tolist() == rows2[::8].tolist()
    nq, rows_q = lay.strided(8).queries(9).sample_rows("cpu")
    assert nq == 5 and rows_q.tolist() == [p for p in order for _ in range(9)]
    # a pinned keep vector reaches sample i's rows wherever they lie
    dp = AffineDropPath(4, drop_prob=0.5).train()
    dp.keep = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0])
    with torch.enable_grad():
        got = dp.row_factors(1, lay.stacked().rows, "cpu", lay.stacked())
        batch = dp.row_factors(10, 1, "cpu")
    assert got.tolist() == batch[rows2].tolist() and set(got.tolist()) == {0.0, 2.0}
    with pytest.raises(AssertionError):
        ragged.Layout([(2, 32, True)]).sample_rows("cpu")          # a row space without batch positions cannot take per-sample factors


def test_row_space_under_autograd_is_refused_only_where_it_stays_unsupported():
    from vrdone_amd.models import ragged
    like = torch.zeros(1)
    with torch.enable_grad():
        lay = ragged.Layout([(2, 32, True), (1, 64, True)])
        assert lay.with_order([1, 2, 0]).new(8, like).shape == (1, 128, 8)
        assert lay.with_order([1, 2, 0]).stacked().strided(2).new(8, like).shape == (1, 128, 8)
        with pytest.raises(AssertionError):
            lay.new(8, like)                                       # not a training step's layout
        with pytest.raises(AssertionError):
            lay.with_refs([96, 96]).with_order([1, 2, 0]).new(8, like)          # absolute position rows keep the batch form
        x = torch.zeros(1, 128, 8, requires_grad=True)
        with pytest.raises(AssertionError):
            ragged._part(x, 0, 2, 32)                              # no operation slices a row space under autograd
        assert ragged._part(x, 0, 2, 64).shape == (2, 64, 8)       # (all rows: a view)
