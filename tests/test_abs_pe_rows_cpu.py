"""Host side of absolute position rows at tight padding and in the row space (`use_abs_pe: True`): the per-reference-length
position tables (backbones.position_table / position_plan / position_operands), the layouts that carry the pairs' reference
lengths (ragged.Layout.with_refs), the tight-padding plan of such a model, and the C interface.  No GPU."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, load_case
from vrdone_amd.models import eval_batches as E
from vrdone_amd.models import ragged
from vrdone_amd.models.eval_batches import Bucket

torch.set_grad_enabled(False)


def _model(name="vidvrd", abs_pe=True):
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, _ = load_case(name)
    return MaskVRD(dict(mc, use_abs_pe=abs_pe), device="cpu").eval(), mc


def _reference_table(pe, max_len, t_ref):
    """reference models/backbones.py:187-196 for a batch padded to t_ref frames, as (t_ref, D) rows"""
    if t_ref >= max_len:
        pe = F.interpolate(pe, t_ref, mode='linear', align_corners=False)
    return pe[0, :, :t_ref].t()


def test_position_table_is_the_reference_formula_below_at_and_above_max_len():
    model, mc = _model()
    bb, L = model.backbone, mc["max_seq_len"]
    pe = bb.pos_embd
    assert pe.shape == (1, mc["embd_dim"], L)
    for t_ref in (1, L // 2, L - 1, L, L + 1, L + 48, 2 * L, 3 * L, 3 * L + 16):
        got = bb.position_table(t_ref)
        assert got.shape == (t_ref, mc["embd_dim"]) and got.dtype == torch.float32 and got.is_contiguous()
        assert torch.equal(got, _reference_table(pe, L, t_ref)), t_ref
        assert bb.position_table(t_ref) is got                       # kept per t_ref
    # at max_len the interpolation is the identity: the training path (table as is) and the eval path agree there
    assert torch.equal(bb.position_table(L), pe[0].t())
    # the rows a pair receives do not depend on the length it is computed at: frame t gets row t of its reference length's table
    m = torch.zeros(2, L, dtype=torch.bool)
    m[0, :L], m[1, :7] = True, True
    rows = bb._position_rows(m).view(2, L, -1)
    assert torch.equal(rows[0], bb.position_table(L)) and torch.equal(rows[1, :7], bb.position_table(L)[:7]) and not rows[1, 7:].any()


def test_position_tables_follow_the_buffer_they_were_built_from():
    model, mc = _model()
    bb, L = model.backbone, mc["max_seq_len"]
    a, a2 = bb.position_table(L // 2), bb.position_table(2 * L)
    a_was, a2_was = a.clone(), a2.clone()                           # (a table below max_len may be a view of the buffer)
    plan = bb.position_plan([L, 2 * L])
    bb.pos_embd.mul_(2.0)                                           # same storage, new version
    b, b2 = bb.position_table(L // 2), bb.position_table(2 * L)
    assert b is not a and torch.equal(b, 2.0 * a_was)
    assert b2 is not a2 and torch.equal(b2, _reference_table(bb.pos_embd, L, 2 * L)) and torch.allclose(b2, 2.0 * a2_was, rtol=1e-6, atol=0)
    assert bb.position_plan([L, 2 * L]) is not plan and torch.equal(bb.position_plan([L, 2 * L])[0][L:], b2)
    bb.pos_embd = bb.pos_embd.clone()                               # other storage
    assert bb.position_table(L // 2) is not b and torch.equal(bb.position_table(L // 2), b)


def test_tight_plan_of_an_abs_pe_model():
    """An abs-PE model shortens its pairs like any other (this failed while position rows were tied to the launch's length)."""
    model, mc = _model()
    plain, _ = _model(abs_pe=False)
    assert model.use_abs_pe and mc["max_seq_len"] == 96
    assert model.tight_len(30, 288) == 64 and model.tight_len(201, 288) == 224
    for L, T in ((30, 288), (201, 288), (288, 288), (287, 288), (2, 96), (7, 96), (50, 96), (95, 96), (100, 144), (33, 240)):
        assert model.tight_len(L, T) == plain.tight_len(L, T)
    for n in (0, 1, model.ROWS_MIN_PAIRS - 1, model.ROWS_MIN_PAIRS, model.ROWS_MIN_PAIRS + 1, 5000):
        assert model._eval_rows_form(n) == plain._eval_rows_form(n) == (n >= model.ROWS_MIN_PAIRS)
    model.ROWS_MIN_PAIRS = 8
    assert model._eval_rows_form(8) and not model._eval_rows_form(7)
    model.row_space = False
    assert not model._eval_rows_form(5000)
    # forward_test's plan: the same buckets as a model without position rows, and entity rows are never shared per tracklet
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(2, 400, (300,), generator=g).tolist()
    model.row_space = True
    for m in (model, plain):
        m.ROWS_MIN_PAIRS, m.ROWS_MIN_ROWS = 8, 2048
    assert model.eval_plan(lens) == plain.eval_plan(lens) and len(set(model.eval_plan(lens)[1])) > 2
    assert model.backbone.entity_reach() is None and plain.backbone.entity_reach() is not None


def test_mask_vrd_tight_plan_has_buckets_for_an_abs_pe_model():
    model, _ = _model()
    model.TIGHT_MIN_ROWS = model.ROWS_MIN_ROWS = 0
    lens = [288, 201, 30]
    m = (torch.arange(288)[None] < torch.tensor(lens)[:, None])[:, None]
    for rows in (True, False):
        model.row_space = rows
        plan = model._tight_plan(m, m.reshape(3, 288))
        assert plan is not None and plan["rows"] == rows and sorted(b.T for b in plan["buckets"]) == [64, 224, 288]
        m = m.clone()                                               # (the plan is kept on the mask tensor)


def test_pos_first_bookkeeping_with_two_reference_lengths():
    """One buffer for the tables of a call's distinct reference lengths, and per sequence the first row of its length's table."""
    model, mc = _model()
    bb = model.backbone
    refs = [96, 192, 96, 96, 192, 96]
    table, first = bb.position_plan(refs)
    assert table.shape == (96 + 192, mc["embd_dim"]) and table.is_contiguous()
    assert first.dtype == torch.int32 and first.tolist() == [0, 96, 0, 0, 96, 0]
    assert torch.equal(table[:96], bb.position_table(96)) and torch.equal(table[96:], bb.position_table(192))
    assert bb.position_plan(refs)[0] is table                       # kept: a video's plan repeats from call to call
    one_table, zeros = bb.position_plan([192] * 5)
    assert one_table is bb.position_table(192) and zeros.tolist() == [0] * 5
    # a stacked row space: the sequences in row order, subject and object sequences sharing their pair's entry
    lay = ragged.Layout([(2, 32, True), (3, 64, True), (1, 96, False)]).with_refs([96, (96, 240, 192), 96])
    assert lay.seq_refs() == [96, 96, 96, 240, 192, 96]
    st = lay.stacked()
    assert st.segs == lay.twice() and st.seq_refs() == lay.seq_refs() * 2
    table, first = bb.position_operands(st)
    assert table.shape[0] == 96 + 192 + 240
    start = {96: 0, 192: 96, 240: 96 + 192}
    assert first.tolist() == [start[r] for r in lay.seq_refs()] * 2
    for s, r in enumerate(st.seq_refs()):
        assert torch.equal(table[int(first[s]):int(first[s]) + r], bb.position_table(r))
    assert bb.position_operands(st) == (table, first) and bb.position_operands(st)[1] is first
    # the batch form: 2B sequences, one entry per pair repeated for the object half; without lengths, the sequences' own
    b = ragged.Layout.batch(3, 64).with_refs([(96, 192, 96)]).stacked()
    assert b.axis == 0 and b.segs == [(0, 6, 64)] and b.seq_refs() == [96, 192, 96] * 2
    assert ragged.Layout.batch(6, 64).t_refs is None and ragged.Layout.batch(6, 64).seq_refs() is None     # (the cached layouts stay bare)
    table, first = bb.position_operands(ragged.Layout.batch(4, 128))
    assert table is bb.position_table(128) and first.tolist() == [0] * 4
    with pytest.raises(AssertionError):                             # a pair is never computed at more frames than its reference length
        bb.position_operands(ragged.Layout.batch(2, 128).with_refs([96]))
    with pytest.raises(AssertionError):
        ragged.Layout([(2, 32, True)]).with_refs([(96,)])


def test_position_launches_cover_every_sequence_once():
    """One launch for one group of sequences (the two halves of a bucket merge), else row groups in runs of 32 with the sequences
    counted through."""
    assert ragged._pos_launches(ragged.Layout.batch(6, 64)) == [(None, 64, 0, 6)]
    assert ragged._pos_launches(ragged.Layout([(5, 32, True)]).stacked()) == [(None, 32, 0, 10)]
    lay = ragged.Layout([(1 + i % 3, 32 * (1 + i // 2), True) for i in range(20)]).stacked()
    got = ragged._pos_launches(lay)
    assert [len(segs) for segs, _, _, _ in got] == [32, 8] and all(T is None for _, T, _, _ in got)
    assert [seg for segs, _, _, _ in got for seg in segs] == lay.segs
    at = 0
    for segs, _, s0, n in got:
        assert s0 == at and n == sum(k for _, k, _ in segs)
        at += n
    assert at == len(lay.with_refs([96 * 8] * 40).seq_refs())


def test_sources_hand_their_buckets_the_pairs_reference_lengths():
    src = E.Source()
    assert src.refs_of(Bucket(64, range(0, 3), 3, True)) is None
    src.refs = [96, 96, 96, 192, 240, 192]
    assert src.refs_of(Bucket(64, range(0, 3), 3, True)) == 96
    assert src.refs_of(Bucket(64, range(2, 5), 3, True)) == (96, 192, 240)
    assert src.refs_of(Bucket(32, None, 4, True)) is None            # a filler bucket
    (piece,), = E.waves([Bucket(64, range(1, 6), 5, False)], 8)
    assert src.refs_of(piece) == (96, 96, 192, 240, 192)


def test_the_two_entry_points_are_declared_bound_and_exported():
    from vrdone_amd import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vrdone_hip.h")).read(), flags=re.S)
    assert "#define VRD_ABI_VERSION 37" in header and _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    for name, n_args in (("vrd_layernorm_pos", 18), ("vrd_position_rows", 13)):
        proto = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto is not None, name
        assert len(proto.group(1).split(",")) == n_args == len(_hip._SIGNATURES[name][1])
        assert "const vrd_row_segs* segs" in proto.group(1) and "const int32_t* pos_first" in proto.group(1)
        assert hasattr(_hip.lib, name)
    # refused on the host, before any launch: null pointers, widths, a misaligned table, groups outside the rows
    lib = _hip.lib
    assert lib.vrd_position_rows(None, 256, 64, 256, 16, 256, 96, 16, 16, None, 32, 0, None) == -1
    assert lib.vrd_position_rows(16, 256, 64, 128, 16, 256, 96, 16, 16, None, 32, 0, None) == -1 and b"C must be" in lib.vrd_last_error()
    assert lib.vrd_position_rows(16, 256, 64, 256, 20, 256, 96, 16, 16, None, 32, 0, None) == -1 and b"position table" in lib.vrd_last_error()
    assert lib.vrd_position_rows(16, 256, 64, 256, 16, 256, 96, 16, 16, None, 48, 0, None) == -1 and b"row groups" in lib.vrd_last_error()
    import ctypes as C
    segs = _hip.RowSegs.of([(0, 2, 32), (64, 1, 64)])
    assert lib.vrd_position_rows(16, 256, 127, 256, 16, 256, 96, 16, 16, C.pointer(segs), 0, 0, None) == -1 and b"row groups" in lib.vrd_last_error()
    assert lib.vrd_layernorm_pos(16, 256, 16, 256, 127, 256, 16, 16, 1, 16, 256, 96, 16, 16, C.pointer(segs), 0, 0, None) == -1
    assert b"row groups" in lib.vrd_last_error()
    assert lib.vrd_layernorm_pos(16, 256, 16, 256, 128, 256, 16, 16, 1, 16, 256, 96, None, 16, C.pointer(segs), 0, 0, None) == -1
    assert lib.vrd_layernorm_pos(16, 256, 16, 256, 128, 256, 16, 16, 1, 16, 256, 96, 16, 16, None, 32, 7, None) == -1 and b"out_pair" in lib.vrd_last_error()


def test_padded_source_runs_a_batch_per_reference_length_and_keeps_the_pair_order():
    """Channel-major features go through _mask_vrd, which takes ONE reference length per batch: a bucket whose pairs come from
    slices of different padded lengths is split by that length and put back together in the bucket's own order."""
    calls = []

    class Model:
        def _batch(self, feats, ids, T):
            return torch.tensor([float(feats[i]) for i in ids]), T

        def _mask_vrd(self, x, m, with_aux=None, t_ref=None):
            calls.append((x.tolist(), m, t_ref))
            return {"pred_logits": x[:, None] * 10.0, "pred_masks": x[:, None, None] + 0.5, "output_mask": None}

    src = E.Padded(Model(), [100 + p for p in range(8)])
    b = Bucket(64, range(2, 7), 5, False)
    out = src.outputs(b)                                            # a model without position rows: one batch, no length
    assert calls == [([102.0, 103.0, 104.0, 105.0, 106.0], 64, None)] and out["pred_logits"][:, 0].tolist() == [1020.0, 1030.0, 1040.0, 1050.0, 1060.0]
    del calls[:]
    src.refs = [96, 96, 240, 192, 240, 192, 192, 96]
    out = src.outputs(b)
    assert calls == [([102.0, 104.0], 64, 240), ([103.0, 105.0, 106.0], 64, 192)]
    assert out["pred_logits"][:, 0].tolist() == [1020.0, 1030.0, 1040.0, 1050.0, 1060.0]
    assert out["pred_masks"][:, 0, 0].tolist() == [102.5, 103.5, 104.5, 105.5, 106.5]
    del calls[:]
    src.outputs(Bucket(64, range(0, 2), 2, True))                   # one length in the bucket: one batch at that length
    assert calls == [([100.0, 101.0], 64, 96)]
