"""Absolute position rows (`use_abs_pe: True`) from per-sequence tables on a real MI355X: vrd_layernorm_pos / vrd_position_rows
against vrd_layernorm fed the materialised rows (bit for bit), abs-PE models at tight padding and in the row space against the
reference's goldens and against the same batch at its own padded length, and forward_test / forward_test_videos of an abs-PE
model against a forward_test of the real reference (scripts/make_golden_abs_pe.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_case
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
LOGIT_TOL, MASK_TOL = 2e-4, 2e-3                 # tests/test_gpu_model.py: against the reference's goldens
BF16X3_TIE = {"bf16x3": 5e-6}                    # (as tests/test_gpu_model.py: ties of the reference's scores the 17-bit mode may permute)


def c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


_models = {}


def get_model(name):
    """the abs-PE variant of a shipped config (no shipped config sets the switch), synthetic weights"""
    if name not in _models:
        from vrdone_amd.models.maskvrd import MaskVRD
        mc, ic, keys = load_case(name)
        mc = dict(mc, use_abs_pe=True)
        model = MaskVRD(mc, device=DEV)
        model.load_state_dict(O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]), strict=True)
        model = model.to(DEV).eval()
        model._config_eval(ic)
        _models[name] = (model, mc, ic)
    return _models[name]


def close(got, want, atol):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, atol=atol, rtol=0)


@pytest.fixture(params=["bf16x3", "f16x3", "f32"])
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


# ------------------------------------------------------------------------------------------------ (a) the two kernels
SEGS = [(0, 2, 32), (64, 1, 64)]                # (first row, sequences, frames): rows 0 .. 127
T_REFS = (32, 96, 288)                          # the three sequences' reference lengths; table max_len 96: as is, as is, interpolated
GUARD_ROWS, GUARD_COLS = 16, 32                 # poisoned rows behind the groups, poisoned columns between the rows of a slab
POISON = -777.25
FORMATS = [("f32", False), ("bf16x3", True), ("f16x3", True)]       # f32 rows and both pair formats


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tables(C, spike=None):
    """(table of the three reference lengths one behind the other, first table row of each) from a random (1, C, 96) buffer"""
    g = torch.Generator().manual_seed(C)
    pe = torch.randn(1, C, 96, generator=g)
    if spike is not None:
        pe[0, 5, 3] = spike
    parts, first, at = [], [], 0
    for t in T_REFS:
        rows = pe if t < 96 else F.interpolate(pe, t, mode='linear', align_corners=False)
        parts.append(rows[0, :, :t].t())
        first.append(at)
        at += t
    return torch.cat(parts).contiguous().to(DEV), torch.tensor(first, dtype=torch.int32, device=DEV)


def _prefix(T, how):
    return {"T": T, "T-1": T - 1, "1": 1, "0": 0}[how]


def _case(C, segs, firsts, lens, spike=None):
    """x, LayerNorm parameters, the table, pos_first, the mask (guard rows marked valid: a kernel that touched them would show)
    and the materialised position rows of a launch over the groups `segs` followed by GUARD_ROWS rows"""
    g = torch.Generator().manual_seed(7 * C + len(segs))
    rows = max(off + n * T for off, n, T in segs) + GUARD_ROWS
    x = torch.randn(rows, C, generator=g).to(DEV)
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1.0).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)
    table, first_of = _tables(C, spike)
    first = first_of[torch.tensor(firsts)].contiguous()
    mask = torch.ones(rows, dtype=torch.bool)
    mat = torch.zeros(rows, C)
    s = 0
    for off, n, T in segs:
        for b in range(n):
            L = _prefix(T, lens[s])
            mask[off + b * T + L:off + (b + 1) * T] = False
            mat[off + b * T:off + b * T + L] = table[int(first[s]):int(first[s]) + L].cpu()
            s += 1
    return x, gamma, beta, table, first, mask.to(DEV), mat.to(DEV)


def _slab(rows, C):
    buf = torch.full((rows, C + GUARD_COLS), POISON, device=DEV)
    return buf, buf[:, :C]


LENS = [("T", "T-1", "1"), ("0", "T", "T-1"), ("1", "0", "T")]       # every prefix length, on every sequence's place in turn


@pytest.mark.parametrize("lens", LENS, ids=lambda v: "/".join(v))
@pytest.mark.parametrize("mode,pair", FORMATS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", [256, 512])
def test_layernorm_pos_and_position_rows_over_row_groups(C, relu, mode, pair, lens):
    """Two row groups, three sequences pointing into the tables of t_ref 32, 96 and 288: vrd_layernorm_pos has the bits of
    vrd_layernorm fed the materialised rows, vrd_position_rows the bits of those rows written by vrd_layernorm's store path (f32:
    the rows themselves); the guard rows behind the groups and the guard columns between the rows keep their poison.  (The issue's
    groups leave no row between them: rows 0 .. 63 and 64 .. 127.)  Tolerance 0: the arithmetic is the same."""
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(mode)
    try:
        x, gamma, beta, table, first, mask, mat = _case(C, SEGS, [0, 1, 2], lens)
        rows, live = x.shape[0], x.shape[0] - GUARD_ROWS
        want_buf, want = _slab(rows, C)
        ops.layernorm(x[:live], gamma, beta, relu=relu, post_add=mat[:live], out=want[:live], pair=pair)
        got_buf, got = _slab(rows, C)
        res = ops.layernorm_pos(x, gamma, beta, table, first, mask, segs=SEGS, relu=relu, out=got, pair=pair)
        assert isinstance(res, ops.Pair) == pair
        assert torch.equal(_bits(got_buf), _bits(want_buf))            # the rows, and the poison around them
        assert bool((got_buf[live:] == POISON).all()) and bool((got_buf[:, C:] == POISON).all())
        # the rows alone
        pos_buf, pos = _slab(rows, C)
        ops.position_rows(table, first, mask, segs=SEGS, out=pos, pair=pair)
        if pair:
            # (what the pair store makes of the materialised rows: LayerNorm of a constant row with gamma 0, beta 0 is +0, plus the row)
            ref_buf, ref = _slab(rows, C)
            zero = torch.zeros(C, device=DEV)
            ops.layernorm(torch.ones(live, C, device=DEV), zero, zero, post_add=mat[:live], out=ref[:live], pair=True)
            assert torch.equal(_bits(pos_buf), _bits(ref_buf))
            assert torch.equal(ops.Pair(pos[:live], C).float(), ops.Pair(ref[:live], C).float())
        else:
            assert torch.equal(_bits(pos[:live]), _bits(mat[:live]))
        assert bool((pos_buf[live:] == POISON).all()) and bool((pos_buf[:, C:] == POISON).all())
    finally:
        ops.set_precision(old)


@pytest.mark.parametrize("lens", LENS, ids=lambda v: "/".join(v))
@pytest.mark.parametrize("mode,pair", FORMATS)
@pytest.mark.parametrize("C", [256, 512])
def test_layernorm_pos_and_position_rows_in_the_batch_form(C, mode, pair, lens):
    """No row groups (segs NULL): B = 3 sequences of T = 64 rows pointing into the tables of t_ref 96, 288 and 288; the rows
    behind the batch and the guard columns keep their poison."""
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(mode)
    try:
        x, gamma, beta, table, first, mask, mat = _case(C, [(0, 3, 64)], [1, 2, 2], lens)
        live = 3 * 64
        want_buf, want = _slab(x.shape[0], C)
        ops.layernorm(x[:live], gamma, beta, relu=True, post_add=mat[:live], out=want[:live], pair=pair)
        got_buf, got = _slab(x.shape[0], C)
        ops.layernorm_pos(x[:live].view(3, 64, C), gamma, beta, table, first, mask[:live].view(3, 64), relu=True, out=got[:live].view(3, 64, C), pair=pair)
        assert torch.equal(_bits(got_buf), _bits(want_buf))
        assert bool((got_buf[live:] == POISON).all()) and bool((got_buf[:, C:] == POISON).all())
        pos_buf, pos = _slab(x.shape[0], C)
        ops.position_rows(table, first, mask[:live].view(3, 64), out=pos[:live].view(3, 64, C), pair=pair)
        if pair:
            ref_buf, ref = _slab(x.shape[0], C)
            zero = torch.zeros(C, device=DEV)
            ops.layernorm(torch.ones(live, C, device=DEV), zero, zero, post_add=mat[:live], out=ref[:live], pair=True)
            assert torch.equal(_bits(pos_buf), _bits(ref_buf))
        else:
            assert torch.equal(_bits(pos[:live]), _bits(mat[:live]))
        assert bool((pos_buf[live:] == POISON).all()) and bool((pos_buf[:, C:] == POISON).all())
        # the default output of position_rows: a fresh (B, T, C) tensor
        fresh = ops.position_rows(table, first, mask[:live].view(3, 64), pair=pair)
        assert torch.equal(_bits(fresh.t if pair else fresh).view(live, -1), _bits(pos[:live]).view(live, -1))
    finally:
        ops.set_precision(old)


@pytest.mark.parametrize("segs", [SEGS, None], ids=["groups", "batch"])
@pytest.mark.parametrize("C", [256, 512])
def test_a_table_entry_out_of_the_f16_range_is_reported_under_the_layernorm_tag(C, segs):
    """One table entry at 5000 on a valid frame, f16 pair rows out: tag 2 of the range flag (vrd_layernorm's), from either kernel;
    the same launch without the spike, or with the spike behind a pair's valid frames, reports nothing."""
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision("f16x3")
    try:
        flag = ops.f16_range_flag()
        groups, firsts = (SEGS, [0, 1, 2]) if segs is not None else ([(0, 3, 64)], [1, 2, 2])
        for spike, lens, want in ((5000.0, ("T", "T", "T"), 2), (None, ("T", "T", "T"), 0), (5000.0, ("1", "1", "1"), 0)):
            # (the spike sits in frame 3 of the buffer: in the tables of 32 and 96 as it is, spread over frames 8 .. 10 of 288)
            x, gamma, beta, table, first, mask, _ = _case(C, groups, firsts, lens, spike)
            live = x.shape[0] - GUARD_ROWS
            kw = dict(segs=segs) if segs is not None else dict(T=64)
            xs, ms = (x, mask) if segs is not None else (x[:live], mask[:live])
            flag.zero_()
            ops.layernorm_pos(xs, gamma, beta, table, first, ms, relu=True, pair=True, **kw)
            assert ops.f16_range_exceeded() == want
            flag.zero_()
            ops.layernorm_pos(xs, gamma, beta, table, first, ms, relu=True, pair=False, **kw)           # f32 rows have no range
            assert ops.f16_range_exceeded() == 0
            out = torch.zeros(xs.shape[0], C, device=DEV)
            ops.position_rows(table, first, ms, out=out, pair=True, **kw)
            assert ops.f16_range_exceeded() == want
            flag.zero_()
    finally:
        ops.f16_range_flag().zero_()
        ops.set_precision(old)


# ------------------------------------------------------------------------------------------------ (b) the reference's goldens
@pytest.mark.parametrize("form", ["buckets", "rows"])
@pytest.mark.parametrize("name,B,T,lens", [("vidvrd", 3, 96, [96, 50, 7]), ("vidvrd", 3, 288, [288, 201, 30]), ("vidor_x", 2, 128, [128, 77])])
def test_abs_pe_goldens_at_tight_padding(name, B, T, lens, form, precision):
    """tests/golden/abs_pe.npz (the real reference's `_mask_vrd` with `use_abs_pe: True`) with every pair computed at its tight
    length, bucket by bucket and in one row space: the position rows are those of the batch's padded length T whatever the
    bucket's.  More than one bucket: that is what an abs-PE model did not get before."""
    model, mc, _ = get_model(name)
    g = np.load(os.path.join(GOLDEN, "abs_pe.npz"))
    x, m = O.synth_pairs(B, c_in(mc), T, lens, seed=4321 + T)
    xd, md = x.to(DEV), m.to(DEV)
    try:
        model.TIGHT_MIN_ROWS = 0
        if form == "rows":
            model.ROWS_MIN_ROWS = 0
        else:
            model.row_space = False
        plan = model._tight_plan(md, md.reshape(B, T))
        assert plan is not None and len(plan["buckets"]) > 1 and plan["rows"] == (form == "rows")
        assert sorted(b.T for b in plan["buckets"]) == sorted(model.tight_len(L, T) for L in lens)
        out = model._mask_vrd(xd, md, with_aux=False)
    finally:
        for key in ("TIGHT_MIN_ROWS", "ROWS_MIN_ROWS", "row_space"):
            model.__dict__.pop(key, None)
    close(out["pred_logits"], g[f"{name}/T{T}_pred_logits"], LOGIT_TOL)
    close(out["pred_masks"], g[f"{name}/T{T}_pred_masks"], MASK_TOL)


# ------------------------------------------------------------------------------------------------ (c) tight / row space = full length
@pytest.mark.parametrize("name", ["vidvrd", "vidor_x"])
def test_abs_pe_tight_buckets_and_row_space_equal_the_full_length_run(name, precision):
    """24 pairs at T = 288: tight buckets and the row space against the same batch at its own padded length (tight_padding off).
    Tolerances of the same comparison in tests/test_gpu_model.py (test_tight_padding_gives_the_same_outputs,
    test_row_space_form_gives_the_same_outputs): 2e-5 on logits (2e-4 in bf16x3), 10 x that on mask logits; -10 on padded frames."""
    model, mc, _ = get_model(name)
    B, T = 24, 288
    gen = torch.Generator().manual_seed(377)
    lens = torch.randint(2, T - 30, (B,), generator=gen)
    lens[:8] = torch.tensor([288, 287, 2, 33, 286, 280, 96, 97])
    x, m = O.synth_pairs(B, c_in(mc), T, lens.tolist(), seed=378)
    xd, md = x.to(DEV), m.to(DEV)
    try:
        model.TIGHT_MIN_ROWS = model.ROWS_MIN_ROWS = 64
        plan = model._tight_plan(md, md.reshape(B, T))
        assert plan is not None and plan["rows"] and len(plan["buckets"]) >= 4
        rows = model._mask_vrd(xd, md)
        model.row_space = False
        plan = model._tight_plan(md.clone(), md.reshape(B, T))
        assert plan is not None and not plan["rows"] and len(plan["buckets"]) >= 4
        tight = model._mask_vrd(xd, md.clone())
        model.tight_padding = False
        full = model._mask_vrd(xd, md.clone())
    finally:
        model.tight_padding = True
        for key in ("TIGHT_MIN_ROWS", "ROWS_MIN_ROWS", "row_space"):
            model.__dict__.pop(key, None)
    tol = 2e-4 if precision == "bf16x3" else 2e-5
    pad = ~m[:, 0][:, None, :].expand(-1, full["pred_masks"].shape[1], -1)
    for got in (tight, rows):
        close(got["pred_logits"], full["pred_logits"], tol)
        close(got["pred_masks"], full["pred_masks"], 10 * tol)
        assert torch.equal(got["output_mask"], full["output_mask"]) and len(got["aux_outputs"]) == len(full["aux_outputs"]) == 3
        for a, b in zip(got["aux_outputs"], full["aux_outputs"]):
            close(a["pred_logits"], b["pred_logits"], tol)
            close(a["pred_masks"], b["pred_masks"], 10 * tol)
        assert bool((got["pred_masks"].cpu()[pad] == -10.0).all())


# ------------------------------------------------------------------------------------------------ (d) forward_test
def _on_device(data):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}


def test_abs_pe_forward_test_matches_reference_golden(precision):
    """tests/golden/forward_test_vidvrd_abs_pe.json: the real reference's forward_test with `use_abs_pe: True` on 494 pairs =
    three slices of its max_so_pair loop whose long pairs it pads to 192 / 240 / 240 frames -- all above max_seq_len, so every
    slice adds the table re-interpolated to its own length.  Here the pairs run at their tight lengths in one row space, pairs
    of different slices side by side in a bucket.  Compared like test_forward_test_many_slices_matches_reference_golden."""
    from golden_cases import SLICES, compare_forward_test
    model, mc, ic = get_model("vidvrd")
    with open(os.path.join(GOLDEN, "forward_test_vidvrd_abs_pe.json")) as f:
        ref = json.load(f)
    data = synth_proposal(c_in=c_in(mc), **SLICES)
    lens = [int(f.shape[1]) for f in data["so_features_list"]]
    assert len(data["sids"]) == ref["n_pairs"] > 2 * mc["max_so_pair"] and lens == ref["pair_lengths"]
    t_refs = model._reference_pad(lens)
    assert sorted(set(t_refs)) == sorted(set(ref["slice_t_long"] + [mc["max_seq_len"]])) and max(t_refs) > mc["max_seq_len"]
    order, t_pad = model.eval_plan(lens)
    assert model._eval_rows_form(len(lens)) and len(set(t_pad)) > 3
    assert any(len({t_refs[i] for i in range(len(lens)) if t_pad[i] == t}) > 1 for t in set(t_pad))      # reference lengths mix in a bucket
    res = model(_on_device(data))
    compare_forward_test(res, ref, ic["n_max_pair"], 5e-6, slack=0, tie_tol=BF16X3_TIE.get(precision, 0.0))
    try:                                      # ... and bucket by bucket (videos below ROWS_MIN_PAIRS pairs take this form)
        model.ROWS_MIN_PAIRS = 1 << 20
        res = model(_on_device(data))
    finally:
        del model.ROWS_MIN_PAIRS
    compare_forward_test(res, ref, ic["n_max_pair"], 5e-6, slack=0, tie_tol=BF16X3_TIE.get(precision, 0.0))


def test_abs_pe_forward_test_videos_equals_one_call_per_video(precision):
    """Two multi-slice videos whose slices have different reference lengths above max_seq_len in one call: per video what
    forward_test returns for it alone."""
    from golden_cases import SLICES
    model, mc, ic = get_model("vidvrd")
    videos = [_on_device(synth_proposal(c_in=c_in(mc), **SLICES)),
              _on_device(synth_proposal(c_in=c_in(mc), **dict(SLICES, n_tracklets=19, seed=2719, max_len=300)))]
    for v in videos:
        refs = model._reference_pad([int(f.shape[1]) for f in v["so_features_list"]])
        assert len(v["sids"]) > mc["max_so_pair"] and len({t for t in refs if t > mc["max_seq_len"]}) >= 2
    want = [model.forward_test(v) for v in videos]
    got = model.forward_test_videos(videos)
    assert len(got) == 2
    for g, w in zip(got, want):
        assert g is not None and w is not None
        for key in ("triplets", "so_tids", "pred_durations", "so_trajs", "triple_scores", "triple_scores_avg"):
            assert g[key] == w[key], key
