"""Training batches built on the device (proposals.TrainSource + train_tables -> vrd_gather_train -> MaskVRD.forward_training)
against the list form (proposals.train_getitem -> MaskVRD._train_batch -> backbone._unpack) on a real MI355X: the operand
buffers, the target masks, and whole training steps, eagerly and as HIP-graph replays."""
import random
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (frame size, trajectory intervals, [(subject, object, [relations as fractions of the shared frames])]) per video.  Sequence
# lengths at stride 1: 96, 2, 95 | 147 -> cropped to 96 (twice), 40 on an interval that starts mid-video
VIDEOS = [((320, 240), {0: [0, 130], 1: [10, 106], 2: [128, 130], 3: [5, 100]},
           [(0, 1, [(0.0, 1.0), (0.2, 0.5)]), (0, 2, [(0.0, 1.0)]), (0, 3, [(0.1, 0.9), (0.5, 1.0), (0.0, 0.3)])]),
          ((640, 360), {0: [0, 150], 1: [3, 150], 2: [20, 60]},
           [(0, 1, [(0.0, 1.0), (0.3, 0.6)]), (2, 0, [(0.25, 0.75)]), (1, 0, [(0.1, 0.8)])])]
LENS = [96, 2, 95, 96, 40, 96]
# the CLIP case: 64, 2, and 80 -> cropped to 64
CLIP_VIDEO = [((320, 240), {0: [0, 90], 1: [4, 68], 2: [88, 90], 3: [10, 90]},
               [(0, 1, [(0.0, 1.0), (0.2, 0.5)]), (0, 2, [(0.0, 1.0)]), (3, 0, [(0.1, 0.9)])])]


def _entries(V, Cc=0, scale=1.0, seed=3, videos=VIDEOS):
    """Cache entries (the dict of proposals.load_train_video) of `videos`, trajectory lengths times `scale`."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (w, h), spans, keys in videos:
        spans = {t: [[int(a * scale), max(int(b * scale), int(a * scale) + 2)]] for t, (a, b) in spans.items()}
        e = {"video_hw": (h, w), "relation_merged": defaultdict(list), "relation_keys": [], "visual_features": {}, "entity_bboxes": {},
             "entity_classes": {t: 1 for t in spans}, "traj_intervals": spans}
        if Cc:
            e["clip_features"] = {}
        for t, ((a, b),) in spans.items():
            e["visual_features"][t] = [torch.randn(b - a, V, generator=g)]
            xy = torch.rand(b - a, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5]) - 4.0          # (some stick out: clamped)
            e["entity_bboxes"][t] = [torch.cat([xy, xy + 8 + torch.rand(b - a, 2, generator=g) * torch.tensor([w * 0.4, h * 0.4])], dim=1)]
            if Cc:
                e["clip_features"][t] = [torch.randn(b - a, Cc, generator=g)]
        for s, o, rels in keys:
            lo, hi = max(spans[s][0][0], spans[o][0][0]), min(spans[s][0][1], spans[o][0][1])
            for k, (fa, fb) in enumerate(rels):
                e["relation_merged"][(s, o, 0, 0)].append({"predicate": 1 + (3 * s + o + k) % 50, "begin_fid": lo + int(fa * (hi - lo)),
                                                           "end_fid": lo + max(int(fb * (hi - lo)), int(fa * (hi - lo)) + 1)})
            e["relation_keys"].append([s, o, 0, 0])
        out.append(e)
    return out


def _feeds(entries, T, seed):
    """(lists of train_getitem, (TrainSource, TrainTables)) of one step over all entries, from equally seeded generators."""
    from vrdone_amd import proposals
    r1, r2 = random.Random(seed), random.Random(seed)
    lists = {k: [] for k in ("so_features_list", "preds_list", "masks_list", "segs_list")}
    for e in entries:
        for k, v in proposals.train_getitem(e, 1, T, rng=r1).items():
            lists[k] += v
    src = proposals.TrainSource.concat([proposals.TrainSource.from_entry(e, DEV) for e in entries])
    tables = proposals.TrainTables.concat([proposals.train_tables(v, 1, T, rng=r2) for v in src.videos])
    assert r1.getstate() == r2.getstate() and len(tables) == len(lists["so_features_list"])
    return lists, src, tables


def _model(name, **overrides):
    from vrdone_amd import configs, synth
    from vrdone_amd.models.maskvrd import MaskVRD
    cfg = dict(configs.model_config(name), **overrides)
    torch.manual_seed(0)
    return synth.load_synthetic_weights(MaskVRD(cfg, device=DEV)).to(DEV).train(), cfg


@pytest.fixture(scope="module")
def vidvrd():
    model, cfg = _model("vidvrd")
    entries = _entries(cfg["visual_dim"])
    lists, src, tables = _feeds(entries, cfg["max_seq_len"], seed=1)
    assert tables.lens.tolist() == LENS and int((tables.lead > 0).sum()) >= 1, "the fixture was meant to crop behind frame 0"
    return model, cfg, entries, lists, src, tables


def _shifted(src):
    """The same source with every array one float further into its buffer: no row is 16-byte aligned."""
    from vrdone_amd.proposals import TrainSource

    def placed(t):
        if t is None:
            return None
        buf = torch.full((t.numel() + 65,), float("nan"), device=DEV)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    return TrainSource(placed(src.vis), placed(src.clip), placed(src.boxes), src.videos)


def _raw(t):
    return t.t if hasattr(t, "t") and not torch.is_tensor(t) else t


def _check_operands(model, lists, src, tables, precision):
    """vrd_gather_train's buffers against backbone._unpack of the list form's padded batch; returns the gathered tuple."""
    from vrdone_amd import ops
    bb, T = model.backbone, model.max_seq_len
    B = len(tables)
    with torch.no_grad(), ops.use_precision(precision):
        x, m = model._train_batch([f.to(DEV) for f in lists["so_features_list"]])
        w_vis, w_clip, w_so, w_ent = bb._unpack(x)
        got = ops.gather_train(src, tables, T, bb.n_bbox_so, bb.n_bbox_entity, ops.pair_mode())
        vis, clip, so_box, ent, mask, targets = got
        assert (precision == "f32") == torch.is_tensor(vis)             # pair rows in the split-precision modes
        assert torch.equal(_raw(vis), _raw(w_vis)), "visual rows differ"
        assert (clip is None) == (w_clip is None) and (clip is None or torch.equal(_raw(clip), _raw(w_clip))), "CLIP rows differ"
        assert mask.dtype == torch.bool and torch.equal(mask, m[:, 0])
        # the bound of tests/test_gpu_model.py::test_gather_pairs_matches_the_reference_dataloader: everything but the three
        # logarithms bit-equal to the host formulas, those within 2e-6
        d_log = float((so_box[..., 2:] - w_so[..., 2:]).abs().max())
        print(f"[{precision}] box features: max |device log - host log| = {d_log:.3e}, bit-equal: {torch.equal(so_box, w_so)}")
        assert torch.equal(so_box[..., :2], w_so[..., :2]) and torch.equal(ent, w_ent)
        np.testing.assert_allclose(so_box[..., 2:].cpu().numpy(), w_so[..., 2:].cpu().numpy(), rtol=0, atol=2e-6)
        for p, L in enumerate(tables.lens.tolist()):                    # padded frames are exactly zero
            for buf in (_raw(vis)[p, L:], _raw(vis)[B + p, L:], so_box[p, L:], ent[p, L:], ent[B + p, L:]) + \
                    (() if clip is None else (_raw(clip)[p, L:], _raw(clip)[B + p, L:])):
                assert not bool(buf.any())
        assert torch.equal(targets, torch.cat(lists["masks_list"]).to(DEV)), "target masks differ"
        # ... and the same bits from rows that are not 16-byte aligned (the scalar-load form)
        again = ops.gather_train(_shifted(src), tables, T, bb.n_bbox_so, bb.n_bbox_entity, ops.pair_mode())
        for a, b in zip(got, again):
            assert (a is None and b is None) or torch.equal(_raw(a), _raw(b)), "unaligned source rows give other bits"
    return got


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_operand_buffers_and_targets_match_the_list_form(vidvrd, precision):
    model, cfg, entries, lists, src, tables = vidvrd
    _check_operands(model, lists, src, tables, precision)


def test_narrow_rows_take_the_scalar_form():
    """Feature widths that are no multiple of 4 (no float4 shape): the same rows, through the kernel's scalar form."""
    from vrdone_amd import ops
    entries = _entries(18, Cc=6, scale=0.25)
    T = 32
    lists, src, tables = _feeds(entries, T, seed=2)
    vis, clip, so_box, ent, mask, targets = ops.gather_train(src, tables, T, 5, 8, False)
    B = len(tables)
    for p, f in enumerate(lists["so_features_list"]):
        L, ft = f.shape[1], f.T.contiguous().to(DEV)
        assert torch.equal(vis[p, :L], ft[:, :18]) and torch.equal(vis[B + p, :L], ft[:, 18:36])
        assert torch.equal(clip[p, :L], ft[:, 36:42]) and torch.equal(clip[B + p, :L], ft[:, 42:48])
        assert torch.equal(ent[p, :L], ft[:, 53:61]) and torch.equal(ent[B + p, :L], ft[:, 61:69])
        assert not bool(vis[p, L:].any()) and not bool(clip[B + p, L:].any()) and mask[p].sum().item() == L
    assert torch.equal(targets, torch.cat(lists["masks_list"]).to(DEV))


def test_f16_range_flag_reports_from_the_gather(vidvrd):
    """A feature beyond the f16 operand range in a gathered row sets tag 1 (boundary tensors) when the gather writes f16 planes."""
    from vrdone_amd import ops
    from vrdone_amd.proposals import TrainSource
    model, cfg, entries, lists, src, tables = vidvrd
    bb, T = model.backbone, model.max_seq_len
    flag = ops.f16_range_flag(DEV)
    hot = TrainSource(src.vis.clone(), None, src.boxes, src.videos)
    hot.vis[int(tables.o_row[2]) + 7, 513] = 5000.0
    with torch.no_grad(), ops.use_precision("f16x3"):
        for source, want in ((src, 0), (hot, 1)):
            flag.zero_()
            ops.gather_train(source, tables, T, bb.n_bbox_so, bb.n_bbox_entity, True)
            assert int(flag.item()) == want
    flag.zero_()


def _step(model, data, seed=5):
    """One deterministic forward + backward: (loss dict as floats, gradients by parameter name)."""
    torch.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        losses = model(data)
        losses["total_loss"].backward()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().tobytes() for k, v in losses.items()}, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _with_device_boxes(lists, got):
    """The list form's features with their 21 box channels replaced by the ones vrd_gather_train computed."""
    _, _, so_box, ent, _, _ = got
    B = so_box.shape[0]
    feats = []
    for p, f in enumerate(lists["so_features_list"]):
        f, L = f.to(DEV).clone(), f.shape[1]
        f[-21:-16] = so_box[p, :L].T
        f[-16:-8] = ent[p, :L].T
        f[-8:] = ent[B + p, :L].T
        feats.append(f)
    return dict({k: [t.to(DEV) for t in v] for k, v in lists.items()}, so_features_list=feats)


def _assert_same_step(a, b, what):
    assert a[0].keys() == b[0].keys() and all(a[0][k] == b[0][k] for k in a[0]), f"{what}: loss dicts differ"
    assert a[1].keys() == b[1].keys()
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), f"{what}: .grad of {n} differs"


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_training_step_from_the_source_is_the_list_forms_step(vidvrd, precision):
    """Deterministic mode, one step (stochastic depth on): forward_training from {'train_source', 'train_tables'} gives the loss
    dict and every parameter's .grad of the list form, bit for bit -- eagerly, and as HIP-graph replays over two steps with
    different tables (the second step's gather rewrites the recording's input buffers).

    The three logarithmic box channels of the device gather may differ from torch.log on the host in the last bit (the bound of
    the eval gather's test: 2e-6; measured 4.8e-7, not bit-equal; the run prints the figure), so the list form is fed the device-built 21 box channels here:
    every other channel, the masks, the targets and the whole network must then agree exactly."""
    from vrdone_amd import ops, train_graph
    model, cfg, entries, lists, src, tables = vidvrd
    T = cfg["max_seq_len"]
    lists2, src2, tables2 = _feeds(entries, T, seed=8)
    assert tables2.lens.tolist() == LENS and tables2.s_row.tolist() != tables.s_row.tolist(), "the second step was meant to crop elsewhere"
    with ops.use_precision(precision), ops.use_deterministic(True):
        want = []
        for ls, s, t in ((lists, src, tables), (lists2, src2, tables2)):
            with torch.no_grad():
                got = ops.gather_train(s, t, T, 5, 8, False)
            want.append(_step(model, _with_device_boxes(ls, got)))
        assert any(not torch.equal(a, b) for a, b in zip(want[0][1].values(), want[1][1].values()))
        for k, (s, t) in enumerate(((src, tables), (src2, tables2))):
            _assert_same_step(_step(model, {"train_source": s, "train_tables": t}), want[k], f"eager step {k}")
        try:
            model.enable_training_graphs()
            for k, (s, t) in enumerate(((src, tables), (src2, tables2))):
                _assert_same_step(_step(model, {"train_source": s, "train_tables": t}), want[k], f"graph-replayed step {k}")
            assert len(train_graph.recordings(model)) == 1          # the second step replayed the first one's recording
        finally:
            model.enable_training_graphs(False)
            train_graph.forget(model)
            model.zero_grad(set_to_none=True)


def test_forward_loss_from_the_source(vidvrd):
    """The validation loss (torch.no_grad(): fused inference kernels, pair rows written by the gather in the f16x3 mode) from
    the source equals the list form's at the same padded length."""
    from vrdone_amd import ops
    model, cfg, entries, lists, src, tables = vidvrd
    with ops.use_precision("f16x3"), torch.no_grad():
        got = ops.gather_train(src, tables, cfg["max_seq_len"], 5, 8, False)
        try:
            model.tight_padding = False                 # (the list form would otherwise run every pair at its own tight length)
            want = model.forward_loss(_with_device_boxes(lists, got))
        finally:
            del model.tight_padding
        have = model.forward_loss({"train_source": src, "train_tables": tables})
    assert want.keys() == have.keys()
    for k in want:
        assert torch.equal(want[k], have[k]), k


def test_clip_features_and_a_step_of_the_clip_model():
    """The vidor_x model (visual + CLIP rows) at max_seq_len 64, the shortest its window / pyramid divisibility allows, 3 keys."""
    from vrdone_amd import ops
    model, cfg = _model("vidor_x", max_seq_len=64)
    entries = _entries(cfg["visual_dim"], Cc=cfg["clip_dim"], videos=CLIP_VIDEO)
    lists, src, tables = _feeds(entries, 64, seed=4)
    assert src.n_clip == cfg["clip_dim"] and tables.lens.tolist() == [64, 2, 64] and int(tables.lead[2]) > 0
    got = _check_operands(model, lists, src, tables, "f32")
    with ops.use_precision("f32"), ops.use_deterministic(True):
        _assert_same_step(_step(model, {"train_source": src, "train_tables": tables}), _step(model, _with_device_boxes(lists, got)), "CLIP step")


def test_the_list_keys_are_not_needed(vidvrd):
    """forward_training reads nothing but the source and the tables (before the feature this call raised KeyError)."""
    model, cfg, entries, lists, src, tables = vidvrd
    with torch.no_grad():
        out = model({"train_source": src, "train_tables": tables})
    assert np.isfinite(float(out["total_loss"]))
