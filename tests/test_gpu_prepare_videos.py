"""vrdone_amd.proposals.prepare_test_videos on the MI355X: the eval proposals of many videos prepared in one call (box clamp,
tracklet de-dup, pair tables; csrc/vrd_proposals.hip) against the host path prepare_test_proposal -- the parent's code,
unchanged -- and, for the de-dup alone, oracle.proposal.dedup_tracklets.  Visual width 8 wherever the features do not matter."""
import numpy as np
import pytest
import torch

from golden_cases import PROPOSAL_CASES
from oracle import proposal as OP

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
V = 8


# --------------------------------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------------------------------
def host_proposals(raws, stride, offsets, min_frames, threshold=0.9):
    from vrdone_amd.proposals import prepare_test_proposal
    offsets = [offsets] * len(raws) if isinstance(offsets, int) else offsets
    return [prepare_test_proposal(r, stride, off, min_frames, "cpu", threshold) if r else {} for r, off in zip(raws, offsets)]


def assert_same_proposal(got, want, what=""):
    """One video's device-prepared proposal against the host path's: every field of the dict and of its pair source."""
    assert bool(got) == bool(want), f"{what}: {'no' if not got else 'a'} proposal where the host path has {'one' if want else 'none'}"
    if not want:
        assert got == {}
        return
    assert set(got) == set(want), what
    for k in ("sids", "oids", "so_offset", "cat_ids", "cat_scores", "traj_durations"):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f"{what}: {k}"
    assert len(got["bboxes_list"]) == len(want["bboxes_list"])
    for k, (a, b) in enumerate(zip(got["bboxes_list"], want["bboxes_list"])):
        assert a.device.type == "cpu" and torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: bboxes_list[{k}]"
    g, w = got["pair_source"], want["pair_source"]
    assert g.boxes.is_cuda and g.vis.is_cuda and g.s_row.is_cuda
    # the device's clamped boxes: bit-equal to the host list and to the host path's array
    assert torch.equal(g.boxes.cpu().view(torch.int32), torch.cat(got["bboxes_list"]).view(torch.int32)), f"{what}: device boxes"
    for name in ("vis", "clip", "boxes", "s_row", "o_row", "lens_dev"):
        a, b = getattr(g, name), getattr(w, name)
        assert (a is None) == (b is None), f"{what}: {name}"
        if b is not None:
            assert a.dtype == b.dtype and a.is_contiguous() and torch.equal(a.cpu(), b), f"{what}: {name}"
    assert g.lens == w.lens and g.stride == w.stride and g.wh == w.wh and (g.n_visual, g.n_clip) == (w.n_visual, w.n_clip), what
    assert g.first_row.dtype == w.first_row.dtype and g.first_row.tolist() == w.first_row.tolist(), f"{what}: first_row"
    ids = np.arange(len(g))
    for a, b in zip(g.stream_plan(ids), w.stream_plan(ids)):          # (the host copies of the row tables a consumer plans with)
        assert np.array_equal(a, b), f"{what}: stream_plan"


def assert_same_call(raws, stride, offsets, min_frames, threshold=0.9):
    from vrdone_amd.proposals import prepare_test_videos
    got = prepare_test_videos(raws, stride, offsets, min_frames, DEV, threshold)
    want = host_proposals(raws, stride, offsets, min_frames, threshold)
    assert len(got) == len(raws)
    for v, (g, w) in enumerate(zip(got, want)):
        assert_same_proposal(g, w, f"video {v}")
    return got, want


def video(tracks, wh=(640, 480), cats=None, pairs=None, seed=0):
    """A raw video from [(first frame, (frames, 4) boxes)]: one category unless `cats` says otherwise, every ordered pair of
    tracklets that share a frame unless `pairs` lists the candidates."""
    g = torch.Generator().manual_seed(seed)
    spans = [(a, a + len(b)) for a, b in tracks]
    n = len(tracks)
    if pairs is None:
        pairs = [(s, o) for s in range(n) for o in range(n) if s != o and min(spans[s][1], spans[o][1]) > max(spans[s][0], spans[o][0])]
    return {"sids": torch.tensor([p[0] for p in pairs], dtype=torch.int64), "oids": torch.tensor([p[1] for p in pairs], dtype=torch.int64),
            "cat_ids": torch.tensor(cats if cats is not None else [3] * n), "cat_scores": torch.rand(n, generator=g),
            "bboxes_list": [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4).clone() for _, b in tracks],
            "traj_durations": torch.tensor(spans, dtype=torch.int64),
            "visual_features_list": [torch.randn(e - a, V, generator=g) for a, e in spans], "video_wh": wh}


def still(frames, box):
    return torch.tensor([box], dtype=torch.float32).repeat(frames, 1)


def host_drops(raw, threshold=0.9):
    """The drop set of the host path, checked against the oracle's restatement of the reference loop."""
    from vrdone_amd.proposals import _clamped, shadowed_tracklets
    w, h = raw["video_wh"]
    boxes = [_clamped(b, w, h) for b in raw["bboxes_list"]]
    spans = [tuple(s) for s in raw["traj_durations"].tolist()]
    gone = shadowed_tracklets(boxes, spans, raw["cat_ids"].tolist(), threshold)
    kept = OP.dedup_tracklets(boxes, raw["traj_durations"], raw["cat_ids"], threshold)
    assert sorted(set(range(len(boxes))) - set(kept)) == gone
    return gone


def device_drops(raws, threshold=0.9, stride=1, offsets=0, min_frames=2):
    from vrdone_amd.proposals import run_proposal_kernels
    run = run_proposal_kernels(raws, stride, offsets, min_frames, DEV, threshold)
    gone, first = run.dev["dropped"].cpu().numpy(), run.packed.tables["trk_first"]
    assert set(np.unique(gone).tolist()) <= {0, 1}
    return [np.nonzero(gone[first[v]:first[v + 1]])[0].tolist() for v in range(len(raws))]


def pair_ratios(raw):
    """inter / area_j and inter / area_i of every tracklet pair the de-dup compares (same category, a shared frame), as the host
    forms them."""
    from vrdone_amd.proposals import _clamped
    w, h = raw["video_wh"]
    boxes = [_clamped(b, w, h) for b in raw["bboxes_list"]]
    spans, cats, out = raw["traj_durations"].tolist(), raw["cat_ids"].tolist(), []
    for i in range(len(boxes)):
        for j in range(i + 1, len(boxes)):
            lo, hi = max(spans[i][0], spans[j][0]), min(spans[i][1], spans[j][1])
            if cats[i] != cats[j] or hi <= lo:
                continue
            bi, bj = boxes[i][lo - spans[i][0]:hi - spans[i][0]], boxes[j][lo - spans[j][0]:hi - spans[j][0]]
            wh = (torch.minimum(bi[:, 2:], bj[:, 2:]) - torch.maximum(bi[:, :2], bj[:, :2]) + 1).clamp_(min=0)
            terms = [wh[:, 0] * wh[:, 1], (bi[:, 2] - bi[:, 0] + 1).mul(bi[:, 3] - bi[:, 1] + 1), (bj[:, 2] - bj[:, 0] + 1).mul(bj[:, 3] - bj[:, 1] + 1)]
            out.append({"pair": (i, j), "f32": [float(t.sum()) for t in terms], "f64": [float(t.double().sum()) for t in terms]})
    return out


# --------------------------------------------------------------------------------------------------------------------
# 1. the reference dataloader's goldens
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROPOSAL_CASES))
def test_reference_goldens(name, golden_dir):
    vid_kw, dl_kw = PROPOSAL_CASES[name]
    raw = OP.synth_raw_video(**vid_kw)                                  # (the golden's own widths: its draws depend on them)
    assert host_drops(raw) == [1]                                       # the case's shadowed tracklet
    got, _ = assert_same_call([raw], dl_kw["feat_stride"], dl_kw["stride_offset"], dl_kw["proposal_min_frames"])
    g = np.load(f"{golden_dir}/proposal.npz")
    got = got[0]
    assert got["sids"].tolist() == g[f"{name}/sids"].tolist() and got["oids"].tolist() == g[f"{name}/oids"].tolist()
    assert got["so_offset"].tolist() == g[f"{name}/so_offset"].tolist()
    assert got["pair_source"].lens == g[f"{name}/lens"].tolist() == got["pair_source"].lens_dev.tolist()
    np.testing.assert_array_equal(got["pair_source"].boxes.cpu().numpy().view(np.int32), g[f"{name}/boxes_clamped"].view(np.int32))
    np.testing.assert_array_equal(torch.cat(got["bboxes_list"]).numpy().view(np.int32), g[f"{name}/boxes_clamped"].view(np.int32))


# --------------------------------------------------------------------------------------------------------------------
# 2. many videos in one call
# --------------------------------------------------------------------------------------------------------------------
def many_videos(n_visual=V, n_clip=0, big=True):
    """Six raws: 2 tracklets (no pair long enough), {}, 3, 5 + 3 shadowed copies, 12 (> 64 candidates), 34 (> 1024 candidates)."""
    from vrdone_amd.synth import synth_raw_video
    kw = dict(n_visual=n_visual, n_clip=n_clip)
    raws = [synth_raw_video(2, min_len=3, max_len=3, seed=31, wh=(320, 240), **kw), {},
            synth_raw_video(3, min_len=8, max_len=30, seed=32, wh=(1920, 1080), **kw),
            synth_raw_video(5, min_len=20, max_len=50, seed=33, wh=(640, 360), n_shadowed=3, **kw),
            synth_raw_video(12, min_len=40, max_len=60, seed=34, wh=(1280, 720), n_categories=3, **kw)]
    if big:
        raws.append(synth_raw_video(34, min_len=50, max_len=60, seed=35, wh=(480, 640), n_categories=4, **kw))
    return raws, [0, 1, 1, 0, 1, 0][:len(raws)]


def test_many_videos_in_one_call():
    raws, offsets = many_videos(n_clip=4)
    assert [len(r["bboxes_list"]) if r else 0 for r in raws] == [2, 0, 3, 8, 12, 34]
    assert len(raws[4]["sids"]) > 64 and len(raws[5]["sids"]) > 1024    # the scan crosses waves, and 256-candidate steps
    assert len(host_drops(raws[3])) >= 3
    got, want = assert_same_call(raws, 2, offsets, 4)
    assert want[0] == {} and want[1] == {} and all(want[2:])
    assert len(want[4]["sids"]) > 64 and len(want[5]["sids"]) > 1024
    # every source is a view of the one uploaded array
    sources = [g["pair_source"] for g in got if g]
    base = sources[0].boxes.untyped_storage().data_ptr()
    for s in sources:
        assert {t.untyped_storage().data_ptr() for t in (s.vis, s.clip, s.boxes)} == {base}
    assert len({s.s_row.untyped_storage().data_ptr() for s in sources} | {s.lens_dev.untyped_storage().data_ptr() for s in sources}) == 1


# --------------------------------------------------------------------------------------------------------------------
# 3. the walk's semantics, hand-built (one category, integer boxes; 100 x 100 pixels under the +1 convention)
# --------------------------------------------------------------------------------------------------------------------
FULL, LEFT91, RIGHT15, LEFT85 = [0, 0, 99, 99], [0, 0, 90, 99], [85, 0, 99, 99], [0, 0, 84, 99]


def walk_cases():
    b_boxes = torch.cat([still(20, FULL), still(20, LEFT85), still(20, FULL)])        # B over [0, 60): 85 % of A inside [20, 40)
    return {
        # (a) B shadows A (0.925), row A ends before C; B does not shadow C (0.85).  Without the `break` C would go too.
        "a_break": (video([(10, still(40, FULL)), (0, b_boxes), (20, still(20, FULL))]), [0]),
        # (b) X drops J; J would shadow I (J covers I, X only 6 of its 15 columns), but a dropped j is skipped
        "b_dropped_j_skipped": (video([(0, still(40, LEFT91)), (10, still(20, RIGHT15)), (5, still(30, FULL))]), [2]),
        # (c) X drops J; the dropped J, as i, still drops I
        "c_dropped_i_still_drops": (video([(0, still(40, LEFT91)), (5, still(30, FULL)), (10, still(20, RIGHT15))]), [1, 2]),
        # (d) 9000 / 10000 is not more than 0.9
        "d_at_threshold": (video([(0, still(30, FULL)), (5, still(20, [10, 0, 109, 99]))]), []),
        "d_above_threshold": (video([(0, still(30, FULL)), (5, still(20, [9, 0, 108, 99]))]), [1]),
        # (e) durations that only touch; (f) different categories
        "e_touching": (video([(0, still(10, FULL)), (10, still(10, FULL))]), []),
        "f_categories": (video([(0, still(10, FULL)), (0, still(10, FULL))], cats=[3, 4]), []),
        "f_same_category": (video([(0, still(10, FULL)), (0, still(10, FULL))]), [1]),
    }


def test_walk_semantics_hand_built():
    cases = walk_cases()
    for name, (raw, want) in cases.items():
        assert host_drops(raw) == want, name                           # first: the reference loop gives what the case says
    # (a) without the break: A would go on to C, which it covers completely
    r = {tuple(p["pair"]): p["f64"] for p in pair_ratios(cases["a_break"][0])}
    assert r[0, 1][0] / r[0, 1][1] == 0.925 and r[0, 2][0] / r[0, 2][2] == 1.0 and r[1, 2][0] / r[1, 2][2] == 0.85
    r = pair_ratios(cases["d_at_threshold"][0])[0]["f64"]
    assert r[0] / r[2] == 0.9 and not r[0] / r[2] > 0.9
    raws = [raw for raw, _ in cases.values()]
    got = device_drops(raws)
    for name, g, (_, want) in zip(cases, got, cases.values()):
        assert g == want, name
    assert_same_call(raws, 1, 0, 2)
    # the threshold is an argument: at 0.5 the 0.85 of (a) counts too, and B then drops C as well as A
    assert host_drops(cases["a_break"][0], 0.5) == [0, 2] == device_drops([cases["a_break"][0]], 0.5)[0]


# --------------------------------------------------------------------------------------------------------------------
# 4. frame-count edges of the reduction: one frame decides
# --------------------------------------------------------------------------------------------------------------------
def test_frame_count_edges():
    raws, names = [], []
    for shared in (1, 63, 64, 65, 130):
        for at in sorted({0, shared - 1, min(64, shared - 1), shared // 2}):
            for special, name in (([5, 0, 104, 99], "above"), ([11, 0, 110, 99], "below")):
                # j inside i's duration; every shared frame overlaps 90 of j's 100 columns, but the one at `at`: 95 or 89
                j = still(shared, [10, 0, 109, 99])
                j[at] = torch.tensor(special, dtype=torch.float32)
                raws.append(video([(0, still(shared + 5, FULL)), (2, j)]))
                names.append((shared, at, name))
    assert any(len(r["bboxes_list"][1]) == 1 for r in raws)           # a one-frame tracklet
    want = []
    for raw, name in zip(raws, names):
        for p in pair_ratios(raw):
            assert p["f32"] == p["f64"] and all(x < 2 ** 24 for x in p["f64"]), name       # integer sums: exact in either precision
        want.append(host_drops(raw))
        assert want[-1] == ([1] if name[2] == "above" else []), name
    got = device_drops(raws)
    for name, g, w in zip(names, got, want):
        assert g == w, name
    assert_same_call(raws, 1, 0, 2)


# --------------------------------------------------------------------------------------------------------------------
# 5. general float boxes
# --------------------------------------------------------------------------------------------------------------------
FLOAT_SEEDS = (41, 42, 43)


def test_general_float_boxes():
    from vrdone_amd.synth import synth_raw_video
    raws = [synth_raw_video(9, V, 20, 120, seed=s, n_categories=3, n_shadowed=4) for s in FLOAT_SEEDS]
    compared = 0
    for s, raw in zip(FLOAT_SEEDS, raws):
        for p in pair_ratios(raw):
            inter, area_i, area_j = p["f32"]
            for ratio in (inter / area_i, inter / area_j):
                assert abs(ratio - 0.9) > 1e-4, f"seed {s} pair {p['pair']}: ratio {ratio} too close to the threshold for a bit-exact test"
            compared += 1
        assert len(host_drops(raw)) >= 1
    assert compared >= 12
    want = [host_drops(raw) for raw in raws]
    assert device_drops(raws) == want
    assert_same_call(raws, 1, 0, 2)
    assert_same_call(raws, 4, [0, 3, 2], 8)


# --------------------------------------------------------------------------------------------------------------------
# 6. pair-table edges
# --------------------------------------------------------------------------------------------------------------------
def _far(frames, k):
    """boxes of tracklet k, apart from every other's"""
    return still(frames, [40 * k, 10, 40 * k + 30, 60])


def test_pair_table_edges():
    # shared frames with tracklet 0 over [0, 40): 5, 6 and 7
    raw = video([(0, _far(40, 0)), (35, _far(20, 1)), (34, _far(20, 2)), (33, _far(20, 3))], cats=[1, 2, 3, 4])
    got, _ = assert_same_call([raw], 1, 0, 6)
    assert list(zip(got[0]["sids"].tolist(), got[0]["oids"].tolist())) == [(0, 2), (0, 3), (1, 2), (1, 3), (2, 0), (2, 1), (2, 3),
                                                                            (3, 0), (3, 1), (3, 2)]
    # stride 3 from offset 1: 4 shared frames give one step (frame 1), 5 give two (1, 4)
    raw = video([(0, _far(40, 0)), (36, _far(20, 1)), (35, _far(20, 2))], cats=[1, 2, 3], pairs=[(0, 1), (0, 2), (2, 0), (1, 0)])
    got, _ = assert_same_call([raw], 3, 1, 2)
    assert list(zip(got[0]["sids"].tolist(), got[0]["oids"].tolist())) == [(0, 2), (2, 0)] and got[0]["pair_source"].lens == [2, 2]
    # ... and with the offset at the last shared frame of the longer pair nothing is left: the video has no proposal
    assert_same_call([raw, raw], 3, [4, 1], 2)
    # a dropped subject, a dropped object, and candidates in an order of their own (tracklet 2 is a copy of tracklet 1)
    raw = video([(0, _far(30, 0)), (0, _far(30, 1)), (2, _far(20, 1)), (5, _far(25, 3))], cats=[1, 2, 2, 3],
                pairs=[(3, 0), (2, 0), (1, 3), (0, 2), (0, 1), (3, 2), (1, 0), (3, 1), (0, 3)])
    assert host_drops(raw) == [2]
    got, _ = assert_same_call([raw], 1, 0, 2)
    assert list(zip(got[0]["sids"].tolist(), got[0]["oids"].tolist())) == [(3, 0), (1, 3), (0, 1), (1, 0), (3, 1), (0, 3)]


# --------------------------------------------------------------------------------------------------------------------
# 7. errors and repeatability
# --------------------------------------------------------------------------------------------------------------------
def test_empty_box_raises_and_names_the_video():
    from vrdone_amd.proposals import prepare_test_proposal, prepare_test_videos
    good = video([(0, _far(10, 0)), (0, _far(10, 1))], cats=[1, 2])
    bad = video([(0, _far(10, 0)), (0, _far(10, 1))], cats=[1, 2], wh=(64, 48))
    bad["bboxes_list"][1][7] = torch.tensor([70.0, 10.0, 90.0, 40.0])          # right of the frame: x1 clamps to 63 < x0
    with pytest.raises(ValueError, match="empty after clamping"):
        prepare_test_proposal(bad, 1, 0, 2, "cpu")                              # the host path refuses it too
    with pytest.raises(ValueError, match=r"video 2\b.*empty after clamping"):
        prepare_test_videos([good, {}, bad, good], 1, 0, 2, DEV)
    nan = video([(0, _far(10, 0)), (0, _far(10, 1))], cats=[1, 2])
    nan["bboxes_list"][0][3, 1] = float("nan")
    with pytest.raises(ValueError, match=r"video 0\b"):
        prepare_test_videos([nan, good], 1, 0, 2, DEV)
    # plain validation: the device is as it was, and the next call works
    torch.cuda.synchronize()
    assert_same_call([good, good], 1, 0, 2)


def test_a_repeat_gives_the_same_bytes():
    from vrdone_amd.proposals import run_proposal_kernels
    raws, offsets = many_videos(big=False)
    raws.append(walk_cases()["c_dropped_i_still_drops"][0])
    a = run_proposal_kernels(raws, 2, offsets + [0], 4, DEV)
    b = run_proposal_kernels(raws, 2, offsets + [0], 4, DEV)
    assert set(a.dev) == set(b.dev) and {"trk_err", "shadow", "dropped", "s_row", "o_row", "lens", "kept_s", "kept_o", "count",
                                         "video_err", "boxes"} <= set(a.dev)
    for k in a.dev:
        assert torch.equal(a.dev[k].reshape(-1).view(torch.uint8), b.dev[k].reshape(-1).view(torch.uint8)), k
        assert a.dev[k].data_ptr() != b.dev[k].data_ptr() or a.dev[k].numel() == 0
    for k in a.host:
        assert np.array_equal(a.host[k], b.host[k]) and np.array_equal(a.host[k], a.dev[k].cpu().numpy()), k


def test_launches_and_copies_do_not_grow_with_the_call(monkeypatch):
    """Four launches, one upload and one copy back, for one small video as for six."""
    from vrdone_amd import _hip, ops, proposals
    calls = []
    for name in ("vrd_proposal_clamp", "vrd_proposal_shadow", "vrd_proposal_walk", "vrd_proposal_pairs"):
        fn = getattr(_hip.lib, name)
        monkeypatch.setattr(ops.lib, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    to, cpu, copy_ = torch.Tensor.to, torch.Tensor.cpu, torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: (calls.append("upload") if not self.is_cuda else None, to(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, src, *a, **k: (
        calls.append("upload" if self.is_cuda else "download") if self.is_cuda != src.is_cuda else None, copy_(self, src, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("download") if self.is_cuda else None, cpu(self, *a, **k))[1])
    raws, offsets = many_videos()
    for n in (3, 6):
        del calls[:]
        proposals.prepare_test_videos(raws[:n], 2, offsets[:n], 4, DEV)
        assert calls == ["upload", "vrd_proposal_clamp", "vrd_proposal_shadow", "vrd_proposal_walk", "vrd_proposal_pairs", "download"], n


# --------------------------------------------------------------------------------------------------------------------
# 8. end to end
# --------------------------------------------------------------------------------------------------------------------
def test_forward_test_videos_on_device_prepared_proposals():
    from conftest import load_case
    from oracle import vrd_oracle as O
    from vrdone_amd.models.maskvrd import MaskVRD
    from vrdone_amd.proposals import prepare_test_proposal, prepare_test_videos
    mc, ic, keys = load_case("vidvrd")
    model = MaskVRD(mc, device=DEV)
    model.load_state_dict(O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]), strict=True)
    model = model.to(DEV).eval()
    model._config_eval(ic)
    raws, offsets = many_videos(n_visual=model.backbone.n_visual, n_clip=model.backbone.n_clip, big=False)
    stride = ic["feat_stride"]
    offsets = [off % stride for off in offsets]
    got = prepare_test_videos(raws, stride, offsets, 4, torch.device(DEV))
    want = [prepare_test_proposal(r, stride, off, 4, torch.device(DEV)) if r else {} for r, off in zip(raws, offsets)]
    assert [bool(g) for g in got] == [bool(w) for w in want] == [False, False, True, True, True]
    a = model.forward_test_videos([g for g in got if g])
    b = model.forward_test_videos([w for w in want if w])
    assert any(x is not None for x in b)
    assert a == b
    # ... and one of them alone through forward_test
    assert model.forward_test(got[3]) == model.forward_test(want[3])
