"""Host half of the device-built training batch (vrdone_amd/proposals.py: TrainSource, train_tables): the index tables make
train_getitem's decisions -- same draws from `random`, same `continue` rules, same crops -- without touching a feature row, and
address exactly the rows train_getitem slices.  CPU only: the source's arrays stay on 'cpu' here; the gather kernel is tested in
tests/test_gpu_train_source.py."""
import copy
import os
import random
import re

import numpy as np
import pytest
import torch

from oracle import proposal as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN = 24          # shorter than the long pairs of the synthetic video, also at stride 2: the crop draws


def _entry(tmp, name="vid0", seed=21, wh=(320, 240)):
    """The cache entry of tests/test_proposals_cpu.py's `train_video` fixture (a trajectory with a gap: its second interval starts
    mid-video; several relations on one pair; pairs longer than MAX_LEN * 2 frames), plus two trajectories that give
      key (5, 6, 0, 0): the intervals share ONE frame -- dropped for having fewer than 2 frames;
      key (0, 6, 0, 0): its only relation is empty (begin == end) -- no surviving relation."""
    from vrdone_amd.proposals import load_train_video
    anno_dir, feat_dir, ent, pred = P.write_synth_train_files(str(tmp), video_name=name, seed=seed, wh=wh)
    v = load_train_video(f"{anno_dir}/{name}.json", f"{feat_dir}/{name}.pkl", ent, pred)
    g = torch.Generator().manual_seed(seed + 100)
    n_visual = v["visual_features"][0][0].shape[1]
    a0, e0 = v["traj_intervals"][0][0]
    mid = (a0 + e0) // 2
    for idx, (a, e) in ((5, (mid - 9, mid + 1)), (6, (mid, mid + 21))):
        n = e - a
        v["traj_intervals"][idx] = [[a, e]]
        v["visual_features"][idx] = [torch.randn(n, n_visual, generator=g)]
        xy = torch.rand(n, 2, generator=g) * 100 + 5
        v["entity_bboxes"][idx] = [torch.cat([xy, xy + 20 + torch.rand(n, 2, generator=g) * 60], dim=1)]
        v["entity_classes"][idx] = 1
    assert e0 >= mid + 21
    v["relation_merged"][(5, 6, 0, 0)].append({"predicate": 2, "begin_fid": mid, "end_fid": mid + 1})
    v["relation_merged"][(0, 6, 0, 0)].append({"predicate": 3, "begin_fid": mid + 4, "end_fid": mid + 4})
    v["relation_keys"] += [[5, 6, 0, 0], [0, 6, 0, 0]]
    return v


def _with_clip(v, n_clip=8, seed=5):
    v = copy.deepcopy(v)
    g = torch.Generator().manual_seed(seed)
    v["clip_features"] = {k: [torch.randn(t.shape[0], n_clip, generator=g) for t in per] for k, per in v["visual_features"].items()}
    return v


@pytest.fixture(scope="module")
def train_video(tmp_path_factory):
    return _entry(tmp_path_factory.mktemp("train"))


@pytest.fixture(scope="module")
def second_video(tmp_path_factory):
    return _entry(tmp_path_factory.mktemp("train2"), name="vid1", seed=22, wh=(640, 360))


def _same_decisions(entry, video, source, stride, max_len, cut, max_preds, dur, seed, index=0):
    """train_tables(video, ...) against train_getitem(entry, ...) from equally seeded generators; returns the tables."""
    from vrdone_amd.proposals import _entity_box_features, train_getitem, train_tables
    r1, r2 = random.Random(seed), random.Random(seed)
    want = train_getitem(entry, stride, max_len, cut, max_preds, dur, rng=r1)
    got = train_tables(video, stride, max_len, cut, max_preds, dur, rng=r2)
    assert r1.getstate() == r2.getstate(), "train_tables drew differently from `random`"
    feats = want.get("so_features_list", [])
    assert len(got) == len(feats) and got.lens.tolist() == [int(f.shape[1]) for f in feats]
    assert len(set(got.keys)) == len(got) and all(list(k) in entry["relation_keys"] for k in got.keys)
    assert got.src.tolist() == [index] * len(got)
    vis, boxes = source.vis.numpy(), source.boxes
    clip = None if source.clip is None else source.clip.numpy()
    V, Cc = source.n_visual, source.n_clip
    h, w = entry["video_hw"]
    assert tuple(source.frame_wh[index]) == (w, h)
    for k, f in enumerate(feats):
        assert torch.equal(got.preds[k], want["preds_list"][k]) and got.preds[k].dtype == want["preds_list"][k].dtype
        assert torch.equal(got.segs[k], want["segs_list"][k]) and got.segs[k].dtype == want["segs_list"][k].dtype
        L, f = int(got.lens[k]), f.numpy()
        rows = lambda r0: slice(int(r0), int(r0) + L * stride, stride)          # noqa: E731
        np.testing.assert_array_equal(vis[rows(got.s_row[k])], f[:V].T)
        np.testing.assert_array_equal(vis[rows(got.o_row[k])], f[V:2 * V].T)
        if Cc:
            np.testing.assert_array_equal(clip[rows(got.s_row[k])], f[2 * V:2 * V + Cc].T)
            np.testing.assert_array_equal(clip[rows(got.o_row[k])], f[2 * V + Cc:2 * V + 2 * Cc].T)
        # the rule the kernel differentiates the boxes by: a cropped sequence (lead > 0) looks one sub-sampled frame back
        back = min(int(got.lead[k]), 1)
        for r0, c0 in ((got.s_row[k], 2 * V + 2 * Cc + 5), (got.o_row[k], 2 * V + 2 * Cc + 13)):
            b = boxes[int(r0) - back * stride:int(r0) + L * stride:stride]
            assert b.shape[0] == L + back
            np.testing.assert_array_equal(_entity_box_features(b, w, h)[back:].numpy(), f[c0:c0 + 8].T)
    return got


CASES = {   # name -> (feat_stride, max_seq_len, cut_max_preds, proposal_max_preds, pair_duration, CLIP rows)
    "stride1": (1, MAX_LEN, False, 0, None, False),
    "stride2": (2, MAX_LEN, False, 0, None, False),
    "stride1_duration": (1, MAX_LEN, False, 0, (1, 6), False),
    "stride2_duration": (2, MAX_LEN, False, 0, (0, 4), False),
    "stride1_cut": (1, MAX_LEN, True, 1, None, False),
    "stride2_cut_duration": (2, MAX_LEN, True, 1, (2, 7), False),
    "stride1_uncropped": (1, 96, False, 0, None, False),
    "stride1_clip": (1, MAX_LEN, False, 0, None, True),
    "stride2_clip": (2, MAX_LEN, False, 0, (0, 5), True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tables_make_the_decisions_of_train_getitem(name, train_video):
    from vrdone_amd.proposals import TrainSource
    stride, max_len, cut, max_preds, dur, with_clip = CASES[name]
    entry = _with_clip(train_video) if with_clip else train_video
    src = TrainSource.from_entry(entry, "cpu")
    assert (src.clip is not None) == with_clip and src.vis.shape[0] == src.boxes.shape[0]
    seen_crop = seen_lead = seen_mid = seen_none = 0
    for seed in range(6):
        got = _same_decisions(entry, src, src, stride, max_len, cut, max_preds, dur, seed)
        seen_crop += int((got.lens == max_len).sum())
        seen_lead += int((got.lead > 0).sum())
        seen_mid += sum(k[2] > 0 and entry["traj_intervals"][k[0]][k[2]][0] > 0 for k in got.keys)
        if dur is None and not cut:
            # the video's cases: the one-frame key and the key without a surviving relation never appear
            assert (5, 6, 0, 0) not in got.keys and (0, 6, 0, 0) not in got.keys
            if max_len == 96:
                assert len(got) == len(entry["relation_keys"]) - 2            # nothing is cropped: every other key survives
            # a key whose every relation is longer than two windows: no window keeps half of one -- the crop gives None
            hopeless = [k for k, rels in entry["relation_merged"].items()
                        if all(r["end_fid"] - r["begin_fid"] > (2 * max_len + 1) * stride for r in rels)]
            assert not set(hopeless) & set(got.keys)
            seen_none += len(hopeless)
    if (stride, max_len, dur, cut) == (1, MAX_LEN, None, False):
        assert seen_none, "no key whose crop gives None"
    if stride == 1:           # (at stride 2 that key's only relation is longer than twice the window: the crop drops it)
        assert seen_mid, "no key on an interval that starts mid-video"
    if max_len == MAX_LEN:
        assert seen_crop and seen_lead, "no pair was cropped: the case does not reach truncate_feats' draws"


def test_an_empty_entry_yields_no_sample():
    from vrdone_amd.proposals import TrainSource, train_getitem, train_tables
    src = TrainSource.from_entry({}, "cpu")
    r1, r2 = random.Random(3), random.Random(3)
    assert train_getitem({}, 1, MAX_LEN, rng=r1) == {} and len(train_tables(src, 1, MAX_LEN, rng=r2)) == 0
    assert r1.getstate() == r2.getstate()


def test_concat_keeps_every_video_its_rows_and_frame_size(train_video, second_video):
    from vrdone_amd.proposals import TrainSource, TrainTables
    a, b = TrainSource.from_entry(train_video, "cpu"), TrainSource.from_entry(second_video, "cpu")
    cat = TrainSource.concat([a, TrainSource.from_entry({}, "cpu"), b])
    assert len(cat) == 3 and cat.vis.shape[0] == a.vis.shape[0] + b.vis.shape[0]
    assert cat.frame_wh[0].tolist() == [320, 240] and cat.frame_wh[2].tolist() == [640, 360]
    assert [v.index for v in cat.videos] == [0, 1, 2] and cat.videos[2].row0 == a.vis.shape[0]
    ta = _same_decisions(train_video, cat.videos[0], cat, 2, MAX_LEN, False, 0, (0, 3), 4, index=0)
    tb = _same_decisions(second_video, cat.videos[2], cat, 2, MAX_LEN, False, 0, None, 5, index=2)
    alone = _same_decisions(second_video, b, b, 2, MAX_LEN, False, 0, None, 5)
    assert (tb.s_row - alone.s_row).tolist() == [a.vis.shape[0]] * len(tb) and (tb.o_row - alone.o_row).tolist() == [a.vis.shape[0]] * len(tb)
    both = TrainTables.concat([ta, tb])
    assert len(both) == len(ta) + len(tb) and both.src.tolist() == [0] * len(ta) + [2] * len(tb)
    assert both.sizes == ta.sizes + tb.sizes and both.keys == ta.keys + tb.keys
    both.check(cat)
    with pytest.raises(ValueError):
        both.check(a)                      # the second video's rows lie outside the first source
    with pytest.raises(ValueError):
        TrainSource.concat([a, TrainSource.from_entry(_with_clip(second_video), "cpu")])


def test_device_tables_are_one_aligned_buffer(train_video):
    """TrainTables.on_device: every table is a view of one uploaded buffer, aligned to its element size, and holds the host values."""
    from vrdone_amd.proposals import TrainSource, train_tables
    src = TrainSource.from_entry(train_video, "cpu")
    t = train_tables(src, 2, MAX_LEN, rng=random.Random(1))
    d = t.on_device(src)
    assert d is t.on_device(src)
    base = d["s_row"].untyped_storage().data_ptr()
    for name, ten in d.items():
        assert ten.untyped_storage().data_ptr() == base and ten.data_ptr() % ten.element_size() == 0, name
    assert d["s_row"].tolist() == t.s_row.tolist() and d["lens"].tolist() == t.lens.tolist() and d["lead"].tolist() == t.lead.tolist()
    assert d["preds"].tolist() == torch.cat(t.preds).tolist() and torch.equal(d["segs"], torch.cat(t.segs))
    assert d["seg_lo"].tolist() == torch.cat(t.segs)[:, 0].long().tolist() and d["seq_wh"].tolist() == [[320.0, 240.0]] * len(t)


def test_gather_train_binding_matches_the_header():
    """vrd_gather_train is declared, exported and bound field for field; the ABI number did not move."""
    from vrdone_amd import _hip
    header = open(os.path.join(REPO, "include", "vrdone_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vrd_gather_train_args", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [part.strip().split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _hip.GatherTrainArgs._fields_]
    assert "vrd_gather_train" in _hip._SIGNATURES and hasattr(_hip.lib, "vrd_gather_train")
    assert "#define VRD_ABI_VERSION 37" in header and _hip.ABI_VERSION == 37
    a = _hip.GatherTrainArgs()
    assert _hip.lib.vrd_gather_train(a, None) != 0 and b"vrd_gather_train" in _hip.lib.vrd_last_error()
