"""Host side of vrdone_amd.proposals.prepare_test_videos (eval proposals prepared on the device): the C ABI of the four new
entries, the packer of the flat tables, the new keywords of synth_raw_video, the argument errors.  No GPU: the kernels are
tested in tests/test_gpu_prepare_videos.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

ENTRIES = ("vrd_proposal_clamp", "vrd_proposal_shadow", "vrd_proposal_walk", "vrd_proposal_pairs")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vrdone_hip.h")).read(), flags=re.S)


def test_header_declares_the_entries_and_the_binding_matches():
    from vrdone_amd import _hip
    header = _header()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const vrd_proposal_args\*\s*a\s*,\s*void\*\s*stream\s*\)\s*;", header), name
        res, args = _hip._SIGNATURES[name]
        assert res is ctypes.c_int and args == [ctypes.POINTER(_hip.ProposalArgs), ctypes.c_void_p]
        assert hasattr(_hip.lib, name)


def test_struct_mirror_has_the_header_layout():
    """Field by field: name, order and C type of vrd_proposal_args against the ctypes mirror."""
    from vrdone_amd import _hip
    body = re.search(r"typedef struct \{([^}]*)\} vrd_proposal_args", _header()).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype = decl.split(",")[0].rsplit(" ", 1)[0]             # "const int64_t*" of "const int64_t* trk"; "int32_t" of "int32_t a, b"
        for part in decl[len(ctype):].split(","):
            fields.append((part.strip(), ctype))
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [f for f, _ in fields] == [f for f, _ in _hip.ProposalArgs._fields_]
    for (name, ctype), (_, bound) in zip(fields, _hip.ProposalArgs._fields_):
        assert bound is (ctypes.c_void_p if "*" in ctype else kinds[ctype]), (name, ctype, bound)


def test_abi_version_is_unchanged():
    from vrdone_amd import _hip
    assert _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    assert re.search(r"#define\s+VRD_ABI_VERSION\s+37\b", open(os.path.join(REPO, "include", "vrdone_hip.h")).read())


def test_null_struct_is_refused_by_name():
    from vrdone_amd import _hip
    for name in ENTRIES:
        assert getattr(_hip.lib, name)(None, None) != 0 and name.encode() in _hip.lib.vrd_last_error()


def _raw(spans, cats, pairs, wh, n_visual=3, n_clip=0):
    g = torch.Generator().manual_seed(len(spans))
    raw = {"sids": torch.tensor([p[0] for p in pairs], dtype=torch.int64), "oids": torch.tensor([p[1] for p in pairs], dtype=torch.int64),
           "cat_ids": torch.tensor(cats), "cat_scores": torch.rand(len(spans), generator=g),
           "bboxes_list": [torch.tensor([[1.0, 2.0, 30.0, 40.0]]).repeat(e - a, 1) for a, e in spans],
           "traj_durations": torch.tensor(spans, dtype=torch.int64),
           "visual_features_list": [torch.randn(e - a, n_visual, generator=g) for a, e in spans], "video_wh": wh}
    if n_clip:
        raw["clip_features_list"] = [torch.randn(e - a, n_clip, generator=g) for a, e in spans]
    return raw


def test_packer_against_hand_written_tables():
    from vrdone_amd.proposals import pack_test_videos
    a = _raw([(0, 5), (3, 7), (10, 12)], [4, 4, 9], [(1, 0), (0, 1), (2, 0)], (640, 360))
    b = _raw([(2, 4), (0, 9), (1, 3), (5, 6)], [1, 2, 1, 1], [(3, 1), (0, 2)], (320.0, 240.0))
    t = pack_test_videos([a, {}, b], [0, 5, 2])
    want = {
        # first row, first frame, frames, category, video
        "trk": [[0, 0, 5, 4, 0], [5, 3, 4, 4, 0], [9, 10, 2, 9, 0],
                [11, 2, 2, 1, 2], [13, 0, 9, 2, 2], [22, 1, 2, 1, 2], [24, 5, 1, 1, 2]],
        "video_max": [[639.0, 359.0], [0.0, 0.0], [319.0, 239.0]],
        "trk_first": [0, 3, 3, 7],
        "tri_first": [0, 3, 3, 9],                  # 3 * 2 / 2 and 4 * 3 / 2 unordered pairs
        "cand_first": [0, 3, 3, 5],
        "cand_s": [1, 0, 2, 3, 0], "cand_o": [0, 1, 0, 1, 2],
        "stride_offset": [0, 5, 2],
    }
    dtypes = {"trk": np.int64, "video_max": np.float32, "trk_first": np.int32, "tri_first": np.int64, "cand_first": np.int64,
              "cand_s": np.int32, "cand_o": np.int32, "stride_offset": np.int32}
    assert set(t.tables) == set(want)
    for k, w in want.items():
        assert t.tables[k].dtype == dtypes[k], k
        assert t.tables[k].tolist() == w, k
    assert t.video_row.tolist() == [0, 11, 11, 25] and t.widths == (3, None) and t.n_videos == 3
    assert t.video_wh == [(640, 360), None, (320.0, 240.0)]
    # one offset for every video; no video at all
    assert pack_test_videos([a, b], 3).tables["stride_offset"].tolist() == [3, 3]
    empty = pack_test_videos([{}, {}], 0)
    assert empty.tables["trk"].shape == (0, 5) and empty.tables["tri_first"].tolist() == [0, 0, 0] and len(empty.tables["cand_s"]) == 0


def _old_synth_raw_video(n_tracklets, n_visual, min_len, max_len, seed=7, n_clip=0, wh=(1280, 720)):
    """synth_raw_video as it was before the keywords n_categories / n_shadowed, draw for draw."""
    g = torch.Generator().manual_seed(seed)
    video_len = max_len + 8
    spans, boxes, vis, clip = [], [], [], []
    for _ in range(n_tracklets):
        n = int(torch.randint(min_len, max_len + 1, (1,), generator=g))
        t0 = int(torch.randint(0, video_len - n + 1, (1,), generator=g))
        spans.append((t0, t0 + n))
        corner = torch.rand(n, 2, generator=g) * torch.tensor([wh[0] * 0.6, wh[1] * 0.6])
        boxes.append(torch.cat([corner, corner + torch.rand(n, 2, generator=g) * torch.tensor([wh[0] * 0.3, wh[1] * 0.3]) + 8.0], dim=1))
        vis.append(torch.randn(n, n_visual, generator=g))
        if n_clip:
            clip.append(torch.randn(n, n_clip, generator=g))
    sids, oids = [], []
    for s in range(n_tracklets):
        for o in range(n_tracklets):
            if s != o and min(spans[s][1], spans[o][1]) > max(spans[s][0], spans[o][0]):
                sids.append(s)
                oids.append(o)
    out = {"sids": torch.tensor(sids), "oids": torch.tensor(oids), "cat_ids": torch.arange(1, n_tracklets + 1),
           "cat_scores": torch.rand(n_tracklets, generator=g), "bboxes_list": boxes,
           "traj_durations": torch.tensor(spans, dtype=torch.int64), "visual_features_list": vis, "video_wh": wh}
    if n_clip:
        out["clip_features_list"] = clip
    return out


@pytest.mark.parametrize("kw", [dict(n_tracklets=6, n_visual=8, min_len=4, max_len=40, seed=3),
                                dict(n_tracklets=9, n_visual=4, min_len=2, max_len=12, seed=11, n_clip=5, wh=(320, 240))])
def test_synth_raw_video_defaults_are_unchanged(kw):
    from vrdone_amd.synth import synth_raw_video
    want, got = _old_synth_raw_video(**kw), synth_raw_video(**kw)
    assert list(want) == list(got)
    for k, w in want.items():
        if isinstance(w, list):
            assert len(w) == len(got[k]) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(w, got[k])), k
        elif torch.is_tensor(w):
            assert w.dtype == got[k].dtype and torch.equal(w, got[k]), k
        else:
            assert w == got[k], k


def test_synth_raw_video_shadowed_tracklets_are_dropped():
    from vrdone_amd.proposals import _clamped, shadowed_tracklets
    from vrdone_amd.synth import synth_raw_video
    base = synth_raw_video(5, 8, 10, 60, seed=2)
    raw = synth_raw_video(5, 8, 10, 60, seed=2, n_shadowed=2)
    n = len(raw["bboxes_list"])
    assert n == 7 and len(raw["visual_features_list"]) == len(raw["cat_ids"]) == len(raw["cat_scores"]) == len(raw["traj_durations"]) == 7
    assert all(torch.equal(x, y) for x, y in zip(base["bboxes_list"], raw["bboxes_list"][:5]))
    assert set(raw["cat_ids"][5:].tolist()) <= set(raw["cat_ids"][:5].tolist())
    spans = [tuple(s) for s in raw["traj_durations"].tolist()]
    assert all(b.shape == (e - a, 4) and v.shape == (e - a, 8) for b, v, (a, e) in zip(raw["bboxes_list"], raw["visual_features_list"], spans))
    boxes = [_clamped(b, *raw["video_wh"]) for b in raw["bboxes_list"]]
    dropped = shadowed_tracklets(boxes, spans, raw["cat_ids"].tolist())
    assert len(dropped) >= 2 and set(dropped) >= {5, 6}
    assert int(raw["sids"].max()) == 6                       # the copies take part in the candidate pairs
    # categories drawn from a few: several tracklets share one, and the draw does not disturb the rest of the video
    few = synth_raw_video(12, 8, 10, 60, seed=2, n_categories=3)
    assert set(few["cat_ids"].tolist()) <= {1, 2, 3} and len(few["cat_ids"]) == 12
    plain = synth_raw_video(12, 8, 10, 60, seed=2)
    assert torch.equal(few["cat_scores"], plain["cat_scores"]) and torch.equal(few["sids"], plain["sids"])


def test_argument_errors():
    from vrdone_amd.proposals import pack_test_videos, prepare_test_videos
    spans = [(0, 5), (3, 7)]
    ok = _raw(spans, [1, 1], [(0, 1), (1, 0)], (64, 48))
    with pytest.raises(ValueError, match="video 1.*outside"):
        pack_test_videos([ok, _raw(spans, [1, 1], [(0, 2)], (64, 48))], 0)
    with pytest.raises(ValueError, match="outside"):
        pack_test_videos([_raw(spans, [1, 1], [(-1, 0)], (64, 48))], 0)
    with pytest.raises(ValueError, match="feature widths"):
        pack_test_videos([ok, _raw(spans, [1, 1], [(0, 1)], (64, 48), n_visual=4)], 0)
    with pytest.raises(ValueError, match="feature widths"):
        pack_test_videos([ok, _raw(spans, [1, 1], [(0, 1)], (64, 48), n_clip=2)], 0)
    with pytest.raises(ValueError, match="stride offsets"):
        pack_test_videos([ok, ok], [0])
    with pytest.raises(ValueError, match="negative"):
        pack_test_videos([ok], -1)
    short = _raw(spans, [1, 1], [(0, 1)], (64, 48))
    short["bboxes_list"][1] = short["bboxes_list"][1][:-1]
    with pytest.raises(ValueError, match="tracklet 1"):
        pack_test_videos([short], 0)
    # the device path has no CPU form
    for device in (None, "cpu"):
        with pytest.raises(ValueError, match="prepare_test_proposal"):
            prepare_test_videos([ok], 1, 0, 2, device)
