"""Host side of the multi-video eval call (MaskVRD.forward_test_videos): PairSource.concat's row tables, frame-size tables and
stream plan against the per-video sources, and the grouping of vrdone_amd.evaluate.batched_forward_test.  CPU only."""
import numpy as np
import pytest
import torch

from golden_cases import PROPOSAL_CASES
from oracle import proposal as P


def _sources():
    from vrdone_amd.proposals import prepare_test_proposal
    out = []
    for i, (name, wh) in enumerate([("vidvrd", (640, 360)), ("vidvrd", (1280, 720)), ("vidvrd", (333, 517))]):
        vid_kw, dl_kw = PROPOSAL_CASES[name]
        raw = P.synth_raw_video(**dict(vid_kw, seed=vid_kw["seed"] + i, n_visual=16, wh=wh))
        out.append(prepare_test_proposal(raw, dl_kw["feat_stride"], dl_kw["stride_offset"], dl_kw["proposal_min_frames"], "cpu")["pair_source"])
    return out


def test_pair_source_concat_tables():
    from vrdone_amd.proposals import PairSource
    srcs = _sources()
    cat = PairSource.concat(srcs)
    assert len(cat) == sum(len(s) for s in srcs) and cat.lens == [L for s in srcs for L in s.lens]
    assert cat.stride == srcs[0].stride and cat.n_visual == srcs[0].n_visual and cat.clip is None
    row0, pair0 = 0, 0
    for j, s in enumerate(srcs):
        n, rows = len(s), s.boxes.shape[0]
        # every pair addresses its own video's rows, which hold that video's data
        assert torch.equal(cat.s_row[pair0:pair0 + n], s.s_row + row0) and torch.equal(cat.o_row[pair0:pair0 + n], s.o_row + row0)
        assert torch.equal(cat.vis[row0:row0 + rows], s.vis) and torch.equal(cat.boxes[row0:row0 + rows], s.boxes)
        # tracklet table: each video's tracklets, moved by the rows in front of it
        k = len(s.first_row) - 1
        at = sum(len(t.first_row) - 1 for t in srcs[:j])
        assert (cat.first_row[at:at + k + 1] == s.first_row + row0).all()
        # frame sizes per pair and per row
        assert cat.pair_wh[pair0:pair0 + n].tolist() == [list(s.wh)] * n
        assert cat.rows_wh(np.arange(row0, row0 + rows)).tolist() == [list(s.wh)] * rows
        pair0 += n
        row0 += rows
    assert cat.first_row[-1] == row0 and len(cat.first_row) == sum(len(s.first_row) - 1 for s in srcs) + 1
    assert srcs[0].pair_wh is None and srcs[0].rows_wh([0]) is None and srcs[0].pair_wh_of(None) is None


def test_pair_source_concat_stream_plan():
    """The merged source's streams are the per-video streams, one tracklet each, at the moved rows."""
    from vrdone_amd.proposals import PairSource
    srcs = _sources()
    cat = PairSource.concat(srcs)
    start, length, stream, j0 = cat.stream_plan(np.arange(len(cat)))
    want_start, want_len, want_stream, want_j0 = [], [], [], []
    row0, base = 0, 0
    for s in srcs:
        st, ln, sm, j = s.stream_plan(np.arange(len(s)))
        want_start.append(st + row0)
        want_len.append(ln)
        want_stream.append(sm + base)
        want_j0.append(j)
        row0 += s.boxes.shape[0]
        base += len(st)
    assert start.tolist() == np.concatenate(want_start).tolist() and length.tolist() == np.concatenate(want_len).tolist()
    assert stream.tolist() == np.concatenate(want_stream, axis=1).tolist() and j0.tolist() == np.concatenate(want_j0, axis=1).tolist()
    # every stream lies inside one tracklet
    trk = np.searchsorted(cat.first_row, start, side="right") - 1
    assert (start + (length - 1) * cat.stride < cat.first_row[trk + 1]).all()


def test_pair_source_concat_refuses_mixed_strides():
    from vrdone_amd.proposals import PairSource
    a = _sources()[0]
    b = PairSource(a.vis, a.clip, a.boxes, a.s_row, a.o_row, a.lens_dev, a.stride + 1, a.wh, a.first_row)
    with pytest.raises(ValueError):
        PairSource.concat([a, b])


class _StubModel:
    def __init__(self):
        self.calls = []

    def forward_test_videos(self, videos):
        self.calls.append([v["name"] for v in videos])
        return [None if v["name"] % 3 == 0 else {"name": v["name"]} for v in videos]


def _prop(name, n_pairs):
    return {"name": name, "sids": torch.zeros(n_pairs, dtype=torch.int64)}


def test_batched_forward_test_groups_in_order():
    from vrdone_amd.evaluate import batched_forward_test
    props = [_prop(0, 10), {}, _prop(1, 30), None, _prop(2, 50), _prop(4, 5), _prop(5, 100), _prop(7, 1), {}, _prop(8, 2)]
    model = _StubModel()
    out = list(batched_forward_test(model, iter(props), max_videos=3, max_pairs=90))
    assert [p for p, _ in out] == props                                 # every proposal, in input order
    for p, r in out:
        if not p or p["name"] % 3 == 0:
            assert r is None
        else:
            assert r == {"name": p["name"]}
    # groups: at most 3 videos and 90 pairs (a bigger video alone); the empty proposals take no place
    assert model.calls == [[0, 1, 2], [4], [5], [7, 8]]
    model = _StubModel()
    assert list(batched_forward_test(model, [{}, None])) == [({}, None), (None, None)] and model.calls == []
    with pytest.raises(ValueError):
        list(batched_forward_test(model, props, max_videos=0))
