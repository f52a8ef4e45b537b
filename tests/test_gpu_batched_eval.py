"""MaskVRD.forward_test_videos (many videos in one eval call) on the MI355X: per video the same result as forward_test on that
video alone; the reference goldens still hold inside a batch; the per-sequence frame size of vrd_gather_pairs; the segmented
selection kernel vrd_select_triplets against torch's nonzero + stable argsort; the f16x3 range fallback."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from oracle import proposal as OP
from oracle import vrd_oracle as O
from oracle.synth import synth_proposal

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
BF16X3_TIE = {"bf16x3": 5e-6}       # (as tests/test_gpu_model.py: ties of the reference's scores the 17-bit mode may permute)

_models = {}


def get_model(name):
    if name not in _models:
        from vrdone_amd.models.maskvrd import MaskVRD
        mc, ic, keys = load_case(name)
        sd = O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"])
        model = MaskVRD(mc, device=DEV)
        model.load_state_dict(sd, strict=True)
        model = model.to(DEV).eval()
        model._config_eval(ic)
        _models[name] = (model, mc, ic)
    return _models[name]


def c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


@pytest.fixture(params=["bf16x3", "f16x3", "f32"])
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def _on_device(data):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV) if torch.is_tensor(v) else v) for k, v in data.items()}


# (tracklets, min frames, max frames, frame size): six videos, one of them of more than 256 pairs (the row-space form), one whose
# pairs are all shorter than the test's pred_min_frames (no triplet: None)
VIDEOS = [(6, 20, 60, (640, 360)), (18, 40, 60, (1280, 720)), (4, 8, 8, (320, 240)), (10, 10, 90, (320, 240)),
          (4, 30, 50, (1920, 1080)), (12, 20, 40, (480, 640))]
NO_TRIPLET = 2
PRED_MIN_FRAMES = 10


def _raw_videos(bb):
    from vrdone_amd import synth
    return [synth.synth_raw_video(n, bb.n_visual, lo, hi, seed=100 + i, n_clip=bb.n_clip, wh=wh)
            for i, (n, lo, hi, wh) in enumerate(VIDEOS)]


def _same(got, want):
    if want is None:
        assert got is None
        return
    assert got is not None
    for key in ("triplets", "so_tids", "pred_durations", "so_trajs"):
        assert got[key] == want[key], key
    for key in ("triple_scores", "triple_scores_avg"):
        np.testing.assert_allclose(np.array(got[key]), np.array(want[key]), atol=1e-5, rtol=0)


@pytest.mark.parametrize("name", ["vidvrd", "vidor"])
@pytest.mark.parametrize("form", ["tracklets", "pair_matrices"])
def test_forward_test_videos_equals_one_call_per_video(name, form, precision):
    from vrdone_amd.proposals import prepare_test_proposal
    model, mc, ic = get_model(name)
    stride = ic["feat_stride"]
    raws = _raw_videos(model.backbone)
    offsets = [i % stride for i in range(len(raws))]                  # (vidor: so_offset 0..3)
    if form == "tracklets":
        videos = [prepare_test_proposal(r, stride, off, 2, torch.device(DEV)) for r, off in zip(raws, offsets)]
    else:
        videos = [_on_device(OP.test_getitem(r, feat_stride=stride, stride_offset=off, proposal_min_frames=2))
                  for r, off in zip(raws, offsets)]
    assert all(videos) and len(videos[1]["sids"]) > model.ROWS_MIN_PAIRS
    old = model.pred_min_frames
    try:
        model.pred_min_frames = PRED_MIN_FRAMES
        want = [model.forward_test(v) for v in videos]
        got = model.forward_test_videos(videos)
    finally:
        model.pred_min_frames = old
    assert len(got) == len(videos)
    assert want[NO_TRIPLET] is None and sum(w is not None for w in want) == len(videos) - 1
    for g, w in zip(got, want):
        _same(g, w)


def test_reference_goldens_inside_a_batch(precision):
    """The proposals behind forward_test_vidvrd.json / forward_test_vidor_x.json between other videos of one call."""
    from golden_cases import VIDOR_X, compare_forward_test
    for name, golden, make in (("vidvrd", "forward_test_vidvrd.json", lambda c: synth_proposal(6, c, 20, 130, seed=4321)),
                               ("vidor_x", "forward_test_vidor_x.json", lambda c: synth_proposal(c_in=c, **VIDOR_X))):
        model, mc, ic = get_model(name)
        with open(os.path.join(GOLDEN, golden)) as f:
            ref = json.load(f)
        others = [synth_proposal(n, c_in(mc), lo, hi, seed=s, feat_stride=ic["feat_stride"], random_offset=ic["feat_stride"] > 1)
                  for n, lo, hi, s in ((5, 20, 90, 11), (3, 10, 40, 12), (8, 30, 200, 13))]
        videos = [_on_device(v) for v in (others[0], make(c_in(mc)), others[1], others[2])]
        got = model.forward_test_videos(videos)
        compare_forward_test(got[1], ref, ic["n_max_pair"], 5e-6, slack=0, tie_tol=BF16X3_TIE.get(precision, 0.0))


@pytest.mark.parametrize("pair_wide", [False, True])
def test_gather_with_a_frame_size_table(pair_wide):
    from golden_cases import PROPOSAL_CASES
    from vrdone_amd import ops
    from vrdone_amd.proposals import PairSource, prepare_test_proposal
    vid_kw, dl_kw = PROPOSAL_CASES["strided"]
    srcs = []
    for i, wh in enumerate([(640, 360), (1280, 720), (333, 517)]):
        raw = OP.synth_raw_video(**dict(vid_kw, seed=vid_kw["seed"] + i, wh=wh))
        srcs.append(prepare_test_proposal(raw, dl_kw["feat_stride"], dl_kw["stride_offset"], dl_kw["proposal_min_frames"], DEV)["pair_source"])
    T = max(max(s.lens) for s in srcs) + 3
    # the table holding the scalar frame size: bit for bit the scalar call
    src = srcs[1]
    sel = torch.arange(len(src), device=DEV)
    s_row, o_row, lens = src.s_row.contiguous(), src.o_row.contiguous(), src.lens_dev.contiguous()
    a = ops.gather_rows(src, s_row, o_row, lens, T, 5, 8, pair_wide)
    b = ops.gather_rows(src, s_row, o_row, lens, T, 5, 8, pair_wide,
                        seq_wh=torch.tensor([src.wh], dtype=torch.float32, device=DEV).expand(len(src), 2).contiguous())
    for x, y in zip(a, b):
        x, y = (x.t if isinstance(x, ops.Pair) else x), (y.t if isinstance(y, ops.Pair) else y)
        assert (x is None and y is None) or torch.equal(x, y)
    # mixed sizes in one call: each pair equals the scalar call of its own video
    cat = PairSource.concat(srcs)
    got = ops.gather_pairs(cat, torch.arange(len(cat), device=DEV), T, 5, 8, pair_wide)
    P, at = len(cat), 0
    for s in srcs:
        n = len(s)
        want = ops.gather_pairs(s, torch.arange(n, device=DEV), T, 5, 8, pair_wide)
        for j, (x, y) in enumerate(zip(got, want)):
            x, y = (x.t if isinstance(x, ops.Pair) else x), (y.t if isinstance(y, ops.Pair) else y)
            if x is None:
                assert y is None
            elif j in (0, 1, 3):            # [subject | object] halves
                assert torch.equal(x[at:at + n], y[:n]) and torch.equal(x[P + at:P + at + n], y[n:]), j
            elif j in (2, 4):
                assert torch.equal(x[at:at + n], y), j
        at += n


def _torch_select(cand, s_sc, o_sc, offs, so_start, so_end, fs, pmf, n_max):
    """forward_test's selection for one video, as torch ops on the device (models/maskvrd.py)."""
    P, Q, W = cand.shape
    k = (W - 2) // 2
    if P == 0:
        return [], []
    ints = cand.view(torch.int32)
    first, last = ints[:, :, 2 * k].long(), ints[:, :, 2 * k + 1]
    start = first * fs + offs[:, None]
    end = last.long() * fs + offs[:, None] + 1
    keep = (last >= 0) & ((end - start) >= pmf)
    assert bool(((start >= 0) & (end <= (so_end - so_start)[:, None]))[keep].all())
    keep = keep[:, :, None].expand(P, Q, k).reshape(-1)
    pair_of = torch.arange(P, device=DEV).repeat_interleave(Q * k)
    tri = torch.stack([s_sc[pair_of], cand[:, :, :k].reshape(-1), o_sc[pair_of]], dim=1)
    avg = tri.mean(dim=-1)
    c = torch.nonzero(keep).flatten()
    order = c[torch.argsort(avg[c], descending=True, stable=True)[:n_max]]
    return order.tolist(), avg[order].tolist()


@pytest.mark.parametrize("n_max", [1, 7, 200, 4096])
def test_select_triplets_equals_torch(n_max):
    from vrdone_amd import ops
    g = torch.Generator().manual_seed(n_max)
    Q, k, fs, pmf = 9, 8, 4, 5
    n_pairs = [0, 3, 40, 1, 0, 700, 17, 2070]
    P = sum(n_pairs)
    cand = torch.empty(P, Q, 2 * k + 2)
    cand[:, :, :k] = torch.randint(0, 6, (P, Q, k), generator=g).float() / 8          # many exact ties
    cand[:, :, :k] = torch.where(torch.rand(P, Q, k, generator=g) < 0.05, -0.0, cand[:, :, :k])
    ints = cand.view(torch.int32)
    ints[:, :, k:2 * k] = torch.randint(1, 50, (P, Q, k), generator=g, dtype=torch.int32)
    first = torch.randint(0, 20, (P, Q), generator=g, dtype=torch.int32)
    last = first + torch.randint(-1, 6, (P, Q), generator=g, dtype=torch.int32)
    last = torch.where(torch.rand(P, Q, generator=g) < 0.2, -1, last)
    ints[:, :, 2 * k], ints[:, :, 2 * k + 1] = torch.where(last < 0, -1, first), last
    s_sc = torch.randint(0, 4, (P,), generator=g).float() / 4
    o_sc = torch.randint(0, 4, (P,), generator=g).float() / 4
    offs = torch.randint(0, 4, (P,), generator=g, dtype=torch.int32)
    so_start = torch.randint(0, 50, (P,), generator=g, dtype=torch.int32)
    so_end = so_start + 200
    vp = torch.tensor(np.concatenate([[0], np.cumsum(n_pairs)]), dtype=torch.int32)
    d = lambda t: t.to(DEV).contiguous()          # noqa: E731
    count, index, score = ops.select_triplets(d(cand), d(s_sc), d(o_sc), d(offs), d(so_start), d(so_end), d(vp), fs, pmf, n_max,
                                              max(n_pairs))
    count, index, score = count.cpu(), index.cpu(), score.cpu()
    for v in range(len(n_pairs)):
        a, b = int(vp[v]), int(vp[v + 1])
        want, want_avg = _torch_select(d(cand[a:b]), d(s_sc[a:b]), d(o_sc[a:b]), d(offs[a:b]).long(), d(so_start[a:b]).long(),
                                       d(so_end[a:b]).long(), fs, pmf, n_max)
        n = int(count[v, 0])
        assert n == len(want) and int(count[v, 1]) == 0, v
        assert index[v, :n].tolist() == want, v
        assert (index[v, n:] == -1).all()
        assert score[v, :n].tolist() == want_avg, v


def test_select_triplets_score_is_torch_mean_bit_for_bit():
    """1e6 random triples (one single-candidate video each): the kernel's score equals torch's GPU mean of the three."""
    from vrdone_amd import ops
    g = torch.Generator().manual_seed(5)
    N = 1_000_000
    s, p, o = (torch.rand(N, generator=g) * torch.exp2(torch.randint(-12, 1, (N,), generator=g).float()) for _ in range(3))
    cand = torch.zeros(N, 1, 4)
    cand[:, 0, 0] = p
    cand.view(torch.int32)[:, 0, 3] = 1                    # first 0, last 1: kept (2 frames)
    want = torch.stack([s.to(DEV), p.to(DEV), o.to(DEV)], dim=1).mean(dim=-1)
    z = torch.zeros(N, dtype=torch.int32, device=DEV)
    count, index, score = ops.select_triplets(cand.to(DEV), s.to(DEV), o.to(DEV), z, z, z + 100,
                                              torch.arange(N + 1, dtype=torch.int32, device=DEV), 1, 2, 1, 1)
    assert bool((count[:, 0] == 1).all()) and bool((index[:, 0] == 0).all())
    diff = int((score[:, 0].view(torch.int32) != want.view(torch.int32)).sum())
    assert diff == 0, f"{diff} of {N} scores differ from torch's mean"


def test_f16x3_range_flag_in_a_batched_call_repeats_the_videos():
    """Inputs beyond the f16x3 operand range in one video of a call: the call warns and every video's result equals its own
    forward_test (which repeats the big video in f32)."""
    from vrdone_amd import ops
    model, mc, _ = get_model("vidvrd")
    data = synth_proposal(4, c_in(mc), 20, 60, seed=99)
    big = dict(data, so_features_list=[f * 3.0e4 for f in data["so_features_list"]])
    videos = [_on_device(v) for v in (synth_proposal(5, c_in(mc), 20, 80, seed=7), big, synth_proposal(3, c_in(mc), 20, 60, seed=8))]
    with ops.use_precision("f16x3"):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = model.forward_test_videos(videos)
            want = [model.forward_test(v) for v in videos]
        assert any("multi-video call" in str(x.message) for x in w)
    with ops.use_precision("f32"):
        f32 = model.forward_test(videos[1])
    assert got == want
    assert got[1]["triplets"] == f32["triplets"] and got[1]["triple_scores_avg"] == f32["triple_scores_avg"]


def test_sharded_model_refuses_a_multi_video_call():
    model, mc, _ = get_model("vidvrd")
    try:
        model.shard_pairs()
        with pytest.raises(NotImplementedError):
            model.forward_test_videos([_on_device(synth_proposal(3, c_in(mc), 20, 60, seed=8))])
    finally:
        model.shard_pairs(enable=False)
