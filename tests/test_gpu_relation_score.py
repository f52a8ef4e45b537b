"""Relation scoring on the MI355X: vrd_relation_viou against evaluate.viou (bit for bit on quarter-pixel boxes, 1e-12 off the
grid), vrd_match_relations against eval_detection_scores' greedy loop on constructed cases, and DeviceRelationScorer end to end
against EvaluationFormatConvertor + eval_visual_relation on the model's own predictions (vidvrd, and vidor at feat_stride 4)."""
import numpy as np
import pytest
import torch

from conftest import load_case
from oracle import vrd_oracle as O
from relation_score_cases import (ENTITY, ENTITY_ID, PRED, PRED_ID, fake_result, greedy_hits, grid_video, host_prediction, on_grid)
from vrdone_amd import evaluate as E
from vrdone_amd import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


# ------------------------------------------------------------------------------------------------------------ helpers
def track(rng, n, grid=True):
    """(n, 4) f32 boxes of a drifting track, coordinates below 2048"""
    corner = rng.random((1, 2)) * [900, 500] + np.cumsum(rng.random((n, 2)) * 0.5, axis=0) % 300
    size = rng.random((1, 2)) * 300 + 8 + rng.random((n, 2)) * 4
    b = torch.from_numpy(np.concatenate([corner, corner + size], axis=1).astype(np.float32))
    assert float(b.max()) < 2048
    return (on_grid(b) if grid else b).numpy()


def shifted(t, dx, dy=0.0):
    return (t + np.asarray([dx, dy, dx, dy], dtype=np.float32)).astype(np.float32)


def rel(sub, obj, start, triplet=(1, 1, 2), score=None):
    r = {"triplet": tuple(triplet), "duration": (start, start + len(sub)), "sub_traj": np.asarray(sub, dtype=np.float32),
         "obj_traj": np.asarray(obj, dtype=np.float32)}
    assert len(sub) == len(obj)
    if score is not None:
        r["score"] = score
    return r


def as_lists(r):
    return dict(r, sub_traj=r["sub_traj"].tolist(), obj_traj=r["obj_traj"].tolist())


def pack(records, gap=0):
    """boxes (rows, 4) and the (n, 4) int64 table of `records`; gap: rows of NaN in front of, between and behind the tracks"""
    nan = np.full((gap, 4), np.nan, dtype=np.float32)
    parts, table, row = [nan], [], gap
    for r in records:
        n = len(r["sub_traj"])
        table.append([row, row + n + gap, r["duration"][0], n])
        parts += [r["sub_traj"].reshape(-1, 4), nan, r["obj_traj"].reshape(-1, 4), nan]
        row += 2 * (n + gap)
    boxes = np.concatenate(parts, axis=0).astype(np.float32) if records else np.zeros((0, 4), dtype=np.float32)
    return torch.from_numpy(boxes).to(DEV), torch.tensor(table, dtype=torch.int64).reshape(-1, 4).to(DEV)


def device_viou(pairs, gap=0):
    """ops.relation_viou over candidates (prediction record, ground-truth record), one prediction and one ground truth each"""
    from vrdone_amd import ops
    pb, pt = pack([p for p, _ in pairs], gap)
    gb, gt = pack([g for _, g in pairs], gap)
    cand = torch.arange(len(pairs), dtype=torch.int32).repeat_interleave(2).reshape(-1, 2).to(DEV)
    return ops.relation_viou(pb, pt, gb, gt, cand.contiguous()).cpu().numpy()


def host_viou(pairs):
    return np.array([min(E.viou(p["sub_traj"].tolist(), p["duration"], g["sub_traj"].tolist(), g["duration"]),
                         E.viou(p["obj_traj"].tolist(), p["duration"], g["obj_traj"].tolist(), g["duration"])) for p, g in pairs])


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def grid_pairs():
    """the exactness cases of vrd_relation_viou, boxes on the quarter-pixel grid; index of the 1.0 and of the 0.5 case"""
    rng = np.random.default_rng(5)
    pairs = []
    for n in (1, 2, 63, 64, 65, 129, 1000):                      # one lane, a partial wave, one wave +- 1, several strides
        s, o = track(rng, n), track(rng, n)
        pairs.append((rel(s, o, 5), rel(shifted(s, 3.25, -1.5), shifted(o, -2.0, 0.75), 5)))
    s, o = track(rng, 10), track(rng, 10)
    pairs.append((rel(s, o, 0), rel(s, o, 20)))                  # disjoint durations
    pairs.append((rel(s, o, 0), rel(s, o, 10)))                  # touching: hi == lo
    n_zero = len(pairs)
    s, o = track(rng, 100), track(rng, 100)
    pairs.append((rel(s, o, 0), rel(shifted(s[30:50], 1.25), shifted(o[30:50], 0.5), 30)))           # one duration inside the other
    s2, o2 = track(rng, 80), track(rng, 80)
    pairs.append((rel(s[10:80], o[10:80], 10), rel(shifted(s2, 2.0), o2, 40)))                       # offset starts
    pairs.append((rel(s, o, 7), rel(s.copy(), o.copy(), 7)))                                         # identical: 1.0
    box, box2 = np.asarray([[10, 20, 109.75, 79.5]], dtype=np.float32), np.asarray([[300.25, 40, 420, 99]], dtype=np.float32)
    pairs.append((rel(box.repeat(66, 0), box2.repeat(66, 0), 3), rel(box.repeat(33, 0), box2.repeat(33, 0), 3)))   # half: 0.5
    return pairs, n_zero, len(pairs) - 2, len(pairs) - 1


# ---------------------------------------------------------------------------------------------------- vrd_relation_viou
def test_relation_viou_on_the_grid_is_bit_equal_to_the_host():
    pairs, n_zero, i_one, i_half = grid_pairs()
    got, want = device_viou(pairs), host_viou(pairs)
    print("device", got.tolist(), "host", want.tolist())
    assert (bits(got) == bits(want)).all(), (got - want).tolist()
    assert got[n_zero - 2] == 0.0 and got[n_zero - 1] == 0.0 and got[i_one] == 1.0 and got[i_half] == 0.5
    assert (got[:n_zero - 2] > 0).all() and (got[:n_zero - 2] < 1).all()
    assert (bits(device_viou(pairs)) == bits(got)).all()                     # a repeat is bit-equal


def test_relation_viou_off_the_grid_within_1e12():
    """<= 4096 frames x 2^-53 per sum is under 5e-13 relative; the quotient adds a few 2^-53."""
    rng = np.random.default_rng(6)
    pairs = []
    for n in (1, 3, 64, 100, 777, 1500, 4096):
        for _ in range(4):
            s, o = track(rng, n, grid=False), track(rng, n, grid=False)
            cut = int(rng.integers(0, n))
            jig = lambda t: (t + rng.normal(0, 3, t.shape)).astype(np.float32)          # noqa: E731
            pairs.append((rel(s, o, 11), rel(jig(s[cut:]), jig(o[cut:]), 11 + cut)))
    got, want = device_viou(pairs), host_viou(pairs)
    err = np.abs(got - want) / want
    print("max relative error", float(err.max()))
    assert (want > 0).all() and float(err.max()) <= 1e-12


def test_relation_viou_reads_nothing_outside_its_tracks():
    pairs, *_ = grid_pairs()
    dense, guarded = device_viou(pairs), device_viou(pairs, gap=3)
    assert np.isfinite(guarded).all() and (bits(guarded) == bits(dense)).all()


# -------------------------------------------------------------------------------------------------- vrd_match_relations
BOX = np.asarray([[0, 0, 99, 99]], dtype=np.float32)               # 100 x 100: moved by d columns, IoU = (100 - d) / (100 + d)
FAR = np.asarray([[1000, 1000, 1099, 1099]], dtype=np.float32)


def still(d, n=4, start=0, triplet=(1, 1, 2), score=None):
    """a relation whose subject and object stand still, d columns off BOX"""
    return rel(shifted(BOX, d).repeat(n, 0), shifted(BOX, d).repeat(n, 0), start, triplet, score)


def constructed_videos():
    """(name, ground truths, predictions in input order) per video"""
    half = [rel(BOX.repeat(8, 0), BOX.repeat(8, 0), 0, score=0.9)], [rel(BOX.repeat(4, 0), BOX.repeat(4, 0), 0)]
    seventy = [still(abs(g - 66) * 0.25, triplet=(3, 3, 3)) for g in range(70)]       # ov rises up to index 66 (a lane's second candidate)
    return [
        # the better-scored prediction takes the ground truth the later one overlaps better: that one misses
        ("greedy", [still(0)], [still(0, score=0.8), still(25, score=0.9)]),
        ("equal scores", [still(0)], [still(10, score=0.5), still(0, score=0.5), still(0, score=0.5)]),
        ("ov == threshold", half[1], half[0]),
        ("equal ov", [still(0), still(0), still(0)], [still(5, score=0.3), still(5, score=0.2)]),
        ("70 candidates", seventy, [still(0, triplet=(3, 3, 3), score=0.7), still(2, triplet=(3, 3, 3), score=0.6)]),
        ("no candidate", [still(0)], [still(0, triplet=(9, 9, 9), score=0.4), still(0, score=0.1)]),
        ("no prediction", [still(0), still(3)], []),
        ("all miss", [rel(FAR.repeat(4, 0), FAR.repeat(4, 0), 0)], [still(0, score=0.5)]),
    ]


def scoring_order(preds):
    return sorted(range(len(preds)), key=lambda i: preds[i]["score"], reverse=True)


def device_hits(videos, threshold=0.5):
    """ops.relation_viou + ops.match_relations over [(ground truths, predictions)]: (hit per prediction in scoring order, with
    ground-truth indices counted over all videos; ov)"""
    from vrdone_amd import ops
    gts = [g for gt, _ in videos for g in gt]
    preds, pred_first, cand, cand_first, g0 = [], [0], [], [0], 0
    for gt, pr in videos:
        for i in scoring_order(pr):
            cand += [[len(preds), g0 + g] for g, r in enumerate(gt) if r["triplet"] == pr[i]["triplet"]]
            preds.append(pr[i])
            cand_first.append(len(cand))
        pred_first.append(len(preds))
        g0 += len(gt)
    pb, pt = pack(preds)
    gb, gtab = pack(gts)
    i32 = lambda x, shape: torch.tensor(x, dtype=torch.int32).reshape(shape).to(DEV)      # noqa: E731
    cand_dev = i32(cand, (-1, 2))
    ov = ops.relation_viou(pb, pt, gb, gtab, cand_dev)
    hit = ops.match_relations(i32(pred_first, (-1,)), i32(cand_first, (-1,)), cand_dev, ov, len(gts), threshold)
    return hit.cpu().numpy(), ov.cpu().numpy()


def host_hits(videos, threshold=0.5):
    out, g0 = [], 0
    for gt, pr in videos:
        h = greedy_hits([as_lists(g) for g in gt], [as_lists(pr[i]) for i in scoring_order(pr)], threshold)
        out.append(np.where(h >= 0, h + g0, -1))
        g0 += len(gt)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def test_match_relations_on_constructed_cases():
    cases = constructed_videos()
    videos = [(gt, pr) for _, gt, pr in cases]
    want = host_hits(videos)
    got, ov = device_hits(videos)
    print("hit", got.tolist(), "host", want.tolist())
    # the cases are what they claim to be (host side), video by video
    at, g0, by_name = 0, 0, {}
    for name, gt, pr in cases:
        by_name[name] = (want[at:at + len(pr)] - np.where(want[at:at + len(pr)] >= 0, g0, 0)).tolist()
        at, g0 = at + len(pr), g0 + len(gt)
    assert by_name == {"greedy": [0, -1], "equal scores": [0, -1, -1], "ov == threshold": [0], "equal ov": [0, 1],
                       "70 candidates": [66, 58], "no candidate": [-1, 0], "no prediction": [], "all miss": [-1]}
    assert got.tolist() == want.tolist()
    again, ov2 = device_hits(videos)
    assert again.tolist() == got.tolist() and (bits(ov2) == bits(ov)).all()
    # each video alone gives its part of the joint call
    at, g0 = 0, 0
    for gt, pr in videos:
        alone, _ = device_hits([(gt, pr)])
        assert np.where(alone >= 0, alone + g0, -1).tolist() == got[at:at + len(pr)].tolist()
        at, g0 = at + len(pr), g0 + len(gt)
    # a threshold above every overlap but the exact ones
    assert device_hits(videos, 0.9)[0].tolist() == host_hits(videos, 0.9).tolist()


def test_match_relations_three_videos_of_200_predictions():
    videos = []
    for i in range(3):
        video = grid_video(8, 20, 50, seed=40 + i)
        res = fake_result(video, 200, seed=50 + i, n_scores=9)
        doc = synth.synth_relation_ground_truth(["v"], [video], [res], ENTITY, PRED, per_video=60, seed=i)["v"]
        gt = [rel(r["sub_traj"], r["obj_traj"], r["duration"][0], (ENTITY_ID[r["triplet"][0]], PRED_ID[r["triplet"][1]], ENTITY_ID[r["triplet"][2]]))
              for r in doc]
        pr = [rel(res["so_trajs"][j][0], res["so_trajs"][j][1], res["pred_durations"][j][0], res["triplets"][j], res["triple_scores_avg"][j])
              for j in range(200)]
        videos.append((gt, pr))
    want = host_hits(videos)
    assert (want >= 0).sum() >= 30 and (want < 0).sum() >= 30
    got, ov = device_hits(videos)
    assert got.tolist() == want.tolist()
    parts, g0 = [], 0
    for gt, pr in videos:
        alone, _ = device_hits([(gt, pr)])
        parts.append(np.where(alone >= 0, alone + g0, -1))
        g0 += len(gt)
    assert np.concatenate(parts).tolist() == got.tolist()
    again, ov2 = device_hits(videos)
    assert again.tolist() == got.tolist() and (bits(ov2) == bits(ov)).all()


# ---------------------------------------------------------------------------------------------------------- end to end
_models = {}


def get_model(name):
    if name not in _models:
        from vrdone_amd.models.maskvrd import MaskVRD
        mc, ic, keys = load_case(name)
        model = MaskVRD(mc, device=DEV)
        model.load_state_dict(O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]), strict=True)
        model = model.to(DEV).eval()
        model._config_eval(ic)
        _models[name] = (model, ic)
    return _models[name]


def grid_proposals(model, stride, specs):
    from vrdone_amd.proposals import prepare_test_proposal
    videos = []
    for i, (n, lo, hi, wh, offset) in enumerate(specs):
        raw = synth.synth_raw_video(n, model.backbone.n_visual, lo, hi, seed=300 + i, n_clip=model.backbone.n_clip, wh=wh)
        raw["bboxes_list"] = [on_grid(b) for b in raw["bboxes_list"]]          # (the clamp to the frame keeps them on the grid)
        videos.append(prepare_test_proposal(raw, stride, offset, 2, torch.device(DEV)))
    assert all(videos)
    return videos


def check_end_to_end(dataset_type, names, videos, forward, model, min_hits, min_misses):
    results = forward(videos)
    assert all(r is not None and "so_trajs" in r for r in results)
    doc = synth.synth_relation_ground_truth([E.EvaluationFormatConvertor(dataset_type, ENTITY, PRED)._reset_video_name(n) for n in names],
                                            videos, results, ENTITY, PRED, per_video=20, seed=1)
    # the comparison is not vacuous: hits, misses and a triplet with two ground truths, on the host path
    prediction = host_prediction(dataset_type, names, results)
    hit_scores = np.concatenate([E.eval_detection_scores(doc[v], prediction[v], 0.5)[2] for v in doc])
    assert np.isfinite(hit_scores).sum() >= min_hits and (~np.isfinite(hit_scores)).sum() >= min_misses
    assert any(len({tuple(r["triplet"]) for r in rels}) < len(rels) for rels in doc.values())
    want = E.eval_visual_relation(doc, prediction, viou_threshold=0.5)
    gt = E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, DEV, dataset_type=dataset_type)
    scorer = E.DeviceRelationScorer(gt, viou_threshold=0.5)
    scorer.add(names, videos, results)
    assert scorer.summary() == want
    mean_ap, rec, prec = want
    assert scorer.result() == {"RelDet_mAP": mean_ap, **{f"RelDet_AR@{k}": v for k, v in rec.items()},
                               **{f"RelTag_AP@{k}": v for k, v in prec.items()}}
    # the same without so_trajs: the key is absent, everything else identical, the score the same
    try:
        model.with_so_trajs = False
        bare = forward(videos)
    finally:
        del model.with_so_trajs
    assert bare == [{k: v for k, v in r.items() if k != "so_trajs"} for r in results]
    assert all(list(b) == [k for k in r if k != "so_trajs"] for b, r in zip(bare, results))
    scorer = E.DeviceRelationScorer(gt, viou_threshold=0.5)
    scorer.add(names, videos, bare)
    assert scorer.summary() == want
    assert forward(videos) == results                           # the default call is unchanged
    return results


def test_scorer_end_to_end_vidvrd():
    model, ic = get_model("vidvrd")
    videos = grid_proposals(model, ic["feat_stride"], [(6, 20, 60, (640, 360), 0), (10, 10, 90, (320, 240), 0), (12, 20, 40, (480, 640), 0)])
    names = ["ILSVRC2015_train_00005015", "ILSVRC2015_train_00010001", "ILSVRC2015_train_00010002"]
    results = check_end_to_end("vidvrd", names, videos, model.forward_test_videos, model, 10, 10)
    # forward_test, one video: the flag holds there too
    one = model.forward_test(videos[0])
    try:
        model.with_so_trajs = False
        bare = model.forward_test(videos[0])
    finally:
        del model.with_so_trajs
    assert "so_trajs" in one and bare == {k: v for k, v in one.items() if k != "so_trajs"}
    # scored_forward_test: the results of batched_forward_test with the same groups, and their score
    want = [r for _, r in E.batched_forward_test(model, videos, max_videos=2)]
    doc = synth.synth_relation_ground_truth(names, videos, results, ENTITY, PRED, per_video=20, seed=1)
    scorer = E.DeviceRelationScorer(E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, DEV))
    got = list(E.scored_forward_test(model, zip(names, videos), scorer, max_videos=2))
    assert [p for p, _ in got] == videos and [r for _, r in got] == want
    assert scorer.summary() == E.eval_visual_relation(doc, host_prediction("vidvrd", names, want))


def test_scorer_end_to_end_vidor_stride_4():
    model, ic = get_model("vidor")
    assert ic["feat_stride"] == 4
    videos = grid_proposals(model, 4, [(4, 80, 240, (640, 360), 1)])          # tracklets of 20-60 feature steps, stride offset 1
    check_end_to_end("vidor", ["0001_3598080384"], videos, model.forward_test_videos, model, 1, 1)
