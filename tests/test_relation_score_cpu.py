"""Relation scoring on the device, the parts that need no GPU: the C ABI of vrd_relation_viou / vrd_match_relations (the library
validates arguments before any device access), RelationGroundTruth's tables, the candidate and order tables of
DeviceRelationScorer.add against a brute-force loop, and the metric assembly against eval_visual_relation / eval_relation with a
host matcher in place of the two kernels."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from relation_score_cases import (ENTITY, ENTITY_ID, PRED, PRED_ID, fake_result, grid_video, host_matcher, host_prediction)
from vrdone_amd import evaluate as E
from vrdone_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_declares_exports_and_binds_the_two_entry_points():
    from vrdone_amd import _hip
    header = open(os.path.join(REPO, "include", "vrdone_hip.h")).read()
    assert re.search(r"#define VRD_ABI_VERSION 37\b", header) and _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    assert len(_hip.KERNEL_NAMES) == 14
    for name, struct in (("vrd_relation_viou", "vrd_viou_args"), ("vrd_match_relations", "vrd_match_args")):
        assert re.search(r"int %s\(const %s\* a, void\* stream\);" % (name, struct), header), name
        assert hasattr(_hip.lib, name) and name in _hip._SIGNATURES


def _viou_args(**kw):
    from vrdone_amd import _hip
    a = _hip.ViouArgs()
    a.pred_boxes = a.gt_boxes = a.pred = a.gt = a.cand = a.ov = 256          # dummy aligned addresses: never dereferenced
    a.pred_rows, a.gt_rows, a.n_pred, a.n_gt, a.n_cand = 8, 8, 2, 2, 3
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _match_args(**kw):
    from vrdone_amd import _hip
    a = _hip.MatchArgs()
    a.pred_first = a.cand_first = a.cand = a.ov = a.detected = a.hit = 256
    a.n_videos, a.n_pred, a.n_cand, a.n_gt, a.threshold = 1, 2, 3, 2, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_cand=-1), dict(n_pred=-2), dict(n_gt=-1), dict(pred_rows=-1), dict(gt_rows=-5),
                                 dict(pred=None), dict(gt=None), dict(cand=None), dict(ov=None), dict(pred_boxes=None),
                                 dict(gt_boxes=None)])
def test_relation_viou_refuses_bad_arguments_before_any_device_work(bad):
    from vrdone_amd import _hip
    assert _hip.lib.vrd_relation_viou(ctypes.byref(_viou_args(**bad)), None) < 0
    assert "vrd_relation_viou" in _hip.lib.vrd_last_error().decode()


@pytest.mark.parametrize("bad", [dict(n_videos=-1), dict(n_pred=-1), dict(n_cand=-3), dict(n_gt=-1), dict(pred_first=None),
                                 dict(cand_first=None), dict(cand=None), dict(ov=None), dict(detected=None), dict(hit=None)])
def test_match_relations_refuses_bad_arguments_before_any_device_work(bad):
    from vrdone_amd import _hip
    assert _hip.lib.vrd_match_relations(ctypes.byref(_match_args(**bad)), None) < 0
    assert "vrd_match_relations" in _hip.lib.vrd_last_error().decode()


def test_empty_calls_are_successful_no_ops():
    from vrdone_amd import _hip
    lib = _hip.lib
    assert lib.vrd_relation_viou(ctypes.byref(_viou_args(n_cand=0, cand=None, ov=None)), None) == 0
    assert lib.vrd_relation_viou(ctypes.byref(_viou_args(n_cand=0, n_pred=0, n_gt=0, pred_rows=0, gt_rows=0, pred=None, gt=None, cand=None,
                                                         ov=None, pred_boxes=None, gt_boxes=None)), None) == 0
    assert lib.vrd_match_relations(ctypes.byref(_match_args(n_videos=0, pred_first=None)), None) == 0
    assert lib.vrd_match_relations(ctypes.byref(_match_args(n_pred=0, n_cand=0, cand_first=None, hit=None, cand=None, ov=None)), None) == 0


# ------------------------------------------------------------------------------------------------ RelationGroundTruth
def _two_videos():
    b = [1.0, 2.0, 11.0, 12.0]
    c = [3.25, 4.5, 20.0, 30.75]
    return {"3598080384": [{"triplet": ["entity2", "pred5", "entity3"], "duration": [4, 7], "sub_traj": [b] * 3, "obj_traj": [c] * 3},
                           {"triplet": ["entity3", "pred1", "entity2"], "duration": [0, 1], "sub_traj": [c], "obj_traj": [b]}],
            "empty": [],
            "777": [{"triplet": ["entity2", "pred5", "entity3"], "duration": [10, 12], "sub_traj": [b, c], "obj_traj": [c, b]}]}


def test_ground_truth_tables_hand_worked():
    b, c = [1.0, 2.0, 11.0, 12.0], [3.25, 4.5, 20.0, 30.75]
    gt = E.RelationGroundTruth(_two_videos(), ENTITY_ID, PRED_ID, None, dataset_type="vidor")
    assert gt.videos == ["3598080384", "777"] and gt.empty_videos == {"empty"} and len(gt) == 3
    assert gt.video_index == {"3598080384": 0, "777": 1}
    assert gt.video_first.tolist() == [0, 2, 3]
    # [subject's first row, object's first row, first frame, frames]: 3 + 3 rows, then 1 + 1, then 2 + 2
    assert gt.relations.tolist() == [[0, 3, 4, 3], [6, 7, 0, 1], [8, 10, 10, 2]] and gt.relations.dtype == np.int64
    assert gt.triplets.tolist() == [[2, 5, 3], [3, 1, 2], [2, 5, 3]]
    assert gt.boxes.dtype == np.float32 and gt.boxes.tolist() == [b] * 3 + [c] * 3 + [c, b] + [b, c] + [c, b]
    assert gt.boxes_dev is None and gt.relations_dev is None
    assert gt.video_key("0001_3598080384") == "3598080384"                  # the vidor rule of the convertor
    assert E.RelationGroundTruth(_two_videos(), ENTITY_ID, PRED_ID, None).video_key("0001_3598080384") == "0001_3598080384"
    on_cpu = E.RelationGroundTruth(_two_videos(), ENTITY_ID, PRED_ID, "cpu")
    assert torch.equal(on_cpu.boxes_dev, torch.from_numpy(gt.boxes)) and torch.equal(on_cpu.relations_dev, torch.from_numpy(gt.relations))


def test_ground_truth_refuses_unknown_names_and_short_tracks():
    doc = _two_videos()
    doc["777"][0]["triplet"] = ["entity2", "leapfrog", "entity3"]
    with pytest.raises(ValueError, match="leapfrog"):
        E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    doc = _two_videos()
    doc["777"][0]["triplet"] = ["entity2", "pred5", "unicorn"]
    with pytest.raises(ValueError, match="unicorn"):
        E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    doc = _two_videos()
    doc["777"][0]["obj_traj"] = doc["777"][0]["obj_traj"][:1]
    with pytest.raises(ValueError, match="777"):
        E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    with pytest.raises(NotImplementedError):
        E.RelationGroundTruth(_two_videos(), ENTITY_ID, PRED_ID, None, dataset_type="coco")


# ------------------------------------------------------------------------------------------ candidate and order tables
def _world(seed=0):
    """Videos, results and a ground truth: video 0 has 3 predictions, video 1 has 150, video 2 is added but absent from the
    ground truth, video 3 has a None result, "never" is in the ground truth only, "blank" has an empty relation list."""
    names = ["v0", "v1", "v2", "v3"]
    videos = [grid_video(4, 10, 30, seed + 1), grid_video(7, 20, 50, seed + 2), grid_video(3, 10, 20, seed + 3),
              grid_video(3, 10, 20, seed + 4)]
    results = [fake_result(videos[0], 3, seed + 5), fake_result(videos[1], 150, seed + 6), fake_result(videos[2], 20, seed + 7), None]
    doc = synth.synth_relation_ground_truth(names, videos, results, ENTITY, PRED, per_video=30, seed=seed)
    doc["v3"] = list(doc["v1"][:4])                         # ground truth of a video without predictions
    doc["never"] = list(doc["v1"][2:9])
    doc["blank"] = []
    del doc["v2"]
    return names, videos, results, doc


def test_add_builds_order_and_candidates_like_a_brute_force_loop():
    names, videos, results, doc = _world()
    # a triplet with 70 ground truths, one prediction of it, and a prediction whose triplet has no ground truth
    seventy = dict(doc["v0"][0], triplet=[ENTITY[results[0]["triplets"][1][0]], PRED[7], ENTITY[results[0]["triplets"][1][2]]])
    doc["v0"] = doc["v0"] + [dict(seventy) for _ in range(70)]
    results[0]["triplets"][1][1] = 7
    results[0]["triplets"][2][1] = 199
    gt = E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    scorer = E.DeviceRelationScorer(gt, matcher=lambda t: np.full(len(t["pred"]), -1))
    t = scorer.tables(names, videos, results)
    assert [gt.videos[v] for v in t["videos"]] == ["v0", "v1"]                # v2: no ground truth; v3: no prediction
    assert t["pred_first"].tolist() == [0, 3, 153] and t["pred_first"].dtype == np.int32
    assert t["cand_first"].dtype == np.int32 and t["cand"].dtype == np.int32 and t["pred"].dtype == np.int64
    want_cand, want_pred, n_seventy, n_none = [], [], 0, 0
    for j, name in enumerate(["v0", "v1"]):
        res, video = results[j], videos[j]
        scores = res["triple_scores_avg"]
        assert len(set(scores)) < len(scores) or len(scores) == 3           # equal scores are part of the case
        order = sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)
        assert t["order"][j].tolist() == order and t["scores"][j].tolist() == [scores[i] for i in order]
        first_row = np.concatenate([[0], np.cumsum([len(b) for b in video["bboxes_list"]])]) + sum(
            sum(len(b) for b in videos[k]["bboxes_list"]) for k in range(j))
        spans = video["traj_durations"].tolist()
        a = int(gt.video_first[gt.video_index[name]])
        for i in order:
            (s, o), (start, end) = res["so_tids"][i], res["pred_durations"][i]
            want_pred.append([first_row[s] + start - spans[s][0], first_row[o] + start - spans[o][0], start, end - start])
            names3 = [ENTITY[res["triplets"][i][0]], PRED[res["triplets"][i][1]], ENTITY[res["triplets"][i][2]]]
            mine = [a + g for g, rel in enumerate(doc[name]) if rel["triplet"] == names3]
            n_seventy += len(mine) == 70
            n_none += len(mine) == 0
            want_cand.append(mine)
    assert n_seventy == 1 and n_none >= 1
    assert t["pred"].tolist() == want_pred
    assert t["cand_first"].tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want_cand])]).tolist()
    assert t["cand"].tolist() == [[p, g] for p, c in enumerate(want_cand) for g in c]
    assert sum(len(b) for b in t["pred_boxes"]) == sum(len(b) for v in videos[:2] for b in v["bboxes_list"])


def test_add_refuses_a_prediction_outside_its_tracklet():
    names, videos, results, doc = _world()
    gt = E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    results[0]["pred_durations"][0] = [0, 10 ** 6]
    with pytest.raises(ValueError, match="v0"):
        E.DeviceRelationScorer(gt, matcher=lambda t: None).tables(names, videos, results)


# ------------------------------------------------------------------------------------------------------ metric assembly
@pytest.mark.parametrize("seed", [0, 11])
@pytest.mark.parametrize("threshold", [0.5, 0.7])
def test_scorer_equals_eval_visual_relation_with_a_host_matcher(seed, threshold, tmp_path):
    names, videos, results, doc = _world(seed)
    want = E.eval_visual_relation(doc, host_prediction("vidvrd", names, results), viou_threshold=threshold)
    hits = sum(np.isfinite(E.eval_detection_scores(doc[n], host_prediction("vidvrd", [n], [r])[n], threshold)[2]).sum()
               for n, r in zip(names, results) if n in doc)
    assert hits >= 10 and want[0] < 1.0                           # not a vacuous comparison
    gt = E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    scorer = E.DeviceRelationScorer(gt, viou_threshold=threshold, matcher=host_matcher(gt, threshold))
    scorer.add(names[:1], videos[:1], results[:1])                  # two calls: one video, then three
    scorer.add(names[1:], videos[1:], results[1:])
    assert scorer.summary() == want
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(doc))
    cfg = {"prepare_gt_config": {"gt_relations_path": str(path)}, "inference_config": {"viou_th": threshold}}
    assert scorer.result() == E.eval_relation("vidvrd", prediction_results=host_prediction("vidvrd", names, results), config=cfg)
    # other return counts than the defaults
    other = E.DeviceRelationScorer(gt, threshold, det_nreturns=(2, 20), tag_nreturns=(3,), matcher=host_matcher(gt, threshold))
    other.add(names, videos, results)
    assert other.summary() == E.eval_visual_relation(doc, host_prediction("vidvrd", names, results), threshold, (2, 20), (3,))


def test_scorer_applies_the_vidor_name_rule():
    names, videos, results, doc = _world(3)
    vidor = [f"00{i}_{n}" for i, n in enumerate(names)]
    want = E.eval_visual_relation(doc, host_prediction("vidor", vidor, results))
    gt = E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None, dataset_type="vidor")
    scorer = E.DeviceRelationScorer(gt, matcher=host_matcher(gt, 0.5))
    scorer.add(vidor, videos, results)
    assert scorer.summary() == want


def test_default_matcher_is_the_device_path_without_a_host_fallback():
    names, videos, results, doc = _world()
    gt = E.RelationGroundTruth(doc, ENTITY_ID, PRED_ID, None)
    with pytest.raises(RuntimeError, match="no host fallback"):
        E.DeviceRelationScorer(gt).add(names, videos, results)


def test_scored_forward_test_groups_like_batched_forward_test():
    """A model stub: the groups, the yielded pairs and what reaches the scorer."""
    class Model:
        calls = []

        def forward_test_videos(self, group):
            self.calls.append([p["id"] for p in group])
            return [None if p["id"] == 2 else {"id": p["id"]} for p in group]

    class Scorer:
        seen = []

        def add(self, names, videos, results):
            self.seen.append((list(names), [p["id"] for p in videos], [r and r["id"] for r in results]))

    props = [{"id": 0, "sids": [0] * 3}, {}, {"id": 2, "sids": [0] * 3}, {"id": 3, "sids": [0] * 5}, None, {"id": 5, "sids": [0]}]
    named = [(f"n{i}", p) for i, p in enumerate(props)]
    model, scorer = Model(), Scorer()
    got = list(E.scored_forward_test(model, named, scorer, max_videos=2, max_pairs=8))
    plain = Model()
    plain.calls = []
    want = list(E.batched_forward_test(plain, props, max_videos=2, max_pairs=8))
    assert [(p, r) for p, r in got] == [(p, r) for p, r in want]
    assert model.calls == plain.calls == [[0, 2], [3, 5]]
    assert scorer.seen == [(["n0", "n2"], [0, 2], [0, None]), (["n3", "n5"], [3, 5], [3, 5])]


def test_with_so_trajs_is_a_class_default():
    from vrdone_amd.models.maskvrd import MaskVRD
    assert MaskVRD.with_so_trajs is True
