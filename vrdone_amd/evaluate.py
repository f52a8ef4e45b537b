"""Evaluation glue behind `forward_test`: result dict -> the benchmark's JSON records, and the relation
detection / tagging metrics.

* `EvaluationFormatConvertor` -- interface and output of reference utils/evaluate.py:12-73 (what eval.py:102,151 calls).
  The id -> name tables are the reference checkout's `dataloaders/category.py` (data, not restated here): they are
  imported from the checkout when the drop-in launcher has put it on sys.path, or passed in.
* `eval_visual_relation` / `eval_relation` -- interface of utils/evaluate.py:77-170.  The scoring functions they call
  (`eval_detection_scores`, `eval_tagging_scores`, `voc_ap`, `viou`) live in the un-vendored third-party package
  VidVRD-helper (xdshang/VidVRD-helper, `evaluation/visual_relation_detection.py`, `evaluation/common.py`; the reference
  pins no version), which is absent from the reference tree: they are restated here from the published algorithm and
  **parity is unpinned** -- tests check them on hand-worked cases and invariants only.  The vIoU of all (prediction, ground
  truth) candidates of a video is evaluated with array operations per pair of trajectories instead of a Python loop per
  frame.
* `RelationGroundTruth` / `DeviceRelationScorer` / `scored_forward_test` -- the same metrics with the vIoU and the greedy
  matching on the device (csrc/vrd_score.hip), fed by forward_test's results and the proposals' tracklet boxes instead of
  the convertor's records; opt-in, and pinned (`==`) to the host functions of this module.
"""
import json
import os
from collections import defaultdict

import numpy as np


def _reference_tables(dataset_type):
    try:
        from dataloaders import category          # the reference checkout (dropin/run.py puts it on sys.path)
    except ImportError as e:
        raise ImportError("EvaluationFormatConvertor needs the id -> name tables of the reference checkout's "
                          "dataloaders/category.py: run from the checkout (dropin/run.py) or pass "
                          "entity_id_to_name / pred_id_to_name") from e
    return (getattr(category, f"{dataset_type}_category_id_to_name"), getattr(category, f"{dataset_type}_pred_id_to_name"))


class EvaluationFormatConvertor:
    """forward_test's result dict -> {video name: [relation records]} (reference utils/evaluate.py:12-73)."""

    def __init__(self, dataset_type, entity_id_to_name=None, pred_id_to_name=None):
        self.dataset_type = dataset_type.lower()
        if self.dataset_type not in ("vidvrd", "vidor"):
            raise NotImplementedError(dataset_type)
        if entity_id_to_name is None or pred_id_to_name is None:
            entity_id_to_name, pred_id_to_name = _reference_tables(self.dataset_type)
        self.entity_id_to_name, self.pred_id_to_name = entity_id_to_name, pred_id_to_name

    def _reset_video_name(self, video_name):
        if self.dataset_type == "vidor":            # "0001_3598080384" -> "3598080384"
            parts = video_name.split('_')
            assert len(parts) == 2
            return parts[1]
        return video_name

    def to_eval_format_pr(self, video_name, pr_triplet):
        """pr_triplet: what MaskVRD.forward_test returns (None -- no candidate survived -- gives an empty list; the
        reference's caller skips such videos before it gets here, eval.py:148-149)."""
        video_name = self._reset_video_name(video_name)
        if pr_triplet is None:
            return {video_name: []}
        records = []
        for i, (s_cat, pred_cat, o_cat) in enumerate(pr_triplet['triplets']):
            start, end = pr_triplet["pred_durations"][i][0], pr_triplet["pred_durations"][i][1]
            sub, obj = pr_triplet["so_trajs"][i]
            assert len(sub) == len(obj) == end - start
            records.append({
                "triplet": [self.entity_id_to_name[s_cat], self.pred_id_to_name[pred_cat], self.entity_id_to_name[o_cat]],
                "duration": (start, end),
                "score": float(pr_triplet["triple_scores_avg"][i]),
                "sub_traj": sub,
                "obj_traj": obj,
            })
        return {video_name: records}


# --------------------------------------------------------------------------------------------------------------------
# VidVRD-helper's scoring, restated (parity unpinned, see the module docstring)
# --------------------------------------------------------------------------------------------------------------------
def _volume(traj):
    t = np.asarray(traj, dtype=np.float64).reshape(-1, 4)
    return float(((t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1)).sum())


def viou(traj_1, duration_1, traj_2, duration_2):
    """Volumetric IoU of two box tracks; durations are [start, end) frame ids, boxes (x0, y0, x1, y1) with the +1 pixel
    convention (VidVRD-helper evaluation/common.py `viou`)."""
    lo, hi = max(duration_1[0], duration_2[0]), min(duration_1[1], duration_2[1])
    if hi <= lo:
        return 0.0
    a = np.asarray(traj_1, dtype=np.float64).reshape(-1, 4)[lo - duration_1[0]:hi - duration_1[0]]
    b = np.asarray(traj_2, dtype=np.float64).reshape(-1, 4)[lo - duration_2[0]:hi - duration_2[0]]
    w = np.clip(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]) + 1, 0, None)
    h = np.clip(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]) + 1, 0, None)
    overlap = float((w * h).sum())
    return overlap / (_volume(traj_1) + _volume(traj_2) - overlap)


def voc_ap(rec, prec):
    """Area under the monotone precision envelope (VOC 2010+ average precision; evaluation/common.py `voc_ap`)."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def _prec_rec(hit_scores, n_gt):
    tp = np.isfinite(hit_scores)
    cum_tp = np.cumsum(tp).astype(np.float32)
    cum_fp = np.cumsum(~tp).astype(np.float32)
    eps = np.finfo(np.float32).eps
    return cum_tp / np.maximum(cum_tp + cum_fp, eps), cum_tp / np.maximum(n_gt, eps)


def eval_detection_scores(gt_relations, pred_relations, viou_threshold):
    """Greedy matching in descending score order: a prediction hits the not-yet-detected ground truth of the same triplet
    with the largest min(subject vIoU, object vIoU) >= threshold.  Returns (precision, recall, hit scores: the score of a
    hit, -inf of a miss)."""
    preds = sorted(pred_relations, key=lambda r: r['score'], reverse=True)
    detected = np.zeros(len(gt_relations), dtype=bool)
    hit_scores = np.full(len(preds), -np.inf)
    by_triplet = defaultdict(list)
    for g, rel in enumerate(gt_relations):
        by_triplet[tuple(rel['triplet'])].append(g)
    for p, pred in enumerate(preds):
        best, best_g = -np.inf, -1
        for g in by_triplet.get(tuple(pred['triplet']), ()):
            if detected[g]:
                continue
            gt = gt_relations[g]
            ov = min(viou(pred['sub_traj'], pred['duration'], gt['sub_traj'], gt['duration']),
                     viou(pred['obj_traj'], pred['duration'], gt['obj_traj'], gt['duration']))
            if ov >= viou_threshold and ov > best:
                best, best_g = ov, g
        if best_g >= 0:
            hit_scores[p] = pred['score']
            detected[best_g] = True
    prec, rec = _prec_rec(hit_scores, len(gt_relations))
    return prec, rec, hit_scores


def eval_tagging_scores(gt_relations, pred_relations):
    """Trajectories ignored: the distinct predicted triplets in descending score order against the set of ground-truth
    triplets."""
    preds = sorted(pred_relations, key=lambda r: r['score'], reverse=True)
    gt_triplets = {tuple(r['triplet']) for r in gt_relations}
    seen, hit_scores = set(), []
    for r in preds:
        t = tuple(r['triplet'])
        if t not in seen:
            seen.add(t)
            hit_scores.append(r['score'] if t in gt_triplets else -np.inf)
    hit_scores = np.asarray(hit_scores, dtype=np.float64)
    prec, rec = _prec_rec(hit_scores, len(gt_triplets))
    return prec, rec, hit_scores


def eval_visual_relation(groundtruth, prediction, viou_threshold=0.5, det_nreturns=(50, 100), tag_nreturns=(1, 5, 10)):
    """(mean AP, {n: recall@n}, {n: tagging precision@n}); reference utils/evaluate.py:77-126."""
    video_ap = {}
    tot_scores, tot_tp, prec_at_n = defaultdict(list), defaultdict(list), defaultdict(list)
    tot_gt = 0
    for vid, gt_relations in groundtruth.items():
        if len(gt_relations) == 0:
            continue
        tot_gt += len(gt_relations)
        preds = prediction.get(vid, [])
        det_prec, det_rec, det_scores = eval_detection_scores(gt_relations, preds, viou_threshold)
        video_ap[vid] = voc_ap(det_rec, det_prec)
        tp = np.isfinite(det_scores)
        for n in det_nreturns:
            cut = min(n, det_scores.size)
            tot_scores[n].append(det_scores[:cut])
            tot_tp[n].append(tp[:cut])
        tag_prec, _, _ = eval_tagging_scores(gt_relations, preds)
        for n in tag_nreturns:
            cut = min(n, tag_prec.size)
            prec_at_n[n].append(tag_prec[cut - 1] if cut > 0 else 0.0)
    mean_ap = float(np.mean(list(video_ap.values())))
    rec_at_n = {}
    for n in det_nreturns:
        scores, tps = np.concatenate(tot_scores[n]), np.concatenate(tot_tp[n])
        tps = tps[np.argsort(scores)[::-1]]
        rec = np.cumsum(tps).astype(np.float32) / np.maximum(tot_gt, np.finfo(np.float32).eps)
        rec_at_n[n] = float(rec[-1])
    return mean_ap, rec_at_n, {n: float(np.mean(prec_at_n[n])) for n in tag_nreturns}


def eval_relation(dataset_type, prediction_results=None, json_results_path=None, config=None):
    """reference utils/evaluate.py:128-170, except that a missing ground-truth file is an error: building it needs the
    dataset classes of VidVRD-helper (utils/prepare_eval_labels.py), which are the reference's own job."""
    if prediction_results is None:
        assert json_results_path is not None
        with open(json_results_path) as f:
            prediction_results = json.load(f)
    else:
        assert json_results_path is None
    assert config is not None
    gt_path = config['prepare_gt_config']['gt_relations_path']
    if gt_path is None or not os.path.exists(gt_path):
        raise FileNotFoundError(f"ground-truth relations {gt_path!r} not found: generate them with the reference's "
                                "utils/prepare_eval_labels.py (needs VidVRD-helper's dataset classes)")
    with open(gt_path) as f:
        gt_relations = json.load(f)
    mean_ap, rec_at_n, mprec_at_n = eval_visual_relation(gt_relations, prediction_results,
                                                         viou_threshold=config['inference_config']['viou_th'])
    result = {"RelDet_mAP": mean_ap}
    result.update({f"RelDet_AR@{k}": v for k, v in rec_at_n.items()})
    result.update({f"RelTag_AP@{k}": v for k, v in mprec_at_n.items()})
    return result


def batched_forward_test(model, proposals, max_videos=16, max_pairs=4096):
    """The reference's eval loop (eval.py:136-150: one `model(proposal)` per video) over groups of videos: consecutive
    proposals are grouped until `max_videos` videos or `max_pairs` pairs (a group holds at least one video) and evaluated with
    ONE `model.forward_test_videos` call each.  Yields (proposal, result) in input order; result is what
    `model(proposal)` returns (None for a video without triplets).  Empty proposals ({} / None, which eval.py skips) pass
    through with a None result and take no place in a group."""
    if max_videos < 1 or max_pairs < 1:
        raise ValueError("batched_forward_test: max_videos and max_pairs must be >= 1")
    group, n_pairs = [], 0

    def pairs(p):
        return len(p["sids"])

    def flush():
        results = model.forward_test_videos([p for p in group if p]) if any(group) else []
        it = iter(results)
        for p in group:
            yield p, (next(it) if p else None)

    for p in proposals:
        if p and group and (sum(1 for q in group if q) >= max_videos or n_pairs + pairs(p) > max_pairs):
            yield from flush()
            group, n_pairs = [], 0
        group.append(p)
        if p:
            n_pairs += pairs(p)
    if group:
        yield from flush()


# --------------------------------------------------------------------------------------------------------------------
# Scoring on the device: the vIoU of every (prediction, ground truth) candidate and the greedy matching as two kernels per
# eval call (csrc/vrd_score.hip), reading the tracklet boxes where forward_test's proposals already hold them.  The
# functions above are the reference this path is tested against; the metric arithmetic behind the matching (`_prec_rec`,
# `voc_ap`, `eval_tagging_scores`, the per-n accumulation) is theirs, unchanged.
# --------------------------------------------------------------------------------------------------------------------
_ID_BITS = 14          # every triplet id < 16384: (video, subject, predicate, object) packs into one int64 key


def _triplet_keys(video, triplets):
    """One int64 per relation: the video's index and the three ids of `triplets` (n, 3); equal keys <=> same video and triplet."""
    t = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= 1 << _ID_BITS):
        raise ValueError(f"triplet ids must lie in [0, {1 << _ID_BITS}): got {int(t.min())} .. {int(t.max())}")
    v = np.asarray(video, dtype=np.int64)
    return ((((v << _ID_BITS) | t[:, 0]) << _ID_BITS | t[:, 1]) << _ID_BITS) | t[:, 2]


class RelationGroundTruth:
    """The ground-truth relations `eval_relation` loads ({video: [{triplet, duration, sub_traj, obj_traj}]}) as flat tables,
    uploaded once to `device` (None: host tables only):
      videos            names of the videos with at least one relation, in the file's order (`video_index`: name -> index);
                        `empty_videos`: the names with an empty list -- skipped by the metric, as on the host
      boxes             (rows, 4) f32: every relation's subject track, then its object track, video by video
      relations         (n_gt, 4) int64 [subject's first row, object's first row, first frame, frames], each video's relations
                        in its own order; video v owns relations video_first[v] .. video_first[v + 1] - 1
      triplets          (n_gt, 3) int64 ids through entity_name_to_id / pred_name_to_id (an unknown name is a ValueError)
    Boxes are kept as float32, the format of the tracklet boxes they are compared with.  `dataset_type` "vidor" makes
    `video_key` drop the folder prefix of a video name, as EvaluationFormatConvertor does."""

    def __init__(self, gt_relations, entity_name_to_id, pred_name_to_id, device, dataset_type="vidvrd"):
        self.dataset_type = dataset_type.lower()
        if self.dataset_type not in ("vidvrd", "vidor"):
            raise NotImplementedError(dataset_type)
        self.device = device
        self.videos, self.empty_videos = [], set()
        boxes, relations, triplets, first, row = [], [], [], [0], 0
        for vid, rels in gt_relations.items():
            if len(rels) == 0:
                self.empty_videos.add(vid)
                continue
            self.videos.append(vid)
            for r in rels:
                ids = []
                for name, table, what in zip(r["triplet"], (entity_name_to_id, pred_name_to_id, entity_name_to_id),
                                             ("entity", "predicate", "entity")):
                    if name not in table:
                        raise ValueError(f"RelationGroundTruth: unknown {what} name {name!r} in a relation of video {vid!r}")
                    ids.append(int(table[name]))
                start, end = int(r["duration"][0]), int(r["duration"][1])
                sub = np.asarray(r["sub_traj"], dtype=np.float32).reshape(-1, 4)
                obj = np.asarray(r["obj_traj"], dtype=np.float32).reshape(-1, 4)
                if end < start or len(sub) != end - start or len(obj) != end - start:
                    raise ValueError(f"RelationGroundTruth: a relation of video {vid!r} has duration {(start, end)} but "
                                     f"{len(sub)} subject and {len(obj)} object boxes")
                relations.append((row, row + (end - start), start, end - start))
                row += 2 * (end - start)
                boxes += [sub, obj]
                triplets.append(ids)
            first.append(len(relations))
        self.boxes = np.concatenate(boxes, axis=0) if boxes else np.zeros((0, 4), dtype=np.float32)
        self.relations = np.asarray(relations, dtype=np.int64).reshape(-1, 4)
        self.triplets = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
        self.video_first = np.asarray(first, dtype=np.int64)
        self.video_index = {vid: i for i, vid in enumerate(self.videos)}
        video_of = np.repeat(np.arange(len(self.videos), dtype=np.int64), np.diff(self.video_first))
        keys = _triplet_keys(video_of, self.triplets)
        self._key_order = np.argsort(keys, kind="stable")        # equal keys stay in ascending relation index
        self._keys_sorted = keys[self._key_order]
        self.boxes_dev = self.relations_dev = None
        if device is not None:
            import torch
            self.boxes_dev = torch.from_numpy(self.boxes).to(device)
            self.relations_dev = torch.from_numpy(self.relations).to(device)

    def __len__(self):
        return len(self.relations)

    def video_key(self, video_name):
        """The name the ground truth lists a dataset video under (EvaluationFormatConvertor._reset_video_name)."""
        if self.dataset_type == "vidor":            # "0001_3598080384" -> "3598080384"
            parts = video_name.split('_')
            assert len(parts) == 2
            return parts[1]
        return video_name

    def candidates(self, video, triplets):
        """For predictions with `triplets` (n, 3) of the videos with indices `video` (n,): cand_first (n + 1,) and cand
        (n_cand, 2) int32 [prediction, relation] -- prediction p's candidates, the relations of its video with its triplet, are
        rows cand_first[p] .. cand_first[p + 1] - 1, in ascending relation index."""
        keys = _triplet_keys(video, triplets)
        lo, hi = np.searchsorted(self._keys_sorted, keys, side="left"), np.searchsorted(self._keys_sorted, keys, side="right")
        cand_first = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
        pred_of = np.repeat(np.arange(len(keys), dtype=np.int64), hi - lo)
        within = np.arange(cand_first[-1], dtype=np.int64) - cand_first[pred_of]
        cand = np.stack([pred_of, self._key_order[lo[pred_of] + within]], axis=1).astype(np.int32)
        return cand_first, cand


def _tracklet_boxes(video):
    """A proposal's clamped tracklet boxes as a list of (rows, 4) tensors and the tracklets' first rows in their concatenation:
    from `pair_source`, its plain-tensor fields, or `bboxes_list`."""
    source = video.get("pair_source")
    if source is not None:
        if source.first_row is None:
            raise ValueError("DeviceRelationScorer: the pair_source has no tracklet table (first_row)")
        return [source.boxes], np.asarray(source.first_row, dtype=np.int64)
    if "tracklet_boxes" in video:
        return [video["tracklet_boxes"]], video["tracklet_first_row"].cpu().numpy().astype(np.int64)
    boxes = list(video["bboxes_list"])
    return boxes, np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int64)


class DeviceRelationScorer:
    """`eval_visual_relation` fed by forward_test's results instead of the convertor's records: `add` scores the videos of one
    eval call against a RelationGroundTruth with one vrd_relation_viou and one vrd_match_relations launch (one table upload, one
    copy back), `summary` / `result` return what eval_visual_relation / eval_relation return.  The results need no `so_trajs`
    (MaskVRD.with_so_trajs = False): a prediction's tracks are rows of its proposal's tracklet boxes.
    matcher: a function from the tables of one `add` call to hit (n_pred,) -- >= 0 for a prediction that hits a ground truth
    (the device path gives the relation's index), -1 for a miss; the default is the device path."""

    def __init__(self, ground_truth, viou_threshold=0.5, det_nreturns=(50, 100), tag_nreturns=(1, 5, 10), matcher=None):
        self.gt = ground_truth
        self.viou_threshold = float(viou_threshold)
        self.det_nreturns, self.tag_nreturns = tuple(det_nreturns), tuple(tag_nreturns)
        self.matcher = matcher if matcher is not None else self._device_matcher
        self._det_scores, self._preds = {}, {}          # video index -> hit scores in scoring order / tagging records

    def tables(self, video_names, videos, results):
        """The tables of one `add` call (host arrays), or None when no video of the call has both ground truth and predictions:
          videos      (V,) ground-truth indices of the scored videos, in the call's order
          order       per scored video, the scoring order of its predictions: np.argsort(-score, kind="stable")
          scores      per scored video, its scores in that order (float64)
          pred        (n_pred, 4) int64 [subject's first row, object's first row, first frame, frames] in scoring order, the rows
                      counted in the concatenation of `pred_boxes`; pred_first (V + 1,) int32; triplets (n_pred, 3) likewise
          pred_boxes  list of (rows, 4) box tensors, as the proposals hold them
          cand_first  (n_pred + 1,) int32, cand (n_cand, 2) int32 [prediction, ground-truth relation]
        Videos outside the ground truth (or with an empty relation list there) are ignored; a ground-truth video with a None
        or empty result is recorded as having no prediction."""
        gt = self.gt
        video_names, videos, results = list(video_names), list(videos), list(results)
        if not len(video_names) == len(videos) == len(results):
            raise ValueError("DeviceRelationScorer.add: video_names, videos and results must have one entry per video")
        vids, orders, scores, pred, triplets, boxes, row0 = [], [], [], [], [], [], 0
        for name, video, res in zip(video_names, videos, results):
            v = gt.video_index.get(gt.video_key(name))
            if v is None:
                continue
            if res is None or len(res["triplets"]) == 0:
                self._det_scores[v], self._preds[v] = np.full(0, -np.inf), []
                continue
            score = np.asarray(res["triple_scores_avg"], dtype=np.float64)
            order = np.argsort(-score, kind="stable")       # sorted(key=score, reverse=True): equal scores keep their order
            parts, first_row = _tracklet_boxes(video)
            tids = np.asarray(res["so_tids"], dtype=np.int64).reshape(-1, 2)[order]
            dur = np.asarray(res["pred_durations"], dtype=np.int64).reshape(-1, 2)[order]
            t0 = np.asarray(video["traj_durations"].cpu() if hasattr(video["traj_durations"], "cpu") else video["traj_durations"],
                            dtype=np.int64).reshape(-1, 2)[:, 0]
            frames = dur[:, 1] - dur[:, 0]
            rows = first_row[tids] + dur[:, :1] - t0[tids]                      # the rows MaskVRD._so_trajs slices
            if (frames < 0).any() or (rows < first_row[tids]).any() or (rows + frames[:, None] > first_row[tids + 1]).any():
                raise ValueError(f"DeviceRelationScorer.add: a prediction of video {name!r} lies outside its tracklets' frames")
            pred.append(np.concatenate([rows + row0, dur[:, :1], frames[:, None]], axis=1))
            triplets.append(np.asarray(res["triplets"], dtype=np.int64).reshape(-1, 3)[order])
            vids.append(v)
            orders.append(order)
            scores.append(score[order])
            boxes += parts
            row0 += int(first_row[-1])
            self._preds[v] = [{"triplet": tuple(t), "score": s} for t, s in zip(res["triplets"], score.tolist())]
        if not vids:
            return None
        counts = [len(o) for o in orders]
        triplets = np.concatenate(triplets)
        cand_first, cand = gt.candidates(np.repeat(np.asarray(vids, dtype=np.int64), counts), triplets)
        if cand_first[-1] >= 2 ** 31:
            raise ValueError("DeviceRelationScorer.add: too many candidates for one call")
        return {"videos": np.asarray(vids, dtype=np.int64), "order": orders, "scores": scores,
                "pred": np.concatenate(pred).astype(np.int64), "pred_first": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                "triplets": triplets, "pred_boxes": boxes, "cand_first": cand_first.astype(np.int32), "cand": cand}

    def add(self, video_names, videos, results):
        """Score the videos of one eval call: `videos` are the proposals given to forward_test / forward_test_videos, `results`
        what the model returned for them (None: no prediction), `video_names` the dataset's names."""
        t = self.tables(video_names, videos, results)
        if t is None:
            return
        hit = np.asarray(self.matcher(t))
        assert hit.shape == (len(t["pred"]),)
        for j, v in enumerate(t["videos"].tolist()):
            a, b = t["pred_first"][j], t["pred_first"][j + 1]
            self._det_scores[v] = np.where(hit[a:b] >= 0, t["scores"][j], -np.inf)

    def _device_matcher(self, t):
        import torch
        from . import ops
        gt = self.gt
        if gt.boxes_dev is None:
            raise RuntimeError("DeviceRelationScorer: the ground truth was built without a device (no host fallback)")
        dev = gt.boxes_dev.device
        n_pred, n_cand, n_videos = len(t["pred"]), len(t["cand"]), len(t["videos"])
        parts = [b.to(device=dev, dtype=torch.float32) for b in t["pred_boxes"]]
        boxes = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)).contiguous()
        # every table of the call in one upload: [pred (int64) | cand | pred_first | cand_first (int32)]
        n32 = 2 * n_cand + n_videos + 1 + n_pred + 1
        buf = np.zeros(4 * n_pred + (n32 + 1) // 2, dtype=np.int64)
        buf[:4 * n_pred] = t["pred"].reshape(-1)
        i32 = buf[4 * n_pred:].view(np.int32)
        i32[:2 * n_cand] = t["cand"].reshape(-1)
        i32[2 * n_cand:2 * n_cand + n_videos + 1] = t["pred_first"]
        i32[2 * n_cand + n_videos + 1:n32] = t["cand_first"]
        d = torch.from_numpy(buf).to(dev)
        d32 = d[4 * n_pred:].view(torch.int32)
        cand = d32[:2 * n_cand].view(n_cand, 2)
        ov = ops.relation_viou(boxes, d[:4 * n_pred].view(n_pred, 4), gt.boxes_dev, gt.relations_dev, cand)
        hit = ops.match_relations(d32[2 * n_cand:2 * n_cand + n_videos + 1], d32[2 * n_cand + n_videos + 1:n32], cand, ov,
                                  len(gt), self.viou_threshold)
        return hit.cpu().numpy()

    def summary(self):
        """(mean AP, {n: recall@n}, {n: tagging precision@n}): eval_visual_relation over everything added so far.  A
        ground-truth video never added counts as having no prediction."""
        gt = self.gt
        video_ap = {}
        tot_scores, tot_tp, prec_at_n = defaultdict(list), defaultdict(list), defaultdict(list)
        tot_gt = 0
        for v, vid in enumerate(gt.videos):
            n_gt = int(gt.video_first[v + 1] - gt.video_first[v])
            tot_gt += n_gt
            det_scores = self._det_scores.get(v, np.full(0, -np.inf))
            det_prec, det_rec = _prec_rec(det_scores, n_gt)
            video_ap[vid] = voc_ap(det_rec, det_prec)
            tp = np.isfinite(det_scores)
            for n in self.det_nreturns:
                cut = min(n, det_scores.size)
                tot_scores[n].append(det_scores[:cut])
                tot_tp[n].append(tp[:cut])
            gt_records = [{"triplet": tuple(t)} for t in gt.triplets[gt.video_first[v]:gt.video_first[v + 1]].tolist()]
            tag_prec, _, _ = eval_tagging_scores(gt_records, self._preds.get(v, []))
            for n in self.tag_nreturns:
                cut = min(n, tag_prec.size)
                prec_at_n[n].append(tag_prec[cut - 1] if cut > 0 else 0.0)
        mean_ap = float(np.mean(list(video_ap.values())))
        rec_at_n = {}
        for n in self.det_nreturns:
            scores, tps = np.concatenate(tot_scores[n]), np.concatenate(tot_tp[n])
            tps = tps[np.argsort(scores)[::-1]]
            rec = np.cumsum(tps).astype(np.float32) / np.maximum(tot_gt, np.finfo(np.float32).eps)
            rec_at_n[n] = float(rec[-1])
        return mean_ap, rec_at_n, {n: float(np.mean(prec_at_n[n])) for n in self.tag_nreturns}

    def result(self):
        """The dict of eval_relation."""
        mean_ap, rec_at_n, mprec_at_n = self.summary()
        result = {"RelDet_mAP": mean_ap}
        result.update({f"RelDet_AR@{k}": v for k, v in rec_at_n.items()})
        result.update({f"RelTag_AP@{k}": v for k, v in mprec_at_n.items()})
        return result


def scored_forward_test(model, named_proposals, scorer, max_videos=16, max_pairs=4096):
    """batched_forward_test over (video name, proposal) pairs that also feeds every group's results to `scorer.add`: yields
    what batched_forward_test yields, (proposal, result) in input order."""
    names = []

    class _Scored:
        @staticmethod
        def forward_test_videos(group):
            results = model.forward_test_videos(group)
            scorer.add(names[:len(group)], group, results)
            del names[:len(group)]
            return results

    def proposals():
        for name, p in named_proposals:
            if p:
                names.append(name)
            yield p

    yield from batched_forward_test(_Scored, proposals(), max_videos=max_videos, max_pairs=max_pairs)
