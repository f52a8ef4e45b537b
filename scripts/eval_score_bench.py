#!/usr/bin/env python3
"""What scoring an eval sweep costs, per video, on the video set of scripts/eval_batch_bench.py (64 synthetic vidvrd videos, 16
per forward_test_videos call) against a synthetic ground truth of ~20 relations per video made from the model's own predictions
(vrdone_amd.synth.synth_relation_ground_truth):
  (a) host_scoring      EvaluationFormatConvertor.to_eval_format_pr per video + eval_visual_relation (the results precomputed)
  (b) device_scoring    DeviceRelationScorer.add per group of 16 + summary() (the same results; ground truth already uploaded)
  (c) forward_so_trajs  forward_test_videos as it is by default
  (d) forward_bare      forward_test_videos with model.with_so_trajs = False
Each figure is the median of `--reps` timed passes after a warm-up pass, the four variants taken in turn within every repetition
(host clock around work that ends in a device synchronise); `spread` is (max - min) / median of a variant's passes.  The
metric of (b) must equal that of (a).  Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vrdone_amd import _hip, configs, ops, synth  # noqa: E402
from vrdone_amd import evaluate as E  # noqa: E402
from vrdone_amd.models.maskvrd import MaskVRD  # noqa: E402
from vrdone_amd.proposals import prepare_test_proposal  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=64)
ap.add_argument("--max-videos", type=int, default=16)
ap.add_argument("--relations", type=int, default=20, help="ground-truth relations drawn per video")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--precision", default="f16x3")
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
ops.set_precision(args.precision)
cfg = configs.model_config("vidvrd")
ic = configs.inference_config("vidvrd")
model = synth.load_synthetic_weights(MaskVRD(cfg, device="cuda")).cuda().eval()
model._config_eval(ic)
SIZES = [(640, 360), (1280, 720), (1920, 1080), (480, 640), (320, 240)]


def video_set(frames, seed0):                 # (the set of scripts/eval_batch_bench.py)
    g = torch.Generator().manual_seed(seed0)
    out = []
    while len(out) < args.videos:
        n = int(torch.randint(4, 17, (1,), generator=g))
        raw = synth.synth_raw_video(n, model.backbone.n_visual, frames[0], frames[1], seed=seed0 + len(out) * 7 + n,
                                    wh=SIZES[len(out) % len(SIZES)])
        prop = prepare_test_proposal(raw, ic["feat_stride"], 0, 2, torch.device("cuda"))
        if prop:
            out.append(prop)
    return out


def forward(vids):
    return [r for _, r in E.batched_forward_test(model, vids, max_videos=args.max_videos)]


rows = []
for frames, seed in (((10, 60), 1000), ((20, 90), 2000)):
    vids = video_set(frames, seed)
    names = [f"video{i:04d}" for i in range(len(vids))]
    results = forward(vids)
    entity = {i: f"entity{i}" for i in range(64)}
    pred = {i: f"pred{i}" for i in range(cfg["num_classes"] + 1)}
    doc = synth.synth_relation_ground_truth(names, vids, results, entity, pred, per_video=args.relations, seed=seed)
    conv = E.EvaluationFormatConvertor("vidvrd", entity, pred)
    gt = E.RelationGroundTruth(doc, {v: k for k, v in entity.items()}, {v: k for k, v in pred.items()}, "cuda")
    groups = [slice(i, i + args.max_videos) for i in range(0, len(vids), args.max_videos)]

    def host_scoring():
        prediction = {}
        for name, res in zip(names, results):
            prediction.update(conv.to_eval_format_pr(name, res))
        return E.eval_visual_relation(doc, prediction, viou_threshold=ic["viou_th"])

    def device_scoring():
        scorer = E.DeviceRelationScorer(gt, viou_threshold=ic["viou_th"])
        for s in groups:
            scorer.add(names[s], vids[s], results[s])
        return scorer.summary()

    def forward_bare():
        model.with_so_trajs = False
        try:
            return forward(vids)
        finally:
            del model.with_so_trajs

    variants = [("host_scoring", host_scoring), ("device_scoring", device_scoring), ("forward_so_trajs", lambda: forward(vids)),
                ("forward_bare", forward_bare)]
    out = {name: fn() for name, fn in variants}                  # warm-up pass
    same_metric = out["host_scoring"] == out["device_scoring"]
    same_results = out["forward_bare"] == [r and {k: v for k, v in r.items() if k != "so_trajs"} for r in out["forward_so_trajs"]]
    times = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    _hip.prof_enable(True)
    _hip.prof_reset()
    device_scoring()
    torch.cuda.synchronize()
    post = _hip.prof_read()["postprocess"]
    _hip.prof_enable(False)
    row = {"frames": f"{frames[0]}-{frames[1]}", "videos": len(vids), "videos_per_call": args.max_videos,
           "predictions": sum(len(r["triplets"]) for r in results if r), "ground_truths": len(gt),
           "metric": {"mAP": out["host_scoring"][0], "recall": out["host_scoring"][1], "tagging": out["host_scoring"][2]},
           "device_metric_equals_host": same_metric, "bare_results_equal_default": same_results,
           "scoring_kernel_launches_per_pass": post["launches"], "scoring_kernel_ms_per_video": round(post["ms"] / len(vids), 4)}
    for name, _ in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        row[name] = {"ms_per_video": round(med * 1e3 / len(vids), 3), "spread": round((t[-1] - t[0]) / med, 3)}
    rows.append(row)
    print(json.dumps(row), flush=True)
doc = {"what": "eval scoring per video: host convertor + eval_visual_relation against DeviceRelationScorer, and forward_test_videos "
               "with and without so_trajs (scripts/eval_score_bench.py)",
       "precision": args.precision, "config": "vidvrd", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
