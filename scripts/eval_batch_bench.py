#!/usr/bin/env python3
"""Videos per second of the eval call on many small videos: one MaskVRD.forward_test per video (the reference eval.py's
batch_size=1 loop) against MaskVRD.forward_test_videos over groups of up to `max_videos` videos
(vrdone_amd.evaluate.batched_forward_test).  Synthetic videos of the sizes vidvrd / vidor mostly have (4-16 tracklets of
10-60 or 20-90 frames, a few dozen to a few hundred pairs) and mixed frame sizes, built from per-tracklet features on the
device (proposals.prepare_test_proposal).  Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vrdone_amd import _hip, configs, ops, synth  # noqa: E402
from vrdone_amd.evaluate import batched_forward_test  # noqa: E402
from vrdone_amd.models.maskvrd import MaskVRD  # noqa: E402
from vrdone_amd.proposals import prepare_test_proposal  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=64)
ap.add_argument("--max-videos", default="1,4,8,16,32")
ap.add_argument("--reps", type=int, default=3, help="timed passes over the video set per variant (the median is reported)")
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


def video_set(frames, seed0):
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


def timed(fn):
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2]


def launches(fn):
    _hip.prof_enable(True)
    _hip.prof_reset()
    fn()
    torch.cuda.synchronize()
    prof = _hip.prof_read()
    _hip.prof_enable(False)
    return sum(v["launches"] for v in prof.values()), sum(v["ms"] for v in prof.values())


rows = []
for frames, seed in (((10, 60), 1000), ((20, 90), 2000)):
    vids = video_set(frames, seed)
    n_pairs = [len(v["sids"]) for v in vids]
    per_video = lambda: [model.forward_test(v) for v in vids]                                    # noqa: E731
    want = per_video()                                     # (warm-up: operand caches, first-call stream pools)
    variants = [("per_video_loop", None, per_video)]
    for mv in [int(x) for x in args.max_videos.split(",")]:
        variants.append(("forward_test_videos", mv, lambda mv=mv: [r for _, r in batched_forward_test(model, vids, max_videos=mv)]))
    for name, mv, fn in variants:
        got = fn()
        same = all((a is None and b is None) or (a is not None and b is not None and a["triplets"] == b["triplets"])
                   for a, b in zip(got, want))
        dt = timed(fn)
        n_launch, kernel_ms = launches(fn)
        rows.append({"frames": f"{frames[0]}-{frames[1]}", "videos": len(vids), "mean_pairs": round(sum(n_pairs) / len(vids), 1),
                     "max_pairs": max(n_pairs), "variant": name, "max_videos": mv, "ms_per_video": round(dt * 1e3 / len(vids), 3),
                     "videos_per_s": round(len(vids) / dt, 1), "pairs_per_s": round(sum(n_pairs) / dt),
                     "hip_launches_per_video": round(n_launch / len(vids), 1), "hip_kernel_ms_per_video": round(kernel_ms / len(vids), 3),
                     "triplets_equal_per_video_loop": same})
        print(json.dumps(rows[-1]), flush=True)
doc = {"what": "eval throughput on small synthetic videos: per-video forward_test against forward_test_videos (scripts/eval_batch_bench.py)",
       "precision": args.precision, "config": "vidvrd", "device": torch.cuda.get_device_name(0), "rows": rows}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
