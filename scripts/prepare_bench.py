#!/usr/bin/env python3
"""What preparing eval proposals costs, per video: the host path (vrdone_amd.proposals.prepare_test_proposal, one call per
video: box clamp, vIoU de-dup and pair tables as Python loops, then the upload) against the device path (prepare_test_videos,
one call for all videos of the workload: one upload, four launches, one copy back).  Synthetic vidvrd-sized videos
(vrdone_amd.synth.synth_raw_video with n_categories / n_shadowed, so that the de-dup has same-category pairs to compare and
tracklets to drop), visual width of the vidvrd config, tracklets of up to 256 frames:
  small   16 videos of 10-12 tracklets over 3 categories, 2 of them shadowed copies
  large   one video of 46 tracklets over 5 categories, 6 of them shadowed copies
Each figure is the median of `--reps` timed passes after a warm-up pass, the two variants taken in turn within every repetition;
a pass is `--inner` repeats of the variant (host clock around work that ends in a device synchronise), `spread` is (max - min) /
median of a variant's passes.  The host time is the yardstick: the same code as before the device path existed, in the same run
on the same box.  The proposals of the two paths must be equal.  Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vrdone_amd import configs, synth  # noqa: E402
from vrdone_amd.proposals import _clamped, prepare_test_proposal, prepare_test_videos, shadowed_tracklets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.reps >= 7
assert torch.cuda.is_available(), "the device path needs the GPU: there is nothing to compare without it"
torch.set_grad_enabled(False)
DEV = torch.device("cuda")
cfg, ic = configs.model_config("vidvrd"), configs.inference_config("vidvrd")
V, STRIDE, MIN_FRAMES = cfg["visual_dim"], ic["feat_stride"], 2
SIZES = [(640, 360), (1280, 720), (1920, 1080), (480, 640), (320, 240)]

WORKLOADS = {
    "small": [synth.synth_raw_video(8 + i % 3, V, 40, 256, seed=500 + i, wh=SIZES[i % len(SIZES)], n_categories=3, n_shadowed=2)
              for i in range(16)],
    "large": [synth.synth_raw_video(40, V, 40, 256, seed=900, n_categories=5, n_shadowed=6)],
}


def same(a, b):
    if not a or not b:
        return a == b
    sa, sb = a["pair_source"], b["pair_source"]
    return (all(torch.equal(a[k], b[k]) for k in ("sids", "oids", "so_offset")) and sa.lens == sb.lens and
            all(torch.equal(x, y) for x, y in zip(a["bboxes_list"], b["bboxes_list"])) and
            all(torch.equal(getattr(sa, k), getattr(sb, k)) for k in ("vis", "boxes", "s_row", "o_row", "lens_dev")) and
            sa.first_row.tolist() == sb.first_row.tolist())


rows = []
for name, raws in WORKLOADS.items():
    def host():
        return [prepare_test_proposal(r, STRIDE, 0, MIN_FRAMES, DEV) for r in raws]

    def device():
        return prepare_test_videos(raws, STRIDE, 0, MIN_FRAMES, DEV)

    variants = [("host", host), ("device", device)]
    out = {k: fn() for k, fn in variants}                          # warm-up pass
    times = {k: [] for k, _ in variants}
    for _ in range(args.reps):
        for k, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.inner)
    dropped = [len(shadowed_tracklets([_clamped(b, *r["video_wh"]) for b in r["bboxes_list"]],
                                      [tuple(s) for s in r["traj_durations"].tolist()], r["cat_ids"].tolist())) for r in raws]
    row = {"workload": name, "videos": len(raws), "tracklets": [len(r["bboxes_list"]) for r in raws],
           "categories": max(len(set(r["cat_ids"].tolist())) for r in raws), "tracklets_dropped": sum(dropped),
           "candidate_pairs": sum(len(r["sids"]) for r in raws), "kept_pairs": sum(len(p["sids"]) for p in out["host"] if p),
           "tracklet_rows": sum(sum(len(b) for b in r["bboxes_list"]) for r in raws),
           "device_proposals_equal_host": all(same(a, b) for a, b in zip(out["device"], out["host"]))}
    for k, _ in variants:
        t = sorted(times[k])
        med = t[len(t) // 2]
        row[k] = {"ms_per_video": round(med * 1e3 / len(raws), 3), "ms_per_call": round(med * 1e3 / (len(raws) if k == "host" else 1), 3),
                  "spread": round((t[-1] - t[0]) / med, 3)}
    row["host_over_device"] = round(row["host"]["ms_per_video"] / row["device"]["ms_per_video"], 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
doc = {"what": "eval proposal preparation per video: host prepare_test_proposal per video against one prepare_test_videos call "
               "(scripts/prepare_bench.py)",
       "config": "vidvrd", "visual_dim": V, "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "rows": rows}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
