#!/usr/bin/env python3
"""Training golden at 16 heads (head_dim 32, global attention) from the REAL reference (build container only), on the CPU.

    python scripts/make_golden_h16_train.py

One training step of case `vidvrd_h16` of tests/local_heads_cases.py (vidvrd.yaml with n_head = fuse_head = 16) on the batch
LH.TRAIN_C256, stochastic depth off, the matcher's assignments recorded, gradients sampled with LW.GRAD_STRIDE: the pattern of
train_case() in scripts/make_golden_heads.py, whose helpers this imports.  Writes under tests/golden/
  train_step_vidvrd_h16.json, _a.npz, _b.npz, ...   (format of train_step_vidvrd_c256.*; as many parts as keep each one no larger
                                                     than the parts of train_step_vidvrd_w5_*)
"""
import os
os.environ.setdefault("PYTORCH_JIT", "0")
import json
import string
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_heads import LH, MT, OUT, build, load_cfg, ref_blocks      # noqa: E402  (puts the reference on sys.path)

CASE = "vidvrd_h16"
STEM = "train_step_" + CASE


def part_limit():
    return max(os.path.getsize(os.path.join(OUT, f"train_step_vidvrd_w5_{p}.npz")) for p in "ab")


def train_case():
    spec = LH.MODEL_CASES[CASE]
    _, mc = load_cfg(spec["base"] + ".yaml")
    mc = LH.model_config(mc, CASE)
    model, keys, _ = build(mc)
    for p in model.parameters():
        p.requires_grad_(True)
    lens, data = MT.batch(mc, **LH.TRAIN_C256)
    orig = ref_blocks.drop_path
    ref_blocks.drop_path = lambda x, drop_prob=0.0, training=False: x
    recorded = []
    real_match = model.bipartite_match

    def match(*a, **kw):
        idx, lm = real_match(*a, **kw)
        recorded.append([[i.tolist(), j.tolist()] for i, j in idx])
        return idx, lm
    model.bipartite_match = match
    loss = MT.run(model, data)
    del model.bipartite_match
    ref_blocks.drop_path = orig
    grads, stats = [], {}
    for name, p in model.named_parameters():
        g = p.grad.detach()
        stats[name] = [float(g.double().sum()), float(g.double().abs().sum()), float(g.double().norm())]
        grads.append((f"nodrop/{name}", LH.sample(g).numpy().copy()))
    meta = {"B": LH.TRAIN_C256["B"], "T": LH.TRAIN_C256["T"], "lengths": lens, "sample_stride": LH.LW.GRAD_STRIDE, "state_keys": keys,
            "cases": {"nodrop": {"losses": {k: float(v.detach()) for k, v in loss.items()}, "grad_stats": stats, "indices": recorded}}}
    limit = part_limit()
    for n_parts in range(2, len(string.ascii_lowercase) + 1):
        for f in os.listdir(OUT):
            if f.startswith(STEM + "_") and f.endswith(".npz"):
                os.remove(os.path.join(OUT, f))
        sizes = []
        for i in range(n_parts):
            path = os.path.join(OUT, f"{STEM}_{string.ascii_lowercase[i]}.npz")
            np.savez_compressed(path, **dict(grads[i::n_parts]))
            sizes.append(os.path.getsize(path))
        if max(sizes) <= limit:
            break
    else:
        raise SystemExit("no split keeps the parts inside the limit")
    with open(os.path.join(OUT, STEM + ".json"), "w") as f:
        json.dump(meta, f)
    print(CASE, "total_loss", float(loss["total_loss"]), "parts", sizes, "limit", limit)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_grad_enabled(True)
    train_case()
