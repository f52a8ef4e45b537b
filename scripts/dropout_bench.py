#!/usr/bin/env python3
"""What attention / projection dropout costs a training step: the vidvrd 24-pair step of scripts/train_step.py (forward, backward,
gradient clipping, AdamW, EMA) at (dropattn, dropout) = (0.1, 0.1) against (0, 0), eager and as HIP graphs.

The variants ALTERNATE: a pass times `--steps` steps of every (rates, graphs) variant in turn and keeps each variant's median step;
the result is the median over `--passes` passes with the spread (min, max) of the pass medians.  `--rates 0` measures the (0, 0)
variants only -- that form runs on a checkout without the feature too, for the comparison with the parent commit.

    python scripts/dropout_bench.py --out profiles/dropout_train_step.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("VRDONE_TREE", os.path.dirname(HERE)))


def load_train_step():
    spec = importlib.util.spec_from_file_location("train_step", os.path.join(os.environ.get("VRDONE_TREE", os.path.dirname(HERE)), "scripts",
                                                                             "train_step.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


class Variant:
    def __init__(self, ts, rates, graphs, device, seed=0):
        from vrdone_amd import configs, synth
        from vrdone_amd.ema import ModelEma
        from vrdone_amd.models.maskvrd import MaskVRD
        cfg = configs.model_config("vidvrd")
        if any(rates):
            cfg = dict(cfg, dropattn=rates[0], dropout=rates[1])
        torch.manual_seed(seed)
        self.name = f"dropattn {rates[0]}, dropout {rates[1]}, {'graphs' if graphs else 'eager'}"
        self.model = synth.load_synthetic_weights(MaskVRD(cfg, device=device)).to(device).train()
        if graphs:
            self.model.enable_training_graphs()
        self.ema = ModelEma(self.model, decay=0.999)
        self.opt = torch.optim.AdamW(ts.param_groups(self.model, 0.05), lr=1e-4)
        self.data = ts.synthetic_batch(cfg, configs.input_channels(cfg), device, n_pairs=24, seed=seed)
        self.medians = []

    def step(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = self.model(self.data)
        self.opt.zero_grad(set_to_none=True)
        loss["total_loss"].backward()
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), 1.0)
        self.opt.step()
        self.ema.update(self.model)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rates", default="0,0.1", help="comma-separated rates r: the variants (dropattn, dropout) = (r, r)")
    ap.add_argument("--out")
    args = ap.parse_args()
    ts = load_train_step()
    rates = [float(r) for r in args.rates.split(",")]
    variants = [Variant(ts, (r, r), graphs, "cuda") for graphs in (False, True) for r in rates]
    for v in variants:
        for _ in range(args.warmup):            # (records the graphs)
            v.step()
    for _ in range(args.passes):
        for v in variants:
            v.medians.append(statistics.median(v.step() for _ in range(args.steps)))
    res = {"what": "vidvrd 24 pairs x 96 frames, one training step (forward, backward, clip, AdamW, EMA), wall ms between synchronisations",
           "passes": args.passes, "steps_per_pass": args.steps, "device": torch.cuda.get_device_name(0), "variants": {}}
    for v in variants:
        res["variants"][v.name] = {"median_ms": round(statistics.median(v.medians), 3), "min_ms": round(min(v.medians), 3),
                                   "max_ms": round(max(v.medians), 3), "pass_medians_ms": [round(m, 3) for m in v.medians]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
