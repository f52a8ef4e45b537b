#!/usr/bin/env python3
"""What training a ragged batch in one row space (`MaskVRD.train_rows`) does to a training step: the step of scripts/train_step.py
(forward, backward, gradient clipping, AdamW, EMA; its own synthetic batches, pair lengths U[8, T]) with the switch off and on, for
the vidor step (48 pairs x 512 frames) and the vidvrd step (24 pairs x 96 frames), eager, f16x3.

The variants of a workload share ONE model and ALTERNATE: a pass times `--steps` steps of every variant in turn and keeps each
variant's median step; the result is the median over `--passes` passes with the spread (min, max) of the pass medians.  `--sweep`
adds a row-space variant per value of TRAIN_ROWS_MIN_ROWS (the bucket-merging threshold of the training plan) -- the value at which
the vidor step is fastest is the default to set.  Per variant also: the form the step took, its bucket table, rows computed
against rows padded, and the library's launches per step (the profiler hooks, in a step of their own behind the timed ones).

    python scripts/train_rows_bench.py --out profiles/train_rows_bench.json
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
sys.path.insert(0, os.path.dirname(HERE))

WORKLOADS = {"vidor": 48, "vidvrd": 24}          # config -> pairs of its training step


def load_train_step():
    spec = importlib.util.spec_from_file_location("train_step", os.path.join(HERE, "train_step.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


class Workload:
    def __init__(self, ts, config, n_pairs, device, seed=0):
        from vrdone_amd import configs, synth
        from vrdone_amd.ema import ModelEma
        from vrdone_amd.models.maskvrd import MaskVRD
        self.cfg = cfg = configs.model_config(config)
        torch.manual_seed(seed)
        self.config, self.n_pairs = config, n_pairs
        self.model = synth.load_synthetic_weights(MaskVRD(cfg, device=device)).to(device).train()
        self.ema = ModelEma(self.model, decay=0.999)
        self.opt = torch.optim.AdamW(ts.param_groups(self.model, 0.05), lr=1e-4)
        self.data = ts.synthetic_batch(cfg, configs.input_channels(cfg), device, n_pairs=n_pairs, seed=seed)
        self.lens = [int(f.shape[1]) for f in self.data["so_features_list"]]

    def step(self, variant):
        self.model.train_rows = variant["rows"]
        if variant["min_rows"] is not None:
            self.model.TRAIN_ROWS_MIN_ROWS = variant["min_rows"]
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

    def describe(self, variant):
        """form, bucket table, rows and launches of one more step of the variant"""
        from vrdone_amd import _hip
        _hip.prof_enable(True)
        _hip.prof_reset()
        try:
            self.step(variant)
            prof = _hip.prof_read()
        finally:
            _hip.prof_enable(False)
            _hip.prof_reset()
        plan = self.model.train_rows_plan(self.lens) if self.model.train_form == "rows" else []
        padded = self.n_pairs * self.cfg["max_seq_len"]
        return {"train_form": self.model.train_form, "buckets": [[len(ids), t, flat] for t, ids, flat in plan], "rows_padded": padded,
                "rows_computed": sum(len(ids) * t for t, ids, _ in plan) if plan else padded,
                "launches_per_step": int(sum(v["launches"] for v in prof.values())),
                "launches_by_family": {k: v["launches"] for k, v in prof.items() if v["launches"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="vidor,vidvrd")
    ap.add_argument("--sweep", default="", help="comma-separated TRAIN_ROWS_MIN_ROWS values: a row-space variant each (besides the default's)")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out")
    args = ap.parse_args()
    from vrdone_amd import ops
    ops.set_precision(args.precision)
    ts = load_train_step()
    variants = [dict(name="batch form (switch off)", rows=False, min_rows=None), dict(name="row space, default threshold", rows=True, min_rows=None)]
    variants += [dict(name=f"row space, TRAIN_ROWS_MIN_ROWS {int(v)}", rows=True, min_rows=int(v)) for v in args.sweep.split(",") if v]
    res = {"what": "one training step (forward, backward, clip, AdamW, EMA) of scripts/train_step.py's synthetic batch, pair lengths U[8, T]; "
                   "wall ms between synchronisations, variants alternating in one process on one model",
           "precision": args.precision, "passes": args.passes, "steps_per_pass": args.steps, "device": torch.cuda.get_device_name(0),
           "workloads": {}}
    for config in args.workloads.split(","):
        work = Workload(ts, config, WORKLOADS[config], "cuda")
        default_min_rows = work.model.TRAIN_ROWS_MIN_ROWS
        runs = [dict(v, min_rows=default_min_rows if v["rows"] and v["min_rows"] is None else v["min_rows"], medians=[]) for v in variants]
        for v in runs:
            for _ in range(args.warmup):
                work.step(v)
        for _ in range(args.passes):
            for v in runs:
                v["medians"].append(statistics.median(work.step(v) for _ in range(args.steps)))
        out = res["workloads"][f"{config} {work.n_pairs} x {work.cfg['max_seq_len']}"] = {"default_TRAIN_ROWS_MIN_ROWS": default_min_rows, "variants": {}}
        for v in runs:
            out["variants"][v["name"]] = dict(median_ms=round(statistics.median(v["medians"]), 3), min_ms=round(min(v["medians"]), 3),
                                              max_ms=round(max(v["medians"]), 3), pass_medians_ms=[round(m, 3) for m in v["medians"]],
                                              **work.describe(v))
        del work
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
