#!/usr/bin/env python3
"""Cost of the deterministic mode (vrdone_amd/ops.py set_deterministic): default and deterministic training steps alternating in
one process, on the vidvrd 24-pair x 96-frame batch of scripts/train_step.py and the vidor 48-pair x 512-frame one, eagerly
and with enable_training_graphs().  Per mode: median and spread of forward + backward wall ms and (eager) the BACKWARD-family
kernel ms from the library's HIP-event profiler.

    python scripts/determinism_ab.py --rounds 15 --out profiles/r08_deterministic_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def summary(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 3), "min": round(xs[0], 3), "max": round(xs[-1], 3),
            "p25": round(xs[len(xs) // 4], 3), "p75": round(xs[(3 * len(xs)) // 4], 3), "n": len(xs)}


def measure(config, n_pairs, graphs, rounds, warmup):
    import train_step
    from vrdone_amd import _hip, configs, ops, synth
    from vrdone_amd.models.maskvrd import MaskVRD
    cfg = configs.model_config(config)
    torch.manual_seed(0)
    model = synth.load_synthetic_weights(MaskVRD(cfg, device="cuda")).to("cuda").train()
    if graphs:
        model.enable_training_graphs()
    data = train_step.synthetic_batch(cfg, configs.input_channels(cfg), "cuda", n_pairs=n_pairs)
    out = {mode: {"step_ms": [], "backward_kernel_ms": []} for mode in ("default", "deterministic")}
    for i in range(warmup + rounds):
        for mode in ("default", "deterministic") if i % 2 == 0 else ("deterministic", "default"):
            with ops.use_deterministic(mode == "deterministic"):
                if not graphs:
                    _hip.prof_enable(True)
                    _hip.prof_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = model(data)
                model.zero_grad(set_to_none=True)
                loss["total_loss"].backward()
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0)
                if not graphs:
                    bwd = _hip.prof_read()["backward"]["ms"]
                    _hip.prof_enable(False)
            if i >= warmup:
                out[mode]["step_ms"].append(ms)
                if not graphs:
                    out[mode]["backward_kernel_ms"].append(bwd)
    res = {}
    for mode, d in out.items():
        res[mode] = {"step_ms": summary(d["step_ms"])}
        if d["backward_kernel_ms"]:
            res[mode]["backward_kernel_ms"] = summary(d["backward_kernel_ms"])
    res["step_cost_pct"] = round(100.0 * (res["deterministic"]["step_ms"]["median"] / res["default"]["step_ms"]["median"] - 1.0), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vrdone_amd import ops
    result = {"what": "forward + backward of one training step, default vs deterministic mode alternating in one process",
              "precision": ops.get_precision(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "workloads": {}}
    for name, config, n_pairs in (("vidvrd_24x96", "vidvrd", 24), ("vidor_48x512", "vidor", 48)):
        for graphs in (False, True):
            key = f"{name}_{'graphs' if graphs else 'eager'}"
            result["workloads"][key] = measure(config, n_pairs, graphs, args.rounds, args.warmup)
            print(key, json.dumps(result["workloads"][key]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v["step_cost_pct"] for k, v in result["workloads"].items()}))


if __name__ == "__main__":
    main()
