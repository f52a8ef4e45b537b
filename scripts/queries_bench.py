#!/usr/bin/env python3
"""What the query count costs, and that lifting its cap costs the shipped configs nothing.

Workloads (vidvrd.yaml, default precision): the 24-pair training step of scripts/train_step.py (forward, backward, gradient
clipping, AdamW, EMA), eager and as HIP graphs, and forward_test on a 226-pair synthetic video (16 tracklets, 20-90 frames).

  * at `predictor.num_queries` = 9 on two checkouts, `--parent DIR` (built) and this one: a worker process per checkout, both kept
    alive, the passes ALTERNATING between them; each 9-query timing of this checkout has to lie inside the parent's own pass spread;
  * for information at 24 and 64 queries on this checkout, the training step with the device tail (fused criterion, vrd_assign ->
    vrd_assign_wave) and with `model.device_matching = False` (costs to the host, scipy per pair: where such a model went before
    the device tail took more than 16 queries).

A pass times `--steps` steps / calls of every variant in turn and keeps each variant's median; the result is the median over
`--passes` passes with the spread (min, max) of the pass medians.

    python scripts/queries_bench.py --parent /path/to/parent/checkout --out profiles/queries_bench.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.environ.get("VRDONE_TREE", os.path.dirname(HERE))


def load_train_step():
    spec = importlib.util.spec_from_file_location("train_step", os.path.join(TREE, "scripts", "train_step.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


def config(Q):
    from vrdone_amd import configs
    cfg = configs.model_config("vidvrd")
    return cfg if Q == cfg["predictor"]["num_queries"] else dict(cfg, predictor=dict(cfg["predictor"], num_queries=Q))


class TrainVariant:
    def __init__(self, ts, Q, graphs, device_tail):
        import torch
        from vrdone_amd import configs, synth
        from vrdone_amd.ema import ModelEma
        from vrdone_amd.models.maskvrd import MaskVRD
        cfg = config(Q)
        torch.manual_seed(0)
        self.name = f"train Q={Q} {'graphs' if graphs else 'eager'}" + ("" if device_tail else " host matching")
        self.model = synth.load_synthetic_weights(MaskVRD(cfg, device="cuda")).to("cuda").train()
        self.model.device_matching = device_tail
        if graphs:
            self.model.enable_training_graphs()
        self.ema = ModelEma(self.model, decay=0.999)
        self.opt = torch.optim.AdamW(ts.param_groups(self.model, 0.05), lr=1e-4)
        self.data = ts.synthetic_batch(cfg, configs.input_channels(cfg), "cuda", n_pairs=24, seed=0)
        self.torch = torch

    def step(self):
        torch = self.torch
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


class EvalVariant:
    def __init__(self, Q):
        import torch
        from vrdone_amd import configs, synth
        from vrdone_amd.models.maskvrd import MaskVRD
        cfg = config(Q)
        self.name = f"forward_test Q={Q} 226 pairs"
        self.model = synth.load_synthetic_weights(MaskVRD(cfg, device="cuda")).to("cuda").eval()
        self.model._config_eval(configs.inference_config("vidvrd"))
        self.data = synth.synth_video(16, configs.input_channels(cfg), 20, 90, seed=3, device="cuda")
        assert len(self.data["sids"]) == 226
        self.torch = torch

    def step(self):
        torch = self.torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            self.model(self.data)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def worker(queries, steps, warmup):
    """One checkout's variants; a pass per line read from stdin, its medians as one JSON line on stdout."""
    sys.path.insert(0, TREE)
    ts = load_train_step()
    variants = []
    for Q in queries:
        tails = (True,) if Q <= 16 else (True, False)
        variants += [TrainVariant(ts, Q, graphs, tail) for tail in tails for graphs in (False, True)]
        variants.append(EvalVariant(Q))
    for v in variants:
        for _ in range(warmup):                  # (records the graphs)
            v.step()
    print(json.dumps({"ready": [v.name for v in variants]}), flush=True)
    for line in sys.stdin:
        if line.strip() != "pass":
            break
        print(json.dumps({v.name: statistics.median(v.step() for _ in range(steps)) for v in variants}), flush=True)


def start(tree, queries, args):
    env = dict(os.environ, VRDONE_TREE=tree)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--queries", ",".join(map(str, queries)), "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=tree)
    return p, read_json(p)["ready"]


def read_json(p):
    """the worker's next JSON line (anything else a library prints on stdout is passed on)"""
    while True:
        line = p.stdout.readline()
        if not line:
            raise RuntimeError("a worker ended early")
        if line.startswith("{"):
            return json.loads(line)
        sys.stderr.write(line)


def one_pass(p):
    p.stdin.write("pass\n")
    p.stdin.flush()
    return read_json(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (omit: this checkout alone)")
    ap.add_argument("--queries", default="9,24,64")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    queries = [int(q) for q in args.queries.split(",")]
    if args.worker:
        return worker(queries, args.steps, args.warmup)
    procs = {}
    if args.parent:
        procs["parent"] = start(os.path.abspath(args.parent), [q for q in queries if q <= 16], args)
    procs["this"] = start(os.path.dirname(HERE), queries, args)
    medians = {side: {name: [] for name in names} for side, (_, names) in procs.items()}
    for _ in range(args.passes):
        for side, (p, _) in procs.items():       # parent, this, parent, this, ...
            for name, ms in one_pass(p).items():
                medians[side][name].append(ms)
    for p, _ in procs.values():
        p.stdin.close()
        p.wait(timeout=60)
    import torch
    res = {"what": "vidvrd.yaml: 24 pairs x 96 frames, one training step (forward, backward, clip, AdamW, EMA); forward_test on a 226-pair "
                   "video; wall ms between synchronisations, median over the passes of each pass's median, passes alternating "
                   "between the checkouts",
           "passes": args.passes, "steps_per_pass": args.steps, "device": torch.cuda.get_device_name(0), "checkouts": {}}
    for side, per in medians.items():
        res["checkouts"][side] = {name: {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                                         "pass_medians_ms": [round(m, 3) for m in ms]} for name, ms in per.items()}
    if "parent" in res["checkouts"]:
        res["inside_parent_spread"] = {}
        for name, ref in res["checkouts"]["parent"].items():
            mine = res["checkouts"]["this"][name]["median_ms"]
            res["inside_parent_spread"][name] = bool(ref["min_ms"] <= mine <= ref["max_ms"]) or mine < ref["min_ms"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
