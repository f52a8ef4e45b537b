#!/usr/bin/env python3
"""What feeding a training step costs: the list form (proposals.train_getitem per video on the host, the lists moved to the
device, `scripts/train_step.py --entry-lists`) against the device form (proposals.train_tables + a device-resident TrainSource,
`--device-source`), alternating in one GPU visit, one process per run, the order flipped on the second pair; the first process of
a visit runs cold (LABNOTES) and is discarded.  Per run: the median over steps 2 .. 11 of `data_ms` (cache entries -> what
model(...) is handed, between two synchronisations), of `step_ms` (the step itself, batch assembly on the device included) and
of their sum.  The steps replay the network as HIP graphs (`--graphs`) unless --eager.

--baseline-tree DIR: the list form's runs use DIR/scripts/train_step.py -- a checkout of the parent commit with ITS library
built and this commit's scripts/train_step.py copied over its own (the list feed calls nothing the parent lacks); the list form on
this commit's library is then run once more per workload for comparison.

    python scripts/train_source_ab.py --baseline-tree ../parent --out profiles/r10_train_source_ab.json      # on the GPU box
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WORKLOADS = {"vidvrd_24x96": [], "vidor_48x512": ["--config", "vidor", "--pairs", "48"]}
FEEDS = {"lists": ["--entry-lists"], "source": ["--device-source"]}


def one_run(workload, feed, steps, limit, graphs, tree=None):
    script = os.path.join(tree, "scripts", "train_step.py") if tree else os.path.join(HERE, "train_step.py")
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, script, "--steps", str(steps)] + (["--graphs"] if graphs else [])
    out = subprocess.run(cmd + WORKLOADS[workload] + FEEDS[feed], capture_output=True, text=True)
    if out.returncode != 0:                    # a failed run ends the visit: nothing more is started on the device
        sys.exit(f"{workload} / {feed} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    log = json.loads(out.stdout.strip().splitlines()[-1])
    steady = slice(2, steps)
    total = [d + s for d, s in zip(log["data_ms"], log["step_ms"])]
    med = lambda xs: round(statistics.median(xs[steady]), 3)          # noqa: E731
    res = {"data_ms": med(log["data_ms"]), "step_ms": med(log["step_ms"]), "data_plus_step_ms": med(total),
           "data_ms_min": round(min(log["data_ms"][steady]), 3), "data_ms_max": round(max(log["data_ms"][steady]), 3),
           "final_loss": log["total_loss"][-1]}
    if "source_upload_ms" in log:
        res["source_upload_ms"] = round(log["source_upload_ms"], 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=2, help="lists / source pairs per workload")
    ap.add_argument("--limit", type=int, default=300, help="seconds a run may take")
    ap.add_argument("--eager", action="store_true", help="eager steps instead of HIP-graph replays")
    ap.add_argument("--baseline-tree", default=None)
    args = ap.parse_args()
    graphs = not args.eager
    base = "lists_parent_library" if args.baseline_tree else "lists"
    result = {"steps": args.steps, "steady_steps": f"2..{args.steps - 1}", "graphs": graphs, "baseline": base, "workloads": {}}
    one_run("vidvrd_24x96", "lists", args.steps, args.limit, graphs, args.baseline_tree)              # the cold first process: discarded
    for workload in WORKLOADS:
        runs = {base: [], "source": []}
        for r in range(args.rounds):
            for form in ((base, "source") if r % 2 == 0 else ("source", base)):
                runs[form].append(one_run(workload, "source" if form == "source" else "lists", args.steps, args.limit, graphs,
                                          args.baseline_tree if form == base else None))
        if args.baseline_tree:
            runs["lists"] = [one_run(workload, "lists", args.steps, args.limit, graphs)]
        spread = {k: round(max(max(r[k] for r in runs[f]) - min(r[k] for r in runs[f]) for f in (base, "source")), 3)
                  for k in ("data_ms", "step_ms", "data_plus_step_ms")}
        result["workloads"][workload] = {"runs": runs, "run_to_run_spread": spread}
        print(workload, json.dumps(result["workloads"][workload]), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
