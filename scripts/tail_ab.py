#!/usr/bin/env python3
"""What clip + AdamW cost a training step: torch's clip_grad_norm_ + AdamW.step against vrdone_amd.optim.FusedAdamW
(`scripts/train_step.py --fused-tail`), alternating in one GPU visit, one process per run; torch's own AdamW(fused=True) once as a
second baseline.  The first process of a visit runs cold (LABNOTES) and is discarded.  Per run: the median over steps 2 .. 11 of
`tail_ms` (wall time of clip + step between two synchronisations) and of `step_ms`.

    python scripts/tail_ab.py --out profiles/r09_tail_ab.json          # on the GPU box
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WORKLOADS = {"vidvrd_24x96": [], "vidor_48x512": ["--config", "vidor", "--pairs", "48"]}
TAILS = {"torch": [], "fused": ["--fused-tail"], "torch_fused": ["--torch-fused"]}


def one_run(workload, tail, steps, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(HERE, "train_step.py"), "--steps", str(steps)]
    out = subprocess.run(cmd + WORKLOADS[workload] + TAILS[tail], capture_output=True, text=True)
    if out.returncode != 0:                    # a failed run ends the visit: nothing more is started on the device
        sys.exit(f"{workload} / {tail} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    log = json.loads(out.stdout.strip().splitlines()[-1])
    steady = slice(2, steps)
    return {"tail_ms": round(statistics.median(log["tail_ms"][steady]), 3), "step_ms": round(statistics.median(log["step_ms"][steady]), 3),
            "tail_ms_min": round(min(log["tail_ms"][steady]), 3), "tail_ms_max": round(max(log["tail_ms"][steady]), 3),
            "final_loss": log["total_loss"][-1]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=2, help="torch / fused pairs per workload")
    ap.add_argument("--limit", type=int, default=300, help="seconds a run may take")
    args = ap.parse_args()
    result = {"steps": args.steps, "steady_steps": f"2..{args.steps - 1}", "workloads": {}}
    one_run("vidvrd_24x96", "torch", args.steps, args.limit)              # the cold first process: discarded
    for workload in WORKLOADS:
        runs = {tail: [] for tail in TAILS}
        for r in range(args.rounds):
            for tail in (("torch", "fused") if r % 2 == 0 else ("fused", "torch")):
                runs[tail].append(one_run(workload, tail, args.steps, args.limit))
        runs["torch_fused"].append(one_run(workload, "torch_fused", args.steps, args.limit))
        spread = max(max(r["tail_ms"] for r in runs[t]) - min(r["tail_ms"] for r in runs[t]) for t in ("torch", "fused"))
        result["workloads"][workload] = {"runs": runs, "tail_ms_run_to_run_spread": round(spread, 3)}
        print(workload, json.dumps(result["workloads"][workload]), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
