#!/usr/bin/env python3
"""Eval speed of a model with absolute position rows (`use_abs_pe: True`, vidvrd.yaml): this tree against its parent commit.

Workloads, on an abs-PE model: the ragged batch of `bench.py --full` (2048 pairs, lengths U[2, 256] with seed 1235, T_pad 288, a
fresh mask tensor every step) through `_mask_vrd`; `forward_test` on the synthetic 226-pair video of scripts/queries_bench.py (16
tracklets of 20-90 frames: below MaskVRD.ROWS_MIN_PAIRS, so bucket by bucket); and `forward_test` on the 2070-pair video of
`bench.py --full` (46 tracklets of 200-256 frames: the row-space form).  The parent commit
computes every pair of such a model at the reference's padded length, bucket by bucket; this tree at the tight lengths, in one
row space.  The two trees cannot share a process (one package name, one library each), so every pass starts a fresh child per
tree, parent and this one in turn; the figure of a tree is the median over the passes, with its spread.

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/vrdone_amd/csrc          # (any checkout of the parent, built)
    python scripts/abs_pe_bench.py --parent /tmp/parent [--passes 9]                      # -> profiles/abs_pe_bench.json

Without --parent only this tree is measured.  `--use-abs-pe 0` measures a model WITHOUT position rows the same way (the
comparison the figures are read against: such models got tight padding and the row space earlier).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    """one tree, one process: ms per step of the ragged batch and ms per forward_test call, as one JSON line"""
    sys.path.insert(0, args.tree)
    import torch
    from vrdone_amd import configs, ops, synth
    from vrdone_amd.models.maskvrd import MaskVRD
    dev = torch.device("cuda", 0)
    cfg = dict(configs.model_config("vidvrd"), use_abs_pe=bool(args.use_abs_pe))
    c_in = configs.input_channels(cfg)
    model = synth.load_synthetic_weights(MaskVRD(cfg, device=dev)).to(dev).eval()
    model._config_eval(configs.inference_config("vidvrd"))
    if args.precision:
        ops.set_precision(args.precision)
    d = model.max_div_factor
    t_pad = (max(args.frames, cfg["max_seq_len"]) + d - 1) // d * d
    lens = torch.randint(2, args.frames + 1, (args.pairs,), generator=torch.Generator().manual_seed(1235))
    lens[0] = args.frames
    x, m = synth.synth_pairs(args.pairs, c_in, t_pad, lens.tolist(), seed=1234, device=dev)
    out = {"tree": os.path.abspath(args.tree), "precision": ops.get_precision(), "T_pad": t_pad}
    with torch.no_grad():
        for _ in range(args.warmup):
            model._mask_vrd(x, m.clone(), with_aux=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = model._mask_vrd(x, m.clone(), with_aux=False)
        torch.cuda.synchronize()
        out["ragged_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / args.steps
        assert bool(torch.isfinite(res["pred_logits"]).all()) and not ops.f16_range_exceeded(dev)
        plan = model._tight_plan(m, m.reshape(args.pairs, t_pad)) if model.tight_padding else None
        out["ragged_buckets"] = 1 if plan is None else len(plan["buckets"])
        out["ragged_row_space"] = bool(plan and plan["rows"])
        del x, m, res
        torch.cuda.empty_cache()
        for key, spec in (("forward_test", (16, c_in, 20, 90, 3)), ("forward_test_large", (46, c_in, 200, args.frames, 7))):
            video = synth.synth_video(*spec[:4], seed=spec[4], device=dev)
            times = []
            for _ in range(2 + args.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = model(video)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            out[key + "_pairs"], out[key + "_triplets"] = len(video["sids"]), len(res["triplets"])
            out[key + "_ms"] = statistics.median(times[2:])
            del video
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "passes": [round(v, 3) for v in values]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9, help="timed forward_test calls per pass (median)")
    ap.add_argument("--precision", default="")
    ap.add_argument("--use-abs-pe", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "abs_pe_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", REPO)]
    runs = {name: [] for name, _ in trees}
    for p in range(args.passes):
        for name, tree in trees:           # parent and this tree in turn: drift of the machine hits both alike
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--pairs", str(args.pairs), "--frames", str(args.frames),
                   "--warmup", str(args.warmup), "--steps", str(args.steps), "--calls", str(args.calls), "--precision", args.precision,
                   "--use-abs-pe", str(args.use_abs_pe)]
            env = dict(os.environ, PYTHONPATH=tree)
            res = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=args.timeout)
            if res.returncode != 0:         # (a child that failed ends the measurement: nothing more is started on the device)
                raise SystemExit(f"pass {p} ({name}) failed with {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
            line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
            runs[name].append(line)
            print(f"pass {p} {name}: ragged {line['ragged_ms_per_step']:.2f} ms/step ({line['ragged_buckets']} buckets), forward_test "
                  f"{line['forward_test_pairs']} pairs {line['forward_test_ms']:.2f} ms, {line['forward_test_large_pairs']} pairs "
                  f"{line['forward_test_large_ms']:.2f} ms", flush=True)
    result = {"workloads": {"ragged": f"{args.pairs} pairs, lengths U[2, {args.frames}] (seed 1235), a fresh mask every step, _mask_vrd",
                            "forward_test": "synth_video(16 tracklets, 20..90 frames, seed 3), one eval call",
                            "forward_test_large": f"synth_video(46 tracklets, 200..{args.frames} frames, seed 7), one eval call"},
              "use_abs_pe": bool(args.use_abs_pe), "passes": args.passes, "steps_per_pass": args.steps, "calls_per_pass": args.calls}
    for name, _ in trees:
        first = runs[name][0]
        result[name] = {"precision": first["precision"], "T_pad": first["T_pad"], "ragged_buckets": first["ragged_buckets"],
                        "ragged_row_space": first["ragged_row_space"], "forward_test_pairs": first["forward_test_pairs"],
                        "forward_test_large_pairs": first["forward_test_large_pairs"],
                        "ragged_ms_per_step": spread([r["ragged_ms_per_step"] for r in runs[name]]),
                        "forward_test_ms": spread([r["forward_test_ms"] for r in runs[name]]),
                        "forward_test_large_ms": spread([r["forward_test_large_ms"] for r in runs[name]])}
    if args.parent:
        for key in ("ragged_ms_per_step", "forward_test_ms", "forward_test_large_ms"):
            result[f"speedup_{key.rsplit('_ms', 1)[0]}"] = result["parent"][key]["median"] / result["this"][key]["median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k.startswith("speedup")} or result["this"]))


if __name__ == "__main__":
    main()
