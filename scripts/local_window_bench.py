#!/usr/bin/env python3
"""Per-launch time of the banded-attention forward (vrd_local_attn, strip kernels) per window, at the benchmark's row count:
2048 x 288 rows, C = 512, 4 heads, f32 rows in and out, no rel_pe, all frames valid.

    python scripts/local_window_bench.py --windows 3 9 19 --out profiles/local_window_forward.json

Device events around each launch, the windows taken in turn so that drift hits all of them alike; the median and the
spread over --iters launches per window, and the rate over the bytes the algorithm needs (q, k, v read once, the
output written once: 16 * rows * C bytes).  Needs the MI355X."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[3, 9, 19])
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=288)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from vrdone_amd import ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = (torch.randn(a.pairs, a.frames, 512, device=dev, generator=g) for _ in range(3))
    mask = torch.ones(a.pairs, a.frames, dtype=torch.bool, device=dev)
    out = torch.empty_like(q)
    times = {w: [] for w in a.windows}
    with torch.no_grad(), ops.use_precision("f32"):
        for it in range(a.warmup + a.iters):
            for w in a.windows:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                ops.local_attention(q, k, v, mask, a.heads, w // 2, out=out)
                t1.record()
                t1.synchronize()
                if it >= a.warmup:
                    times[w].append(t0.elapsed_time(t1))
    rows = a.pairs * a.frames
    need = 16.0 * rows * 512
    res = {"shape": {"pairs": a.pairs, "frames": a.frames, "C": 512, "heads": a.heads}, "iters": a.iters,
           "lib": os.environ.get("VRDONE_HIP_LIB", "default"), "windows": {}}
    for w, ts in times.items():
        med = statistics.median(ts)
        res["windows"][str(w)] = {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                                  "needed_bytes_per_s_TB": round(need / (med * 1e-3) / 1e12, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
