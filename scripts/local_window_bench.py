#!/usr/bin/env python3
"""Per-launch time of the banded-attention forward (vrd_local_attn, strip kernels) per window, at the benchmark's row count:
2048 x 288 rows, C = 512, 4 heads, f32 rows in and out, no rel_pe, all frames valid.

    python scripts/local_window_bench.py --windows 3 9 19 --out profiles/local_window_forward.json
    python scripts/local_window_bench.py --width 256 --heads 8 --backward        # another shape; the backward's two launches too

Device events around each launch, the windows taken in turn so that drift hits all of them alike; the median and the
spread over --iters launches per window, and the rate over the bytes the algorithm needs (q, k, v read once, the
output written once: 16 * rows * C bytes; the backward reads q, k, v, dO and writes dq, dk, dv: 28 * rows * C, its
rows x heads x W scratch not counted).  Needs the MI355X."""
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
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--backward", action="store_true", help="also time vrd_local_attn_bwd (both of its launches as one)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from vrdone_amd import _hip, ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    C, rows = a.width, a.pairs * a.frames
    q, k, v = (torch.randn(a.pairs, a.frames, C, device=dev, generator=g) for _ in range(3))
    mask = torch.ones(a.pairs, a.frames, dtype=torch.bool, device=dev)
    out = torch.empty_like(q)
    times = {w: [] for w in a.windows}
    btimes = {w: [] for w in a.windows}
    if a.backward:
        dO = torch.randn(a.pairs, a.frames, C, device=dev, generator=g)
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        scratch = torch.empty(2 * rows * a.heads * max(a.windows), device=dev)
        mask8 = mask.view(torch.uint8)

    def backward(w):
        _hip.check(_hip.lib.vrd_local_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), C, dO.data_ptr(), C, mask8.data_ptr(), None,
                                               a.pairs, a.frames, C, a.heads, w // 2, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), C,
                                               scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "vrd_local_attn_bwd")
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
                if a.backward:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    backward(w)
                    t1.record()
                    t1.synchronize()
                    if it >= a.warmup:
                        btimes[w].append(t0.elapsed_time(t1))
    need = 16.0 * rows * C
    res = {"shape": {"pairs": a.pairs, "frames": a.frames, "C": C, "heads": a.heads}, "iters": a.iters,
           "lib": os.environ.get("VRDONE_HIP_LIB", "default"), "windows": {}}
    for w, ts in times.items():
        med = statistics.median(ts)
        res["windows"][str(w)] = {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                                  "needed_bytes_per_s_TB": round(need / (med * 1e-3) / 1e12, 3)}
        if a.backward:
            bt = btimes[w]
            bmed = statistics.median(bt)
            res["windows"][str(w)]["backward"] = {"median_ms": round(bmed, 4), "min_ms": round(min(bt), 4), "max_ms": round(max(bt), 4),
                                                  "needed_bytes_per_s_TB": round(28.0 * rows * C / (bmed * 1e-3) / 1e12, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
