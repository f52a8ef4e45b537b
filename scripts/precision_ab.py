"""f16x3 against f16x1 (one f16 MFMA product per GEMM and global attention), interleaved in ONE process on one GPU: the bench
workload (vidvrd, 2048 pairs x 256 frames, T_pad 288, MaskVRD._mask_vrd without auxiliary outputs) and one small-video
forward_test_videos call.  Per mode: step ms (median of the timed steps), pairs/s, per-family kernel ms of one profiled step
(vrd_prof_read) and, for the dominant GEMM family, its executed FLOPs and their fraction of the 2.5 PF f16 MFMA roof.

    python scripts/precision_ab.py [--steps 6] [--out profiles/r07_f16x1_ab.json]

bench.py itself has no entry for f16x1 (its DTYPE table names the reference-grade modes only); this script is where the mode's
speed is measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_F16_MFMA_TFLOPS = 2500.0
FAMILIES = ["GEMM", "LAYERNORM", "DWCONV_LN", "LOCAL_ATTN", "ATTN_SMALL", "ATTN_FLASH", "POOL", "MASK_HEAD", "TRANSPOSE",
            "POSTPROC", "GEMM_X3", "GEMM_X3_DMA", "GEMM_X3_BIG", "BACKWARD"]
MODES = ("f16x3", "f16x1")


def prof_step(lib, fn):
    lib.vrd_prof_reset()
    lib.vrd_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.vrd_prof_enable(0)
    fam = {}
    for i, name in enumerate(FAMILIES):
        ms, n, fl, by, sk = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        lib.vrd_prof_read(i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
        lib.vrd_prof_read_skipped(i, C.byref(sk))
        if n.value:
            fam[name] = {"ms": round(ms.value, 3), "launches": n.value, "flops_executed": fl.value - sk.value}
    lib.vrd_prof_reset()
    return fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07_f16x1_ab.json"))
    args = ap.parse_args()
    from vrdone_amd import _hip, configs, ops, synth
    from vrdone_amd.models.maskvrd import MaskVRD
    from oracle.synth import synth_proposal
    torch.set_grad_enabled(False)
    dev = "cuda:0"
    cfg = configs.model_config("vidvrd")
    model = synth.load_synthetic_weights(MaskVRD(cfg, device=dev)).to(dev).eval()
    P, T = args.pairs, 288
    x, m = synth.synth_pairs(P, configs.input_channels(cfg), T, [256] * P, seed=1, device=dev)
    x, m = x.to(dev), m.to(dev)
    lib = _hip.lib

    def step():
        return model._mask_vrd(x, m, with_aux=False)

    from vrdone_amd import configs as cf
    model._config_eval(cf.inference_config("vidvrd"))
    video = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in
             synth_proposal(6, configs.input_channels(cfg), 20, 130, seed=4321).items()}
    small = [video] + [{k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in
                        synth_proposal(n, configs.input_channels(cfg), lo, hi, seed=s).items()}
                       for n, lo, hi, s in ((5, 20, 90, 11), (3, 10, 40, 12), (8, 30, 200, 13))]

    times = {md: [] for md in MODES}
    ft = {md: [] for md in MODES}
    for md in MODES:
        with ops.use_precision(md):
            for _ in range(args.warmup):
                step()
                model.forward_test_videos(small)
    torch.cuda.synchronize()
    for i in range(args.steps):                      # interleaved: f16x3, f16x1, f16x1, f16x3, ...
        order = MODES if i % 2 == 0 else MODES[::-1]
        for md in order:
            with ops.use_precision(md):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                times[md].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                model.forward_test_videos(small)
                torch.cuda.synchronize()
                ft[md].append((time.perf_counter() - t0) * 1e3)
    res = {"workload": f"vidvrd _mask_vrd, {P} pairs x 256 frames, T_pad {T}, with_aux=False; forward_test_videos on 4 small videos",
           "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "modes": {}}
    for md in MODES:
        with ops.use_precision(md):
            fam = prof_step(lib, step)
        dom = max((k for k in fam if k.startswith("GEMM")), key=lambda k: fam[k]["ms"])
        d = fam[dom]
        step_ms = statistics.median(times[md])
        res["modes"][md] = {
            "step_ms_median": round(step_ms, 3), "step_ms_all": [round(t, 3) for t in times[md]],
            "pairs_per_s": round(P / step_ms * 1e3, 1),
            "forward_test_videos_ms_median": round(statistics.median(ft[md]), 3),
            "kernel_ms_profiled_step": fam,
            "dominant_gemm": {"family": dom, "ms": d["ms"], "flops_executed": d["flops_executed"],
                              "tflops": round(d["flops_executed"] / d["ms"] / 1e9, 1),
                              "fraction_of_2p5_pf_one_product_roof": round(d["flops_executed"] / d["ms"] / 1e9 / PEAK_F16_MFMA_TFLOPS, 4)}}
    res["speedup_step_f16x1_over_f16x3"] = round(res["modes"]["f16x3"]["step_ms_median"] / res["modes"]["f16x1"]["step_ms_median"], 3)
    res["speedup_forward_test_videos"] = round(res["modes"]["f16x3"]["forward_test_videos_ms_median"] /
                                               res["modes"]["f16x1"]["forward_test_videos_ms_median"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "modes"} |
                     {md: {"step_ms": res["modes"][md]["step_ms_median"], "dominant": res["modes"][md]["dominant_gemm"]} for md in MODES}))


if __name__ == "__main__":
    main()
