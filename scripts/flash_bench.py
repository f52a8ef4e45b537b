#!/usr/bin/env python3
"""A/B of the two split-precision flash-attention kernels on the benchmark's SOS shape (one launch = 2048 sequences x 4 heads x
288 rows, 256 valid): per-launch time of each, max difference between them, and against the f32 VALU kernel on a sample.

    python scripts/flash_bench.py [--B 2048] [--T 288] [--valid 256] [--heads 4] [--hd 128]

At head_dim 32 there is one flash kernel (32 queries per wave), so --hd 32 times two ROUTES of global attention instead: pair rows
through vrd_attention_pair (the split modes' eval route) and the same values as f32 rows through the vector-unit kernel
(ops.attention(..., algo=1): the route of the exact-f32 mode and of training), alternating in one process, several repeats each,
median and spread reported per shape.

    python scripts/flash_bench.py --hd 32 [--cases 16:2048:96:96,16:2048:288:256,8:2048:96:96] [--repeats 5] [--json out.json]

--hd 32 --train times one forward + backward of autograd.Attention (ops.attention under autograd) on the flash route of training
(vrd_attention_rows + vrd_attention_bwd) against the route it replaces (autograd.FUSED_ATTN_BWD = False: the vector-unit forward
and the five-product backward), in f16x3 and bf16x3, at training-sized shapes; --train-step adds whole training steps of the
16-head config (scripts/train_step.py --heads 16 in child processes, VRDONE_FUSED_ATTN_BWD=0 / 1 alternating).

    python scripts/flash_bench.py --hd 32 --train [--train-step] [--json profiles/flash_hd32_train_bench.json]

--segs times global attention over the bucket table of the benchmark's ragged variant (2048 pairs, lengths U[2, 256] at T_pad 288,
the vidvrd model's tight-padding buckets) as ragged.attention issues it: the per-bucket loop over its side streams against the
buckets as the row groups of ONE call (vrd_attention_pair_segs), the latter with either item order of the persistent kernel
(VRD_FLASH_WALK=0: strided over the groups sorted by cost; 1: contiguous runs cut by cumulative cost).  vidvrd's 4 heads x 128
and vidor_x's 8 heads x 64, alternating in one process, medians and spread over --repeats windows.

    python scripts/flash_bench.py --segs [--repeats 7] [--json profiles/attn_segs_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vrdone_amd import ops  # noqa: E402


def to_pair(t):
    """pair rows of the current precision mode: bf16 planes of x, or f16 planes of x * 2^F16_ACT_EXP"""
    from vrdone_amd import _hip
    f16 = ops.get_precision() == "f16x3"
    el = torch.float16 if f16 else torch.bfloat16
    y = t * 2.0 ** _hip.F16_ACT_EXP if f16 else t
    hi = y.to(el)
    lo = (y - hi.float()).to(el)
    C = t.shape[-1]
    raw = torch.stack([hi.reshape(*t.shape[:-1], C // 32, 32), lo.reshape(*t.shape[:-1], C // 32, 32)], dim=-2)
    return ops.Pair(raw.reshape(*t.shape[:-1], 2 * C).contiguous().view(torch.float32), C)


def time_ms(fn, iters):
    """per-call time of `iters` back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def routes_hd32(a, dev):
    """head_dim 32: the pair-row flash route against the f32-row vector-unit route, per case heads:B:T:valid"""
    results = []
    for case in (a.cases or EVAL_CASES).split(","):
        heads, B, T, valid = (int(x) for x in case.split(":"))
        g = torch.Generator(device=dev).manual_seed(1)
        C = heads * 32
        qf, kf, vf = (torch.randn(B, T, C, device=dev, generator=g) for _ in range(3))
        qp, kp, vp = (to_pair(t) for t in (qf, kf, vf))
        mask = (torch.arange(T, device=dev)[None] < valid).expand(B, T).contiguous()
        routes = {"flash_pair": lambda: ops.attention(qp, kp, vp, mask, heads, pair=a.pair, q_mask=mask),
                  "small_f32": lambda: ops.attention(qf, kf, vf, mask, heads, algo=1)}
        times = {name: [] for name in routes}
        with torch.no_grad():
            outs = {}
            for name, fn in routes.items():
                for _ in range(3):
                    outs[name] = fn()
            torch.cuda.synchronize()
            for _ in range(a.repeats):                      # alternating: a drift of the machine hits both routes alike
                for name, fn in routes.items():
                    times[name].append(time_ms(fn, a.iters))
        new = outs["flash_pair"].float() if a.pair else outs["flash_pair"]
        diff = (new[mask] - outs["small_f32"][mask]).abs().max().item()
        rec = {"heads": heads, "head_dim": 32, "B": B, "T": T, "valid": valid, "precision": ops.get_precision(), "iters": a.iters,
               "max_abs_diff": diff}
        for name, ts in times.items():
            rec[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
        f, s = rec["flash_pair"], rec["small_f32"]
        # the new route wins when its slowest repeat beats the other's fastest: a difference beyond the spread of both
        rec["flash_wins_beyond_spread"] = f["max_ms"] < s["min_ms"]
        rec["speedup_median"] = s["median_ms"] / f["median_ms"]
        print(f"{heads:2d} x 32, B {B}, T {T} ({valid} valid), {rec['precision']}: flash on pair rows {f['median_ms']:.3f} ms "
              f"[{f['min_ms']:.3f}, {f['max_ms']:.3f}]   vector-unit kernel on f32 rows {s['median_ms']:.3f} ms [{s['min_ms']:.3f}, "
              f"{s['max_ms']:.3f}]   x{rec['speedup_median']:.2f}   max |diff| {diff:.2e}", flush=True)
        results.append(rec)
        del qf, kf, vf, qp, kp, vp, outs, new
    return results


EVAL_CASES = "16:2048:96:96,16:2048:288:256,8:2048:96:96"
TRAIN_CASES = "16:256:96:96,8:256:96:96,16:48:512:512,16:256:32:32"       # heads:B:T:valid


def train_hd32(a, dev):
    """head_dim 32, forward + backward: the flash route of training against the route it replaces, per case and split mode"""
    from vrdone_amd import autograd
    results = []
    for prec in ("f16x3", "bf16x3"):
        ops.set_precision(prec)
        for case in (a.cases or TRAIN_CASES).split(","):
            heads, B, T, valid = (int(x) for x in case.split(":"))
            g = torch.Generator(device=dev).manual_seed(1)
            C = heads * 32
            q, k, v = (torch.randn(B, T, C, device=dev, generator=g).requires_grad_(True) for _ in range(3))
            dO = torch.randn(B, T, C, device=dev, generator=g)
            mask = (torch.arange(T, device=dev)[None] < valid).expand(B, T).contiguous()

            def fwd_bwd(fused):
                autograd.FUSED_ATTN_BWD = fused
                with torch.enable_grad():
                    out = ops.attention(q, k, v, mask, heads)
                    grads = torch.autograd.grad(out, (q, k, v), dO)
                return (out.detach(), *grads)
            routes = {"flash": lambda: fwd_bwd(True), "parent": lambda: fwd_bwd(False)}
            times, outs = {name: [] for name in routes}, {}
            try:
                for name, fn in routes.items():
                    for _ in range(3):
                        outs[name] = fn()
                torch.cuda.synchronize()
                for _ in range(a.repeats):                      # alternating: a drift of the machine hits both routes alike
                    for name, fn in routes.items():
                        times[name].append(time_ms(fn, a.iters))
            finally:
                autograd.FUSED_ATTN_BWD = True
            diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(outs["flash"], outs["parent"]))
            rec = {"heads": heads, "head_dim": 32, "B": B, "T": T, "valid": valid, "precision": prec, "iters": a.iters,
                   "what": "forward + backward of autograd.Attention", "max_rel_diff": diff}
            for name, ts in times.items():
                rec[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
            f, s = rec["flash"], rec["parent"]
            # beyond the run-to-run spread of the same run: one route's slowest repeat beats the other's fastest
            rec["flash_wins_beyond_spread"] = f["max_ms"] < s["min_ms"]
            rec["flash_loses_beyond_spread"] = s["max_ms"] < f["min_ms"]
            rec["speedup_median"] = s["median_ms"] / f["median_ms"]
            print(f"{heads:2d} x 32, B {B}, T {T} ({valid} valid), {prec}: flash {f['median_ms']:.3f} ms [{f['min_ms']:.3f}, "
                  f"{f['max_ms']:.3f}]   parent route {s['median_ms']:.3f} ms [{s['min_ms']:.3f}, {s['max_ms']:.3f}]   "
                  f"x{rec['speedup_median']:.2f}   max rel diff {diff:.2e}", flush=True)
            results.append(rec)
            del q, k, v, dO, outs
    return results


def train_steps(a):
    """whole training steps of the 16-head config on either route, eager and with the network replayed as HIP graphs:
    scripts/train_step.py in child processes, the two routes alternating"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_step.py")
    doc = {"what": f"scripts/train_step.py --heads 16 --steps {a.steps} [--graphs]: median step_ms after two warm-up steps, one figure per "
                   "child process, VRDONE_FUSED_ATTN_BWD=0 / 1 alternating; the default precision mode"}
    for mode, extra in (("eager", []), ("graphs", ["--graphs"])):
        runs = {"0": [], "1": []}
        for _ in range(2):
            for flag in ("0", "1"):
                env = dict(os.environ, VRDONE_FUSED_ATTN_BWD=flag)
                out = subprocess.run([sys.executable, script, "--heads", "16", "--steps", str(a.steps), *extra], env=env, check=True,
                                     capture_output=True, text=True, timeout=300).stdout
                log = json.loads(out.strip().splitlines()[-1])
                runs[flag].append(statistics.median(log["step_ms"][2:]))       # (the first steps carry warm-up and graph capture)
                print(f"train_step --heads 16 ({mode}), VRDONE_FUSED_ATTN_BWD={flag}: median step {runs[flag][-1]:.2f} ms", flush=True)
        doc[mode] = {"fused_attn_bwd_0_ms": runs["0"], "fused_attn_bwd_1_ms": runs["1"]}
    return doc


def segs_bench(a, dev):
    """the per-bucket loop of ragged.attention against the one call over the buckets as row groups, on the ragged benchmark's table"""
    from vrdone_amd import configs
    from vrdone_amd.models import ragged
    from vrdone_amd.models.maskvrd import MaskVRD
    pairs, frames, t_pad = 2048, 256, 288
    lens = torch.randint(2, frames + 1, (pairs,), generator=torch.Generator().manual_seed(1235))          # bench.py's ragged leg
    lens[0] = frames
    lens = lens.tolist()
    model = MaskVRD(configs.model_config("vidvrd"), device="cpu")
    want = {}
    for i, t2 in enumerate(model.tight_buckets(lens, [t_pad] * pairs, model.ROWS_MIN_ROWS)):          # MaskVRD._tight_plan's buckets
        want.setdefault((lens[i] <= t2 - 2, t2), []).append(i)
    order = sorted(want, key=lambda k: (not k[0], k[1]))
    lay = ragged.Layout([(len(want[key]), key[1], key[0]) for key in order])
    valid = torch.cat([(torch.arange(key[1])[None] < torch.tensor([lens[i] for i in want[key]])[:, None]).reshape(-1) for key in order])[None]
    mask = valid.to(dev).contiguous()
    results = []
    for heads, hd, what in ((4, 128, "vidvrd"), (8, 64, "vidor_x")):
        C = heads * hd
        g = torch.Generator(device=dev).manual_seed(1)
        q, k, v = (to_pair(torch.randn(1, lay.rows, C, device=dev, generator=g)) for _ in range(3))

        def route(on, walk):
            def fn():
                ragged.ATTN_SEGS = on
                if walk is None:
                    os.environ.pop("VRD_FLASH_WALK", None)
                else:
                    os.environ["VRD_FLASH_WALK"] = walk
                return ragged.attention(q, k, v, mask, mask, heads, lay, lay, pair=True)
            return fn
        routes = {"bucket_loop": route(False, None), "segs_strided_sorted": route(True, "0"), "segs_contiguous_by_cost": route(True, "1")}
        times, outs = {name: [] for name in routes}, {}
        try:
            with torch.no_grad():
                for name, fn in routes.items():
                    for _ in range(3):
                        outs[name] = fn()
                torch.cuda.synchronize()
                for _ in range(a.repeats):                      # alternating: a drift of the machine hits every route alike
                    for name, fn in routes.items():
                        times[name].append(time_ms(fn, a.iters))
        finally:
            ragged.ATTN_SEGS = False
            os.environ.pop("VRD_FLASH_WALK", None)
        same = all(torch.equal(outs["bucket_loop"].t.view(torch.int32), o.t.view(torch.int32)) for o in outs.values())
        rec = {"what": f"global attention over the ragged benchmark's bucket table, {what} shape", "heads": heads, "head_dim": hd,
               "pairs": pairs, "lengths": f"U[2, {frames}] (seed 1235)", "T_pad": t_pad, "rows": lay.rows,
               "groups": [[n, T] for _, n, T in lay.segs], "precision": ops.get_precision(), "iters": a.iters, "repeats": a.repeats,
               "side_streams": ragged.ATTN_LANES, "bit_equal": same}
        for name, ts in times.items():
            rec[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
        b = rec["bucket_loop"]
        print(f"{what}: {heads} x {hd}, {len(lay.segs)} groups, {lay.rows} rows, {rec['precision']}, outputs bit-equal: {same}", flush=True)
        for name in routes:
            r = rec[name]
            print(f"  {name:24s} {r['median_ms']:7.3f} ms [{r['min_ms']:.3f}, {r['max_ms']:.3f}]   x{b['median_ms'] / r['median_ms']:.2f}", flush=True)
        results.append(rec)
        del q, k, v, outs
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--T", type=int, default=288)
    ap.add_argument("--valid", type=int, default=256)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pair", action="store_true", help="pair-row output (what the model asks for)")
    ap.add_argument("--cases", help="--hd 32: heads:B:T:valid, comma separated (default " + EVAL_CASES + "; --train: " + TRAIN_CASES + ")")
    ap.add_argument("--train", action="store_true", help="--hd 32: forward + backward, the flash route of training against the route it replaces")
    ap.add_argument("--train-step", action="store_true", help="--hd 32 --train: also whole training steps at 16 heads on either route")
    ap.add_argument("--steps", type=int, default=12, help="--train-step: steps per child process")
    ap.add_argument("--repeats", type=int, default=5, help="--hd 32: timed windows per route, alternating")
    ap.add_argument("--json", help="--hd 32: append the records of this run to this JSON list (--train: write the run's document there)")
    ap.add_argument("--segs", action="store_true", help="the ragged benchmark's bucket table: per-bucket loop against one row-group call")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ops.set_precision(os.environ.get("FB_PREC", "bf16x3"))          # FB_PREC=f16x3: the default mode's element format
    if a.segs:
        recs = segs_bench(a, dev)
        if a.json:
            doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
            doc.setdefault("kernel_level", []).extend(recs)
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(doc, f, indent=1)
        return
    if a.hd == 32 and a.train:
        doc = {"attention": train_hd32(a, dev)}
        if a.train_step:
            doc["train_step"] = train_steps(a)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(doc, f, indent=1)
        return
    if a.hd == 32:
        recs = routes_hd32(a, dev)
        if a.json:
            old = json.load(open(a.json)) if os.path.exists(a.json) else []
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(old + recs, f, indent=1)
        return
    g = torch.Generator(device=dev).manual_seed(1)
    C = a.heads * a.hd
    q, k, v = (to_pair(torch.randn(a.B, a.T, C, device=dev, generator=g)) for _ in range(3))
    mask = (torch.arange(a.T, device=dev)[None] < a.valid).expand(a.B, a.T).contiguous()
    res = {}
    with torch.no_grad():
        for name, flag in (("w32 (2 waves/SIMD)", "0"), ("w64 (1 wave/SIMD)", "1"), ("w32 again", "0"), ("w64 again", "1")):
            os.environ["VRD_FLASH_W64"] = flag
            for _ in range(3):
                out = ops.attention(q, k, v, mask, a.heads, pair=a.pair, q_mask=mask)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                out = ops.attention(q, k, v, mask, a.heads, pair=a.pair, q_mask=mask)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            flops = 4.0 * a.B * a.heads * a.valid * a.valid * a.hd
            print(f"{name:22s} {ms:8.3f} ms / launch   {flops / ms / 1e9:7.1f} TFLOP/s executed", flush=True)
            res[flag] = out
    if a.pair:
        res = {k: v.float() for k, v in res.items()}
    d = (res["0"] - res["1"]).abs().max().item()
    print(f"max |w32 - w64| = {d:.3e}   (outputs are O(1))")
    # an f32 reference on a few sequences
    os.environ.pop("VRD_FLASH_W64")
    n = min(a.B, 8)
    qf, kf, vf = (t.float()[:n] for t in (q, k, v))
    ref = ops.attention(qf.contiguous(), kf.contiguous(), vf.contiguous(), mask[:n].contiguous(), a.heads, algo=1)
    live = mask[:n]
    for flag in ("0", "1"):
        print(f"kernel {flag}: max |x - f32 VALU kernel| on {n} sequences = {(res[flag][:n][live] - ref[live]).abs().max().item():.3e}")


if __name__ == "__main__":
    main()
