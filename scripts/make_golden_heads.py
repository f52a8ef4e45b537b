#!/usr/bin/env python3
"""Width / head-count goldens from the REAL reference (build container only): banded attention at width 256 (8, 4, 2 heads)
and at width 512 with 16 heads (head_dim 32), on the CPU.

    python scripts/make_golden_heads.py            # everything
    python scripts/make_golden_heads.py --only-ops # tests/golden/local_heads.npz alone

Writes, under tests/golden/ (cases and seeded inputs: tests/local_heads_cases.py):
  local_heads.npz             core/<case>/...   the reference LocalMaskedMHCA's attention core on seeded q / k / v: output, dq, dk, dv, d rel_pe
                              mhca/<case>/...   the whole LocalMaskedMHCA with name-seeded weights: output, dx, parameter gradients (+ l2 norms)
                              sos/...           the vidor_local decoder layer (LocalMaskedMHCA_QKV) at width 256, 8 heads
  local_heads_model.npz       _mask_vrd of vidvrd.yaml at width 256, at 16 heads, at width 256 with 2 heads, of vidor_local.yaml at width 256
  forward_test_vidvrd_c256.json   forward_test records of vidvrd.yaml at width 256
  train_step_vidvrd_c256.json, _a.npz, _b.npz    one training step at width 256 (format of train_step_vidvrd_w5.*, stochastic depth
                              off); the JSON also lists the reference model's state_dict keys and shapes
Activations keep every 17th channel, large gradients every 499th element (as scripts/make_golden_window.py).
"""
import os
os.environ.setdefault("PYTORCH_JIT", "0")
import json
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, REPO, build, c_in, load_cfg      # noqa: E402  (puts the reference on sys.path)
import make_golden_train as MT                               # noqa: E402
from make_golden_window import seeded, sub                   # noqa: E402
from models import blocks as ref_blocks                      # noqa: E402  (reference)
from models import local_transformer as ref_lt               # noqa: E402
from oracle import vrd_oracle as O                           # noqa: E402
from oracle.synth import synth_proposal                      # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))
import local_heads_cases as LH                               # noqa: E402


def core_case(C, H, W, rel, arrs):
    q, k, v, dO, rel_pe = LH.core_inputs(C, H, W, rel)
    m = LH.mask(W)
    mod = ref_blocks.LocalMaskedMHCA(C, H, window_size=W, use_rel_pe=rel).eval()
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    if rel:
        with torch.no_grad():
            mod.rel_pe.copy_(rel_pe)
    seen = {}
    hooks = [getattr(mod, n).register_forward_hook(lambda _m, _i, _o, t=t: t) for n, t in zip(("query", "key", "value"), leaves)]
    hooks.append(mod.proj.register_forward_pre_hook(lambda _m, inp: seen.__setitem__("core", inp[0])))
    mod(torch.zeros_like(q), m)
    for h in hooks:
        h.remove()
    seen["core"].backward(dO)
    p = f"core/{LH.tag(C, H, W, rel)}/"
    arrs[p + "out"] = sub(seen["core"])
    for n, t in zip(("dq", "dk", "dv"), leaves):
        arrs[p + n] = sub(t.grad)
    if rel:
        arrs[p + "drel"] = mod.rel_pe.grad.numpy().copy()


def mhca_case(C, H, W, rel, arrs):
    x, dy = LH.mhca_inputs(C, H, W, rel)
    mod = seeded(ref_blocks.LocalMaskedMHCA(C, H, window_size=W, use_rel_pe=rel), LH.mhca_prefix(C, H, W, rel))
    x = x.clone().requires_grad_(True)
    out, _ = mod(x, LH.mask(W))
    out.backward(dy)
    p = f"mhca/{LH.tag(C, H, W, rel)}/"
    arrs[p + "out"], arrs[p + "dx"] = sub(out), sub(x.grad)
    for n, prm in mod.named_parameters():
        arrs[p + "d/" + n] = LH.sample(prm.grad).numpy().copy()
        arrs[p + "norm/" + n] = np.float64(prm.grad.double().norm())          # l2 norm of the whole gradient


def sos_case(arrs):
    x, y, dy, m = LH.sos_inputs()
    s = LH.SOS_CASE
    mod = seeded(ref_lt.MaskedConvTransformerDecoderLayer(s["C"], s["H"], path_pdrop=0.1, n_qx_stride=1, n_kv_stride=1, with_ffn=False,
                                                          use_local=True, win_size=s["W"]), LH.SOS_PREFIX)
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = mod(x, y, m, m)[0]
    out.backward(dy)
    arrs["sos/out"], arrs["sos/dx"], arrs["sos/dy"] = sub(out), sub(x.grad), sub(y.grad)


def ops_cases():
    arrs = {}
    with torch.enable_grad():
        for case in LH.OP_CASES:
            core_case(*case, arrs)
        for case in LH.MHCA_CASES:
            mhca_case(*case, arrs)
        sos_case(arrs)
    np.savez_compressed(os.path.join(OUT, "local_heads.npz"), **arrs)
    print("local_heads.npz:", len(arrs), "arrays,", os.path.getsize(os.path.join(OUT, "local_heads.npz")), "bytes")


def model_cases():
    arrs = {}
    for case, spec in LH.MODEL_CASES.items():
        _, mc = load_cfg(spec["base"] + ".yaml")
        mc = LH.model_config(mc, case)
        model, _, _ = build(mc)
        x, m = O.synth_pairs(len(spec["lens"]), c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
        with torch.no_grad():
            out = model._mask_vrd(x, m)
        arrs[f"{case}/pred_logits"] = out["pred_logits"].numpy()
        arrs[f"{case}/pred_masks"] = out["pred_masks"].numpy()
        print(case, "logits std", float(out["pred_logits"].std()), "masks std", float(out["pred_masks"].std()))
    np.savez_compressed(os.path.join(OUT, "local_heads_model.npz"), **arrs)


def forward_test_case():
    cfg, mc = load_cfg("vidvrd.yaml")
    mc = LH.model_config(mc, "vidvrd_c256")
    model, _, _ = build(mc)
    model._config_eval(cfg["inference_config"])
    data = synth_proposal(c_in=c_in(mc), **LH.FORWARD_TEST_C256)
    with torch.no_grad():
        res = model(data)
    res["so_trajs_digest"] = [[len(t[0]), float(np.sum(np.asarray(t, dtype=np.float64)))] for t in res.pop("so_trajs")]
    res["n_pairs"] = len(data["sids"])
    res["pair_lengths"] = [int(f.shape[1]) for f in data["so_features_list"]]
    with open(os.path.join(OUT, "forward_test_vidvrd_c256.json"), "w") as f:
        json.dump(res, f)
    print("forward_test c256: pairs", res["n_pairs"], "triplets", len(res["triplets"]))


def train_case():
    _, mc = load_cfg("vidvrd.yaml")
    mc = LH.model_config(mc, "vidvrd_c256")
    model, keys, _ = build(mc)
    for p in model.parameters():
        p.requires_grad_(True)
    lens, data = MT.batch(mc, **LH.TRAIN_C256)
    orig = ref_blocks.drop_path
    ref_blocks.drop_path = lambda x, drop_prob=0.0, training=False: x
    recorded = []
    real_match = model.bipartite_match

    def match(*a, **kw):
        idx, lm = real_match(*a, **kw)
        recorded.append([[i.tolist(), j.tolist()] for i, j in idx])
        return idx, lm
    model.bipartite_match = match
    loss = MT.run(model, data)
    del model.bipartite_match
    ref_blocks.drop_path = orig
    parts, stats = ({}, {}), {}
    for n, (name, p) in enumerate(model.named_parameters()):
        g = p.grad.detach()
        stats[name] = [float(g.double().sum()), float(g.double().abs().sum()), float(g.double().norm())]
        parts[n % 2][f"nodrop/{name}"] = LH.sample(g).numpy().copy()
    meta = {"B": LH.TRAIN_C256["B"], "T": LH.TRAIN_C256["T"], "lengths": lens, "sample_stride": LH.LW.GRAD_STRIDE,
            "state_keys": keys,
            "cases": {"nodrop": {"losses": {k: float(v.detach()) for k, v in loss.items()}, "grad_stats": stats, "indices": recorded}}}
    for part, arrs in zip("ab", parts):
        np.savez_compressed(os.path.join(OUT, f"train_step_vidvrd_c256_{part}.npz"), **arrs)
    with open(os.path.join(OUT, "train_step_vidvrd_c256.json"), "w") as f:
        json.dump(meta, f)
    print("train c256 total_loss", float(loss["total_loss"]))


if __name__ == "__main__":
    torch.manual_seed(0)
    ops_cases()
    if "--only-ops" not in sys.argv:
        model_cases()
        forward_test_case()
        torch.set_grad_enabled(True)
        train_case()
    for f in sorted(os.listdir(OUT)):
        if "c256" in f or f.startswith("local_heads"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
