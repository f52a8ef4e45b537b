#!/usr/bin/env python3
"""Local-window goldens from the REAL reference (build container only): banded attention at windows the shipped configs
do not use (5, 11, 19; the reference's own sliding-chunk code fails at window 3), on the CPU.

    python scripts/make_golden_window.py            # everything
    python scripts/make_golden_window.py --only-ops # tests/golden/local_window.npz alone

Writes, under tests/golden/ (cases and seeded inputs: tests/local_window_cases.py):
  local_window.npz            core/<case>/...   the reference LocalMaskedMHCA's attention core (blocks.py:949-986) on seeded q / k / v
                                                (put in place of its projections' outputs by hooks): output, dq, dk, dv, d rel_pe
                              mhca/<case>/...   the whole LocalMaskedMHCA with name-seeded weights: output, dx, parameter gradients (+ l2 norms)
                              sos/w<W>/...      the vidor_local decoder layer (LocalMaskedMHCA_QKV): output and input gradients
  local_window_model.npz      _mask_vrd of vidvrd.yaml at windows 5 and 19 and of vidor_local.yaml at window 5
  forward_test_vidvrd_w19.json   forward_test records at window 19
  train_step_vidvrd_w5.json, _a.npz, _b.npz    one training step at window 5 (format of train_step_vidvrd.*, stochastic depth off)
Activations keep every 17th channel, large gradients every 499th element.
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
from models import blocks as ref_blocks                      # noqa: E402  (reference)
from models import local_transformer as ref_lt               # noqa: E402
from oracle import vrd_oracle as O                           # noqa: E402
from oracle.synth import synth_proposal                      # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))
import local_window_cases as LW                              # noqa: E402


def sub(t):
    return t.detach()[:, ::LW.CH_STRIDE].contiguous().numpy()


def seeded(module, prefix):
    keys = [(f"{prefix}.{k}", list(v.shape)) for k, v in module.state_dict().items()]
    sd = O.synth_state_dict(keys)
    module.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items()}, strict=True)
    return module.eval()


def core_case(W, H, rel, arrs):
    q, k, v, dO, rel_pe = LW.core_inputs(W, H, rel)
    m = LW.mask(W)
    mod = ref_blocks.LocalMaskedMHCA(LW.C, H, window_size=W, use_rel_pe=rel).eval()
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
    p = f"core/{LW.tag(W, H, rel)}/"
    arrs[p + "out"] = sub(seen["core"])
    for n, t in zip(("dq", "dk", "dv"), leaves):
        arrs[p + n] = sub(t.grad)
    if rel:
        arrs[p + "drel"] = mod.rel_pe.grad.numpy().copy()


def mhca_case(W, H, rel, arrs):
    x, dy = LW.mhca_inputs(W, H, rel)
    mod = seeded(ref_blocks.LocalMaskedMHCA(LW.C, H, window_size=W, use_rel_pe=rel), LW.mhca_prefix(W, H, rel))
    x = x.clone().requires_grad_(True)
    out, _ = mod(x, LW.mask(W))
    out.backward(dy)
    p = f"mhca/{LW.tag(W, H, rel)}/"
    arrs[p + "out"], arrs[p + "dx"] = sub(out), sub(x.grad)
    for n, prm in mod.named_parameters():
        arrs[p + "d/" + n] = LW.sample(prm.grad).numpy().copy()
        arrs[p + "norm/" + n] = np.float64(prm.grad.double().norm())          # l2 norm of the whole gradient


def sos_case(W, arrs):
    x, y, dy, m = LW.sos_inputs(W)
    mod = seeded(ref_lt.MaskedConvTransformerDecoderLayer(LW.C, 8, path_pdrop=0.1, n_qx_stride=1, n_kv_stride=1, with_ffn=False,
                                                          use_local=True, win_size=W), f"op.sos_local_w{W}")
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = mod(x, y, m, m)[0]
    out.backward(dy)
    p = f"sos/w{W}/"
    arrs[p + "out"], arrs[p + "dx"], arrs[p + "dy"] = sub(out), sub(x.grad), sub(y.grad)


def ops_cases():
    arrs = {}
    with torch.enable_grad():
        for W, H, rel in LW.OP_CASES:
            core_case(W, H, rel, arrs)
            mhca_case(W, H, rel, arrs)
        for W in LW.SOS_WINDOWS:
            sos_case(W, arrs)
    np.savez_compressed(os.path.join(OUT, "local_window.npz"), **arrs)
    print("local_window.npz:", len(arrs), "arrays,", os.path.getsize(os.path.join(OUT, "local_window.npz")), "bytes")


def model_cases():
    arrs = {}
    for case, spec in LW.MODEL_CASES.items():
        _, mc = load_cfg(spec["base"] + ".yaml")
        mc = LW.model_config(mc, case)
        model, _, _ = build(mc)
        x, m = O.synth_pairs(len(spec["lens"]), c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
        with torch.no_grad():
            out = model._mask_vrd(x, m)
        arrs[f"{case}/pred_logits"] = out["pred_logits"].numpy()
        arrs[f"{case}/pred_masks"] = out["pred_masks"].numpy()
        print(case, "logits std", float(out["pred_logits"].std()), "masks std", float(out["pred_masks"].std()))
    np.savez_compressed(os.path.join(OUT, "local_window_model.npz"), **arrs)


def forward_test_case():
    cfg, mc = load_cfg("vidvrd.yaml")
    mc = LW.model_config(mc, "vidvrd_w19")
    model, _, _ = build(mc)
    model._config_eval(cfg["inference_config"])
    data = synth_proposal(c_in=c_in(mc), **LW.FORWARD_TEST_W19)
    with torch.no_grad():
        res = model(data)
    res["so_trajs_digest"] = [[len(t[0]), float(np.sum(np.asarray(t, dtype=np.float64)))] for t in res.pop("so_trajs")]
    res["n_pairs"] = len(data["sids"])
    res["pair_lengths"] = [int(f.shape[1]) for f in data["so_features_list"]]
    with open(os.path.join(OUT, "forward_test_vidvrd_w19.json"), "w") as f:
        json.dump(res, f)
    print("forward_test w19: pairs", res["n_pairs"], "triplets", len(res["triplets"]))


def train_case():
    _, mc = load_cfg("vidvrd.yaml")
    mc = LW.model_config(mc, "vidvrd_w5")
    model, _, _ = build(mc)
    for p in model.parameters():
        p.requires_grad_(True)
    lens, data = MT.batch(mc, **LW.TRAIN_W5)
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
        parts[n % 2][f"nodrop/{name}"] = LW.sample(g).numpy().copy()
    meta = {"B": LW.TRAIN_W5["B"], "T": LW.TRAIN_W5["T"], "lengths": lens, "sample_stride": LW.GRAD_STRIDE,
            "cases": {"nodrop": {"losses": {k: float(v.detach()) for k, v in loss.items()}, "grad_stats": stats, "indices": recorded}}}
    for part, arrs in zip("ab", parts):
        np.savez_compressed(os.path.join(OUT, f"train_step_vidvrd_w5_{part}.npz"), **arrs)
    with open(os.path.join(OUT, "train_step_vidvrd_w5.json"), "w") as f:
        json.dump(meta, f)
    print("train w5 total_loss", float(loss["total_loss"]))


if __name__ == "__main__":
    torch.manual_seed(0)
    ops_cases()
    if "--only-ops" not in sys.argv:
        model_cases()
        forward_test_case()
        torch.set_grad_enabled(True)
        train_case()
    for f in sorted(os.listdir(OUT)):
        if "w5" in f or "w19" in f or f.startswith("local_window"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
