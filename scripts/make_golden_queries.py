#!/usr/bin/env python3
"""Query-count goldens from the REAL reference (build container only, on the CPU): `predictor.num_queries` at 24, 33 and 64.

    python scripts/make_golden_queries.py

Writes, under tests/golden/ (cases and seeds: tests/queries_cases.py):
  queries_model_a.npz, _b, _c     _mask_vrd of vidvrd.yaml at 24 and 64 queries and of vidor_x.yaml at 33 (head_dim 32 in the
                                  predictor, CLIP backbone) on a 6-pair ragged batch, one case a file: <case>/pred_logits,
                                  pred_masks of the final head whole, <case>/aux<i>_pred_logits every 5th class and
                                  aux<i>_pred_masks every 7th frame, and <case>/f64m32_pred_logits, f64m32_pred_masks: the
                                  reference's float64 run of the same (as scripts/make_golden_f64.py) MINUS the float32 run, stored
                                  as float32 (the difference is ~1e-5: its own rounding, 1e-12, is nothing beside it)
  forward_test_vidvrd_q24.json    forward_test records of vidvrd.yaml at 24 queries on the proposal of forward_test_vidvrd.json
  train_step_vidvrd_q24.json, _a.npz, _b.npz    one training step at 24 queries with 1 .. 24 relations a pair (format of
                                  train_step_vidvrd_c256.*, stochastic depth off, the matcher's indices recorded)
"""
import os
os.environ.setdefault("PYTORCH_JIT", "0")
import json
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, REPO, build, load_cfg            # noqa: E402  (puts the reference on sys.path)
import make_golden_train as MT                               # noqa: E402
from models import blocks as ref_blocks                      # noqa: E402  (reference)
from oracle import vrd_oracle as O                           # noqa: E402
from oracle.synth import synth_proposal                      # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))
import queries_cases as QC                                   # noqa: E402


def model_cases():
    parts = {}
    for case, spec in QC.MODEL_CASES.items():
        _, mc = load_cfg(spec["base"] + ".yaml")
        mc = QC.model_config(mc, spec["Q"])
        model, _, _ = build(mc)
        x, m = O.synth_pairs(len(spec["lens"]), QC.c_in(mc), spec["T"], spec["lens"], seed=spec["seed"])
        arrs = parts[case] = {}                      # (a file per case: each under the repository's size limit)
        with torch.no_grad():
            out = model._mask_vrd(x, m)
            for pre, lg, mk in QC.heads(out):
                arrs[f"{case}/{pre}pred_logits"] = (lg if not pre else lg[..., ::QC.CLASS_STRIDE]).contiguous().numpy()
                arrs[f"{case}/{pre}pred_masks"] = (mk if not pre else mk[..., ::QC.MASK_T_STRIDE]).contiguous().numpy()
            out64 = model.double()._mask_vrd(x.double(), m)
        assert out64["pred_logits"].dtype == torch.float64
        arrs[f"{case}/f64m32_pred_logits"] = (out64["pred_logits"] - out["pred_logits"].double()).float().numpy()
        arrs[f"{case}/f64m32_pred_masks"] = (out64["pred_masks"] - out["pred_masks"].double()).float().numpy()
        e_l = float((out["pred_logits"].double() - out64["pred_logits"]).abs().max())
        e_m = float((out["pred_masks"].double() - out64["pred_masks"]).abs().max())
        print(f"{case}: logits std {float(out['pred_logits'].std()):.3f}, |ref32 - ref64| logits {e_l:.3e} masks {e_m:.3e}")
    assert list(parts) == list(QC.MODEL_CASES)
    for part, arrs in zip("abc", parts.values()):
        np.savez_compressed(os.path.join(OUT, f"queries_model_{part}.npz"), **arrs)


def forward_test_case():
    cfg, mc = load_cfg("vidvrd.yaml")
    mc = QC.model_config(mc, 24)
    model, _, _ = build(mc)
    model._config_eval(cfg["inference_config"])
    data = synth_proposal(c_in=QC.c_in(mc), **QC.FORWARD_TEST_Q24)
    with torch.no_grad():
        res = model(data)
    res["so_trajs_digest"] = [[len(t[0]), float(np.sum(np.asarray(t, dtype=np.float64)))] for t in res.pop("so_trajs")]
    res["n_pairs"] = len(data["sids"])
    res["pair_lengths"] = [int(f.shape[1]) for f in data["so_features_list"]]
    with open(os.path.join(OUT, "forward_test_vidvrd_q24.json"), "w") as f:
        json.dump(res, f)
    print("forward_test q24: pairs", res["n_pairs"], "triplets", len(res["triplets"]))


def train_case():
    _, mc = load_cfg("vidvrd.yaml")
    mc = QC.model_config(mc, 24)
    model, keys, _ = build(mc)
    for p in model.parameters():
        p.requires_grad_(True)
    lens, _, _, data = QC.train_batch(mc)
    sizes = [len(p) for p in data["preds_list"]]
    assert max(sizes) == 24 and min(sizes) == 1, sizes
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
        parts[n % 2][f"nodrop/{name}"] = QC.sample(g).numpy().copy()
    meta = {"B": QC.TRAIN_Q24["B"], "T": QC.TRAIN_Q24["T"], "lengths": lens, "sizes": sizes, "num_queries": 24,
            "sample_stride": QC.GRAD_STRIDE, "state_keys": keys,
            "cases": {"nodrop": {"losses": {k: float(v.detach()) for k, v in loss.items()}, "grad_stats": stats, "indices": recorded}}}
    for part, arrs in zip("ab", parts):
        np.savez_compressed(os.path.join(OUT, f"train_step_vidvrd_q24_{part}.npz"), **arrs)
    with open(os.path.join(OUT, "train_step_vidvrd_q24.json"), "w") as f:
        json.dump(meta, f)
    print("train q24 total_loss", float(loss["total_loss"]), "relations per pair", sizes)


if __name__ == "__main__":
    torch.manual_seed(0)
    model_cases()
    forward_test_case()
    torch.set_grad_enabled(True)
    train_case()
    for f in sorted(os.listdir(OUT)):
        if "q24" in f or f.startswith("queries_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
