#!/usr/bin/env python3
"""Generate the checkout-side fixtures of tests/golden/ from the REAL reference (needs a checkout of it; the tests that
read these fixtures do not):

    python scripts/make_golden_checkout.py /path/to/vrdone        (or VRD_REFERENCE=/path/to/vrdone)

- category_tables.json: the id -> name tables of the checkout's dataloaders/category.py (data that
  vrdone_amd.evaluate imports from the checkout at run time; tests/test_evaluate_cpu.py serves them from a mock checkout)
- reference_optimizer_vidvrd.json: the reference's own utils/train_utils.py run on the drop-in model (dropin/ ahead of
  the checkout, as dropin/run.py arranges it): build_optimizer's two parameter groups by name, and the lag ModelEma shows
  after one update of a model whose every weight moved by +1 (tests/test_host.py)
"""
import json
import os
import sys

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VRD_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "dataloaders")):
    sys.exit("usage: python scripts/make_golden_checkout.py <reference checkout>")
sys.path[:0] = [os.path.join(REPO, "dropin"), REPO, REF]      # `models.*` = the drop-in, `utils.*` / `dataloaders.*` = the checkout
from models.maskvrd import MaskVRD                             # noqa: E402  (the drop-in, through dropin/models)
from utils.train_utils import build_optimizer, ModelEma        # noqa: E402  (reference)
from dataloaders import category                               # noqa: E402  (reference)
from vrdone_amd import configs                                 # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
assert MaskVRD.__module__.startswith("vrdone_amd."), MaskVRD.__module__


def tables():
    out = {}
    for ds in ("vidvrd", "vidor"):
        ent, pred = getattr(category, f"{ds}_category_id_to_name"), getattr(category, f"{ds}_pred_id_to_name")
        out[ds] = {"entity_id_to_name": [[int(k), v] for k, v in ent.items()], "pred_id_to_name": [[int(k), v] for k, v in pred.items()]}
    return out


def optimizer():
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "vidvrd.yaml")))
    assert cfg["model_config"] == configs.model_config("vidvrd")      # the test builds the model from vrdone_amd.configs
    model = MaskVRD(cfg["model_config"], device="cpu")
    opt = build_optimizer(model, cfg["training_config"])
    name = {id(p): n for n, p in model.named_parameters()}
    groups = [{"weight_decay": g["weight_decay"], "params": [name[id(p)] for p in g["params"]]} for g in opt.param_groups]
    ema = ModelEma(model)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    ema.update(model)
    k = "backbone.stem.0.ln1.bias"
    lag = float((ema.module.state_dict()[k] - model.state_dict()[k]).abs().max())
    return {"config": "vidvrd", "param_groups": groups, "ema_probe": k, "ema_lag": lag}


if __name__ == "__main__":
    with open(os.path.join(OUT, "category_tables.json"), "w") as f:
        json.dump(tables(), f)
    with open(os.path.join(OUT, "reference_optimizer_vidvrd.json"), "w") as f:
        json.dump(optimizer(), f)
    print("wrote category_tables.json, reference_optimizer_vidvrd.json")
