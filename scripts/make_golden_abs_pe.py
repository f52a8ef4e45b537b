#!/usr/bin/env python3
"""tests/golden/forward_test_vidvrd_abs_pe.json from the REAL reference (build container only, like scripts/make_golden.py, whose
helpers this reuses; nothing already committed is regenerated): `forward_test` under vidvrd.yaml with `use_abs_pe: True` on the
many-slices video of scripts/make_golden_r2.py -- 494 pairs = three slices of the reference's max_so_pair loop
(models/maskvrd.py:208-227) whose long pairs are padded to 192 / 240 / 240 frames, all above max_seq_len: every slice adds the
position table re-interpolated to ITS padded length (models/backbones.py:187-196), the short pairs the table as it is.

    python scripts/make_golden_abs_pe.py
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, build, c_in, load_cfg          # noqa: E402  (puts the reference on sys.path)
from make_golden_r2 import SLICES, digest                   # noqa: E402
from oracle.synth import synth_proposal                     # noqa: E402

torch.set_grad_enabled(False)


def main():
    cfg, mc = load_cfg("vidvrd.yaml")
    mc = dict(mc, use_abs_pe=True)
    model, _, _ = build(mc)
    model._config_eval(cfg["inference_config"])
    t0 = time.time()
    data = synth_proposal(c_in=c_in(mc), **SLICES)
    lens = [int(f.shape[1]) for f in data["so_features_list"]]
    P, S, d = len(lens), mc["max_so_pair"], model.max_div_factor
    t_long = [(max(lens[s:s + S] + [mc["max_seq_len"]]) + d - 1) // d * d for s in range(0, P, S)]
    print("abs-PE slices case: pairs", P, "slice T_long", t_long, "long pairs", sum(n > mc["max_seq_len"] for n in lens))
    assert P > 2 * S and len(set(t_long)) >= 2 and max(t_long) > mc["max_seq_len"], "need slices with different padded lengths above max_seq_len"
    res = digest(model(data), data)
    del res["so_offset"]                # (all zero in this video; the inputs are regenerated from the seed)
    res["slice_t_long"] = t_long
    with open(os.path.join(OUT, "forward_test_vidvrd_abs_pe.json"), "w") as f:
        json.dump(res, f)
    print("  triplets", len(res["triplets"]), f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
