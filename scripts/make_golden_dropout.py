#!/usr/bin/env python3
"""Training-step golden WITH attention / projection dropout from the REAL reference (build container only, CPU): the `pinned`
case of scripts/make_golden_train.py -- configs/vidvrd.yaml, 24 pairs x 96 frames, recorded matchings, pinned stochastic depth --
with `dropattn = 0.1` and `dropout = 0.1`.

The reference draws its dropout masks from torch's generator; vrdone_amd computes them as a pure function of (step seed, site,
element id) (vrdone_amd/dropout.py).  So each nn.Dropout of the backbone's TransformerBlocks -- `attn.attn_drop`,
`attn.proj_drop`, `mlp.2`, `mlp.4`: the only modules the two keys reach (reference models/backbones.py:89-91,137-139) -- is replaced
by a module that multiplies by that function's mask for a fixed seed, laid out in the reference's order: `att` (B, T', n_head,
2w+1) for the attention site, (B, C, T') for the row sites.  A module counts the samples it has seen (the stem blocks run once per
stream: their second call continues the first one's rows).  Everything else is the reference's own forward_training + autograd.

Stored in tests/golden/train_step_vidvrd_dropout.npz and its second half train_step_vidvrd_dropout_b.npz (data only): losses, matchings, gradient statistics and samples in the format
of train_step_vidvrd.npz / .json (the json as one string entry `meta`), plus the seed, the rates, the site table and the first
SAMPLE_BITS keep decisions of every dropout call as the reference's modules applied them (packed bits, flat in the reference's
layout), which tests/test_dropout_cpu.py regenerates from the seed.
"""
import os
os.environ.setdefault("PYTORCH_JIT", "0")
import json
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, build, load_cfg                                  # noqa: E402  (puts the reference on sys.path)
from make_golden_train import SAMPLE, batch, keep_vector, run                 # noqa: E402
from models import blocks as ref_blocks                                       # noqa: E402  (reference)
from vrdone_amd import dropout as D                                           # noqa: E402

SEED = 0x5EEDD0C0FFEE1234            # the pinned 64-bit step seed
P_ATTN, P_PROJ = 0.1, 0.1
SAMPLE_BITS = 4096


class MirrorDropout(nn.Module):
    """Stands in for one nn.Dropout of the reference: x * keep / (1 - p) with keep from vrdone_amd.dropout."""

    def __init__(self, name, p, log):
        super().__init__()
        self.name, self.p, self.site, self.samples, self.log = name, p, D.site_id(name), 0, log

    def forward(self, x):
        B = x.shape[0]
        if x.dim() == 4:                                # att (B, T', n_head, 2w+1): already in id order
            T, H, W = x.shape[1:]
            keep = D.attn_mask(SEED, self.site, self.samples * T, B * T, H, W, self.p).reshape(B, T, H, W)
        else:                                           # (B, C, T'): ids run over (row = sample * T' + t, c)
            C, T = x.shape[1:]
            keep = D.row_mask(SEED, self.site, self.samples * T, B * T, C, self.p).reshape(B, T, C).transpose(0, 2, 1)
        self.log.append((self.name, self.samples, list(x.shape), np.packbits(np.ascontiguousarray(keep).reshape(-1)[:SAMPLE_BITS])))
        self.samples += B
        return x * torch.from_numpy(np.ascontiguousarray(keep).astype(np.float32) * D.keep_scale(self.p))


def main():
    cfg, mc = load_cfg("vidvrd.yaml")
    mc["dropattn"], mc["dropout"] = P_ATTN, P_PROJ
    model, _, _ = build(mc)
    for p in model.parameters():
        p.requires_grad_(True)
    spec = dict(B=24, T=96, seed_len=2024, seed_x=3, seed_gt=2025)
    lens, data = batch(mc, **spec)
    log, sites = [], {}
    for bname, blk in model.named_modules():
        if isinstance(blk, ref_blocks.TransformerBlock):
            assert bname.startswith("backbone."), bname
            for sub, p in (("attn.attn_drop", P_ATTN), ("attn.proj_drop", P_PROJ), ("mlp.2", P_PROJ), ("mlp.4", P_PROJ)):
                parent, leaf = sub.split(".")
                holder = getattr(blk, parent)
                old = holder[int(leaf)] if leaf.isdigit() else getattr(holder, leaf)
                assert isinstance(old, nn.Dropout) and old.p == p, (bname, sub, old)
                new = MirrorDropout(f"{bname}.{sub}", p, log)
                if leaf.isdigit():
                    holder[int(leaf)] = new
                else:
                    setattr(holder, leaf, new)
                sites[new.name] = new.site
    left = [n for n, m in model.named_modules() if isinstance(m, nn.Dropout) and m.p > 0]
    assert not left, left                             # the two keys reach nothing else
    # the pinned stochastic depth of make_golden_train.py's `pinned` case
    keeps = {}
    for name, mod in model.named_modules():
        if isinstance(mod, ref_blocks.AffineDropPath) and mod.drop_prob > 0:
            keeps[name] = keep_vector(name, 2 * spec["B"], 1.0 - mod.drop_prob)
            state = {"calls": 0}

            def fwd(x, mod=mod, name=name, state=state):
                n = x.shape[0]
                k = keeps[name][state["calls"] * n:(state["calls"] + 1) * n]
                assert k.numel() == n, (name, state["calls"])
                state["calls"] += 1
                return (mod.scale * x).div(1.0 - mod.drop_prob) * k.view(n, *([1] * (x.dim() - 1)))
            mod.forward = fwd
    recorded = []
    real_match = model.bipartite_match

    def match(*a, **kw):
        idx, lm = real_match(*a, **kw)
        recorded.append([[i.tolist(), j.tolist()] for i, j in idx])
        return idx, lm
    model.bipartite_match = match
    loss = run(model, data)
    assert len(recorded) == 4
    arrs, stats = {}, {}
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        g = p.grad.detach()
        stats[name] = [float(g.double().sum()), float(g.double().abs().sum()), float(g.double().norm())]
        arrs[f"dropout/{name}"] = (g if g.numel() <= 2048 else g.flatten()[::SAMPLE]).numpy().copy()
    calls = []
    for i, (name, sample0, shape, bits) in enumerate(log):
        calls.append({"site": name, "sample0": sample0, "shape": shape})
        arrs[f"mask/{i}"] = bits
    meta = {"B": spec["B"], "T": spec["T"], "lengths": lens, "sample_stride": SAMPLE, "seed": SEED, "dropattn": P_ATTN,
            "dropout": P_PROJ, "sites": sites, "mask_calls": calls, "mask_bits": SAMPLE_BITS,
            "keep": {k: v.int().tolist() for k, v in keeps.items()},
            "cases": {"dropout": {"losses": {k: float(v.detach()) for k, v in loss.items()}, "grad_stats": stats, "indices": recorded}}}
    # two files (no committed file beyond 1 MiB): the meta entry, the masks and the first half of the gradients, then the rest
    grads = sorted(k for k in arrs if k.startswith("dropout/"))
    second = set(grads[len(grads) // 2:])
    arrs["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "train_step_vidvrd_dropout.npz"), **{k: v for k, v in arrs.items() if k not in second})
    np.savez_compressed(os.path.join(OUT, "train_step_vidvrd_dropout_b.npz"), **{k: arrs[k] for k in second})
    print("total_loss", float(loss["total_loss"]), "dropout calls", len(log), "sites", len(sites))


if __name__ == "__main__":
    torch.set_grad_enabled(True)
    main()
