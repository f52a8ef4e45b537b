"""Cases, seeds and shapes of the query-count goldens (tests/golden/queries_model*.npz, forward_test_vidvrd_q24.json,
train_step_vidvrd_q24*): `predictor.num_queries` above the 9 / 10 of the shipped configs, up to the cap of 64.
scripts/make_golden_queries.py imports this file, so the generator and the tests hold the same numbers; nothing here needs the
reference or a GPU."""
import os

import numpy as np
import torch

import local_window_cases as LW

MAX_QUERIES = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# _mask_vrd: (golden case the other settings come from, queries, padded length, ragged lengths with a 2-frame and a full-length
# pair, seed).  24 = two passes of the mask head (16 + 8), 64 = the cap (four full passes, one wave of queries in the matcher),
# 33 = two passes and one query, with head_dim 32 in the predictor's attention and the CLIP backbone.
MODEL_CASES = {
    "vidvrd_q24": dict(base="vidvrd", Q=24, T=96, lens=[96, 61, 40, 17, 9, 2], seed=7024),
    "vidvrd_q64": dict(base="vidvrd", Q=64, T=96, lens=[96, 61, 40, 17, 9, 2], seed=7064),
    "vidor_x_q33": dict(base="vidor_x", Q=33, T=512, lens=[512, 301, 77, 40, 9, 2], seed=7033),
}
# the final head is stored whole, in f32 and as the float64 run's difference from it; the auxiliary heads keep every 7th frame of
# the mask logits and every 5th class of the logits
MASK_T_STRIDE, CLASS_STRIDE = 7, 5
FORWARD_TEST_Q24 = dict(n_tracklets=6, min_len=20, max_len=130, seed=4321)        # the proposal of forward_test_vidvrd.json
TRAIN_Q24 = dict(B=24, T=96, seed_len=2024, seed_x=3, seed_gt=2032, max_rel=24)   # golden_cases.TRAIN's batch, 1 .. 24 relations a pair
sample = LW.sample
GRAD_STRIDE = LW.GRAD_STRIDE


def model_config(mc, Q):
    """A golden case's model config at Q queries."""
    return dict(mc, predictor=dict(mc["predictor"], num_queries=Q))


def state_keys(keys, mc):
    """A golden case's [(key, shape)] at the query count of mc: only the query embedding's rows change."""
    Q = mc["predictor"]["num_queries"]
    return [(k, (Q, s[1]) if k == "predictor.query_embed.weight" else tuple(s)) for k, s in keys]


def c_in(mc):
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    return 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"]


def train_batch(mc, device="cpu", spec=TRAIN_Q24):
    """golden_cases.train_batch with synth_relations(..., max_rel=spec["max_rel"]): (lengths, x, m, batch in the dataloader's
    training format)."""
    from oracle import vrd_oracle as O
    from oracle.synth import synth_relations
    B, T = spec["B"], spec["T"]
    lens = torch.randint(2, T + 1, (B,), generator=torch.Generator().manual_seed(spec["seed_len"])).tolist()
    x, m = O.synth_pairs(B, c_in(mc), T, lens, seed=spec["seed_x"])
    gp, gm, gs = synth_relations(lens, T, mc["num_classes"], max_rel=spec["max_rel"], seed=spec["seed_gt"])
    to = lambda ts: [t.to(device) for t in ts]      # noqa: E731
    data = {"so_features_list": to([x[i, :, :n].contiguous() for i, n in enumerate(lens)]),
            "preds_list": to(gp), "masks_list": to(gm), "segs_list": to(gs)}
    return lens, x, m, data


def load_npz(stem):
    """{key: array} of tests/golden/<stem>.npz, or of its parts <stem>_a.npz, <stem>_b.npz, ... when it is stored split."""
    # (queries_model: one part per case of MODEL_CASES; train_step_vidvrd_q24: two halves of the parameter list)
    out = {}
    single = os.path.join(GOLDEN, stem + ".npz")
    paths = [single] if os.path.exists(single) else [p for p in (os.path.join(GOLDEN, f"{stem}_{c}.npz") for c in "abcd") if os.path.exists(p)]
    assert paths, stem
    for p in paths:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def heads(out):
    """[(prefix, logits, masks)] of a _mask_vrd result: the final head, then the auxiliary ones"""
    res = [("", out["pred_logits"], out["pred_masks"])]
    res += [(f"aux{i}_", a["pred_logits"], a["pred_masks"]) for i, a in enumerate(out.get("aux_outputs", []))]
    return res
