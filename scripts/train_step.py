#!/usr/bin/env python3
"""A training loop body on the HIP path: own code mirroring the reference's train.py:176-191 (forward -> zero_grad ->
backward -> clip_grad_norm_ -> AdamW step -> EMA update) with its optimizer recipe (utils/train_utils.py:35-95: AdamW,
no weight decay on biases, LayerNorm / scale parameters and embeddings; configs/vidvrd.yaml training_config), on the
24-pair synthetic batch of BASELINE config 3 (6 videos x 4 pairs, T = max_seq_len = 96).

    python scripts/train_step.py --steps 5          # on the GPU box

--entry-lists / --device-source feed the steps from synthetic per-video cache entries (what proposals.load_train_video
returns) instead of one fixed batch: per step either proposals.train_getitem on the host and the lists moved to the device, or
proposals.train_tables and a device-resident proposals.TrainSource (the batch is then gathered by one kernel launch inside the
step).  `data_ms` is the wall time of that feeding stage, from the cache entries to what model(...) is handed, between two
synchronisations; the batch assembly on the device (the per-pair copies of the list form, the gather launch of the source form)
is part of `step_ms` as it always was.  The source's one-time upload is `source_upload_ms`.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def param_groups(model, weight_decay):
    """decay: conv / linear weights; no decay: biases, LayerNorm affine, drop-path scales, embeddings (the split of the
    reference's build_optimizer)."""
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        leaf = name.rsplit(".", 1)[-1]
        is_ln = p.dim() == 3 and p.shape[0] == 1 and p.shape[2] == 1
        (no_decay if (leaf in ("bias", "scale") or is_ln or "query_embed" in name) else decay).append(p)
    return [{"params": decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0.0}]


def synthetic_batch(cfg, c_in, device, n_pairs=24, seed=0):
    from vrdone_amd import synth
    T = cfg["max_seq_len"]
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(8, T + 1, (n_pairs,), generator=g).tolist()
    x, _ = synth.synth_pairs(n_pairs, c_in, T, lens, seed=seed + 1)
    preds, masks, segs = [], [], []
    for L in lens:
        n = int(torch.randint(1, 4, (1,), generator=g))
        a = torch.randint(0, max(L - 2, 1), (n,), generator=g)
        b = torch.minimum(a + 1 + torch.randint(1, L, (n,), generator=g), torch.tensor(L))
        m = torch.zeros(n, T)
        for r in range(n):
            m[r, a[r]:b[r]] = 1
        preds.append(torch.randint(1, cfg["num_classes"] + 1, (n,), generator=g))
        masks.append(m)
        segs.append(torch.stack([a, b], dim=1))
    to = lambda ts: [t.to(device) for t in ts]      # noqa: E731
    return {"so_features_list": to([x[i, :, :n].contiguous() for i, n in enumerate(lens)]),
            "preds_list": to(preds), "masks_list": to(masks), "segs_list": to(segs)}


def synthetic_entries(cfg, n_pairs, seed=0, keys_per_video=4):
    """n_pairs / keys_per_video training cache entries (the dict of proposals.load_train_video): three trajectories per video,
    keys_per_video relation keys among them, 1-3 relations per key of which the first covers at least 60 % of the pair -- so
    every key survives the max_seq_len crop of the pairs that are up to a quarter longer than it, and a step always has
    n_pairs sequences."""
    from collections import defaultdict
    assert n_pairs % keys_per_video == 0 and keys_per_video <= 6
    T, V = cfg["max_seq_len"], cfg["visual_dim"]
    Cc = cfg["clip_dim"] if cfg.get("with_clip_feature", False) else 0
    g = torch.Generator().manual_seed(seed + 77)
    rnd = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))          # noqa: E731
    entries = []
    for v in range(n_pairs // keys_per_video):
        n_frames = rnd(T // 2, T + T // 4)
        w, h = [(320, 240), (640, 360), (1280, 720)][v % 3]
        spans = {t: [[rnd(0, 6), n_frames - rnd(0, 6)]] for t in range(3)}
        e = {"video_hw": (h, w), "relation_merged": defaultdict(list), "relation_keys": [], "visual_features": {}, "entity_bboxes": {},
             "entity_classes": {t: t + 1 for t in range(3)}, "traj_intervals": spans}
        if Cc:
            e["clip_features"] = {}
        for t, ((a, b),) in spans.items():
            e["visual_features"][t] = [torch.randn(b - a, V, generator=g)]
            xy = torch.rand(b - a, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5])
            e["entity_bboxes"][t] = [torch.cat([xy, xy + 8 + torch.rand(b - a, 2, generator=g) * torch.tensor([w * 0.4, h * 0.4])], dim=1)]
            if Cc:
                e["clip_features"][t] = [torch.randn(b - a, Cc, generator=g)]
        for s, o in [(0, 1), (1, 0), (0, 2), (2, 1), (1, 2), (2, 0)][:keys_per_video]:
            lo, hi = max(spans[s][0][0], spans[o][0][0]), min(spans[s][0][1], spans[o][0][1])
            n = hi - lo
            for r in range(rnd(1, 3)):
                length = rnd(-(-6 * n // 10), n) if r == 0 else rnd(2, n)
                begin = lo + rnd(0, n - length)
                e["relation_merged"][(s, o, 0, 0)].append({"predicate": rnd(1, cfg["num_classes"]), "begin_fid": begin, "end_fid": begin + length})
            e["relation_keys"].append([s, o, 0, 0])
        entries.append(e)
    return entries


def run(steps=3, seed=0, device="cuda", lr=1e-4, weight_decay=0.05, clip=1.0, ema_decay=0.999, verbose=True, drop_path=True,
        graphs=False, config="vidvrd", n_pairs=24, profile=False, deterministic=False, fused_tail=False, torch_fused=False,
        feed=None, heads=None, dropattn=0.0, dropout=0.0, rows=False, rows_min_rows=None):
    """rows: MaskVRD.train_rows -- steps that qualify run in the row space (log["train_form"], ["buckets"] = [[pairs, frames, flat]],
    ["rows_computed"] against ["rows_padded"] of the last step); rows_min_rows: MaskVRD.TRAIN_ROWS_MIN_ROWS.
    dropattn / dropout: the config's attention / projection dropout rates (the backbone's TransformerBlocks).
    heads: n_head = fuse_head of the config replaced (16 at width 512: head_dim 32 in the SOS layers' global attention).
    feed: None (one fixed synthetic batch), "lists" or "source" (per step from synthetic cache entries, see the module text).
    fused_tail: clip + AdamW as vrdone_amd.optim.FusedAdamW.step(max_grad_norm=clip) (three launches) instead of torch's
    clip_grad_norm_ + AdamW.step; torch_fused: torch's own AdamW(fused=True), the second baseline of that comparison.
    log["tail_ms"]: wall time of clip + optimiser step, between two synchronisations."""
    from vrdone_amd import _hip, configs, ops, synth
    if deterministic:
        ops.set_deterministic(True)           # bit-reproducible steps (vrdone_amd/ops.py); the log then carries their sha256
    from vrdone_amd.models.maskvrd import MaskVRD
    cfg = configs.model_config(config)
    if heads:
        cfg = dict(cfg, n_head=heads, fuse_head=heads)
    if dropattn or dropout:
        cfg = dict(cfg, dropattn=dropattn, dropout=dropout)
    torch.manual_seed(seed)
    model = synth.load_synthetic_weights(MaskVRD(cfg, device=device)).to(device).train()
    if not drop_path:
        from vrdone_amd.models.blocks import AffineDropPath
        for mod in model.modules():
            if isinstance(mod, AffineDropPath):
                mod.drop_prob = 0.0
    if graphs:
        model.enable_training_graphs()        # forward + backward of the network as two HIP-graph replays (train_graph.py)
    model.train_rows = bool(rows)
    if rows_min_rows is not None:
        model.TRAIN_ROWS_MIN_ROWS = int(rows_min_rows)
    from vrdone_amd.ema import ModelEma
    ema = ModelEma(model, decay=ema_decay)                                # one-launch EMA (vrd_ema_update), same values
    if fused_tail:
        from vrdone_amd.optim import FusedAdamW
        opt = FusedAdamW(param_groups(model, weight_decay), lr=lr)
    else:
        opt = torch.optim.AdamW(param_groups(model, weight_decay), lr=lr, **({"fused": True} if torch_fused else {}))
    log = {"total_loss": [], "step_ms": [], "tail_ms": [], "params_without_grad": [], "nonfinite_grads": []}
    if feed is None:
        data = synthetic_batch(cfg, configs.input_channels(cfg), device, n_pairs=n_pairs, seed=seed)
    else:
        import random
        from vrdone_amd import proposals
        assert feed in ("lists", "source")
        entries = synthetic_entries(cfg, n_pairs, seed=seed)
        log["data_ms"] = []
        if feed == "source":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            source = proposals.TrainSource.concat([proposals.TrainSource.from_entry(e, device) for e in entries])
            torch.cuda.synchronize()
            log["source_upload_ms"] = 1e3 * (time.perf_counter() - t0)

        def feed_step(step):
            rng = random.Random(1000 * seed + step)
            T = cfg["max_seq_len"]
            if feed == "source":
                tables = proposals.TrainTables.concat([proposals.train_tables(v, 1, T, rng=rng) for v in source.videos])
                tables.on_device(source)                                  # the one upload of the step
                return {"train_source": source, "train_tables": tables}
            out = {k: [] for k in ("so_features_list", "preds_list", "masks_list", "segs_list")}
            for e in entries:
                for k, v in proposals.train_getitem(e, 1, T, rng=rng).items():
                    out[k] += [t.to(device, non_blocking=True) for t in v]     # utils.dict_to_device, utils/misc.py:98-112
            return out
    start = [p.detach().clone() for p in model.parameters()]
    zero_grad = set()
    for step in range(steps):
        if feed is not None:
            torch.cuda.synchronize()
            t_data = time.perf_counter()
            data = feed_step(step)
            torch.cuda.synchronize()
            log["data_ms"].append(1e3 * (time.perf_counter() - t_data))
        if profile and step == steps - 1:                                 # per-kernel-family time of the last step (HIP events)
            _hip.prof_enable(True)
            _hip.prof_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss_dict = model(data)                                           # train.py:182
        opt.zero_grad(set_to_none=True)
        loss_dict["total_loss"].backward()                                # train.py:186
        named = list(model.named_parameters())
        log["params_without_grad"] += [name for name, p in named if p.grad is None]
        with_grad = [(name, p.grad) for name, p in named if p.grad is not None]
        norms = torch.stack(torch._foreach_norm([g for _, g in with_grad])).cpu()       # one multi-tensor launch, one sync
        log["nonfinite_grads"] += [with_grad[i][0] for i in torch.nonzero(~torch.isfinite(norms)).flatten().tolist()]
        zero = {with_grad[i][0] for i in torch.nonzero(norms == 0).flatten().tolist()}     # gradient identically zero in every step
        zero_grad = zero if step == 0 else zero_grad & zero
        torch.cuda.synchronize()
        t_tail = time.perf_counter()
        if fused_tail:
            opt.step(max_grad_norm=clip if clip > 0 else None)           # both in three launches (vrdone_amd/optim.py)
        else:
            if clip > 0:
                torch.nn.utils.clip_grad_norm_(model.parameters(), clip)     # train.py:187-188
            opt.step()
        torch.cuda.synchronize()
        log["tail_ms"].append(1e3 * (time.perf_counter() - t_tail))
        ema.update(model)                                                 # train.py:194 (ModelEma.update, utils/train_utils.py:21-29)
        torch.cuda.synchronize()
        log["step_ms"].append(1e3 * (time.perf_counter() - t0))
        log["total_loss"].append(float(loss_dict["total_loss"].detach()))
        if verbose:
            fed = f"  data {log['data_ms'][-1]:.1f} ms" if feed is not None else ""
            print(f"step {step}: total_loss {log['total_loss'][-1]:.4f}  ({log['step_ms'][-1]:.1f} ms){fed}", flush=True)
    if rows:
        lens = [int(f.shape[1]) for f in data["so_features_list"]] if "so_features_list" in data else []
        plan = model.train_rows_plan(lens) if model.train_form == "rows" else []
        log["train_form"] = model.train_form
        log["buckets"] = [[len(ids), t, flat] for t, ids, flat in plan]
        log["rows_padded"] = len(lens) * cfg["max_seq_len"]
        log["rows_computed"] = sum(len(ids) * t for t, ids, _ in plan) if plan else log["rows_padded"]
        if verbose:
            print(f"train_form {model.train_form}: buckets (pairs x frames) " + ", ".join(f"{n} x {t}" + ("" if flat else " (not flat)")
                                                                                          for n, t, flat in log["buckets"]) +
                  f"; rows computed / padded {log['rows_computed']} / {log['rows_padded']}", flush=True)
    if profile:
        prof = _hip.prof_read()
        _hip.prof_enable(False)
        log["kernel_ms_last_step"] = {k: round(v["ms"], 3) for k, v in prof.items() if v["launches"]}
        log["kernel_launches_last_step"] = {k: v["launches"] for k, v in prof.items() if v["launches"]}
    with torch.no_grad():          # (multi-tensor ops: a per-parameter expression here was 3 x 521 x 2 launches in the step profile)
        for key, params in (("param_delta_norm", model.parameters()), ("ema_delta_norm", ema.module.parameters())):
            norms = torch.stack(torch._foreach_norm(torch._foreach_sub([p.detach() for p in params], start)))
            log[key] = float(torch.linalg.vector_norm(norms))
            if key == "param_delta_norm":
                names = [name for name, _ in model.named_parameters()]
                log["params_unmoved"] = [names[i] for i in torch.nonzero(norms == 0).flatten().tolist()]
                log["params_zero_grad"] = [name for name in names if name in zero_grad]
    if deterministic:
        log["sha256"] = state_digest(model, ema)
    return log


def state_digest(model, ema):
    """sha256 over the bytes of every gradient of the last step, every parameter and every EMA tensor, in module order."""
    import hashlib
    h = hashlib.sha256()
    tensors = [p.grad for p in model.parameters() if p.grad is not None] + [p.detach() for p in model.parameters()]
    tensors += list(ema.module.state_dict().values())
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graphs", action="store_true", help="replay the network's forward / backward as HIP graphs")
    ap.add_argument("--config", default="vidvrd", help="vidvrd (24 pairs x 96 frames) | vidor (48 pairs x 512 frames: --pairs 48)")
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--profile", action="store_true", help="per-kernel-family HIP-event time of the last step")
    ap.add_argument("--fused-tail", action="store_true", help="clip + AdamW as three launches (vrdone_amd.optim.FusedAdamW)")
    ap.add_argument("--torch-fused", action="store_true", help="torch.optim.AdamW(fused=True): the other baseline of the tail comparison")
    ap.add_argument("--deterministic", action="store_true", help="bit-reproducible steps; prints the sha256 of gradients, parameters, EMA")
    ap.add_argument("--device-source", action="store_true", help="per step: proposals.train_tables + a device-resident TrainSource (prints data_ms)")
    ap.add_argument("--entry-lists", action="store_true", help="per step: proposals.train_getitem on the same cache entries, lists moved to the device (prints data_ms)")
    ap.add_argument("--heads", type=int, help="n_head and fuse_head of the config (16: head_dim 32 at width 512)")
    ap.add_argument("--dropattn", type=float, default=0.0, help="the config's `dropattn`: dropout on the banded attention's probabilities")
    ap.add_argument("--dropout", type=float, default=0.0, help="the config's `dropout`: projection and MLP dropout of the TransformerBlocks")
    ap.add_argument("--rows", action="store_true", help="MaskVRD.train_rows: ragged batches in one row space; prints train_form and the bucket table")
    ap.add_argument("--rows-min-rows", type=int, help="MaskVRD.TRAIN_ROWS_MIN_ROWS, the bucket-merging threshold of the training plan")
    args = ap.parse_args()
    assert not (args.device_source and args.entry_lists)
    print(json.dumps(run(steps=args.steps, seed=args.seed, graphs=args.graphs, config=args.config, n_pairs=args.pairs, profile=args.profile,
                         deterministic=args.deterministic, fused_tail=args.fused_tail, torch_fused=args.torch_fused,
                         feed="source" if args.device_source else "lists" if args.entry_lists else None, heads=args.heads,
                         dropattn=args.dropattn, dropout=args.dropout, rows=args.rows, rows_min_rows=args.rows_min_rows)))
