"""Deterministic synthetic weights and inputs for smoke / bench runs (there are no datasets or
checkpoints on the box).  Name-seeded so every process regenerates identical tensors:
O(1) drop-path scales (the 1e-4 init would hide every attention / MLP branch), LayerNorm affine
near identity, conv weights N(0,1)/sqrt(fan_in) so activations stay O(1)."""
import hashlib
import math

import torch


def synth_tensor(name, shape, ln_bias_std=0.1):
    shape = tuple(shape)
    if name == "empty_weight":
        return None
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
    g = torch.Generator().manual_seed(seed)
    leaf = name.rsplit(".", 1)[-1]
    is_ln = len(shape) == 3 and shape[0] == 1 and shape[2] == 1
    if leaf == "scale":
        return torch.rand(shape, generator=g) + 0.5
    if is_ln:
        return 1.0 + 0.1 * torch.randn(shape, generator=g) if leaf == "weight" else ln_bias_std * torch.randn(shape, generator=g)
    if leaf == "bias":
        return 0.02 * torch.randn(shape, generator=g)
    fan_in = 1 if "query_embed" in name else max(1, math.prod(shape[1:]))
    return torch.randn(shape, generator=g) / math.sqrt(fan_in)


def load_synthetic_weights(model):
    """Overwrite every parameter of `model` in place (buffers such as empty_weight are kept)."""
    sd = model.state_dict()
    new = {}
    for name, t in sd.items():
        s = synth_tensor(name, t.shape)
        new[name] = t if s is None else s.to(t.dtype)
    model.load_state_dict(new, strict=True)
    return model


def synth_pairs(n_pairs, c_in, t_pad, lengths=None, seed=1234, device="cpu"):
    """x ~ N(0,1) * mask of shape (B, C_in, T_pad); mask (B, 1, T_pad) bool with mask[b, t] = t < len_b."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n_pairs, c_in, t_pad, generator=g, device=device)
    if lengths is None:
        lengths = torch.full((n_pairs,), t_pad, dtype=torch.long)
    lengths = torch.as_tensor(lengths).to(device)
    mask = (torch.arange(t_pad, device=device)[None, :] < lengths[:, None])[:, None, :]
    return x * mask.to(x.dtype), mask


def synth_video(n_tracklets, c_in, min_len, max_len, seed=7, device="cpu"):
    """One synthetic video for MaskVRD.forward_test: n tracklets with random durations inside a (max_len + 8)-frame
    video and every ordered pair whose overlap is >= 2 frames (46 tracklets -> up to 2070 pairs), in the dataloader's
    eval format (dataloaders/vidvrd.py:706-715): per-pair features as an (L, C_in) matrix viewed (C_in, L)."""
    g = torch.Generator().manual_seed(seed)
    video_len = max_len + 8
    span, boxes = [], []
    for _ in range(n_tracklets):
        n = int(torch.randint(min_len, max_len + 1, (1,), generator=g))
        t0 = int(torch.randint(0, video_len - n + 1, (1,), generator=g))
        span.append((t0, t0 + n))
        corner = torch.rand(n, 2, generator=g) * 100.0
        boxes.append(torch.cat([corner, corner + torch.rand(n, 2, generator=g) * 50.0 + 1.0], dim=1).to(device))
    sids, oids, feats = [], [], []
    for s in range(n_tracklets):
        for o in range(n_tracklets):
            overlap = min(span[s][1], span[o][1]) - max(span[s][0], span[o][0])
            if s != o and overlap >= 2:
                sids.append(s)
                oids.append(o)
                feats.append(torch.randn(overlap, c_in, generator=g).to(device).permute(1, 0))
    return {"sids": torch.tensor(sids, device=device), "oids": torch.tensor(oids, device=device),
            "so_features_list": feats, "bboxes_list": boxes,
            "cat_ids": torch.randint(1, 36, (n_tracklets,), generator=g).to(device),
            "cat_scores": torch.rand(n_tracklets, generator=g).to(device),
            "traj_durations": torch.tensor(span, device=device), "so_offset": torch.zeros(len(sids), dtype=torch.long, device=device)}


def synth_raw_video(n_tracklets, n_visual, min_len, max_len, seed=7, n_clip=0, wh=(1280, 720), n_categories=None, n_shadowed=0):
    """One synthetic video in the form the reference's `_prepare_test` hands to `_test_getitem`
    (dataloaders/vidvrd.py:459-550) and vrdone_amd.proposals.prepare_test_proposal takes: per-TRACKLET visual (and CLIP)
    features and boxes on the host, durations [start, end), distinct categories, every ordered pair of tracklets that
    share a frame.
    n_categories: the categories are drawn from 1 .. n_categories instead (several tracklets per category: the vIoU de-dup
    has pairs to compare).  n_shadowed: that many more tracklets behind the n_tracklets, each a same-category near-copy of
    one of those -- a sub-span of its duration, its boxes moved by a pixel or two -- which the de-dup drops.  Both draw from
    a generator of their own: with the defaults the video is what it was without them, bit for bit."""
    g = torch.Generator().manual_seed(seed)
    g_extra = torch.Generator().manual_seed(seed + 7919)
    video_len = max_len + 8
    spans, boxes, vis, clip = [], [], [], []
    for _ in range(n_tracklets):
        n = int(torch.randint(min_len, max_len + 1, (1,), generator=g))
        t0 = int(torch.randint(0, video_len - n + 1, (1,), generator=g))
        spans.append((t0, t0 + n))
        corner = torch.rand(n, 2, generator=g) * torch.tensor([wh[0] * 0.6, wh[1] * 0.6])
        boxes.append(torch.cat([corner, corner + torch.rand(n, 2, generator=g) * torch.tensor([wh[0] * 0.3, wh[1] * 0.3]) + 8.0], dim=1))
        vis.append(torch.randn(n, n_visual, generator=g))
        if n_clip:
            clip.append(torch.randn(n, n_clip, generator=g))
    cat_ids = torch.arange(1, n_tracklets + 1)
    if n_categories is not None:
        cat_ids = torch.randint(1, n_categories + 1, (n_tracklets,), generator=g_extra)
    copied = []
    for _ in range(n_shadowed):
        src = int(torch.randint(0, n_tracklets, (1,), generator=g_extra))
        n = spans[src][1] - spans[src][0]
        cut = torch.randint(0, n // 4 + 1, (2,), generator=g_extra).tolist() if n >= 4 else [0, 0]
        a, e = cut[0], n - cut[1]
        spans.append((spans[src][0] + a, spans[src][0] + e))
        boxes.append(boxes[src][a:e] + (torch.rand(e - a, 4, generator=g_extra) * 3.0 - 1.5))
        vis.append(torch.randn(e - a, n_visual, generator=g_extra))
        if n_clip:
            clip.append(torch.randn(e - a, n_clip, generator=g_extra))
        copied.append(src)
    cat_scores = torch.rand(n_tracklets, generator=g)
    if copied:
        cat_ids = torch.cat([cat_ids, cat_ids[copied]])
        cat_scores = torch.cat([cat_scores, torch.rand(n_shadowed, generator=g_extra)])
    n_all = n_tracklets + n_shadowed
    sids, oids = [], []
    for s in range(n_all):
        for o in range(n_all):
            if s != o and min(spans[s][1], spans[o][1]) > max(spans[s][0], spans[o][0]):
                sids.append(s)
                oids.append(o)
    out = {"sids": torch.tensor(sids), "oids": torch.tensor(oids), "cat_ids": cat_ids,
           "cat_scores": cat_scores, "bboxes_list": boxes,
           "traj_durations": torch.tensor(spans, dtype=torch.int64), "visual_features_list": vis, "video_wh": wh}
    if n_clip:
        out["clip_features_list"] = clip
    return out


def synth_relation_ground_truth(video_names, videos, results, entity_id_to_name, pred_id_to_name, per_video=20, seed=0,
                                absent_predicate=0):
    """A ground-truth relation file ({video: [{triplet, duration, sub_traj, obj_traj}]}, what evaluate.eval_relation loads) made
    from a model's own predictions, so that scoring them finds hits and misses: per video `per_video` relations in five kinds,
    taken from predictions spread over the ranks --
      0  the prediction's own tracks (vIoU 1);  1  both tracks moved by ~1/8 of the box width (vIoU ~0.78);
      2  both tracks moved by ~2/3 of the box width (vIoU ~0.2);  3  kind 1 again for the same prediction, shorter by its last
      quarter (a second ground truth of one triplet);  4  a triplet with the predicate `absent_predicate`, which no prediction has.
    videos: the proposals (`bboxes_list`, `traj_durations`); results: forward_test's (`so_tids`, `pred_durations`, `triplets`);
    a None result gives an empty list.  Shifts are whole quarter pixels, so boxes on a quarter-pixel grid stay on it."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, video, res in zip(video_names, videos, results):
        rels = out[name] = []
        if res is None:
            continue
        n = len(res["triplets"])
        spans = torch.as_tensor(video["traj_durations"]).cpu().tolist()
        picks = torch.randperm(n, generator=g)[:per_video].sort().values.tolist()
        for j, i in enumerate(picks):
            kind = j % 5
            (s, o), (start, end) = res["so_tids"][i], res["pred_durations"][i]
            tracks = [video["bboxes_list"][t].cpu()[start - spans[t][0]:end - spans[t][0]].clone() for t in (s, o)]
            triplet = list(res["triplets"][i])
            if kind == 4:
                triplet[1] = absent_predicate
            if kind in (1, 2, 3):
                for t in tracks:
                    width = float((t[:, 2] - t[:, 0] + 1).mean())
                    dx = round(width * (2 / 3 if kind == 2 else 1 / 8) * 4) / 4
                    t[:, 0] += dx
                    t[:, 2] += dx
            if kind == 3:
                end = max(start + 1, end - (end - start) // 4)
                tracks = [t[:end - start] for t in tracks]
            rels.append({"triplet": [entity_id_to_name[triplet[0]], pred_id_to_name[triplet[1]], entity_id_to_name[triplet[2]]],
                         "duration": [start, end], "sub_traj": tracks[0].tolist(), "obj_traj": tracks[1].tolist()})
            if kind == 3:                  # ... and the same prediction's kind-1 relation over the whole duration next to it
                rels.append(dict(rels[-1], duration=list(res["pred_durations"][i]),
                                 sub_traj=tracks[0].tolist() + [tracks[0][-1].tolist()] * (res["pred_durations"][i][1] - end),
                                 obj_traj=tracks[1].tolist() + [tracks[1][-1].tolist()] * (res["pred_durations"][i][1] - end)))
    return out
