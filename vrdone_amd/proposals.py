"""Eval-time pair construction on the device (with the host half of 8f-2).

The reference's test dataloader (dataloaders/vidvrd.py:552-715, dataloaders/vidor.py:640-735) clamps the tracklet
boxes to the frame, drops tracklets shadowed by a same-category tracklet (vIoU > 0.9), and then builds, per ordered
(subject, object) pair, an (L, C_in) matrix on the host by slicing / concatenating the two tracklets' per-frame features
and computing 21 box-feature channels -- every tracklet is copied into 2 (N - 1) pair matrices, which then travel to the
device one by one (utils/misc.py:98-112).

`prepare_test_proposal` keeps the cheap, irregular part on the host (clamp, de-dup, the pair list and its offsets) and
uploads each tracklet's rows ONCE; `MaskVRD.forward_test` then gathers pair rows and computes their box features on the
device (`vrd_gather_pairs`), straight into the backbone's operand buffers.  The returned dict is the reference's eval
proposal with `pair_source` in place of `so_features_list`; everything else (`sids`, `oids`, `cat_ids`, `cat_scores`,
`traj_durations`, `bboxes_list`, `so_offset`) is what `_test_getitem` returns.
"""
import threading

import numpy as np
import torch


class PairSource:
    """Per-tracklet rows on the device + per-pair tables: pair p = `lens[p]` frames, frame t = row s_row[p] + t*stride of
    the subject's tracklet and o_row[p] + t*stride of the object's in the concatenated (sum L, .) arrays."""

    def __init__(self, vis, clip, boxes, s_row, o_row, lens, stride, wh, first_row=None, host_tables=None):
        self.vis, self.clip, self.boxes = vis, clip, boxes
        self.s_row, self.o_row, self.lens_dev = s_row, o_row, lens
        # host_tables: (s_row, o_row, lens) as numpy arrays, from a caller that has them on the host already
        # (prepare_test_videos): spares the copy back, a synchronisation per source
        self.lens = lens.tolist() if host_tables is None else host_tables[2].tolist()
        self.stride, self.wh = int(stride), (float(wh[0]), float(wh[1]))
        self.n_visual = vis.shape[1]
        self.n_clip = 0 if clip is None else clip.shape[1]
        # first_row (n_tracklets + 1,): tracklet k owns rows [first_row[k], first_row[k + 1]) -- what lets the model run its
        # per-entity stage once per tracklet (stream_plan); None: pairs only
        self.first_row = None if first_row is None else np.asarray(first_row, dtype=np.int64)
        self._rows_host = None if host_tables is None else (host_tables[0], host_tables[1])
        # frame sizes of a source that holds several videos (concat): video j owns the tracklet rows [video_row[j],
        # video_row[j + 1]) and its pairs' boxes are normalised by video_wh[j]; pair_wh (P, 2) on the device.  None: one video
        self.video_row = self.video_wh = self.pair_wh = None

    @classmethod
    def concat(cls, sources):
        """One source over the tracklets and pairs of several videos (MaskVRD.forward_test_videos): the tracklet rows one
        after the other, every source's s_row / o_row / first_row moved by the rows in front of it, so that each tracklet,
        stream and pair stays its own; and the per-pair / per-row frame-size tables the gathers normalise the boxes by."""
        sources = list(sources)
        assert sources, "PairSource.concat needs at least one source"
        stride = sources[0].stride
        if any(s.stride != stride for s in sources):
            raise ValueError("PairSource.concat: the sources have different sub-sampling strides")
        if len({s.clip is None for s in sources}) > 1 or len({(s.n_visual, s.n_clip) for s in sources}) > 1:
            raise ValueError("PairSource.concat: the sources have different feature widths")
        n_rows = [s.boxes.shape[0] for s in sources]
        row0 = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int64)
        first_row = None
        if all(s.first_row is not None for s in sources):
            first_row = np.concatenate([s.first_row[:-1] + r for s, r in zip(sources, row0[:-1])] + [row0[-1:]])
        cat = lambda ts: torch.cat(ts, dim=0).contiguous()         # noqa: E731
        out = cls(cat([s.vis for s in sources]), None if sources[0].clip is None else cat([s.clip for s in sources]),
                  cat([s.boxes for s in sources]), cat([s.s_row + int(r) for s, r in zip(sources, row0[:-1])]),
                  cat([s.o_row + int(r) for s, r in zip(sources, row0[:-1])]), cat([s.lens_dev for s in sources]), stride,
                  sources[0].wh, first_row=first_row)
        out.video_row = row0
        out.video_wh = np.asarray([s.wh for s in sources], dtype=np.float32)
        counts = [len(s) for s in sources]
        out.pair_wh = torch.from_numpy(np.repeat(out.video_wh, counts, axis=0)).to(sources[0].boxes.device)
        return out

    def pair_wh_of(self, sel):
        """(len(sel), 2) device frame sizes of the pairs `sel` (device indices), or None for a one-video source."""
        return None if self.pair_wh is None else self.pair_wh[sel].contiguous()

    def rows_wh(self, rows):
        """(n, 2) float32 frame sizes of the videos that own the tracklet rows `rows` (numpy), or None for a one-video source."""
        if self.video_wh is None:
            return None
        return self.video_wh[np.searchsorted(self.video_row, np.asarray(rows, dtype=np.int64), side="right") - 1]

    def __len__(self):
        return len(self.lens)

    FIELDS = ("tracklet_visual", "tracklet_boxes", "tracklet_first_row", "pair_s_row", "pair_o_row", "pair_lens", "video_wh")

    def fields(self):
        """The source as plain proposal entries -- tensors and one int, the only value types the reference's eval loop
        lets through (`utils.dict_to_device`, utils/misc.py:98-112, raises on anything else): what a dataset running in
        DataLoader workers returns (CPU tensors); `from_fields` puts the object back together in `forward_test`."""
        d = {"tracklet_visual": self.vis, "tracklet_boxes": self.boxes, "tracklet_first_row": torch.as_tensor(self.first_row),
             "pair_s_row": self.s_row, "pair_o_row": self.o_row, "pair_lens": self.lens_dev,
             "video_wh": torch.tensor(self.wh, dtype=torch.float32), "pair_stride": self.stride}
        if self.clip is not None:
            d["tracklet_clip"] = self.clip
        return d

    @classmethod
    def from_fields(cls, d, device):
        to = lambda t: t.to(device)            # noqa: E731
        w, h = d["video_wh"].tolist()
        return cls(to(d["tracklet_visual"]), to(d["tracklet_clip"]) if "tracklet_clip" in d else None, to(d["tracklet_boxes"]),
                   to(d["pair_s_row"]), to(d["pair_o_row"]), to(d["pair_lens"]), int(d["pair_stride"]), (w, h),
                   first_row=d["tracklet_first_row"].cpu().numpy())

    def stream_plan(self, ids):
        """The sub-sampled tracklets ("streams") the pairs `ids` read from.  A pair's subject frames are rows
        s_row + t*stride of one tracklet: frames phase, phase + stride, ... of it, from frame number j0 on, with
        phase = (s_row - tracklet start) % stride.  Returns (start row (n,), length (n,)) of the distinct
        (tracklet, phase) streams, and per pair in `ids` the (stream index, j0) of its subject and of its object:
        numpy arrays stream (2, len(ids)), j0 (2, len(ids))."""
        assert self.first_row is not None
        if self._rows_host is None:
            self._rows_host = (self.s_row.cpu().numpy(), self.o_row.cpu().numpy())
        ids = np.asarray(ids, dtype=np.int64)
        rows = np.stack([self._rows_host[0][ids], self._rows_host[1][ids]])              # (2, n)
        trk = np.searchsorted(self.first_row, rows, side="right") - 1
        rel = rows - self.first_row[trk]
        phase, j0 = rel % self.stride, rel // self.stride
        key, stream = np.unique(trk * self.stride + phase, return_inverse=True)
        k_trk, k_phase = key // self.stride, key % self.stride
        start = self.first_row[k_trk] + k_phase
        length = -(-(self.first_row[k_trk + 1] - start) // self.stride)
        return start, length.astype(np.int32), stream.reshape(rows.shape), j0


def _clamped(boxes, w, h):
    b = boxes.clone()
    b[:, 0:2].clamp_(min=0)
    b[:, 2].clamp_(max=w - 1)
    b[:, 3].clamp_(max=h - 1)
    if not bool(((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])).all()):
        raise ValueError("a tracklet box is empty after clamping to the frame")
    return b


def shadowed_tracklets(boxes, spans, cat_ids, threshold=0.9):
    """Indices of tracklets to drop (reference dataloaders/vidvrd.py:577-636): walking tracklets i < j of one category
    whose durations overlap, j goes when i spans j's whole duration and the per-frame box intersections (+1 pixel
    convention) sum to more than `threshold` of j's summed box area; i goes (and its scan stops) in the mirrored case."""
    n = len(boxes)
    gone = np.zeros(n, dtype=bool)
    for i in range(n):
        for j in range(i + 1, n):
            if gone[j] or cat_ids[i] != cat_ids[j]:
                continue
            lo, hi = max(spans[i][0], spans[j][0]), min(spans[i][1], spans[j][1])
            if hi <= lo:
                continue
            bi = boxes[i][lo - spans[i][0]:hi - spans[i][0]]
            bj = boxes[j][lo - spans[j][0]:hi - spans[j][0]]
            wh = (torch.minimum(bi[:, 2:], bj[:, 2:]) - torch.maximum(bi[:, :2], bj[:, :2]) + 1).clamp_(min=0)
            inter = float((wh[:, 0] * wh[:, 1]).sum())
            a_i = float((bi[:, 2] - bi[:, 0] + 1).mul(bi[:, 3] - bi[:, 1] + 1).sum())
            a_j = float((bj[:, 2] - bj[:, 0] + 1).mul(bj[:, 3] - bj[:, 1] + 1).sum())
            if inter / a_j > threshold and spans[i][0] <= spans[j][0] and spans[i][1] >= spans[j][1]:
                gone[j] = True
            elif inter / a_i > threshold and spans[j][0] <= spans[i][0] and spans[j][1] >= spans[i][1]:
                gone[i] = True
                break
    return np.nonzero(gone)[0].tolist()


def load_test_video(info_pkl, features_pkl):
    """The two per-video pickles of the reference's test split -> the dict its `_test_getitem` (and
    `prepare_test_proposal`) takes; restates `_prepare_test`, dataloaders/vidvrd.py:459-550.
      info_pkl      {'traj_proposal': {num_proposals, cat_ids (N,), scores (N,), bboxes_list [N x (L_i, 4)],
                     traj_durations (N, 2) with INCLUSIVE end frames, video_wh}}
      features_pkl  {frame id: {'frame_id', 'tids' [tracklet ids present], 'visual_features' [one (V,) row per tid]}}
    Returns {} for a video with fewer than two tracklets or without a pair of tracklets that share a frame."""
    import pickle
    with open(info_pkl, "rb") as f:
        prop = pickle.load(f)["traj_proposal"]
    if prop["num_proposals"] < 2:
        return {}
    spans = np.asarray(prop["traj_durations"]).astype(np.int64).copy()
    spans[:, 1] += 1                                           # [start, end)
    n = len(spans)
    s_id, o_id = np.meshgrid(np.arange(n), np.arange(n))       # the reference's pair order: object-major
    s_id, o_id = s_id.flatten(), o_id.flatten()
    keep = s_id != o_id
    s_id, o_id = s_id[keep], o_id[keep]
    overlap = np.minimum(spans[s_id, 1], spans[o_id, 1]) > np.maximum(spans[s_id, 0], spans[o_id, 0])
    if not overlap.any():
        return {}
    s_id, o_id = s_id[overlap], o_id[overlap]
    with open(features_pkl, "rb") as f:
        frames = pickle.load(f)
    rows = [[] for _ in range(n)]
    for fid in sorted(frames):
        rec = frames[fid]
        assert rec["frame_id"] == fid
        for i, tid in enumerate(rec["tids"]):
            assert spans[tid][0] <= fid < spans[tid][1]
            rows[tid].append(np.asarray(rec["visual_features"][i]))
    assert all(len(r) == spans[t][1] - spans[t][0] for t, r in enumerate(rows)), "a tracklet misses frames in the feature file"
    return {"sids": torch.as_tensor(s_id, dtype=torch.int64), "oids": torch.as_tensor(o_id, dtype=torch.int64),
            "cat_ids": torch.as_tensor(np.asarray(prop["cat_ids"]), dtype=torch.int64),
            "cat_scores": torch.as_tensor(np.asarray(prop["scores"]), dtype=torch.float32),
            "bboxes_list": [torch.as_tensor(np.asarray(b), dtype=torch.float32) for b in prop["bboxes_list"]],
            "traj_durations": torch.as_tensor(spans, dtype=torch.int64),
            "visual_features_list": [torch.as_tensor(np.stack(r, axis=0), dtype=torch.float32) for r in rows],
            "video_wh": prop["video_wh"]}


def prepare_test_proposal(raw, feat_stride, stride_offset, proposal_min_frames, device, viou_threshold=0.9):
    """raw: the dict `_prepare_test` hands to `_test_getitem` (sids, oids, cat_ids, cat_scores, bboxes_list,
    traj_durations [start, end), visual_features_list, optional clip_features_list, video_wh).  Returns {} when no pair
    survives, else the eval proposal with a device-resident `pair_source` -- or, with device=None, with the source as
    plain CPU tensor entries (PairSource.fields): the form for a dataset's `_test_getitem` under the reference's unmodified
    eval loop (DataLoader workers, `utils.dict_to_device`)."""
    w, h = raw["video_wh"]
    boxes = [_clamped(b, w, h) for b in raw["bboxes_list"]]
    spans = [(int(a), int(e)) for a, e in raw["traj_durations"].tolist()]
    dropped = set(shadowed_tracklets(boxes, spans, raw["cat_ids"].tolist(), viou_threshold))
    first_row = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])            # tracklet -> first row of its frames
    sids, oids, s_row, o_row, lens = [], [], [], [], []
    for s, o in zip(raw["sids"].tolist(), raw["oids"].tolist()):
        if s in dropped or o in dropped:
            continue
        lo, hi = max(spans[s][0], spans[o][0]), min(spans[s][1], spans[o][1])
        shared = hi - lo
        steps = len(range(stride_offset, shared, feat_stride)) if shared > 0 else 0
        if shared < proposal_min_frames or steps < 2:
            continue
        sids.append(s)
        oids.append(o)
        s_row.append(first_row[s] + lo - spans[s][0] + stride_offset)
        o_row.append(first_row[o] + lo - spans[o][0] + stride_offset)
        lens.append(steps)
    if not sids:
        return {}
    clip = raw.get("clip_features_list")
    flat = device is None
    device = "cpu" if flat else device
    src = PairSource(
        torch.cat(raw["visual_features_list"], dim=0).to(device=device, dtype=torch.float32).contiguous(),
        None if clip is None else torch.cat(clip, dim=0).to(device=device, dtype=torch.float32).contiguous(),
        torch.cat(boxes, dim=0).to(device=device, dtype=torch.float32).contiguous(),
        torch.tensor(s_row, dtype=torch.int64, device=device), torch.tensor(o_row, dtype=torch.int64, device=device),
        torch.tensor(lens, dtype=torch.int32, device=device), feat_stride, (w, h), first_row=first_row)
    out = {"sids": torch.tensor(sids), "oids": torch.tensor(oids), "cat_ids": raw["cat_ids"], "cat_scores": raw["cat_scores"],
           "traj_durations": raw["traj_durations"], "bboxes_list": boxes,
           "so_offset": torch.full((len(sids),), stride_offset, dtype=torch.int64)}
    if flat:
        out.update(src.fields())
    else:
        out["pair_source"] = src
    return out


# --------------------------------------------------------------------------------------------------------------------
# The same preparation for many videos in one call, on the device (csrc/vrd_proposals.hip): `pack_test_videos` lays the
# raw dicts out as flat tables, `prepare_test_videos` uploads them with the tracklet rows in ONE copy, runs the clamp, the
# de-dup and the pair tables in four launches and reads the counts, the kept ids and the error flags back in ONE copy.
# --------------------------------------------------------------------------------------------------------------------
class ProposalTables:
    """pack_test_videos' result.  `tables`: the host side of vrd_proposal_args' input tables (include/vrdone_hip.h), numpy --
    trk (n_trk, 5) int64 [first row, first frame, frames, category, video], video_max (n_videos, 2) float32 [w - 1, h - 1],
    trk_first (n_videos + 1,) int32, tri_first / cand_first (n_videos + 1,) int64, cand_s / cand_o (n_cand,) int32 (tracklet
    numbers inside the video), stride_offset (n_videos,) int32.  video_row (n_videos + 1,): video v owns the rows
    [video_row[v], video_row[v + 1]) of the concatenated box / feature arrays.  widths: (visual, CLIP or None).  An empty raw
    ({}) keeps its place as a video without tracklets, so a video's index is its position in the call."""

    def __init__(self, tables, video_row, widths, video_wh):
        self.tables, self.video_row, self.widths, self.video_wh = tables, video_row, widths, video_wh
        self.n_videos = len(video_wh)


def pack_test_videos(raws, stride_offsets=0):
    """The flat tables over all videos of `raws` (each what load_test_video returns, or {}); stride_offsets: an int, or one per
    video.  Host only, touches no feature row.  ValueError on videos of different feature widths, on a candidate id outside its
    video's tracklets, on tracklets whose boxes / features do not have one row per frame, on a negative offset."""
    raws = list(raws)
    nv = len(raws)
    if isinstance(stride_offsets, (int, np.integer)):
        offsets = [int(stride_offsets)] * nv
    else:
        offsets = [int(x) for x in stride_offsets]
        if len(offsets) != nv:
            raise ValueError(f"pack_test_videos: {len(offsets)} stride offsets for {nv} videos")
    if any(x < 0 for x in offsets):
        raise ValueError("pack_test_videos: a stride offset is negative")
    trk, cand_s, cand_o, widths = [], [], [], set()
    video_max, video_wh = np.zeros((nv, 2), dtype=np.float32), [None] * nv
    trk_first, tri_first, cand_first, video_row = (np.zeros(nv + 1, dtype=np.int64) for _ in range(4))
    for v, raw in enumerate(raws):
        n = 0
        if raw:
            spans = np.asarray(raw["traj_durations"], dtype=np.int64).reshape(-1, 2)
            n = len(spans)
            frames = spans[:, 1] - spans[:, 0]
            boxes, vis, clip = raw["bboxes_list"], raw["visual_features_list"], raw.get("clip_features_list")
            cats = np.asarray(raw["cat_ids"], dtype=np.int64).reshape(-1)
            if not (len(boxes) == len(vis) == len(cats) == n and (clip is None or len(clip) == n)) or n == 0:
                raise ValueError(f"pack_test_videos: video {v}: the per-tracklet lists have different lengths (or are empty)")
            for k in range(n):
                rows = (int(frames[k]),)
                if tuple(boxes[k].shape) != rows + (4,) or boxes[k].dtype != torch.float32 or tuple(vis[k].shape[:1]) != rows or \
                        vis[k].dim() != 2 or (clip is not None and (clip[k].dim() != 2 or tuple(clip[k].shape[:1]) != rows)) or rows[0] < 0:
                    raise ValueError(f"pack_test_videos: video {v}: tracklet {k} needs one float32 box row and one feature row per "
                                     f"frame of its duration")
            widths.update((vis[k].shape[1], None if clip is None else clip[k].shape[1]) for k in range(n))
            s, o = (np.asarray(raw[key], dtype=np.int64).reshape(-1) for key in ("sids", "oids"))
            if len(s) != len(o):
                raise ValueError(f"pack_test_videos: video {v}: {len(s)} subject ids, {len(o)} object ids")
            if len(s) and (min(s.min(), o.min()) < 0 or max(s.max(), o.max()) >= n):
                raise ValueError(f"pack_test_videos: video {v}: a candidate pair names a tracklet outside the video's {n}")
            first = video_row[v] + np.concatenate([[0], np.cumsum(frames)])
            trk.append(np.stack([first[:-1], spans[:, 0], frames, cats, np.full(n, v, dtype=np.int64)], axis=1))
            cand_s.append(s)
            cand_o.append(o)
            w, h = raw["video_wh"]
            video_wh[v] = (w, h)
            video_max[v] = (w - 1, h - 1)                      # rounded to f32 as torch.clamp_ rounds its scalar bound
            video_row[v + 1] = first[-1]
        else:
            video_row[v + 1] = video_row[v]
        trk_first[v + 1] = trk_first[v] + n
        tri_first[v + 1] = tri_first[v] + n * (n - 1) // 2
        cand_first[v + 1] = cand_first[v] + (len(cand_s[-1]) if raw else 0)
    if len(widths) > 1:
        raise ValueError(f"pack_test_videos: the videos have different feature widths (visual, CLIP): {sorted(widths, key=str)}")
    if trk_first[-1] >= 2 ** 31:
        raise ValueError("pack_test_videos: more than 2^31 - 1 tracklets in one call")
    cat = lambda parts, dtype, shape: (np.concatenate(parts) if parts else np.zeros(shape, dtype=np.int64)).astype(dtype)     # noqa: E731
    tables = {"trk": cat(trk, np.int64, (0, 5)), "video_max": video_max, "trk_first": trk_first.astype(np.int32),
              "tri_first": tri_first, "cand_first": cand_first, "cand_s": cat(cand_s, np.int32, (0,)),
              "cand_o": cat(cand_o, np.int32, (0,)), "stride_offset": np.asarray(offsets, dtype=np.int32).reshape(nv)}
    return ProposalTables(tables, video_row, widths.pop() if widths else (0, None), video_wh)


def _carve(parts, align=16):
    """Byte offsets of `parts` [(name, numpy dtype, shape)] laid one after the other, each on an `align`-byte line: ({name:
    (first byte, bytes, dtype, shape)}, total bytes)."""
    at, out = 0, {}
    for name, dtype, shape in parts:
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        out[name] = (at, nbytes, np.dtype(dtype), tuple(shape))
        at += -(-nbytes // align) * align
    return out, at


_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
             np.dtype(np.uint8): torch.uint8}


def _carved(buf, layout, name):
    at, nbytes, dtype, shape = layout[name]
    return buf[at:at + nbytes].view(_TORCH_OF[dtype]).view(shape)


# The page-locked host buffer an upload is assembled in: kept between calls and grown on demand.  A fresh pageable buffer of a
# call's size (100 MB for 16 small videos at visual width 1024) costs its page faults at every call and travels through the
# driver's own staging copy; this one goes to the device in one DMA.  A call ends with a synchronisation behind that copy, so
# the next call may overwrite the buffer; the lock keeps two threads from sharing it.
_staging, _staging_lock = [None], threading.Lock()


def _staging_buffer(nbytes):
    if _staging[0] is None or _staging[0].numel() < nbytes:
        _staging[0] = None                                       # (release the old one first)
        _staging[0] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=True)
    return _staging[0][:nbytes]


class ProposalRun:
    """run_proposal_kernels' result: `packed` (ProposalTables), `dev` {name: device tensor} -- the uploaded rows (boxes clamped in
    place, vis, clip), the uploaded tables and every table the kernels wrote (trk_err, shadow, dropped, s_row, o_row, lens,
    kept_s, kept_o, count, video_err) --, `host` {name: numpy} the copy of s_row .. video_err read back, `boxes_cpu` per video
    the list of clamped CPU boxes (None for an empty raw)."""

    def __init__(self, packed, dev, host, boxes_cpu):
        self.packed, self.dev, self.host, self.boxes_cpu = packed, dev, host, boxes_cpu


def run_proposal_kernels(raws, feat_stride, stride_offsets, proposal_min_frames, device, viou_threshold=0.9):
    """The device half of prepare_test_videos (same arguments, same errors): pack, upload once, launch the four kernels, read
    back once.  Returns a ProposalRun, or None when the call holds no tracklet."""
    from . import ops
    if device is None or torch.device(device).type != "cuda":
        raise ValueError("prepare_test_videos runs on the device: for device=None (the flat CPU form) or a CPU device call "
                         "prepare_test_proposal per video")
    if int(feat_stride) < 1:
        raise ValueError(f"prepare_test_videos: feat_stride {feat_stride} < 1")
    raws = list(raws)
    t = pack_test_videos(raws, stride_offsets)
    tab, nv = t.tables, t.n_videos
    n_trk, n_cand, n_tri, R = tab["trk"].shape[0], len(tab["cand_s"]), int(tab["tri_first"][-1]), int(t.video_row[-1])
    if n_trk == 0:
        return None
    V, Cc = t.widths
    # ---- one host buffer, one upload: the rows first (boxes on 16-byte lines for the kernels' float4 accesses), then the tables
    rows = [("boxes", np.float32, (R, 4)), ("vis", np.float32, (R, V))] + ([] if Cc is None else [("clip", np.float32, (R, Cc))])
    layout, nbytes = _carve(rows + [(k, a.dtype, a.shape) for k, a in tab.items()])
    with _staging_lock:
        host = _staging_buffer(nbytes)
        full = [raw for raw in raws if raw]
        for name, key in (("boxes", "bboxes_list"), ("vis", "visual_features_list"), ("clip", "clip_features_list"))[:len(rows)]:
            parts = [x for raw in full for x in raw[key]]
            dst = _carved(host, layout, name)
            if all(x.dtype == torch.float32 for x in parts):
                torch.cat(parts, dim=0, out=dst)
            else:
                dst.copy_(torch.cat(parts, dim=0))
        for k, a in tab.items():
            _carved(host, layout, k).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        host_boxes = _carved(host, layout, "boxes")
        dev = torch.device(device)
        with torch.cuda.device(dev):
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            buf.copy_(host, non_blocking=True)                         # the call's one upload
            out_layout, out_bytes = _carve([("s_row", np.int64, (n_cand,)), ("o_row", np.int64, (n_cand,)), ("lens", np.int32, (n_cand,)),
                                            ("kept_s", np.int32, (n_cand,)), ("kept_o", np.int32, (n_cand,)), ("count", np.int32, (nv,)),
                                            ("video_err", np.int32, (nv,))])
            tmp_layout, tmp_bytes = _carve([("shadow", np.uint8, (n_tri,)), ("dropped", np.uint8, (n_trk,)), ("trk_err", np.uint8, (n_trk,))])
            out, tmp = torch.empty(out_bytes, dtype=torch.uint8, device=dev), torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
            d = {k: _carved(buf, layout, k) for k in layout}
            d.update({k: _carved(out, out_layout, k) for k in out_layout})
            d.update({k: _carved(tmp, tmp_layout, k) for k in tmp_layout})
            args = ops.proposal_args(d, feat_stride, proposal_min_frames, viou_threshold)
            ops.proposal_clamp(args)
            ops.proposal_shadow(args)
            ops.proposal_walk(args)
            ops.proposal_pairs(args)
            # (the host's share while the device works: the clamped CPU boxes of `bboxes_list`, same bounds, same comparisons)
            boxes_cpu = [None] * nv
            for v, raw in enumerate(raws):
                if raw:
                    b = host_boxes[t.video_row[v]:t.video_row[v + 1]].clone()
                    b[:, 0:2].clamp_(min=0)
                    b[:, 2].clamp_(max=float(tab["video_max"][v, 0]))
                    b[:, 3].clamp_(max=float(tab["video_max"][v, 1]))
                    boxes_cpu[v] = list(torch.split(b, tab["trk"][tab["trk_first"][v]:tab["trk_first"][v + 1], 2].tolist()))
            res = out.cpu()                                            # the call's one synchronisation
    h = {k: _carved(res, out_layout, k).numpy() for k in out_layout}
    bad = np.nonzero(h["video_err"])[0]
    if len(bad):
        v = int(bad[0])
        if h["video_err"][v] == 1:
            raise ValueError(f"prepare_test_videos: video {v}: a tracklet box is empty after clamping to the frame")
        raise RuntimeError(f"prepare_test_videos: video {v}: the kernels refused its tables")
    return ProposalRun(t, d, h, boxes_cpu)


def prepare_test_videos(raws, feat_stride, stride_offsets, proposal_min_frames, device, viou_threshold=0.9):
    """prepare_test_proposal for many videos in one call, on the device: raws is a list of the dicts `load_test_video` returns
    (or {}), stride_offsets an int or one int per video.  Returns a list with one entry per video: the dict
    prepare_test_proposal(raw, ..., device) returns -- {} where it returns {}, and for a raw that is {} -- with a `pair_source`
    whose vis / clip / boxes are views of the one uploaded array and whose s_row / o_row / first_row count from the video's own
    first row, so forward_test, forward_test_videos, PairSource.concat and DeviceRelationScorer take them as they are.

    One host-to-device copy (the tracklet rows of all videos and the flat tables of pack_test_videos), four launches (box clamp;
    the shadow bits of every same-video tracklet pair; the reference's greedy de-dup walk; the pair tables, compacted per video)
    and one device-to-host copy (the pair tables, the per-video counts and the error flags), whatever the number of videos,
    tracklets or pairs.  `bboxes_list` holds the boxes clamped on the host, bit-equal to the device's copy.  The upload is
    assembled in a page-locked host buffer that the module keeps between calls (as large as the largest call so far).

    ValueError: videos of different feature widths, a candidate id outside its video's tracklets (before anything is uploaded);
    a box that is empty after clamping (found by the clamp kernel, read with the results; the message names the video).
    `device` must be a HIP device: the flat CPU form of prepare_test_proposal (device=None, for DataLoader workers) stays
    host-only -- build it with prepare_test_proposal."""
    raws = list(raws)
    run = run_proposal_kernels(raws, feat_stride, stride_offsets, proposal_min_frames, device, viou_threshold)
    if run is None:
        return [{} for _ in raws]
    t, d, h, boxes_cpu = run.packed, run.dev, run.host, run.boxes_cpu
    tab, Cc = t.tables, t.widths[1]
    results = []
    for v, raw in enumerate(raws):
        k = int(h["count"][v])
        if not raw or k == 0:
            results.append({})
            continue
        c0, c1 = int(tab["cand_first"][v]), int(tab["cand_first"][v]) + k
        r0, r1 = int(t.video_row[v]), int(t.video_row[v + 1])
        first_row = tab["trk"][tab["trk_first"][v]:tab["trk_first"][v + 1], 0] - r0
        src = PairSource(d["vis"][r0:r1], None if Cc is None else d["clip"][r0:r1], d["boxes"][r0:r1], d["s_row"][c0:c1],
                         d["o_row"][c0:c1], d["lens"][c0:c1], feat_stride, t.video_wh[v],
                         first_row=np.concatenate([first_row, [r1 - r0]]), host_tables=tuple(h[n][c0:c1].copy() for n in ("s_row", "o_row", "lens")))
        results.append({"sids": torch.from_numpy(h["kept_s"][c0:c1].astype(np.int64)), "oids": torch.from_numpy(h["kept_o"][c0:c1].astype(np.int64)),
                        "cat_ids": raw["cat_ids"], "cat_scores": raw["cat_scores"], "traj_durations": raw["traj_durations"],
                        "bboxes_list": boxes_cpu[v], "so_offset": torch.full((k,), int(tab["stride_offset"][v]), dtype=torch.int64),
                        "pair_source": src})
    return results


# --------------------------------------------------------------------------------------------------------------------
# Training side: the per-video ground-truth cache and the per-step sample construction of the reference's
# training dataloader.  Host code (the sample construction draws from Python's `random`, call for call like the reference,
# so that a seeded run sees the same crops); the model side takes the resulting lists as `forward_training` input -- or, further
# down, a device-resident TrainSource and the index tables of `train_tables`, from which it gathers the batch itself.
# --------------------------------------------------------------------------------------------------------------------
def load_train_video(anno_json, gt_features_pkl, entity_cat_name_to_id, pred_cat_name_to_id):
    """One training video's cache entry; restates `_prepare_train`, dataloaders/vidvrd.py:172-322.
      anno_json        VidVRD annotation: {'height', 'width', 'trajectories' [per frame: [{'tid', 'bbox': {xmin, ymin, xmax,
                       ymax}}]], 'subject/objects' [{'tid', 'category'}], 'relation_instances' [{'subject_tid',
                       'object_tid', 'predicate', 'begin_fid', 'end_fid'}]}
      gt_features_pkl  {1-based frame id: {'frame_id', 'tids' array, 'visual_features' (n, V) array}} of the ground-truth boxes
    Trajectories are renumbered 0..n-1 in tid order and cut into intervals of consecutive frames; relation instances of
    one (subject, object, predicate) that overlap in time are merged; every relation is keyed by (subject, object, subject
    interval, object interval).  Returns {} for a video without relations, else {'video_hw', 'relation_merged' {key:
    [{'predicate', 'begin_fid', 'end_fid'}]}, 'relation_keys' [[...]], 'visual_features' / 'entity_bboxes' {index: [per
    interval tensor]}, 'entity_classes', 'traj_intervals' {index: [[start, end)]}}."""
    import copy
    import json
    import pickle
    from collections import defaultdict
    with open(anno_json) as f:
        anno = json.load(f)
    if len(anno["relation_instances"]) == 0:
        return {}
    with open(gt_features_pkl, "rb") as f:
        frames = pickle.load(f)
    present = defaultdict(list)
    for fid, frame in enumerate(anno["trajectories"]):
        for box in frame:
            present[box["tid"]].append(fid)
    tids = sorted(present)
    index_of = {tid: i for i, tid in enumerate(tids)}
    frame_keys = sorted(frames)
    visual, bboxes, intervals = {}, {}, {}
    for tid in tids:
        fids = np.asarray(sorted(present[tid]))
        cut = np.nonzero(np.diff(fids) > 1)[0]
        starts = fids[np.concatenate([[0], cut + 1])]
        ends = fids[np.concatenate([cut, [len(fids) - 1]])] + 1
        spans = [[int(a), int(e)] for a, e in zip(starts, ends)]
        idx = index_of[tid]
        intervals[idx] = spans
        vis_i, box_i = [], []
        for a, e in spans:
            rows = []
            for k in frame_keys:                         # frame ids in the feature file start at 1
                if k - 1 < a:
                    continue
                if k - 1 >= e:
                    break
                rec = frames[k]
                assert rec["frame_id"] == k
                at = np.nonzero(np.asarray(rec["tids"]) == tid)[0]
                assert len(at) == 1
                rows.append(np.asarray(rec["visual_features"])[at])
            vis_i.append(torch.tensor(np.concatenate(rows, axis=0)))
            bb = [[b["bbox"]["xmin"], b["bbox"]["ymin"], b["bbox"]["xmax"], b["bbox"]["ymax"]]
                  for frame in anno["trajectories"][a:e] for b in frame if b["tid"] == tid]
            assert len(bb) == e - a
            box_i.append(torch.tensor(bb, dtype=torch.float32))
        visual[idx], bboxes[idx] = vis_i, box_i
    classes = {index_of[so["tid"]]: entity_cat_name_to_id[so["category"]] for so in anno["subject/objects"]}

    # merge instances of the same (subject, object, predicate) that overlap in time, in order of their first frame
    insts = sorted(copy.deepcopy(anno["relation_instances"]), key=lambda r: r["begin_fid"])
    merged, seen = [], [False] * len(insts)
    for i, base in enumerate(insts):
        if seen[i]:
            continue
        seen[i] = True
        for j in range(i + 1, len(insts)):
            other = insts[j]
            if (other["subject_tid"], other["object_tid"], other["predicate"]) != (base["subject_tid"], base["object_tid"], base["predicate"]):
                continue
            assert other["begin_fid"] > base["begin_fid"]
            if other["begin_fid"] <= base["end_fid"]:
                assert other["end_fid"] > base["end_fid"]
                base["end_fid"] = other["end_fid"]
                seen[j] = True
        merged.append(copy.deepcopy(base))
    merged.sort(key=lambda r: r["begin_fid"])

    # (the keys are collected in a set and listed in ITS iteration order, like the reference: `pair_duration` slices index
    # that list, and for tuples of ints the order is a deterministic function of the insertions)
    relation_merged, keys = defaultdict(list), set()
    for r in merged:
        s, o = index_of[r["subject_tid"]], index_of[r["object_tid"]]
        bf, ef = r["begin_fid"], r["end_fid"]
        s_iv = [k for k, (a, e) in enumerate(intervals[s]) if a <= bf and e >= ef]
        o_iv = [k for k, (a, e) in enumerate(intervals[o]) if a <= bf and e >= ef]
        assert len(s_iv) == 1 and len(o_iv) == 1, "a relation must lie inside one interval of each trajectory"
        key = (s, o, s_iv[0], o_iv[0])
        assert max(intervals[s][s_iv[0]][0], intervals[o][o_iv[0]][0]) < min(intervals[s][s_iv[0]][1], intervals[o][o_iv[0]][1])
        relation_merged[key].append({"predicate": pred_cat_name_to_id[r["predicate"]], "begin_fid": bf, "end_fid": ef})
        keys.add(key)
    return {"video_hw": (anno["height"], anno["width"]), "relation_merged": relation_merged,
            "relation_keys": [list(k) for k in keys], "visual_features": visual, "entity_bboxes": bboxes,
            "entity_classes": classes, "traj_intervals": intervals}


def _truncate_window(L, pred, segment, max_seq_len, trunc_thresh=0.5, max_times=10, rng=None):
    """The decision half of `truncate_feats`: (start, kept predicates, their segments relative to start) of the max_seq_len
    window out of L > max_seq_len steps, or None; the same draws from `rng`."""
    import random
    rng = rng or random
    for _ in range(max_times):
        st = rng.randint(0, L - max_seq_len)
        ed = st + max_seq_len
        left = torch.clamp(segment[:, 0], min=st).float()
        right = torch.clamp(segment[:, 1], max=ed).float()
        inter = (right - left).clamp(min=0)
        keep = inter / (segment[:, 1] - segment[:, 0]).abs() >= trunc_thresh
        if int(keep.sum()) > 0:
            return st, pred[keep], torch.stack((left[keep], right[keep]), dim=1) - st
    return None


def truncate_feats(so_feat, pred, segment, max_seq_len, trunc_thresh=0.5, max_times=10, rng=None):
    """Random max_seq_len crop of a pair that keeps at least one relation >= trunc_thresh inside (reference
    utils/misc.py:219-273, which derives from ActionFormer); None when ten draws find none.  so_feat (C, L), segment
    (N, 2) in feature steps.  Draws `rng.randint(0, L - max_seq_len)` per try, like the reference's `random.randint`."""
    L = so_feat.shape[1]
    if L <= max_seq_len:
        return so_feat, pred, segment
    win = _truncate_window(L, pred, segment, max_seq_len, trunc_thresh, max_times, rng)
    if win is None:
        return None
    st, pred, segment = win
    return so_feat[:, st:st + max_seq_len], pred, segment


def _so_box_features(sb, ob):
    """utils/misc.py:158-178 (what vrd_gather_pairs computes on the device for the eval path)."""
    s_cx, s_cy = (sb[:, 2] + sb[:, 0]) / 2, (sb[:, 3] + sb[:, 1]) / 2
    o_cx, o_cy = (ob[:, 2] + ob[:, 0]) / 2, (ob[:, 3] + ob[:, 1]) / 2
    s_w, s_h, o_w, o_h = sb[:, 2] - sb[:, 0], sb[:, 3] - sb[:, 1], ob[:, 2] - ob[:, 0], ob[:, 3] - ob[:, 1]
    return torch.stack([(s_cx - o_cx) / o_cx, (s_cy - o_cy) / o_cy, torch.log(s_w / o_w), torch.log(s_h / o_h),
                        torch.log(s_w * s_h / (o_w * o_h))], dim=1)


def _entity_box_features(b, w, h):
    """utils/misc.py:181-217: normalised centre / size and their frame-to-frame differences (first frame extrapolated)."""
    x0, x1, y0, y1 = b[:, 0] / w, b[:, 2] / w, b[:, 1] / h, b[:, 3] / h
    geo = torch.stack([(x1 + x0) / 2, (y1 + y0) / 2, x1 - x0, y1 - y0], dim=1)
    d = geo[1:] - geo[:-1]
    first = d[0:1] - (d[1:2] - d[0:1]) if len(d) > 1 else d[0:1]
    d = torch.cat([first, d], dim=0)
    return torch.stack([geo[:, 0], d[:, 0], geo[:, 1], d[:, 1], geo[:, 2], d[:, 2], geo[:, 3], d[:, 3]], dim=1)


def train_getitem(video, feat_stride, max_seq_len, cut_max_preds=False, proposal_max_preds=0, pair_duration=None, rng=None):
    """The training sample of one video (or of its relation keys [pair_duration[0], pair_duration[1])): restates
    `_train_getitem`, dataloaders/vidvrd.py:324-457.  Per relation key: a random sub-sampling offset, the subject / object
    features of the frames both intervals share, the 21 box-feature channels, the relations as [ceil((fid - start -
    offset) / stride)] segments, a random max_seq_len crop, 0/1 masks.  Returns {} when nothing survives, else
    {'so_features_list' [(C_in, L)], 'preds_list', 'masks_list' [(N, max_seq_len)], 'segs_list'}.  A cache entry with
    'clip_features' {index: [per interval (L, Cc)]} (the VidOR loader with CLIP features, dataloaders/vidor.py:346-415) puts
    the subject / object CLIP rows behind the visual ones."""
    import copy
    import random
    rng = rng or random
    if not video:
        return {}
    video = copy.deepcopy(video)
    merged, keys = video["relation_merged"], video["relation_keys"]
    if pair_duration is not None:
        keys = keys[pair_duration[0]:pair_duration[1]]
        merged = {k: v for k, v in merged.items() if list(k) in keys}
    h, w = video["video_hw"]
    boxes = {t: [_clamped(b, w, h) for b in per] for t, per in video["entity_bboxes"].items()}
    feats_out, preds_out, masks_out, segs_out = [], [], [], []
    for key in merged:
        offset = rng.randint(0, feat_stride - 1)
        s, o, si, oi = key
        if cut_max_preds and proposal_max_preds < len(merged[key]):
            continue
        s_iv, o_iv = video["traj_intervals"][s][si], video["traj_intervals"][o][oi]
        lo, hi = max(s_iv[0], o_iv[0]), min(s_iv[1], o_iv[1])
        pick = lambda per, iv: per[lo - iv[0]:hi - iv[0]][offset::feat_stride]      # noqa: E731
        s_feat, o_feat = pick(video["visual_features"][s][si], s_iv), pick(video["visual_features"][o][oi], o_iv)
        if s_feat.shape[0] < 2:
            continue
        sb, ob = pick(boxes[s][si], s_iv), pick(boxes[o][oi], o_iv)
        clip = video.get("clip_features")
        wide = [s_feat, o_feat] if clip is None else [s_feat, o_feat, pick(clip[s][si], s_iv), pick(clip[o][oi], o_iv)]
        so_feat = torch.cat(wide + [_so_box_features(sb, ob), _entity_box_features(sb, w, h), _entity_box_features(ob, w, h)],
                            dim=-1).permute(1, 0)
        preds, segs = [], []
        for r in merged[key]:
            left = np.ceil((r["begin_fid"] - lo - offset) / feat_stride)
            right = np.ceil((r["end_fid"] - lo - offset) / feat_stride)
            if left < right:
                preds.append(r["predicate"])
                segs.append([left, right])
        if not preds:
            continue
        cropped = truncate_feats(so_feat, torch.tensor(preds, dtype=torch.int64), torch.tensor(np.array(segs), dtype=torch.int64),
                                 max_seq_len, rng=rng)
        if cropped is None:
            continue
        so_feat, preds, segs = cropped
        segs_out.append(segs)
        masks = torch.zeros(len(segs), max_seq_len, dtype=torch.float32)
        for m, (a, e) in zip(masks, segs.to(torch.int64).tolist()):
            assert 0 <= a < e <= max_seq_len
            m[a:e] = 1
        feats_out.append(so_feat)
        preds_out.append(preds)
        masks_out.append(masks)
    if not feats_out:
        return {}
    return {"so_features_list": feats_out, "preds_list": preds_out, "masks_list": masks_out, "segs_list": segs_out}


# --------------------------------------------------------------------------------------------------------------------
# Training batches built on the device: `TrainSource` keeps a cache entry's rows on the device, `train_tables` makes
# train_getitem's decisions (same draws, same `continue` rules) on indices alone, and MaskVRD.forward_training gathers
# the operand buffers and the target masks from the two in one launch (vrd_gather_train).
# --------------------------------------------------------------------------------------------------------------------
class TrainVideo:
    """The host side of one video inside a TrainSource: its relation tables, and where each trajectory interval's rows
    start in the source's arrays (`first_row[(trajectory, interval)]`, counted from `row0`)."""

    def __init__(self, index, row0, entry, first_row, n_rows):
        self.index, self.row0, self.first_row, self.n_rows = int(index), int(row0), first_row, int(n_rows)
        self.video_hw = tuple(entry["video_hw"]) if entry else None
        self.relation_merged = entry["relation_merged"] if entry else {}
        self.relation_keys = entry["relation_keys"] if entry else []
        self.traj_intervals = entry["traj_intervals"] if entry else {}

    def moved(self, index, row0):
        new = TrainVideo.__new__(TrainVideo)
        new.__dict__.update(self.__dict__)
        new.index, new.row0 = int(index), int(row0)
        return new

    def __bool__(self):
        return bool(self.relation_keys)


class TrainSource:
    """A training cache entry (load_train_video) with its per-frame rows on the device: vis (R, V), clip (R, Cc) or None and
    the clamped boxes (R, 4), interval after interval in (trajectory, interval) order -- the layout of PairSource --; the
    relation tables stay on the host (`videos`).  `concat` puts several videos into one row space: a step of train_policy
    spans several videos."""

    def __init__(self, vis, clip, boxes, videos):
        self.vis, self.clip, self.boxes, self.videos = vis, clip, boxes, list(videos)
        self.n_visual = 0 if vis is None else vis.shape[1]
        self.n_clip = 0 if clip is None else clip.shape[1]
        # (n videos, 2) w, h: what sequence p's boxes are normalised by, looked up through TrainTables.src
        self.frame_wh = np.asarray([(v.video_hw[1], v.video_hw[0]) if v.video_hw else (1, 1) for v in self.videos], dtype=np.float32)

    @classmethod
    def from_entry(cls, entry, device):
        if not entry:
            return cls(None, None, None, [TrainVideo(0, 0, {}, {}, 0)])
        h, w = entry["video_hw"]
        first_row, vis, boxes, clip, at = {}, [], [], [], 0
        for t in sorted(entry["visual_features"]):
            for i, rows in enumerate(entry["visual_features"][t]):
                first_row[(t, i)] = at
                at += rows.shape[0]
                vis.append(rows)
                boxes.append(_clamped(entry["entity_bboxes"][t][i], w, h))
                assert boxes[-1].shape[0] == rows.shape[0]
                if "clip_features" in entry:
                    clip.append(entry["clip_features"][t][i])
        put = lambda ts: torch.cat(ts, dim=0).to(device=device, dtype=torch.float32).contiguous()        # noqa: E731
        return cls(put(vis), put(clip) if clip else None, put(boxes), [TrainVideo(0, 0, entry, first_row, at)])

    @classmethod
    def concat(cls, sources):
        """One source over the rows of several: video j of the result is `videos[j]`, its rows moved behind those of the
        sources in front of it; every video keeps its own frame size.  Empty sources (no rows) keep their place in `videos`."""
        sources = list(sources)
        assert sources, "TrainSource.concat needs at least one source"
        full = [s for s in sources if s.vis is not None]
        if len({(s.n_visual, s.n_clip) for s in full}) > 1:
            raise ValueError("TrainSource.concat: the sources have different feature widths")
        videos, at = [], 0
        for s in sources:
            for v in s.videos:
                videos.append(v.moved(len(videos), at + v.row0))
            at += 0 if s.vis is None else s.vis.shape[0]
        if not full:
            return cls(None, None, None, videos)
        cat = lambda ts: torch.cat(ts, dim=0).contiguous()         # noqa: E731
        return cls(cat([s.vis for s in full]), None if full[0].clip is None else cat([s.clip for s in full]),
                   cat([s.boxes for s in full]), videos)

    def __len__(self):
        return len(self.videos)


class TrainTables:
    """train_tables' result: per surviving relation key the first subject / object row in the source (sub-sampling offset
    and crop folded in), its length, `lead` (sub-sampled frames in front of the crop: what the first frame's box differences
    look back to) and the video it belongs to; per key `preds` (N,) int64 and `segs` (N, 2) like train_getitem's lists."""

    def __init__(self, stride, max_seq_len, keys=(), s_row=(), o_row=(), lens=(), lead=(), src=(), preds=(), segs=()):
        self.stride, self.max_seq_len = int(stride), int(max_seq_len)
        self.keys = list(keys)
        self.s_row, self.o_row = np.asarray(s_row, dtype=np.int64), np.asarray(o_row, dtype=np.int64)
        self.lens, self.lead, self.src = (np.asarray(a, dtype=np.int32) for a in (lens, lead, src))
        self.preds, self.segs = list(preds), list(segs)
        self._device = None

    def __len__(self):
        return len(self.keys)

    @property
    def sizes(self):
        return [int(p.shape[0]) for p in self.preds]

    @classmethod
    def concat(cls, tables):
        """The keys of several tables (the (video, pair_duration) slices of one train_policy step, all addressing ONE
        TrainSource) one after the other."""
        tables = list(tables)
        assert tables and len({(t.stride, t.max_seq_len) for t in tables}) == 1
        cat = lambda name: np.concatenate([getattr(t, name) for t in tables])          # noqa: E731
        return cls(tables[0].stride, tables[0].max_seq_len, [k for t in tables for k in t.keys], cat("s_row"), cat("o_row"),
                   cat("lens"), cat("lead"), cat("src"), [p for t in tables for p in t.preds], [s for t in tables for s in t.segs])

    def check(self, source):
        """Every row the gather will read lies inside the source (the kernel trusts the tables)."""
        n_rows = 0 if source.boxes is None else source.boxes.shape[0]
        back = np.minimum(self.lead, 1).astype(np.int64) * self.stride
        last = (self.lens.astype(np.int64) - 1) * self.stride
        for row in (self.s_row, self.o_row):
            if len(row) and (int((row - back).min()) < 0 or int((row + last).max()) >= n_rows):
                raise ValueError("TrainTables: a sequence reaches outside its source's rows (tables of another source?)")
        if len(self.src) and (int(self.src.min()) < 0 or int(self.src.max()) >= len(source.videos)):
            raise ValueError("TrainTables: video index outside the source")
        if len(self.lens) and (int(self.lens.min()) < 2 or int(self.lens.max()) > self.max_seq_len):
            raise ValueError("TrainTables: sequence lengths must lie in [2, max_seq_len]")

    def on_device(self, source):
        """The tables as device tensors, uploaded once, in ONE host-to-device copy: {s_row, o_row (K,) int64; lens, lead (K,)
        int32; seq_wh (K, 2) float32; seg_lo, seg_hi (G,) int32; preds (G,) int64; segs (G, 2) in the dtype torch.cat gives
        the per-key lists}."""
        dev = source.boxes.device
        if self._device is not None and self._device[0] is source:
            return self._device[1]
        self.check(source)
        segs = torch.cat(self.segs, dim=0)
        seg_i = segs.to(torch.int64)
        if not bool(((seg_i[:, 0] >= 0) & (seg_i[:, 0] < seg_i[:, 1]) & (seg_i[:, 1] <= self.max_seq_len)).all()):
            raise ValueError("TrainTables: a relation segment lies outside [0, max_seq_len]")
        parts = [("s_row", self.s_row), ("o_row", self.o_row), ("preds", torch.cat(self.preds).to(torch.int64).numpy()),
                 ("segs", segs.contiguous().numpy().reshape(-1)), ("lens", self.lens), ("lead", self.lead),
                 ("seq_wh", source.frame_wh[self.src].reshape(-1)), ("seg_lo", seg_i[:, 0].numpy().astype(np.int32)),
                 ("seg_hi", seg_i[:, 1].numpy().astype(np.int32))]
        parts.sort(key=lambda kv: -kv[1].dtype.itemsize)               # 8-byte tables first: every view stays aligned
        raw = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for _, a in parts])
        buf = torch.from_numpy(raw).to(dev)
        out, at = {}, 0
        for name, a in parts:
            out[name] = buf[at:at + a.nbytes].view(torch.from_numpy(a[:0].copy()).dtype)
            at += a.nbytes
        out["seq_wh"] = out["seq_wh"].view(-1, 2)
        out["segs"] = out["segs"].view(-1, 2)
        self._device = (source, out)
        return out


def train_tables(video, feat_stride, max_seq_len, cut_max_preds=False, proposal_max_preds=0, pair_duration=None, rng=None):
    """train_getitem's decisions without its tensors: `video` is a one-video TrainSource or one of a concatenated source's
    `videos`; same arguments, same draws from `rng` in the same order (the sub-sampling offset per key, the crop draws of
    truncate_feats), same `continue` rules.  Touches no feature row.  Returns TrainTables (len 0 when nothing survives)."""
    import random
    rng = rng or random
    if isinstance(video, TrainSource):
        assert len(video.videos) == 1, "train_tables takes one video: pass source.videos[j] of a concatenated source"
        video = video.videos[0]
    out = TrainTables(feat_stride, max_seq_len)
    if not video:
        return out
    merged, keys = video.relation_merged, video.relation_keys
    if pair_duration is not None:
        keys = keys[pair_duration[0]:pair_duration[1]]
        merged = {k: v for k, v in merged.items() if list(k) in keys}
    rows = {name: [] for name in ("s_row", "o_row", "lens", "lead")}
    for key in merged:
        offset = rng.randint(0, feat_stride - 1)
        s, o, si, oi = key
        if cut_max_preds and proposal_max_preds < len(merged[key]):
            continue
        s_iv, o_iv = video.traj_intervals[s][si], video.traj_intervals[o][oi]
        lo, hi = max(s_iv[0], o_iv[0]), min(s_iv[1], o_iv[1])
        L = len(range(offset, max(hi - lo, 0), feat_stride))              # frames of per[lo - iv[0]:hi - iv[0]][offset::feat_stride]
        if L < 2:
            continue
        preds, segs = [], []
        for r in merged[key]:
            left = np.ceil((r["begin_fid"] - lo - offset) / feat_stride)
            right = np.ceil((r["end_fid"] - lo - offset) / feat_stride)
            if left < right:
                preds.append(r["predicate"])
                segs.append([left, right])
        if not preds:
            continue
        preds, segs, st = torch.tensor(preds, dtype=torch.int64), torch.tensor(np.array(segs), dtype=torch.int64), 0
        if L > max_seq_len:
            win = _truncate_window(L, preds, segs, max_seq_len, rng=rng)
            if win is None:
                continue
            st, preds, segs = win
            L = max_seq_len
        first = lo + offset + st * feat_stride
        rows["s_row"].append(video.row0 + video.first_row[(s, si)] + first - s_iv[0])
        rows["o_row"].append(video.row0 + video.first_row[(o, oi)] + first - o_iv[0])
        rows["lens"].append(L)
        rows["lead"].append(st)
        out.keys.append(tuple(key))
        out.preds.append(preds)
        out.segs.append(segs)
    return TrainTables(feat_stride, max_seq_len, out.keys, rows["s_row"], rows["o_row"], rows["lens"], rows["lead"],
                       [video.index] * len(out.keys), out.preds, out.segs)


def train_policy(video_num_pairs, num_pairs):
    """Steps of at most num_pairs relation keys, videos cut across steps where needed: [[(video, (first, last))]] per step;
    restates `apply_policy`, dataloaders/vidvrd.py:100-135."""
    policy, current = [[]], 0
    for name, n in video_num_pairs:
        if n + current < num_pairs:
            policy[-1].append([name, (0, n)])
            current += n
            continue
        start = 0
        while n + current >= num_pairs:
            take = num_pairs - current
            policy[-1].append([name, (start, start + take)])
            n -= take
            start += take
            current = 0
            policy.append([])
        if n > 0:
            policy[-1].append([name, (start, start + n)])
            current += n
    return policy
