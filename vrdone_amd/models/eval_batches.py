"""Eval batching: everything between "a list of pairs with lengths" and "the heads' outputs per pair", each step written once.

`MaskVRD` decides the policy (tight_len, tight_buckets, eval_plan, _chunk_size, _eval_rows_form: models/maskvrd.py); the
network is composed in the modules' `cl` methods over a `ragged.Layout`.  What lies between is here:

  * planning, on the host: a `Bucket` is the pairs of one padded length that share a launch; `runs` finds the buckets of a
    sorted pair list, `waves` cuts buckets into launch waves of at most `step` pairs, `add_filler` puts the all-padding
    sequences that round a row space to a multiple of 256 rows behind the last flat bucket, `pair_order` is the order and
    padded length of every pair of a call;
  * input sources: where a bucket's operands come from -- the dataloader's per-pair matrices (`Matrices`, ops.pack_pairs),
    per-tracklet features (`Tracklets`, ops.gather_pairs), those with the entity stage run once per tracklet
    (`SharedStreams`), or plain padded features (`Padded`: MaskVRD._batch, then _mask_vrd);
  * sinks: `store_candidates` writes a vrd_postprocess result into the candidate record, `new_outputs` / `scatter_heads`
    keep the batch-shaped output dict of `_mask_vrd`;
  * drivers: `_mask_vrd` in one row space (`mask_vrd_rows`), `MaskVRD.pair_candidates` bucket by bucket
    (`candidates_buckets`, with the eval_graph.py hook) and in one row space per wave (`candidates_rows`).
"""
import math
from collections import namedtuple

import torch

from . import ragged


def _ops():
    from .. import ops      # deferred: planning needs no GPU and no built library
    return ops


# T: padded length; sel: the bucket's pairs in the input source -- a device int32 index tensor into the caller's batch
# (MaskVRD._tight_plan), a range of positions in the call's pair list (pair_candidates), None for a filler bucket;
# n: pairs; flat: every sequence ends in two padded frames (the dense k = 3 convs run flat over such buckets: models/ragged.py)
Bucket = namedtuple("Bucket", "T sel n flat")
# what a source hands the backbone for one bucket.  kind "parts": vis, clip, so_box, ent, mask -- raw features, the entity stage
# is still to run; kind "so": so, so_box, mask -- the entity stage's rows
Operands = namedtuple("Operands", "kind vis clip so_box ent so mask")
# what the steps of one pair_candidates call share
Run = namedtuple("Run", "model source lens_dev k cand")


# ---- planning (host only) ---------------------------------------------------------------------------------------------------
def runs(ids, t_pad, lens=None):
    """The buckets of consecutive equal padded length in the pair list `ids`, sel = range of positions in `ids`.  With `lens`
    (`ids` sorted by length within a padded length) a run's pairs within one frame of their padded length (no two padded frames
    behind them) are a bucket of their own behind the flat one; without, one bucket per run and nothing known about flat."""
    out, at = [], 0
    while at < len(ids):
        T = t_pad[ids[at]]
        end = at + 1
        while end < len(ids) and t_pad[ids[end]] == T:
            end += 1
        cut = at
        while lens is not None and cut < end and lens[ids[cut]] <= T - 2:
            cut += 1
        if cut > at:
            out.append(Bucket(T, range(at, cut), cut - at, True))
        if cut < end:
            out.append(Bucket(T, range(cut, end), end - cut, False))
        at = end
    return out


def waves(buckets, step):
    """`buckets` cut into launch waves of `step` pairs (the last one takes the rest); a bucket that crosses a wave's end is split."""
    out, wave, room = [], [], step
    for b in buckets:
        at = 0
        while at < b.n:
            take = min(b.n - at, room)
            wave.append(Bucket(b.T, b.sel[at:at + take], take, b.flat))
            at += take
            room -= take
            if room == 0:
                out.append(wave)
                wave, room = [], step
    if wave:
        out.append(wave)
    return out


def add_filler(wave, t_max):
    """The wave with its flat buckets first (stable: each kind keeps its order) and, behind the last flat one, the filler buckets
    (sel None, all-padding sequences) its row count asks for: ragged.filler_buckets."""
    wave = sorted(wave, key=lambda b: not b.flat)
    at = sum(1 for b in wave if b.flat)
    wave[at:at] = [Bucket(T, None, n, True) for n, T in ragged.filler_buckets(sum(b.n * b.T for b in wave), t_max)]
    return wave


def pair_order(model, lens, t_refs):
    """(order, t_pad) of the pairs of one call: the tight padded length of every pair under its reference length t_refs[i], and
    the pairs by (padded length, valid length, index) -- every padded length then is one run."""
    t_pad = model.tight_buckets(lens, t_refs, model.ROWS_MIN_ROWS if model._eval_rows_form(len(lens)) else None)
    return sorted(range(len(lens)), key=lambda i: (t_pad[i], lens[i], i)), t_pad


# ---- input sources ----------------------------------------------------------------------------------------------------------
def _parts(t):
    return Operands("parts", t[0], t[1], t[2], t[3], None, t[4])


class Source:
    """Where the operands of a bucket of pair_candidates come from.  `operands(bucket)` is the one method a source has to have
    (`Padded`, which goes through _mask_vrd, has `outputs` in its place); the rest is what the drivers make of it.
    refs: the reference's padded length of the pair at every position of the call's pair list, for a model with absolute position
    rows (pair_candidates sets it; None otherwise)."""
    refs = None

    def refs_of(self, b):
        """the reference lengths of the pairs of bucket b (one int where they agree), or None: no position rows / a filler bucket"""
        if self.refs is None or b.sel is None:
            return None
        r = self.refs[b.sel.start:b.sel.stop]
        return r[0] if len(set(r)) == 1 else tuple(r)

    def prepare(self, wave):
        """before the operands of the buckets of `wave` are asked for one by one"""

    def from_streams(self, b):
        return False

    def features(self, b):
        """the backbone's pyramid and masks of bucket b, in the batch form"""
        o, bb = self.operands(b), self.model.backbone
        if o.kind == "so":
            return bb.pair_stage(o.so, o.so_box, o.mask)
        return bb.cl_parts(o.vis, o.clip, o.so_box, o.ent, o.mask, self.refs_of(b))

    def outputs(self, b):
        """the output dict of bucket b on its own, in launch waves"""
        model = self.model
        return model._merge([model._heads(*self.features(piece), False) for piece, in waves([b], model._chunk_size(b.n))])


class Matrices(Source):
    """The dataloader's frame-major (L, C_in) matrix per pair, as ops.pair_table's (pointers, lengths) on the device: they go
    straight into the backbone's operand buffers.  A small bucket's whole device side can be a recorded graph (eval_graph.py)."""

    def __init__(self, model, tables, c_in=None):
        self.model, self.tables, self.c_in, self._storage = model, tables, c_in, None

    def operands(self, b):
        ops, bb = _ops(), self.model.backbone
        return _parts(ops.pack_pairs(self.tables[0][b.sel.start:b.sel.stop], self.tables[1][b.sel.start:b.sel.stop], b.T, bb.n_visual,
                                     bb.n_clip, bb.n_bbox_so, bb.n_bbox_entity, ops.pair_mode()))

    def replay(self, b, k):
        """vrd_postprocess's outputs of bucket b from a recorded graph, or None"""
        from .. import eval_graph
        # (a recording is made per padded length; position rows follow the pairs' reference lengths: such a model runs eagerly)
        if b.n > eval_graph.MAX_PAIRS or self.refs is not None:
            return None
        if self._storage is None:                   # (one walk over the parameters per call instead of one per bucket)
            self._storage = eval_graph.storage_key(self.model)
        return eval_graph.bucket_candidates(self.model, self.tables[0][b.sel.start:b.sel.stop], self.tables[1][b.sel.start:b.sel.stop],
                                            b.T, k, self.c_in, self._storage)


class Tracklets(Source):
    """A proposals.PairSource: pair rows are gathered on the device from the per-tracklet features, the box features computed
    there (vrd_gather_pairs).  ids_dev: the call's pair list on the device; shared: SharedStreams' per-tracklet rows."""

    def __init__(self, model, pairs, ids_dev, shared=None):
        self.model, self.pairs, self.ids_dev, self.shared, self._edge = model, pairs, ids_dev, shared, None

    def operands(self, b):
        ops, bb = _ops(), self.model.backbone
        assert (self.pairs.n_visual, self.pairs.n_clip) == (bb.n_visual, bb.n_clip)
        return _parts(ops.gather_pairs(self.pairs, self.ids_dev[b.sel.start:b.sel.stop], b.T, bb.n_bbox_so, bb.n_bbox_entity, ops.pair_mode()))


class SharedStreams(Tracklets):
    """Tracklets with the backbone's entity stage run ONCE PER TRACKLET (`streams`) instead of twice per pair: a pair's entity
    rows are put together from its tracklets' rows and, within `reach` frames of the window's edges, from short pieces run
    through the same stage (`pieces`, `entity_rows`).  Buckets too short for that (T <= 2 piece buffers) are plain Tracklets."""

    @staticmethod
    def streams(model, source, ids):
        """The entity stage per tracklet (per sub-sampling phase) for the pairs `ids` of a proposals.PairSource:
        (rows (n_streams * Ts, D), stream_row (2, len(ids)) int64 device = row of frame 0 of each pair's subject / object,
        (piece length, piece buffer length), reach).  None when the stage cannot be shared: switched off, no tracklet table, or
        global attention in the first stem block (backbones.entity_reach)."""
        import numpy as np
        bb = model.backbone
        reach = bb.entity_reach()
        if not model.share_tracklets or reach is None or source.first_row is None:
            return None
        ops = _ops()
        dev = model.device
        start, length, stream, j0 = source.stream_plan(ids)
        chunk = 2 * (bb.mha_win_size[0] // 2)                  # the local attention takes whole chunks (blocks.py:828)
        unit = math.lcm(32, chunk)
        Ts = -(-int(length.max()) // unit) * unit
        stream_row = torch.from_numpy(stream.astype(np.int64) * Ts + j0).to(dev)       # uploads first, kernels after
        starts, lengths = torch.from_numpy(start).to(dev), torch.from_numpy(length).to(dev)
        wh = source.rows_wh(start)                             # (a source of several videos: each stream's own frame size)
        wh = None if wh is None else torch.from_numpy(wh).to(dev)
        n = len(start)
        D = bb.s_fuse_norm.num_channels
        rows = torch.empty(n, Ts, D, device=dev, dtype=torch.float32)
        step = max(1, (2 * model.pair_chunk * 288) // Ts)
        for c0 in range(0, n, step):
            c1 = min(c0 + step, n)
            # (the gather writes a subject and an object half; a stream is both)
            vis, clip, _, ent, m = ops.gather_rows(source, starts[c0:c1], starts[c0:c1], lengths[c0:c1], Ts, bb.n_bbox_so,
                                                   bb.n_bbox_entity, ops.pair_mode(), seq_wh=None if wh is None else wh[c0:c1])
            h = c1 - c0
            rows[c0:c1] = bb.entity_stage(vis[:h], clip[:h] if clip is not None else None, ent[:h], m)
        piece = -(-2 * reach // chunk) * chunk
        return rows, stream_row, (piece, piece + chunk), reach

    def pieces(self, sel, T):
        """The window-edge pieces of the pairs `sel` (device indices) through the entity stage: (4B, L, D) = [subject start |
        subject end | object start | object end] pieces.  T: the pairs' padded length (an int, or one per pair as a device
        tensor: the pairs of several buckets in one batch)."""
        ops = _ops()
        bb, source = self.model.backbone, self.pairs
        _, _, (piece, L), _ = self.shared
        s_row, o_row, lens = source.s_row[sel], source.o_row[sel], source.lens_dev[sel].contiguous()
        # start pieces: the first `piece` frames.  End pieces: the last `piece` frames followed by padding, as in the pair's
        # own rows -- or, for a pair that fills its T frames, the last L frames filling the buffer (vrd_assemble_args)
        end_len = torch.where(lens == T, L, piece).to(torch.int32)
        end_len = torch.where(lens > piece, end_len, torch.zeros_like(end_len))
        tail = (lens - end_len).clamp(min=0).long() * source.stride
        piece_s = torch.cat([s_row, s_row + tail])                  # [start pieces | end pieces]
        piece_o = torch.cat([o_row, o_row + tail])
        piece_len = torch.cat([lens.clamp(max=piece), end_len])
        wh = source.pair_wh_of(sel)
        vis, clip, _, ent, m = ops.gather_rows(source, piece_s, piece_o, piece_len, L, bb.n_bbox_so, bb.n_bbox_entity,
                                               ops.pair_mode(), seq_wh=None if wh is None else torch.cat([wh, wh]))
        return bb.entity_stage(vis, clip, ent, torch.cat([m, m], dim=0))                   # (4B, L, D)

    def entity_rows(self, sel, at, T, pieces=None):
        """(2B, T, D) entity-stage rows of the pairs `sel` (device indices; positions at.. of the id list the streams were
        planned for), the pairs' box features (B, T, S) and mask: frames further than `reach` from both window edges come
        from the per-tracklet rows, the rest from L-frame pieces at the edges run through the same stage (`pieces`: those,
        when the caller has them already -- `prepare` over the pairs of several buckets at once)."""
        ops = _ops()
        bb, source = self.model.backbone, self.pairs
        rows, stream_row, (piece, L), reach = self.shared
        B = sel.shape[0]
        s_row, o_row, lens = source.s_row[sel], source.o_row[sel], source.lens_dev[sel].contiguous()
        if pieces is None:
            pieces = self.pieces(sel, T)
        _, _, so_box, _, mask = ops.gather_rows(source, s_row.contiguous(), o_row.contiguous(), lens, T, bb.n_bbox_so,
                                                bb.n_bbox_entity, False, boxes_only=True, seq_wh=source.pair_wh_of(sel))
        so = ops.assemble_pairs(rows, pieces, stream_row[:, at:at + B].reshape(-1), lens, T, piece, reach)
        return so, so_box, mask

    def from_streams(self, b):
        return b.sel is not None and b.T > 2 * self.shared[2][1]

    def prepare(self, wave):
        """the window-edge pieces of all buckets of the wave that take their entity rows from the streams: ONE pass through the
        entity stage (they are L frames long whatever the bucket)"""
        mine = [b for b in wave if self.from_streams(b)]
        self._edge = None
        if len(mine) > 1:
            sel_all = torch.cat([self.ids_dev[b.sel.start:b.sel.stop] for b in mine])
            t_all = torch.cat([torch.full((b.n,), b.T, dtype=torch.int32, device=sel_all.device) for b in mine])
            self._edge = (self.pieces(sel_all, t_all), [b.sel.start for b in mine], [b.n for b in mine])

    def operands(self, b):
        if not self.from_streams(b):
            return super().operands(b)
        pieces = None
        if self._edge is not None:
            every, starts, sizes = self._edge
            q0, n_all = sum(sizes[:starts.index(b.sel.start)]), sum(sizes)
            pieces = torch.cat([every[j * n_all + q0:j * n_all + q0 + b.n] for j in range(4)])
        so, so_box, mask = self.entity_rows(self.ids_dev[b.sel.start:b.sel.stop], b.sel.start, b.T, pieces)
        return Operands("so", None, None, so_box, None, so, mask)


class Padded(Source):
    """Per-pair features in any other form (channel-major tensors): a zero-padded batch per bucket (MaskVRD._batch) through
    MaskVRD._mask_vrd, which plans its own launches."""

    def __init__(self, model, feats):
        self.model, self.feats = model, feats

    def outputs(self, b):
        refs = self.refs_of(b)
        if not isinstance(refs, tuple):
            x, m = self.model._batch(self.feats, b.sel, b.T)
            return self.model._mask_vrd(x, m, with_aux=False, t_ref=refs)
        # pairs of one padded length whose reference lengths differ (long pairs of several slices): a batch per reference length
        groups = {}
        for pos, r in zip(b.sel, refs):
            groups.setdefault(r, []).append(pos)
        outs = [self.model._mask_vrd(*self.model._batch(self.feats, ps, b.T), with_aux=False, t_ref=r) for r, ps in groups.items()]
        back = torch.empty(b.n, dtype=torch.int64)
        back[torch.tensor([pos - b.sel.start for ps in groups.values() for pos in ps])] = torch.arange(b.n)
        back = back.to(outs[0]["pred_logits"].device)
        return {key: torch.cat([o[key] for o in outs])[back] for key in ("pred_logits", "pred_masks")}


def _filler_operands(bb, b, kind, dev):
    """a filler bucket: zero rows under an all-false mask -- entity rows when every bucket of the wave brings those, else raw
    features (the entity stage's row space is rounded too)"""
    zeros = lambda n, width: torch.zeros(n, b.T, width, device=dev, dtype=torch.float32)               # noqa: E731
    no_mask = torch.zeros(b.n, b.T, dtype=torch.bool, device=dev)
    if kind == "so":
        so = zeros(2 * b.n, bb.s_fuse_norm.num_channels)
        return Operands("so", None, None, zeros(b.n, bb.n_bbox_so), None, so, no_mask)
    wide = (lambda w: _ops().Pair(zeros(2 * b.n, w), w)) if _ops().pair_mode() else (lambda w: zeros(2 * b.n, w))         # noqa: E731
    return Operands("parts", wide(bb.n_visual), wide(bb.n_clip) if bb.n_clip else None, zeros(b.n, bb.n_bbox_so),
                    zeros(2 * b.n, bb.n_bbox_entity), None, no_mask)


# ---- sinks ------------------------------------------------------------------------------------------------------------------
def store_candidates(cand, c0, c1, post, k):
    """vrd_postprocess's (top scores, top classes, first, last frame) of the pairs at c0..c1 into the candidate record
    (P, Q, 2k + 2) float32 = [top-k scores | top-k class ids | first | last frame], the integer fields bit-cast"""
    ints = cand.view(torch.int32)
    cand[c0:c1, :, :k] = post[0]
    ints[c0:c1, :, k:2 * k] = post[1]
    ints[c0:c1, :, 2 * k] = post[2]
    ints[c0:c1, :, 2 * k + 1] = post[3]


def new_outputs(B, T, Q, K1, n_aux, dev):
    """the batch-shaped output dict of _mask_vrd: pred_logits (B, Q, K+1), pred_masks (B, Q, T) filled with the predictor's value
    on padded frames (predictor.py:39), one such pair per auxiliary layer"""
    new = lambda: {"pred_logits": torch.empty(B, Q, K1, device=dev), "pred_masks": torch.full((B, Q, T), -10.0, device=dev)}  # noqa: E731
    return dict(new(), aux_outputs=[new() for _ in range(n_aux)]) if n_aux else new()


def scatter_heads(dst, idx64, t2, logits, masks):
    """one layer's heads of a bucket (pairs idx64 of the batch, t2 frames) into its output dict"""
    dst["pred_logits"][idx64] = logits
    dst["pred_masks"][idx64, :, :t2] = masks


class _ScatterHeads(torch.autograd.Function):
    """One layer's heads of all buckets of a row space -> the batch-shaped (pred_logits (B, Q, K+1), pred_masks (B, Q, T) with the
    predictor's fill on padded frames): what scatter_heads writes bucket by bucket, as one differentiable step of a training pass.
    Backward gathers: a bucket's rows of the two gradients, its own frames of the masks'."""

    @staticmethod
    def forward(ctx, T, idx64, frames, logits, *segs):
        B, (Q, K1) = logits.shape[0], logits.shape[1:]
        out = new_outputs(B, T, Q, K1, 0, logits.device)
        p = 0
        for i64, t2, seg in zip(idx64, frames, segs):
            scatter_heads(out, i64, t2, logits[p:p + i64.numel()], seg)
            p += i64.numel()
        assert p == B
        ctx.idx64, ctx.frames = idx64, frames
        return out["pred_logits"], out["pred_masks"]

    @staticmethod
    def backward(ctx, d_logits, d_masks):
        every = torch.cat(ctx.idx64) if len(ctx.idx64) > 1 else ctx.idx64[0]
        return (None, None, None, d_logits[every], *(d_masks[i64, :, :t2] for i64, t2 in zip(ctx.idx64, ctx.frames)))


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def unpack_rows(bb, x, index, lay):
    """backbones.py _unpack for the buckets of `lay`, bucket i the pairs index[i] (int32, device) of the caller's batch
    x (B, C_in, T) -> vis, clip, so_box, ent in the row space (vis / clip / ent stacked [subject | object])."""
    ops = _ops()
    R = lay.rows
    V, Cc, S, E = bb.n_visual, bb.n_clip, bb.n_bbox_so, bb.n_bbox_entity
    pair = ops.pair_mode()

    def stacked(c0, width, as_pair):
        h = lay.stacked().new(width, x)
        for (off, n, T), idx in zip(lay.segs, index):
            ops.bct_to_btc(x, c0, width, ragged._part(h, off, n, T), pair=as_pair, frames=T, index=idx)
            ops.bct_to_btc(x, c0 + width, width, ragged._part(h, R + off, n, T), pair=as_pair, frames=T, index=idx)
        return ops.Pair(h, width) if as_pair else h

    o0 = 2 * V + 2 * Cc
    so_box = lay.new(S, x)
    for (off, n, T), idx in zip(lay.segs, index):
        ops.bct_to_btc(x, o0, S, ragged._part(so_box, off, n, T), frames=T, index=idx)
    return stacked(0, V, pair), (stacked(2 * V, Cc, pair) if Cc else None), so_box, stacked(o0 + S, E, False)


def backbone_rows(bb, x, index, lay, mask):
    """backbones.py cl for the buckets of `lay` over the caller's batch x (B, C_in, T); mask: flat (1, R) validity of the rows"""
    vis, clip, so_box, ent = unpack_rows(bb, x, index, lay)
    so = bb.entity_stage(vis, clip, ent, torch.cat([mask, mask], dim=1), lay.stacked())
    return bb.pair_stage(so, so_box, mask, lay)


def mask_vrd_rows(model, x, masks2d, buckets, with_aux, t_ref=None, order=None):
    """MaskVRD._mask_vrd for `buckets` (sel: pair indices into the batch x (B, C_in, T)), each launch wave of at most ~pair_chunk
    pairs in one row space -> the batch-shaped output dict, at the batch's own padded length.
    t_ref: the reference's padded length of the pairs (default: the batch's T).
    order: a training step (autograd recording; MaskVRD._train_rows_step) -- the buckets' pair indices on the host, bucket by
    bucket: all B pairs in one wave without filler buckets, the layout knows every sequence's batch position (stochastic depth),
    and the heads reach the output dict through a differentiable scatter."""
    (B, T), dev, out = masks2d.shape, x.device, None
    if order is not None:
        return _train_rows(model, x, masks2d, buckets, with_aux, order)
    for wave in waves(buckets, model._chunk_size(B)):
        plan = add_filler(wave, T)
        # (a filler bucket recomputes the first frames of some pair under an all-false mask: finite numbers nobody reads)
        index = [b.sel if b.sel is not None else wave[0].sel[:1].repeat(b.n) for b in plan]
        lay = ragged.Layout([(b.n, b.T, b.flat) for b in plan])
        if model.use_abs_pe:            # (a filler bucket has no valid frame: any table serves it)
            lay = lay.with_refs([T if t_ref is None else t_ref] * len(plan))
        idx64 = [i.long() for i in index]
        mask = torch.cat([masks2d[i64, :b.T].reshape(-1) if b.sel is not None else torch.zeros(b.n * b.T, dtype=torch.bool, device=dev)
                          for b, i64 in zip(plan, idx64)]).view(1, lay.rows)
        heads = model._heads(*backbone_rows(model.backbone, x, index, lay, mask), with_aux, lay)
        if out is None:
            out = new_outputs(B, T, *heads[-1][0].shape[1:], len(heads) - 1, dev)
        for dst, (logits, segs) in zip(out.get("aux_outputs", []) + [out], heads):
            p = 0
            for b, i64, seg in zip(plan, idx64, segs):
                if b.sel is not None:
                    scatter_heads(dst, i64, b.T, logits[p:p + b.n], seg)
                p += b.n
    out["output_mask"] = masks2d[:, None, :]
    return out


def _train_rows(model, x, masks2d, plan, with_aux, order):
    """mask_vrd_rows under autograd: see there"""
    B, T = masks2d.shape
    assert sum(b.n for b in plan) == B == len(order)
    index = [b.sel for b in plan]
    lay = ragged.Layout([(b.n, b.T, b.flat) for b in plan]).with_order(order)
    idx64 = [i.long() for i in index]
    mask = torch.cat([masks2d[i64, :b.T].reshape(-1) for b, i64 in zip(plan, idx64)]).view(1, lay.rows)
    heads = model._heads(*backbone_rows(model.backbone, x, index, lay, mask), with_aux, lay)
    frames = [b.T for b in plan]
    layers = [dict(zip(("pred_logits", "pred_masks"), _ScatterHeads.apply(T, idx64, frames, logits, *segs))) for logits, segs in heads]
    out = layers[-1]
    if len(layers) > 1:
        out["aux_outputs"] = layers[:-1]
    out["output_mask"] = masks2d[:, None, :]
    return out


def bucket_candidates(model, table, lens_dev, T, k):
    """The device side of one bucket of forward_test: the pairs `table` (device pointers to their (L, C_in) matrices) /
    `lens_dev` at padded length T -> vrd_postprocess's (top scores, top classes, first, last frame).  No host read-back,
    shapes fixed by (T, number of pairs): what eval_graph.py records."""
    out = model._heads(*Matrices(model, (table, lens_dev)).features(Bucket(T, range(table.numel()), table.numel(), False)), False)
    return _ops().postprocess(out["pred_logits"].contiguous(), out["pred_masks"].contiguous(), lens_dev, k)


def candidates_buckets(run, ids, t_pad):
    """pair_candidates bucket by bucket: every run of one padded length in `ids` as a batch of its own"""
    for b in runs(ids, t_pad):
        c0, c1 = b.sel.start, b.sel.stop
        post = run.source.replay(b, run.k) if isinstance(run.source, Matrices) else None
        if post is None:
            out = run.source.outputs(b)
            post = _ops().postprocess(out["pred_logits"].contiguous(), out["pred_masks"].contiguous(), run.lens_dev[c0:c1], run.k)
        store_candidates(run.cand, c0, c1, post, run.k)


def _gather(run, wave):
    """the operands of every bucket of the wave, in wave order"""
    src = run.source
    real = [b for b in wave if b.sel is not None]
    src.prepare(real)
    kind = "so" if all(src.from_streams(b) for b in real) else "parts"
    return [src.operands(b) if b.sel is not None else _filler_operands(run.model.backbone, b, kind, run.cand.device) for b in wave]


def _raw_entity_stage(bb, wave, got, refs=None):
    """The entity stage of the buckets that bring raw features, in a row space of their own, [subject | object] like the joint
    one -> (its rows (1, 2 R_e, D), R_e), or (None, 0) without such a bucket.  refs: the buckets' reference lengths (Layout.with_refs)."""
    ops = _ops()
    raw = [(b, o) for b, o in zip(wave, got) if o.kind == "parts"]
    if not raw:
        return None, 0
    lay = ragged.Layout([(b.n, b.T, b.flat) for b, _ in raw])
    if refs is not None:
        lay = lay.with_refs([r for r, o in zip(refs, got) if o.kind == "parts"])

    def stacked(ts):
        if ts[0] is None:
            return None
        both = [ragged._raw(t) for t in ts]
        halves = [t[:t.shape[0] // 2] for t in both] + [t[t.shape[0] // 2:] for t in both]
        flat_rows = torch.cat([h.reshape(-1, h.shape[-1]) for h in halves]).view(1, 2 * lay.rows, -1)
        return ops.Pair(flat_rows, ts[0].width, ts[0].fmt) if isinstance(ts[0], ops.Pair) else flat_rows
    mask = torch.cat([o.mask.reshape(-1) for _, o in raw]).view(1, lay.rows)
    return bb.entity_stage(stacked([o.vis for _, o in raw]), stacked([o.clip for _, o in raw]), stacked([o.ent for _, o in raw]),
                           torch.cat([mask, mask], dim=1), lay.stacked()), lay.rows


def _joint_rows(wave, got, so_raw, rows_raw, lay):
    """the entity-stage rows of the whole wave: every bucket's subject rows, then every bucket's object rows"""
    halves, at = ([], []), 0
    for b, o in zip(wave, got):
        rows = b.n * b.T
        if o.kind == "so":
            halves[0].append(o.so[:b.n].reshape(rows, -1))
            halves[1].append(o.so[b.n:].reshape(rows, -1))
        else:
            halves[0].append(so_raw[0, at:at + rows])
            halves[1].append(so_raw[0, rows_raw + at:rows_raw + at + rows])
            at += rows
    return torch.cat(halves[0] + halves[1]).view(1, 2 * lay.rows, -1)


def candidates_rows(run, lens, ids, t_pad):
    """pair_candidates with the buckets of a wave in ONE row space (models/ragged.py): the entity stage of the buckets that do
    not take it from the per-tracklet rows, then the pair stage, neck and predictor once over all rows."""
    model, bb = run.model, run.model.backbone
    for wave in waves(runs(ids, t_pad, lens), model._chunk_size(len(ids))):
        wave = add_filler(wave, 1 << 30)
        lay = ragged.Layout([(b.n, b.T, b.flat) for b in wave])
        got = _gather(run, wave)
        mask = torch.cat([o.mask.reshape(-1) for o in got]).view(1, lay.rows)
        so_box = torch.cat([o.so_box.reshape(-1, bb.n_bbox_so) for o in got]).view(1, lay.rows, -1)
        # (absolute position rows: every pair's reference length, a filler bucket's own -- it has no valid frame)
        refs = None if run.source.refs is None else [b.T if b.sel is None else run.source.refs_of(b) for b in wave]
        so = _joint_rows(wave, got, *_raw_entity_stage(bb, wave, got, refs), lay)
        del got
        logits, segs = model._heads(*bb.pair_stage(so, so_box, mask, lay), False, lay)[-1]
        p = 0
        for b, seg in zip(wave, segs):
            if b.sel is not None:
                c0, c1 = b.sel.start, b.sel.stop
                post = _ops().postprocess(logits[p:p + b.n].contiguous(), seg, run.lens_dev[c0:c1], run.k)
                store_candidates(run.cand, c0, c1, post, run.k)
            p += b.n


def pair_candidates(model, feats, lens, ids, t_pad, k, source=None, t_refs=None):
    """MaskVRD.pair_candidates: the candidate record of the pairs `ids` (already grouped by padded length)."""
    ops = _ops()
    dev = model.device
    cand = torch.empty(len(ids), model.predictor.num_queries, 2 * k + 2, device=dev, dtype=torch.float32)
    if not ids:
        return cand
    # every host->device table goes up before the first kernel is queued (such a copy waits for the queue)
    lens_dev = torch.tensor([lens[i] for i in ids], dtype=torch.int32, device=dev)
    if source is not None:
        ids_dev = torch.tensor(ids, dtype=torch.int64, device=dev)
        shared = SharedStreams.streams(model, source, ids)
        src = Tracklets(model, source, ids_dev) if shared is None else SharedStreams(model, source, ids_dev, shared)
    else:
        local = [feats[i] for i in ids]
        tables = ops.pair_table(local)      # None unless the features are the dataloader's frame-major matrices
        src = Padded(model, local) if tables is None else Matrices(model, tables, int(local[0].shape[0]))
    if model.use_abs_pe:
        if t_refs is None:
            t_refs = model._reference_pad(lens)
        src.refs = [t_refs[i] for i in ids]
    run = Run(model, src, lens_dev, k, cand)
    if model._eval_rows_form(len(lens)) and not isinstance(src, Padded):
        # all padded lengths of the video in one row space, in waves of ~pair_chunk pairs
        candidates_rows(run, lens, ids, t_pad)
    else:
        candidates_buckets(run, ids, t_pad)
    return cand
