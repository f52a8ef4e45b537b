"""Layouts: where the sequences of an activation lie in its rows, and the operations that need to know.

The network is composed once, in the modules' `cl` methods (blocks.py, local_transformer.py, backbones.py, fpns.py,
predictor.py).  Most of it works row by row -- LayerNorm, every k = 1 conv GEMM with its epilogue (bias, GELU, channel scale,
residuals, row mask), which is the bulk of the FLOPs -- and does not care which rows share a launch.  The rest needs the
(sequences, frames) structure: depthwise conv + LayerNorm (stride 1 / 2, FPN upsample-add), the banded and the global
attention, the pyramid's max-pool, the dense k = 3 convs, the mask head, and taking the subject / object halves of a stacked
buffer.  Those operations live here and take a `Layout`; the `cl` methods pass their layout(s) on to them.  Nothing here takes a
model or a backbone: which pairs share a row space, where their operands come from and where the heads' outputs go is
models/eval_batches.py (it builds the layouts; `filler_buckets` here tells it how to round their row count).  Two forms exist:

  * the batch form (`Layout.batch`, what a `cl` method reads from its tensors' shape when no layout is given): B sequences of
    T frames as a (B, T, C) tensor.  Every operation here is then the one `ops.*` call on that tensor, and under autograd its
    result is the tensor the op recorded.  Training runs in this form unless `MaskVRD.train_rows` is set.
  * the row space: `MaskVRD._mask_vrd` computes the pairs of a batch at the shortest padded lengths that give
    the reference's outputs (`tight padding`, models/maskvrd.py), pairs of equal padded length as one bucket.  Run bucket by
    bucket, every launch of the network shrinks with its bucket, and below ~260 k rows a bucket's GEMMs fall off the 256 x 256
    kernel.  So all buckets lie back to back in one (1, R, C) buffer per activation -- bucket i = rows [off_i, off_i + n_i * T_i)
    as n_i sequences of T_i frames --, the row-by-row kernels run ONCE over all rows, and only the operations here walk the
    buckets (or hand them to a kernel as its row groups, vrd_row_segs).

The dense k = 3 convs of the embedding stage run once over the rows of a row space too: a k = 3 conv reads its two neighbour rows,
and in a flat row space frame 0 of a sequence would read the last frame of the sequence before it, where the reference's
Conv1d(padding=1) reads zero.  That last frame is zeroed in the conv's input.  It is read by itself, by the frame before it and by
the next sequence's first frame: the first two are padded frames here (tight padding keeps a coarsest-level stride of padded
frames behind every pair it shortens; pairs within one frame of their padded length are bucketed apart, behind the others, and
their buckets' k = 3 convs run one by one) whose outputs the row mask zeroes, which makes the flat conv equal to the per-sequence
one on every valid row.

Under autograd (a training step with `MaskVRD.train_rows`) every operation here hands its layout's groups to ONE differentiable
op (vrdone_amd/autograd.py: `segs`), whose backward is one launch over all groups (depthwise conv, banded attention, max-pool)
or the batch form's entry point group by group on pointer offsets into one gradient tensor (global attention, mask head): no
operation slices the row space under autograd -- torch's slice backward would allocate and add a full-size zero tensor per group.
What stays inference-only: dwconv_ln_multi, absolute position rows (layernorm_pos, position_rows; a layout with t_refs) and `drop`.

Subject and object rows of the shared-weight stages are stacked as [all subject buckets | all object buckets] (`stacked`), so
that either half is a contiguous range with the same bucket layout; in the batch form that is one bucket of 2B sequences.
Reference: models/maskvrd.py:363-414 pads every pair to one length and computes every padded frame.
"""
from contextlib import nullcontext

import torch


def _ops():
    from .. import ops      # deferred: constructing / loading a model needs no GPU
    return ops


_MAX_SEGS = 32          # _hip.MAX_SEGS: groups of sequences one launch takes


class Layout:
    """Where the buckets lie in the rows of one pyramid level: segs = [(first row, sequences, frames)].
    Buckets whose sequences all end in two padded frames (`flat`) come first: over their rows [0, rows_flat) the dense k = 3
    convs run as one flat launch (see the module text); the others' k = 3 convs run bucket by bucket.
    axis: the tensor axis the sequences are stacked along -- 1 in the row space (1, R, C), 0 in the batch form (B, T, C)."""

    def __init__(self, buckets, axis=1):
        """buckets: [(sequences, frames, flat)]"""
        segs, flat, off = [], [], 0
        for n, T, f in buckets:
            segs.append((off, n, T))
            flat.append(bool(f))
            off += n * T
        assert flat == sorted(flat, reverse=True), "buckets that take the flat k = 3 convs come first"
        self._set(segs, flat, axis)

    def _set(self, segs, flat, axis):
        assert axis == 1 or len(segs) == 1
        self.segs, self.flat, self.axis = segs, flat, axis
        self.rows = sum(n * T for _, n, T in segs)
        self.rows_flat = sum(n * T for (_, n, T), f in zip(segs, flat) if f)
        self.lead = (1, self.rows) if axis else segs[0][1:]           # a tensor's shape in front of its channels
        self._tails, self._stacked = {}, None
        self.t_refs = None          # see with_refs
        self.order = None           # see with_order
        self._order_rows = {}

    @classmethod
    def _of_segs(cls, segs, flat, axis):
        lay = cls.__new__(cls)
        lay._set(segs, flat, axis)
        return lay

    _batches = {}

    @classmethod
    def batch(cls, n, T):
        """the batch form: one bucket of n sequences of T frames, as an (n, T, C) tensor"""
        lay = cls._batches.get((n, T))
        if lay is None:
            lay = cls._batches[(n, T)] = cls([(n, T, False)], axis=0)
        return lay

    @classmethod
    def of(cls, lay, x):
        """`lay`, or without one the batch form of the (B, T, ...) tensor / mask x"""
        return lay if lay is not None else cls.batch(x.shape[0], x.shape[1])

    def with_refs(self, t_refs):
        """This layout with the reference padded lengths of its sequences: t_refs[i] for bucket i, one int for all its sequences
        or one per sequence.  Absolute position rows are the reference's table of that length (backbones.position_operands),
        whatever length the sequence is computed at here; nothing else reads them."""
        assert len(t_refs) == len(self.segs) and all(isinstance(r, int) or len(r) == n for r, (_, n, _) in zip(t_refs, self.segs))
        lay = Layout._of_segs(self.segs, self.flat, self.axis)
        lay.t_refs = [r if isinstance(r, int) else tuple(r) for r in t_refs]
        return lay

    def with_order(self, order):
        """This layout with the batch position of every one of its sequences, in row order: `order` is a permutation of
        range(sequences) -- a training step in the row space lays the pairs out bucket by bucket, and per-sample state drawn in
        batch order (stochastic depth: blocks.AffineDropPath.row_factors) has to reach sample i's rows wherever they lie."""
        order = [int(i) for i in order]
        assert sorted(order) == list(range(sum(n for _, n, _ in self.segs)))
        lay = Layout._of_segs(self.segs, self.flat, self.axis)
        lay.t_refs, lay.order = self.t_refs, order
        return lay

    def _derived(self, lay, order=None):
        """`lay`, a layout of this one's sequences at other frame counts, with this one's batch positions (or `order`)"""
        if self.order is not None and lay.order is None:
            lay.order = self.order if order is None else order
            lay._order_rows = self._order_rows if order is None else {}
        return lay

    def sample_rows(self, device):
        """(samples, None) in the batch form, whose sequences are the samples in order; in a row space (samples, the batch
        position of every row's sequence as an int64 tensor on `device`), built once per layout and frame count."""
        n_seq = sum(n for _, n, _ in self.segs)
        if self.axis == 0:
            return n_seq, None
        assert self.order is not None, "a row space that takes per-sample factors needs its sequences' batch positions (with_order)"
        key = (tuple(self.segs), str(device))
        rows = self._order_rows.get(key)
        if rows is None:
            frames = torch.tensor([T for _, n, T in self.segs for _ in range(n)])
            rows = self._order_rows[key] = torch.repeat_interleave(torch.tensor(self.order), frames).to(device)
        return n_seq, rows

    def seq_refs(self):
        """the reference padded length of every sequence, in row order (None: no lengths given, the sequences' own)"""
        if self.t_refs is None:
            return None
        return [t for r, (_, n, _) in zip(self.t_refs, self.segs) for t in ((r,) * n if isinstance(r, int) else r)]

    def twice(self):
        """segs of the stacked [subject | object] rows"""
        return self.segs + [(self.rows + off, n, T) for off, n, T in self.segs]

    def stacked(self):
        """the layout of the stacked [subject | object] rows; the two halves of one bucket are one bucket of twice the sequences"""
        if self._stacked is None:
            if self.axis == 0:
                self._stacked = Layout.batch(2 * self.segs[0][1], self.segs[0][2])
            else:
                self._stacked = Layout._of_segs(self.twice(), self.flat * 2, 1)
            if self.t_refs is not None:         # (subject and object sequences share their pair's length)
                self._stacked = self._stacked.with_refs(self.t_refs * 2 if self.axis else [r if isinstance(r, int) else r * 2 for r in self.t_refs])
            if self.order is not None:          # (the batch form stacks [all subjects | all objects]: object i is sample B + i)
                self._stacked = self._derived(self._stacked, self.order + [len(self.order) + i for i in self.order])
        return self._stacked

    def strided(self, s):
        """the layout of the same sequences at every s-th frame"""
        if s == 1:
            return self
        if self.axis == 0:
            return Layout.batch(self.segs[0][1], self.segs[0][2] // s)
        return self._derived(Layout._of_segs([(off // s, n, T // s) for off, n, T in self.segs], self.flat, 1))

    def queries(self, Q):
        """Q rows per sequence (the predictor's queries), the sequences in the same order"""
        if self.axis == 0:
            return Layout.batch(self.segs[0][1], Q)
        return self._derived(Layout([(n, Q, False) for _, n, _ in self.segs]))

    def min_frames(self):
        return min(T for _, _, T in self.segs)

    def tail_rows(self, halves, device):
        """last row of every sequence of the flat buckets (of both halves of a stacked row space), built ON the device: a table
        uploaded from the host in the middle of a call would wait for every launch queued before it"""
        key = (halves, str(device))
        if key not in self._tails:
            idx = [torch.arange(h * self.rows + off + T - 1, h * self.rows + off + n * T, T, dtype=torch.int64, device=device)
                   for h in range(halves) for (off, n, T), f in zip(self.segs, self.flat) if f]
            self._tails[key] = (torch.cat(idx) if len(idx) > 1 else idx[0]) if idx else None
        return self._tails[key]

    def new(self, width, like, zeros=False):
        """a fresh f32 activation of `width` channels in this layout, on the device of `like`"""
        # under autograd a row space is one a training step laid out (with_order), without reference lengths: absolute position
        # rows keep the batch form in training
        assert self.axis == 0 or not torch.is_grad_enabled() or (self.order is not None and self.t_refs is None), \
            "a row space under autograd is a training step's (Layout.with_order), without reference lengths; any other is an inference form"
        return (torch.zeros if zeros else torch.empty)(*self.lead, width, device=_raw(like).device, dtype=torch.float32)

    def halves(self, x):
        """the subject and the object half of the tensor x of self.stacked()"""
        at, R = (slice(None),) * self.axis, self.lead[self.axis]
        return x[at + (slice(None, R),)], x[at + (slice(R, None),)]

    def part(self, x, seg):
        """the rows of the group seg = (first row, sequences, frames) of x (tensor, mask, Pair or None) as (sequences, frames, ...);
        in the batch form the one bucket is the tensor itself"""
        return x if self.axis == 0 else _part(x, *seg)

    def whole(self, y):
        """the (sequences, frames, ...) result y of a launch over all rows, in this layout's own form"""
        if self.axis == 0:
            return y
        ops = _ops()
        if isinstance(y, ops.Pair):
            return ops.Pair(self.whole(y.t), y.width, y.fmt)
        return y.view(1, y.shape[0] * y.shape[1], *y.shape[2:])


def _part(x, off, n, T):
    """rows [off, off + n T) of the flat (1, R, ...) operand x (tensor, mask, Pair or None) as (n, T, ...)"""
    if x is None:
        return None
    ops = _ops()
    if isinstance(x, ops.Pair):
        return ops.Pair(_part(x.t, off, n, T), x.width, x.fmt)
    if off == 0 and n * T == x.shape[1]:              # all rows: a view of the tensor itself (under autograd: no slice node)
        return x.view(n, T, *x.shape[2:])
    assert not (torch.is_grad_enabled() and x.requires_grad), "no operation slices a row space under autograd (see the module text)"
    return x[0, off:off + n * T].unflatten(0, (n, T))


def _merged(segs):
    """buckets of one frame count (the two halves of one bucket, the predictor's queries) are one launch"""
    if len(segs) > 1 and all(T == segs[0][2] for _, _, T in segs):
        return [(segs[0][0], sum(n for _, n, _ in segs), segs[0][2])]
    return segs


def _raw(x):
    return x.t if isinstance(x, _ops().Pair) else x


def _recorded(lay):
    """a row space under autograd: the operation hands the layout's groups to one differentiable op (see the module text)"""
    return lay.axis == 1 and torch.is_grad_enabled()


class _SplitRows(torch.autograd.Function):
    """The row runs [(first row, sequences, frames)] of x (1, R, C) as (sequences, frames, C) tensors.  Backward copies the runs'
    gradients into ONE (1, R, C) tensor (the runs cover all rows); slicing x run by run would have torch allocate and add a
    full-size zero tensor per run.  Its counterpart towards the result is torch.cat, whose backward takes views."""

    @staticmethod
    def forward(ctx, x, runs):
        assert sum(n * T for _, n, T in runs) == x.shape[1]
        ctx.runs, ctx.shape = runs, x.shape
        return tuple(x[0, off:off + n * T].unflatten(0, (n, T)).clone() for off, n, T in runs)

    @staticmethod
    def backward(ctx, *grads):
        dx = torch.empty(ctx.shape, device=grads[0].device, dtype=grads[0].dtype)
        for (off, n, T), g in zip(ctx.runs, grads):
            dx[0, off:off + n * T] = g.reshape(n * T, -1)
        return dx, None


def _rows_of(x, sl):
    ops = _ops()
    return ops.Pair(x.t[:, sl], x.width, x.fmt) if isinstance(x, ops.Pair) else x[:, sl]


def dwconv_ln(lay, x, sets, mask_out, *, stride=1, x_up=None, pre_ln=None):
    """ops.dwconv_ln over the buckets of x's layout `lay`: outputs and mask_out at every stride-th frame, x_up the rows of the
    coarser level.  One launch: a single group of sequences in the kernel's own form, several as its row groups (vrd_row_segs)."""
    ops = _ops()
    if _recorded(lay):
        return ops.dwconv_ln(x, sets, mask_out=mask_out, stride=stride, x_up=x_up, pre_ln=pre_ln, segs=list(lay.segs))
    segs = _merged(lay.segs)
    if len(segs) == 1:
        off, n, T = segs[0]
        res = ops.dwconv_ln(lay.part(x, segs[0]), sets, mask_out=lay.part(mask_out, (off // stride, n, T // stride)), stride=stride,
                            x_up=lay.part(x_up, (off // 2, n, T // 2)), pre_ln=pre_ln)
        return [lay.whole(r) for r in res]
    Cout = sets[0]["weight"].shape[0]
    bufs = [torch.empty(1, lay.rows // stride, Cout, device=x.device, dtype=torch.float32) for _ in sets]
    for g0 in range(0, len(segs), _MAX_SEGS):
        part = segs[g0:g0 + _MAX_SEGS]
        r0, r1 = part[0][0], part[-1][0] + part[-1][1] * part[-1][2]
        rel = [(off - r0, n, T) for off, n, T in part]
        ops.dwconv_ln(x[:, r0:r1], [dict(st, out=b[:, r0 // stride:r1 // stride]) for st, b in zip(sets, bufs)],
                      mask_out=None if mask_out is None else mask_out[:, r0 // stride:r1 // stride], stride=stride,
                      x_up=None if x_up is None else x_up[:, r0 // 2:r1 // 2], pre_ln=pre_ln, segs=rel)
    return [ops.Pair(b, Cout) if ops._fmt(st.get("pair")) else b for st, b in zip(sets, bufs)]


def dwconv_ln_multi(lay, x, sets, mask_out, *, pre_ln=None):
    """ops.dwconv_ln_multi over the buckets of x's layout `lay` (stride 1): up to five sets from one pass over the rows of x"""
    ops = _ops()
    segs = _merged(lay.segs)
    if len(segs) == 1:
        res = ops.dwconv_ln_multi(lay.part(x, segs[0]), sets, mask_out=lay.part(mask_out, segs[0]), pre_ln=pre_ln)
        return [lay.whole(r) for r in res]
    Cout = sets[0]["weight"].shape[0]
    bufs = [torch.empty(1, lay.rows, Cout, device=x.device, dtype=torch.float32) for _ in sets]
    for g0 in range(0, len(segs), _MAX_SEGS):
        part = segs[g0:g0 + _MAX_SEGS]
        r0, r1 = part[0][0], part[-1][0] + part[-1][1] * part[-1][2]
        ops.dwconv_ln_multi(x[:, r0:r1], [dict(st, out=b[:, r0:r1]) for st, b in zip(sets, bufs)],
                            mask_out=None if mask_out is None else mask_out[:, r0:r1], pre_ln=pre_ln,
                            segs=[(off - r0, n, T) for off, n, T in part])
    return [ops.Pair(b, Cout) if ops._fmt(st.get("pair")) else b for st, b in zip(sets, bufs)]


def _pos_launches(lay):
    """the launches of a position-row kernel over the sequences of `lay`: [(segs or None, T or None, first sequence, sequences)]
    -- one for a single group of sequences, else one per _MAX_SEGS buckets as its row groups"""
    if len(_merged(lay.segs)) == 1:
        (_, n, T), = _merged(lay.segs)
        return [(None, T, 0, n)]
    out, at = [], 0
    for g0 in range(0, len(lay.segs), _MAX_SEGS):
        part = lay.segs[g0:g0 + _MAX_SEGS]
        seqs = sum(n for _, n, _ in part)
        out.append((part, None, at, seqs))
        at += seqs
    return out


def layernorm_pos(lay, x, norm, mask, pos, *, relu=False, out=None, pair=False):
    """ops.layernorm_pos over the sequences of `lay`: LayerNorm (+ ReLU) of the rows x, then the position row of every valid
    frame.  pos = (table, first): the tables of the call's reference lengths and the first table row of every sequence of `lay`
    in row order (backbones.position_operands)."""
    ops = _ops()
    table, first = pos
    if out is None:
        out = lay.new(x.shape[-1], x)
    for segs, T, s0, n in _pos_launches(lay):
        ops.layernorm_pos(x, norm.weight, norm.bias, table, first[s0:s0 + n], mask, T=T, segs=segs, relu=relu, out=out, pair=pair)
    return ops.Pair(out, x.shape[-1]) if pair else out


def position_rows(lay, mask, pos):
    """the masked position rows of the sequences of `lay` as (rows, C) f32 rows: what layernorm_pos adds (the CLIP variant adds
    them as a GEMM's residual)"""
    ops = _ops()
    table, first = pos
    out = torch.empty(lay.rows, table.shape[-1], device=table.device, dtype=torch.float32)
    for segs, T, s0, n in _pos_launches(lay):
        ops.position_rows(table, first[s0:s0 + n], mask, T=T, segs=segs, out=out)
    return out


def attention(q, k, v, kv_mask, q_mask, n_head, qlay, klay, *, half_win=None, rel_pe=None, pair=False, drop=None):
    """Global (half_win None) or banded attention of the queries in `qlay` over the keys in `klay`: bucket by bucket, or the
    buckets as the row groups of one kernel call (banded attention; global attention on pair rows with ATTN_SEGS).
    q_mask: rows the caller masks afterwards (global attention only).
    drop: the attn_drop call of a training step (blocks.Drop; banded attention in the batch form only)."""
    ops = _ops()
    qsegs, ksegs = qlay.segs, klay.segs
    if drop is not None:
        assert half_win is not None and len(qsegs) == 1 and qlay.axis == 0, "attention dropout: banded attention in the batch form"
        return qlay.whole(ops.local_attention(qlay.part(q, qsegs[0]), klay.part(k, ksegs[0]), klay.part(v, ksegs[0]),
                                              klay.part(kv_mask, ksegs[0]), n_head, half_win, rel_pe=rel_pe, drop=drop))
    # buckets of one frame count on both sides (the predictor's query self-attention: every bucket is n x Q rows) are one launch
    if len(_merged(qsegs)) == 1 and len(_merged(ksegs)) == 1:
        qsegs, ksegs = _merged(qsegs), _merged(ksegs)
    if _recorded(qlay):
        assert drop is None and klay.axis == 1
        if half_win is not None:
            assert list(qsegs) == list(ksegs)
            return ops.local_attention(q, k, v, kv_mask, n_head, half_win, rel_pe=rel_pe, segs=list(qsegs))
        return ops.attention(q, k, v, kv_mask, n_head, segs=(list(qsegs), list(ksegs)))

    def one(qs, ks, out=None):
        assert qs[1] == ks[1]
        qp, kp, vp, mp = qlay.part(q, qs), klay.part(k, ks), klay.part(v, ks), klay.part(kv_mask, ks)
        if half_win is not None:
            assert qs[2] == ks[2]
            return ops.local_attention(qp, kp, vp, mp, n_head, half_win, pair=pair, rel_pe=rel_pe, out=out)
        return ops.attention(qp, kp, vp, mp, n_head, pair=pair, q_mask=qlay.part(q_mask, qs), out=out)

    if len(qsegs) == 1:
        return qlay.whole(one(qsegs[0], ksegs[0]))
    Cc = q.shape[-1]
    dev = _raw(q).device
    out = torch.empty(1, qlay.rows, Cc, device=dev, dtype=torch.float32)
    if half_win is not None and len(qsegs) <= _MAX_SEGS:      # banded attention: the buckets as the kernel's row groups
        assert list(qsegs) == list(ksegs)
        r = ops.local_attention(q, k, v, kv_mask, n_head, half_win, pair=pair, rel_pe=rel_pe, out=out, segs=list(qsegs))
        return ops.Pair(out, Cc, r.fmt) if isinstance(r, ops.Pair) else out
    if half_win is None and ATTN_SEGS and all(isinstance(x, ops.Pair) for x in (q, k, v)):
        # global attention on pair rows, opted in: the buckets as the row groups of one call (two launches at the most), in
        # runs of _MAX_SEGS buckets; f32 rows (the exact mode, the generic kernel, training) keep the bucket walk below
        for g0 in range(0, len(qsegs), _MAX_SEGS):
            r = ops.attention(q, k, v, kv_mask, n_head, pair=pair, q_mask=q_mask, out=out,
                              segs=(list(qsegs[g0:g0 + _MAX_SEGS]), list(ksegs[g0:g0 + _MAX_SEGS])))
        return ops.Pair(out, Cc, r.fmt) if isinstance(r, ops.Pair) else out
    # global attention walks the buckets; a bucket's launch is n x heads x query blocks workgroups of one per CU -- 4.02 rounds
    # of the chip for 257 pairs x 4 heads take five --, so the buckets' launches alternate between ATTN_LANES streams and fill
    # each other's last rounds
    lanes = _lanes(dev) if half_win is None and len(qsegs) > 2 else None
    if lanes:
        main = torch.cuda.current_stream(dev)
        ready = torch.cuda.Event()
        ready.record(main)
        for lane in lanes:
            lane.wait_event(ready)
    for i, (qs, ks) in enumerate(zip(qsegs, ksegs)):
        at = i % (len(lanes) + 1) if lanes else 0
        with torch.cuda.stream(lanes[at - 1]) if at else nullcontext():
            r = one(qs, ks, _part(out, *qs))
    if lanes:
        for lane in lanes:
            main.wait_stream(lane)
    return ops.Pair(out, Cc, r.fmt) if isinstance(r, ops.Pair) else out


ATTN_LANES = int(__import__("os").environ.get("VRDONE_ROWS_ATTN_STREAMS", "2"))      # streams the buckets' global attention alternates between
# opt-in (VRDONE_ROWS_ATTN_SEGS=1): global attention on pair rows takes the buckets as the row groups of one call instead of
# walking them over the side streams (a module value, like ATTN_LANES: tests and A/B runs flip it in one process)
ATTN_SEGS = __import__("os").environ.get("VRDONE_ROWS_ATTN_SEGS", "0") == "1"
_side_streams = {}


def _lanes(dev):
    """the side streams of `dev` (ATTN_LANES - 1 of them), or None: one stream, or a capture in progress"""
    if ATTN_LANES <= 1 or torch.cuda.is_current_stream_capturing():
        return None
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), ATTN_LANES)
    if key not in _side_streams:
        _side_streams[key] = [torch.cuda.Stream(device=dev) for _ in range(ATTN_LANES - 1)]
    return _side_streams[key]


def maxpool_mask(lay, x, mask):
    """ops.maxpool_mask (the pyramid's stride-2 skip path) bucket by bucket -> (pooled rows, mask) in lay.strided(2)"""
    ops = _ops()
    if _recorded(lay):
        return ops.maxpool_mask(x, mask, segs=list(lay.segs))
    if len(lay.segs) == 1:
        y, m_out = ops.maxpool_mask(lay.part(x, lay.segs[0]), lay.part(mask, lay.segs[0]))
        return lay.whole(y), lay.whole(m_out)
    y = torch.empty(1, lay.rows // 2, x.shape[-1], device=x.device, dtype=torch.float32)
    m_out = torch.empty(1, lay.rows // 2, device=x.device, dtype=torch.bool)
    for off, n, T in lay.segs:
        ops.maxpool_mask(_part(x, off, n, T), _part(mask, off, n, T), out=(_part(y, off // 2, n, T // 2), _part(m_out, off // 2, n, T // 2)))
    return y, m_out


def conv3(lay, h, conv, row_mask, *, out=None, out_pair=False, norm=None):
    """A dense k = 3 conv * mask over the sequences of `lay`.  In a row space: one flat launch per run of buckets whose sequences
    end in two padded frames (their last rows zeroed in the input first), bucket by bucket for the others.
    norm: the LayerNorm (+ ReLU) behind a few-channel conv, fused into the same launches (ops.conv_ln); with few input channels
    and no norm the conv alone runs as that row kernel."""
    ops = _ops()
    assert conv.kernel_size[0] == 3
    ln = {} if norm is None else dict(gamma=norm.weight.reshape(-1), beta=norm.bias.reshape(-1), relu=True)
    small = ops.conv_ln_ok(h, conv.weight, conv.bias, *((norm.weight, norm.bias) if norm is not None else ()))
    assert small or norm is None

    def one(x, m, o):
        if small:
            return ops.conv_ln(x, conv.weight, conv.bias, row_mask=m, out=o, pair=out_pair, **ln)
        return ops.conv_gemm(x, conv.weight, conv.bias, row_mask=m, out=o, out_pair=out_pair)
    if lay.axis == 0:
        return one(h, row_mask, out)
    tails = lay.tail_rows(1, _raw(h).device)
    if torch.is_grad_enabled():
        # under autograd: the zeroing of the tail rows is recorded (those rows receive no gradient), and the flat run and the
        # other buckets are the runs of one split -- a single flat run is the tensor itself
        if tails is not None:
            h = h.index_fill(1, tails, 0.0) if h.requires_grad else h.index_fill_(1, tails, 0.0)
        runs, flat_before = [], False          # (a stacked layout has its flat buckets in front of either half)
        for (off, n, T), f in zip(lay.segs, lay.flat):
            if f and flat_before and runs[-1][0] + runs[-1][2] == off:
                runs[-1] = (runs[-1][0], 1, runs[-1][2] + n * T)
            else:
                runs.append((off, 1, n * T) if f else (off, n, T))
            flat_before = f
        if len(runs) == 1:
            return one(h, row_mask, None)
        parts = _SplitRows.apply(h, runs) if h.requires_grad else [_part(h, *run) for run in runs]
        outs = [one(x, _part(row_mask, *run), None) for x, run in zip(parts, runs)]
        return torch.cat([o.reshape(1, -1, o.shape[-1]) for o in outs], dim=1)
    N = conv.weight.shape[0]
    if out is None:
        out = lay.new(N, h)
    if tails is not None:
        _raw(h)[0].index_fill_(0, tails, 0.0)            # (f32 rows or pair rows: all-zero bits are the value zero in both)
    at = 0
    while at < len(lay.segs):
        off, n, T = lay.segs[at]
        if lay.flat[at]:
            while at + 1 < len(lay.segs) and lay.flat[at + 1]:
                at += 1
            sl = slice(off, lay.segs[at][0] + lay.segs[at][1] * lay.segs[at][2])
            one(_rows_of(h, sl), row_mask[:, sl], out[:, sl])
        else:
            one(_part(h, off, n, T), _part(row_mask, off, n, T), _part(out, off, n, T))
        at += 1
    return ops.Pair(out, N) if out_pair else out


def mask_head(lay, emb, feat, out_mask, fill):
    """ops.mask_head bucket by bucket: emb (B, Q, Dp) of all pairs in bucket order -> [mask logits (n_i, Q, T_i) per bucket]"""
    ops = _ops()
    if _recorded(lay):
        return list(ops.mask_head(emb, feat, out_mask, fill, segs=list(lay.segs)))
    if len(lay.segs) == 1:
        return [ops.mask_head(emb, lay.part(feat, lay.segs[0]), lay.part(out_mask, lay.segs[0]), fill)]
    segs_out, p = [], 0
    for off, n, T in lay.segs:
        segs_out.append(ops.mask_head(emb[p:p + n], _part(feat, off, n, T), _part(out_mask, off, n, T), fill))
        p += n
    return segs_out


def filler_buckets(rows, t_max):
    """[(sequences, frames)] of all-padding sequences that round a row space of `rows` rows up to a multiple of 256: the
    256 x 256 GEMM kernel takes row counts that are multiples of 64 (its epilogue has no row predicates), and with 256 that
    holds for the first three pyramid levels -- the launches large enough for that kernel.  Sequences of 32 frames, plus one of
    32 + (8, 16 or 24) when the buckets' lengths are not all multiples of 32 (reference padded lengths are multiples of the
    window stride, e.g. 48); none when such a sequence would be longer than t_max (the frames the caller's batch has)."""
    need = (-rows) % 256
    if need == 0 or rows % 8 or rows < 65536:          # (below ~65 k rows no launch reaches the 256 x 256 kernel)
        return []
    odd = need % 32
    first = 32 + odd if odd else 0
    if first > t_max or t_max < 32:
        return []
    if need < first:
        need += 256
    out = [(1, first)] if first else []
    if need - first:
        out.insert(0, ((need - first) // 32, 32))
    return out
