"""Backbone of the relation encoder: embedding convs, entity-box fusion, stem (local-window
transformer on subject and object) interleaved with subject<->object mutual attention, s/o
fusion and the stride-2 pyramid branch.  Same constructor and parameter tree as the reference's
models/backbones.py; the forward chains HIP kernels on channels-last buffers.

Subject and object share the embedding / stem weights (reference backbones.py:172-177,
213-214), so both streams run as ONE batch of 2B sequences; concatenations are never
materialised -- producers write into column slabs of the consumer's input buffer.
"""
import torch
from torch import nn

from . import ragged
from .blocks import ConvMLP, LayerNorm, Layout, MaskedConv1D, TransformerBlock, _from_cl, _mask2d, _ops, get_sinusoid_encoding
from .local_transformer import MaskedConvTransformerDecoderLayer, MaskedMHCA_QKV

# The subject / object layers of pair_stage read each original stream three times per stage (see _sos_stream).  From
# SOS_MERGE_MIN_ROWS rows per stream on (VRDONE_SOS_MERGE_MIN_ROWS), inference reads it once: SOS_MERGE_FORM "c" = one
# vrd_dwconv_ln_multi launch of five sets, "b" = two (the stream's own q / k / v, then the other layer's k / v).  Same bits as
# the three vrd_dwconv_ln launches; below the threshold, and under autograd, nothing changes.  Module values: tests and A/B
# runs flip them in one process.
SOS_MERGE_MIN_ROWS = int(__import__("os").environ.get("VRDONE_SOS_MERGE_MIN_ROWS", str(1 << 15)))
SOS_MERGE_FORM = __import__("os").environ.get("VRDONE_SOS_MERGE_FORM", "c")


def _sos_merge(s_attn, o_attn, rows):
    if torch.is_grad_enabled() or rows < SOS_MERGE_MIN_ROWS:
        return False
    mods = [m for layer in (s_attn, o_attn) for m in (layer.self_attn, layer.multihead_attn)]
    return all(isinstance(m, MaskedMHCA_QKV) and m.n_embd == 512 and
               all(getattr(m, f"{n}_conv").conv.kernel_size == (3,) for n in ("query", "key", "value")) for m in mods)


def _sos_stream(lay, x, mask, own, other):
    """The depthwise-conv + LayerNorm branches that read the stream x: its own layer's self-attention q / k (behind ln1) and v
    (raw), and the other layer's cross-attention k / v (raw) -> (self_ready of `own`, cross_ready of `other`) for the layers' cl"""
    sa, ca = own.self_attn, other.multihead_attn
    sets = [dict(sa._branch_set("query"), normed=True), dict(sa._branch_set("key"), normed=True), sa._branch_set("value"),
            ca._branch_set("key"), ca._branch_set("value")]
    pre_ln = (own.ln1.weight, own.ln1.bias)
    if SOS_MERGE_FORM == "b":
        res = ragged.dwconv_ln_multi(lay, x, sets[:3], mask, pre_ln=pre_ln) + ragged.dwconv_ln_multi(lay, x, sets[3:], mask)
    else:
        res = ragged.dwconv_ln_multi(lay, x, sets, mask, pre_ln=pre_ln)
    return dict(zip(("query", "key", "value"), res[:3])), dict(zip(("key", "value"), res[3:]))


class MaskConvTransformerBackbone(nn.Module):
    def __init__(self, n_visual, n_bbox_entity, n_bbox_so, n_embd, n_head, n_embd_ks, fuse_ks, n_fuse_head,
                 fuse_path_drop, fuse_qx_stride, fuse_kv_stride, max_len, arch=(2, 2, 3), mha_win_size=[-1] * 4,
                 scale_factor=2, with_ln=False, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0, use_abs_pe=False,
                 use_rel_pe=False, use_local=True):
        super().__init__()
        assert len(arch) == 3 and len(mha_win_size) == 1 + arch[-1]
        assert with_ln, "built for embd_with_ln=True"
        assert scale_factor == 2 and n_embd_ks == 3
        self.n_visual, self.n_bbox_entity, self.n_bbox_so = n_visual, n_bbox_entity, n_bbox_so
        self.n_clip = 0
        self.arch, self.mha_win_size, self.max_len = arch, mha_win_size, max_len
        self.relu = nn.ReLU(inplace=True)
        self.scale_factor, self.use_abs_pe, self.use_rel_pe = scale_factor, use_abs_pe, use_rel_pe

        if use_abs_pe:      # reference backbones.py:70-72 (not part of the checkpoint)
            self.register_buffer("pos_embd", get_sinusoid_encoding(max_len, n_embd) / (n_embd ** 0.5), persistent=False)
        self.visual_embd, self.visual_embd_norm = self._embedding(n_visual, n_embd, n_embd_ks, arch[0])
        self.bbox_entity_embd = MaskedConv1D(n_bbox_entity, n_embd, n_embd_ks, stride=1, padding=n_embd_ks // 2)
        self.bbox_entity_norm = LayerNorm(n_embd)
        self.visual_bbox_fuse = ConvMLP(n_embd * 2, n_embd, n_embd, kernel_size=fuse_ks, num_layers=2)

        self.stem = nn.ModuleList()
        self.s_attn = nn.ModuleList()
        self.o_attn = nn.ModuleList()
        for _ in range(arch[1]):
            self.stem.append(TransformerBlock(n_embd, n_head, n_ds_strides=(1, 1), attn_pdrop=attn_pdrop,
                                              proj_pdrop=proj_pdrop, path_pdrop=path_pdrop,
                                              mha_win_size=mha_win_size[0], use_rel_pe=use_rel_pe))
            for mutual in (self.s_attn, self.o_attn):
                mutual.append(MaskedConvTransformerDecoderLayer(
                    n_embd=n_embd, n_head=n_fuse_head, path_pdrop=fuse_path_drop, n_qx_stride=fuse_qx_stride,
                    n_kv_stride=fuse_kv_stride, with_ffn=False, use_local=use_local,
                    win_size=mha_win_size[0] if use_local else None))
        self.s_fuse_norm = LayerNorm(n_embd)
        self.o_fuse_norm = LayerNorm(n_embd)
        self.so_fuse = ConvMLP(n_embd * 2, n_embd, n_embd, kernel_size=fuse_ks, num_layers=2)
        self.bbox_so_embd = MaskedConv1D(n_bbox_so, n_embd, n_embd_ks, stride=1, padding=n_embd_ks // 2)
        self.so_visual_bbox_fuse = ConvMLP(n_embd * 2, n_embd, n_embd, kernel_size=fuse_ks, num_layers=2)

        self.branch = nn.ModuleList(
            TransformerBlock(n_embd, n_head, n_ds_strides=(scale_factor, scale_factor), attn_pdrop=attn_pdrop,
                             proj_pdrop=proj_pdrop, path_pdrop=path_pdrop, mha_win_size=mha_win_size[1 + i],
                             use_rel_pe=use_rel_pe)
            for i in range(arch[2]))
        self._zero_biases()

    @staticmethod
    def _embedding(n_in, n_embd, ks, depth):
        convs, norms = nn.ModuleList(), nn.ModuleList()
        for i in range(depth):
            convs.append(MaskedConv1D(n_in if i == 0 else n_embd, n_embd, ks, stride=1, padding=ks // 2, bias=False))
            norms.append(LayerNorm(n_embd))
        return convs, norms

    def _zero_biases(self):
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Conv1d)) and m.bias is not None:
                nn.init.zeros_(m.bias)

    def in_channels(self):
        return 2 * self.n_visual + 2 * self.n_clip + self.n_bbox_so + 2 * self.n_bbox_entity

    # -------------------------------------------------------------------------------------
    def _unpack(self, x, frames=None, index=None):
        """Boundary layout (B, C_in, T) -> the channels-last operand buffers of cl_parts: the subject and
        object slabs of every shared-weight stage are stacked on the batch axis (2B sequences); the wide
        visual / clip slabs feed GEMMs only, so they are pair rows in the split-precision modes.
        frames / index: only the first `frames` frames of the pairs x[index] (ops.bct_to_btc)."""
        ops = _ops()
        B, _, T = x.shape
        if index is not None:
            B = index.numel()
        if frames is not None:
            T = frames
        V, Cc, S, E = self.n_visual, self.n_clip, self.n_bbox_so, self.n_bbox_entity
        pair = ops.pair_mode()

        def stacked(c0, width, as_pair):
            h = torch.empty(2, B, T, width, device=x.device, dtype=torch.float32)
            ops.bct_to_btc(x, c0, width, h[0], pair=as_pair, frames=frames, index=index)
            ops.bct_to_btc(x, c0 + width, width, h[1], pair=as_pair, frames=frames, index=index)
            h = h.view(2 * B, T, width)
            return ops.Pair(h, width) if as_pair else h

        o0 = 2 * V + 2 * Cc
        so_box = torch.empty(B, T, S, device=x.device, dtype=torch.float32)
        ops.bct_to_btc(x, o0, S, so_box, frames=frames, index=index)
        return (stacked(0, V, pair), stacked(2 * V, Cc, pair) if Cc else None, so_box, stacked(o0 + S, E, False))

    @staticmethod
    def _embed(h, convs, norms, mask2, out, lay, post_add=None, pos=None):
        """k=3 conv * mask -> LN -> ReLU stack on the stacked sequences of `lay`; the last LN writes into `out`, a column
        slab of the consumer GEMM's input buffer (pair rows in bf16x3 mode).  Absolute position rows behind the last LN: post_add
        (materialised, one per row of a batch: the autograd path) or pos (position_operands: per-sequence tables, inference)."""
        ops = _ops()
        last = len(convs) - 1
        if last == 0 and post_add is None and pos is None and ops.conv_ln_ok(h, convs[0].conv.weight, convs[0].conv.bias, norms[0].weight, norms[0].bias):
            # few input channels (the box features): conv, mask, LayerNorm and ReLU as one row kernel, straight into the consumer's slab
            return ragged.conv3(lay, h, convs[0].conv, mask2, out=out, out_pair=ops.pair_mode(), norm=norms[0])
        for i, (conv, norm) in enumerate(zip(convs, norms)):
            h = ragged.conv3(lay, h, conv.conv, mask2)
            if i == last and pos is not None:
                return ragged.layernorm_pos(lay, h, norm, mask2, pos, relu=True, out=out, pair=ops.pair_mode())
            h = norm.cl(h, relu=True, out=out if i == last else None, pair=ops.pair_mode(), post_add=post_add if i == last else None)
        return h

    def cl(self, x, mask, t_refs=None):
        """x: (B, C_in, T) contiguous fp32 (the boundary layout), mask: (B, T) bool; t_refs: see cl_parts.
        Returns channels-last feats [(B, T/2^l, D)] and masks [(B, T/2^l)]."""
        assert x.shape[1] == self.in_channels(), f"expected {self.in_channels()} input channels, got {x.shape[1]}"
        return self.cl_parts(*self._unpack(x.contiguous()), mask, t_refs)

    def cl_parts(self, vis, clip, so_box, ent, mask, t_refs=None):
        """vis (2B, T, V), clip (2B, T, Cc) or None, so_box (B, T, S), ent (2B, T, E): channels-last operand
        buffers (from _unpack or ops.pack_pairs); mask (B, T) bool.
        t_refs: the length the reference pads the pairs to (an int, or one per pair) where that is not T -- the pairs of a
        tight-padding bucket; only absolute position rows depend on it (position_table)."""
        lay2 = None
        if t_refs is not None and self.use_abs_pe:
            lay2 = Layout.batch(*mask.shape).with_refs([t_refs if isinstance(t_refs, int) else tuple(t_refs)]).stacked()
        return self.pair_stage(self.entity_stage(vis, clip, ent, torch.cat([mask, mask], dim=0), lay2), so_box, mask)

    def entity_reach(self):
        """How many frames either side of a frame the entity stage reads (embedding convs, then the first stem block's
        depthwise conv and attention window), or None when that stage is not local (global attention)."""
        win = self.mha_win_size[0]
        if self.use_abs_pe:          # the position rows count frames of the PAIR's window
            return None
        if win <= 1 or any(c.kernel_size[0] != 1 for c in self.visual_bbox_fuse.layers):
            return None
        return self.arch[0] + 1 + win // 2        # k = 3 embedding convs, k = 3 depthwise conv, half a window

    def _position_rows(self, mask2):
        """Absolute position encoding as one row per (sequence, frame): the table's first T frames (linearly re-interpolated
        to T frames once T reaches max_len, eval only) on valid frames, zeros on padded ones (reference backbones.py:180-196)."""
        n, T = mask2.shape
        pe = self.pos_embd
        if self.training:
            assert T <= self.max_len, "Reached max length."
        elif T >= self.max_len:
            pe = torch.nn.functional.interpolate(pe, T, mode='linear', align_corners=False)
        rows = pe[0, :, :T].t()                                              # (T, D)
        return (rows[None] * mask2[..., None].to(rows.dtype)).reshape(n * T, -1).contiguous()

    def position_table(self, t_ref):
        """The (t_ref, D) position rows of a pair the reference pads to t_ref frames (reference backbones.py:187-196): the
        sinusoid table's first t_ref frames as they are below max_len, the table linearly re-interpolated to t_ref frames from
        max_len on (at max_len itself that is the table).  They do not depend on the length the pair is computed at: frame t of
        the pair gets row t.  Kept per t_ref for as long as pos_embd is the tensor it was built from."""
        pe = self.pos_embd
        key = (pe.data_ptr(), pe._version, str(pe.device))
        cache = self.__dict__.setdefault("_pos_tables", {})
        if cache.get("key") != key:
            cache.clear()
            cache["key"] = key
        t_ref = int(t_ref)
        if t_ref not in cache:
            rows = pe if t_ref < self.max_len else torch.nn.functional.interpolate(pe, t_ref, mode='linear', align_corners=False)
            cache[t_ref] = rows[0, :, :t_ref].t().contiguous()
        return cache[t_ref]

    _POS_PLANS = 64          # position_plan results kept (a video's bucket plan repeats from call to call)

    def position_plan(self, refs):
        """(table, pos_first) of a call whose sequences, in row order, have the reference lengths `refs` (subject and object
        sequences share their pair's entry): the tables of the distinct lengths one behind the other, (sum of lengths, D), and per
        sequence the first row of its length's table, int32 on pos_embd's device."""
        refs = tuple(int(r) for r in refs)
        self.position_table(refs[0])                  # (a replaced pos_embd empties the cache, the plans with it)
        cache = self._pos_tables
        plans = cache.setdefault("plans", {})
        hit = plans.get(refs)
        if hit is None:
            if len(plans) >= self._POS_PLANS:
                plans.clear()
            distinct = sorted(set(refs))
            start, at = {}, 0
            for t in distinct:
                start[t] = at
                at += t
            table = torch.cat([self.position_table(t) for t in distinct]) if len(distinct) > 1 else self.position_table(distinct[0])
            dev = self.pos_embd.device
            if len(distinct) == 1:                    # (built on the device: no upload in the middle of a call)
                first = torch.zeros(len(refs), dtype=torch.int32, device=dev)
            else:
                first = torch.tensor([start[t] for t in refs], dtype=torch.int32).to(dev)
            hit = plans[refs] = (table, first)
        return hit

    def position_operands(self, lay):
        """position_plan for the sequences of `lay`: their reference lengths (Layout.with_refs), their own where none are given"""
        t_refs = lay.t_refs if lay.t_refs is not None else [T for _, _, T in lay.segs]
        key = tuple((r, n) for r, (_, n, _) in zip(t_refs, lay.segs))           # (hashed in C: a call has thousands of sequences)
        self.position_table(lay.segs[0][2])
        plans = self._pos_tables.setdefault("plans", {})
        hit = plans.get(key)
        if hit is None:
            refs = [t for r, n in key for t in ((r,) * n if isinstance(r, int) else r)]
            frames = [T for _, n, T in lay.segs for _ in range(n)]
            assert all(r >= T for r, T in zip(refs, frames)), "a sequence is never computed at more frames than the reference pads it to"
            hit = self.position_plan(refs)
            plans[key] = hit
        return hit

    def entity_stage(self, vis, clip, ent, mask2, lay=None):
        """Everything that sees ONE entity's frames only -- embeddings, visual/box fusion and the first stem block, all
        with weights shared between subject and object (reference backbones.py:172-214): n sequences in, (n, T, D) out.
        Every op in it is local in time (see entity_reach), which is what lets forward_test run it once per tracklet
        instead of once per pair.  lay: the layout of the rows (default: the batch form of n sequences)."""
        ops = _ops()
        lay = Layout.of(lay, mask2)
        Cc = self.n_clip
        D = self.s_fuse_norm.num_channels
        new = lambda width: lay.new(width, mask2)          # noqa: E731

        # concatenation buffers hold two D-wide slabs; in bf16x3 mode both slabs are pair rows (width D)
        pair = ops.pair_mode()
        cat = (lambda t: ops.Pair(t, D)) if pair else (lambda t: t)          # noqa: E731

        # [visual (+clip) | entity box] -> visual_bbox_fuse
        # (ops.join: the slab-filled buffer, or -- under autograd, where ops return fresh tensors -- the concatenation)
        fuse_in = new(2 * D)
        # absolute position rows: pe[t] on valid frames, 0 on padded ones.  Inference: per-sequence tables of the pairs' reference
        # lengths, looked up by the kernel that adds them (pos); under autograd the materialised (n * T, D) rows of a batch (pe)
        pe = pos = None
        if self.use_abs_pe and torch.is_grad_enabled():
            assert lay.axis == 0 and lay.t_refs is None, "training runs in the batch form, at the batch's own padded length"
            pe = self._position_rows(mask2)
        elif self.use_abs_pe:
            pos = self.position_operands(lay)
        if Cc:
            vc = new(2 * D)
            a = self._embed(vis, self.visual_embd, self.visual_embd_norm, mask2, vc[..., :D], lay)
            b = self._embed(clip, self.clip_embd, self.clip_embd_norm, mask2, vc[..., D:], lay)
            # (CLIP variant: the position rows are added behind the visual / CLIP fusion, backbones.py:362-384)
            if pos is not None:
                pe = ragged.position_rows(lay, mask2, pos)
            a = self.visual_clip_fuse.cl(cat(ops.join(vc, (a, b))), row_mask=mask2, out=fuse_in[..., :D], out_pair=pair, res=pe)
        else:
            a = self._embed(vis, self.visual_embd, self.visual_embd_norm, mask2, fuse_in[..., :D], lay, post_add=pe, pos=pos)
        b = self._embed(ent, [self.bbox_entity_embd], [self.bbox_entity_norm], mask2, fuse_in[..., D:], lay)
        so = self.visual_bbox_fuse.cl(cat(ops.join(fuse_in, (a, b))), row_mask=mask2)
        so, _ = self.stem[0].cl(so, mask2, lay=lay)
        return so

    def pair_stage(self, so, so_box, mask, lay=None):
        """so: (2B, T, D) entity-stage output, subject rows then object rows; from the first subject<->object attention on.
        lay: the layout of the pairs' rows (of so_box and mask; so is in lay.stacked()); default: the batch form."""
        ops = _ops()
        lay = Layout.of(lay, mask)
        lay2 = lay.stacked()
        D = self.s_fuse_norm.num_channels
        mask2 = torch.cat([mask, mask], dim=lay.axis)
        pair = ops.pair_mode()
        cat = (lambda t: ops.Pair(t, D)) if pair else (lambda t: t)          # noqa: E731

        for i, (s_attn, o_attn) in enumerate(zip(self.s_attn, self.o_attn)):
            if i:
                so, _ = self.stem[i].cl(so, mask2, lay=lay2)
            s, o = lay.halves(so)
            nxt = lay2.new(D, mask)
            out_s, out_o = lay.halves(nxt)
            kw_s, kw_o = {}, {}
            if _sos_merge(s_attn, o_attn, lay.rows):
                # each original stream is read ONCE for its three readers (its own self-attention q / k and v, the other
                # layer's cross-attention k / v) instead of once per reader
                kw_s["self_ready"], kw_o["cross_ready"] = _sos_stream(lay, s, mask, s_attn, o_attn)
                kw_o["self_ready"], kw_s["cross_ready"] = _sos_stream(lay, o, mask, o_attn, s_attn)
            s2, _ = s_attn.cl(s, o, mask, mask, stream_add=s, out=out_s, qlay=lay, klay=lay, **kw_s)      # s + s_attn(s, o)
            o2, _ = o_attn.cl(o, s, mask, mask, stream_add=o, out=out_o, qlay=lay, klay=lay, **kw_o)      # uses the pre-update s
            so = ops.join(nxt, (s2, o2), dim=lay.axis)

        s, o = lay.halves(so)
        so_in = lay.new(2 * D, mask)
        a = self.s_fuse_norm.cl(s, out=so_in[..., :D], pair=pair)
        b = self.o_fuse_norm.cl(o, out=so_in[..., D:], pair=pair)
        pair_box = lay.new(2 * D, mask)
        a = self.so_fuse.cl(cat(ops.join(so_in, (a, b))), row_mask=mask, out=pair_box[..., :D], out_pair=pair)
        b = ragged.conv3(lay, so_box, self.bbox_so_embd.conv, mask, out=pair_box[..., D:], out_pair=pair)
        e = self.so_visual_bbox_fuse.cl(cat(ops.join(pair_box, (a, b))), row_mask=mask)

        feats, masks = [e], [mask]
        for blk in self.branch:
            e, mask = blk.cl(e, mask, lay=lay)
            lay = lay.strided(blk.attn.n_kv_stride)
            feats.append(e)
            masks.append(mask)
        return feats, masks

    def forward(self, x, mask):
        feats, masks = self.cl(x, _mask2d(mask))
        return tuple(_from_cl(f) for f in feats), tuple(m[:, None, :] for m in masks)


class MaskConvTransformerBackboneWithCLIP(MaskConvTransformerBackbone):
    """Adds the CLIP-feature embedding and its fusion MLP (reference models/backbones.py:250-436)."""

    def __init__(self, n_visual, n_clip, n_bbox_entity, n_bbox_so, n_embd, n_head, n_embd_ks, fuse_ks, n_fuse_head,
                 fuse_path_drop, fuse_qx_stride, fuse_kv_stride, max_len, arch=(2, 2, 3), mha_win_size=[-1] * 4,
                 scale_factor=2, with_ln=False, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0, use_abs_pe=False,
                 use_rel_pe=False, use_local=True):
        super().__init__(n_visual=n_visual, n_bbox_entity=n_bbox_entity, n_bbox_so=n_bbox_so, n_embd=n_embd,
                         n_head=n_head, n_embd_ks=n_embd_ks, fuse_ks=fuse_ks, n_fuse_head=n_fuse_head,
                         fuse_path_drop=fuse_path_drop, fuse_qx_stride=fuse_qx_stride, fuse_kv_stride=fuse_kv_stride,
                         max_len=max_len, arch=arch, mha_win_size=mha_win_size, scale_factor=scale_factor,
                         with_ln=with_ln, attn_pdrop=attn_pdrop, proj_pdrop=proj_pdrop, path_pdrop=path_pdrop,
                         use_abs_pe=use_abs_pe, use_rel_pe=use_rel_pe, use_local=use_local)
        self.n_clip = n_clip
        self.clip_embd, self.clip_embd_norm = self._embedding(n_clip, n_embd, n_embd_ks, arch[0])
        self.visual_clip_fuse = ConvMLP(n_embd * 2, n_embd, n_embd, kernel_size=fuse_ks, num_layers=2)
        self._zero_biases()
