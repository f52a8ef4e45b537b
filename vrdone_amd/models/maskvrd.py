"""MaskVRD facade: the reference's constructor, forward / _config_eval / _mask_vrd API and
checkpoint layout (models/maskvrd.py:16-167), with the relation-encoding hot path running on
hand-written HIP kernels and the eval post-processing (models/maskvrd.py:247-328) vectorised on
the device instead of a per-candidate Python loop.

Training: `model.train()(input_data)` returns the reference's loss dict (maskvrd.py:168-198) and
`loss_dict['total_loss'].backward()` runs the backward kernels of vrdone_amd/autograd.py; under torch.no_grad() the same
call is a validation pass on the fused inference kernels (no drop-path sampling).
"""
import gc
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from .backbones import MaskConvTransformerBackbone, MaskConvTransformerBackboneWithCLIP
from .blocks import TransformerBlock, _factor_pool, _ops, begin_dropout_step
from .. import train_graph
from . import eval_batches, losses
from .fpns import FPN1D_Fuse
from .predictor import MaskedTransformerPredictor


class MaskVRD(nn.Module):
    MAX_QUERIES = 64          # predictor.num_queries: 1..64 (mask head, device matcher and criterion kernels)

    def __init__(self, config, device):
        super().__init__()
        self.visual_dim = config['visual_dim']
        self.clip_dim = config.get('clip_dim', None)
        self.bbox_entity_dim = config['bbox_entity_dim']
        self.bbox_so_dim = config['bbox_so_dim']
        self.embd_dim = config['embd_dim']
        self.max_so_pair = config['max_so_pair']
        self.with_fuzzy = config.get('with_fuzzy', False)
        self.scale_range = config.get('scale_range', None)
        assert not self.with_fuzzy or self.scale_range is not None
        self.loss_types = config['loss_types']
        self.cost_factor = config["cost_coeff_dict"]
        self.loss_factor = config["loss_coeff_dict"]

        empty_weight = torch.ones(config["num_classes"] + 1)      # class 0 = "no relation"
        empty_weight[0] = self.loss_factor['eos_coef']
        self.register_buffer("empty_weight", empty_weight)

        self.backbone_arch = tuple(config['backbone_arch'])
        self.scale_factor = config['scale_factor']
        n_levels = self.backbone_arch[-1] + 1
        self.fpn_strides = [self.scale_factor ** i for i in range(config['fpn_start_level'], n_levels)]
        self.max_seq_len = config['max_seq_len']
        self.mha_win_size = [config['n_mha_win_size']] * n_levels
        # every level's length must split into local-attention chunks (reference maskvrd.py:57-63)
        self.max_div_factor = 1
        for s, w in zip(self.fpn_strides, self.mha_win_size):
            stride = s * (w // 2) * 2 if w > 1 else s
            assert self.max_seq_len % stride == 0, "max_seq_len must be divisible by fpn stride and window size"
            self.max_div_factor = max(self.max_div_factor, stride)
        self.use_abs_pe = config['use_abs_pe']
        self.use_rel_pe = config['use_rel_pe']

        self.with_clip_feature = config.get('with_clip_feature', False)
        common = dict(
            n_visual=self.visual_dim, n_bbox_entity=self.bbox_entity_dim, n_bbox_so=self.bbox_so_dim,
            n_embd=self.embd_dim, n_head=config['n_head'], n_embd_ks=config['embd_kernel_size'],
            fuse_ks=config['fuse_ks'], n_fuse_head=config['fuse_head'], fuse_path_drop=config['fuse_path_drop'],
            fuse_qx_stride=config['fuse_qx_stride'], fuse_kv_stride=config['fuse_kv_stride'],
            max_len=self.max_seq_len, arch=self.backbone_arch, mha_win_size=self.mha_win_size,
            scale_factor=self.scale_factor, with_ln=config['embd_with_ln'], attn_pdrop=config['dropattn'],
            proj_pdrop=config['dropout'], path_pdrop=config['droppath'], use_abs_pe=self.use_abs_pe,
            use_rel_pe=self.use_rel_pe, use_local=config['use_local'])
        if self.with_clip_feature:
            assert self.clip_dim is not None
            self.backbone = MaskConvTransformerBackboneWithCLIP(n_clip=self.clip_dim, **common)
        else:
            self.backbone = MaskConvTransformerBackbone(**common)
        if isinstance(self.embd_dim, (list, tuple)):
            self.embd_dim = sum(self.embd_dim)
        self.neck = FPN1D_Fuse(in_channels=[self.embd_dim] * n_levels, out_channel=config['fpn_dim'],
                               scale_factor=self.scale_factor, start_level=config['fpn_start_level'],
                               with_ln=config['fpn_with_ln'], norm_first=config['fpn_norm_first'])
        # one wave holds a pair's queries in the device matcher (vrd_assign_wave), 64 rows of mask embeddings pass the mask head
        # (vrd_mask_head): the reference has no cap, this code base's is 64
        n_queries = config['predictor']['num_queries']
        if not 1 <= int(n_queries) <= self.MAX_QUERIES:
            raise ValueError(f"predictor.num_queries must be 1..{self.MAX_QUERIES} (got {n_queries})")
        self.predictor = MaskedTransformerPredictor(**config['predictor'])
        self.deep_supervision = config['predictor']['deep_supervision']
        self.device = device
        # pairs per launch wave inside _mask_vrd: bounds the live intermediates (the 4x MLP hidden is
        # 2*chunk*T*2048 floats = 9.7 GB at 2048 pairs x 288 frames, of 288 GB).  Measured: 256 -> 1024 pairs +15 %,
        # 1024 -> 2048 +2.5 % (fewer launches of the small predictor / pyramid GEMMs, longer tile runs)
        self.pair_chunk = 2048
        self.share_tracklets = True     # forward_test from a PairSource: entity stage once per tracklet (eval_batches.SharedStreams)
        self.device_matching = True       # Hungarian assignment on the device (vrd_assign); False: scipy on the host
        self.device_criterion = True      # ... and the losses straight from its result, no trip to the host (_criterion_on_device)
        # `dropattn` / `dropout`: the backbone's TransformerBlocks drop by (step seed, site, element id) (vrdone_amd/dropout.py); a
        # site is named after its module in the reference's tree, which the checkpoint layout makes this tree's names too
        for name, mod in self.named_modules():
            if isinstance(mod, TransformerBlock):
                mod.set_dropout_names(name)
        self.dropout_rates = (float(config['dropattn']), float(config['dropout']))
        # None: every training step draws its 64-bit seed on the device from torch's generator; an integer pins it (tests, goldens:
        # the counterpart of AffineDropPath.keep)
        self.dropout_seed = None

    @torch.no_grad()
    def _config_eval(self, infer_config):
        assert self.training is False
        self.topk = infer_config['topk']
        self.n_max_pair = infer_config['n_max_pair']
        self.feat_stride = infer_config['feat_stride']
        self.pred_min_frames = infer_config['pred_min_frames']

    def forward(self, input_data):
        return self.forward_training(input_data) if self.training else self.forward_test(input_data)

    # ------------------------------------------------------------------------------------------
    # ---- tight padding --------------------------------------------------------------------------------------------------
    # The reference pads every pair of a batch to one length (max_seq_len, or the longest pair of the slice rounded up:
    # models/maskvrd.py:363-414) and computes every padded frame.  A pair's result does not depend on HOW MANY padded frames
    # follow it, only on there being one at every pyramid level (the frame behind the last valid one is what the depthwise
    # convs, the pools and the FPN read across the end: LayerNorm(0) = beta there, zero padding if the sequence simply
    # ends): with `down` = the coarsest level's stride, any padded length T' with T' / down > ceil(L / down) gives the
    # same outputs on the pair's frames (checked in float64 on the oracle: 1e-14; tests/test_oracle_golden.py).  Absolute
    # position rows (use_abs_pe) are no exception: frame t of a pair gets row t of the table of the REFERENCE's padded length
    # (re-interpolated from max_seq_len on), which is known per pair and travels with it (Layout.with_refs,
    # backbones.position_table) -- the length the pair is computed at does not enter.  So a
    # pair of L frames is computed at the smallest such multiple of TIGHT_UNIT below the batch's padded length, pairs of
    # equal T' as one batch; the outputs are laid out at the batch's padded length like the reference's.
    tight_padding = os.environ.get("VRDONE_TIGHT_PADDING", "1") != "0"
    TIGHT_UNIT = int(os.environ.get("VRDONE_TIGHT_UNIT", "32"))
    # a bucket of fewer rows (2 * pairs * T') joins the next longer one: below ~4 rounds of 256 x 256 GEMM tiles the small-shape
    # kernels take over and cost more than the padding saves (scripts/dev/tight_sweep.sh, profiles/r04_lab_tight_padding.txt:
    # ragged U[2, 256] batch of 2048 pairs 105.7 ms without, 106.8 / 100.7 ms with buckets of >= 131 k / 262 k rows)
    TIGHT_MIN_ROWS = int(os.environ.get("VRDONE_TIGHT_MIN_ROWS", "262144"))

    def tight_len(self, L, T):
        """The padded length a pair of L valid frames is computed at inside a batch padded to T frames."""
        down = self.scale_factor ** self.backbone_arch[-1]
        if not self.tight_padding or L >= T or T % down:
            return T
        need = down * (-(-L // down) + 1)
        unit = self.TIGHT_UNIT * down // math.gcd(self.TIGHT_UNIT, down)
        t = -(-need // unit) * unit
        return t if t < T else T

    def tight_buckets(self, lens, t_refs, min_rows=None):
        """Padded length per pair: tight_len of its reference length t_refs[i], then buckets of fewer than min_rows (TIGHT_MIN_ROWS) rows
        hand their pairs to the next longer bucket (a longer padding gives the same result; a handful of pairs per launch
        wave would run the small-shape kernels at a fraction of the large ones' rate) -- up to the pair's own reference length,
        never beyond.  Pairs that cannot shrink (no padded frame to spare: tight_len == their reference length) stay where the
        reference puts them."""
        if min_rows is None:
            min_rows = self.TIGHT_MIN_ROWS
        tight = [self.tight_len(L, T) for L, T in zip(lens, t_refs)]
        out = list(tight)
        flexible = {}
        rows = {}
        for i, (t, T) in enumerate(zip(tight, t_refs)):
            rows[t] = rows.get(t, 0) + 2 * t
            if t < T:
                flexible.setdefault(t, []).append(i)
        sizes = sorted(rows)
        for k, t in enumerate(sizes[:-1]):
            if rows[t] < min_rows and t in flexible:
                nxt = sizes[k + 1]
                moved = [i for i in flexible[t] if t_refs[i] >= nxt]        # (never beyond the reference's own padded length)
                flexible[t] = [i for i in flexible[t] if t_refs[i] < nxt]
                for i in moved:
                    out[i] = nxt
                rows[t] -= 2 * t * len(moved)
                rows[nxt] += 2 * nxt * len(moved)
                flexible.setdefault(nxt, []).extend(moved)
        return out

    # One row space for all buckets (models/ragged.py; the drivers: models/eval_batches.py): the row-by-row kernels -- LayerNorm,
    # every dense conv GEMM -- run once over all rows, so a bucket no longer has to fill the chip on its own and the buckets can be as fine as TIGHT_UNIT allows;
    # only the kernels that need (sequences, frames) structure walk the buckets.  ROWS_MIN_ROWS: below this a bucket's own
    # launches (depthwise convs, attention) are too small to be worth a launch each.
    row_space = os.environ.get("VRDONE_ROW_SPACE", "1") != "0"
    ROWS_MIN_ROWS = int(os.environ.get("VRDONE_ROWS_MIN_ROWS", "4096"))
    # forward_test takes the row-space form from this many pairs per video: below it the form's own host work (row-group tables,
    # the per-bucket walks of a finer bucket plan) costs more than its flat launches save -- 48 pairs 7.7 against 6.4 ms per call,
    # 226 pairs 12.2 / 11.9, 540 pairs 18.9 / 23.1 (profiles/r06_forward_test_small.json)
    ROWS_MIN_PAIRS = int(os.environ.get("VRDONE_ROWS_MIN_PAIRS", "256"))

    # Training in the row space (opt-in; VRDONE_TRAIN_ROWS=1): a step whose batch is ragged -- proposals.train_getitem keeps a
    # pair's own length -- computes every pair at its tight padded length, all lengths in one row space, forward and backward
    # (models/ragged.py under autograd), instead of padding every pair to max_seq_len.  _train_rows_step says which steps qualify;
    # the others take the batch form exactly as with the switch off.  `train_form` is the form the last training step took.
    train_rows = os.environ.get("VRDONE_TRAIN_ROWS", "0") == "1"
    # the bucket-merging threshold of the training plan (tight_buckets' min_rows; rows counted as 2 * pairs * T'): the value at which
    # the vidor step (48 pairs x 512 frames, lengths U[8, 512]) is fastest in the row space (scripts/train_rows_bench.py --sweep,
    # profiles/train_rows_bench.json: 0 -> 15 buckets, 4096 -> 7, 16384 -> 3; every further bucket costs the global attention and the
    # mask head a launch pair of its own)
    TRAIN_ROWS_MIN_ROWS = int(os.environ.get("VRDONE_TRAIN_ROWS_MIN_ROWS", "4096"))
    train_form = "batch"

    def train_rows_plan(self, lens, T=None):
        """The bucket plan of a training batch of pairs of `lens` valid frames padded to T (default max_seq_len) frames:
        [(T', [batch positions], flat)] -- tight_buckets under TRAIN_ROWS_MIN_ROWS, the buckets whose pairs all end in two padded
        frames (flat: the dense k = 3 convs run flat over them, models/ragged.py) first, each kind by length.  Host only."""
        T = self.max_seq_len if T is None else T
        want = {}
        for i, t2 in enumerate(self.tight_buckets(lens, [T] * len(lens), self.TRAIN_ROWS_MIN_ROWS)):
            want.setdefault((lens[i] <= t2 - 2, t2), []).append(i)
        return [(t2, want[(flat, t2)], flat) for flat, t2 in sorted(want, key=lambda k: (not k[0], k[1]))]

    def _train_rows_step(self, batched_masks):
        """The plan of a training step that takes the row space, or None (the batch form): the switch is set, both dropout rates
        are 0 (element ids count batch rows), no absolute position rows (training keeps the materialised ones), the batch is one
        launch wave, and the plan has at least two buckets or shrinks the one it has.  (The caller has made sure of the rest: a
        list-form batch, training graphs off.)"""
        known = getattr(batched_masks, "_vrd_lens", None)
        B, T = batched_masks.shape[0], batched_masks.shape[-1]
        if (not self.train_rows or any(self.dropout_rates) or self.use_abs_pe or known is None or known[0] != batched_masks._version
                or len(known[1]) != B or B > self._chunk_size(B)):
            return None
        plan = self.train_rows_plan(known[1], T)
        # (subject and object halves of a bucket are a row group each: one launch takes ragged._MAX_SEGS groups)
        if (len(plan) == 1 and plan[0][0] == T) or 2 * len(plan) > eval_batches.ragged._MAX_SEGS:
            return None
        return plan

    # forward_test / forward_test_videos build the winners' box tracks (`so_trajs`, ~100 k Python lists per video) only while
    # this is True.  A caller that scores on the device (evaluate.DeviceRelationScorer reads the tracklet boxes where they
    # are) sets it to False on its model: the key is then absent and every other key unchanged
    with_so_trajs = True

    def _eval_rows_form(self, n_pairs):
        return self.row_space and n_pairs >= self.ROWS_MIN_PAIRS

    def _tight_plan(self, batched_masks, masks2d):
        """{"buckets": [eval_batches.Bucket(T', pair indices (n,) int32 on the device, n, flat)], "rows": the buckets can share one
        row space} for a batch whose masks are prefixes (t < len), or None when the batch runs as it is (nothing to gain, masks with holes).
        One small device-to-host copy per mask tensor (cached on it)."""
        key = (batched_masks.data_ptr(), batched_masks._version, tuple(batched_masks.shape), self.row_space, self.TIGHT_MIN_ROWS,
               self.ROWS_MIN_ROWS)
        hit = getattr(batched_masks, "_vrd_tight_plan", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        B, T = masks2d.shape
        known = getattr(batched_masks, "_vrd_lens", None)       # the lengths the mask was built from (MaskVRD._batch): no read-back
        lens_h = known[1] if known is not None and known[0] == batched_masks._version and len(known[1]) == B else None
        if lens_h is None:
            lens = masks2d.sum(dim=1)
            last = T - torch.argmax(masks2d.flip(1).to(torch.uint8), dim=1)        # index behind the last valid frame
            host = torch.stack([lens, last]).cpu()
            lens_h = host[0].tolist() if bool((host[0] == host[1]).logical_or(host[0] == 0).all()) else None
        plan = None
        if lens_h is not None:
            rows = self.row_space
            want = {}
            for i, t2 in enumerate(self.tight_buckets(lens_h, [T] * B, self.ROWS_MIN_ROWS if rows else None)):
                # the row-space form runs the dense k = 3 convs flat over the buckets whose sequences all end in two padded
                # frames (models/ragged.py); a pair within one frame of its padded length goes into a bucket of its own kind
                want.setdefault((not rows or lens_h[i] <= t2 - 2, t2), []).append(i)
            if not all(t == T for _, t in want):           # (nothing shrinks: the batch runs as it is)
                dev = masks2d.device
                order = sorted(want, key=lambda k: (not k[0], k[1])) if rows else sorted(want, key=lambda k: k[1])
                # (one upload for all buckets' pair indices; a bucket's are a slice of it)
                every = torch.tensor([i for key in order for i in want[key]], dtype=torch.int32).to(dev)
                buckets, at = [], 0
                for flat, t2 in order:
                    n = len(want[(flat, t2)])
                    buckets.append(eval_batches.Bucket(t2, every[at:at + n], n, flat))
                    at += n
                plan = {"buckets": buckets, "rows": rows}
        batched_masks._vrd_tight_plan = (key, plan)
        return plan

    # buckets side by side: a bucket's launches are a fraction of the batch's, and from the third pyramid level on they no longer
    # fill the chip (a 256 x 256 GEMM tile per CU needs 65 k rows); buckets are independent, so they run on TIGHT_STREAMS HIP
    # streams and fill each other's tails.  (The first call runs them one after the other: it builds the per-weight operand
    # caches every later call only reads.)
    TIGHT_STREAMS = int(os.environ.get("VRDONE_TIGHT_STREAMS", "1"))

    def _tight_side_streams(self, dev):
        pool = self.__dict__.setdefault("_tight_stream_pool", {})
        key = (str(dev), _ops().get_precision())
        if key not in pool:
            pool[key] = None if self.TIGHT_STREAMS <= 1 else []          # first call in this mode: sequential, caches get built
            return None
        if pool[key] is not None and not pool[key]:
            pool[key] = [torch.cuda.Stream(device=dev) for _ in range(self.TIGHT_STREAMS - 1)]
        return pool[key]

    def _mask_vrd_tight(self, x, masks2d, plan, with_aux, t_ref=None):
        """_mask_vrd bucket by bucket (see `tight padding` above); outputs in the batch's own padded length.
        t_ref: the reference's padded length of the pairs (default: the batch's)."""
        B, T = masks2d.shape
        dev = x.device
        out = None
        t_ref = T if t_ref is None else t_ref
        main = torch.cuda.current_stream(dev)
        plan = plan["buckets"]
        side = self._tight_side_streams(dev) if len(plan) > 1 and not torch.cuda.is_current_stream_capturing() else None
        lanes = [main] + list(side or [])
        fork = None
        for k, (t2, idx, n, _) in enumerate(plan):
            lane = lanes[k % len(lanes)] if out is not None else main           # (the first bucket also shapes the outputs)
            if lane is not main:
                lane.wait_event(fork)
            with torch.cuda.stream(lane):
                idx64 = idx.long()
                m_all = masks2d[idx64, :t2].contiguous()
                step = self._chunk_size(n)
                for c0 in range(0, n, step):
                    sel, sel64 = idx[c0:c0 + step].contiguous(), idx64[c0:c0 + step]
                    m = m_all[c0:c0 + step]
                    o = self._heads(*self.backbone.cl_parts(*self.backbone._unpack(x, frames=t2, index=sel), m, t_ref), with_aux)
                    if out is None:
                        out = eval_batches.new_outputs(B, T, *o["pred_logits"].shape[1:], len(o.get("aux_outputs", ())), dev)
                        if len(lanes) > 1:
                            fork = torch.cuda.Event()
                            fork.record(main)            # the output buffers (and everything before this call) exist from here on
                    for dst, src in [(out, o)] + list(zip(out.get("aux_outputs", []), o.get("aux_outputs", []))):
                        eval_batches.scatter_heads(dst, sel64, t2, src["pred_logits"], src["pred_masks"])
        for lane in lanes[1:]:
            main.wait_stream(lane)
        out["output_mask"] = masks2d[:, None, :]
        return out

    def _mask_vrd(self, batched_inputs, batched_masks, with_aux=None, t_ref=None, train_plan=None):
        """(B, C_in, T) fp32, (B, 1, T) bool -> dict(pred_logits (B,Q,K+1), pred_masks (B,Q,T),
        [aux_outputs], output_mask (B,1,T)); backbone -> neck -> predictor like the reference.
        t_ref: the length the reference pads these pairs to when that is not T (a batch that a caller padded tighter, eval only);
        absolute position rows follow it.
        train_plan: the plan of a training step in the row space (_train_rows_step; autograd recording)."""
        if not batched_inputs.is_cuda:
            raise RuntimeError("MaskVRD._mask_vrd runs on the HIP device only; move the model and inputs to 'cuda'")
        B = batched_inputs.shape[0]
        masks2d = batched_masks.reshape(B, batched_masks.shape[-1]).contiguous()
        if self.tight_padding and not torch.is_grad_enabled() and batched_masks.dtype == torch.bool and batched_inputs.is_contiguous():
            plan = self._tight_plan(batched_masks, masks2d)
            if plan is not None:
                if plan["rows"]:
                    return eval_batches.mask_vrd_rows(self, batched_inputs, masks2d, plan["buckets"], with_aux, t_ref)
                return self._mask_vrd_tight(batched_inputs, masks2d, plan, with_aux, t_ref)
        if self.training and torch.is_grad_enabled():
            self._begin_training_pass(batched_inputs.device)
        if train_plan is not None:
            assert self.training and torch.is_grad_enabled() and batched_inputs.is_contiguous()
            order = [i for _, ids, _ in train_plan for i in ids]
            every = torch.tensor(order, dtype=torch.int32).to(masks2d.device)          # (one upload for all buckets' pair indices)
            buckets, at = [], 0
            for t2, ids, flat in train_plan:
                buckets.append(eval_batches.Bucket(t2, every[at:at + len(ids)], len(ids), flat))
                at += len(ids)
            return eval_batches.mask_vrd_rows(self, batched_inputs, masks2d, buckets, with_aux, order=order)
        outs = []
        step = self._chunk_size(B)
        for b0 in range(0, B, step):
            x = batched_inputs[b0:b0 + step]
            m = masks2d[b0:b0 + step]
            outs.append(self._heads(*self.backbone.cl(x, m, t_ref), with_aux))
        return self._merge(outs)

    def _begin_training_pass(self, device):
        """What a differentiable pass over the network starts with, inside a recording when training graphs are on: the derived
        weight operands and, for a model that drops, the step's seed and the restart of its modules' sample counters."""
        # the split-precision operands of all dense conv weights (forward and input-gradient form) in one launch instead of one
        # per weight and form (they are rebuilt after every optimiser update)
        _ops().presplit_weights(self._dense_conv_weights(), self.__dict__.setdefault("_split_plans", {}))
        if any(self.dropout_rates):
            begin_dropout_step(self, device, self.dropout_seed)

    def _mask_vrd_parts(self, vis, clip, so_box, ent, masks2d, with_aux=None):
        """`_mask_vrd` from the backbone's operand buffers (ops.gather_train) instead of the (B, C_in, T) boundary tensor:
        what `_mask_vrd` runs behind `backbone._unpack`, in one launch wave."""
        B = masks2d.shape[0]
        if B > self._chunk_size(B):
            raise ValueError(f"a device-built training batch runs as one launch wave: {B} sequences exceed pair_chunk = {self.pair_chunk}")
        if self.training and torch.is_grad_enabled():
            self._begin_training_pass(masks2d.device)
        return self._heads(*self.backbone.cl_parts(vis, clip, so_box, ent, masks2d), with_aux)

    def __deepcopy__(self, memo):
        """copy.deepcopy(model) (ModelEma does it, utils/train_utils.py:13): the derived-operand caches stay behind -- their
        job tables point at THIS model's buffers, and the copy builds its own on first use."""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("_split_plans", "_dense_convs"):
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def _dense_conv_weights(self):
        """The Conv1d weights that reach vrd_gemm (groups == 1), in module order; looked up on every call: training graphs swap
        the modules' parameters for aliases of the same storage while they record."""
        convs = self.__dict__.get("_dense_convs")
        if convs is None:
            convs = self.__dict__["_dense_convs"] = [mod for mod in self.modules() if isinstance(mod, nn.Conv1d) and mod.groups == 1]
        return [mod.weight for mod in convs if mod.weight.is_contiguous()]

    def _chunk_size(self, n):
        """Pairs per launch wave: one wave up to 1.25 x pair_chunk, otherwise equal waves (a 2070-pair video is one wave,
        not 2048 + 22: a 22-pair wave runs the small-shape kernels at a fraction of the large ones' rate)."""
        if n <= self.pair_chunk + self.pair_chunk // 4:
            return max(n, 1)
        waves = -(-n // self.pair_chunk)
        return -(-n // waves)

    def _heads(self, feats, masks, with_aux, lay=None):
        """neck + predictor.  lay: the layout of the full-resolution rows; without one the batch form and the reference's dict,
        with one the predictor's per-bucket heads (predictor.py `heads`: buckets differ in length)."""
        lays = lay and [lay.strided(self.scale_factor ** l) for l in range(len(feats))]
        fpn_feat, _ = self.neck.cl(feats, masks, lays)
        if lay is None:
            return self.predictor.cl(feats[-1], fpn_feat, masks[-1], masks[0], with_aux=with_aux)
        return self.predictor.heads(feats[-1], fpn_feat, masks[-1], masks[0], with_aux, klay=lays[-1], lay0=lay)

    @staticmethod
    def _merge(outs):
        if len(outs) == 1:
            return outs[0]
        merged = {k: torch.cat([o[k] for o in outs], dim=0) for k in ("pred_logits", "pred_masks", "output_mask")}
        if "aux_outputs" in outs[0]:
            merged["aux_outputs"] = [{k: torch.cat([o["aux_outputs"][i][k] for o in outs], dim=0)
                                      for k in ("pred_logits", "pred_masks")}
                                     for i in range(len(outs[0]["aux_outputs"]))]
        return merged

    def forward_training(self, input_data):
        """Loss dict of reference maskvrd.py:169-199: batching, network, Hungarian matching and the class / focal /
        dice losses (+ one set per auxiliary decoder layer), ending in 'total_loss'.
        input_data: the dataloader's lists (so_features_list, preds_list, masks_list, segs_list: proposals.train_getitem) or
        {'train_source': proposals.TrainSource, 'train_tables': proposals.TrainTables}: the batch is then gathered on the device.
        With autograd recording (a training step, train.py:182-186) the network runs the differentiable HIP ops of
        vrdone_amd/autograd.py, AffineDropPath samples per-sample keep factors, and total_loss.backward() reaches
        every parameter.  Under torch.no_grad() it is the validation loss on the fused inference kernels."""
        ops = _ops()
        # f16x3 mode: an activation beyond the f16 operand range (+-4094) is reported by the kernel that met it in a flag word
        # on the device (ops.f16_range_flag; a NaN would not reach the loss reliably).  The word is read once, behind the
        # step's own launches, and such a step is taken again in the f32 mode -- the arithmetic of the reference (train.py:182-186).
        pdev = next(self.parameters()).device
        if torch.is_grad_enabled():
            ops.check_differentiable("MaskVRD.forward_training")
        if ops.get_deterministic():
            # (the stochastic-depth factors of this call are drawn in this call: the same seed gives the same step)
            _factor_pool.reset()
        guard = ops.f16_planes() and pdev.type == "cuda" and os.environ.get("VRDONE_RANGE_GUARD", "1") != "0"
        if guard:
            flag = ops.f16_range_flag(pdev)
            flag.zero_()
        graphs = torch.is_grad_enabled() and self.training and train_graph.enabled(self)
        if torch.is_grad_enabled() and self.training:
            self.train_form = "batch"            # (until the step turns out to take the row space)
        if 'train_source' in input_data:
            # a batch built on the device (proposals.TrainSource / train_tables): one gather launch writes the operand buffers of
            # the backbone's first stage and the target masks -- no (B, C_in, T) tensor, no vrd_bct_to_btc
            source, tables = input_data['train_source'], input_data['train_tables']
            if graphs:
                predictions, targets = train_graph.mask_vrd_source(self, source, tables)
            else:
                bb = self.backbone
                *parts, m2, targets = ops.gather_train(source, tables, self.max_seq_len, bb.n_bbox_so, bb.n_bbox_entity, ops.pair_mode())
                predictions = self._mask_vrd_parts(*parts, m2, with_aux=self.deep_supervision)
            d, sizes = tables.on_device(source), tables.sizes
            ground_truth = {'preds_list': d["preds"].split(sizes), 'masks_list': targets.split(sizes), 'segs_list': d["segs"].split(sizes)}
        else:
            ground_truth = input_data
            x, m = self._train_batch(input_data['so_features_list'])
            if graphs:
                predictions = train_graph.mask_vrd(self, x, m)        # two HIP-graph replays instead of ~2,000 launches
            else:
                plan = self._train_rows_step(m) if self.training and torch.is_grad_enabled() else None
                if plan is not None:
                    self.train_form = "rows"
                predictions = self._mask_vrd(x, m, with_aux=self.deep_supervision, train_plan=plan)
        losses = self.criterion(predictions, ground_truth)
        if guard:
            # (one 4-byte read behind the step's launches: a host synchronisation, like the loss.item() of the reference's loop,
            # train.py:188-191.  Under torch.distributed every rank must take the same branch -- a rank that repeated its step
            # alone would leave its peers waiting in the gradient all-reduce while it records a new f32 graph --, so the flag is
            # reduced over the default group first: MAX keeps "some rank saw it")
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                seen = (flag != 0).to(torch.int32)
                torch.distributed.all_reduce(seen, op=torch.distributed.ReduceOp.MAX)
                bits = int(flag.item()) or (64 if int(seen.item()) else 0)        # (64: "other" -- a peer's producer)
            else:
                bits = int(flag.item())
            if bits:
                import warnings
                flag.zero_()
                warnings.warn(f"vrdone_amd: an activation beyond the {ops.get_precision()} mode's operand range (" + ops.describe_range(bits) +
                              "): taking this step in the f32 mode")
                del losses, predictions
                with ops.use_precision("f32"):
                    return self.forward_training(input_data)
        return losses

    def enable_training_graphs(self, enable=True):
        """Training steps replay the network's forward and backward as HIP graphs, recorded once per batch shape
        (vrdone_amd/train_graph.py: what is recorded, and the limits -- one backward per forward; gradients are cleared with
        zero_grad(set_to_none=True) between steps, a kept .grad is added to through a copy.  Works under DDP: the graphs are
        recorded on aliases of the parameters, the reducer's hooks fire outside them)."""
        train_graph.enable(self, enable)
        return self

    @torch.no_grad()
    def forward_loss(self, input_data):
        return self.forward_training(input_data)

    def criterion(self, predictions, input_data):
        """predictions of _mask_vrd (with aux_outputs when deep_supervision) + the dataloader's ground truth
        (preds_list (N_i,) int64, masks_list (N_i, T) 0/1 float, segs_list (N_i, 2) int64) -> loss dict.  The matching
        runs without autograd (like the reference's @torch.no_grad() matcher, maskvrd.py:417); the losses are plain
        differentiable tensor code."""
        dev = predictions['pred_logits'].device
        gt_preds = [t.to(dev) for t in input_data['preds_list']]
        gt_masks = [t.to(dev) for t in input_data['masks_list']]
        gt_segs = input_data.get('segs_list', None)
        if self.with_fuzzy:
            assert gt_segs is not None
        if gt_segs is not None:
            gt_segs = [t.to(dev) for t in gt_segs]
        pred_logits, pred_masks, out_mask = predictions['pred_logits'], predictions['pred_masks'], predictions['output_mask']
        aux = predictions['aux_outputs'] if self.deep_supervision else None
        sizes = [len(p) for p in gt_preds]
        Q = pred_logits.shape[1]
        # the fused criterion keeps one int per (pair, query) row in its workgroup's 48 KiB of LDS (vrd_criterion_losses): batches
        # beyond ~12 k rows take the tensor form below, like anything else it does not cover
        fits = pred_logits.shape[0] * Q * 4 + 256 <= 48 * 1024
        if (self.device_matching and self.device_criterion and pred_logits.is_cuda and sizes and 0 < max(sizes) <= Q <= 64 and fits
                and 'bipartite_match' not in self.__dict__):          # (tests pin the matching by replacing the method)
            loss_dict = self._criterion_on_device(pred_logits, pred_masks, out_mask, aux, sizes, gt_preds, gt_masks, gt_segs)
        else:
            indices, loss_mask = self.bipartite_match(pred_logits, gt_preds, pred_masks, gt_masks, gt_segs, _mask=out_mask)
            loss_dict = self.loss(indices, pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, _mask=out_mask,
                                  loss_mask=loss_mask, aux_outputs=aux)
        loss_dict['total_loss'] = torch.stack(list(loss_dict.values())).sum()
        return loss_dict

    def _criterion_on_device(self, pred_logits, pred_masks, out_mask, aux_outputs, sizes, gt_preds, gt_masks, gt_segs):
        """The loss dict of `bipartite_match` + `loss` without a trip to the host: the device assignment (vrd_assign) gives
        the query of every relation, which is all the losses need -- target[pair of g, query of g] = class of g, and the
        matched mask rows in relation order (the reference gathers them pair by pair in query order, maskvrd.py:500-527:
        the same rows, so the same sums up to their order).  The host never waits for the predictions, so the eager loss
        launches queue up behind the network instead of starting when it has finished; the relation tables (owner,
        offsets) are built once for the final head and the auxiliary layers."""
        dev = pred_logits.device
        ops = _ops()
        G = sum(sizes)
        ids, tgt_masks = torch.cat(gt_preds, dim=0), torch.cat(gt_masks, dim=0)
        valid = out_mask[:, 0]
        assert tgt_masks.shape == (G, valid.shape[-1])
        segs, scale_range = self._fuzzy(gt_segs)
        names = {"labels": ["loss_class"], "masks": ["loss_mask", "loss_dice"]}
        keys = [k for name in self.loss_types for k in names[name]]          # the reference's order of terms
        layers = [(pred_logits, pred_masks)] + [(aux['pred_logits'], aux['pred_masks']) for aux in (aux_outputs or [])]
        if len(layers) <= 4:
            # four launches for all layers: costs, assignment, losses (+ one for their gradients) -- csrc/vrd_criterion.hip
            vals, _, failed = losses.device_criterion(layers, valid, sizes, ids, tgt_masks, segs, scale_range, self.empty_weight,
                                                      (self.cost_factor['cost_class'], self.cost_factor['cost_mask'],
                                                       self.cost_factor['cost_dice']))
            # a pair whose costs are NaN / infinite comes back unassigned.  The reference's scipy call raises there; this path
            # never waits for the device, so it poisons the losses instead (they are NaN anyway: same logits)
            vals = vals + torch.where(failed, torch.full((), float("nan"), device=dev), torch.zeros((), device=dev))
            factor = {"loss_class": self.loss_factor['loss_class'], "loss_mask": self.loss_factor['loss_mask'],
                      "loss_dice": self.loss_factor['loss_dice']}
            col = {"loss_class": 0, "loss_mask": 1, "loss_dice": 2}
            out = {k: factor[k] * vals[0, col[k]] for k in keys}
            for i in range(len(layers) - 1):
                out.update({f"{k}_{i}": factor[k] * vals[i + 1, col[k]] for k in keys})
            return out
        owner = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev), output_size=G)
        tables = ops.assign_tables(sizes, dev)
        loss_mask = valid[owner]
        num_masks = float(max(G, 1))
        weight = self.empty_weight.to(dev)

        def layer(logits, masks):
            with torch.no_grad():
                c_class, c_mask, c_dice = losses.pair_costs(logits, masks, valid, ids, tgt_masks, owner, segs, scale_range)
                cost = (self.cost_factor['cost_class'] * c_class + self.cost_factor['cost_mask'] * c_mask +
                        self.cost_factor['cost_dice'] * c_dice)
                q_of = ops.assign(cost.contiguous(), sizes, tables).long()
                failed = (q_of < 0).any()
                q_of = q_of.clamp_min(0)
            poison = torch.where(failed, torch.full((), float("nan"), device=dev), torch.zeros((), device=dev))
            terms = {}
            if "labels" in self.loss_types:
                target = torch.zeros(logits.shape[:2], dtype=torch.int64, device=dev)
                target[owner, q_of] = ids
                terms["loss_class"] = self.loss_factor['loss_class'] * F.cross_entropy(logits.transpose(1, 2), target, weight) + poison
            if "masks" in self.loss_types:
                focal, dice = losses.matched_losses(masks[owner, q_of], tgt_masks, num_masks, loss_mask, segs, scale_range)
                terms["loss_mask"] = self.loss_factor['loss_mask'] * focal + poison
                terms["loss_dice"] = self.loss_factor['loss_dice'] * dice + poison
            return terms
        terms = layer(pred_logits, pred_masks)
        out = {k: terms[k] for k in keys}
        for i, aux in enumerate(aux_outputs or []):
            terms = layer(aux['pred_logits'], aux['pred_masks'])
            out.update({f"{k}_{i}": terms[k] for k in keys})
        return out

    # ---- matching and losses (reference maskvrd.py:417-588) ----
    def _fuzzy(self, gt_segs):
        return (torch.cat(gt_segs, dim=0), self.scale_range) if self.with_fuzzy else (None, None)

    @torch.no_grad()
    def bipartite_match(self, pred_logits, gt_preds, pred_masks, gt_masks, gt_segs, _mask):
        """Hungarian assignment of each pair's relations to its queries on
        cost_class * CE + cost_mask * focal + cost_dice * dice (reference maskvrd.py:417-496).
        Returns [(query_idx, relation_idx)] per pair (int64, CPU) and loss_mask (sum N_i, T) bool.
        Only each pair's own (Q, N_i) block is priced (losses.pair_costs); the block goes to the host once."""
        from scipy.optimize import linear_sum_assignment
        dev = pred_logits.device
        sizes = [len(p) for p in gt_preds]
        owner = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
        valid = _mask[:, 0]
        tgt_masks = torch.cat(gt_masks, dim=0)
        assert tgt_masks.shape == (sum(sizes), valid.shape[-1])
        segs, scale_range = self._fuzzy(gt_segs)
        c_class, c_mask, c_dice = losses.pair_costs(pred_logits, pred_masks, valid, torch.cat(gt_preds, dim=0),
                                                    tgt_masks, owner, segs, scale_range)
        cost = (self.cost_factor['cost_class'] * c_class + self.cost_factor['cost_mask'] * c_mask +
                self.cost_factor['cost_dice'] * c_dice)                             # (sum N_i, Q)
        Q = cost.shape[1]
        indices = []
        if cost.is_cuda and sizes and 0 < max(sizes) <= Q <= 64 and self.device_matching:
            # every pair's assignment on the device (vrd_assign); one small copy brings the result back in the reference's
            # format: per pair (query indices ascending, the relation each one got)
            q_of = _ops().assign(cost.contiguous(), sizes).cpu().long()
            if bool((q_of < 0).any()):          # NaN / infinite costs: scipy's linear_sum_assignment raises the same way
                raise ValueError("matrix contains invalid numeric entries")
            for block in q_of.split(sizes):
                rows, order = torch.sort(block)
                indices.append((rows, order))
        else:
            for block in cost.cpu().split(sizes, dim=0):
                rows, cols = linear_sum_assignment(block.T.numpy())
                indices.append((torch.as_tensor(rows, dtype=torch.int64), torch.as_tensor(cols, dtype=torch.int64)))
        return indices, valid[owner]

    def _get_src_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        return batch_idx, torch.cat([src for src, _ in indices])

    @staticmethod
    def _matched_targets(per_pair, indices, dev):
        """cat([t[j] for t, (_, j) in zip(per_pair, indices)]) -- the reference's gather of every pair's matched relations
        (maskvrd.py:500-503,520-527) -- with ONE index upload: the per-pair lists are concatenated and indexed with the
        matcher's columns shifted by each pair's offset (one small host-to-device copy per pair was ~300 per step)."""
        sizes = [int(t.shape[0]) for t in per_pair]
        offs = [0]
        for n in sizes[:-1]:
            offs.append(offs[-1] + n)
        j_all = torch.cat([j + o for (_, j), o in zip(indices, offs)]).to(dev)
        return torch.cat(list(per_pair), dim=0)[j_all]

    def _get_tgt_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        return batch_idx, torch.cat([tgt for _, tgt in indices])

    def loss_labels(self, pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, indices, num_masks, loss_mask):
        """eos-weighted cross-entropy over all (pair, query): matched queries carry their relation's predicate,
        the rest class 0 (reference maskvrd.py:498-513)."""
        dev = pred_logits.device
        b, q = (t.to(dev) for t in self._get_src_permutation_idx(indices))
        target = torch.zeros(pred_logits.shape[:2], dtype=torch.int64, device=dev)
        target[b, q] = self._matched_targets(gt_preds, indices, dev)
        ce = F.cross_entropy(pred_logits.transpose(1, 2), target, self.empty_weight.to(dev))
        return {"loss_class": self.loss_factor['loss_class'] * ce}

    def loss_masks(self, pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, indices, num_masks, loss_mask):
        """focal + dice loss between each matched query's mask and its relation's (fuzzy) mask over the pair's
        valid frames (reference maskvrd.py:515-551)."""
        dev = pred_masks.device
        b, q = (t.to(dev) for t in self._get_src_permutation_idx(indices))
        target = self._matched_targets(gt_masks, indices, dev)
        picked = pred_masks[b, q]
        assert picked.shape == target.shape
        segs = self._matched_targets(gt_segs, indices, dev) if self.with_fuzzy else None
        focal, dice = losses.matched_losses(picked, target, num_masks, loss_mask, segs,
                                            self.scale_range if self.with_fuzzy else None)
        return {"loss_mask": self.loss_factor['loss_mask'] * focal, "loss_dice": self.loss_factor['loss_dice'] * dice}

    def get_loss(self, loss, pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, indices, num_masks, loss_mask):
        loss_map = {"labels": self.loss_labels, "masks": self.loss_masks}
        assert loss in loss_map, f"do you really want to compute {loss} loss?"
        return loss_map[loss](pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, indices, num_masks, loss_mask)

    def loss(self, indices, pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, _mask, loss_mask, aux_outputs=None):
        """All loss terms for the final predictions, and `<name>_<i>` for auxiliary layer i with its own matching
        (reference maskvrd.py:570-588).  num_masks = total number of relations, at least 1."""
        num_masks = float(max(sum(len(gt) for gt in gt_preds), 1))
        out = {}
        for name in self.loss_types:
            out.update(self.get_loss(name, pred_logits, pred_masks, gt_preds, gt_masks, gt_segs, indices, num_masks,
                                     loss_mask))
        for i, aux in enumerate(aux_outputs or []):
            a_logits, a_masks = aux['pred_logits'], aux['pred_masks']
            a_idx, a_lm = self.bipartite_match(a_logits, gt_preds, a_masks, gt_masks, gt_segs, _mask=_mask)
            for name in self.loss_types:
                terms = self.get_loss(name, a_logits, a_masks, gt_preds, gt_masks, gt_segs, a_idx, num_masks, a_lm)
                out.update({f"{k}_{i}": v for k, v in terms.items()})
        return out

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def preprocessing(self, feats_list, padding_val=0.0):
        """Eval batching of reference maskvrd.py:363-414: pairs no longer than max_seq_len are
        zero-padded to max_seq_len, longer ones to the longest rounded up to max_div_factor."""
        assert padding_val == 0.0
        if self.training:
            return self._train_batch(feats_list)
        dev = self.device
        lens = [int(f.shape[1]) for f in feats_list]
        ids = ([i for i, n in enumerate(lens) if n <= self.max_seq_len],
               [i for i, n in enumerate(lens) if n > self.max_seq_len])
        d = self.max_div_factor
        t_pad = (self.max_seq_len, (max(lens + [self.max_seq_len]) + d - 1) // d * d)
        inputs, masks = [], []
        for part_ids, T in zip(ids, t_pad):
            x, m = self._batch(feats_list, part_ids, T) if part_ids else (None, None)
            inputs.append(x)
            masks.append(m)
        return tuple(inputs), tuple(masks), ids

    def _train_batch(self, feats_list):
        """Training batching (reference maskvrd.py:338-360): every pair zero-padded to max_seq_len."""
        assert max(int(f.shape[1]) for f in feats_list) <= self.max_seq_len, \
            "Input length must be smaller than max_seq_len during training"
        return self._batch(feats_list, range(len(feats_list)), self.max_seq_len)

    def _batch(self, feats_list, ids, T):
        """Zero-padded (len(ids), C_in, T) batch and its (len(ids), 1, T) validity mask on the device."""
        dev = self.device
        x = torch.zeros(len(ids), feats_list[0].shape[0], T, device=dev, dtype=torch.float32)
        for r, i in enumerate(ids):
            x[r, :, :feats_list[i].shape[1]].copy_(feats_list[i], non_blocking=True)
        lens = [int(feats_list[i].shape[1]) for i in ids]
        n = torch.tensor(lens, device=dev)
        m = (torch.arange(T, device=dev)[None, :] < n[:, None])[:, None, :]
        m._vrd_lens = (m._version, lens)              # (what _tight_plan would otherwise read back from the device)
        return x, m

    def shard_pairs(self, group=None, enable=True):
        """Pair-sharded evaluation: with torch.distributed initialised, every rank of `group` calls
        forward_test with the SAME video, runs the network on its share of the pairs, and the ranks exchange compact
        per-pair candidates (vrdone_amd.parallel.gather_candidates) in front of the global top-n_max_pair selection;
        every rank returns the same result.  Off by default (each process evaluates its own videos, like eval.py)."""
        self._shard = (group,) if enable else None
        return self

    def eval_plan(self, lens):
        """Batching plan of one video's pairs.  The reference walks the pairs in slices of max_so_pair and pads the long
        pairs of a slice to that slice's longest (maskvrd.py:208-227, :373-379).  A pair's result depends only on its
        own padded length, so each pair gets the padded length its slice gives it, and pairs are ordered by (padded
        length, valid length, index): every padded length then is ONE batch (short pairs of all slices share
        max_seq_len), and dealing that order round-robin gives every rank of a sharded run the same mix of lengths.
        Returns (order: list of pair ids, t_pad: padded length per pair id)."""
        # (the reference's padded length of every pair; then the shortest ones that give the same results: `tight padding`)
        return eval_batches.pair_order(self, lens, self._reference_pad(lens))

    def _reference_pad(self, lens):
        """The padded length the reference gives each pair of one video: max_seq_len, or its max_so_pair slice's longest rounded up."""
        P, d = len(lens), self.max_div_factor
        t_pad = [0] * P
        for s0 in range(0, P, self.max_so_pair):
            sl = range(s0, min(s0 + self.max_so_pair, P))
            t_long = (max([lens[i] for i in sl] + [self.max_seq_len]) + d - 1) // d * d
            for i in sl:
                t_pad[i] = self.max_seq_len if lens[i] <= self.max_seq_len else t_long
        return t_pad

    def _entity_streams(self, source, ids):
        return eval_batches.SharedStreams.streams(self, source, ids)

    def _shared_entity_rows(self, source, sel, shared, at, T, pieces=None):
        return eval_batches.SharedStreams(self, source, None, shared).entity_rows(sel, at, T, pieces)

    def pair_candidates(self, feats, lens, ids, t_pad, k, source=None, t_refs=None):
        """Network + per-(pair, query) post-processing kernel for the pairs `ids` (already grouped by padded length), bucket by
        bucket or, from _eval_rows_form's size on, all padded lengths of a launch wave in one row space (models/eval_batches.py).
        source: a proposals.PairSource -- pair rows are then gathered on the device from the per-tracklet features
        (vrd_gather_pairs) and `feats` is not used; with its tracklet table the entity stage of the backbone runs once
        per tracklet instead of twice per pair (eval_batches.SharedStreams).
        t_refs: the reference's padded length per pair id (default: _reference_pad(lens), one video's); absolute position rows follow it.
        Returns ONE float32 tensor (len(ids), Q, 2k + 2) = [top-k scores | top-k class ids | first | last frame], the
        three integer fields bit-cast: the compact candidate record that sharded runs exchange (SURVEY 8e option i)."""
        return eval_batches.pair_candidates(self, feats, lens, ids, t_pad, k, source, t_refs)

    @torch.no_grad()
    def forward_test(self, input_data):
        """Same inputs / outputs as reference maskvrd.py:201-337.  Per (pair, query) the softmax,
        class top-k and mask -> [start, end] run in one HIP kernel; the candidate filter and the
        global top-n_max_pair selection are batched tensor ops; only the <= n_max_pair winners
        are brought to the host.  After shard_pairs() the pairs are split over the ranks of the process group."""
        from .. import parallel
        dev = self.device
        source = input_data.get('pair_source')          # proposals.prepare_test_proposal: per-tracklet features on the device
        if source is None and 'tracklet_visual' in input_data:     # ... or its plain-tensor form (PairSource.fields)
            from ..proposals import PairSource
            source = PairSource.from_fields(input_data, dev)
        feats = None if source is not None else input_data['so_features_list']
        P = len(input_data['sids'])
        Q, k = self.predictor.num_queries, self.topk
        lens = list(source.lens) if source is not None else [int(f.shape[1]) for f in feats]
        assert len(lens) == P
        order, t_pad = self.eval_plan(lens)
        t_refs = self._reference_pad(lens)              # (the lengths eval_plan shortened: absolute position rows follow them)
        shard = getattr(self, "_shard", None)
        rank, world = parallel.rank_world(shard[0]) if shard else (0, 1)
        mine = order[rank::world]                      # round-robin over the length-sorted order
        unsort = torch.empty(P, dtype=torch.int64)
        unsort[torch.tensor(order, dtype=torch.int64)] = torch.arange(P)
        unsort = unsort.to(dev)                         # uploaded before the first kernel is queued
        ops = _ops()
        f16 = ops.f16_planes()
        if f16:
            flag = ops.f16_range_flag(next(self.parameters()).device)
            flag.zero_()
        cand = self.pair_candidates(feats, lens, mine, t_pad, k, source=source, t_refs=t_refs)
        if f16:
            # an activation beyond the f16 operand range is reported in the device's flag word (a NaN would not reach the
            # scores reliably: the ReLUs and max-pools on the way drop it).  Without leaving the stream the flag poisons this
            # rank's scores, so that the finite-scores test below -- after the exchange, identical on every rank -- sees it
            cand[:, :, :k] += torch.where(flag > 0, float("nan"), 0.0).to(cand.dtype)
        if world > 1 or (shard and parallel.forced()):
            cand = parallel.gather_candidates(cand, P, shard[0])       # (P, Q, 2k + 2) in `order`
        if f16 and not bool(torch.isfinite(cand[:, :, :k]).all()):
            # the f16x3 mode's operand planes hold |x| < 4094 (vrd_common.h).  The reference computes such a video in float32:
            # so does the repeat.  (After the exchange: every rank of a sharded run sees the same candidates and takes the
            # same branch.)
            import warnings
            warnings.warn(f"vrdone_amd: an activation beyond the {ops.get_precision()} mode's operand range (or non-finite inputs): repeating "
                          "this video in the f32 mode")
            with ops.use_precision("f32"):
                return self.forward_test(input_data)
        cand = cand[unsort]                             # back to the dataloader's pair order
        ints = cand.view(torch.int32)
        top_score = cand[:, :, :k].contiguous()
        top_cat = ints[:, :, k:2 * k].contiguous()
        first, last = ints[:, :, 2 * k].contiguous(), ints[:, :, 2 * k + 1].contiguous()

        to = lambda t: torch.as_tensor(t).to(dev)     # noqa: E731
        sids, oids = to(input_data['sids']).long(), to(input_data['oids']).long()
        durs = to(input_data['traj_durations']).long()
        cat_ids, cat_scores = to(input_data['cat_ids']).long(), to(input_data['cat_scores']).float()
        offs = to(input_data['so_offset']).long()
        so_start = torch.maximum(durs[sids, 0], durs[oids, 0])
        so_end = torch.minimum(durs[sids, 1], durs[oids, 1])
        start = first.long() * self.feat_stride + offs[:, None]                      # (P, Q)
        end = last.long() * self.feat_stride + offs[:, None] + 1
        keep = (last >= 0) & ((end - start) >= self.pred_min_frames)
        assert bool(((start >= 0) & (end <= (so_end - so_start)[:, None]))[keep].all())
        keep = keep[:, :, None].expand(P, Q, k).reshape(-1)
        if not bool(keep.any()):
            return None
        p_score = top_score.reshape(-1)
        pair_of = torch.arange(P, device=dev).repeat_interleave(Q * k)
        query_of = torch.arange(Q, device=dev).repeat_interleave(k).repeat(P)
        tri = torch.stack([cat_scores[sids[pair_of]], p_score, cat_scores[oids[pair_of]]], dim=1)
        avg = tri.mean(dim=-1)
        cand = torch.nonzero(keep).flatten()             # reference candidate order: pair, query, class rank
        order = cand[torch.argsort(avg[cand], descending=True, stable=True)[:self.n_max_pair]]

        pp, qq = pair_of[order], query_of[order]
        sel_s, sel_o = sids[pp], oids[pp]
        st, en = start[pp, qq], end[pp, qq]
        host = torch.stack([sel_s, sel_o, cat_ids[sel_s], top_cat.reshape(-1)[order].long(), cat_ids[sel_o],
                            so_start[pp] + st, so_start[pp] + en,
                            so_start[pp] - durs[sel_s, 0] + st, so_start[pp] - durs[sel_o, 0] + st, en - st],
                           dim=1).cpu().tolist()
        out = {
            "triplets": [r[2:5] for r in host],
            "triple_scores": tri[order].cpu().tolist(),
            "triple_scores_avg": avg[order].cpu().tolist(),
        }
        if self.with_so_trajs:
            out["so_trajs"] = self._so_trajs(input_data['bboxes_list'], host)
        out["pred_durations"] = [r[5:7] for r in host]
        out["so_tids"] = [r[0:2] for r in host]
        return out

    @staticmethod
    def _so_trajs(boxes, host):
        """The box tracks of the winners `host` (rows [subject, object, .., .., .., .., .., subject's first box, object's first
        box, frames]) from the video's per-tracklet boxes."""
        # box tracks of the winners: every tracklet that appears is copied to the host ONCE (one concatenation, one
        # copy); each triplet then converts its slice of the host array to fresh Python lists.  The reference slices
        # and .tolist()s two device tensors per triplet (maskvrd.py:302-306): 400 device round trips.
        used = sorted({r[0] for r in host} | {r[1] for r in host})
        flat = torch.cat([boxes[t] for t in used], dim=0).cpu().numpy()
        rows_of, at = {}, 0
        for t in used:
            rows_of[t] = flat[at:at + len(boxes[t])]
            at += len(boxes[t])
        # ~100 k small lists are created here; the cyclic collector would walk the whole process (every module and
        # parameter of the model) several times on the way, for objects that cannot form cycles
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            so_trajs = []
            for r in host:
                s_rows = rows_of[r[0]][r[7]:r[7] + r[9]].tolist()
                o_rows = rows_of[r[1]][r[8]:r[8] + r[9]].tolist()
                assert len(s_rows) == len(o_rows)
                so_trajs.append([s_rows, o_rows])
        finally:
            if gc_was_on:
                gc.enable()
        return so_trajs

    @torch.no_grad()
    def forward_test_videos(self, videos):
        """forward_test for a list of videos in one pass: item i of the result is what forward_test(videos[i]) returns (None
        for a video without a triplet, or for an empty / None entry).  The pairs of all videos run through the network as one
        batch -- a pair's outputs depend only on its own padded length (tight padding), and every pair keeps the reference's
        padded length of its own video's max_so_pair slice -- then one vrd_select_triplets launch picks every video's
        top-n_max_pair triplets and the winners of all videos come to the host in one copy.  The videos come in one form:
        `pair_source`, its plain-tensor fields, or `so_features_list`.  Eval launches cost the same for 50 pairs as for a few
        hundred: evaluating a few dozen small videos per call is what this is for (vrdone_amd.evaluate.batched_forward_test)."""
        import numpy as np
        if getattr(self, "_shard", None):
            raise NotImplementedError("forward_test_videos: a multi-video call does not shard its pairs over ranks; call "
                                      "forward_test per video after shard_pairs(), or shard_pairs(enable=False)")
        videos = list(videos)
        results = [None] * len(videos)
        live = [i for i, v in enumerate(videos) if v]
        if not live:
            return results
        form = {("source" if "pair_source" in videos[i] else "fields" if "tracklet_visual" in videos[i] else "feats") for i in live}
        if len(form) > 1:
            raise ValueError("forward_test_videos: the videos of one call must come in one form (pair_source, its plain-tensor "
                             "fields, or so_features_list)")
        form = form.pop()
        dev = self.device
        Q, k = self.predictor.num_queries, self.topk
        if form == "feats":
            source = None
            feats = [f for i in live for f in videos[i]['so_features_list']]
            lens_v = [[int(f.shape[1]) for f in videos[i]['so_features_list']] for i in live]
        else:
            from ..proposals import PairSource
            srcs = [videos[i]['pair_source'] if form == "source" else PairSource.from_fields(videos[i], dev) for i in live]
            source, feats = PairSource.concat(srcs), None
            lens_v = [list(s.lens) for s in srcs]
        counts = [len(lv) for lv in lens_v]
        lens = [L for lv in lens_v for L in lv]
        P = len(lens)
        # the reference's padded lengths video by video, then one tight-padding plan over all pairs of the call
        t_refs = [t for lv in lens_v for t in self._reference_pad(lv)]
        order, t_pad = eval_batches.pair_order(self, lens, t_refs)

        # per-pair tables on the host, in one upload: [s score | o score | so_offset | so_start | so_end | video pair offsets]
        base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        table = np.zeros(5 * P + len(live) + 1, dtype=np.int32)
        scores = table[:2 * P].view(np.float32)
        host_in = []
        for j, i in enumerate(live):
            d = videos[i]
            h = lambda t: torch.as_tensor(t).cpu().numpy()          # noqa: E731
            sids, oids = h(d['sids']).astype(np.int64), h(d['oids']).astype(np.int64)
            assert len(sids) == counts[j]
            durs, cat_scores = h(d['traj_durations']).astype(np.int64), h(d['cat_scores']).astype(np.float32)
            so_start = np.maximum(durs[sids, 0], durs[oids, 0])
            so_end = np.minimum(durs[sids, 1], durs[oids, 1])
            offs = h(d['so_offset']).astype(np.int64)
            a, b = base[j], base[j + 1]
            scores[a:b], scores[P + a:P + b] = cat_scores[sids], cat_scores[oids]
            table[2 * P + a:2 * P + b], table[3 * P + a:3 * P + b], table[4 * P + a:4 * P + b] = offs, so_start, so_end
            host_in.append((sids, oids, durs, cat_scores, h(d['cat_ids']).astype(np.int64), offs, so_start))
        table[5 * P:] = base
        unsort = np.empty(P, dtype=np.int64)
        unsort[np.asarray(order, dtype=np.int64)] = np.arange(P)
        table_dev = torch.from_numpy(table).to(dev)              # uploaded before the first kernel is queued
        unsort_dev = torch.from_numpy(unsort).to(dev)
        f_dev = table_dev[:2 * P].view(torch.float32)

        ops = _ops()
        f16 = ops.f16_planes()
        if f16:
            flag = ops.f16_range_flag(next(self.parameters()).device)
            flag.zero_()
        cand = self.pair_candidates(feats, lens, order, t_pad, k, source=source, t_refs=t_refs)[unsort_dev]     # each video's own pair order
        ints = cand.view(torch.int32)
        vp = table_dev[5 * P:]
        count, index, score = ops.select_triplets(cand, f_dev[:P], f_dev[P:], table_dev[2 * P:3 * P], table_dev[3 * P:4 * P],
                                                  table_dev[4 * P:5 * P], vp, self.feat_stride, self.pred_min_frames,
                                                  self.n_max_pair, max(counts))
        # the winners' record fields, all videos at once: pair row, query, rank -> score, class, first, last frame
        idx = index.clamp(min=0).long()
        row = (vp[:-1, None].long() + idx // (Q * k)) * Q + (idx // k) % Q
        rank = (idx % k)[..., None]
        rec = ints.view(P * Q, 2 * k + 2)[row]                                                 # (V, n_max_pair, 2k + 2)
        fields = [count.reshape(-1), index.reshape(-1), rec.gather(-1, rank).reshape(-1), rec.gather(-1, rank + k).reshape(-1),
                  rec[..., 2 * k].reshape(-1), rec[..., 2 * k + 1].reshape(-1), score.view(torch.int32).reshape(-1)]
        if f16:
            # the range flag, and whether any score is not finite (forward_test's test for a repeat in f32)
            fields.append(flag.reshape(-1).to(torch.int32))
            fields.append((~torch.isfinite(cand[:, :, :k])).any().reshape(1).to(torch.int32))
        host = torch.cat(fields).cpu().numpy()
        V, N = len(live), self.n_max_pair
        if f16 and (host[-2] != 0 or host[-1] != 0):
            import warnings
            warnings.warn(f"vrdone_amd: an activation beyond the {ops.get_precision()} mode's operand range (or non-finite inputs) in a "
                          "multi-video call: repeating its videos one by one")
            for i in live:
                results[i] = self.forward_test(videos[i])
            return results
        at = 0

        def take(n, dtype=np.int32):
            nonlocal at
            out = host[at:at + n].view(dtype)
            at += n
            return out
        cnt = take(2 * V).reshape(V, 2)
        sel, p_score, p_cat = take(V * N).reshape(V, N), take(V * N, np.float32).reshape(V, N), take(V * N).reshape(V, N)
        first, last, avg = take(V * N).reshape(V, N), take(V * N).reshape(V, N), take(V * N, np.float32).reshape(V, N)
        assert not cnt[:, 1].any() and (cnt[:, 0] >= 0).all(), "a kept candidate lies outside its pair's shared frames"
        for j, i in enumerate(live):
            n = int(cnt[j, 0])
            if n == 0:
                continue
            sids, oids, durs, cat_scores, cat_ids, offs, so_start = host_in[j]
            fl = sel[j, :n].astype(np.int64)
            pp = fl // (Q * k)
            sel_s, sel_o = sids[pp], oids[pp]
            st = first[j, :n].astype(np.int64) * self.feat_stride + offs[pp]
            en = last[j, :n].astype(np.int64) * self.feat_stride + offs[pp] + 1
            rows = np.stack([sel_s, sel_o, cat_ids[sel_s], p_cat[j, :n].astype(np.int64), cat_ids[sel_o],
                             so_start[pp] + st, so_start[pp] + en,
                             so_start[pp] - durs[sel_s, 0] + st, so_start[pp] - durs[sel_o, 0] + st, en - st], axis=1).tolist()
            tri = np.stack([cat_scores[sel_s], p_score[j, :n], cat_scores[sel_o]], axis=1)
            out = {
                "triplets": [r[2:5] for r in rows],
                "triple_scores": tri.tolist(),
                "triple_scores_avg": avg[j, :n].tolist(),
            }
            if self.with_so_trajs:
                out["so_trajs"] = self._so_trajs(videos[i]['bboxes_list'], rows)
            out["pred_durations"] = [r[5:7] for r in rows]
            out["so_tids"] = [r[0:2] for r in rows]
            results[i] = out
        return results
