"""MaskFormer-style 1-D mask-segmentation head: query decoder over the coarsest level, class
logits per query and a per-query temporal mask = <mask embedding, mask features>.  Same
constructor and parameter tree as the reference's models/predictor.py."""
import math

from torch import nn

from . import ragged
from .blocks import ConvMLP, LayerNorm, Layout, _mask2d, _ops, _to_cl
from .local_transformer import MaskedConvTransformerDecoderOnly


class MaskedTransformerPredictor(nn.Module):
    def __init__(self, n_input, n_embd, n_head, n_hidden, num_queries, num_classes, attn_pdrop=0.0, proj_pdrop=0.0,
                 path_pdrop=0.1, cls_prior_prob=0.01, n_qx_stride=0, n_kv_stride=1, num_layers=4,
                 deep_supervision=False, enforce_input_project=False):
        super().__init__()
        self.transformer = MaskedConvTransformerDecoderOnly(
            n_embd, n_head, n_hidden, attn_pdrop=attn_pdrop, proj_pdrop=proj_pdrop, path_pdrop=path_pdrop,
            n_qx_stride=n_qx_stride, n_kv_stride=n_kv_stride, num_layers=num_layers,
            return_intermediate=deep_supervision)
        self.num_queries = num_queries
        self.query_embed = nn.Embedding(num_queries, n_embd)
        self.input_norm = LayerNorm(n_input)
        self.input_proj = None
        if n_input != n_embd or enforce_input_project:
            self.input_proj = nn.Conv1d(n_input, n_embd, kernel_size=1)
            nn.init.zeros_(self.input_proj.bias)
        self.aux_loss = deep_supervision
        self.class_embed = nn.Conv1d(n_embd, num_classes + 1, 1)      # + background
        nn.init.constant_(self.class_embed.bias, -math.log((1 - cls_prior_prob) / cls_prior_prob))
        self.mask_embed = ConvMLP(n_embd, n_embd, n_embd, 3)

    def heads(self, x, mask_features, mask, output_mask, with_aux=None, fill=-10.0, klay=None, lay0=None):
        """x, mask: the coarsest level's rows in the layout klay; mask_features, output_mask: the full-resolution rows in lay0
        (default: the batch form, x (B, T/8, D), mask_features (B, T, Dp), mask (B, T/8), output_mask (B, T)).
        -> [(logits (B, Q, K+1), [mask logits (n_i, Q, T_i) per bucket of lay0])] for the last decoder layer, preceded by the
        other layers' when with_aux asks for them."""
        ops = _ops()
        klay, lay0 = Layout.of(klay, mask), Layout.of(lay0, output_mask)
        src = self.input_norm.cl(x, pair=ops.pair_mode() and self.input_proj is not None)
        if self.input_proj is not None:
            src = ops.conv_gemm(src, self.input_proj.weight, self.input_proj.bias, row_mask=mask)
        qlay = klay.queries(self.num_queries)
        hs = self.transformer.cl(src, mask, self.query_embed.weight, self._with_aux(with_aux), klay)
        out = []
        # (the last layer's head first: under autograd the order of the heads is the order in which the gradients of their shared
        # weights and of mask_features are summed)
        for h in hs[-1:] + hs[:-1]:
            h = qlay.part(h, (0, qlay.rows // self.num_queries, self.num_queries))      # (B, Q, C)
            logits = ops.conv_gemm(h, self.class_embed.weight, self.class_embed.bias)
            out.append((logits, ragged.mask_head(lay0, self.mask_embed.cl(h), mask_features, output_mask, fill)))
        return out[1:] + out[:1]

    def _with_aux(self, with_aux):
        """with_aux=None follows the reference (all decoder layers' heads when deep_supervision);
        with_aux=False computes the last layer only (what forward_test reads, maskvrd.py:206)."""
        return bool((self.aux_loss if with_aux is None else with_aux) and self.aux_loss)

    def cl(self, x, mask_features, mask, output_mask, with_aux=None, non_attn_const=-10):
        """The batch form: x (B, T/8, D), mask_features (B, T, Dp), mask (B, T/8), output_mask (B, T) -> the reference's dict."""
        heads = [(logits, seg) for logits, (seg,) in self.heads(x, mask_features, mask, output_mask, with_aux, float(non_attn_const))]
        out = dict(zip(("pred_logits", "pred_masks"), heads[-1]))
        if self._with_aux(with_aux):
            out["aux_outputs"] = [dict(zip(("pred_logits", "pred_masks"), h)) for h in heads[:-1]]
        out["output_mask"] = output_mask[:, None, :]
        return out

    def forward(self, x, mask_features, mask, output_mask, non_attn_const=(-10)):
        return self.cl(_to_cl(x), _to_cl(mask_features), _mask2d(mask), _mask2d(output_mask),
                       non_attn_const=non_attn_const)
