"""Float64 emulation of the f16x1 mode's operand rounding (include/vrdone_hip.h, vrd_gemm_args.products = 1): what the one-product
GEMM and flash-attention kernels compute, up to their f32 accumulation.

    activations  f16(x * 2^4) / 2^4                       (VRD_F16_ACT_EXP = 4; subnormals kept)
    weights      f16(w * 2^e) / 2^e, max |w| * 2^e in [2^14, 2^15)  (one power of two per weight tensor, vrd_split_weight)
    attention    scores from the rounded q and k, softmax in float64, P rounded once as f16(P * 2^4) / 2^4, output from the
                 rounded P and v, divided by the sum of the UNROUNDED P (the kernels' f32 running sum)

oracle_f16x1() applies the same rounding to the CPU oracle (oracle/vrd_oracle.py) as a whole: inside it every conv the HIP path
runs as a split-precision GEMM (groups == 1, Cin * k % 32 == 0) and every global attention it runs on the flash kernels
(head_dim 64 / 128, >= 32 queries) is replaced by its emulation, so O.mask_vrd / O.forward_test compute what the f16x1 mode
computes, up to f32 accumulation order and where the kernels set the reference point of P's rounding.

Used by the f16x1 tests to calibrate their tolerances; no GPU needed."""
import contextlib
import math

import torch
import torch.nn.functional as F

ACT_EXP = 4


def round_act(x):
    """f16 rounding of an activation at the fixed scale 2^4, back in float64"""
    s = 2.0 ** ACT_EXP
    return (x.double() * s).to(torch.float16).double() / s


def weight_exp(w):
    """the per-tensor exponent e of vrd_split_weight: max |w| * 2^e in [2^14, 2^15)"""
    m = float(w.abs().max())
    if m == 0.0:
        return 0
    return 14 - math.floor(math.log2(m))


def round_weight(w):
    e = weight_exp(w)
    return (w.double() * 2.0 ** e).to(torch.float16).double() / 2.0 ** e


def conv1d(x, w, bias=None):
    """channels-last (B, T, Cin) x (N, Cin, k) conv with zero padding, on the rounded operands (float64)"""
    k = w.shape[-1]
    xs = round_act(x).transpose(1, 2)
    y = torch.nn.functional.conv1d(xs, round_weight(w), None if bias is None else bias.double(), padding=k // 2)
    return y.transpose(1, 2)


def attention(q, k, v, kv_mask, n_head):
    """q: (B, Tq, C), k / v: (B, Tk, C), kv_mask (B, Tk) bool or None -> (B, Tq, C) float64.  P is rounded relative to the row
    maximum (the test inputs keep that maximum in the first key tile, where the kernels set their reference point)."""
    B, Tq, C = q.shape
    Tk = k.shape[1]
    hd = C // n_head
    qh = round_act(q).reshape(B, Tq, n_head, hd).transpose(1, 2)
    kh = round_act(k).reshape(B, Tk, n_head, hd).transpose(1, 2)
    vh = round_act(v).reshape(B, Tk, n_head, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    if kv_mask is not None:
        s = s.masked_fill(~kv_mask[:, None, None, :], float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    p_hi = round_act(p)
    return (p_hi @ vh / l).transpose(1, 2).reshape(B, Tq, C)


def _conv1d(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    k = weight.shape[-1]
    if groups != 1 or (weight.shape[1] * k) % 32 or stride != 1 or dilation != 1 or not x.is_floating_point():
        return F.conv1d(x, weight, bias, stride=stride, padding=padding, dilation=dilation, groups=groups)
    y = F.conv1d(round_act(x), round_weight(weight), None if bias is None else bias.double(), padding=padding)
    return y.to(x.dtype)


class _Functional:
    """torch.nn.functional with conv1d replaced by the emulated one"""

    def __getattr__(self, name):
        return _conv1d if name == "conv1d" else getattr(F, name)


def _full_attention(orig):
    def attn(q, k, v, kv_mask, n_head):
        B, C, Tq = q.shape
        if C // n_head not in (64, 128) or Tq < 32:          # the HIP path's exact-f32 attention
            return orig(q, k, v, kv_mask, n_head)
        out = attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), kv_mask[:, 0], n_head)
        return out.transpose(1, 2).to(q.dtype)
    return attn


@contextlib.contextmanager
def oracle_f16x1():
    """the CPU oracle with the f16x1 mode's operand rounding (see the module docstring)"""
    from oracle import vrd_oracle as O
    saved = O.F, O.full_attention
    O.F, O.full_attention = _Functional(), _full_attention(O.full_attention)
    try:
        yield O
    finally:
        O.F, O.full_attention = saved
