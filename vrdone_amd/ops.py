"""Tensor-level wrappers over the C ABI (include/vrdone_hip.h).

Activations are fp32 HIP tensors in channels-last form, shape ``(B, T, C)`` (or any
``(..., C)``) whose last stride is 1 and whose rows are uniformly strided, so a column slab of a
wider buffer (``buf[..., 512:1024]``) is a legal operand: that is how concatenations are built
without copies.  Masks are ``torch.bool``/``uint8`` tensors of shape ``(B, T)``.

PyTorch is used for device memory and the current stream only; every op below runs one
hand-written HIP kernel.  Nothing here works on CPU tensors.
"""
import collections
import ctypes as C
import os

import torch

from . import _hip
from ._hip import ACT_GELU, ACT_NONE, ACT_RELU, lib  # noqa: F401


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current stream of the current device as a hipStream_t.  (Through the raw-handle call: torch.cuda.current_stream()
    builds a Stream object per call, ~5 us of the ~15 us an op of this module spends on the host -- a forward_test call on a
    real-sized video is ~230 launches and bound by exactly that.)"""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t):
    """(data_ptr, n_rows, n_cols, leading dimension) of a channels-last operand."""
    if not t.is_cuda:
        raise RuntimeError("vrdone_amd ops need HIP tensors (no CPU path exists for the hot path)")
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    if t.stride(-1) != 1:
        raise ValueError("channels-last operand must have unit stride along channels")
    cols = t.shape[-1]
    rows = t.numel() // cols
    if t.dim() == 1 or rows == 1:
        return t.data_ptr(), rows, cols, cols
    ld = t.stride(-2)
    for d in range(t.dim() - 3, -1, -1):       # outer dims must collapse onto the row index
        if t.shape[d] != 1 and t.stride(d) != t.stride(d + 1) * t.shape[d + 1]:
            raise ValueError(f"rows are not uniformly strided: shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), rows, cols, ld


def _ptr(t):
    return None if t is None else t.data_ptr()


def _param_ptr(t, like, what="parameter"):
    """Device pointer of a parameter tensor handed to a kernel as a flat f32 array (None stays None): it must be a
    contiguous float32 tensor on the activations' device -- a model left on the CPU, or after .half() / .double(),
    raises here instead of faulting on the GPU."""
    if t is None:
        return None
    if not t.is_cuda or t.device != like.device:
        raise RuntimeError(f"{what} lives on {t.device}, the activations on {like.device}: move the model with .to(device)")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t.data_ptr()


class Pair:
    """A channels-last tensor stored in the GEMM-operand "pair" format of the split-precision modes: the 4*C bytes of a
    C-channel row (C % 32 == 0) hold, per block of 32 channels, [32 x 16-bit hi | 32 x 16-bit lo] instead of 32 floats --
    bf16 planes of x (fmt PAIR_BF16, the bf16x3 mode) or f16 planes of x * 2^F16_ACT_EXP (PAIR_F16, the f16x3 mode).  `t` is
    the f32-typed buffer (same shape / strides as the f32 tensor would have); `width` records the width of the producer's
    slab (the format itself does not depend on it).  Only conv_gemm() and attention() consume a Pair."""
    __slots__ = ("t", "width", "fmt")

    def __init__(self, t, width, fmt=None):
        self.t, self.width, self.fmt = t, width, pair_fmt() if fmt is None else fmt
        assert self.fmt in (_hip.PAIR_BF16, _hip.PAIR_F16)

    @property
    def shape(self):
        return self.t.shape

    def __getitem__(self, idx):      # batch slicing (rows) keeps the format
        return Pair(self.t[idx], self.width, self.fmt)

    def float(self):
        """Decode to f32 (hi + lo); for tests."""
        f16 = self.fmt == _hip.PAIR_F16
        raw = self.t.contiguous().view(torch.float16 if f16 else torch.bfloat16)                 # (..., 2*C)
        blocks = raw.reshape(*raw.shape[:-1], -1, 2, 32).float()
        val = (blocks[..., 0, :] + blocks[..., 1, :]).reshape(*self.t.shape)
        return val * 2.0 ** -_hip.F16_ACT_EXP if f16 else val


def flash_pair_ok(n_head, channels, Tq):
    """True when global attention of this shape runs the split-precision flash kernel on pair-row q/k/v."""
    hd = channels // n_head
    # head_dim 32: the three-product modes only (vrd_attention_pair has no one-product form there: f16x1 stays on f32 rows and the
    # vector-unit kernel).  No higher threshold than 32 query rows: measured per launch (scripts/flash_bench.py --hd 32 --pair, MI355X,
    # 2048 sequences of T rows, f16x3), this route / attn_small on f32 rows: 16 heads T = 32: 0.17 / 3.9 ms, 64: 0.28 / 13.4,
    # 96: 0.43 / 30.2, 288 (256 valid): 1.64 / 323; 8 heads T = 32: 0.06 / 1.56, 96: 0.21 / 14.5 (run-to-run spread below 5 %)
    if hd == 32:
        return pair_mode() and _precision in ("bf16x3", "f16x3") and Tq >= 32
    return pair_mode() and hd in (64, 128) and Tq >= 32


def pair_mode():
    """True when producers should emit pair rows for GEMM-only consumers: a split-precision mode and autograd not recording
    (a differentiable forward keeps every activation as plain f32 rows, see vrdone_amd/autograd.py)."""
    return _precision in ("bf16x3", "f16x3", "f16x1") and not torch.is_grad_enabled()


def pair_fmt():
    """enum vrd_pair_format of the current precision mode's pair rows and split weights (0 in the f32 mode)."""
    return {"bf16x3": _hip.PAIR_BF16, "f16x3": _hip.PAIR_F16, "f16x1": _hip.PAIR_F16}.get(_precision, _hip.PAIR_NONE)


def f16_planes():
    """True in the modes whose operands are f16 planes of power-of-two scaled values (f16x3, f16x1): the modes with an operand
    range (f16_range_flag) and an f32 repeat when it is exceeded."""
    return _precision in ("f16x3", "f16x1")


def products():
    """MFMA products per split-precision operand pair of the current mode, as vrd_gemm_args.products / vrd_attention_pair take
    it: 1 in the f16x1 mode (a_hi * w_hi only), 0 (= the three-product form) otherwise."""
    return 1 if _precision == "f16x1" else 0


def check_differentiable(what="autograd"):
    """The f16x1 mode is forward-only: anything that would record autograd in it raises ValueError."""
    if _precision == "f16x1":
        raise ValueError(f"{what}: the f16x1 precision mode is forward-only (one f16 product per GEMM / attention, no backward); "
                         "run under torch.no_grad() or switch to f16x3 / bf16x3 / f32 for training")


def split_backward():
    """True when the backward GEMMs (input and weight gradients) run as split-precision products: bf16 planes in the bf16x3 mode;
    in the f16x3 mode f16 planes of the gradient times a per-tensor power of two (backward_fmt, grad_scale) -- reference-grade
    products like the forward pass's (the reference differentiates in float32, train.py:182-186)."""
    return _precision in ("bf16x3", "f16x3")


_F16_BACKWARD = os.environ.get("VRDONE_F16_BACKWARD", "1") != "0"       # A/B switch: 0 = the f16x3 mode's backward on bf16 planes


def backward_fmt():
    """element format of the backward GEMMs' split operands"""
    return _hip.PAIR_F16 if (_precision == "f16x3" and _F16_BACKWARD) else _hip.PAIR_BF16


_grad_scales = {}


def grad_scale(g, slot=0):
    """{2^e, 2^-e} (device floats [0], [1] of a buffer of _hip.ABSMAX_SCALE_FLOATS) with max |g| 2^e in [2^13, 2^14) for the (rows, C) gradient `g`
    (vrd_absmax_scale, one launch), or None when g's rows are not float4-aligned (the caller then keeps the bf16 planes).  The
    buffer is one per (device, stream): it is only read by the launches that directly follow on the same stream; launches
    recorded into a graph get one of their own per call (from the graph's pool)."""
    pg, rows, cols, ldg = _rows(g)
    if cols % 4 or ldg % 4 or pg % 16:
        return None
    if torch.cuda.is_current_stream_capturing():
        # (a slice of a zeroed block of the recording: one fill node per block instead of one per call -- ~140 per recorded step)
        from .autograd import _zeros
        buf = _zeros(_hip.ABSMAX_SCALE_FLOATS, device=g.device)
    else:
        key = (g.device, torch.cuda.current_stream(g.device).cuda_stream, slot)      # (slot: a consumer that needs two at once)
        buf = _grad_scales.get(key)
        if buf is None:
            buf = _grad_scales[key] = torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=g.device, dtype=torch.float32)
    _hip.check(lib.vrd_absmax_scale(pg, ldg, rows, cols, buf.data_ptr(), _stream()), "vrd_absmax_scale")
    return buf


def _fmt(pair):
    """an op's `pair=` flag -> the out_pair argument of its C entry point"""
    return pair_fmt() if pair else _hip.PAIR_NONE


def recording(*tensors):
    """True when autograd is recording and one of the tensors needs a gradient: the op then runs as the
    torch.autograd.Function(s) of vrdone_amd/autograd.py (HIP kernels forward and backward)."""
    rec = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)
    if rec:
        check_differentiable()
    return rec


def join(buf, parts, dim=-1):
    """The concatenation of `parts` along `dim`: `buf`, which the producers already filled through `out=` slabs, or
    -- under autograd, where ops return fresh tensors and ignore `out=` -- torch.cat(parts)."""
    if torch.is_grad_enabled() and any(torch.is_tensor(q) and q.requires_grad for q in parts):
        return torch.cat(parts, dim=dim)
    return buf


def _unwrap(x):
    return (x.t, x.width) if isinstance(x, Pair) else (x, 0)


def _as_pair(t, width, fmt):
    """what an op returns for the buffer `t` it wrote with out_pair = fmt: the Pair, or t itself for f32 rows (fmt 0)"""
    return Pair(t, width, fmt) if fmt else t


def _mask_ptr(m, rows):
    if m is None:
        return None
    if m.dtype not in (torch.bool, torch.uint8) or not m.is_contiguous() or m.numel() != rows:
        raise ValueError(f"mask must be a contiguous bool/uint8 tensor with one byte per row ({m.numel()} vs {rows})")
    return m.data_ptr()


# Derived weight layouts are cached ON the parameter object (so they die with it and can never be
# confused with another tensor that later reuses the same address), keyed on (data_ptr, version).
_capture_keep = []


def _capturing():
    """True while the current stream records a HIP graph (vrdone_amd/train_graph.py): derived operands are then built
    inside the graph on every replay -- a cache hit would leave their kernels out of the recording, and every replay
    would see the operand of the weights (or mask) as they were at capture time."""
    on = torch.cuda.is_current_stream_capturing()
    if not on and _capture_keep:
        _capture_keep.clear()
    return on


def _keep_for_capture(val):
    """Operands built during a capture stay referenced until it is over: call sites hand their addresses to a launch and
    drop the tensor, which the cache normally keeps alive -- freed inside a capture, the pool would give the memory to the
    next allocation before the launch that reads it."""
    _capture_keep.append(val)
    return val


def _version_key(t):
    return (t.data_ptr(), t._version)


def _entry(owner, slot, key):
    """The (key, value, scope) entry of `slot` on `owner` when it was made for `key`, else None.  scope: the presplit_scope
    whose capture presplit_weights published the entry in, None for an entry made outside any capture."""
    hit = getattr(owner, slot, None)
    return hit if hit is not None and hit[0] == key else None


def _derived(owner, slot, key, build):
    """The operand `build()` derives from `owner` (a weight, a mask), cached in its attribute `slot` for as long as `key`
    -- (address, version) of everything it was derived from -- holds."""
    hit = _entry(owner, slot, key)
    if _capturing():
        # inside a recording only what presplit_weights built inside the SAME recording scope counts (its launch is part of
        # the graph; train_graph opens one scope around a recording's forward and backward graphs); nothing is stored
        if hit is not None and hit[2] is not None and hit[2] is _presplit_scope:
            return hit[1]
        return _keep_for_capture(build())
    if hit is None:
        hit = (key, build(), None)
        setattr(owner, slot, hit)
    return hit[1]


def packed_conv_weight(w):
    """Conv1d weight (N, Cin, k) -> (N, k*Cin) tap-major for k = 3; k = 1 weights are used in place."""
    if w.shape[-1] == 1:
        return w
    return _derived(w, "_vrd_packed", _version_key(w), lambda: w.detach().permute(0, 2, 1).contiguous())


# GEMM precision mode.
#   "bf16x3": every f32 product a*w is formed as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on the bf16
#            MFMA with f32 accumulation (x = x_hi + x_lo split in bf16): ~17 significand bits per product.
#            Measured end to end: logits within 7e-5 of the reference (stated tolerance 1e-3).
#   "f16x3": the same three products on the f16 MFMA, operands scaled by exact powers of two (activations 2^4, weights per
#            tensor): ~22 significand bits per product.  The reference-grade mode: end to end it is as far from a float64
#            run of the reference as the reference's own float32 run is (x1.0-1.3, tests/golden/mask_vrd_f64.npz), at the
#            speed of bf16x3.  Forward products only: the backward GEMMs of this mode are bf16x3's (gradients have no
#            fixed scale to split an f16 pair at).  The default.
#            Activations beyond +-4094 overflow the f16 planes.  Every kernel that writes such planes reports it in a flag word
#            on the device (f16_range_flag()); MaskVRD.forward_test, forward_training and forward_loss read the word with their
#            results and repeat the call in the f32 mode; a direct caller of _mask_vrd checks f16_range_exceeded() itself.
#   "f16x1": the f16x3 operands with ONE product, a_hi*w_hi (and in the global attention q_hi*k_hi, then p_hi*v_hi with the
#            probabilities rounded once, f16(P * 2^4)): ~11 significand bits per operand.  An opt-in inference mode, NOT
#            reference-grade: logits ~4e-3 and mask logits ~5e-2 from the reference (the north star's 1e-3 is missed), the same
#            forward_test records on the golden videos.  Forward only: anything that would record autograd raises ValueError.
#            Same range flag and f32 repeat as f16x3.  bench.py has no entry for it (scripts/precision_ab.py measures it).
#   "f32":   exact f32 MFMA products (bit-level fmaf chains); logits within 9e-6; ~2.8x slower end to end (bench.py).
# Select with set_precision() or the VRDONE_PRECISION environment variable.  Everything outside the
# conv GEMMs and the global attention (LayerNorm, depthwise convs, softmax, banded attention) is f32 in all modes.
_PRECISIONS = ("f32", "bf16x3", "f16x3", "f16x1")
_precision = os.environ.get("VRDONE_PRECISION", "f16x3")
if _precision not in _PRECISIONS:
    raise ValueError(f"VRDONE_PRECISION must be one of {_PRECISIONS}, got {_precision!r}")


def set_precision(mode):
    global _precision
    if mode not in _PRECISIONS:
        raise ValueError(f"precision must be one of {_PRECISIONS}, got {mode!r}")
    _precision = mode


def get_precision():
    return _precision


class use_precision:
    """`with ops.use_precision("f32"):` -- the mode inside the block, the previous one after it."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = get_precision()
        set_precision(self.mode)
        return self

    def __exit__(self, *exc):
        set_precision(self.prev)
        return False


# Deterministic mode: a training step's losses, gradients, updated parameters and EMA weights are the same bits for the same
# seed, inputs, precision mode and device type -- whatever the workgroup schedule, the allocator's alignment, the scratch offered,
# eager or HIP-graph execution, this process or another.  It passes VRD_DETERMINISTIC to the parameter-gradient kernels (partial
# sums added in index order, no float atomics, shape-only chunking: include/vrdone_hip.h) and re-draws the stochastic-depth
# factors of every forward_training call (models/blocks.py, _FactorPool).  Opt-in: set_deterministic() / use_deterministic() /
# VRDONE_DETERMINISTIC=0|1; undecided, it follows torch.are_deterministic_algorithms_enabled() or torch.backends.cudnn.deterministic,
# the switches the reference's utils.set_seed sets.  Read at forward time; every autograd Function records it for its backward.
_deterministic = None                    # None: follow torch's flags
_env_det = os.environ.get("VRDONE_DETERMINISTIC")
if _env_det is not None:
    if _env_det not in ("0", "1"):
        raise ValueError(f"VRDONE_DETERMINISTIC must be 0 or 1, got {_env_det!r}")
    _deterministic = _env_det == "1"


def set_deterministic(on):
    """True / False: the mode on / off whatever torch's flags say; None: follow torch's flags again."""
    global _deterministic
    _deterministic = None if on is None else bool(on)


def get_deterministic():
    if _deterministic is not None:
        return _deterministic
    return bool(torch.are_deterministic_algorithms_enabled() or torch.backends.cudnn.deterministic)


class use_deterministic:
    """`with ops.use_deterministic(True):` -- the mode inside the block, the previous setting (explicit or following torch) after it."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = _deterministic
        set_deterministic(self.on)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


def grad_flags():
    """`flags` of the parameter-gradient kernels in the current mode."""
    return _hip.DETERMINISTIC if get_deterministic() else 0


# ---- the f16x3 mode's operand range (include/vrdone_hip.h, vrd_f16_range_flag)
_range_flags = {}


class _DeviceWord:
    """one int32 of library-owned device memory, presented to torch through __cuda_array_interface__"""

    def __init__(self, ptr):
        self.__cuda_array_interface__ = {"shape": (1,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def f16_range_flag(device=None):
    """The device's f16 operand-range flag as a 1-element int32 tensor (a view of the library's word, not a copy): non-zero
    once any producer of f16 pair rows met a value beyond +-4094 since the word was last cleared; the bits name the
    producing kernel families (_hip.RANGE_TAGS).  Read it WITH a call's results (`.clone()` on the same stream, or one
    `.item()` where the results are synchronised anyway) and clear it with `.zero_()`."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    flag = _range_flags.get(dev.index)
    if flag is None:
        with torch.cuda.device(dev):
            ptr = C.c_void_p()
            _hip.check(lib.vrd_f16_range_flag(C.byref(ptr)), "vrd_f16_range_flag")
            flag = _range_flags[dev.index] = torch.as_tensor(_DeviceWord(ptr.value), device=dev)
    return flag


def f16_range_exceeded(device=None, clear=True):
    """True when the flag is set (one 4-byte read: a host synchronisation); clears it by default.  `describe_range(bits)` names
    the producers."""
    flag = f16_range_flag(device)
    bits = int(flag.item())
    if bits and clear:
        flag.zero_()
    return bits


def describe_range(bits):
    return ", ".join(name for bit, name in _hip.RANGE_TAGS.items() if bits & bit) or "none"


class SplitWeight:
    """A weight's split-precision operand: `t` the (R, K/32, 2, 32) 16-bit planes, `fmt` their element format and (PAIR_F16)
    `scale` the 4 device floats vrd_split_weight wrote: [0] = 2^-(e_w + F16_ACT_EXP), the GEMM's accumulator factor."""
    __slots__ = ("t", "fmt", "scale")

    def __init__(self, t, fmt, scale=None):
        self.t, self.fmt, self.scale = t, fmt, scale

    def data_ptr(self):
        return self.t.data_ptr()

    def set_args(self, a):
        """W_split, split_fmt and w_scale of a GemmArgs"""
        a.W_split, a.split_fmt = self.t.data_ptr(), self.fmt
        a.w_scale = self.scale.data_ptr() if self.scale is not None else None


def _split_forms(shape, fwd_fmt, bwd_fmt):
    """The split operands a Conv1d weight of `shape` (N, Cin, k) has, as vrd_split_weight / a vrd_split_job reads them from the
    parameter: (cache attribute -- one per element format --, fmt, offset of the first element, R rows, Q, taps, and the
    parameter's strides along r, tap and q).  The forward operand (fwd_fmt; Cin*k % 32 == 0) is the tap-major packed weight,
    the input-gradient operand (bwd_fmt; N*k % 32 == 0) the (Cin, k*N) matrix [c][tap*N + n] = w[n][c][k-1-tap]: transposed,
    taps flipped.  A format of None leaves that operand out."""
    N, Cin, k = shape
    f16 = lambda fmt: "_f16" if fmt == _hip.PAIR_F16 else ""      # noqa: E731
    if fwd_fmt is not None and (Cin * k) % 32 == 0:
        yield ("_vrd_split" + f16(fwd_fmt), fwd_fmt, 0, N, Cin, k, Cin * k, 1, k)
    if bwd_fmt is not None and (N * k) % 32 == 0:
        yield ("_vrd_split_t" + f16(bwd_fmt), bwd_fmt, k - 1, Cin, N, k, k, -1, Cin * k)


def _alloc_split(R, K, fmt, device):
    """the empty SplitWeight of an (R, K) operand: planes, and in the f16 format the 4 floats of its scale"""
    f16 = fmt == _hip.PAIR_F16
    return SplitWeight(torch.empty(R, K // 32, 2, 32, device=device, dtype=torch.float16 if f16 else torch.bfloat16), fmt,
                       torch.empty(4, device=device, dtype=torch.float32) if f16 else None)


def _split_operand(w, forms):
    """the one operand of `forms` (_split_forms), from w's cache or built by a launch of its own"""
    form = next(forms, None)
    assert form is not None, "the K of a split operand (Cin*k forward, N*k input gradient) must be a multiple of 32"
    slot, fmt, offset, R, Q, taps, sr, st, sq = form

    def build():
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
        out = _alloc_split(R, taps * Q, fmt, w.device)
        _hip.check(lib.vrd_split_weight(w.data_ptr() + 4 * offset, R, Q, taps, sr, st, sq, out.data_ptr(), fmt, _ptr(out.scale), _stream()),
                   "vrd_split_weight")
        return out
    return _derived(w, slot, _version_key(w), build)


def split_conv_weight(w, fmt=None):
    """SplitWeight of the tap-major packed weight (K = Cin*k, K % 32 == 0): (N, K/32, 2, 32) 16-bit, per block of 32 K
    positions [32 x hi | 32 x lo] -- the pair-row block format of vrd_common.h, so one 128-byte line holds what a K step
    needs from a weight row -- in the current mode's element format.  Built once per weight, weight version and format."""
    return _split_operand(w, _split_forms(w.shape, pair_fmt() if fmt is None else fmt, None))


def split_conv_weight_dgrad(w, fmt=None):
    """The same operand for the input-gradient GEMM of the conv (K = N*k), straight from the parameter, in the backward
    GEMMs' element format (backward_fmt; `fmt`: the format the op's forward ran under, autograd.Linear)."""
    return _split_operand(w, _split_forms(w.shape, None, backward_fmt() if fmt is None else fmt))


# ---- all split operands of a training step in one launch
_presplit_scope = None     # token of the recording scope that is open (train_graph), None outside
_presplit_on = os.environ.get("VRDONE_PRESPLIT", "1") != "0"        # A/B switch


class presplit_scope:
    """`with ops.presplit_scope():` around the graph captures of one recording: operands that presplit_weights builds inside
    are accepted by the captures of the same scope (the backward graph reads what the forward graph's launch wrote).
    `plans` collects every plan a capture inside the scope used: the captured launches hold only raw device pointers into
    its job table, chunk tables and operand buffers, so the recording keeps this list for as long as its graphs live
    (presplit_weights drops a model's plans of other modes / replaced parameters from the model's own dict)."""

    def __enter__(self):
        global _presplit_scope
        self.plans = []
        self.prev, _presplit_scope = _presplit_scope, self
        return self

    def __exit__(self, *exc):
        global _presplit_scope
        _presplit_scope = self.prev
        return False


# what one vrd_split_weights launch needs: the job table on the device, every 32 x 32 tile's job and index within it, the jobs'
# (weight address, cache attribute, persistent SplitWeight) and their number
_SplitPlan = collections.namedtuple("_SplitPlan", "table chunk_job chunk_index outs n_jobs")


def _split_plan(weights, plans):
    """presplit_weights' plan for `weights` in the current mode, found in `plans` or built into it; None when there is nothing
    to split or when it would have to be built (and uploaded) during a graph capture."""
    fmt, bfmt = pair_fmt(), backward_fmt()
    # (the plan is keyed on the weights' addresses, shapes and the element format: another model whose parameters land on
    # the same addresses with other shapes, or a change of mode, builds its own)
    key = (fmt, bfmt) + tuple((w.data_ptr(), tuple(w.shape)) for w in weights)
    for old in [k for k in plans if k != key]:        # operands of another mode / of parameters that were replaced
        del plans[old]
    plan = plans.get(key)
    if plan is not None or _capturing():
        return plan
    jobs, outs, chunk_job, chunk_index = [], [], [], []
    for w in weights:
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 3
        for slot, jf, offset, R, Q, taps, sr, st, sq in _split_forms(w.shape, fmt, bfmt):
            out = _alloc_split(R, taps * Q, jf, w.device)
            jobs.append(_hip.SplitJob(src=w.data_ptr() + 4 * offset, out=out.data_ptr(), R=R, Q=Q, taps=taps, fmt=jf, sr=sr, st=st,
                                      sq=sq, scale=_ptr(out.scale)))
            n_tiles = -(-R // 32) * (taps * Q // 32)          # 32 x 32 tiles: row block x K block
            chunk_job.extend([len(jobs) - 1] * n_tiles)
            chunk_index.extend(range(n_tiles))
            outs.append((w.data_ptr(), slot, out))
    if not jobs:
        return None
    dev = weights[0].device
    table = torch.frombuffer(bytearray(bytes((_hip.SplitJob * len(jobs))(*jobs))), dtype=torch.uint8).to(dev)
    plan = plans[key] = _SplitPlan(table, torch.tensor(chunk_job, dtype=torch.int32, device=dev),
                                   torch.tensor(chunk_index, dtype=torch.int32, device=dev), outs, len(jobs))
    return plan


def presplit_weights(weights, plans):
    """The split-precision operands of `weights` (Conv1d parameters (N, Cin, k)) -- the forward operand where Cin*k % 32 == 0
    and the input-gradient operand where N*k % 32 == 0 -- built by ONE vrd_split_weights launch into persistent buffers and
    left in the weights' operand caches (the attributes split_conv_weight / split_conv_weight_dgrad look at) for the current
    version of each weight.  A training step otherwise
    re-splits every weight with a launch of its own, twice (after every optimiser update): 242 launches on the 24-pair batch.
    plans: a dict the caller owns (the model's): tuple of weight addresses -> _SplitPlan (job table on the device, chunk
    tables, the persistent operand buffers).  Plans of another mode or of replaced parameters are dropped from it here; a graph
    recording that captured a plan's launch keeps its own reference (presplit_scope.plans), so the buffers its replays
    read and write outlive the dict entry.
    The job table is built (and uploaded) on the first call for a set of weights -- outside any graph capture: inside one,
    without a table, nothing is done and the per-weight launches run as before."""
    if _precision not in ("bf16x3", "f16x3", "f16x1") or not weights or not _presplit_on:
        return
    plan = _split_plan(weights, plans)
    if plan is None:
        return
    scope = _presplit_scope if _capturing() else None
    if scope is not None and not any(q is plan for q in scope.plans):
        scope.plans.append(plan)
    by_ptr = {w.data_ptr(): w for w in weights}
    # nothing moved since the last call (an evaluation of the same weights, a second forward): keep the operands
    if not _capturing() and all(_entry(by_ptr[ptr], slot, _version_key(by_ptr[ptr])) is not None for ptr, slot, _ in plan.outs):
        return
    _hip.check(lib.vrd_split_weights(plan.table.data_ptr(), plan.n_jobs, plan.chunk_job.data_ptr(), plan.chunk_index.data_ptr(),
                                     plan.chunk_job.numel(), _stream()), "vrd_split_weights")
    for ptr, slot, out in plan.outs:
        setattr(by_ptr[ptr], slot, (_version_key(by_ptr[ptr]), out, scope))


def bct_to_btc(x, c0, count, out, pair=False, frames=None, index=None):
    """channels [c0, c0+count) of x (B, C, T) -> out (B, T, count-wide slab).
    frames: only the first `frames` of the T frames; index (n,) int32 device: out sequence i = x[index[i]] (n sequences)."""
    Bx, Ct, Tx = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda
    T = Tx if frames is None else frames
    B = Bx if index is None else index.numel()
    assert index is None or (index.dtype == torch.int32 and index.is_cuda and index.is_contiguous())
    p, rows, cols, ld = _rows(out)
    assert rows == B * T and cols == count and T <= Tx
    fmt = _fmt(pair)
    _hip.check(lib.vrd_bct_to_btc(x.data_ptr(), B, Ct, T, c0, count, p, ld, fmt, Tx, _ptr(index), _stream()), "vrd_bct_to_btc")
    return _as_pair(out, count, fmt)


def pair_table(feats):
    """Device pointer table + lengths of the dataloader's per-pair feature list (one upload for the whole video,
    done before any kernel is queued: a host->device copy waits for everything already queued on the GPU).
    Every feats[i] must be the (C_in, L) view of a contiguous (L, C_in) float32 matrix on the device."""
    dev = feats[0].device
    C_in = feats[0].shape[0]
    for f in feats:
        if not (f.is_cuda and f.dtype == torch.float32 and f.shape[0] == C_in and f.stride(0) == 1 and
                (f.shape[1] == 1 or f.stride(1) == C_in)):
            return None
    return (torch.tensor([f.data_ptr() for f in feats], dtype=torch.int64, device=dev),
            torch.tensor([f.shape[1] for f in feats], dtype=torch.int32, device=dev))


def _new_f32(device):
    """shape -> an uninitialised float32 buffer on `device`"""
    return lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32)


def _len_mask(lens, T, device):
    """(B, T) bool validity mask of sequences of lens[b] frames"""
    return torch.arange(T, device=device)[None, :] < lens[:, None]


def _wide_pairs(vis, clip, V, Cc, fmt):
    """the wide visual / clip buffers a batch builder filled with pair_wide = fmt, as its callers get them: Pairs when fmt;
    a buffer that was not built stays None"""
    return tuple(t if t is None else _as_pair(t, width, fmt) for t, width in ((vis, V), (clip, Cc)))


def pack_pairs(table, lens, T, V, Cc, S, E, pair_wide):
    """Batch the pairs described by `table` (B device pointers) / `lens` (B) straight into the backbone's
    channels-last operand buffers (see vrd_pack_pairs).
    Returns (vis (2B,T,V) tensor|Pair, clip or None, so_box (B,T,S), ent (2B,T,E), mask (B,T) bool)."""
    B = table.shape[0]
    dev = table.device
    assert table.dtype == torch.int64 and lens.dtype == torch.int32 and table.is_contiguous() and lens.is_contiguous()
    new = _new_f32(dev)
    vis, so_box, ent = new(2 * B, T, V), new(B, T, S), new(2 * B, T, E)
    clip = new(2 * B, T, Cc) if Cc else None
    a = _hip.PackArgs()
    a.src, a.lens = table.data_ptr(), lens.data_ptr()
    a.P, a.C_in, a.T, a.V, a.Cc, a.S, a.E = B, 2 * V + 2 * Cc + S + 2 * E, T, V, Cc, S, E
    a.vis, a.clip, a.so_box, a.ent = vis.data_ptr(), _ptr(clip), so_box.data_ptr(), ent.data_ptr()
    a.pair_wide = _fmt(pair_wide)
    _hip.check(lib.vrd_pack_pairs(C.byref(a), _stream()), "vrd_pack_pairs")
    return (*_wide_pairs(vis, clip, V, Cc, a.pair_wide), so_box, ent, _len_mask(lens, T, dev))


def gather_pairs(source, sel, T, S, E, pair_wide):
    """Batch the pairs `sel` (device int64 indices into a proposals.PairSource) straight from the per-tracklet rows into
    the backbone's operand buffers, computing the box features on the way (vrd_gather_pairs).
    Returns (vis, clip or None, so_box, ent, mask) like pack_pairs."""
    return gather_rows(source, source.s_row[sel].contiguous(), source.o_row[sel].contiguous(), source.lens_dev[sel].contiguous(),
                       T, S, E, pair_wide, seq_wh=source.pair_wh_of(sel))


def gather_rows(source, s_row, o_row, lens, T, S, E, pair_wide, boxes_only=False, seq_wh=None):
    """gather_pairs for explicit tables: sequence p = lens[p] frames starting at rows s_row[p] (subject half of the
    outputs) and o_row[p] (object half) of the source's per-tracklet arrays, stepping by the source's stride.
    boxes_only: the wide visual / clip rows are not gathered (returned as None).
    seq_wh: (B, 2) float32 device frame size per sequence (a source of several videos, PairSource.concat), else the
    source's one frame size."""
    assert S == 5 and E == 8, "the reference's box features are 5 (pair) + 8 (entity) channels (utils/misc.py:158-217)"
    B = lens.shape[0]
    dev = source.vis.device
    V, Cc = source.n_visual, source.n_clip
    assert s_row.dtype == o_row.dtype == torch.int64 and lens.dtype == torch.int32 and s_row.shape == o_row.shape == (B,)
    new = _new_f32(dev)
    so_box, ent = new(B, T, S), new(2 * B, T, E)
    vis = None if boxes_only else new(2 * B, T, V)
    clip = new(2 * B, T, Cc) if Cc and not boxes_only else None
    a = _hip.GatherArgs()
    a.vis, a.clip, a.boxes = source.vis.data_ptr(), _ptr(source.clip), source.boxes.data_ptr()
    a.s_row, a.o_row, a.lens = s_row.data_ptr(), o_row.data_ptr(), lens.data_ptr()
    a.P, a.T, a.V, a.Cc, a.stride = B, T, V, Cc, source.stride
    a.w, a.h = source.wh
    a.out_vis, a.out_clip, a.out_so_box, a.out_ent = _ptr(vis), _ptr(clip), so_box.data_ptr(), ent.data_ptr()
    a.pair_wide = _fmt(pair_wide)
    if seq_wh is not None:
        assert seq_wh.dtype == torch.float32 and seq_wh.shape == (B, 2) and seq_wh.is_contiguous() and seq_wh.device == dev
        a.seq_wh = seq_wh.data_ptr()
    _hip.check(lib.vrd_gather_pairs(C.byref(a), _stream()), "vrd_gather_pairs")
    return (*_wide_pairs(vis, clip, V, Cc, a.pair_wide), so_box, ent, _len_mask(lens, T, dev))


def train_buffers(B, T, V, Cc, S, E, device):
    """Fresh operand buffers of a B-sequence training batch, in gather_train's `out=` order: [vis (2B, T, V), so_box
    (B, T, S), ent (2B, T, E), mask (B, T) bool] + [clip (2B, T, Cc)] when Cc."""
    new = _new_f32(device)
    bufs =[new(2 * B, T, V), new(B, T, S), new(2 * B, T, E), torch.empty(B, T, device=device, dtype=torch.bool)]
    return bufs + ([new(2 * B, T, Cc)] if Cc else [])


def gather_train(source, tables, T, S, E, pair_wide, out=None):
    """The training batch of `tables` (proposals.TrainTables) from the rows of `source` (proposals.TrainSource), one launch
    (vrd_gather_train): the backbone's operand buffers at T frames -- written into `out` (train_buffers' list: a training
    graph's input buffers) when given -- and the (G, T) 0/1 target masks of all relations.
    Returns (vis, clip or None, so_box, ent, mask (B, T) bool, targets)."""
    assert S == 5 and E == 8, "the reference's box features are 5 (pair) + 8 (entity) channels (utils/misc.py:158-217)"
    B = len(tables)
    if B == 0:
        raise ValueError("gather_train: the tables hold no sequence")
    dev = source.vis.device
    V, Cc = source.n_visual, source.n_clip
    if tables.max_seq_len != T:
        raise ValueError(f"gather_train: tables made for max_seq_len {tables.max_seq_len}, batch length {T}")
    d = tables.on_device(source)
    G = d["preds"].shape[0]
    bufs = train_buffers(B, T, V, Cc, S, E, dev) if out is None else out
    vis, so_box, ent, mask = bufs[:4]
    clip = bufs[4] if Cc else None
    assert vis.shape == (2 * B, T, V) and so_box.shape == (B, T, S) and ent.shape == (2 * B, T, E) and mask.shape == (B, T)
    assert mask.dtype == torch.bool and all(t.is_contiguous() and t.device == dev for t in bufs)
    for t in (source.vis, source.clip, source.boxes):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.device == dev)
    targets = torch.empty(G, T, device=dev, dtype=torch.float32)
    a = _hip.GatherTrainArgs()
    a.vis, a.clip, a.boxes = source.vis.data_ptr(), _ptr(source.clip), source.boxes.data_ptr()
    a.s_row, a.o_row, a.lens, a.lead = d["s_row"].data_ptr(), d["o_row"].data_ptr(), d["lens"].data_ptr(), d["lead"].data_ptr()
    a.seq_wh, a.seg_lo, a.seg_hi = d["seq_wh"].data_ptr(), d["seg_lo"].data_ptr(), d["seg_hi"].data_ptr()
    a.P, a.G, a.T, a.V, a.Cc, a.stride = B, G, T, V, Cc, tables.stride
    a.out_vis, a.out_clip, a.out_so_box, a.out_ent = vis.data_ptr(), _ptr(clip), so_box.data_ptr(), ent.data_ptr()
    a.out_mask, a.out_targets = mask.data_ptr(), targets.data_ptr()
    a.pair_wide = _fmt(pair_wide)
    _hip.check(lib.vrd_gather_train(C.byref(a), _stream()), "vrd_gather_train")
    return (*_wide_pairs(vis, clip, V, Cc, a.pair_wide), so_box, ent, mask, targets)


def assemble_pairs(streams, snippets, stream_row, lens, T, piece, reach):
    """(2P, T, D) entity-stage rows of P pairs from rows computed once per tracklet (`streams`, any shape (..., D);
    stream_row (2P,) int64 = row of frame 0 of each subject then object) and the window-edge pieces `snippets`
    (4P, L, D) of `piece` frames; see vrd_assemble_args."""
    P = lens.shape[0]
    D = streams.shape[-1]
    L = snippets.shape[1]
    assert snippets.shape == (4 * P, L, D) and stream_row.shape == (2 * P,) and stream_row.dtype == torch.int64
    assert lens.dtype == torch.int32 and streams.is_contiguous() and snippets.is_contiguous()
    out = torch.empty(2 * P, T, D, device=streams.device, dtype=torch.float32)
    a = _hip.AssembleArgs()
    a.streams, a.snippets, a.stream_row, a.lens = streams.data_ptr(), snippets.data_ptr(), stream_row.data_ptr(), lens.data_ptr()
    a.P, a.T, a.D, a.L, a.piece, a.reach = P, T, D, L, piece, reach
    a.out = out.data_ptr()
    _hip.check(lib.vrd_assemble_pairs(C.byref(a), _stream()), "vrd_assemble_pairs")
    return out


def btc_to_bct(x):
    """(B, T, C) channels-last -> new (B, C, T) tensor."""
    if recording(x):
        from . import autograd
        return autograd.FromChannelsLast.apply(x)
    B, T, Cc = x.shape
    p, rows, cols, ld = _rows(x)
    out = torch.empty(B, Cc, T, device=x.device, dtype=torch.float32)
    _hip.check(lib.vrd_btc_to_bct(p, ld, B, Cc, T, out.data_ptr(), _stream()), "vrd_btc_to_bct")
    return out


def to_channels_last(x):
    """(B, C, T) -> (B, T, C)."""
    if recording(x):
        from . import autograd
        return autograd.ToChannelsLast.apply(x)
    B, Cc, T = x.shape
    out = torch.empty(B, T, Cc, device=x.device, dtype=torch.float32)
    return bct_to_btc(x.contiguous(), 0, Cc, out)


_skip_padding = os.environ.get("VRDONE_SKIP_PADDING", "1") != "0"
SKIP_MIN_ROWS = 65536        # below this the 256 x 256 GEMM kernel (the one that takes the block list) is not used


def row_blocks(mask):
    """Padding map of a (B, T) validity mask for vrd_gemm: (order, n_active per segment, segment length) -- two device
    int32 tensors made by vrd_row_blocks -- or None when the rows do not split into aligned 32-row blocks.  Cached on
    the mask tensor object (keyed on its address and version counter), so it dies with it."""
    def build():
        rows = mask.numel()
        if not (rows % 32 == 0 and mask.is_contiguous() and mask.data_ptr() % 16 == 0 and mask.dtype in (torch.bool, torch.uint8)):
            return None
        # about eight segments (one per XCD of the GEMM's tile order), each a whole number of 256-row tiles
        nblk = rows // 32
        seg_len = 8 * (((nblk + 7) // 8 + 7) // 8)
        order = torch.empty(nblk, device=mask.device, dtype=torch.int32)
        count = torch.empty((nblk + seg_len - 1) // seg_len, device=mask.device, dtype=torch.int32)
        _hip.check(lib.vrd_row_blocks(mask.data_ptr(), rows, seg_len, order.data_ptr(), count.data_ptr(), _stream()),
                   "vrd_row_blocks")
        return order, count, seg_len
    return _derived(mask, "_vrd_row_blocks", _version_key(mask), build)


def _gemm_struct(x, N, Cin, k, W, split, bias=None, act=ACT_NONE, row_mask=None, scale=None, res=None, res_masked=False, res2=None,
                 out=None, out_pair=False, skip_rows=None):
    """(vrd_gemm_args, result) of one GEMM problem: the rows of x (tensor or Pair, Cin channels) against an (N, k*Cin) tap-major
    operand -- `W` its f32 form (None: there is none), `split` its SplitWeight (None: exact f32 products) -- with conv_gemm's
    epilogue.  Nothing is launched."""
    x, a_width = _unwrap(x)
    pa, rows, cols, lda = _rows(x)
    assert cols == Cin, f"input has {cols} channels, weight expects {Cin}"
    T = x.shape[-2]
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
    pc, rows_c, cols_c, ldc = _rows(out)
    assert rows_c == rows and cols_c == N
    a = _hip.GemmArgs()
    # (the split-precision kernels do not read the f32 weight pointer: without an f32 form it points at the split operand)
    a.W = split.data_ptr() if W is None else _param_ptr(W, x, "conv weight")
    if split is not None:
        split.set_args(a)
    a.A, a.lda, a.bias = pa, lda, _param_ptr(bias, x, "conv bias")
    a.C, a.ldc = pc, ldc
    a.M, a.N, a.Cin, a.taps, a.T = rows, N, Cin, k, T
    a.act = act
    a.row_mask = _mask_ptr(row_mask, rows)
    a.scale = _param_ptr(scale, x, "drop-path scale")
    a.a_pair_width = a_width
    a.c_pair = _fmt(out_pair)
    if skip_rows is None:
        skip_rows = row_mask
    # (the kernels that take the block list: the 256 x 256 split kernel -- pair-row input -- and the exact-f32 kernel)
    f32_kernel = not a_width and split is None
    if _skip_padding and skip_rows is not None and (a_width or f32_kernel) and rows >= SKIP_MIN_ROWS and skip_rows.numel() == rows:
        blocks = row_blocks(skip_rows)
        if blocks is not None:
            a.row_blocks, a.row_blocks_active = blocks[0].data_ptr(), blocks[1].data_ptr()
            a.row_block_seg_len = blocks[2]
    if res is not None:
        pr, rr, rc, ldr = _rows(res)
        assert rr == rows and rc == N
        a.res, a.ldres, a.res_masked = pr, ldr, 1 if res_masked else 0
    if res2 is not None:
        pr, rr, rc, ldr = _rows(res2)
        assert rr == rows and rc == N
        a.res2, a.ldres2 = pr, ldr
    return a, _as_pair(out, N, a.c_pair)


def gemm_args(x, weight, bias=None, *, act=ACT_NONE, row_mask=None, scale=None, res=None, res_masked=False, res2=None, out=None,
              out_pair=False, skip_rows=None, split_fmt=None):
    """(a, result): the vrd_gemm_args of conv_gemm(x, weight, bias, ...) without autograd and the tensor or Pair its launch will
    have written.  Nothing is launched: launch_gemm(a) does that, gemm_family(a) names the kernel family it runs on."""
    N, Cin, k = weight.shape
    x_fmt, a_width = (x.fmt, x.width) if isinstance(x, Pair) else (0, 0)
    if a_width:
        assert pair_fmt() and x_fmt == pair_fmt() and Cin % 32 == 0, "pair input needs the split-precision mode it was made in and Cin % 32 == 0"
    w_fmt = pair_fmt() if split_fmt is None else split_fmt
    assert not (a_width and w_fmt != x_fmt) and not (out_pair and w_fmt != pair_fmt())
    split = split_conv_weight(weight, w_fmt) if w_fmt and (Cin * k) % 32 == 0 else None
    a, result = _gemm_struct(x, N, Cin, k, packed_conv_weight(weight), split, bias, act, row_mask, scale, res, res_masked, res2, out,
                             out_pair, skip_rows)
    if split is not None and w_fmt == _hip.PAIR_F16 and split_fmt is None:
        a.products = products()
    return a, result


def gemm_family(a):
    """The kernel family (_hip.K_GEMM* = enum vrd_kernel_id) the library runs the vrd_gemm_args `a` on (vrd_gemm_family)."""
    fam = lib.vrd_gemm_family(C.byref(a))
    if fam < 0:
        _hip.check(fam, "vrd_gemm_family")
    return fam


def launch_gemm(a):
    _hip.check(lib.vrd_gemm(C.byref(a), _stream()), "vrd_gemm")


def conv_gemm(x, weight, bias=None, *, act=ACT_NONE, row_mask=None, scale=None, res=None, res_masked=False,
              res2=None, out=None, out_pair=False, skip_rows=None, row_scale=None, split_fmt=None, drop=None):
    """Dense Conv1d (k = 1 or 3, stride 1, zero padding k//2) with the fused epilogue of
    vrd_gemm.  x: (B, T, Cin) tensor or Pair; weight: the Conv1d parameter (N, Cin, k).
    out_pair: write the result as pair rows of width N (returns a Pair).
    skip_rows: validity mask of the rows; aligned 32-row blocks without a valid row skip the contraction (exact with
    row_mask, which is then the default; without row_mask those rows hold bias-only filler, so pass it only where
    no valid row ever reads a padded one: projections feeding masked attention, an MLP's hidden layer).
    row_scale (rows,): per-row factor on the branch term (stochastic depth, blocks.py:1107-1120); autograd path only.
    drop: a training step's dropout call (models.blocks.Drop) on the activated GEMM output, before scale / residuals (proj_drop and
    the MLP dropouts, blocks.py:988,1057,1059); autograd path only.
    split_fmt: element format of the split products instead of the mode's (the unfused backward GEMMs pass PAIR_BF16; 0 = exact
    f32 products whatever the mode, None = the mode's format).
    Under autograd (`recording`) the op runs as autograd.conv_gemm and returns a fresh tensor (`out` is ignored)."""
    # row_scale (stochastic depth, sampled whenever the model trains) lives in the autograd form's epilogue: it goes there even
    # when nothing of this call needs a gradient (a frozen sub-module under requires_grad_(False), reference blocks.py:1107-1120
    # drops paths regardless)
    if not isinstance(x, Pair) and (recording(x, weight, bias, scale, res, res2) or row_scale is not None or drop is not None):
        from . import autograd
        assert not out_pair
        return autograd.conv_gemm(x, weight, bias, act=act, row_mask=row_mask, scale=scale, row_scale=row_scale, res=res,
                                  res_masked=res_masked, res2=res2, drop=drop)
    assert row_scale is None, "row_scale (drop-path sampling) exists for plain f32 rows only"
    assert drop is None, "dropout exists for plain f32 rows only"
    a, result = gemm_args(x, weight, bias, act=act, row_mask=row_mask, scale=scale, res=res, res_masked=res_masked, res2=res2, out=out,
                          out_pair=out_pair, skip_rows=skip_rows, split_fmt=split_fmt)
    launch_gemm(a)
    return result


def dgrad_args(dy, weight, *, row_mask=None, a_scale=None, fmt=None, out=None):
    """(a, dx): the vrd_gemm_args of conv_dgrad(dy, weight, ...) and the tensor its launch will have written (`out`, or a new
    one).  Nothing is launched (as gemm_args)."""
    N, Cin, k = weight.shape
    assert (N * k) % 32 == 0 and not isinstance(dy, Pair)
    wt = split_conv_weight_dgrad(weight, fmt)
    a, dx = _gemm_struct(dy, Cin, N, k, None, wt, row_mask=row_mask, out=out)
    if wt.fmt == _hip.PAIR_F16:      # dy is a gradient: its f16 planes need its own power-of-two factor
        assert a_scale is not None
        a.a_scale = a_scale.data_ptr()
    return a, dx


def conv_dgrad(dy, weight, *, row_mask=None, a_scale=None, fmt=None, out=None):
    """The conv's input gradient as a GEMM on the parameter's transposed operand (split_conv_weight_dgrad, format `fmt`): the
    weight (N, Cin, k) acts as the (Cin, N, k) tap-flipped conv on the f32 rows of the gradient dy (N channels).  Split-precision
    only (autograd.Linear checks).  a_scale: in the f16 format the rows of dy are split at the power-of-two factor of
    grad_scale(dy) (vrd_gemm_args.a_scale)."""
    a, dx = dgrad_args(dy, weight, row_mask=row_mask, a_scale=a_scale, fmt=fmt, out=out)
    launch_gemm(a)
    return dx


def split_forward(x, weight, bias=None, **kwargs):
    """True when conv_gemm(x, weight, ...) runs a split-precision GEMM kernel in the current mode, False when it lands on the
    exact-f32 kernel: the library's own answer for the arguments conv_gemm builds (vrd_gemm_family), nothing is launched.  In the
    f16 modes only the split kernels check f32 rows against the operand range (tag 16 of f16_range_flag)."""
    return gemm_family(gemm_args(x, weight, bias, **kwargs)[0]) != _hip.K_GEMM


def conv_gemm_batch(calls):
    """Several conv_gemm calls -- [(args, kwargs), ...], at most 4 -- handed to the library together (vrd_gemm_batch):
    GEMMs that differ only in input, weight, bias and output, like the q / k / v projections of an attention block, run
    as one launch.  Returns the list of results."""
    assert 1 <= len(calls) <= 4
    if torch.is_grad_enabled():         # differentiable path: one op per projection
        return [conv_gemm(*args, **kwargs) for args, kwargs in calls]
    collected, results = zip(*(gemm_args(*args, **kwargs) for args, kwargs in calls))
    _hip.check(lib.vrd_gemm_batch((_hip.GemmArgs * len(collected))(*collected), len(collected), _stream()), "vrd_gemm_batch")
    return list(results)


def layernorm(x, gamma, beta, *, relu=False, post_add=None, out=None, pair=False):
    """Channel LayerNorm.  post_add: (period, C) rows added after the affine, row r gets
    post_add[r % period].  pair: write pair rows (returns a Pair)."""
    if recording(x, gamma, beta, post_add):
        from . import autograd
        assert not pair
        return autograd.layernorm(x, gamma, beta, relu=relu, post_add=post_add)
    px, rows, cols, ldx = _rows(x)
    if out is None:
        out = torch.empty(*x.shape, device=x.device, dtype=torch.float32)
    py, rows_y, cols_y, ldy = _rows(out)
    assert rows_y == rows and cols_y == cols
    pa, lda, period = None, 0, 0
    if post_add is not None:
        pa, period, ca, lda = _rows(post_add)
        assert ca == cols
    assert gamma.numel() == cols and beta.numel() == cols
    _hip.check(lib.vrd_layernorm(px, ldx, py, ldy, rows, cols, _param_ptr(gamma, x, "LayerNorm weight"),
                                 _param_ptr(beta, x, "LayerNorm bias"), 1 if relu else 0,
                                 pa, lda, period, _fmt(pair), _stream()), "vrd_layernorm")
    return _as_pair(out, cols, _fmt(pair))


def _pos_args(table, first, mask, rows, cols, segs, T):
    """the (pos_table, ld_pos, pos_rows, pos_first, mask, segs, T) arguments of vrd_layernorm_pos / vrd_position_rows for a launch
    over `rows` rows: segs = [(first row, sequences, frames)] or None for rows / T sequences of T rows"""
    pt, n_pos, c_pos, ld_pos = _rows(table)
    assert c_pos == cols, f"position table of {c_pos} channels for rows of {cols}"
    if segs is None:
        seqs, seg_table = rows // T, None
    else:
        seqs, seg_table, T = sum(n for _, n, _ in segs), C.pointer(_hip.RowSegs.of(segs)), 0
    if not first.is_cuda or first.dtype != torch.int32 or not first.is_contiguous() or first.numel() != seqs:
        raise ValueError(f"pos_first must be a contiguous int32 HIP tensor with one entry per sequence ({first.numel()} vs {seqs})")
    return pt, ld_pos, n_pos, first.data_ptr(), _mask_ptr(mask, rows), seg_table, T


def layernorm_pos(x, gamma, beta, table, first, mask, *, T=None, segs=None, relu=False, out=None, pair=False):
    """layernorm() with absolute position rows from per-sequence tables in place of post_add (vrd_layernorm_pos; inference only):
    sequence s, frame t gets table[first[s] + t] where mask is set.  table: (rows of all tables, C) f32; first: int32 per sequence,
    on the device; mask: one byte per row of x.  The rows of x are sequences of T frames, or the groups `segs` = [(first row,
    sequences, frames)] (rows outside the groups are left alone).  Same bits as layernorm() with the materialised rows as post_add."""
    assert not recording(x, gamma, beta), "per-sequence position tables are an inference form: training adds the periodic post_add rows"
    px, rows, cols, ldx = _rows(x)
    if out is None:
        out = torch.empty(*x.shape, device=x.device, dtype=torch.float32)
    py, rows_y, cols_y, ldy = _rows(out)
    assert rows_y == rows and cols_y == cols and gamma.numel() == cols and beta.numel() == cols
    _hip.check(lib.vrd_layernorm_pos(px, ldx, py, ldy, rows, cols, _param_ptr(gamma, x, "LayerNorm weight"),
                                     _param_ptr(beta, x, "LayerNorm bias"), 1 if relu else 0,
                                     *_pos_args(table, first, mask, rows, cols, segs, T if T is not None else x.shape[-2]),
                                     _fmt(pair), _stream()), "vrd_layernorm_pos")
    return _as_pair(out, cols, _fmt(pair))


def position_rows(table, first, mask, *, T=None, segs=None, out=None, pair=False):
    """The masked position rows layernorm_pos() adds, on their own (vrd_position_rows): (rows of mask, C) f32 or pair rows.
    out: the buffer (required with `segs` that leave rows out: those rows keep what they hold)."""
    cols = table.shape[-1]
    if out is None:
        out = torch.empty(*mask.shape, cols, device=table.device, dtype=torch.float32)
    py, rows, cols_y, ldy = _rows(out)
    assert cols_y == cols
    _hip.check(lib.vrd_position_rows(py, ldy, rows, cols, *_pos_args(table, first, mask, rows, cols, segs,
                                                                     T if T is not None else mask.shape[-1]),
                                     _fmt(pair), _stream()), "vrd_position_rows")
    return _as_pair(out, cols, _fmt(pair))


CONV_LN_MAXK = 32
_conv_ln_on = os.environ.get("VRDONE_CONV_LN", "1") != "0"


def conv_ln_ok(x, weight, *tensors):
    """The fused few-channel conv -> LayerNorm row kernel takes this call: inference, f32 rows, taps * Cin <= 32, 256 / 512 outputs."""
    N, Cin, k = weight.shape
    return (_conv_ln_on and not isinstance(x, Pair) and k in (1, 3) and Cin * k <= CONV_LN_MAXK and (3 + k) * Cin <= 64 and N in (256, 512) and
            not recording(x, weight, *tensors))


def conv_ln(x, weight, bias, *, row_mask=None, gamma=None, beta=None, relu=False, out=None, pair=False):
    """Dense Conv1d with few input channels (k = 1 or 3, zero padding k // 2) * row_mask -> [LayerNorm(gamma, beta)] -> [ReLU] as one
    row kernel (vrd_conv_ln): the box-feature embeddings.  x: (B, T, Cin) f32 rows; out: (B, T, N) buffer or column slab of one;
    pair: write pair rows (returns a Pair)."""
    N, Cin, k = weight.shape
    px, rows, cols, ldx = _rows(x)
    assert cols == Cin and weight.is_contiguous()
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
    py, rows_y, cols_y, ldy = _rows(out)
    assert rows_y == rows and cols_y == N
    a = _hip.ConvLnArgs()
    a.x, a.ldx, a.rows = px, ldx, rows
    a.Cin, a.taps, a.T, a.N = Cin, k, x.shape[-2], N
    a.w, a.bias = _param_ptr(weight, x, "conv weight"), _param_ptr(bias, x, "conv bias")
    a.row_mask = _mask_ptr(row_mask, rows)
    a.gamma, a.beta = _param_ptr(gamma, x, "LayerNorm weight"), _param_ptr(beta, x, "LayerNorm bias")
    a.relu = 1 if relu else 0
    a.y, a.ldy, a.out_pair = py, ldy, _fmt(pair)
    _hip.check(lib.vrd_conv_ln(C.byref(a), _stream()), "vrd_conv_ln")
    return _as_pair(out, N, a.out_pair)


_CONST_ROWS = {}


def _const_row(n, fill, device):
    """A constant vector (the stand-in of an absent bias / LayerNorm affine in a parameter image), made once per size: in a
    training step the images are rebuilt for every weight, which was ~170 fill launches per step."""
    key = (n, float(fill), str(device))
    t = _CONST_ROWS.get(key)
    if t is None:
        t = _CONST_ROWS[key] = torch.full((n,), fill, device=device, dtype=torch.float32)
    return t


def _dwconv_block(w, bias, gamma, beta):
    """The on-chip parameter image of one dwconv_ln set (vrd_dwconv_ln_args.packed): taps tap-major | bias | gamma |
    beta.  Cached on the weight, keyed on the (address, version) of all four tensors."""
    parts = (w, bias, gamma, beta)
    key = tuple(_version_key(t) if t is not None else None for t in parts)
    Cout, g, k = w.shape
    one = lambda t, fill: _const_row(Cout, fill, w.device) if t is None else t.detach().float().reshape(-1)  # noqa: E731
    return _derived(w, "_vrd_dw_block", key, lambda: torch.cat(
        [w.detach().float().permute(1, 2, 0).reshape(-1), one(bias, 0.0), one(gamma, 1.0), one(beta, 0.0)]).contiguous())


def dwconv_ln(x, sets, *, mask_out=None, stride=1, x_up=None, pre_ln=None, segs=None):
    """Fused depthwise conv * mask -> LayerNorm for up to three weight sets sharing x.
    sets: list of dicts(weight=(C, g, k) Conv1d weight, bias=None, gamma=None, beta=None, relu=False, out=None).
    pre_ln = (gamma, beta): the input rows are LayerNorm'ed as they are read (the block's ln1).
    segs: x is a ragged row space (1, R, C) -- [(first row, sequences, frames)] groups of sequences back to
    back (vrd_row_segs); outputs, mask_out and x_up follow the same grouping at their own frame counts.
    Returns the list of outputs, each (B, T/stride, C)."""
    if recording(x, x_up, *(t for st in sets for t in (st["weight"], st.get("bias"), st.get("gamma"), st.get("beta"))),
                 *(pre_ln or ())):
        from . import autograd
        return autograd.dwconv_ln(x, sets, mask_out=mask_out, stride=stride, x_up=x_up, pre_ln=pre_ln, segs=segs)
    B, Tin, Cx = x.shape
    w0 = sets[0]["weight"]
    Cout, g, k = w0.shape
    px, rows, cols, ldx = _rows(x)
    assert cols == Cout * g
    Tout = Tin // stride
    a = _hip.DwconvLnArgs()
    seg_table = None
    if segs is not None:
        assert B == 1 and sum(n * T for _, n, T in segs) == Tin
        seg_table = _hip.RowSegs.of(segs)
        a.segs = C.pointer(seg_table)
    a.x, a.ldx = px, ldx
    if x_up is not None:
        pu, ru, cu, ldu = _rows(x_up)
        assert cu == cols and ru * 2 == rows
        a.x_up, a.ldx_up = pu, ldu
    a.B, a.Tin, a.C, a.ksize, a.stride, a.group_in = B, Tin, Cout, k, stride, g
    if pre_ln is not None:
        assert g == 1 and x_up is None
        a.pre_gamma, a.pre_beta = _param_ptr(pre_ln[0], x, "LayerNorm weight"), _param_ptr(pre_ln[1], x, "LayerNorm bias")
    a.mask_out = _mask_ptr(mask_out, B * Tout)
    a.n_out = len(sets)
    outs, blocks = [], []
    for i, s in enumerate(sets):
        assert tuple(s["weight"].shape) == (Cout, g, k) and s["weight"].is_contiguous()
        o = s.get("out")
        if o is None:
            o = torch.empty(B, Tout, Cout, device=x.device, dtype=torch.float32)
        po, ro, co, ldo = _rows(o)
        assert ro == B * Tout and co == Cout
        a.w[i], a.bias[i] = _param_ptr(s["weight"], x, "depthwise weight"), _param_ptr(s.get("bias"), x, "depthwise bias")
        a.gamma[i], a.beta[i] = (_param_ptr(s.get("gamma"), x, "LayerNorm weight"),
                                 _param_ptr(s.get("beta"), x, "LayerNorm bias"))
        # (held until the launch is queued: one weight tensor in two sets with different LayerNorm parameters replaces its own
        # cache entry, and the first set's image would be freed, and its memory handed out again, before the kernel reads it)
        blocks.append(_dwconv_block(s["weight"], s.get("bias"), s.get("gamma"), s.get("beta")))
        a.packed[i] = blocks[-1].data_ptr()
        a.relu[i] = 1 if s.get("relu") else 0
        a.y[i], a.ldy[i] = po, ldo
        a.out_pair[i] = _fmt(s.get("pair"))
        outs.append(_as_pair(o, Cout, a.out_pair[i]))
    _hip.check(lib.vrd_dwconv_ln(C.byref(a), _stream()), "vrd_dwconv_ln")
    return outs


def dwconv_ln_multi(x, sets, *, mask_out=None, pre_ln=None, segs=None):
    """dwconv_ln for up to five 512-channel k = 3 sets over one stream, read once (vrd_dwconv_ln_multi; inference only).  A set
    with normed=True reads the rows behind the input LayerNorm pre_ln = (gamma, beta), the others read them as they are; the other
    keys of a set and `segs` are dwconv_ln's.  Every output has the bits of the dwconv_ln launch with that set and input form."""
    assert not recording(x, *(t for st in sets for t in (st["weight"], st.get("bias"), st.get("gamma"), st.get("beta"))),
                         *(pre_ln or ())), "the multi-set pass has no backward: training takes dwconv_ln"
    B, Tin, Cx = x.shape
    px, rows, cols, ldx = _rows(x)
    a = _hip.DwconvLnMultiArgs()
    if segs is not None:
        assert B == 1 and sum(n * T for _, n, T in segs) == Tin
        a.segs = C.pointer(_hip.RowSegs.of(segs))
    a.x, a.ldx, a.B, a.Tin, a.C = px, ldx, B, Tin, cols
    a.mask_out = _mask_ptr(mask_out, B * Tin)
    a.n_out = len(sets)
    if any(s.get("normed") for s in sets):
        a.pre_gamma, a.pre_beta = _param_ptr(pre_ln[0], x, "LayerNorm weight"), _param_ptr(pre_ln[1], x, "LayerNorm bias")
    outs, blocks = [], []
    for i, s in enumerate(sets[:_hip.DWCONV_MULTI_SETS]):
        assert tuple(s["weight"].shape) == (cols, 1, 3) and (s.get("gamma") is None) == (s.get("beta") is None)
        o = s.get("out")
        if o is None:
            o = torch.empty(B, Tin, cols, device=x.device, dtype=torch.float32)
        po, ro, co, ldo = _rows(o)
        assert ro == B * Tin and co == cols
        _param_ptr(s["weight"], x, "depthwise weight")          # (the checks only: the kernel reads the set's image)
        blocks.append(_dwconv_block(s["weight"], s.get("bias"), s.get("gamma"), s.get("beta")))      # (held until the launch is queued)
        a.packed[i] = blocks[-1].data_ptr()
        a.has_ln[i], a.relu[i], a.pre_ln[i] = int(s.get("gamma") is not None), int(bool(s.get("relu"))), int(bool(s.get("normed")))
        a.y[i], a.ldy[i], a.out_pair[i] = po, ldo, _fmt(s.get("pair"))
        outs.append(_as_pair(o, cols, a.out_pair[i]))
    _hip.check(lib.vrd_dwconv_ln_multi(C.byref(a), _stream()), "vrd_dwconv_ln_multi")
    return outs


def _rel_pe_ptr(rel_pe, like, n_head, half_win):
    if rel_pe is None:
        return None
    assert rel_pe.numel() == n_head * (2 * half_win + 1) and rel_pe.dtype == torch.float32 and rel_pe.is_contiguous()
    assert rel_pe.device == like.device
    return rel_pe.data_ptr()


def local_attention(q, k, v, mask, n_head, half_win, pair=False, rel_pe=None, out=None, segs=None, drop=None):
    """rel_pe: None or the module's (1, 1, n_head, window) relative position bias (reference blocks.py:739-743).
    out: (B, T, C) contiguous rows to write instead of a fresh tensor (inference path).
    segs: q / k / v / mask are a ragged row space (1, R, ...): [(first row, sequences, frames)] (vrd_row_segs).
    half_win: window // 2 of an odd window from 3 to 19.
    drop (training): the attn_drop call (models.blocks.Drop: seed tensor, site, first row's number, rate) -- dropout on the window
    probabilities; such a call runs as autograd.LocalAttention whether or not an input needs a gradient (it drops regardless)."""
    if not (isinstance(half_win, int) and 1 <= half_win <= 9):
        raise ValueError(f"local_attention: the window must be odd, from 3 to 19 (half_win = window // 2 an integer from 1 to 9), "
                         f"got half_win {half_win!r}")
    width = q.shape[-1]
    if not (width in (256, 512) and isinstance(n_head, int) and n_head > 0 and width % n_head == 0 and width // n_head in (32, 64, 128)):
        raise ValueError(f"local_attention: built for width 256 or 512 with head_dim = width / n_head of 32, 64 or 128 "
                         f"(16, 8 or 4 heads at 512; 8, 4 or 2 at 256), got width {width}, n_head {n_head!r}")
    if recording(q, k, v, rel_pe) or drop is not None:
        from . import autograd
        assert drop is None or (segs is None and not pair)
        return autograd.LocalAttention.apply(q, k, v, mask, n_head, half_win, rel_pe, drop, segs)
    B, T, Cc = q.shape
    rel = _rel_pe_ptr(rel_pe, q, n_head, half_win)
    pq, rows, cols, ld = _rows(q)
    pk, _, _, ldk = _rows(k)
    pv, _, _, ldv = _rows(v)
    assert ld == ldk == ldv
    if out is None:
        out = torch.empty(B, T, Cc, device=q.device, dtype=torch.float32)
    assert out.shape == (B, T, Cc) and out.is_contiguous()
    if segs is not None:
        assert B == 1 and sum(n * t for _, n, t in segs) == T
        table = _hip.RowSegs.of(segs)
        _hip.check(lib.vrd_local_attn_segs(pq, pk, pv, ld, _mask_ptr(mask, rows), rel, C.byref(table), Cc, n_head, half_win,
                                           out.data_ptr(), Cc, _fmt(pair), _stream()), "vrd_local_attn_segs")
        return _as_pair(out, Cc, _fmt(pair))
    _hip.check(lib.vrd_local_attn(pq, pk, pv, ld, _mask_ptr(mask, rows), rel, B, T, Cc, n_head, half_win,
                                  out.data_ptr(), Cc, _fmt(pair), _stream()), "vrd_local_attn")
    return _as_pair(out, Cc, _fmt(pair))


def attention(q, k, v, kv_mask, n_head, algo=0, pair=False, q_mask=None, out=None, segs=None):
    """Global masked attention; q: (B, Tq, C), k/v: (B, Tk, C); kv_mask (B, Tk) or None.
    out: (B, Tq, C) contiguous rows to write instead of a fresh tensor (inference path).
    pair: pair-row output when the flash kernel runs (otherwise a plain tensor is returned).
    q_mask (B, Tq): rows the caller masks afterwards; the split-precision kernel leaves out query tiles without a valid
    row (they read 0).
    segs (inference path, pair-row operands only): (qsegs, ksegs) -- q / q_mask / out are a ragged row space (1, Rq, ...) of the
    groups qsegs = [(first row, sequences, frames)], k / v / kv_mask one of ksegs (vrd_row_segs; the same sequences per group on
    both sides): every group's attention in one call (vrd_attention_pair_segs), bit for bit the group-by-group calls."""
    if not isinstance(q, Pair) and recording(q, k, v):
        # (with segs: f32 rows under autograd, every group on the entry points of the batch form -- autograd.Attention)
        from . import autograd
        return autograd.Attention.apply(q, k, v, kv_mask, n_head, segs)
    if segs is not None:
        return _attention_segs(q, k, v, kv_mask, n_head, pair, q_mask, out, *segs)
    fmt, (B, Tq, Cc), (_, Tk, _), pq, ldq, pk, pv, ldk, rows_k, out = _qkv_rows(q, k, v, out)
    if fmt:
        out_fmt = fmt if pair else 0
        _hip.check(lib.vrd_attention_pair(pq, ldq, pk, pv, ldk, _mask_ptr(kv_mask, rows_k), _mask_ptr(q_mask, B * Tq), B, Tq, Tk, n_head,
                                          Cc // n_head, out.data_ptr(), Cc, out_fmt, fmt, _stream(),
                                          products() if fmt == _hip.PAIR_F16 else 0),
                   "vrd_attention_pair")
        return _as_pair(out, Cc, out_fmt)
    hd = Cc // n_head
    flash = algo == 2 or (algo == 0 and hd in (64, 128))      # mirrors vrd_attention's auto choice
    out_fmt = _fmt(pair and flash)
    _hip.check(lib.vrd_attention(pq, ldq, pk, pv, ldk, _mask_ptr(kv_mask, rows_k), B, Tq, Tk, n_head, hd,
                                 out.data_ptr(), Cc, algo, out_fmt, _stream()), "vrd_attention")
    return _as_pair(out, Cc, out_fmt)


def _qkv_rows(q, k, v, out):
    """The operands of a global attention call, all three Pairs of one format and full width or all three f32 rows:
    (fmt -- 0 for f32 rows --, q's shape, k's shape, q's address and leading dimension, k's and v's addresses and their common
    leading dimension, k's row count, out: the contiguous rows of q's shape to write, fresh unless given)."""
    fmt = 0
    if isinstance(q, Pair):
        assert isinstance(k, Pair) and isinstance(v, Pair) and q.width == k.width == v.width == q.shape[-1]
        assert q.fmt == k.fmt == v.fmt
        fmt = q.fmt
        q, k, v = q.t, k.t, v.t
    pq, _, _, ldq = _rows(q)
    pk, rows_k, _, ldk = _rows(k)
    pv, _, _, ldv = _rows(v)
    assert ldk == ldv
    if out is None:
        out = torch.empty(q.shape, device=q.device, dtype=torch.float32)
    assert out.shape == q.shape and out.is_contiguous()
    return fmt, q.shape, k.shape, pq, ldq, pk, pv, ldk, rows_k, out


def _attention_segs(q, k, v, kv_mask, n_head, pair, q_mask, out, qsegs, ksegs):
    if not (isinstance(q, Pair) and isinstance(k, Pair) and isinstance(v, Pair)):
        raise TypeError("attention(segs=...): the row groups of one call exist for pair-row operands only (the split-precision "
                        "flash kernel); f32 rows go group by group")
    fmt, (B, Rq, Cc), k_shape, pq, ldq, pk, pv, ldk, rows_k, out = _qkv_rows(q, k, v, out)
    qsegs, ksegs = list(qsegs), list(ksegs)
    assert len(qsegs) == len(ksegs) >= 1 and all(a[1] == b[1] for a, b in zip(qsegs, ksegs))
    Rk = k_shape[1]
    assert B == 1 and k_shape[0] == 1 and v.shape == k_shape
    assert all(0 <= off and off + n * T <= Rq for off, n, T in qsegs) and all(0 <= off and off + n * T <= Rk for off, n, T in ksegs)
    out_fmt = fmt if pair else 0
    for g0 in range(0, len(qsegs), _hip.MAX_SEGS):              # a call takes MAX_SEGS groups: consecutive runs of them
        tq, tk = _hip.RowSegs.of(qsegs[g0:g0 + _hip.MAX_SEGS]), _hip.RowSegs.of(ksegs[g0:g0 + _hip.MAX_SEGS])
        _hip.check(lib.vrd_attention_pair_segs(pq, ldq, pk, pv, ldk, _mask_ptr(kv_mask, rows_k), _mask_ptr(q_mask, Rq), C.byref(tq),
                                               C.byref(tk), n_head, Cc // n_head, out.data_ptr(), Cc, out_fmt, fmt,
                                               _stream(), products() if fmt == _hip.PAIR_F16 else 0),
                   "vrd_attention_pair_segs")
    return _as_pair(out, Cc, out_fmt)


def maxpool_mask(x, mask_in, out=None, segs=None):
    """MaxPool1d(3, 2, 1)(x) * mask[::2]; returns (pooled (B, T/2, C), mask_out (B, T/2) bool).
    out: (pooled, mask_out) contiguous buffers to write instead of fresh tensors (inference path).
    segs (autograd path): x (1, R, C) / mask_in (1, R) are a ragged row space of the groups [(first row, sequences, frames)]."""
    if recording(x):
        from . import autograd
        return autograd.MaxPoolMask.apply(x, mask_in, segs)
    assert segs is None, "maxpool_mask(segs=...) is the autograd form; inference walks the groups (models/ragged.py)"
    B, T, Cc = x.shape
    px, rows, cols, ldx = _rows(x)
    if out is None:
        y = torch.empty(B, T // 2, Cc, device=x.device, dtype=torch.float32)
        m_out = torch.empty(B, T // 2, device=x.device, dtype=torch.bool)
    else:
        y, m_out = out
        assert y.shape == (B, T // 2, Cc) and y.is_contiguous() and m_out.shape == (B, T // 2) and m_out.is_contiguous()
        assert m_out.dtype == torch.bool
    _hip.check(lib.vrd_maxpool_mask(px, ldx, B, T, Cc, _mask_ptr(mask_in, rows), y.data_ptr(), Cc, m_out.data_ptr(),
                                    _stream()), "vrd_maxpool_mask")
    return y, m_out


def mask_head(emb, feat, out_mask, fill=-10.0, segs=None):
    """emb (B, Q, Dp), feat (B, T, Dp), out_mask (B, T) -> (B, Q, T).
    segs (autograd path): feat (1, R, Dp) / out_mask (1, R) are a ragged row space of the groups [(first row, sequences, frames)],
    emb their sequences in order -> one (n_i, Q, T_i) tensor per group."""
    if recording(emb, feat):
        from . import autograd
        return autograd.MaskHead.apply(emb, feat, out_mask, fill, segs)
    assert segs is None, "mask_head(segs=...) is the autograd form; inference walks the groups (models/ragged.py)"
    B, Q, Dp = emb.shape
    T = feat.shape[1]
    pe, _, _, lde = _rows(emb)
    pf, rows_f, _, ldf = _rows(feat)
    seg = torch.empty(B, Q, T, device=emb.device, dtype=torch.float32)
    _hip.check(lib.vrd_mask_head(pe, lde, pf, ldf, _mask_ptr(out_mask, rows_f), B, Q, T, Dp, fill, seg.data_ptr(),
                                 _stream()), "vrd_mask_head")
    return seg


def assign_tables(sizes, dev):
    """(first row, relation count) of every pair as device int32 tensors: what vrd_assign walks."""
    first, at = [], 0
    for n in sizes:
        first.append(at)
        at += n
    return torch.tensor(first, dtype=torch.int32, device=dev), torch.tensor(sizes, dtype=torch.int32, device=dev)


def assign(cost, sizes, tables=None, wave=False):
    """Minimum-cost assignment of every pair's relations to its queries on the device (vrd_assign): cost (sum N, Q) f32,
    rows grouped pair by pair, sizes = [N_p] (each <= Q <= 64); tables = assign_tables(sizes, device) when the caller
    assigns several cost matrices of the same batch.  Returns the query of every relation, (sum N,) int32.
    Up to 16 queries one thread solves a pair, above that one wave (vrd_assign_wave); wave=True asks for the wave form at
    any Q -- the two follow one pivoting rule and agree on every input."""
    assert cost.is_cuda and cost.dtype == torch.float32 and cost.dim() == 2 and cost.stride(1) == 1
    G, Q = cost.shape
    assert sum(sizes) == G and max(sizes) <= Q <= 64
    first_d, count_d = tables if tables is not None else assign_tables(sizes, cost.device)
    out = torch.full((G,), -1, dtype=torch.int32, device=cost.device)
    fn, name = (lib.vrd_assign_wave, "vrd_assign_wave") if wave else (lib.vrd_assign, "vrd_assign")
    _hip.check(fn(cost.data_ptr(), cost.stride(0), first_d.data_ptr(), count_d.data_ptr(), len(sizes), Q, out.data_ptr(), _stream()), name)
    return out


def postprocess(logits, masks, valid_len, topk):
    """logits (P, Q, K1), masks (P, Q, T), valid_len (P,) int32 ->
    (top_score (P,Q,k) f32, top_cat (P,Q,k) i32, seg_first (P,Q) i32, seg_last (P,Q) i32)."""
    P, Q, K1 = logits.shape
    T = masks.shape[-1]
    assert logits.is_contiguous() and masks.is_contiguous() and valid_len.dtype == torch.int32
    dev = logits.device
    ts = torch.empty(P, Q, topk, device=dev, dtype=torch.float32)
    tc = torch.empty(P, Q, topk, device=dev, dtype=torch.int32)
    sf = torch.empty(P, Q, device=dev, dtype=torch.int32)
    sl = torch.empty(P, Q, device=dev, dtype=torch.int32)
    _hip.check(lib.vrd_postprocess(logits.data_ptr(), masks.data_ptr(), valid_len.data_ptr(), P, Q, K1, T, topk,
                                   ts.data_ptr(), tc.data_ptr(), sf.data_ptr(), sl.data_ptr(), _stream()),
               "vrd_postprocess")
    return ts, tc, sf, sl


def select_triplets(cand, s_score, o_score, so_offset, so_start, so_end, video_pairs, feat_stride, pred_min_frames, n_max_pair,
                    max_video_pairs):
    """forward_test's candidate filter + top-n_max_pair selection for several videos in one launch (vrd_select_triplets).
    cand (P_total, Q, 2k + 2) f32 candidate records; s_score / o_score (P_total,) f32; so_offset / so_start / so_end
    (P_total,) int32; video_pairs (n_videos + 1,) int32 pair offsets -- all on the device.  Returns (count (n_videos, 2) int32
    = [selected, out-of-range kept candidates], index (n_videos, n_max_pair) int32 flat candidate index within the video
    (-1 padded), score (n_videos, n_max_pair) f32)."""
    P, Q, W = cand.shape
    k = (W - 2) // 2
    n_videos = video_pairs.shape[0] - 1
    assert cand.is_contiguous() and cand.dtype == torch.float32 and W == 2 * k + 2 and n_videos >= 1
    for t in (s_score, o_score):
        assert t.dtype == torch.float32 and t.shape == (P,) and t.is_contiguous()
    for t in (so_offset, so_start, so_end):
        assert t.dtype == torch.int32 and t.shape == (P,) and t.is_contiguous()
    assert video_pairs.dtype == torch.int32 and video_pairs.is_contiguous()
    dev = cand.device
    count = torch.empty(n_videos, 2, device=dev, dtype=torch.int32)
    index = torch.empty(n_videos, n_max_pair, device=dev, dtype=torch.int32)
    score = torch.empty(n_videos, n_max_pair, device=dev, dtype=torch.float32)
    a = _hip.SelectArgs()
    a.cand, a.s_score, a.o_score = cand.data_ptr(), s_score.data_ptr(), o_score.data_ptr()
    a.so_offset, a.so_start, a.so_end, a.video_pairs = so_offset.data_ptr(), so_start.data_ptr(), so_end.data_ptr(), video_pairs.data_ptr()
    a.n_videos, a.max_video_pairs, a.Q, a.k = n_videos, max_video_pairs, Q, k
    a.feat_stride, a.pred_min_frames, a.n_max_pair = feat_stride, pred_min_frames, n_max_pair
    a.out_count, a.out_index, a.out_score = count.data_ptr(), index.data_ptr(), score.data_ptr()
    _hip.check(lib.vrd_select_triplets(C.byref(a), _stream()), "vrd_select_triplets")
    return count, index, score


def relation_viou(pred_boxes, pred, gt_boxes, gt, cand):
    """ov (n_cand,) float64 = min(subject vIoU, object vIoU) of every (prediction, ground truth) candidate (vrd_relation_viou):
    evaluate.viou's formula in f64, one wave per candidate.  pred_boxes / gt_boxes: (rows, 4) f32 flat box arrays; pred / gt:
    (n, 4) int64 relation tables [subject's first row, object's first row, first frame, frames]; cand: (n_cand, 2) int32
    [prediction, ground truth] -- all contiguous, on the device."""
    for t in (pred_boxes, gt_boxes):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 4 and t.is_contiguous()
    for t in (pred, gt):
        assert t.dtype == torch.int64 and t.dim() == 2 and t.shape[1] == 4 and t.is_contiguous()
    assert cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[1] == 2 and cand.is_contiguous()
    # (the kernel reads a box as one 16-byte load; a view that starts off that alignment is copied)
    pred_boxes, gt_boxes = (t.clone() if t.data_ptr() % 16 else t for t in (pred_boxes, gt_boxes))
    ov = torch.empty(cand.shape[0], device=cand.device, dtype=torch.float64)
    a = _hip.ViouArgs()
    a.pred_boxes, a.pred_rows, a.gt_boxes, a.gt_rows = pred_boxes.data_ptr(), pred_boxes.shape[0], gt_boxes.data_ptr(), gt_boxes.shape[0]
    a.pred, a.gt, a.cand = pred.data_ptr(), gt.data_ptr(), cand.data_ptr()
    a.n_pred, a.n_gt, a.n_cand, a.ov = pred.shape[0], gt.shape[0], cand.shape[0], ov.data_ptr()
    _hip.check(lib.vrd_relation_viou(C.byref(a), _stream()), "vrd_relation_viou")
    return ov


def match_relations(pred_first, cand_first, cand, ov, n_gt, threshold):
    """hit (n_pred,) int32: eval_detection_scores' greedy matching for every video of the call in one launch
    (vrd_match_relations).  pred_first (n_videos + 1,) int32: video v owns predictions pred_first[v] .. pred_first[v + 1] - 1,
    in scoring order; cand_first (n_pred + 1,) int32: prediction p owns candidates cand_first[p] .. cand_first[p + 1] - 1, in
    ascending ground-truth index; cand (n_cand, 2) int32; ov (n_cand,) float64; n_gt: rows of the ground-truth table.
    hit[p] = the matched ground truth, -1 for a miss."""
    for t in (pred_first, cand_first):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.shape[0] >= 1 and t.is_contiguous()
    assert cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[1] == 2 and cand.is_contiguous()
    assert ov.dtype == torch.float64 and ov.shape == (cand.shape[0],) and ov.is_contiguous()
    dev = pred_first.device
    n_pred = cand_first.shape[0] - 1
    hit = torch.full((n_pred,), -1, device=dev, dtype=torch.int32)
    detected = torch.empty(n_gt, device=dev, dtype=torch.uint8)
    a = _hip.MatchArgs()
    a.pred_first, a.cand_first, a.cand, a.ov = pred_first.data_ptr(), cand_first.data_ptr(), cand.data_ptr(), ov.data_ptr()
    a.n_videos, a.n_pred, a.n_cand, a.n_gt = pred_first.shape[0] - 1, n_pred, cand.shape[0], n_gt
    a.threshold, a.detected, a.hit = float(threshold), detected.data_ptr(), hit.data_ptr()
    _hip.check(lib.vrd_match_relations(C.byref(a), _stream()), "vrd_match_relations")
    return hit


# ---- eval proposals (csrc/vrd_proposals.hip): what vrdone_amd.proposals.prepare_test_videos launches
_PROPOSAL_TABLES = (   # field of vrd_proposal_args -> (dtype, elements as a function of the counts)
    ("boxes", torch.float32, lambda n: 4 * n["rows"]), ("trk", torch.int64, lambda n: 5 * n["trk"]),
    ("video_max", torch.float32, lambda n: 2 * n["videos"]), ("trk_first", torch.int32, lambda n: n["videos"] + 1),
    ("tri_first", torch.int64, lambda n: n["videos"] + 1), ("cand_first", torch.int64, lambda n: n["videos"] + 1),
    ("cand_s", torch.int32, lambda n: n["cand"]), ("cand_o", torch.int32, lambda n: n["cand"]),
    ("stride_offset", torch.int32, lambda n: n["videos"]), ("trk_err", torch.uint8, lambda n: n["trk"]),
    ("shadow", torch.uint8, lambda n: n["tri"]), ("dropped", torch.uint8, lambda n: n["trk"]),
    ("s_row", torch.int64, lambda n: n["cand"]), ("o_row", torch.int64, lambda n: n["cand"]),
    ("lens", torch.int32, lambda n: n["cand"]), ("kept_s", torch.int32, lambda n: n["cand"]),
    ("kept_o", torch.int32, lambda n: n["cand"]), ("count", torch.int32, lambda n: n["videos"]),
    ("video_err", torch.int32, lambda n: n["videos"]))


def proposal_args(tables, feat_stride, min_frames, threshold):
    """vrd_proposal_args over `tables`: {field: contiguous device tensor} for every pointer of the struct (include/vrdone_hip.h).
    The counts come from the tensors -- videos from trk_first, tracklets from trk (n, 5), tracklet pairs from shadow, candidates
    from cand_s, box rows from boxes (rows, 4) -- and every other table must hold exactly what they ask for."""
    n = {"videos": tables["trk_first"].numel() - 1, "trk": tables["trk"].shape[0], "tri": tables["shadow"].numel(),
         "cand": tables["cand_s"].numel(), "rows": tables["boxes"].shape[0]}
    dev = tables["boxes"].device
    a = _hip.ProposalArgs()
    for name, dtype, size in _PROPOSAL_TABLES:
        t = tables[name]
        if not t.is_cuda or t.device != dev:
            raise RuntimeError("vrdone_amd ops need HIP tensors (no CPU path exists for the hot path)")
        if t.dtype != dtype or not t.is_contiguous() or t.numel() != size(n):
            raise ValueError(f"proposal_args: {name} must be a contiguous {dtype} tensor of {size(n)} elements, "
                             f"got {t.dtype} {tuple(t.shape)}")
        setattr(a, name, t.data_ptr())
    a.rows, a.n_videos, a.n_trk, a.n_tri, a.n_cand = n["rows"], n["videos"], n["trk"], n["tri"], n["cand"]
    a.feat_stride, a.min_frames, a.threshold = int(feat_stride), int(min_frames), float(threshold)
    return a


def proposal_clamp(a):
    """Clamp every tracklet's boxes to its video's frame, in place; trk_err says where a box came out empty (vrd_proposal_clamp)."""
    _hip.check(lib.vrd_proposal_clamp(C.byref(a), _stream()), "vrd_proposal_clamp")


def proposal_shadow(a):
    """One byte per same-video tracklet pair i < j: bit 0 "i shadows j", bit 1 "j shadows i" (vrd_proposal_shadow)."""
    _hip.check(lib.vrd_proposal_shadow(C.byref(a), _stream()), "vrd_proposal_shadow")


def proposal_walk(a):
    """The reference's greedy de-dup walk over the shadow bytes: dropped (n_trk,), video_err (n_videos,) (vrd_proposal_walk)."""
    _hip.check(lib.vrd_proposal_walk(C.byref(a), _stream()), "vrd_proposal_walk")


def proposal_pairs(a):
    """The pair tables of every video: kept candidates compacted to the front of each video's slice (vrd_proposal_pairs)."""
    _hip.check(lib.vrd_proposal_pairs(C.byref(a), _stream()), "vrd_proposal_pairs")
