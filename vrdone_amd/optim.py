"""Gradient-norm clipping and AdamW as three kernel launches (csrc/vrd_optim.hip).

The reference's step (train.py:185-194) runs `torch.nn.utils.clip_grad_norm_` and `torch.optim.AdamW.step` between the
backward and the EMA update: a Python walk over the ~520 parameters and chunked `_foreach_*` launches.  Here

    opt = FusedAdamW(param_groups, lr=...)            # instead of torch.optim.AdamW(...)
    opt.step(max_grad_norm=clip)                      # instead of clip_grad_norm_(...); opt.step()

runs `vrd_grad_sumsq` -> `vrd_grad_norm_finish` -> `vrd_adamw_step` over tables of device pointers, like `ModelEma.update`
does with `vrd_ema_update`.  `FusedAdamW` IS a `torch.optim.AdamW`: same constructor, `param_groups` and per-parameter state
(`step`, `exp_avg`, `exp_avg_sq`), so checkpoints interchange with torch's in both directions and LR schedulers work on it
unchanged.  `clip_grad_norm_` below is the standalone clip (torch's signature; launches 1, 2 and `vrd_scale_tensors`).

What the kernels do not cover takes torch's own implementation, for the whole step: a parameter or gradient that is not a
contiguous f32 tensor on one HIP device, amsgrad / maximize / capturable / differentiable / fused=True, tensor-valued lr or
betas.  Nothing here synchronises with the host.
"""
import torch

from . import _hip
from .ops import _stream

_CHUNK = 4096                       # elements per workgroup (OPT_CHUNK of csrc/vrd_optim.hip)
_ROW = _hip.ADAMW_GROUP_FLOATS


def build_chunk_map(numels, present=None):
    """(chunk_tensor, chunk_index): chunk c of a launch is elements chunk_index[c] * 4096 ... of tensor chunk_tensor[c].  Tensors
    without elements, and those whose `present` entry is false (no gradient this step), get no chunk."""
    chunk_tensor, chunk_index = [], []
    for t, n in enumerate(numels):
        if present is not None and not present[t]:
            continue
        c = -(-n // _CHUNK)
        chunk_tensor += [t] * c
        chunk_index += range(c)
    return chunk_tensor, chunk_index


def adamw_row(lr, weight_decay, beta1, beta2, eps, step):
    """One row of vrd_adamw_step's hyper-parameter table, in double (the scalars of torch's non-capturable update,
    torch/optim/adam.py); the upload rounds them to f32 like torch's kernels round their scalar arguments."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return [lr * weight_decay, beta1, beta2, eps, lr / bias_correction1, bias_correction2 ** 0.5, 1 - beta1, 1 - beta2]


def _on_kernel(t):
    return t.dtype == torch.float32 and t.is_cuda and t.layout == torch.strided and t.is_contiguous()


class _Tables:
    """Device tables of one set of tensors: what never changes while the set stands (numel, chunk map, the norm's partial sums)
    and one int64 buffer for what a call uploads (gradient pointers, float4 flags, hyper-parameter rows), filled from pinned
    host memory in ONE asynchronous copy.  A pinned buffer is reused only once its last copy has left it (an event per buffer,
    polled -- never waited for)."""

    def __init__(self, numels, present, device, extra_words=0):
        self.n, self.device = len(numels), device
        chunk_tensor, chunk_index = build_chunk_map(numels, present)
        self.n_chunks = len(chunk_tensor)
        self.numel = torch.tensor(numels, dtype=torch.int64, device=device)
        self.chunk_tensor = torch.tensor(chunk_tensor, dtype=torch.int32, device=device)
        self.chunk_index = torch.tensor(chunk_index, dtype=torch.int32, device=device)
        self.partial = torch.empty(max(self.n_chunks, 1), dtype=torch.float64, device=device)
        self.vec_at = self.n                                   # word offsets into the upload: [grad pointers | vec | extra]
        self.extra_at = self.vec_at + (self.n + 1) // 2
        self.words = self.extra_at + extra_words
        self.dev = torch.empty(self.words, dtype=torch.int64, device=device)
        self.grad_ptr = self.dev.data_ptr()
        self.vec_ptr = self.grad_ptr + 8 * self.vec_at
        self.extra_ptr = self.grad_ptr + 8 * self.extra_at
        self._ring = []

    def upload(self, grad_ptrs, vec, extra=None):
        for host, event in self._ring:
            if event.query():
                break
        else:
            host, event = torch.empty(self.words, dtype=torch.int64, pin_memory=True), torch.cuda.Event()
            self._ring.append((host, event))
        host[:self.n] = torch.tensor(grad_ptrs, dtype=torch.int64)
        host[self.vec_at:self.extra_at].view(torch.int32)[:self.n] = torch.tensor(vec, dtype=torch.int32)
        if extra is not None:
            rows = torch.tensor(extra, dtype=torch.float32).flatten()
            host[self.extra_at:].view(torch.float32)[:rows.numel()] = rows
        self.dev.copy_(host, non_blocking=True)
        event.record()

    def grad_norm(self, max_norm):
        """launches 1 and 2: -> device tensor [total_norm, clip_coef]"""
        out = torch.empty(2, dtype=torch.float32, device=self.device)
        s = _stream()
        _hip.check(_hip.lib.vrd_grad_sumsq(self.grad_ptr, self.numel.data_ptr(), self.vec_ptr, self.chunk_tensor.data_ptr(),
                                           self.chunk_index.data_ptr(), self.n_chunks, self.partial.data_ptr(), s), "vrd_grad_sumsq")
        _hip.check(_hip.lib.vrd_grad_norm_finish(self.partial.data_ptr(), self.n_chunks, float(max_norm), out.data_ptr(), s),
                   "vrd_grad_norm_finish")
        return out


_clip_tables = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ (train.py:187-188) as three launches: the gradients are scaled in place by
    min(1, max_norm / (total_norm + 1e-6)) and the total 2-norm comes back as a device tensor.  Other norm types,
    error_if_nonfinite, a non-positive max_norm and gradients the kernels do not cover go to torch's function."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm = float(max_norm)
    if (not grads or float(norm_type) != 2.0 or error_if_nonfinite or not max_norm > 0 or not all(_on_kernel(g) for g in grads)
            or any(g.device != grads[0].device for g in grads)):
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    numels = tuple(g.numel() for g in grads)
    if not any(numels):
        return torch.zeros((), device=grads[0].device)
    with torch.cuda.device(grads[0].device):
        key = (grads[0].device, numels)
        tables = _clip_tables.get(key)
        if tables is None:
            if len(_clip_tables) >= 8:
                _clip_tables.clear()
            tables = _clip_tables[key] = _Tables(numels, None, grads[0].device)
        ptrs = [g.data_ptr() for g in grads]
        tables.upload(ptrs, [ptr & 15 == 0 for ptr in ptrs])
        out = tables.grad_norm(max_norm)
        _hip.check(_hip.lib.vrd_scale_tensors(tables.grad_ptr, tables.numel.data_ptr(), tables.vec_ptr, tables.chunk_tensor.data_ptr(),
                                              tables.chunk_index.data_ptr(), tables.n_chunks, out.data_ptr() + 4, _stream()),
                   "vrd_scale_tensors")
    torch.autograd.graph.increment_version(grads)
    return out[0]


class _Plan:
    """What FusedAdamW keeps between steps while no parameter moved and the same parameters have gradients."""
    pass


class FusedAdamW(torch.optim.AdamW):
    """torch.optim.AdamW whose `step` is one kernel launch over all parameters (three with `max_grad_norm`).

    `step(max_grad_norm=c)` folds `clip_grad_norm_(parameters, c)` into the update: the gradients stay unscaled, the update
    uses g * clip_coef, and `last_grad_norm` holds the total norm (a device tensor; None when the step did not ask for one).
    A non-positive `max_grad_norm` measures the norm without clipping.  State tensors are the ones torch creates, at the
    moment torch creates them (a parameter's first step with a gradient), so `state_dict()` is a torch.optim.AdamW
    checkpoint.  The device tables are rebuilt when a parameter moved, the set of parameters with a gradient changed, or
    the state was replaced (`load_state_dict`, `add_param_group`); code that swaps state tensors by hand calls
    `invalidate()`."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._plan = None
        self.last_grad_norm = None

    def invalidate(self):
        self._plan = None

    def load_state_dict(self, state_dict):
        self._plan = None
        return super().load_state_dict(state_dict)

    def add_param_group(self, param_group):
        self._plan = None
        return super().add_param_group(param_group)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plan = None
        self.__dict__.setdefault("last_grad_norm", None)

    @staticmethod
    def _group_on_kernel(group):
        if group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"] or group.get("fused"):
            return False
        scalars = (group["lr"], group["weight_decay"], group["eps"]) + tuple(group["betas"])
        return not any(isinstance(v, torch.Tensor) for v in scalars)

    def _torch_step(self, max_grad_norm):
        """the whole step through torch's implementation"""
        self._plan = None
        self.last_grad_norm = None
        if max_grad_norm is not None:
            params = [p for group in self.param_groups for p in group["params"]]
            if max_grad_norm > 0:
                self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
            else:
                self.last_grad_norm = torch.nn.utils.get_total_norm([p.grad for p in params if p.grad is not None])
        super().step()

    def _build_plan(self, params, groups_of, key, device):
        plan = _Plan()
        plan.key = key
        present = [k != 0 for k in key]
        plan.params = [p for p, on in zip(params, present) if on]
        rows, row_of, ptr = {}, [], {"p": [], "m": [], "v": []}
        plan.steps = []
        for p, gi, on in zip(params, groups_of, present):
            if not on:
                row_of.append(0)
                for v in ptr.values():
                    v.append(0)
                continue
            state = self.state[p]
            if len(state) == 0:                    # torch's lazy initialisation (Adam._init_group), non-capturable form
                state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = state["exp_avg"], state["exp_avg_sq"]
            if not (_on_kernel(m) and _on_kernel(v) and m.device == device and v.device == device and m.numel() == p.numel()
                    and v.numel() == p.numel() and isinstance(state["step"], torch.Tensor)):
                return None
            plan.steps.append(state["step"])
            row_of.append(rows.setdefault((gi, float(state["step"])), len(rows)))
            ptr["p"].append(p.data_ptr()), ptr["m"].append(m.data_ptr()), ptr["v"].append(v.data_ptr())
        plan.rows = list(rows)                                         # [(group index, steps taken so far)]
        plan.align = [a | b | c for a, b, c in zip(ptr["p"], ptr["m"], ptr["v"])]
        plan.tables = _Tables([p.numel() for p in params], present, device, extra_words=len(rows) * _ROW // 2)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=device)      # noqa: E731
        plan.param, plan.exp_avg, plan.exp_avg_sq = i64(ptr["p"]), i64(ptr["m"]), i64(ptr["v"])
        plan.row_of = torch.tensor(row_of, dtype=torch.int32, device=device)
        return plan

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
        if not all(self._group_on_kernel(g) for g in self.param_groups):
            self._torch_step(max_grad_norm)
            return loss
        params, groups_of = [], []
        for gi, group in enumerate(self.param_groups):
            params += group["params"]
            groups_of += [gi] * len(group["params"])
        # one walk: which parameters have a gradient, where it lives, and whether the kernels cover it
        key, grad_ptrs, device = [], [], None
        for p in params:
            g = p.grad
            if g is None:
                key.append(0), grad_ptrs.append(0)
                continue
            if device is None:
                device = p.device
            if not (_on_kernel(p) and _on_kernel(g) and p.device == device and g.device == device and g.numel() == p.numel()):
                self._torch_step(max_grad_norm)
                return loss
            key.append(p.data_ptr() or -1), grad_ptrs.append(g.data_ptr())           # (an empty tensor's pointer is 0)
        self.last_grad_norm = None
        if device is None:                                                      # no gradient anywhere: torch's step does nothing
            return loss
        key = tuple(key)
        with torch.cuda.device(device):
            plan = self._plan
            if plan is None or plan.key != key:
                plan = self._plan = self._build_plan(params, groups_of, key, device)
                if plan is None:
                    self._torch_step(max_grad_norm)
                    return loss
            t = plan.tables
            torch._foreach_add_(plan.steps, 1)
            plan.rows = [(gi, n + 1) for gi, n in plan.rows]
            hyper = []
            for gi, n in plan.rows:
                group = self.param_groups[gi]
                hyper.append(adamw_row(group["lr"], group["weight_decay"], group["betas"][0], group["betas"][1], group["eps"], n))
            if t.n_chunks == 0:                                                 # gradients without elements only
                if max_grad_norm is not None:
                    self.last_grad_norm = torch.zeros((), device=device)
                return loss
            t.upload(grad_ptrs, [(a | g) & 15 == 0 for a, g in zip(plan.align, grad_ptrs)], hyper)
            coef = 0
            if max_grad_norm is not None:
                out = t.grad_norm(max_grad_norm)
                self.last_grad_norm, coef = out[0], out.data_ptr() + 4
            _hip.check(_hip.lib.vrd_adamw_step(plan.param.data_ptr(), t.grad_ptr, plan.exp_avg.data_ptr(), plan.exp_avg_sq.data_ptr(),
                                               t.numel.data_ptr(), plan.row_of.data_ptr(), t.vec_ptr, t.extra_ptr, len(plan.rows),
                                               t.chunk_tensor.data_ptr(), t.chunk_index.data_ptr(), t.n_chunks, coef or None, _stream()),
                       "vrd_adamw_step")
        # The kernel wrote through raw pointers: tell autograd's version counters, as ModelEma.update does.  ops caches split and
        # packed weights on the parameters keyed on (data_ptr, _version); without the bump the next forward reuses stale ones.
        torch.autograd.graph.increment_version(plan.params)
        return loss
