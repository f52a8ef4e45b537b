"""vrdone_amd.optim on the GPU: gradient-norm clip + AdamW as three launches (csrc/vrd_optim.hip) against torch's own
clip_grad_norm_ + AdamW, on a synthetic parameter set that meets every path of the kernels -- one element, fewer than a float4,
one short of a chunk, exactly a chunk, one past it, three chunks with a tail, 18 chunks; a parameter that is a view one float
into its storage and a gradient that is one (the scalar form, decided per tensor and per step); a parameter without a
gradient; two groups with different lr and weight decay; gradient magnitudes from 1e-4 to 1e2.

The accuracy bound is the project's (test_reference_grade_against_float64): the error against a float64 run of the same
update, over all elements, is at most twice the error torch's own f32 update makes against it.

Measured on an MI355X (max error against float64 over all elements after four steps, fused / torch-f32; clipped | not clipped):
    param 7.28e-7 / 7.28e-7 = 1.00 | 7.92e-7 / 7.92e-7 = 1.00      exp_avg 3.07e-10 / 3.12e-10 = 0.98 | 9.29e-6 / 6.83e-6 = 1.36
    exp_avg_sq 7.29e-14 / 6.00e-14 = 1.21 | 3.74e-5 / 4.45e-5 = 0.84
    total norm (2.64e4 .. 2.66e4), steps 0 .. 3: fused 9.6e-4, 9.7e-4, 5.2e-4, 2.6e-4; torch-f32 9.6e-4, 9.9e-4, 1.4e-3, 1.7e-3"""
import os

import pytest
import torch

from conftest import REPO, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUMELS = [1, 3, 4095, 4096, 4097, 8193, 70000, 100]              # the last one never gets a gradient
SCALES = [1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0]
PARAM_VIEW, GRAD_VIEW = 4, 5                                      # numel 4097: the parameter is a view at +4 bytes; 8193: the gradient
CLIPPED, UNCLIPPED = 1.0, 1e9                                     # max_norm below / above every total norm of these gradients
STEPS = 4


@pytest.fixture(autouse=True)
def _autograd_on():
    """Other GPU test modules switch autograd off globally at import; the model tests here need it recording."""
    with torch.enable_grad():
        yield


def _offset_view(values):
    base = torch.empty(values.numel() + 1, dtype=values.dtype, device=DEV)
    base[1:] = values
    return base[1:]


def make_params(dtype=torch.float32, order=None, pad=0):
    """The synthetic set on the device; `order` / `pad`: allocate in another order with spacers in between (other addresses)."""
    g = torch.Generator().manual_seed(1)
    values = [torch.randn(n, generator=g) for n in NUMELS]
    params, spacers = [None] * len(values), []
    for i in (order or range(len(values))):
        if pad:
            spacers.append(torch.empty(pad * (i + 1), device=DEV))
        v = values[i].to(device=DEV, dtype=dtype)
        params[i] = torch.nn.Parameter(_offset_view(v) if i == PARAM_VIEW else v)
    assert params[PARAM_VIEW].data_ptr() % 16 == (4 if dtype == torch.float32 else 8) and params[PARAM_VIEW].is_contiguous()
    return params


def groups(params):
    return [{"params": params[0::2], "weight_decay": 0.05, "lr": 1e-3}, {"params": params[1::2], "weight_decay": 0.0, "lr": 3e-4}]


def set_grads(params, step, poison=None):
    g = torch.Generator().manual_seed(100 + step)
    for i, scale in enumerate(SCALES):
        grad = torch.randn(NUMELS[i], generator=g) * scale
        if poison is not None and i == poison[0]:
            grad[poison[1]] = float("inf")
        grad = grad.to(device=DEV, dtype=params[i].dtype)
        params[i].grad = _offset_view(grad) if i == GRAD_VIEW else grad
    assert params[-1].grad is None


def state_of(opt, params, key):
    return [opt.state[p][key] if key else p.detach() for p in params[:-1]]


def torch_run(dtype, max_norm, steps=STEPS, poison=None):
    params = make_params(dtype)
    opt = torch.optim.AdamW(groups(params), foreach=False)
    norms = []
    for step in range(steps):
        set_grads(params, step, poison)
        norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm).double().cpu())
        opt.step()
    return params, opt, norms


def fused_run(max_norm, steps=STEPS, poison=None, **kw):
    from vrdone_amd.optim import FusedAdamW
    params = make_params(**kw)
    opt = FusedAdamW(groups(params))
    norms = []
    for step in range(steps):
        set_grads(params, step, poison)
        opt.step(max_grad_norm=max_norm)
        norms.append(opt.last_grad_norm.double().cpu() if max_norm is not None else None)
    return params, opt, norms


_refs = {}


def references(max_norm):
    """torch's f32 and float64 runs of the same four steps, computed once per max_norm and left unchanged"""
    if max_norm not in _refs:
        _refs[max_norm] = (torch_run(torch.float32, max_norm), torch_run(torch.float64, max_norm))
    return _refs[max_norm]


def max_err(tensors, ref64):
    return max(float((a.double() - b).abs().max()) for a, b in zip(tensors, ref64))


def bits_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("max_norm", [CLIPPED, UNCLIPPED])
def test_update_is_as_close_to_float64_as_torchs(max_norm):
    (p32, o32, n32), (p64, o64, n64) = references(max_norm)
    pf, of, nf = fused_run(max_norm)
    assert all((float(n) > max_norm) == (max_norm == CLIPPED) for n in n64)            # the case is what its name says
    for key in (None, "exp_avg", "exp_avg_sq"):
        ref = state_of(o64, p64, key)
        e_fused, e_torch = max_err(state_of(of, pf, key), ref), max_err(state_of(o32, p32, key), ref)
        print(f"max_norm {max_norm:g} {key or 'param'}: fused {e_fused:.3e} torch-f32 {e_torch:.3e} ratio {e_fused / max(e_torch, 1e-300):.2f}")
        assert e_torch > 0 and e_fused <= 2 * e_torch, (key, e_fused, e_torch)
    for step in range(STEPS):
        e_fused, e_torch = abs(float(nf[step] - n64[step])), abs(float(n32[step] - n64[step]))
        print(f"max_norm {max_norm:g} step {step} total norm {float(n64[step]):.6e}: fused {e_fused:.3e} torch-f32 {e_torch:.3e}")
        assert e_fused <= 2 * e_torch, (step, e_fused, e_torch)
    for p in pf[:-1]:                                                                    # the folded clip leaves the gradients alone
        assert p.grad is not None
    assert len(of.state[pf[0]]) == 3 and float(of.state[pf[0]]["step"]) == STEPS and pf[-1] not in of.state
    untouched = make_params()[-1]
    assert torch.equal(pf[-1].detach(), untouched.detach())                              # no gradient: not touched


def test_folded_clip_equals_clip_then_step_bit_for_bit():
    from vrdone_amd.optim import FusedAdamW, clip_grad_norm_
    pa, oa, na = fused_run(CLIPPED)
    pb = make_params()
    ob = FusedAdamW(groups(pb))
    for step in range(STEPS):
        set_grads(pb, step)
        before = [p.grad.clone() for p in pb[:-1]]
        norm = clip_grad_norm_(pb, CLIPPED)
        assert torch.equal(norm.double().cpu(), na[step])
        coef = torch.tensor(CLIPPED) / (norm.cpu() + 1e-6)
        for p, g in zip(pb, before):                                                     # scaled in place, by torch's coefficient
            assert torch.allclose(p.grad, g * float(coef), rtol=1e-6, atol=0)
        ob.step()
    for key in (None, "exp_avg", "exp_avg_sq"):
        assert bits_equal(state_of(oa, pa, key), state_of(ob, pb, key)), key


def test_norm_below_max_norm_gives_coefficient_one():
    from vrdone_amd.optim import clip_grad_norm_
    pa, oa, _ = fused_run(UNCLIPPED)
    pb, ob, _ = fused_run(None)
    for key in (None, "exp_avg", "exp_avg_sq"):
        assert bits_equal(state_of(oa, pa, key), state_of(ob, pb, key)), key         # g * coef == g for every g: coef == 1
    ps = make_params()
    set_grads(ps, 0)
    before = [p.grad.clone() for p in ps[:-1]]
    norm = clip_grad_norm_(ps, UNCLIPPED)
    want = torch.nn.utils.get_total_norm([g.double() for g in before])
    assert abs(float(norm) - float(want)) <= 1e-6 * float(want)
    assert bits_equal([p.grad for p in ps[:-1]], before)


def test_same_inputs_at_other_addresses_give_the_same_bits():
    pa, oa, na = fused_run(CLIPPED)
    pb, ob, nb = fused_run(CLIPPED, order=list(reversed(range(len(NUMELS)))), pad=1031)
    assert [p.data_ptr() for p in pa] != [p.data_ptr() for p in pb]
    assert all(torch.equal(a, b) for a, b in zip(na, nb))
    for key in (None, "exp_avg", "exp_avg_sq"):
        assert bits_equal(state_of(oa, pa, key), state_of(ob, pb, key)), key


def test_launch_count_is_three_with_a_norm_and_one_without():
    from vrdone_amd import _hip
    from vrdone_amd.optim import FusedAdamW
    params = make_params()
    opt = FusedAdamW(groups(params))
    counts = []
    for step, max_norm in enumerate((CLIPPED, None, CLIPPED, None)):
        set_grads(params, step)
        _hip.prof_enable(True)
        _hip.prof_reset()
        opt.step(max_grad_norm=max_norm)
        torch.cuda.synchronize()
        prof = _hip.prof_read()
        _hip.prof_enable(False)
        counts.append(prof["backward"]["launches"])
        assert sum(v["launches"] for v in prof.values()) == counts[-1]
        assert (opt.last_grad_norm is None) == (max_norm is None)
    assert counts == [3, 1, 3, 1]


def test_one_infinite_gradient_gives_torchs_pattern_of_non_finite_parameters():
    poison = (3, 17)
    p32, _, n32 = torch_run(torch.float32, CLIPPED, steps=2, poison=poison)
    pf, _, nf = fused_run(CLIPPED, steps=2, poison=poison)
    assert all(torch.isinf(n) for n in nf) and all(torch.isinf(n) for n in n32)
    total = 0
    for a, b in zip(pf, p32):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))
        total += int((~torch.isfinite(a)).sum())
    assert total == 1 and not bool(torch.isfinite(pf[poison[0]][poison[1]]))


def test_forward_after_a_fused_step_sees_the_new_weights():
    """The update writes the parameters through raw pointers.  ops caches split and packed weights on the parameter objects
    keyed on their version counters: a forward AFTER a step has to equal a fresh model loaded from the stepped state_dict()
    (the form of test_ema_module_forward_follows_its_updates)."""
    from golden_cases import train_batch
    from oracle import vrd_oracle as O
    from vrdone_amd.models.maskvrd import MaskVRD
    from vrdone_amd.optim import FusedAdamW
    mc, _, keys = load_case("vidvrd")
    cc = mc["clip_dim"] if mc.get("with_clip_feature", False) else 0
    model = MaskVRD(mc, device=DEV)
    model.load_state_dict(O.synth_state_dict(keys, eos_coef=mc["loss_coeff_dict"]["eos_coef"]), strict=True)
    model = model.to(DEV)
    _, x, m, data = train_batch(mc, 2 * mc["visual_dim"] + 2 * cc + mc["bbox_so_dim"] + 2 * mc["bbox_entity_dim"], device=DEV)
    x, m = x.to(DEV), m.to(DEV)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    model.eval()
    with torch.no_grad():
        before = model._mask_vrd(x, m, with_aux=False)["pred_logits"].clone()          # fills the derived-operand caches
    model.train()
    model(data)["total_loss"].backward()
    opt.step(max_grad_norm=1.0)
    model.eval()
    with torch.no_grad():
        after = model._mask_vrd(x, m, with_aux=False)["pred_logits"]
        fresh = MaskVRD(mc, device=DEV).to(DEV).eval()
        fresh.load_state_dict(model.state_dict())
        want = fresh._mask_vrd(x, m, with_aux=False)["pred_logits"]
    assert bool(torch.isfinite(opt.last_grad_norm)) and float((after - before).abs().max()) > 1e-3
    assert torch.equal(after, want)


def _train_step():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_step", os.path.join(REPO, "scripts", "train_step.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


def test_training_steps_with_the_fused_tail_reduce_the_loss():
    """Four steps of scripts/train_step.py with the fused tail: the loss goes down and every parameter moves -- every parameter
    that CAN: the first decoder layer normalises an all-zero target (`tgt`, models/predictor.py), so the gradient of its
    ln1.weight is sum(dy * 0), identically zero (like that of its self-attention value weight, which weight decay still
    moves), and with no weight decay on LayerNorm weights AdamW (torch's too) leaves a parameter with zero gradient where it is.  A parameter may stay only if every step gave it a gradient of exactly zero."""
    log = _train_step().run(steps=4, seed=0, device=DEV, verbose=False, fused_tail=True, lr=2e-5, drop_path=False)
    assert len(log["total_loss"]) == 4 and all(torch.isfinite(torch.tensor(log["total_loss"])))
    assert log["total_loss"][-1] < log["total_loss"][0]
    assert log["params_without_grad"] == [] and log["nonfinite_grads"] == []
    layer0 = "predictor.transformer.decoder.layers.0."                                  # what multiplies the all-zero target
    assert set(log["params_zero_grad"]) <= {layer0 + "ln1.weight", layer0 + "self_attn.value.weight"}
    assert set(log["params_unmoved"]) <= set(log["params_zero_grad"])                   # every other parameter moved
    assert log["param_delta_norm"] > 0 and 0 < log["ema_delta_norm"] < log["param_delta_norm"]
    assert len(log["tail_ms"]) == 4 and all(t > 0 for t in log["tail_ms"])


def test_deterministic_training_steps_with_the_fused_tail_repeat_bit_for_bit():
    from vrdone_amd import ops
    ts = _train_step()
    with ops.use_deterministic(True):
        a, b = (ts.run(steps=2, seed=0, device=DEV, verbose=False, fused_tail=True, lr=2e-5, drop_path=False, deterministic=True)
                for _ in range(2))
    assert a["total_loss"] == b["total_loss"] and a["sha256"] == b["sha256"]
