"""Host side of vrdone_amd.optim (gradient-norm clip + AdamW over pointer tables, csrc/vrd_optim.hip): what needs no GPU.
On CPU parameters FusedAdamW takes torch's own path, so it must BE torch.optim.AdamW there; its state is torch's state; the
chunk map is plain Python; the new entry points are declared, bound and exported under the same names."""
import copy
import ctypes
import os
import re

import torch

from conftest import REPO

NEW = ("vrd_grad_sumsq", "vrd_grad_norm_finish", "vrd_adamw_step", "vrd_scale_tensors")


def _params(seed=0, sizes=(1, 3, 37, 5000)):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes]


def _groups(ps):
    return [{"params": ps[0::2], "weight_decay": 0.05, "lr": 1e-2}, {"params": ps[1::2], "weight_decay": 0.0, "lr": 3e-3}]


def _set_grads(sets, step):
    g = torch.Generator().manual_seed(100 + step)
    for i, group in enumerate(zip(*sets)):
        grad = torch.randn(group[0].shape, generator=g) * 10.0 ** (i - 2)
        for p in group:
            p.grad = grad.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_cpu_parameters_take_torchs_path_bit_for_bit():
    from vrdone_amd.optim import FusedAdamW, clip_grad_norm_
    a, b, c = _params(), _params(), _params()
    fused, ref = FusedAdamW(_groups(a)), torch.optim.AdamW(_groups(b))
    standalone = FusedAdamW(_groups(c))
    assert isinstance(fused, torch.optim.AdamW)
    for step in range(4):
        _set_grads((a, b, c), step)
        fused.step(max_grad_norm=1.0)
        want = torch.nn.utils.clip_grad_norm_(b, 1.0)
        ref.step()
        got = clip_grad_norm_(c, 1.0)
        standalone.step()
        assert torch.equal(fused.last_grad_norm, want) and torch.equal(got, want)
        assert _same(a, b) and _same(c, b), step
    for p, q in zip(a, b):
        assert set(fused.state[p]) == set(ref.state[q]) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.equal(fused.state[p]["step"], ref.state[q]["step"]) and fused.state[p]["step"].dtype == ref.state[q]["step"].dtype
        assert torch.equal(fused.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])


def test_state_dict_round_trips_with_torch_adamw_in_both_directions():
    from vrdone_amd.optim import FusedAdamW
    a, b = _params(), _params()
    fused, ref = FusedAdamW(_groups(a)), torch.optim.AdamW(_groups(b))
    for step in range(2):
        _set_grads((a, b), step)
        fused.step()
        ref.step()
    sd_fused, sd_ref = fused.state_dict(), ref.state_dict()
    assert sd_fused["param_groups"] == sd_ref["param_groups"]
    assert sd_fused["state"].keys() == sd_ref["state"].keys()
    # fused -> torch and torch -> fused, onto fresh optimisers over copies of the parameters; then two more steps everywhere
    a2, b2 = [torch.nn.Parameter(p.detach().clone()) for p in a], [torch.nn.Parameter(p.detach().clone()) for p in b]
    fused2, ref2 = FusedAdamW(_groups(a2)), torch.optim.AdamW(_groups(b2))
    ref2.load_state_dict(copy.deepcopy(sd_fused))          # (load_state_dict keeps tensors it need not cast: no shared state)
    fused2.load_state_dict(copy.deepcopy(sd_ref))
    sched = torch.optim.lr_scheduler.LambdaLR(fused2, lambda e: 0.5 ** e)          # a scheduler that writes group['lr'] works on it
    sched_ref = torch.optim.lr_scheduler.LambdaLR(ref, lambda e: 0.5 ** e)
    for step in range(2, 4):
        _set_grads((a, b, a2, b2), step)
        fused.step()
        ref2.step()
        assert _same(a, b2), step
        ref.step()
        fused2.step()
        sched.step()
        sched_ref.step()
        assert _same(b, a2), step
    assert fused2.param_groups[0]["lr"] == ref.param_groups[0]["lr"] == 1e-2 * 0.25


def test_chunk_map():
    from vrdone_amd.optim import _CHUNK, build_chunk_map
    numels = [0, 1, 3, 4095, 4096, 4097, 8193]
    ct, ci = build_chunk_map(numels)
    assert _CHUNK == 4096
    assert ct == [1, 2, 3, 4, 5, 5, 6, 6, 6] and ci == [0, 0, 0, 0, 0, 1, 0, 1, 2]
    for t, n in enumerate(numels):                              # every element of every tensor in exactly one chunk
        covered = sorted(i for c, i in zip(ct, ci) if c == t)
        assert covered == list(range(-(-n // _CHUNK)))
        assert all(i * _CHUNK < n for i in covered)
    # a parameter without a gradient keeps its place in the tables and gets no chunk
    present = [True, True, False, True, True, False, True]
    ct, ci = build_chunk_map(numels, present)
    assert ct == [1, 3, 4, 6, 6, 6] and ci == [0, 0, 0, 0, 1, 2]
    assert build_chunk_map([0, 0]) == ([], []) and build_chunk_map([5], [False]) == ([], [])


def test_hyper_parameter_row_is_torchs_scalars():
    from vrdone_amd import _hip
    from vrdone_amd.optim import adamw_row
    lr, wd, b1, b2, eps, t = 3e-4, 0.05, 0.9, 0.999, 1e-8, 7
    row = adamw_row(lr, wd, b1, b2, eps, t)
    assert len(row) == _hip.ADAMW_GROUP_FLOATS == 8
    assert row == [lr * wd, b1, b2, eps, lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5, 1 - b1, 1 - b2]
    # why 1 - beta travels on its own: formed in f32 from the rounded beta it is off by far more than an f32 rounding
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))            # noqa: E731
    assert abs(f32(1.0 - f32(b2)) - (1 - b2)) > 1e-5 * (1 - b2) and abs(f32(1 - b2) - (1 - b2)) < 1e-7 * (1 - b2)


def test_new_entry_points_are_declared_bound_and_exported():
    from vrdone_amd import _hip
    header = open(os.path.join(REPO, "include", "vrdone_hip.h")).read()
    assert "#define VRD_ABI_VERSION 37" in header and _hip.ABI_VERSION == 37        # (37: vrd_gemm_wgrad_x3_plan came with a bump; these entry points had come without one)
    assert "#define VRD_ADAMW_GROUP_FLOATS 8" in header
    declared = set(re.findall(r"\bint\s+(vrd_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(REPO, "vrdone_amd", "csrc", "libvrdone_hip.so"))
    for name in NEW:
        assert name in declared and name in _hip._SIGNATURES and hasattr(lib, name), name
    assert "VRD_K_OPTIM" not in header and len(_hip.KERNEL_NAMES) == 14                # they profile under "backward"


def test_entry_points_validate_before_any_launch():
    from vrdone_amd import _hip
    lib = _hip.lib
    one = ctypes.c_void_p(16)
    assert lib.vrd_grad_sumsq(None, one, one, one, one, 1, one, None) != 0 and b"vrd_grad_sumsq" in lib.vrd_last_error()
    assert lib.vrd_grad_sumsq(one, one, one, one, one, 0, one, None) != 0
    assert lib.vrd_grad_norm_finish(one, 0, 1.0, one, None) != 0 and b"vrd_grad_norm_finish" in lib.vrd_last_error()
    assert lib.vrd_grad_norm_finish(one, 1, float("nan"), one, None) != 0
    assert lib.vrd_adamw_step(one, one, one, one, one, one, one, one, 0, one, one, 1, None, None) != 0
    assert b"vrd_adamw_step" in lib.vrd_last_error()
    assert lib.vrd_adamw_step(one, one, None, one, one, one, one, one, 1, one, one, 1, None, None) != 0
    assert lib.vrd_scale_tensors(one, one, one, one, one, 1, None, None) != 0 and b"vrd_scale_tensors" in lib.vrd_last_error()
