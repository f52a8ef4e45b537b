"""Every output element of the backward GEMM kernels at small shapes, on the MI355X (tests/bwd_gemm_cases.py holds the case table
with the plan each weight-gradient case expects, the float64 reference, the derived bounds and the checker;
tests/test_bwd_gemm_cases_cpu.py shows the checker catches the faults this file exists for).

The weight-gradient forms are chosen by shape, CU count, alignment and the VRD_WGRAD_LDS / VRD_WGRAD_BIG switches, the
input-gradient GEMM's tile by VRD_X3_DMA / VRD_X3_SMALL; those are read once per process, so each group (GROUP_ENV) runs in a
fresh child process -- this file run as a script, `python tests/test_gpu_bwd_gemm_tiles.py <group>` -- one at a time, each under a
time limit.  The child loops over the group's cases and formats; in each it asserts the plan the library reports
(vrd_gemm_wgrad_x3_plan) or the kernel family (vrd_gemm_family) before the launch, then guards intact, inputs unchanged, every
element of dW, db and dx finite and within its bound, and the same bits from a second run where the sums are ordered
(deterministic mode, partial tiles).  After a child that ended on a fault, an abort, a HIP error or its time limit no further child is
started: the remaining tests fail at once."""
import ctypes
import os
import subprocess
import sys
import time
import traceback

import pytest
import torch

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import bwd_gemm_cases as B
import window_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = tuple(B.GROUP_ENV)
# seconds: ten times the child's duration on the first run on an MI355X (LABNOTES.md), at least 60
LIMIT = {"wave": 60, "lds128": 60, "lds256": 60, "default": 60, "dgrad128": 60, "dgrad64": 60}
ERROR_STATUS = 3                               # the child's status after an exception that is no failed check (a HIP error)
FATAL = (124, 137, 134, 139, -6, -11, ERROR_STATUS)      # time limit, abort, segmentation fault, HIP error: nothing more is started on the GPU


# ---------------------------------------------------------------------------------------------------------------- child
def _scale_buffer(h, mode, inp, ops, _hip):
    """device {2^e, 2^-e} of the f16 format for the window h: vrd_absmax_scale where the rows are float4-shaped (and then it must
    give the exponent the reference splits at), written by hand otherwise (ops.grad_scale refuses such rows)"""
    if mode != "f16":
        return None
    buf = ops.grad_scale(h.view)
    want = torch.tensor([2.0 ** inp.gexp, 2.0 ** -inp.gexp])
    if buf is None:
        buf = torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV)
        buf[:2] = want.to(DEV)
    else:
        got = buf[:2].cpu()
        assert torch.equal(got, want), f"case {inp.case.name}: vrd_absmax_scale gave {got.tolist()}, the gradient's exponent is {inp.gexp}"
    return buf


def _run_wgrad(case, mode, ops, _hip, saved):
    lib = _hip.lib
    inp = B.make_inputs(case, mode, DEV)
    M, T, N, Cin, k = case.M, case.T, case.N, case.Cin, case.k
    NK = N * Cin * k
    pg, ldg, px, ldx = inp.hG.view.data_ptr(), inp.hG.ld, inp.hX.view.data_ptr(), inp.hX.ld
    mask = inp.mask.to(DEV) if inp.mask is not None else None
    pm = mask.data_ptr() if mask is not None else None
    flags = _hip.DETERMINISTIC if case.det else 0
    pdw, pdb = inp.fW.view.data_ptr(), (inp.fB.view.data_ptr() if inp.fB is not None else None)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    mirror = B.plan_of(case, n_cu)
    scratch = None
    if case.scratch or case.det:          # what the header says always suffices, and the column-sum kernels' 1,057 rows
        scratch = B.Flat(mirror.chunks * (NK + 2 * N) + 1100 * N, DEV, "scratch")
    ps, ns = (scratch.view.data_ptr(), scratch.n) if scratch is not None else (None, 0)
    if case.kind == "x3":
        out = (ctypes.c_int64 * _hip.WGRAD_PLAN_INTS)()
        _hip.check(lib.vrd_gemm_wgrad_x3_plan(pg, ldg, px, ldx, M, N, Cin, k, pdw, 1 if pdb else 0, ps, ns, flags, out), "vrd_gemm_wgrad_x3_plan")
        form = {_hip.WGRAD_WAVE: "wave", _hip.WGRAD_LDS128: "lds128", _hip.WGRAD_LDS256: "lds256"}[out[0]]
        plan = B.Plan(form, bool(out[1]), out[2], out[3], out[4], bool(out[5]))
        got = (plan.form, plan.vec, plan.chunks >= 2, plan.tile_partials)
        assert got == case.plan, f"case {case.name} [{mode}]: the library plans {plan}, the case is for (form, vec, several chunks, partial tiles) = {case.plan}"
        assert plan == mirror, f"case {case.name} [{mode}]: the library plans {plan}, the mirror of tests/bwd_gemm_cases.py {mirror} ({n_cu} CUs)"
        assert out[6] <= ns, f"case {case.name} [{mode}]: the plan asks for {out[6]} floats of scratch, the test made {ns}"
        gs = _scale_buffer(inp.hG, mode, inp, ops, _hip)
        pgs = gs.data_ptr() if gs is not None else None
        call = lambda: _hip.check(lib.vrd_gemm_wgrad_x3(pg, ldg, px, ldx, pm, M, N, Cin, k, T, pdw, pdb, ps, ns, pgs, ops._stream(), flags),          # noqa: E731
                                  "vrd_gemm_wgrad_x3")
    else:
        plan = mirror
        call = lambda: _hip.check(lib.vrd_gemm_wgrad(pg, ldg, px, ldx, pm, M, N, Cin, k, T, pdw, ps, ns, ops._stream(), flags), "vrd_gemm_wgrad")          # noqa: E731
    call()
    torch.cuda.synchronize()
    ratios = B.verify(inp, plan, scratch)
    if mask is not None:
        assert torch.equal(mask.cpu(), inp.mask), f"case {case.name} [{mode}]: the row mask was written"
    first = [f.view.clone() for f in (inp.fW, inp.fB) if f is not None]
    if case.det or plan.tile_partials:          # ordered sums: a second run from the same start gives the same bits
        inp.fW.view.copy_(inp.dw0.reshape(-1).to(DEV))
        if inp.fB is not None:
            inp.fB.view.copy_(inp.db0.to(DEV))
        call()
        torch.cuda.synchronize()
        for f, a in zip([f for f in (inp.fW, inp.fB) if f is not None], first):
            if f is inp.fB and not case.det:          # (the default mode's bias sums are atomics)
                continue
            assert W.bits_equal(f.view, a), f"case {case.name} [{mode}]: {f.name} differs between two runs"
    if "pair_a" in case.tags:
        saved[(case.data, mode)] = [a.cpu() for a in first]
    if "pair_b" in case.tags:          # the same shape one float off a 16-byte line: scalar loads add in the same order
        for a, b, what in zip(saved[(case.data, mode)], first, ("dW", "db")):
            assert W.bits_equal(a, b.cpu()), f"case {case.name} [{mode}]: {what} differs from the aligned run's"
    key = ("f32" if case.kind == "f32" else plan.form) + (" det" if case.det else "")
    return key, ratios


def _run_dgrad(case, mode, ops, _hip):
    inp = B.make_inputs(case, mode, DEV)
    fmt = _hip.PAIR_F16 if mode == "f16" else _hip.PAIR_BF16
    w = inp.w.to(DEV)
    mask = inp.mask.reshape(case.M // case.T, case.T).to(DEV) if inp.mask is not None else None
    gs = _scale_buffer(inp.hG, mode, inp, ops, _hip)
    a, dx = ops.dgrad_args(inp.hG.view, w, row_mask=mask, a_scale=gs, fmt=fmt, out=inp.hC.view)
    fam = ops.gemm_family(a)
    assert fam == _hip.K_GEMM_X3, f"case {case.name} [{mode}]: the library chose kernel family {fam}, the group is for K_GEMM_X3 ({_hip.K_GEMM_X3})"
    ops.launch_gemm(a)
    torch.cuda.synchronize()
    ratios = B.verify(inp, None)
    if mask is not None:
        assert torch.equal(mask.cpu().reshape(-1), inp.mask), f"case {case.name} [{mode}]: the row mask was written"
    return "dgrad", ratios


def _child(group):
    from vrdone_amd import _hip, ops
    t0 = time.time()
    failures, worst, saved = [], {}, {}
    with torch.no_grad():
        for case in B.cases_of(group):
            for mode in case.modes:
                try:
                    key, ratios = _run_dgrad(case, mode, ops, _hip) if case.kind == "dgrad" else _run_wgrad(case, mode, ops, _hip, saved)
                except AssertionError as e:
                    failures.append(str(e) or repr(e))
                    continue
                except Exception:          # a HIP error: the device may have faulted -- this child runs nothing more on it
                    traceback.print_exc()
                    print(f"DEVICE ERROR in group {group}, case {case.name} [{mode}]", flush=True)
                    os._exit(ERROR_STATUS)
                for what, r in ratios.items():
                    if r >= worst.get((key, mode, what), (0.0, ""))[0]:
                        worst[(key, mode, what)] = (r, case.name)
                print(f"{group} {case.name} [{mode}]: error / bound " + ", ".join(f"{w} {r:.3f}" for w, r in ratios.items()), flush=True)
    for (key, mode, what), (ratio, name) in sorted(worst.items()):
        print(f"WORST {group} {key} {mode} {what}: {ratio:.3f} ({name})")
    print(f"DURATION {group}: {time.time() - t0:.1f} s in the child's own loop, {len(failures)} failures")
    for f in failures:
        print("FAILED " + f)
    sys.stdout.flush()
    sys.exit(1 if failures else 0)


# --------------------------------------------------------------------------------------------------------------- parent
_state = {"done": {}, "dead": None}


@pytest.fixture(scope="module", autouse=True)
def _fresh():
    _state.update(done={}, dead=None)
    yield


def _run_group(group):
    """the group's child, once per module run; (return code, output)"""
    if group in _state["done"]:
        return _state["done"][group]
    assert _state["dead"] is None, f"no further GPU child is started: the child of group {_state['dead']} ended on a fault, an abort or its time limit"
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT[group]), sys.executable, os.path.abspath(__file__), group],
                       cwd=REPO, env=dict(os.environ, **B.GROUP_ENV[group]), capture_output=True, text=True)
    print(f"child {group}: status {r.returncode}, {time.time() - t0:.1f} s wall")
    print(r.stdout[-8000:])
    if r.returncode in FATAL:
        _state["dead"] = group
    _state["done"][group] = (r.returncode, r.stdout + r.stderr[-3000:])
    return _state["done"][group]


@pytest.mark.parametrize("group", GROUPS)
def test_every_element_of_every_case(group):
    rc, out = _run_group(group)
    failed = [line for line in out.splitlines() if line.startswith("FAILED ")]
    assert rc == 0, f"group {group}: child status {rc}\n" + ("\n".join(failed) if failed else out[-4000:])
    ran = sum(1 for line in out.splitlines() if "error / bound" in line)
    assert ran == sum(len(c.modes) for c in B.cases_of(group))
    assert f"DURATION {group}:" in out and "WORST " in out


if __name__ == "__main__":
    _child(sys.argv[1])
