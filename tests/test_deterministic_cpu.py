"""The deterministic mode's switch, its graph-recording key and the C ABI of its gradient kernels (no GPU needed: the
library validates arguments -- the mode's scratch requirement included -- before any device access)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_CALLS = ("vrd_gemm_wgrad", "vrd_gemm_wgrad_x3", "vrd_colsum", "vrd_dwconv_wgrad", "vrd_layernorm_bwd")


@pytest.fixture
def torch_flags():
    """restore torch's determinism switches and the mode's explicit setting after a test"""
    from vrdone_amd import ops
    algo, warn, cudnn, explicit = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                                   torch.backends.cudnn.deterministic, ops._deterministic)
    yield
    torch.use_deterministic_algorithms(algo, warn_only=warn)
    torch.backends.cudnn.deterministic = cudnn
    ops.set_deterministic(explicit)


def test_default_is_off_with_torch_flags_at_their_defaults():
    code = ("import torch; from vrdone_amd import ops; "
            "assert not torch.are_deterministic_algorithms_enabled() and not torch.backends.cudnn.deterministic; "
            "print(ops.get_deterministic())")
    env = {k: v for k, v in os.environ.items() if k != "VRDONE_DETERMINISTIC"}
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "False"


@pytest.mark.parametrize("value,want", [("1", "True"), ("0", "False")])
def test_environment_variable_decides_over_torch_flags(value, want):
    # "0" holds even with torch's flag on; "1" without it
    code = ("import torch; torch.backends.cudnn.deterministic = True; from vrdone_amd import ops; print(ops.get_deterministic()); "
            "ops.set_deterministic(None); print(ops.get_deterministic())")
    env = dict(os.environ, VRDONE_DETERMINISTIC=value)
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [want, "True"]          # set_deterministic(None): torch's flag decides again


def test_bad_environment_value_is_refused():
    env = dict(os.environ, VRDONE_DETERMINISTIC="yes")
    out = subprocess.run([sys.executable, "-c", "import vrdone_amd.ops"], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "VRDONE_DETERMINISTIC" in out.stderr


def test_torch_flags_turn_the_mode_on(torch_flags):
    from vrdone_amd import ops
    ops.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = False
    assert not ops.get_deterministic()
    torch.backends.cudnn.deterministic = True                 # what the reference's utils.set_seed sets
    assert ops.get_deterministic()
    torch.backends.cudnn.deterministic = False
    torch.use_deterministic_algorithms(True)
    assert ops.get_deterministic()
    torch.use_deterministic_algorithms(False)
    assert not ops.get_deterministic()


def test_explicit_call_decides_over_torch_flags(torch_flags):
    from vrdone_amd import ops
    torch.backends.cudnn.deterministic = True
    ops.set_deterministic(False)
    assert not ops.get_deterministic()
    torch.backends.cudnn.deterministic = False
    ops.set_deterministic(True)
    assert ops.get_deterministic() and ops.grad_flags() == 1


def test_context_manager_nests_and_restores(torch_flags):
    from vrdone_amd import ops
    ops.set_deterministic(None)
    torch.backends.cudnn.deterministic = False
    with ops.use_deterministic(True):
        assert ops.get_deterministic()
        with ops.use_deterministic(False):
            assert not ops.get_deterministic() and ops.grad_flags() == 0
        assert ops.get_deterministic()
    assert ops._deterministic is None and not ops.get_deterministic()
    torch.backends.cudnn.deterministic = True                 # the restored setting follows torch again
    assert ops.get_deterministic()


def test_graph_recording_key_changes_with_the_switch(torch_flags):
    from vrdone_amd import ops, train_graph

    class Tiny(torch.nn.Module):
        deep_supervision, pair_chunk = True, 64

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(2))

    model, x, m = Tiny(), torch.zeros(2, 3, 4), torch.zeros(2, 4)
    with ops.use_deterministic(False):
        off = train_graph.recording_key(model, x, m)
    with ops.use_deterministic(True):
        on = train_graph.recording_key(model, x, m)
    assert off != on and off[:-1] == on[:-1]


def test_abi_flags_arguments_and_scratch_query():
    from vrdone_amd import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vrdone_hip.h")).read(), flags=re.S)
    assert re.search(r"#define VRD_DETERMINISTIC 1\b", header) and _hip.DETERMINISTIC == 1
    assert re.search(r"#define VRD_ERR_SCRATCH \(-3\)", header) and _hip.ERR_SCRATCH == -3
    for name in GRAD_CALLS:
        proto = re.search(r"int %s\(([^)]*)\);" % name, header).group(1)
        assert proto.split(",")[-1].split() == ["int", "flags"], name
        assert proto.split(",")[-2].split() == ["void*", "stream"], name
        _, argtypes = _hip._SIGNATURES[name]
        assert argtypes[-1] is ctypes.c_int and argtypes[-2] is ctypes.c_void_p, name
    proto = re.search(r"int vrd_gemm_wgrad\(([^)]*)\);", header).group(1)
    assert "float* scratch" in proto and "int64_t scratch_floats" in proto


def _need():
    from vrdone_amd import _hip
    n = ctypes.c_int64(-1)
    assert _hip.lib.vrd_scratch_required(ctypes.byref(n)) == 0
    return n.value


def test_deterministic_calls_without_scratch_are_refused_before_any_launch():
    """Dummy (aligned, non-null) device addresses: with the flag the scratch check comes before any device access."""
    from vrdone_amd import _hip
    lib, D, P = _hip.lib, _hip.DETERMINISTIC, 256
    rows, C = 49152, 512
    # vrd_colsum, 49 k rows x 512 columns (two column blocks of the float4 form): 512 row blocks + 16 rows of the second level
    assert lib.vrd_colsum(P, C, None, 0, 1, 0, 1, 0, 1, None, None, rows, C, P, None, 0, None, D) == _hip.ERR_SCRATCH
    assert _need() == (512 + 16) * C
    assert "deterministic" in lib.vrd_last_error().decode()
    assert lib.vrd_colsum(P, C, None, 0, 1, 0, 1, 0, 1, None, None, rows, C, P, P, (512 + 16) * C - 1, None, D) == _hip.ERR_SCRATCH
    # misaligned scratch is refused too (the alignment of the scratch must not pick another form)
    assert lib.vrd_colsum(P, C, None, 0, 1, 0, 1, 0, 1, None, None, rows, C, P, P + 4, 1 << 30, None, D) == _hip.ERR_SCRATCH
    # the misaligned operand of the same shape asks for the same scratch: same form, same tree
    assert lib.vrd_colsum(P + 4, C, None, 0, 1, 0, 1, 0, 1, None, None, rows, C, P, None, 0, None, D) == _hip.ERR_SCRATCH
    assert _need() == (512 + 16) * C
    # vrd_gemm_wgrad: 96 row chunks of 512 rows -> 96 partial tiles
    assert lib.vrd_gemm_wgrad(P, 512, P, 512, None, rows, 512, 512, 3, 96, P, None, 0, None, D) == _hip.ERR_SCRATCH
    assert _need() == 96 * 512 * 1536
    assert lib.vrd_gemm_wgrad_x3(P, 512, P, 512, None, rows, 512, 512, 1, 96, P, P, None, 0, None, None, D) == _hip.ERR_SCRATCH
    assert _need() > 512 * 512
    assert lib.vrd_dwconv_wgrad(P, C, P, 2 * C, 3, 2, 2, 96, None, rows, C, P, P, None, 0, None, D) == _hip.ERR_SCRATCH
    assert lib.vrd_layernorm_bwd(P, C, P, C, rows, C, P, P, 0, P, C, P, P, None, 0, None, D) == _hip.ERR_SCRATCH
    # unknown flag bits are an argument error
    assert lib.vrd_colsum(P, C, None, 0, 1, 0, 1, 0, 1, None, None, rows, C, P, None, 0, None, 2) == -1


def test_scratch_need_matches_the_recorded_chunking():
    """tests/golden/det_scratch_need.json (scripts/record_det_scratch_need.py): the scratch every deterministic gradient call of a
    grid of shapes asked for when the file was recorded.  The need is the kernel form, the row chunks / row blocks and the depth
    of the reduction tree in one number -- the summation order -- so it must not move; aligned and shifted operands ask for the
    same.  One float less than the need is refused again."""
    from vrdone_amd import _hip
    with open(os.path.join(REPO, "tests", "golden", "det_scratch_need.json")) as f:
        doc = json.load(f)
    assert {c["fn"] for c in doc["calls"]} == set(GRAD_CALLS)
    wrong = []
    for c in doc["calls"]:
        fn, args, at, need = getattr(_hip.lib, c["fn"]), list(c["args"]), doc["scratch_arg"][c["fn"]], c["need"]
        assert args[at] is None and args[at + 1] == 0 and args[-1] == _hip.DETERMINISTIC
        if need == 0:
            # no scratch: the call goes on to its launches, which dummy addresses allow only where there is no device to reach
            if not torch.cuda.is_available() and fn(*args) == _hip.ERR_SCRATCH:
                wrong.append((c, _need()))
            continue
        if fn(*args) != _hip.ERR_SCRATCH or _need() != need:
            wrong.append((c, _need()))
        args[at], args[at + 1] = 256, need - 1
        if fn(*args) != _hip.ERR_SCRATCH or _need() != need:
            wrong.append((c, "one float short", _need()))
    assert not wrong, wrong[:10]


def test_flags_default_to_zero_for_earlier_callers():
    """Callers written before `flags` existed (ctypes, one argument short) get the default mode."""
    from vrdone_amd import _hip
    # without the flag, no scratch is needed: a bad argument is what stops this call, not the scratch check
    rc = _hip.lib.vrd_colsum(256, 4, None, 0, 1, 0, 1, 0, 1, None, None, 0, 4, 256, None, 0, None)
    assert rc == -1 and "bad arguments" in _hip.lib.vrd_last_error().decode()
