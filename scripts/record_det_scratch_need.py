"""Record vrd_scratch_required() of a grid of deterministic gradient calls into tests/golden/det_scratch_need.json.

The library refuses a deterministic call without scratch before any device access, so dummy addresses do (no GPU needed).  The
need encodes the kernel form, the row chunks / row blocks and the depth of the reduction tree: the summation order.  Run it
with the library whose chunking is the reference (VRDONE_HIP_LIB), VRD_WGRAD_LDS / VRD_WGRAD_BIG unset:
    python scripts/record_det_scratch_need.py
tests/test_deterministic_cpu.py::test_scratch_need_matches_the_recorded_chunking replays the file."""
import ctypes
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
P, T, D = 256, 16, 1            # an aligned dummy address, frames per sequence, VRD_DETERMINISTIC
# position of `scratch` in each call's argument list (`scratch_floats` follows it)
SCRATCH_ARG = {"vrd_colsum": 14, "vrd_dwconv_wgrad": 13, "vrd_layernorm_bwd": 13, "vrd_gemm_wgrad": 11, "vrd_gemm_wgrad_x3": 12}


def calls():
    rows_l, c_l = (16, 528, 1056, 49152, 3_000_000), (4, 6, 256, 260, 512)
    for rows, C, b, sh in itertools.product(rows_l, c_l, ("none", "same", "strided"), (0, 4)):
        ldb, cst, cof, shift = {"none": (0, 1, 0, 0), "same": (C, 1, 0, 0), "strided": (2 * C, 2, 1, -1)}[b]
        yield "vrd_colsum", [P + sh, C, P + sh if b != "none" else None, ldb, cst, cof, 1, shift, T, None, None, rows, C, P, None, 0, None, D]
    for rows, C, bias, (ks, gin, st), sh in itertools.product(rows_l, c_l, (True, False), ((3, 1, 1), (3, 2, 2), (1, 2, 2)), (0, 4)):
        yield "vrd_dwconv_wgrad", [P + sh, C, P + sh, C * gin, ks, st, gin, T, None, rows, C, P, P if bias else None, None, 0, None, D]
    for rows, C in itertools.product((32, 1056, 49152, 200000), (256, 512)):
        yield "vrd_layernorm_bwd", [P, C, P, C, rows, C, P, P, 0, P, C, P, P, None, 0, None, D]
    for M in (512, 1024, 49152):
        yield "vrd_gemm_wgrad", [P, 512, P, 512, None, M, 512, 512, 3, T, P, None, 0, None, D]
    for M, (N, Cin), taps, bias, f16 in itertools.product((192, 256, 4224, 65536, 49152), ((128, 128), (256, 256), (512, 512), (133, 63)),
                                                          (1, 3), (True, False), (True, False)):
        yield "vrd_gemm_wgrad_x3", [P, N, P, Cin, None, M, N, Cin, taps, T, P, P if bias else None, None, 0, P if f16 else None, None, D]


def main():
    assert "VRD_WGRAD_LDS" not in os.environ and "VRD_WGRAD_BIG" not in os.environ
    import torch
    from vrdone_amd import _hip
    rows = []
    for fn, args in calls():
        assert args[SCRATCH_ARG[fn]] is None and args[SCRATCH_ARG[fn] + 1] == 0
        # a call that needs no scratch goes on to its launches: with dummy addresses only where there is no device to reach
        if fn == "vrd_gemm_wgrad" and args[5] <= 512 or fn == "vrd_gemm_wgrad_x3" and args[5] < 256 and args[11] is None:
            assert not torch.cuda.is_available(), "record the no-scratch rows on a machine without a GPU"
        rc = getattr(_hip.lib, fn)(*args)
        need = ctypes.c_int64(-1)
        assert _hip.lib.vrd_scratch_required(ctypes.byref(need)) == 0
        assert rc != -1, (fn, args, _hip.lib.vrd_last_error())
        rows.append({"fn": fn, "args": args, "need": need.value if rc == _hip.ERR_SCRATCH else 0})
    out = os.path.join(REPO, "tests", "golden", "det_scratch_need.json")
    with open(out, "w") as f:
        f.write('{"scratch_arg": %s,\n "calls": [\n' % json.dumps(SCRATCH_ARG))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} calls, {sum(r['need'] == 0 for r in rows)} without scratch -> {out}")


if __name__ == "__main__":
    main()
