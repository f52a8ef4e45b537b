"""Every output element of the split-precision GEMM kernels at small shapes, on the MI355X (tests/gemm_tile_cases.py holds the case
table, the float64 reference, the derived bound and the checker; tests/test_gemm_tile_cases_cpu.py shows the checker catches the
faults this file exists for).

The 256 x 256 and 128 x 256 LDS-DMA kernels serve only problems of 512 tiles or more unless the kernel-selection switches of
csrc/ force them (GROUP_ENV).  Those are read once per process, so each forced-kernel group runs in a fresh child process --
this file run as a script, `python tests/test_gpu_gemm_tiles.py <group> <directory>` -- one at a time, each under a time limit.
The child loops over the group's cases and the split modes; in each case it asserts the kernel family the library reports,
guards intact, inputs unchanged, every element written and within the bound, and saves the outputs the agreement tests compare.
After a child that ended on a fault, an abort or its time limit no further child is started: the remaining tests fail at once."""
import os
import subprocess
import sys
import time
import traceback

import pytest
import torch

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import gemm_tile_cases as G
import window_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = tuple(G.GROUP_ENV)
# seconds: ten times the child's duration on the first run on an MI355X (LABNOTES.md), at least 60
LIMIT = {"big": 60, "big_one_tile": 60, "big_grid2": 60, "big_grid3": 60, "dma": 60, "x3_128": 60, "x3_64": 60}
ERROR_STATUS = 3                               # the child's status after an exception that is no failed check (a HIP error)
FATAL = (124, 137, 134, 139, -6, -11, ERROR_STATUS)      # time limit, abort, segmentation fault, HIP error: nothing more is started on the GPU


# ---------------------------------------------------------------------------------------------------------------- child
def _run_case(case, mode, group, ops, _hip):
    """one case in one mode on the GPU; returns (error-to-bound ratio, {name: tensor} to save)"""
    inp = G.make_inputs(case, mode, DEV)
    fmt = _hip.PAIR_BF16 if mode == "bf16x3" else _hip.PAIR_F16
    mask = inp.mask.to(DEV) if inp.mask is not None else None
    kw = {}
    if "gelu" in case.epi:
        kw["act"] = ops.ACT_GELU
    elif "relu" in case.epi:
        kw["act"] = ops.ACT_RELU
    if "mask" in case.epi:
        kw["row_mask"] = mask
    if case.layout == "pad_skip":
        kw["skip_rows"] = mask
    if inp.scale is not None:
        kw["scale"] = inp.scale.to(DEV)
    if inp.hR is not None:
        kw["res"], kw["res_masked"] = inp.hR.view, "res_masked" in case.epi
    if inp.hR2 is not None:
        kw["res2"] = inp.hR2.view
    want_family = getattr(_hip, G.GROUP_FAMILY[group])
    maps = case.layout in ("pad_map", "pad_skip")
    old_skip, old_min = ops._skip_padding, ops.SKIP_MIN_ROWS
    ops._skip_padding, ops.SKIP_MIN_ROWS = maps, 0 if maps else old_min
    try:
        def calls(m, pair):
            out = []
            with ops.use_precision(m):
                for p in inp.problems:
                    a = (ops.Pair(p.hA.view, case.Cin, fmt), p.w.to(DEV), p.bias.to(DEV) if p.bias is not None else None)
                    out.append((a, dict(kw, out=(p.hP if pair else p.hC).view, out_pair=pair)))
                fam = [ops.gemm_family(ops.gemm_args(*a, **k)[0]) for a, k in out]
                if case.layout == "batch3":
                    ops.conv_gemm_batch(out)
                else:
                    ops.conv_gemm(*out[0][0], **out[0][1])
            assert fam and all(f == want_family for f in fam), \
                f"case {case.name} [{m}]: the library chose kernel family {fam}, the group {group} is for {want_family}"
        if mode == "f16x1":          # the three-product result of the same call first: the yardstick of the one-product criterion
            calls("f16x3", False)
            torch.cuda.synchronize()
            for p in inp.problems:
                p.got3 = p.hC.result().cpu()
                p.hC.buf.view(torch.int32).copy_(p.hC.before)
        calls(mode, False)
        if case.pair_out:
            calls(mode, True)
        torch.cuda.synchronize()
    finally:
        ops._skip_padding, ops.SKIP_MIN_ROWS = old_skip, old_min
    rows = None
    if maps:
        blocks = ops.row_blocks(mask)
        assert blocks is not None, f"case {case.name}: no padding map"
    if case.layout == "pad_skip":
        # 256-row tile j is slots 8 j .. 8 j + 7 of the block list and contracts when its segment holds a valid block: every row of
        # such a tile is computed (against float64); the tiles without one skip -- their rows are finite filler, not the product
        order, count, seg_len = blocks[0].cpu().long(), blocks[1].cpu().tolist(), blocks[2]
        assert (count, seg_len) == G.segment_counts(inp.mask), f"case {case.name}: padding map {count}, {seg_len}"
        computed = torch.zeros(case.B * case.T // 32, dtype=torch.bool)
        for j, n in enumerate(count):
            computed[order[8 * j:8 * j + 8]] = n > 0
        rows = computed.repeat_interleave(32).reshape(case.B, case.T)
        assert bool((rows | ~G.valid_block_rows(inp)).all()) and 0 in count, f"case {case.name}: tiles {count}"
    ratio = G.verify(inp, rows)
    if case.layout == "pad_skip":
        p = inp.problems[0]
        ref, mag, lip = G.reference(inp, p)
        got = p.hC.result().cpu().double()
        assert not torch.allclose(got[~rows], ref[~rows], atol=1e-3), f"case {case.name} [{mode}]: the skipped tiles hold the product"
    save = {}
    if case.agree and mode != "f16x1":
        save[case.name] = inp.problems[0].hC.result().cpu()
        if case.pair_out:
            save[case.name + ":pair"] = inp.problems[0].hP.result().cpu()
    return ratio, save


def _child(group, outdir):
    from vrdone_amd import _hip, ops
    t0 = time.time()
    failures, saved, worst = [], {}, {}
    with torch.no_grad():
        for case in G.cases_of(group):
            for mode in case.modes:
                try:
                    ratio, save = _run_case(case, mode, group, ops, _hip)
                except AssertionError as e:
                    failures.append(str(e) or repr(e))
                    continue
                except Exception:          # a HIP error: the device may have faulted -- this child runs nothing more on it
                    traceback.print_exc()
                    print(f"DEVICE ERROR in group {group}, case {case.name} [{mode}]", flush=True)
                    os._exit(ERROR_STATUS)
                saved.update({f"{mode}/{k}": v for k, v in save.items()})
                key = (G.GROUP_FAMILY[group], mode)
                if ratio > worst.get(key, (0.0, ""))[0]:
                    worst[key] = (ratio, case.name)
                print(f"{group} {case.name} [{mode}]: error / bound {ratio:.3f}", flush=True)
    torch.save(saved, os.path.join(outdir, f"{group}.pt"))
    for (fam, mode), (ratio, name) in sorted(worst.items()):
        print(f"WORST {group} {fam} {mode}: {ratio:.3f} ({name})")
    print(f"DURATION {group}: {time.time() - t0:.1f} s in the child's own loop, {len(failures)} failures")
    for f in failures:
        print("FAILED " + f)
    sys.exit(1 if failures else 0)


# --------------------------------------------------------------------------------------------------------------- parent
_state = {"dir": None, "done": {}, "dead": None}


@pytest.fixture(scope="module", autouse=True)
def _outdir(tmp_path_factory):
    _state.update(dir=str(tmp_path_factory.mktemp("gemm_tiles")), done={}, dead=None)
    yield


def _run_group(group):
    """the group's child, once per module run; (return code, output)"""
    if group in _state["done"]:
        return _state["done"][group]
    assert _state["dead"] is None, f"no further GPU child is started: the child of group {_state['dead']} ended on a fault, an abort or its time limit"
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT[group]), sys.executable, os.path.abspath(__file__), group, _state["dir"]],
                       cwd=REPO, env=dict(os.environ, **G.GROUP_ENV[group]), capture_output=True, text=True)
    print(f"child {group}: status {r.returncode}, {time.time() - t0:.1f} s wall")
    print(r.stdout[-6000:])
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
    assert ran == sum(len(c.modes) for c in G.cases_of(group))


def _saved(group):
    rc, out = _run_group(group)
    assert rc == 0, f"group {group}: child status {rc}"
    return torch.load(os.path.join(_state["dir"], f"{group}.pt"))


def _differing(agree):
    outs = {g: _saved(g) for g in G.ALL6}
    keys = [f"{m}/{c.name}{s}" for c in G.CASES if c.agree == agree for m in c.modes for s in (("", ":pair") if c.pair_out else ("",))]
    assert keys and all(k in outs[g] for g in G.ALL6 for k in keys)
    return keys, [(k, g) for k in keys for g in G.ALL6[1:] if not W.bits_equal(outs[g][k], outs[G.ALL6[0]][k])]


def test_bias_only_outputs_are_the_same_bits_on_every_kernel():
    """include/vrdone_hip.h: the split kernels form the same products in the same order, so the choice of kernel never changes a
    bit -- in bf16x3 and in f16x3, on the 256 x 256 kernel (persistent on one workgroup per tile-chain, persistent on two
    workgroups, one tile per workgroup), the 128 x 256, the 128 x 128 and the 64 x 64 kernel."""
    keys, differ = _differing("bits")
    assert len(keys) >= 2 * 30
    assert not differ, f"{len(differ)} of {len(keys)} outputs differ from the group {G.ALL6[0]}'s: {differ[:12]}"


LEAN = ("big", "big_one_tile", "big_grid2")          # the 256 x 256 kernel's lean epilogue (gemm_epilogue_lean_tr)
GENERAL = ("dma", "x3_128", "x3_64")                 # gemm_epilogue / gemm_epilogue_tile32


def test_other_epilogues_across_kernels():
    """The same comparison for the other epilogues (no bias, GELU, row mask, column scale, the residuals, pair output; M = 512,
    N = 320, Cin = 128, k = 1 and 3).  Every form is the same bits on the three forms of the 256 x 256 kernel, and the same bits
    on the three other kernels.  Between the two sets scale / res / res2 / no bias / all-together are the same bits as well; GELU,
    row mask and masked residual give the same VALUES with different signs of zero (LABNOTES.md): the lean epilogue multiplies by
    mask * scale and adds only the terms that exist, so a zero -- a masked row, or GELU of x < -5.6, which is x * 0 -- keeps the
    sign of what it was made from, while the general epilogue evaluates v * mask * scale + res * rmk + res2 with absent terms as
    +0, and -0 + 0 is +0.  Asserted as exactly that: equal values."""
    outs = {g: _saved(g) for g in G.ALL6}
    keys = [f"{m}/{c.name}{s}" for c in G.CASES if c.agree == "other" for m in c.modes for s in (("", ":pair") if c.pair_out else ("",))]
    assert len(keys) == 2 * 2 * (8 + 2 * 9)
    wrong = []
    for k in keys:
        form = k.split("/")[1].split(":")[0].replace("_pair", "").split("_", 2)[2]
        for family in (LEAN, GENERAL):
            wrong += [(k, g, "bits inside a set") for g in family[1:] if not W.bits_equal(outs[g][k], outs[family[0]][k])]
        a, b = outs[LEAN[0]][k], outs[GENERAL[0]][k]
        if form in ("gelu", "mask", "resm"):
            if k.endswith(":pair"):          # pair rows: compare the decoded values
                a, b = G.decode_pair(a, k.startswith("f16x3")), G.decode_pair(b, k.startswith("f16x3"))
            if not torch.equal(a, b):          # (equal finite values: bits can then differ only in the sign of a zero)
                wrong.append((k, GENERAL[0], "values"))
        elif not W.bits_equal(a, b):
            wrong.append((k, GENERAL[0], "bits between the sets"))
    assert not wrong, f"{len(wrong)} comparisons failed: {wrong[:12]}"


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
