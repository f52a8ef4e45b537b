"""The case table, plan mirror, reference, bounds and checker of tests/bwd_gemm_cases.py against an f32 emulation of the kernels'
arithmetic on the CPU: the emulation passes every case with half of the rounding terms granted -- which shows that the float64
reference alone stays inside the derived bounds --, the table holds what it claims to hold, the library's own plan query agrees
with the mirror where it needs no device, and each Python stand-in of a kernel fault, the classes
tests/test_gpu_bwd_gemm_tiles.py exists to catch, is reported.  No GPU, and no wrong kernel is ever run on one."""
import ctypes

import pytest
import torch

import bwd_gemm_cases as B
import window_cases as W


@pytest.fixture(autouse=True)
def no_grad():
    with torch.no_grad():
        yield


def run(case, mode, fault=None, slack=1.0):
    inp, plan = B.make_inputs(case, mode), B.plan_of(case)
    B.emulate(inp, plan, fault)
    return B.verify(inp, plan, slack=slack)


@pytest.mark.parametrize("group", list(B.GROUP_ENV))
def test_the_emulation_stays_inside_half_of_the_rounding_terms(group):
    worst = {}
    for c in B.cases_of(group):
        for mode in c.modes:
            for what, r in run(c, mode, slack=0.5).items():
                assert r <= 1.0
                if r >= worst.get((what, mode), (0.0, ""))[0]:
                    worst[(what, mode)] = (r, c.name)
    assert worst
    for (what, mode), (r, name) in sorted(worst.items()):
        print(f"{group} {what} [{mode}]: largest error over (split term + half of the rounding terms) {r:.3f} ({name})")


def _instantiation(c, mode, plan):
    """(BIG, VEC, TAPS, F16, DET) of wgrad_x3_lds_kernel for an LDS case"""
    return (plan.form == "lds256", plan.vec, c.k, mode == "f16", c.det)


def test_the_named_plans_are_the_mirrors_and_every_reachable_instantiation_has_a_case():
    lds, wave, f32, exits = set(), set(), set(), set()
    for c in B.CASES:
        assert c.group in B.GROUP_ENV and c.M % c.T == 0 and c.M < 6000, c.name
        if c.kind == "dgrad":
            assert c.plan is None and (c.N * c.k) % 32 == 0 and c.N % 4 == 0 and c.group.startswith("dgrad"), c.name
            continue
        assert c.group in B.WGRAD_GROUPS, c.name
        # the switches hold in the default mode only: a deterministic case belongs to the group without any, an exact-f32 case to `wave`
        assert not c.det or c.group == "default" or c.kind == "f32", c.name
        plan = B.plan_of(c)
        if c.kind == "f32":
            f32.add((c.det, plan.chunks > 1))
            continue
        assert c.plan == (plan.form, plan.vec, plan.chunks >= 2, plan.tile_partials), (c.name, c.plan, plan)
        for mode in c.modes:
            if plan.form == "wave":
                wave.add((mode == "f16", c.det))
            else:
                lds.add(_instantiation(c, mode, plan))
                exits.add((plan.form, "one" if plan.chunks == 1 else "det" if c.det else "partials" if plan.tile_partials else "atomics"))
    # plan_wgrad_x3: without the flag the 256 tile needs float4 loads, so <1, false, *, *, false> cannot be reached: 28 of 32
    reachable = {(big, vec, k, f16, det) for big in (False, True) for vec in (False, True) for k in (1, 3) for f16 in (False, True)
                 for det in (False, True) if not (big and not vec and not det)}
    assert len(reachable) == 28 and lds == reachable, sorted(reachable - lds)
    assert wave == {(f, d) for f in (False, True) for d in (False, True)}
    assert f32 == {(False, False), (False, True), (True, False), (True, True)}          # (flag, several chunks)
    assert exits >= {("lds128", "one"), ("lds128", "partials"), ("lds128", "atomics"), ("lds128", "det"), ("lds256", "partials"),
                     ("lds256", "atomics"), ("lds256", "det")}


def _form(c):
    return "f32" if c.kind == "f32" else B.plan_of(c).form


def test_the_table_holds_the_edges_it_is_for():
    wg = [c for c in B.CASES if c.kind != "dgrad"]
    by = lambda form, tag: [c for c in wg if _form(c) == form and tag in c.tags]          # noqa: E731
    forms = ("wave", "lds128", "lds256", "f32")
    # k = 3 sequence lengths on every form that takes k = 3
    for form in forms:
        assert {c.T for c in by(form, "k3") if c.k == 3} >= {1, 2, 3, 5, 7, 9, 31, 32, 33, 36, 48, 100}, form
        for m in ("none", "ends", "step", "chunk", "all"):
            assert by(form, "mask_" + m), (form, m)
    # the last chunk of one to four steps, full and partial, on the two-slab loop, the one-slab loop and the 256 tile
    for sel in (lambda c: c.plan == B.BY_NAME["l128_rows_d0_vec"].plan and c.k == 1, lambda c: c.plan[:2] == ("lds128", False) and c.k == 1,
                lambda c: c.plan[0] == "lds256" and c.k == 1):
        assert {c.M - 256 for c in wg if c.kind == "x3" and "rows" in c.tags and sel(c)} >= {0, 1, 31, 32, 33, 64, 65, 96, 97}
    assert {c.M for c in by("wave", "rows")} >= {1, 63, 64, 129} and {c.M for c in by("f32", "rows")} >= {1, 63, 64, 129}
    # tile tails one short and one past
    tails = lambda form, t: ({c.N for c in by(form, "tail")}, {c.Cin * c.k for c in by(form, "tail")})          # noqa: E731
    for form, t in (("wave", 64), ("f32", 64), ("lds128", 128)):
        n, k = tails(form, t)
        assert {t - 1, t + 1} <= n and {t - 1, t + 1} <= k, form
    n, k = tails("lds256", 256)
    assert 260 in n and 260 in k and 264 in {c.Cin * c.k for c in by("lds256", "k3")}          # (the 256 tile takes whole float4 groups only ...
    refused = {(c.N, c.Cin) for c in wg if "refused" in c.tags}
    assert {(255, 256), (257, 256), (256, 255), (256, 257), (252, 256), (256, 252)} <= refused          # ... and these shapes refuse it)
    assert all(B.plan_of(c).form == "lds128" for c in wg if "refused" in c.tags)
    # scalar loads three ways and a four-column group that straddles a tap
    assert by("lds128", "scalar_cin") and by("lds128", "scalar_ld") and by("lds128", "scalar_shift") and any(c.N % 4 for c in by("lds128", "tail"))
    assert {c.Cin for c in by("lds128", "straddle")} == {21, 63}
    assert {(c.Cin, c.k) for c in by("f32", "few_channels")} >= {(5, 3), (8, 3)}
    # a masked chunk is a whole workgroup's rows; a chunk boundary inside a sequence on every form
    for c in wg:
        plan, rows = B.plan_of(c), B.block_rows(c, B.plan_of(c))
        if any(t == "mask_chunk" for t in c.tags):
            _, a, b = c.mask
            assert plan.chunks >= 2 and a % rows == 0 and b - a == rows, c.name
        if any(t == "mask_step" for t in c.tags):
            _, a, b = c.mask
            assert a % 32 == 0 and b - a == 32 and (a // 32) % (rows // 32) not in (0,), c.name
    for form in forms:
        assert any(c.k == 3 and B.plan_of(c).chunks >= 2 and B.block_rows(c, B.plan_of(c)) % c.T for c in wg if _form(c) == form), form
    assert any("one_chunk" in c.tags and B.plan_of(c).chunks == 1 and B.plan_of(c).form == "lds128" for c in wg)
    # deterministic: ragged N and K with the bias rows behind several partial tiles; 256 tiles from M * tiles >= 65536 on; pairs
    rag = [c for c in wg if c.det and "ragged" in c.tags]
    assert any(c.N % 4 and c.bias and B.plan_of(c).tile_partials for c in rag) and any((c.Cin * c.k) % 4 and c.k == 3 for c in rag)
    for c in wg:
        if "heavy" in c.tags:
            assert c.M * -(-c.N // 256) * -(-c.Cin * c.k // 256) >= 65536 and B.plan_of(c).form == "lds256", c.name
    heavy = {(c.N, c.Cin, c.k) for c in wg if "heavy" in c.tags and c.det}
    assert heavy == {(1024, 1024, 1), (512, 512, 3)} and B.BY_NAME["det_l256_k3"].T == 36 and B.BY_NAME["det_l256_k3"].M > 5462
    assert 4096 < B.BY_NAME["det_l256_k1"].M < 4200
    a = {c.data: c for c in wg if "pair_a" in c.tags}
    b = {c.data: c for c in wg if "pair_b" in c.tags}
    assert set(a) == set(b) and len(a) == 4 and all(b[d].align == "shift" and a[d].align == "ok" and a[d]._replace(name="", align="", plan=None, tags=())
                                                    == b[d]._replace(name="", align="", plan=None, tags=()) for d in a)
    # f16 planes: the gradient at 1e-9, 1 and 1e6 times the seeded values, |x| up to 4000 -- on every split form
    for form in ("wave", "lds128", "lds256"):
        assert {c.gmul for c in wg if _form(c) == form and "f16" in c.modes} >= {1e-9, 1.0, 1e6}, form
        assert any(c.xmax == 4000.0 for c in by(form, "x4000")), form
        assert by(form, "nobias"), form
    # dgrad
    for group, tile in (("dgrad128", 128), ("dgrad64", 64)):
        cs = B.cases_of(group)
        assert {c.T for c in cs if c.k == 3} >= {1, 2, 3, 7, 33, 36} and {c.Cin for c in cs} >= {tile - 1, tile, tile + 1}
        assert any(c.k == 1 and c.mask == "rand" for c in cs) and min(c.N for c in cs) == 32 and {c.gmul for c in cs} >= {1e-9, 1.0, 1e6}
        assert all(B.layout(c)["ldg"] > c.N for c in cs)          # dy in a wider buffer


def test_the_library_reports_the_mirrors_plan_where_that_needs_no_device():
    """vrd_gemm_wgrad_x3_plan against plan_of for the deterministic cases: their chunking assumes a fixed CU figure and consults no
    switch, so the query runs host arithmetic only (pointers count by their alignment)."""
    from vrdone_amd import _hip
    ptr = lambda off: ctypes.cast(1 << 20 | 4 * off, _hip.c_f32p)          # noqa: E731
    n = 0
    for c in B.CASES:
        if c.kind != "x3" or not c.det:
            continue
        lay, want = B.layout(c), B.plan_of(c)
        out = (ctypes.c_int64 * _hip.WGRAD_PLAN_INTS)()
        rc = _hip.lib.vrd_gemm_wgrad_x3_plan(ptr(lay["cg"]), lay["ldg"], ptr(lay["cx"]), lay["ldx"], c.M, c.N, c.Cin, c.k, ptr(lay["dw_off"]),
                                             1 if c.bias else 0, None, 0, _hip.DETERMINISTIC, out)
        assert rc == 0, _hip.lib.vrd_last_error()
        form = {_hip.WGRAD_WAVE: "wave", _hip.WGRAD_LDS128: "lds128", _hip.WGRAD_LDS256: "lds256"}[out[0]]
        assert (form, bool(out[1]) if form != "wave" else False, out[2], out[3], out[4], bool(out[5])) == tuple(want), (c.name, list(out), want)
        NK = c.N * c.Cin * c.k
        assert out[6] >= (want.chunks * NK if want.tile_partials else 0) + (want.chunks * c.N if c.bias and want.tile_partials else 0), c.name
        n += 1
    assert n >= 20
    out = (ctypes.c_int64 * _hip.WGRAD_PLAN_INTS)()
    assert _hip.lib.vrd_gemm_wgrad_x3_plan(ptr(0), 8, ptr(0), 8, 4, 16, 8, 1, ptr(0), 0, None, 0, 0, out) != 0          # ldg < N
    assert b"vrd_gemm_wgrad_x3_plan" in _hip.lib.vrd_last_error()


FAULT_CASES = [("row_dropped_at_chunk_boundary", "l128_mask_none", "dW"), ("row_dropped_at_chunk_boundary", "l256_mask_none_k3", "dW"),
               ("row_dropped_at_chunk_boundary", "f32_mask_none_k3", "dW"), ("row_dropped_at_chunk_boundary", "wave_mask_none", "dW"),
               ("tap_across_sequence_end", "l128_k3_t3_scalar", "dW"), ("tap_across_sequence_end", "l256_k3_t33", "dW"),
               ("tap_across_sequence_end", "f32_k3_t1_c5", "dW"), ("tap_across_sequence_end", "wave_k3_t100", "dW"),
               ("rows_past_m_contracted", "l128_mask_none", "dW"), ("rows_past_m_contracted", "l256_mask_none", "dW"),
               ("lo_hi_product_left_out", "l128_rows_d1_vec", "dW"), ("lo_hi_product_left_out", "wave_m129", "dW"),
               ("k_tail_from_neighbouring_tap", "l128_k3_t7_scalar", "dW"), ("k_tail_from_neighbouring_tap", "l128_tail_k3_c43", "dW"),
               ("mask_byte_of_neighbouring_row", "l128_rows_d0_vec", "dW"), ("mask_byte_of_neighbouring_row", "l256_mask_ends", "dW"),
               ("partial_tile_missing", "l256_rows_d1", "dW"), ("partial_tile_missing", "det_l128_ragged_n127_c129_k1", "dW"),
               ("dw_overwritten", "l128_one_chunk", "dW"), ("dw_overwritten", "wave_m1", "dW"), ("dw_overwritten", "l256_rows_d97", "dW"),
               ("bias_from_unmasked_rows", "l128_mask_ends", "db"), ("bias_from_unmasked_rows", "det_l128_mask_chunk", "db")]


@pytest.mark.parametrize("fault,name,what", FAULT_CASES)
def test_each_stand_in_fault_is_reported(fault, name, what):
    assert fault in B.FAULTS and {f for f, _, _ in FAULT_CASES} == set(B.FAULTS)
    case = B.BY_NAME[name]
    for mode in case.modes:
        if fault == "lo_hi_product_left_out" and mode == "f32":
            continue
        with pytest.raises(AssertionError, match=f"{what}: .* outside the bound") as e:
            run(case, mode, fault)
        assert name in str(e.value) and f"[{mode}]" in str(e.value)


def test_stale_scratch_and_written_guards_are_reported():
    """a partial tile that was never written leaves NaN in dW; a store beyond dW, db or the scratch changes a guard"""
    case = B.BY_NAME["l128_mask_chunk"]
    inp, plan = B.make_inputs(case, "bf16"), B.plan_of(case)
    B.emulate(inp, plan)
    inp.fW.view[5] += W.sentinel()
    with pytest.raises(AssertionError, match="not finite"):
        B.verify(inp, plan)
    inp = B.emulate(B.make_inputs(case, "bf16"), plan)
    inp.fW.buf[inp.fW.start + inp.fW.n] = 0.0
    with pytest.raises(AssertionError, match="guard elements of 'dW'"):
        B.verify(inp, plan)
    inp = B.emulate(B.make_inputs(case, "bf16"), plan)
    inp.hX.buf[0, 0] = 1.0
    with pytest.raises(AssertionError, match="input buffer was written"):
        B.verify(inp, plan)


def test_a_report_names_tile_tap_and_channel():
    with pytest.raises(AssertionError) as e:
        run(B.BY_NAME["l256_k3_t33"], "f16", "tap_across_sequence_end")
    msg = str(e.value)
    assert "case l256_k3_t33 [f16] dW" in msg and "256 x 256 tile (" in msg and "tap " in msg and "channel " in msg
    assert "got " in msg and "want " in msg and "bound " in msg


def test_the_absmax_exponent_puts_the_largest_gradient_into_the_f16_headroom():
    for scale in (1e-9, 1.0, 1e6, 2.0 ** 13, 2.0 ** 14 - 1):
        t = torch.tensor([[0.3 * scale, -scale]])
        e = B.absmax_exp(t)
        assert 2.0 ** 13 <= scale * 2.0 ** e < 2.0 ** 14
    assert B.absmax_exp(torch.zeros(2, 2)) == 0
