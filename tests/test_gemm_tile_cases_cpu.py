"""The case table, reference, tolerance and checker of tests/gemm_tile_cases.py against an f32 emulation of the three-product
arithmetic on the CPU: the emulation passes every case of the table in both split modes -- which shows that the float64
reference alone stays inside the derived bound --, and each Python stand-in of a kernel fault, the classes
tests/test_gpu_gemm_tiles.py exists to catch, is reported.  No GPU, and no wrong kernel is ever run on one."""
import pytest
import torch

import gemm_tile_cases as G
import window_cases as W


@pytest.fixture(autouse=True)
def no_grad():
    with torch.no_grad():
        yield


def run(case, mode, fault=None):
    inp = G.make_inputs(case, mode)
    if mode == "f16x1":          # (the one-product cases: against tests/f16x1_emulation.py, relative to the three-product result)
        G.emulate(inp, products=3)
        for p in inp.problems:
            p.got3 = p.hC.result()
        G.emulate(inp, products=1)
    else:
        G.emulate(inp, fault)
    return G.verify(inp)


def test_the_table_is_what_the_kernels_admit():
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)
    for c in G.CASES:
        M, K = c.B * c.T, c.Cin * c.k
        assert M < 2048 and c.Cin % 32 == 0 and c.groups and set(c.groups) <= set(G.GROUP_ENV)
        if set(c.groups) & set(G.BIG_GROUPS):          # choose_x3 and gemm_epilogue_lean_ok (vrd_gemm.hip, vrd_gemm_epilogue.h)
            assert M % 64 == 0 and c.N % 64 == 0 and c.N >= 256 and K >= 96 and (c.k == 1 or c.T >= 32), c.name
            assert "relu" not in c.epi and ("gelu" not in c.epi or set(c.epi) <= {"bias", "gelu"}), c.name
            if c.modes == ("f16x1",):
                assert c.Cin % 64 == 0 and K >= 192, c.name
        if "dma" in c.groups:                          # gemm_x3_dma_ok
            assert c.N >= 192, c.name
        if c.pair_out:
            assert c.N % 32 == 0, c.name
        if c.layout in ("pad_map", "pad_skip"):
            assert M % 32 == 0, c.name
        if c.agree:
            assert set(G.ALL6) <= set(c.groups), c.name
    # the K-step counts, ring phases and tails the table exists for
    big = [c for c in G.CASES if "big" in c.groups or "big_grid2" in c.groups]
    assert {c.Cin * c.k // 32 for c in big if c.modes == G.X3} >= set(range(3, 10))
    assert {c.Cin // 32 for c in G.cases_of("dma") if c.k == 1} >= {1, 2, 3, 4, 5, 7}
    assert {(c.B * c.T) % 256 for c in G.cases_of("big")} >= {0, 64, 128, 192} and {c.N % 256 for c in G.cases_of("big")} >= {0, 64, 128, 192}
    ring5 = G.BY_NAME["big_ring_c160"]                 # nkt = 5, seven tiles per workgroup: g0 = 0, 5, 4, 3, 2, 1, 0
    assert {(5 * i) % 6 for i in range(7)} == set(range(6)) and ring5.B * ring5.T // 256 * (ring5.N // 256) == 14


def test_pair_rows_round_trip():
    x = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(2)) * 3
    for f16 in (False, True):
        raw = G.encode_pair(x, f16)
        assert raw.shape == x.shape and raw.dtype == torch.float32
        dec = G.decode_pair(raw, f16)
        assert float(((dec - x.double()).abs() / x.double().abs().clamp_min(1e-3)).max()) < 2.0 ** -15
        hi, lo = G.pair_planes(raw, f16)
        assert torch.equal(hi, (x * (16.0 if f16 else 1.0)).to(torch.float16 if f16 else torch.bfloat16).float())
        assert torch.equal(G.decode_pair(G.encode_pair(dec.float(), f16), f16), dec)          # hi + lo survives the split unchanged


def test_padding_cases_have_the_tiles_they_are_for():
    c = G.BY_NAME["big_ring_c160_pad_skip"]
    inp = G.make_inputs(c, "bf16x3")
    counts, seg_len = G.segment_counts(inp.mask)
    assert seg_len == 8 and counts == [0, 1, 1, 0, 1, 1, 1]          # one 256-row tile per segment: tiles 0 and 3 skip
    # (tile_of in vrd_gemm_x3_big.hip, 14 tiles on 2 workgroups: workgroup 0 walks row tiles 0 2 4 6 0 2 4, workgroup 1 walks 1 3 5 6 1 3 5)
    assert int(G.valid_block_rows(inp).sum()) == 5 * 32
    for c in G.CASES:
        if c.layout == "pad_map":
            blocks = G.make_inputs(c, "bf16x3").mask.reshape(-1, 32).any(1)
            assert 0 < int((~blocks).sum()) < len(blocks), c.name


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3", "f16x1"])
def test_the_emulation_passes_every_case(mode):
    worst = {}
    for c in G.CASES:
        if mode in c.modes:
            r = run(c, mode)
            assert r < 1.0
            worst[c.name] = r
    assert worst
    top = max(worst, key=worst.get)
    print(f"{mode}: {len(worst)} cases, largest error-to-bound ratio {worst[top]:.3f} ({top})")


FAULT_CASES = [("dropped_product", "big_ksteps_c160", "outside the bound"), ("dropped_product", "big_ksteps_c96", "outside the bound"),
               ("stale_first_step", "big_ksteps_c160", "outside the bound"), ("stale_first_step", "big_ring_c160_gelu", "outside the bound"),
               ("blocks_exchanged", "big_ksteps_c128_mask", "outside the bound"), ("blocks_exchanged", "big_tail_m320_n320", "outside the bound"),
               ("tile_unwritten", "big_tail_m576_n448", "not finite"), ("tile_unwritten", "big_tail_m576_n448_pair", "not finite"),
               ("tap_reads_neighbour_first", "big_k3_t36_c32", "outside the bound"), ("tap_reads_neighbour_last", "big_k3_t36_c32", "outside the bound"),
               ("tap_reads_neighbour_first", "dma_k3_t7_c64", "outside the bound"), ("tap_reads_neighbour_last", "dma_k3_t1_c32", "outside the bound"),
               ("column_tail_overrun", "big_tail_m320_n320", "guard elements"), ("column_tail_overrun", "dma_tail_m130_n197", "guard elements")]


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("fault,name,message", FAULT_CASES)
def test_each_stand_in_fault_is_reported(fault, name, message, mode):
    assert fault in G.FAULTS
    with pytest.raises(AssertionError, match=message) as e:
        run(G.BY_NAME[name], mode, fault)
    assert name in str(e.value) and mode in str(e.value)
    assert {f for f, _, _ in FAULT_CASES} == set(G.FAULTS)


def test_a_report_names_tile_row_and_frame():
    """what a failure says: readable without a second run"""
    c = G.BY_NAME["big_k3_t36_c32"]
    with pytest.raises(AssertionError) as e:
        run(c, "f16x3", "tap_reads_neighbour_first")
    msg = str(e.value)
    assert "case big_k3_t36_c32 [f16x3]" in msg and "frame 0 of 36 in sequence" in msg and "256x256 tile (" in msg and "128x256 tile (" in msg
    assert "got " in msg and "want " in msg and "bound " in msg


def test_the_bound_is_tighter_than_the_old_constants_allow_at_small_k():
    """at K <= 96 a correct bf16x3 product exceeds the 3e-6 of test_gemm_split_bf16_precision (measured at K >= 256), and the
    derived bound still holds it"""
    c = G.BY_NAME["dma_ksteps_c32"]
    inp = G.emulate(G.make_inputs(c, "bf16x3"))
    ref, mag, lip = G.reference(inp, inp.problems[0])
    rel = float(((inp.problems[0].hC.result().double() - ref).abs() / mag).max())
    assert 3e-6 < rel < G.U["bf16x3"] + 3 * 2.0 ** -24
