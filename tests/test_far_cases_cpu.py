"""The case table of tests/far_cases.py: every case crosses the offset lines derived from vrdone_amd/configs.py, no period divides
a wrap distance, the checker of tests/test_gpu_far_rows.py sees each faulty address model that the shipped sizes can reach, and
every case fits the memory cap.  Index arithmetic only: no GPU, no large memory, and no wrong kernel is ever run."""
import pytest
import torch

import far_cases as Fc

CASES = list(Fc.CASES.values())
ids = [c.name for c in CASES]


def test_the_lines_follow_from_the_shipped_configs():
    """recomputed here from configs.py, not read from the table: today's configs give exactly the classes the table was built on"""
    from vrdone_amd import configs
    need = {}
    for name in ("vidvrd", "vidor", "vidor_local", "vidor_x"):
        cfg = configs.model_config(name)
        rows = 2 * (2048 + 2048 // 4) * cfg["max_seq_len"]                  # MaskVRD._chunk_size: one wave up to 1.25 x pair_chunk
        widths = dict(fpn=cfg["fpn_dim"], embd=cfg["embd_dim"], qkv=3 * cfg["embd_dim"], hidden=4 * cfg["embd_dim"],
                      ent_box=cfg["bbox_entity_dim"], so_box=cfg["bbox_so_dim"], visual=cfg["visual_dim"])
        ext = {k: rows * w * 4 for k, w in widths.items()}
        ext["edge_pieces"] = 2 * 2560 * 16 * cfg["embd_dim"] * 4          # two window-edge pieces of 8 frames per entity stream
        ext["source"] = 4096 * configs.input_channels(cfg) * cfg["max_seq_len"] * 4
        for k, e in ext.items():
            need.setdefault(k, set()).update(ln for ln, at in Fc.LINES.items() if e > at)
    for cls, lines in need.items():
        assert set(Fc.required_lines(cls)) == lines, cls
    assert need["embd"] == {"L31B", "L32B"} and need["hidden"] == need["source"] == set(Fc.LINES) and need["fpn"] == {"L31B"}
    assert need["ent_box"] == need["so_box"] == need["edge_pieces"] == set() and need["visual"] == need["qkv"] == {"L31B", "L32B", "L31E"}


def test_the_wave_size_is_the_models():
    from vrdone_amd.models.maskvrd import MaskVRD
    from vrdone_amd import configs
    model = MaskVRD(configs.model_config("vidvrd"), device="cpu")
    assert model._chunk_size(Fc.WAVE_PAIRS) == Fc.WAVE_PAIRS and model._chunk_size(Fc.WAVE_PAIRS + 1) < Fc.WAVE_PAIRS


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_every_buffer_crosses_its_lines_with_a_full_and_a_ragged_tile_behind(case):
    for b in case.bufs:
        rows = case.rows(b)
        for ln in Fc.required_lines(b.cls):
            first = -(-Fc.LINES[ln] // b.pitch_bytes)                          # the first row that starts behind the line
            tile = -(-case.tile * b.seq_rows // min(x.seq_rows for x in case.bufs)) if b.seq_rows > 1 else 1
            assert rows - first > tile, (b.name, ln, rows, first, tile)
    if case.unit == 1:
        assert case.rows() % 64 == 7                                       # a ragged last tile at any tile size
    else:
        assert case.rows() % case.seq_len == 0
    assert case.guard_rows() == 2                                          # poisoned rows behind the last row of every output
    assert case.seq_len == Fc.T or case.why, "a sequence length other than 64 needs its reason"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_no_period_divides_a_wrap_distance(case):
    for b in case.bufs:
        for model in Fc.MODELS:
            assert Fc.wrap_distance_ok(case, b, model), (b.name, model)
        # stated in rows, as a power-of-two pitch allows: the wrap distance in rows modulo the period is non-zero
        if b.pitch & (b.pitch - 1) == 0:
            for _, wrap, _ in Fc.MODELS.values():
                assert (wrap // b.pitch_bytes) % case.period_rows(b) != 0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_each_reachable_faulty_address_model_is_seen(case):
    """Every row behind a model's line shows the fault: as poison (an output row written elsewhere) or as other data (an input row
    read from a place that is no whole number of periods away, or from outside the buffer).  A model whose line no shipped size of
    the buffer's class reaches (an element index at a 512-wide buffer) cannot show, in the test or in the product."""
    reached = set()
    for b in case.bufs:
        for model, (line, _, _) in Fc.MODELS.items():
            behind, shown = Fc.sees(case, b, model)
            if line in Fc.required_lines(b.cls):
                assert behind > 0 and shown == behind, (b.name, model, behind, shown)
                reached.add(model)
            else:
                assert behind == 0
    lines = {ln for b in case.bufs for ln in Fc.required_lines(b.cls)}
    assert reached == {m for m, (line, _, _) in Fc.MODELS.items() if line in lines} and reached


def test_wrapped_offsets():
    assert Fc.wrapped((1 << 31) + 8, "signed byte offset") == 8 - (1 << 31) and Fc.wrapped((1 << 31) + 8, "unsigned byte offset") == (1 << 31) + 8
    assert Fc.wrapped((1 << 32) + 8, "unsigned byte offset") == 8 and Fc.wrapped((1 << 32) + 8, "signed element index") == (1 << 32) + 8
    assert Fc.wrapped((1 << 33) + 8, "signed element index") == 8 - (1 << 33) and Fc.wrapped((1 << 34) + 8, "unsigned element index") == 8


def test_a_period_that_divides_the_wrap_distance_would_be_blind():
    """the condition is not vacuous: 64 sequences of 64 rows at a 2 KiB pitch repeat exactly at 2^32 bytes"""
    c = Fc.CASES["layernorm_512_plain"]
    b = c.bufs[0]
    assert (1 << 32) % (64 * 64 * b.pitch_bytes) == 0 and (1 << 32) % (c.period_rows(b) * b.pitch_bytes) != 0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fits_the_memory_cap(case):
    assert case.bytes() + (64 << 20) <= Fc.MEMORY_CAP, f"{case.bytes() / 2 ** 30:.2f} GiB"


def test_the_table_covers_the_families():
    names = set(Fc.CASES)
    for must in ("bct_to_btc_vec", "bct_to_btc_scalar", "btc_to_bct", "pack_pairs", "gather_pairs", "assemble_pairs", "layernorm_256_plain", "layernorm_512_pair", "conv_ln_entity",
                 "dwconv_ln_row_groups", "maxpool_mask", "activation_gelu", "local_attn_hd32_w3", "local_attn_segs_hd128_w19_rel",
                 "gemm_f32_k1", "gemm_x3_k3", "gemm_big_k1", "gemm_dma_k3", "gemm_mlp_split", "attention_flash_f32rows",
                 "attention_pair_w64_hd128", "attention_pair_w32_hd32"):
        assert must in names, must
    assert {f"dwconv_ln_{k}" for k in Fc.DW_CASES} <= names
    k = Fc.SLAB_FALLBACK
    assert k["Tk"] * k["ldkv"] * 4 >= 1 << 31 and k["B"] * k["Tk"] * k["ldkv"] * 4 < Fc.MEMORY_CAP          # one item's K / V slab: 2 GiB and more


def test_the_sentinel_survives_int32_views():
    import window_cases as W
    assert int(torch.full((1,), W.SENTINEL_BITS, dtype=torch.int32).view(torch.float32).view(torch.int32)) == W.SENTINEL_BITS
