"""Training dropout without a GPU: the host mirror of the keep decisions (vrdone_amd/dropout.py) against the published
Philox4x32-10 known-answer vectors and its own statistics, the continued-row rule, the C ABI additions, the model option and the
refusals that remain, and the reference fixture's recorded masks (tests/golden/train_step_vidvrd_dropout.npz,
scripts/make_golden_dropout.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from vrdone_amd import dropout as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's kat_vectors for philox4x32-10: (counter, key, result)
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = D.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_words_are_the_counter_blocks_words():
    """id takes word id & 3 of the block with counter (id >> 2 low, high, site, 0) and key = the seed's two words"""
    seed, site = 0x299F31D0A4093822, 0x13198A2E
    first = np.uint64((0x05A308D3 << 34) | (0x243F6A88 << 2))           # block (0x243f6a88, 0x05a308d3): an id beyond 2^62
    got = D.words(seed, site, first + np.arange(4, dtype=np.uint64))
    want = D.philox4x32_10(np.array([0x243F6A88, 0x05A308D3, site, 0], dtype=np.uint64), np.array([0xA4093822, 0x299F31D0], dtype=np.uint64))
    assert got.tolist() == want.tolist()
    # an unaligned run crosses blocks where id & 3 wraps
    run = D.words(seed, site, first + np.uint64(2) + np.arange(5, dtype=np.uint64))
    nxt = D.words(seed, site, first + np.uint64(4) + np.arange(4, dtype=np.uint64))
    assert run.tolist() == want[2:].tolist() + nxt[:3].tolist()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    """|rate - (1 - p)| <= 5 sqrt(p (1 - p) / n) on 120 x 512 ids (6.1e-3 at p = 0.1, 1.0e-2 at p = 0.5)"""
    n = 120 * 512
    for seed, site in ((1, D.site_id("backbone.stem.0.attn.proj_drop")), (0xFEDCBA9876543210, 7)):
        keep = D.keep_mask(seed, site, 0, n, p)
        assert keep.dtype == np.uint8 and set(np.unique(keep)) <= {0, 1}
        assert abs(float(keep.mean()) - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)
    assert D.threshold(p) == int(np.floor(float(np.float32(p)) * 2.0 ** 32))
    assert D.keep_scale(p).dtype == np.float32 and D.keep_scale(p) == np.float32(1) / (np.float32(1) - np.float32(p))
    assert D.keep_mask(3, 4, 0, 1000, 0.0).all()


def test_two_calls_of_b_equal_one_call_of_2b():
    """The continued-row rule: a module's second call continues where its first ended."""
    seed, B, T, C, H, W = 99, 3, 10, 12, 4, 7
    site = D.site_id("backbone.stem.1.mlp.2")
    whole = D.row_mask(seed, site, 0, 2 * B * T, C, 0.5)
    assert np.array_equal(np.concatenate([D.row_mask(seed, site, 0, B * T, C, 0.5), D.row_mask(seed, site, B * T, B * T, C, 0.5)]), whole)
    assert np.array_equal(whole.reshape(-1), D.keep_mask(seed, site, 0, 2 * B * T * C, 0.5))
    att = D.attn_mask(seed, site, 0, 2 * B * T, H, W, 0.5)
    assert np.array_equal(np.concatenate([D.attn_mask(seed, site, 0, B * T, H, W, 0.5), D.attn_mask(seed, site, B * T, B * T, H, W, 0.5)]), att)
    assert att.shape == (2 * B * T, H, W) and int(D.attn_ids(5, 2, H, W)[1, 2, 3]) == (6 * H + 2) * W + 3
    assert int(D.row_ids(5, 2, C)[1, 3]) == 6 * C + 3
    # ids beyond 2^32 are their own elements, not the low words' again
    assert not np.array_equal(D.keep_mask(seed, site, 2 ** 40, 256, 0.5), D.keep_mask(seed, site, 0, 256, 0.5))
    assert D.site_id("backbone.stem.0.attn.attn_drop") == 1935489813


NEW = ("vrd_dropout_mask", "vrd_dropout_rows", "vrd_local_attn_drop", "vrd_local_attn_drop_bwd")


def test_new_symbols_are_declared_bound_and_exported():
    from vrdone_amd import _hip
    header = open(os.path.join(REPO, "include", "vrdone_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _hip._SIGNATURES and hasattr(_hip.lib, name), name
    assert re.search(r"#define VRD_ABI_VERSION 37\b", header) and _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    # the entry points these mirror keep their prototypes
    assert len(_hip._SIGNATURES["vrd_local_attn"][1]) == 15 and len(_hip._SIGNATURES["vrd_local_attn_bwd"][1]) == 19
    assert len(_hip._SIGNATURES["vrd_local_attn_drop"][1]) == 18 and len(_hip._SIGNATURES["vrd_local_attn_drop_bwd"][1]) == 23


def test_bad_rates_are_refused_before_any_launch():
    from vrdone_amd import _hip
    for p in (1.0, -0.1):
        assert _hip.lib.vrd_dropout_mask(None, 0, 0, 4, p, None, None) != 0
    assert _hip.lib.vrd_dropout_rows(None, 4, 1, 4, None, 0, 0, 0.5, None, 4, None) != 0
    assert b"vrd_dropout_rows" in _hip.lib.vrd_last_error()


def test_model_with_both_keys_builds_and_loads_a_rate_zero_state_dict():
    from vrdone_amd.models.blocks import TransformerBlock
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, _ = load_case("vidvrd")
    plain = MaskVRD(dict(mc), device="cpu")
    mc = dict(mc, dropattn=0.1, dropout=0.1)
    model = MaskVRD(mc, device="cpu")
    assert list(model.state_dict()) == list(plain.state_dict())
    model.load_state_dict(plain.state_dict(), strict=True)
    assert model.dropout_rates == (0.1, 0.1) and model.dropout_seed is None and plain.dropout_rates == (0.0, 0.0)
    blocks = {n: m for n, m in model.named_modules() if isinstance(m, TransformerBlock)}
    assert sorted(blocks) == [f"backbone.branch.{i}" for i in range(3)] + [f"backbone.stem.{i}" for i in range(2)]
    for name, blk in blocks.items():
        assert blk.drop_sites == {k: D.site_id(f"{name}.{k}") for k in ("mlp.2", "mlp.4")}
        assert blk.attn.drop_sites == {k: D.site_id(f"{name}.attn.{k}") for k in ("attn_drop", "proj_drop")}
        assert blk._drop_rates == {"mlp.2": 0.1, "mlp.4": 0.1} and blk.attn._drop_rates == {"attn_drop": 0.1, "proj_drop": 0.1}
        # the rule of AffineDropPath.row_factors: training AND autograd recording
        blk.train()
        with torch.enable_grad():
            assert blk.dropout_active() and blk.attn.dropout_active()
        with torch.no_grad():
            assert not blk.dropout_active()
        blk.eval()
        with torch.enable_grad():
            assert not blk.dropout_active() and not blk.attn.dropout_active()
    for blk in (m for m in plain.modules() if isinstance(m, TransformerBlock)):
        blk.train()
        with torch.enable_grad():
            assert not blk.dropout_active() and not blk.attn.dropout_active()


def test_recording_key_follows_rates_and_pinned_seed():
    from vrdone_amd import train_graph
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, _ = load_case("vidvrd")
    x, m = torch.zeros(2, 3, 4), torch.zeros(2, 4)
    a, b = MaskVRD(dict(mc), device="cpu"), MaskVRD(dict(mc, dropattn=0.1), device="cpu")
    assert train_graph.recording_key(a, x, m) != train_graph.recording_key(b, x, m)
    free = train_graph.recording_key(b, x, m)
    b.dropout_seed = 5
    assert train_graph.recording_key(b, x, m) != free


def test_out_of_scope_refusals_name_their_key():
    from vrdone_amd.models import blocks, local_transformer as LT
    from vrdone_amd.models.maskvrd import MaskVRD
    with pytest.raises(AssertionError, match="MaskedMHCA: attn_pdrop"):
        blocks.MaskedMHCA(512, 4, 1, 1, attn_pdrop=0.1)
    with pytest.raises(AssertionError, match="MaskedMHCA: attn_pdrop"):
        blocks.TransformerBlock(512, 4, attn_pdrop=0.1, mha_win_size=-1)
    blocks.TransformerBlock(512, 4, proj_pdrop=0.1, mha_win_size=-1)              # in scope: proj_drop and the MLP sites
    for kw, what in ((dict(attn_pdrop=0.1), "attn_pdrop"), (dict(proj_pdrop=0.1), "proj_pdrop")):
        with pytest.raises(AssertionError, match="MaskedMHA: " + what):
            blocks.MaskedMHA(512, 4, **kw)
        with pytest.raises(AssertionError, match="MaskedMHA: " + what):
            LT.MaskedMHA_QKV(512, 4, **kw)
        with pytest.raises(AssertionError, match="MaskedMHCA_QKV: " + what):
            LT.MaskedMHCA_QKV(512, 4, **kw)
        with pytest.raises(AssertionError, match="LocalMaskedMHCA_QKV: " + what):
            LT.LocalMaskedMHCA_QKV(512, 4, 9, n_qx_stride=1, **kw)
        with pytest.raises(AssertionError, match="MaskedConvTransformerDecoderLayer: " + what):
            LT.MaskedConvTransformerDecoderLayer(512, 4, **kw)
    with pytest.raises(AssertionError, match="ConvMLP: drop"):
        blocks.ConvMLP(512, 512, 512, 2, drop=0.1)
    mc, _, _ = load_case("vidvrd")
    for key in ("attn_pdrop", "proj_pdrop"):                                      # the predictor's own keys
        cfg = dict(mc, predictor=dict(mc["predictor"], **{key: 0.1}))
        with pytest.raises(AssertionError, match="MaskedConvTransformerDecoderLayer: " + key):
            MaskVRD(cfg, device="cpu")
    with pytest.raises(AssertionError, match="outside"):
        blocks.TransformerBlock(512, 4, proj_pdrop=1.0, mha_win_size=7)


def test_standalone_module_needs_a_step():
    from vrdone_amd.models import blocks
    blk = blocks.TransformerBlock(512, 4, proj_pdrop=0.5, mha_win_size=7).train()
    blocks._dropout_step.seeds.clear()
    with torch.enable_grad(), pytest.raises(RuntimeError, match="begin_dropout_step"):
        blk._drops(2, 8, "cpu")
    seed = blocks.begin_dropout_step(blk, "cpu", seed=(1 << 64) - 2)
    assert seed.dtype == torch.int64 and int(seed) == -2                           # the 64-bit word, as torch stores it
    with torch.enable_grad():
        first, second = blk._drops(2, 8, "cpu"), blk._drops(3, 8, "cpu")
    assert first["mlp.2"].row0 == 0 and second["mlp.2"].row0 == 16 and blk._drop_samples == 5
    assert first["mlp.4"].site == D.site_id("mlp.4") and first["mlp.2"].p == 0.5 and first["mlp.2"].seed is seed
    blocks.begin_dropout_step(blk, "cpu", seed=1)
    assert blk._drop_samples == 0


def _fixture():
    z = np.load(os.path.join(GOLDEN, "train_step_vidvrd_dropout.npz"))
    return z, json.loads(str(z["meta"]))


def test_fixture_masks_regenerate_from_its_seed():
    z, meta = _fixture()
    assert meta["dropattn"] == 0.1 and meta["dropout"] == 0.1 and meta["B"] == 24 and meta["T"] == 96
    blocks = [f"backbone.stem.{i}" for i in range(2)] + [f"backbone.branch.{i}" for i in range(3)]
    assert meta["sites"] == {f"{b}.{s}": D.site_id(f"{b}.{s}") for b in blocks for s in D.BLOCK_SITES}
    calls = meta["mask_calls"]
    # a stem block runs once per stream (two calls of 24 samples, the second continuing the first), a branch block once
    per_site = {}
    for c in calls:
        per_site.setdefault(c["site"], []).append(c["sample0"])
    assert set(per_site) == set(meta["sites"])
    assert all(v == ([0, 24] if ".stem." in k else [0]) for k, v in per_site.items()), per_site
    n = meta["mask_bits"]
    for i, c in enumerate(calls):
        site, shape = meta["sites"][c["site"]], c["shape"]
        if len(shape) == 4:                                  # att (B, T', n_head, window): id order
            B, T, H, Wn = shape
            want = D.attn_mask(meta["seed"], site, c["sample0"] * T, B * T, H, Wn, meta["dropattn"]).reshape(-1)[:n]
        else:                                                # (B, C, T'): the first n elements are sample 0, channels 0 .., frames 0 .. T' - 1
            B, C, T = shape
            flat = np.arange(n)
            ids = (np.uint64(c["sample0"] * T) + (flat % T).astype(np.uint64)) * np.uint64(C) + (flat // T).astype(np.uint64)
            assert n <= C * T
            want = D.keep_ids(meta["seed"], site, ids, meta["dropout"])
        assert np.array_equal(np.unpackbits(z[f"mask/{i}"])[:n], want), c
    assert os.path.getsize(os.path.join(GOLDEN, "train_step_vidvrd_dropout.npz")) <= min(
        1 << 20, os.path.getsize(os.path.join(GOLDEN, "train_step_vidvrd.npz")))
