"""Global attention over a ragged row space in one call (vrd_attention_pair_segs) without a GPU: the entry is declared, exported
and bound at ABI 37, its host-side argument checks refuse by name, and ragged.attention takes the route only when it is switched
on (ragged.ATTN_SEGS / VRDONE_ROWS_ATTN_SEGS=1), for pair-row operands, in runs of 32 row groups."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vrd_attention_pair_segs"


def test_entry_is_declared_exported_and_bound():
    from vrdone_amd import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vrdone_hip.h")).read(), flags=re.S)
    assert "#define VRD_ABI_VERSION 37" in header and _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    proto = re.search(r"int vrd_attention_pair_segs\(([^)]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    assert names == ["q", "ldq", "k", "v", "ldkv", "kv_mask", "q_mask", "qsegs", "ksegs", "n_head", "head_dim", "out", "ldo", "out_pair",
                     "pair_fmt", "stream", "products"]
    restype, argtypes = _hip._SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(names)
    assert argtypes[7] is argtypes[8] and argtypes[7]._type_ is _hip.RowSegs
    assert getattr(_hip.lib, NAME).argtypes == argtypes               # (resolving the attribute is the export check)


def _table(groups):
    from vrdone_amd import _hip
    t = _hip.RowSegs()
    t.count = len(groups)
    for i, (row, n, T) in enumerate(groups[:_hip.MAX_SEGS]):
        t.row[i], t.n[i], t.T[i] = row, n, T
    return t


def _call(qg, kg, H=4, hd=64, fmt=2, products=0):
    """host-side validation happens before any device access: dummy (aligned, non-null) addresses suffice"""
    from vrdone_amd import _hip
    tq, tk = _table(qg), _table(kg)
    rc = _hip.lib.vrd_attention_pair_segs(256, 512, 256, 256, 512, None, None, ctypes.byref(tq), ctypes.byref(tk), H, hd, 256, 512, 0, fmt, None,
                                          products)
    return rc, _hip.lib.vrd_last_error().decode()


G2 = [(0, 2, 64), (128, 1, 32)]
REFUSALS = {
    "count 0": (dict(qg=[], kg=[]), "groups"),
    "count 33": (dict(qg=[(32 * i, 1, 32) for i in range(33)], kg=[(32 * i, 1, 32) for i in range(33)]), "groups"),
    "tables disagree in count": (dict(qg=G2, kg=G2[:1]), "disagree"),
    "tables disagree in n": (dict(qg=G2, kg=[(0, 2, 64), (128, 2, 32)]), "disagree"),
    "T = 0": (dict(qg=[(0, 2, 64), (128, 1, 0)], kg=G2), "sizes"),
    "Tk = 0": (dict(qg=G2, kg=[(0, 2, 0), (0, 1, 32)]), "sizes"),
    "head_dim 16": (dict(qg=G2, kg=G2, H=16, hd=16), r"head_dim must be .*\(got 16\)"),
    "products 1 at head_dim 32": (dict(qg=G2, kg=G2, H=8, hd=32, products=1), "head_dim 32 has no one-product form"),
    "Tk 4097": (dict(qg=G2, kg=[(0, 2, 64), (128, 1, 4097)]), "4097.*4096 keys"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_host_side_refusals_name_the_entry(case):
    kw, what = REFUSALS[case]
    rc, msg = _call(**kw)
    assert rc < 0 and msg.startswith(NAME + ":") and re.search(what, msg), (rc, msg)


# ------------------------------------------------------------------------------------------------------ ragged.attention
class _Recorder:
    """stands in for ops.attention: records every call, returns what the real one would (out, as a Pair when pair=True)"""

    def __init__(self, ops):
        self.ops, self.calls = ops, []

    def __call__(self, q, k, v, kv_mask, n_head, algo=0, pair=False, q_mask=None, out=None, segs=None):
        self.calls.append(dict(q=q, k=k, segs=segs, out=out, kv_mask=kv_mask, q_mask=q_mask))
        if out is None:
            out = torch.empty(tuple(q.shape))
        return self.ops.Pair(out, out.shape[-1], q.fmt) if pair and isinstance(q, self.ops.Pair) else out


@pytest.fixture
def route(monkeypatch):
    from vrdone_amd import ops
    from vrdone_amd.models import ragged
    rec = _Recorder(ops)
    monkeypatch.setattr(ops, "attention", rec)
    monkeypatch.setattr(ragged, "ATTN_LANES", 1)                      # (no side streams: there is no device here)
    return ragged, ops, rec


def _operands(ops, lay, as_pair, Cw=256):
    t = [torch.zeros(1, lay.rows, Cw) for _ in range(3)]
    mask = torch.ones(1, lay.rows, dtype=torch.bool)
    return ([ops.Pair(x, Cw, 2) for x in t] if as_pair else t), mask


def test_switch_is_off_by_default_and_a_module_value():
    from vrdone_amd.models import ragged
    assert os.environ.get("VRDONE_ROWS_ATTN_SEGS", "0") == "1" or ragged.ATTN_SEGS is False


def test_switched_on_a_multi_group_global_call_is_one_segs_call(route, monkeypatch):
    ragged, ops, rec = route
    monkeypatch.setattr(ragged, "ATTN_SEGS", True)
    lay = ragged.Layout([(3, 32, True), (1, 40, True), (2, 96, True)])
    (q, k, v), mask = _operands(ops, lay, True)
    r = ragged.attention(q, k, v, mask, mask, 4, lay, lay, pair=True)
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert c["segs"] == (lay.segs, lay.segs) and c["q"] is q and c["k"] is k and c["kv_mask"] is mask and c["q_mask"] is mask
    assert sum(n * T for _, n, T in c["segs"][0]) == lay.rows == c["out"].shape[1]
    assert isinstance(r, ops.Pair) and r.t is c["out"] and r.t.shape == (1, lay.rows, 256)


def test_switched_off_and_for_f32_rows_the_buckets_are_walked(route, monkeypatch):
    ragged, ops, rec = route
    lay = ragged.Layout([(3, 32, True), (1, 40, True), (2, 96, True)])
    for on, as_pair in ((False, True), (True, False), (False, False)):
        monkeypatch.setattr(ragged, "ATTN_SEGS", on)
        rec.calls.clear()
        (q, k, v), mask = _operands(ops, lay, as_pair)
        ragged.attention(q, k, v, mask, mask, 4, lay, lay, pair=False)
        assert len(rec.calls) == 3 and all(c["segs"] is None for c in rec.calls), (on, as_pair)
        assert [tuple(c["q"].shape[:2]) for c in rec.calls] == [(3, 32), (1, 40), (2, 96)]


def test_switched_on_banded_attention_and_single_groups_keep_their_routes(route, monkeypatch):
    ragged, ops, rec = route
    monkeypatch.setattr(ragged, "ATTN_SEGS", True)
    one = ragged.Layout([(3, 32, True)])
    (q, k, v), mask = _operands(ops, one, True)
    ragged.attention(q, k, v, mask, mask, 4, one, one)
    assert len(rec.calls) == 1 and rec.calls[0]["segs"] is None


def test_forty_groups_are_two_segs_calls(route, monkeypatch):
    ragged, ops, rec = route
    monkeypatch.setattr(ragged, "ATTN_SEGS", True)
    lay = ragged.Layout([(1 + i % 2, 32 + 8 * i, True) for i in range(40)])
    (q, k, v), mask = _operands(ops, lay, True)
    ragged.attention(q, k, v, mask, None, 4, lay, lay)
    assert [len(c["segs"][0]) for c in rec.calls] == [32, 8] and [len(c["segs"][1]) for c in rec.calls] == [32, 8]
    assert rec.calls[0]["segs"][0] + rec.calls[1]["segs"][0] == lay.segs
    assert rec.calls[0]["out"] is rec.calls[1]["out"]
