"""What the attention entry points answer to bad arguments (no GPU needed: they check their arguments before anything touches a
device).  tests/golden/attn_arg_errors.json (scripts/record_attn_arg_errors.py) holds argument sets that each break one check of
vrd_local_attn, _segs, _drop, _bwd, _drop_bwd, vrd_attention_pair or _pair_segs, with the return code and the text of
vrd_last_error() that the library gave when the file was recorded: the shape rule and the checks of csrc/vrd_local_attn.h,
vrd_local_attn.hip, vrd_local_attn_bwd.hip and vrd_attn_x3.hip answer every one of them the same way."""
import ctypes
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"vrd_local_attn", "vrd_local_attn_segs", "vrd_local_attn_drop", "vrd_local_attn_bwd", "vrd_local_attn_drop_bwd",
                "vrd_attention_pair", "vrd_attention_pair_segs"}


def _calls():
    with open(os.path.join(REPO, "tests", "golden", "attn_arg_errors.json")) as f:
        return json.load(f)["calls"]


def _decode(arg, keep):
    """a stored argument -> what ctypes takes ({"segs": [[first row, sequences, frames]], "count": ...} is a vrd_row_segs)"""
    from vrdone_amd import _hip
    if not isinstance(arg, dict):
        return arg
    t = _hip.RowSegs()
    t.count = arg.get("count", len(arg["segs"]))
    for i, (row, n, T) in enumerate(arg["segs"]):
        t.row[i], t.n[i], t.T[i] = row, n, T
    keep.append(t)
    return ctypes.byref(t)


def test_the_file_names_every_entry_point_and_no_call_that_would_launch():
    calls = _calls()
    assert {c["fn"] for c in calls} == ENTRY_POINTS
    # a set that returned 0 would go on to a launch, with dummy addresses
    assert all(c["rc"] == -1 and c["error"] for c in calls)


def test_every_recorded_argument_set_is_refused_with_the_recorded_text():
    from vrdone_amd import _hip
    wrong = []
    for c in _calls():
        keep = []
        rc = getattr(_hip.lib, c["fn"])(*[_decode(a, keep) for a in c["args"]])
        err = _hip.lib.vrd_last_error().decode()
        assert rc != 0, (c["fn"], c["breaks"])
        if (rc, err) != (c["rc"], c["error"]):
            wrong.append((c["fn"], c["breaks"], rc, err, c["error"]))
    assert not wrong, wrong[:5]
