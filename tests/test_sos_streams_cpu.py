"""vrd_dwconv_ln_multi (one depthwise-conv + LayerNorm pass over a subject / object stream for all its readers) without a GPU:
the symbol is declared, exported and bound field for field, the ABI number did not move, and the host refuses bad arguments by
name before anything is launched."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "vrdone_hip.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_declared_exported_and_bound():
    from vrdone_amd import _hip
    assert re.search(r"\bint\s+vrd_dwconv_ln_multi\s*\(\s*const\s+vrd_dwconv_ln_multi_args\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", _header())
    assert hasattr(C.CDLL(_hip.LIB_PATH), "vrd_dwconv_ln_multi")
    res, args = _hip._SIGNATURES["vrd_dwconv_ln_multi"]
    assert res is C.c_int and args == [C.POINTER(_hip.DwconvLnMultiArgs), C.c_void_p]


def test_abi_number_stays():
    from vrdone_amd import _hip
    assert _hip.ABI_VERSION == 37 and _hip.lib.vrd_abi_version() == 37
    assert re.search(r"#define\s+VRD_ABI_VERSION\s+37\b", open(HEADER).read())


def test_struct_is_bound_field_for_field():
    """names, order, array lengths and C types of vrd_dwconv_ln_multi_args against the ctypes mirror"""
    from vrdone_amd import _hip
    text = _header()
    sets = int(re.search(r"#define\s+VRD_DWCONV_MULTI_SETS\s+(\d+)", text).group(1))
    assert sets == 5 == _hip.DWCONV_MULTI_SETS
    body = re.search(r"typedef struct \{([^}]*)\} vrd_dwconv_ln_multi_args", text).group(1)
    want = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *rest = decl.split(",")
        ctype = first.rsplit(" ", 1)[0]
        names = [first.rsplit(" ", 1)[1]] + [r.strip() for r in rest]
        for n in names:
            ptr = "*" in ctype or n.startswith("*")
            m = re.fullmatch(r"\*?(\w+)(?:\[(\w+)\])?", n)
            length = {None: None, "VRD_DWCONV_MULTI_SETS": sets}[m.group(2)]
            base = "ptr" if ptr else {"int64_t": "i64", "int32_t": "i32"}[ctype.replace("const ", "").strip()]
            want.append((m.group(1), base, length))

    def kind(t):
        if hasattr(t, "_length_"):
            return kind(t._type_)[0], t._length_
        if t is C.c_int64:
            return "i64", None
        if t is C.c_int32:
            return "i32", None
        assert t is C.c_void_p or issubclass(t, C._Pointer), t
        return "ptr", None
    got = [(name,) + kind(t) for name, t in _hip.DwconvLnMultiArgs._fields_]
    assert got == want
    # the array members take what the header's layout gives them: 8-byte members on 8-byte offsets, no surprise in the size
    assert _hip.DwconvLnMultiArgs.y.offset % 8 == 0 and _hip.DwconvLnMultiArgs.ldy.offset % 8 == 0
    assert _hip.DwconvLnMultiArgs.segs.offset + 8 == C.sizeof(_hip.DwconvLnMultiArgs)


def _good():
    """arguments the host accepts (fake, aligned device addresses: a refusal comes before any launch)"""
    from vrdone_amd import _hip
    a = _hip.DwconvLnMultiArgs()
    a.x, a.ldx, a.B, a.Tin, a.C, a.n_out = 0x10000, 512, 1, 16, 512, 2
    for o in range(2):
        a.packed[o], a.y[o], a.ldy[o] = 0x20000 + 0x4000 * o, 0x40000 + 0x4000 * o, 512
    a.pre_ln[1] = 1
    a.pre_gamma, a.pre_beta = 0x60000, 0x61000
    return a


def _refused(a, *words):
    from vrdone_amd import _hip
    rc = _hip.lib.vrd_dwconv_ln_multi(C.byref(a), None)
    err = _hip.lib.vrd_last_error().decode()
    assert rc == -1, "a bad argument is refused on the host, before a launch"
    assert err.startswith("vrd_dwconv_ln_multi:"), err
    for w in words:
        assert w in err, err


@pytest.mark.parametrize("n_out", [0, 6, -1])
def test_refuses_zero_and_more_than_five_sets(n_out):
    a = _good()
    a.n_out = n_out
    _refused(a, "n_out must be 1..5")


@pytest.mark.parametrize("C_", [256, 0, 1024])
def test_refuses_other_widths(C_):
    a = _good()
    a.C = C_
    _refused(a, "C must be 512", str(C_))


@pytest.mark.parametrize("field", ["x", "packed", "y", "pre_gamma", "pre_beta"])
def test_refuses_misaligned_pointers(field):
    a = _good()
    if field in ("packed", "y"):
        getattr(a, field)[1] += 4
        _refused(a, "bad output set 1")
    else:
        setattr(a, field, getattr(a, field) + 4)
        _refused(a, "bad x layout" if field == "x" else "input LayerNorm")


def test_refuses_rows_that_lose_alignment_and_missing_operands():
    a = _good()
    a.ldy[0] = 514
    _refused(a, "bad output set 0")
    a = _good()
    a.ldx = 508
    _refused(a, "bad x layout")
    a = _good()
    a.pre_gamma = None
    _refused(a, "input LayerNorm")
    a = _good()
    a.packed[0] = None
    _refused(a, "bad output set 0")
    a = _good()
    a.out_pair[1] = 3
    _refused(a, "pair format of set 1")
    assert _good().x == 0x10000           # (and the accepted form is not launched here: no GPU)
