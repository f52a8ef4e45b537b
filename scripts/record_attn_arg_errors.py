"""Record what the attention entry points answer to bad arguments into tests/golden/attn_arg_errors.json.

The seven entry points of the banded attention (vrd_local_attn, _segs, _drop, _bwd, _drop_bwd) and of the pair-row flash attention
(vrd_attention_pair, _pair_segs) check their arguments before anything touches a device, so dummy addresses do (no GPU needed):
256 is an aligned pointer, 260 a misaligned one; row-group tables are real RowSegs.  Every argument set below breaks exactly one
check of its entry point, and every check is broken by at least one set; each set is stored with the return code and
vrd_last_error().  Run it with the library whose answers are the reference (VRDONE_HIP_LIB), VRD_FLASH_* unset:
    python scripts/record_attn_arg_errors.py
tests/test_attn_args_cpu.py replays the file."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
P, Q = 256, 260                 # an aligned and a misaligned dummy address


def segs(*groups, count=None):
    """a row-group table as it is stored: [(first row, sequences, frames)], `count` where it is not the number of groups"""
    d = {"segs": [list(g) for g in groups]}
    if count is not None:
        d["count"] = count
    return d


# name -> (argument names in ABI order, a valid set)
LOCAL = dict(q=P, k=P, v=P, ld=512, mask=P, rel_pe=None, B=2, T=20, C=512, n_head=8, half_win=3, out=P, ldo=512, out_pair=0, stream=None)
BWD = dict(q=P, k=P, v=P, ld=512, dO=P, lddo=512, mask=P, rel_pe=None, B=2, T=20, C=512, n_head=8, half_win=3)
BWD_OUT = dict(dq=P, dk=P, dv=P, ldd=512, scratch=P, stream=None)
DROP = dict(seed=P, site=3, row0=0, p=0.25)
PAIR = dict(q=P, ldq=512, k=P, v=P, ldkv=512, kv_mask=None, q_mask=None, B=2, Tq=40, Tk=40, n_head=8, head_dim=64, out=P, ldo=512,
            out_pair=0, pair_fmt=2, stream=None, products=0)
TABLE = segs((0, 2, 20), (40, 1, 36))
BASE = {
    "vrd_local_attn": LOCAL,
    "vrd_local_attn_segs": {**{k: v for k, v in LOCAL.items() if k not in ("B", "T")}, "segs": TABLE},
    "vrd_local_attn_drop": {**{k: v for k, v in LOCAL.items() if k not in ("out", "ldo", "out_pair", "stream")}, **DROP, "out": P, "ldo": 512,
                            "stream": None},
    "vrd_local_attn_bwd": {**BWD, **BWD_OUT},
    "vrd_local_attn_drop_bwd": {**BWD, **DROP, **BWD_OUT},
    "vrd_attention_pair": PAIR,
    "vrd_attention_pair_segs": {**{k: v for k, v in PAIR.items() if k not in ("B", "Tq", "Tk")}, "qsegs": TABLE, "ksegs": TABLE},
}
ORDER = {
    "vrd_local_attn_segs": "q k v ld mask rel_pe segs C n_head half_win out ldo out_pair stream".split(),
    "vrd_attention_pair_segs": "q ldq k v ldkv kv_mask q_mask qsegs ksegs n_head head_dim out ldo out_pair pair_fmt stream products".split(),
}

ENVELOPE = [dict(C=384, n_head=6), dict(C=512, n_head=3), dict(C=512, n_head=2), dict(C=256, n_head=16), dict(n_head=0), dict(C=1024, n_head=8)]
WINDOW = [dict(half_win=0), dict(half_win=10), dict(half_win=-1)]


def local_cases(fn, ptrs, lds, aligned):
    """the checks the five banded entry points have in common: null pointers, the envelope, the window, the layout"""
    for name in ptrs:
        yield fn, f"null {name}", {name: None}
    for e in ENVELOPE:
        yield fn, "envelope", e
    for w in WINDOW:
        yield fn, "window", w
    for name in lds:
        yield fn, f"{name} < C", {name: 508}
        yield fn, f"{name} % 4", {name: 514}
    for name in aligned:
        yield fn, f"misaligned {name}", {name: Q}
    yield fn, "layout at C = 256", dict(C=256, n_head=4, **{lds[0]: 252})


def cases():
    fn = "vrd_local_attn"
    yield fn, "B", dict(B=0)
    yield fn, "T", dict(T=0)
    yield from local_cases(fn, "q k v mask out".split(), ("ld", "ldo"), "q k v out".split())
    fn = "vrd_local_attn_segs"
    yield fn, "null table", dict(segs=None)
    yield from local_cases(fn, "q k v mask out".split(), ("ld", "ldo"), "q k v out".split())
    yield fn, "no group", dict(segs=segs((0, 2, 20), count=0))
    yield fn, "too many groups", dict(segs=segs((0, 2, 20), count=33))
    yield fn, "group without sequences", dict(segs=segs((0, 2, 20), (40, 0, 36)))
    yield fn, "group without frames", dict(segs=segs((0, 2, 0), (40, 1, 36)))
    yield fn, "group at a negative row", dict(segs=segs((0, 2, 20), (-4, 1, 36)))
    fn = "vrd_local_attn_drop"
    for bad in (dict(p=1.0), dict(p=-0.125), dict(row0=-1)):
        yield fn, "rate / row0", bad
    yield fn, "B", dict(B=0)
    yield fn, "T", dict(T=0)
    yield from local_cases(fn, "q k v mask out seed".split(), ("ld", "ldo"), "q k v out".split())
    # p = 0 is vrd_local_attn, with its texts
    yield fn, "p = 0: envelope", dict(p=0.0, C=384, n_head=6)
    yield fn, "p = 0: window", dict(p=0.0, half_win=10)
    yield fn, "p = 0: null q", dict(p=0.0, q=None)
    yield fn, "p = 0: layout", dict(p=0.0, ldo=508)
    fn = "vrd_local_attn_bwd"
    ptrs, al = "q k v dO mask dq dk dv scratch".split(), "q k v dO dq dk dv".split()
    yield from local_cases(fn, ptrs, ("ld", "lddo", "ldd"), al)
    fn = "vrd_local_attn_drop_bwd"
    for bad in (dict(p=1.0), dict(p=-0.125), dict(row0=-1)):
        yield fn, "rate / row0", bad
    yield fn, "null seed", dict(seed=None)
    yield from local_cases(fn, ptrs, ("ld", "lddo", "ldd"), al)
    yield fn, "p = 0 without a seed: envelope", dict(p=0.0, seed=None, C=384, n_head=6)
    yield fn, "p = 0 without a seed: window", dict(p=0.0, seed=None, half_win=10)

    def pair_cases(fn):
        for name in "q k v out".split():
            yield fn, f"null {name}", {name: None}
        for hd in (48, 16, 256, 0):
            yield fn, "head_dim", dict(head_dim=hd, n_head=8)
        yield fn, "n_head", dict(n_head=0)
        yield fn, "n_head", dict(n_head=65536, ldq=65536 * 64, ldkv=65536 * 64, ldo=65536 * 64)
        for name in ("ldq", "ldkv", "ldo"):
            yield fn, f"{name} < width", {name: 508}
            yield fn, f"{name} % 4", {name: 514}
        for name in "q k v out".split():
            yield fn, f"misaligned {name}", {name: Q}
        for fmt in (0, 3):
            yield fn, "pair_fmt", dict(pair_fmt=fmt, out_pair=0)
        yield fn, "out_pair", dict(out_pair=1, pair_fmt=2)
        yield fn, "out_pair", dict(out_pair=2, pair_fmt=1)
        yield fn, "products", dict(products=2)
        yield fn, "products", dict(products=1, pair_fmt=1)
        yield fn, "one product at head_dim 32", dict(products=1, head_dim=32, n_head=16)

    fn = "vrd_attention_pair"
    yield from pair_cases(fn)
    for bad in (dict(B=0), dict(B=65536), dict(Tq=0), dict(Tk=0)):
        yield fn, "sizes", bad
    # the key-bias row: refused by the launch function of the chosen kernel, before it reaches the device
    yield fn, "Tk > 4096", dict(Tk=5000)
    # (the kernel with 64 queries per wave has room for more tile flags behind its ring: it refuses from 6,080 keys on)
    yield fn, "Tk > 4096, 64 queries per wave", dict(Tk=8000, Tq=160, n_head=4, head_dim=128)
    yield fn, "Tk > 4096, head_dim 32", dict(Tk=5000, n_head=16, head_dim=32)
    fn = "vrd_attention_pair_segs"
    yield from pair_cases(fn)
    yield fn, "null qsegs", dict(qsegs=None)
    yield fn, "null ksegs", dict(ksegs=None)
    yield fn, "no group", dict(qsegs=segs((0, 2, 20), count=0), ksegs=segs((0, 2, 20), count=0))
    yield fn, "too many groups", dict(qsegs=segs((0, 2, 20), count=33), ksegs=segs((0, 2, 20), count=33))
    yield fn, "tables of different length", dict(ksegs=segs((0, 2, 20)))
    yield fn, "group: sequences differ", dict(ksegs=segs((0, 2, 20), (40, 2, 36)))
    yield fn, "group: no sequence", dict(qsegs=segs((0, 2, 20), (40, 0, 36)), ksegs=segs((0, 2, 20), (40, 0, 36)))
    yield fn, "group: too many sequences", dict(qsegs=segs((0, 65536, 1)), ksegs=segs((0, 65536, 1)))
    yield fn, "group: no query", dict(qsegs=segs((0, 2, 0), (40, 1, 36)))
    yield fn, "group: no key", dict(ksegs=segs((0, 2, 20), (40, 1, 0)))
    yield fn, "group: negative query row", dict(qsegs=segs((0, 2, 20), (-4, 1, 36)))
    yield fn, "group: negative key row", dict(ksegs=segs((-4, 2, 20), (40, 1, 36)))
    yield fn, "group: Tk > 4096", dict(ksegs=segs((0, 2, 20), (40, 1, 5000)))
    w = 65535 * 32
    yield fn, "too many workgroups", dict(n_head=65535, head_dim=32, ldq=w, ldkv=w, ldo=w, qsegs=segs((0, 65535, 1)), ksegs=segs((0, 65535, 1)))


def decode(arg, keep):
    """a stored argument -> what ctypes takes; `keep` holds the tables alive over the call"""
    if not isinstance(arg, dict):
        return arg
    import ctypes
    from vrdone_amd import _hip
    t = _hip.RowSegs()
    t.count = arg.get("count", len(arg["segs"]))
    for i, (row, n, T) in enumerate(arg["segs"]):
        t.row[i], t.n[i], t.T[i] = row, n, T
    keep.append(t)
    return ctypes.byref(t)


def main():
    assert not [k for k in os.environ if k.startswith("VRD_FLASH_")], "VRD_FLASH_* change which kernel a shape is sent to"
    from vrdone_amd import _hip
    rows = []
    for fn, breaks, change in cases():
        base = BASE[fn]
        assert set(change) <= set(base), (fn, change)
        named = {**base, **change}
        args = [named[name] for name in ORDER.get(fn, list(base))]
        keep = []
        rc = getattr(_hip.lib, fn)(*[decode(a, keep) for a in args])
        err = _hip.lib.vrd_last_error().decode()
        assert rc == -1, (fn, breaks, args, rc, err)       # anything else went past the checks, towards a device
        rows.append({"fn": fn, "breaks": breaks, "args": args, "rc": rc, "error": err})
    assert {r["fn"] for r in rows} == set(BASE)
    out = os.path.join(REPO, "tests", "golden", "attn_arg_errors.json")
    with open(out, "w") as f:
        f.write('{"calls": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n]}\n")
    print(f"{len(rows)} argument sets, {len({r['error'] for r in rows})} distinct texts -> {out}")


if __name__ == "__main__":
    main()
