"""Global attention over a ragged row space in one call (vrd_attention_pair_segs, ops.attention(segs=...), the opt-in route of
ragged.attention) on a real MI355X.  The call is vrd_attention_pair applied to every row group, so the central check needs no
tolerance: the whole output equals, bit for bit, what the per-group calls write into a buffer of the same shape.

The table (sequences, Tq = Tk) = (3, 32), (1, 40), (2, 96), (1, 160), (2, 288), (1, 64), in that row order: a length that is no
multiple of 32, both sides of the 64-queries-per-wave threshold (160 query rows at head_dim 128) in one call, a second 256-query
block, a short group behind a long one.  A second table has Tq != Tk in every group.  VRD_FLASH_GRID=3 makes a persistent
workgroup walk items across group boundaries (both walks, VRD_FLASH_WALK 0 / 1); VRD_FLASH_W64 0 / 1 forces either kernel family
on every group it exists for."""
import ctypes
import functools

import pytest
import torch

import far_cases as Fc
import window_cases as W
from test_gpu_f16_range import check_producer, launches
from test_gpu_windows import _to_pair as to_pair_fmt
from test_gpu_windows import close, ok, p, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT = ("f16x3", "bf16x3")
TOL = 2e-4          # tests/test_gpu_ops.py::test_flash_attention_pair_rows: the same kernels, the same formats, inputs of the same scale
NAME = "vrd_attention_pair_segs"
HEADS = {32: 8, 64: 4, 128: 2}          # width 256
CW = 256

TABLE = [(3, 32, 32), (1, 40, 40), (2, 96, 96), (1, 160, 160), (2, 288, 288), (1, 64, 64)]           # (sequences, Tq, Tk)
# valid keys / queries per sequence, in row order: (length) or (length, (hole from, hole to)).  Keys: sequence 4 (96 frames, 64 valid)
# and 8 (288, 256 valid) end in a fully masked key tile, sequence 7 has a hole over two whole tiles and parts of two more.
# Queries: the last 32-query tile of sequences 4, 6 and 8 is fully masked (8: its whole second 256-query block).
KV_VALID = [32, 7, 1, 33, 64, 96, 130, (288, (100, 200)), 256, 50]
Q_VALID = [32, 7, 1, 33, 40, 96, 100, 288, 256, 64]
TABLE_X = [(2, 64, 32), (1, 32, 288)]                                                                # Tq != Tk
KV_VALID_X = [32, 9, (288, (40, 140))]
Q_VALID_X = [64, 20, 32]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def segs_of(table):
    qs, ks, rq, rk = [], [], 0, 0
    for n, Tq, Tk in table:
        qs.append((rq, n, Tq))
        ks.append((rk, n, Tk))
        rq, rk = rq + n * Tq, rk + n * Tk
    return qs, ks, rq, rk


def row_mask(segs, valid):
    """one bool per row of the row space"""
    out, it = [], iter(valid)
    for _, n, T in segs:
        for _ in range(n):
            spec = next(it)
            length, hole = spec if isinstance(spec, tuple) else (spec, None)
            m = torch.arange(T) < length
            if hole:
                m[hole[0]:hole[1]] = False
            out.append(m)
    return torch.cat(out)


@functools.lru_cache(maxsize=None)
def inputs(which, hd):
    """f32 q (Rq, C), k, v (Rk, C) and the row masks of a table, on the host, made once per (table, head_dim)"""
    table, kv_valid, q_valid = (TABLE, KV_VALID, Q_VALID) if which == "main" else (TABLE_X, KV_VALID_X, Q_VALID_X)
    qs, ks, rq, rk = segs_of(table)
    g = torch.Generator().manual_seed(1000 + hd + len(table))
    q = torch.randn(rq, CW, generator=g) * 2.0
    k, v = torch.randn(rk, CW, generator=g), torch.randn(rk, CW, generator=g)
    for (r0, n, Tk), (q0, _, Tq) in zip(ks, qs):           # a dominant late (valid) key in every group's first head: the running-max rescale
        k[r0 + min(70, Tk - 1) // 32 * 32, :hd] = q[q0 + min(5, Tq - 1), :hd] * 2.0
    return dict(q=q, k=k, v=v, km=row_mask(ks, kv_valid), qm=row_mask(qs, q_valid), qsegs=qs, ksegs=ks, rq=rq, rk=rk)


def want_f64(c, H, masked):
    """float64 masked softmax, sequence by sequence -> (Rq, C) on the host"""
    out = torch.zeros(c["rq"], CW, dtype=torch.float64)
    hd = CW // H
    for (q0, n, Tq), (k0, _, Tk) in zip(c["qsegs"], c["ksegs"]):
        for b in range(n):
            qa, ka = q0 + b * Tq, k0 + b * Tk
            q = c["q"][qa:qa + Tq].double().reshape(Tq, H, hd).transpose(0, 1)
            k = c["k"][ka:ka + Tk].double().reshape(Tk, H, hd).transpose(0, 1)
            v = c["v"][ka:ka + Tk].double().reshape(Tk, H, hd).transpose(0, 1)
            s = q @ k.transpose(1, 2) / hd ** 0.5
            if masked:
                s = s.masked_fill(~c["km"][ka:ka + Tk][None, None, :], float("-inf"))
            out[qa:qa + Tq] = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(Tq, CW)
    return out


def tile_live(c):
    """per query row: its 32-query tile (counted inside its sequence) holds a valid query"""
    out = []
    for q0, n, Tq in c["qsegs"]:
        for b in range(n):
            m = c["qm"][q0 + b * Tq:q0 + (b + 1) * Tq]
            out.append(torch.nn.functional.pad(m, (0, (-Tq) % 32)).reshape(-1, 32).any(-1).repeat_interleave(32)[:Tq])
    return torch.cat(out)


class Case:
    """the operands of one table in windows with poisoned guard bands (tests/window_cases.py) and leading dimensions that are
    distinct and wider than the width: q alone, k and v as column slabs of one buffer, two outputs of one shape"""

    def __init__(self, which, hd, fmt):
        self.c = c = inputs(which, hd)
        self.H, self.hd, self.fmt = HEADS[hd], hd, fmt
        lds = W.LdSeq()
        enc = lambda t: to_pair_fmt(t.to(DEV), fmt)          # noqa: E731
        self.hq = W.embed(enc(c["q"]), ld=lds(CW), name="q")
        self.hkv = W.embed(torch.cat([enc(c["k"]), enc(c["v"])], dim=-1), ld=lds(2 * CW), name="kv")
        self.k, self.v = self.hkv.view[:, :CW], self.hkv.view[:, CW:]
        ld_out = lds(CW)
        self.out = lambda name: W.embed_out((c["rq"], CW), DEV, ld=ld_out, name=name)          # noqa: E731
        assert len({self.hq.ld, self.hkv.ld, ld_out}) == 3 and min(self.hq.ld, self.hkv.ld, ld_out) > CW
        self.km, self.qm = c["km"].to(DEV), c["qm"].to(DEV)

    def segs(self, ho, kv_mask=True, q_mask=True, out_pair=False, products=0, qsegs=None, ksegs=None):
        from vrdone_amd import _hip
        tq, tk = _hip.RowSegs.of(qsegs or self.c["qsegs"]), _hip.RowSegs.of(ksegs or self.c["ksegs"])
        ok(_hip.lib.vrd_attention_pair_segs(p(self.hq.view), self.hq.ld, p(self.k), p(self.v), self.hkv.ld, p(self.km) if kv_mask else None,
                                            p(self.qm) if q_mask else None, ctypes.byref(tq), ctypes.byref(tk), self.H, self.hd, p(ho.view),
                                            ho.ld, self.fmt if out_pair else 0, self.fmt, stream(), products), NAME)

    def buckets(self, ho, kv_mask=True, q_mask=True, out_pair=False, products=0):
        """vrd_attention_pair on every group's rows of the same buffers"""
        from vrdone_amd import _hip
        for (q0, n, Tq), (k0, _, Tk) in zip(self.c["qsegs"], self.c["ksegs"]):
            ok(_hip.lib.vrd_attention_pair(p(self.hq.view[q0:]), self.hq.ld, p(self.k[k0:]), p(self.v[k0:]), self.hkv.ld,
                                           p(self.km[k0:]) if kv_mask else None, p(self.qm[q0:]) if q_mask else None, n, Tq, Tk, self.H, self.hd,
                                           p(ho.view[q0:]), ho.ld, self.fmt if out_pair else 0, self.fmt, stream(), products), "vrd_attention_pair")


def set_env(monkeypatch, w64, walk, grid="3"):
    for name, val in (("VRD_FLASH_W64", w64), ("VRD_FLASH_WALK", walk), ("VRD_FLASH_GRID", grid)):          # all read per call
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def fmt_of(mode):
    from vrdone_amd import _hip
    return {"f16x3": _hip.PAIR_F16, "bf16x3": _hip.PAIR_BF16}[mode]


# ------------------------------------------------------------------------------- a. bit equality with the per-bucket launches
def equal_to_buckets(case, monkeypatch, w64, products=0):
    for walk in ("0", "1"):
        set_env(monkeypatch, w64, walk)
        for masks in (True, False):
            for out_pair in (False, True):
                got, ref = case.out("out"), case.out("per bucket")
                case.segs(got, masks, masks, out_pair, products)
                case.buckets(ref, masks, masks, out_pair, products)
                torch.cuda.synchronize()
                what = f"walk {walk}, masks {masks}, out_pair {out_pair}"
                assert torch.equal(got.view.view(torch.int32), ref.view.view(torch.int32)), what
                assert torch.equal(got.buf.view(torch.int32), ref.buf.view(torch.int32)), what + " (the guard bands too)"
                if not out_pair:
                    assert bool(torch.isfinite(got.view).all()), what


@pytest.mark.parametrize("w64", [None, "0", "1"])
@pytest.mark.parametrize("mode", SPLIT)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_bit_equal_to_per_bucket_launches(hd, mode, w64, monkeypatch):
    equal_to_buckets(Case("main", hd, fmt_of(mode)), monkeypatch, w64)


@pytest.mark.parametrize("w64", [None, "0", "1"])
@pytest.mark.parametrize("hd", [64, 128])
def test_bit_equal_one_product_form(hd, w64, monkeypatch):
    equal_to_buckets(Case("main", hd, fmt_of("f16x3")), monkeypatch, w64, products=1)


@pytest.mark.parametrize("w64", [None, "1"])
@pytest.mark.parametrize("mode", SPLIT)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_bit_equal_with_different_query_and_key_lengths(hd, mode, w64, monkeypatch):
    equal_to_buckets(Case("cross", hd, fmt_of(mode)), monkeypatch, w64)


def test_default_grid_and_ops_entry(monkeypatch):
    """without the grid cap (one workgroup per item), through ops.attention(segs=...) on contiguous rows: the per-group ops.attention"""
    from vrdone_amd import ops
    set_env(monkeypatch, None, None, None)
    for mode in SPLIT:
        with ops.use_precision(mode):
            fmt = ops.pair_fmt()
            c = inputs("main", 128)
            q, k, v = (ops.Pair(to_pair_fmt(c[n].to(DEV), fmt)[None], CW, fmt) for n in "qkv")
            km, qm = c["km"].to(DEV)[None], c["qm"].to(DEV)[None]
            got = ops.attention(q, k, v, km, 2, q_mask=qm, segs=(c["qsegs"], c["ksegs"]))
            got_pair = ops.attention(q, k, v, km, 2, q_mask=qm, pair=True, segs=(c["qsegs"], c["ksegs"]))
            assert got.shape == (1, c["rq"], CW) and isinstance(got_pair, ops.Pair) and got_pair.fmt == fmt
            assert launches(lambda: ops.attention(q, k, v, km, 2, q_mask=qm, segs=(c["qsegs"], c["ksegs"])), "attn_flash") == [2]
            for (q0, n, Tq), (k0, _, Tk) in zip(c["qsegs"], c["ksegs"]):
                part = lambda x, r0, T: (ops.Pair(x.t[0, r0:r0 + n * T].unflatten(0, (n, T)), CW, fmt) if isinstance(x, ops.Pair)      # noqa: E731
                                         else x[0, r0:r0 + n * T].unflatten(0, (n, T)))
                args = (part(q, q0, Tq), part(k, k0, Tk), part(v, k0, Tk), part(km, k0, Tk), 2)
                assert torch.equal(got[0, q0:q0 + n * Tq].unflatten(0, (n, Tq)), ops.attention(*args, q_mask=part(qm, q0, Tq)))
                assert W.bits_equal(got_pair.t[0, q0:q0 + n * Tq].unflatten(0, (n, Tq)), ops.attention(*args, q_mask=part(qm, q0, Tq), pair=True).t)
    with pytest.raises(TypeError, match="pair-row"):
        x = torch.zeros(1, 64, CW, device=DEV)
        ops.attention(x, x, x, None, 2, segs=([(0, 2, 32)], [(0, 2, 32)]))


# -------------------------------------------------------------------------------------------------------- b. against float64
@pytest.mark.parametrize("mode", SPLIT)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_against_float64(hd, mode, monkeypatch):
    """f32 inputs split by the library's own copy-type producer (vrd_bct_to_btc with pair rows out), the table of (a), against a
    float64 masked softmax per sequence at the bound of test_flash_attention_pair_rows (TOL)"""
    from vrdone_amd import ops
    set_env(monkeypatch, None, None, None)
    c, H = inputs("main", hd), HEADS[hd]
    with ops.use_precision(mode):
        split = lambda t: ops.bct_to_btc(t.t().contiguous()[None].to(DEV), 0, CW, torch.empty(1, t.shape[0], CW, device=DEV), pair=True)      # noqa: E731
        q, k, v = split(c["q"]), split(c["k"]), split(c["v"])
        assert all(isinstance(x, ops.Pair) for x in (q, k, v))
        km, qm = c["km"].to(DEV)[None], c["qm"].to(DEV)[None]
        segs = (c["qsegs"], c["ksegs"])
        got = ops.attention(q, k, v, km, H, segs=segs)
        err = float((got[0].double().cpu() - want_f64(c, H, True)).abs().max())
        print(f"[head_dim {hd} / {mode}] max error {err:.2e} (bound {TOL:.0e})")
        close(got[0], want_f64(c, H, True), TOL, "kv_mask")
        close(ops.attention(q, k, v, km, H, pair=True, segs=segs).float()[0], want_f64(c, H, True), TOL, "pair rows out")
        close(ops.attention(q, k, v, None, H, segs=segs)[0], want_f64(c, H, False), TOL, "no masks")
        masked = ops.attention(q, k, v, km, H, q_mask=qm, segs=segs)[0]
        live = tile_live(c).to(DEV)
        close(masked[live], want_f64(c, H, True)[live.cpu()], TOL, "live query tiles")
        assert bool((masked[~live] == 0).all())


# ------------------------------------------------------------------------------------------------- c. guard bands, d. repeats
@pytest.mark.parametrize("w64", ["0", "1"])
@pytest.mark.parametrize("mode", SPLIT)
def test_guard_bands_dead_tiles_and_repeats(mode, w64, monkeypatch):
    set_env(monkeypatch, w64, None)
    case = Case("main", 64, fmt_of(mode))
    live = tile_live(case.c).to(DEV)
    assert not bool(live.all())
    for out_pair in (False, True):
        first, again = case.out("out"), case.out("again")
        case.segs(first, out_pair=out_pair)
        case.segs(again, out_pair=out_pair)
        torch.cuda.synchronize()
        for h in (first, again):
            W.assert_guards_intact(h)              # rows in front of and behind the window, columns beyond the width
        W.assert_unchanged(case.hq)
        W.assert_unchanged(case.hkv)
        assert torch.equal(first.buf.view(torch.int32), again.buf.view(torch.int32)), "two calls on the same inputs differ"
        assert bool((first.view[~live].view(torch.int32) == 0).all()), "fully masked query tiles read 0"
        if not out_pair:
            W.assert_written_and_finite(first)
            close(first.view[live], want_f64(case.c, case.H, True)[live.cpu()], TOL, "live query tiles")


def test_rows_no_group_names_are_left_alone(monkeypatch):
    """a table that names only groups 1, 3 and 4 of the main one: the other rows of the output keep the sentinel"""
    set_env(monkeypatch, None, None)
    case = Case("main", 128, fmt_of("bf16x3"))
    pick = [1, 3, 4]
    qsegs, ksegs = [case.c["qsegs"][i] for i in pick], [case.c["ksegs"][i] for i in pick]
    got, ref = case.out("out"), case.out("per bucket")
    case.segs(got, qsegs=qsegs, ksegs=ksegs)
    case.buckets(ref)
    torch.cuda.synchronize()
    named = torch.zeros(case.c["rq"], dtype=torch.bool, device=DEV)
    for q0, n, Tq in qsegs:
        named[q0:q0 + n * Tq] = True
    assert torch.equal(got.view[named], ref.view[named])
    assert bool((got.view[~named].view(torch.int32) == W.SENTINEL_BITS).all())
    W.assert_guards_intact(got)


# ------------------------------------------------------------------------------------------------------ e. f16 range flag
def test_f16_range_flag_matches_the_per_bucket_entry():
    """vrd_attention_pair writes f16 pair rows without reporting (tests/test_gpu_f16_range.py::test_attention_on_pair_rows_stays_silent:
    its outputs are averages of value rows that were checked when they were written), i.e. under tag 0; so does the row-group entry,
    probed at a group boundary: the value comes out in the last row of the last group."""
    from vrdone_amd import ops
    c = inputs("main", 64)
    segs = (c["qsegs"], c["ksegs"])
    last = c["rq"] - 1

    def run(value):
        fmt = ops.pair_fmt()
        v = c["v"].clone()
        k0, n, Tk = c["ksegs"][-1]
        v[k0 + (n - 1) * Tk:, CW - 1] = value                 # every key of the last sequence: the softmax average is the value
        q, k, vp = (ops.Pair(to_pair_fmt(t.to(DEV), fmt)[None], CW, fmt) for t in (c["q"], c["k"], v))
        out = ops.attention(q, k, vp, c["km"].to(DEV)[None], 4, pair=True, segs=segs)
        assert isinstance(out, ops.Pair) and out.fmt == fmt
        want = torch.full((1, 1), float(value), dtype=torch.float64, device=DEV)
        return out.float()[0, last:, CW - 1:].contiguous(), want          # the last channel of the last row, decoded

    check_producer(run, 0, rel=1e-4, modes=("bf16x3",))


# ------------------------------------------------------------------------------------------------------------ f. far rows
@pytest.mark.parametrize("w64", ["0", "1"])
def test_far_rows(w64, monkeypatch):
    """One case per kernel family (head_dim 64, where both exist): short groups in front, one that starts beyond 2^31 bytes and one,
    the last, beyond 2^32 bytes of every buffer, gaps of unnamed rows between them filled with the sentinel.  The first and the last
    group equal per-bucket launches on copies of their rows; unnamed output rows keep the sentinel."""
    from vrdone_amd import ops
    set_env(monkeypatch, w64, None)
    hd, H = 64, 4
    row_bytes = CW * 4
    groups = [(0, 2, 32), (64, 1, 96), (160, 2, 64), ((1 << 31) // row_bytes + 8, 1, 64), ((1 << 32) // row_bytes + 8, 2, 40)]
    R = groups[-1][0] + groups[-1][1] * groups[-1][2] + Fc.GUARD_ROWS
    assert groups[3][0] * row_bytes > 1 << 31 and groups[4][0] * row_bytes > 1 << 32 and 4 * R * row_bytes <= Fc.MEMORY_CAP
    gen = torch.Generator().manual_seed(77)
    with ops.use_precision("bf16x3"):
        fmt = ops.pair_fmt()
        bufs = [torch.full((1, R, CW), W.SENTINEL_BITS, dtype=torch.int32, device=DEV) for _ in range(4)]
        q, k, v, out = (b.view(torch.float32) for b in bufs)
        mask = torch.zeros(1, R, dtype=torch.bool, device=DEV)
        for r0, n, T in groups:
            for t, scale in ((q, 2.0), (k, 1.0), (v, 1.0)):
                t[0, r0:r0 + n * T] = to_pair_fmt((torch.randn(n * T, CW, generator=gen) * scale).to(DEV), fmt)
            mask[0, r0:r0 + n * T] = (torch.arange(n * T) % T < max(1, T - 9 * (r0 % 3))).to(DEV)
        pr = lambda t: ops.Pair(t, CW, fmt)          # noqa: E731
        ops.attention(pr(q), pr(k), pr(v), mask, H, q_mask=mask, out=out, segs=(groups, groups))
        torch.cuda.synchronize()
        at = 0
        for r0, n, T in groups:
            assert bool((bufs[3][0, at:r0] == W.SENTINEL_BITS).all()), f"unnamed output rows {at} .. {r0} were written"
            at = r0 + n * T
            assert bool(torch.isfinite(out[0, r0:at]).all())
        assert bool((bufs[3][0, at:] == W.SENTINEL_BITS).all())
        for r0, n, T in (groups[0], groups[3], groups[-1]):
            part = lambda t: t[0, r0:r0 + n * T].clone().unflatten(0, (n, T))          # noqa: E731
            plain = ops.attention(pr(part(q)), pr(part(k)), pr(part(v)), part(mask), H, q_mask=part(mask))
            assert torch.equal(out[0, r0:r0 + n * T].unflatten(0, (n, T)), plain), f"group at row {r0}"
    del bufs, q, k, v, out


# ---------------------------------------------------------------------------------------------------------- g. model level
LENS = [5, 17, 24, 24, 25, 40, 56, 33, 57, 94, 95, 96]          # tests/test_gpu_model.py launch_cases(): rows_global


def same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def model_runs(name):
    """(run _mask_vrd on a ragged batch, run forward_test on a multi-bucket video), both in the row space"""
    from oracle import vrd_oracle as O
    from test_gpu_model import c_in, get_model
    from vrdone_amd import synth
    model, mc, _, _ = get_model(name)
    x, m = O.synth_pairs(len(LENS), c_in(mc), 96, LENS, seed=41)
    xd, md = x.to(DEV), m.to(DEV)
    video = synth.synth_video(8, c_in(mc), 10, 60, seed=3, device=DEV)

    def mask_vrd():
        try:
            model.ROWS_MIN_ROWS = 64
            plan = model._tight_plan(md, md.reshape(len(LENS), 96))
            assert plan and plan["rows"] and len(plan["buckets"]) > 1, plan
            return model._mask_vrd(xd, md)
        finally:
            model.__dict__.pop("ROWS_MIN_ROWS", None)

    def forward_test():
        old_chunk = model.pair_chunk
        try:
            model.ROWS_MIN_PAIRS, model.ROWS_MIN_ROWS, model.pair_chunk = 8, 64, 20
            assert model._eval_rows_form(len(video["sids"]))
            return model(video)
        finally:
            model.__dict__.pop("ROWS_MIN_PAIRS", None)
            model.__dict__.pop("ROWS_MIN_ROWS", None)
            model.pair_chunk = old_chunk
    return mask_vrd, forward_test


@pytest.mark.parametrize("mode", SPLIT)
@pytest.mark.parametrize("name", ["vidvrd", "vidor"])
def test_model_outputs_do_not_depend_on_the_switch(name, mode, monkeypatch):
    """_mask_vrd on a ragged batch (vidvrd: head_dim 128, vidor: 64) and forward_test on a multi-bucket video (vidvrd: the synthetic
    video is in that dataset's format)"""
    from vrdone_amd import ops
    from vrdone_amd.models import ragged
    set_env(monkeypatch, None, None, None)
    with ops.use_precision(mode):
        for run in model_runs(name)[:2 if name == "vidvrd" else 1]:
            monkeypatch.setattr(ragged, "ATTN_SEGS", False)
            off = run()
            n_off = launches(run, "attn_flash")[0]
            monkeypatch.setattr(ragged, "ATTN_SEGS", True)
            on = run()
            n_on = launches(run, "attn_flash")[0]
            assert same(on, off), run.__name__
            print(f"[{name} / {mode}] {run.__name__}: attn_flash launches {n_off} -> {n_on}")
            assert 0 < n_on < n_off, run.__name__


def test_model_launch_counts_with_the_switch(monkeypatch):
    """vidvrd's _mask_vrd on the rows_global batch of tests/test_gpu_model.py (four buckets): 52 attn_flash launches with the bucket
    walk (LAUNCHES["rows_global"]).  8 of the network's global-attention calls have pair-row operands (the SOS self / cross
    attention: 8 x 4 launches); the predictor's attention projects to f32 rows and stays on the f32 flash kernel bucket by bucket,
    whatever the switch says (20 launches).  With the switch each of the 8 is one call of at most two launches, and here -- head_dim
    128, no bucket of 160 frames: one kernel family -- exactly one: 8 + 20 = 28.  In the exact f32 mode no operand is a pair row
    and the switch changes nothing."""
    from vrdone_amd import ops
    from vrdone_amd.models import ragged
    set_env(monkeypatch, None, None, None)
    run, _ = model_runs("vidvrd")
    counts, calls = {}, []
    real = ops.attention
    monkeypatch.setattr(ops, "attention", lambda *a, **kw: (calls.append(kw.get("segs") is not None), real(*a, **kw))[1])
    for mode in ("f16x3", "f32"):
        with ops.use_precision(mode):
            for on in (False, True):
                monkeypatch.setattr(ragged, "ATTN_SEGS", on)
                run()
                counts[mode, on] = launches(run)
    assert counts["f16x3", False]["attn_flash"] == 52 and counts["f16x3", True]["attn_flash"] == 28
    assert sum(calls) == 2 * 8, "row-group calls of the two f16x3 runs with the switch on"
    assert counts["f16x3", True]["attn_flash"] <= 2 * 8 + 20
    assert {k: v for k, v in counts["f16x3", True].items() if k != "attn_flash"} == \
        {k: v for k, v in counts["f16x3", False].items() if k != "attn_flash"}
    assert counts["f32", True] == counts["f32", False]
