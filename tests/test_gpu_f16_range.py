"""The f16 operand-range flag (include/vrdone_hip.h, "operand range of the VRD_PAIR_F16 format") kernel by kernel on a real MI355X.

Every kernel that writes f16 pair rows, or splits f32 rows into f16 planes while staging them, must OR its tag into the device's
flag word when a value x with |x * 2^4| >= 65520 passes through it.  The tests drive each producer so that one output (or staged
input) is an exact copy of a chosen number and check, per store path:

  1. the out-of-range value sets exactly the producer's tag;
  2. the in-range value leaves the word at 0 and (copy-type producers) decodes bit for bit;
  3. bf16x3 and f32 leave the word at 0 on the out-of-range value and give the float64 expression's result;
  4. in f16x3 a consumer GEMM with all-ones weights is non-finite in exactly the rows that hold the value (once per producer).

Values: 4095 (4095 * 16 = 65520 rounds to inf) / 4094 (decodes exactly) where the producer copies; 8192 / 2048 where arithmetic
sits between the value and the store (softmax averages of a constant v).  tests/test_f16_range_cpu.py derives them from the format.

Ledger: producer -> tag -> test
  vrd_bct_to_btc (vec / scalar kernel, frames=, index=)                 1   test_bct_to_btc
  vrd_pack_pairs                                                        1   test_pack_pairs
  vrd_gather_pairs (ops.gather_pairs / gather_rows)                     1   test_gather_rows
  vrd_assemble_pairs (f32 rows only: reports nothing, its consumer does) -   test_assemble_pairs_writes_f32_rows_its_consumer_reports
  vrd_layernorm (C 256 / 512, relu, post_add, out= slab)                2   test_layernorm
  vrd_conv_ln (Cin 8 k 3, Cin 5 k 1, N 256 / 512)                       2   test_conv_ln
  vrd_dwconv_ln (all instantiations, stride, x_up, pre_ln, segs)        4   test_dwconv_ln, test_dwconv_ln_segs
  vrd_gemm c_pair: exact-f32 / x3 64- and 128-tile / x3-DMA / x3-big    8   test_gemm_pair_output
  vrd_gemm_batch c_pair (one launch of three)                           8   test_gemm_batch_third_call
  vrd_gemm A split while staged (k 1 / 3, a_scale)                     16   test_gemm_staged_rows, test_gemm_staged_rows_a_scale
  vrd_attention_rows, vrd_attention_bwd (q / k / v split)              16   test_attention_rows_and_bwd
  vrd_local_attn / _segs (strip kernel; per-row kernel)                32   test_local_attention, test_local_attention_per_row_kernel
  vrd_attention on f32 rows (flash kernel; VALU kernels: f32 only)     32   test_attention_f32_rows, test_attention_small_kernels_write_f32
  vrd_attention_pair (reports nothing by design)                        -   test_attention_on_pair_rows_stays_silent
  vrd_gemm_wgrad_x3 with g_scale (X split unchecked)                    -   test_wgrad_x3_out_of_range_x, test_linear_backward_*
  the word itself                                                           test_word_semantics
A new producer gets a line here and a test that calls check_producer()."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG, OK = 4095.0, 4094.0          # copy-type producers
ABIG, AOK = 8192.0, 2048.0        # producers with arithmetic between the value and the store
LIMIT = 4095.0


@pytest.fixture(autouse=True)
def _no_grad_f16x3():
    """pair rows exist only while autograd is not recording (ops.pair_mode); every test starts in f16x3 with a clear word"""
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision("f16x3")
    with torch.no_grad():
        ops.f16_range_flag().zero_()
        yield
    ops.f16_range_flag().zero_()
    ops.set_precision(old)


def zero():
    from vrdone_amd import ops
    ops.f16_range_flag().zero_()


def bits():
    from vrdone_amd import ops
    return ops.f16_range_exceeded()


def dec(out):
    from vrdone_amd import ops
    return (out.float() if isinstance(out, ops.Pair) else out).double()


def tolerance(want, mode, is_pair, rel):
    """bound on |decoded - want|: the format's decode error (vrd_common.h: f16 pair 2^-22 |y| while lo is normal, 2^-25 absolute in
    y = 16 x below; bf16 pair 2^-17 |x|; f32 rows none) plus `rel` |want| for the producer's own f32 arithmetic"""
    w = want.abs()
    t = rel * w
    if is_pair and mode == "f16x3":
        t = t + 2.0 ** -22 * w + 2.0 ** -29
    elif is_pair and mode == "bf16x3":
        t = t + 2.0 ** -17 * w
    return t


def consumer_bad_rows(pair):
    """rows of a GEMM with all-ones weights over the pair rows that come out non-finite"""
    from vrdone_amd import ops
    Cw = pair.shape[-1]
    y = ops.conv_gemm(pair, torch.ones(32, Cw, 1, device=DEV))
    return (~torch.isfinite(y)).any(-1).reshape(-1)


def check_producer(run, tag, big=BIG, ok=OK, rel=0.0, consumer=False, modes=("bf16x3", "f32")):
    """run(value) -> (output Pair / tensor, float64 expectation on the device): the four assertions of the module docstring.
    rel = 0: a copy-type producer, the value must come back bit for bit."""
    from vrdone_amd import ops
    with ops.use_precision("f16x3"):
        zero()
        out, want = run(big)
        got = bits()
        assert got == tag, f"out-of-range value: flag word {got} ({ops.describe_range(got)}), expected {tag}"
        if consumer:
            assert isinstance(out, ops.Pair)
            bad = consumer_bad_rows(out)
            assert bits() == 0, "a GEMM on pair rows reports nothing"
            assert torch.equal(bad, (want.abs() >= LIMIT * (1 - rel)).any(-1).reshape(-1)), "non-finite rows of the consumer GEMM"
        zero()
        out, want = run(ok)
        got = bits()
        assert got == 0, f"in-range value: flag word {got} ({ops.describe_range(got)})"
        val = dec(out)
        assert bool(torch.isfinite(val).all())
        if rel == 0.0:
            assert bool((want == ok).any()) and torch.equal(val[want == ok], want[want == ok]), "the in-range value must decode exactly"
        assert bool(((val - want).abs() <= tolerance(want, "f16x3", isinstance(out, ops.Pair), rel)).all())
    for mode in modes:
        with ops.use_precision(mode):
            zero()
            out, want = run(big)
            got = bits()
            assert got == 0, f"{mode}: flag word {got} ({ops.describe_range(got)})"
            val = dec(out)
            assert bool(torch.isfinite(val).all()), mode
            err = (val - want).abs()
            assert bool((err <= tolerance(want, mode, isinstance(out, ops.Pair), rel)).all()), (mode, float(err.max()))


def launches(run, *families):
    """launch counts of the named kernel families while run() executes"""
    from vrdone_amd import _hip
    _hip.prof_enable(True)
    _hip.prof_reset()
    try:
        run()
        torch.cuda.synchronize()
        rec = _hip.prof_read()
    finally:
        _hip.prof_enable(False)
        _hip.prof_reset()
    return {k: v["launches"] for k, v in rec.items() if v["launches"]} if not families else [rec[f]["launches"] for f in families]


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


# ------------------------------------------------------------------------------------------------ tag 1: boundary tensors
@pytest.mark.parametrize("T,Tx,c0,pos", [
    (72, 72, 16, (0, 0, 0)), (72, 72, 16, (1, 71, 63)), (72, 72, 16, (1, 64, 33)),       # vector kernel: 16-byte rows, two t tiles
    (71, 71, 16, (0, 0, 0)), (71, 71, 16, (1, 70, 63)), (72, 72, 13, (1, 65, 31)),       # scalar kernel: odd T / c0 off alignment
    (68, 72, 16, (1, 67, 60)), (67, 72, 16, (1, 66, 61)),                                # frames= (vector / scalar)
])
def test_bct_to_btc(T, Tx, c0, pos):
    from vrdone_amd import ops
    B, Ct, count = 2, 96, 64
    b, t, c = pos

    def run(value):
        x = torch.zeros(B, Ct, Tx, device=DEV)
        x[b, c0 + c, t] = value
        if c0 % 4:
            x = torch.cat([torch.zeros(1, device=DEV), x.reshape(-1)])[1:].view(B, Ct, Tx)      # source off 16-byte alignment
        out = ops.bct_to_btc(x, c0, count, torch.empty(B, T, count, device=DEV), pair=True, frames=None if T == Tx else T)
        return out, x[:, c0:c0 + count, :T].transpose(1, 2).double()
    check_producer(run, 1, consumer=pos == (1, 64, 33))


def test_bct_to_btc_index():
    from vrdone_amd import ops
    Bx, Ct, T, count = 3, 64, 40, 64
    index = torch.tensor([2, 0], dtype=torch.int32, device=DEV)

    def run(value):
        x = torch.zeros(Bx, Ct, T, device=DEV)
        x[2, 63, 39] = value          # source sequence 2 = output sequence 0
        x[1, 5, 5] = value            # a sequence the index leaves out: must not count
        out = ops.bct_to_btc(x, 0, count, torch.empty(2, T, count, device=DEV), pair=True, index=index)
        return out, x[index.long()].transpose(1, 2).double()
    check_producer(run, 1)
    zero()
    x = torch.zeros(Bx, Ct, T, device=DEV)
    x[1, 5, 5] = BIG
    ops.bct_to_btc(x, 0, count, torch.empty(2, T, count, device=DEV), pair=True, index=index)
    assert bits() == 0, "a source sequence that is not gathered was reported"


PACK_SHAPES = [(1024, 0), (1024, 512)]                       # (visual, clip) widths of the vidvrd / vidor_x configs
PACK_LENS = [40, 8, 23]                                      # B = 3 pairs, T = 40; the shortest pair has 8 frames
PACK_POS = [("vis", 0, 0, 0), ("vis", 1, 7, 1023), ("vis_obj", 2, 22, 517), ("clip", 1, 7, 511), ("clip_obj", 0, 39, 0)]


# (a configuration without CLIP features has no clip slab to place an element in)
PACK_CASES = [(V, Cc, *pos) for V, Cc in PACK_SHAPES for pos in PACK_POS if Cc or not pos[0].startswith("clip")]


@pytest.mark.parametrize("V,Cc,slab,p,t,c", PACK_CASES)
def test_pack_pairs(V, Cc, slab, p, t, c):
    from vrdone_amd import ops
    T, S, E, B = 40, 5, 8, 3
    C_in = 2 * V + 2 * Cc + S + 2 * E
    col = {"vis": 0, "vis_obj": V, "clip": 2 * V, "clip_obj": 2 * V + Cc}[slab] + c
    lens = torch.tensor(PACK_LENS, dtype=torch.int32, device=DEV)

    def run(value):
        mats = [torch.zeros(n, C_in, device=DEV) for n in PACK_LENS]
        mats[p][t, col] = value
        mats[0][5, 2 * V + 2 * Cc + 2] = value                 # a box feature (f32 slab): must not count
        table = torch.tensor([m.data_ptr() for m in mats], dtype=torch.int64, device=DEV)
        vis, clip, so_box, ent, mask = ops.pack_pairs(table, lens, T, V, Cc, S, E, True)
        full = torch.zeros(B, T, C_in, device=DEV, dtype=torch.float64)
        for i, m in enumerate(mats):
            full[i, :m.shape[0]] = m.double()
        want_vis = torch.cat([full[..., :V], full[..., V:2 * V]])
        want_clip = torch.cat([full[..., 2 * V:2 * V + Cc], full[..., 2 * V + Cc:2 * V + 2 * Cc]]) if Cc else None
        assert float(so_box[0, 5, 2]) == value
        return (clip, want_clip) if slab.startswith("clip") else (vis, want_vis)
    check_producer(run, 1, consumer=(slab == "vis_obj"))


@pytest.mark.parametrize("V,Cc,slab,p,t,c", PACK_CASES)
def test_gather_rows(V, Cc, slab, p, t, c):
    from vrdone_amd import ops
    from vrdone_amd.proposals import PairSource
    T, B = 40, 3
    n_rows = 90                                               # two tracklets' worth of rows; pairs start at different offsets
    s_row = torch.tensor([0, 41, 10], dtype=torch.int64, device=DEV)
    o_row = torch.tensor([45, 3, 60], dtype=torch.int64, device=DEV)
    lens = torch.tensor(PACK_LENS, dtype=torch.int32, device=DEV)
    boxes = torch.tensor([10.0, 20.0, 110.0, 220.0], device=DEV).repeat(n_rows, 1) + torch.arange(n_rows, device=DEV)[:, None].float()
    obj = slab.endswith("_obj")
    src_row = int((o_row if obj else s_row)[p]) + t

    def run(value):
        vis, clip = torch.zeros(n_rows, V, device=DEV), (torch.zeros(n_rows, Cc, device=DEV) if Cc else None)
        (clip if slab.startswith("clip") else vis)[src_row, c] = value
        source = PairSource(vis, clip, boxes, s_row, o_row, lens, 1, (1280, 720))
        o_vis, o_clip, so_box, ent, mask = ops.gather_rows(source, s_row, o_row, lens, T, 5, 8, True)
        feat, outp = (clip, o_clip) if slab.startswith("clip") else (vis, o_vis)
        want = torch.zeros(2 * B, T, feat.shape[1], device=DEV, dtype=torch.float64)
        for i in range(B):
            n = PACK_LENS[i]
            want[i, :n] = feat[int(s_row[i]):int(s_row[i]) + n].double()
            want[B + i, :n] = feat[int(o_row[i]):int(o_row[i]) + n].double()
        assert bool(torch.isfinite(so_box).all() and torch.isfinite(ent).all())
        return outp, want
    # (a source row may serve several pairs: the expectation above says which output rows hold the value)
    check_producer(run, 1, consumer=(slab == "vis" and p == 1))


def test_assemble_pairs_writes_f32_rows_its_consumer_reports():
    """vrd_assemble_pairs copies f32 rows (it has no pair-row form): the word stays 0 whatever passes, and the GEMM that splits its
    rows reports them (tag 16)."""
    from vrdone_amd import ops
    P, T, D, L, piece, reach = 3, 40, 512, 12, 8, 3
    lens = torch.tensor(PACK_LENS, dtype=torch.int32, device=DEV)
    streams = torch.zeros(200, D, device=DEV)
    snippets = torch.zeros(4 * P, L, D, device=DEV)
    stream_row = torch.tensor([0, 40, 50, 80, 120, 130], dtype=torch.int64, device=DEV)
    streams[0 + 20, 511] = BIG             # pair 0 (40 frames), subject, frame 20: from the stream rows
    snippets[2 * P + 1, 1, 0] = BIG        # pair 1 (8 frames <= piece), object start piece, frame 1
    out = ops.assemble_pairs(streams, snippets, stream_row, lens, T, piece, reach)
    assert bits() == 0
    assert float(out[0, 20, 511]) == BIG and float(out[P + 1, 1, 0]) == BIG and int((out == BIG).sum()) == 2
    ops.conv_gemm(out, torch.zeros(32, D, 1, device=DEV))
    assert bits() == 16


# ------------------------------------------------------------------------------------------------ tag 2: layernorm, conv_ln
@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("how", ["beta_first", "beta_last", "relu", "post_add", "slab"])
def test_layernorm(C, rows, how):
    from vrdone_amd import ops
    x = rnd(rows, C, seed=C + rows)
    c = {"beta_first": 0, "beta_last": C - 1, "relu": 4 * 63 + 3, "post_add": C // 2 + 1, "slab": C - 4}[how]
    r = rows - 1

    def run(value):
        gamma, beta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        want = torch.zeros(rows, C, device=DEV, dtype=torch.float64)
        kw = {}
        if how == "post_add":                 # period = rows: one row of the call carries the value
            add = torch.zeros(rows, C, device=DEV)
            add[r, c] = value
            kw["post_add"] = add
            want[r, c] = value
        else:
            beta[c] = value
            want[:, c] = value
        if how == "relu":
            kw["relu"] = True
            beta[0] = -value                  # clipped by the ReLU before the store: must not count
        if how == "slab":
            buf = torch.zeros(rows, 3 * C, device=DEV)
            kw["out"] = buf[:, C:2 * C]
        return ops.layernorm(x, gamma, beta, pair=True, **kw), want
    check_producer(run, 2, consumer=(how in ("post_add", "beta_last") and rows == 257))


@pytest.mark.parametrize("Cin,k", [(8, 3), (5, 1)])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("how", ["ln_first", "ln_last", "bias_row"])
def test_conv_ln(Cin, k, N, how):
    from vrdone_amd import ops
    B, T = 3, 11                              # 33 rows: trips of 4 rows per wave, the last one partial
    x = rnd(B, T, Cin, seed=N + Cin)
    assert ops.conv_ln_ok(x, torch.empty(N, Cin, k, device=DEV))
    c = {"ln_first": 0, "ln_last": N - 1, "bias_row": N - 5}[how]

    def run(value):
        want = torch.zeros(B, T, N, device=DEV, dtype=torch.float64)
        if how == "bias_row":                 # no LayerNorm: W = 0, bias carries the value, the row mask keeps the call's last row only
            w, bias = torch.zeros(N, Cin, k, device=DEV), torch.zeros(N, device=DEV)
            bias[c] = value
            mask = torch.zeros(B, T, dtype=torch.bool, device=DEV)
            mask[B - 1, T - 1] = True
            want[B - 1, T - 1, c] = value
            return ops.conv_ln(x, w, bias, row_mask=mask, pair=True), want
        w, bias = rnd(N, Cin, k, seed=1), rnd(N, seed=2)
        gamma, beta = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        beta[c] = value
        want[..., c] = value
        return ops.conv_ln(x, w, bias, gamma=gamma, beta=beta, pair=True), want
    check_producer(run, 2, consumer=(how == "bias_row"))


# ------------------------------------------------------------------------------------------------ tag 4: dwconv_ln
DW_VARIANTS = [(512, 3, 1, 1, False), (512, 3, 2, 1, False), (256, 3, 1, 1, True), (256, 3, 1, 2, False), (256, 1, 1, 1, False),
               (512, 1, 1, 1, False)]          # the (NV, KS, GIN) instantiations, as tests/test_gpu_ops.py::test_dwconv_ln_variants lists them


def _one_hot(C, gin, ks):
    w = torch.zeros(C, gin, ks, device=DEV)
    w[:, 0, ks // 2] = 1.0                    # y[c] = x[gin * c] at the centre tap
    return w


# (the input LayerNorm exists for group_in == 1 without x_up)
DW_CASES = [(*v, T, which) for v in DW_VARIANTS for T in (24, 33) for which in ("ln", "copy", "pre_ln")
            if which != "pre_ln" or (v[3] == 1 and not v[4])]


@pytest.mark.parametrize("C,ks,stride,gin,up,T,which", DW_CASES)
def test_dwconv_ln(C, ks, stride, gin, up, T, which):
    """Set 0: LayerNorm with gamma = 0 (beta carries the value into every row); set 1: no LayerNorm, a one-hot centre tap copies x;
    set 2: the same copy into an f32 output -- out of range there, it must not count."""
    from vrdone_amd import ops
    if (stride == 2 or up) and T % 2:
        T += 1                                # stride 2 / x_up need an even frame count: 34 instead of 33
    B = 3
    Tout = T // stride
    x0 = rnd(B, T, C * gin, seed=C + ks + T)
    c = C - 1 if which != "copy" else (C - 3 if gin == 1 else 5)
    bo, to = B - 1, Tout - 1                  # last row of the call = last row of a partial strip
    mask = torch.ones(B, Tout, dtype=torch.bool, device=DEV)

    def run(value):
        x = x0.clone()
        want = torch.zeros(B, Tout, C, device=DEV, dtype=torch.float64)
        xu = torch.zeros(B, T // 2, C * gin, device=DEV) if up else None
        kw = dict(mask_out=mask, stride=stride, x_up=xu)
        f32_big = torch.zeros(B, T, C * gin, device=DEV)
        if which == "ln":
            gamma, beta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            beta[c] = value
            want[..., c] = value
            sets = [dict(weight=rnd(C, gin, ks, seed=3), gamma=gamma, beta=beta, pair=True)]
        elif which == "copy":
            x.zero_()
            if up:
                xu[bo, to // 2, gin * c] = value                     # the value arrives through the coarser level: two frames
                want[bo, to // 2 * 2:to // 2 * 2 + 2, c] = value
            else:
                x[bo, to * stride, gin * c] = value
                want[bo, to, c] = value
            sets = [dict(weight=_one_hot(C, gin, ks), pair=True)]
        else:
            pg, pb = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            pb[c] = value
            want[..., c] = value
            kw["pre_ln"] = (pg, pb)
            sets = [dict(weight=_one_hot(C, gin, ks), pair=True)]
        if gin == 1 and which != "pre_ln":
            # an f32 output set of the same call, far out of range in a place of its own
            wf = torch.zeros(C, gin, ks, device=DEV)
            wf[:, 0, ks // 2] = 3.0
            sets.append(dict(weight=wf, bias=torch.full((C,), 1.0e6, device=DEV)))
        outs = ops.dwconv_ln(x, sets, **kw)
        if len(outs) > 1:
            assert not isinstance(outs[1], ops.Pair) and float(outs[1].abs().max()) >= 1.0e6
        return outs[0], want
    check_producer(run, 4, consumer=(which == "copy" and T == 24))


@pytest.mark.parametrize("C,ks,stride", [(512, 3, 1), (512, 3, 2), (256, 3, 1), (256, 1, 1), (512, 1, 1)])
@pytest.mark.parametrize("layout", ["third_of_three", "second_of_three_ln", "behind_f32"])
def test_dwconv_ln_every_output_set(C, ks, stride, layout):
    """The q / k / v form of the call: up to three weight sets share x.  Only the set under test carries the value -- the third of
    three pair-row sets (a copy), the second of three (through its LayerNorm's beta), or a pair-row set behind an f32 set that is
    itself far out of range.  The sets in front must come out in range and unchanged."""
    from vrdone_amd import ops
    B, T = 3, 24
    Tout = T // stride
    bo, to, c = B - 1, Tout - 1, C - 2
    mask = torch.ones(B, Tout, dtype=torch.bool, device=DEV)
    half = torch.zeros(C, 1, ks, device=DEV)
    half[:, 0, ks // 2] = 0.5

    def run(value):
        x = torch.zeros(B, T, C, device=DEV)
        want = torch.zeros(B, Tout, C, device=DEV, dtype=torch.float64)
        if layout == "second_of_three_ln":
            x[bo, to * stride, c] = 1.0
            gamma, beta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            beta[c] = value
            want[..., c] = value
            sets = [dict(weight=half, pair=True), dict(weight=half, gamma=gamma, beta=beta, pair=True), dict(weight=half, pair=True)]
            at, quiet = 1, (0, 2)
        else:
            x[bo, to * stride, c] = value
            want[bo, to, c] = value
            if layout == "third_of_three":        # sets 0 and 1 halve x: 2047.5 at most, in range
                sets = [dict(weight=half, pair=True), dict(weight=half, pair=True), dict(weight=_one_hot(C, 1, ks), pair=True)]
                at, quiet = 2, (0, 1)
            else:
                sets = [dict(weight=_one_hot(C, 1, ks), bias=torch.full((C,), 1.0e6, device=DEV)), dict(weight=_one_hot(C, 1, ks), pair=True)]
                at, quiet = 1, ()
        outs = ops.dwconv_ln(x, sets, mask_out=mask, stride=stride)
        for o in quiet:
            assert float(dec(outs[o]).abs().max()) == (0.5 if layout == "second_of_three_ln" else value / 2)
        if layout == "behind_f32":
            assert not isinstance(outs[0], ops.Pair) and float(outs[0].min()) >= 1.0e6
        return outs[at], want
    check_producer(run, 4, consumer=(C == 512 and ks == 3))


@pytest.mark.parametrize("C,ks,stride", [(512, 3, 1), (512, 3, 2), (256, 1, 1)])
def test_dwconv_ln_segs(C, ks, stride):
    from vrdone_amd import ops
    segs = [(0, 2, 16), (32, 1, 24)]          # (first row, sequences, frames): 56 rows, the last group's last strip is partial
    R = 56
    Ro = R // stride
    row_in, row_out = R - stride, Ro - 1      # the last output row of the call

    def run(value):
        x = torch.zeros(1, R, C, device=DEV)
        x[0, row_in, 7] = value
        want = torch.zeros(1, Ro, C, device=DEV, dtype=torch.float64)
        want[0, row_out, 7] = value
        mask = torch.ones(1, Ro, dtype=torch.bool, device=DEV)
        return ops.dwconv_ln(x, [dict(weight=_one_hot(C, 1, ks), pair=True)], mask_out=mask, stride=stride, segs=segs)[0], want
    check_producer(run, 4, consumer=True)


# ------------------------------------------------------------------------------------------------ tag 8: GEMM pair outputs
# (kernel family, M, Cin, pair-row A): shapes from vrd_gemm's own thresholds (csrc/vrd_gemm.hip, choose_x3; vrd_gemm_x3.hip):
#   exact f32: K % 32 != 0;  x3 64-tile: fewer than 256 tiles of 128 x 128;  x3 128-tile: N = 320 is 3 tile columns, 86 tile rows
#   make 258;  DMA: pair-row A, N >= 192, ceil(M / 128) * ceil(N / 256) >= 512 -> 256 tile rows, K = 32 keeps the 256 x 256 kernel
#   out (it needs K >= 96);  big: K = 96, M % 64 == 0, ceil(M / 256) * 2 >= 512 -> 255 * 256 + 64 rows.
# Every M ends in a partial tile of its kernel, N = 320 in a partial tile column of every kernel.
GEMM_KERNELS = {
    "f32_7": ("gemm_f32_mfma", 7, 40, False), "f32_300": ("gemm_f32_mfma", 300, 40, False),
    "x3_7": ("gemm_x3_mfma", 7, 64, False), "x3_300": ("gemm_x3_mfma", 300, 64, True),
    "x3_128": ("gemm_x3_mfma", 85 * 128 + 20, 32, False),
    "dma": ("gemm_x3_dma", 255 * 128 + 20, 32, True),
    "big": ("gemm_x3_big", 255 * 256 + 64, 96, True),
}
GEMM_N = 320


def _gemm_run(M, Cin, apair, epi, pos, N=GEMM_N):
    """W = 0; the value sits in bias (every row) or in res2 (one element): epi = "bias" | "rows" (row_mask + scale + res + res2) |
    "unaligned" (rows, with res2 a column view one float off 16-byte alignment: vrd_gemm then cannot take its float4 epilogue and
    writes straight from the accumulator layout, element by element)"""
    from vrdone_amd import ops
    m, n = pos
    w = torch.zeros(N, Cin, 1, device=DEV)
    a = torch.zeros(M, Cin, device=DEV)

    def run(value):
        x = ops.Pair(a, Cin) if (apair and ops.pair_fmt()) else a
        bias = torch.zeros(N, device=DEV)
        want = torch.zeros(M, N, device=DEV, dtype=torch.float64)
        kw = {}
        if epi == "bias":
            bias[n] = value
            want[:, n] = value
        else:
            res2 = torch.zeros(M, N + 1, device=DEV)[:, 1:] if epi == "unaligned" else torch.zeros(M, N, device=DEV)
            res2[m, n] = value
            want[m, n] = value
            kw = dict(row_mask=torch.ones(M, dtype=torch.bool, device=DEV), scale=torch.ones(N, device=DEV),
                      res=torch.zeros(M, N, device=DEV), res2=res2)
        return ops.conv_gemm(x, w, bias, out_pair=bool(ops.pair_fmt()), **kw), want
    return run


# (the 64-tile kernel has one epilogue, the DMA and 256 x 256 kernels need 16-byte aligned rows: the element-wise epilogue is
# reached by the exact-f32 kernel and the 128-tile split kernel)
GEMM_CASES = [(name, epi) for name in GEMM_KERNELS for epi in ("bias", "rows")] + [("f32_300", "unaligned"), ("x3_128", "unaligned")]


@pytest.mark.parametrize("name,epi", GEMM_CASES)
def test_gemm_pair_output(name, epi):
    from vrdone_amd import ops
    family, M, Cin, apair = GEMM_KERNELS[name]
    run = _gemm_run(M, Cin, apair, epi, (M - 1, GEMM_N - 1))
    got = launches(lambda: run(OK))
    assert got == {family: 1}, f"the call was meant for {family}: {got}"
    # (the f32 mode has no pair rows: its leg checks the f32 output of the exact-f32 kernel on the same shape)
    check_producer(run, 8, consumer=(epi != "bias"))
    if epi != "bias":                         # ... and the first row / first column
        check_producer(_gemm_run(M, Cin, apair, epi, (0, 0)), 8, modes=())


def test_gemm_batch_third_call():
    """vrd_gemm_batch: three problems the 256 x 256 kernel takes run as ONE launch; the value is in the third one's bias."""
    from vrdone_amd import ops
    _, M, Cin, _ = GEMM_KERNELS["big"]
    a = torch.zeros(M, Cin, device=DEV)
    ws = [torch.zeros(GEMM_N, Cin, 1, device=DEV) for _ in range(3)]

    def batch(value):
        biases = [torch.zeros(GEMM_N, device=DEV) for _ in range(3)]
        biases[2][GEMM_N - 1] = value
        return ops.conv_gemm_batch([((ops.Pair(a, Cin), ws[i], biases[i]), dict(out_pair=True)) for i in range(3)])
    assert launches(lambda: batch(OK)) == {"gemm_x3_big": 1}
    zero()
    outs = batch(BIG)
    assert bits() == 8
    assert bool(consumer_bad_rows(outs[2]).all()) and not bool(consumer_bad_rows(outs[0]).any())
    zero()
    outs = batch(OK)
    assert bits() == 0
    assert float(outs[2].float()[M - 1, GEMM_N - 1]) == OK and float(outs[1].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ tag 16: rows split while staged
@pytest.mark.parametrize("M,T,Cin,k,N,pos", [
    (300, 100, 64, 1, 160, (0, 0)), (300, 100, 64, 1, 160, (299, 63)),                    # 64-row tiles: first row, last row of the partial tile
    (85 * 128 + 20, 1, 32, 1, 320, (85 * 128 + 19, 31)),                                   # 128-row tiles, last K column
    (300, 100, 32, 3, 160, (64, 31)), (300, 100, 32, 3, 160, (199, 0)), (300, 100, 32, 3, 160, (200, 5)),
])                                            # k = 3: the first row behind a tile of 64 (a neighbour tap of the tile before), sequence ends
def test_gemm_staged_rows(M, T, Cin, k, N, pos):
    """conv_gemm on f32 rows in f16x3: A is split as it is staged.  W = 0 keeps the output (f32 rows) at 0 in the other modes; in
    f16x3 the split kernel must report the row it could not represent (and its output is NaN there: 0 * inf)."""
    from vrdone_amd import ops
    w = torch.zeros(N, Cin, k, device=DEV)
    x = torch.zeros(M // T, T, Cin, device=DEV)
    x.view(M, Cin)[pos[0], pos[1]] = BIG
    assert ops.split_forward(x, w)
    assert launches(lambda: ops.conv_gemm(x, w), "gemm_x3_mfma") == [1]
    zero()
    y = ops.conv_gemm(x, w)
    assert bits() == 16
    bad = (~torch.isfinite(y)).any(-1).reshape(-1).nonzero().flatten().tolist()
    t = pos[0] % T
    touched = [pos[0] + d for d in ((-1, 0, 1) if k == 3 else (0,)) if 0 <= t + d < T]
    assert bad == touched, "rows of the output that the out-of-range element enters"
    x.view(M, Cin)[pos[0], pos[1]] = OK
    y = ops.conv_gemm(x, w)
    assert bits() == 0 and float(y.abs().max()) == 0.0
    x.view(M, Cin)[pos[0], pos[1]] = BIG
    for mode in ("bf16x3", "f32"):
        with ops.use_precision(mode):
            y = ops.conv_gemm(x, w)
            assert bits() == 0 and float(y.abs().max()) == 0.0, mode


def test_gemm_staged_rows_a_scale():
    """The input-gradient GEMM splits its rows at the caller's factor (vrd_gemm_args.a_scale): the flag follows x * a_scale[0], not
    x * 2^4."""
    from vrdone_amd import _hip, ops
    M, Nw, Cw = 300, 64, 32                   # dy (M, Nw) . W (Nw, Cw, 1) -> dx (M, Cw)
    w = torch.zeros(Nw, Cw, 1, device=DEV)
    for factor, value, want in [(1.0, 65519.0, 0), (1.0, 65520.0, 16), (1.0, BIG, 0), (0.25, 4 * BIG, 0), (0.25, 65520.0 * 4, 16),
                                (64.0, BIG / 4, 16), (64.0, 1023.0, 0)]:
        scale = torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV)
        scale[0], scale[1] = factor, 1.0 / factor
        dy = torch.zeros(M, Nw, device=DEV)
        dy[M - 1, Nw - 1] = value
        zero()
        ops.conv_dgrad(dy, w, a_scale=scale, fmt=_hip.PAIR_F16)
        assert bits() == want, (factor, value)


@pytest.mark.parametrize("where", ["q", "k", "v"])
@pytest.mark.parametrize("pos", [(0, 0, 0), (1, 39, 127)])
def test_attention_rows_and_bwd(where, pos):
    """vrd_attention_rows (the training forward) and vrd_attention_bwd split q / k / v as they stage them: head_dim 64, B = 2,
    Tq = Tk = 40 (a partial second tile on both axes).  The bf16 form of either leaves the word alone."""
    from vrdone_amd import _hip, ops
    lib = _hip.lib
    B, T, H, hd = 2, 40, 2, 64
    Cw = H * hd
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = {n: rnd(B, T, Cw, seed=i, scale=0.1) for i, n in enumerate(("q", "k", "v", "dO"))}

    def forward(fmt):
        out, lse = torch.empty(B, T, Cw, device=DEV), torch.empty(B, H, T, device=DEV)
        _hip.check(lib.vrd_attention_rows(t["q"].data_ptr(), Cw, t["k"].data_ptr(), t["v"].data_ptr(), Cw, None, B, T, T, H, hd, fmt,
                                          out.data_ptr(), Cw, lse.data_ptr(), st), "vrd_attention_rows")
        return out, lse

    def backward(out, lse, f16):
        dq, dk, dv = (torch.empty(B, T, Cw, device=DEV) for _ in range(3))
        scratch = torch.empty(2, B, H, T, device=DEV)
        so = ops.grad_scale(t["dO"], slot=0) if f16 else None
        sv = ops.grad_scale(t["v"], slot=1) if f16 else None
        _hip.check(lib.vrd_attention_bwd(t["q"].data_ptr(), Cw, t["k"].data_ptr(), t["v"].data_ptr(), Cw, out.data_ptr(), t["dO"].data_ptr(),
                                         Cw, None, B, T, T, H, hd, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                         None if lse is None else lse.data_ptr(), scratch.data_ptr(),
                                         None if so is None else so.data_ptr(), None if sv is None else sv.data_ptr(), st), "vrd_attention_bwd")
        return dq, dk, dv

    clean_out, clean_lse = forward(_hip.PAIR_F16)
    assert bits() == 0
    backward(clean_out, clean_lse, True)
    assert bits() == 0
    for value, want in ((BIG, 16), (OK, 0), (-BIG, 16)):
        t[where][pos] = value
        zero()
        out, lse = forward(_hip.PAIR_F16)
        assert bits() == want, ("vrd_attention_rows", value)
        # the backward on its own (no forward of this call ran on these rows: lse recomputed, and with the forward's lse)
        for keep in (None, clean_lse):
            zero()
            backward(clean_out, keep, True)
            assert bits() == want, ("vrd_attention_bwd", value, keep is None)
    t[where][pos] = BIG
    zero()
    out, lse = forward(_hip.PAIR_BF16)
    grads = backward(out, lse, False)
    assert bits() == 0
    assert all(bool(torch.isfinite(g).all()) for g in (out, *grads))
    if where == "v":                          # the value passes through as a softmax average: against float64
        q, k, v = (t[n].double().view(B, T, H, hd).transpose(1, 2) for n in ("q", "k", "v"))
        ref = (torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1) @ v).transpose(1, 2).reshape(B, T, Cw)
        assert float((out.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())       # (bf16x3 bound of tests/test_gpu_backward.py)


# ------------------------------------------------------------------------------------------------ tag 32: attention outputs
def _local_case(n_head, half_win, segs, b, c):
    """v is constant along t in channel c of one sequence, so every output row of that sequence is value * sum(p) = value (1 +- 1e-6)"""
    from vrdone_amd import ops
    Cw = 512
    if segs:
        shape, rows = (1, 88, Cw), slice(48, 88)                     # [(0, 2, 24), (48, 1, 40)]: the last group
    else:
        shape, rows = (3, 40, Cw), None                              # strips of 16 rows: the third of a sequence is partial
    q, k = rnd(*shape, seed=1, scale=0.5), rnd(*shape, seed=2, scale=0.5)
    mask = torch.ones(shape[:2], dtype=torch.bool, device=DEV)

    def run(value):
        v = torch.zeros(*shape, device=DEV)
        want = torch.zeros(*shape, device=DEV, dtype=torch.float64)
        if segs:
            v[0, rows, c] = value
            want[0, rows, c] = value
        else:
            v[b, :, c] = value
            want[b, :, c] = value
        return ops.local_attention(q, k, v, mask, n_head, half_win, pair=True, segs=[(0, 2, 24), (48, 1, 40)] if segs else None), want
    return run


# the probabilities of a row sum to 1 within (W + 2) roundings of 2^-24 (W <= 9 window slots, f32 exp and reciprocal): 2e-6
LOCAL_REL = 2e-6


@pytest.mark.parametrize("n_head", [4, 8])
@pytest.mark.parametrize("half_win", [3, 4])
@pytest.mark.parametrize("segs,b,c", [(False, 0, 0), (False, 2, 511), (True, 0, 259)])
def test_local_attention(n_head, half_win, segs, b, c):
    run = _local_case(n_head, half_win, segs, b, c)
    assert launches(lambda: run(AOK), "local_attn") == [1]
    check_producer(run, 32, big=ABIG, ok=AOK, rel=LOCAL_REL, consumer=(c == 511 and half_win == 3))


def _per_row_child():
    """runs in a fresh process with VRD_LOCAL_STRIP=0 (the library reads the switch once): the one-wave-per-row kernel"""
    assert os.environ.get("VRD_LOCAL_STRIP") == "0" and "vrdone_amd" not in sys.modules
    from vrdone_amd import ops
    with torch.no_grad():
        ops.set_precision("f16x3")
        for n_head in (4, 8):
            check_producer(_local_case(n_head, 3, False, 2, 511), 32, big=ABIG, ok=AOK, rel=LOCAL_REL, consumer=True)
            check_producer(_local_case(n_head, 4, False, 0, 0), 32, big=ABIG, ok=AOK, rel=LOCAL_REL)
    print("per-row kernel: ok")


def test_local_attention_per_row_kernel():
    """The per-row banded kernel runs only under VRD_LOCAL_STRIP=0, which the library reads once per process: a child process.
    Both banded kernels record under the same profiler family (local_attn), so launch counts cannot tell them apart: that the
    child ran the per-row kernel rests on vrd_local_attn honouring the switch (csrc/vrd_local_attn.hip, local_attn_launch), which the
    child checks is set in its own environment before the library is loaded."""
    env = dict(os.environ, VRD_LOCAL_STRIP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "per-row"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "per-row kernel: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _attn_case(hd, Tq, Tk, b, c, n_head=2):
    from vrdone_amd import ops
    B, Cw = 2, n_head * hd
    q, k = rnd(B, Tq, Cw, seed=3, scale=0.3), rnd(B, Tk, Cw, seed=4, scale=0.3)

    def run(value):
        v = torch.zeros(B, Tk, Cw, device=DEV)
        v[b, :, c] = value
        want = torch.zeros(B, Tq, Cw, device=DEV, dtype=torch.float64)
        want[b, :, c] = value
        return ops.attention(q, k, v, None, n_head, pair=True), want
    return run


@pytest.mark.parametrize("hd,Tq,Tk,b,c", [(64, 40, 40, 0, 0), (64, 40, 77, 1, 127), (128, 40, 40, 1, 255), (128, 130, 40, 0, 128),
                                          (64, 9, 36, 1, 64),           # (9 queries: head_dim 64 still takes the flash kernel)
                                          (64, 128, 40, 1, 127), (128, 128, 40, 0, 255)])     # 4 query tiles: the NW = 4 instantiations
def test_attention_f32_rows(hd, Tq, Tk, b, c):
    """vrd_attention on f32 q / k / v with pair-row output: the exact-f32 flash kernel (head_dim 64 / 128).  sum(p) = 1 within the
    f32 roundings of up to 77 accumulated probabilities and the final reciprocal: 1e-5."""
    run = _attn_case(hd, Tq, Tk, b, c)
    assert launches(lambda: run(AOK)) == {"attn_flash": 1}
    check_producer(run, 32, big=ABIG, ok=AOK, rel=1e-5, consumer=(Tq == 40 and Tk == 40 and hd == 64))


@pytest.mark.parametrize("Tq", [9, 40])
def test_attention_small_kernels_write_f32(Tq):
    """head_dim 32 goes to the VALU kernels (LDS-staged for Tq <= 16), which write f32 rows only: pair=True returns a plain tensor,
    nothing is converted and the word stays 0."""
    from vrdone_amd import ops
    run = _attn_case(32, Tq, 36, 1, 63)
    assert launches(lambda: run(AOK)) == {"attn_small": 1}
    out, want = run(ABIG)
    assert not isinstance(out, ops.Pair) and bits() == 0
    assert float((out.double() - want).abs().max()) <= 1e-5 * ABIG


def test_attention_on_pair_rows_stays_silent():
    """vrd_attention_pair reports nothing by design (its value rows were checked when they were written): in-range inputs give a
    finite output and leave the word at 0."""
    from vrdone_amd import ops
    B, T, H, Cw = 2, 40, 4, 256
    gamma, beta = torch.zeros(Cw, device=DEV), torch.zeros(Cw, device=DEV)
    beta[Cw - 1] = OK
    v = ops.layernorm(rnd(B, T, Cw, seed=5), gamma, beta, pair=True)
    q = ops.layernorm(rnd(B, T, Cw, seed=6), torch.ones(Cw, device=DEV), torch.zeros(Cw, device=DEV), pair=True)
    k = ops.layernorm(rnd(B, T, Cw, seed=7), torch.ones(Cw, device=DEV), torch.zeros(Cw, device=DEV), pair=True)
    assert bits() == 0
    out = ops.attention(q, k, v, None, H)
    assert bits() == 0 and bool(torch.isfinite(out).all())
    assert float((out[..., Cw - 1] - OK).abs().max()) <= 1e-4 * OK and float(out[..., :Cw - 1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the word
def test_word_semantics():
    """Bits accumulate across launches until cleared; f16_range_exceeded(clear=False) leaves them; a launch on a second stream is
    seen after synchronisation."""
    from vrdone_amd import ops
    Cw = 256
    x, gamma, beta = rnd(5, Cw), torch.zeros(Cw, device=DEV), torch.zeros(Cw, device=DEV)
    beta[3] = BIG
    src = torch.zeros(1, 32, 8, device=DEV)
    src[0, 1, 2] = BIG
    assert ops.f16_range_exceeded(clear=False) == 0
    ops.layernorm(x, gamma, beta, pair=True)
    assert ops.f16_range_exceeded(clear=False) == 2
    beta[3] = OK
    ops.layernorm(x, gamma, beta, pair=True)                       # an in-range launch does not clear
    assert ops.f16_range_exceeded(clear=False) == 2
    ops.bct_to_btc(src, 0, 32, torch.empty(1, 8, 32, device=DEV), pair=True)
    assert ops.f16_range_exceeded(clear=False) == 3 and ops.f16_range_exceeded(clear=False) == 3
    assert ops.describe_range(3).count(",") == 1
    assert ops.f16_range_exceeded() == 3 and ops.f16_range_exceeded() == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.bct_to_btc(src, 0, 32, torch.empty(1, 8, 32, device=DEV), pair=True)
    side.synchronize()
    assert ops.f16_range_exceeded() == 1


# ------------------------------------------------------------------------------------------------ weight gradient on an out-of-range X
@pytest.mark.parametrize("M", [200, 300])     # 200 rows: the wave-per-tile kernel; 300 (>= 256): the LDS kernel
@pytest.mark.parametrize("k", [1, 3])
def test_wgrad_x3_out_of_range_x(M, k):
    """vrd_gemm_wgrad_x3 with g_scale splits X at 2^4 without a tracker.  Decided and pinned here: the call either reports, or
    every dW entry of the element's column(s) is non-finite and every other column is the float64 result (tolerance of
    tests/test_gpu_backward.py::test_linear_backward for the mode, 2e-4 of the largest entry) -- never a finite wrong number."""
    from vrdone_amd import _hip
    N, Cin, T = 96, 64, 100
    g = torch.Generator().manual_seed(M + k)
    G, X = torch.randn(M, N, generator=g), torch.randn(M, Cin, generator=g)
    r, ci = 150, 37                            # mid-sequence: all three taps of a k = 3 conv see the row
    X[r, ci] = BIG
    Gd, Xd = G.to(DEV), X.to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale = torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV)
    _hip.check(_hip.lib.vrd_absmax_scale(Gd.data_ptr(), N, M, N, scale.data_ptr(), st), "vrd_absmax_scale")
    dW = torch.zeros(N, k * Cin, device=DEV)
    zero()
    _hip.check(_hip.lib.vrd_gemm_wgrad_x3(Gd.data_ptr(), N, Xd.data_ptr(), Cin, None, M, N, Cin, k, T, dW.data_ptr(), None, None, 0,
                                          scale.data_ptr(), st), "vrd_gemm_wgrad_x3")
    flagged = bits()
    Xs = X.double().view(M // T, T, Cin)
    taps = [torch.nn.functional.pad(Xs, (0, 0, 1, 1))[:, t:t + T].reshape(M, Cin) for t in range(3)] if k == 3 else [X.double()]
    want = torch.cat([G.double().t() @ xt for xt in taps], 1)
    cols = [tap * Cin + ci for tap in range(k)]
    other = [j for j in range(k * Cin) if j not in cols]
    got = dW.double().cpu()
    assert flagged in (0, 16), f"flag word {flagged}: only tag 16 (rows split while staged) could name this kernel"
    if not flagged:
        assert not bool(torch.isfinite(got[:, cols]).any()), "a finite weight gradient in a column that saw an out-of-range X"
    # reported or not, the columns the element does not enter are the float64 result
    assert bool(torch.isfinite(got[:, other]).all())
    err = float((got[:, other] - want[:, other]).abs().max()) / float(want[:, other].abs().max())
    assert err <= 2e-4, err


@pytest.mark.parametrize("k,Cin,N,split", [(3, 8, 64, False), (1, 40, 64, False), (1, 64, 64, True), (3, 32, 64, True)])
def test_linear_backward_takes_the_f16_wgrad_only_behind_a_split_forward(k, Cin, N, split):
    """autograd.Linear in f16x3 on an x with one element at 4095.  Behind a forward on the exact-f32 kernel (Cin * k % 32 != 0:
    nothing checked x) the weight gradient must be the exact-f32 one -- finite and right, the word 0; behind a split forward the
    forward's own report (tag 16) covers the tensor the weight gradient splits again."""
    from vrdone_amd import ops
    g = torch.Generator().manual_seed(k * 10 + Cin)
    B, T = 3, 40
    x = torch.randn(B, T, Cin, generator=g)
    x[1, 20, Cin - 1] = BIG
    w = torch.randn(N, Cin, k, generator=g) / (Cin * k) ** 0.5
    dy = torch.randn(B, T, N, generator=g)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    assert ops.split_forward(xd.detach(), wd.detach()) == split
    with torch.enable_grad():
        zero()
        y = ops.conv_gemm(xd, wd, None)
        fwd_bits = bits()
        y.backward(dy.to(DEV))
    assert fwd_bits == (16 if split else 0)
    if split:
        return                                 # (the caller repeats the step in f32: MaskVRD.forward_training)
    assert bits() == 0
    xr, wr = x.transpose(1, 2).double().requires_grad_(True), w.double().requires_grad_(True)
    with torch.enable_grad():
        torch.nn.functional.conv1d(xr, wr, padding=k // 2).backward(dy.transpose(1, 2).double())
    for name, a, r in (("dW", wd.grad, wr.grad), ("dx", xd.grad, xr.grad.transpose(1, 2))):
        a = a.double().cpu()
        assert bool(torch.isfinite(a).all()), name
        assert float((a - r).abs().max()) <= 2e-4 * float(r.abs().max()), name          # (test_linear_backward's f16x3 bound)


if __name__ == "__main__" and sys.argv[1:] == ["per-row"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _per_row_child()
