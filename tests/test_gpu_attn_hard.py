"""The training attention kernels on the hard inputs of tests/attn_hard_cases.py, on a real MI355X: sharp rows, dominant masked
keys, exact ties, exactly uniform rows, gradients 2^12 apart between sequences, one-key sequences.

  a  ops.attention under autograd in f32 / bf16x3 / f16x3, on the route _flash_attention_route picks and with FUSED_ATTN_BWD off
  b  the C ABI vrd_attention_rows / vrd_attention_bwd with the forward's lse and with lse = NULL
  c  autograd.Attention over a row space of two groups: bit-equal to the calls group by group
  d  dO times 2^k gives dq, dk, dv times 2^k bit for bit, global and banded, every mode
  e  two backward calls back to back on one stream with dO 2^12 apart (the grad-scale slots), eager and as one replayed graph
  f  ops.local_attention backward, its row-group form and its drop form at p = 0 on the banded cases
Every output is judged per (sequence, head) block against the bounds derived in attn_hard_cases (first-order propagation of the
split, plane and f32 terms; tests/test_attn_hard_cases_cpu.py proves them on an emulation); each test prints its largest
error / bound ratio per output, mode and route, and the last one prints the table of the run."""
import pytest
import torch

import attn_hard_cases as A
from test_gpu_windows import ok, p, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARITH_OF = {"f32": "f32", "bf16x3": "bf16", "f16x3": "f16"}
MODES = tuple(ARITH_OF)
WORST = {}                      # (what, mode, route, output) -> (ratio, case)


def note(what, mode, route, res, case):
    for n, r in res.items():
        r = float(r.max())
        if r >= WORST.get((what, mode, route, n), (-1.0, ""))[0]:
            WORST[(what, mode, route, n)] = (r, case)
    print(f"[{what} {mode} route {route}] {case}: " + ", ".join(f"{n} {float(r.max()):.3e}" for n, r in res.items()))


def route_of(case, mode, fused=True):
    """the arithmetic of the backward route autograd._flash_attention_route gives the case"""
    from vrdone_amd import autograd
    arith = ARITH_OF[mode]
    old = autograd.FUSED_ATTN_BWD
    try:
        autograd.FUSED_ATTN_BWD = fused
        return arith if autograd._flash_attention_route(arith != "f32", case.hd, case.Tq, case.Tk) else "f32"
    finally:
        autograd.FUSED_ATTN_BWD = old


_inputs = {}


def inputs(case):
    if case.name not in _inputs:
        _inputs[case.name] = A.make_inputs(case)
    return _inputs[case.name]


def run(inp, mode, fused=True, dO=None):
    """ops.attention under autograd on the device: dict of out, dq, dk, dv"""
    from vrdone_amd import autograd, ops
    old = autograd.FUSED_ATTN_BWD
    try:
        autograd.FUSED_ATTN_BWD = fused
        with ops.use_precision(mode), torch.enable_grad():
            qd, kd, vd = (t.clone().to(DEV).requires_grad_(True) for t in (inp.q, inp.k, inp.v))
            out = ops.attention(qd, kd, vd, inp.km.to(DEV), A.H)
            out.backward((inp.dO if dO is None else dO).to(DEV))
    finally:
        autograd.FUSED_ATTN_BWD = old
    return dict(out=out.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)


def check(got, inp, route, what, mode):
    res = A.ratios(got, inp, route)
    note(what, mode, route, res, inp.case.name)
    if inp.case.spread and route != "f32":
        rel = A.block_rel(got, inp)
        for n in ("dq", "dk", "dv"):
            print(f"    {n} per sequence, dO 2^{inp.case.spread}: error / bound " + ", ".join(f"{float(r):.3e}" for r in res[n].amax(1)) +
                  "; error / largest entry of the block " + ", ".join(f"{float(r):.3e}" for r in rel[n]))
            for b, e in enumerate(inp.case.spread):
                sharp = "sharp" if inp.case.kind == "late_dominant" else "flat"
                for kind, val in (("error / bound", float(res[n][b].max())), ("error / largest entry", float(rel[n][b]))):
                    key = (f"{what}, {sharp} rows, sequences at dO 2^{e}: {kind}", mode, route, n)
                    if val >= WORST.get(key, (-1.0, ""))[0]:             # (nan -- a block that is exactly zero -- never enters)
                        WORST[key] = (val, inp.case.name)
                # what vrd_attn_bwd.hip states for the f16 planes: a dS entry carries 2^-25 / (s_s |dS|); with s_s max|dO| max|v| about
                # 2^10, |dS| about |dO| |v| / Tk on flat rows and randn maxima 4.5 times the typical entry, that is
                # 2^-25 x 20 Tk 2^k / 2^10 for a block at 2^-k of the largest dO: 0.8e-5 at Tk = 200 and k = 6 per entry (less in a sum),
                # so 2e-5 of the block's largest entry -- the per-tensor tolerance of
                # test_gpu_attn_train_hd32 -- holds per block at 2^0 and 2^-6; at 2^-12 only the derived bound holds
                if route == "f16" and e >= -6:
                    assert not float(rel[n][b]) > 2e-5, f"{inp.case.name} {n}, sequence {b} at dO 2^{e}: {float(rel[n][b]):.3e} of the block"
    assert A.masked_keys_are_zero(got, inp), f"{inp.case.name}: dk / dv at a masked key is not exactly zero"
    for n, r in res.items():
        assert float(r.max()) <= 1.0, f"{inp.case.name} [{mode}, route {route}] {n}: block errors over their bounds\n{r}"


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ------------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("mode,fused", [("f32", True), ("bf16x3", True), ("bf16x3", False), ("f16x3", True), ("f16x3", False)])
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_attention_under_autograd(case, mode, fused):
    inp = inputs(case)
    route = route_of(case, mode, fused)
    assert fused or route == "f32"
    check(run(inp, mode, fused), inp, route, "autograd" if fused else "five-product", mode)


# ------------------------------------------------------------------------------------------------------------------- b
ABI_CASES = [c for c in A.CASES if c.hd in (32, 64) and c.Tq >= 32 and (c.kind in ("late_dominant", "masked_dominant") or c.spread)]


@pytest.mark.parametrize("fmt_name", ["bf16", "f16"])
@pytest.mark.parametrize("case", ABI_CASES, ids=lambda c: c.name)
def test_c_abi_with_the_forwards_lse_and_without(case, fmt_name):
    from vrdone_amd import _hip, ops
    fmt = _hip.PAIR_F16 if fmt_name == "f16" else _hip.PAIR_BF16
    inp = inputs(case)
    hd, Tq, Tk = case.hd, case.Tq, case.Tk
    Cw = A.H * hd
    q, k, v, dO = (t.to(DEV) for t in (inp.q, inp.k, inp.v, inp.dO))
    kd = inp.km.to(DEV)
    out = torch.full((A.B, Tq, Cw), float("nan"), device=DEV)
    lse = torch.full((A.B, A.H, Tq), float("nan"), device=DEV)
    ok(_hip.lib.vrd_attention_rows(p(q), Cw, p(k), p(v), Cw, p(kd), A.B, Tq, Tk, A.H, hd, fmt, p(out), Cw, p(lse), stream()),
       "vrd_attention_rows")
    assert bool(torch.isfinite(lse).all()), "lse is written for every query"
    got = {}
    with ops.use_precision(fmt_name + "x3"):
        for which, use in (("lse", lse), ("null", None)):
            so = ops.grad_scale(dO, slot=0) if fmt_name == "f16" else None
            sv = ops.grad_scale(v, slot=1) if fmt_name == "f16" else None
            dq, dk, dv = (torch.full((A.B, t, Cw), float("nan"), device=DEV) for t in (Tq, Tk, Tk))
            scratch = torch.full((2 * A.B * A.H * Tq,), float("nan"), device=DEV)
            ok(_hip.lib.vrd_attention_bwd(p(q), Cw, p(k), p(v), Cw, p(out), p(dO), Cw, p(kd), A.B, Tq, Tk, A.H, hd, p(dq), p(dk), p(dv),
                                          p(use), p(scratch), p(so), p(sv), stream()), "vrd_attention_bwd")
            got[which] = dict(out=out, dq=dq, dk=dk, dv=dv)
            check(got[which], inp, fmt_name, "C ABI, " + ("the forward's lse" if use is not None else "lse = NULL"), fmt_name + "x3")
    bnd = A.bounds(inp, fmt_name)
    for n in ("dq", "dk", "dv"):
        diff = A.heads((got["lse"][n] - got["null"][n]).abs().double().cpu()).amax((-2, -1))
        assert bool((diff <= bnd[n]).all()), f"{n}: the forward's lse and the recomputed one disagree beyond the bound\n{diff / bnd[n]}"


# ------------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("mode", MODES)
def test_row_space_of_two_groups_is_the_calls_group_by_group(mode):
    """autograd.Attention with segs: a flash-route group (40 x 200) and a small one (9 x 12) in one row space"""
    from vrdone_amd import ops
    groups = [inputs(A.BY_NAME["masked_dominant_hd64_40x200"]), inputs(A.BY_NAME["grad_spread_sharp_hd64_9x12"])]
    alone = [run(g, mode) for g in groups]
    qsegs, ksegs, rq, rk = [], [], 0, 0
    for g in groups:
        qsegs.append((rq, A.B, g.case.Tq))
        ksegs.append((rk, A.B, g.case.Tk))
        rq, rk = rq + A.B * g.case.Tq, rk + A.B * g.case.Tk
    flat = lambda name: torch.cat([getattr(g, name).reshape(1, -1, getattr(g, name).shape[-1]) for g in groups], 1)      # noqa: E731
    with ops.use_precision(mode), torch.enable_grad():
        qd, kd, vd = (flat(n).to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
        km = torch.cat([g.km.reshape(1, -1) for g in groups], 1).to(DEV)
        out = ops.attention(qd, kd, vd, km, A.H, segs=(qsegs, ksegs))
        out.backward(flat("dO").to(DEV))
    got = dict(out=out.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)
    for g, one, qs, ks in zip(groups, alone, qsegs, ksegs):
        for n in A.NAMES:
            off, _, T = qs if n in ("out", "dq") else ks
            part = got[n][0, off:off + A.B * T].reshape(A.B, T, -1)
            assert same_bits(part, one[n]), (g.case.name, n)
        check(one, g, route_of(g.case, mode), "row space", mode)


# ------------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("base", A.POW2_BASES)
def test_dO_times_a_power_of_two_scales_the_gradients_bit_for_bit(base, mode):
    inp = inputs(A.BY_NAME[base])
    unit = run(inp, mode)
    for kk in A.POW2:
        scaled = run(inp, mode, dO=inp.dO * 2.0 ** kk)
        assert same_bits(scaled["out"], unit["out"])
        for n in ("dq", "dk", "dv"):
            assert same_bits(scaled[n], unit[n] * 2.0 ** kk), f"{base} [{mode}] {n}: dO 2^{kk} is not {n} 2^{kk}"


# ------------------------------------------------------------------------------------------------------------------- e
def _leaves(inp):
    return [t.clone().to(DEV).requires_grad_(True) for t in (inp.q, inp.k, inp.v)]


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("graph", [False, True])
def test_two_backward_calls_back_to_back_keep_their_own_scales(graph, mode):
    """dO scales 2^12 apart in two calls that follow each other on one stream: each is bit-equal to the call run alone (the slot 0 /
    slot 1 grad-scale buffers are rewritten by the second call while the first may still run); once more as one captured graph,
    replayed twice.  The graph is a chain: no parallel branches."""
    from vrdone_amd import ops
    a, b = inputs(A.BY_NAME["grad_spread_hd64_130x77"]), inputs(A.BY_NAME["late_dominant_hd32_40x200"])
    dOs = (a.dO * 2.0 ** 12, b.dO)
    alone = [run(a, mode, dO=dOs[0]), run(b, mode, dO=dOs[1])]
    torch.cuda.synchronize()
    km = [a.km.to(DEV), b.km.to(DEV)]
    g_dev = [d.to(DEV) for d in dOs]
    leaves = [_leaves(a), _leaves(b)]

    def pair():
        outs = [ops.attention(*leaves[i], km[i], A.H) for i in range(2)]
        return [torch.autograd.grad(outs[i], leaves[i], g_dev[i]) for i in range(2)]

    with ops.use_precision(mode), torch.enable_grad():
        if not graph:
            grads = pair()
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                pair()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            rec = torch.cuda.CUDAGraph()
            with torch.cuda.graph(rec):
                grads = pair()
            for t in grads[0] + grads[1]:
                t.fill_(float("nan"))
            rec.replay()
            rec.replay()
    torch.cuda.synchronize()
    for i, inp in enumerate((a, b)):
        for n, t in zip(("dq", "dk", "dv"), grads[i]):
            assert same_bits(t, alone[i][n]), (inp.case.name, n, "graph" if graph else "eager")


# ------------------------------------------------------------------------------------------------------------------- f
def run_band(inp, mode, form="plain", dO=None):
    from vrdone_amd import ops
    from vrdone_amd.models.blocks import Drop
    with ops.use_precision(mode), torch.enable_grad():
        qd, kd, vd = (t.clone().to(DEV).requires_grad_(True) for t in (inp.q, inp.k, inp.v))
        rel = inp.rel_pe.clone().to(DEV).requires_grad_(True)
        drop = Drop(torch.full((1,), 1234, dtype=torch.int64, device=DEV), 3, 0, 0.0) if form == "drop" else None
        out = ops.local_attention(qd, kd, vd, inp.mask.to(DEV), A.H, inp.case.W // 2, rel_pe=rel, drop=drop)
        out.backward((inp.dO if dO is None else dO).to(DEV))
    return dict(out=out.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad, drel=rel.grad)


def check_band(got, inp, what, mode):
    res = A.band_ratios(got, inp)
    note(what, mode, "f32", res, inp.case.name)
    dead = ~inp.mask
    for n in ("dk", "dv"):
        assert not bool(got[n].cpu()[dead].ne(0).any()), f"{inp.case.name}: {n} at a masked key is not exactly zero"
    for n, r in res.items():
        assert float(r.max()) <= 1.0, f"{inp.case.name} [{mode}] {n}: block errors over their bounds\n{r}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", A.BAND_CASES, ids=lambda c: c.name)
def test_banded_backward_plain_and_drop_form(case, mode):
    inp = A.make_band_inputs(case)
    plain = run_band(inp, mode)
    check_band(plain, inp, "banded", mode)
    drop = run_band(inp, mode, "drop")
    check_band(drop, inp, "banded, drop form at p = 0", mode)
    for kk in A.POW2:                                                   # (d) for banded attention
        scaled = run_band(inp, mode, dO=inp.dO * 2.0 ** kk)
        for n in ("dq", "dk", "dv", "drel"):
            assert same_bits(scaled[n], plain[n] * 2.0 ** kk), f"{case.name} [{mode}] {n}: dO 2^{kk} is not {n} 2^{kk}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", A.WINDOWS)
def test_banded_backward_row_groups(W, mode):
    """the row space [(0, 2, 24), (48, 1, 40)]: every group's rows are the bits of its own call, d rel_pe is the groups' sum"""
    from vrdone_amd import ops
    groups = [A.make_band_inputs(c) for c in A.BAND_GROUPS[W]]
    assert [(len(g.case.lens), g.case.T) for g in groups] == [(n, T) for _, n, T in A.BAND_SEGS]
    alone = [run_band(g, mode) for g in groups]
    for g, one in zip(groups, alone):
        check_band(one, g, "banded, row groups", mode)
    flat = lambda name: torch.cat([getattr(g, name).reshape(1, -1, *getattr(g, name).shape[2:]) for g in groups], 1)      # noqa: E731
    with ops.use_precision(mode), torch.enable_grad():
        qd, kd, vd = (flat(n).to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
        rel = groups[0].rel_pe.clone().to(DEV).requires_grad_(True)
        out = ops.local_attention(qd, kd, vd, flat("mask").to(DEV), A.H, W // 2, rel_pe=rel, segs=A.BAND_SEGS)
        out.backward(flat("dO").to(DEV))
    got = dict(out=out.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)
    for (off, n, T), one, g in zip(A.BAND_SEGS, alone, groups):
        for name in A.NAMES:
            assert same_bits(got[name][0, off:off + n * T].reshape(n, T, -1), one[name]), (g.case.name, name)
    want = sum(A.band_reference(g)["drel"] for g in groups)
    bnd = sum(A.band_bounds(g)["drel"] for g in groups)
    r = (rel.grad.double().cpu() - want).abs() / bnd
    print(f"[banded, row groups {mode}] w{W} drel {float(r.max()):.3e}")
    assert bool(torch.isfinite(rel.grad).all()) and float(r.max()) <= 1.0


# -------------------------------------------------------------------------------------------------------------- report
def test_zz_report_the_largest_ratios_of_this_run():
    for (what, mode, route, n), (r, case) in sorted(WORST.items()):
        print(f"REPORT {what} | {mode} | route {route} | {n} | {r:.3e} | {case}")
