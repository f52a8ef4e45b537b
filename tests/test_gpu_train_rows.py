"""Training in the row space (`MaskVRD.train_rows`): the sequence-walking backward kernels over row groups (vrd_row_segs), the
autograd Functions that take a layout, and whole training steps against the reference's own gradients.

Kernels: vrd_local_attn_bwd_segs, vrd_dwconv_bwd_segs and vrd_maxpool_bwd_segs change no per-row arithmetic, so every output row
is held BIT-EQUAL to the existing entry point called group by group; rows between the groups are poisoned in every input and
must stay poison in every output (window_cases: sentinel NaNs, guard bands, distinct leading dimensions).  vrd_dwconv_wgrad_segs
sums across groups, so its order of summation differs: it is held to float64 under the bound of
tests/test_gpu_backward.py::test_column_sums_with_and_without_scratch (2e-5 of the largest entry), and with VRD_DETERMINISTIC a
repeat must be bit-equal.  The groups are [(0, 2, 32), (72, 1, 8), (80, 3, 16)]: a gap of 8 rows behind the first group, a
sequence shorter than the widest window (19 on 8 frames), one fully valid sequence, one with a single valid frame, one all-masked.

Steps: the four shipped configs on the goldens of tests/test_gpu_train.py, with the switch on and TRAIN_ROWS_MIN_ROWS = 0 (3 / 5 /
4 / 4 buckets), under exactly that module's bounds in all three precision modes; the row-space step against the batch-form step of
the same model within twice those bounds (triangle inequality); a non-flat bucket; the fallbacks; a deterministic repeat."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import window_cases as wc
from conftest import GOLDEN
from golden_cases import TRAIN_SPECS, compare_grads, replay_matching, train_batch
from test_gpu_backward import rel_close
from test_gpu_f16_range import launches
from test_gpu_train import POOL_FREE, build, c_in

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEGS = [(0, 2, 32), (72, 1, 8), (80, 3, 16)]          # (first row, sequences, frames); rows 64..71 belong to no group
ROWS = 128


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


@pytest.fixture(params=["f32", "bf16x3", "f16x3"])
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def stream():
    return torch.cuda.current_stream().cuda_stream


def row_segs(segs):
    from vrdone_amd import _hip
    return C.byref(_hip.RowSegs.of(segs))


def in_groups(segs, rows, div=1):
    """bool (rows // div,): the rows of the groups at 1 / div of the frames"""
    m = torch.zeros(rows // div, dtype=torch.bool)
    for off, n, T in segs:
        m[off // div:(off + n * T) // div] = True
    return m


def group_mask(segs, rows, seed, div=1):
    """one byte per row: the first sequence fully valid, the second a single valid frame, the third all-masked, the others random
    prefixes; rows outside the groups hold 1 (a kernel that read them would use them)"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.ones(rows // div, dtype=torch.uint8)
    s = 0
    for off, n, T in segs:
        off, T = off // div, T // div
        for b in range(n):
            valid = [T, 1, 0][s] if s < 3 else int(torch.randint(1, T + 1, (1,), generator=g))
            mask[off + b * T:off + (b + 1) * T] = (torch.arange(T) < valid).to(torch.uint8)
            s += 1
    return mask.to(DEV)


def operand(rows, cols, seed, segs, ld, div=1, name="", halves=False):
    """random (rows // div, cols) rows in a poisoned buffer of pitch ld, the rows outside the groups poisoned too
    (halves: multiples of 1 / 2, so that neighbours tie)"""
    t = torch.randn(rows // div, cols, generator=torch.Generator().manual_seed(seed))
    if halves:
        t = t.mul(2).round().div(2)
    t[~in_groups(segs, rows, div)] = wc.sentinel()
    return wc.embed(t.to(DEV), ld=ld, name=name)


def check_output(h, want, segs, rows, div=1, what=""):
    """group rows bit-equal to `want` (rows // div, cols) and finite, the other rows still poison, the guards intact"""
    inside = in_groups(segs, rows, div).to(DEV)
    got = h.result()
    assert bool(torch.isfinite(got[inside]).all()), what
    assert wc.bits_equal(got[inside], want[inside]), f"{what}: rows differ from the group-by-group calls"
    gap = got[~inside].view(torch.int32)
    assert bool((gap == wc.SENTINEL_BITS).all()), f"{what}: rows outside the groups were written"
    wc.assert_guards_intact(h)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("Cc,heads", [(256, 8), (512, 4)])
@pytest.mark.parametrize("half_win", [1, 9])
def test_local_attn_bwd_segs_equals_the_calls_group_by_group(Cc, heads, half_win):
    from vrdone_amd import _hip
    lib = _hip.lib
    W = 2 * half_win + 1
    ld, ldo, ldd = Cc + 64, Cc + 96, Cc + 128
    q, k, v = (operand(ROWS, Cc, 10 + i, SEGS, ld, name=n) for i, n in enumerate("qkv"))
    dO = operand(ROWS, Cc, 20, SEGS, ldo, name="dO")
    mask = group_mask(SEGS, ROWS, 3)
    rel = (0.3 * torch.randn(heads, W, generator=torch.Generator().manual_seed(4))).to(DEV)
    outs = [wc.embed_out((ROWS, Cc), DEV, ld=ldd, name=n) for n in ("dq", "dk", "dv")]
    scratch = torch.full((2 * ROWS * heads * W,), float("nan"), device=DEV)
    ptr = lambda h: h.view.data_ptr()          # noqa: E731
    _hip.check(lib.vrd_local_attn_bwd_segs(ptr(q), ptr(k), ptr(v), ld, ptr(dO), ldo, mask.data_ptr(), rel.data_ptr(), row_segs(SEGS), Cc,
                                           heads, half_win, *(ptr(o) for o in outs), ldd, scratch.data_ptr(), stream()),
               "vrd_local_attn_bwd_segs")
    want = [torch.zeros(ROWS, Cc, device=DEV) for _ in outs]
    ds_rows = []
    for off, n, T in SEGS:
        sl = slice(off, off + n * T)
        sc = torch.empty(2 * n * T * heads * W, device=DEV)
        dq, dk, dv = (torch.empty(n * T, Cc, device=DEV) for _ in range(3))
        gq, gk, gv, go = (h.view[sl].contiguous() for h in (q, k, v, dO))
        gm = mask[sl].contiguous()
        _hip.check(lib.vrd_local_attn_bwd(gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), Cc, go.data_ptr(), Cc, gm.data_ptr(), rel.data_ptr(),
                                          n, T, Cc, heads, half_win, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), Cc, sc.data_ptr(), stream()),
                   "vrd_local_attn_bwd")
        for w, g in zip(want, (dq, dk, dv)):
            w[sl] = g
        ds_rows.append(sc[n * T * heads * W:])
    for h, w in zip(outs, want):
        check_output(h, w, SEGS, ROWS, what=h.name)
    wc.check([], [q, k, v, dO])
    # dS of the groups' frames lies without gaps behind the P rows of the scratch: d rel_pe stays one sum
    frames = sum(n * T for _, n, T in SEGS)
    dS = scratch[ROWS * heads * W:ROWS * heads * W + frames * heads * W]
    assert wc.bits_equal(dS, torch.cat(ds_rows))
    assert bool(torch.isnan(scratch[ROWS * heads * W + frames * heads * W:]).all()), "the scratch behind the groups' dS rows was written"


def _dwconv_bwd_args(dD, ws, n_out, B, Tin, Cout, ks, stride, gin, mask_out, dx, lddx, dx_up, lddx_up):
    from vrdone_amd import _hip
    a = _hip.DwconvBwdArgs()
    for i in range(n_out):
        a.dD[i], a.lddd[i], a.w[i] = dD[i][0], dD[i][1], ws[i].data_ptr()
    a.n_out, a.B, a.Tin, a.C, a.ksize, a.stride, a.group_in = n_out, B, Tin, Cout, ks, stride, gin
    a.mask_out, a.dx, a.lddx = mask_out, dx, lddx
    if dx_up is not None:
        a.dx_up, a.lddx_up = dx_up, lddx_up
    return a


@pytest.mark.parametrize("Cout,ks,stride,gin,up,n_out", [
    (512, 3, 1, 1, False, 3),         # the float4 kernel, three sets (a block's q / k / v convs)
    (256, 3, 1, 1, False, 1),
    (256, 3, 2, 1, False, 2),         # stride 2 (a branch block)
    (256, 3, 1, 1, True, 1),          # the FPN's upsample-add
    (512, 3, 2, 1, True, 1),          # stride 2 with x_up
    (256, 3, 1, 2, False, 1),         # group_in = 2 (the FPN's top level)
    (256, 1, 1, 2, True, 1),
])
def test_dwconv_bwd_segs_equals_the_calls_group_by_group(Cout, ks, stride, gin, up, n_out):
    from vrdone_amd import _hip
    lib = _hip.lib
    Cx = Cout * gin
    ld = wc.LdSeq()
    dDs = [operand(ROWS, Cout, 30 + i, SEGS, ld(Cout), div=stride, name=f"dD{i}") for i in range(n_out)]
    ws = [torch.randn(Cout, gin, ks, generator=torch.Generator().manual_seed(40 + i)).to(DEV) for i in range(n_out)]
    mask = group_mask(SEGS, ROWS, 5, div=stride)
    dx = wc.embed_out((ROWS, Cx), DEV, ld=ld(Cx), name="dx")
    dx_up = wc.embed_out((ROWS // 2, Cx), DEV, ld=ld(Cx), name="dx_up") if up else None
    a = _dwconv_bwd_args([(h.view.data_ptr(), h.ld) for h in dDs], ws, n_out, 0, 0, Cout, ks, stride, gin, mask.data_ptr(),
                         dx.view.data_ptr(), dx.ld, dx_up.view.data_ptr() if up else None, dx_up.ld if up else 0)
    _hip.check(lib.vrd_dwconv_bwd_segs(C.byref(a), row_segs(SEGS), stream()), "vrd_dwconv_bwd_segs")
    want, want_up = torch.zeros(ROWS, Cx, device=DEV), torch.zeros(ROWS // 2, Cx, device=DEV)
    for off, n, T in SEGS:
        so = slice(off // stride, (off + n * T) // stride)
        parts = [h.view[so].contiguous() for h in dDs]
        g, gu = torch.empty(n * T, Cx, device=DEV), torch.empty(n * T // 2, Cx, device=DEV)
        gm = mask[so].contiguous()
        b = _dwconv_bwd_args([(p.data_ptr(), Cout) for p in parts], ws, n_out, n, T, Cout, ks, stride, gin, gm.data_ptr(),
                             g.data_ptr(), Cx, gu.data_ptr() if up else None, Cx)
        _hip.check(lib.vrd_dwconv_bwd(C.byref(b), stream()), "vrd_dwconv_bwd")
        want[off:off + n * T] = g
        want_up[off // 2:(off + n * T) // 2] = gu
    check_output(dx, want, SEGS, ROWS, what="dx")
    if up:
        check_output(dx_up, want_up, SEGS, ROWS, div=2, what="dx_up")
    wc.check([], dDs)


@pytest.mark.parametrize("Cc", [256, 512])
def test_maxpool_bwd_segs_equals_the_calls_group_by_group(Cc):
    from vrdone_amd import _hip
    lib = _hip.lib
    ld = wc.LdSeq()
    x = operand(ROWS, Cc, 50, SEGS, ld(Cc), name="x", halves=True)          # (ties: the gradient goes to a window's first maximum)
    dy = operand(ROWS, Cc, 51, SEGS, ld(Cc), div=2, name="dy")
    mask = group_mask(SEGS, ROWS, 6)
    dx = wc.embed_out((ROWS, Cc), DEV, ld=ld(Cc), name="dx")
    _hip.check(lib.vrd_maxpool_bwd_segs(x.view.data_ptr(), x.ld, dy.view.data_ptr(), dy.ld, row_segs(SEGS), Cc, mask.data_ptr(),
                                        dx.view.data_ptr(), dx.ld, stream()), "vrd_maxpool_bwd_segs")
    want = torch.zeros(ROWS, Cc, device=DEV)
    for off, n, T in SEGS:
        sl, so = slice(off, off + n * T), slice(off // 2, (off + n * T) // 2)
        g = torch.empty(n * T, Cc, device=DEV)
        gx, gy, gm = x.view[sl].contiguous(), dy.view[so].contiguous(), mask[sl].contiguous()
        _hip.check(lib.vrd_maxpool_bwd(gx.data_ptr(), Cc, gy.data_ptr(), Cc, n, T, Cc, gm.data_ptr(), g.data_ptr(), Cc, stream()),
                   "vrd_maxpool_bwd")
        want[sl] = g
    check_output(dx, want, SEGS, ROWS, what="dx")
    wc.check([], [x, dy])


@pytest.mark.parametrize("Cout,ks,stride,gin", [(512, 3, 1, 1), (256, 3, 2, 1), (256, 3, 1, 2), (256, 1, 1, 2)])
def test_dwconv_wgrad_segs_against_float64_and_deterministic_repeat(Cout, ks, stride, gin):
    from vrdone_amd import _hip
    lib = _hip.lib
    Cx = Cout * gin
    ld = wc.LdSeq()
    dD = operand(ROWS, Cout, 60, SEGS, ld(Cout), div=stride, name="dD")
    x = operand(ROWS, Cx, 61, SEGS, ld(Cx), name="x")
    mask = group_mask(SEGS, ROWS, 7, div=stride)
    mask[(~in_groups(SEGS, ROWS, stride)).to(DEV)] = 1
    part = torch.full((1024 * 4 * Cx + 64,), float("nan"), device=DEV)

    def run(scratch, floats, flags):
        dw, db = torch.ones(Cout, gin, ks, device=DEV), torch.ones(Cout, device=DEV)
        rc = lib.vrd_dwconv_wgrad_segs(dD.view.data_ptr(), dD.ld, x.view.data_ptr(), x.ld, ks, stride, gin, row_segs(SEGS), mask.data_ptr(),
                                       Cout, dw.data_ptr(), db.data_ptr(), scratch, floats, stream(), flags)
        _hip.check(rc, "vrd_dwconv_wgrad_segs")
        return dw, db

    want_w, want_b = torch.zeros(Cout, gin, ks, dtype=torch.float64), torch.zeros(Cout, dtype=torch.float64)
    for off, n, T in SEGS:
        To = T // stride
        so = slice(off // stride, off // stride + n * To)
        G = (dD.view[so].double() * mask[so, None].double()).cpu().view(n, To, Cout)
        xs = x.view[off:off + n * T].double().cpu().view(n, T, Cout, gin)
        want_b += G.sum((0, 1))
        for kk in range(ks):
            for t in range(To):
                ti = stride * t + kk - ks // 2
                if 0 <= ti < T:
                    want_w[:, :, kk] += torch.einsum("bc,bcg->cg", G[:, t], xs[:, ti])
    for what, (dw, db) in (("atomics", run(None, 0, 0)), ("partial sums", run(part.data_ptr(), part.numel(), 0))):
        rel_close(dw, want_w + 1, 2e-5, f"dw ({what})")
        rel_close(db, want_b + 1, 2e-5, f"dbias ({what})")
    # the deterministic mode says how much scratch it needs when it gets none
    assert lib.vrd_dwconv_wgrad_segs(dD.view.data_ptr(), dD.ld, x.view.data_ptr(), x.ld, ks, stride, gin, row_segs(SEGS), mask.data_ptr(),
                                     Cout, part.data_ptr(), None, None, 0, stream(), _hip.DETERMINISTIC) == _hip.ERR_SCRATCH
    need = C.c_int64(0)
    _hip.check(lib.vrd_scratch_required(C.byref(need)), "vrd_scratch_required")
    assert 0 < need.value <= part.numel()
    first, again = run(part.data_ptr(), part.numel(), _hip.DETERMINISTIC), run(part.data_ptr(), part.numel(), _hip.DETERMINISTIC)
    rel_close(first[0], want_w + 1, 2e-5, "dw (deterministic)")
    rel_close(first[1], want_b + 1, 2e-5, "dbias (deterministic)")
    assert wc.bits_equal(first[0], again[0]) and wc.bits_equal(first[1], again[1])
    wc.check([], [dD, x])


def test_backward_launches_do_not_grow_with_the_groups():
    """DepthwiseConv, LocalAttention and MaxPoolMask: the backward of a five-group layout is as many launches as that of one group"""
    from vrdone_amd import ops
    Cc, heads = 256, 8
    five, one = [(0, 1, 32), (32, 2, 16), (64, 1, 32), (96, 1, 16), (112, 2, 8)], [(0, 4, 32)]
    gen = torch.Generator().manual_seed(8)
    leaf = lambda *s: torch.randn(*s, generator=gen).to(DEV).requires_grad_()          # noqa: E731
    mask = torch.ones(1, ROWS, dtype=torch.bool, device=DEV)
    w, rel = leaf(Cc, 1, 3), leaf(1, 1, heads, 7)

    def counts(make):
        out = []
        for segs in (five, one):
            y = make(segs)
            g = torch.randn(y.shape, generator=gen).to(DEV)
            out.append(launches(lambda: y.backward(g), "backward")[0])
        return out

    for name, make in (("DepthwiseConv", lambda segs: ops.dwconv_ln(leaf(1, ROWS, Cc), [dict(weight=w)], mask_out=mask[:, ::2].contiguous(),
                                                                     stride=2, segs=segs)[0]),
                       ("LocalAttention", lambda segs: ops.local_attention(leaf(1, ROWS, Cc), leaf(1, ROWS, Cc), leaf(1, ROWS, Cc), mask, heads, 3,
                                                                           rel_pe=rel, segs=segs)),
                       ("MaxPoolMask", lambda segs: ops.maxpool_mask(leaf(1, ROWS, Cc), mask, segs=segs)[0])):
        n5, n1 = counts(make)
        assert n5 == n1 > 0, (name, n5, n1)


# ------------------------------------------------------------------------------------------------ steps
def golden(name):
    with open(os.path.join(GOLDEN, f"train_step_{name}.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, f"train_step_{name}.npz"))


def prepared(name, case, meta):
    """the model of a golden step with its stochastic depth off (`nodrop`) or pinned, and the batch"""
    from vrdone_amd.models.blocks import AffineDropPath
    model, mc, _ = build(name)
    lens, _, _, data = train_batch(mc, c_in(mc), device=DEV, **({} if name == "vidvrd" else {"spec": TRAIN_SPECS[name]}))
    assert lens == meta["lengths"]
    model.train()
    for mod_name, mod in model.named_modules():
        if isinstance(mod, AffineDropPath):
            if case == "nodrop":
                mod.drop_prob = 0.0
            else:
                mod.keep = torch.tensor(meta["keep"][mod_name], dtype=torch.float32)
    return model, data


def step(model, data, rows, recorded=None):
    """one training step in the row space (`rows`) or the batch form -> (losses, {name: gradient}, pairs whose matching differs)"""
    model.train_rows, model.TRAIN_ROWS_MIN_ROWS = rows, 0
    model.__dict__.pop("bipartite_match", None)
    differing = replay_matching(model, recorded) if recorded is not None else []
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        loss = model(data)
        loss["total_loss"].backward()
    return {k: float(v.detach()) for k, v in loss.items()}, {n: p.grad.detach().clone() for n, p in model.named_parameters()}, differing


def record_matching(model):
    """have model.bipartite_match keep its assignments, in replay_matching's format -> the list they are appended to"""
    real, seen = model.bipartite_match, []

    def match(*args, **kwargs):
        idx, lm = real(*args, **kwargs)
        seen.append([(i.tolist(), j.tolist()) for i, j in idx])
        return idx, lm
    model.bipartite_match = match
    return seen


def distance(a, b, atol_frac=1e-4):
    """(worst, median) over the parameters of |a - b| relative to |b| (+ atol_frac of the largest gradient norm), as compare_grads"""
    biggest = max(float(g.double().norm()) for g in b.values())
    errs = [float((a[n].double() - b[n].double()).norm()) / (float(b[n].double().norm()) + atol_frac * biggest) for n in b]
    return max(errs), float(np.median(errs))


@pytest.mark.parametrize("name,case,buckets", [("vidvrd", "nodrop", 3), ("vidvrd", "pinned", 3), ("vidor", "nodrop", 5),
                                                ("vidor_x", "nodrop", 4), ("vidor_local", "nodrop", 4)])
def test_row_space_step_matches_reference_gradients(name, case, buckets, precision):
    """The bounds are those of test_gpu_train.py::test_training_step_matches_reference_gradients (vidvrd) and
    ::test_training_step_vidor_matches_reference_gradients (the others), unchanged."""
    meta, g = golden(name)
    model, data = prepared(name, case, meta)
    model.TRAIN_ROWS_MIN_ROWS = 0
    assert len(model.train_rows_plan(meta["lengths"])) == buckets
    recorded = meta["cases"][case]["indices"]
    loss, grads, differing = step(model, data, True, recorded)
    assert model.train_form == "rows"
    want = meta["cases"][case]["losses"]
    loss_tol = 1e-5 if precision == "f32" else 2e-4
    median_tol = 2e-5 if precision == "f32" else 5e-4
    assert set(loss) == set(want)
    for k, v in want.items():
        assert abs(loss[k] - v) <= loss_tol * max(1.0, abs(v)), (k, loss[k], v)
    named = list(grads.items())
    if name == "vidvrd":
        assert all(len(call) <= 6 for call in differing), differing
        worst, median = compare_grads(named, g, meta, case, rtol=3e-2, atol_frac=1e-4, median_tol=median_tol, outlier_tol=1e-3, max_outliers=3,
                                      outlier_scope=None if case == "nodrop" and precision != "bf16x3" else POOL_FREE)
    else:
        assert all(len(call) <= 2 for call in differing), differing
        worst, median = compare_grads(named, g, meta, case, rtol=3e-2, atol_frac=1e-4, median_tol=5e-4)
        strict = [(n, gr) for n, gr in named if re.match(POOL_FREE, n)]
        assert len(strict) > 250
        compare_grads(strict, g, meta, case, rtol=3e-2, atol_frac=1e-4, median_tol=median_tol, outlier_tol=1e-3, max_outliers=3)
    # the same step in the batch form: both forms lie within the bounds above of the reference, so within twice of each other
    loss_b, grads_b, _ = step(model, data, False, recorded)
    assert model.train_form == "batch"
    d_worst, d_median = distance(grads, grads_b)
    d_loss = max(abs(loss[k] - loss_b[k]) / max(1.0, abs(loss_b[k])) for k in loss_b)
    print(f"[{name}/{case}/{precision}] rows against the reference: worst {worst:.2e}, median {median:.2e}; rows against the batch form: "
          f"worst {d_worst:.2e}, median {d_median:.2e}, losses {d_loss:.2e}")
    assert d_loss <= 2 * loss_tol and d_worst <= 2 * 3e-2 and d_median <= 2 * (median_tol if name == "vidvrd" else 5e-4)


def test_non_flat_bucket_against_the_batch_form():
    """pairs within one frame of their padded length are a bucket of their own behind the flat ones (their k = 3 convs run per bucket)"""
    from vrdone_amd import ops
    meta, _ = golden("vidvrd")
    model, data = prepared("vidvrd", "nodrop", meta)
    T = model.max_seq_len
    for key in ("so_features_list",):          # pairs 0 and 1 at T and T - 1 frames (their targets keep their own frames)
        for i, L in ((0, T), (1, T - 1)):
            f = data[key][i]
            data[key][i] = torch.cat([f, f.flip(1)] * (T // f.shape[1] + 1), dim=1)[:, :L].contiguous()
    lens = [int(f.shape[1]) for f in data["so_features_list"]]
    model.TRAIN_ROWS_MIN_ROWS = 0
    plan = model.train_rows_plan(lens)
    assert [flat for _, _, flat in plan].count(False) == 1 and plan[-1][0] == T and sorted(plan[-1][1]) == [0, 1]
    with ops.use_precision("f32"):
        # (the batch form's own matching, replayed in the row space: a near-tie between two queries must not decide the comparison)
        model.train_rows = False
        seen = record_matching(model)
        with torch.enable_grad():
            model(data)
        loss_b, grads_b, _ = step(model, data, False, seen)
        assert model.train_form == "batch"
        loss_r, grads_r, differing = step(model, data, True, seen)
        assert model.train_form == "rows" and all(len(call) <= 6 for call in differing), differing
    d_worst, d_median = distance(grads_r, grads_b)
    print(f"non-flat bucket, f32: rows against the batch form: worst {d_worst:.2e}, median {d_median:.2e}")
    # (f32 mode: twice the bounds each form is held to against the reference, as above)
    assert all(abs(loss_r[k] - loss_b[k]) <= 2e-5 * max(1.0, abs(loss_b[k])) for k in loss_b)
    assert d_worst <= 2 * 3e-2 and d_median <= 2 * 2e-5


@pytest.mark.parametrize("why", ["graphs", "dropout", "abs_pe", "train_source"])
def test_steps_that_do_not_qualify_take_the_batch_form_bit_for_bit(why):
    """deterministic mode, equal seeds: the switch changes neither the form nor a bit of a step that does not qualify"""
    import test_gpu_train_source as ts
    from vrdone_amd import ops
    overrides = {"dropout": dict(dropout=0.1), "abs_pe": dict(use_abs_pe=True)}.get(why, {})

    def run(rows):
        model, cfg = ts._model("vidvrd", **overrides)
        if why == "train_source":
            _, src, tables = ts._feeds(ts._entries(cfg["visual_dim"]), cfg["max_seq_len"], seed=1)
            data = {"train_source": src, "train_tables": tables}
        else:
            _, _, _, data = train_batch(cfg, c_in(cfg), device=DEV)
        if why == "graphs":
            model.enable_training_graphs()
        model.train_rows, model.TRAIN_ROWS_MIN_ROWS, model.dropout_seed = rows, 0, 7
        ops.set_deterministic(True)
        try:
            _, grads = ts._step(model, data)
        finally:
            ops.set_deterministic(False)
        return model.train_form, grads

    (form_on, on), (form_off, off) = run(True), run(False)
    assert form_on == form_off == "batch"
    assert all(wc.bits_equal(on[n], off[n]) for n in off)


def test_deterministic_repeat_of_a_row_space_step_is_bit_equal():
    from vrdone_amd import ops
    meta, _ = golden("vidvrd")
    model, data = prepared("vidvrd", "nodrop", meta)
    ops.set_deterministic(True)
    try:
        with ops.use_precision("f16x3"):
            _, first, _ = step(model, data, True)
            assert model.train_form == "rows"
            _, again, _ = step(model, data, True)
    finally:
        ops.set_deterministic(False)
    assert all(wc.bits_equal(first[n], again[n]) for n in first)
