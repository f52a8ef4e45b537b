"""Training-side global attention at head_dim 32 on the flash kernels (vrd_attention_rows / vrd_attention_bwd, csrc/vrd_attn_bwd.hip
instantiated at HD = 32: 64-byte plane rows, one float4 per thread and tile) on a real MI355X.

  a  ops.attention under autograd against float64 autograd of the oracle, and against the five-product route where that exists
  b  a gradient in one head leaves every other head's dq / dk / dv exactly zero
  c  the C ABI on strided windows with NaN guard bands, with the forward's lse and with lse = NULL
  d  the f16 operand-range flag of both entry points
  e  bit-equal repeats
  f  head_dim 16 and 128 are refused by name
  g  one training step of `vidvrd_h16` against the reference fixture (tests/test_attn_train_hd32_cpu.py validates it on the CPU),
     eager and as HIP graphs, with the attention launches of the step counted
Bounds: those of tests/test_gpu_backward.py::test_global_attention_backward_fused (relative to the largest entry: 1e-4 in bf16x3,
2e-5 in f16x3) and of tests/test_gpu_local_heads.py::test_training_step_width_256_matches_reference_gradients."""
import ctypes as C

import pytest
import torch

import local_heads_cases as LH
import test_attn_train_hd32_cpu as FX
import test_gpu_f16_range as R
import test_gpu_local_heads as GH
import window_cases as W
from oracle import vrd_oracle as O
from test_gpu_windows import cl, ld_of, lens_mask, ok, p, rel_close, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f16x3": 2e-5}           # test_global_attention_backward_fused
RANGE_GEMM_IN = 16                              # _hip.RANGE_TAGS


@pytest.fixture(params=["bf16x3", "f16x3"])
def split(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def inputs(n_head, Cw, Tq, Tk, masked, B=3):
    """(q, k, v, dO) as (B, T, C) rows and the key mask (None: every key valid)"""
    g = torch.Generator().manual_seed(Tq * 7 + Tk + n_head)
    km = lens_mask(B, Tk, [Tk, Tk // 2 + 3, 2]) if masked else None
    q, dO = torch.randn(B, Tq, Cw, generator=g), torch.randn(B, Tq, Cw, generator=g)
    k, v = torch.randn(B, Tk, Cw, generator=g), torch.randn(B, Tk, Cw, generator=g)
    return q, k, v, dO, km


_refs = {}


def reference(n_head, Cw, Tq, Tk, masked):
    """float64 autograd of the oracle's attention: (out, dq, dk, dv), computed once per shape"""
    key = (n_head, Cw, Tq, Tk, masked)
    if key not in _refs:
        q, k, v, dO, km = inputs(*key)
        with torch.enable_grad():
            qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
            mk = km[:, None] if masked else torch.ones(q.shape[0], 1, Tk, dtype=torch.bool)
            out = O.full_attention(cl(qr), cl(kr), cl(vr), mk, n_head)
            out.backward(cl(dO.double()))
        _refs[key] = (cl(out.detach()), qr.grad, kr.grad, vr.grad)
    return _refs[key]


def run(n_head, q, k, v, dO, km):
    """ops.attention under autograd on the device: (out, dq, dk, dv)"""
    from vrdone_amd import ops
    qd, kd, vd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, v))
    with torch.enable_grad():
        out = ops.attention(qd, kd, vd, None if km is None else km.to(DEV), n_head)
        out.backward(dO.to(DEV))
    return out.detach(), qd.grad, kd.grad, vd.grad


def five_product(fn):
    from vrdone_amd import autograd
    old = autograd.FUSED_ATTN_BWD
    try:
        autograd.FUSED_ATTN_BWD = False
        return fn()
    finally:
        autograd.FUSED_ATTN_BWD = old


NAMES = ("out", "dq", "dk", "dv")
SHAPES = [(16, 512, 96, 96, True),          # the model's own shape
          (8, 256, 32, 32, True),           # the smallest routed shape
          (8, 256, 40, 77, True),           # partial tiles on both axes
          (16, 512, 130, 64, False),        # two query workgroups; unmasked
          (8, 256, 72, 200, True),          # two key workgroups in the dk / dv kernel
          (8, 256, 33, 1056, True)]         # beyond the five-product route's 1024 keys: no comparison with it


# ------------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("n_head,Cw,Tq,Tk,masked", SHAPES)
def test_attention_forward_backward_matches_float64(n_head, Cw, Tq, Tk, masked, split):
    q, k, v, dO, km = inputs(n_head, Cw, Tq, Tk, masked)
    got = run(n_head, q, k, v, dO, km)
    for name, a, r in zip(NAMES, got, reference(n_head, Cw, Tq, Tk, masked)):
        err = float((a.double().cpu() - r).abs().max()) / float(r.abs().max())
        print(f"[{split} H{n_head} {Tq}x{Tk}] {name}: {err:.3e} of the largest entry")
    for name, a, r in zip(NAMES, got, reference(n_head, Cw, Tq, Tk, masked)):
        rel_close(a, r, TOL[split], name)
    if masked:                                   # masked keys: exactly zero dk / dv
        for name, a in (("dk", got[2]), ("dv", got[3])):
            assert not bool(a[1, Tk // 2 + 3:].any()) and not bool(a[2, 2:].any()), name
    if Tk <= 1024:
        old = five_product(lambda: run(n_head, q, k, v, dO, km))
        for name, a, r in zip(NAMES, got, old):
            rel_close(a, r, 1e-4, name + " vs the five-product route")


# ------------------------------------------------------------------------------------------------------------------- b
def test_gradient_of_one_head_stays_in_that_head(split):
    n_head, Cw, Tq, Tk = 8, 256, 40, 77
    hd = Cw // n_head
    q, k, v, dO, km = inputs(n_head, Cw, Tq, Tk, True)
    dO[..., :Cw - hd] = 0.0
    _, dq, dk, dv = run(n_head, q, k, v, dO, km)
    for name, a in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool(torch.isfinite(a).all()), name
        assert not bool(a[..., :Cw - hd].any()), f"{name}: a head without a gradient got one"
        assert bool(a[0, :, Cw - hd:].any()), name


# ------------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("fmt_name", ["bf16", "f16"])
def test_attention_rows_and_bwd_windows_hd32(fmt_name):
    """tests/test_gpu_windows.py::test_attention_rows_and_bwd_windows at head_dim 32: q / dq at ldq, k | v and dk | dv sharing rows
    at ldkv, out / dO at ldo; the backward with the forward's lse and with lse = NULL (pass 1 recomputes it)."""
    from vrdone_amd import _hip
    fmt = _hip.PAIR_F16 if fmt_name == "f16" else _hip.PAIR_BF16
    tol = TOL[fmt_name + "x3"]
    B, H, hd, Tq, Tk = 3, 8, 32, 40, 77
    Cw = H * hd
    q, k, v, dO, km = inputs(H, Cw, Tq, Tk, True)
    k, v = k * km[..., None], v * km[..., None]                 # (padded rows inside a window are zeros: the product's contract)
    with torch.enable_grad():
        qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
        outr = cl(O.full_attention(cl(qr), cl(kr), cl(vr), km[:, None], H))
        outr.backward(dO.double())
    kd = km.to(DEV)

    def scales(dOv, vv):
        if fmt != _hip.PAIR_F16:
            return None, None
        so, sv = (torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV) for _ in range(2))
        ok(_hip.lib.vrd_absmax_scale(p(dOv), ld_of(dOv), B * Tq, Cw, p(so), stream()), "vrd_absmax_scale")
        ok(_hip.lib.vrd_absmax_scale(p(vv), ld_of(vv), B * Tk, Cw, p(sv), stream()), "vrd_absmax_scale")
        return so, sv

    def forward(qv, kv, vv, ov):
        lse = torch.full((B, H, Tq), float("nan"), device=DEV)
        ok(_hip.lib.vrd_attention_rows(p(qv), ld_of(qv), p(kv), p(vv), ld_of(kv), p(kd), B, Tq, Tk, H, hd, fmt, p(ov), ld_of(ov), p(lse), stream()),
           "vrd_attention_rows")
        return lse

    def backward(qv, kv, vv, ov, dOv, dqv, dkv, dvv, lse):
        so, sv = scales(dOv, vv)
        scratch = torch.full((2 * B * H * Tq,), float("nan"), device=DEV)
        ok(_hip.lib.vrd_attention_bwd(p(qv), ld_of(qv), p(kv), p(vv), ld_of(kv), p(ov), p(dOv), ld_of(ov), p(kd), B, Tq, Tk, H, hd, p(dqv), p(dkv),
                                      p(dvv), p(lse), p(scratch), p(so), p(sv), stream()), "vrd_attention_bwd")

    ldq, ldkv, ldo = Cw + 64, 2 * Cw + 96, Cw + 128
    hq = W.embed(q.to(DEV), ld=ldq, name="q")
    hkv = W.embed(torch.cat([k, v], -1).to(DEV), ld=ldkv, name="k|v")
    ho, hdo = W.embed_out((B, Tq, Cw), DEV, ld=ldo, name="out"), W.embed(dO.to(DEV), ld=ldo, name="dO")
    kv, vv = hkv.view[..., :Cw], hkv.view[..., Cw:]
    lse = forward(hq.view, kv, vv, ho.view)
    plain_out = torch.empty(B, Tq, Cw, device=DEV)
    plse = forward(q.to(DEV), k.to(DEV), v.to(DEV), plain_out)
    assert bool(torch.isfinite(lse).all()), "lse is written for every query"
    assert W.bits_equal(lse, plse) and W.bits_equal(ho.view, plain_out)
    rel_close(ho.view, outr, tol, "out")
    for which, use in (("the forward's lse", lse), ("lse = NULL", None)):
        hdq = W.embed_out((B, Tq, Cw), DEV, ld=ldq, name="dq")
        hdkv = W.embed_out((B, Tk, 2 * Cw), DEV, ld=ldkv, name="dk|dv")
        dkv, dvv = hdkv.view[..., :Cw], hdkv.view[..., Cw:]
        backward(hq.view, kv, vv, ho.view, hdo.view, hdq.view, dkv, dvv, use)
        plain = [torch.empty(B, t, Cw, device=DEV) for t in (Tq, Tk, Tk)]               # dq, dk, dv
        backward(q.to(DEV), k.to(DEV), v.to(DEV), plain_out, dO.to(DEV), *plain, None if use is None else plse)
        W.check([ho, hdq, hdkv], [hq, hkv, hdo])
        for name, got, ref, pl in (("dq", hdq.view, qr.grad, plain[0]), ("dk", dkv, kr.grad, plain[1]), ("dv", dvv, vr.grad, plain[2])):
            rel_close(got, ref, tol, f"{name} ({which})")
            rel_close(got, pl, tol, f"{name} ({which}) vs the dense call")
            assert W.bits_equal(got, pl), (name, which)


# ------------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("where", ["q", "k", "v"])
@pytest.mark.parametrize("row", ["first", "last"])
def test_f16_range_flag_hd32(where, row):
    """tests/test_gpu_f16_range.py::test_attention_rows_and_bwd at head_dim 32: an element beyond the f16 operand range in the last
    channel of the last head, at the first or the last row, is reported by vrd_attention_rows and by vrd_attention_bwd on its own."""
    from vrdone_amd import _hip, ops
    lib = _hip.lib
    B, T, H, hd = 2, 40, 2, 32
    Cw = H * hd
    pos = (0, 0, Cw - 1) if row == "first" else (B - 1, T - 1, Cw - 1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = {n: R.rnd(B, T, Cw, seed=i, scale=0.1) for i, n in enumerate(("q", "k", "v", "dO"))}

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
                                         Cw, None, B, T, T, H, hd, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p(lse), scratch.data_ptr(),
                                         p(so), p(sv), st), "vrd_attention_bwd")
        return dq, dk, dv

    with ops.use_precision("f16x3"), torch.no_grad():
        R.zero()
        clean_out, clean_lse = forward(_hip.PAIR_F16)
        assert R.bits() == 0
        backward(clean_out, clean_lse, True)
        assert R.bits() == 0
        try:
            for value, want in ((R.BIG, RANGE_GEMM_IN), (R.OK, 0), (-R.BIG, RANGE_GEMM_IN)):
                t[where][pos] = value
                R.zero()
                forward(_hip.PAIR_F16)
                assert R.bits() == want, ("vrd_attention_rows", value)
                for keep in (None, clean_lse):          # the backward on its own: lse recomputed, and with a forward's lse
                    R.zero()
                    backward(clean_out, keep, True)
                    assert R.bits() == want, ("vrd_attention_bwd", value, keep is None)
            t[where][pos] = R.BIG
            R.zero()
            out, lse = forward(_hip.PAIR_BF16)
            grads = backward(out, lse, False)
            assert R.bits() == 0
            assert all(bool(torch.isfinite(g).all()) for g in (out, *grads))
        finally:
            R.zero()


# ------------------------------------------------------------------------------------------------------------------- e
def test_repeats_are_bit_equal(split):
    n_head, Cw, Tq, Tk, masked = SHAPES[1]
    args = inputs(n_head, Cw, Tq, Tk, masked)
    first, second = run(n_head, *args), run(n_head, *args)
    for name, a, b in zip(NAMES, first, second):
        assert W.bits_equal(a, b), name


# ------------------------------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("hd", [16, 128])
def test_other_head_sizes_are_refused_by_name(hd):
    from vrdone_amd import _hip
    B, T, H = 1, 32, 2
    Cw = H * hd
    q, k, v, dO, out, dq, dk, dv = (torch.zeros(B, T, Cw, device=DEV) for _ in range(8))
    lse, scratch = torch.zeros(B, H, T, device=DEV), torch.zeros(2 * B * H * T, device=DEV)
    with pytest.raises(RuntimeError, match=rf"vrd_attention_rows: head_dim must be 32 or 64 \(got {hd}\)"):
        ok(_hip.lib.vrd_attention_rows(p(q), Cw, p(k), p(v), Cw, None, B, T, T, H, hd, _hip.PAIR_BF16, p(out), Cw, p(lse), stream()),
           "vrd_attention_rows")
    with pytest.raises(RuntimeError, match=rf"vrd_attention_bwd: head_dim must be 32 or 64 \(got {hd}\)"):
        ok(_hip.lib.vrd_attention_bwd(p(q), Cw, p(k), p(v), Cw, p(out), p(dO), Cw, None, B, T, T, H, hd, p(dq), p(dk), p(dv), p(lse), p(scratch),
                                      None, None, stream()), "vrd_attention_bwd")


# ------------------------------------------------------------------------------------------------------------------- g
@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16x3"])
def test_training_step_16_heads_matches_reference_gradients(graphs, precision):
    """model.train()(batch) -> total_loss.backward() of vidvrd at 16 heads against the reference's own training step: the bounds of
    tests/test_gpu_local_heads.py::test_training_step_width_256_matches_reference_gradients.  In f32 the route does not change and
    the fixture still has to hold.  Split modes, eager: the SOS layers' attention launches are flash launches, none is left on the
    generic vector-unit kernel; the figures come from the same step on the five-product route."""
    from golden_cases import compare_grads, replay_matching, train_batch
    from vrdone_amd import ops, train_graph
    from vrdone_amd.models.blocks import AffineDropPath
    with ops.use_precision(precision):
        model, mc, _ = GH.build_model(FX.CASE, train=True)
        meta, gt = FX.load_fixture()
        lens, _, _, data = train_batch(mc, GH.c_in(mc), device=DEV, spec=LH.TRAIN_C256)
        assert lens == meta["lengths"]
        for mod in model.modules():
            if isinstance(mod, AffineDropPath):
                mod.drop_prob = 0.0
        state = {}

        def step():
            if "bipartite_match" in vars(model):
                del model.bipartite_match               # the recorded assignments cover one step: start them again
            state["differing"] = replay_matching(model, meta["cases"]["nodrop"]["indices"])
            model.zero_grad(set_to_none=True)
            with torch.enable_grad():
                state["loss"] = model(data)
                state["loss"]["total_loss"].backward()

        model.enable_training_graphs(graphs)
        try:
            if graphs:
                step()
                step()                                  # (the second step replays what the first recorded)
                assert len(train_graph.recordings(model)) == 1
            elif precision == "f32":
                step()
            else:
                small, flash = R.launches(step, "attn_small", "attn_flash")
        finally:
            model.enable_training_graphs(False)
            train_graph.forget(model)
        loss, differing = state["loss"], state["differing"]
        grads = [(n, prm.grad.clone()) for n, prm in model.named_parameters()]
        want = meta["cases"]["nodrop"]["losses"]
        assert set(loss) == set(want)
        for k, v in want.items():
            print(f"[h16/{precision}/graphs={graphs}] {k}: {float(loss[k].detach()):.7f} (reference {v:.7f})")
        for k, v in want.items():
            assert abs(float(loss[k].detach()) - v) <= (1e-5 if precision == "f32" else 2e-4) * max(1.0, abs(v)), (k, float(loss[k]), v)
        assert all(len(call) <= 6 for call in differing), differing
        worst, median = compare_grads(grads, gt, meta, "nodrop", rtol=3e-2, atol_frac=1e-4,
                                      median_tol=2e-5 if precision == "f32" else 5e-4, outlier_tol=1e-3, max_outliers=3,
                                      outlier_scope=None if precision != "bf16x3" else GH.POOL_FREE)
        print(f"[h16/{precision}/graphs={graphs}] relative gradient error: worst {worst:.2e}, median {median:.2e}")
        if not graphs and precision != "f32":
            small_old, flash_old = five_product(lambda: R.launches(step, "attn_small", "attn_flash"))
            print(f"[h16/{precision}] attn_small launches {small} (five-product route {small_old}), attn_flash {flash} ({flash_old})")
            sos = small_old - small                     # forward launches of the SOS layers' attention on the generic kernel
            assert sos > 0, "the five-product route runs the SOS layers' attention forward on the generic kernel"
            # every one of them is a flash launch on the new route (one vrd_attention_rows per forward); what is left on the generic
            # kernel never took either route (fewer than 32 queries or keys: the predictor's 9-query attention)
            assert flash - flash_old == sos, (small, small_old, flash, flash_old)
