"""Global attention at head_dim 32 on the split-precision flash kernel (vrd_attn_x3.hip, attn_flash_x3_kernel<32, 4, F16>) on a
real MI355X: vrd_attention_pair / ops.attention on pair rows against the float64 oracle at the bound of the entry point's
existing test (tests/test_gpu_ops.py::test_flash_attention_pair_rows, 2e-4), on strided windows with poisoned guard bands
(tests/test_gpu_windows.py::test_attention_pair_windows), the refusals that stay, and the routing of a model with 16 heads at
width 512 (tests/local_heads_cases.py, vidvrd_h16).

In the pair-row layout a 32-channel head is exactly one [32 hi | 32 lo] block of 128 bytes, so one case gives every head its
own seed and compares head by head: a kernel that reads the neighbouring head's block fails it."""
import pytest
import torch

import local_heads_cases as LH
import window_cases as W
from oracle import vrd_oracle as O
from test_gpu_f16_range import launches
from test_gpu_ops import _to_pair, close
from test_gpu_windows import _to_pair as to_pair_fmt
from test_gpu_windows import cl, lens_mask, ok, out_win, p, same_bits, slabs, stream, win
from test_gpu_windows import close as close_what

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT = ("f16x3", "bf16x3")
TOL = 2e-4          # tests/test_gpu_ops.py::test_flash_attention_pair_rows
F = torch.nn.functional


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(params=SPLIT)
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


def oracle(q, k, v, mask, H):
    """(B, T, C) in, (B, Tq, C) float64 out"""
    return O.full_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), mask[:, None], H).transpose(1, 2)


def tile_live(qm, Tq):
    """per query row: its tile of 32 queries holds a valid one"""
    B = qm.shape[0]
    return F.pad(qm, (0, (-Tq) % 32)).reshape(B, -1, 32).any(-1).repeat_interleave(32, dim=1)[:, :Tq]


# ------------------------------------------------------------------------------------------------------- a. the oracle
# (16, 32, 144, 144): five query tiles, a full workgroup of four waves and one of a single wave.  (8, 32, 32, 2080): 65 key tiles
# (every tile is visited from 65 on), keys beyond the 2048 of the vector-unit kernel.
@pytest.mark.parametrize("B,H,hd,Tq,Tk", [(3, 8, 32, 96, 96), (3, 16, 32, 40, 77), (3, 16, 32, 144, 144), (1, 8, 32, 32, 2080)])
def test_pair_rows_against_oracle(B, H, hd, Tq, Tk, precision):
    from vrdone_amd import ops
    gen = torch.Generator().manual_seed(H + hd + Tq + Tk)
    C = H * hd
    q = torch.randn(B, Tq, C, generator=gen) * 2.0
    k = torch.randn(B, Tk, C, generator=gen)
    v = torch.randn(B, Tk, C, generator=gen)
    k[:, min(70, Tk - 1), :hd] = q[:, 5, :hd] * 2.0          # a dominant late key: forces the running-max rescale
    if Tk > 2048:
        k[:, Tk - 1, hd:2 * hd] = q[:, Tq - 1, hd:2 * hd] * 2.0      # ... and one in the last key tile, in the second head
    lens = torch.tensor([Tk, max(1, Tk // 3), 1][:B])
    mask = torch.arange(Tk)[None] < lens[:, None]
    want = oracle(q, k, v, mask, H)
    qp, kp, vp = (_to_pair(t.to(DEV)) for t in (q, k, v))
    got = ops.attention(qp, kp, vp, mask.to(DEV), H)
    print(f"[{H}x{hd} Tq {Tq} Tk {Tk} / {precision}] max error {float((got.cpu().double() - want).abs().max()):.2e}")
    close(got, want, TOL)
    got_pair = ops.attention(qp, kp, vp, mask.to(DEV), H, pair=True)
    assert isinstance(got_pair, ops.Pair)
    close(got_pair.float(), want, TOL)
    close(ops.attention(qp, kp, vp, None, H), oracle(q, k, v, torch.ones(B, Tk, dtype=torch.bool), H), TOL)
    # q_mask: rows of a 32-query tile that holds a valid query are bit-identical to the call without it; tiles (and whole
    # workgroups) of padding read 0
    qlens = torch.tensor([Tq, min(Tq, 33), 1][:B]) if B > 1 else torch.tensor([1])
    qm = torch.arange(Tq)[None] < qlens[:, None]
    masked = ops.attention(qp, kp, vp, mask.to(DEV), H, q_mask=qm.to(DEV))
    live = tile_live(qm, Tq).to(DEV)
    assert torch.equal(masked[live], got[live])
    assert bool((masked[~live] == 0).all())


def test_every_head_reads_its_own_block(precision):
    """q, k, v of every head from a seed of its own, compared with the oracle head by head (n_head = 1 on the head's 32 channels)"""
    from vrdone_amd import ops
    B, H, hd, Tq, Tk = 3, 16, 32, 40, 77
    slab = lambda seed, T, s: torch.randn(B, T, hd, generator=torch.Generator().manual_seed(seed)) * s      # noqa: E731
    q = torch.cat([slab(1000 + h, Tq, 2.0) for h in range(H)], dim=-1)
    k = torch.cat([slab(2000 + h, Tk, 1.0) for h in range(H)], dim=-1)
    v = torch.cat([slab(3000 + h, Tk, 1.0) for h in range(H)], dim=-1)
    mask = torch.arange(Tk)[None] < torch.tensor([Tk, Tk // 3, 1])[:, None]
    qp, kp, vp = (_to_pair(t.to(DEV)) for t in (q, k, v))
    got = ops.attention(qp, kp, vp, mask.to(DEV), H)
    got_pair = ops.attention(qp, kp, vp, mask.to(DEV), H, pair=True).float()
    for h in range(H):
        c = slice(h * hd, (h + 1) * hd)
        want = oracle(q[..., c], k[..., c], v[..., c], mask, 1)
        close(got[..., c], want, TOL)
        close(got_pair[..., c], want, TOL)


# ------------------------------------------------------------------------------------------------------------ b. windows
@pytest.mark.parametrize("w64", [None, "1"])
@pytest.mark.parametrize("mode", SPLIT)
def test_pair_windows(mode, w64, monkeypatch):
    """vrd_attention_pair on strided windows with NaN guard bands, with and without q_mask: the bits of the contiguous call, the
    guards untouched.  VRD_FLASH_W64=1 (no 64-queries-per-wave kernel at this head_dim) falls back to the same kernel."""
    from vrdone_amd import _hip, ops
    if w64 is None:
        monkeypatch.delenv("VRD_FLASH_W64", raising=False)
    else:
        monkeypatch.setenv("VRD_FLASH_W64", w64)
    with ops.use_precision(mode):
        fmt = ops.pair_fmt()
        g = torch.Generator().manual_seed(189)
        B, H, hd, Tq, Tk = 3, 16, 32, 40, 77
        Cw = H * hd
        km = lens_mask(B, Tk, [Tk, Tk // 3, 1])
        q = torch.randn(B, Tq, Cw, generator=g) * 2.0
        k, v = (torch.randn(B, Tk, Cw, generator=g) * km[..., None] for _ in range(2))
        k[:, 70, :hd] = q[:, 5, :hd] * 2.0 * km[:, 70, None]            # a dominant late key: the running-max rescale
        want = cl(O.full_attention(cl(q.double()), cl(k.double()), cl(v.double()), km[:, None], H))
        qp, kp, vp = (to_pair_fmt(t.to(DEV), fmt) for t in (q, k, v))
        qm = lens_mask(B, Tq, [Tq, 20, 1])
        live = tile_live(qm, Tq)
        kd, qd = km.to(DEV), qm.to(DEV)
        for q_mask in (None, qd):
            lds = W.LdSeq()
            hq = win(qp, lds, "q")
            hkv, (kv, vv) = slabs([kp, vp], lds, "kv")
            ho = out_win((B, Tq, Cw), lds, "out")
            assert len({hq.ld, hkv.ld, ho.ld}) == 3
            ok(_hip.lib.vrd_attention_pair(p(hq.view), hq.ld, p(kv), p(vv), hkv.ld, p(kd), p(q_mask), B, Tq, Tk, H, hd, p(ho.view), ho.ld, 0, fmt,
                                           stream(), ops.products()), "vrd_attention_pair")
            plain = ops.attention(ops.Pair(qp, Cw, fmt), ops.Pair(kp, Cw, fmt), ops.Pair(vp, Cw, fmt), kd, H, q_mask=q_mask)
            W.check([ho], [hq, hkv])
            same_bits(ho, plain, "out")
            if q_mask is None:
                close_what(ho.view, want, TOL, "out")
            else:
                close_what(ho.view[live.to(DEV)], want[live], TOL, "out (live query tiles)")
                assert bool((ho.view[~live.to(DEV)] == 0).all())


# -------------------------------------------------------------------------------------------------- c. refusals that stay
def _pair_call(H, hd, products, fmt):
    from vrdone_amd import _hip
    B, T, Cw = 1, 32, H * hd
    x = torch.zeros(B, T, Cw, device=DEV)
    out = torch.empty_like(x)
    return _hip.lib.vrd_attention_pair(x.data_ptr(), Cw, x.data_ptr(), x.data_ptr(), Cw, None, None, B, T, T, H, hd, out.data_ptr(), Cw, 0, fmt,
                                       stream(), products)


def test_one_product_form_is_refused_at_head_dim_32():
    from vrdone_amd import _hip
    rc = _pair_call(8, 32, 1, _hip.PAIR_F16)
    assert rc < 0
    with pytest.raises(RuntimeError, match="head_dim"):
        _hip.check(rc, "vrd_attention_pair")
    assert _pair_call(8, 64, 1, _hip.PAIR_F16) == 0                      # (the one-product form itself is still there)
    torch.cuda.synchronize()


def test_head_dim_16_is_still_refused():
    from vrdone_amd import _hip
    for fmt in (_hip.PAIR_F16, _hip.PAIR_BF16):
        rc = _pair_call(16, 16, 0, fmt)
        assert rc < 0
        with pytest.raises(RuntimeError, match=r"head_dim must be .*\(got 16\)"):
            _hip.check(rc, "vrd_attention_pair")


def test_f16x1_mode_keeps_f32_rows_at_head_dim_32():
    from vrdone_amd import ops
    with ops.use_precision("f16x1"):
        assert not ops.flash_pair_ok(16, 512, 96) and ops.flash_pair_ok(8, 512, 96)
    with ops.use_precision("f16x3"):
        assert ops.flash_pair_ok(16, 512, 96) and ops.flash_pair_ok(8, 256, 32) and not ops.flash_pair_ok(16, 512, 31)
    with ops.use_precision("f32"):
        assert not ops.flash_pair_ok(16, 512, 96)


# ------------------------------------------------------------------------------------------------------------ d. routing
_model = []


def h16_model():
    from test_gpu_local_heads import build_model, c_in
    if not _model:
        model, mc, ic = build_model("vidvrd_h16")
        model._config_eval(ic)
        _model.append((model, c_in(mc)))
    return _model[0]


def _counts(mode, lens, min_rows=None):
    """launches per family of one _mask_vrd call of the vidvrd_h16 model in `mode`; min_rows: run in the row space with buckets from
    that many rows on (tests/test_gpu_model.py launch_cases)"""
    from vrdone_amd import ops
    model, cin = h16_model()
    T = LH.MODEL_CASES["vidvrd_h16"]["T"]
    x, m = O.synth_pairs(len(lens), cin, T, lens, seed=41)
    xd, md = x.to(DEV), m.to(DEV)

    def run():
        try:
            if min_rows:
                model.ROWS_MIN_ROWS = min_rows
                plan = model._tight_plan(md, md.reshape(len(lens), T))
                assert plan and plan["rows"] and len(plan["buckets"]) > 1, plan
            model._mask_vrd(xd, md, with_aux=False)
        finally:
            model.__dict__.pop("ROWS_MIN_ROWS", None)
    with ops.use_precision(mode):
        run()                                   # (the first call in a mode builds the per-weight operand caches)
        return launches(run)


@pytest.mark.parametrize("mode", SPLIT)
def test_model_with_16_heads_runs_the_flash_kernel_in_the_batch_form(mode):
    """four pairs of 96 frames: 8 SOS self / cross attentions + the predictor's 4 x (self, cross), the figure tests/test_gpu_model.py
    pins for vidvrd itself"""
    got = _counts(mode, [96] * 4)
    assert got.get("attn_small", 0) == 0 and got.get("attn_flash", 0) == 16, got


@pytest.mark.parametrize("mode", SPLIT)
def test_model_with_16_heads_runs_the_flash_kernel_in_the_row_space(mode):
    got = _counts(mode, LH.MODEL_CASES["vidvrd_h16"]["lens"], min_rows=64)
    assert got.get("attn_small", 0) == 0 and got.get("attn_flash", 0) >= 1, got


def test_model_with_16_heads_keeps_the_vector_unit_kernel_in_f32_mode():
    got = _counts("f32", [96] * 4)
    assert got.get("attn_small", 0) > 0, got
