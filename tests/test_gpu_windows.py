"""Every row kernel of the C ABI on strided windows with poisoned guard bands (tests/window_cases.py), on a real MI355X.

Each case embeds ALL row operands of an entry point in wider buffers -- every operand at its own leading dimension, 2 guard
rows in front, 3 behind, 32 guard columns to the left and at least 32 to the right, all holding one quiet NaN with a payload --
and asserts
  (a) the window result is finite and correct against a float64 reference, at the tolerance the op's existing direct test uses
      (tests/test_gpu_ops.py `close`, tests/test_gpu_backward.py `rel_close`);
  (b) it equals, bit for bit, the same call on plain contiguous copies (the windows are 16-byte aligned, so the host code picks
      the same kernel); sums accumulated across workgroups are bit-compared under VRD_DETERMINISTIC and held to (a) without it;
  (c) every guard element of every output buffer, and every element of every input buffer, is unchanged.
Inputs keep the product's contract: padded rows INSIDE a window are zeros, as the masked producers leave them; only memory
outside the windows is poisoned.  A kernel that uses C where ld belongs, ldx where lddy belongs, stores past its last row or
column, or loads a guard and multiplies it by a zero mask fails here (tests/test_window_cases_cpu.py shows the checker seeing
each of these)."""
import ctypes as C
import itertools
import math

import pytest
import torch

import window_cases as W
from oracle import vrd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT = ("bf16x3", "f16x3")
F = torch.nn.functional


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(params=["f32", "bf16x3", "f16x3"])
def precision(request):
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(old)


# ---------------------------------------------------------------------------------------------------------------- helpers
def close(got, want, atol, what=""):
    """tests/test_gpu_ops.py `close`: absolute, against the float64 reference"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) if got.numel() else 0.0
    assert err <= atol, f"{what}: max abs error {err:.3e} (tolerance {atol:.1e})"


def rel_close(got, want, rtol, what=""):
    """tests/test_gpu_backward.py `rel_close`: relative to the largest entry of the float64 reference"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    assert err <= rtol, f"{what}: max error {err:.3e} of the largest entry (tolerance {rtol:.1e})"


def same_bits(h, plain, what):
    assert W.bits_equal(h.view, plain), f"{what}: the window result differs from the contiguous call's bits"


def win(t, lds, name):
    return W.embed(t.to(DEV), ld=lds(t.shape[-1]), name=name)


def out_win(shape, lds, name):
    return W.embed_out(shape, DEV, ld=lds(shape[-1]), name=name)


def slabs(parts, lds, name):
    """`parts` (same shape) as the column slabs of ONE window (q / k / v of a 3C-wide projection buffer): (handle, views)"""
    h = win(torch.cat(parts, dim=-1), lds, name)
    c = parts[0].shape[-1]
    return h, [h.view[..., i * c:(i + 1) * c] for i in range(len(parts))]


def out_slabs(shape, n, lds, name):
    h = out_win(tuple(shape[:-1]) + (n * shape[-1],), lds, name)
    return h, [h.view[..., i * shape[-1]:(i + 1) * shape[-1]] for i in range(n)]


def lens_mask(B, T, lens):
    return torch.arange(T)[None] < torch.tensor(lens)[:, None]


def std_lens(T):
    return [T, T // 2, 2]


def stream():
    from vrdone_amd import ops
    return ops._stream()


def ok(rc, what):
    from vrdone_amd import _hip
    _hip.check(rc, what)


def p(t):
    return None if t is None else t.data_ptr()


def ld_of(v):
    return v.stride(-2)


def cl(x):          # (B, C, T) <-> (B, T, C)
    return x.transpose(1, 2).contiguous()


def scratch_buf(n=1 << 22):
    return torch.full((n,), float("nan"), device=DEV)


# ------------------------------------------------------------------------------------------------------ row ops, forward
@pytest.mark.parametrize("variant", ["plain", "relu", "post_add"])
@pytest.mark.parametrize("Cw", [256, 512])
def test_layernorm_windows(Cw, variant):
    from vrdone_amd import ops
    g = torch.Generator().manual_seed(Cw + len(variant))
    B, T = 3, 24
    m = lens_mask(B, T, std_lens(T))
    x = (torch.randn(B, T, Cw, generator=g) * 3 + 1) * m[..., None]
    gam, bet = torch.randn(1, Cw, 1, generator=g), torch.randn(1, Cw, 1, generator=g)
    pos = torch.randn(T, Cw, generator=g) if variant == "post_add" else None
    want = cl(O.channel_ln(cl(x.double()), gam.double(), bet.double()))
    if variant == "relu":
        want = torch.relu(want)
    if pos is not None:
        want = want + pos.double()[None]
    lds = W.LdSeq()
    hx, hy = win(x, lds, "x"), out_win((B, T, Cw), lds, "y")
    hp = win(pos, lds, "post_add") if pos is not None else None
    kw = dict(relu=variant == "relu", post_add=None if hp is None else hp.view)
    ops.layernorm(hx.view, gam.to(DEV), bet.to(DEV), out=hy.view, **kw)
    plain = ops.layernorm(x.to(DEV), gam.to(DEV), bet.to(DEV), relu=kw["relu"], post_add=None if pos is None else pos.to(DEV))
    W.check([hy], [hx] + ([hp] if hp else []))
    close(hy.view, want, 3e-6, "y")
    same_bits(hy, plain, "y")


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("Cin", [5, 8])
def test_conv_ln_windows(Cin, N):
    from vrdone_amd import ops
    g = torch.Generator().manual_seed(Cin * 10 + N)
    B, T = 3, 24
    m = lens_mask(B, T, std_lens(T))
    x = torch.randn(B, T, Cin, generator=g) * 3 * m[..., None]
    w = torch.randn(N, Cin, 3, generator=g) / (3 * Cin) ** 0.5
    b = torch.randn(N, generator=g) * 0.3
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    ln = Cin == 8                                           # the entity embedding has the LayerNorm + ReLU, the pair embedding not
    want = F.conv1d(x.double().transpose(1, 2), w.double(), b.double(), padding=1).transpose(1, 2) * m[..., None]
    if ln:
        mu = want.mean(-1, keepdim=True)
        var = ((want - mu) ** 2).mean(-1, keepdim=True)
        want = torch.relu((want - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double())
    lds = W.LdSeq()
    hx, hy = win(x, lds, "x"), out_win((B, T, N), lds, "y")
    kw = dict(row_mask=m.to(DEV), gamma=gamma.to(DEV) if ln else None, beta=beta.to(DEV) if ln else None, relu=ln)
    ops.conv_ln(hx.view, w.to(DEV), b.to(DEV), out=hy.view, **kw)
    plain = ops.conv_ln(x.to(DEV), w.to(DEV), b.to(DEV), **kw)
    W.check([hy], [hx])
    close(hy.view, want, 2e-5 * max(1.0, float(want.abs().max())), "y")          # test_few_channel_conv_layernorm_row_kernel's bound
    same_bits(hy, plain, "y")


DW_CASES = {          # tests/test_gpu_backward.py test_dwconv_ln_backward: stride, group_in, k, n_out, C, pre_ln, x_up, LayerNorm, bias
    "qkv_s1": (1, 1, 3, 3, 512, True, False, True, False),
    "qkv_s2": (2, 1, 3, 3, 512, True, False, True, False),
    "fpn_top": (1, 2, 3, 1, 256, False, False, True, False),
    "fpn_up": (1, 1, 3, 1, 256, False, True, True, False),
    "mask_features": (1, 1, 3, 1, 256, False, False, False, True),
    "k1": (1, 1, 1, 1, 256, False, False, True, False),
}


def _dwconv_case(case, segs=None):
    from vrdone_amd import ops
    stride, gin, k, n_out, Cw, pre, up, with_ln, with_bias = DW_CASES[case]
    g = torch.Generator().manual_seed(len(case) + Cw)
    B, T = 3, 24
    Cin = Cw * gin
    m_in = lens_mask(B, T, std_lens(T))
    m_out = m_in[:, ::stride].contiguous()
    x = torch.randn(B, T, Cin, generator=g) * m_in[..., None]
    xu = torch.randn(B, T // 2, Cin, generator=g) * m_in[:, ::2, None] if up else None
    ws = [torch.randn(Cw, gin, k, generator=g) / (gin * k) ** 0.5 for _ in range(n_out)]
    bs = [torch.randn(Cw, generator=g) * 0.1 if with_bias else None for _ in range(n_out)]
    gs = [1 + 0.1 * torch.randn(1, Cw, 1, generator=g) if with_ln else None for _ in range(n_out)]
    es = [0.1 * torch.randn(1, Cw, 1, generator=g) if with_ln else None for _ in range(n_out)]
    pg, pb = 1 + 0.1 * torch.randn(1, Cin, 1, generator=g), 0.1 * torch.randn(1, Cin, 1, generator=g)
    xin = cl(x.double())
    if pre:
        xin = O.channel_ln(xin, pg.double(), pb.double())
    if up:
        xin = xin + cl(xu.double()).repeat_interleave(2, dim=2)
    wants = []
    for i in range(n_out):
        d = O.masked_conv1d(xin, m_in[:, None], ws[i].double(), None if bs[i] is None else bs[i].double(), stride=stride, groups=Cw)[0]
        if with_ln:
            d = O.channel_ln(d, gs[i].double(), es[i].double())
        wants.append(cl(d))
    dv = lambda t: None if t is None else t.to(DEV)     # noqa: E731
    lds = W.LdSeq()
    shape = (lambda b, t, c: (1, b * t, c)) if segs else (lambda b, t, c: (b, t, c))
    hx = win(x.reshape(shape(B, T, Cin)), lds, "x")
    hu = win(xu.reshape(shape(B, T // 2, Cin)), lds, "x_up") if up else None
    hys = [out_win(shape(B, T // stride, Cw), lds, f"y{i}") for i in range(n_out)]
    assert len({h.ld for h in [hx] + hys + ([hu] if hu else [])}) == n_out + 1 + bool(up)
    base = [dict(weight=dv(ws[i]), bias=dv(bs[i]), gamma=dv(gs[i]), beta=dv(es[i])) for i in range(n_out)]
    sets = [dict(s, out=hys[i].view) for i, s in enumerate(base)]
    pre_ln = (pg.to(DEV), pb.to(DEV)) if pre else None
    mo = m_out.to(DEV)
    ops.dwconv_ln(hx.view, sets, mask_out=mo.reshape(1, -1) if segs else mo, stride=stride, x_up=None if hu is None else hu.view, pre_ln=pre_ln,
                  segs=segs)
    plain = ops.dwconv_ln(x.to(DEV), base, mask_out=mo, stride=stride, x_up=dv(xu), pre_ln=pre_ln)
    W.check(hys, [hx] + ([hu] if hu else []))
    for i in range(n_out):
        # test_dwconv_ln_variants holds the kernel to 2e-5, test_dwconv_ln_input_layernorm (pre_ln) to 3e-5
        close(hys[i].view.reshape(wants[i].shape), wants[i], 3e-5 if pre else 2e-5, f"y{i}")
        same_bits(hys[i], plain[i].reshape(hys[i].view.shape), f"y{i}")


@pytest.mark.parametrize("case", list(DW_CASES))
def test_dwconv_ln_windows(case):
    _dwconv_case(case)


def test_dwconv_ln_row_groups_windows():
    """the same through vrd_row_segs: two groups (1 and 2 sequences of 24 frames), stride 2, three sets, the input LayerNorm"""
    _dwconv_case("qkv_s2", segs=[(0, 1, 24), (24, 2, 24)])


@pytest.mark.parametrize("Cw", [256, 512])
def test_maxpool_mask_windows(Cw):
    from vrdone_amd import _hip, ops
    g = torch.Generator().manual_seed(Cw)
    B, T = 3, 16
    m = lens_mask(B, T, std_lens(T))
    x = torch.randn(B, T, Cw, generator=g) * m[..., None]
    want = F.max_pool1d(cl(x.double()), 3, 2, 1).transpose(1, 2) * m[:, ::2, None]
    lds = W.LdSeq()
    hx, hy = win(x, lds, "x"), out_win((B, T // 2, Cw), lds, "y")
    m_out = torch.full((B, T // 2 + 16,), 7, dtype=torch.uint8, device=DEV)        # mask bytes: B * T/2 written, the rest kept
    md = m.to(DEV)
    ok(_hip.lib.vrd_maxpool_mask(p(hx.view), hx.ld, B, T, Cw, p(md), p(hy.view), hy.ld, p(m_out), stream()), "vrd_maxpool_mask")
    plain, pm = ops.maxpool_mask(x.to(DEV), md)
    W.check([hy], [hx])
    close(hy.view, want, 0, "y")
    same_bits(hy, plain, "y")
    flat = m_out.view(-1)
    assert torch.equal(flat[:B * T // 2].view(B, T // 2).bool().cpu(), m[:, ::2]) and bool((flat[B * T // 2:] == 7).all())


def test_mask_head_windows():
    from vrdone_amd import _hip, ops
    g = torch.Generator().manual_seed(59)
    B, Q, T, Dp = 3, 9, 50, 256
    m = lens_mask(B, T, [T, T // 2, 3])
    emb, feat = torch.randn(B, Q, Dp, generator=g), torch.randn(B, T, Dp, generator=g) * m[..., None]
    want = torch.einsum("bqc,btc->bqt", emb.double(), feat.double()).masked_fill(~m[:, None], -10.0)
    lds = W.LdSeq()
    he, hf = win(emb, lds, "emb"), win(feat, lds, "feat")
    # seg is (B, Q, T) contiguous by contract: guard rows in front of and behind it
    hs = W.embed_out((B * Q, T), DEV, ld=T, c0=0, rows_before=8, rows_after=8, name="seg")
    md = m.to(DEV)
    ok(_hip.lib.vrd_mask_head(p(he.view), he.ld, p(hf.view), hf.ld, p(md), B, Q, T, Dp, -10.0, p(hs.view), stream()), "vrd_mask_head")
    # ... and through the wrapper, which hands the views' strides on
    got = ops.mask_head(he.view, hf.view, md)
    plain = ops.mask_head(emb.to(DEV), feat.to(DEV), md)
    W.check([hs], [he, hf])
    close(hs.view.view(B, Q, T), want, 5e-5, "seg")
    same_bits(hs, plain.view(B * Q, T), "seg")
    assert W.bits_equal(got, plain)


# ---------------------------------------------------------------------------------------------------- attention, forward
LOCAL_CASES = [(512, 8, 4), (512, 4, 9), (256, 8, 1)]          # (C, heads, half_win): windows 9, 19, 3 -- one case per strip kernel form


def _local_inputs(Cw, H, hw, rel):
    g = torch.Generator().manual_seed(Cw + 10 * H + hw + int(rel))
    B, T = 3, 24
    m = lens_mask(B, T, std_lens(T))
    q, k, v, dO = (torch.randn(B, T, Cw, generator=g) * m[..., None] for _ in range(4))
    rel_pe = torch.randn(1, 1, H, 2 * hw + 1, generator=g) if rel else None
    return B, T, m, q, k, v, dO, rel_pe


@pytest.mark.parametrize("rel", [False, True])
@pytest.mark.parametrize("Cw,H,hw", LOCAL_CASES)
def test_local_attention_windows(Cw, H, hw, rel):
    from vrdone_amd import _hip, ops
    B, T, m, q, k, v, _, rel_pe = _local_inputs(Cw, H, hw, rel)
    want = cl(O.banded_attention(cl(q.double()), cl(k.double()), cl(v.double()), m[:, None], H, hw,
                                 rel_pe=None if rel_pe is None else rel_pe.double()))
    md, rd = m.to(DEV), None if rel_pe is None else rel_pe.to(DEV)
    plain = ops.local_attention(q.to(DEV), k.to(DEV), v.to(DEV), md, H, hw, rel_pe=rd)
    for segs in (None, [(0, 1, T), (T, 2, T)]):
        lds = W.LdSeq()
        hqkv, (qv, kv, vv) = slabs([q, k, v], lds, "qkv")
        ho = out_win((B, T, Cw), lds, "out")
        assert hqkv.ld != 3 * Cw and ho.ld not in (Cw, hqkv.ld)
        if segs is None:
            ok(_hip.lib.vrd_local_attn(p(qv), p(kv), p(vv), hqkv.ld, p(md), p(rd), B, T, Cw, H, hw, p(ho.view), ho.ld, 0, stream()),
               "vrd_local_attn")
        else:
            table = _hip.RowSegs.of(segs)
            ok(_hip.lib.vrd_local_attn_segs(p(qv), p(kv), p(vv), hqkv.ld, p(md), p(rd), C.byref(table), Cw, H, hw, p(ho.view), ho.ld, 0,
                                            stream()), "vrd_local_attn_segs")
        W.check([ho], [hqkv])
        close(ho.view, want, 2e-5, "out")
        same_bits(ho, plain, "out (row groups)" if segs else "out")


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("H,hd,Tq,Tk", [(4, 128, 40, 77), (4, 64, 9, 36)])
def test_global_attention_windows(algo, H, hd, Tq, Tk):
    from vrdone_amd import _hip, ops
    g = torch.Generator().manual_seed(H + hd + Tq + Tk)
    B, Cw = 3, H * hd
    km = lens_mask(B, Tk, [Tk, max(1, Tk // 3), 1])
    q = torch.randn(B, Tq, Cw, generator=g) * 2.0
    k, v = (torch.randn(B, Tk, Cw, generator=g) * km[..., None] for _ in range(2))
    want = cl(O.full_attention(cl(q.double()), cl(k.double()), cl(v.double()), km[:, None], H))
    lds = W.LdSeq()
    hq = win(q, lds, "q")
    hkv, (kv, vv) = slabs([k, v], lds, "kv")
    ho = out_win((B, Tq, Cw), lds, "out")
    assert len({hq.ld, hkv.ld, ho.ld}) == 3
    kd = km.to(DEV)
    ok(_hip.lib.vrd_attention(p(hq.view), hq.ld, p(kv), p(vv), hkv.ld, p(kd), B, Tq, Tk, H, hd, p(ho.view), ho.ld, algo, 0, stream()),
       "vrd_attention")
    plain = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), kd, H, algo=algo)
    W.check([ho], [hq, hkv])
    close(ho.view, want, 3e-5, "out")
    same_bits(ho, plain, "out")


def _to_pair(t, fmt):
    """f32 (B, T, C) -> pair rows (tests/test_gpu_ops.py _to_pair; mirrors vrd::store_pair4)"""
    from vrdone_amd import _hip
    f16 = fmt == _hip.PAIR_F16
    dt = torch.float16 if f16 else torch.bfloat16
    t = t * 2.0 ** _hip.F16_ACT_EXP if f16 else t
    hi = t.to(dt)
    lo = (t - hi.float()).to(dt)
    Cw = t.shape[-1]
    raw = torch.stack([hi.reshape(*t.shape[:-1], Cw // 32, 32), lo.reshape(*t.shape[:-1], Cw // 32, 32)], dim=-2)
    return raw.reshape(*t.shape[:-1], 2 * Cw).contiguous().view(torch.float32)


@pytest.mark.parametrize("w64", ["0", "1"])
@pytest.mark.parametrize("mode", SPLIT)
def test_attention_pair_windows(mode, w64, monkeypatch):
    """both flash kernels on pair rows; q_mask leaves the second query tile of two sequences out (those rows read 0 and the guards
    next to them stay whole)"""
    from vrdone_amd import _hip, ops
    monkeypatch.setenv("VRD_FLASH_W64", w64)
    with ops.use_precision(mode):
        fmt = ops.pair_fmt()
        g = torch.Generator().manual_seed(189)
        B, H, hd, Tq, Tk = 3, 8, 64, 40, 77
        Cw = H * hd
        km = lens_mask(B, Tk, [Tk, Tk // 3, 1])
        q = torch.randn(B, Tq, Cw, generator=g) * 2.0
        k, v = (torch.randn(B, Tk, Cw, generator=g) * km[..., None] for _ in range(2))
        k[:, 70, :hd] = q[:, 5, :hd] * 2.0 * km[:, 70, None]            # a dominant late key: the running-max rescale
        want = cl(O.full_attention(cl(q.double()), cl(k.double()), cl(v.double()), km[:, None], H))
        qp, kp, vp = (_to_pair(t.to(DEV), fmt) for t in (q, k, v))
        qm = lens_mask(B, Tq, [Tq, 20, 1])
        live = F.pad(qm, (0, (-Tq) % 32)).reshape(B, -1, 32).any(-1).repeat_interleave(32, dim=1)[:, :Tq]
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
                close(ho.view, want, 2e-4, "out")                        # test_flash_attention_pair_rows' bound
            else:
                close(ho.view[live.to(DEV)], want[live], 2e-4, "out (live query tiles)")
                assert bool((ho.view[~live.to(DEV)] == 0).all())


# ------------------------------------------------------------------------------------------------------------------- GEMM
def _gemm_case(B, T, Cin, N, k, pair_in, sample, expect_family):
    """ops.conv_gemm with input, out=, res and res2 slabs, each at its own leading dimension; plain, and mask * scale + two
    residuals.  Reference: float64 on the sequences `sample`."""
    from vrdone_amd import _hip, ops
    g = torch.Generator(device=DEV).manual_seed(B * 7 + N + k)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)     # noqa: E731
    mask = torch.rand(B, T, generator=g, device=DEV) > 0.2
    mask[B - 1, 2:] = False
    x = rn(B, T, Cin) * mask[..., None]
    w = rn(N, Cin, k) / (Cin * k) ** 0.5
    bias, scale = rn(N), torch.rand(N, generator=g, device=DEV) + 0.5
    res, res2 = rn(B, T, N), rn(B, T, N)
    fmt = ops.pair_fmt()
    xin = _to_pair(x, fmt) if pair_in else x
    wrap = (lambda t: ops.Pair(t, Cin, fmt)) if pair_in else (lambda t: t)
    xs = x[sample].double().cpu().transpose(1, 2)
    y = F.conv1d(xs, w.double().cpu(), bias.double().cpu(), padding=k // 2).transpose(1, 2)
    mk = mask[sample].double().cpu()[..., None]
    scale_tol = 5.0 if ops.get_precision() == "bf16x3" else 1.0          # tests/test_gpu_ops.py GEMM_TOL_SCALE
    for full in (False, True):
        lds = W.LdSeq()
        hx, ho = win(xin, lds, "x"), out_win((B, T, N), lds, "out")
        ins = [hx]
        kw, kw_plain = {}, {}
        want = y
        if full:
            hr, hr2 = win(res, lds, "res"), win(res2, lds, "res2")
            ins += [hr, hr2]
            assert len({hx.ld - Cin, ho.ld - N, hr.ld - N, hr2.ld - N}) == 4
            kw = dict(row_mask=mask, scale=scale, res=hr.view, res_masked=True, res2=hr2.view)
            kw_plain = dict(kw, res=res, res2=res2)
            want = y * mk * scale.double().cpu() + res[sample].double().cpu() * mk + res2[sample].double().cpu()
        a, _ = ops.gemm_args(wrap(hx.view), w, bias, out=ho.view, **kw)
        family = [ops.gemm_family(a)]
        ops.launch_gemm(a)
        assert family[0] == expect_family, f"the call ran kernel family {family[0]}, the case is built for {expect_family}"
        plain = ops.conv_gemm(wrap(xin), w, bias, **kw_plain)
        W.check([ho], ins)
        same_bits(ho, plain, "out")
        close(ho.view[sample], want, (2e-5 if pair_in else 3e-5) * scale_tol, "out")     # test_gemm_large_tile_kernels / test_gemm_shapes_and_epilogue


@pytest.mark.parametrize("k", [1, 3])
def test_gemm_small_tile_windows(k, precision):
    """M = 120 rows, N = 133, Cin = 64: ragged in M and N for the exact-f32 kernel (f32 mode) and the 128 x 128 split kernel"""
    from vrdone_amd import _hip
    _gemm_case(3, 40, 64, 133, k, False, [0, 1, 2], _hip.K_GEMM if precision == "f32" else _hip.K_GEMM_X3)


def test_gemm_few_channels_windows(precision):
    """K = 15 (the pair box embedding): scalar A loads, rows that are not 16-byte aligned, the exact-f32 kernel in every mode"""
    from vrdone_amd import _hip
    _gemm_case(3, 40, 5, 256, 3, False, [0, 1, 2], _hip.K_GEMM)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("body", ["big", "dma"])
@pytest.mark.parametrize("mode", SPLIT)          # (the LDS-DMA kernels are split-precision kernels)
def test_gemm_large_tile_windows(mode, body, k):
    """The LDS-DMA kernels need two rounds of their tiles, as in test_gemm_large_tile_kernels: the smallest such launches with a
    ragged last tile in M and N.  256 x 256 body: 65,600 rows (a 64-row last tile) x 320 columns = 514 tiles; 128 x 256 body:
    65,300 rows (M % 64 != 0 keeps the 256 x 256 kernel out) x 300 columns."""
    from vrdone_amd import _hip, ops
    with ops.use_precision(mode):
        if body == "big":
            _gemm_case(1025, 64, 128, 320, k, True, [0, 1, 512, 1023, 1024], _hip.K_GEMM_X3_BIG)
        else:
            _gemm_case(653, 100, 128, 300, k, True, [0, 1, 326, 651, 652], _hip.K_GEMM_X3_DMA)


# --------------------------------------------------------------------------------------------------------------- backward
def _det_pair(run):
    """run(flags) -> list of accumulated sums.  Returns (default-mode results, deterministic-mode results)."""
    from vrdone_amd import _hip
    return run(0), run(_hip.DETERMINISTIC)


@pytest.mark.parametrize("Cw,relu", [(512, False), (256, True)])
def test_layernorm_bwd_windows(Cw, relu):
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(Cw + relu)
    B, T = 3, 24
    m = lens_mask(B, T, std_lens(T))
    x = (torch.randn(B, T, Cw, generator=g) * 2 + 0.3) * m[..., None]
    dy = torch.randn(B, T, Cw, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(Cw, generator=g), 0.1 * torch.randn(Cw, generator=g)
    with torch.enable_grad():
        xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        yr = cl(O.channel_ln(cl(xr), gr.view(1, Cw, 1), br.view(1, Cw, 1)))
        (torch.relu(yr) if relu else yr).backward(dy.double())
    gd, bd, sc = gamma.to(DEV), beta.to(DEV), scratch_buf()

    def call(xv, dyv, dxv, flags):
        dg, db = torch.zeros(Cw, device=DEV), torch.zeros(Cw, device=DEV)
        ok(_hip.lib.vrd_layernorm_bwd(p(xv), ld_of(xv), p(dyv), ld_of(dyv), B * T, Cw, p(gd), p(bd), int(relu), p(dxv), ld_of(dxv), p(dg), p(db),
                                      p(sc), sc.numel(), stream(), flags), "vrd_layernorm_bwd")
        return dg, db

    for flags in (0, _hip.DETERMINISTIC):
        lds = W.LdSeq()
        hx, hdy, hdx = win(x, lds, "x"), win(dy, lds, "dy"), out_win((B, T, Cw), lds, "dx")
        assert len({hx.ld, hdy.ld, hdx.ld}) == 3
        dg, db = call(hx.view, hdy.view, hdx.view, flags)
        pdx = torch.empty(B, T, Cw, device=DEV)
        pdg, pdb = call(x.to(DEV), dy.to(DEV), pdx, flags)
        W.check([hdx], [hx, hdy])
        rel_close(hdx.view, xr.grad, 2e-5, "dx")
        same_bits(hdx, pdx, "dx")
        rel_close(dg, gr.grad, 2e-5, "dgamma")
        rel_close(db, br.grad, 2e-5, "dbeta")
        if flags:
            assert W.bits_equal(dg, pdg) and W.bits_equal(db, pdb), "deterministic dgamma / dbeta depend on the leading dimensions"


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_activation_windows(act, grad):
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(len(act) + grad)
    B, T, Cw = 3, 24, 260                                            # (C % 4 == 0 is all the kernel asks)
    m = lens_mask(B, T, std_lens(T))
    x = torch.randn(B, T, Cw, generator=g) * 2 * m[..., None]
    dy = torch.randn(B, T, Cw, generator=g) if grad else None
    fn = torch.relu if act == "relu" else F.gelu
    with torch.enable_grad():
        xr = x.double().requires_grad_(True)
        yr = fn(xr)
        if grad:
            yr.backward(dy.double())
    want = xr.grad if grad else yr.detach()
    code = _hip.ACT_RELU if act == "relu" else _hip.ACT_GELU
    lds = W.LdSeq()
    hx, ho = win(x, lds, "x"), out_win((B, T, Cw), lds, "out")
    hd = win(dy, lds, "dy") if grad else None
    ok(_hip.lib.vrd_activation(p(hx.view), hx.ld, p(hd.view) if grad else None, hd.ld if grad else 0, B * T, Cw, code, p(ho.view), ho.ld,
                               stream()), "vrd_activation")
    xd, dyd, plain = x.to(DEV), dy.to(DEV) if grad else None, torch.empty(B, T, Cw, device=DEV)
    ok(_hip.lib.vrd_activation(p(xd), Cw, p(dyd), Cw if grad else 0, B * T, Cw, code, p(plain), Cw, stream()), "vrd_activation")
    W.check([ho], [hx] + ([hd] if grad else []))
    rel_close(ho.view, want, 2e-5, "out")
    same_bits(ho, plain, "out")


def test_rowcol_scale_windows():
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(17)
    B, T, Cw = 3, 24, 260
    m = lens_mask(B, T, std_lens(T))
    v, res, res2 = (torch.randn(B, T, Cw, generator=g) for _ in range(3))
    cs, rs = torch.rand(Cw, generator=g) + 0.5, torch.rand(B * T, generator=g) * 1.5
    mf = m.double()[..., None]
    want = v.double() * cs.double() * rs.double().view(B, T, 1) * mf + res.double() * mf + res2.double()
    csd, rsd, md = cs.to(DEV), rs.to(DEV), m.to(DEV)
    lds = W.LdSeq()
    hv, hr, hr2, ho = win(v, lds, "v"), win(res, lds, "res"), win(res2, lds, "res2"), out_win((B, T, Cw), lds, "out")
    assert len({hv.ld, hr.ld, hr2.ld, ho.ld}) == 4
    ok(_hip.lib.vrd_rowcol_scale(p(hv.view), hv.ld, B * T, Cw, p(csd), p(rsd), p(md), p(hr.view), hr.ld, 1, p(hr2.view), hr2.ld, p(ho.view), ho.ld,
                                 stream()), "vrd_rowcol_scale")
    vd, rd, r2d, plain = v.to(DEV), res.to(DEV), res2.to(DEV), torch.empty(B, T, Cw, device=DEV)
    ok(_hip.lib.vrd_rowcol_scale(p(vd), Cw, B * T, Cw, p(csd), p(rsd), p(md), p(rd), Cw, 1, p(r2d), Cw, p(plain), Cw, stream()), "vrd_rowcol_scale")
    W.check([ho], [hv, hr, hr2])
    rel_close(ho.view, want, 2e-5, "out")
    same_bits(ho, plain, "out")


@pytest.mark.parametrize("stride,gin,n_out,up", [(1, 1, 3, False), (2, 1, 3, False), (1, 2, 1, False), (1, 1, 1, True)])
def test_dwconv_backward_windows(stride, gin, n_out, up):
    """vrd_dwconv_bwd (the float4 form, the element form at stride 2 / two inputs per group / with dx_up) and vrd_dwconv_wgrad"""
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(stride * 10 + gin + n_out + up)
    B, T, k = 3, 24, 3
    Cw = 256 if gin == 2 or up else 512
    Cin, To = Cw * gin, T // stride
    m_in = lens_mask(B, T, std_lens(T))
    m_out = m_in[:, ::stride].contiguous()
    x = torch.randn(B, T, Cin, generator=g) * m_in[..., None]
    ws = [torch.randn(Cw, gin, k, generator=g) / (gin * k) ** 0.5 for _ in range(n_out)]
    dDs = [torch.randn(B, To, Cw, generator=g) for _ in range(n_out)]
    with torch.enable_grad():
        xr = cl(x.double()).requires_grad_(True)
        ur = torch.zeros(B, Cin, T // 2, dtype=torch.float64, requires_grad=True) if up else None
        wr = [w.double().requires_grad_(True) for w in ws]
        br = [torch.zeros(Cw, dtype=torch.float64, requires_grad=True) for _ in ws]
        xin = xr + ur.repeat_interleave(2, dim=2) if up else xr
        loss = sum((O.masked_conv1d(xin, m_in[:, None], wr[i], br[i], stride=stride, groups=Cw)[0] * cl(dDs[i].double())).sum()
                   for i in range(n_out))
        loss.backward()
    md, wd = m_out.to(DEV), [w.to(DEV) for w in ws]

    def bwd(dD_views, dx_view, dxu_view):
        a = _hip.DwconvBwdArgs()
        for i, d in enumerate(dD_views):
            a.dD[i], a.lddd[i], a.w[i] = p(d), ld_of(d), p(wd[i])
        a.n_out, a.B, a.Tin, a.C, a.ksize, a.stride, a.group_in = n_out, B, T, Cw, k, stride, gin
        a.mask_out, a.dx, a.lddx = p(md), p(dx_view), ld_of(dx_view)
        if dxu_view is not None:
            a.dx_up, a.lddx_up = p(dxu_view), ld_of(dxu_view)
        ok(_hip.lib.vrd_dwconv_bwd(C.byref(a), stream()), "vrd_dwconv_bwd")

    lds = W.LdSeq()
    hds = [win(d, lds, f"dD{i}") for i, d in enumerate(dDs)]
    hdx = out_win((B, T, Cin), lds, "dx")
    hdu = out_win((B, T // 2, Cin), lds, "dx_up") if up else None
    hx = win(x, lds, "x")
    assert len({h.ld - h.cols for h in hds + [hdx, hx] + ([hdu] if up else [])}) == n_out + 2 + bool(up)
    bwd([h.view for h in hds], hdx.view, hdu.view if up else None)
    pdx = torch.empty(B, T, Cin, device=DEV)
    pdu = torch.empty(B, T // 2, Cin, device=DEV) if up else None
    bwd([d.to(DEV) for d in dDs], pdx, pdu)
    W.check([hdx] + ([hdu] if up else []), hds)
    rel_close(hdx.view, cl(xr.grad), 2e-5, "dx")
    same_bits(hdx, pdx, "dx")
    if up:
        rel_close(hdu.view, cl(ur.grad), 2e-5, "dx_up")
        same_bits(hdu, pdu, "dx_up")
    # weight and bias gradient of set 0, dD and x at their own leading dimensions
    sc = scratch_buf()

    def wgrad(dv, xv, flags):
        dw, db = torch.zeros(Cw, gin, k, device=DEV), torch.zeros(Cw, device=DEV)
        ok(_hip.lib.vrd_dwconv_wgrad(p(dv), ld_of(dv), p(xv), ld_of(xv), k, stride, gin, To, p(md), B * To, Cw, p(dw), p(db), p(sc), sc.numel(),
                                     stream(), flags), "vrd_dwconv_wgrad")
        return dw, db

    for flags in (0, _hip.DETERMINISTIC):
        dw, db = wgrad(hds[0].view, hx.view, flags)
        pdw, pdb = wgrad(dDs[0].to(DEV), x.to(DEV), flags)
        rel_close(dw, wr[0].grad, 2e-5, "dw")
        rel_close(db, br[0].grad, 2e-5, "dbias")
        if flags:
            assert W.bits_equal(dw, pdw) and W.bits_equal(db, pdb), "deterministic dw / dbias depend on the leading dimensions"
    W.check([], hds + [hx])


@pytest.mark.parametrize("rel", [False, True])
@pytest.mark.parametrize("Cw,H,hw", LOCAL_CASES)
def test_local_attention_bwd_windows(Cw, H, hw, rel):
    from vrdone_amd import _hip
    B, T, m, q, k, v, dO, rel_pe = _local_inputs(Cw, H, hw, rel)
    Wn = 2 * hw + 1
    with torch.enable_grad():
        qr, kr, vr = (cl(t.double()).requires_grad_(True) for t in (q, k, v))
        relr = rel_pe.double().requires_grad_(True) if rel else None
        O.banded_attention(qr, kr, vr, m[:, None], H, hw, rel_pe=relr).backward(cl(dO.double()))
    md, rd = m.to(DEV), rel_pe.to(DEV) if rel else None

    def call(qv, kv, vv, dOv, dqv, dkv, dvv):
        scratch = torch.full((2 * B * T * H * Wn,), float("nan"), device=DEV)
        ok(_hip.lib.vrd_local_attn_bwd(p(qv), p(kv), p(vv), ld_of(qv), p(dOv), ld_of(dOv), p(md), p(rd), B, T, Cw, H, hw, p(dqv), p(dkv), p(dvv),
                                       ld_of(dqv), p(scratch), stream()), "vrd_local_attn_bwd")
        return scratch[B * T * H * Wn:].view(B * T, H, Wn)

    lds = W.LdSeq()
    hqkv, (qv, kv, vv) = slabs([q, k, v], lds, "qkv")
    hdo = win(dO, lds, "dO")
    hg, (dqv, dkv, dvv) = out_slabs((B, T, Cw), 3, lds, "dq|dk|dv")
    assert len({hqkv.ld, hdo.ld, hg.ld}) == 3 and hdo.ld != Cw and hg.ld != 3 * Cw
    dS = call(qv, kv, vv, hdo.view, dqv, dkv, dvv)
    plain = [torch.empty(B, T, Cw, device=DEV) for _ in range(3)]
    pdS = call(q.to(DEV), k.to(DEV), v.to(DEV), dO.to(DEV), *plain)
    W.check([hg], [hqkv, hdo])
    for name, got, ref, pl in (("dq", dqv, qr.grad, plain[0]), ("dk", dkv, kr.grad, plain[1]), ("dv", dvv, vr.grad, plain[2])):
        rel_close(got, cl(ref), 2e-5, name)
        assert W.bits_equal(got, pl), name
    assert W.bits_equal(dS, pdS)
    if rel:
        rel_close(dS.sum(0).view(1, 1, H, Wn), relr.grad, 2e-5, "d rel_pe")


@pytest.mark.parametrize("fmt_name", ["bf16", "f16"])
def test_attention_rows_and_bwd_windows(fmt_name):
    """vrd_attention_rows + vrd_attention_bwd (head_dim 64, Tq 40, Tk 77): q / dq at ldq, k | v and dk | dv at ldkv, out / dO at ldo"""
    from vrdone_amd import _hip
    fmt = _hip.PAIR_F16 if fmt_name == "f16" else _hip.PAIR_BF16
    tol = 2e-5 if fmt_name == "f16" else 1e-4                         # test_global_attention_backward_fused
    g = torch.Generator().manual_seed(40 * 7 + 77)
    B, H, hd, Tq, Tk = 3, 8, 64, 40, 77
    Cw = H * hd
    km = lens_mask(B, Tk, [Tk, Tk // 2 + 3, 2])
    q, dO = torch.randn(B, Tq, Cw, generator=g), torch.randn(B, Tq, Cw, generator=g)
    k, v = (torch.randn(B, Tk, Cw, generator=g) * km[..., None] for _ in range(2))
    with torch.enable_grad():
        qr, kr, vr = (cl(t.double()).requires_grad_(True) for t in (q, k, v))
        outr = O.full_attention(qr, kr, vr, km[:, None], H)
        outr.backward(cl(dO.double()))
    kd = km.to(DEV)

    def scales(dOv, vv):
        if fmt != _hip.PAIR_F16:
            return None, None
        so, sv = (torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV) for _ in range(2))
        ok(_hip.lib.vrd_absmax_scale(p(dOv), ld_of(dOv), B * Tq, Cw, p(so), stream()), "vrd_absmax_scale")
        ok(_hip.lib.vrd_absmax_scale(p(vv), ld_of(vv), B * Tk, Cw, p(sv), stream()), "vrd_absmax_scale")
        return so, sv

    def call(qv, kv, vv, ov, dOv, dqv, dkv, dvv):
        lse = torch.full((B, H, Tq), float("nan"), device=DEV)
        ok(_hip.lib.vrd_attention_rows(p(qv), ld_of(qv), p(kv), p(vv), ld_of(kv), p(kd), B, Tq, Tk, H, hd, fmt, p(ov), ld_of(ov), p(lse), stream()),
           "vrd_attention_rows")
        so, sv = scales(dOv, vv)
        scratch = torch.full((2 * B * H * Tq,), float("nan"), device=DEV)
        ok(_hip.lib.vrd_attention_bwd(p(qv), ld_of(qv), p(kv), p(vv), ld_of(kv), p(ov), p(dOv), ld_of(ov), p(kd), B, Tq, Tk, H, hd, p(dqv), p(dkv),
                                      p(dvv), p(lse), p(scratch), p(so), p(sv), stream()), "vrd_attention_bwd")
        return lse

    ldq, ldkv, ldo = Cw + 64, 2 * Cw + 96, Cw + 128
    hq, hdq = W.embed(q.to(DEV), ld=ldq, name="q"), W.embed_out((B, Tq, Cw), DEV, ld=ldq, name="dq")
    hkv = W.embed(torch.cat([k, v], -1).to(DEV), ld=ldkv, name="k|v")
    hdkv = W.embed_out((B, Tk, 2 * Cw), DEV, ld=ldkv, name="dk|dv")
    ho, hdo = W.embed_out((B, Tq, Cw), DEV, ld=ldo, name="out"), W.embed(dO.to(DEV), ld=ldo, name="dO")
    kv, vv = hkv.view[..., :Cw], hkv.view[..., Cw:]
    dkv, dvv = hdkv.view[..., :Cw], hdkv.view[..., Cw:]
    lse = call(hq.view, kv, vv, ho.view, hdo.view, hdq.view, dkv, dvv)
    plain = [torch.empty(B, t, Cw, device=DEV) for t in (Tq, Tq, Tk, Tk)]               # out, dq, dk, dv
    plse = call(q.to(DEV), k.to(DEV), v.to(DEV), plain[0], dO.to(DEV), plain[1], plain[2], plain[3])
    W.check([ho, hdq, hdkv], [hq, hkv, hdo])
    rel_close(ho.view, cl(outr), tol, "out")
    for name, got, ref, pl in (("out", ho.view, None, plain[0]), ("dq", hdq.view, qr.grad, plain[1]), ("dk", dkv, kr.grad, plain[2]),
                               ("dv", dvv, vr.grad, plain[3])):
        if ref is not None:
            rel_close(got, cl(ref), tol, name)
        assert W.bits_equal(got, pl), name
    assert W.bits_equal(lse, plse) and bool(torch.isfinite(lse).all())


def test_attn_bwd_probs_windows():
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(9 + 36)
    B, H, hd, Tq, Tk = 3, 4, 64, 9, 36
    Cw = H * hd
    km = lens_mask(B, Tk, [Tk, Tk // 2, 2])
    q, dO = torch.randn(B, Tq, Cw, generator=g), torch.randn(B, Tq, Cw, generator=g)
    k, v = (torch.randn(B, Tk, Cw, generator=g) * km[..., None] for _ in range(2))
    heads = lambda t: t.double().view(B, -1, H, hd).transpose(1, 2)          # noqa: E731  (B, H, T, hd)
    s = (heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(hd)).masked_fill(~km[:, None, None, :], float("-inf"))
    P = torch.softmax(s, -1)
    dP = heads(dO) @ heads(v).transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    kd = km.to(DEV)

    def call(qv, kv, vv, dOv, Pv, dSv):
        ok(_hip.lib.vrd_attn_bwd_probs(p(qv), ld_of(qv), p(kv), p(vv), ld_of(kv), p(dOv), ld_of(dOv), p(kd), B, Tq, Tk, H, hd, p(Pv), p(dSv), stream()),
           "vrd_attn_bwd_probs")

    lds = W.LdSeq()
    hq, hdo = win(q, lds, "q"), win(dO, lds, "dO")
    hkv, (kv, vv) = slabs([k, v], lds, "k|v")
    assert len({hq.ld, hdo.ld, hkv.ld - Cw}) == 3
    # P and dS are (B, n_head, Tq, Tk) contiguous by contract: guard rows in front and behind
    hP, hS = (W.embed_out((B * H * Tq, Tk), DEV, ld=Tk, c0=0, rows_before=4, rows_after=4, name=n) for n in ("P", "dS"))
    call(hq.view, kv, vv, hdo.view, hP.view, hS.view)
    pP, pS = (torch.empty(B * H * Tq, Tk, device=DEV) for _ in range(2))
    call(q.to(DEV), k.to(DEV), v.to(DEV), dO.to(DEV), pP, pS)
    W.check([hP, hS], [hq, hdo, hkv])
    rel_close(hP.view, P.reshape(-1, Tk), 2e-5, "P")
    rel_close(hS.view, dS.reshape(-1, Tk), 2e-5, "dS")
    same_bits(hP, pP, "P")
    same_bits(hS, pS, "dS")


def _maxpool_bwd(x, dy, m):
    """(window handles, contiguous result, float64 autograd of max_pool1d * mask)"""
    from vrdone_amd import _hip
    B, T, Cw = x.shape
    with torch.enable_grad():
        xr = cl(x.double()).requires_grad_(True)
        (F.max_pool1d(xr, 3, 2, 1) * m[:, None, ::2].double()).backward(cl(dy.double()))
    md = m.to(DEV)
    lds = W.LdSeq()
    hx, hdy, hdx = win(x, lds, "x"), win(dy, lds, "dy"), out_win((B, T, Cw), lds, "dx")
    assert len({hx.ld, hdy.ld, hdx.ld}) == 3
    ok(_hip.lib.vrd_maxpool_bwd(p(hx.view), hx.ld, p(hdy.view), hdy.ld, B, T, Cw, p(md), p(hdx.view), hdx.ld, stream()), "vrd_maxpool_bwd")
    plain = torch.empty(B, T, Cw, device=DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    ok(_hip.lib.vrd_maxpool_bwd(p(xd), Cw, p(dyd), Cw, B, T, Cw, p(md), p(plain), Cw, stream()), "vrd_maxpool_bwd")
    W.check([hdx], [hx, hdy])
    same_bits(hdx, plain, "dx")
    return hdx, cl(xr.grad)


def test_maxpool_bwd_windows():
    g = torch.Generator().manual_seed(3)
    B, T, Cw = 3, 16, 260
    m = lens_mask(B, T, std_lens(T))
    x = torch.randn(B, T, Cw, generator=g) * m[..., None]
    hdx, want = _maxpool_bwd(x, torch.randn(B, T // 2, Cw, generator=g), m)
    rel_close(hdx.view, want, 1e-6, "dx")


def test_maxpool_bwd_ties_go_to_the_first_maximum():
    """Inputs rounded to halves in [-1, 1]: most windows of three hold a tie, and the gradient must go to the FIRST maximum
    (ATen's rule; tests/test_window_cases_cpu.py shows it on the CPU).  Lengths 9, 5 and 2 end on valid last rows whose value is
    forced to 0.0 in half of the channels: a tie between the last valid row and the zero padded row behind it, in windows
    whose centre (an even frame) is valid (length 9: frame 8 is the centre of window (7, 8, 9)) and in masked windows."""
    g = torch.Generator().manual_seed(11)
    B, T, Cw = 3, 16, 256
    lens = [9, 5, 2]
    m = lens_mask(B, T, lens)
    x = (torch.randn(B, T, Cw, generator=g).clamp(-1, 1) * 2).round() / 2 * m[..., None]
    for b, n in enumerate(lens):
        x[b, n - 1, ::2] = 0.0
    # ties are the rule, not the exception
    win3 = F.pad(cl(x), (1, 1), value=float("-inf")).unfold(2, 3, 2)
    assert float(((win3 == win3.max(-1, keepdim=True).values).sum(-1) > 1).float().mean()) > 0.5
    hdx, want = _maxpool_bwd(x, torch.randn(B, T // 2, Cw, generator=g), m)
    rel_close(hdx.view, want, 1e-6, "dx")                              # test_maxpool_and_mask_head_backward's bound


@pytest.mark.parametrize("x3", [False, True])
def test_gemm_wgrad_windows(x3):
    """vrd_gemm_wgrad (exact f32) and vrd_gemm_wgrad_x3 (bf16 planes; with dbias): M = 120, N = 96, Cin = 40, k = 3, T = 40"""
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(120 + 96 + x3)
    B, T, N, Cin, k = 3, 40, 96, 40, 3
    M = B * T
    m = lens_mask(B, T, std_lens(T))
    G = torch.randn(B, T, N, generator=g)
    X = torch.randn(B, T, Cin, generator=g) * m[..., None]
    Gm = (G * m[..., None]).double().reshape(M, N)
    taps = [F.pad(X.double(), (0, 0, 1, 1))[:, t:t + T].reshape(M, Cin) for t in range(3)]
    want = torch.cat([Gm.t() @ xt for xt in taps], 1)
    md, sc = m.to(DEV), scratch_buf()

    def call(Gv, Xv, flags):
        dW, db = torch.zeros(N, k * Cin, device=DEV), torch.zeros(N, device=DEV)
        if x3:
            ok(_hip.lib.vrd_gemm_wgrad_x3(p(Gv), ld_of(Gv), p(Xv), ld_of(Xv), p(md), M, N, Cin, k, T, p(dW), p(db), p(sc), sc.numel(), None, stream(),
                                          flags), "vrd_gemm_wgrad_x3")
        else:
            ok(_hip.lib.vrd_gemm_wgrad(p(Gv), ld_of(Gv), p(Xv), ld_of(Xv), p(md), M, N, Cin, k, T, p(dW), p(sc), sc.numel(), stream(), flags),
               "vrd_gemm_wgrad")
        return dW, db

    lds = W.LdSeq()
    hG, hX = win(G, lds, "G"), win(X, lds, "X")
    assert hG.ld - N != hX.ld - Cin and hG.ld != N and hX.ld != Cin
    for flags in (0, _hip.DETERMINISTIC):
        dW, db = call(hG.view, hX.view, flags)
        pdW, pdb = call(G.to(DEV), X.to(DEV), flags)
        rel_close(dW, want, 2e-4 if x3 else 2e-5, "dW")                 # test_weight_gradient_through_partial_tiles / test_linear_backward
        if x3:
            rel_close(db, Gm.sum(0), 2e-5, "dbias")
        if flags:
            assert W.bits_equal(dW, pdW) and W.bits_equal(db, pdb), "deterministic dW / dbias depend on the leading dimensions"
    W.check([], [hG, hX])


# -------------------------------------------------------------------------------------------------------------------- bmm
def _bmm_operand(Z0, Z1, rows, cols, odd, transposed, g):
    """values (Z0, Z1, rows, cols), the device tensor holding them and its (z0, z1, row, col) strides in floats: padded in every
    dimension (distinct z strides); odd: a row pitch of 77 floats, else every stride a multiple of 4; transposed: stored
    (cols, rows), i.e. the row index has stride 1."""
    val = torch.randn(Z0, Z1, rows, cols, generator=g)
    r, c = (cols, rows) if transposed else (rows, cols)
    pitch = 77 if odd else (c + 3) // 4 * 4 + 4
    store = torch.zeros(Z0, Z1 + 1, r + (0 if odd else 4 - r % 4), pitch)
    store[:, :Z1, :r, :c] = val.transpose(2, 3) if transposed else val
    d = store.to(DEV)
    s = d.stride()
    return val, d, (s[0], s[1], s[3], s[2]) if transposed else (s[0], s[1], s[2], s[3])


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("layout", ["row_major_vec", "transposed_vec", "row_major_odd", "transposed_odd"])
def test_bmm_windows(layout, accumulate):
    """vrd_bmm through autograd.bmm against a float64 einsum: M, N in {31, 33, 65} and K in {15, 17, 40} straddle the
    32 x 32 x 16 threshold between the one-thread-per-output kernel and the matrix-core tiles, and the 64-tile edge; both
    branches of the float4 test (every stride % 4 == 0 / a pitch of 77); row-major and transposed A and B; Z0 x Z1 = 3 x 4 with
    distinct z strides; alpha != 1; C embedded with guards (with accumulate the window starts from finite values)."""
    from vrdone_amd import autograd
    g = torch.Generator().manual_seed(len(layout) + accumulate)
    Z0, Z1, alpha = 3, 4, 0.125 * 3
    transposed, odd = layout.startswith("transposed"), layout.endswith("odd")
    for M, N, K in itertools.product((31, 33, 65), (31, 33, 65), (15, 17, 40)):
        A, Ad, sa = _bmm_operand(Z0, Z1, M, K, odd, transposed, g)
        Bv, Bd, sb = _bmm_operand(Z0, Z1, K, N, odd, transposed, g)
        if not odd:
            assert all(s % 4 == 0 or s == 1 for s in sa + sb)
        assert (sa[2] == 1) == transposed and (sb[2] == 1) == transposed
        init = torch.randn(Z0 * Z1 * M, N, generator=g)
        want = alpha * torch.einsum("zyik,zykn->zyin", A.double(), Bv.double()).reshape(-1, N)
        if accumulate:
            want = want + init.double()
        hc = W.embed(init.to(DEV), ld=N + 64 + 4 * (M % 3), output=not accumulate, name="C")
        sc = (Z1 * M * hc.ld, M * hc.ld, hc.ld, 1)
        autograd.bmm(Ad, sa, Bd, sb, hc.view, sc, Z0, Z1, M, N, K, alpha=alpha, accumulate=accumulate)
        plain = init.to(DEV).clone()
        autograd.bmm(Ad, sa, Bd, sb, plain, (Z1 * M * N, M * N, N, 1), Z0, Z1, M, N, K, alpha=alpha, accumulate=accumulate)
        W.assert_written_and_finite(hc)
        W.assert_guards_intact(hc)
        rel_close(hc.view, want, 2e-5, f"C ({M} x {N} x {K})")          # the attention backward it serves
        same_bits(hc, plain, f"C ({M} x {N} x {K})")


# ---------------------------------------------------------------------------------------------------- alignment refusals
def _refusal_calls():
    """name -> callable(shift_floats, ld_extra, out) -> rc: a valid call of the entry point on 16-byte aligned rows when both are
    0; shift_floats moves one row operand's pointer by that many floats, ld_extra is added to one leading dimension."""
    from vrdone_amd import _hip
    lib = _hip.lib
    B, T, Cw, H = 2, 8, 256, 4
    rows = B * T
    z = lambda *s: torch.zeros(*s, device=DEV)          # noqa: E731
    x, y, w3 = z(rows + 1, Cw), z(rows + 1, Cw), z(rows + 1, 3 * Cw)
    vec, mask = torch.ones(2 * Cw, device=DEV), torch.ones(rows, dtype=torch.uint8, device=DEV)
    q, k, v = w3[:, :Cw], w3[:, Cw:2 * Cw], w3[:, 2 * Cw:]
    off = lambda t, s: t.data_ptr() + 4 * s          # noqa: E731
    calls = {}
    calls["vrd_layernorm"] = lambda s, e, o: lib.vrd_layernorm(off(x, s), Cw + e, p(o), Cw, rows, Cw, p(vec), p(vec), 0, None, 0, 0, 0, stream())
    calls["vrd_maxpool_mask"] = lambda s, e, o: lib.vrd_maxpool_mask(off(x, s), Cw + e, B, T, Cw, p(mask), p(o), Cw, p(mask.clone()), stream())
    calls["vrd_mask_head"] = lambda s, e, o: lib.vrd_mask_head(p(x), Cw, off(y, s), Cw + e, p(mask), B, 2, T, Cw, -10.0, p(o), stream())
    calls["vrd_local_attn"] = lambda s, e, o: lib.vrd_local_attn(off(q, s), p(k), p(v), 3 * Cw + e, p(mask), None, B, T, Cw, H, 2, p(o), Cw, 0,
                                                                 stream())
    calls["vrd_attention"] = lambda s, e, o: lib.vrd_attention(p(q), 3 * Cw, off(k, s), p(v), 3 * Cw + e, p(mask), B, T, T, H, 64, p(o), Cw, 0, 0,
                                                               stream())
    calls["vrd_attention_pair"] = lambda s, e, o: lib.vrd_attention_pair(p(q), 3 * Cw, off(k, s), p(v), 3 * Cw + e, p(mask), None, B, T, T, H, 64,
                                                                         p(o), Cw, 0, _hip.PAIR_BF16, stream(), 0)
    calls["vrd_rowcol_scale"] = lambda s, e, o: lib.vrd_rowcol_scale(p(x), Cw, rows, Cw, p(vec), None, p(mask), off(y, s), Cw + e, 0, None, 0, p(o),
                                                                     Cw, stream())
    calls["vrd_activation"] = lambda s, e, o: lib.vrd_activation(p(x), Cw, off(y, s), Cw + e, rows, Cw, _hip.ACT_GELU, p(o), Cw, stream())
    calls["vrd_layernorm_bwd"] = lambda s, e, o: lib.vrd_layernorm_bwd(p(x), Cw, off(y, s), Cw + e, rows, Cw, p(vec), p(vec), 0, p(o), Cw, p(z(Cw)),
                                                                       p(z(Cw)), None, 0, stream(), 0)
    calls["vrd_local_attn_bwd"] = lambda s, e, o: lib.vrd_local_attn_bwd(p(q), p(k), p(v), 3 * Cw, off(y, s), Cw + e, p(mask), None, B, T, Cw, H, 2,
                                                                         p(o), p(z(rows, Cw)), p(z(rows, Cw)), Cw, p(z(2 * rows * H * 5)), stream())
    calls["vrd_attn_bwd_probs"] = lambda s, e, o: lib.vrd_attn_bwd_probs(p(q), 3 * Cw, off(k, s), p(v), 3 * Cw + e, p(y), Cw, p(mask), B, T, T, H, 64,
                                                                         p(o), p(z(B * H * T * T)), stream())
    calls["vrd_attention_rows"] = lambda s, e, o: lib.vrd_attention_rows(p(q), 3 * Cw, off(k, s), p(v), 3 * Cw + e, p(mask), B, T, T, H, 64,
                                                                         _hip.PAIR_BF16, p(o), Cw, p(z(B * H * T)), stream())
    calls["vrd_attention_bwd"] = lambda s, e, o: lib.vrd_attention_bwd(p(q), 3 * Cw, off(k, s), p(v), 3 * Cw + e, p(x), p(y), Cw, p(mask), B, T, T, H, 64,
                                                                       p(o), p(z(rows, Cw)), p(z(rows, Cw)), None, p(z(2 * B * H * T)), None, None,
                                                                       stream())

    def conv_ln(s, e, o):
        a = _hip.ConvLnArgs()
        xin, w = z(rows, 8), z(Cw, 8, 3)
        a.x, a.ldx, a.rows, a.Cin, a.taps, a.T, a.N, a.w = p(xin), 8, rows, 8, 3, T, Cw, p(w)
        a.y, a.ldy = off(o, s), Cw + e
        return lib.vrd_conv_ln(C.byref(a), stream())

    def dwconv_ln(s, e, o):
        a = _hip.DwconvLnArgs()
        w = z(Cw, 1, 3)
        a.x, a.ldx, a.B, a.Tin, a.C, a.ksize, a.stride, a.group_in, a.n_out = off(x, s), Cw + e, B, T, Cw, 3, 1, 1, 1
        a.w[0], a.y[0], a.ldy[0] = p(w), p(o), Cw
        return lib.vrd_dwconv_ln(C.byref(a), stream())

    def gemm_pair_out(s, e, o):
        a = _hip.GemmArgs()
        w = z(Cw, 8)
        a.A, a.lda, a.W, a.C, a.ldc, a.M, a.N, a.Cin, a.taps, a.T = p(z(rows, 8)), 8, p(w), off(o, s), Cw + 4 * e, rows, Cw, 8, 1, T
        a.c_pair = _hip.PAIR_BF16
        return lib.vrd_gemm(C.byref(a), stream())

    calls["vrd_conv_ln"], calls["vrd_dwconv_ln"], calls["vrd_gemm (pair rows out)"] = conv_ln, dwconv_ln, gemm_pair_out
    return calls


REFUSALS = ["vrd_layernorm", "vrd_conv_ln", "vrd_dwconv_ln", "vrd_maxpool_mask", "vrd_mask_head", "vrd_local_attn", "vrd_attention",
            "vrd_attention_pair", "vrd_gemm (pair rows out)", "vrd_rowcol_scale", "vrd_activation", "vrd_layernorm_bwd", "vrd_local_attn_bwd",
            "vrd_attn_bwd_probs", "vrd_attention_rows", "vrd_attention_bwd"]


@pytest.mark.parametrize("name", REFUSALS)
def test_misaligned_rows_are_refused_before_any_launch(name):
    """The entry points that read or write rows with 16-byte accesses and have no scalar form say so in the header; each has its
    VRD_CHECK_ARG: a row pointer 4 bytes off a 16-byte boundary, or a leading dimension that is no multiple of 4 floats, returns
    an error naming the entry point, and nothing is launched (the output still holds the sentinel).  Only calls the host code
    refuses are made here; the entry points with a scalar form for such rows (vrd_gemm, vrd_gemm_wgrad*, vrd_colsum,
    vrd_dwconv_wgrad, vrd_dwconv_bwd, vrd_maxpool_bwd, vrd_bmm, vrd_absmax_scale's callers) have no such rule."""
    from vrdone_amd import _hip
    call = _refusal_calls()[name]
    for shift, extra in ((1, 0), (0, 1)):
        o = W.embed_out((17, 1024), DEV, ld=1024, c0=0, rows_before=0, rows_after=0, name="out").buf
        rc = call(shift, extra, o)
        torch.cuda.synchronize()
        assert rc < 0, f"{name} accepted rows that are not 16-byte aligned (pointer shift {shift} floats, ld + {extra})"
        assert name.split(" ")[0].encode() in _hip.lib.vrd_last_error()
        assert bool((o.view(torch.int32) == W.SENTINEL_BITS).all()), f"{name} wrote its output although it returned an error"


def test_leading_dimensions_narrower_than_the_row_are_refused():
    """vrd_local_attn_bwd, vrd_attn_bwd_probs and vrd_dwconv_ln's x_up took a leading dimension below the row width (rows that
    overlap: the outputs of one row would land in the next); each now has the check every other entry point had."""
    from vrdone_amd import _hip
    lib = _hip.lib
    B, T, Cw, H = 2, 8, 256, 4
    rows = B * T
    z = lambda *s: torch.zeros(*s, device=DEV)          # noqa: E731
    x, mask = z(rows, Cw), torch.ones(rows, dtype=torch.uint8, device=DEV)
    o = W.embed_out((17, 1024), DEV, ld=1024, c0=0, rows_before=0, rows_after=0, name="out").buf
    narrow = Cw - 4
    assert lib.vrd_local_attn_bwd(p(x), p(x), p(x), Cw, p(x), Cw, p(mask), None, B, T, Cw, H, 2, p(o), p(o), p(o), narrow, p(z(2 * rows * H * 5)),
                                  stream()) < 0
    assert b"vrd_local_attn_bwd" in lib.vrd_last_error()
    assert lib.vrd_attn_bwd_probs(p(x), narrow, p(x), p(x), Cw, p(x), Cw, p(mask), B, T, T, H, 64, p(o), p(o), stream()) < 0
    assert b"vrd_attn_bwd_probs" in lib.vrd_last_error()
    a = _hip.DwconvLnArgs()
    w = z(Cw, 1, 3)
    a.x, a.ldx, a.B, a.Tin, a.C, a.ksize, a.stride, a.group_in, a.n_out = p(x), Cw, B, T, Cw, 3, 1, 1, 1
    a.x_up, a.ldx_up = p(x), narrow
    a.w[0], a.y[0], a.ldy[0] = p(w), p(o), Cw
    assert lib.vrd_dwconv_ln(C.byref(a), stream()) < 0 and b"vrd_dwconv_ln" in lib.vrd_last_error()
    torch.cuda.synchronize()
    assert bool((o.view(torch.int32) == W.SENTINEL_BITS).all())
