"""Deterministic mode on the GPU: the parameter-gradient kernels give the same bits whatever the alignment, the scratch offered
and the concurrent work; a training step (forward, backward, clip, AdamW, EMA) repeats bit for bit eagerly, as HIP-graph
replays, across processes, and when torch's own determinism flags switch the mode on; and it stays reference-grade."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, T = 49152, 96            # ~49 k rows: 96 chunks of the f32 kernel, hundreds of row blocks (> 32 partial rows) elsewhere


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


def _need():
    from vrdone_amd import _hip
    n = ctypes.c_int64(-1)
    _hip.check(_hip.lib.vrd_scratch_required(ctypes.byref(n)), "vrd_scratch_required")
    return n.value


def _placed(t, off, fill=float("nan")):
    """t copied to a fresh device buffer `off` floats past its start (off = 1: no longer 16-byte aligned)"""
    buf = torch.full((t.numel() + off + 64,), fill, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t.to(DEV))
    return v


def _variants(call, outs, offsets=(0, 1, 4)):
    """call(ins_offset, outs, scratch_ptr, floats) -> rc.  Every variant's outputs (cpu): 5 repeats, shifted operands, exact and
    oversized scratch, a large GEMM on a second stream at the same time.  Too-small scratch must be refused."""
    from vrdone_amd import _hip
    rc = call(0, [torch.zeros_like(o) for o in outs], None, 0)
    need = _need() if rc == _hip.ERR_SCRATCH else 0
    assert rc in (0, _hip.ERR_SCRATCH), _hip.lib.vrd_last_error()
    if need:
        small = torch.zeros(need, device=DEV)
        assert call(0, [torch.zeros_like(o) for o in outs], small.data_ptr(), need - 1) == _hip.ERR_SCRATCH
    results = []
    big = torch.randn(8192, 8192, device=DEV)

    def one(off, extra, side=False):
        o = [_placed(torch.zeros_like(x), off, 0.0) for x in outs]
        sc = torch.full((need + extra + 8,), float("nan"), device=DEV)
        if side:
            s2 = torch.cuda.Stream()
            s2.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s2):
                prod = big @ big
        _hip.check(call(off, o, sc.data_ptr() if need else None, need + extra if need else 0), "deterministic call")
        if side:
            torch.cuda.current_stream().wait_stream(s2)
            del prod
        torch.cuda.synchronize()
        return [x.cpu() for x in o]

    for _ in range(5):
        results.append(one(0, 0))
    for off in offsets:
        results.append(one(off, 0))
        results.append(one(off, 1 << 20))
    results.append(one(0, 12345, side=True))
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert torch.equal(a, b), "deterministic result differs between runs"
    return results[0]


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-30))


def _wgrad_want(G, X, mask, k, T=T):
    Gm = (G * mask[:, None]).double()
    Xs = X.double().view(-1, T, X.shape[1])
    taps = [torch.nn.functional.pad(Xs, (0, 0, 1, 1))[:, t:t + T].reshape(-1, X.shape[1]) for t in range(3)] if k == 3 else [X.double()]
    return torch.cat([Gm.t() @ xt for xt in taps], 1), Gm.sum(0)


@pytest.mark.parametrize("plane", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("k", [1, 3])
def test_weight_gradient_bits(plane, k):
    from vrdone_amd import _hip
    N = Cin = 512
    g = torch.Generator().manual_seed(7 * k)
    G, X = torch.randn(ROWS, N, generator=g), torch.randn(ROWS, Cin, generator=g)
    mask = (torch.rand(ROWS, generator=g) < 0.8).to(torch.uint8)
    ins = {off: (_placed(G, off), _placed(X, off)) for off in (0, 1, 4)}
    md = mask.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    scale = None
    if plane == "f16":           # (vrd_absmax_scale wants aligned rows: the factor of the aligned copy, the same values)
        scale = torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV)
        _hip.check(_hip.lib.vrd_absmax_scale(ins[0][0].data_ptr(), N, ROWS, N, scale.data_ptr(), stream), "vrd_absmax_scale")

    def call(off, outs, sp, n):
        Gd, Xd = ins[off]
        if plane == "f32":
            return _hip.lib.vrd_gemm_wgrad(Gd.data_ptr(), N, Xd.data_ptr(), Cin, md.data_ptr(), ROWS, N, Cin, k, T, outs[0].data_ptr(),
                                           sp, n, stream, _hip.DETERMINISTIC)
        gs = scale.data_ptr() if plane == "f16" else None
        return _hip.lib.vrd_gemm_wgrad_x3(Gd.data_ptr(), N, Xd.data_ptr(), Cin, md.data_ptr(), ROWS, N, Cin, k, T, outs[0].data_ptr(),
                                          outs[1].data_ptr(), sp, n, gs, stream, _hip.DETERMINISTIC)

    outs = [torch.zeros(N, k * Cin, device=DEV)] + ([] if plane == "f32" else [torch.zeros(N, device=DEV)])
    res = _variants(call, outs)
    want, want_b = _wgrad_want(G, X, mask, k)
    assert _rel(res[0], want) <= (1e-6 if plane == "f32" else 2e-5 if plane == "f16" else 2e-4)
    if plane != "f32":
        assert _rel(res[1], want_b) <= 2e-6


@pytest.mark.parametrize("strided_b", [False, True])
def test_column_sum_bits(strided_b):
    from vrdone_amd import _hip
    C = 512
    g = torch.Generator().manual_seed(3)
    a = torch.randn(ROWS, C, generator=g)
    mask = (torch.rand(ROWS, generator=g) < 0.8).to(torch.uint8)
    rs = torch.rand(ROWS, generator=g)
    # strided b: the (rows, 2 C) conv input of a group_in = 2 depthwise conv, column c * 2 + 1, one row back (shift -1)
    b = torch.randn(ROWS, 2 * C if strided_b else C, generator=g)
    ins = {off: (_placed(a, off), _placed(b, off)) for off in (0, 1, 4)}
    md, rd = mask.to(DEV), rs.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    cst, cof, shift = (2, 1, -1) if strided_b else (1, 0, 0)

    def call(off, outs, sp, n):
        ad, bd = ins[off]
        return _hip.lib.vrd_colsum(ad.data_ptr(), C, bd.data_ptr(), b.shape[1], cst, cof, 1, shift, T, md.data_ptr(), rd.data_ptr(),
                                   ROWS, C, outs[0].data_ptr(), sp, n, stream, _hip.DETERMINISTIC)

    (got,) = _variants(call, [torch.zeros(C, device=DEV)])
    w = (a * mask[:, None] * rs[:, None]).double()
    if strided_b:
        bb = b.double().view(-1, T, 2 * C)[:, :, 1::2]
        bb = torch.nn.functional.pad(bb, (0, 0, 1, 0))[:, :T].reshape(ROWS, C)        # row t reads b[t - 1], 0 at t = 0
    else:
        bb = b.double()
    assert _rel(got, (w * bb).sum(0)) <= 1e-6


@pytest.mark.parametrize("ks,gin,stride", [(3, 2, 2), (3, 1, 1), (1, 2, 2)])
def test_depthwise_weight_gradient_bits(ks, gin, stride):
    from vrdone_amd import _hip
    C = 512
    g = torch.Generator().manual_seed(ks + 10 * gin)
    dD = torch.randn(ROWS, C, generator=g)
    x = torch.randn(ROWS * stride, C * gin, generator=g)
    mask = (torch.rand(ROWS, generator=g) < 0.8).to(torch.uint8)
    ins = {off: (_placed(dD, off), _placed(x, off)) for off in (0, 1, 4)}
    md = mask.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(off, outs, sp, n):
        dd, xd = ins[off]
        return _hip.lib.vrd_dwconv_wgrad(dd.data_ptr(), C, xd.data_ptr(), C * gin, ks, stride, gin, T, md.data_ptr(), ROWS, C,
                                         outs[0].data_ptr(), outs[1].data_ptr(), sp, n, stream, _hip.DETERMINISTIC)

    dw, db = _variants(call, [torch.zeros(C, gin, ks, device=DEV), torch.zeros(C, device=DEV)])
    Gm = (dD * mask[:, None]).double().view(-1, T, C)
    xs = x.double().view(-1, stride * T, C, gin)
    want = torch.zeros(C, gin, ks, dtype=torch.float64)
    for kk in range(ks):
        ti = stride * torch.arange(T) + kk - ks // 2
        ok = (ti >= 0) & (ti < stride * T)
        xv = xs[:, ti.clamp(0, stride * T - 1)] * ok[None, :, None, None]
        want[:, :, kk] = (Gm[..., None] * xv).sum((0, 1))
    assert _rel(dw, want) <= 1e-6
    assert _rel(db, Gm.sum((0, 1))) <= 1e-6


@pytest.mark.parametrize("C", [256, 512])
def test_layernorm_backward_bits(C):
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(C)
    x, dy = torch.randn(ROWS, C, generator=g), torch.randn(ROWS, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ins = {off: (_placed(x, off), _placed(dy, off)) for off in (0, 4)}        # (the kernel wants 16-byte aligned rows)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    dx = torch.empty(ROWS, C, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(off, outs, sp, n):
        xd, dyd = ins[off]
        return _hip.lib.vrd_layernorm_bwd(xd.data_ptr(), C, dyd.data_ptr(), C, ROWS, C, gd.data_ptr(), bd.data_ptr(), 0, dx.data_ptr(), C,
                                          outs[0].data_ptr(), outs[1].data_ptr(), sp, n, stream, _hip.DETERMINISTIC)

    dg, db = _variants(call, [torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)], offsets=(0, 4))
    xd = x.double()
    xhat = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
    assert _rel(dg, (dy.double() * xhat).sum(0)) <= 1e-6
    assert _rel(db, dy.double().sum(0)) <= 1e-6


# Small inputs: the same calls where the scratch holds few partial rows -- 33 of them (the first two-level reduction), one block,
# two chunks, tile partials + bias rows + their levels in one buffer.  _variants' NaN-filled scratch shows a region read before it
# was written or a level written over another.  Tolerances: those of the 49 k-row tests above.
TS = 16            # frames per sequence of the small inputs


def _small_colsum(rows, C):
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(rows + C)
    a, b = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    mask, rs = (torch.rand(rows, generator=g) < 0.8).to(torch.uint8), torch.rand(rows, generator=g)
    ins = {off: (_placed(a, off), _placed(b, off)) for off in (0, 1, 4)}
    md, rd = mask.to(DEV), rs.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(off, outs, sp, n):
        ad, bd = ins[off]
        return _hip.lib.vrd_colsum(ad.data_ptr(), C, bd.data_ptr(), C, 1, 0, 1, 0, TS, md.data_ptr(), rd.data_ptr(), rows, C, outs[0].data_ptr(),
                                   sp, n, stream, _hip.DETERMINISTIC)

    (got,) = _variants(call, [torch.zeros(C, device=DEV)])
    assert _rel(got, ((a * mask[:, None] * rs[:, None]).double() * b.double()).sum(0)) <= 1e-6


def _small_dwconv(rows, C, ks, gin, stride):
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(rows + ks + 10 * gin)
    dD, x = torch.randn(rows, C, generator=g), torch.randn(rows * stride, C * gin, generator=g)
    mask = (torch.rand(rows, generator=g) < 0.8).to(torch.uint8)
    ins = {off: (_placed(dD, off), _placed(x, off)) for off in (0, 1, 4)}
    md = mask.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(off, outs, sp, n):
        dd, xd = ins[off]
        return _hip.lib.vrd_dwconv_wgrad(dd.data_ptr(), C, xd.data_ptr(), C * gin, ks, stride, gin, TS, md.data_ptr(), rows, C,
                                         outs[0].data_ptr(), outs[1].data_ptr(), sp, n, stream, _hip.DETERMINISTIC)

    dw, db = _variants(call, [torch.zeros(C, gin, ks, device=DEV), torch.zeros(C, device=DEV)])
    Gm = (dD * mask[:, None]).double().view(-1, TS, C)
    xs = x.double().view(-1, stride * TS, C, gin)
    want = torch.zeros(C, gin, ks, dtype=torch.float64)
    for kk in range(ks):
        ti = stride * torch.arange(TS) + kk - ks // 2
        ok = (ti >= 0) & (ti < stride * TS)
        want[:, :, kk] = (Gm[..., None] * (xs[:, ti.clamp(0, stride * TS - 1)] * ok[None, :, None, None])).sum((0, 1))
    assert _rel(dw, want) <= 1e-6
    assert _rel(db, Gm.sum((0, 1))) <= 1e-6


def _small_layernorm(rows, C):
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(rows + C)
    x, dy = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ins = {off: (_placed(x, off), _placed(dy, off)) for off in (0, 4)}        # (the kernel wants 16-byte aligned rows)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    dx = torch.empty(rows, C, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(off, outs, sp, n):
        xd, dyd = ins[off]
        return _hip.lib.vrd_layernorm_bwd(xd.data_ptr(), C, dyd.data_ptr(), C, rows, C, gd.data_ptr(), bd.data_ptr(), 0, dx.data_ptr(), C,
                                          outs[0].data_ptr(), outs[1].data_ptr(), sp, n, stream, _hip.DETERMINISTIC)

    dg, db = _variants(call, [torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)], offsets=(0, 4))
    xd = x.double()
    xhat = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
    assert _rel(dg, (dy.double() * xhat).sum(0)) <= 1e-6
    assert _rel(db, dy.double().sum(0)) <= 1e-6


def _small_wgrad(plane, M, N, Cin, k):
    """f32: vrd_gemm_wgrad; bf16 / f16: vrd_gemm_wgrad_x3 with dbias"""
    from vrdone_amd import _hip
    g = torch.Generator().manual_seed(M + N + k)
    G, X = torch.randn(M, N, generator=g), torch.randn(M, Cin, generator=g)
    mask = (torch.rand(M, generator=g) < 0.8).to(torch.uint8)
    ins = {off: (_placed(G, off), _placed(X, off)) for off in (0, 1, 4)}
    md = mask.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    scale = None
    if plane == "f16":           # (vrd_absmax_scale wants float4 rows: the factor of a copy padded with zero columns, the same maximum)
        N4 = (N + 3) // 4 * 4
        Gp = torch.zeros(M, N4, device=DEV)
        Gp[:, :N] = G.to(DEV)
        scale = torch.zeros(_hip.ABSMAX_SCALE_FLOATS, device=DEV)
        _hip.check(_hip.lib.vrd_absmax_scale(Gp.data_ptr(), N4, M, N4, scale.data_ptr(), stream), "vrd_absmax_scale")

    def call(off, outs, sp, n):
        Gd, Xd = ins[off]
        if plane == "f32":
            return _hip.lib.vrd_gemm_wgrad(Gd.data_ptr(), N, Xd.data_ptr(), Cin, md.data_ptr(), M, N, Cin, k, TS, outs[0].data_ptr(), sp, n, stream,
                                           _hip.DETERMINISTIC)
        gs = scale.data_ptr() if plane == "f16" else None
        return _hip.lib.vrd_gemm_wgrad_x3(Gd.data_ptr(), N, Xd.data_ptr(), Cin, md.data_ptr(), M, N, Cin, k, TS, outs[0].data_ptr(),
                                          outs[1].data_ptr(), sp, n, gs, stream, _hip.DETERMINISTIC)

    outs = [torch.zeros(N, k * Cin, device=DEV)] + ([] if plane == "f32" else [torch.zeros(N, device=DEV)])
    res = _variants(call, outs)
    if M * N * Cin > 1 << 30:    # (the float64 products of the largest case on the device: seconds on the CPU)
        assert k == 1
        Gm = (G * mask[:, None]).double().to(DEV)
        want, want_b = (Gm.t() @ X.double().to(DEV)).cpu(), Gm.sum(0).cpu()
    else:
        want, want_b = _wgrad_want(G, X, mask, k, TS)
    assert _rel(res[0], want) <= (1e-6 if plane == "f32" else 2e-5 if plane == "f16" else 2e-4)
    if plane != "f32":
        assert _rel(res[1], want_b) <= 2e-6


SMALL_CASES = {
    "colsum-528x8": (_small_colsum, 528, 8),                     # float4 form, 33 partial rows
    "colsum-1056x6": (_small_colsum, 1056, 6),                   # scalar form, 33 partial rows
    "colsum-16x4": (_small_colsum, 16, 4),                       # one block, no second level
    "dwconv-528x8-k3g1s1": (_small_dwconv, 528, 8, 3, 1, 1),
    "dwconv-1056x8-k3g2s2": (_small_dwconv, 1056, 8, 3, 2, 2),
    "layernorm-1056x256": (_small_layernorm, 1056, 256),
    "layernorm-1056x512": (_small_layernorm, 1056, 512),
    "x3-bf16-192x133x63-k3": (_small_wgrad, "bf16", 192, 133, 63, 3),       # wave kernel + its own column-sum launch
    "x3-f16-192x133x63-k3": (_small_wgrad, "f16", 192, 133, 63, 3),
    "x3-bf16-4224x128x128-k1": (_small_wgrad, "bf16", 4224, 128, 128, 1),   # 33 chunks: tiles, bias rows and a two-level bias tree
    "x3-f16-4224x128x128-k1": (_small_wgrad, "f16", 4224, 128, 128, 1),
    "x3-f16-65536x256x256-k1": (_small_wgrad, "f16", 65536, 256, 256, 1),   # the 256 x 256 tiles
    "wgrad-1024x96x40-k3": (_small_wgrad, "f32", 1024, 96, 40, 3),          # two chunks
}


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_small_shapes_bits(case):
    fn, *args = SMALL_CASES[case]
    fn(*args)


# ------------------------------------------------------------------------------------------------------------- model level
def _run(**kw):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import train_step
    from vrdone_amd import ops
    with ops.use_deterministic(True):
        return train_step.run(steps=1, verbose=False, deterministic=True, **kw)


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("config", ["vidvrd", "vidor", "vidor_x", "vidor_local"])
def test_training_step_repeats_bit_for_bit(config, precision):
    """seed -> one full step (stochastic depth on), twice, eagerly and with training graphs: losses, gradients, parameters and EMA
    are the same bits; and the graphed step is the eager step."""
    from vrdone_amd import ops
    with ops.use_precision(precision):
        e1, e2 = _run(config=config), _run(config=config)
        g1, g2 = _run(config=config, graphs=True), _run(config=config, graphs=True)
    assert e1["total_loss"] == e2["total_loss"] and e1["sha256"] == e2["sha256"], "eager steps differ"
    assert g1["total_loss"] == g2["total_loss"] and g1["sha256"] == g2["sha256"], "graphed steps differ"
    assert g1["total_loss"] == e1["total_loss"] and g1["sha256"] == e1["sha256"], "graphed and eager steps differ"


def test_two_processes_give_the_same_bits():
    digests = []
    for _ in range(2):
        out = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(REPO, "scripts", "train_step.py"), "--steps", "3",
                              "--deterministic"], cwd=REPO, capture_output=True, text=True, timeout=700)
        assert out.returncode == 0, out.stderr[-2000:]
        digests.append(json.loads(out.stdout.strip().splitlines()[-1])["sha256"])
    assert digests[0] == digests[1]


@pytest.mark.parametrize("flag", ["cudnn", "algorithms"])
def test_torch_flags_switch_the_mode_on(flag):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import train_step
    from vrdone_amd import ops
    prev = (torch.backends.cudnn.deterministic, torch.are_deterministic_algorithms_enabled(), ops._deterministic,
            os.environ.get("CUBLAS_WORKSPACE_CONFIG"))
    try:
        ops.set_deterministic(None)
        if flag == "cudnn":
            torch.backends.cudnn.deterministic = True
        else:
            os.environ["CUBLAS_WORKSPACE_CONFIG"] = ":4096:8"          # as the reference's utils.set_seed does
            torch.use_deterministic_algorithms(True)
        assert ops.get_deterministic()
        log = train_step.run(steps=1, verbose=False)
        assert log["nonfinite_grads"] == [] and log["param_delta_norm"] > 0
    finally:
        torch.backends.cudnn.deterministic = prev[0]
        torch.use_deterministic_algorithms(prev[1])
        ops.set_deterministic(prev[2])
        if prev[3] is None:
            os.environ.pop("CUBLAS_WORKSPACE_CONFIG", None)
        else:
            os.environ["CUBLAS_WORKSPACE_CONFIG"] = prev[3]


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("case", ["nodrop", "pinned"])
def test_deterministic_step_meets_the_reference_goldens(case, precision):
    """The reference-gradient check of tests/test_gpu_train.py, same bounds, in the deterministic mode."""
    import test_gpu_train
    from vrdone_amd import ops
    with ops.use_precision(precision), ops.use_deterministic(True):
        test_gpu_train.test_training_step_matches_reference_gradients(case, precision)
