"""Every forward kernel's rows beyond the 32-bit offset lines (tests/far_cases.py), on a real MI355X.

Each test makes ONE call over all R rows of its case through the ops wrapper or C entry point the model uses, on periodic inputs
(61 ragged sequences, repeated) and outputs that start as the sentinel NaN of tests/window_cases.py, and asserts
  (a) period 0 of every output against a float64 reference of that one period, at the tolerance of the family's existing direct
      test (named at each `close`);
  (b) EVERY later period, and the trailing partial one, equals period 0 bit for bit (compared on the device, in slices);
  (c) the guard rows behind the last row, and the columns beside a window, still hold the sentinel, and no written row does;
  (d) the inputs are unchanged (a device checksum per buffer before and after).
A kernel that computes one offset in 32 bits -- signed or unsigned, in bytes or in elements -- reads or writes a wrapped address
behind the line: a far row then holds other data or poison (tests/test_far_cases_cpu.py shows the checker seeing each of these).
All buffers of a case are carved from one arena, allocated once (the cases are sized against a 32 GiB cap)."""
import ctypes as C

import pytest
import torch

import far_cases as Fc
import window_cases as W
from oracle import vrd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = torch.nn.functional
T, NSEQ = Fc.T, Fc.NSEQ
PEAKS = []                                         # peak device memory of every test that took the arena, in bytes
ARENA_BYTES = Fc.MEMORY_CAP - (1 << 30)          # the cases need up to 29.8 GiB; the rest of the cap is for references and temporaries


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


# ------------------------------------------------------------------------------------------------------------------ the arena
class Arena:
    buf = None

    def __init__(self):
        if Arena.buf is None:
            free, total = torch.cuda.mem_get_info()
            if free < ARENA_BYTES + (2 << 30):
                print(f"far rows: {free} bytes of device memory free, {ARENA_BYTES + (2 << 30)} needed")
                pytest.skip(f"device memory: {free} bytes free, {ARENA_BYTES + (2 << 30)} needed")
            Arena.buf = torch.empty(ARENA_BYTES // 4, dtype=torch.int32, device=DEV)
        self.at = 0
        self.inputs, self.outputs = [], []

    def take(self, rows, pitch):
        """(rows, pitch) int32, 256-byte aligned, filled with the sentinel"""
        n = rows * pitch
        assert (self.at + n) * 4 <= ARENA_BYTES, "the case does not fit its arena"
        t = Arena.buf[self.at:self.at + n].view(rows, pitch)
        self.at += (n + 63) // 64 * 64
        t.fill_(W.SENTINEL_BITS)
        return t

    def input(self, name, period, rows, pitch=None):
        """period (P, width) f32 (or pair rows in f32 clothing) on the device -> (rows, width) f32 view of a (rows, pitch) buffer that
        repeats it"""
        P, width = period.shape
        pitch = width if pitch is None else pitch
        raw = self.take(rows, pitch)
        win, p = raw[:, :width], period.contiguous().view(torch.int32)
        n = rows // P
        if n:
            win[:n * P].unflatten(0, (n, P)).copy_(p[None].expand(n, P, width))
        win[n * P:] = p[:rows - n * P]
        self.inputs.append((name, raw, checksum(raw)))
        return win.view(torch.float32)

    def output(self, name, rows, width, pitch=None, guard=Fc.GUARD_ROWS):
        pitch = width if pitch is None else pitch
        raw = self.take(rows + guard, pitch)
        self.outputs.append((name, raw, rows, width))
        return raw[:rows, :width].view(torch.float32)

    def halves(self, name, half_rows, width, guard=Fc.GUARD_ROWS):
        """a (2, half_rows, width) output, subject rows then object rows, each half with its own periods: checked as two outputs
        (the guard rows lie behind the second).  Returns the whole buffer's f32 view."""
        raw = self.take(2 * half_rows + guard, width)
        self.outputs.append((name + " (subject half)", raw[:half_rows], half_rows, width))
        self.outputs.append((name + " (object half)", raw[half_rows:], half_rows, width))
        return raw[:2 * half_rows].view(torch.float32)

    def check(self, periods):
        """(b), (c), (d); periods: {output name: rows of one period}"""
        torch.cuda.synchronize()
        for name, raw, rows, width in self.outputs:
            assert bool((raw[rows:] == W.SENTINEL_BITS).all()), f"{name}: the guard rows behind row {rows - 1} were written"
            assert bool((raw[:, width:] == W.SENTINEL_BITS).all()), f"{name}: the columns beside the window were written"
            P = periods[name.split(" (")[0]]
            win = raw[:rows, :width]
            assert not bool((win[:P] == W.SENTINEL_BITS).any()), f"{name}: poison left in period 0"
            first = win[:P]
            step = max(1, (64 << 20) // (P * width)) * P                   # slices of about 256 MiB
            for s in range(P, rows, step):
                blk = win[s:min(s + step, rows)]
                n = blk.shape[0] // P
                bad = None
                if n and not bool((blk[:n * P].unflatten(0, (n, P)) == first[None]).all()):
                    bad = (blk[:n * P].unflatten(0, (n, P)) != first[None]).any(-1).flatten()
                elif blk.shape[0] % P and not bool((blk[n * P:] == first[:blk.shape[0] - n * P]).all()):
                    bad = torch.cat([torch.zeros(n * P, dtype=torch.bool, device=DEV), (blk[n * P:] != first[:blk.shape[0] - n * P]).any(-1)])
                if bad is not None:
                    r = s + int(torch.nonzero(bad)[0])
                    poison = bool((win[r] == W.SENTINEL_BITS).any())
                    raise AssertionError(f"{name}: row {r} of {rows} (byte offset {r * raw.shape[1] * 4:#x}) differs from row {r % P} of period 0"
                                         f"{' -- it holds poison: never written' if poison else ''}; {int(bad.sum())} such rows in this slice")
        for name, raw, before in self.inputs:
            assert checksum(raw) == before, f"input {name} was written"


def checksum(raw):
    """sum of the buffer's int32 words, in int64, in slices (a whole-buffer sum would first widen a 27 GiB buffer to int64)"""
    flat = raw.reshape(-1) if raw.is_contiguous() else raw.contiguous().view(-1)
    total = torch.zeros((), dtype=torch.int64, device=raw.device)
    for s in range(0, flat.numel(), 1 << 26):
        total += flat[s:s + (1 << 26)].sum(dtype=torch.int64)
    return int(total)


@pytest.fixture
def arena():
    # what other modules of the session keep on the device (cached models) is not this test's
    others = torch.cuda.memory_allocated() - (ARENA_BYTES if Arena.buf is not None else 0)
    a = Arena()
    torch.cuda.reset_peak_memory_stats()
    yield a
    peak = torch.cuda.max_memory_allocated() - others
    PEAKS.append(peak)
    assert peak <= Fc.MEMORY_CAP, f"the test held {peak / 2 ** 30:.2f} GiB of device memory, the cap is {Fc.MEMORY_CAP >> 30} GiB"


@pytest.fixture(scope="module", autouse=True)
def _release_the_arena():
    yield
    Arena.buf = None
    torch.cuda.empty_cache()


def cases_for(*names):
    """(case, mode) parameters of the named cases, one per precision mode the case is listed for"""
    out = []
    for n in names:
        c = Fc.CASES[n]
        out += [pytest.param(c, m, id=f"{n}-{m}") for m in c.modes]
    return out


def named(prefix):
    return [n for n in Fc.CASES if n.startswith(prefix)]


def use(m):
    from vrdone_amd import ops
    return ops.use_precision(m)


# ---------------------------------------------------------------------------------------------------------------- helpers
def close(got, want, atol, what=""):
    """tests/test_gpu_ops.py `close`: absolute, against the float64 reference"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) if got.numel() else 0.0
    print(f"{what}: max abs error {err:.3e} (tolerance {atol:.1e})")
    assert err <= atol, f"{what}: max abs error {err:.3e} (tolerance {atol:.1e})"


def rel_close(got, want, rtol, what=""):
    """tests/test_gpu_backward.py `rel_close`: relative to the largest entry of the float64 reference"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    print(f"{what}: max error {err:.3e} of the largest entry (tolerance {rtol:.1e})")
    assert err <= rtol, f"{what}: max error {err:.3e} of the largest entry (tolerance {rtol:.1e})"


def pair_close(got_pair, want, atol, what):
    """pair rows: the f32 result rounded to hi + lo, 2^-15 relative (test_pair_row_format_round_trip, test_gemm_large_tile_kernels),
    on top of the f32 result's own bound"""
    got, want = got_pair.float().double().cpu(), want.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    err = (got - want).abs() - 2.0 ** -15 * want.abs().clamp_min(1e-3)
    print(f"{what}: max abs error beyond the pair rounding {float(err.max()):.3e} (tolerance {atol:.1e})")
    assert float(err.max()) <= atol, f"{what}: max abs error beyond the pair rounding {float(err.max()):.3e} (tolerance {atol:.1e})"


def to_pair(t, fmt):
    """f32 (..., C) -> pair rows (tests/test_gpu_ops.py _to_pair; mirrors vrd::store_pair4)"""
    from vrdone_amd import _hip
    f16 = fmt == _hip.PAIR_F16
    dt = torch.float16 if f16 else torch.bfloat16
    t = t * 2.0 ** _hip.F16_ACT_EXP if f16 else t
    hi = t.to(dt)
    lo = (t - hi.float()).to(dt)
    Cw = t.shape[-1]
    raw = torch.stack([hi.reshape(*t.shape[:-1], Cw // 32, 32), lo.reshape(*t.shape[:-1], Cw // 32, 32)], dim=-2)
    return raw.reshape(*t.shape[:-1], 2 * Cw).contiguous().view(torch.float32)


def period_lens(seed, frames=T):
    lens = torch.randint(1, frames + 1, (NSEQ,), generator=torch.Generator().manual_seed(seed))
    lens[:4] = torch.tensor([frames, frames // 2, 2, 1])
    return lens


def lens_mask(lens, frames=T):
    return torch.arange(frames)[None] < lens[:, None]


def tiled(period, n):
    """a small per-sequence tensor (mask bytes, lengths) of one period, repeated to n sequences, on the device"""
    reps = -(-n // period.shape[0])
    return period.repeat(reps, *([1] * (period.dim() - 1)))[:n].contiguous().to(DEV)


def cl(x):          # (B, C, T) <-> (B, T, C)
    return x.transpose(1, 2).contiguous()


def stream():
    from vrdone_amd import ops
    return ops._stream()


def ok(rc, what):
    from vrdone_amd import _hip
    _hip.check(rc, what)


def p(t):
    return None if t is None else t.data_ptr()


def dv(t):
    return None if t is None else t.to(DEV)


def rows3(t, frames):
    """(R, C) rows -> (B, frames, C) view"""
    return t.unflatten(0, (t.shape[0] // frames, frames))


# ------------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("case,m", cases_for("bct_to_btc_vec", "bct_to_btc_scalar"))
def test_bct_to_btc_far(case, m, arena):
    """the (B, C_in, T) source beyond 2^32 elements; frames= and index= (sequence i comes from item i +- 61: far items feed far rows)"""
    from vrdone_amd import ops
    prm = case.params
    frames, c0, count = prm["frames"], prm["c0"], prm["count"]
    Cin = case.bufs[0].pitch // T
    B = case.nseq()
    g = torch.Generator().manual_seed(c0 + frames)
    src_p = torch.randn(NSEQ, Cin * T, generator=g)
    with use(m):
        pair = ops.pair_mode() and count % 32 == 0
        # vrd_bct_to_btc's choice between its two kernels (float4 loads need every one of these; the arena is 256-byte aligned)
        vec = frames % 4 == 0 and T % 4 == 0 and count % 4 == 0
        assert vec == (case.body == "bct_to_btc_vec_kernel"), "the case's sizes do not select the kernel body it names"
        src = arena.input("src", src_p.to(DEV), B, Cin * T).view(B, Cin, T)
        dst = arena.output("dst", B * frames, count)
        i = torch.arange(B)
        blk = i // NSEQ
        j = torch.where(blk % 2 == 0, i + NSEQ, i - NSEQ)
        index = torch.where(j < B, j, i).to(torch.int32).to(DEV)
        got = ops.bct_to_btc(src, c0, count, rows3(dst, frames), pair=pair, frames=frames, index=index)
        want = src_p.view(NSEQ, Cin, T)[:, c0:c0 + count, :frames].transpose(1, 2).reshape(NSEQ * frames, count)
        arena.check({"dst": NSEQ * frames})
        if pair:
            pair_close(ops.Pair(dst[:NSEQ * frames], count, got.fmt), want, 0, "dst (pair rows)")
        else:
            close(dst[:NSEQ * frames], want, 0, "dst")                         # test_layout_round_trip: a copy is exact


def test_btc_to_bct_far(arena):
    from vrdone_amd import _hip
    case = Fc.CASES["btc_to_bct"]
    B, Cw = case.nseq(), Fc.E
    g = torch.Generator().manual_seed(3)
    x_p = torch.randn(NSEQ * T, Cw, generator=g)
    x = arena.input("src", x_p.to(DEV), B * T)
    dst = arena.output("dst", B * T, Cw)                              # (B, C, T) contiguous: the same bytes as B * T rows of C
    ok(_hip.lib.vrd_btc_to_bct(p(x), Cw, B, Cw, T, p(dst), stream()), "vrd_btc_to_bct")
    arena.check({"dst": NSEQ * T})
    close(dst[:NSEQ * T].view(NSEQ, Cw, T), x_p.view(NSEQ, T, Cw).transpose(1, 2), 0, "dst")


def _pair_sources(seed):
    """period data of the three batching kernels: lengths, and which tracklet feeds the object half of pair p (p + 17 mod 61)"""
    lens_p = period_lens(seed)
    o_of = (torch.arange(NSEQ) + 17) % NSEQ
    return lens_p, lens_mask(lens_p), o_of


def _check_slab(got, want, fmt, what):
    from vrdone_amd import ops
    if fmt:
        pair_close(ops.Pair(got, got.shape[-1], fmt), want, 0, what + " (pair rows)")
    else:
        close(got, want, 0, what)                                              # a copy is exact (test_layout_round_trip)


@pytest.mark.parametrize("m", Fc.ALL)
def test_pack_pairs_far(m, arena):
    """vrd_pack_pairs: the outputs are the large buffers -- vis (2, P, T, 1024) crosses 2^31 elements, clip (2, P, T, 512) 2^32 bytes;
    the P source pointers name 61 small (T, C_in) matrices in turn"""
    from vrdone_amd import _hip, ops
    case = Fc.CASES["pack_pairs"]
    P, V, Cc, S, E = case.nseq() // 2, 1024, 512, 5, 8
    Cin = 2 * V + 2 * Cc + S + 2 * E
    lens_p, m_p, _ = _pair_sources(11)
    src = (torch.randn(NSEQ, T, Cin, generator=torch.Generator().manual_seed(12))).to(DEV)
    with use(m):
        fmt = ops.pair_fmt() if ops.pair_mode() else 0
        table = torch.tensor([src[i % NSEQ].data_ptr() for i in range(P)], dtype=torch.int64, device=DEV)
        lens = tiled(lens_p.to(torch.int32), P)
        vis, clip = arena.halves("vis", P * T, V), arena.halves("clip", P * T, Cc)
        ent, so_box = arena.halves("ent", P * T, E), arena.output("so_box", P * T, S)
        before = checksum(src.view(torch.int32))
        a = _hip.PackArgs()
        a.src, a.lens = table.data_ptr(), lens.data_ptr()
        a.P, a.C_in, a.T, a.V, a.Cc, a.S, a.E = P, Cin, T, V, Cc, S, E
        a.vis, a.clip, a.so_box, a.ent = p(vis), p(clip), p(so_box), p(ent)
        a.pair_wide = fmt
        ok(_hip.lib.vrd_pack_pairs(C.byref(a), stream()), "vrd_pack_pairs")
        arena.check({"vis": NSEQ * T, "clip": NSEQ * T, "ent": NSEQ * T, "so_box": NSEQ * T})
        assert checksum(src.view(torch.int32)) == before
        w = (src.cpu() * m_p[..., None]).reshape(NSEQ * T, Cin)
        n, h = NSEQ * T, P * T
        for side in (0, 1):
            _check_slab(vis[side * h:side * h + n], w[:, side * V:(side + 1) * V], fmt, f"vis half {side}")
            _check_slab(clip[side * h:side * h + n], w[:, 2 * V + side * Cc:2 * V + (side + 1) * Cc], fmt, f"clip half {side}")
            _check_slab(ent[side * h:side * h + n], w[:, 2 * V + 2 * Cc + S + side * E:2 * V + 2 * Cc + S + (side + 1) * E], 0, f"ent half {side}")
        _check_slab(so_box[:n], w[:, 2 * V + 2 * Cc:2 * V + 2 * Cc + S], 0, "so_box")


@pytest.mark.parametrize("m", Fc.ALL)
def test_gather_pairs_far(m, arena):
    """vrd_gather_pairs from 61 tracklets of 64 frames: the wide rows are copies (exact); the box features of the small buffers are
    held, bit for bit, to the same call on the first 61 pairs alone (tests/test_gpu_model.py checks their arithmetic)"""
    from vrdone_amd import _hip, ops
    case = Fc.CASES["gather_pairs"]
    P, V, Cc, S, E = case.nseq() // 2, 1024, 512, 5, 8
    lens_p, m_p, o_of = _pair_sources(13)
    g = torch.Generator().manual_seed(14)
    svis, sclip = torch.randn(NSEQ * T, V, generator=g).to(DEV), torch.randn(NSEQ * T, Cc, generator=g).to(DEV)
    xy = torch.rand(NSEQ * T, 2, generator=g) * 500
    boxes = torch.cat([xy, xy + 20 + torch.rand(NSEQ * T, 2, generator=g) * 200], dim=-1).contiguous().to(DEV)
    with use(m):
        fmt = ops.pair_fmt() if ops.pair_mode() else 0
        s_row = tiled(torch.arange(NSEQ, dtype=torch.int64) * T, P)
        o_row = tiled(o_of.to(torch.int64) * T, P)
        lens = tiled(lens_p.to(torch.int32), P)

        def call(n_pairs, vis, clip, so_box, ent):
            a = _hip.GatherArgs()
            a.vis, a.clip, a.boxes = p(svis), p(sclip), p(boxes)
            a.s_row, a.o_row, a.lens = p(s_row), p(o_row), p(lens)
            a.P, a.T, a.V, a.Cc, a.stride = n_pairs, T, V, Cc, 1
            a.w, a.h = 1280.0, 720.0
            a.out_vis, a.out_clip, a.out_so_box, a.out_ent = p(vis), p(clip), p(so_box), p(ent)
            a.pair_wide = fmt
            ok(_hip.lib.vrd_gather_pairs(C.byref(a), stream()), "vrd_gather_pairs")

        vis, clip = arena.halves("vis", P * T, V), arena.halves("clip", P * T, Cc)
        ent, so_box = arena.halves("ent", P * T, E), arena.output("so_box", P * T, S)
        before = [checksum(t.view(torch.int32)) for t in (svis, sclip, boxes)]
        call(P, vis, clip, so_box, ent)
        arena.check({"vis": NSEQ * T, "clip": NSEQ * T, "ent": NSEQ * T, "so_box": NSEQ * T})
        assert [checksum(t.view(torch.int32)) for t in (svis, sclip, boxes)] == before
        n, h = NSEQ * T, P * T
        small = [torch.empty(2 * n, V, device=DEV), torch.empty(2 * n, Cc, device=DEV), torch.empty(n, S, device=DEV), torch.empty(2 * n, E, device=DEV)]
        call(NSEQ, *small)
        live = m_p.reshape(n, 1)
        for side, src_seq in ((0, torch.arange(NSEQ)), (1, o_of)):
            rows = (src_seq[:, None] * T + torch.arange(T)[None]).reshape(-1)
            _check_slab(vis[side * h:side * h + n], svis.cpu()[rows] * live, fmt, f"vis half {side}")
            _check_slab(clip[side * h:side * h + n], sclip.cpu()[rows] * live, fmt, f"clip half {side}")
            assert W.bits_equal(ent[side * h:side * h + n], small[3][side * n:(side + 1) * n]), f"ent half {side}"
        assert W.bits_equal(so_box[:n], small[2]) and bool(torch.isfinite(small[2]).all()) and bool(torch.isfinite(small[3]).all())


def test_assemble_pairs_far(arena):
    """vrd_assemble_pairs: (2P, T, 512) rows from 61 per-tracklet streams and the window-edge pieces [subject start P | subject end P |
    object start P | object end P], every group periodic with data of its own"""
    from vrdone_amd import _hip
    case = Fc.CASES["assemble_pairs"]
    P, D = case.nseq() // 2, Fc.E
    L, piece, reach = (case.params[k] for k in ("L", "piece", "reach"))
    lens_p, m_p, o_of = _pair_sources(15)
    g = torch.Generator().manual_seed(16)
    streams = torch.randn(NSEQ * T, D, generator=g)
    groups = [torch.randn(NSEQ * L, D, generator=g) for _ in range(4)]
    sd = streams.to(DEV)
    raw = arena.take(4 * P * L, D)
    for i in range(4):
        part, per = raw[i * P * L:(i + 1) * P * L], groups[i].to(DEV).view(torch.int32)
        n = P * L // (NSEQ * L)
        part[:n * NSEQ * L].unflatten(0, (n, NSEQ * L)).copy_(per[None].expand(n, NSEQ * L, D))
        part[n * NSEQ * L:] = per[:P * L - n * NSEQ * L]
    arena.inputs.append(("snippets", raw, checksum(raw)))
    stream_row = torch.cat([tiled(torch.arange(NSEQ, dtype=torch.int64) * T, P), tiled(o_of.to(torch.int64) * T, P)])
    lens = tiled(lens_p.to(torch.int32), P)
    out = arena.halves("out", P * T, D)
    a = _hip.AssembleArgs()
    a.streams, a.snippets, a.stream_row, a.lens = p(sd), raw.data_ptr(), p(stream_row), p(lens)
    a.P, a.T, a.D, a.L, a.piece, a.reach = P, T, D, L, piece, reach
    a.out = p(out)
    before = checksum(sd.view(torch.int32))
    ok(_hip.lib.vrd_assemble_pairs(C.byref(a), stream()), "vrd_assemble_pairs")
    arena.check({"out": NSEQ * T})
    assert checksum(sd.view(torch.int32)) == before
    for side, src_seq in ((0, torch.arange(NSEQ)), (1, o_of)):
        want = torch.zeros(NSEQ, T, D)
        for q in range(NSEQ):
            n = int(lens_p[q])
            end_len = L if n == T else piece
            for t in range(n):
                if n <= piece or t < reach:
                    want[q, t] = groups[2 * side][q * L + t]
                elif t >= n - reach:
                    want[q, t] = groups[2 * side + 1][q * L + t - (n - end_len)]
                else:
                    want[q, t] = streams[int(src_seq[q]) * T + t]
        close(out[side * P * T:side * P * T + NSEQ * T], want.view(-1, D), 0, f"out half {side}")


# ------------------------------------------------------------------------------------------------------------------ the checker
def test_the_checker_sees_planted_changes(arena):
    """Arena.check on buffers of a case's size that torch filled: passes as built, and reports one changed far element, one row left
    as poison, a written guard row, and a changed input (no kernel of the library runs here)"""
    case = Fc.CASES["layernorm_512_plain"]
    R, P, Cw = case.rows(), NSEQ * T, Fc.E
    per = torch.randn(P, Cw, generator=torch.Generator().manual_seed(1)).to(DEV)
    x = arena.input("x", per, R)
    y = arena.output("y", R, Cw)
    n = R // P
    y[:n * P].unflatten(0, (n, P)).copy_(per[None].expand(n, P, Cw))
    y[n * P:] = per[:R - n * P]
    arena.check({"y": P})
    far = (1 << 32) // (Cw * 4) + 5
    keep = y[far, 3].clone()
    y[far, 3] += 1.0
    with pytest.raises(AssertionError, match=f"row {far} of"):
        arena.check({"y": P})
    y[far, 3] = keep
    y[R - 1].view(torch.int32).fill_(W.SENTINEL_BITS)
    with pytest.raises(AssertionError, match="poison"):
        arena.check({"y": P})
    y[R - 1] = per[(R - 1) % P]
    arena.check({"y": P})
    arena.outputs[0][1][R, 7] = 0
    with pytest.raises(AssertionError, match="guard rows"):
        arena.check({"y": P})
    arena.outputs[0][1][R, 7] = W.SENTINEL_BITS
    x[far, 0] += 1.0
    with pytest.raises(AssertionError, match="input x was written"):
        arena.check({"y": P})


# ------------------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("case,m", cases_for(*named("layernorm_")))
def test_layernorm_far(case, m, arena):
    from vrdone_amd import ops
    Cw, variant, pair = case.bufs[0].pitch, case.params["variant"], case.params["pair"]
    R, P = case.rows(), NSEQ * T
    g = torch.Generator().manual_seed(Cw + len(variant))
    x_p = torch.randn(P, Cw, generator=g) * 3 + 1
    x_p[5 * T + 9:6 * T] = 0                                                   # padded rows read 0
    gam, bet = torch.randn(1, Cw, 1, generator=g), torch.randn(1, Cw, 1, generator=g)
    pos = torch.randn(T, Cw, generator=g) if variant == "post_add" else None      # row r gets pos[r % 64]; 64 divides the period
    want = O.channel_ln(x_p.double().t()[None], gam.double(), bet.double())[0].t()
    if variant == "relu":
        want = torch.relu(want)
    if pos is not None:
        want = want + pos.double().repeat(NSEQ, 1)
    with use(m):
        x = arena.input("x", x_p.to(DEV), R)
        y = arena.output("y", R, Cw)
        got = ops.layernorm(x, gam.to(DEV), bet.to(DEV), relu=variant == "relu", post_add=dv(pos), out=y, pair=pair)
        arena.check({"y": P})
        if pair:
            pair_close(ops.Pair(y[:P], Cw, got.fmt), want, 3e-6, "y (pair rows)")
        else:
            close(y[:P], want, 3e-6, "y")                                      # test_layernorm_kernel_options


@pytest.mark.parametrize("name", named("conv_ln_"))
def test_conv_ln_far(name, arena):
    from vrdone_amd import ops
    case = Fc.CASES[name]
    Cin, ln, N = case.params["Cin"], case.params["ln"], Fc.E
    B = case.nseq()
    g = torch.Generator().manual_seed(Cin * 10 + N)
    m_p = lens_mask(period_lens(Cin))
    x_p = torch.randn(NSEQ, T, Cin, generator=g) * 3 * m_p[..., None]
    w = torch.randn(N, Cin, 3, generator=g) / (3 * Cin) ** 0.5
    b = torch.randn(N, generator=g) * 0.3
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    want = F.conv1d(x_p.double().transpose(1, 2), w.double(), b.double(), padding=1).transpose(1, 2) * m_p[..., None]
    if ln:
        mu = want.mean(-1, keepdim=True)
        var = ((want - mu) ** 2).mean(-1, keepdim=True)
        want = torch.relu((want - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double())
    x = arena.input("x", x_p.view(-1, Cin).to(DEV), B * T)
    y = arena.output("y", B * T, N)
    ops.conv_ln(rows3(x, T), w.to(DEV), b.to(DEV), row_mask=tiled(m_p, B), gamma=dv(gamma) if ln else None, beta=dv(beta) if ln else None,
                relu=ln, out=rows3(y, T))
    arena.check({"y": NSEQ * T})
    close(y[:NSEQ * T], want.reshape(-1, N), 2e-5 * max(1.0, float(want.abs().max())), "y")          # test_few_channel_conv_layernorm_row_kernel


@pytest.mark.parametrize("name", named("dwconv_ln_"))
def test_dwconv_ln_far(name, arena):
    from vrdone_amd import ops
    case = Fc.CASES[name]
    stride, gin, k, n_out, Cw, pre, up, with_ln, with_bias = Fc.DW_CASES[case.params["case"]]
    segs = case.params.get("segs", False)
    B = case.nseq()
    g = torch.Generator().manual_seed(len(name) + Cw)
    Cin = Cw * gin
    m_in = lens_mask(period_lens(len(name)))
    m_out = m_in[:, ::stride].contiguous()
    x_p = torch.randn(NSEQ, T, Cin, generator=g) * m_in[..., None]
    xu_p = torch.randn(NSEQ, T // 2, Cin, generator=g) * m_in[:, ::2, None] if up else None
    ws = [torch.randn(Cw, gin, k, generator=g) / (gin * k) ** 0.5 for _ in range(n_out)]
    bs = [torch.randn(Cw, generator=g) * 0.1 if with_bias else None for _ in range(n_out)]
    gs = [1 + 0.1 * torch.randn(1, Cw, 1, generator=g) if with_ln else None for _ in range(n_out)]
    es = [0.1 * torch.randn(1, Cw, 1, generator=g) if with_ln else None for _ in range(n_out)]
    pg, pb = 1 + 0.1 * torch.randn(1, Cin, 1, generator=g), 0.1 * torch.randn(1, Cin, 1, generator=g)
    xin = cl(x_p.double())
    if pre:
        xin = O.channel_ln(xin, pg.double(), pb.double())
    if up:
        xin = xin + cl(xu_p.double()).repeat_interleave(2, dim=2)
    wants = []
    for i in range(n_out):
        d = O.masked_conv1d(xin, m_in[:, None], ws[i].double(), None if bs[i] is None else bs[i].double(), stride=stride, groups=Cw)[0]
        if with_ln:
            d = O.channel_ln(d, gs[i].double(), es[i].double())
        wants.append(cl(d).reshape(-1, Cw))
    To = T // stride
    x = arena.input("x", x_p.view(-1, Cin).to(DEV), B * T)
    xu = arena.input("x_up", xu_p.view(-1, Cin).to(DEV), B * T // 2) if up else None
    ys = [arena.output(f"y{i}", B * To, Cw) for i in range(n_out)]
    shape = (lambda t, fr: t[None]) if segs else rows3
    sets = [dict(weight=dv(ws[i]), bias=dv(bs[i]), gamma=dv(gs[i]), beta=dv(es[i]), out=shape(ys[i], To)) for i in range(n_out)]
    mo = tiled(m_out, B)
    B1 = B // 2 + 1                                                            # two row groups; the second starts far out
    ops.dwconv_ln(shape(x, T), sets, mask_out=mo.reshape(1, -1) if segs else mo, stride=stride, x_up=None if xu is None else shape(xu, T // 2),
                  pre_ln=(pg.to(DEV), pb.to(DEV)) if pre else None, segs=[(0, B1, T), (B1 * T, B - B1, T)] if segs else None)
    arena.check({f"y{i}": NSEQ * To for i in range(n_out)})
    for i in range(n_out):
        # test_dwconv_ln_variants holds the kernel to 2e-5, test_dwconv_ln_input_layernorm (pre_ln) to 3e-5
        close(ys[i][:NSEQ * To], wants[i], 3e-5 if pre else 2e-5, f"y{i}")


def test_maxpool_mask_far(arena):
    from vrdone_amd import ops
    case = Fc.CASES["maxpool_mask"]
    B, Cw = case.nseq(), Fc.E
    g = torch.Generator().manual_seed(Cw)
    m_p = lens_mask(period_lens(7))
    x_p = torch.randn(NSEQ, T, Cw, generator=g) * m_p[..., None]
    want = F.max_pool1d(cl(x_p.double()), 3, 2, 1).transpose(1, 2) * m_p[:, ::2, None]
    x = arena.input("x", x_p.view(-1, Cw).to(DEV), B * T)
    y = arena.output("y", B * T // 2, Cw)
    m_out = torch.full((B, T // 2), True, device=DEV)
    md = tiled(m_p, B)
    ops.maxpool_mask(rows3(x, T), md, out=(rows3(y, T // 2), m_out))
    arena.check({"y": NSEQ * T // 2})
    close(y[:NSEQ * T // 2], want.reshape(-1, Cw), 0, "y")                     # test_maxpool_mask_kernel: exact
    assert torch.equal(m_out, md[:, ::2])


@pytest.mark.parametrize("name", named("activation_"))
def test_activation_far(name, arena):
    from vrdone_amd import _hip
    case = Fc.CASES[name]
    act, Cw, R, P = case.params["act"], case.bufs[0].pitch, case.rows(), NSEQ * T
    g = torch.Generator().manual_seed(len(act))
    x_p = torch.randn(P, Cw, generator=g) * 2
    want = (torch.relu if act == "relu" else F.gelu)(x_p.double())
    x = arena.input("x", x_p.to(DEV), R)
    y = arena.output("y", R, Cw)
    ok(_hip.lib.vrd_activation(p(x), Cw, None, 0, R, Cw, _hip.ACT_RELU if act == "relu" else _hip.ACT_GELU, p(y), Cw, stream()), "vrd_activation")
    arena.check({"y": P})
    rel_close(y[:P], want, 2e-5, "y")                                          # test_activation_windows


@pytest.mark.parametrize("name", named("local_attn_"))
def test_local_attention_far(name, arena):
    from vrdone_amd import _hip
    case = Fc.CASES[name]
    hd, hw, rel, segs = (case.params[k] for k in ("hd", "hw", "rel", "segs"))
    Cw, B = Fc.E, case.nseq()
    H = Cw // hd
    g = torch.Generator().manual_seed(hd + hw + int(rel))
    m_p = lens_mask(period_lens(hd + hw))
    q, k, v = (torch.randn(NSEQ, T, Cw, generator=g) * m_p[..., None] for _ in range(3))
    rel_pe = torch.randn(1, 1, H, 2 * hw + 1, generator=g) if rel else None
    want = cl(O.banded_attention(cl(q.double()), cl(k.double()), cl(v.double()), m_p[:, None], H, hw, rel_pe=None if rel_pe is None else rel_pe.double()))
    qkv = arena.input("qkv", torch.cat([q, k, v], dim=-1).view(-1, 3 * Cw).to(DEV), B * T)
    out = arena.output("out", B * T, Cw)
    md, rd = tiled(m_p, B), dv(rel_pe)
    qv, kv, vv = (qkv[:, i * Cw:(i + 1) * Cw] for i in range(3))
    if segs:
        B1 = B // 2 + 1
        table = _hip.RowSegs.of([(0, B1, T), (B1 * T, B - B1, T)])
        ok(_hip.lib.vrd_local_attn_segs(p(qv), p(kv), p(vv), 3 * Cw, p(md), p(rd), C.byref(table), Cw, H, hw, p(out), Cw, 0, stream()),
           "vrd_local_attn_segs")
    else:
        ok(_hip.lib.vrd_local_attn(p(qv), p(kv), p(vv), 3 * Cw, p(md), p(rd), B, T, Cw, H, hw, p(out), Cw, 0, stream()), "vrd_local_attn")
    arena.check({"out": NSEQ * T})
    close(out[:NSEQ * T], want.reshape(-1, Cw), 2e-5, "out")                   # test_local_attention_kernel / test_local_attention_windows


# ------------------------------------------------------------------------------------------------------------------- GEMM
def _family_of(case):
    from vrdone_amd import _hip
    return getattr(_hip, case.body)


def _gemm(family, *args, **kwargs):
    """ops.conv_gemm(*args, **kwargs) on plain tensors; `family` receives the kernel family the library runs the call on"""
    from vrdone_amd import ops
    a, result = ops.gemm_args(*args, **kwargs)
    family.append(ops.gemm_family(a))
    ops.launch_gemm(a)
    return result


@pytest.mark.parametrize("case,m", cases_for(*[n for n in named("gemm_") if "mlp" not in n]))
def test_gemm_far(case, m, arena):
    """512 -> 512, k = 1 / 3, mask * scale + two residuals; x, res, res2 and out each at their own pitch"""
    from vrdone_amd import ops
    k, pair_in = case.params["k"], case.params["pair_in"]
    Ts, B, Cin, N = case.seq_len, case.nseq(), Fc.E, Fc.E
    P = NSEQ * Ts
    g = torch.Generator().manual_seed(k + 2 * pair_in + Ts)
    m_p = lens_mask(period_lens(k + Ts, Ts), Ts)
    x_p = torch.randn(NSEQ, Ts, Cin, generator=g) * m_p[..., None]
    w = torch.randn(N, Cin, k, generator=g) / (Cin * k) ** 0.5
    bias, scale = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
    res_p, res2_p = torch.randn(P, N, generator=g), torch.randn(P, N, generator=g)
    mk = m_p.double().reshape(P, 1)
    y = F.conv1d(x_p.double().transpose(1, 2), w.double(), bias.double(), padding=k // 2).transpose(1, 2).reshape(P, N)
    want = y * mk * scale.double() + res_p.double() * mk + res2_p.double()
    pitches = {b.name: b.pitch for b in case.bufs}
    with use(m):
        fmt = ops.pair_fmt()
        xin = to_pair(x_p.view(P, Cin).to(DEV), fmt) if pair_in else x_p.view(P, Cin).to(DEV)
        x = arena.input("x", xin, B * Ts, pitches["x"])
        res = arena.input("res", res_p.to(DEV), B * Ts, pitches["res"])
        res2 = arena.input("res2", res2_p.to(DEV), B * Ts, pitches["res2"])
        out = arena.output("out", B * Ts, N, pitches["out"])
        xv = rows3(x, Ts)
        family = []
        _gemm(family, ops.Pair(xv, Cin, fmt) if pair_in else xv, w.to(DEV), bias.to(DEV), row_mask=tiled(m_p, B), scale=scale.to(DEV),
              res=rows3(res, Ts), res_masked=True, res2=rows3(res2, Ts), out=rows3(out, Ts))
        assert family[0] == _family_of(case), f"the call ran kernel family {family[0]}, the case is built for {case.body}"
        arena.check({"out": P})
        scale_tol = 5.0 if m == "bf16x3" else 1.0                              # tests/test_gpu_ops.py GEMM_TOL_SCALE
        close(out[:P], want, (2e-5 if pair_in else 3e-5) * scale_tol, "out")     # test_gemm_large_tile_kernels / test_gemm_shapes_and_epilogue


@pytest.mark.parametrize("case,m", cases_for("gemm_mlp_f32", "gemm_mlp_split"))
def test_gemm_mlp_far(case, m, arena):
    """the up-projection (512 -> 2048, GELU, pair rows out in the split modes) and the down-projection (2048 -> 512, mask, scale,
    residual) as the transformer block calls them, chained through ONE hidden buffer that crosses 2^32 elements"""
    from vrdone_amd import ops
    B, Cw, Hd, P = case.nseq(), Fc.E, Fc.H, NSEQ * T
    g = torch.Generator().manual_seed(77)
    m_p = lens_mask(period_lens(77))
    x_p = torch.randn(NSEQ, T, Cw, generator=g) * m_p[..., None]
    w1, b1 = torch.randn(Hd, Cw, 1, generator=g) / Cw ** 0.5, torch.randn(Hd, generator=g)
    w2, b2 = torch.randn(Cw, Hd, 1, generator=g) / Hd ** 0.5, torch.randn(Cw, generator=g)
    scale = torch.rand(Cw, generator=g) + 0.5
    res_p = torch.randn(P, Cw, generator=g)
    want_h = F.gelu(x_p.double().view(P, Cw) @ w1[..., 0].double().t() + b1.double())
    with use(m):
        fmt, pair = ops.pair_fmt(), case.params["pair"]
        xin = to_pair(x_p.view(P, Cw).to(DEV), fmt) if pair else x_p.view(P, Cw).to(DEV)
        x = arena.input("x", xin, B * T)
        hid = arena.output("hidden", B * T, Hd)
        out = arena.output("out", B * T, Cw)
        res = arena.input("res", res_p.to(DEV), B * T)
        md = tiled(m_p, B)
        xv, fam = rows3(x, T), []
        h = _gemm(fam, ops.Pair(xv, Cw, fmt) if pair else xv, w1.to(DEV), b1.to(DEV), act=ops.ACT_GELU, out=rows3(hid, T), out_pair=pair,
                  skip_rows=md)
        _gemm(fam, h, w2.to(DEV), b2.to(DEV), row_mask=md, scale=scale.to(DEV), res=rows3(res, T), out=rows3(out, T))
        assert fam == [_family_of(case)] * 2, f"the calls ran kernel families {fam}, the case is built for {case.body}"
        arena.check({"hidden": P, "out": P})
        scale_tol = 5.0 if m == "bf16x3" else 1.0                              # tests/test_gpu_ops.py GEMM_TOL_SCALE
        valid = m_p.reshape(P)                                                 # skip_rows: padded row blocks hold bias-only filler
        if pair:
            pair_close(ops.Pair(hid[:P][valid.to(DEV)], Hd, fmt), want_h[valid], 2e-5 * scale_tol, "hidden (pair rows)")     # test_gemm_large_tile_kernels
            h0 = ops.Pair(hid[:P], Hd, fmt).float().double().cpu()
        else:
            close(hid[:P][valid.to(DEV)], want_h[valid], 3e-5, "hidden")       # test_gemm_shapes_and_epilogue (130 x 2048 x 512)
            h0 = hid[:P].double().cpu()
        mk = m_p.double().reshape(P, 1)
        want = (h0 @ w2[..., 0].double().t() + b2.double()) * mk * scale.double() + res_p.double()
        close(out[:P], want, (2e-5 if pair else 3e-5) * scale_tol, "out")


# ------------------------------------------------------------------------------------------------------ global attention
def _attention_inputs(hd, seed):
    Cw = Fc.E
    g = torch.Generator().manual_seed(seed)
    km = lens_mask(period_lens(seed))
    q = torch.randn(NSEQ, T, Cw, generator=g) * 2.0
    k, v = (torch.randn(NSEQ, T, Cw, generator=g) * km[..., None] for _ in range(2))
    k[:, 50, :hd] = q[:, 5, :hd] * 2.0 * km[:, 50, None]                       # a dominant late key: the running-max rescale
    want = cl(O.full_attention(cl(q.double()), cl(k.double()), cl(v.double()), km[:, None], Cw // hd))
    return km, q, k, v, want.reshape(-1, Cw)


def test_attention_flash_far(arena):
    """vrd_attention algo 2 on f32 rows; k and v are slabs of one 1536-wide row"""
    from vrdone_amd import ops
    case = Fc.CASES["attention_flash_f32rows"]
    hd, Cw, B, P = case.params["hd"], Fc.E, case.nseq(), NSEQ * T
    km, q, k, v, want = _attention_inputs(hd, 41)
    with use("f32"):
        qd = arena.input("q", q.view(P, Cw).to(DEV), B * T)
        kv = arena.input("kv", torch.cat([k, v], dim=-1).view(P, 2 * Cw).to(DEV), B * T, 3 * Cw)
        out = arena.output("out", B * T, Cw)
        ops.attention(rows3(qd, T), rows3(kv[:, :Cw], T), rows3(kv[:, Cw:], T), tiled(km, B), Cw // hd, algo=2, out=rows3(out, T))
        arena.check({"out": P})
        close(out[:P], want, 3e-5, "out")                                      # test_global_attention_kernels / test_global_attention_windows


@pytest.mark.parametrize("case,m", cases_for(*named("attention_pair_")))
def test_attention_pair_far(case, m, arena, monkeypatch):
    """both split-precision flash kernels on pair rows at every head size each supports; k and v slabs of one 1536-wide row"""
    from vrdone_amd import ops
    hd, w64 = case.params["hd"], case.params["w64"]
    monkeypatch.setenv("VRD_FLASH_W64", str(w64))                              # read per call (vrd_attention_pair)
    Cw, B, P = Fc.E, case.nseq(), NSEQ * T
    km, q, k, v, want = _attention_inputs(hd, 43 + hd)
    with use(m):
        fmt = ops.pair_fmt()
        qp, kp, vp = (to_pair(t.view(P, Cw).to(DEV), fmt) for t in (q, k, v))
        qd = arena.input("q", qp, B * T)
        kv = arena.input("kv", torch.cat([kp, vp], dim=-1), B * T, 3 * Cw)
        out = arena.output("out", B * T, Cw)
        pr = lambda t: ops.Pair(rows3(t, T), Cw, fmt)          # noqa: E731
        ops.attention(pr(qd), pr(kv[:, :Cw]), pr(kv[:, Cw:]), tiled(km, B), Cw // hd, out=rows3(out, T))
        arena.check({"out": P})
        close(out[:P], want, 2e-4, "out")                                      # test_flash_attention_pair_rows' bound


@pytest.mark.parametrize("m", Fc.SPLIT)
def test_attention_pair_slab_beyond_2gib_takes_the_other_kernel(m, arena, monkeypatch):
    """A leading dimension at which ONE batch item's K / V slab reaches 2 GiB: the 64-queries-per-wave kernel's LDS-DMA offsets are
    32-bit, vrd_attention_pair has to run the other flash kernel (whose result the same call on compact rows gives bit for bit, with
    the switch forcing it there), and the second item, whose rows start behind the line, has to be right."""
    from vrdone_amd import _hip, ops
    kk = Fc.SLAB_FALLBACK
    B, Tq, Tk, hd, H, ld = kk["B"], kk["Tq"], kk["Tk"], kk["hd"], kk["heads"], kk["ldkv"]
    Cw = H * hd
    assert Tk * ld * 4 >= 1 << 31
    g = torch.Generator().manual_seed(5)
    km = lens_mask(torch.tensor([Tk, Tk // 3]), Tk)
    q = torch.randn(B, Tq, Cw, generator=g) * 2.0
    k, v = (torch.randn(B, Tk, Cw, generator=g) * km[..., None] for _ in range(2))
    want = cl(O.full_attention(cl(q.double()), cl(k.double()), cl(v.double()), km[:, None], H))
    with use(m):
        fmt = ops.pair_fmt()
        qp, kp, vp = (to_pair(t.to(DEV), fmt) for t in (q, k, v))
        raw = arena.take(B * Tk, ld)
        raw[:, :2 * Cw] = torch.cat([kp, vp], dim=-1).view(B * Tk, 2 * Cw).view(torch.int32)
        before = checksum(raw)
        kv = raw.view(torch.float32)
        out = arena.output("out", B * Tq, Cw)
        kd = km.to(DEV)
        monkeypatch.setenv("VRD_FLASH_W64", "1")
        ok(_hip.lib.vrd_attention_pair(p(qp), Cw, p(kv), p(kv[:, Cw:]), ld, p(kd), None, B, Tq, Tk, H, hd, p(out), Cw, 0, fmt, stream(),
                                       ops.products()), "vrd_attention_pair")
        monkeypatch.setenv("VRD_FLASH_W64", "0")
        plain = ops.attention(ops.Pair(qp, Cw, fmt), ops.Pair(kp, Cw, fmt), ops.Pair(vp, Cw, fmt), kd, H)
        torch.cuda.synchronize()
        assert checksum(raw) == before and bool((arena.outputs[0][1][B * Tq:] == W.SENTINEL_BITS).all())
        close(out.view(B, Tq, Cw), want, 2e-4, "out")                          # test_flash_attention_pair_rows' bound
        assert W.bits_equal(out.view(B, Tq, Cw), plain), "the call did not run the 32-queries-per-wave kernel"
