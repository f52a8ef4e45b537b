"""vrd_dwconv_ln_multi on a real MI355X: up to five depthwise-conv + LayerNorm sets from one pass over a stream of rows.

The entry point promises the BITS of today's launches: every output set equals, bit for bit, the vrd_dwconv_ln call with that
set's parameters on the raw rows (pre_ln = 0) or behind the input LayerNorm (pre_ln = 1) -- whatever the number of sets sharing
the pass, the output format (f32 rows, bf16 or f16 pair rows) and the layout (B sequences of T frames, or a ragged row space).
All operands sit in strided windows with poisoned guard bands (tests/window_cases.py): nothing outside a window may be written.
Model level: with the threshold forced to 0 the `vidvrd` predictions are the default route's, and the `dwconv_ln` family loses
exactly two launches per stream and stage (one launch of five sets) or one (two launches)."""
import pytest
import torch

import window_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
CW, B = 512, 3
# sets of the pass: (reads normalised rows, has LayerNorm, has bias, ReLU, pair rows in the split modes); the first three are a
# stream's own q / k (behind ln1) and v, the last two the other layer's k / v -- here one of them without LayerNorm and one
# writing f32 rows in every mode, so that both output formats and both tails of a set run next to each other
SETS = [(True, True, False, False, True), (True, True, False, False, False), (False, True, False, False, True),
        (False, False, True, True, True), (False, True, True, True, False)]
PICKS = {2: [2, 0], 3: [0, 1, 2], 5: [0, 1, 2, 3, 4]}          # which of them a pass of n sets takes (raw and normalised mixed)


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


def _lens(T):
    """sequence 0 full, sequence 1 fully padded, sequence 2 a few valid frames: from T = 17 on its strips behind the first
    (rows 16 ..) are padding only"""
    return [T, 0, max(1, min(5, T // 2))]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    sets = []
    for normed, ln, bias, relu, pair in SETS:
        sets.append(dict(weight=(torch.randn(CW, 1, 3, generator=g) / 3 ** 0.5).to(DEV),
                         bias=(torch.randn(CW, generator=g) * 0.1).to(DEV) if bias else None,
                         gamma=(1 + 0.1 * torch.randn(CW, generator=g)).to(DEV) if ln else None,
                         beta=(0.1 * torch.randn(CW, generator=g)).to(DEV) if ln else None, relu=relu, pair=pair, normed=normed))
    pre = ((1 + 0.1 * torch.randn(CW, generator=g)).to(DEV), (0.1 * torch.randn(CW, generator=g)).to(DEV))
    return sets, pre


def _raw(t):
    from vrdone_amd import ops
    return t.t if isinstance(t, ops.Pair) else t


def _today(x, sets, mask, pre, segs=None):
    """the reference: one vrd_dwconv_ln launch per set, on contiguous tensors"""
    from vrdone_amd import ops
    outs = []
    for s in sets:
        st = {k: v for k, v in s.items() if k != "normed"}
        outs.append(_raw(ops.dwconv_ln(x, [st], mask_out=mask, pre_ln=pre if s["normed"] else None, segs=segs)[0]))
    return outs


def _case(T_or_segs, precision):
    """(x window, mask, sets, pre, today's outputs, segs) of one layout, made once per (layout, precision)"""
    key = (str(T_or_segs), precision)
    if key not in _case.made:
        segs = T_or_segs if isinstance(T_or_segs, list) else None
        g = torch.Generator().manual_seed(7 + len(key[0]))
        if segs:
            frames = [T for _, cnt, T in segs for _ in range(cnt)]
            lens = [17, 3, 0, 20][:len(frames)]          # full | its second strip padding only | padded | its third strip padding only
            assert len(frames) == 4 and all(n <= T for n, T in zip(lens, frames))
            mask = torch.cat([torch.arange(T) < n for n, T in zip(lens, frames)])[None]
        else:
            mask = torch.arange(T_or_segs)[None, :] < torch.tensor(_lens(T_or_segs))[:, None]
        x = torch.randn(*mask.shape, CW, generator=g) * mask[..., None]          # (padded rows are zeros, as their producers leave them)
        sets, pre = _params(11)
        xd, md = x.to(DEV), mask.to(DEV)
        _case.made[key] = (xd, md, sets, pre, _today(xd, sets, md, pre, segs), segs)
    return _case.made[key]


_case.made = {}


def _check_pass(T_or_segs, n, precision):
    from vrdone_amd import ops
    xd, md, sets, pre, today, segs = _case(T_or_segs, precision)
    lds = W.LdSeq()
    rows = xd.shape[0] * xd.shape[1]
    # (windows of the rows as a matrix; the (sequences, frames, C) operand is that window with its strides spelled out -- a
    # one-frame axis has no stride of its own to read the row pitch from)
    seq = lambda h: torch.as_strided(h.buf, xd.shape, (xd.shape[1] * h.ld, h.ld, 1), h.offset)          # noqa: E731
    hx = W.embed(xd.reshape(rows, CW), ld=lds(CW), name="x")
    hys = [W.embed_out((rows, CW), DEV, ld=lds(CW), name=f"y{i}") for i in PICKS[n]]
    assert len({h.ld for h in [hx] + hys}) == n + 1
    got = ops.dwconv_ln_multi(seq(hx), [dict(sets[i], out=seq(h)) for i, h in zip(PICKS[n], hys)], mask_out=md, pre_ln=pre, segs=segs)
    torch.cuda.synchronize()
    for i, h, out in zip(PICKS[n], hys, got):
        is_pair = isinstance(out, ops.Pair)
        assert is_pair == (sets[i]["pair"] and precision != "f32")
        W.assert_guards_intact(h)
        if not is_pair:
            W.assert_written_and_finite(h)
        assert W.bits_equal(h.view, today[i].reshape(rows, CW)), f"set {i} of a pass of {n} ({precision}, {T_or_segs}) differs from today's launch"
    W.assert_unchanged(hx)


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 33])
def test_bits_of_todays_launches(T, n, precision):
    """sequence ends at every T, the strip boundary at 16 rows, a fully padded sequence, padding-only strips behind valid frames"""
    _check_pass(T, n, precision)


@pytest.mark.parametrize("n", [3, 5])
def test_bits_of_todays_launches_row_groups(n, precision):
    """a ragged row space: two sequences of 17 frames, then two of 33"""
    _check_pass([(0, 2, 17), (34, 2, 33)], n, precision)


def test_f16_range_flag():
    """a pair-row set fed a value beyond the f16 planes' range ORs the LayerNorm tag (2) into the range word; the twin in range,
    and the same value into an f32 set, leave it clear"""
    from vrdone_amd import ops
    old = ops.get_precision()
    ops.set_precision("f16x3")
    try:
        w = torch.zeros(CW, 1, 3, device=DEV)
        w[:, 0, 1] = 1.0                                    # the identity: out = x
        for value, pair, want in ((8192.0, True, 2), (2048.0, True, 0), (8192.0, False, 0)):
            x = torch.zeros(1, 17, CW, device=DEV)
            x[0, 16, 300] = value
            ops.f16_range_flag().zero_()
            quiet = dict(weight=w, pair=True, normed=True)   # a normalised neighbour: in range whatever the input
            out = ops.dwconv_ln_multi(x, [quiet, dict(weight=w, pair=pair)], pre_ln=(torch.ones(CW, device=DEV), torch.zeros(CW, device=DEV)))[1]
            got = ops.f16_range_exceeded()
            assert got == want, (value, pair, got, ops.describe_range(got))
            if want == 0:
                val = out.float() if isinstance(out, ops.Pair) else out
                assert float(val[0, 16, 300]) == value and float(val.abs().sum()) == value
    finally:
        ops.f16_range_flag().zero_()
        ops.set_precision(old)


def _mask_vrd_runs(lens, T, rows_form):
    from test_gpu_model import get_model, c_in
    from oracle import vrd_oracle as O
    model, mc, _, _ = get_model("vidvrd")
    x, m = O.synth_pairs(len(lens), c_in(mc), T, lens, seed=41)
    xd, md = x.to(DEV), m.to(DEV)

    def run():
        try:
            if rows_form:
                model.ROWS_MIN_ROWS = 64
            plan = model._tight_plan(md, md.reshape(len(lens), T))
            assert bool(plan and plan["rows"]) == rows_form, plan
            return model._mask_vrd(xd, md, with_aux=False)
        finally:
            model.__dict__.pop("ROWS_MIN_ROWS", None)
    return model, run


@pytest.mark.parametrize("layout", ["batch", "rows"])
def test_model_predictions_and_launch_counts(layout, monkeypatch):
    """`vidvrd` _mask_vrd on a 4-pair batch and on a ragged 6-pair batch (row space): the merged routes give the default route's
    predictions exactly; the dwconv_ln family loses two launches per stream and stage in form c, one in form b; at the default
    threshold the route is today's"""
    from test_gpu_f16_range import launches
    from vrdone_amd.models import backbones
    lens, rows_form = ([96, 60, 17, 2], False) if layout == "batch" else ([5, 17, 24, 40, 95, 96], True)
    model, run = _mask_vrd_runs(lens, 96, rows_form)
    stages = len(model.backbone.s_attn)
    assert stages >= 1 and backbones.SOS_MERGE_MIN_ROWS > 6 * 96
    want = run()
    base, = launches(run, "dwconv_ln")
    for form, fewer in (("c", 2), ("b", 1)):
        monkeypatch.setattr(backbones, "SOS_MERGE_MIN_ROWS", 0)
        monkeypatch.setattr(backbones, "SOS_MERGE_FORM", form)
        got = run()
        n, = launches(run, "dwconv_ln")
        assert n == base - fewer * 2 * stages, (form, n, base, stages)
        assert set(got) == set(want)
        for k in want:
            if torch.is_tensor(want[k]):
                assert W.bits_equal(got[k], want[k]), (form, k)
        monkeypatch.undo()
    again, = launches(run, "dwconv_ln")
    assert again == base
