"""Host side of eval batching (vrdone_amd/models/eval_batches.py): the bucket plan -- runs of one padded length, launch waves,
filler buckets, the pair order of a call.  No GPU and no built library: the module imports `ops` only when a driver runs."""
import pytest
import torch

from vrdone_amd.models import eval_batches as E
from vrdone_amd.models import ragged
from vrdone_amd.models.eval_batches import Bucket


def _positions(sel):
    return sel.tolist() if isinstance(sel, torch.Tensor) else list(sel)


PLANS = {
    "one": [(64, 10, True)],
    "three": [(32, 5, True), (64, 7, True), (96, 1, False)],
    "long": [(32, 1, True), (64, 40, True), (96, 2, True), (96, 3, False)],
}


@pytest.mark.parametrize("plan,step", [("one", 4),          # a bucket across three waves
                                       ("one", 10), ("one", 11), ("three", 5), ("three", 6), ("three", 1),
                                       ("three", 100),       # a step larger than the total
                                       ("long", 13),         # the 40-pair bucket across four waves
                                       ("long", 46), ("long", 23)])
def test_waves_cut_every_bucket_list_into_full_waves(plan, step):
    """Every position once, every wave but the last holds exactly `step` pairs, the pieces keep T and flat, and a range and a
    tensor `sel` give the same cuts."""
    shape = PLANS[plan]
    total = sum(n for _, n, _ in shape)
    as_range, as_tensor, at = [], [], 0
    for T, n, flat in shape:
        as_range.append(Bucket(T, range(at, at + n), n, flat))
        as_tensor.append(Bucket(T, torch.arange(at, at + n, dtype=torch.int32), n, flat))
        at += n
    of = {p: (b.T, b.flat) for b in as_range for p in b.sel}
    got_r, got_t = E.waves(as_range, step), E.waves(as_tensor, step)
    assert len(got_r) == len(got_t) == -(-total // step)
    if plan == "one" and step == 4:
        assert [[b.n for b in w] for w in got_r] == [[4], [4], [2]]
    seen = []
    for wave_r, wave_t in zip(got_r, got_t):
        assert [(b.T, b.n, b.flat) for b in wave_r] == [(b.T, b.n, b.flat) for b in wave_t]
        for b, bt in zip(wave_r, wave_t):
            assert isinstance(b.sel, range) and isinstance(bt.sel, torch.Tensor) and bt.sel.dtype == torch.int32
            assert _positions(b.sel) == _positions(bt.sel) and len(b.sel) == b.n > 0
            assert all(of[p] == (b.T, b.flat) for p in b.sel)
            seen += _positions(b.sel)
    assert seen == list(range(total))               # every position exactly once, in order
    sizes = [sum(b.n for b in w) for w in got_r]
    assert all(s == step for s in sizes[:-1]) and 0 < sizes[-1] <= step


def test_runs_split_by_padded_length_and_by_flat():
    """`flat` is true exactly for lens <= T - 2, the non-flat run of a padded length follows its flat one, and without `lens`
    there is one run per padded length."""
    lens = [5, 30, 31, 32, 17, 62, 63, 64, 40, 96, 20, 94]
    t_pad = [32, 32, 32, 32, 32, 64, 64, 64, 64, 96, 96, 96]
    ids = sorted(range(len(lens)), key=lambda i: (t_pad[i], lens[i], i))
    got = E.runs(ids, t_pad, lens)
    assert [(b.T, b.n, b.flat) for b in got] == [(32, 3, True), (32, 2, False), (64, 2, True), (64, 2, False), (96, 2, True), (96, 1, False)]
    at = 0
    for b in got:
        assert b.sel == range(at, at + b.n)
        assert all((lens[ids[p]] <= b.T - 2) == b.flat and t_pad[ids[p]] == b.T for p in b.sel)
        at += b.n
    assert at == len(ids)
    plain = E.runs(ids, t_pad)
    assert [(b.T, b.sel) for b in plain] == [(32, range(0, 5)), (64, range(5, 9)), (96, range(9, 12))]
    # a padded length whose pairs are all of one kind is one run; nothing to plan, nothing planned
    assert [(b.T, b.n, b.flat) for b in E.runs([0, 1], [32, 32], [31, 32])] == [(32, 2, False)]
    assert [(b.T, b.n, b.flat) for b in E.runs([0, 1], [32, 32], [3, 30])] == [(32, 2, True)]
    assert E.runs([], [], []) == []


@pytest.mark.parametrize("rows", [65536, 65536 + 32, 65536 + 48, 317344, 311104, 23792 * 4, 100000, 4096 + 32])
def test_add_filler_puts_the_filler_behind_the_last_flat_bucket(rows):
    """Flat buckets first, fillers directly behind the last flat one, and the row total is a multiple of 256 exactly when
    ragged.filler_buckets returns something (the row counts of test_row_space_layout_and_filler_buckets)."""
    t_tail = 32 + rows % 32 if rows % 32 else 64                  # one odd bucket carries what is no multiple of 32
    body = rows - t_tail - 3 * 96
    assert body > 0 and body % 32 == 0
    wave = [Bucket(96, range(0, 2), 2, False), Bucket(32, range(2, 2 + body // 32), body // 32, True), Bucket(96, range(0, 1), 1, False),
            Bucket(t_tail, range(0, 1), 1, True)]
    assert sum(b.n * b.T for b in wave) == rows
    got = E.add_filler(list(wave), 288)
    fill = ragged.filler_buckets(rows, 288)
    flat = [b.flat for b in got]
    assert flat == sorted(flat, reverse=True)
    assert [b for b in got if b.sel is not None] == [wave[1], wave[3], wave[0], wave[2]]          # stable within each kind
    n_flat = 2
    assert [(b.n, b.T) for b in got[n_flat:n_flat + len(fill)]] == fill
    assert all(b.sel is None and b.flat for b in got[n_flat:n_flat + len(fill)]) and len(got) == len(wave) + len(fill)
    total = sum(b.n * b.T for b in got)
    assert (total % 256 == 0) == (bool(fill) or rows % 256 == 0)          # (65536 rows are a multiple without any)
    assert bool(fill) == (rows % 256 != 0 and rows >= 65536)
    ragged.Layout([(b.n, b.T, b.flat) for b in got])                # (asserts the flat buckets come first)
    if rows % 32:                                  # no room for the 32 + 16-frame sequence in a batch of 40 frames: no filler
        assert E.add_filler(list(wave), 40) == [wave[1], wave[3], wave[0], wave[2]]


def test_eval_plan_and_the_multi_video_order_agree_on_one_video():
    """MaskVRD.eval_plan is eval_batches.pair_order under the video's reference padded lengths: what forward_test_videos
    computes for a call of that one video."""
    from conftest import load_case
    from vrdone_amd.models.maskvrd import MaskVRD
    mc, _, _ = load_case("vidvrd")
    model = MaskVRD(mc, device="cpu").eval()
    g = torch.Generator().manual_seed(21)
    lens = torch.randint(2, 400, (300,), generator=g).tolist()
    model.ROWS_MIN_ROWS = 2048
    for min_pairs in (8, 1 << 20):                   # the row-space form's finer buckets, and the bucket-by-bucket policy
        model.ROWS_MIN_PAIRS = min_pairs
        order, t_pad = model.eval_plan(lens)
        assert (order, t_pad) == E.pair_order(model, lens, model._reference_pad(lens))
        assert sorted(order) == list(range(len(lens))) and len(set(t_pad)) > 1
        assert [(t_pad[i], lens[i], i) for i in order] == sorted((t_pad[i], lens[i], i) for i in range(len(lens)))
        assert t_pad == model.tight_buckets(lens, model._reference_pad(lens), 2048 if min_pairs == 8 else None)
