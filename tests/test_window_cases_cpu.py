"""The window checker of tests/window_cases.py against Python stand-ins of a row op that address flat memory through
(offset, leading dimension) like a kernel of the C ABI does: a correct one passes, and each planted fault -- the classes
tests/test_gpu_windows.py exists to catch -- is reported.  No GPU, and no wrong kernel is ever run on one."""
import pytest
import torch

import window_cases as W

ROWS, C = 7, 12


def standin(x, ldx, xoff, y, ldy, yoff, mask, rows, cols, fault=None):
    """y[r, c] = (2 x[r, c] + 1) * mask[r] on flat buffers, element (r, c) at off + r * ld + c."""
    if fault == "ignores_ld":
        ldy = cols                                   # the row width where the leading dimension belongs
    for r in range(rows):
        for c in range(cols):
            if fault == "unwritten" and r == rows - 1 and c == cols - 1:
                continue
            v = 2.0 * x[xoff + r * ldx + c] + 1.0
            if fault == "reads_guard_times_zero" and c == cols - 1:
                v = v + x[xoff + r * ldx + cols] * 0.0                   # one element past the row: load, then multiply by a zero mask
            y[yoff + r * ldy + c] = v * mask[r]
    if fault == "past_last_row":
        y[yoff + rows * ldy] = 0.0                   # a partial tile that stores one row too many
    if fault == "left_of_c0":
        y[yoff + 3 * ldy - 1] = 0.0
    if fault == "own_nan_in_guard":
        y[yoff + cols] = float("nan")                # a NaN, but not the sentinel's bits


def run(fault, poison=W.POISON):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(ROWS, C, generator=g)
    mask = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    lds = W.LdSeq()
    hx = W.embed(x, ld=lds(C), poison=poison, name="x")
    hy = W.embed_out((ROWS, C), "cpu", ld=lds(C), name="y")
    assert hx.ld != hy.ld and hx.ld != C and hy.ld != C
    standin(hx.flat, hx.ld, hx.offset, hy.flat, hy.ld, hy.offset, mask, ROWS, C, fault)
    W.check([hy], [hx])
    want = (2.0 * x + 1.0) * mask[:, None]
    assert torch.equal(hy.result(), want)
    return hy


def test_the_sentinel_is_a_quiet_nan_with_a_payload():
    s = W.sentinel()
    assert bool(torch.isnan(s))
    bits = int(s.view(torch.int32))
    assert bits == W.SENTINEL_BITS and bits & 0x7FC00000 == 0x7FC00000 and bits & 0x3FFFFF != 0
    assert bits != int(torch.tensor(float("nan")).view(torch.int32))         # not the NaN arithmetic produces


def test_embed_layout_and_defaults():
    t = torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(2, 3, 8)
    h = W.embed(t)
    assert h.buf.shape == (2 + 6 + 3, 8 + 64) and h.c0 == 32 and h.view.shape == t.shape
    assert h.view.stride() == (3 * 72, 72, 1) and h.view.data_ptr() % 16 == h.buf.data_ptr() % 16
    assert torch.equal(h.view, t)
    assert int((h.buf.view(torch.int32) == W.SENTINEL_BITS).sum()) == h.buf.numel() - t.numel()
    assert float(h.flat[h.offset + 4 * h.ld + 5]) == float(t[1, 1, 5])
    o = W.embed_out((6, 8), "cpu")
    assert bool((o.buf.view(torch.int32) == W.SENTINEL_BITS).all())
    # bit patterns that are not numbers survive the trip (pair rows are 16-bit planes in f32 clothing)
    odd = torch.tensor([[0x7F800001, -1, 0x00000001, 0x7FC5A5A5]], dtype=torch.int32).view(torch.float32)
    assert W.bits_equal(W.embed(odd, ld=36).view, odd)


def test_a_correct_op_passes():
    run(None)


@pytest.mark.parametrize("fault,message", [("ignores_ld", "not finite|guard elements"), ("past_last_row", "guard elements"),
                                           ("left_of_c0", "guard elements"), ("reads_guard_times_zero", "not finite"),
                                           ("unwritten", "not finite"), ("own_nan_in_guard", "guard elements")])
def test_each_planted_fault_is_reported(fault, message):
    with pytest.raises(AssertionError, match=message):
        run(fault)


def test_only_a_poisoned_guard_shows_a_read_that_is_multiplied_by_zero():
    """with finite guards (what every earlier test had next to its windows) the same fault passes: the poison is what sees it"""
    run("reads_guard_times_zero", poison=123.0)


def test_an_input_buffer_that_was_written_is_reported():
    h = W.embed(torch.zeros(3, 4))
    h.view[1, 2] = 1.0
    with pytest.raises(AssertionError, match="input buffer"):
        W.assert_unchanged(h)
    W.assert_guards_intact(h)              # the guards themselves are whole


def test_bits_equal_sees_the_sign_of_zero():
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0])) and not W.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


def test_max_pool_gradient_on_the_cpu_goes_to_the_first_maximum():
    """The rule maxpool_bwd_kernel implements (ATen's), shown on the reference the GPU tie test compares with."""
    x = torch.tensor([[[1.0, 1.0, 1.0, 0.5, 1.0, 1.0]]], dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():          # (GPU test modules switch autograd off globally when they are collected)
        y = torch.nn.functional.max_pool1d(x, 3, 2, 1)          # windows (-, 0, 1), (1, 2, 3), (3, 4, 5)
    y.backward(torch.tensor([[[1.0, 10.0, 100.0]]], dtype=torch.float64))
    assert x.grad.flatten().tolist() == [1.0, 10.0, 0.0, 0.0, 100.0, 0.0]
