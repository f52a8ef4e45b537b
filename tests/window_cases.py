"""Strided windows with poisoned guard bands (tests/test_window_cases_cpu.py, tests/test_gpu_windows.py).

The C ABI addresses every activation as rows of a wider buffer (pointer + leading dimension).  embed() places a tensor into
such a buffer: `rows_before` guard rows, then the rows of the tensor at column c0 of rows `ld` floats wide, then `rows_after`
guard rows.  Everything outside the window holds one quiet NaN with a recognisable payload, compared as int32: a kernel that
writes anything into a guard -- a NaN of its own included -- changes the bits; a kernel that reads a guard and multiplies by
zero returns NaN.  An output buffer starts as the sentinel everywhere, the window included, so an element that is never written
stays non-finite.  Nothing here needs a GPU."""
import torch

SENTINEL_BITS = 0x7FC5A5A5          # quiet NaN (exponent all ones, top mantissa bit set), payload 0x5A5A5
LD_EXTRA, C0, ROWS_BEFORE, ROWS_AFTER = 64, 32, 2, 3       # c0 = 32 floats = 128 bytes: the window stays 16-byte (and pair-block) aligned


def sentinel(device="cpu"):
    """the poison value as a float32 scalar tensor"""
    return torch.tensor([SENTINEL_BITS], dtype=torch.int32, device=device).view(torch.float32)[0]


POISON = object()          # default of embed(poison=): the sentinel NaN


class Window:
    """What embed() returns: `view` is the operand to hand to the op (shape of the embedded tensor, last stride 1, row pitch
    ld); `buf` the whole (rows_before + rows + rows_after, ld) buffer; `flat`, `offset`, `ld` address it the way a kernel does:
    element (r, c) of the window is flat[offset + r * ld + c]."""

    def __init__(self, buf, view, row0, rows, c0, cols, output, name):
        self.buf, self.view, self.row0, self.rows, self.c0, self.cols = buf, view, row0, rows, c0, cols
        self.ld = buf.shape[1]
        self.offset = row0 * self.ld + c0
        self.flat = buf.view(-1)
        self.output, self.name = output, name
        self.before = buf.view(torch.int32).clone()           # the bits at embed time

    def inside(self):
        """bool mask of the buffer: True on the window"""
        m = torch.zeros(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        m[self.row0:self.row0 + self.rows, self.c0:self.c0 + self.cols] = True
        return m

    def result(self):
        """a contiguous copy of the window"""
        return self.view.clone()


def embed(t, ld=None, c0=C0, rows_before=ROWS_BEFORE, rows_after=ROWS_AFTER, poison=POISON, output=False, name=""):
    """Place `t` ((rows, C) or (B, T, C) float32, any device) into a buffer of row pitch `ld` (default C + 64) filled with
    `poison` (default: the sentinel NaN; a float for experiments).  output=True: the window starts as the sentinel too -- `t`
    only gives shape and device."""
    assert t.dtype == torch.float32 and t.dim() in (2, 3)
    cols = t.shape[-1]
    rows = t.numel() // cols
    ld = cols + LD_EXTRA if ld is None else ld
    assert ld >= c0 + cols and rows_before >= 0 and rows_after >= 0
    total = rows_before + rows + rows_after
    bits = torch.full((total, ld), SENTINEL_BITS, dtype=torch.int32, device=t.device)
    buf = bits.view(torch.float32)
    if poison is not POISON:
        buf.fill_(poison)
    win = buf[rows_before:rows_before + rows, c0:c0 + cols]
    if output:
        bits[rows_before:rows_before + rows, c0:c0 + cols] = SENTINEL_BITS
    else:
        # (through int32: the operand may be pair rows, 16-bit planes in f32 clothing, whose bit patterns must survive)
        bits[rows_before:rows_before + rows, c0:c0 + cols] = t.contiguous().view(torch.int32).reshape(rows, cols)
    view = win if t.dim() == 2 else win.unflatten(0, (t.shape[0], t.shape[1]))
    assert view.stride(-1) == 1 and view.stride(-2) == ld
    return Window(buf, view, rows_before, rows, c0, cols, output, name)


def embed_out(shape, device, **kw):
    """an output window of this shape"""
    return embed(torch.empty(shape, dtype=torch.float32, device=device), output=True, **kw)


def _describe(h, bad):
    idx = torch.nonzero(bad)[:4].tolist()
    return (f"window '{h.name}' (rows {h.row0}..{h.row0 + h.rows - 1}, columns {h.c0}..{h.c0 + h.cols - 1} of a "
            f"{tuple(h.buf.shape)} buffer): {int(bad.sum())} elements, first at (row, column) {idx}")


def assert_guards_intact(h):
    """every element outside the window holds the bits it held at embed time"""
    changed = (h.buf.view(torch.int32) != h.before) & ~h.inside()
    assert not bool(changed.any()), "guard elements were written -- " + _describe(h, changed)


def assert_unchanged(h):
    """an input buffer: window and guards hold the bits they held at embed time"""
    changed = h.buf.view(torch.int32) != h.before
    assert not bool(changed.any()), "an input buffer was written -- " + _describe(h, changed)


def assert_written_and_finite(h):
    """an output window: every element finite (an element that was never written is still the sentinel NaN; one computed from a
    guard is NaN too)"""
    bad = ~torch.isfinite(h.buf) & h.inside()
    assert not bool(bad.any()), "window elements are not finite (never written, or computed from a guard) -- " + _describe(h, bad)


def check(outputs, inputs=()):
    """the checks every case makes on its buffers; values are compared by the caller"""
    for h in outputs:
        assert h.output
        assert_written_and_finite(h)
        assert_guards_intact(h)
    for h in inputs:
        assert_unchanged(h)


def bits_equal(a, b):
    """bit for bit (distinguishes -0.0 from 0.0 and NaN payloads, unlike torch.equal)"""
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


class LdSeq:
    """Distinct leading dimensions for the operands of one case: width + 64, + 96, + 128 ... (multiples of 32 floats, so pair
    rows keep their 128-byte blocks), never equal to the width or to each other for operands of the same width."""

    def __init__(self, start=LD_EXTRA, step=32):
        self.extra, self.step = start, step

    def __call__(self, width):
        ld = width + self.extra
        self.extra += self.step
        return ld
