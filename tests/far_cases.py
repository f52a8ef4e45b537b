"""Rows beyond the 32-bit offset lines (tests/test_far_cases_cpu.py, tests/test_gpu_far_rows.py).

A launch wave of the eval path holds up to WAVE_PAIRS = 1.25 x pair_chunk pairs (MaskVRD._chunk_size), two entity streams each, at
the config's max_seq_len.  An operand of that wave lies mostly beyond the offsets a 32-bit number can hold.  Four lines, in bytes:

    L31B = 2^31 bytes   a signed byte offset wraps          L31E = 2^31 elements (2^33 bytes)   a signed element index wraps
    L32B = 2^32 bytes   an unsigned byte offset wraps       L32E = 2^32 elements (2^34 bytes)   an unsigned element index wraps

extents() computes, per shipped config (vrdone_amd/configs.py) and operand class, how far the largest wave reaches; a class has to be
tested behind every line some config's extent crosses (required_lines).  Today (rows = 2 * 2560 * max_seq_len; GiB and the last line
crossed; the box features, 5 and 8 floats wide, and the window-edge pieces of vrd_assemble_pairs stay below 0.1 GiB):

    config              rows  fpn (256)  embd (512)  visual (1024)  qkv (3 x 512)  hidden (2048)  source (4096, C_in, T)
    vidvrd           491,520  0.47       0.94         1.88           2.81 L31B      3.75 L31B     4096 x 2069 x  96   3.03 L31B
    vidor(_local)  2,621,440  2.50 L31B  5.00 L32B   10.00 L31E     15.00 L31E     20.00 L32E     4096 x 2069 x 512  16.16 L32E
    vidor_x        2,621,440  2.50 L31B  5.00 L32B   10.00 L31E     15.00 L31E     20.00 L32E     4096 x 3093 x 512  24.16 L32E

The source is the caller's whole (B, C_in, T) batch, SOURCE_BATCH_PAIRS = 4096 pairs in BASELINE config 5: vrd_bct_to_btc gathers a wave's
sequences from it through index=, so it is one buffer however many waves the batch makes.

Backward and training kernels are not covered: a training batch is 24-48 pairs, 48 x 2 x 512 = 49,152 rows, 0.38 GiB at the hidden
width -- three orders of magnitude below the first line.  The criterion, post-processing and scoring buffers are smaller still.

The method.  Inputs are PERIODIC: one period is NSEQ = 61 ragged sequences of T = 64 seeded random rows (masks and lengths as the
window cases build them), repeated to fill R rows; outputs start as the sentinel NaN of tests/window_cases.py.  Position does not
enter these kernels' arithmetic, so every later period of an output has to equal period 0 bit for bit, and period 0 is compared
with a float64 reference.  A kernel that computes an offset in 32 bits reads or writes a wrapped address: the period's size must not
divide the wrap distance (wrapped reads would fetch the same data), which sees() checks for every buffer and address model.

Nothing here needs a GPU."""
from dataclasses import dataclass, field

T = 64
NSEQ = 61                      # odd: 61 * 2^k never divides a power of two
GUARD_ROWS = 2
WAVE_PAIRS = 2560              # MaskVRD._chunk_size: one wave up to pair_chunk + pair_chunk // 4
SOURCE_BATCH_PAIRS = 4096      # the (B, C_in, T) batch vrd_bct_to_btc gathers a wave's sequences from (BASELINE config 5)
MEMORY_CAP = 32 << 30

LINES = {"L31B": 1 << 31, "L32B": 1 << 32, "L31E": 1 << 33, "L32E": 1 << 34}          # byte offsets
# faulty address models: name -> (the line at which the first wrap happens, wrap distance in bytes, signed)
MODELS = {
    "signed byte offset": ("L31B", 1 << 32, True),
    "unsigned byte offset": ("L32B", 1 << 32, False),
    "signed element index": ("L31E", 1 << 34, True),
    "unsigned element index": ("L32E", 1 << 34, False),
}


def class_width(cfg, cls):
    return {"ent_box": cfg["bbox_entity_dim"], "so_box": cfg["bbox_so_dim"], "fpn": cfg["fpn_dim"], "embd": cfg["embd_dim"],
            "visual": cfg["visual_dim"], "qkv": 3 * cfg["embd_dim"], "hidden": 4 * cfg["embd_dim"]}[cls]


ROW_CLASSES = ("ent_box", "so_box", "fpn", "embd", "visual", "qkv", "hidden")
EDGE_FRAMES = 16               # frames of window-edge pieces per entity stream (vrd_assemble_args.snippets: two pieces of L = 8)


def extents():
    """{config: {class: bytes}} of the largest wave's operands"""
    from vrdone_amd import configs
    out = {}
    for name in ("vidvrd", "vidor", "vidor_local", "vidor_x"):
        cfg = configs.model_config(name)
        rows = 2 * WAVE_PAIRS * cfg["max_seq_len"]
        e = {cls: rows * class_width(cfg, cls) * 4 for cls in ROW_CLASSES}
        e["source"] = SOURCE_BATCH_PAIRS * configs.input_channels(cfg) * cfg["max_seq_len"] * 4
        e["edge_pieces"] = 2 * WAVE_PAIRS * EDGE_FRAMES * cfg["embd_dim"] * 4
        e["rows"] = rows
        out[name] = e
    return out


def required_lines(cls, ext=None):
    """the lines some shipped config's operand of this class crosses, nearest first"""
    ext = extents() if ext is None else ext
    return [ln for ln, at in LINES.items() if any(e[cls] > at for e in ext.values())]


@dataclass
class Buf:
    """One operand buffer: `pitch` floats per row, `seq_rows` rows per sequence of the case (T, T // stride for a strided output,
    1 for the (B, C_in, T) source whose "row" is one batch item), role "in" / "out", operand class `cls`."""
    name: str
    role: str
    cls: str
    pitch: int
    seq_rows: int = T

    @property
    def pitch_bytes(self):
        return self.pitch * 4


@dataclass
class Case:
    """entry: the C entry point / ops wrapper; body: the kernel body that must run; modes: precision modes; tile: rows of one tile
    (workgroup) of that body; unit: the row count is a multiple of it (T for kernels that take sequences, 1 for kernels that take
    any row count); every output gets GUARD_ROWS poisoned rows behind its last row; why: a sentence where a size is not the default."""
    name: str
    entry: str
    body: str
    modes: tuple
    bufs: list
    tile: int = 64
    unit: int = T
    seq_len: int = T
    why: str = ""
    params: dict = field(default_factory=dict)

    def lines(self, b):
        return required_lines(b.cls)

    def nseq(self):
        """sequences (units of seq_len rows) so that every buffer has a full tile and a ragged last tile behind its last line"""
        need = 0
        for b in self.bufs:
            rows = -(-LINES[self.lines(b)[-1]] // b.pitch_bytes) if self.lines(b) else 0           # first row that starts behind the line
            need = max(need, -(-rows // b.seq_rows))
        n = need + -(-self.tile // min(b.seq_rows for b in self.bufs)) + 1
        while self.params.get("ragged") and (n * self.seq_len) % 64 == 0:
            n += 1
        n += n % 2 if self.params.get("halves") else 0          # subject rows then object rows: an even number of entity sequences
        return n

    def rows(self, b=None):
        """R: rows of buffer `b` (default: of a buffer at seq_len rows per sequence).  unit == 1: the last sequence is cut to 7 rows
        (a ragged last tile of any tile size); otherwise the ragged tile is the last, single, sequence."""
        per = self.seq_len if b is None else b.seq_rows
        r = self.nseq() * per
        return r - (per - 7) if self.unit == 1 else r

    def period_rows(self, b):
        return NSEQ * b.seq_rows

    def guard_rows(self):
        return GUARD_ROWS

    def bytes(self):
        return sum((self.rows(b) + (self.guard_rows() if b.role == "out" else 0)) * b.pitch_bytes for b in self.bufs)


def wrapped(offset, model):
    """the byte offset a kernel with this faulty address model uses in place of `offset` (a Python int)"""
    _, wrap, signed = MODELS[model]
    o = offset % wrap
    return o - wrap if signed and o >= wrap // 2 else o


def sees(case, b, model):
    """(rows behind the model's line, rows among them where the fault shows).  Row r of an output is written somewhere else and
    stays poison; row r of an input is read from row r' (or from outside the buffer) and shows when r - r' is no multiple of the
    period.  Index arithmetic only (int64 vectors over the rows behind the line)."""
    import torch
    line, wrap, signed = MODELS[model]
    if line not in case.lines(b):
        return 0, 0
    pb, period = b.pitch_bytes, case.period_rows(b) * b.pitch_bytes
    first = -(-LINES[line] // pb)
    o = torch.arange(first, case.rows(b), dtype=torch.int64) * pb
    w = o % wrap
    if signed:
        w = torch.where(w >= wrap // 2, w - wrap, w)
    shown = w != o
    if b.role == "in":
        shown &= (w < 0) | ((o - w) % period != 0)
    return int(o.numel()), int(shown.sum())


def wrap_distance_ok(case, b, model):
    """the period does not divide the wrap distance"""
    return MODELS[model][1] % (case.period_rows(b) * b.pitch_bytes) != 0


# ------------------------------------------------------------------------------------------------------------------ the table
ALL, SPLIT, F32 = ("f32", "bf16x3", "f16x3"), ("bf16x3", "f16x3"), ("f32",)
E, H, Q3, FP = 512, 2048, 1536, 256


def _rowop(name, entry, body, modes, width, cls, outs=1, stride=1, up=False, unit=T, tile=64, in_width=None, in_cls=None, **params):
    bufs = [Buf("x", "in", in_cls or cls, in_width or width, T)]
    if up:
        bufs.append(Buf("x_up", "in", cls, width, T // 2))
    bufs += [Buf(f"y{i}", "out", cls, width, T // stride) for i in range(outs)]
    return Case(name, entry, body, modes, bufs, tile=tile, unit=unit, params=params)


def _cases():
    c = []
    # ---- layout
    c.append(Case("bct_to_btc_vec", "ops.bct_to_btc", "bct_to_btc_vec_kernel", ALL,
                  [Buf("src", "in", "source", 3093 * T, 1), Buf("dst", "out", "embd", E, 60)], tile=1, unit=T,
                  params=dict(frames=60, c0=2048, count=512),
                  why="the 512 CLIP channels of config 5's 3093; frames=60 of 64 and index= (every item from its own place)"))
    c.append(Case("bct_to_btc_scalar", "ops.bct_to_btc", "bct_to_btc_kernel", F32,
                  [Buf("src", "in", "source", 3093 * T, 1), Buf("dst", "out", "embd", E, 62)], tile=1, unit=T,
                  params=dict(frames=62, c0=2563, count=510), why="frames=62 and 510 channels from channel 2563: the scalar kernel"))
    c.append(Case("btc_to_bct", "ops.btc_to_bct", "btc_to_bct_kernel", F32,
                  [Buf("src", "in", "embd", E, T), Buf("dst", "out", "embd", E, T)], tile=64, unit=T,
                  why="the (B, C, T) output is addressed as B * T rows of C floats: the same extent"))
    for entry in ("pack_pairs", "gather_pairs"):
        c.append(Case(entry, f"vrd_{entry}", f"{entry}_kernel", ALL,
                      [Buf("vis", "out", "visual", 1024, T), Buf("clip", "out", "embd", E, T), Buf("ent", "out", "ent_box", 8, T), Buf("so_box", "out", "so_box", 5, T // 2)],
                      tile=4, params=dict(halves=True), why="the outputs are the large buffers: (2, P, T, V) subject rows then object rows; the sources are 61 small matrices"))
    c.append(Case("assemble_pairs", "vrd_assemble_pairs", "assemble_pairs_kernel", F32,
                  [Buf("snippets", "in", "edge_pieces", E, EDGE_FRAMES), Buf("out", "out", "embd", E, T)], tile=4, params=dict(halves=True, L=8, piece=4, reach=2)))
    # ---- row kernels
    for w, cls in ((FP, "fpn"), (E, "embd")):
        for variant in ("plain", "relu", "post_add"):
            c.append(_rowop(f"layernorm_{w}_{variant}", "ops.layernorm", f"layernorm_kernel<{w // 256}>", F32, w, cls, unit=1, tile=4, variant=variant,
                            pair=False))
        c.append(_rowop(f"layernorm_{w}_pair", "ops.layernorm", f"layernorm_kernel<{w // 256}>", SPLIT, w, cls, unit=1, tile=4, variant="plain", pair=True))
    c.append(_rowop("conv_ln_entity", "ops.conv_ln", "conv_ln_kernel", F32, E, "embd", in_width=8, in_cls="ent_box", Cin=8, ln=True))
    c.append(_rowop("conv_ln_pair_box", "ops.conv_ln", "conv_ln_kernel", F32, E, "embd", in_width=5, in_cls="so_box", Cin=5, ln=False))
    for name, (stride, gin, k, n_out, w, pre, up, ln, bias) in DW_CASES.items():
        c.append(_rowop(f"dwconv_ln_{name}", "ops.dwconv_ln", "dwconv_ln_kernel", F32, w, "embd" if w == E else "fpn", outs=n_out, stride=stride, up=up,
                        in_width=w * gin, case=name))
    c.append(_rowop("dwconv_ln_row_groups", "ops.dwconv_ln(segs=)", "dwconv_ln_kernel", F32, E, "embd", outs=3, stride=2, case="qkv_s2", segs=True))
    c.append(_rowop("maxpool_mask", "ops.maxpool_mask", "maxpool_mask_kernel", F32, E, "embd", stride=2))
    for act in ("relu", "gelu"):
        c.append(_rowop(f"activation_{act}", "vrd_activation", "activation_kernel", F32, E, "embd", unit=1, tile=4, act=act))
    for hd in (32, 64, 128):
        for hw in (1, 9):
            for rel in (False, True):
                for segs in (False, True):
                    c.append(Case(f"local_attn{'_segs' if segs else ''}_hd{hd}_w{2 * hw + 1}{'_rel' if rel else ''}",
                                  "vrd_local_attn_segs" if segs else "vrd_local_attn", "local attention strip kernel", F32,
                                  [Buf("qkv", "in", "qkv", Q3, T), Buf("out", "out", "embd", E, T)], params=dict(hd=hd, hw=hw, rel=rel, segs=segs)))
    # ---- GEMM
    for k in (1, 3):
        c.append(Case(f"gemm_f32_k{k}", "ops.conv_gemm", "K_GEMM", F32, _gemm_bufs(), tile=128, params=dict(k=k, pair_in=False, ragged=False)))
        c.append(Case(f"gemm_x3_k{k}", "ops.conv_gemm", "K_GEMM_X3", SPLIT, _gemm_bufs(), tile=128, params=dict(k=k, pair_in=False, ragged=False)))
        c.append(Case(f"gemm_big_k{k}", "ops.conv_gemm", "K_GEMM_X3_BIG", SPLIT, _gemm_bufs(), tile=256, params=dict(k=k, pair_in=True, ragged=False)))
        c.append(Case(f"gemm_dma_k{k}", "ops.conv_gemm", "K_GEMM_X3_DMA", SPLIT, _gemm_bufs(T + 4), tile=128, seq_len=T + 4, params=dict(k=k, pair_in=True, ragged=True),
                      why="sequences of 68 rows: M % 64 != 0 keeps the 256 x 256 body out (as test_gemm_large_tile_windows does)"))
    c.append(Case("gemm_mlp_f32", "ops.conv_gemm x 2", "K_GEMM", F32, _mlp_bufs(), tile=128, params=dict(pair=False)))
    c.append(Case("gemm_mlp_split", "ops.conv_gemm x 2", "K_GEMM_X3_BIG", SPLIT, _mlp_bufs(), tile=256, params=dict(pair=True)))
    # ---- global attention
    c.append(Case("attention_flash_f32rows", "ops.attention(algo=2)", "attn_flash_kernel", F32,
                  [Buf("q", "in", "embd", E, T), Buf("kv", "in", "qkv", Q3, T), Buf("out", "out", "embd", E, T)], params=dict(hd=64)))
    for w64 in (0, 1):
        for hd in ((32, 64, 128) if not w64 else (64, 128)):
            c.append(Case(f"attention_pair_{'w64' if w64 else 'w32'}_hd{hd}", "ops.attention(Pair)", "attn_flash_x3_w64_kernel" if w64 else "attn_flash_x3_kernel",
                          SPLIT, [Buf("q", "in", "embd", E, T), Buf("kv", "in", "qkv", Q3, T), Buf("out", "out", "embd", E, T)],
                          params=dict(hd=hd, w64=w64), why="Tq = 64 is the 64-queries-per-wave kernel's smallest full tile" if w64 else ""))
    return c


DW_CASES = {          # tests/test_gpu_windows.py DW_CASES: stride, group_in, k, n_out, C, pre_ln, x_up, LayerNorm, bias
    "qkv_s1": (1, 1, 3, 3, 512, True, False, True, False),
    "qkv_s2": (2, 1, 3, 3, 512, True, False, True, False),
    "fpn_top": (1, 2, 3, 1, 256, False, False, True, False),
    "fpn_up": (1, 1, 3, 1, 256, False, True, True, False),
    "mask_features": (1, 1, 3, 1, 256, False, False, False, True),
    "k1": (1, 1, 1, 1, 256, False, False, True, False),
}


def _gemm_bufs(seq=T):
    """512 -> 512 with the full epilogue: every operand at its own pitch (width + 32, + 64, + 96 floats; x at its width)"""
    return [Buf("x", "in", "embd", E, seq), Buf("res", "in", "embd", E + 32, seq), Buf("res2", "in", "embd", E + 64, seq), Buf("out", "out", "embd", E + 96, seq)]


def _mlp_bufs():
    """up-projection 512 -> hidden (GELU), down-projection hidden -> 512 through one hidden buffer"""
    return [Buf("x", "in", "embd", E, T), Buf("res", "in", "embd", E, T), Buf("hidden", "out", "hidden", H, T), Buf("out", "out", "embd", E, T)]


CASES = {c.name: c for c in _cases()}

# the slab fallback of vrd_attention_pair (vrd_attn_x3.hip: "its LDS-DMA offsets are 32-bit"): one small case of its own, no period
SLAB_FALLBACK = dict(B=2, Tq=64, Tk=64, hd=64, heads=8, ldkv=(1 << 31) // (4 * 64) + 64)
