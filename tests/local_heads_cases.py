"""Parameters and seeded inputs of the width / head-count goldens (tests/golden/local_heads*.npz, forward_test_vidvrd_c256.json,
train_step_vidvrd_c256*): banded attention at width 256 and at head_dim 32, which the shipped configs (width 512, 4 or 8
heads) do not use.  scripts/make_golden_heads.py imports this file, so the generator and the tests hold the same numbers;
nothing here needs the reference.  Sequences, lengths and thinning are those of tests/local_window_cases.py."""
import torch

import local_window_cases as LW

WINDOWS = (3, 5, 7, 9, 11, 13, 15, 17, 19)
REF_WINDOWS = LW.REF_WINDOWS        # (5, 11, 19): the reference cannot run window 3 (local_window_cases.py)
# (width, heads): head_dim 32 at width 512; head_dim 32, 64 and 128 at width 256.  At width 512 windows up to 9 run the
# whole-row strip kernel and the others the half-row one, so 5 | 11, 19 hold a golden of either form; at width 256 one kernel
# (four channels a lane, one wave per strip) runs every window.
SHAPES = ((512, 16), (256, 8), (256, 4), (256, 2))
B = LW.B
CH_STRIDE = LW.CH_STRIDE            # 17 is odd: the stored channels visit every slot of a lane's 4 or 8 and every head (test_local_heads_cpu)
sample = LW.sample
seq_len, lengths, mask = LW.seq_len, LW.lengths, LW.mask
OP_CASES = [(C, H, W, rel) for C, H in SHAPES for W in REF_WINDOWS for rel in (False, True)]
ALL_OP_CASES = [(C, H, W, rel) for C, H in SHAPES for W in WINDOWS for rel in (False, True)]
# whole modules: the smallest and the largest golden window, rel_pe at the first
MHCA_CASES = [(C, H, W, W == 5) for C, H in SHAPES for W in (5, 19)]
SOS_CASE = dict(C=256, H=8, W=9)    # the vidor_local decoder layer (its own window) at width 256


def tag(C, H, W, rel):
    return f"c{C}_h{H}_w{W}_{'rel' if rel else 'norel'}"


def core_inputs(C, H, W, rel):
    """q, k, v and the output's gradient, (B, C, T) each, and the (1, 1, H, W) bias or None -- what the reference's banded
    attention core ran on."""
    g = torch.Generator().manual_seed(400000 + 100 * C + 1000 * W + 10 * H + int(rel))
    T = seq_len(W)
    q, k, v, dO = (torch.randn(B, C, T, generator=g) for _ in range(4))
    rel_pe = torch.randn(1, 1, H, W, generator=g) if rel else None
    return q, k, v, dO, rel_pe


def mhca_inputs(C, H, W, rel):
    """Input (zero on padded frames) and output gradient of the whole LocalMaskedMHCA; its weights are name-seeded under
    mhca_prefix."""
    g = torch.Generator().manual_seed(500000 + 100 * C + 1000 * W + 10 * H + int(rel))
    T = seq_len(W)
    x = torch.randn(B, C, T, generator=g) * mask(W)
    dy = torch.randn(B, C, T, generator=g)
    return x, dy


def mhca_prefix(C, H, W, rel):
    return "op.local_mhca_" + tag(C, H, W, rel)


def sos_inputs():
    C, W = SOS_CASE["C"], SOS_CASE["W"]
    g = torch.Generator().manual_seed(600000 + C + W)
    T = seq_len(W)
    m = mask(W)
    x, y = torch.randn(B, C, T, generator=g) * m, torch.randn(B, C, T, generator=g) * m
    dy = torch.randn(B, C, T, generator=g)
    return x, y, dy, m


SOS_PREFIX = "op.sos_local_c256"

# model level: (golden case the other settings come from, what replaces them, padded length, lengths, seed)
MODEL_CASES = {
    "vidvrd_c256": dict(base="vidvrd", set=dict(embd_dim=256), T=96, lens=[96, 61, 17, 2], seed=6256),
    "vidvrd_h16": dict(base="vidvrd", set=dict(n_head=16, fuse_head=16), T=96, lens=[96, 61, 17, 2], seed=6016),
    "vidvrd_c256_h2": dict(base="vidvrd", set=dict(embd_dim=256, n_head=2, fuse_head=4), T=96, lens=[96, 61, 17, 2], seed=6002),
    "vidor_local_c256": dict(base="vidor_local", set=dict(embd_dim=256), T=512, lens=[512, 333, 77, 20], seed=6512),
}
FORWARD_TEST_C256 = LW.FORWARD_TEST_W19       # the proposals of the window-19 test
TRAIN_C256 = LW.TRAIN_W5                      # the batch of train_step_vidvrd


def model_config(mc, case):
    """The golden case's model config with the case's settings replaced; the predictor reads the backbone's width."""
    spec = MODEL_CASES[case]
    mc = dict(mc, **spec["set"])
    if "embd_dim" in spec["set"]:
        mc["predictor"] = dict(mc["predictor"], n_input=spec["set"]["embd_dim"])
    return mc


def load_npz_parts(path_stem):
    return LW.load_npz_parts(path_stem)
