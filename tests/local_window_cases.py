"""Parameters and seeded inputs of the local-window goldens (tests/golden/local_window*.npz, forward_test_vidvrd_w19.json,
train_step_vidvrd_w5*): banded attention at the windows the shipped configs do not use.  scripts/make_golden_window.py
imports this file, so the generator and the tests hold the same numbers; nothing here needs the reference."""
import torch

WINDOWS = (3, 5, 11, 19)
# The reference itself cannot run window 3: its sliding-chunk code (blocks.py:871-873, `1 - window_overlap :` with
# window_overlap = 1) fails with a shape error in the first forward.  Goldens exist for 5, 11 and 19; window 3 is held to the
# oracle, which these goldens (and those at 7 / 9) pin.
REF_WINDOWS = (5, 11, 19)
HEADS = (4, 8)
B, C = 3, 512
CH_STRIDE = 17          # stored activations keep every 17th channel: all heads, every channel slot of a lane's 8 (or 4)
GRAD_FULL, GRAD_STRIDE = 2048, 499       # parameter gradients: full up to 2048 elements, else every 499th (as train_step_*.npz)
OP_CASES = [(W, H, rel) for W in REF_WINDOWS for H in HEADS for rel in (False, True)]
ALL_OP_CASES = [(W, H, rel) for W in WINDOWS for H in HEADS for rel in (False, True)]


def seq_len(W):
    """The smallest multiple of the reference's chunk (2 * (W // 2) frames) that is >= 34: two strips of 16 and a partial one."""
    chunk = 2 * (W // 2)
    return chunk * -(-34 // chunk)


def lengths(W):
    """Ragged: a length that is no multiple of 16, a sequence of half a window, a fully masked one."""
    return [seq_len(W) - 3, W // 2, 0]


def mask(W):
    T = seq_len(W)
    return (torch.arange(T)[None] < torch.tensor(lengths(W))[:, None])[:, None]              # (B, 1, T)


def tag(W, H, rel):
    return f"w{W}_h{H}_{'rel' if rel else 'norel'}"


def core_inputs(W, H, rel):
    """q, k, v and the output's gradient, (B, C, T) each, and the (1, 1, H, W) bias or None -- what the reference's banded
    attention core (blocks.py:949-986) ran on."""
    g = torch.Generator().manual_seed(100000 + 1000 * W + 10 * H + int(rel))
    T = seq_len(W)
    q, k, v, dO = (torch.randn(B, C, T, generator=g) for _ in range(4))
    rel_pe = torch.randn(1, 1, H, W, generator=g) if rel else None
    return q, k, v, dO, rel_pe


def mhca_inputs(W, H, rel):
    """Input (zero on padded frames) and output gradient of the whole LocalMaskedMHCA; its weights are name-seeded under
    mhca_prefix (rel_pe: O(1) values, oracle.vrd_oracle.synth_tensor)."""
    g = torch.Generator().manual_seed(200000 + 1000 * W + 10 * H + int(rel))
    T = seq_len(W)
    x = torch.randn(B, C, T, generator=g) * mask(W)
    dy = torch.randn(B, C, T, generator=g)
    return x, dy


def mhca_prefix(W, H, rel):
    return "op.local_mhca_" + tag(W, H, rel)


SOS_WINDOWS = (5, 19)


def sos_inputs(W):
    """The vidor_local decoder layer (8 heads, LocalMaskedMHCA_QKV self and cross attention, no FFN) at window W: two streams,
    the output gradient, the shared mask."""
    g = torch.Generator().manual_seed(300000 + W)
    T = seq_len(W)
    m = mask(W)
    x, y = torch.randn(B, C, T, generator=g) * m, torch.randn(B, C, T, generator=g) * m
    dy = torch.randn(B, C, T, generator=g)
    return x, y, dy, m


def sample(g):
    g = g.detach()
    return g if g.numel() <= GRAD_FULL else g.flatten()[::GRAD_STRIDE]


# model level: (golden case the weights' names and the other settings come from, window, max_seq_len = padded length, lengths, seed)
MODEL_CASES = {
    "vidvrd_w5": dict(base="vidvrd", win=5, T=96, lens=[96, 61, 17, 2], seed=5005),
    # 144: the smallest max_seq_len the reference's divisibility assert takes at window 19 and strides 1 .. 8
    "vidvrd_w19": dict(base="vidvrd", win=19, T=144, lens=[144, 97, 41, 9], seed=5019),
    "vidor_local_w5": dict(base="vidor_local", win=5, T=512, lens=[512, 333, 77, 20], seed=5105),
}
FORWARD_TEST_W19 = dict(n_tracklets=6, min_len=20, max_len=200, seed=1919)
TRAIN_W5 = dict(B=24, T=96, seed_len=2024, seed_x=3, seed_gt=2025)           # the batch of train_step_vidvrd, window 5


def model_config(mc, case):
    """The golden case's model config with the window (and the maximal length that goes with it) replaced."""
    spec = MODEL_CASES[case]
    return dict(mc, n_mha_win_size=spec["win"], max_seq_len=spec["T"])


def load_npz_parts(path_stem):
    """train_step_vidvrd_w5 is stored in two files to keep each under the repository's size limit."""
    import numpy as np
    out = {}
    for part in ("a", "b"):
        with np.load(f"{path_stem}_{part}.npz") as z:
            out.update({k: z[k] for k in z.files})
    return out
