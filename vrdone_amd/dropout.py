"""Host mirror of the training dropout's keep decisions (numpy only: the tests and scripts/make_golden_dropout.py import it).

A decision is a pure function of (step seed, site, element id) -- no mask tensor is ever stored; the backward kernels compute
it again (csrc/vrd_philox.h is the device side of the same function):

  generator  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
  key        the 64-bit step seed (low word, high word)
  counter    (id >> 2 as two words, site, 0); element `id` takes word id & 3 of the block, so four consecutive ids -- the four
             channels of a float4 lane -- cost one call
  keep       iff word >= floor(p * 2^32), p the rate as a float32; kept values are multiplied by 1 / (1 - p), formed once in f32

Element ids (64-bit) continue through a training step: `row = sample * T' + t`, where `sample` counts the samples a module has
seen in this step (a module's second call continues where its first ended, so a stem block gives the same masks whether the
subject and object streams run as two calls of B samples or one call of 2 B):
  row sites (attn.proj_drop, mlp.2, mlp.4)    id = row * C + c
  attention site (attn.attn_drop)             id = (row * n_head + head) * (2 w + 1) + slot: the flat index of the reference's `att`
A site is zlib.crc32 of the reference's module name, e.g. "backbone.stem.0.attn.attn_drop"; op-level callers pass any integer.
"""
import zlib

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

BLOCK_SITES = ("attn.attn_drop", "attn.proj_drop", "mlp.2", "mlp.4")      # the four nn.Dropout of a reference TransformerBlock


def philox4x32_10(counter, key):
    """counter: (..., 4) and key: (..., 2) arrays of 32-bit words (broadcast against each other) -> (..., 4) uint32 words."""
    c = np.asarray(counter, dtype=np.uint64) & _U32
    k = np.asarray(key, dtype=np.uint64) & _U32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _U32, (k1 + np.uint64(PHILOX_W1)) & _U32
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _U32, (p0 >> _S32) ^ c3 ^ k1, p0 & _U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def site_id(name):
    """The site word of a dropout module: zlib.crc32 of its name in the reference's module tree."""
    return zlib.crc32(name.encode()) & 0xFFFFFFFF


def threshold(p):
    """floor(p * 2^32) of the rate as a float32 (what the kernels compare a word against)."""
    p32 = float(np.float32(p))
    if not 0.0 <= p32 < 1.0:
        raise ValueError(f"a dropout rate lies in [0, 1), got {p!r}")
    return int(np.floor(p32 * 4294967296.0))


def keep_scale(p):
    """1 / (1 - p), formed once in float32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(seed, site, ids):
    """The 32-bit word of every element id (any shape, 64-bit ids)."""
    ids = np.asarray(ids, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    blk = ids >> np.uint64(2)
    counter = np.stack([blk & _U32, blk >> _S32, np.full_like(blk, int(site) & 0xFFFFFFFF), np.zeros_like(blk)], axis=-1)
    out = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    return np.take_along_axis(out, (ids & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def keep_ids(seed, site, ids, p):
    """uint8 keep decisions of arbitrary element ids."""
    return (words(seed, site, ids).astype(np.uint64) >= np.uint64(threshold(p))).astype(np.uint8)


def keep_mask(seed, site, first_id, n, p):
    """uint8 keep decisions of the n consecutive ids from first_id on."""
    return keep_ids(seed, site, np.uint64(int(first_id)) + np.arange(int(n), dtype=np.uint64), p)


def row_ids(row0, rows, C):
    """(rows, C) ids of a row site: (row0 + r) * C + c."""
    r = np.uint64(int(row0)) + np.arange(int(rows), dtype=np.uint64)
    return r[:, None] * np.uint64(C) + np.arange(int(C), dtype=np.uint64)[None, :]


def attn_ids(row0, rows, n_head, window):
    """(rows, n_head, window) ids of the attention site: ((row0 + r) * n_head + head) * window + slot."""
    first = np.uint64(int(row0)) * np.uint64(n_head * window)
    return (first + np.arange(int(rows) * n_head * window, dtype=np.uint64)).reshape(int(rows), n_head, window)


def row_mask(seed, site, row0, rows, C, p):
    return keep_ids(seed, site, row_ids(row0, rows, C), p)


def attn_mask(seed, site, row0, rows, n_head, window, p):
    return keep_ids(seed, site, attn_ids(row0, rows, n_head, window), p)
