"""
numpy mirror of csrc/dropout.hip (frcnn_dropout): Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as
1, 2, 3", SC'11; the Random123 constants) and the keep rule.  No GPU.

Element i of a dropout call reads word (i & 3) of philox4x32_10(counter = (i >> 2 lo32, i >> 2 hi32, stream_id, rank),
key = (seed lo32, seed hi32)); it is kept when float32((w >> 8) * 2^-24) < float32(1 - p).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counters (arrays or scalars, uint32) and key (two uint32) -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint32).astype(np.uint64) for v in (c0, c1, c2, c3)]
    c = np.broadcast_arrays(*c)
    c = [v.copy() for v in c]
    k0, k1 = np.uint32(k0), np.uint32(k1)
    for r in range(10):
        if r:
            k0 = np.uint32((int(k0) + int(W0)) & 0xFFFFFFFF)
            k1 = np.uint32((int(k1) + int(W1)) & 0xFFFFFFFF)
        p0 = M0 * c[0]                      # < 2^64: exact in uint64
        p1 = M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return [v.astype(np.uint32) for v in c]


def seed_words(seed):
    """int64 seed (as torch draws it) -> (lo32, hi32) of its two's-complement bits."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def random_words(n, seed, stream_id, rank):
    """The n uint32 words frcnn_dropout draws for elements 0..n-1."""
    k0, k1 = seed_words(seed)
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    out = philox4x32_10((g & _MASK32).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                        np.uint32(stream_id), np.uint32(rank), k0, k1)
    return np.stack(out, axis=1).reshape(-1)[:n]


def keep_mask(n, p, seed, stream_id, rank):
    """uint8 [n]: 1 where frcnn_dropout keeps the element."""
    u = (random_words(n, seed, stream_id, rank) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u < np.float32(1.0) - np.float32(p)).astype(np.uint8)


def scale_of(p):
    """The kept elements' factor: float32(1 / (1 - p)) computed in double (inf for p == 1, where nothing is kept)."""
    return np.float32(np.inf) if p >= 1.0 else np.float32(1.0 / (1.0 - float(p)))


def dropout(x, p, seed, stream_id, rank):
    """float32 array -> (y, keep) as frcnn_dropout leaves them."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    keep = keep_mask(x.size, p, seed, stream_id, rank)
    if p == 0:
        return x.copy(), keep
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.where(keep.astype(bool), x * scale_of(p), np.float32(0.0)).astype(np.float32)
    return y, keep
