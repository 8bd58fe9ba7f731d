"""Cases of fasterrcnn_amd.ops.paste_masks_in_image / paste_masks_aligned / masks_to_boxes, their float64 truths and tolerances; numpy and
torch on the CPU only.

A truth is the contract of include/frcnn_hip.h evaluated in float64 (numpy, one box at a time) on the given float32 inputs, with the
INTEGER boxes of paste_masks_in_image taken from the float32 sequence (numpy float32 scalars round every operation on its own).

The value tolerance (derived, not measured): every float32 step up to the sample coordinate is relative-error 2^-24 on a magnitude of at
most M' + 1, at most five steps precede the blend, in two dimensions, plus the blend's own roundings, so with A_k = max|mask_k| a pasted
float32 value lies within tol_k = (10 (M' + 1) + 8) 2^-24 A_k of the truth; M' = M + 2 padding for paste_masks_in_image, max(Mh, Mw)
for paste_masks_aligned.

Everything is tiny: images 37 x 53, 33 x 47, 19 x 70 and one 64 x 64, K <= 8, M in {1, 2, 7, 14, 28}, plus one M at the stated maximum
on a 16 x 16 image.  The library cuts an image into pieces of 1024 vectors (16 bytes; 4 bytes in the byte paste), so one 150 x 231
image (8.5 pieces of a float32 or a pasted byte image, 2.1 of masks_to_boxes' bytes) is added for the seams between blocks; its cases
are the "pieces" ones."""
import functools

import numpy as np
import torch

from fasterrcnn_amd import ops

F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
HALF = DTYPES[1:]
MAX_SIDE = ops.MAX_PASTE_MASK_SIDE
CORNER = ops.PASTE_CORNER
NAN, INF = float("nan"), float("inf")


# ---- the contracts in float64 ------------------------------------------------------------------------------------------------------
def scale(m, p):
    return np.float32((m + 2 * p) / m)


def integer_boxes(boxes, m, p):
    """(X0, Y0, X1, Y1) int64 [K] of the float32 sequence and the rows with only finite coordinates."""
    b = np.asarray(boxes, dtype=np.float32)
    s, half = scale(m, p), np.float32(0.5)
    out = np.zeros((4, len(b)), dtype=np.int64)
    finite = np.isfinite(b).all(1)
    with np.errstate(all="ignore"):
        for k in np.nonzero(finite)[0]:
            for lo, hi, i0, i1 in ((b[k, 0], b[k, 2], 0, 2), (b[k, 1], b[k, 3], 1, 3)):
                h = np.float32(np.float32(hi - lo) * half)
                c = np.float32(np.float32(hi + lo) * half)
                h = np.float32(h * s)
                for v, i in ((np.float32(c - h), i0), (np.float32(c + h), i1)):
                    out[i, k] = int(np.trunc(np.clip(np.float64(v), -CORNER, CORNER)))
    return out[0], out[1], out[2], out[3], finite


def fused_corner(lo, hi, m, p, sign):
    """trunc of x_c + sign * w_half * s with the product NOT rounded (what a fused multiply-add computes), for the float32 pair (lo, hi)."""
    lo, hi = np.float32(lo), np.float32(hi)
    h = np.float64(np.float32(np.float32(hi - lo) * np.float32(0.5)))
    c = np.float64(np.float32(np.float32(hi + lo) * np.float32(0.5)))
    return int(np.trunc(np.float32(c + sign * h * np.float64(scale(m, p)))))


def _axis_in_image(coords, origin, size, mp):
    d = (coords - origin).astype(np.float64)
    s = np.maximum(mp / float(np.float32(size)) * (d + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), mp - 1)
    return i0, i0 + (i0 < mp - 1), s - i0


def _blend(p, iy, iy1, ly, ix, ix1, lx):
    ly, lx = ly[:, None], lx[None, :]
    return (1 - ly) * ((1 - lx) * p[np.ix_(iy, ix)] + lx * p[np.ix_(iy, ix1)]) + ly * ((1 - lx) * p[np.ix_(iy1, ix)] + lx * p[np.ix_(iy1, ix1)])


def truth_in_image(masks, boxes, shape, p):
    """float64 [K, H, W] of paste_masks_in_image on float32 (or 16-bit-valued) masks [K, 1, M, M]."""
    mk = masks[:, 0].double().numpy()
    k, m = mk.shape[:2]
    h, w = shape
    mp = m + 2 * p
    x0, y0, x1, y1, finite = integer_boxes(boxes.numpy(), m, p)
    out = np.zeros((k, h, w))
    for i in range(k):
        if not finite[i] or x1[i] < x0[i] or y1[i] < y0[i]:
            continue
        bw, bh = max(x1[i] - x0[i] + 1, 1), max(y1[i] - y0[i] + 1, 1)
        xs, ys = np.arange(max(x0[i], 0), min(x0[i] + bw, w)), np.arange(max(y0[i], 0), min(y0[i] + bh, h))
        if len(xs) == 0 or len(ys) == 0:
            continue
        out[i][np.ix_(ys, xs)] = _blend(np.pad(mk[i], p), *_axis_in_image(ys, y0[i], bh, mp), *_axis_in_image(xs, x0[i], bw, mp))
    return torch.from_numpy(out)


def support_in_image(boxes, m, p, shape):
    """Per box the integer box clipped to the image, (x_min, y_min, x_max, y_max) inclusive, or None for an all-zero image."""
    x0, y0, x1, y1, finite = integer_boxes(boxes.numpy(), m, p)
    res = []
    for i in range(len(x0)):
        lo_x, lo_y, hi_x, hi_y = max(x0[i], 0), max(y0[i], 0), min(x1[i], shape[1] - 1), min(y1[i], shape[0] - 1)
        res.append((int(lo_x), int(lo_y), int(hi_x), int(hi_y)) if finite[i] and x1[i] >= x0[i] and y1[i] >= y0[i] and lo_x <= hi_x and lo_y <= hi_y else None)
    return res


def support_of(image):
    """The bounding rows and columns of the non-zero pixels of image [H, W], or None."""
    nz = (image != 0).nonzero()
    if nz.numel() == 0:
        return None
    return int(nz[:, 1].min()), int(nz[:, 0].min()), int(nz[:, 1].max()), int(nz[:, 0].max())


def dead_aligned(boxes):
    b = boxes.numpy()
    with np.errstate(all="ignore"):
        return ~(np.isfinite(b).all(1) & (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1]))


def truth_aligned(masks, boxes, shape):
    """float64 [K, H, W] of paste_masks_aligned's value before the threshold, masks [K, Mh, Mw]; a dead row is all zero."""
    mk = masks.double().numpy()
    k, mh, mw = mk.shape
    h, w = shape
    b = boxes.numpy().astype(np.float64)
    dead = dead_aligned(boxes)
    out = np.zeros((k, h, w))
    for i in range(k):
        if dead[i]:
            continue
        p = np.pad(mk[i], 1)
        terms = []
        for n, c0, c1, m in ((h, b[i, 1], b[i, 3], mh), (w, b[i, 0], b[i, 2], mw)):
            s = (np.arange(n) + 0.5 - c0) / (c1 - c0) * m - 0.5
            ok = (s > -1) & (s < m)
            f = np.where(ok, np.floor(s), 0.0)
            terms.append((ok, f.astype(np.int64) + 1, f.astype(np.int64) + 2, np.where(ok, s - f, 0.0)))
        (ok_y, iy, iy1, ly), (ok_x, ix, ix1, lx) = terms
        out[i] = np.where(ok_y[:, None] & ok_x[None, :], _blend(p, iy, iy1, ly, ix, ix1, lx), 0.0)
    return torch.from_numpy(out)


def tolerance(masks, m_prime):
    """tol_k [K] of the module docstring."""
    a = masks.double().abs().reshape(masks.shape[0], -1).amax(1) if masks.shape[0] else torch.zeros(0, dtype=F64)
    return (10 * (m_prime + 1) + 8) * 2.0 ** -24 * a


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.RandomState(seed)


def random_boxes(rng, k, shape, spill=6.0):
    """Boxes of at least 2 pixels a side that lie in or hang over the image."""
    h, w = shape
    x = np.sort(rng.uniform(-spill, w + spill, (k, 2)), axis=1)
    y = np.sort(rng.uniform(-spill, h + spill, (k, 2)), axis=1)
    x[:, 1] += 2
    y[:, 1] += 2
    return torch.from_numpy(np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32))


def random_masks(rng, k, mh, mw, dtype=F32, four=True):
    m = torch.from_numpy(rng.uniform(0.0, 1.0, (k, 1, mh, mw) if four else (k, mh, mw)).astype(np.float32))
    return m.to(dtype)


# paste_masks_in_image, values: name -> (image, K, M, padding, seed)
IN_IMAGE = {
    "m1": ((37, 53), 4, 1, 1, 1), "m2_p0": ((33, 47), 5, 2, 0, 2), "m7": ((33, 47), 8, 7, 1, 3), "m14": ((19, 70), 6, 14, 1, 4),
    "m28": ((37, 53), 8, 28, 1, 5), "m28_p2": ((64, 64), 3, 28, 2, 6), "m14_p0": ((37, 53), 4, 14, 0, 7),
    "m_max": ((16, 16), 2, MAX_SIDE, 1, 8), "pieces": ((150, 231), 3, 28, 1, 9),
}


@functools.lru_cache(maxsize=None)
def in_image_case(name, dtype=F32):
    """(masks [K, 1, M, M] of dtype, boxes [K, 4] float32, image shape, padding); a 16-bit case holds the float32 values rounded."""
    shape, k, m, p, seed = IN_IMAGE[name]
    rng = _rng(seed)
    boxes = random_boxes(rng, k, shape)
    if name == "pieces":                       # one box over most of the image, one inside a single piece, one across the first seam
        boxes = torch.tensor([[-3.5, 4.25, 236.0, 140.5], [40.2, 100.7, 90.9, 118.3], [7.1, 10.2, 60.6, 40.9]], dtype=F32)
    return random_masks(rng, k, m, m, dtype), boxes, shape, p


@functools.lru_cache(maxsize=None)
def in_image_truth(name, dtype=F32):
    masks, boxes, shape, p = in_image_case(name, dtype)
    return truth_in_image(masks, boxes, shape, p)


# paste_masks_in_image, exact: M = 14, padding 1 (M' = 16), mask values multiples of 2^-8, integer sizes 8 .. 64: r is 2, 1, 1/2, 1/4
EXACT_SIZES = ((8, 8), (16, 16), (32, 32), (64, 64), (8, 64), (32, 16))
EXACT_SHAPE, EXACT_M, EXACT_P = (64, 64), 14, 1


@functools.lru_cache(maxsize=None)
def exact_case():
    rng = _rng(20)
    s = float(scale(EXACT_M, EXACT_P))
    rows = []
    for i, (bw, bh) in enumerate(EXACT_SIZES):
        x_c, y_c = 5.0 + 3 * i + bw / 2.0, 2.0 + 2 * i + bh / 2.0            # corners at integer + 0.5: a truncation far from a seam
        hw, hh = (bw - 1) / 2.0 / s, (bh - 1) / 2.0 / s
        rows.append([x_c - hw, y_c - hh, x_c + hw, y_c + hh])
    masks = torch.from_numpy(rng.randint(0, 257, (len(rows), 1, EXACT_M, EXACT_M)).astype(np.float32) / 256)
    return masks, torch.tensor(rows, dtype=F32), EXACT_SHAPE, EXACT_P


# paste_masks_in_image, the seams of the integer box, on all-ones masks.  A padded all-ones mask has a zero border, so the support is
# the whole integer box only while the box is narrower than M' / (2 padding - 1): boxes stay below 29 px at (M 28, padding 1), 5 px at
# (M 14, padding 2); tests/test_ops_mask_cpu.py asserts that the truth's support is the clipped integer box for every row here.
SEAM_SHAPE = (37, 53)
SEAMS = {   # name -> (M, padding, rows)
    "sides": (28, 1, [[-6.3, 10.2, 9.8, 20.7], [44.4, 8.1, 60.2, 25.5], [20.3, -7.7, 33.3, 6.6], [11.2, 30.1, 29.9, 44.4]]),
    "two_sides": (28, 1, [[-4.2, -5.5, 8.8, 7.7], [45.5, 30.3, 58.8, 41.1], [-3.3, 29.5, 6.6, 47.7], [40.1, -9.9, 66.6, 4.4]]),
    "outside": (28, 1, [[-30.5, 5.0, -12.5, 15.0], [60.0, 5.0, 70.0, 15.0], [5.0, -25.0, 15.0, -10.0], [5.0, 45.0, 15.0, 55.0],
                        [-40.0, -40.0, -20.0, -20.0]]),
    "one_pixel": (28, 1, [[10.3, 12.3, 10.6, 12.6], [0.1, 0.1, 0.2, 0.2], [52.2, 36.2, 52.7, 36.7]]),
    "toward_zero": (28, 1, [[-0.4, -0.4, 6.5, 7.5], [-3.2, -3.2, 5.5, 4.5], [-0.9, 3.5, 4.9, 9.5]]),
    "inverted": (28, 1, [[20.0, 10.0, 5.0, 25.0], [5.0, 25.0, 20.0, 10.0], [30.0, 30.0, 10.0, 10.0]]),
    "non_finite": (28, 1, [[NAN, 5.0, 15.0, 15.0], [5.0, 5.0, INF, 15.0], [5.0, -INF, 15.0, 15.0], [5.0, 5.0, 15.0, NAN], [3.0, 4.0, 12.0, 13.0]]),
    "padding_0": (14, 0, [[-6.3, 10.2, 9.8, 20.7], [3.3, 2.2, 50.5, 35.5], [10.3, 12.3, 10.6, 12.6], [44.4, 28.1, 60.2, 45.5]]),
    "padding_2": (14, 2, [[10.2, 11.1, 13.1, 14.2], [-1.5, 20.5, 1.4, 23.3], [50.6, 33.4, 53.9, 35.9], [30.3, 5.5, 30.6, 5.8]]),
    # saturated corners: the image lies in the middle of the first two boxes; the third saturates to the single corner 2^29
    "huge": (28, 1, [[-1e30, -1e30, 1e30, 1e30], [-3e38, 0.0, 3e38, 10.0], [1e9, 1e9, 2e9, 2e9]]),
}

def seam_case(name):
    m, p, rows = SEAMS[name]
    boxes = torch.tensor(rows, dtype=F32)
    return torch.ones((len(rows), 1, m, m), dtype=F32), boxes, SEAM_SHAPE, p


FMA_M, FMA_P = 14, 1


@functools.lru_cache(maxsize=None)
def fma_boxes():
    """Boxes on which a fused multiply-add changes an integer corner, found by a deterministic search: w_half = i / 1024 and integers n
    with x_c -+ fl(w_half s) exactly n, w_half s inexact, (x1, x2) reproducing (x_c, w_half), the corner inside SEAM_SHAPE so that the
    pasted support shows it, and the box narrower than M' so that an all-ones mask fills it.  Returns {kind: float32 [n, 4]} for kind in
    X0, X1, Y0, Y1 (at most 8 each)."""
    s = scale(FMA_M, FMA_P)
    half = np.float32(0.5)
    i = np.arange(1, int(6.0 * 1024))
    wh = (i / 1024.0).astype(np.float32)
    t = (wh * s).astype(np.float32)
    inexact = wh.astype(np.float64) * np.float64(s) != t.astype(np.float64)
    found = {"lo": [], "hi": []}
    for n in range(1, 16):
        for kind, sign in (("lo", -1.0), ("hi", 1.0)):
            c = (np.float32(n) - np.float32(sign) * t).astype(np.float32)         # x_c + sign t = n
            lo, hi = (c - wh).astype(np.float32), (c + wh).astype(np.float32)
            ok = inexact & ((c + np.float32(sign) * t).astype(np.float32) == np.float32(n))
            ok &= (((hi - lo).astype(np.float32) * half).astype(np.float32) == wh) & (((hi + lo).astype(np.float32) * half).astype(np.float32) == c)
            fused = np.trunc((c.astype(np.float64) + sign * wh.astype(np.float64) * np.float64(s)).astype(np.float32))
            ok &= fused != n
            for j in np.nonzero(ok)[0]:
                found[kind].append((float(lo[j]), float(hi[j]), n))
    res = {}
    for kind, axis in (("lo", "X0"), ("hi", "X1"), ("lo", "Y0"), ("hi", "Y1")):
        picks = found[kind][:: max(1, len(found[kind]) // 8)][:8]
        rows = [[lo, 10.25, hi, 17.5] if axis[0] == "X" else [12.25, lo, 19.5, hi] for lo, hi, _ in picks]
        res[axis] = torch.tensor(rows, dtype=F32).reshape(-1, 4)
    return res


# paste_masks_aligned: name -> (image, K, Mh, Mw, seed)
ALIGNED = {
    "a7": ((37, 53), 6, 7, 7, 31), "a14": ((33, 47), 8, 14, 14, 32), "a28": ((19, 70), 5, 28, 28, 33), "a1": ((33, 47), 3, 1, 1, 34),
    "a2": ((64, 64), 4, 2, 2, 35), "a7x14": ((37, 53), 6, 7, 14, 36), "a_max": ((16, 16), 2, MAX_SIDE, MAX_SIDE, 37),
    "pieces": ((150, 231), 3, 28, 28, 38),
}
UINT8_CASES = ("a7", "a14", "a28", "a7x14", "pieces")                      # M <= 28
THRESHOLDS = (0.5, 0.0, 0.9)
ALIGNED_SEAMS = torch.tensor([
    [-6.3, 10.2, 9.8, 20.7], [44.4, -8.1, 60.2, 25.5], [11.2, 30.1, 29.9, 44.4],     # over the image sides
    [12.5, 5.0, 12.5, 20.0],                                                          # x1 == x0
    [30.0, 5.0, 20.0, 20.0], [5.0, 20.0, 20.0, 5.0],                                  # a negative width, a negative height
    [NAN, 5.0, 15.0, 15.0], [5.0, 5.0, INF, 15.0],                                    # non-finite rows
    [20.3, 11.4, 20.6, 11.9],                                                         # smaller than a pixel
    [-400.0, -300.0, 500.0, 350.0],                                                   # much larger than the image
    [3.3, 2.2, 50.5, 35.5]], dtype=F32)
ALIGNED_SEAMS_SHAPE = (37, 53)


@functools.lru_cache(maxsize=None)
def aligned_case(name, dtype=F32):
    """(masks [K, Mh, Mw] of dtype, boxes [K, 4] float32, image shape)."""
    if name == "seams":
        rng = _rng(30)
        return random_masks(rng, len(ALIGNED_SEAMS), 7, 14, dtype, four=False), ALIGNED_SEAMS, ALIGNED_SEAMS_SHAPE
    shape, k, mh, mw, seed = ALIGNED[name]
    rng = _rng(seed)
    boxes = random_boxes(rng, k, shape)
    if name == "pieces":
        boxes = torch.tensor([[-3.5, 4.25, 236.0, 140.5], [40.2, 100.7, 90.9, 118.3], [7.1, 10.2, 60.6, 40.9]], dtype=F32)
    return random_masks(rng, k, mh, mw, dtype, four=False), boxes, shape


@functools.lru_cache(maxsize=None)
def aligned_truth(name, dtype=F32):
    masks, boxes, shape = aligned_case(name, dtype)
    return truth_aligned(masks, boxes, shape)


# masks_to_boxes
BOX_DTYPES = (torch.bool, torch.uint8, torch.float32, torch.float16, torch.bfloat16)


def boxes_truth(masks):
    """float32 [N, 4] by a loop over the masks: the extrema of the non-zero pixels, (0, 0, 0, 0) without one."""
    out = torch.zeros((masks.shape[0], 4), dtype=F32)
    for i, m in enumerate(masks):
        s = support_of(m)
        if s is not None:
            out[i] = torch.tensor(s, dtype=F32)
    return out


@functools.lru_cache(maxsize=None)
def boxes_case(name, dtype):
    """masks [N, H, W] of dtype."""
    rng = _rng(40)
    if name == "random":
        m = torch.from_numpy((rng.uniform(size=(6, 33, 47)) < 0.01).astype(np.float32))
        m[3, 5:20, 7:30] = torch.from_numpy((rng.uniform(size=(15, 23)) < 0.5).astype(np.float32))
    elif name == "corners":
        m = torch.zeros((4, 37, 53))
        m[0, 0, 0] = m[1, 0, 52] = m[2, 36, 0] = m[3, 36, 52] = 1
    elif name == "full":
        m = torch.ones((2, 19, 70))
    elif name == "empty_between":
        m = torch.zeros((3, 33, 47))
        m[0, 3:9, 4:30] = 1
        m[2, 30, 46] = 1
    elif name == "pieces":                         # 150 x 231: several pieces per mask for every element size
        m = torch.zeros((3, 150, 231))
        m[0, 149, 230] = m[0, 0, 100] = 1
        m[1, 70:75, 3] = 1
        m[2] = torch.from_numpy((rng.uniform(size=(150, 231)) < 0.001).astype(np.float32))
    else:
        raise KeyError(name)
    return m.to(dtype)


BOXES_CASES = ("random", "corners", "full", "empty_between", "pieces")
