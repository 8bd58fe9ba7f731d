"""Cases of fasterrcnn_amd.ops.heatmaps_to_keypoints, a float32 mirror of the kernel, a float64 truth and a derived error bound; numpy and
torch on the CPU only.

(a) mirror(): the contract of include/frcnn_hip.h in numpy float32, every operation a separate float32 ufunc in the header's order
    (source coordinate, weights, rows combined first, each sum from the left, the (value, index) order, the float32 x and y).  The
    kernel must give its x, y and logit bit for bit.

(b) truth(): the same bicubic resize (Keys' kernel, A = -0.75, scale * (d + 0.5) - 0.5 not clamped, tap indices clamped) in float64 on
    the float32 inputs, with the integer sizes W, H taken from the float32 sequence, and the defined cases of the header (a constant map
    is its own image; a refused RoI gives NaNs).

(c) bound(): per output element, derived, not measured (u = 2^-24; n source pixels of an axis):
    - A weight is a cubic in t evaluated by Horner's rule.  Following the six roundings of an outer weight through magnitudes of at
      most 1.5, 3, 4.5, 3, 3.1 and 0.12, and the rounding of its argument t + 1 (2 u, times a slope of at most 0.75), its absolute
      error is at most 38 u; the four roundings of an inner weight (magnitudes 1.25, 2.25, 2.25, 2.25, 1) and of 1 - t give 10 u.
      EPS = (38, 10, 10, 38) u.
    - The sixteen products and the two sums of four, each from the left, cost at most 9 u of sum |cy_a| |cx_b| |M_ab| (4 u per sum of
      four products, the first carried through the second, second-order terms rounded up).
    - The source coordinate: scale is one rounded division, scale * (d + 0.5) one rounded product of magnitude at most n, - 0.5 one
      more rounding; t = src - floor(src) is exact.  So |src_float32 - src| <= DELTA(n) = 3 u (n + 1).  The interpolant is C1 in src,
      across the knots too (where the taps shift by one), so the value moves by at most DELTA times the local slope, and the slope along
      an axis is at most sum |c'_b| |other weights| |M_ab| with |c'| <= SLOPE = (0.75, 1.35, 1.35, 0.75): the suprema over t of the
      derivatives of the outer and inner cubics, which also cover the neighbouring interval at a knot; the second-order term is 1e-4
      of the first.
    bound(y, x) = [EPS_y x |cx|] + [(|cy| + EPS_y) x EPS_x] + 9 u [|cy| x |cx|] + DELTA(mh) [SLOPE x |cx|] + DELTA(mw) [|cy| x SLOPE],
    where [P x Q] is the resize of |M| with row weights P and column weights Q.  It holds for every evaluation of the sixteen products
    with float32 weights of this form, in any order: the kernel's and torch's F.interpolate alike.  A (RoI, keypoint) pair's bound is
    the largest over its image.
    prob = 1 / sum exp(M - v): v is within the pair's bound B of the truth's maximum; M - v is one rounding of magnitude at most
    D = max |M - v|; expf is accurate to an ulp (2 u); a sum of n positive terms in ANY order loses at most n u; the division u.
    So |prob - truth| <= 1.01 truth (B + (D + n + 3) u).

Everything is tiny: K = 3, maps of side 1, 2, 3, 7, 5 x 9, 14, 28, 56 and the stated maximum; the largest image is 300 x 411."""
import functools
import math

import numpy as np
import torch

from fasterrcnn_amd import ops

F32, F64 = torch.float32, torch.float64
HALF = (torch.float16, torch.bfloat16)
K = 3
MAX_MAP = ops.MAX_KEYPOINT_MAP_SIDE
MAX_SIDE = ops.MAX_KEYPOINT_ROI_SIDE
WAVES = ops.KEYPOINT_BLOCK_THREADS // 64          # output rows of one pass of a block
LANES = 64                                        # pixels of a row one wave takes per step
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -24
EPS = np.array([38.0, 10.0, 10.0, 38.0]) * U
SLOPE = np.array([0.75, 1.35, 1.35, 0.75])
LEFT_OUT_SHARE = 0.05

f32 = np.float32


def box(w, h, x1=3.25, y1=7.5):
    return (x1, y1, x1 + w, y1 + h)


# name -> ((mh, mw), boxes).  Sizes are (w, h) of the box; W = ceil(max(w, 1)).
CASES = {
    # every tap clamps; a 1 x 1 map is a constant map
    "m1": ((1, 1), [box(1, 1), box(5, 3), box(20, 7)]),
    # taps clamp on both sides
    "m2": ((2, 2), [box(1, 1), box(4, 4), box(9, 5), box(30, 17), box(2, 1)]),
    # taps clamp on one side
    "m3": ((3, 3), [box(1, 1), box(3, 3), box(10, 4), box(2, 2), box(31, 18)]),
    # one pixel, one row, one column, fractional sizes on either side of an integer, sizes under 1, inverted boxes, a shrinking resize
    "m7": ((7, 7), [box(1, 1), box(20, 1), box(1, 20), box(13, 5), box(12.999, 5.001), box(13.001, 4.999), box(0.5, 0.25), box(-4, 9),
                    box(9, -4), box(3, 4), box(6.5, 21.75, -11.5, -3.25), box(200, 150)]),
    # a non-square map, both ways round
    "rect": ((5, 9), [box(3, 2), box(17, 11), box(9, 5), box(40, 64)]),
    # one pixel fewer than a wave's step, exactly a step, one more; one row fewer than a pass, exactly a pass, one more
    "seams": ((14, 14), [box(LANES - 1, WAVES - 1), box(LANES, WAVES), box(LANES + 1, WAVES + 1), box(LANES, WAVES + 1),
                         box(LANES + 1, WAVES - 1), box(2 * LANES + 1, 2 * WAVES + 1), box(2 * LANES, 2 * WAVES)]),
    # the usual head: an image smaller than the map (taps skip source pixels) and much larger ones
    "m56": ((56, 56), [box(20, 20), box(57, 200), box(300, 411), box(133.3, 80.7)]),
    # the largest map
    "m_max": ((MAX_MAP, MAX_MAP), [box(20, 20), box(130, 117), box(1, 1)]),
    # the largest side, either way, and the last fractional size under it
    "side": ((7, 7), [box(MAX_SIDE, 2), box(2.5, MAX_SIDE - 0.5)]),
    # the mask heads' other sizes; the identity resize (scale 1: every weight is 0 or 1)
    "m14": ((14, 14), [box(14, 14), box(50, 31), box(7, 7)]),
    "m28": ((28, 28), [box(28, 28), box(90, 45)]),
}
SEEDS = {name: 100 + i for i, name in enumerate(CASES)}


@functools.lru_cache(maxsize=None)
def case(name, dtype=F32):
    """(maps [R, K, mh, mw] of dtype, rois [R, 4] float32), the maps randn * 3 (a 16-bit dtype: rounded to it)."""
    (mh, mw), boxes = CASES[name]
    g = torch.Generator().manual_seed(SEEDS[name])
    maps = torch.randn((len(boxes), K, mh, mw), generator=g) * 3
    return maps.to(dtype), torch.tensor(boxes, dtype=F32)


# ---- the float32 sequence shared by the mirror and the truth ------------------------------------------------------------------------
def sizes(roi):
    """(w, h, W, H) of one float32 RoI by the header's float32 sequence, or None for a refused one."""
    x1, y1, x2, y2 = (f32(v) for v in roi)
    if not np.isfinite([x1, y1, x2, y2]).all():
        return None
    with np.errstate(over="ignore"):
        w, h = np.maximum(f32(x2 - x1), f32(1)), np.maximum(f32(y2 - y1), f32(1))
    wc, hc = np.ceil(w), np.ceil(h)
    if not (wc <= MAX_SIDE and hc <= MAX_SIDE):
        return None
    return w, h, int(wc), int(hc)


def coordinates(roi, w, h, wc, hc, xi, yi):
    """The float32 (x, y) of pixel (xi, yi): (xi + 0.5) * (w / W) + x1."""
    x = f32(f32(f32(xi) + f32(0.5)) * f32(w / f32(wc))) + f32(roi[0])
    y = f32(f32(f32(yi) + f32(0.5)) * f32(h / f32(hc))) + f32(roi[1])
    return f32(x), f32(y)


def is_constant(m):
    return bool((m == m.flat[0]).all())


# ---- (a) the float32 mirror ------------------------------------------------------------------------------------------------------------
def taps32(n, big_n):
    d = np.arange(big_n, dtype=f32)
    scale = f32(n) / f32(big_n)
    src = scale * (d + f32(0.5)) - f32(0.5)
    f = np.floor(src)
    t = src - f
    i = f.astype(np.int64)
    idx = np.stack([np.clip(i - 1 + j, 0, n - 1) for j in range(4)], 1)
    u0, u2 = t + f32(1), f32(1) - t
    u3 = u2 + f32(1)
    c0 = ((f32(-0.75) * u0 + f32(3.75)) * u0 - f32(6)) * u0 + f32(3)
    c1 = (f32(1.25) * t - f32(2.25)) * t * t + f32(1)
    c2 = (f32(1.25) * u2 - f32(2.25)) * u2 * u2 + f32(1)
    c3 = ((f32(-0.75) * u3 + f32(3.75)) * u3 - f32(6)) * u3 + f32(3)
    c = np.stack([c0, c1, c2, c3], 1)
    assert c.dtype == f32 and src.dtype == f32
    return idx, c


def first_maximum(flat):
    """The (value, index) order of the header: a NaN above every number, the first one; else the first of the largest."""
    nan = np.isnan(flat)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(flat))


def mirror_image(m, big_h, big_w):
    mh, mw = m.shape
    iy, cy = taps32(mh, big_h)
    ix, cx = taps32(mw, big_w)
    with np.errstate(all="ignore"):
        v = ((cy[:, 0, None] * m[iy[:, 0]] + cy[:, 1, None] * m[iy[:, 1]]) + cy[:, 2, None] * m[iy[:, 2]]) + cy[:, 3, None] * m[iy[:, 3]]
        img = ((cx[None, :, 0] * v[:, ix[:, 0]] + cx[None, :, 1] * v[:, ix[:, 1]]) + cx[None, :, 2] * v[:, ix[:, 2]]) + cx[None, :, 3] * v[:, ix[:, 3]]
    assert img.dtype == f32
    return img


def mirror(maps, rois):
    """float32 [R, K, 4] = (x, y, logit, prob): x, y, logit as the kernel must give them, bit for bit; prob in float32, any order."""
    maps, rois = maps.float().numpy(), rois.numpy().astype(f32)
    r, k = maps.shape[:2]
    out = np.full((r, k, 4), np.nan, dtype=f32)
    for i in range(r):
        s = sizes(rois[i])
        if s is None:
            continue
        w, h, wc, hc = s
        for j in range(k):
            m = maps[i, j]
            if is_constant(m):
                pos, v = 0, m.flat[0]
            else:
                img = mirror_image(m, hc, wc).reshape(-1)
                pos = first_maximum(img)
                v = img[pos]
            x, y = coordinates(rois[i], w, h, wc, hc, pos % wc, pos // wc)
            with np.errstate(all="ignore"):
                out[i, j] = (x, y, v, f32(1) / np.sum(np.exp(m - v), dtype=f32))
    return torch.from_numpy(out)


# ---- (b) the float64 truth and (c) the bound -------------------------------------------------------------------------------------------
def taps64(n, big_n):
    src = (n / big_n) * (np.arange(big_n, dtype=np.float64) + 0.5) - 0.5
    f = np.floor(src)
    t = src - f
    i = f.astype(np.int64)
    idx = np.stack([np.clip(i - 1 + j, 0, n - 1) for j in range(4)], 1)
    a = -0.75

    def inner(x):
        return ((a + 2) * x - (a + 3)) * x * x + 1

    def outer(x):
        return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
    return idx, np.stack([outer(t + 1), inner(t), inner(1 - t), outer(2 - t)], 1)


def resize64(m, iy, py, ix, px):
    """sum over a, b of py[y, a] px[x, b] m[iy[y, a], ix[x, b]]: [H, W] float64, rows first."""
    with np.errstate(all="ignore"):
        v = sum(py[:, a, None] * m[iy[:, a]] for a in range(4))
        return sum(px[None, :, b] * v[:, ix[:, b]] for b in range(4))


class Pair:
    """The truth of one (RoI, keypoint): image [H, W] float64 (None when refused), pos / value of its maximum under the header's order,
    gap to the second largest value (inf for one pixel or a constant map), bound (the pair's), prob."""


def truth_pair(m, s):
    p = Pair()
    p.sizes = s
    if s is None:
        p.image = None
        return p
    w, h, wc, hc = s
    m = m.astype(np.float64)
    p.constant = is_constant(m)
    if p.constant:
        p.image = np.full((hc, wc), m.flat[0])
        p.pos, p.value, p.gap, p.bound = 0, m.flat[0], INF, 0.0
    else:
        mh, mw = m.shape
        iy, cy = taps64(mh, hc)
        ix, cx = taps64(mw, wc)
        p.image = resize64(m, iy, cy, ix, cx)
        flat = p.image.reshape(-1)
        p.pos = first_maximum(flat)
        p.value = flat[p.pos]
        if flat.size > 1 and not np.isnan(flat).any():
            top = np.partition(flat, flat.size - 2)[-2:]
            p.gap = float(top[1] - top[0])
        else:
            p.gap = INF
        ma, ay, ax = np.abs(m), np.abs(cy), np.abs(cx)
        ey, ex = np.broadcast_to(EPS, cy.shape), np.broadcast_to(EPS, cx.shape)
        sy, sx = np.broadcast_to(SLOPE, cy.shape), np.broadcast_to(SLOPE, cx.shape)
        b = (resize64(ma, iy, ey, ix, ax) + resize64(ma, iy, ay + ey, ix, ex) + 9 * U * resize64(ma, iy, ay, ix, ax)
             + 3 * U * (mh + 1) * resize64(ma, iy, sy, ix, ax) + 3 * U * (mw + 1) * resize64(ma, iy, ay, ix, sx))
        p.bound = float(np.max(b)) if np.isfinite(b).all() else INF
    with np.errstate(all="ignore"):
        d = m - p.value
        p.prob = 1.0 / np.sum(np.exp(d))
        p.prob_tol = 1.01 * p.prob * (p.bound + (np.max(np.abs(d)) + m.size + 3) * U)
    return p


def truth_of(maps, rois):
    """[[Pair] * K] * R for float32-valued maps [R, K, mh, mw] and float32 rois."""
    maps, rois = maps.float().numpy(), rois.numpy().astype(f32)
    return [[truth_pair(maps[i, j], sizes(rois[i])) for j in range(maps.shape[1])] for i in range(maps.shape[0])]


@functools.lru_cache(maxsize=None)
def truth(name, dtype=F32):
    return truth_of(*case(name, dtype))


def position_of(got_xy, roi, s):
    """The pixel (xi, yi) whose float32 coordinates are got_xy exactly, as an index yi * W + xi; None if there is none."""
    w, h, wc, hc = s
    xs = np.array([coordinates(roi, w, h, wc, hc, xi, 0)[0] for xi in range(wc)])
    ys = np.array([coordinates(roi, w, h, wc, hc, 0, yi)[1] for yi in range(hc)])
    xi, yi = np.nonzero(xs == f32(got_xy[0]))[0], np.nonzero(ys == f32(got_xy[1]))[0]
    if len(xi) != 1 or len(yi) != 1:
        return None
    return int(yi[0]) * wc + int(xi[0])


def judge(got, maps, rois, pairs):
    """The rules of the issue for got [R, K, 4] against the truth: returns (largest |error| / bound over optimality and logit, largest
    prob error / its tolerance, pairs left out of the position comparison, pairs); raises AssertionError on a position that differs
    outside the left-out pairs or on coordinates that are no pixel's."""
    got, rois = got.double().numpy(), rois.numpy().astype(f32)
    worst, worst_prob, left_out, total = 0.0, 0.0, 0, 0
    for i, row in enumerate(pairs):
        for j, p in enumerate(row):
            total += 1
            x, y, logit, prob = got[i, j]
            if p.image is None:
                assert np.isnan(got[i, j]).all(), (i, j, got[i, j])
                continue
            pos = position_of((x, y), rois[i], p.sizes)
            assert pos is not None, (i, j, x, y)
            at = p.image.reshape(-1)[pos]
            if p.bound == 0:
                assert pos == p.pos and logit == p.value, (i, j, pos, logit)
            else:
                worst = max(worst, (p.value - at) / p.bound, abs(logit - p.value) / p.bound)
                if p.gap > 2 * p.bound:
                    assert pos == p.pos, (i, j, pos, p.pos, p.gap, p.bound)
                else:
                    left_out += 1
            if np.isfinite(p.prob) and p.prob_tol > 0:
                worst_prob = max(worst_prob, abs(prob - p.prob) / p.prob_tol)
    return worst, worst_prob, left_out, total


# ---- the defined cases --------------------------------------------------------------------------------------------------------------
def two_peaks():
    """8 x 8 zero maps with two equal peaks, resized by exactly 2 (every coordinate and weight exact): the images hold their maximum
    at eight pixels (each peak lies between four), bit for bit; the smallest y * W + x wins.  Returns (maps [1, K, 8, 8], rois [1, 4], the winning (xi, yi) per map)."""
    maps = torch.zeros((1, K, 8, 8))
    for j, (a, b) in enumerate((((2, 2), (5, 5)), ((2, 5), (5, 2)), ((5, 1), (5, 5)))):       # (row, column) pairs
        maps[0, j][a] = maps[0, j][b] = 4.0
    return maps, torch.tensor([box(16, 16)], dtype=F32)


def refused_rois():
    big = 3.0e38
    return torch.tensor([box(MAX_SIDE + 1, 4), box(4, MAX_SIDE + 0.5), (NAN, 0, 5, 5), (0, 0, INF, 5), (0, -INF, 5, 5), (-big, 0, big, 5),
                         box(9, 9)], dtype=F32)


def check_defined_cases(f, dev, bitwise):
    """Asserts the defined cases of the header on f(maps, rois) -> [R, K, 4] with its inputs on dev: the twin on the CPU, the operator and
    the twin on the GPU.  bitwise: f is the operator, whose numbers beside the defined ones are the mirror's bit for bit."""
    run = lambda maps, rois: f(maps.to(dev), rois.to(dev)).cpu()                # noqa: E731
    roi = torch.tensor([box(13, 5)], dtype=F32)
    # a constant map: (0, 0), its own value, 1 / (mh mw); -0.0 == +0.0
    maps = torch.full((1, K, 7, 9), 2.7)
    maps[0, 1] = 0.0
    maps[0, 1, 3, 3] = -0.0
    maps[0, 2] = -1e30
    got = run(maps, roi)
    x0, y0 = coordinates(roi[0].numpy(), *sizes(roi[0].numpy()), 0, 0)
    for j, v in enumerate((2.7, 0.0, -1e30)):
        assert got[0, j, 0] == x0 and got[0, j, 1] == y0 and got[0, j, 2] == np.float32(v), got[0, j]
        assert abs(float(got[0, j, 3]) - 1 / 63) <= 1e-6 / 63
    # two equal peaks: the smaller y * W + x
    maps, rois = two_peaks()
    got = run(maps, rois)
    want = mirror(maps, rois)
    truth = truth_of(maps, rois)[0]
    for j in range(K):
        p = truth[j]
        assert p.gap == 0 and int((p.image == p.value).sum()) == 8 and position_of(got[0, j, :2].numpy(), rois[0].numpy(), p.sizes) == p.pos
        assert torch.equal(got[0, j, :3], want[0, j, :3]) and float(got[0, j, 2]) == p.value
    # a NaN: the first pixel whose taps touch it; logit and prob are NaN
    maps, rois = case("m7")
    maps = maps[3:6].clone()
    maps[0, 0, 3, 4] = NAN
    maps[1, 1, 0, 0] = NAN
    maps[2, 2, 6, 6] = NAN
    maps[2, 0, 2, 2] = INF                                                      # inf with numbers: NaNs around it (inf - inf in the taps)
    maps[2, 1, 5, 1] = -INF
    rois = rois[3:6]
    got, want = run(maps, rois), mirror(maps, rois)
    nan = want[..., 2].isnan()
    assert torch.equal(got[..., :2][nan], want[..., :2][nan]) and torch.equal(got[..., 2].isnan(), nan)
    assert not bitwise or torch.equal(got[..., :3].nan_to_num(7.0), want[..., :3].nan_to_num(7.0))
    assert [bool(v) for v in got[..., 2].isnan().flatten()] == [True, False, False, False, True, False, True, True, True]
    assert torch.equal(got[..., 3].isnan(), got[..., 2].isnan())
    s = sizes(rois[1].numpy())
    assert position_of(got[1, 1, :2].numpy(), rois[1].numpy(), s) == 0       # the NaN at map (0, 0) reaches image pixel (0, 0)
    # an all -inf map is a constant map: (0, 0), -inf, prob NaN; all +inf likewise
    maps = torch.full((1, K, 7, 9), -INF)
    maps[0, 1] = INF
    maps[0, 2, 2, 2] = 1.0                                                      # -inf with one number: NaNs around it, not a constant map
    got = run(maps, roi)
    assert got[0, 0, 0] == x0 and got[0, 0, 1] == y0 and got[0, 0, 2] == -INF and math.isnan(got[0, 0, 3])
    assert got[0, 1, 0] == x0 and got[0, 1, 1] == y0 and got[0, 1, 2] == INF and math.isnan(got[0, 1, 3])
    assert math.isnan(got[0, 2, 2]) and math.isnan(got[0, 2, 3]) and got[0, 2, 0] == x0 and got[0, 2, 1] == y0
    # refused RoIs: four NaNs; the others are not disturbed
    rois = refused_rois()
    maps = torch.randn((len(rois), K, 7, 7), generator=torch.Generator().manual_seed(5)) * 3
    got = run(maps, rois)
    assert bool(got[:-1].isnan().all()) and bool(got[-1].isfinite().all())
    assert not bitwise or torch.equal(got[-1:, :, :3], mirror(maps[-1:], rois[-1:])[..., :3])
    # R == 0 and K == 0
    assert run(torch.zeros(0, K, 7, 7), torch.zeros(0, 4)).shape == (0, K, 4)
    assert run(torch.zeros(4, 0, 7, 7), torch.zeros(4, 4)).shape == (4, 0, 4)
