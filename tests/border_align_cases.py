"""Cases and the restatement of BorderAlign (fasterrcnn_amd.ops.border_align), shared by tests/test_ops_border_cpu.py and
tests/test_ops_border_gpu.py.  The definition is the one include/frcnn_hip.h states (mmcv's border_align restated, unpinned).

reference(case, dtype) is the contract as a loop over (image, box, edge, sample) on numpy scalars of `dtype`, vectorised over the channels
only (every channel of an edge group shares the sample's cells and weights): in float64 it is the truth, with its analytic d_input; in
float32 it is the mirror, written in the kernels' order, whose error against the truth measures the bound of the tolerance tests:
    err(a) = max|a - truth| / max|truth|,   err_gpu <= 4 * max(err_ref, 2**-24),   max|truth| > 0.1.

A flipped argmax moves a whole gradient to another cell, so check_conditions asserts for every element of every tolerance case, with no
element masked: the samples that are not exactly equal to the best one in float64 lie more than 1e-3 * max|truth| below it, and the samples
that are exactly equal to it are exactly equal in the float32 mirror too (equal by construction, not by luck of rounding), so the mirror's
argmax is the truth's.  Two constructions give that: "dyadic" cases have integer map values and every box coordinate and stride a multiple
of 1 / 8, so every position, weight, product and sum is exact in float32 (sample values are multiples of 1 / 64 below 2**6) and ties are
exact; "random" cases are small and take the first seed (base, base + 1000, ...) whose case meets the conditions.
"""
import functools

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
CULL_LIST = 64                                     # ops.BORDER_ALIGN_CULL_LIST (asserted by the CPU test): the boxes a wave tests at once
CULL_BOXES = 16 * CULL_LIST + 1                    # the boxes of "cull": sixteen full groups and one box in a seventeenth
GAP = 1e-3
BELOW = float(np.nextafter(np.float32(-1.0), np.float32(-2.0)))           # one float32 step beyond -1


def above(v):
    """One float32 step beyond v > 0."""
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


NAN, INF = float("nan"), float("inf")

# name: (N, C, H, W), pool_size, kind of map, boxes (a kind or explicit rows per image), seed
CASES = {
    "1x1": ((1, 1, 1, 1), 1, "dyadic", [[(-1, -1, 1, 1), (0, 0, 0, 0), (-0.5, -0.5, 0.5, 0.5), (0.25, -1, 1, 0.5), (-2, 0, 2, 0)]], 1),
    "1xW-c3": ((1, 3, 1, 7), 10, "dyadic", "dyadic", 2),
    "Hx1-c5": ((1, 5, 6, 1), 10, "dyadic", "dyadic", 3),
    "c9-pool64": ((1, 9, 9, 11), 64, "dyadic", "dyadic", 4),
    "c260-two-images": ((2, 260, 5, 4), 10, "dyadic", "dyadic", 5),
    "c1-pool1-random": ((1, 1, 4, 5), 1, "random", "random", 6),
    "c3-two-images-random": ((2, 3, 6, 7), 10, "random", "random", 7),
    # coordinates exactly at -1, 0, H - 1, H and W, and one float32 step beyond -1 and beyond H and W (those samples are 0); an inverted box
    # (pool_size 1, and each stepped coordinate's partner chosen so that x2 - x1 and x1 + (x2 - x1) are exact in float32: the value jumps
    # to 0 at -1 and at the map's size, so the truth and the mirror must put the far end on the same side)
    "edges": ((1, 4, 5, 6), 1, "random",
              [[(-1, -1, 6, 5), (0, 0, 5, 4), (BELOW, 1, 0.5, 2), (1, BELOW, 2, 0.5), (5, 1, above(6), 3), (1, 4, 3, above(5)), (6, 5, -1, -1),
                (-1, 4, 0, 5)]], 8),
    # an inverted box, a zero-width box, a zero-height box and a zero-area box beside a normal one
    "degenerate": ((1, 4, 6, 7), 10, "dyadic", [[(1, 1, 4.75, 3.5), (5, 4.5, 1.25, 0.75), (2.5, 1, 2.5, 4.75), (1, 3.25, 4.75, 3.25),
                                                (3.5, 2.25, 3.5, 2.25)]], 9),
    "constant": ((1, 4, 6, 7), 10, "constant", "dyadic-inside", 10),
    "last-maximum": ((1, 1, 6, 7), 10, "peak", [[(1, 2, 6, 4.5)]], 11),
    "cull": ((1, 1, 3, 3), 1, "dyadic", "cull", 12),
}
TOLERANCE_CASES = list(CASES)
ZERO_STRIDE = {"degenerate": {2: (0, 2), 3: (1, 3), 4: (0, 1, 2, 3)}}     # box row: the edges whose stride is 0 (argmax 0, all on sample 0)
PEAK = (2, 6)                                      # (y, x) of the single maximum of "last-maximum": the top edge's last sample


def _dyadic_boxes(gen, k, h, w, pool, inside=False):
    """Coordinates and strides on multiples of 1 / 8: x1 in the map (or up to two cells outside it), widths pool * stride."""
    def q(lo, hi, n):
        return torch.randint(int(lo * 8), int(hi * 8) + 1, (n,), generator=gen).to(F64) / 8
    step = 1.0 if pool >= 64 else 8.0                                       # strides up to 1 cell (pool 64: 1 / 8 of a cell)
    rows = []
    for _ in range(k):
        if inside:
            x1, y1 = q(0, (w - 1) / 2, 1), q(0, (h - 1) / 2, 1)
            sx = torch.randint(0, max(int((w - 1 - float(x1)) * 8 / pool), 0) + 1, (1,), generator=gen).to(F64) / 8
            sy = torch.randint(0, max(int((h - 1 - float(y1)) * 8 / pool), 0) + 1, (1,), generator=gen).to(F64) / 8
        else:
            x1, y1 = q(-2, w + 1, 1), q(-2, h + 1, 1)
            sx = torch.randint(-int(step), int(step) + 1, (1,), generator=gen).to(F64) / 8
            sy = torch.randint(-int(step), int(step) + 1, (1,), generator=gen).to(F64) / 8
        rows.append(torch.cat([x1, y1, x1 + pool * sx, y1 + pool * sy]))
    return torch.stack(rows)


def _build(name, seed):
    (n, c, h, w), pool, map_kind, box_kind, _ = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    if map_kind == "dyadic":
        x = torch.randint(-4, 5, (n, 4 * c, h, w), generator=gen).to(F32)
    elif map_kind == "random":
        x = torch.randn((n, 4 * c, h, w), generator=gen, dtype=F32)
    elif map_kind == "constant":
        x = torch.full((n, 4 * c, h, w), 1.5, dtype=F32)
    elif map_kind == "peak":
        x = torch.zeros((n, 4 * c, h, w), dtype=F32)
        x[:, :, PEAK[0], PEAK[1]] = 2.0
    else:
        raise KeyError(map_kind)
    if isinstance(box_kind, list):
        boxes = torch.tensor(box_kind, dtype=F64)
    elif box_kind == "dyadic":
        boxes = torch.stack([_dyadic_boxes(gen, 3, h, w, pool) for _ in range(n)])
    elif box_kind == "dyadic-inside":
        boxes = torch.stack([_dyadic_boxes(gen, 4, h, w, pool, inside=True) for _ in range(n)])
    elif box_kind == "random":                     # K = 5, not H W; a different set per image; some reach beyond the map
        k = 5
        x1 = torch.rand((n, k), generator=gen, dtype=F64) * (w + 1) - 1.5
        y1 = torch.rand((n, k), generator=gen, dtype=F64) * (h + 1) - 1.5
        bw = (torch.rand((n, k), generator=gen, dtype=F64) - 0.3) * w
        bh = (torch.rand((n, k), generator=gen, dtype=F64) - 0.3) * h
        boxes = torch.stack([x1, y1, x1 + bw, y1 + bh], 2)
    elif box_kind == "cull":                       # more boxes than a wave tests at once, all over a 3 x 3 map: every tile meets later groups
        boxes = _dyadic_boxes(gen, CULL_BOXES, h, w, pool)[None]
    else:
        raise KeyError(box_kind)
    boxes = boxes.to(F32)
    grad = torch.randn((n, c, boxes.shape[1], 4), generator=gen, dtype=F32)
    return {"name": name, "input": x, "boxes": boxes, "pool_size": pool, "grad": grad, "seed": seed}


def _axis(v, size, ft):
    """roi_align's rule for one coordinate known to lie in [-1, size]: (low, high, weight of low, weight of high) in the scalar type ft."""
    if v <= 0:
        v = ft(0)
    low = int(v)
    if low >= size - 1:
        low = high = size - 1
        v = ft(low)
    else:
        high = low + 1
    wh = v - ft(low)
    return low, high, ft(1) - wh, wh


def samples(case, dtype):
    """Every sample of the case in numpy scalars of `dtype`: plan[n][k][e][i] = None (outside the range: exactly 0, no gradient) or
    (yl, yh, xl, xh, w1, w2, w3, w4), and vals [N, C, K, 4, P + 1]."""
    ft = np.float64 if dtype == F64 else np.float32
    x = case["input"].numpy().astype(ft)
    boxes = case["boxes"].numpy().astype(ft)
    pool = case["pool_size"]
    n, c4, h, w = x.shape
    c, k = c4 // 4, boxes.shape[1]
    vals = np.zeros((n, c, k, 4, pool + 1), dtype=ft)
    plan = [[[[None] * (pool + 1) for _ in range(4)] for _ in range(k)] for _ in range(n)]
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(n):
            for r in range(k):
                x1, y1, x2, y2 = boxes[b, r]
                for e in range(4):
                    along_x = e % 2 == 0
                    s = ((x2 - x1) if along_x else (y2 - y1)) / ft(pool)
                    step = -s if e >= 2 else s
                    x0, y0 = (x2, y2) if e >= 2 else (x1, y1)
                    dx, dy = (step, ft(0)) if along_x else (ft(0), step)
                    fm = x[b, e * c:(e + 1) * c]
                    for i in range(pool + 1):
                        sx, sy = x0 + ft(i) * dx, y0 + ft(i) * dy
                        if not (-1 <= sy <= h and -1 <= sx <= w):          # a NaN fails
                            continue
                        yl, yh, wyl, wyh = _axis(sy, h, ft)
                        xl, xh, wxl, wxh = _axis(sx, w, ft)
                        w1, w2, w3, w4 = wyl * wxl, wyl * wxh, wyh * wxl, wyh * wxh
                        plan[b][r][e][i] = (yl, yh, xl, xh, w1, w2, w3, w4)
                        vals[b, :, r, e, i] = ((fm[:, yl, xl] * w1 + fm[:, yl, xh] * w2) + fm[:, yh, xl] * w3) + fm[:, yh, xh] * w4
    return plan, vals


def reference(case, dtype):
    """(output [N, C, K, 4], argmax int64 [N, C, K, 4], d_input [N, 4 C, H, W], vals) of the contract in `dtype`, as torch tensors."""
    ft = np.float64 if dtype == F64 else np.float32
    plan, vals = samples(case, dtype)
    best = vals[..., 0].copy()
    arg = np.zeros(best.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(1, vals.shape[-1]):
            m = vals[..., i] > best                                         # a NaN sample never wins; a NaN at i = 0 stays
            best[m] = vals[..., i][m]
            arg[m] = i
    grad = case["grad"].numpy().astype(ft)
    n, c, k, _ = best.shape
    dx = np.zeros(tuple(case["input"].shape), dtype=ft)
    for b in range(n):
        for r in range(k):
            for e in range(4):
                for i, cells in enumerate(plan[b][r][e]):
                    if cells is None:
                        continue
                    ch = np.nonzero(arg[b, :, r, e] == i)[0]
                    if ch.size == 0:
                        continue
                    yl, yh, xl, xh, w1, w2, w3, w4 = cells
                    g = grad[b, ch, r, e]
                    for yy, (wa, wb) in ((yl, (w1, w2)), (yh, (w3, w4))):  # a collapsed pair is one cell: its second weight is 0
                        dx[b, e * c + ch, yy, xl] += g * wa
                        dx[b, e * c + ch, yy, xh] += g * wb
    return torch.from_numpy(best), torch.from_numpy(arg), torch.from_numpy(dx), torch.from_numpy(vals)


def conditions_hold(case, truth, mirror):
    """The argmax condition and max|truth| > 0.1 (see the module's docstring); returns a message, or None when they hold."""
    out, arg, dx, vals = truth
    m_out, m_arg, m_dx, m_vals = mirror
    if not (float(out.abs().max()) > 0.1 and float(dx.abs().max()) > 0.1):
        return "max|truth| <= 0.1"
    if not bool(torch.isfinite(vals).all()):
        return "non-finite samples"
    best = vals.max(dim=-1, keepdim=True).values
    tied = vals == best
    if bool(((best - vals)[~tied] <= GAP * float(out.abs().max())).any()):
        return "a runner-up within 1e-3 max|truth| of the best sample"
    m_best = torch.where(tied, m_vals, torch.full_like(m_vals, -INF)).max(dim=-1, keepdim=True).values
    if not bool((m_vals[tied] == m_best.expand_as(m_vals)[tied]).all()):
        return "samples tied in float64 differ in float32"
    if not torch.equal(arg, m_arg):
        return "the float32 mirror's argmax differs"
    return None


def check_conditions(case, truth, mirror):
    message = conditions_hold(case, truth, mirror)
    assert message is None, (case["name"], message)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The case with its float64 truth and float32 mirror, (case, truth, mirror), computed once; a "random" case takes the first seed of
    base, base + 1000, ... that meets the conditions."""
    base = CASES[name][4]
    for attempt in range(64):
        case = _build(name, base + 1000 * attempt)
        truth, mirror = reference(case, F64), reference(case, F32)
        if CASES[name][2] != "random" or conditions_hold(case, truth, mirror) is None:
            return case, truth, mirror
    raise AssertionError("no seed of %s meets the conditions" % name)


def rel_err(a, truth):
    return float((a.double() - truth.double()).abs().max()) / float(truth.double().abs().max())


def nonfinite_case():
    """A normal box beside boxes of NaN and infinite coordinates: every sample of those is outside the range (zeros out, no gradient)."""
    case = dict(_build("c3-two-images-random", 7))
    n, k = case["boxes"].shape[:2]
    bad = torch.tensor([(NAN, NAN, NAN, NAN), (INF, INF, INF, INF), (-INF, -INF, INF, INF), (-INF, -INF, -INF, -INF), (NAN, 1, 3, INF),
                        (INF, NAN, -INF, 2)], dtype=F32)
    case["boxes"] = torch.cat([case["boxes"][:, :1], bad[None].expand(n, -1, -1)], dim=1).contiguous()
    gen = torch.Generator().manual_seed(70)
    case["grad"] = torch.randn((n, case["input"].shape[1] // 4, 1 + bad.shape[0], 4), generator=gen, dtype=F32)
    return case


def nan_pixel_case():
    """A NaN pixel at (2, 3) of every channel: box 0's top and left edges start on it (i = 0: the NaN stays), box 1's top edge reaches it at
    i = 2 and its other edges never (the NaN never replaces the running value), box 2 never touches it."""
    case = dict(_build("degenerate", 9))
    case["input"] = case["input"].clone()
    case["input"][:, :, 2, 3] = NAN
    case["pool_size"] = 4
    case["boxes"] = torch.tensor([[(3, 2, 5, 4), (1, 2, 5, 4.5), (0, 3.5, 1.5, 5)]], dtype=F32)
    gen = torch.Generator().manual_seed(71)
    case["grad"] = torch.randn((1, 4, 3, 4), generator=gen, dtype=F32)
    return case
