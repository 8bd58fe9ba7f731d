"""Cases and two float64 restatements of Precise RoI Pooling (fasterrcnn_amd.ops.prroi_pool), shared by tests/test_ops_prroi_cpu.py and
tests/test_ops_prroi_gpu.py.  The definition is the one include/frcnn_hip.h states (mmcv's prroi_pool restated, unpinned).

Restatement A (forward_ref, grads_ref) is the separable one: the weight matrices Wy [K, oh, H] and Wx [K, ow, W] from the two unit pieces
either side of each cell, one contraction, and the analytic box gradient from the four line integrals.  It runs in float64 (the truth) or
in float32 (whose error against the truth measures the bound of the GPU tests) and writes its float32 expressions in the kernels' order.
Restatement B (forward_direct, input_grad_direct, roi_grad_direct) shares no expression with it: a double loop over the cells with the
weights as differences of the antiderivative of hat, bin edges as X1 + p (X2 - X1) / n, and the box gradient by central differences of
the float64 forward.  The CPU test requires the two to agree.

The operator is C1 in the box wherever the box has area, so no bin is masked: integer coordinates are not seams.  check_conditions
asserts what the relative errors of the GPU tests need: every compared quantity has max|truth| > 0.1 (the cases scale grad for it).
"""
import functools

import torch

F32, F64 = torch.float32, torch.float64
CULL_LIST = 1024                                   # ops.PRROI_CULL_LIST (asserted by the CPU test)
STEP = 2.0 ** -20                                  # central differences of restatement B


def f32(v):
    """A Python float rounded to float32, as the kernels receive spatial_scale."""
    return float(torch.tensor(v, dtype=F32))


# name: (N, C, H, W), output_size, spatial_scale, RoI kind, grad scale, seed
CASES = {
    # boxes inside the map, in map coordinates after the scale 0.5; the first two have every bin edge on an integer
    "6x7-integer-edges": ((1, 4, 6, 7), (2, 3), 0.5, "integer", 1.0, 31),
    "c6-7x7": ((1, 6, 9, 11), (7, 7), 1.0, "inside", 1.0, 32),
    "c260-two-images": ((2, 260, 5, 4), (3, 5), 1.0, "inside", 1.0, 33),
    "borders": ((1, 4, 6, 7), (2, 3), 1.0, "borders", 1.0, 34),
    "beyond": ((1, 4, 6, 7), (2, 3), 1.0, "beyond", 1.0, 35),
    "1x1": ((1, 4, 1, 1), (2, 2), 1.0, "one-cell", 1.0, 36),
    "narrow": ((1, 4, 6, 7), (7, 7), 1.0, "narrow", 1.0, 37),
    "out64": ((1, 4, 5, 4), (64, 64), 1.0, "inside", 1.0, 38),
    "whole-1x1": ((1, 4, 6, 7), (1, 1), 1.0, "whole", 4.0, 39),
    "cull": ((1, 4, 3, 3), (1, 1), 1.0, "cull", 1.0, 40),
}
BEYOND_ROW = 1                                     # the row of "beyond" that lies wholly outside the one-cell margin


def _rois(gen, n, h, w, kind, scale):
    """float32 [K, 5] in image coordinates (map coordinates / scale)."""
    def u(k, lo, hi):
        return torch.rand((k,), generator=gen, dtype=F64) * (hi - lo) + lo
    if kind == "integer":
        box = torch.tensor([[0.0, 1.0, 6.0, 5.0], [3.0, 0.0, 6.0, 4.0], [1.3, 0.7, 4.9, 4.1]], dtype=F64)
    elif kind == "inside":
        k = 6
        x1, y1 = u(k, 0.0, 0.45 * (w - 1)), u(k, 0.0, 0.45 * (h - 1))
        x2, y2 = x1 + u(k, 0.3, 0.5) * (w - 1), y1 + u(k, 0.3, 0.5) * (h - 1)
        box = torch.stack([x1, y1, x2, y2], 1)
    elif kind == "borders":                        # left, top, right, bottom, and all four at once
        box = torch.tensor([[-2.3, 1.2, 2.6, 4.1], [1.4, -1.7, 5.2, 2.3], [3.3, 0.6, w + 1.4, 3.9], [0.8, 2.2, 4.4, h + 0.8],
                            [-1.5, -1.5, w + 0.5, h + 0.5]], dtype=F64)
    elif kind == "beyond":
        box = torch.tensor([[1.2, 0.9, 5.1, 4.3], [w + 0.5, 1.0, w + 3.0, 4.0], [0.4, 1.1, 3.0, 3.7]], dtype=F64)
    elif kind == "one-cell":
        box = torch.tensor([[-0.7, -0.6, 0.8, 0.9], [-0.2, -1.4, 0.5, 0.3], [0.1, 0.2, 1.6, 0.7]], dtype=F64)
    elif kind == "narrow":
        # 7 / 128 of a cell wide and high, so with out 7 x 7 every bin is 1 / 128 of a cell and lies inside one unit piece; the corners lie
        # on odd multiples of 2**-20, so every bin edge and every midpoint is exact in float32 (23 bits).  The unit-piece weights are then
        # exact and the float32 restatement's error stays at a few 2**-24, where a difference of antiderivatives -- squares of 21-bit
        # numbers, rounded to 2**-25, at most 1 / 128 apart -- is off by about 2**-18 of a weight: the ratio rule tells the two apart.
        k = 6
        x1 = u(k, 0.5, w - 1.5).floor() + ((u(k, 0.05, 0.85) * 2 ** 19).floor() * 2 + 1) / 2 ** 20
        y1 = u(k, 0.5, h - 1.5).floor() + ((u(k, 0.05, 0.85) * 2 ** 19).floor() * 2 + 1) / 2 ** 20
        box = torch.stack([x1, y1, x1 + 7.0 / 128, y1 + 7.0 / 128], 1)
    elif kind == "whole":
        box = torch.tensor([[-1.0, -1.0, float(w), float(h)], [0.0, 0.0, w - 1.0, h - 1.0]], dtype=F64)
    elif kind == "cull":
        k = CULL_LIST + 6
        x1, y1 = u(k, -0.9, 1.6), u(k, -0.9, 1.6)
        box = torch.stack([x1, y1, x1 + u(k, 0.2, 1.2), y1 + u(k, 0.2, 1.2)], 1)
    else:
        raise KeyError(kind)
    b = (torch.arange(box.shape[0]) % n).to(F64)
    return torch.cat([b[:, None], box / scale], 1).to(F32)


@functools.lru_cache(maxsize=None)
def make_case(name):
    (n, c, h, w), out, scale, kind, grad_scale, seed = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    case = {"name": name, "input": torch.randn((n, c, h, w), generator=gen, dtype=F32), "output_size": out, "spatial_scale": f32(scale)}
    case["rois"] = _rois(gen, n, h, w, kind, case["spatial_scale"])
    case["grad"] = torch.randn((case["rois"].shape[0], c) + out, generator=gen, dtype=F32) * grad_scale
    return case


def degenerate_rois(n):
    """A normal RoI of image 0 followed by the RoIs that pool to zeros (a map of at least 6 x 7 cells, scale 1), and their names."""
    inf, nan = float("inf"), float("nan")
    rows = [("normal", [0.0, 1.2, 0.9, 5.1, 4.3]), ("zero width", [0.0, 2.0, 1.0, 2.0, 4.0]), ("inverted", [0.0, 4.0, 3.0, 1.0, 1.0]),
            ("nan", [0.0, 1.0, nan, 4.0, 4.0]), ("+inf", [0.0, 1.0, 1.0, inf, 4.0]), ("1e30", [0.0, 1.0, 1.0, 1e30, 1e30]),
            ("1e30 start", [0.0, 1e30, 1.0, 4.0, 4.0]), ("batch -1", [-1.0, 1.2, 0.9, 5.1, 4.3]), ("batch N", [float(n), 1.2, 0.9, 5.1, 4.3]),
            ("batch nan", [nan, 1.2, 0.9, 5.1, 4.3]), ("-inf", [0.0, -inf, 1.0, 4.0, 4.0])]
    return torch.tensor([r for _, r in rows], dtype=F32), [name for name, _ in rows]


# ---- restatement A: separable, analytic gradients ------------------------------------------------------------------------------------------
def geometry(case, dtype, rois=None):
    r = (case["rois"] if rois is None else rois).to(dtype)
    n = case["input"].shape[0]
    oh, ow = case["output_size"]
    s = case["spatial_scale"]
    g = {"x1": r[:, 1] * s, "y1": r[:, 2] * s, "x2": r[:, 3] * s, "y2": r[:, 4] * s}
    g["bw"], g["bh"] = (g["x2"] - g["x1"]).clamp(min=0) / ow, (g["y2"] - g["y1"]).clamp(min=0) / oh
    g["area"] = g["bw"] * g["bh"]
    g["valid"] = (g["area"] > 0) & torch.isfinite(g["area"]) & (r[:, 0] > -1) & (r[:, 0] < n)
    g["image"] = torch.where(g["valid"], r[:, 0], torch.zeros_like(r[:, 0])).to(torch.int64)
    # a RoI that is not pooled gets a harmless box: its results are zeroed at the end
    for key, fill in (("x1", 0.0), ("y1", 0.0), ("bw", 1.0), ("bh", 1.0), ("area", 1.0)):
        g[key] = torch.where(g["valid"], g[key], torch.full_like(g[key], fill))
    for axis, start, size, n_out in (("x", g["x1"], g["bw"], ow), ("y", g["y1"], g["bh"], oh)):
        p = torch.arange(n_out, dtype=dtype)[None, :]
        g[axis + "s"] = start[:, None] + p * size[:, None]
        g[axis + "e"] = g[axis + "s"] + size[:, None]
    return g


def weights(s, e, cells):
    """[K, n_out, cells]: the integral of hat(x - i) over [s, e] on the two unit pieces either side of i."""
    c = torch.arange(cells, dtype=s.dtype)
    s, e = s[..., None], e[..., None]
    zero = torch.zeros((), dtype=s.dtype)
    p, q = torch.maximum(s, c - 1), torch.minimum(e, c)
    rising = torch.where(q > p, (q - p) * (((p + q) * 0.5 - c) + 1), zero)
    p, q = torch.maximum(s, c), torch.minimum(e, c + 1)
    falling = torch.where(q > p, (q - p) * (1 - ((p + q) * 0.5 - c)), zero)
    return rising + falling


def hat(t, cells):
    c = torch.arange(cells, dtype=t.dtype)
    return (1 - (t[..., None] - c).abs()).clamp(min=0)


def _zero_invalid(t, g):
    return torch.where(g["valid"].reshape((-1,) + (1,) * (t.dim() - 1)), t, torch.zeros((), dtype=t.dtype))


def forward_ref(case, dtype, rois=None):
    """[K, C, oh, ow] in dtype."""
    g = geometry(case, dtype, rois)
    x = case["input"].to(dtype)[g["image"]]                                               # [K, C, H, W]
    h, w = x.shape[2:]
    wy, wx = weights(g["ys"], g["ye"], h), weights(g["xs"], g["xe"], w)
    cols = torch.einsum("kph,kchw->kcpw", wy, x)
    out = torch.einsum("kcpw,kqw->kcpq", cols, wx) / g["area"][:, None, None, None]
    return _zero_invalid(out, g)


def grads_ref(case, dtype, grad=None):
    """(d_input [N, C, H, W], d_rois [K, 5]) by the formulas of include/frcnn_hip.h."""
    g = geometry(case, dtype)
    xin = case["input"].to(dtype)
    x = xin[g["image"]]
    h, w = x.shape[2:]
    oh, ow = case["output_size"]
    grad = _zero_invalid((case["grad"] if grad is None else grad).to(dtype), g)
    area = g["area"][:, None, None]
    wy, wx = weights(g["ys"], g["ye"], h), weights(g["xs"], g["xe"], w)
    per_roi = torch.einsum("kcpq,kphqw->kchw", grad, (wy[:, :, :, None, None] * wx[:, None, None, :, :]) / area[:, :, :, None, None])
    dx = torch.zeros_like(xin).index_add_(0, g["image"], per_roi)
    cols = torch.einsum("kph,kchw->kcpw", wy, x)                                          # integrated over y
    rows = torch.einsum("kqw,kchw->kcqh", wx, x)                                          # integrated over x
    g_out = (grad * torch.einsum("kcpw,kqw->kcpq", cols, wx)).sum(1) / area              # sum over c of grad out  [K, oh, ow]
    g_xs = (grad * torch.einsum("kcpw,kqw->kcpq", cols, hat(g["xs"], w))).sum(1)
    g_xe = (grad * torch.einsum("kcpw,kqw->kcpq", cols, hat(g["xe"], w))).sum(1)
    g_ys = (grad * torch.einsum("kcqh,kph->kcpq", rows, hat(g["ys"], h))).sum(1)
    g_ye = (grad * torch.einsum("kcqh,kph->kcpq", rows, hat(g["ye"], h))).sum(1)
    bw, bh = g["bw"][:, None, None], g["bh"][:, None, None]
    d_xs, d_xe = (g_out * bh - g_xs) / area, (g_xe - g_out * bh) / area
    d_ys, d_ye = (g_out * bw - g_ys) / area, (g_ye - g_out * bw) / area
    ax = (torch.arange(ow, dtype=dtype) / ow)[None, None, :]
    bx = (torch.arange(1, ow + 1, dtype=dtype) / ow)[None, None, :]
    ay = (torch.arange(oh, dtype=dtype) / oh)[None, :, None]
    by = (torch.arange(1, oh + 1, dtype=dtype) / oh)[None, :, None]
    cols5 = [torch.zeros_like(g["area"]), (d_xs * (1 - ax) + d_xe * (1 - bx)).sum((1, 2)), (d_ys * (1 - ay) + d_ye * (1 - by)).sum((1, 2)),
             (d_xs * ax + d_xe * bx).sum((1, 2)), (d_ys * ay + d_ye * by).sum((1, 2))]
    drois = _zero_invalid(torch.stack(cols5, 1) * case["spatial_scale"], g)
    return dx, drois


# ---- restatement B: direct, float64 ---------------------------------------------------------------------------------------------------------
def _antiderivative(t):
    """The integral of hat from -inf to t."""
    return torch.where(t <= -1, torch.zeros_like(t), torch.where(t <= 0, (t + 1) ** 2 / 2, torch.where(t < 1, 1 - (1 - t) ** 2 / 2,
                                                                                                         torch.ones_like(t))))


def _direct_bins(case, rois):
    r = (case["rois"] if rois is None else rois).to(F64)
    n = case["input"].shape[0]
    oh, ow = case["output_size"]
    box = r[:, 1:] * case["spatial_scale"]
    valid = (box[:, 2] > box[:, 0]) & (box[:, 3] > box[:, 1]) & torch.isfinite(box).all(1) & (r[:, 0] > -1) & (r[:, 0] < n)
    box = torch.where(valid[:, None], box, torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=F64))
    image = torch.where(valid, r[:, 0], torch.zeros_like(r[:, 0])).to(torch.int64)
    px, py = torch.arange(ow + 1, dtype=F64)[None, :] / ow, torch.arange(oh + 1, dtype=F64)[None, :] / oh
    ex = box[:, 0:1] + px * (box[:, 2:3] - box[:, 0:1])                                   # [K, ow + 1] bin edges
    ey = box[:, 1:2] + py * (box[:, 3:4] - box[:, 1:2])
    area = ((box[:, 2] - box[:, 0]) / ow) * ((box[:, 3] - box[:, 1]) / oh)
    return valid, image, ex, ey, area


def _cell_weight(ex, ey, area, j, i):
    """[K, oh, ow]: the weight of cell (j, i) in every bin, divided by the bin's area."""
    wx = _antiderivative(ex[:, 1:] - i) - _antiderivative(ex[:, :-1] - i)
    wy = _antiderivative(ey[:, 1:] - j) - _antiderivative(ey[:, :-1] - j)
    return wy[:, :, None] * wx[:, None, :] / area[:, None, None]


def forward_direct(case, rois=None):
    valid, image, ex, ey, area = _direct_bins(case, rois)
    x = case["input"].to(F64)
    out = torch.zeros((image.shape[0], x.shape[1]) + tuple(case["output_size"]), dtype=F64)
    for j in range(x.shape[2]):
        for i in range(x.shape[3]):
            out += _cell_weight(ex, ey, area, j, i)[:, None] * x[image, :, j, i][:, :, None, None]
    return torch.where(valid[:, None, None, None], out, torch.zeros((), dtype=F64))


def input_grad_direct(case):
    valid, image, ex, ey, area = _direct_bins(case, None)
    grad = torch.where(valid[:, None, None, None], case["grad"].to(F64), torch.zeros((), dtype=F64))
    dx = torch.zeros(case["input"].shape, dtype=F64)
    for j in range(dx.shape[2]):
        for i in range(dx.shape[3]):
            dx[:, :, j, i].index_add_(0, image, (grad * _cell_weight(ex, ey, area, j, i)[:, None]).sum((2, 3)))
    return dx


def roi_grad_direct(case):
    """d_rois [K, 5] by central differences of sum(grad * forward_direct) in each box coordinate (the RoIs are independent)."""
    grad = case["grad"].to(F64)
    rois = case["rois"].to(F64)
    cols = [torch.zeros((rois.shape[0],), dtype=F64)]
    for c in range(1, 5):
        plus, minus = rois.clone(), rois.clone()
        plus[:, c] += STEP
        minus[:, c] -= STEP
        cols.append(((forward_direct(case, plus) - forward_direct(case, minus)) * grad).sum((1, 2, 3)) / (2 * STEP))
    return torch.stack(cols, 1)


def surface(case, b, x, y):
    """f(x, y) of image b in float64: [C, ...] for coordinate tensors of any shape."""
    plane = case["input"][b].to(F64)
    h, w = plane.shape[1:]
    wy = (1 - (y[..., None] - torch.arange(h, dtype=F64)).abs()).clamp(min=0)
    wx = (1 - (x[..., None] - torch.arange(w, dtype=F64)).abs()).clamp(min=0)
    return torch.einsum("...h,...w,chw->c...", wy, wx, plane)


# ---- the conditions of the comparisons ------------------------------------------------------------------------------------------------------
def rel_err(a, truth):
    return float((a.double() - truth.double()).abs().max() / truth.double().abs().max())


def check_conditions(case, truth):
    """Every quantity of the float64 truth (output, d_input, d_rois) is large enough for a relative error: max|truth| > 0.1; and the
    float32 and float64 geometries pool the same RoIs."""
    for label, t in zip(("output", "d_input", "d_rois"), truth):
        assert bool(torch.isfinite(t).all()), (case["name"], label)
        assert float(t.abs().max()) > 0.1, (case["name"], label, float(t.abs().max()))
    assert torch.equal(geometry(case, F32)["valid"], geometry(case, F64)["valid"]), case["name"]
    assert bool(geometry(case, F64)["valid"].any()), case["name"]
