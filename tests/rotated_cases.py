"""Cases and torch restatements of the rotated-box operators (fasterrcnn_amd.ops.box_iou_rotated, nms_rotated, roi_align_rotated), shared
by tests/test_ops_rot_cpu.py and tests/test_ops_rot_gpu.py.  The definitions are the ones include/frcnn_hip.h states (mmcv's
box_iou_rotated, nms_rotated and roi_align_rotated restated, unpinned).

The restatements run on the CPU in float64 (the truth) or float32 (whose error against the truth measures the bound of the GPU tests).

IoU: the centre difference first, box 1's corners in box 2's frame, Sutherland-Hodgman against box 2's four half-planes, the area as a
fan of triangles -- vectorised over pairs with a fixed list of 8 vertices and a count per pair.  tests/test_ops_rot_cpu.py checks it
against independent facts (symmetry, the axis-aligned formula, closed-form configurations).

NMS: the greedy pass over the float64 IoU matrix.  The generator resamples every box that has a pair whose float64 IoU lies within
MARGIN = 1e-4 of the case's threshold -- 30 times the worst float32 IoU error measured for this method (3.4e-6, near-identical pairs) --
so that a float32 IoU decides every pair as the truth does and the kept set is exact.

roi_align_rotated: the forward vectorised over (RoI, ph, pw, iy, ix, channel), d_input written out explicitly (each sample sends
grad / count times its four bilinear weights), not by autograd.  The value jumps where a sample coordinate crosses -1 or the map size:
near_seam(case) marks, in float64, every (RoI, bin) with a sample coordinate within DELTA = 2**-10 of -1 or of the size; marked bins get
a zero upstream gradient and are left out of comparisons.  check_conditions asserts per case that at most 5 % of the bins are marked,
that the float32 and float64 sampling grids (ceil) are equal, and that the float32 coordinates are within DELTA / 4 of the float64 ones,
so that an unmarked sample is on the same side of both seams in both."""
import functools
import math

import torch

F32, F64 = torch.float32, torch.float64
DELTA = 2.0 ** -10
MARGIN = 1e-4
MIN_AREA = 1e-14
CULL_LIST = 1024                                   # ops.ROI_ALIGN_ROTATED_CULL_LIST (asserted by the CPU test)
ANGLES = (0.0, math.pi / 4, -math.pi / 4, math.pi / 2, math.pi, 2 * math.pi + 0.3, -7.0)


def f32(v):
    """A Python float rounded to float32, as the kernels receive thresholds and scales."""
    return float(torch.tensor(v, dtype=F32))


def rel_err(a, truth):
    return float((a.double() - truth.double()).abs().max() / truth.double().abs().max())


# ---- IoU ----------------------------------------------------------------------------------------------------------------------------
def box_ok(b):
    """The zero rule's complement: finite components, w >= 0, h >= 0, w h >= 1e-14."""
    return torch.isfinite(b).all(1) & (b[:, 2] >= 0) & (b[:, 3] >= 0) & (b[:, 2] * b[:, 3] >= MIN_AREA)


def _clip(v, n, axis, sign, bound):
    """One Sutherland-Hodgman pass over polygons v [P, 8, 2] with n [P] vertices: keeps sign * coordinate[axis] <= bound [P]."""
    rows = torch.arange(v.shape[0])
    out, m = torch.zeros_like(v), torch.zeros_like(n)
    prev = v[rows, (n - 1).clamp(min=0)]
    for i in range(8):
        q = v[:, i]
        act = i < n
        pd, qd = sign * prev[:, axis], sign * q[:, axis]
        pin, qin = pd <= bound, qd <= bound
        cross = act & (pin != qin) & (m < 8)
        t = (bound - pd) / (qd - pd)
        other = prev[:, 1 - axis] + t * (q[:, 1 - axis] - prev[:, 1 - axis])
        pt = torch.stack([sign * bound, other] if axis == 0 else [other, sign * bound], 1)
        idx = cross.nonzero()[:, 0]
        out[idx, m[idx]] = pt[idx]
        m = m + cross
        keep = act & qin & (m < 8)
        idx = keep.nonzero()[:, 0]
        out[idx, m[idx]] = q[idx]
        m = m + keep
        prev = torch.where(act[:, None], q, prev)
    return out, m


def iou_pairs(boxes1, boxes2, mode="iou", dtype=F64):
    """[P]: the IoU (mode "iof": inter / area 1) of boxes1[p] and boxes2[p], (cx, cy, w, h, angle), clockwise convention, in dtype."""
    a, b = boxes1.to(dtype), boxes2.to(dtype)
    valid = box_ok(a) & box_ok(b)
    unit = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0], dtype=dtype)
    a, b = torch.where(valid[:, None], a, unit), torch.where(valid[:, None], b, unit)
    ca, sa, cb, sb = torch.cos(a[:, 4]), torch.sin(a[:, 4]), torch.cos(b[:, 4]), torch.sin(b[:, 4])
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    ox, oy = dx * cb + dy * sb, dy * cb - dx * sb
    cd, sd = ca * cb + sa * sb, sa * cb - ca * sb
    one = torch.ones((), dtype=dtype)
    cd = torch.where(sd == 0, torch.where(cd < 0, -one, one), cd)
    sd = torch.where(cd == 0, torch.where(sd < 0, -one, one), sd)
    hw, hh = 0.5 * a[:, 2], 0.5 * a[:, 3]
    ux, uy, vx, vy = hw * cd, hw * sd, -hh * sd, hh * cd
    v = torch.zeros((a.shape[0], 8, 2), dtype=dtype)
    v[:, 0, 0], v[:, 0, 1] = (ox + ux) + vx, (oy + uy) + vy
    v[:, 1, 0], v[:, 1, 1] = (ox - ux) + vx, (oy - uy) + vy
    v[:, 2, 0], v[:, 2, 1] = (ox - ux) - vx, (oy - uy) - vy
    v[:, 3, 0], v[:, 3, 1] = (ox + ux) - vx, (oy + uy) - vy
    n = torch.full((a.shape[0],), 4, dtype=torch.int64)
    bw, bh = 0.5 * b[:, 2], 0.5 * b[:, 3]
    for axis, sign, bound in ((0, 1.0, bw), (1, 1.0, bh), (0, -1.0, bw), (1, -1.0, bh)):
        v, n = _clip(v, n, axis, sign, bound)
    total = torch.zeros((a.shape[0],), dtype=dtype)
    e = v[:, 1] - v[:, 0]
    for i in range(2, 8):
        f = v[:, i] - v[:, 0]
        act = (i < n) & (n >= 3)
        total = total + torch.where(act, e[:, 0] * f[:, 1] - f[:, 0] * e[:, 1], torch.zeros((), dtype=dtype))
        e = torch.where(act[:, None], f, e)
    inter = 0.5 * total.abs()
    area_a, area_b = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
    iou = inter / area_a if mode == "iof" else inter / ((area_a + area_b) - inter)
    return torch.where(valid, iou, torch.zeros((), dtype=dtype))


def iou_matrix(boxes1, boxes2, mode="iou", dtype=F64):
    n, m = boxes1.shape[0], boxes2.shape[0]
    return iou_pairs(boxes1.repeat_interleave(m, 0), boxes2.repeat(n, 1), mode, dtype).view(n, m)


def corners_to_rotated(xyxy, angle=0.0):
    """(x1, y1, x2, y2) as (cx, cy, w, h, angle)."""
    x1, y1, x2, y2 = xyxy.unbind(1)
    return torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, torch.full_like(x1, angle)], 1)


def rotated_to_corners(b):
    """The corner form (x1, y1, x2, y2) of boxes at angle 0."""
    return torch.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], 1)


def random_boxes(gen, n, extent=60.0, lo=8.0, hi=30.0, centre=0.0):
    """n overlapping boxes: centres in [centre, centre + extent]^2, sides in [lo, hi], the angles of ANGLES first, then uniform in
    [-pi, pi]; float32."""
    u = lambda a, b: torch.rand((n,), generator=gen, dtype=F64) * (b - a) + a     # noqa: E731
    ang = u(-math.pi, math.pi)
    for i, v in enumerate(ANGLES[:n]):
        ang[i] = v
    return torch.stack([u(centre, centre + extent), u(centre, centre + extent), u(lo, hi), u(lo, hi), ang], 1).to(F32)


IOU_SIZES = ((1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (63, 130), (130, 65), (64, 1))
NAN, INF = float("nan"), float("inf")
# rows of the "special" case, each against all of them (the diagonal holds the identical pairs)
SPECIAL = (
    (20.0, 20.0, 30.0, 10.0, 0.3), (20.0, 20.0, 30.0, 10.0, 0.3),           # identical
    (20.0, 20.0, 10.0, 30.0, 0.3 + math.pi / 2),                           # the same rectangle written the other way
    (50.0, 40.0, 1e-3, 500.0, 0.3), (50.0, 40.0, 1e-3, 500.0, 0.3), (50.0, 40.0, 1e-3, 500.0, 0.3 + math.pi / 2),   # slivers
    (60.0, 45.0, 500.0, 1e-3, -1.1),
    (20.0, 20.0, 1e-8, 1e-8, 0.0), (20.0, 20.0, 1e-7, 0.9e-7, 0.5), (20.0, 20.0, 0.0, 10.0, 0.0),                    # area < 1e-14
    (20.0, 20.0, -30.0, 10.0, 0.3), (20.0, 20.0, 30.0, -10.0, 0.3), (20.0, 20.0, -30.0, -10.0, 0.3),                # negative sides
    (NAN, 20.0, 30.0, 10.0, 0.3), (20.0, 20.0, NAN, 10.0, 0.3), (20.0, 20.0, 30.0, 10.0, NAN), (20.0, INF, 30.0, 10.0, 0.3),
    (20.0, 20.0, INF, 10.0, 0.3), (20.0, 20.0, 30.0, 10.0, -INF),
    (1e4 + 20.0, 20.0, 30.0, 10.0, 0.3), (20.0, 1e4 + 20.0, 30.0, 10.0, 0.3),                                       # centres 1e4 apart
    (4096.3, 4095.6, 8.0, 7.0, 0.4), (4098.1, 4097.2, 7.5, 8.5, -0.9), (4094.9, 4096.4, 8.2, 7.7, 2.0), (4096.3, 4095.6, 8.0, 7.0, 0.4),
)
ZERO_RULE_ROWS = tuple(range(7, 19))


@functools.lru_cache(maxsize=None)
def iou_case(name):
    """(boxes1 [N, 5], boxes2 [M, 5]) float32: "NxM" random overlapping boxes, "special" the rows of SPECIAL and 16 random ones against
    themselves, "near4096" 40 x 40 boxes of about 8 px centred near 4096."""
    if name == "special":
        b = torch.cat([torch.tensor(SPECIAL, dtype=F64).to(F32), random_boxes(torch.Generator().manual_seed(5), 16)], 0)
        return b, b.clone()
    if name == "near4096":
        gen = torch.Generator().manual_seed(6)
        return random_boxes(gen, 40, 12.0, 6.0, 10.0, 4090.0), random_boxes(gen, 40, 12.0, 6.0, 10.0, 4090.0)
    n, m = (int(v) for v in name.split("x"))
    gen = torch.Generator().manual_seed(100 * n + m)
    return random_boxes(gen, n), random_boxes(gen, m)


IOU_CASES = tuple("%dx%d" % s for s in IOU_SIZES) + ("special", "near4096")


# ---- NMS ----------------------------------------------------------------------------------------------------------------------------
def score_order(scores):
    """Stable descending, NaN scores last in input order (ops._score_order)."""
    s = scores.tolist()
    return sorted(range(len(s)), key=lambda i: (s[i] != s[i], 0.0 if s[i] != s[i] else -s[i], i))


def greedy(over, order, labels=None):
    """The greedy pass: over [n, n] bool (row i suppresses column j), visited in `order`; the kept indices in visiting order."""
    n = over.shape[0]
    gone = torch.zeros((n,), dtype=torch.bool)
    kept = []
    for i in order:
        if gone[i]:
            continue
        kept.append(i)
        gone |= over[i] if labels is None else over[i] & (labels == labels[i])
    return torch.tensor(kept, dtype=torch.int64)


def nms_ref(case):
    """keep by the greedy pass over the float64 IoU of the restatement."""
    iou = iou_matrix(case["boxes"], case["boxes"])
    return greedy(iou > case["thr"], score_order(case["scores"]), case["labels"])


def near_threshold(boxes, thr):
    """bool [n, n]: the pairs (i != j) whose float64 IoU, in either argument order, lies within MARGIN of thr."""
    iou = iou_matrix(boxes, boxes)
    near = ((iou - thr).abs() < MARGIN) | ((iou.t() - thr).abs() < MARGIN)
    return near & ~torch.eye(boxes.shape[0], dtype=torch.bool)


# name: n, threshold, labels, scores ("plain", "tied": eighths, "nan": every seventh NaN), angle0, seed
NMS_CASES = {
    "n1": (1, 0.5, False, "plain", False, 1),
    "n63": (63, 0.3, False, "plain", False, 2),
    "n64-labels": (64, 0.5, True, "tied", False, 3),
    "n65": (65, 0.1, False, "nan", False, 4),
    "n129-labels": (129, 0.3, True, "nan", False, 5),
    "n300": (300, 0.5, False, "tied", False, 6),
    "n300-labels": (300, 0.1, True, "plain", False, 7),
    "n65-angle0": (65, 0.5, False, "plain", True, 8),
    "n300-angle0-labels": (300, 0.3, True, "tied", True, 9),
}


@functools.lru_cache(maxsize=None)
def nms_case(name):
    n, thr, with_labels, score_kind, angle0, seed = NMS_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    thr = f32(thr)
    extent = 25.0 + 2.5 * math.sqrt(n)
    boxes = random_boxes(gen, n, extent)
    if angle0:
        boxes[:, 4] = 0.0
    for _ in range(50):
        bad = near_threshold(boxes, thr).any(1).nonzero()[:, 0]
        if bad.numel() == 0:
            break
        fresh = random_boxes(gen, n, extent)
        boxes[bad, :4] = fresh[bad, :4]
        if not angle0:
            boxes[bad, 4] = fresh[bad, 4]
    scores = torch.rand((n,), generator=gen, dtype=F32)
    if score_kind == "tied":
        scores = torch.round(scores * 8) / 8
    if score_kind == "nan":
        scores[::7] = NAN
    labels = torch.randint(0, 3, (n,), generator=gen) if with_labels else None
    return {"name": name, "boxes": boxes, "scores": scores, "labels": labels, "thr": thr}


# ---- roi_align_rotated ----------------------------------------------------------------------------------------------------------------
# name: (N, C, H, W), output_size, sampling_ratio, aligned, clockwise, spatial_scale, K, RoI kind, seed
# RoI kinds: "mixed" (RoIs of every image interleaved, centres from inside the map to beyond its border; when K >= 16 the angles of
# ANGLES at rows 0..6, a RoI larger than the map at row 8, one wholly outside at row 10, the batch indices -1, N and NaN at rows 9, 11,
# 13, a zero-width RoI at row 14 and a negative-height one at row 15), "cover" (every RoI lies around the centre of a map of one tile, with all its samples on the map: all are listed by that tile).
POOL_CASES = {
    "13x17-c6-7x7": ((2, 6, 13, 17), (7, 7), 2, True, False, 1 / 16, 37, "mixed", 21),
    "13x17-c8-2x3-adaptive": ((2, 8, 13, 17), (2, 3), 0, False, True, 1.0, 37, "mixed", 22),
    "5x4-c6-adaptive": ((2, 6, 5, 4), (2, 3), 0, True, True, 0.25, 37, "mixed", 23),
    "5x4-c8-1x1-unaligned": ((2, 8, 5, 4), (1, 1), 3, False, False, 1.0, 37, "mixed", 24),
    "1x1-c4-1x1": ((1, 4, 1, 1), (1, 1), 2, True, False, 1.0, 5, "mixed", 25),
    "1x1-c4-7x7-adaptive": ((1, 4, 1, 1), (7, 7), 0, True, True, 1.0, 37, "mixed", 26),
    "2x2-cull": ((1, 4, 2, 2), (2, 2), 1, True, False, 1.0, CULL_LIST + 1, "cover", 27),
    "k0": ((1, 4, 5, 4), (2, 3), 2, True, False, 1.0, 0, "mixed", 28),
}
INVALID_ROWS = (9, 11, 13)


def _pool_rois(gen, n, h, w, k, kind, scale):
    u = lambda lo, hi: torch.rand((k,), generator=gen, dtype=F64) * (hi - lo) + lo     # noqa: E731
    ang = u(-math.pi, math.pi)
    if kind == "cover":
        cx, cy, rw, rh = u(0.4 * w, 0.6 * w), u(0.4 * h, 0.6 * h), u(0.5 * w, 0.8 * w), u(0.5 * h, 0.8 * h)
    else:
        cx, cy = u(-0.2 * w, 1.2 * w), u(-0.2 * h, 1.2 * h)
        rw, rh = u(0.5, 0.8 * w + 0.5), u(0.5, 0.8 * h + 0.5)
    b = (torch.arange(k) % n).to(F64)
    if kind == "mixed" and k >= 16:
        for i, v in enumerate(ANGLES):
            ang[i] = v
        rw[8], rh[8] = 2.0 * w, 2.0 * h                                     # larger than the map
        cx[10], cy[10] = 3.0 * w + 5.0, -2.0 * h - 5.0                      # wholly outside
        b[9], b[11], b[13] = -1.0, float(n), NAN
        rw[14] = 0.0
        rh[15] = -2.0
    return torch.stack([b, cx / scale, cy / scale, rw / scale, rh / scale, ang], 1).to(F32)


@functools.lru_cache(maxsize=None)
def pool_case(name):
    (n, c, h, w), out, sr, aligned, clockwise, scale, k, kind, seed = POOL_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    case = {"name": name, "input": torch.randn((n, c, h, w), generator=gen, dtype=F32), "output_size": out, "sampling_ratio": sr,
            "aligned": aligned, "clockwise": clockwise, "spatial_scale": f32(scale)}
    case["rois"] = _pool_rois(gen, n, h, w, k, kind, case["spatial_scale"])
    grad = torch.randn((k, c) + out, generator=gen, dtype=F32)
    case["seam"] = near_seam(case)
    case["grad"] = torch.where(case["seam"][:, None], torch.zeros(()), grad)              # marked bins send nothing
    return case


def geometry(case, dtype):
    """The sampling plan in dtype: per RoI validity, image, grids and count; per sample the image coordinates y, x
    [K, oh, ow, Gh, Gw] and which samples exist (iy < grid_h, ix < grid_w)."""
    r = case["rois"].to(dtype)
    n = case["input"].shape[0]
    oh, ow = case["output_size"]
    k = r.shape[0]
    scale, sr = case["spatial_scale"], case["sampling_ratio"]
    off = 0.5 if case["aligned"] else 0.0
    valid = (r[:, 0] > -1) & (r[:, 0] < n)                                                # NaN fails
    g = {"valid": valid, "image": torch.where(valid, r[:, 0], torch.zeros_like(r[:, 0])).to(torch.int64)}
    cx, cy = r[:, 1] * scale - off, r[:, 2] * scale - off
    rw, rh = r[:, 3] * scale, r[:, 4] * scale
    if not case["aligned"]:
        rw, rh = torch.where(rw < 1, torch.ones_like(rw), rw), torch.where(rh < 1, torch.ones_like(rh), rh)
    t = -r[:, 5] if case["clockwise"] else r[:, 5]
    cos, sin = torch.cos(t), torch.sin(t)
    bin_h, bin_w = rh / oh, rw / ow
    if sr > 0:
        g["grid_h"] = g["grid_w"] = torch.full((k,), sr, dtype=torch.int64)
    else:
        g["grid_h"], g["grid_w"] = torch.ceil(rh / oh).clamp(min=0).to(torch.int64), torch.ceil(rw / ow).clamp(min=0).to(torch.int64)
    g["count"] = (g["grid_h"] * g["grid_w"]).clamp(min=1).to(dtype)
    local = {}
    for axis, start, binsz, grid, n_out in (("y", -rh / 2, bin_h, g["grid_h"], oh), ("x", -rw / 2, bin_w, g["grid_w"], ow)):
        top = max(int(grid.max()), 1) if k else 1
        p = torch.arange(n_out)[None, :, None].to(dtype)
        i = torch.arange(top)[None, None, :]
        binsz, gr = binsz[:, None, None], grid[:, None, None]
        local[axis] = (start[:, None, None] + p * binsz) + ((i.to(dtype) + 0.5) * binsz) / gr.clamp(min=1).to(dtype)   # [K, out, G]
        local["exists_" + axis] = (i < gr).expand(k, n_out, top)
    yy, xx = local["y"][:, :, None, :, None], local["x"][:, None, :, None, :]
    c5, s5 = cos[:, None, None, None, None], sin[:, None, None, None, None]
    g["x"] = (yy * s5 + xx * c5) + cx[:, None, None, None, None]
    g["y"] = (yy * c5 - xx * s5) + cy[:, None, None, None, None]
    g["exists"] = local["exists_y"][:, :, None, :, None] & local["exists_x"][:, None, :, None, :] & valid[:, None, None, None, None]
    return g


def _axis(v, exists, size, dtype):
    """axis_weights over a tensor of coordinates: (accepted, low, high, weight of low, weight of high); NaN fails the range test."""
    ok = exists & (v >= -1) & (v <= size)
    c = torch.where(ok, v, torch.zeros_like(v)).clamp(min=0)
    low = c.detach().floor().to(torch.int64)
    top = low >= size - 1
    low = torch.where(top, torch.full_like(low, size - 1), low)
    high = torch.where(top, low, low + 1)
    c = torch.where(top, low.to(dtype), c)
    wh = c - low.to(dtype)
    return ok, low, high, 1 - wh, wh


def _samples(case, dtype, input=None):
    g = geometry(case, dtype)
    x = (case["input"] if input is None else input).to(dtype).permute(0, 2, 3, 1)          # [N, H, W, C]
    h, w = x.shape[1:3]
    yok, yl, yh, hy, ly = _axis(g["y"], g["exists"], h, dtype)
    xok, xl, xh, hx, lx = _axis(g["x"], g["exists"], w, dtype)
    b = g["image"][:, None, None, None, None]
    s = {"g": g, "x": x, "mask": (yok & xok)[..., None], "b": b, "yl": yl, "yh": yh, "xl": xl, "xh": xh}
    s["w"] = [(hy * hx)[..., None], (hy * lx)[..., None], (ly * hx)[..., None], (ly * lx)[..., None]]
    s["v"] = [x[b, yl, xl], x[b, yl, xh], x[b, yh, xl], x[b, yh, xh]]                       # [K, oh, ow, Gh, Gw, C]
    return s


def forward_ref(case, dtype, input=None):
    """[K, C, oh, ow] in dtype; differentiable in `input` when it is given and requires grad."""
    s = _samples(case, dtype, input)
    (v1, v2, v3, v4), (w1, w2, w3, w4) = s["v"], s["w"]
    val = ((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4
    out = torch.where(s["mask"], val, torch.zeros_like(val)).sum((3, 4)) / s["g"]["count"][:, None, None, None]
    return out.permute(0, 3, 1, 2)


def grad_ref(case, dtype, grad=None):
    """d_input [N, C, H, W], written out: every accepted sample sends grad / count times its four weights to its four corners."""
    s = _samples(case, dtype)
    grad = (case["grad"] if grad is None else grad).to(dtype).permute(0, 2, 3, 1)
    gm = (grad / s["g"]["count"][:, None, None, None])[:, :, :, None, None, :]
    gm = torch.where(s["mask"], gm, torch.zeros_like(gm))                                 # [K, oh, ow, Gh, Gw, C]
    dx = torch.zeros_like(s["x"])
    for (iy, ix), wt in zip(((s["yl"], s["xl"]), (s["yl"], s["xh"]), (s["yh"], s["xl"]), (s["yh"], s["xh"])), s["w"]):
        dx.index_put_(tuple(torch.broadcast_tensors(s["b"], iy, ix)), gm * wt, accumulate=True)
    return dx.permute(0, 3, 1, 2)


def as_corner_case(case):
    """The case at angle 0 and aligned as a deform_roi_cases-style RoIAlign case: rows (b, x1, y1, x2, y2), float64 arithmetic."""
    r = case["rois"].double()
    boxes = rotated_to_corners(r[:, 1:])
    return dict(case, rois=torch.cat([r[:, :1], boxes], 1))


def near_seam(case):
    """bool [K, oh, ow]: the bins with a sample coordinate (float64) within DELTA of -1 or of the map size."""
    g = geometry(case, F64)
    h, w = case["input"].shape[2:]
    mark = torch.zeros_like(g["exists"])
    for v, size in ((g["y"], h), (g["x"], w)):
        mark |= g["exists"] & (((v + 1).abs() < DELTA) | ((v - size).abs() < DELTA))
    return mark.any(-1).any(-1)


def check_conditions(case):
    """The conditions of the module docstring; returns the marked fraction."""
    seam = case["seam"]
    fraction = float(seam.double().mean()) if seam.numel() else 0.0
    assert fraction <= 0.05, (case["name"], fraction)
    g32, g64 = geometry(case, F32), geometry(case, F64)
    assert torch.equal(g32["grid_h"], g64["grid_h"]) and torch.equal(g32["grid_w"], g64["grid_w"]), case["name"]
    for axis in ("y", "x"):
        a, b = g32[axis].double(), g64[axis]
        if g64["exists"].any():
            assert float((a - b)[g64["exists"]].abs().max()) < DELTA / 4, (case["name"], axis)
    return fraction


def masked(t, case):
    """t [K, C, oh, ow] with the near-seam bins zeroed: what the comparisons look at."""
    return torch.where(case["seam"][:, None].to(t.device), torch.zeros((), dtype=t.dtype, device=t.device), t)
