"""Cases and two restatements for fasterrcnn_amd.ops.box_iou_quadri / nms_quadri / points_in_polygons (tests/test_ops_quadri_cpu.py and
tests/test_ops_quadri_gpu.py).  The hull, clip and area helpers are tests/convex_cases.py's: the operators share one notion of polygon.

  truth      float64, one pair at a time with Python branches: Andrew's monotone-chain hull, Sutherland-Hodgman, the shoelace sum; for a
             point, the sign of the cross product with every hull edge on raw coordinates.
  analytic   the kernels' arithmetic (csrc/ops_quadri.hip on csrc/ops_convex.h) on scalars of ONE dtype, in the kernels' order of
             operations: the gift-wrapping hull on coordinates relative to the quadrilateral's smallest point, the bounding-box test, the
             clip on coordinates relative to hull 2's smallest vertex, the fan areas; analytic_pair takes one pair, analytic_pairs is the
             same arithmetic element by element over numpy arrays of that dtype (the CPU test asserts that the two agree bit for bit).
             In float64 it is checked against truth; in float32 its error against truth is err_ref.

Random cases follow one recipe per pair (numpy default_rng(seed)): convex_cases._box's rectangle (centre uniform in [0, 100]^2, w, h =
exp(U(ln 4, ln 40)), angle uniform in [-pi/2, pi/2]) with each corner moved by U(-0.15, 0.15)^2 * (w, h); the partner is the same
quadrilateral shifted by U(-0.3, 0.3)^2 * (w, h), turned by U(-0.3, 0.3) and scaled by exp(U(-0.3, 0.3)); every eighth pair is moved by
3 max(w, h) along x (I = 0); all rounded to float32.

NMS: the greedy pass over the float64 IoU matrix, thresholds rounded to float32 and compared with > as tests/rotated_cases.py has it.
Quadrilaterals come in clusters of eight partners of one base quadrilateral.  The generator resamples every quadrilateral that has a
pair whose float64 IoU, in either argument order, lies within MARGIN = 1e-4 of the case's threshold (it asks for twice that of the
float64 restatement; check_conditions then asserts MARGIN on the truth), so that a float32 IoU decides every pair as the truth does and
the kept set is exact.  MARGIN is 30 times (the factor of rotated_cases.py) the worst |float32 restatement -
truth| measured on the CPU over every NMS case below, 3.6e-7 (check_conditions prints it and asserts the rounding), rounded up to a power of
ten.

points_in_polygons: point i is drawn around polygon i mod M as centre + R(angle) (U(-0.8, 0.8)^2 * (w, h)), so about 0.625^2 = 39 % of
the own pairs are inside; a point whose float64 distance to the line of any hull edge of any polygon of the case is below DELTA = 2**-10
(rotated_cases.DELTA) is resampled, so that the float32 products decide every pair as the truth does."""
import functools
import math

import numpy as np
import torch

from tests import convex_cases as C
from tests import rotated_cases as R

F32, F64 = torch.float32, torch.float64
MIN_AREA = C.MIN_AREA
DELTA = R.DELTA
MARGIN = 1e-4
TILE_ROWS = 32                       # ops.QUADRI_IOU_TILE_ROWS (asserted by the CPU test)
POINT_ROWS = 256                     # ops.POINTS_IN_POLYGONS_TILE_ROWS (asserted by the CPU test)

ALIGNED = {"1": (1, 31), "63": (63, 32), "64": (64, 33), "65": (65, 34), "130": (130, 35), "1000": (1000, 36), "near4096": (40, 37)}
ALIGNED_CASES = tuple(ALIGNED)
MATRIX = {"1x1": (1, 1, 41), "63x65": (63, 65, 42), "64x64": (64, 64, 43), "65x63": (65, 63, 44), "130x7": (130, 7, 45),
          "7x130": (7, 130, 46), "%dx9" % (TILE_ROWS - 1): (TILE_ROWS - 1, 9, 47), "%dx9" % (TILE_ROWS + 1): (TILE_ROWS + 1, 9, 48)}
MATRIX_CASES = tuple(MATRIX)
POINT_SEAMS = {"%dx5" % (POINT_ROWS - 1): (POINT_ROWS - 1, 5, 49), "%dx5" % (POINT_ROWS + 1): (POINT_ROWS + 1, 5, 50)}
POINT_CASES = MATRIX_CASES + tuple(POINT_SEAMS)
MODES = ("iou", "iof")


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _local(rng, wh):
    """The corners of the rectangle wh about the origin, each moved by U(-0.15, 0.15)^2 * wh: [4, 2], counter-clockwise."""
    return (np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]]) + rng.uniform(-0.15, 0.15, (4, 2))) * wh


def _place(local, c, a):
    return local @ C._rot(a).T + c


def _partner(rng, local, c, wh, a):
    shift, turn, scale = rng.uniform(-0.3, 0.3, 2) * wh, rng.uniform(-0.3, 0.3), math.exp(rng.uniform(-0.3, 0.3))
    return _place(local * scale, c + shift, a + turn)


def _f32(rows):
    return torch.from_numpy(np.stack(rows).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(name):
    """Aligned pairs: (quads1 [n, 8], quads2 [n, 8]) float32."""
    n, seed = ALIGNED[name]
    rng = np.random.default_rng(seed)
    first, second = [], []
    for i in range(n):
        c, wh, a = C._box(rng, 4096 + rng.uniform(-50, 50, 2) if name == "near4096" else None)
        local = _local(rng, wh)
        p, q = _partner(rng, local, c, wh, a), _place(local, c, a)
        if i % 8 == 7:
            p = p + np.array([3 * wh.max(), 0.0])
        first.append(p.reshape(8)); second.append(q.reshape(8))
    return _f32(first), _f32(second)


def _columns(rng, m):
    boxes = [C._box(rng) for _ in range(m)]
    return [(c, wh, a, _local(rng, wh)) for c, wh, a in boxes]


@functools.lru_cache(maxsize=None)
def matrix_case(name):
    """(quads1 [n, 8], quads2 [m, 8]) float32: row i is a partner of column i mod m, every eighth one moved away."""
    n, m, seed = MATRIX[name]
    rng = np.random.default_rng(seed)
    cols = _columns(rng, m)
    rows = []
    for i in range(n):
        c, wh, a, local = cols[i % m]
        p = _partner(rng, local, c, wh, a)
        if i % 8 == 7:
            p = p + np.array([3 * wh.max(), 0.0])
        rows.append(p.reshape(8))
    return _f32(rows), _f32([_place(local, c, a).reshape(8) for c, wh, a, local in cols])


def rel_err(a, truth):
    return C.rel_err(a, truth)


# ---- truth: float64, Python floats ------------------------------------------------------------------------------------------------------
def truth_hull(quad):
    """quad: 4 (x, y) Python floats -> the hull's vertices, or None for a dead row."""
    if not all(math.isfinite(c) for p in quad for c in p):
        return None
    h = [quad[i] for i in C.hull_indices(quad)]
    return h if C.shoelace(h) >= MIN_AREA else None


def truth_pair(a, b):
    """(iou, iof) of two quadrilaterals, each 4 (x, y) Python floats."""
    P, Q = truth_hull(a), truth_hull(b)
    if P is None or Q is None:
        return 0.0, 0.0
    a1, a2 = C.shoelace(P), C.shoelace(Q)
    inter = max(C.shoelace(C.clip_polygon(P, Q)), 0.0)
    union = a1 + a2 - inter
    return (inter / union if union >= MIN_AREA else 0.0), inter / a1


def _rows(t):
    return t.double().view(-1, 4, 2).tolist()


@functools.lru_cache(maxsize=None)
def truth(name):
    """The float64 truth of an aligned case: {"iou": [n], "iof": [n]}."""
    v = [truth_pair(a, b) for a, b in zip(*map(_rows, case(name)))]
    return {"iou": torch.tensor([p[0] for p in v], dtype=F64), "iof": torch.tensor([p[1] for p in v], dtype=F64)}


def truth_matrix(q1, q2):
    a, b = _rows(q1), _rows(q2)
    v = [[truth_pair(p, q) for q in b] for p in a]
    return {"iou": torch.tensor([[p[0] for p in r] for r in v], dtype=F64).view(len(a), len(b)),
            "iof": torch.tensor([[p[1] for p in r] for r in v], dtype=F64).view(len(a), len(b))}


@functools.lru_cache(maxsize=None)
def matrix_truth(name):
    return truth_matrix(*matrix_case(name))


# ---- analytic: the kernels' arithmetic in one dtype ---------------------------------------------------------------------------------------
def _np(dtype):
    return np.float64 if dtype in (F64, np.float64) else np.float32


def analytic_hull(vals, T):
    """quad_hull of csrc/ops_quadri.hip for one row of 8 scalars: None for a dead row, else dict(x, y: the hull in raw coordinates, rx,
    ry: relative to the smallest point (ox, oy), area, box: (x0, x1, y0, y1))."""
    vals = [T(v) for v in vals]
    if not C._finite(vals):
        return None
    x, y = vals[0::2], vals[1::2]
    h, rx, ry, ox, oy = C._a_own_hull(x, y)
    area = C._a_fan([rx[i] for i in h], [ry[i] for i in h], T)
    if not area >= T(MIN_AREA):
        return None
    return {"x": [x[i] for i in h], "y": [y[i] for i in h], "rx": [rx[i] for i in h], "ry": [ry[i] for i in h], "ox": ox, "oy": oy,
            "area": area, "box": (min(x), max(x), min(y), max(y))}


def analytic_pair(a, b, mode, T):
    """quad_iou for the hulls a, b of analytic_hull."""
    zero = T(0)
    if a is None or b is None:
        return zero
    (ax0, ax1, ay0, ay1), (bx0, bx1, by0, by1) = a["box"], b["box"]
    if ax1 < bx0 or bx1 < ax0 or ay1 < by0 or by1 < ay0:
        return zero
    inter = C._a_inter([v - b["ox"] for v in a["x"]], [v - b["oy"] for v in a["y"]], b["rx"], b["ry"], T)
    den = a["area"] if mode == "iof" else (a["area"] + b["area"]) - inter
    return inter / den if den >= T(MIN_AREA) else zero


def _v_clip(vx, vy, cnt, ax, ay, ex, ey):
    """cvx_clip over K pairs: vx, vy [K, W] with cnt [K] vertices each, against the line through (ax, ay) with direction (ex, ey), [K]."""
    K, W = vx.shape
    idx = np.arange(W)[None, :]
    valid = idx < cnt[:, None]
    prev = np.where(idx == 0, np.maximum(cnt[:, None] - 1, 0), idx - 1)
    px, py = np.take_along_axis(vx, prev, 1), np.take_along_axis(vy, prev, 1)
    ax, ay, ex, ey = ax[:, None], ay[:, None], ex[:, None], ey[:, None]
    pd = ex * (py - ay) - ey * (px - ax)
    qd = ex * (vy - ay) - ey * (vx - ax)
    cross, inside = valid & ((pd >= 0) != (qd >= 0)), valid & (qd >= 0)
    t = pd / np.where(cross, pd - qd, 1)
    emit = np.stack([cross, inside], 2).reshape(K, 2 * W)
    ox = np.stack([px + t * (vx - px), vx], 2).reshape(K, 2 * W)
    oy = np.stack([py + t * (vy - py), vy], 2).reshape(K, 2 * W)
    pos, count = np.cumsum(emit, 1) - 1, emit.sum(1)
    assert int(count.max(initial=0)) <= W                                     # the cap of CVX_ALL vertices is never met
    nx, ny = np.zeros_like(vx), np.zeros_like(vy)
    rows = np.nonzero(emit)[0]
    nx[rows, pos[emit]], ny[rows, pos[emit]] = ox[emit], oy[emit]
    return nx, ny, count


def _v_fan(vx, vy, cnt):
    total = np.zeros_like(vx[:, 0])
    ex, ey = vx[:, 1] - vx[:, 0], vy[:, 1] - vy[:, 0]
    for k in range(2, vx.shape[1]):
        on = (k < cnt) & (cnt >= 3)
        fx, fy = vx[:, k] - vx[:, 0], vy[:, k] - vy[:, 0]
        total = np.where(on, total + (ex * fy - fx * ey), total)
        ex, ey = np.where(on, fx, ex), np.where(on, fy, ey)
    return total.dtype.type(0.5) * total


def _pad(values, width, T):
    return np.array([list(v) + [v[0]] * (width - len(v)) for v in values], dtype=T).reshape(len(values), width)


def analytic_pairs(hulls1, hulls2, pairs, mode, dtype):
    """quad_iou over the index pairs [(i, j)] of two lists of analytic_hull results, element by element over numpy arrays: [len(pairs)].
    hull 2 is padded to four vertices with its first one (an edge of length zero keeps every vertex and crosses nothing)."""
    T = _np(dtype)
    out = np.zeros(len(pairs), dtype=T)
    live = [k for k, (i, j) in enumerate(pairs) if hulls1[i] is not None and hulls2[j] is not None]
    if not live:
        return out
    a, b = [hulls1[pairs[k][0]] for k in live], [hulls2[pairs[k][1]] for k in live]
    box1, box2 = np.array([h["box"] for h in a], dtype=T), np.array([h["box"] for h in b], dtype=T)
    apart = (box1[:, 1] < box2[:, 0]) | (box2[:, 1] < box1[:, 0]) | (box1[:, 3] < box2[:, 2]) | (box2[:, 3] < box1[:, 2])
    W = 13                                                                  # CVX_ALL, the cap convex_cases._a_clip has too
    ox, oy = np.array([h["ox"] for h in b], dtype=T), np.array([h["oy"] for h in b], dtype=T)
    cnt = np.array([len(h["x"]) for h in a])
    with np.errstate(all="ignore"):
        vx, vy = _pad([h["x"] for h in a], W, T) - ox[:, None], _pad([h["y"] for h in a], W, T) - oy[:, None]
        qx, qy = _pad([h["rx"] for h in b], 4, T), _pad([h["ry"] for h in b], 4, T)
        for e in range(4):
            e1 = (e + 1) % 4
            vx, vy, cnt = _v_clip(vx, vy, cnt, qx[:, e], qy[:, e], qx[:, e1] - qx[:, e], qy[:, e1] - qy[:, e])
        inter = np.maximum(_v_fan(vx, vy, cnt), T(0))
        a1, a2 = np.array([h["area"] for h in a], dtype=T), np.array([h["area"] for h in b], dtype=T)
        den = a1 if mode == "iof" else (a1 + a2) - inter
        ok = ~apart & (den >= T(MIN_AREA))
        out[live] = np.where(ok, inter / np.where(ok, den, T(1)), T(0))
    return out


def _hulls(quads, dtype):
    T = C._scalar(dtype)
    with np.errstate(all="ignore"):
        return [analytic_hull(row, T) for row in quads.tolist()]


def analytic(q1, q2, mode, dtype):
    """The aligned kernel on the CPU in `dtype`: [n]."""
    h1, h2 = _hulls(q1, dtype), _hulls(q2, dtype)
    return torch.from_numpy(analytic_pairs(h1, h2, [(i, i) for i in range(len(h1))], mode, dtype)).to(dtype)


def analytic_matrix(q1, q2, mode, dtype):
    """The matrix kernel on the CPU in `dtype`: [n, m]."""
    h1, h2 = _hulls(q1, dtype), _hulls(q2, dtype)
    pairs = [(i, j) for i in range(len(h1)) for j in range(len(h2))]
    return torch.from_numpy(analytic_pairs(h1, h2, pairs, mode, dtype)).to(dtype).view(len(h1), len(h2))


def analytic_scalar(q1, q2, mode, dtype):
    """analytic() one pair at a time, on scalars with Python branches."""
    T = C._scalar(dtype)
    with np.errstate(all="ignore"):
        v = [analytic_pair(analytic_hull(a, T), analytic_hull(b, T), mode, T) for a, b in zip(q1.tolist(), q2.tolist())]
    return C._tensor(v, dtype).view(len(v))


# ---- NMS ----------------------------------------------------------------------------------------------------------------------------
NMS_SIZES = (1, 64, 65, 200, 1025)
NMS_THRESHOLDS = (0.1, 0.5)
NMS_LABELS = ("none", "three", "straddle")        # no labels; random of 3; three sorted runs whose seams miss the multiples of 64
NMS_SCORES = ("plain", "tied", "nan")             # uniform; rounded to eighths; every seventh NaN -- one kind per (size, threshold)
NMS_GEOMETRIES = tuple((n, thr) for n in NMS_SIZES for thr in NMS_THRESHOLDS)
NMS_CASES = tuple("n%d-t%s-%s" % (n, thr, kind) for n, thr in NMS_GEOMETRIES for kind in NMS_LABELS)


def _overlapping(quads):
    """The index pairs (i, j), i != j, whose float64 bounding boxes are not apart (every other pair has IoU 0 exactly)."""
    v = quads.double().view(-1, 4, 2).numpy()
    lo, hi = v.min(1), v.max(1)
    apart = (hi[:, None, 0] < lo[None, :, 0]) | (hi[None, :, 0] < lo[:, None, 0]) | (hi[:, None, 1] < lo[None, :, 1]) | \
            (hi[None, :, 1] < lo[:, None, 1])
    np.fill_diagonal(apart, True)
    return [tuple(p) for p in np.argwhere(~apart).tolist()]


def iou_pairs(quads, pairs, dtype):
    """The restatement's IoU (mode "iou") of quads[i] with quads[j] for the index pairs, as a float64 numpy array."""
    h = _hulls(quads, dtype)
    return analytic_pairs(h, h, pairs, "iou", dtype).astype(np.float64)


def truth_pairs(quads, pairs):
    rows = _rows(quads)
    return np.array([truth_pair(rows[i], rows[j])[0] for i, j in pairs], dtype=np.float64)


def _clusters(rng, n):
    """n quadrilaterals in clusters of eight partners of one base quadrilateral, the clusters spread so that neighbours touch."""
    groups = -(-n // 8)
    extent = 30.0 * math.sqrt(groups)
    out = []
    for _ in range(groups):
        c, wh, a = C._box(rng, rng.uniform(0, extent, 2))
        local = _local(rng, wh)
        out += [_partner(rng, local, c, wh, a).reshape(8) for _ in range(8)]
    order = rng.permutation(len(out))[:n]
    return np.stack(out)[order]


@functools.lru_cache(maxsize=None)
def nms_geometry(n, thr):
    """dict(quads [n, 8], scores [n], thr rounded to float32, rounds: resampling rounds used, pairs: the overlapping pairs)."""
    k = NMS_GEOMETRIES.index((n, thr))
    rng = np.random.default_rng(100 + k)
    thr = R.f32(thr)
    quads = torch.from_numpy(_clusters(rng, n).astype(np.float32))
    rounds = 0
    for rounds in range(101):
        pairs = _overlapping(quads)
        iou = iou_pairs(quads, pairs, F64)                                   # the restatement in float64: within 1e-12 of the truth
        near = np.abs(iou - thr) < 2 * MARGIN                                # twice the margin here, the margin itself on the truth below
        bad = sorted({p[0] for p, hit in zip(pairs, near) if hit} | {p[1] for p, hit in zip(pairs, near) if hit})
        if not bad:
            break
        fresh = torch.from_numpy(_clusters(rng, n).astype(np.float32))
        quads[bad] = fresh[bad]
    g = torch.Generator().manual_seed(100 + k)
    scores = torch.rand((n,), generator=g, dtype=F32)
    kind = NMS_SCORES[k % 3]
    if kind == "tied":
        scores = torch.round(scores * 8) / 8
    if kind == "nan":
        scores[::7] = float("nan")
    return {"quads": quads, "scores": scores, "thr": thr, "rounds": rounds, "pairs": pairs}


def nms_labels(n, kind, seed=7):
    g = torch.Generator().manual_seed(seed + n)
    if kind == "three":
        return torch.randint(0, 3, (n,), generator=g)
    if kind == "straddle":                                                    # runs of 0.45 n, 0.32 n and the rest, in shuffled positions
        cut = (int(0.45 * n), int(0.77 * n))
        labels = (torch.arange(n) >= cut[0]).long() + (torch.arange(n) >= cut[1]).long()
        return labels[torch.randperm(n, generator=g)]
    return None


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """The geometry of the case's size and threshold with the case's labels."""
    n, thr, kind = name[1:].split("-t")[0], name.split("-t")[1].split("-")[0], name.rsplit("-", 1)[1]
    c = dict(nms_geometry(int(n), float(thr)))
    c.update(name=name, labels=nms_labels(int(n), kind), geometry=(int(n), float(thr)))
    return c


@functools.lru_cache(maxsize=None)
def nms_truth_iou(n, thr):
    """The float64 truth IoU of the geometry's overlapping pairs (every other pair: 0): a numpy array aligned with its "pairs"."""
    c = nms_geometry(n, thr)
    return truth_pairs(c["quads"], c["pairs"])


def nms_keep(c, labels):
    """keep by the greedy pass over the float64 truth, with the given labels."""
    n = c["quads"].shape[0]
    over = torch.zeros((n, n), dtype=torch.bool)
    for (i, j), v in zip(c["pairs"], nms_truth_iou(*c["geometry"]).tolist()):
        over[i, j] = v > c["thr"]
    return R.greedy(over, R.score_order(c["scores"]), labels)


@functools.lru_cache(maxsize=None)
def nms_ref(name):
    c = nms_case(name)
    return nms_keep(c, c["labels"])


# ---- points_in_polygons ---------------------------------------------------------------------------------------------------------------
def _edge_lines(polys):
    """The hull edges of float32 polygons [m, 8] in float64: (a [E, 2], unit normal [E, 2]) over every edge of every live polygon."""
    a, nrm = [], []
    for quad in _rows(polys):
        h = truth_hull(quad)
        for k in range(len(h) if h else 0):
            p, q = h[k], h[(k + 1) % len(h)]
            ln = math.hypot(q[0] - p[0], q[1] - p[1])
            a.append(p); nrm.append(((q[1] - p[1]) / ln, (p[0] - q[0]) / ln))
    return np.array(a, dtype=np.float64).reshape(-1, 2), np.array(nrm, dtype=np.float64).reshape(-1, 2)


def line_distance(points, polys):
    """[n]: the smallest float64 distance of each point to the line of any hull edge of any polygon."""
    a, nrm = _edge_lines(polys)
    p = points.double().numpy()
    return np.abs(((p[:, None, :] - a[None]) * nrm[None]).sum(-1)).min(1)


@functools.lru_cache(maxsize=None)
def point_case(name):
    """(points [n, 2], polygons [m, 8], rounds) float32: point i around polygon i mod m."""
    n, m, seed = (MATRIX if name in MATRIX else POINT_SEAMS)[name]
    rng = np.random.default_rng(1000 + seed)
    cols = _columns(rng, m)
    polys = _f32([_place(local, c, a).reshape(8) for c, wh, a, local in cols])
    draw = lambda i: cols[i % m][0] + C._rot(cols[i % m][2]) @ (rng.uniform(-0.8, 0.8, 2) * cols[i % m][1])      # noqa: E731
    points = _f32([draw(i) for i in range(n)])
    rounds = 0
    for rounds in range(101):
        bad = np.nonzero(line_distance(points, polys) < DELTA)[0].tolist()
        if not bad:
            break
        for i in bad:
            points[i] = torch.from_numpy(draw(i).astype(np.float32))
    return points, polys, rounds


def truth_inside(points, polys):
    """float64 [n, m]: 1 where the point is in the closed hull (cross >= 0 for every edge, on raw coordinates), 0 for a dead row."""
    pts = points.double().tolist()
    out = torch.zeros((len(pts), polys.shape[0]), dtype=F64)
    for j, quad in enumerate(_rows(polys)):
        h = truth_hull(quad)
        if h is None:
            continue
        for i, p in enumerate(pts):
            if all(math.isfinite(v) for v in p):
                out[i, j] = float(all(C._cross(h[k], h[(k + 1) % len(h)], p) >= 0 for k in range(len(h))))
    return out


def analytic_inside(points, polys, dtype):
    """ops_points_in_polygons_kernel on the CPU in `dtype` -> [n, m] of that dtype: every difference relative to the hull's smallest
    vertex, the two rounded products compared."""
    T = C._scalar(dtype)
    hulls = _hulls(polys, dtype)
    pts = [[T(v) for v in p] for p in points.tolist()]
    out = torch.zeros((len(pts), len(hulls)), dtype=dtype)
    with np.errstate(all="ignore"):
        for j, h in enumerate(hulls):
            if h is None:
                continue
            k = len(h["rx"])
            for i, (x, y) in enumerate(pts):
                if not C._finite((x, y)):
                    continue
                px, py = x - h["ox"], y - h["oy"]
                ok = True
                for e in range(k):
                    ax, ay, bx, by = h["rx"][e], h["ry"][e], h["rx"][(e + 1) % k], h["ry"][(e + 1) % k]
                    ok = ok and bool((bx - ax) * (py - ay) >= (by - ay) * (px - ax))
                out[i, j] = float(ok)
    return out


# ---- conditions -------------------------------------------------------------------------------------------------------------------------
def nms_restatement_error():
    """The worst |float32 restatement - truth| of an IoU over every NMS geometry's overlapping pairs."""
    worst = 0.0
    for n, thr in NMS_GEOMETRIES:
        c = nms_geometry(n, thr)
        if c["pairs"]:
            worst = max(worst, float(np.abs(iou_pairs(c["quads"], c["pairs"], F32) - nms_truth_iou(n, thr)).max()))
    return worst


def check_conditions():
    """Every eighth pair of a random case has I = 0 and the others reach an IoU above 0.3; the NMS resampling ended within 100 rounds, no
    pair is left within MARGIN of its threshold, and MARGIN is 30 times the measured float32 error rounded up to a power of ten; no
    point is left within DELTA of an edge's line, the float32 restatement places every point as the truth does, and between 5 % and
    95 % of the own pairs are inside."""
    for name in ALIGNED_CASES:
        n, t = ALIGNED[name][0], truth(name)
        moved = torch.arange(n) % 8 == 7
        assert bool((t["iou"][moved] == 0).all()) and bool((t["iof"][moved] == 0).all()), name
        if n >= 8:
            assert float(t["iou"].max()) > 0.3 and bool((t["iou"][~moved] > 0).any()), name
    for n, thr in NMS_GEOMETRIES:
        c = nms_geometry(n, thr)
        assert c["rounds"] < 100, (n, thr, c["rounds"])
        if c["pairs"]:
            iou = nms_truth_iou(n, thr)
            gap = float(np.abs(iou - c["thr"]).min())
            print("n %d thr %s: %d rounds, %d overlapping pairs, %d above the threshold, nearest IoU %.2e from it"
                  % (n, thr, c["rounds"], len(c["pairs"]), int((iou > c["thr"]).sum()), gap))
            assert gap >= MARGIN, (n, thr, gap)
            assert n < 64 or (0.02 * len(iou) < int((iou > c["thr"]).sum()) < 0.98 * len(iou)), (n, thr)
    for n in NMS_SIZES[1:]:                                                   # a label run straddles a multiple of 64
        runs = torch.sort(nms_labels(n, "straddle")).values
        seams = (runs[1:] != runs[:-1]).nonzero()[:, 0] + 1
        assert len(seams) == 2 and all(int(v) % 64 != 0 for v in seams), (n, seams)
    err = nms_restatement_error()
    print("worst |float32 restatement - truth| over the NMS cases: %.3e" % err)
    assert MARGIN == 10.0 ** math.ceil(math.log10(30 * err)), err
    for name in POINT_CASES:
        points, polys, rounds = point_case(name)
        assert rounds < 100 and float(line_distance(points, polys).min()) >= DELTA, name
        want = truth_inside(points, polys)
        assert torch.equal(analytic_inside(points, polys, F32).double(), want), name
        n, m = want.shape
        own = want[torch.arange(n), torch.arange(n) % m]
        print("%s: %.0f %% of the own pairs inside" % (name, 100 * float(own.mean())))
        if n >= 30:
            assert 0.05 <= float(own.mean()) <= 0.95, name
