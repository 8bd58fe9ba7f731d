"""
Case generators for the box-decision kernels: the IoU-threshold tests of frcnn_nms (csrc/proposals.hip: iou_gt), the per-class detection
NMS (csrc/detect.hip), anchor labelling (csrc/targets.hip) and proposal labelling (csrc/train.hip: label_proposals_kernel).

Random boxes almost never land where a kernel's shortcut around the IoU division could go wrong, so these generators build the pairs that
do: float32 IoU exactly at the threshold, one ulp either side, inside iou_gt's band, degenerate and inverted boxes, tied and odd scores.
Every family is built here once and checked by tests/test_box_decisions_cpu.py with the oracle's own expressions (a family that a later
change empties fails there, on a machine without a GPU); tests/test_box_decisions_gpu.py compares the kernels with the oracle on them.
"""
import numpy as np

F32 = np.float32
NMS_THRESHOLDS = (0.7, 0.5, 0.3, 0.0, 0.999)
NMS_SCALES = ("pixel", "subpixel", "1e5", "subnormal")
KINDS = ("eq", "up", "down", "band")
DET_THR = 0.3


# ---- float32 IoU: the oracle's expression (oracle/frcnn_oracle.py: nms) and a numpy emulation of iou_gt's shortcut ---------------------
def iou_f32(a, b):
    """fl(inter / union) of rows a, b (float32 arrays (..., 4)) exactly as O.nms evaluates it."""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    d0 = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), F32(0))
    d1 = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), F32(0))
    inter = d0 * d1
    sa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    sb = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    with np.errstate(all="ignore"):
        return inter / (sa + sb - inter), inter, sa + sb - inter


def iou_gt_takes_division(a, b, thr):
    """True where csrc/proposals.hip: iou_gt cannot decide from its two bounds and divides."""
    _, inter, uni = iou_f32(a, b)
    with np.errstate(all="ignore"):
        t = F32(thr) * uni
        return ~(uni > 0) | ((inter <= t * F32(1.000001)) & (inter >= t * F32(0.999999)))


def nudge(x, k):
    """x moved by k float32 ulps (x > 0 or subnormal >= 0): k applications of np.nextafter, done on the bit pattern."""
    x = np.asarray(x, F32)
    return (x.view(np.int32) + np.asarray(k, np.int32)).view(F32)


# ---- 1. frcnn_nms at the threshold --------------------------------------------------------------------------------------------------
def _scale_params(scale):
    """(origin range, side range) per scale.  The origin keeps every coordinate positive (nudge() works on positive bit patterns)."""
    return {"pixel": ((1.0, 400.0), (10.0, 600.0)),        # coordinates up to 1000
            "subpixel": ((1.0, 100.0), (0.05, 0.9)),
            "1e5": ((1.0e5, 1.3e5), (20.0, 600.0)),
            "subnormal": ((1e-18, 1e-17), (5e-20, 1.05e-19))}[scale]    # areas 2.5e-39 .. 1.1e-38: float32 subnormals


def threshold_pairs(scale, thr, n_cand=400000, seed=0):
    """Candidate pairs (a, b) whose float32 IoU lies near thr: b is a shifted along x (so that (w - dx) / (w + dx) ~ thr) plus a few ulps
    of noise on three of b's coordinates.  Returns dict kind -> (a, b) arrays (k, 4), the kinds of KINDS, disjoint:
      eq: fl(IoU) == thr;  up / down: one float32 ulp above / below (thr 0: "up" is any IoU in (0, 1e-4), "down" cannot exist);
      band: none of those, but iou_gt's bounds cannot decide the pair and it divides."""
    rng = np.random.RandomState(seed + int(thr * 1000) + 7919 * NMS_SCALES.index(scale))
    (o0, o1), (s0, s1) = _scale_params(scale)
    y = rng.uniform(o0, o1, n_cand); x = rng.uniform(o0, o1, n_cand)
    h = np.exp(rng.uniform(np.log(s0), np.log(s1), n_cand)); w = np.exp(rng.uniform(np.log(s0), np.log(s1), n_cand))
    dx = w * (1.0 - thr) / (1.0 + thr)
    a = np.stack([y, x, y + h, x + w], axis=1).astype(F32)
    b = np.stack([y, x + dx, y + h, x + w + dx], axis=1).astype(F32)
    for c in (0, 1, 3):
        b[:, c] = nudge(b[:, c], rng.randint(-6, 7, n_cand))
    if thr == 0.0:                       # touching boxes (eq) and the smallest overlaps (up): b's left edge on / just inside a's right edge
        b[:, 1] = nudge(a[:, 3], rng.randint(-2, 1, n_cand))
    iou, _, uni = iou_f32(a, b)
    thr_f = F32(thr)
    eq = iou == thr_f
    up = (iou > 0) & (iou < 1e-4) if thr == 0.0 else iou == np.nextafter(thr_f, F32(np.inf))
    down = np.zeros_like(eq) if thr == 0.0 else iou == np.nextafter(thr_f, F32(-np.inf))
    band = iou_gt_takes_division(a, b, thr) & (uni > 0) & ~eq & ~up & ~down
    return {k: (a[m], b[m]) for k, m in (("eq", eq), ("up", up), ("down", down), ("band", band))}


def pack_isolated(lo, hi, idx):
    """Greedily picks from idx the pairs whose bounding boxes (lo, hi) overlap no pair picked before (each pair is decided on its own)."""
    kept = []
    for i in idx:
        if kept:
            k = np.asarray(kept)
            if (np.all(lo[k] <= hi[i], axis=1) & np.all(lo[i] <= hi[k], axis=1)).any():
                continue
        kept.append(i)
    return kept


def _pairs_to_call(a, b):
    boxes = np.empty((2 * a.shape[0], 4), F32)
    boxes[0::2] = a; boxes[1::2] = b                                     # box 2p (the higher score) before box 2p + 1
    return boxes, np.linspace(0.99, 0.01, boxes.shape[0]).astype(F32)


def threshold_calls(scale, thr, per_kind=40, max_calls=12, seed=0):
    """frcnn_nms inputs of isolated pairs, up to per_kind of each kind over at most max_calls calls.  Returns a list of (boxes, scores,
    kinds of the pairs)."""
    fam = threshold_pairs(scale, thr, seed=seed)
    a = np.concatenate([fam[k][0][:per_kind * 20] for k in KINDS]); b = np.concatenate([fam[k][1][:per_kind * 20] for k in KINDS])
    kinds = np.concatenate([np.full(min(fam[k][0].shape[0], per_kind * 20), k) for k in KINDS])
    lo = np.minimum(a[:, :2], b[:, :2]); hi = np.maximum(a[:, 2:], b[:, 2:])
    left = {k: list(np.where(kinds == k)[0]) for k in KINDS}
    quota = {k: per_kind for k in KINDS}
    calls = []
    while len(calls) < max_calls and any(quota[k] and left[k] for k in KINDS):
        want = [i for k in KINDS for i in left[k][:max(quota[k], 0) * 4]]
        got = pack_isolated(lo, hi, want)
        sel = []
        for i in got:
            if quota[kinds[i]] > 0:
                quota[kinds[i]] -= 1; sel.append(i)
        used = set(got)
        for k in KINDS:
            left[k] = [i for i in left[k] if i not in used]
        if not sel:
            break
        boxes, scores = _pairs_to_call(a[sel], b[sel])
        calls.append((boxes, scores, kinds[sel]))
    return calls


def dense_call(scale, thr, per_kind=400, seed=1):
    """Every kind's pairs in one call, overlapping each other freely (the full keep list is compared with the oracle's)."""
    fam = threshold_pairs(scale, thr, seed=seed)
    a = np.concatenate([fam[k][0][:per_kind] for k in KINDS]); b = np.concatenate([fam[k][1][:per_kind] for k in KINDS])
    return _pairs_to_call(a, b)


def filler_boxes(n, x0=3000.0):
    """n disjoint 10 x 10 boxes on a 20 px grid far right of every other family (x >= x0): each is kept."""
    i = np.arange(n)
    y = (i % 200) * 20.0 + 1.0; x = x0 + (i // 200) * 20.0
    return np.stack([y, x, y + 10.0, x + 10.0], axis=1).astype(F32)


def tiled_call(n, pairs, positions):
    """n boxes: the pair p sits at sorted ranks (positions[p], positions[p] + 1) -- a 64-box tile boundary or past 8192 -- the rest are
    fillers.  Scores descend with the rank."""
    a, b = pairs
    boxes = filler_boxes(n)
    for p, r in enumerate(positions):
        boxes[r] = a[p]; boxes[r + 1] = b[p]
    scores = np.linspace(1.0, 0.001, n).astype(F32)
    return boxes, scores


# ---- 2. degenerate boxes ------------------------------------------------------------------------------------------------------------
def degenerate_families():
    """Directed small inputs: name -> (boxes, scores).  Scores descend with the index."""
    fam = {}
    fam["zero_width"] = [[10, 10, 50, 10], [10, 10, 50, 30], [10, 10, 50, 10], [20, 10, 30, 10]]
    fam["zero_height"] = [[10, 10, 10, 50], [10, 10, 30, 50], [10, 10, 10, 50]]
    fam["point"] = [[5, 5, 5, 5], [5, 5, 5, 5], [0, 0, 10, 10], [5, 5, 5, 5]]
    fam["identical"] = [[1, 2, 31, 42]] * 3 + [[1, 2, 31, 42.0001]]
    fam["nested"] = [[0, 0, 100, 100], [10, 10, 90, 90], [0, 0, 100, 70], [0, 0, 100, 71], [40, 40, 60, 60]]
    fam["inverted_one_axis"] = [[0, 10, 10, 0], [2, 2, 8, 8], [10, 0, 0, 10], [3, 3, 9, 9], [0, 0, 10, 10]]
    fam["inverted_both_axes"] = [[10, 10, 0, 0], [2, 2, 8, 8], [0, 0, 10, 10], [10, 10, 0, 0]]
    fam["inverted_touching"] = [[0, 20, 10, 10], [0, 0, 10, 10], [0, 10, 10, 20], [10, 0, 0, 10], [0, 10, 10, 20]]
    out = {}
    for k, v in fam.items():
        b = np.asarray(v, F32)
        out[k] = (b, np.linspace(0.9, 0.1, b.shape[0]).astype(F32))
    # the issue's directed case: a = (0, 10, 10, 0) 0.9, b = (2, 2, 8, 8) 0.8 at 0.7
    out["issue_directed"] = (np.asarray([[0, 10, 10, 0], [2, 2, 8, 8]], F32), np.asarray([0.9, 0.8], F32))
    return out


def cluster_boxes(n, seed, clusters=40):
    rng = np.random.RandomState(seed)
    centers = rng.rand(clusters, 2) * np.array([560, 960]) + 20
    c = centers[rng.randint(0, clusters, size=n)] + rng.randn(n, 2) * 6
    hw = np.abs(rng.randn(n, 2)) * 30 + 30 + rng.rand(n, 2) * 3
    return np.concatenate([c - hw / 2, c + hw / 2], axis=1).astype(F32)


def degenerate_mixed(n=6000, seed=11):
    """Clustered boxes with every degenerate family mixed in: ~1/3 of the rows are degenerate, drawn from the same clusters."""
    rng = np.random.RandomState(seed)
    b = cluster_boxes(n, seed)
    kind = rng.randint(0, 9, n)
    y1, x1, y2, x2 = (b[:, i].copy() for i in range(4))
    m = kind == 0; x2[m] = x1[m]                                             # zero width
    m = kind == 1; y2[m] = y1[m]                                             # zero height
    m = kind == 2; y2[m] = y1[m]; x2[m] = x1[m]                              # point
    m = kind == 3; x1[m], x2[m] = x2[m].copy(), x1[m].copy()                # inverted along x
    m = kind == 4; y1[m], y2[m], x1[m], x2[m] = y2[m].copy(), y1[m].copy(), x2[m].copy(), x1[m].copy()   # both axes
    out = np.stack([y1, x1, y2, x2], axis=1).astype(F32)
    dup = np.where(kind == 5)[0]
    out[dup[1::2]] = out[dup[0::2]][:dup[1::2].shape[0]]                     # identical to another row
    nest = np.where(kind == 6)[0]
    out[nest, 2] = out[nest, 0] + (out[nest, 2] - out[nest, 0]) * F32(0.5)   # (rows near a nested partner in their cluster)
    touch = np.where(kind == 7)[0][1:]
    out[touch, 1] = out[touch - 1, 3]; out[touch, 3] = out[touch - 1, 1] - F32(5)   # inverted, left edge on a neighbour's right edge
    s = rng.rand(n).astype(F32)
    return out, s


# ---- 3. score order -----------------------------------------------------------------------------------------------------------------
def score_families():
    """name -> (boxes, scores): every pair of boxes overlaps at IoU 0.9 (so the order decides which one is kept) and the scores are odd."""
    def chain(scores):
        k = len(scores)
        y = np.arange(k) * 0.0
        x = np.arange(k) * 1.0                                                # each box overlaps its neighbours heavily
        b = np.stack([y, x, y + 100.0, x + 100.0], axis=1).astype(F32)
        return b, np.asarray(scores, F32)
    tiny = np.float32(1e-44)
    return {
        "exact_ties": chain([0.5, 0.5, 0.5, 0.7, 0.5]),
        "signed_zero": chain([0.0, -0.0, 0.0, -0.0]),
        "signed_zero_neg_first": chain([-0.0, 0.0, -0.0, 0.0]),
        "inf": chain([1.0, np.inf, -np.inf, 0.0, np.inf, -np.inf]),
        "subnormal": chain([tiny, 2 * tiny, -tiny, 0.0, -0.0, tiny]),
        "nan": chain([np.nan, 0.5, -np.inf, np.nan, -0.0, -np.nan]),
        "nan_only": chain([np.nan, np.nan, np.nan]),
    }


def isolated_score_call(scores):
    """Disjoint boxes with the given scores: the keep list is exactly the sort order."""
    s = np.asarray(scores, F32)
    return filler_boxes(s.shape[0], x0=0.0), s


# ---- 5. detection NMS ---------------------------------------------------------------------------------------------------------------
def det_decode(props, clip_h=599.0, clip_w=999.0, deltas=None):
    """Boxes frcnn_detections decodes from proposals with zero deltas (or one class's float32 deltas (n, 4)): the oracle's float32 anchor
    then float64 arithmetic (oracle/frcnn_oracle.py: detections / convert_deltas_to_boxes), clipped."""
    from oracle import frcnn_oracle as O
    p = np.asarray(props, F32)
    anchors = np.empty((p.shape[0], 4))
    anchors[:, 0:2] = 0.5 * (p[:, 0:2] + p[:, 2:4])
    anchors[:, 2:4] = p[:, 2:4] - p[:, 0:2]
    d = np.zeros((p.shape[0], 4)) if deltas is None else np.asarray(deltas, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        boxes = O.convert_deltas_to_boxes(d, anchors, np.zeros(4), np.array([0.1, 0.1, 0.2, 0.2]))
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, clip_h)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, clip_w)
    return boxes


def det_pair_class(bi, bj, thr=DET_THR):
    """How detect.hip's bit matrix decides the float64 pair: 'zero' (a box of zero area), 'margin' (inside the float32 pre-filter margin:
    the float64 expression runs), 'band' (inside the 1e-12 band too: the division runs), or 'fast'.  Mirrors lhs / margin in float32."""
    if (bi[2] - bi[0] == 0) or (bi[3] - bi[1] == 0) or (bj[2] - bj[0] == 0) or (bj[3] - bj[1] == 0):
        return "zero"
    a = np.asarray(bi, F32); b = np.asarray(bj, F32)
    oy = min(a[2], b[2]) - max(a[0], b[0]); ox = min(a[3], b[3]) - max(a[1], b[1])
    if oy < F32(-1e-3) or ox < F32(-1e-3):
        return "fast"
    inter = max(oy, F32(0)) * max(ox, F32(0))
    ha, wa, hb, wb = a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]
    lhs = inter - F32(thr) * (ha * wa + hb * wb - inter)
    margin = F32(1e-3) * (ha + wa + hb + wb + F32(1.0))
    if not (-margin <= lhs <= margin):
        return "fast"
    e0 = max(min(bi[2], bj[2]) - max(bi[0], bj[0]), 0.0); e1 = max(min(bi[3], bj[3]) - max(bi[1], bj[1]), 0.0)
    it = e0 * e1
    un = (bi[2] - bi[0]) * (bi[3] - bi[1]) + (bj[2] - bj[0]) * (bj[3] - bj[1]) - it
    rhs = thr * un
    return "band" if (rhs * (1 - 1e-12) <= it <= rhs * (1 + 1e-12)) else "margin"


def detection_case(seed=3):
    """(props [300, 4], classes [300, 21], n): per class a few pairs at 0.3 (float64 IoU exactly 0.3 -- the division path -- built from
    rational sides, and pairs a fraction of a pixel away -- the float64 path), a box clipped to zero area at the image edge, equal class
    scores, and a class with exactly one row above the score threshold.  Deltas are zero."""
    rng = np.random.RandomState(seed)
    props, cls_of, score = [], [], []

    def add(box, c, s):
        props.append(box); cls_of.append(c); score.append(s)

    for c in range(1, 19):
        oy, ox = 30.0 * (c % 6) + 20.0, 160.0 * (c // 6) + 20.0
        k = 1 + (c % 3)
        H = 10.0 * k; W = 13.0 * k
        add([oy, ox, oy + H, ox + W], c, 0.9)
        add([oy, ox, oy + 0.3 * H if c % 2 else oy + H, ox + W if c % 2 else ox + 0.3 * W], c, 0.8)   # nested: IoU 0.3 exactly
        add([oy, ox + 7.0 * k, oy + H, ox + 20.0 * k], c, 0.7)                                      # shifted 7/13: IoU 0.3 exactly
        eps = float(rng.choice([1.0 / 64, 1.0 / 256, 1.0 / 1024]))
        add([oy + 300, ox, oy + 300 + H, ox + W], c, 0.6)
        add([oy + 300, ox + 7.0 * k + eps, oy + 300 + H, ox + 20.0 * k + eps], c, 0.5)              # the float64 path, above 0.3
        add([oy + 300, ox + 7.0 * k - eps, oy + 300 + H, ox + 20.0 * k - eps], c, 0.4)              # ... and below
        add([700.0, ox, 720.0, ox + 30.0], c, 0.55)                                                # clipped to y = 599: zero height
        add([oy + 150, ox, oy + 190, ox + 50], c, 0.45)
        add([oy + 150, ox + 10, oy + 190, ox + 60], c, 0.45)                                       # equal score: index order
    add([500.0, 900.0, 560.0, 980.0], 19, 0.5)                                                     # class 19: exactly one row
    n = len(props)
    p = np.zeros((300, 4), F32)
    p[:n] = np.asarray(props, F32)
    classes = np.zeros((300, 21), F32)
    classes[:, 0] = 0.01
    for i, (c, s) in enumerate(zip(cls_of, score)):
        classes[i, c] = s
    classes[:n, 20] = 0.02                                                                          # class 20: nothing above 0.05
    return p, classes, n, np.asarray(cls_of)


def detection_pair_classes(props, cls_of, n):
    boxes = det_decode(props[:n])
    kinds = []
    for c in np.unique(cls_of):
        idx = np.where(cls_of == c)[0]
        for x in range(len(idx)):
            for y in range(x + 1, len(idx)):
                kinds.append(det_pair_class(boxes[idx[x]], boxes[idx[y]]))
    return kinds


# ---- 6. anchor labelling ------------------------------------------------------------------------------------------------------------
def anchor_maps(image_shape=(3, 600, 1000), fmap=(512, 37, 62)):
    from oracle import frcnn_oracle as O
    return O.generate_anchor_maps(image_shape, fmap, 16)


def anchor_corners_f64(am):
    a = am.reshape(-1, 4)
    c = np.empty(a.shape)
    c[:, 0:2] = a[:, 0:2] - F32(0.5) * a[:, 2:4]
    c[:, 2:4] = a[:, 0:2] + F32(0.5) * a[:, 2:4]
    return c


def iou_rpn(corners, gt):
    """The oracle's float64 anchor IoU (oracle/frcnn_oracle.py: generate_rpn_map, eps 1e-7) of every anchor with one float32 GT box."""
    g = np.asarray(gt, F32)
    tl = np.maximum(corners[:, 0:2], g[0:2]); br = np.minimum(corners[:, 2:4], g[2:4])
    ok = np.all(tl < br, axis=1)
    inter = ok * np.prod(br - tl, axis=1)
    a1 = np.prod(corners[:, 2:4] - corners[:, 0:2], axis=1)
    a2 = np.prod(g[2:4] - g[0:2])                                              # float32, as the reference's math_utils.py:34
    return inter / (a1 + a2 - inter + 1e-7)


def gt_near_threshold(corners, anchor, thr, side, span=1200):
    """A float32 GT box whose float64 IoU with anchor `anchor` is the closest to thr that a search over float32 nudges of its bottom and
    right edges finds, on the given side ('below': < thr, 'at_or_above': >= thr).  Returns (gt, iou)."""
    c = corners[anchor]
    h, w = c[2] - c[0], c[3] - c[1]
    # a GT of the anchor's width, shifted down: IoU = (h - s) / (h + s) -> s = h (1 - thr) / (1 + thr)
    s = h * (1 - thr) / (1 + thr)
    base = np.asarray([c[0] + s, c[1], c[2] + s, c[3]], F32)
    k = np.arange(-span, span + 1)
    y2 = nudge(np.full(k.shape, base[2]), k)
    x2 = nudge(np.full(k.shape, base[3]), k)
    Y2, X2 = np.meshgrid(y2, x2, indexing="ij")
    G = np.stack([np.full(Y2.shape, base[0]), np.full(Y2.shape, base[1]), Y2, X2], axis=-1).reshape(-1, 4).astype(np.float64)
    Gf = G.astype(F32)
    tl = np.maximum(c[None, 0:2], G[:, 0:2]); br = np.minimum(c[None, 2:4], G[:, 2:4])
    ok = np.all(tl < br, axis=1)
    inter = ok * np.prod(br - tl, axis=1)
    iou = inter / (h * w + np.prod(Gf[:, 2:4] - Gf[:, 0:2], axis=1) - inter + 1e-7)     # (the GT area in float32)
    m = iou < thr if side == "below" else iou >= thr
    j = np.where(m)[0][np.argmin(np.abs(iou[m] - thr))]
    return G[j].astype(F32), iou[j]


def rpn_cases(am, vm):
    """name -> float32 GT array (M, 4) for frcnn_rpn_targets against O.generate_rpn_map; "thresholds" comes with its (anchor, thr,
    side) targets in rpn_cases.targets."""
    corners = anchor_corners_f64(am)
    valid = vm.reshape(-1) > 0
    vidx = np.where(valid)[0]
    cases = {}
    # anchors in the middle of the map: a GT placed at a threshold against one anchor, and one on the other side against another
    mid = vidx[len(vidx) // 2]
    gts, targets = [], []
    # the anchor must not be its GT's best one (that would make it positive whatever its IoU): tall anchors, whose GT is shifted by
    # several strides, so that an anchor further down overlaps the GT more
    area = np.prod(corners[:, 2:4] - corners[:, 0:2], axis=1)
    big = vidx[area[vidx] == area[vidx].max()]
    for j, (thr, side) in enumerate([(0.7, "below"), (0.7, "at_or_above"), (0.3, "below"), (0.3, "at_or_above")]):
        for a in big[(len(big) * (2 * j + 1)) // 9:]:
            g, v = gt_near_threshold(corners, a, thr, side, span=600)
            iou = iou_rpn(corners, g)
            if iou[valid].max() > v:
                break
        gts.append(g); targets.append((a, thr, side))
    cases["thresholds"] = np.asarray(gts, F32)
    rpn_cases.targets = targets
    c = corners[mid]
    cy, cx = 0.5 * (c[0] + c[2]), 0.5 * (c[1] + c[3])
    h, w = c[2] - c[0], c[3] - c[1]
    # two GT boxes mirrored about the anchor centre: the same IoU, different centres (the first one's target wins)
    cases["two_gt_tie"] = np.asarray([[cy - h / 2, cx - w / 2 + 24, cy + h / 2, cx + w / 2 + 24],
                                      [cy - h / 2, cx - w / 2 - 24, cy + h / 2, cx + w / 2 - 24]], F32)
    # a GT centred between two anchor centres one stride apart: tied for its maximum
    cases["anchors_tied"] = np.asarray([[cy - h / 2, cx - w / 2 + 8, cy + h / 2, cx + w / 2 + 8]], F32)
    cases["zero_area_gt"] = np.asarray([[200, 300, 200, 420], [100, 100, 260, 300]], F32)
    cases["gt_outside"] = np.asarray([[700, 1100, 800, 1300], [100, 100, 260, 300]], F32)
    cases["gt_invalid_only"] = np.asarray([[0, 0, 6, 6], [300, 500, 420, 700]], F32)
    return cases


# ---- 7. proposal labelling ----------------------------------------------------------------------------------------------------------
def iou_label(p, g):
    """math_utils.py:39-63 in float32 with eps 1e-7 (oracle/train_oracle.py: t_iou)."""
    import torch
    from oracle import train_oracle as TO
    return TO.t_iou(torch.as_tensor(np.asarray(p, F32)).reshape(-1, 4), torch.as_tensor(np.asarray(g, F32)).reshape(-1, 4)).numpy()


def label_case():
    """(proposals (n, 4), gt (m, 4), gt_cls (m,)): IoU exactly 0.5, one ulp below 0.5, exactly 0.1 and 0.0, duplicate GT boxes of
    different classes, a proposal identical to a GT, a zero-area proposal."""
    gt = np.asarray([[0, 0, 10, 20], [300, 300, 400, 400], [300, 300, 400, 400], [500, 500, 600, 550]], F32)
    gt_cls = np.asarray([4, 9, 2, 13], np.int64)
    props = [[0, 0, 10, 10],                    # (0, 0, 10, 20): 200 + 1e-7 -> 200 in float32, IoU 0.5 exactly
             [300, 300, 400, 400],             # identical to GT 1 (and its duplicate, class 2): class 9 wins
             [300, 300, 350, 400],             # IoU 0.5 with the duplicated pair
             [500, 500, 510, 550],             # IoU 0.1 exactly (500 / 5000)
             [500, 550, 600, 600],             # touching: IoU 0.0
             [50, 50, 50, 80],                 # zero area: inf / NaN targets
             [700, 700, 800, 800]]             # nothing: IoU 0
    p = np.asarray(props, F32)
    # one float32 ulp below 0.5: shrink proposal 2's bottom edge until fl(IoU) is 0.5 - ulp
    below = np.nextafter(F32(0.5), F32(0))
    q = np.asarray([[0, 40, 10, 50]], F32)
    g2 = np.asarray([0, 40, 10, 60], F32)
    for k in range(1, 4000):
        q[0, 2] = nudge(F32(10), -k)
        if iou_label(q, g2[None])[0, 0] == below:
            break
    gt = np.vstack([gt, g2[None]]); gt_cls = np.append(gt_cls, 6)
    p = np.vstack([p, q])
    return p, gt, gt_cls
