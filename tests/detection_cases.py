"""
Case generators for the per-class detection NMS (csrc/detect.hip: detections_kernel) at its word, rank, count, class-stride, decode and
pre-filter seams.  Pure numpy; tests/test_detections_cpu.py checks with the oracle that every family is what it claims to be (a family
that a later edit empties fails there, without a GPU), tests/test_detections_gpu.py compares frcnn_detections with the oracle on them.
The float64 decode (det_decode), the scalar path classifier (det_pair_class) and nudge are tests/box_decisions_cases.py's.

A case is the tuple (props, classes, deltas, n, max_rois, ncls, image_h, image_w, score_thr, nms_thr); the arrays have max_rois rows.  A
family returns a list of (name, case, facts): facts holds the structural claims, computed from the decoded boxes and the oracle's rule.

Out of scope (the reference cannot produce them, the kernel is not changed for them): zero-size proposals whose exp overflows and NaN
deltas (0 * inf = NaN: the device fmin / fmax drop a NaN where np.clip keeps it), -0.0 scores, NMS thresholds outside [0, 1].


The float32 pre-filter of the bit matrix: how far it can be from the float64 decision
-------------------------------------------------------------------------------------
The kernel (built with -ffp-contract=off: every operation below rounds once, to nearest) decides a pair in float32 when it can:
    oy = min(a2, b2) - max(a0, b0), ox likewise;  never = oy < -1e-3 or ox < -1e-3                      (not suppressed)
    lhs = I - t * ((ha * wa + hb * wb) - I),  I = max(oy, 0) * max(ox, 0);  margin = 1e-3 * (ha + wa + hb + wb + 1)
    lhs > margin: suppressed;  lhs < -margin: not;  else the reference's float64 expression it / un > t runs.
a, b are the float64 boxes rounded to float32, clipped to [0, H-1] x [0, W-1]; L = max(H, W) - 1; t is the float32 threshold (the float64
path uses the same value widened, so t carries no error); u = 2^-24.  E = it - t * un in exact arithmetic; the float64 path's own rounding
(a few 2^-53 * un) is 1e-8 px^2 at L = 10^4 and is carried by the "+ 1" of the margin below.

1. A coordinate c in [0, L] rounds with |c^ - c| <= u c.  Rounding is monotone, so min / max commute with it.
2. oy (and ox): the two operands carry u (y1 + y2') <= 2 u L together, the subtraction adds u |oy|: |oy^ - oy| <= 2 u L (+ u |oy|).
   That alone would admit the `never` shortcut only while 2 u L < 1e-3 (L < 8388).  Monotonicity gives more: if the float64 boxes touch or
   overlap along y, min(a2, b2) >= max(a0, b0), so the rounded operands are ordered the same way and oy^ >= 0 exactly.  Hence oy^ < 0
   (a fortiori < -1e-3) implies oy < 0, it = 0 and IoU = 0 <= t: the `never` shortcut is exact for every image size and every t >= 0.
3. A side h = y2 - y1: |h^ - h| <= u (y1 + y2) + u h = 2 u y2 <= 2 u L.  So with s = ha + wa + hb + wb, Q = ha wa + hb wb <= L s / 2,
   e0 + e1 <= s / 2 (the overlap is no larger than either box), it <= Q / 2, un <= Q:
     |d(ha wa)| <= 2 u L (ha + wa) + u ha wa      (two sides, one product rounding; second order 4 u^2 L^2)
     |d I|      <= 2 u L (e0 + e1) + u it <= u L s + u Q / 2
     |d(Pa + Pb)| <= 2 u L s + u Q + u Q          (the sum's rounding)
     |d un^|    <= |d(Pa + Pb)| + |d I| + u un
     |d(t un^)| <= t |d un^| + t u un
     lhs = fl(I^ - T^): the last rounding is u |lhs|, and a wrong decision needs |lhs| <= |lhs - E|, so it only scales the bound by 1/(1-u).
   Since E = (1 + t) it - t (Pa + Pb):
     |lhs - E| <= (1 + t)(u L s + u Q / 2) + t (2 u L s + 2 u Q) + 2 t u Q
               <= u L s (1 + 3 t) + u Q (1/2 + 9 t / 2) <= u L s (1.25 + 5.25 t)                         =: BOUND
   Second-order terms (<= 20 u^2 L^2), the float32 rounding of the margin itself (<= 1e-3 * 8 u L) and the float64 path's rounding stay
   below 2e-5 for L <= 7000, against the 1e-3 that the "+ 1" adds to the margin.
4. The margin shortcut is exact when BOUND <= margin for every pair, i.e. u L (1.25 + 5.25 t) <= 1e-3.  With the factor of two kept
   between the bound and the margin:
        (max(image_h, image_w) - 1) * (1.25 + 5.25 t) <= 1e-3 / (2 u) = 8388.608                          (DET_LIMIT_K)
   t = 0.3: sides up to 2970;  0.5: 2165;  0.7: 1704;  1.0: 1291;  0.0: 6711.  launch_detections returns FRCNN_EUNSUPPORTED past it.

Measured (tests/test_detections_cpu.py::test_prefilter_mirror prints them): per threshold and image 10^6 near-threshold pairs (shifted and
nested boxes, sides from 2 % of the image to the whole side, half of them with every coordinate just short of a float32 rounding
boundary) plus the margin family.  Worst |lhs - E| / margin, and in brackets worst |lhs - E| / BOUND:
    t      600 x 1000      the limit (side)        2 x the limit     4 x the limit
    0.0    0.030 (0.41)    0.241 (0.48)  6711      0.482 (0.48)      0.965 (0.48)
    0.3    0.040 (0.24)    0.158 (0.32)  2970      0.317 (0.32)      0.639 (0.32)
    0.5    0.046 (0.20)    0.182 (0.36)  2165      0.364 (0.36)      0.727 (0.36)
    0.7    0.070 (0.24)    0.139 (0.28)  1704      0.284 (0.28)      0.563 (0.28)
No pair that float32 decides disagreed with float64 at any of these sizes: the search found no wrong decision at 2 x or 4 x the limit
either (the error grows linearly with the side, as derived, and reaches 0.96 of the margin at 4 x the limit for t = 0: the first wrong
decisions are to be expected from about 4 x to 8 x the limit, i.e. beyond 12000 px at the 0.3 threshold).  The bound is 2 to 4 times
what these searches reach; the limit keeps its factor of two on top of that.
"""
import math

import numpy as np

from tests import box_decisions_cases as B

F32 = np.float32
DET_THR = B.DET_THR
U = 2.0 ** -24
DET_LIMIT_K = 8388.608          # 1e-3 / (2 u): csrc/detect.hip's DET_LIMIT_K
MARGIN_THRESHOLDS = (0.0, 0.3, 0.5, 0.7)
SENTINEL = -7.5


def thr64(thr):
    """The NMS threshold as the kernel and the oracle see it: a C float, widened."""
    return float(F32(thr))


def image_limit(thr):
    """The largest image side launch_detections accepts at this threshold (the same double expression as csrc/detect.hip)."""
    c = 1.25 + 5.25 * thr64(thr)
    side = int(math.floor(DET_LIMIT_K / c)) + 1
    while (side - 1) * c > DET_LIMIT_K:
        side -= 1
    while side * c <= DET_LIMIT_K:
        side += 1
    return side


def make_case(props, classes, deltas, n, max_rois, ncls, image_h=600, image_w=1000, score_thr=0.05, nms_thr=DET_THR):
    props = np.ascontiguousarray(props, F32); classes = np.ascontiguousarray(classes, F32); deltas = np.ascontiguousarray(deltas, F32)
    assert props.shape == (max_rois, 4) and classes.shape == (max_rois, ncls) and deltas.shape == (max_rois, (ncls - 1) * 4)
    assert max_rois <= 512
    return (props, classes, deltas, int(n), int(max_rois), int(ncls), int(image_h), int(image_w), float(score_thr), float(nms_thr))


def decode_class(case, c):
    """(boxes float64 (k, 4), scores float32 (k,), proposal rows (k,)) of class c's candidates in the kernel's sorted order."""
    props, classes, deltas, n, max_rois, ncls, H, W, sthr, _ = case
    k = min(max(n, 0), max_rois)
    s = classes[:k, c]
    sel = np.where(s > F32(sthr))[0]
    boxes = B.det_decode(props[:k], H - 1.0, W - 1.0, deltas[:k, (c - 1) * 4:c * 4])[sel]
    order = np.argsort(-s[sel].astype(np.float64), kind="stable")
    return boxes[order], s[sel][order], sel[order]


def reference(case):
    """class -> rows (y1, x1, y2, x2, score) float64: O.detections at its fixed 0.3, else its own steps with O.nms at the case's threshold."""
    from oracle import frcnn_oracle as O
    props, classes, deltas, n, max_rois, ncls, H, W, sthr, nthr = case
    k = min(max(n, 0), max_rois)
    with np.errstate(over="ignore", invalid="ignore"):
        if nthr == DET_THR:
            return O.detections(props[:k], classes[:k], deltas[:k], H, W, sthr)
        out = {}
        for c in range(1, ncls):
            s = classes[:k, c]
            sel = np.where(s > F32(sthr))[0]
            boxes = B.det_decode(props[:k], H - 1.0, W - 1.0, deltas[:k, (c - 1) * 4:c * 4])[sel]
            keep = O.nms(boxes, s[sel], nthr)
            out[c] = np.hstack([boxes[keep], s[sel][keep][:, None].astype(np.float64)]) if keep.size else np.zeros((0, 5))
        return out


# ---- the pair expressions, vectorised ------------------------------------------------------------------------------------------------
def pair_mirror(A, Bx, thr):
    """csrc/detect.hip's float32 pair expressions on float64 boxes A, Bx (k, 4), operation for operation (no contraction), with the exact
    quantities next to them.  Returns a dict of arrays."""
    A = np.asarray(A, np.float64); Bx = np.asarray(Bx, np.float64)
    a = A.astype(F32); b = Bx.astype(F32)
    t32 = F32(thr); t = thr64(thr)
    oy = np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]); ox = np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1])
    inter = np.maximum(oy, F32(0)) * np.maximum(ox, F32(0))
    ha, wa, hb, wb = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    lhs = inter - t32 * (ha * wa + hb * wb - inter)
    margin = F32(1e-3) * (ha + wa + hb + wb + F32(1.0))
    assert lhs.dtype == F32 and margin.dtype == F32
    e0 = np.minimum(A[:, 2], Bx[:, 2]) - np.maximum(A[:, 0], Bx[:, 0]); e1 = np.minimum(A[:, 3], Bx[:, 3]) - np.maximum(A[:, 1], Bx[:, 1])
    it = np.maximum(e0, 0.0) * np.maximum(e1, 0.0)
    Ha, Wa, Hb, Wb = A[:, 2] - A[:, 0], A[:, 3] - A[:, 1], Bx[:, 2] - Bx[:, 0], Bx[:, 3] - Bx[:, 1]
    un = Ha * Wa + Hb * Wb - it
    with np.errstate(all="ignore"):
        dec64 = it / un > t
    zero = (Ha == 0) | (Wa == 0) | (Hb == 0) | (Wb == 0)
    never = (oy < F32(-1e-3)) | (ox < F32(-1e-3))
    up = (lhs > margin) & ~never & ~zero
    down = (lhs < -margin) & ~never & ~zero
    rhs = t * un
    band = ~zero & ~never & ~up & ~down & (it >= rhs * (1 - 1e-12)) & (it <= rhs * (1 + 1e-12))
    path = np.where(zero, "zero", np.where(never, "never", np.where(up | down, "fast", np.where(band, "band", "margin"))))
    dec = np.where(zero | never, False, np.where(up, True, np.where(down, False, dec64)))
    return {"lhs": lhs.astype(np.float64), "margin": margin.astype(np.float64), "E": it - t * un, "dec64": dec64, "dec": dec, "path": path,
            "oy": oy.astype(np.float64), "ox": ox.astype(np.float64), "e0": e0, "e1": e1, "s": Ha + Wa + Hb + Wb, "never": never,
            "zero": zero, "f32_decided": never | up | down}


def derived_bound(s, L, thr):
    """BOUND of the module docstring with its second-order terms, and the float64 rounding of the E it is measured against."""
    return U * L * s * (1.25 + 5.25 * thr64(thr)) + 20 * U * U * L * L + 1e-15 * L * L


def _exact_E(A, Bx, t):
    it = np.maximum(np.minimum(A[:, 2], Bx[:, 2]) - np.maximum(A[:, 0], Bx[:, 0]), 0) \
        * np.maximum(np.minimum(A[:, 3], Bx[:, 3]) - np.maximum(A[:, 1], Bx[:, 1]), 0)
    return it - t * ((A[:, 2] - A[:, 0]) * (A[:, 3] - A[:, 1]) + (Bx[:, 2] - Bx[:, 0]) * (Bx[:, 3] - Bx[:, 1]) - it)


def near_threshold_pairs(H, W, thr, k, seed, spread=3.0):
    """k float64 pairs inside [0, H-1] x [0, W-1] whose IoU is within a few margins of thr: shifted copies (along x, y or both) and nested
    boxes, sides log-uniform from 2 % of the image up to the whole side, then one coordinate of b moved so that E lands within +-spread margins."""
    rng = np.random.RandomState(seed)
    Lh, Lw = H - 1.0, W - 1.0
    t = thr64(thr)
    r = 2 * t / (1 + t)                                          # overlap / area of a shifted copy at IoU t
    kind = rng.randint(0, 4, k)
    p = rng.uniform(0, 1 - r, k)                                 # fraction of the height lost to the shift
    p = np.where(kind == 0, 0.0, np.where(kind == 1, 1 - r, p))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(kind == 1, 0.0, 1 - r / (1 - p))
    full = rng.rand(k) < 0.15                                    # a share of the pairs spans the whole image along one axis
    h = np.exp(rng.uniform(np.log(0.02), 0, k)) * Lh / (1 + p); w = np.exp(rng.uniform(np.log(0.02), 0, k)) * Lw / (1 + q)
    h = np.where(full & (kind != 1), Lh / (1 + p), h); w = np.where(full & (kind == 1), Lw / (1 + q), w)
    y = rng.uniform(0, 1, k) * (Lh - h * (1 + p)); x = rng.uniform(0, 1, k) * (Lw - w * (1 + q))
    far = rng.rand(k) < 0.5                                      # pushed against the far edge: the largest coordinates round the worst
    y = np.where(far, Lh - h * (1 + p), y); x = np.where(far, Lw - w * (1 + q), x)
    A = np.stack([y, x, y + h, x + w], axis=1)
    Bx = np.stack([y + p * h, x + q * w, y + p * h + h, x + q * w + w], axis=1)
    nest = kind == 3                                             # b inside a: area ratio t
    if t > 0:
        al = rng.uniform(t, 1, k)
        fy = rng.rand(k) * (1 - al); fx = rng.rand(k) * (1 - t / al)
        Bn = np.stack([A[:, 0] + fy * h, A[:, 1] + fx * w, A[:, 0] + (fy + al) * h, A[:, 1] + (fx + t / al) * w], axis=1)
        Bx = np.where(nest[:, None], Bn, Bx)
    # one coordinate of b that lies inside a (its top edge for the shift along y, its right edge for nested boxes, else its left edge)
    # moves so that E lands on a target within +-3 margins: one secant step (E is linear in that coordinate while it stays inside a)
    col = np.where(kind == 1, 0, np.where(nest & (t > 0), 3, 1))
    rows = np.arange(k)
    target = rng.uniform(-spread, spread, k) * 1e-3 * (2 * (h + w) + 1)
    if t == 0.0:
        target = np.abs(target)                                  # E = it >= 0 at threshold 0: a negative target would only separate the boxes
    step = np.where(col == 3, 1e-3, -1e-3) * np.where(col == 0, h, w)
    E0 = _exact_E(A, Bx, t)
    B1 = Bx.copy(); B1[rows, col] += step
    slope = (_exact_E(A, B1, t) - E0) / step
    ok = np.abs(slope) > 1e-6
    Bx[rows, col] += np.where(ok, (target - E0) / np.where(ok, slope, 1.0), 0.0)
    Bx[:, 0] = np.minimum(Bx[:, 0], Bx[:, 2]); Bx[:, 1] = np.minimum(Bx[:, 1], Bx[:, 3])
    A[:, 0::2] = np.clip(A[:, 0::2], 0, Lh); A[:, 1::2] = np.clip(A[:, 1::2], 0, Lw)
    Bx[:, 0::2] = np.clip(Bx[:, 0::2], 0, Lh); Bx[:, 1::2] = np.clip(Bx[:, 1::2], 0, Lw)
    # half of the pairs: every coordinate moved to just short of a float32 rounding boundary, on a random side, so that each of the eight
    # roundings costs nearly half an ulp
    adv = rng.rand(k) < 0.5
    for X, lim in ((A, (Lh, Lw)), (Bx, (Lh, Lw))):
        x32 = X.astype(F32)
        moved = x32.astype(np.float64) + rng.choice([-0.499, 0.499], X.shape) * np.spacing(x32).astype(np.float64)
        moved[:, 0::2] = np.clip(moved[:, 0::2], 0, lim[0]); moved[:, 1::2] = np.clip(moved[:, 1::2], 0, lim[1])
        X[adv] = moved[adv]
    return A, Bx


# ---- the greedy structure of a sorted class ----------------------------------------------------------------------------------------------
def nms_structure(boxes, thr):
    """(kept flags, over matrix) of float64 boxes in score order under the oracle's rule inter / (area_i + area_j - inter) > thr."""
    b = np.asarray(boxes, np.float64)
    n = b.shape[0]
    d0 = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0)
    d1 = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0)
    inter = d0 * d1
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(all="ignore"):
        over = inter / (area[:, None] + area[None, :] - inter) > thr64(thr)
    alive = np.ones(n, bool); kept = np.zeros(n, bool)
    for i in range(n):
        if alive[i]:
            kept[i] = True
            alive[i + 1:] &= ~over[i, i + 1:]
    return kept, over


# ---- sites: 512 well-separated 16 x 16 boxes on a 600 x 1000 image ------------------------------------------------------------------------
def site_boxes(rows, site=None, shift=None):
    """Row r's box sits on site[r] (default r) of a 16 x 32 grid of 36 x 30 px cells, moved right by shift[r] px (< 12: inside its cell)."""
    r = np.arange(rows)
    site = r if site is None else np.asarray(site)
    shift = np.zeros(rows) if shift is None else np.asarray(shift, np.float64)
    y = 2.0 + 36.0 * (site // 32); x = 2.0 + 30.0 * (site % 32) + shift
    return np.stack([y, x, y + 16.0, x + 16.0], axis=1).astype(F32)


def _one_class(props, scores, n=None, max_rois=None, **kw):
    rows = props.shape[0]
    classes = np.zeros((rows, 2), F32); classes[:, 0] = 0.01; classes[:, 1] = scores
    return make_case(props, classes, np.zeros((rows, 4), F32), rows if n is None else n, rows if max_rois is None else max_rois, 2, **kw)


WORD_EDGE_ROWS = (63, 64, 65, 127, 128, 447, 448, 511)


def words_family():
    scores = np.linspace(0.99, 0.06, 512).astype(F32)           # strictly descending: sorted rank == index
    out = []
    for name in ("patterns", "edges_mirrored", "all_kept"):
        site = np.arange(512); shift = np.zeros(512)
        if name == "patterns":
            for k in range(64):                                  # (e) word 4: every row on a kept row of word 0
                site[256 + k] = k
            for w in range(1, 8):                                # (a) row 0 suppresses a row of every later word
                site[64 * w + 5] = 0; shift[64 * w + 5] = 1
            for c in (1, 3, 6):                                  # (b) a kept row of word c suppresses in its own and in every later word
                site[64 * c + 20] = 64 * c + 10
                for w in range(c + 1, 8):
                    site[64 * w + 11 + c] = 64 * c + 10; shift[64 * w + 11 + c] = 2
            site[158] = 30; shift[158] = 5                       # (c) A = 30 -> B = 158 (IoU 0.52); B overlaps C = 350, A does not (0.23)
            site[350] = 30; shift[350] = 10
            for i, j in ((63, 64), (65, 127), (128, 447), (448, 511)):   # (d) i suppresses j
                site[j] = i
        elif name == "edges_mirrored":                           # (d) with the roles exchanged, and chains through the word edges
            for i, j in ((1, 63), (64, 65), (127, 128), (447, 448)):
                site[j] = i
            shift[448] = 5; site[511] = 447; shift[511] = 10     # 447 suppresses 448 (IoU 0.52); 511 overlaps 448 alone: kept
        props = site_boxes(512, site, shift)
        case = _one_class(props, scores)
        boxes, _, rows = decode_class(case, 1)
        kept, over = nms_structure(boxes, DET_THR)
        word = np.arange(512) // 64
        sup_by = [np.where(kept[:j] & over[:j, j])[0] for j in range(512)]
        facts = {"candidates": int(rows.shape[0]), "rank_is_index": bool(np.array_equal(rows, np.arange(512))),
                 "kept_per_word": [int(kept[word == w].sum()) for w in range(8)], "kept": int(kept.sum()),
                 "suppressors": sorted({int(i) for j in range(512) if not kept[j] for i in sup_by[j]}),
                 "suppressed": sorted(np.where(~kept)[0].tolist())}
        facts["a"] = [bool(any((not kept[j]) and (sup_by[j] < 64).any() for j in range(64 * w, 64 * w + 64))) for w in range(1, 8)]
        facts["b"] = {c: bool(any(kept[i] and all(any((not kept[j]) and i in sup_by[j] for j in range(64 * w, 64 * w + 64))
                                                  for w in range(c, 8)) for i in range(64 * c, 64 * c + 64))) for c in (1, 3, 6)}
        facts["c"] = bool(any(kept[a] and (not kept[b_]) and kept[c_] and over[a, b_] and over[b_, c_] and not over[a, c_]
                              for a in range(64) for b_ in np.where(over[a, 128:192])[0] + 128 for c_ in np.where(over[b_, 320:384])[0] + 320))
        facts["e"] = [w for w in range(1, 8) if not kept[word == w].any()
                      and all((sup_by[j] < 64 * w).all() for j in range(64 * w, 64 * w + 64))]
        out.append(("words_" + name, case, facts))
    return out


# ---- rank: the sort ------------------------------------------------------------------------------------------------------------------------
RANK_N = (1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512)
RANK_VARIANTS = ("permuted", "all_equal", "tie_runs", "every_third", "one_nan", "none", "last_only")


def rank_family():
    out = []
    props = site_boxes(512)
    for n in RANK_N:
        rng = np.random.RandomState(100 + n)
        ncls = len(RANK_VARIANTS) + 1
        classes = np.full((512, ncls), 0.999, F32)               # rows past n are bait: above the threshold in every class, never to be read
        classes[:, 0] = 0.01
        perm = lambda: rng.permutation(np.linspace(0.1, 0.95, n)).astype(F32)
        half = (n + 1) >> 1; h8 = (half + 7) & ~7
        s = {"permuted": perm(), "all_equal": np.full(n, 0.5, F32), "tie_runs": perm(), "every_third": perm(), "one_nan": perm(),
             "none": np.full(n, 0.01, F32), "last_only": np.full(n, 0.01, F32)}
        for v, centre in zip((0.97, 0.96, 0.955), (half, h8, 256)):
            s["tie_runs"][max(centre - 3, 0):min(centre + 3, n)] = v   # (an empty slice where the run lies past n)
        s["every_third"][np.arange(n) % 3 != 0] = 0.01
        s["one_nan"][n // 2] = np.nan
        s["last_only"][n - 1] = 0.7
        for k, v in enumerate(RANK_VARIANTS):
            classes[:n, k + 1] = s[v]
        case = make_case(props, classes, np.zeros((512, (ncls - 1) * 4), F32), n, 512, ncls)
        facts = {"order": {}}
        for k, v in enumerate(RANK_VARIANTS):
            sv = s[v]
            cand = np.where(sv > F32(0.05))[0]
            facts["order"][k + 1] = cand[np.argsort(-sv[cand], kind="stable")]
        out.append(("rank_n%d" % n, case, facts))
    return out


# ---- count: the contract -------------------------------------------------------------------------------------------------------------------
COUNT_MAX_ROIS = (1, 63, 64, 65, 300, 512)


def count_family():
    out = []
    for max_rois in COUNT_MAX_ROIS:
        rng = np.random.RandomState(200 + max_rois)
        site = np.arange(max_rois)
        site[3::4] -= 1                                          # every fourth row on its neighbour's site: suppressed where both are candidates
        props = site_boxes(max_rois, site)
        classes = np.zeros((max_rois, 4), F32); classes[:, 0] = 0.01
        classes[:, 1] = rng.permutation(np.linspace(0.1, 0.95, max_rois))
        classes[::2, 2] = rng.permutation(np.linspace(0.2, 0.9, (max_rois + 1) // 2))
        classes[:, 3] = 0.04                                     # class 3: nothing above the threshold, its zero count must still be written
        for n in (0, max_rois, max_rois + 7, 10 * max_rois):
            case = make_case(props, classes, np.zeros((max_rois, 12), F32), n, max_rois, 4)
            ref = reference(case)
            out.append(("count_max%d_n%d" % (max_rois, n), case, {"counts": [ref[c].shape[0] for c in (1, 2, 3)]}))
    return out


# ---- classes: the class stride -------------------------------------------------------------------------------------------------------------
CLASSES_NCLS = (2, 3, 21, 81, 128)
REFUSALS = ((64, 1), (64, 129), (0, 21), (513, 21))             # (max_rois, ncls): FRCNN_EINVAL


def classes_family():
    out = []
    for ncls in CLASSES_NCLS:
        rng = np.random.RandomState(300 + ncls)
        centre = np.stack([rng.uniform(80, 520, 16), rng.uniform(80, 920, 16)], axis=1)[np.arange(64) % 16] + rng.randn(64, 2) * 5
        hw = rng.uniform(30, 90, (64, 2))
        props = np.concatenate([centre - hw / 2, centre + hw / 2], axis=1).astype(F32)
        deltas = (rng.randn(64, (ncls - 1) * 4) * 0.5).astype(F32)   # different for every (row, class)
        classes = np.zeros((64, ncls), F32); classes[:, 0] = 0.01
        r = np.arange(64)
        for k in range(8):
            classes[r, (8 * r + k) % (ncls - 1) + 1] = rng.uniform(0.1, 0.9, 64).astype(F32)
        case = make_case(props, classes, deltas, 64, 64, ncls)
        per = [decode_class(case, c) for c in range(1, ncls)]
        boxes_of_row0 = np.stack([B.det_decode(props[:1], 599.0, 999.0, deltas[:1, (c - 1) * 4:c * 4])[0] for c in range(1, ncls)])
        facts = {"candidates": [p[2].shape[0] for p in per],
                 "distinct_boxes_of_a_row": int(np.unique(boxes_of_row0, axis=0).shape[0]),
                 "suppressed": int(sum(p[2].shape[0] - nms_structure(p[0], DET_THR)[0].sum() for p in per))}
        out.append(("classes_ncls%d" % ncls, case, facts))
    return out


# ---- decode: nonzero deltas ----------------------------------------------------------------------------------------------------------------
DECODE_VARIANTS = ("moderate", "overflow", "underflow", "pushed_out", "outside_props", "mixed")


def decode_family():
    rng = np.random.RandomState(400)
    rows = 64
    ncls = len(DECODE_VARIANTS) + 1
    centre = np.stack([rng.uniform(40, 560, rows), rng.uniform(40, 960, rows)], axis=1)
    hw = rng.uniform(12, 200, (rows, 2))                         # every proposal has a positive size (see the module docstring)
    props = np.concatenate([centre - hw / 2, centre + hw / 2], axis=1)
    props[0:6] += [-300, 0, -300, 0]; props[6:12] += [0, 700, 0, 700]           # (e) partly outside: above the top, past the right edge
    props[12] = [-80, -90, -10, -20]; props[13] = [650, 100, 700, 180]; props[14] = [100, 1005, 180, 1100]   # wholly outside
    props[15] = [-50, -50, 700, 1100]                                           # larger than the image
    props = props.astype(F32)
    d = {v: (rng.randn(rows, 4)).astype(F32) for v in DECODE_VARIANTS}
    big = np.asarray([4000.0, 3000.0, 1e30, 3.4e38], F32)        # * 0.2: exp -> inf, 3.8e260, inf, inf
    d["overflow"][0:16, 2] = big[np.arange(16) % 4]; d["overflow"][16:32, 3] = big[np.arange(16) % 4]; d["overflow"][32:40, 2:4] = 4000.0
    d["underflow"][0:16, 2] = -big[np.arange(16) % 4]; d["underflow"][16:32, 3] = -big[np.arange(16) % 4]; d["underflow"][32:40, 2:4] = -4000.0
    d["pushed_out"][0:16, 0] = 600.0; d["pushed_out"][16:32, 1] = -900.0        # both corners onto y = H - 1 / onto x = 0
    d["pushed_out"][32:40, 0] = -600.0; d["pushed_out"][40:48, 1] = 900.0       # ... onto y = 0 / onto x = W - 1
    d["pushed_out"][:, 2:4] *= 0.3
    d["outside_props"][:] = 0
    pick = rng.randint(0, 4, rows)
    for r in range(rows):
        d["mixed"][r] = d[DECODE_VARIANTS[pick[r]]][r]
    deltas = np.concatenate([d[v] for v in DECODE_VARIANTS], axis=1)
    classes = np.zeros((rows, ncls), F32); classes[:, 0] = 0.01
    classes[:, 1:] = rng.uniform(0.06, 0.99, (rows, ncls - 1))
    case = make_case(props, classes, deltas, rows, rows, ncls)
    facts = {}
    for k, v in enumerate(DECODE_VARIANTS):
        b = decode_class(case, k + 1)[0]
        h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        facts[v] = {"finite": bool(np.isfinite(b).all()), "whole_height": int(((b[:, 0] == 0) & (b[:, 2] == 599)).sum()),
                    "whole_width": int(((b[:, 1] == 0) & (b[:, 3] == 999)).sum()), "zero_area": int(((h == 0) | (w == 0)).sum()),
                    "zero_at_bottom": int(((b[:, 0] == 599) & (b[:, 2] == 599)).sum()), "zero_at_left": int(((b[:, 1] == 0) & (b[:, 3] == 0)).sum()),
                    "clipped": int(((b[:, 0] == 0) | (b[:, 3] == 999)).sum()), "kept": int(nms_structure(b, DET_THR)[0].sum()), "rows": int(b.shape[0])}
    return [("decode", case, facts)]


# ---- margin: the float32 pre-filter at the edge of its domain ------------------------------------------------------------------------------
MARGIN_KINDS = ("band", "fast_up", "fast_down", "margin_up", "margin_down", "f32_sign_differs", "never_fired", "gap_not_fired", "sliver")


def _band_pairs(H, W, thr):
    """Float32-representable pairs whose float64 IoU is the float32 threshold exactly (the division decides): nested boxes anchored on
    y = 0 or x = 0 whose sides are 2^p and thr * 2^p (thr has 24 bits: the product is a float32), touching boxes for thr 0."""
    t = thr64(thr)
    pairs = []
    for p in range(6, 13):
        side = float(2 ** p)
        if t == 0.0:
            if side + 40 <= W - 1 and side <= H - 1:
                pairs.append(([0, 8, side, 8 + 20], [0, 28, side, 48]))                 # touching along x
            if side + 40 <= H - 1 and side <= W - 1:
                pairs.append(([8, 0, 28, side], [28, 0, 48, side]))                     # touching along y
            continue
        if side <= H - 1:
            pairs.append(([0, 16, side, W - 1.0], [0, 16, t * side, W - 1.0]))           # nested in height, as wide as the image allows
        if side <= W - 1:
            pairs.append(([16, 0, H - 1.0, side], [16, 0, H - 1.0, t * side]))
    return pairs


def margin_case(H, W, thr, seed=0, per_kind=12):
    """One launch: pair p is rows (2p, 2p + 1) and the only candidates of class p + 1.  Returns (name, case, facts)."""
    t = thr64(thr)
    A, Bx = near_threshold_pairs(H, W, thr, 60000, seed + 17)
    A2, B2 = near_threshold_pairs(H, W, thr, 60000, seed + 18, spread=0.03)      # E within the float32 error: the signs can differ
    A = np.concatenate([A, A2]); Bx = np.concatenate([Bx, B2])
    rng = np.random.RandomState(seed + 5)
    # the `never` seam: b starts a few float32 ulps of the coordinate after / before a's far edge, near the image's far edge
    k = 400
    edge = rng.uniform(0.8, 0.97, k) * (H - 1)
    ulps = rng.choice([-40, -20, -8, -3, -1, 1, 3, 8, 20, 40], k)
    e32 = edge.astype(F32)
    b0 = B.nudge(e32, ulps).astype(np.float64)
    x0 = rng.uniform(0, 0.3, k) * (W - 1); w0 = rng.uniform(0.3, 0.69, k) * (W - 1)
    An = np.stack([edge * 0.2, x0, e32.astype(np.float64), x0 + w0], axis=1)
    Bn = np.stack([b0, x0, np.full(k, H - 1.0), x0 + w0], axis=1)
    A = np.concatenate([A, An]); Bx = np.concatenate([Bx, Bn])
    bp = _band_pairs(H, W, thr)
    if bp:
        A = np.concatenate([np.asarray([p[0] for p in bp], np.float64), A]); Bx = np.concatenate([np.asarray([p[1] for p in bp], np.float64), Bx])
    # what the kernel sees: float32 proposals, decoded
    pa = A.astype(F32); pb = Bx.astype(F32)
    Da = B.det_decode(pa, H - 1.0, W - 1.0); Db = B.det_decode(pb, H - 1.0, W - 1.0)
    m = pair_mirror(Da, Db, thr)
    ratio = np.abs(m["lhs"]) / m["margin"]
    gap = np.minimum(m["oy"], m["ox"])
    egap = np.minimum(m["e0"], m["e1"])
    kinds = {"band": m["path"] == "band",
             "fast_up": (m["path"] == "fast") & m["dec"] & (ratio < 1.6),
             "fast_down": (m["path"] == "fast") & ~m["dec"] & (ratio < 1.6) & (gap > 1.0),
             "margin_up": (m["path"] == "margin") & m["dec64"] & ((egap > 1.0) | (t == 0.0)),   # (thr 0: only slivers are this close)
             "margin_down": (m["path"] == "margin") & ~m["dec64"] & (egap > 1.0),
             # float32 alone would decide these wrongly: only the margin sends them to float64 (a hundredth of the margin would not)
             "f32_sign_differs": (m["path"] == "margin") & ((m["lhs"] > 0) != m["dec64"]) & (ratio > 0.02) & (egap > 1.0),
             "never_fired": m["never"] & ~m["zero"] & (gap > -0.05),
             "gap_not_fired": ~m["never"] & ~m["zero"] & (egap < 0) & (egap > -1e-3),
             "sliver": ~m["never"] & ~m["zero"] & (egap > 0) & (egap < 0.01)}
    sel, kind_of = [], []
    for kd in MARGIN_KINDS:
        idx = np.where(kinds[kd])[0]
        side = (Da[idx, 2] - Da[idx, 0]) + (Da[idx, 3] - Da[idx, 1])
        idx = idx[np.argsort(-side, kind="stable")][:per_kind]   # the largest boxes of each kind
        sel += idx.tolist(); kind_of += [kd] * idx.shape[0]
    sel = np.asarray(sel[:127], int); kind_of = kind_of[:127]
    npairs = sel.shape[0]
    ncls = npairs + 1
    rows = 2 * npairs
    props = np.empty((rows, 4), F32); props[0::2] = pa[sel]; props[1::2] = pb[sel]
    classes = np.zeros((rows, ncls), F32); classes[:, 0] = 0.01
    classes[2 * np.arange(npairs), np.arange(npairs) + 1] = 0.9
    classes[2 * np.arange(npairs) + 1, np.arange(npairs) + 1] = 0.8
    case = make_case(props, classes, np.zeros((rows, (ncls - 1) * 4), F32), rows, rows, ncls, H, W, 0.05, thr)
    facts = {"kinds": kind_of, "pairs": (Da[sel], Db[sel]), "suppressed": m["dec64"][sel], "path": m["path"][sel],
             "max_side_fraction": float(np.max([(Da[sel, 2] - Da[sel, 0]).max() / (H - 1), (Da[sel, 3] - Da[sel, 1]).max() / (W - 1)]))}
    return ("margin_%dx%d_thr%g" % (H, W, thr), case, facts)


def margin_images(thr):
    lim = image_limit(thr)
    return ((600, 1000), (lim, lim))


def margin_family():
    return [margin_case(H, W, thr) for thr in MARGIN_THRESHOLDS for (H, W) in margin_images(thr)]


FAMILIES = {"words": words_family, "rank": rank_family, "count": count_family, "classes": classes_family, "decode": decode_family,
            "margin": margin_family}
_cache = {}


def family(name):
    """The family's cases, built once per process and shared (read only)."""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def case_ids():
    return [(f, i) for f in FAMILIES for i in range(len(family(f)))]
