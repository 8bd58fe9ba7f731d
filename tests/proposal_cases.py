"""
Case tables and the exact reference for the proposal stage (csrc/proposals.hip: rpn_decode_kernel, topk_sort_kernel<0, true>,
topk_rank_kernel, topk_emit_kernel, then the NMS), one frcnn_rpn_proposals call per case.

The form those kernels take depends on three quantities, and each case sits on a chosen side of one of their seams:
  * A = 9 fh fw against 24576: the select keeps its keys in registers up to there and re-reads them from memory above;
  * A against 65535: five radix digits below, six from there on (the anchor index + 1 no longer fits 16 bits);
  * sort_n = pow2_at_least(pre_nms) and per = sort_n / 1024: the rank kernel's segment lengths and the emit kernel's branch.

Nothing here needs a tolerance.  The kernel returns its own scores, so selection and order follow from those bits and the anchor index.
The inputs are crafted (to the kernel the anchor map is (A, 4) floats (cy, cx, h, w) and the head (fh fw, ld) floats): the size deltas are
zero, so exp(0) == 1 and the decode is one correctly rounded float32 multiply, add and subtract per coordinate, which numpy float32
repeats bit for bit.  Logits come from a few levels: the pre_nms boundary falls inside a run of equal scores and the index digits decide.
The boxes sit on a grid of sites, a few overlapping ones per site, which keeps the CPU NMS cheap.

tests/test_proposals_cpu.py checks the reference against the oracle and that every case is what its name says;
tests/test_proposals_gpu.py runs the kernels on them.
"""
import functools

import numpy as np

from oracle import frcnn_oracle as O

F32 = np.float32
REG_KEYS = 24576            # topk_sort_kernel: 1024 threads x KPT = 24 keys stay in registers
SHORT_IDX_BELOW = 65535     # topk_sort_kernel: n_keys < 65535 -> five digits
IMAGE_H, IMAGE_W = 600, 1000


def pow2_at_least(v):
    p = 1024
    while p < v:
        p <<= 1
    return p


def sigmoid_f32(x):
    x = np.asarray(x, F32)
    return (F32(1) / (F32(1) + np.exp(-x))).astype(F32)


def below(x):
    return np.nextafter(F32(x), F32(0))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def reference(scores_f32, deltas, anchors, valid, image_h, image_w, pre_nms, post_nms, nms_thr, min_side):
    """
    The stage from its definition (reference models/rpn.py:98-153), float32 with one rounding per operation:
      1. order the valid anchors by (score, index), both descending -- what argsort(stable).flip() gives.  (-0.0 < +0.0 would be the one
         place where the score's value and its bits disagree; a sigmoid never returns -0.0, so it is not modelled);
      2. the first pre_nms;  3. decode;  4. clamp to the image;  5. keep rows with both clipped sides >= min_side, in order;
      6. O.nms(..., nms_thr)[:post_nms].
    """
    scores = np.asarray(scores_f32, F32).reshape(-1)
    deltas = np.asarray(deltas, F32).reshape(-1, 4)
    anchors = np.asarray(anchors, F32).reshape(-1, 4)
    a_n = scores.shape[0]
    idx = np.arange(a_n) if valid is None else np.flatnonzero(np.asarray(valid).reshape(-1) > 0)
    order = idx[np.lexsort((idx, scores[idx]))[::-1]]
    top = order[:pre_nms]
    a, d = anchors[top], deltas[top]
    cy = a[:, 2] * d[:, 0] + a[:, 0]
    cx = a[:, 3] * d[:, 1] + a[:, 1]
    h = a[:, 2] * np.exp(d[:, 2])
    w = a[:, 3] * np.exp(d[:, 3])
    hh, hw = F32(0.5) * h, F32(0.5) * w
    boxes = np.stack([cy - hh, cx - hw, cy + hh, cx + hw], axis=1)
    assert boxes.dtype == F32
    clipped = boxes.copy()
    clipped[:, 0:2] = np.maximum(clipped[:, 0:2], F32(0))
    clipped[:, 2] = np.minimum(clipped[:, 2], F32(image_h))
    clipped[:, 3] = np.minimum(clipped[:, 3], F32(image_w))
    side_h = clipped[:, 2] - clipped[:, 0]
    side_w = clipped[:, 3] - clipped[:, 1]
    keep = (side_h >= F32(min_side)) & (side_w >= F32(min_side))
    cand, cand_scores = clipped[keep], scores[top][keep]
    kept = O.nms(cand, cand_scores, nms_thr)[:post_nms]
    return {"sorted_idx": top.astype(np.int32), "n_selected": int(top.shape[0]), "n_after_filter": int(keep.sum()),
            "proposals": cand[kept], "sorted_scores": scores[top], "boxes": boxes, "clipped": clipped, "side_h": side_h,
            "side_w": side_w, "keep": keep}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
class Case:
    """One frcnn_rpn_proposals call.  `expect` names what tests/test_proposals_cpu.py asserts of the case (from the reference alone)."""

    def __init__(self, name, fh, fw, pre, post=300, levels=3, ld=128, min_side=16.0, present=None, kinds="mixed", score_plan="random",
                 thresholds=False, tol=False, seed=0, **expect):
        self.name, self.fh, self.fw, self.pre, self.post, self.levels, self.ld = name, fh, fw, pre, post, levels, ld
        self.min_side, self.present, self.kinds, self.score_plan, self.thresholds, self.tol = min_side, present, kinds, score_plan, thresholds, tol
        self.seed, self.expect = seed, expect
        self.a = 9 * fh * fw
        self.nms_thr = 0.7
        self.image_h, self.image_w = IMAGE_H, IMAGE_W
        self.sort_n = pow2_at_least(pre)
        self.per = self.sort_n >> 10

    def __repr__(self):
        return self.name

    @property
    def exact(self):
        return not self.tol

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        return _build(self)

    def head(self):
        """(fh fw, ld) float32: 9 logits, 36 deltas, and padding that a wrong row stride would read as data."""
        i = self.inputs()
        head = np.full((self.fh * self.fw, self.ld), 7.0, F32)
        head[:, 0:9] = i["logits"].reshape(-1, 9)
        head[:, 9:45] = i["deltas"].reshape(-1, 36)
        return head

    def reference(self, scores_f32):
        i = self.inputs()
        return reference(scores_f32, i["deltas"], i["anchors"], i["valid"], self.image_h, self.image_w, self.pre, self.post, self.nms_thr,
                         self.min_side)


def threshold_rows(m, image_h, image_w):
    """Boxes (y1, x1, y2, x2) at the filter's and the clip's thresholds, with their tag; the other side is a comfortable 2.5 m inside the
    image.  'eq': the clipped side is exactly m (kept).  'below': the nearest float32 below m (dropped).  'edge': the side reaches m only
    before the clip, once per image edge (dropped).  'outside': wholly outside the image (dropped)."""
    m = float(m)
    lo, hi = 64.0, 64.0 + 2.5 * m          # the comfortable side
    spans = [("eq", 0.0, m), ("eq", 64.0, 64.0 + m), ("eq", -5.0, m), ("below", 0.0, float(below(m))),
             ("edge", -0.5 * m, 0.5 * m), ("edge_far", None, None), ("outside", -3.0 * m, -m), ("outside_far", None, None)]
    rows = []
    for axis, size in ((0, image_h), (1, image_w)):
        for tag, p, q in spans:
            if tag == "edge_far":
                p, q = size - 0.5 * m, size + 0.5 * m
            elif tag == "outside_far":
                p, q = size + m, size + 3.0 * m
            box = [p, lo, q, hi] if axis == 0 else [lo, p, hi, q]
            rows.append((tag.split("_")[0], axis, box))
    return rows


def _build(c):
    rng = np.random.RandomState(1000 + c.seed)
    a_n, s = c.a, c.min_side / 16.0
    # ---- boxes: a grid of sites 48 s apart (the outer ones are cut by the image's edges), per anchor a site, a size and a centre delta
    ny, nx = int(c.image_h // (48 * s)) + 2, int(c.image_w // (48 * s)) + 2
    site = rng.randint(0, ny * nx, size=a_n)
    sizes = np.array([40.0, 40.0, 40.0] if c.tol else [32.0, 36.0, 40.0]) * s
    hw = sizes[rng.randint(0, 3, size=(a_n, 2))]
    if c.kinds == "mixed":
        small = rng.rand(a_n) < 0.3
    elif c.kinds == "parity":                      # (ranks inside a run of equal scores descend with the index: keep / drop alternate)
        small = (np.arange(a_n) & 1) == 1
    elif c.kinds == "all_small":
        small = np.ones(a_n, bool)
    else:
        raise ValueError(c.kinds)
    which = rng.randint(0, 3, size=a_n)            # the side(s) a small box fails on: h, w or both
    hw[small & (which != 1), 0] = 12.0 * s
    hw[small & (which != 0), 1] = 12.0 * s
    anchors = np.empty((a_n, 4), F32)
    anchors[:, 0] = (site // nx) * 48.0 * s
    anchors[:, 1] = (site % nx) * 48.0 * s
    anchors[:, 2:4] = hw
    deltas = np.zeros((a_n, 4), F32)
    jitter = 0.01 if c.tol else 0.05
    deltas[:, 0:2] = rng.uniform(-jitter, jitter, size=(a_n, 2))
    if c.tol:
        deltas[:, 2:4] = rng.uniform(-0.02, 0.02, size=(a_n, 2))
    # ---- logits from `levels` values
    if c.levels == 1:
        level = np.zeros(a_n, np.int64)
    else:
        level = rng.randint(0, c.levels, size=a_n)
    n_levels = c.levels
    if c.score_plan == "straddle":                 # the two upper levels only at index >= 60000, the rest all equal
        level = np.where(np.arange(a_n) >= 60000, rng.randint(1, 3, size=a_n), 0)
        n_levels = 3
    special = np.zeros(0, np.int64)
    tags = []
    if c.score_plan == "wave_of_drops":            # a level above all others for a little more than a wave's ranks, all failing boxes
        special = rng.choice(a_n, size=64 * c.per + 37, replace=False)
        level[special] = n_levels
        n_levels += 1
        anchors[special, 2] = 12.0 * s
    if c.thresholds:
        rows = threshold_rows(c.min_side, c.image_h, c.image_w)
        special = rng.choice(a_n, size=len(rows), replace=False)
        level[special] = n_levels
        n_levels += 1
        for i, (tag, axis, box) in zip(special, rows):
            y1, x1, y2, x2 = (F32(v) for v in box)
            anchors[i] = [F32(0.5) * (y1 + y2), F32(0.5) * (x1 + x2), y2 - y1, x2 - x1]
            deltas[i] = 0
            tags.append((tag, axis))
    logits = (F32(-3.0) + F32(6.0) * level.astype(F32) / F32(max(n_levels - 1, 1))).astype(F32)
    if c.levels == 1 and n_levels == 1:
        logits[:] = F32(0.5)
    valid = None
    if c.present is not None:
        valid = np.zeros(a_n, F32)
        valid[rng.choice(a_n, size=c.present, replace=False)] = 1.0
    return {"logits": logits, "deltas": deltas, "anchors": anchors, "valid": valid, "site": site, "special": special, "tags": tags}


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
A24570 = (42, 65)           # the largest A that stays in registers
A24579 = (1, 2731)          # the smallest streamed one
A37800 = (50, 84)           # an 800 x 1333 image: the streamed path's production shape
A65529 = (9, 809)           # five digits
A65538 = (22, 331)          # six digits: indices 65535 .. 65537 have bit 16 of index + 1 set


def _cases():
    cs = []
    # residency: either side of 24576 and the production shape; pre_nms 6000 inside a run of ties, and pre_nms above what is present
    for tag, shape, side in (("regs", A24570, "regs"), ("streamed", A24579, "streamed"), ("streamed_800x1333", A37800, "streamed")):
        cs.append(Case("residency_%s_pre6000" % tag, *shape, 6000, seed=len(cs), residency=side, tie=True))
        cs.append(Case("residency_%s_pre6000_present4000" % tag, *shape, 6000, present=4000, seed=len(cs), residency=side))
    # digit layout: either side of 65535, three levels and all equal, and winners on both sides of index 65536 in mid-list
    for tag, shape, digits in (("five", A65529, 5), ("six", A65538, 6)):
        cs.append(Case("digits_%s_3_levels" % tag, *shape, 6000, seed=len(cs), digits=digits, tie=True))
        cs.append(Case("digits_%s_all_equal" % tag, *shape, 6000, levels=1, seed=len(cs), digits=digits, tie=True, all_equal=True))
    cs.append(Case("digits_six_straddle_65536", *A65538, 6000, score_plan="straddle", seed=len(cs), digits=6, tie=True, straddle=True))
    # small A, either side of the block's 1024 threads; the head's row stride at its minimum, 48 and 128
    cs.append(Case("small_a9_ld45", 1, 1, 6000, ld=45, seed=len(cs)))
    cs.append(Case("small_a1017_ld48", 1, 113, 300, levels=17, ld=48, seed=len(cs), tie=True))
    cs.append(Case("small_a1026_ld45", 1, 114, 1025, levels=17, ld=45, seed=len(cs)))
    # pre_nms against sort_n and per, A = 24570.  ~1000 levels below 1024 (the boundary still falls inside a run of ~25), 3 or 17 above.
    # Four of them give the first wave of the emit kernel nothing to keep and alternate keep / drop behind it: one level above an
    # all-equal rest, whose ranks descend with the index
    for pre in (1, 31, 32, 33, 1024, 1025, 2048, 3000, 4096, 4097, 8192, 8193, 12000, 16384):
        wave = pre in (2048, 4096, 8192, 12000)
        cs.append(Case("pre%d%s" % (pre, "_wave_of_drops" if wave else ""), *A24570, pre,
                       levels=1000 if pre <= 1025 else 1 if wave else 17 if pre == 3000 else 3, kinds="parity" if wave else "mixed",
                       score_plan="wave_of_drops" if wave else "random", seed=len(cs), tie=pre > 1, wave=wave))
    # present against K through the valid map, A = 1026
    for present in (0, 1, 499, 500, 501):
        cs.append(Case("present%d_pre500" % present, 1, 114, 500, levels=17, present=present, seed=len(cs), tie=present == 501))
    # the filter's and the clip's thresholds, at two values of min_side
    cs.append(Case("thresholds_min_side16", *A24570, 6000, thresholds=True, seed=len(cs), tie=True))
    cs.append(Case("thresholds_min_side100", *A24570, 6000, min_side=100.0, thresholds=True, seed=len(cs), tie=True))
    # compaction with nothing to keep at all
    cs.append(Case("all_filtered", *A24570, 6000, kinds="all_small", seed=len(cs), tie=True, all_filtered=True))
    # non-zero size deltas: the expf path on the new shapes, at the 1e-3 px of test_rpn_proposals_vs_oracle
    cs.append(Case("tolerance_regs", *A24570, 6000, tol=True, seed=len(cs), residency="regs", tie=True))
    cs.append(Case("tolerance_streamed", *A37800, 6000, tol=True, seed=len(cs), residency="streamed", tie=True))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
EXACT = [c for c in CASES if c.exact]
TOLERANCE = [c for c in CASES if c.tol]

# frcnn_nms (MODE 1 of topk_sort_kernel): the generic LDS bitonic sort at sort_n 2048 / 4096 and the generic emit loop with per 2 / 4
NMS_SORT_SIZES = (1025, 2047, 2048, 2049, 4095, 4096, 4097)


def nms_sort_case(n):
    """Clustered boxes with quantised scores: many exact ties, so the stable order (lower index first) matters."""
    rng = np.random.RandomState(n)
    centers = rng.rand(40, 2) * np.array([560, 960]) + 20
    c = centers[rng.randint(0, 40, size=n)] + rng.randn(n, 2) * 6
    hw = np.abs(rng.randn(n, 2)) * 30 + 30 + rng.rand(n, 2) * 3
    boxes = np.concatenate([c - hw / 2, c + hw / 2], axis=1).astype(F32)
    scores = (np.round(rng.rand(n) * 50) / 50).astype(F32)
    return boxes, scores
