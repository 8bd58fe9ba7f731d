"""The contract of fasterrcnn_amd.ops.soft_nms (include/frcnn_hip.h) as a plain numpy loop, and the inputs its tests share.

reference(...) runs the loop in float32 -- every operation rounded on its own, as the kernel does, so naive and linear agree with it bit
for bit -- or in float64, the truth the gaussian scores are measured against.  Per run it reports the output order, the final scores, the
pick order of every problem, and three margins that say how far the run is from a decision a rounding error could flip:
    gap         the smallest relative gap between the best and the second-best live score over all picks,
    margin      the smallest relative distance of any rescored live value from min_score,
    thr_margin  the smallest |ovr - thr| over the overlaps the run computed (what naive and linear decide on).
A case is compared against float64 only if its float64 gap and margin are at least MARGIN = 1e-5, about 40 times the float32 error of the
scores (2.7e-7 of the largest score, measured on the clustered cases); qualifying() walks seeds upward until one does, in at most 8 tries.

Inputs: clustered boxes (about N / 12 clusters in a 600-px frame, centres jittered by a few pixels, sides 30-120 px, scores uniform in
[0.02, 1)), the special cases (identical boxes, exact ties, NaN scores, zero-area boxes, inverted boxes) and the labelled case."""
import functools

import numpy as np

THR, SIGMA, MIN_SCORE = 0.3, 0.5, 0.05
METHODS = {"naive": 0, "linear": 1, "gaussian": 2}
MARGIN = 1e-5
MAX_TRIES = 8
TINY = 1e-300


def _problem(boxes, scores, thr, sigma, low, method, offset, dt):
    """One problem: (pick order as positions, final working scores, gap, margin, thr_margin)."""
    b = boxes.astype(dt)
    s = scores.astype(dt).copy()
    thr, sigma, low, off = dt(np.float32(thr)), dt(np.float32(sigma)), dt(np.float32(low)), dt(offset)
    x1, y1, x2, y2 = (np.ascontiguousarray(b[:, c]) for c in range(4))
    area = (x2 - x1 + off) * (y2 - y1 + off)
    live = np.ones((b.shape[0],), dtype=bool)
    picks, gap, margin, thr_margin = [], np.inf, np.inf, np.inf
    code = METHODS[method]
    with np.errstate(all="ignore"):
        while live.any():
            number = live & ~np.isnan(s)
            if number.any():
                vals = s[number]
                best = vals.max()
                i = int(np.flatnonzero(number & (s == best))[0])            # ties to the smaller index; -0 == +0
                if vals.size > 1:
                    second = np.partition(vals, -2)[-2]
                    g = (float(best) - float(second)) / max(abs(float(best)), TINY)
                    gap = min(gap, g if np.isfinite(g) else 0.0)
            else:
                i = int(np.flatnonzero(live)[0])                              # NaN scores only: in index order
            live[i] = False
            picks.append(i)
            w = np.fmax(0, np.fmin(x2[i], x2) - np.fmax(x1[i], x1) + off)
            h = np.fmax(0, np.fmin(y2[i], y2) - np.fmax(y1[i], y1) + off)
            inter = w * h
            ovr = inter / ((area[i] + area) - inter)
            ovr[np.isnan(ovr)] = 0
            if code == 2:
                weight = np.exp(-(ovr * ovr) / sigma)
            elif code == 1:
                weight = np.where(ovr >= thr, 1 - ovr, dt(1))
            else:
                weight = np.where(ovr >= thr, dt(0), dt(1))
            s = np.where(live, s * weight, s).astype(dt)
            if live.any():
                v = s[live].astype(np.float64)
                d = np.abs(v - float(low)) / np.maximum(np.maximum(np.abs(v), abs(float(low))), TINY)
                d = d[np.isfinite(d)]
                if d.size:
                    margin = min(margin, float(d.min()))
                t = np.abs(ovr[live].astype(np.float64) - float(thr))
                t = t[np.isfinite(t)]
                if t.size:
                    thr_margin = min(thr_margin, float(t.min()))
            live &= ~(s < low)
    return np.asarray(picks, dtype=np.int64), s, gap, margin, thr_margin


def output_order(inds, scores):
    """inds sorted by (descending score, ascending index, NaN last); scores: the final score of each of inds."""
    key = sorted(range(len(inds)), key=lambda k: (bool(np.isnan(scores[k])), 0.0 if np.isnan(scores[k]) else -float(scores[k]),
                                                  int(inds[k])))
    return np.asarray(key, dtype=np.int64)


def reference(boxes, scores, thr=THR, sigma=SIGMA, min_score=MIN_SCORE, method="linear", offset=0, labels=None, dtype=np.float32):
    """The contract on numpy arrays.  Returns a dict: inds int64 [K] and scores [K] (the output), picks (one array of box indices per
    problem, in pick order, problems by ascending label), gap, margin, thr_margin, kept (the fraction of boxes kept)."""
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    n = boxes.shape[0]
    if labels is None:
        problems = [np.arange(n, dtype=np.int64)] if n else []
    else:
        labels = np.asarray(labels).astype(np.int64)
        problems = [np.flatnonzero(labels == v) for v in np.unique(labels)]
    final = scores.astype(dtype).copy()
    picks, gap, margin, thr_margin = [], np.inf, np.inf, np.inf
    for rows in problems:
        p, s, g, m, t = _problem(boxes[rows], scores[rows], thr, sigma, min_score, method, offset, dtype)
        final[rows] = s
        picks.append(rows[p])
        gap, margin, thr_margin = min(gap, g), min(margin, m), min(thr_margin, t)
    kept = np.concatenate(picks) if picks else np.zeros((0,), dtype=np.int64)
    kept = np.sort(kept)
    kept = kept[output_order(kept, final[kept])]
    return {"inds": kept, "scores": final[kept], "picks": picks, "gap": gap, "margin": margin, "thr_margin": thr_margin,
            "kept": kept.size / max(n, 1)}


def merged(parts):
    """Per-problem results [(inds, scores)] merged by (descending score, ascending index, NaN last): (inds, scores)."""
    inds = np.concatenate([p[0] for p in parts])
    scores = np.concatenate([p[1] for p in parts])
    by_index = np.argsort(inds, kind="stable")
    inds, scores = inds[by_index], scores[by_index]
    o = output_order(inds, scores)
    return inds[o], scores[o]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def clustered(n, seed, clusters=None):
    """(boxes float32 [n, 4], scores float32 [n]): about n / 12 clusters (or `clusters`) in a 600-px frame."""
    rng = np.random.RandomState(1000 * seed + 17)
    k = clusters or max(1, int(round(n / 12.0)))
    centres = rng.uniform(70.0, 530.0, (k, 2))
    sides = rng.uniform(30.0, 120.0, (k, 2))
    c = rng.randint(0, k, n)
    ctr = centres[c] + rng.uniform(-5.0, 5.0, (n, 2))
    sd = sides[c] * rng.uniform(0.85, 1.15, (n, 2))
    boxes = np.concatenate([ctr - sd / 2, ctr + sd / 2], axis=1).astype(np.float32)
    scores = rng.uniform(0.02, 1.0, n).astype(np.float32)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def qualifying(n, method, offset=0, thr=THR, sigma=SIGMA, min_score=MIN_SCORE, first_seed=0):
    """The first clustered case from first_seed upward whose float64 run has gap and margin >= MARGIN.  Returns (boxes, scores, the
    float64 reference, the seed); asserts that it takes at most MAX_TRIES seeds."""
    for seed in range(first_seed, first_seed + MAX_TRIES):
        boxes, scores = clustered(n, seed)
        truth = reference(boxes, scores, thr, sigma, min_score, method, offset, dtype=np.float64)
        if truth["gap"] >= MARGIN and truth["margin"] >= MARGIN:
            return boxes, scores, truth, seed
    raise AssertionError("no clustered case of %d boxes (%s) within %d seeds has margins >= %g" % (n, method, MAX_TRIES, MARGIN))


@functools.lru_cache(maxsize=None)
def single(n, method, offset=0, thr=THR, sigma=SIGMA, min_score=MIN_SCORE, seed=0):
    """(boxes, scores, the float32 reference) of the clustered case (n, seed)."""
    boxes, scores = clustered(n, seed)
    return boxes, scores, reference(boxes, scores, thr, sigma, min_score, method, offset)


def pair_iou_margin(boxes, thr):
    """The smallest |IoU - float32(thr)| over all pairs, in float64 (offset 0)."""
    b = boxes.astype(np.float64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    iou = inter / (area[:, None] + area[None, :] - inter)
    return float(np.abs(iou - float(np.float32(thr))).min())


@functools.lru_cache(maxsize=None)
def nms_case(n, thr):
    """The first clustered case whose pairwise float64 IoUs all lie at least MARGIN from thr: (boxes, scores)."""
    for seed in range(MAX_TRIES):
        boxes, scores = clustered(n, 50 + seed)
        if pair_iou_margin(boxes, thr) >= MARGIN and np.unique(scores).size == n:
            return boxes, scores
    raise AssertionError("no clustered case of %d boxes keeps its IoUs %g away from %g" % (n, MARGIN, thr))


SPECIALS = ("identical", "ties", "nan_scores", "zero_area", "inverted")
SPECIAL_SIZES = (48, 150)                                                  # one wave; the whole block


@functools.lru_cache(maxsize=None)
def special(name, n):
    """(boxes, scores, offset) of a special case: the reference mirrors the contract on all of them."""
    boxes, scores = clustered(n, 90)
    boxes, scores = boxes.copy(), scores.copy()
    rng = np.random.RandomState(n)
    if name == "identical":
        boxes[:] = np.float32([10.0, 20.0, 50.0, 80.0])
        scores[::3] = np.float32(0.5)                                       # and a third of them tie
    elif name == "ties":
        scores = (np.round(scores * 8) / 8 + 0.125).astype(np.float32)     # eight distinct values
    elif name == "nan_scores":
        scores[rng.permutation(n)[:n // 6]] = np.nan
    elif name == "zero_area":
        pts = rng.randint(0, 6, (n, 2)).astype(np.float32) * 10            # many coincide: inter = area = 0, ovr = 0 / 0
        boxes = np.concatenate([pts, pts], axis=1)
        boxes[::4, 2:] += 15.0                                              # and some proper boxes around them
    elif name == "inverted":
        rows = rng.permutation(n)[:n // 4]
        boxes[rows] = boxes[rows][:, [2, 3, 0, 1]]                          # x1 > x2 and y1 > y2: negative sides, positive area
        boxes[rows[::2], 1], boxes[rows[::2], 3] = boxes[rows[::2], 3].copy(), boxes[rows[::2], 1].copy()   # x inverted only: negative area
    else:
        raise KeyError(name)
    return boxes, scores, 0


@functools.lru_cache(maxsize=None)
def labelled(small=False):
    """300 labels with 1 to 40 boxes each, shuffled; label values negative, huge and non-contiguous (within int32 when small).
    Returns (boxes, scores, labels int64)."""
    rng = np.random.RandomState(7)
    counts = rng.randint(1, 41, 300)
    if small:
        values = rng.choice(np.arange(-2 ** 31, 2 ** 31 - 1, 7919, dtype=np.int64), 300, replace=False)
    else:
        values = np.concatenate([rng.randint(-2 ** 62, 2 ** 62, 296, dtype=np.int64),
                                 np.asarray([-2 ** 63, 2 ** 63 - 1, -1, 5], dtype=np.int64)])
        assert np.unique(values).size == 300
    labels = np.repeat(values, counts)
    n = labels.size
    boxes, scores = clustered(n, 33, clusters=12)                           # a label's 1 to 40 boxes fall into 12 clusters: they do meet
    perm = rng.permutation(n)
    return boxes, scores, labels[perm]
