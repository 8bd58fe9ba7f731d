"""
numpy restatements of torchvision.ops.ps_roi_align and ps_roi_pool (R-FCN's position-sensitive pooling), the truth that
fasterrcnn_amd.ops.ps_roi_align / ps_roi_pool (csrc/ops_ps.hip) are held to, and the RoI sets their tests share.  No GPU.

Restated from the published algorithm of torchvision's ps_roi_align_kernel.cu / ps_roi_pool_kernel.cu (third party, absent here:
restated, unpinned, like the oracle's nms / roi_align).  float32 arithmetic in the kernels' order of operations; N images, oh x ow bins.
Output channel c of bin (ph, pw) reads input channel (c * oh + ph) * ow + pw; a batch index outside (-1, N) pools to zeros.

ps_roi_align: start / end = coord * scale - 0.5, size = end - start (no clamp), bin = size / out, grid = sampling_ratio if > 0 else
  ceil(size / out), count = grid_h * grid_w (NO max(., 1)); sample (iy outer, ix inner) at start + p * bin + (i + .5) * bin / grid;
  roi_align's bilinear_interpolate; out = sum / count.  With an adaptive grid on a RoI of no height or width the loops do not run and
  the output is float32(0) / count: NaN for count == 0, -0.0 for count < 0.
ps_roi_pool: start = roundf(coord * scale), end = roundf((coord + 1) * scale) (C roundf: half away from zero), integer size
  max(end - start, 1), bin = float(size) / out, window [floor(p * bin), ceil((p + 1) * bin)) + start with each of the four bounds
  clamped to [0, size_of_map - 1]; the (h, w) scan-order sum of the window over its area, 0 for an empty window.
"""
import numpy as np

F = np.float32


def c_round(v):
    """C roundf: half away from zero."""
    return int(np.floor(v + F(0.5))) if v >= 0 else int(np.ceil(v - F(0.5)))


def image_of(roi, n_img):
    """The RoI's image, None for a batch index outside (-1, N) (truncated as torchvision truncates it)."""
    return int(roi[0]) if -1 < roi[0] < n_img else None


def _axis(v, n):
    """One coordinate of bilinear_interpolate: (low, high, weight of low, weight of high), None when the sample contributes nothing."""
    if v < F(-1.0) or v > F(n):
        return None
    v = max(v, F(0.0))
    lo = int(v)
    if lo >= n - 1:
        return n - 1, n - 1, F(1.0), F(0.0)
    hi_w = v - F(lo)
    return lo, lo + 1, F(1.0) - hi_w, hi_w


def align_plan(h, w, roi_xyxy, oh, ow, scale, sr):
    """ps_roi_align's sampling plan of one RoI: (grid_h, grid_w, count, {(ph, pw): [(yl, xl, yh, xh, w1, w2, w3, w4)]}), count the raw
    grid_h * grid_w."""
    scale = F(scale)
    x1, y1, x2, y2 = (F(v) for v in roi_xyxy)
    start_w, start_h = x1 * scale - F(0.5), y1 * scale - F(0.5)
    end_w, end_h = x2 * scale - F(0.5), y2 * scale - F(0.5)
    roi_w, roi_h = end_w - start_w, end_h - start_h
    bin_h, bin_w = roi_h / F(oh), roi_w / F(ow)
    gh = int(sr) if sr > 0 else int(np.ceil(roi_h / F(oh)))
    gw = int(sr) if sr > 0 else int(np.ceil(roi_w / F(ow)))
    plan = {}
    for ph in range(oh):
        ys = [_axis(start_h + F(ph) * bin_h + (F(iy) + F(0.5)) * bin_h / F(gh), h) for iy in range(gh)]
        for pw in range(ow):
            xs = [_axis(start_w + F(pw) * bin_w + (F(ix) + F(0.5)) * bin_w / F(gw), w) for ix in range(gw)]
            s = []
            for ya in ys:
                for xa in xs:
                    if ya is None or xa is None:
                        continue
                    yl, yh, hy, ly = ya
                    xl, xh, hx, lx = xa
                    s.append((yl, xl, yh, xh, hy * hx, hy * lx, ly * hx, ly * lx))
            plan[ph, pw] = s
    return gh, gw, gh * gw, plan


def scaled_size(roi_xyxy, scale):
    """(roi_w, roi_h) of ps_roi_align in float32."""
    scale = F(scale)
    x1, y1, x2, y2 = (F(v) for v in roi_xyxy)
    return (x2 * scale - F(0.5)) - (x1 * scale - F(0.5)), (y2 * scale - F(0.5)) - (y1 * scale - F(0.5))


def nondegenerate(rois, scale):
    """The RoIs with roi_w > 0 and roi_h > 0 after scaling: those on which ps_roi_align is roi_align(aligned=True) on the diagonal."""
    return np.array([all(v > 0 for v in scaled_size(r[1:], scale)) for r in rois], bool)


def ps_roi_align(x, rois, oh, ow, scale, sr):
    """float32 ps_roi_align of x [N, C, H, W] and rois [K, 5] -> [K, C / (oh ow), oh, ow]."""
    n, c, h, w = x.shape
    co = c // (oh * ow)
    out = np.zeros((rois.shape[0], co, oh, ow), F)
    planes = np.arange(co)[:, None, None] * (oh * ow) + np.arange(oh * ow).reshape(oh, ow)[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(rois.shape[0]):
            b = image_of(rois[r], n)
            if b is None:
                continue
            _, _, count, plan = align_plan(h, w, rois[r, 1:], oh, ow, scale, sr)
            for (ph, pw), samples in plan.items():
                fm = x[b, planes[:, ph, pw]]
                acc = np.zeros((co,), F)
                for (yl, xl, yh, xh, w1, w2, w3, w4) in samples:
                    acc = acc + (w1 * fm[:, yl, xl] + w2 * fm[:, yl, xh] + w3 * fm[:, yh, xl] + w4 * fm[:, yh, xh])
                out[r, :, ph, pw] = acc / F(count)
    return out


def ps_roi_align_backward(g, shape, rois, oh, ow, scale, sr):
    """float64 accumulation of the same plan: every corner of every sample receives grad * w / count; a RoI whose loops do not run
    (grid <= 0) sends nothing."""
    n, c, h, w = shape
    co = c // (oh * ow)
    d = np.zeros(shape, np.float64)
    g = g.astype(np.float64)
    for r in range(rois.shape[0]):
        b = image_of(rois[r], n)
        if b is None:
            continue
        gh, gw, count, plan = align_plan(h, w, rois[r, 1:], oh, ow, scale, sr)
        if gh <= 0 or gw <= 0:
            continue
        for (ph, pw), samples in plan.items():
            ci = (np.arange(co) * oh + ph) * ow + pw
            gb = g[r, :, ph, pw] / count
            for (yl, xl, yh, xh, w1, w2, w3, w4) in samples:
                d[b, ci, yl, xl] += float(w1) * gb
                d[b, ci, yl, xh] += float(w2) * gb
                d[b, ci, yh, xl] += float(w3) * gb
                d[b, ci, yh, xh] += float(w4) * gb
    return d


def pool_windows(h, w, roi_xyxy, oh, ow, scale):
    """ps_roi_pool's windows of one RoI: {(ph, pw): (hstart, hend, wstart, wend)}, already clamped to [0, H - 1] / [0, W - 1]."""
    scale = F(scale)
    x1, y1, x2, y2 = (F(v) for v in roi_xyxy)
    rs_w, rs_h = c_round(x1 * scale), c_round(y1 * scale)
    re_w, re_h = c_round((x2 + F(1.0)) * scale), c_round((y2 + F(1.0)) * scale)
    bin_h = F(max(re_h - rs_h, 1)) / F(oh)
    bin_w = F(max(re_w - rs_w, 1)) / F(ow)
    win = {}
    for ph in range(oh):
        hs = min(max(int(np.floor(F(ph) * bin_h)) + rs_h, 0), h - 1)
        he = min(max(int(np.ceil(F(ph + 1) * bin_h)) + rs_h, 0), h - 1)
        for pw in range(ow):
            ws = min(max(int(np.floor(F(pw) * bin_w)) + rs_w, 0), w - 1)
            we = min(max(int(np.ceil(F(pw + 1) * bin_w)) + rs_w, 0), w - 1)
            win[ph, pw] = (hs, he, ws, we)
    return win


def ps_roi_pool(x, rois, oh, ow, scale, dtype=F):
    """ps_roi_pool of x [N, C, H, W]: dtype float32 is torchvision's scan-order (h outer, w inner) float32 sum over the float32 area;
    float64 accumulates the same windows in float64."""
    n, c, h, w = x.shape
    co = c // (oh * ow)
    out = np.zeros((rois.shape[0], co, oh, ow), dtype)
    for r in range(rois.shape[0]):
        b = image_of(rois[r], n)
        if b is None:
            continue
        for (ph, pw), (hs, he, ws, we) in pool_windows(h, w, rois[r, 1:], oh, ow, scale).items():
            if he <= hs or we <= ws:
                continue
            ci = (np.arange(co) * oh + ph) * ow + pw
            acc = np.zeros((co,), dtype)
            for yy in range(hs, he):
                for xx in range(ws, we):
                    acc = acc + x[b, ci, yy, xx].astype(dtype)
            out[r, :, ph, pw] = acc / dtype((he - hs) * (we - ws))
    return out


def ps_roi_pool_backward(g, shape, rois, oh, ow, scale):
    """float64: every cell of a non-empty window receives grad / area."""
    n, c, h, w = shape
    co = c // (oh * ow)
    d = np.zeros(shape, np.float64)
    g = g.astype(np.float64)
    for r in range(rois.shape[0]):
        b = image_of(rois[r], n)
        if b is None:
            continue
        for (ph, pw), (hs, he, ws, we) in pool_windows(h, w, rois[r, 1:], oh, ow, scale).items():
            if he <= hs or we <= ws:
                continue
            ci = (np.arange(co) * oh + ph) * ow + pw
            d[b, ci, hs:he, ws:we] += (g[r, :, ph, pw] / ((he - hs) * (we - ws)))[:, None, None]
    return d


# The deliberately degenerate RoIs of make_rois (image coordinates in units of the map's extent W = w / scale, H = h / scale):
# zero width, zero height, zero both, inverted along x, and one wholly outside the map.
N_DEGENERATE = 4


def make_rois(rng, k, n_img, h, w, scale):
    """[K, 5] float32, K >= 48: batch indices in arbitrary order; boxes inside, across and wholly outside the map; one batch index out
    of range on either side; N_DEGENERATE RoIs without width or height after scaling (at most 10 % of the RoIs for K >= 40)."""
    assert k >= 10 * N_DEGENERATE
    H, W = h / scale, w / scale
    x1 = rng.uniform(-0.2 * W, 0.9 * W, k); y1 = rng.uniform(-0.2 * H, 0.9 * H, k)
    rois = np.stack([rng.randint(0, n_img, k), x1, y1, x1 + rng.uniform(1, 0.8 * W, k), y1 + rng.uniform(1, 0.8 * H, k)], 1)
    special = [[0, 0.25 * W, 0.2 * H, 0.25 * W, 0.7 * H],                 # zero width
               [n_img - 1, 0.1 * W, 0.5 * H, 0.6 * W, 0.5 * H],           # zero height
               [0, 0.5 * W, 0.5 * H, 0.5 * W, 0.5 * H],                   # a point
               [n_img - 1, 0.6 * W, 0.2 * H, 0.3 * W, 0.8 * H],           # inverted along x
               [0, 0, 0, W, H],                                           # the whole map
               [0, -3 * W, -2 * H, -W, -H],                               # wholly outside
               [n_img, 0, 0, W / 2, H / 2], [-1, 0, 0, W / 2, H / 2],     # no such image
               [n_img - 1, W - 3, H - 3, W + 40, H + 40],                 # across the far corner
               [0, 0.3 * W + 0.5 / scale, 0.2 * H + 0.5 / scale, 0.6 * W + 0.5 / scale, 0.7 * H + 1.5 / scale]]   # .5 after scaling
    rois[:len(special)] = np.asarray(special)
    return rois.astype(F)
