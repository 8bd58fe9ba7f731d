"""
Case tables and plain numpy references for the train step's small kernels (csrc/train.hip, softmax_rows of csrc/linear.hip) at the
seams those kernels have: the 256-thread loop of the one-block loss kernels, the 64-RoI chunks and the 64 x 49 hit list of the RoI-pool
scatter, channels beyond one 256-thread pass, the grid caps of the grid-stride kernels and their tails.  No GPU.
tests/test_train_edges_cpu.py holds these references to torch autograd / oracle/train_oracle.py; tests/test_train_edges_gpu.py holds
the kernels to these references.

Two kinds of reference, each written from the operation's definition (not from the kernel):
  * float64 "truth" (rpn_loss_truth, detector_loss_truth, roi_pool_backward_truth, softmax_truth, bn_affine_truth): values and
    gradients in float64 from the float32 inputs;
  * float32 "rounded once" (the *_ref functions): operations that have exactly one correct float32 answer, so the kernel is held to
    the bit.  Every product and sum is a separate np.float32 operation.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24                     # unit roundoff of float32


def rng_of(*key):
    return np.random.RandomState(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def c_round(v):
    """C roundf of a float32: half away from zero (np.round rounds half to even).  v - trunc(v) is exact in float32."""
    v = F(v)
    r = np.trunc(v)
    if abs(v - r) >= F(0.5):
        r += np.sign(v)
    return int(r)


# =====================================================================================================================================
# RPN losses: rpn.py class_loss (F.binary_cross_entropy of the sigmoid scores, masked by the mini-batch) + regression_loss (robust L1,
# sigma^2 = 9, on the object anchors of the mini-batch), both divided by count + 1e-7
# =====================================================================================================================================
RPN_FH, RPN_FW = 5, 7
RPN_P = RPN_FH * RPN_FW                  # 35 cells, 315 anchors
RPN_N_SAMPLE = (0, 1, 255, 256, 257, 315)
RPN_LD = (45, 48, 128)
RPN_MIXES = ("background", "object", "mixed")
# residuals target - prediction for the first object anchors: both sides of 1/sigma^2 = 1/9 in both signs, and exactly 0
RPN_RESIDUALS = (0.05, -0.05, 0.2, -0.2, 0.0, 0.111, -0.111, 0.1112, -0.1112, 1.5, -1.5, 0.0)


def rpn_case(n_sample, ld, mix):
    """head [P][ld] (9 logits | 36 deltas | pad), sample [n_sample] int32 (unique flat anchors, shuffled), rpn_map [9P][6].
    Logits stay within +-4, where the float32 sigmoid is well conditioned, except four at +-120 where float32 and float64 both
    saturate; anchors outside the sample carry object flags and targets too (a kernel that reads them is wrong)."""
    r = rng_of(n_sample, ld, RPN_MIXES.index(mix))
    A = 9 * RPN_P
    head = np.full((RPN_P, ld), 7.0, dtype=F)                       # pad columns: a value that would show
    head[:, 0:9] = np.clip(r.randn(RPN_P, 9) * 2.0, -4.0, 4.0)
    head[:, 9:45] = r.randn(RPN_P, 36) * 0.5
    rest = r.permutation(np.arange(1, A - 1))
    if n_sample >= 2:
        sample = np.concatenate([[0, A - 1], rest[:n_sample - 2]])
    elif n_sample == 1:
        sample = np.array([A - 1])
    else:
        sample = np.zeros((0,), dtype=np.int64)
    sample = sample[r.permutation(n_sample)].astype(np.int32)
    rpn_map = np.zeros((A, 6), dtype=F)
    rpn_map[sample, 0] = 1.0
    rpn_map[:, 1] = (r.rand(A) < 0.4)
    if mix == "background":
        rpn_map[sample, 1] = 0.0
    elif mix == "object":
        rpn_map[sample, 1] = 1.0
    elif n_sample >= 2:
        rpn_map[sample[0], 1], rpn_map[sample[1], 1] = 1.0, 0.0
    rpn_map[:, 2:6] = r.randn(A, 4) * 0.5
    # saturated sigmoids on sampled anchors, with both labels where there are enough samples
    for j, logit in enumerate((120.0, -120.0, 120.0, -120.0)[:min(4, n_sample)]):
        a = int(sample[j])
        head[a // 9, a % 9] = logit
        if mix == "mixed" and n_sample >= 4:
            rpn_map[a, 1] = 1.0 if j < 2 else 0.0
    # residuals on both sides of 1/9, and exactly 0, on the first sampled object anchors; small random ones on the rest
    obj = [int(a) for a in sample if rpn_map[a, 1] != 0]
    for a in obj:
        head[a // 9, 9 + 4 * (a % 9):13 + 4 * (a % 9)] = rpn_map[a, 2:6] - (r.randn(4) * 0.15).astype(F)
    for j, a in enumerate(obj[:3]):
        for c in range(4):
            head[a // 9, 9 + 4 * (a % 9) + c] = rpn_map[a, 2 + c] - F(RPN_RESIDUALS[4 * j + c])
    return head, sample, rpn_map


def rpn_loss_truth(head, sample, rpn_map):
    """(class loss, regression loss, d(class + regression)/d head [P][ld]) in float64.
    The count is `count_nonzero(mask) + 1e-7` as the reference forms it: an integer tensor plus a Python float, i.e. a float32."""
    head64 = head.astype(np.float64)
    n = float(F(len(sample)) + F(1e-7))
    d = np.zeros(head.shape, dtype=np.float64)
    cls_sum = reg_sum = 0.0
    with np.errstate(divide="ignore", over="ignore"):
        for a in sample:
            a = int(a)
            cell, k = a // 9, a % 9
            y = float(rpn_map[a, 1])
            p = 1.0 / (1.0 + np.exp(-head64[cell, k]))
            lp, lq = max(np.log(p), -100.0), max(np.log(1.0 - p), -100.0)        # F.binary_cross_entropy clamps its logs at -100
            cls_sum += -(y * lp + (1.0 - y) * lq)
            pq = p * (1.0 - p)
            d[cell, k] = (p - y) / max(pq, 1e-12) * pq / n                        # its backward, then the sigmoid's
            if y != 0.0:
                for c in range(4):
                    x = float(rpn_map[a, 2 + c]) - head64[cell, 9 + 4 * k + c]
                    if abs(x) < 1.0 / 9.0:
                        loss, dx = 0.5 * x * x * 9.0, 9.0 * x
                    else:
                        loss, dx = abs(x) - 0.5 / 9.0, np.sign(x)
                    reg_sum += y * loss
                    d[cell, 9 + 4 * k + c] = -(y * dx) / n
    return cls_sum / n, reg_sum / n, d


# =====================================================================================================================================
# detector losses: detector.py class_loss -(y log(p + 1e-7)).sum / (S + 1e-7) on softmax outputs p, regression_loss (robust L1,
# sigma^2 = 1, masked) / (S + 1e-7); gradient with respect to [class logits | regressor outputs]
# =====================================================================================================================================
DET_S = (0, 1, 255, 256, 257, 600)
DET_NCLS = (2, 21, 26)


def softmax_f32(x):
    """A float32 softmax (inputs of the detector-loss cases: what it rounds to is part of the case, not of any reference)."""
    x = x.astype(F)
    e = np.exp(x - x.max(axis=1, keepdims=True)).astype(F)
    return (e / e.sum(axis=1, keepdims=True, dtype=F)).astype(F)


def detector_case(S, ncls):
    """classes [S][ncls] (float32 softmax outputs), deltas [S][nd], onehot [S][ncls], gt_deltas [S][2][nd], and the row kinds:
    kind 1: the true class has p == 0.0 exactly (logits -60 / +60), kind 3: the true class has p == 1.0 exactly, kind 5: background."""
    r = rng_of(S, ncls, 77)
    nd = 4 * (ncls - 1)
    logits = (r.randn(S, ncls) * 3).astype(F)
    cls = r.randint(0, ncls, size=S)
    kind = (np.arange(S) + ncls) % 8
    for i in range(S):
        if kind[i] == 1:
            cls[i] = 1 + i % (ncls - 1)
            logits[i, cls[i]] = -60.0
            logits[i, (cls[i] + 1) % ncls] = 60.0
        elif kind[i] == 3:
            cls[i] = 1 + (3 * i) % (ncls - 1)
            logits[i, cls[i]] = 60.0
        elif kind[i] == 5:
            cls[i] = 0
    classes = softmax_f32(logits) if S else np.zeros((0, ncls), dtype=F)
    onehot = np.zeros((S, ncls), dtype=F)
    onehot[np.arange(S), cls] = 1.0
    gtd = np.zeros((S, 2, nd), dtype=F)
    gtd[:, 0, :] = np.repeat(onehot, 4, axis=1)[:, 4:]
    gtd[:, 1, :] = r.randn(S, nd) * 1.5
    deltas = r.randn(S, nd).astype(F)
    return classes, deltas, onehot, gtd, cls, kind


def detector_loss_truth(classes, deltas, onehot, gtd, eps_in_float32=True):
    """(class loss, regression loss, gradient [S][ncls + nd]) in float64.  The 1e-7 is added to p in float32, as detector.py does on its
    float32 tensors (eps_in_float32=False adds it in float64: what the same code computes on float64 tensors)."""
    S, ncls = onehot.shape
    nd = 4 * (ncls - 1)
    n = S + 1e-7
    p = classes.astype(np.float64)
    pe = (classes.astype(F) + F(1e-7)).astype(np.float64) if eps_in_float32 else p + 1e-7
    y = onehot.astype(np.float64)
    l_cls = float(-(y * np.log(pe)).sum() / n)
    g = -(y / pe) / n                                                       # d loss / d p
    d_cls = p * (g - (g * p).sum(axis=1, keepdims=True))                     # softmax backward
    mask, tgt = gtd[:, 0, :].astype(np.float64), gtd[:, 1, :].astype(np.float64)
    x = tgt - deltas.astype(np.float64)
    small = np.abs(x) < 1.0
    loss = np.where(small, 0.5 * x * x, np.abs(x) - 0.5)
    dx = np.where(small, x, np.sign(x))
    l_reg = float((mask * loss).sum() / n)
    return l_cls, l_reg, np.concatenate([d_cls, -(mask * dx) / n], axis=1).reshape(S, ncls + nd)


# =====================================================================================================================================
# RoI pool backward (torchvision RoIPool): maps [fh][fw][C], RoIs (y1, x1, y2, x2) in image pixels, dout [n][pooled][pooled][C]
# =====================================================================================================================================
ROI_SCALE = 1.0 / 16.0
# (fh, fw, C, pooled, n_rois)
ROI_SHAPES = ((5, 6, 4, 7, 1), (9, 11, 260, 3, 65), (6, 7, 1024, 1, 130), (8, 9, 8, 7, 0), (8, 9, 8, 7, 63), (8, 9, 8, 7, 64), (8, 9, 8, 7, 65))


def roi_map(fh, fw, C, seed=0):
    """relu(randn): many exact zeros that tie; one constant patch."""
    r = rng_of(fh, fw, C, seed)
    fm = np.maximum(r.randn(fh, fw, C), 0.0).astype(F)
    fm[1:3, 2:4, :] = 0.75
    return fm


def roi_boxes(fh, fw, n, seed=0):
    """n RoIs at scale 1/16: first the special ones, then random ones.  Corners at multiples of 8 land on x.5 after scaling, where
    roundf (half away from zero) and round-half-to-even differ: 40 -> 2.5 -> 3, 72 -> 4.5 -> 5, -8 -> -0.5 -> -1, -40 -> -2.5 -> -3."""
    r = rng_of(fh, fw, n, seed, 5)
    H, W = 16.0 * fh, 16.0 * fw
    special = [
        [8, 8, 72, 88],                                  # half-way corners, positive
        [-8, -40, 40, 72],                               # half-way corners, negative
        [-50, -30, 40, 60],                              # partly off the map (top left)
        [H - 24, W - 40, H + 100, W + 90],               # partly off the map (bottom right)
        [H + 40, W + 40, H + 200, W + 200],              # wholly off: every bin empty
        [-300, -300, -100, -100],                        # wholly off on the other side
        [0.7 * H, 0.8 * W, 0.2 * H, 0.1 * W],            # inverted: one cell
        [-100, -100, H + 100, W + 100],                  # larger than the map
        [24, 40, 24, 40],                                # a single cell (1.5, 2.5) -> (2, 3), in every bin
        [40, 24, 56, 104],
    ]
    out = np.zeros((n, 4), dtype=F)
    for i in range(n):
        if i < len(special):
            out[i] = special[i]
        else:
            y1, x1 = r.uniform(-32, H), r.uniform(-32, W)
            out[i] = [y1, x1, y1 + r.uniform(0, H), x1 + r.uniform(0, W)]
            if i % 4 == 0:
                out[i] = np.round(out[i] / 8.0) * 8.0                     # more half-way corners
    return out


def full_hit_list_boxes():
    """On the 8 x 9 map: 64 identical RoIs of one cell (3, 4) -- each holds the cell in all 49 bins, 64 x 49 = 3136 hits fill the
    scatter kernel's list exactly -- then the same RoI once more (the next chunk) and a different box."""
    return np.array([[48, 64, 48, 64]] * 65 + [[8, 8, 72, 88]], dtype=F)


def roi_pool_backward_truth(fm, rois, pooled, scale, dout):
    """float64 gradient [fh][fw][C] of the map, with per map cell and channel the number of addends and sum |addend|.
    Corners round half away from zero; bin [floor(p bin), ceil((p + 1) bin)) + start, clamped to the map; the gradient of a bin goes
    to its FIRST maximum in (h, w) scan order (strict '>': argmax of the window flattened in that order), nowhere for an empty bin."""
    fh, fw, C = fm.shape
    scale = F(scale)
    grad = np.zeros((fh * fw, C), dtype=np.float64)
    count = np.zeros((fh * fw, C), dtype=np.int64)
    sum_abs = np.zeros((fh * fw, C), dtype=np.float64)
    ch = np.arange(C)
    for i in range(rois.shape[0]):
        rs_h, rs_w = c_round(F(rois[i, 0]) * scale), c_round(F(rois[i, 1]) * scale)
        re_h, re_w = c_round(F(rois[i, 2]) * scale), c_round(F(rois[i, 3]) * scale)
        roi_h, roi_w = max(re_h - rs_h + 1, 1), max(re_w - rs_w + 1, 1)
        bin_h, bin_w = F(roi_h) / F(pooled), F(roi_w) / F(pooled)
        for ph in range(pooled):
            hs = min(max(int(np.floor(F(ph) * bin_h)) + rs_h, 0), fh)
            he = min(max(int(np.ceil(F(ph + 1) * bin_h)) + rs_h, 0), fh)
            for pw in range(pooled):
                ws = min(max(int(np.floor(F(pw) * bin_w)) + rs_w, 0), fw)
                we = min(max(int(np.ceil(F(pw + 1) * bin_w)) + rs_w, 0), fw)
                if he <= hs or we <= ws:
                    continue
                am = fm[hs:he, ws:we, :].reshape(-1, C).argmax(axis=0)
                cell = (hs + am // (we - ws)) * fw + (ws + am % (we - ws))
                g = dout[i, ph, pw, :].astype(np.float64)
                np.add.at(grad, (cell, ch), g)
                np.add.at(count, (cell, ch), 1)
                np.add.at(sum_abs, (cell, ch), np.abs(g))
    return grad.reshape(fh, fw, C), count.reshape(fh, fw, C), sum_abs.reshape(fh, fw, C)


# =====================================================================================================================================
# softmax, BatchNorm affine (float64 truth)
# =====================================================================================================================================
SOFTMAX_M = (1, 3, 4, 5, 301)
SOFTMAX_NCLS = (1, 2, 21, 63, 64, 65, 81, 127, 128)
SOFTMAX_PAD = 1e30


def softmax_case(M, ncls, ldx):
    """x [M][ldx] with 1e30 in the pad columns.  Row kinds by (row + ncls) % 4: 0 all-equal, 1 logits of magnitude 1e4,
    2 some -inf entries (never all), 3 mild."""
    r = rng_of(M, ncls, ldx)
    x = np.full((M, ldx), SOFTMAX_PAD, dtype=F)
    kind = (np.arange(M) + ncls) % 4
    v = (r.randn(M, ncls) * 3).astype(F)
    for i in range(M):
        if kind[i] == 0:
            v[i] = 3.25
        elif kind[i] == 1:
            v[i] = (1e4 if i % 2 else -1e4) + r.randn(ncls) * 2
        elif kind[i] == 2:
            v[i, 1::3] = -np.inf                                       # entry 0 stays finite
    x[:, :ncls] = v
    return x, kind


def softmax_truth(x, dy=None):
    """float64 row softmax of x [M][ncls]; with dy also the gradient dx = p (dy - sum(dy p))."""
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    if dy is None:
        return p
    dy = dy.astype(np.float64)
    return p, p * (dy - (dy * p).sum(axis=1, keepdims=True))


BN_C = (1, 255, 256, 257, 2048)
BN_EPS = 1e-5


def bn_case(c):
    r = rng_of(c, 31)
    gamma, beta, mean = (r.rand(c) + 0.5).astype(F), r.randn(c).astype(F), r.randn(c).astype(F)
    var = (10.0 ** r.uniform(-8, 0.5, size=c)).astype(F)
    var[0] = 1e-8
    return gamma, beta, mean, var


def bn_affine_truth(gamma, beta, mean, var, eps):
    """Frozen BatchNorm as y = x scale + shift, float64: scale = gamma / sqrt(var + eps), shift = beta - mean scale (eps the float32 the
    entry point receives), and the gradients d scale / d gamma, d shift / d gamma, d shift / d beta, d shift / d mean."""
    inv = 1.0 / np.sqrt(var.astype(np.float64) + float(F(eps)))
    scale = gamma.astype(np.float64) * inv
    shift = beta.astype(np.float64) - mean.astype(np.float64) * scale
    grads = {"dscale_dgamma": inv, "dshift_dgamma": -mean.astype(np.float64) * inv, "dshift_dbeta": np.ones_like(inv), "dshift_dmean": -scale}
    return scale, shift, grads


# =====================================================================================================================================
# float32 "rounded once" references
# =====================================================================================================================================
RELU_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 8192 * 256 + 1203)     # the last: a second stride pass of float4s and a scalar tail
ADD_N = (1, 255, 256, 257, 8192 * 256 + 257)
MAXPOOL_SHAPES = ((2, 2, 4), (3, 3, 4), (2, 7, 8), (7, 2, 12), (38, 63, 68), (258, 256, 512))     # the last: just over the grid cap
TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (33, 31), (64, 65), (2294, 45))
GATHER_ROW_FLOATS = (1, 63, 64, 255, 256, 257, 25088)
PACK_SHAPES = ((9, 1, 1), (9, 5, 3), (1, 64, 7), (49, 3, 2), (9, 512, 520))                        # (taps, cout, cin); the last over the cap
MEAN_SHAPES = ((1, 1, 1, 1), (2, 7, 7, 5), (3, 3, 5, 32), (24, 7, 7, 2048))                        # (N, H, W, C)
SGD_N = (1, 255, 256, 257, 16384 * 256 + 5)
SGD_FOLD_SHAPES = ((9, 5, 3), (1, 64, 7), (9, 512, 1024))                                            # the last over the cap
SGD_CONFIGS = ((0.9, 5e-4), (0.0, 5e-4), (0.9, 0.0), (0.0, 0.0))                                     # (momentum, weight decay); momentum 0: NULL buffer
SGD_LR = 1e-3
TINY = np.float32(1e-45)                 # the smallest positive subnormal


def relu_case(n):
    """y: relu(randn) with +0.0, -0.0, the smallest subnormal and +inf at both ends; dy: randn with +-inf and -0.0.  No NaN."""
    r = rng_of(n, 1)
    y = np.maximum(r.randn(n), 0.0).astype(F)
    dy = r.randn(n).astype(F)
    ys, ds = (0.0, -0.0, TINY, np.inf), (np.inf, -np.inf, -0.0)
    for i in range(min(n, 12)):
        y[i] = ys[i % 4]
        dy[i] = ds[i % 3]
        y[n - 1 - i] = ys[(i + 1) % 4]
        dy[n - 1 - i] = ds[(i + 2) % 3]
    return dy, y


def relu_backward_ref(dy, y):
    return np.where(y > 0, dy, F(0.0)).astype(F)


def add_ref(a, b):
    return (a + b).astype(F)


def maxpool_case(H, W, C):
    """x [H][W][C], dy [H/2][W/2][C].  The first windows hold ties, the kind rotating with window and channel: 0 all four equal,
    1 the 2nd and 3rd equal and largest, 2 the 3rd and 4th equal and largest, 3 +0.0 against -0.0, 4 all -inf, 5 none."""
    r = rng_of(H, W, C, 2)
    x = r.randn(H, W, C).astype(F)
    Ho, Wo = H // 2, W // 2
    dy = r.randn(Ho, Wo, C).astype(F)
    patterns = {0: (1.5, 1.5, 1.5, 1.5), 1: (-1.0, 2.0, 2.0, 0.5), 2: (0.25, -3.0, 2.5, 2.5), 3: (-0.0, 0.0, -0.0, 0.0),
                4: (-np.inf,) * 4}
    for win in range(min(8, Ho * Wo)):
        oy, ox = win // Wo, win % Wo
        for c in range(C):
            k = (win + c) % 6
            if k in patterns:
                for q in range(4):
                    x[2 * oy + (q >> 1), 2 * ox + (q & 1), c] = patterns[k][q]
    return x, dy


def maxpool2x2_backward_ref(x, dy):
    """The gradient of each 2 x 2 window goes to its first maximum in (row, column) order (strict '>'); an odd last row / column gets 0."""
    H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = [x[(q >> 1):2 * Ho:2, (q & 1):2 * Wo:2, :] for q in range(4)]
    m, am = v[0].copy(), np.zeros(v[0].shape, dtype=np.int8)
    for q in range(1, 4):
        up = v[q] > m
        m = np.where(up, v[q], m)
        am = np.where(up, np.int8(q), am)
    dx = np.zeros((H, W, C), dtype=F)
    for q in range(4):
        dx[(q >> 1):2 * Ho:2, (q & 1):2 * Wo:2, :] = np.where(am == q, dy, F(0.0))
    return dx


def transpose_ref(x, rows, cols, ldo):
    """y [cols][ldo]: y[c][r] = x[r][c], columns rows..ldo-1 zero."""
    y = np.zeros((cols, ldo), dtype=F)
    y[:, :rows] = x[:rows, :cols].T
    return y


def gather_ref(src, idx):
    return src[idx.astype(np.int64)]


def pack_conv3x3_dgrad_ref(wp):
    """[tap][co][ci] -> [8 - tap][ci][co]"""
    return np.ascontiguousarray(wp[::-1].transpose(0, 2, 1))


def pack_conv_dgrad_ref(wp):
    """[tap][co][ci] -> [tap][ci][co]"""
    return np.ascontiguousarray(wp.transpose(0, 2, 1))


def scale_rows_ref(src, scale):
    return (src * scale.astype(F)[None, :, None]).astype(F)


def spatial_mean_backward_ref(dy, H, W):
    """backward of x.mean(-1).mean(-1): dx[n][y][x][c] = (dy[n][c] / H) / W, two float32 divisions."""
    N, C = dy.shape
    v = ((dy / F(H)).astype(F) / F(W)).astype(F)
    return np.ascontiguousarray(np.broadcast_to(v[:, None, None, :], (N, H, W, C)))


def sgd_ref(w, g, buf, lr, momentum, weight_decay, first, scale=None):
    """torch.optim.SGD.step in float32, every product and sum rounded on its own:
    g += wd w (wd != 0); buf = first ? g : momentum buf + g (momentum != 0); w = w + -(lr buf).
    Returns (w, buf, folded): buf is None when momentum == 0; folded = w_new * scale[co] of a [taps][cout][cin] master, or None."""
    lr, momentum, weight_decay = F(lr), F(momentum), F(weight_decay)
    g = g.astype(F)
    if weight_decay != 0:
        g = (g + (weight_decay * w).astype(F)).astype(F)
    b = g
    if momentum != 0:
        b = g if first else ((momentum * buf).astype(F) + g).astype(F)
    w_new = (w + (-(lr * b).astype(F))).astype(F)
    folded = None
    if scale is not None:
        folded = (w_new * scale.astype(F)[None, :, None]).astype(F)
    return w_new, (b if momentum != 0 else None), folded
