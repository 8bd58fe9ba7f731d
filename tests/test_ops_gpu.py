"""fasterrcnn_amd.ops on the GPU against the oracle's restatements of torchvision (oracle/frcnn_oracle.py: nms, roi_pool, roi_align,
roi_align_backward), generalised here to N images and rectangular outputs.

Tolerances are those of tests/test_roialign_gpu.py: RoIAlign forward (float32, the same operation order) <= 2e-7 of max|y|, backward
against the float64 accumulation of the same sampling plan <= 2e-6 of max|d| and bit-identical from run to run; RoIPool forward
bit-exact; NMS index lists equal."""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops
from oracle import frcnn_oracle as O

from tests import box_decisions_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


# ---- restatements generalised to rectangular outputs and N images ----------------------------------------------------------------
def align_plan(h, w, roi, oh, ow, scale, sr, aligned):
    """O.roi_align_weights for oh x ow bins (the same float32 expressions): (count, {(ph, pw): [(yl, xl, yh, xh, w1, w2, w3, w4)]})."""
    scale = F(scale)
    offset = F(0.5) if aligned else F(0.0)
    x1, y1, x2, y2 = (F(v) for v in roi)
    start_w, start_h = x1 * scale - offset, y1 * scale - offset
    end_w, end_h = x2 * scale - offset, y2 * scale - offset
    roi_w, roi_h = end_w - start_w, end_h - start_h
    if not aligned:
        roi_w, roi_h = max(roi_w, F(1.0)), max(roi_h, F(1.0))
    bin_h, bin_w = roi_h / F(oh), roi_w / F(ow)
    gh = int(sr) if sr > 0 else int(np.ceil(roi_h / F(oh)))
    gw = int(sr) if sr > 0 else int(np.ceil(roi_w / F(ow)))
    count = max(gh * gw, 1)

    def axis(v, n):
        if v < F(-1.0) or v > F(n):
            return None
        v = max(v, F(0.0))
        lo = int(v)
        if lo >= n - 1:
            return n - 1, n - 1, F(1.0), F(0.0)
        hi_w = v - F(lo)
        return lo, lo + 1, F(1.0) - hi_w, hi_w

    plan = {}
    for ph in range(oh):
        ys = [axis(start_h + F(ph) * bin_h + (F(iy) + F(0.5)) * bin_h / F(gh), h) for iy in range(gh)]
        for pw in range(ow):
            xs = [axis(start_w + F(pw) * bin_w + (F(ix) + F(0.5)) * bin_w / F(gw), w) for ix in range(gw)]
            s = []
            for ya in ys:
                for xa in xs:
                    if ya is None or xa is None:
                        continue
                    yl, yh, hy, ly = ya
                    xl, xh, hx, lx = xa
                    s.append((yl, xl, yh, xh, hy * hx, hy * lx, ly * hx, ly * lx))
            plan[ph, pw] = s
    return count, plan


def align_ref(x, rois, oh, ow, scale, sr, aligned):
    """roi_align (float32, the oracle's order) of x [N, C, H, W] and rois [K, 5]; an out-of-range batch index gives zeros."""
    n, c, h, w = x.shape
    out = np.zeros((rois.shape[0], c, oh, ow), F)
    for r in range(rois.shape[0]):
        b = int(rois[r, 0]) if -1 < rois[r, 0] < n else None
        if b is None:
            continue
        fm = x[b]
        count, plan = align_plan(h, w, rois[r, 1:], oh, ow, scale, sr, aligned)
        for (ph, pw), samples in plan.items():
            acc = np.zeros((c,), F)
            for (yl, xl, yh, xh, w1, w2, w3, w4) in samples:
                acc = acc + (w1 * fm[:, yl, xl] + w2 * fm[:, yl, xh] + w3 * fm[:, yh, xl] + w4 * fm[:, yh, xh])
            out[r, :, ph, pw] = acc / F(count)
    return out


def align_backward_ref(g, shape, rois, oh, ow, scale, sr, aligned):
    """float64 accumulation of the same plan (O.roi_align_backward generalised)."""
    n, c, h, w = shape
    d = np.zeros(shape, np.float64)
    g = g.astype(np.float64)
    for r in range(rois.shape[0]):
        if not (-1 < rois[r, 0] < n):
            continue
        b = int(rois[r, 0])
        count, plan = align_plan(h, w, rois[r, 1:], oh, ow, scale, sr, aligned)
        for (ph, pw), samples in plan.items():
            gb = g[r, :, ph, pw] / count
            for (yl, xl, yh, xh, w1, w2, w3, w4) in samples:
                d[b, :, yl, xl] += float(w1) * gb
                d[b, :, yl, xh] += float(w2) * gb
                d[b, :, yh, xl] += float(w3) * gb
                d[b, :, yh, xh] += float(w4) * gb
    return d


def _c_round(v):
    return int(np.floor(v + F(0.5))) if v >= 0 else int(np.ceil(v - F(0.5)))


def pool_ref(x, rois, oh, ow, scale):
    """roi_pool (O.roi_pool generalised) and its argmax (first maximum in (h, w) scan order, -1 for an empty bin or a bad image)."""
    n, c, h, w = x.shape
    k = rois.shape[0]
    out = np.zeros((k, c, oh, ow), F)
    arg = np.full((k, c, oh, ow), -1, np.int64)
    scale = F(scale)
    for r in range(k):
        if not (-1 < rois[r, 0] < n):
            continue
        fm = x[int(rois[r, 0])]
        rs_w, rs_h = _c_round(rois[r, 1] * scale), _c_round(rois[r, 2] * scale)
        re_w, re_h = _c_round(rois[r, 3] * scale), _c_round(rois[r, 4] * scale)
        bin_h = F(max(re_h - rs_h + 1, 1)) / F(oh)
        bin_w = F(max(re_w - rs_w + 1, 1)) / F(ow)
        for ph in range(oh):
            hs = min(max(int(np.floor(F(ph) * bin_h)) + rs_h, 0), h)
            he = min(max(int(np.ceil(F(ph + 1) * bin_h)) + rs_h, 0), h)
            for pw in range(ow):
                ws = min(max(int(np.floor(F(pw) * bin_w)) + rs_w, 0), w)
                we = min(max(int(np.ceil(F(pw + 1) * bin_w)) + rs_w, 0), w)
                if he > hs and we > ws:
                    win = fm[:, hs:he, ws:we].reshape(c, -1)
                    out[r, :, ph, pw] = win.max(axis=1)
                    j = win.argmax(axis=1)                                   # numpy: the first maximum in (h, w) order
                    arg[r, :, ph, pw] = (hs + j // (we - ws)) * w + ws + j % (we - ws)
    return out, arg


def make_rois(rng, k, n_img, h, w, scale):
    """[K, 5] float32: batch indices in arbitrary order, one out of range, boxes inside, across and outside the map."""
    H, W = h / scale, w / scale
    x1 = rng.uniform(-0.2 * W, 0.9 * W, k); y1 = rng.uniform(-0.2 * H, 0.9 * H, k)
    rois = np.stack([rng.randint(0, n_img, k), x1, y1, x1 + rng.uniform(1, 0.8 * W, k), y1 + rng.uniform(1, 0.8 * H, k)], 1)
    special = [[0, 0, 0, W, H], [n_img - 1, 0.3 * W, 0.2 * H, 0.3 * W + 1.7, 0.2 * H + 2.9], [0, -3 * W, -2 * H, -W, -H],
               [n_img, 0, 0, W / 2, H / 2], [n_img - 1, W - 3, H - 3, W + 40, H + 40], [0, 5, 5, 5, 5]]
    m = min(k, len(special))
    rois[:m] = np.asarray(special[:m])
    return rois.astype(F)


def to_gpu_input(x, channels_last):
    t = torch.from_numpy(x).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def boxes_arg(rois, n_img, as_list):
    r = torch.from_numpy(rois).to(DEV)
    if not as_list:
        return r, rois
    keep = (rois[:, 0] >= 0) & (rois[:, 0] < n_img) & (rois[:, 0] == np.floor(rois[:, 0]))
    order = np.argsort(rois[:, 0] + (~keep) * 1e9, kind="stable")[: int(keep.sum())]
    lst = [torch.from_numpy(rois[order][rois[order][:, 0] == i, 1:].copy()).to(DEV) for i in range(n_img)]
    return lst, rois[order]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- RoIAlign -------------------------------------------------------------------------------------------------------------------------
def test_rectangular_restatement_equals_oracle_on_square_outputs():
    rng = np.random.RandomState(0)
    x = rng.randn(1, 8, 11, 13).astype(F)
    rois = make_rois(rng, 8, 1, 11, 13, 0.25)
    rois[:, 0] = 0
    for sr, aligned in ((2, False), (-1, True), (1, False)):
        assert np.array_equal(align_ref(x, rois, 7, 7, 0.25, sr, aligned), O.roi_align(x, rois, 7, 0.25, sr, aligned))
        g = rng.randn(8, 8, 7, 7).astype(F)
        assert np.array_equal(align_backward_ref(g, x.shape, rois, 7, 7, 0.25, sr, aligned),
                              O.roi_align_backward(g, x.shape, rois, 7, 0.25, sr, aligned))


SIZES = [(7, 7), (14, 14), (7, 3), (1, 1), (32, 32)]
RATIOS = [-1, 0, 1, 2, 4, 16]
CHANNELS = [3, 4, 256, 1024]
FWD_CASES = [(s, sr, CHANNELS[i % 4], (1, 3)[i % 2], bool(i // 2 % 2), bool(i // 3 % 2), bool(i // 5 % 2))
             for i, (s, sr) in enumerate((s, sr) for s in SIZES for sr in RATIOS) if s[0] * s[1] * max(sr, 2) ** 2 <= 16384]


@pytest.mark.parametrize("size,sr,c,n_img,aligned,as_list,channels_last", FWD_CASES)
def test_roi_align_forward(size, sr, c, n_img, aligned, as_list, channels_last):
    rng = np.random.RandomState(sum(size) * 7 + sr + c)
    h, w, scale = 13, 17, 0.25
    k = 8 if c < 1024 else 6
    x = rng.randn(n_img, c, h, w).astype(F)
    rois = make_rois(rng, k, n_img, h, w, scale)
    boxes, rois_used = boxes_arg(rois, n_img, as_list)
    y = ops.roi_align(to_gpu_input(x, channels_last), boxes, size, scale, sr, aligned)
    assert y.shape == (rois_used.shape[0], c, size[0], size[1]) and y.is_contiguous(memory_format=torch.channels_last)
    got = y.cpu().numpy()
    want = align_ref(x, rois_used, size[0], size[1], scale, sr, aligned)
    assert rel(got, want) <= 2e-7
    bad = ~((rois_used[:, 0] > -1) & (rois_used[:, 0] < n_img))
    assert (got[bad] == 0).all()
    if size == (7, 7) and n_img == 1:                              # the square, one-image case is the oracle itself
        assert rel(got[~bad], O.roi_align(x, rois_used[~bad], 7, scale, sr, aligned)) <= 2e-7


BWD_CASES = [  # (n_img, c, h, w, k, size, scale, sr, aligned, channels_last)
    (1, 64, 37, 62, 40, (7, 7), 1 / 16, 2, False, False),
    (3, 4, 13, 17, 12, (7, 3), 0.25, -1, True, True),
    (2, 3, 9, 11, 8, (14, 14), 0.5, 4, False, False),
    (1, 256, 8, 9, 5, (32, 32), 0.5, 1, True, True),
    (2, 8, 12, 10, 6, (5, 5), 1.0, 16, False, True),
    (1, 1024, 6, 7, 5, (7, 7), 0.25, 0, False, False),
]


def run_align_backward(x, boxes, size, scale, sr, aligned, g, channels_last):
    xt = to_gpu_input(x, channels_last).requires_grad_(True)
    y = ops.roi_align(xt, boxes, size, scale, sr, aligned)
    y.backward(torch.from_numpy(g).to(DEV))
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert xt.grad.is_contiguous(memory_format=fmt)
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy()


@pytest.mark.parametrize("n_img,c,h,w,k,size,scale,sr,aligned,channels_last", BWD_CASES)
def test_roi_align_backward(n_img, c, h, w, k, size, scale, sr, aligned, channels_last):
    rng = np.random.RandomState(c + h * w + k)
    x = rng.randn(n_img, c, h, w).astype(F)
    rois = make_rois(rng, k, n_img, h, w, scale)
    g = rng.randn(k, c, size[0], size[1]).astype(F)
    boxes = torch.from_numpy(rois).to(DEV)
    y, d1 = run_align_backward(x, boxes, size, scale, sr, aligned, g, channels_last)
    _, d2 = run_align_backward(x, boxes, size, scale, sr, aligned, g, channels_last)
    assert np.array_equal(d1, d2)
    want = align_backward_ref(g, x.shape, rois, size[0], size[1], scale, sr, aligned)
    assert rel(d1, want) <= 2e-6
    lhs, rhs = float((g.astype(np.float64) * y).sum()), float((d1.astype(np.float64) * x).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)


def test_roi_align_backward_beyond_the_hit_list_caps():
    """Adaptive sampling on RoIs spanning a whole 64 x 100 map, 14 x 14 outputs: 5 x 8 samples per bin (frcnn_roi_align_backward takes
    at most 2 x 2)."""
    rng = np.random.RandomState(3)
    c, h, w = 8, 64, 100
    x = rng.randn(1, c, h, w).astype(F)
    rois = np.asarray([[0, 0, 0, w, h], [0, 0.5, 0.25, w - 0.5, h - 0.75], [0, -10, -10, w + 10, h + 10], [0, 10, 5, 90, 60]], F)
    g = rng.randn(4, c, 14, 14).astype(F)
    boxes = torch.from_numpy(rois).to(DEV)
    y, d1 = run_align_backward(x, boxes, 14, 1.0, -1, False, g, True)
    _, d2 = run_align_backward(x, boxes, 14, 1.0, -1, False, g, True)
    assert np.array_equal(d1, d2)
    assert rel(y, align_ref(x, rois, 14, 14, 1.0, -1, False)) <= 2e-7
    assert rel(d1, align_backward_ref(g, x.shape, rois, 14, 14, 1.0, -1, False)) <= 2e-6
    lhs, rhs = float((g.astype(np.float64) * y).sum()), float((d1.astype(np.float64) * x).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)


# ---- RoIPool ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_img,c,size,channels_last,as_list", [(1, 64, (7, 7), False, False), (3, 3, (7, 3), True, True),
                                                                 (2, 256, (14, 14), True, False), (1, 4, (1, 1), False, True),
                                                                 (2, 8, (32, 32), False, False)])
def test_roi_pool_forward_and_backward(n_img, c, size, channels_last, as_list):
    rng = np.random.RandomState(c + n_img)
    h, w, scale = 20, 32, 1 / 16
    x = rng.randn(n_img, c, h, w).astype(F)
    x[:, :, 3:9, 4:12] = 0.25                                      # constant regions: ties decided by the first maximum
    x[:, :, 12:, 20:] = -1.5
    rois = make_rois(rng, 10, n_img, h, w, scale)
    rois = np.concatenate([rois, np.asarray([[0, 40, 40, 200, 200], [n_img - 1, 300, 190, 520, 330]], F)])   # tie regions
    boxes, rois_used = boxes_arg(rois, n_img, as_list)
    want, arg = pool_ref(x, rois_used, size[0], size[1], scale)
    assert (arg == -1).any()                                       # empty bins are part of the case
    g = rng.randn(*want.shape).astype(F)
    grads = []
    for _ in range(2):
        xt = to_gpu_input(x, channels_last).requires_grad_(True)
        y = ops.roi_pool(xt, boxes, size, scale)
        y.backward(torch.from_numpy(g).to(DEV))
        grads.append(xt.grad.cpu().numpy())
    assert np.array_equal(y.detach().cpu().numpy(), want)
    assert np.array_equal(grads[0], grads[1])
    d = np.zeros((n_img, c, h * w), np.float64)
    for r in range(rois_used.shape[0]):
        if not (-1 < rois_used[r, 0] < n_img):
            continue
        b = int(rois_used[r, 0])
        for ch in range(c):
            a = arg[r, ch].ravel()
            np.add.at(d[b, ch], a[a >= 0], g[r, ch].ravel()[a >= 0].astype(np.float64))
    d = d.reshape(x.shape)
    assert rel(grads[0], d) <= 1e-5
    assert np.array_equal(grads[0] == 0, d == 0)


def test_roi_pool_reference_call_pattern():
    """detector.py:65-72: RoIPool((7, 7), 1/16) on the VGG-16 map of one image with the golden proposals, column-swapped to (b, x1, y1,
    x2, y2): bit for bit frcnn_roi_pool, and its input gradient bit for bit frcnn_roi_pool_backward's (non-zero)."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgg16_600x1000_s0.npz"))
    props = torch.from_numpy(gold["proposals"]).to(DEV)                       # (y1, x1, y2, x2)
    n, c, fh, fw = props.shape[0], 512, 37, 62
    gen = torch.Generator().manual_seed(5)
    fm = torch.relu(torch.randn((1, c, fh, fw), generator=gen)).to(DEV)
    rois = torch.cat([torch.zeros((n, 1), device=DEV), props[:, [1, 0, 3, 2]]], dim=1)
    x = fm.clone().requires_grad_(True)
    y = ops.RoIPool((7, 7), 1.0 / 16.0)(x, rois)
    dout = torch.randn(y.shape, generator=gen).to(DEV)
    y.backward(dout)
    lib = nv.lib()
    fm_hwc = fm[0].permute(1, 2, 0).contiguous()
    cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
    out = torch.empty((n, 7, 7, c), device=DEV)
    nv.check(lib.frcnn_roi_pool(nv.ptr(fm_hwc), fh, fw, c, nv.ptr(props), nv.ptr(cnt), n, 7, 1.0 / 16.0, nv.ptr(out), nv.stream_ptr()),
             "frcnn_roi_pool")
    assert torch.equal(y.permute(0, 2, 3, 1), out)
    wsb = int(lib.frcnn_roi_pool_backward_workspace_bytes(n, 7, c))
    ws = torch.empty((wsb // 4,), device=DEV)
    d_dout = dout.permute(0, 2, 3, 1).contiguous()
    dfm = torch.empty((fh, fw, c), device=DEV)
    nv.check(lib.frcnn_roi_pool_backward(nv.ptr(fm_hwc), fh, fw, c, nv.ptr(props), n, 7, 1.0 / 16.0, nv.ptr(d_dout), nv.ptr(dfm), 0,
                                         nv.ptr(ws), wsb, nv.stream_ptr()), "frcnn_roi_pool_backward")
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    assert torch.equal(x.grad[0].permute(1, 2, 0), dfm)


# ---- NMS ----------------------------------------------------------------------------------------------------------------------------
def check_nms(boxes, scores, thr):
    got = ops.nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), thr)
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    want = O.nms(boxes, scores, thr)
    assert got.cpu().numpy().tolist() == want.tolist()
    return want


# n = 40000 at the two thresholds the reference uses (the oracle's loop over every kept box is the slow part)
NMS_CASES = [(n, thr) for n in (0, 1, 2, 300, 6000, 12000) for thr in (0.0, 0.3, 0.5, 0.7, 1.0)] + [(40000, 0.5), (40000, 0.7)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,thr", NMS_CASES)
def test_nms_matches_oracle(dtype, n, thr):
    rng = np.random.RandomState(n + int(thr * 10))
    boxes = B.cluster_boxes(max(n, 1), n + 1)[:n].astype(dtype)
    if dtype == np.float64:
        boxes = boxes + rng.uniform(-1e-3, 1e-3, boxes.shape)
    scores = rng.rand(n).astype(dtype)
    scores[: n // 10] = 0.5                                               # ties
    check_nms(boxes, scores, thr)


def test_nms_families():
    for scale in B.NMS_SCALES:
        for thr in (0.7, 0.5):
            boxes, scores = B.dense_call(scale, thr)
            check_nms(boxes, scores, thr)
            check_nms(boxes.astype(np.float64), scores, thr)
    for name, (boxes, scores) in sorted(B.degenerate_families().items()):
        for thr in (0.7, 0.3, 0.0):
            check_nms(boxes, scores, thr)
            check_nms(boxes.astype(np.float64), scores.astype(np.float64), thr)
    boxes, scores = B.degenerate_mixed()
    check_nms(boxes, scores, 0.5)
    for name, (boxes, scores) in sorted(B.score_families().items()):
        check_nms(boxes, scores, 0.5)
        check_nms(*B.isolated_score_call(scores), 0.5)


def test_nms_keeps_more_than_2048():
    boxes = B.filler_boxes(10000)
    scores = np.random.RandomState(1).rand(10000).astype(F)
    want = check_nms(boxes, scores, 0.5)
    assert len(want) == 10000


def test_nms_float64_decision_differs_from_float32():
    x = 1.0 / 3.0 - 1e-12                        # IoU (1 - x) / (1 + x): just above 0.5 in float64, below it on the float32-rounded boxes
    b64 = np.asarray([[0.0, 0.0, 1.0, 1.0], [x, 0.0, 1.0 + x, 1.0]], np.float64)
    s = np.asarray([0.9, 0.8], np.float64)
    assert O.nms(b64, s, 0.5).tolist() == [0]
    assert O.nms(b64.astype(F), s.astype(F), 0.5).tolist() == [0, 1]
    assert check_nms(b64, s, 0.5).tolist() == [0]
    assert check_nms(b64.astype(F), s.astype(F), 0.5).tolist() == [0, 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,n_cat", [(0, 5), (1, 3), (500, 7), (6000, 100), (20000, 100)])
def test_batched_nms_matches_per_category_loop(dtype, n, n_cat):
    rng = np.random.RandomState(n + n_cat)
    boxes = B.cluster_boxes(max(n, 1), 3, clusters=20)[:n].astype(dtype)
    scores = rng.rand(n).astype(dtype)
    scores[rng.rand(n) < 0.1] = 0.25                                       # ties across and inside categories
    cats = rng.randint(0, n_cat, n)
    cats[cats % 7 == 3] = 0                                                # some categories empty
    keep = []
    for cat in np.unique(cats):
        idx = np.where(cats == cat)[0]
        keep.append(idx[O.nms(boxes[idx], scores[idx], 0.5)])
    keep = np.concatenate(keep) if keep else np.zeros((0,), np.int64)
    want = keep[np.lexsort((keep, -scores[keep].astype(np.float64)))]
    got = ops.batched_nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(cats).to(DEV), 0.5)
    assert got.cpu().numpy().tolist() == want.tolist()


# ---- opcheck --------------------------------------------------------------------------------------------------------------------------
OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_every_op():
    rng = np.random.RandomState(9)
    x = torch.from_numpy(rng.randn(2, 8, 10, 12).astype(F)).to(DEV).requires_grad_(True)
    rois = torch.from_numpy(make_rois(rng, 6, 2, 10, 12, 0.5)).to(DEV)
    torch.library.opcheck(torch.ops.frcnn.roi_align.default, (x, rois, 0.5, 7, 3, 2, False), test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.roi_pool.default, (x, rois, 0.5, 7, 3), test_utils=OPCHECK)
    g = torch.from_numpy(rng.randn(6, 8, 7, 3).astype(F)).to(DEV)
    torch.library.opcheck(torch.ops.frcnn.roi_align_backward.default, (g, rois, 0.5, 7, 3, 2, False, 2, 8, 10, 12, True),
                          test_utils=OPCHECK)
    _, argmax = torch.ops.frcnn.roi_pool.default(x.detach(), rois, 0.5, 7, 3)
    torch.library.opcheck(torch.ops.frcnn.roi_pool_backward.default, (g, rois, argmax, 0.5, 7, 3, 2, 8, 10, 12, False),
                          test_utils=OPCHECK)
    boxes = torch.from_numpy(B.cluster_boxes(200, 2)).to(DEV)
    scores = torch.from_numpy(rng.rand(200).astype(F)).to(DEV)
    torch.library.opcheck(torch.ops.frcnn.nms.default, (boxes, scores, 0.5), test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.batched_nms.default,
                          (boxes.double(), scores, torch.from_numpy(rng.randint(0, 5, 200)).to(DEV), 0.5), test_utils=OPCHECK)


def test_double_backward_raises():
    x = torch.randn((1, 4, 8, 8), device=DEV, requires_grad=True)
    rois = torch.tensor([[0, 0, 0, 6, 6]], dtype=torch.float32, device=DEV)
    for fn in (lambda: ops.roi_align(x, rois, 2), lambda: ops.roi_pool(x, rois, 2)):
        y = fn()
        v = torch.ones_like(y, requires_grad=True)
        g, = torch.autograd.grad(y, x, grad_outputs=v, create_graph=True)
        with pytest.raises(RuntimeError, match="double backward"):
            g.sum().backward()
