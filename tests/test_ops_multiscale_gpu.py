"""fasterrcnn_amd.ops.multi_scale_roi_align / MultiScaleRoIAlign on the GPU.

The reference is torchvision's ops/poolers.py composition restated here over ops.roi_align: LevelMapper in torch float32 on the same
device, then per level torch.where + roi_align + index_put.  The fused op must equal it bit for bit, forward and backward (torch.equal),
and each level must match the float64-accumulated restatement of tests/test_ops_gpu.py within that file's tolerances."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fasterrcnn_amd import ops
from tests.test_ops_gpu import align_backward_ref, align_ref, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
FPN_SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64]


# ---- torchvision's composition ----------------------------------------------------------------------------------------------------
def tv_level_range(scales):
    return (int(-torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()),
            int(-torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()))


def tv_levels(rois, k_min, k_max, canonical_scale=224, canonical_level=4):
    """LevelMapper (torch float32, on the RoIs' device); a NaN level -> -1 (torchvision's CPU cast), not the GPU's NaN -> int64."""
    b = rois[:, 1:]
    s = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    t = torch.floor(canonical_level + torch.log2(s / canonical_scale) + torch.tensor(1e-6, dtype=s.dtype))
    t = torch.clamp(t, min=k_min, max=k_max)
    return torch.where(torch.isnan(t), torch.full_like(t, -1, dtype=torch.int64), t.to(torch.int64) - k_min)


def as_rois(boxes):
    if isinstance(boxes, torch.Tensor):
        return boxes
    return torch.cat([torch.cat([torch.full_like(b[:, :1], float(i)), b], 1) for i, b in enumerate(boxes)], 0)


def composition(features, boxes, output_size, scales, sr):
    rois = as_rois(boxes)
    if len(features) == 1:
        return ops.roi_align(features[0], rois, output_size, scales[0], sr)
    levels = tv_levels(rois, *tv_level_range(scales))
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    result = torch.zeros((rois.shape[0], features[0].shape[1], oh, ow), device=rois.device)
    for level, (f, s) in enumerate(zip(features, scales)):
        idx = torch.where(levels == level)[0]
        result[idx] = ops.roi_align(f, rois[idx], output_size, s, sr)
    return result


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def make_features(rng, n, c, img_h, img_w, n_levels, channels_last, requires_grad=False):
    feats = []
    for i in range(n_levels):
        h, w = -(-img_h // 2 ** (i + 2)), -(-img_w // 2 ** (i + 2))
        t = torch.from_numpy(rng.randn(n, c, h, w).astype(F)).to(DEV)
        if channels_last if isinstance(channels_last, bool) else channels_last[i]:
            t = t.contiguous(memory_format=torch.channels_last)
        feats.append(t.requires_grad_(requires_grad))
    return feats


def make_boxes(rng, k, n, img_h, img_w):
    """[K, 5]: sizes log-uniform over 8 .. 1200 px (every FPN level), some boxes partly or wholly outside the image, special rows."""
    side = np.exp(rng.uniform(np.log(8), np.log(1200), (k, 2)))
    x1 = rng.uniform(-0.2 * img_w, img_w, k)
    y1 = rng.uniform(-0.2 * img_h, img_h, k)
    rois = np.stack([rng.randint(0, n, k), x1, y1, x1 + side[:, 0], y1 + side[:, 1]], 1)
    special = [[0, 10, 10, 10, 60],                     # zero area: level 0
               [n - 1, 50, 20, 30, 90],                 # inverted x: negative area, no level
               [n, 0, 0, 200, 200],                     # batch index n: zeros
               [-1, 0, 0, 100, 100],                    # batch index -1: zeros
               [0, -3000, -3000, -2000, -2000],         # wholly outside
               [n - 1, img_w - 30, img_h - 30, img_w + 400, img_h + 500],
               [0, 0, 0, 64, 64], [n - 1, 8, 8, 168, 168], [0, 16, 16, 336, 336],   # sqrt(area) 64 .. 1000: one RoI per FPN level
               [n - 1, 0, 0, 640, 640], [0, 0, 0, 1000, 1000]]
    m = min(k, len(special))
    rois[:m] = np.asarray(special[:m])
    return torch.from_numpy(rois.astype(F)).to(DEV)


def boxes_as_list(rois, n):
    """the RoIs of valid images as list[Tensor[L_i, 4]], and the [K, 5] rows in that order"""
    r = rois.cpu().numpy()
    lst = [r[r[:, 0] == i, 1:] for i in range(n)]
    flat = np.concatenate([np.concatenate([np.full((len(b), 1), i, F), b], 1) for i, b in enumerate(lst)], 0)
    return [torch.from_numpy(b.copy()).to(DEV) for b in lst], torch.from_numpy(flat).to(DEV)


def fwd_bwd(fn, features, g):
    xs = [f.detach().clone().requires_grad_(True) for f in features]
    y = fn(xs)
    y.backward(g)
    for x, f in zip(xs, features):
        assert x.grad.shape == f.shape and x.grad.stride() == f.stride()
    return y.detach(), [x.grad for x in xs]


def assert_same(a, b):
    ya, ga = a
    yb, gb = b
    assert torch.equal(ya, yb)
    assert len(ga) == len(gb)
    for i, (x, y) in enumerate(zip(ga, gb)):
        assert torch.equal(x, y), "level %d gradient" % i


# ---- bit-identity with the composition --------------------------------------------------------------------------------------------
CASES = [  # (n_levels, n, c, output_size, sampling_ratio, channels_last, as_list)
    (1, 1, 4, (7, 7), 2, False, False),
    (1, 3, 3, (7, 3), -1, True, True),
    (2, 1, 256, (7, 7), 0, True, False),
    (2, 3, 4, (14, 14), 16, False, True),
    (4, 1, 3, (7, 3), 2, (False, True, True, False), False),
    (4, 3, 256, (7, 7), 2, True, True),
    (4, 3, 4, (14, 14), -1, False, False),
    (5, 1, 4, (7, 7), 16, True, True),
    (5, 3, 3, (7, 3), 0, False, False),
    (5, 3, 256, (14, 14), 2, (True, False, True, False, True), True),
]


@pytest.mark.parametrize("n_levels,n,c,size,sr,channels_last,as_list", CASES)
def test_equals_torchvision_composition(n_levels, n, c, size, sr, channels_last, as_list):
    rng = np.random.RandomState(n_levels * 100 + n * 10 + c + sr)
    img_h, img_w = 320, 448
    feats = make_features(rng, n, c, img_h, img_w, n_levels, channels_last)
    rois = make_boxes(rng, 150, n, img_h, img_w)
    boxes = rois
    if as_list:
        boxes, rois = boxes_as_list(rois, n)
    scales = FPN_SCALES[:n_levels]
    g = torch.from_numpy(rng.randn(rois.shape[0], c, *size).astype(F)).to(DEV)
    fused = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, boxes, size, scales, sr), feats, g)
    want = fwd_bwd(lambda xs: composition(xs, rois, size, scales, sr), feats, g)
    assert fused[0].shape == (rois.shape[0], c) + size and fused[0].is_contiguous(memory_format=torch.channels_last)
    assert_same(fused, want)
    if n_levels > 1:
        levels = tv_levels(rois, *tv_level_range(scales))
        for lv in range(n_levels):                       # every level is exercised
            assert int((levels == lv).sum()) > 0, lv
        assert float(fused[1][0].abs().max()) > 0


@pytest.mark.parametrize("n_levels,n,c,size,sr", [(4, 2, 4, 7, 2), (5, 1, 8, 14, -1), (2, 3, 4, 7, 0)])
def test_against_float64_per_level(n_levels, n, c, size, sr):
    rng = np.random.RandomState(7 + n_levels + sr)
    img_h, img_w = 256, 320
    feats = make_features(rng, n, c, img_h, img_w, n_levels, False)
    rois = make_boxes(rng, 40, n, img_h, img_w)
    scales = FPN_SCALES[:n_levels]
    g = rng.randn(rois.shape[0], c, size, size).astype(F)
    y, grads = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, size, scales, sr), feats, torch.from_numpy(g).to(DEV))
    y = y.cpu().numpy()
    levels = tv_levels(rois, *tv_level_range(scales)).cpu().numpy()
    r = rois.cpu().numpy()
    assert (y[levels < 0] == 0).all()
    for lv in range(n_levels):
        sel = levels == lv
        x = feats[lv].detach().cpu().numpy()
        assert sel.any()
        want = align_ref(x, r[sel], size, size, scales[lv], sr, False)
        assert rel(y[sel], want) <= 2e-7
        d = grads[lv].cpu().numpy()
        dwant = align_backward_ref(g[sel], x.shape, r[sel], size, size, scales[lv], sr, False)
        assert rel(d, dwant) <= 2e-6


# ---- levels -------------------------------------------------------------------------------------------------------------------------
def observed_levels(y):
    """each level's map holds the constant level + 1 and every sample lies inside: the pooled value names the level (0: none)"""
    v = y.mean(dim=(1, 2, 3))
    return torch.round(v).to(torch.int64) - 1


def test_level_boundaries_one_float32_step_at_a_time():
    n_levels, scales = 4, FPN_SCALES[:4]
    img = 1024
    feats = [torch.full((1, 4, img // 2 ** (i + 2), img // 2 ** (i + 2)), float(i + 1), device=DEV) for i in range(n_levels)]
    rows = []
    for sb in (112.0, 224.0, 448.0):                     # sqrt(area) boundaries of levels 0|1, 1|2, 2|3 (k_min = 2)
        h = np.float32(sb)
        w = np.float32(sb * (1 - 2e-5))
        for _ in range(700):                             # ~ +-2e-5 relative, one ulp per box
            rows.append([0, 0, 0, w, h])
            w = np.nextafter(w, np.float32(np.inf))
    rows += [[0, 40, 40, 40, 90], [0, 40, 40, 90, 40], [0, 500, 500, 500, 500]]     # zero area: level 0
    rois = torch.from_numpy(np.asarray(rows, F)).to(DEV)
    want = tv_levels(rois, *tv_level_range(scales))
    y = ops.multi_scale_roi_align(feats, rois, 7, scales, 2)
    got = observed_levels(y)
    assert torch.equal(got, want)
    w = want.cpu().numpy()
    for a, b in ((0, 1), (1, 2), (2, 3)):                # the sweeps cross every boundary
        assert (w == a).any() and (w == b).any()
    assert (w[-3:] == 0).all()
    assert torch.equal(y, composition(feats, rois, 7, scales, 2))


def test_inverted_boxes_bad_images_and_boxes_outside():
    rng = np.random.RandomState(11)
    n, c = 2, 4
    feats = make_features(rng, n, c, 256, 256, 4, True)
    rois = torch.tensor([[0, 50, 20, 30, 90],              # inverted x: negative area
                         [1, 20, 90, 80, 30],              # inverted y
                         [0, float("nan"), 0, 10, 10],     # NaN coordinate
                         [2, 0, 0, 100, 100],              # image 2 of 2
                         [-1, 0, 0, 100, 100],
                         [0.5, 0, 0, 100, 100],            # truncated to image 0, as torchvision does
                         [1, -500, -500, -300, -300],      # wholly outside the image
                         [1, 200, 200, 420, 460],          # partly outside
                         [0, 60, 60, 61, 61]], dtype=torch.float32, device=DEV)
    g = torch.from_numpy(rng.randn(rois.shape[0], c, 7, 7).astype(F)).to(DEV)
    fused = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2), feats, g)
    assert_same(fused, fwd_bwd(lambda xs: composition(xs, rois, 7, FPN_SCALES[:4], 2), feats, g))
    y = fused[0]
    assert (y[:5] == 0).all() and (y[5] != 0).any() and (y[7] != 0).any()
    # the zero-gradient rows: the inverted, NaN and bad-image RoIs send nothing
    g2 = g.clone()
    g2[5:] = 0
    _, grads = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2), feats, g2)
    assert all(float(d.abs().max()) == 0 for d in grads)


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_no_rois():
    rng = np.random.RandomState(1)
    feats = make_features(rng, 2, 4, 128, 128, 4, False)
    for boxes in (torch.zeros((0, 5), device=DEV), [torch.zeros((0, 4), device=DEV)] * 2):
        y, grads = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, boxes, 7, FPN_SCALES[:4], 2), feats,
                           torch.zeros((0, 4, 7, 7), device=DEV))
        assert y.shape == (0, 4, 7, 7)
        assert all(torch.equal(d, torch.zeros_like(d)) for d in grads)


def test_a_level_without_rois_gets_exact_zeros():
    rng = np.random.RandomState(2)
    feats = make_features(rng, 2, 4, 256, 256, 4, (True, False, True, False))
    rois = torch.tensor([[0, 10, 10, 50, 60], [1, 0, 0, 90, 80], [0, 30, 40, 500, 520]], dtype=torch.float32, device=DEV)
    levels = tv_levels(rois, 2, 5).tolist()
    assert levels == [0, 0, 3]                           # levels 1 and 2 empty
    g = torch.randn((3, 4, 7, 7), device=DEV)
    fused = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2), feats, g)
    assert_same(fused, fwd_bwd(lambda xs: composition(xs, rois, 7, FPN_SCALES[:4], 2), feats, g))
    assert torch.equal(fused[1][1], torch.zeros_like(fused[1][1])) and torch.equal(fused[1][2], torch.zeros_like(fused[1][2]))
    assert float(fused[1][0].abs().max()) > 0 and float(fused[1][3].abs().max()) > 0


def test_more_than_1024_rois_over_one_tile():
    rng = np.random.RandomState(3)
    feats = make_features(rng, 1, 8, 256, 256, 4, True)
    one = [[0, 40.25, 50.5, 100.75, 120.125], [0, 20, 20, 300, 280]]   # a level-0 and a level-2 RoI, 1500 copies each, interleaved
    rois = torch.tensor(one * 1500, dtype=torch.float32, device=DEV)
    g = torch.from_numpy(rng.randn(3000, 8, 7, 7).astype(F)).to(DEV)
    fused = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2), feats, g)
    assert_same(fused, fwd_bwd(lambda xs: composition(xs, rois, 7, FPN_SCALES[:4], 2), feats, g))
    assert_same(fused, fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2), feats, g))


def test_levels_given_coarsest_first_pool_to_zeros():
    rng = np.random.RandomState(4)
    feats = make_features(rng, 2, 4, 256, 256, 4, False)[::-1]
    scales = FPN_SCALES[:4][::-1]
    assert tv_level_range(scales) == (5, 2)
    rois = make_boxes(rng, 50, 2, 256, 256)
    g = torch.randn((50, 4, 7, 7), device=DEV)
    fused = fwd_bwd(lambda xs: ops.multi_scale_roi_align(xs, rois, 7, scales, 2), feats, g)
    assert_same(fused, fwd_bwd(lambda xs: composition(xs, rois, 7, scales, 2), feats, g))
    assert torch.equal(fused[0], torch.zeros_like(fused[0]))
    assert all(torch.equal(d, torch.zeros_like(d)) for d in fused[1])


def test_deterministic_and_no_host_sync():
    rng = np.random.RandomState(5)
    feats = make_features(rng, 2, 256, 320, 448, 4, True)
    rois = make_boxes(rng, 400, 2, 320, 448)
    g = torch.from_numpy(rng.randn(400, 256, 7, 7).astype(F)).to(DEV)
    xs = [[f.detach().clone().requires_grad_(True) for f in feats] for _ in range(2)]
    torch.cuda.synchronize()
    outs = []
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x in xs:
            y = ops.multi_scale_roi_align(x, rois, 7, FPN_SCALES[:4], 2)
            y.backward(g)
            outs.append(y.detach())
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(outs[0], outs[1])
    for a, b in zip(xs[0], xs[1]):
        assert torch.equal(a.grad, b.grad)


# ---- op contracts -------------------------------------------------------------------------------------------------------------------
OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck():
    rng = np.random.RandomState(9)
    feats = make_features(rng, 2, 6, 96, 128, 3, (False, True, False), requires_grad=True)
    rois = make_boxes(rng, 20, 2, 96, 128)
    args = (feats, rois, FPN_SCALES[:3], 7, 3, 2, 224.0, 4.0, 2, 4)
    torch.library.opcheck(torch.ops.frcnn.multi_scale_roi_align.default, args, test_utils=OPCHECK)
    g = torch.from_numpy(rng.randn(20, 6, 7, 3).astype(F)).to(DEV)
    torch.library.opcheck(torch.ops.frcnn.multi_scale_roi_align_backward.default,
                          (g, rois, FPN_SCALES[:3], 7, 3, 2, 224.0, 4.0, 2, 4, 2, 6, [f.shape[2] for f in feats],
                           [f.shape[3] for f in feats], [False, True, False]), test_utils=OPCHECK)


def test_double_backward_raises():
    feats = [torch.randn((1, 4, 16, 16), device=DEV, requires_grad=True), torch.randn((1, 4, 8, 8), device=DEV, requires_grad=True)]
    rois = torch.tensor([[0, 0, 0, 30, 30], [0, 0, 0, 60, 50]], dtype=torch.float32, device=DEV)
    y = ops.multi_scale_roi_align(feats, rois, 2, [1 / 4, 1 / 8])
    v = torch.ones_like(y, requires_grad=True)
    g = torch.autograd.grad(y, feats, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        (g[0].sum() + g[1].sum()).backward()


# ---- the module, as torchvision's FPN detectors call it ---------------------------------------------------------------------------
def test_module_drop_in_for_fpn():
    rng = np.random.RandomState(6)
    n, c = 2, 256
    x = OrderedDict()
    for name, (h, w) in zip(["0", "1", "2", "3", "pool"], [(200, 304), (100, 152), (50, 76), (25, 38), (13, 19)]):
        x[name] = torch.from_numpy(rng.randn(n, c, h, w).astype(F)).to(DEV)
    boxes = [make_boxes(rng, 300, 1, 800, 1216)[:, 1:].contiguous() for _ in range(n)]
    m = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    y = m(x, boxes, [(800, 1216), (800, 1216)])
    assert m.scales == [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    want = ops.multi_scale_roi_align([x["0"], x["1"], x["2"], x["3"]], boxes, 7, [1 / 4, 1 / 8, 1 / 16, 1 / 32], 2)
    assert torch.equal(y, want)
    assert torch.equal(y, composition([x["0"], x["1"], x["2"], x["3"]], as_rois(boxes), 7, m.scales, 2))
