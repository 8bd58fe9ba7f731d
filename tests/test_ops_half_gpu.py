"""fasterrcnn_amd.ops on float16 / bfloat16 maps on the GPU.

The contract (torchvision's autocast definition): for T in {float16, bfloat16} and f32op the float32 operator,
    op(x_T, boxes) == f32op(x_T.float(), boxes).to(T)   and   dx_T == f32op_backward(grad_T.float()).to(T),   bit for bit.
Two gates.  The primary one compares bit patterns with the float32 path on the widened tensors (that path is pinned to the oracle by
tests/test_ops_gpu.py and tests/test_ops_multiscale_gpu.py; the 16-bit code is never its own reference).  The independent one compares
with the CPU restatements of tests/test_ops_gpu.py on the widened values: the float32 tolerances used there (2e-7 forward, 2e-6 backward,
of the largest magnitude) plus one rounding to T, u = 2**-11 (float16: 11 significant bits) or 2**-8 (bfloat16: 8) -- derived from the
formats, not measured."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fasterrcnn_amd import ops
from tests.test_ops_gpu import align_backward_ref, align_ref, boxes_arg, make_rois, pool_ref, rel
from tests.test_ops_multiscale_gpu import FPN_SCALES, make_boxes, tv_level_range, tv_levels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CL = torch.channels_last
HALF = [torch.float16, torch.bfloat16]
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}          # one rounding to nearest
OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def bits(t):
    assert t.dtype in HALF
    return t.contiguous().view(torch.int16)


def assert_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(bits(got), bits(want)), what


def half_input(values, dtype, channels_last):
    """float32 numpy values rounded to dtype on the GPU, in the requested memory format."""
    t = torch.from_numpy(values).to(DEV).to(dtype)
    return t.contiguous(memory_format=CL) if channels_last else t


def run(fn, xs, g):
    """fn on fresh leaves of xs, backward of g: (y, [dx])."""
    leaves = [x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for x in xs]
    y = fn(leaves)
    y.backward(g)
    for x, leaf in zip(xs, leaves):
        assert leaf.grad.dtype == x.dtype and leaf.grad.shape == x.shape and leaf.grad.stride() == x.stride()
    return y.detach(), [leaf.grad for leaf in leaves]


def widened(fn, xs, g):
    """The float32 operator on the widened tensors, rounded once: the right-hand side of the contract."""
    dtype = xs[0].dtype
    y, dxs = run(fn, [x.float() for x in xs], g.float())
    assert y.dtype == torch.float32
    return y.to(dtype), [d.to(dtype) for d in dxs]


def assert_contract(fn, xs, g):
    y, dxs = run(fn, xs, g)
    assert y.dtype == xs[0].dtype and y.is_contiguous(memory_format=CL)
    yw, dw = widened(fn, xs, g)
    assert_bits(y, yw, "forward")
    for i, (a, b) in enumerate(zip(dxs, dw)):
        assert_bits(a, b, "gradient of map %d" % i)
    return y, dxs


# ---- 4. primary gate: bit for bit the float32 operator on the widened tensors -------------------------------------------------------
SINGLE = [  # (n, c, h, w, k, output_size, scale, sampling_ratio, aligned, channels_last, as_list)
    (2, 256, 25, 38, 40, (7, 7), 1 / 16, 2, False, True, False),
    (1, 1024, 14, 14, 12, (7, 7), 1 / 16, -1, True, False, True),
    (3, 6, 20, 31, 30, (7, 3), 0.5, 0, False, False, False),            # 6 channels: the zero-padded copy
    (2, 12, 17, 23, 30, (5, 9), 0.25, 3, True, True, True),             # 12 channels
    (2, 8, 10, 12, 20, (2, 2), 1.0, 16, False, False, False),
    (1, 512, 37, 62, 60, (7, 7), 1 / 16, 2, True, True, False),
]


def single_case(case, dtype, seed):
    n, c, h, w, k, size, scale, sr, aligned, channels_last, as_list = case
    rng = np.random.RandomState(seed)
    x = half_input(rng.randn(n, c, h, w).astype(F), dtype, channels_last)
    boxes, rois_used = boxes_arg(make_rois(rng, k, n, h, w, scale), n, as_list)      # a RoI of image n (out of range) unless as_list
    g = half_input(rng.randn(rois_used.shape[0], c, size[0], size[1]).astype(F), dtype, True)
    return x, boxes, rois_used, g


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", SINGLE)
def test_roi_align_equals_float32_op_rounded(case, dtype):
    x, boxes, _, g = single_case(case, dtype, 11)
    size, scale, sr, aligned = case[5], case[6], case[7], case[8]
    assert_contract(lambda xs: ops.roi_align(xs[0], boxes, size, scale, sr, aligned), [x], g)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", SINGLE)
def test_roi_pool_equals_float32_op_rounded(case, dtype):
    x, boxes, _, g = single_case(case, dtype, 12)
    size, scale = case[5], case[6]
    assert_contract(lambda xs: ops.roi_pool(xs[0], boxes, size, scale), [x], g)
    rois = ops._roi_input(x, boxes)
    _, a16 = torch.ops.frcnn.roi_pool(x, rois, scale, *size)
    _, a32 = torch.ops.frcnn.roi_pool(x.float(), rois, scale, *size)
    assert a16.dtype == torch.int32 and torch.equal(a16, a32)            # widening is monotone: the float32 op's argmax


MULTI = [  # (n_levels, n, c, output_size, sampling_ratio, channels_last, as_list)
    (1, 1, 8, (7, 7), 2, False, False),
    (2, 3, 6, (7, 3), -1, True, True),
    (4, 2, 256, (7, 7), 2, True, False),
    (4, 3, 12, (14, 14), 0, (False, True, True, False), True),
    (5, 1, 256, (7, 7), 2, False, False),
]


def pyramid_case(case, dtype, seed, img=(160, 224), k=60):
    n_levels, n, c, size, sr, channels_last, as_list = case
    rng = np.random.RandomState(seed)
    feats = []
    for i in range(n_levels):
        h, w = -(-img[0] // 2 ** (i + 2)), -(-img[1] // 2 ** (i + 2))
        cl = channels_last if isinstance(channels_last, bool) else channels_last[i]
        feats.append(half_input(rng.randn(n, c, h, w).astype(F), dtype, cl))
    rois = make_boxes(rng, k, n, *img)                                  # inverted, zero-area, out-of-range-image rows included
    boxes = rois
    if as_list:
        r = rois.cpu().numpy()
        boxes = [torch.from_numpy(r[r[:, 0] == i, 1:].copy()).to(DEV) for i in range(n)]
    kk = rois.shape[0] if not as_list else sum(b.shape[0] for b in boxes)
    g = half_input(rng.randn(kk, c, size[0], size[1]).astype(F), dtype, True)
    return feats, boxes, g


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", MULTI)
def test_multi_scale_roi_align_equals_float32_op_rounded(case, dtype):
    feats, boxes, g = pyramid_case(case, dtype, 13)
    n_levels, size, sr = case[0], case[3], case[4]
    assert_contract(lambda xs: ops.multi_scale_roi_align(xs, boxes, size, FPN_SCALES[:n_levels], sr), feats, g)


@pytest.mark.parametrize("dtype", HALF)
def test_same_dtype_boxes_are_widened_on_the_host(dtype):
    """Boxes in the map's own 16-bit dtype pool exactly as their float32 widening does."""
    rng = np.random.RandomState(14)
    x = half_input(rng.randn(2, 8, 12, 16).astype(F), dtype, False)
    rois = torch.from_numpy(make_rois(rng, 12, 2, 12, 16, 0.5)).to(DEV).to(dtype)
    assert_bits(ops.roi_align(x, rois, 5, 0.5, 2), ops.roi_align(x, rois.float(), 5, 0.5, 2))
    assert_bits(ops.roi_pool(x, rois, 5, 0.5), ops.roi_pool(x, rois.float(), 5, 0.5))
    lst = [rois[rois[:, 0] == i, 1:] for i in range(2)]
    assert_bits(ops.multi_scale_roi_align([x, x[:, :, ::2, ::2]], lst, 5, [0.5, 0.25], 2),
                ops.multi_scale_roi_align([x, x[:, :, ::2, ::2]], [b.float() for b in lst], 5, [0.5, 0.25], 2))


def special_values(rng, shape, dtype):
    """randn with NaN, +inf, -inf, zeros, subnormals of dtype and of float16, and the largest finite values sprinkled in."""
    v = rng.randn(*shape).astype(F)
    flat = v.reshape(-1)
    tiny = float(torch.finfo(dtype).smallest_normal)
    picks = [np.nan, np.inf, -np.inf, 0.0, -0.0, tiny / 4, -tiny / 8, 2.0 ** -24, 3 * 2.0 ** -24, -2.0 ** -20,
             float(torch.finfo(dtype).max), -float(torch.finfo(dtype).max), 65504.0, 1e-40, -1e-42]
    idx = rng.choice(flat.size, size=min(flat.size // 6, 40 * len(picks)), replace=False)
    for j, i in enumerate(idx):
        flat[i] = picks[j % len(picks)]
    return v


@pytest.mark.parametrize("dtype", HALF)
def test_nan_inf_and_subnormals_convert_as_tensor_to(dtype):
    rng = np.random.RandomState(15)
    n, c, h, w, scale = 2, 16, 12, 14, 0.5
    x = half_input(special_values(rng, (n, c, h, w), dtype), dtype, True)
    assert torch.isnan(x).any() and torch.isinf(x).any()
    rois = torch.from_numpy(make_rois(rng, 24, n, h, w, scale)).to(DEV)
    g = half_input(special_values(rng, (24, c, 7, 5), dtype), dtype, True)
    y, _ = assert_contract(lambda xs: ops.roi_align(xs[0], rois, (7, 5), scale, 2, False), [x], g)
    assert torch.isnan(y).any()
    assert_contract(lambda xs: ops.roi_pool(xs[0], rois, (7, 5), scale), [x], g)
    boxes = make_boxes(rng, 24, n, 24, 28)
    assert_contract(lambda xs: ops.multi_scale_roi_align(xs, boxes, (7, 5), [0.5, 0.25], 2), [x, x[:, :, ::2, ::2].contiguous()], g)


# ---- 5. independent gate: the CPU restatements on the widened values --------------------------------------------------------------------
SMALL = [  # (n, c, h, w, k, output_size, scale, sampling_ratio, aligned, channels_last, as_list)
    (2, 8, 13, 17, 14, (7, 7), 0.25, 2, False, True, False),
    (3, 5, 10, 9, 12, (3, 5), 0.5, -1, True, False, True),
    (1, 16, 9, 11, 10, (4, 4), 1.0, 3, True, False, False),
]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", SMALL)
def test_roi_align_against_cpu_restatement(case, dtype):
    n, c, h, w, k, size, scale, sr, aligned, channels_last, as_list = case
    x, boxes, rois_used, g = single_case(case, dtype, 16)
    y, (dx,) = run(lambda xs: ops.roi_align(xs[0], boxes, size, scale, sr, aligned), [x], g)
    u = UNIT[dtype]
    xw, gw = x.float().cpu().numpy(), g.float().cpu().numpy()                      # widened on the CPU: exact
    assert float(np.abs(xw).max()) < 60000 and float(np.abs(gw).max()) < 60000     # float16's range: no overflow enters
    e_fwd = rel(y.float().cpu().numpy(), align_ref(xw, rois_used, size[0], size[1], scale, sr, aligned))
    e_bwd = rel(dx.float().cpu().numpy(), align_backward_ref(gw, x.shape, rois_used, size[0], size[1], scale, sr, aligned))
    print("roi_align %s %s: forward %.3e (bound %.3e), backward %.3e (bound %.3e)" % (dtype, case[:5], e_fwd, 2e-7 + u, e_bwd, 2e-6 + u))
    assert e_fwd <= 2e-7 + u
    assert e_bwd <= 2e-6 + u


@pytest.mark.parametrize("dtype", HALF)
def test_multi_scale_against_cpu_restatement_per_level(dtype):
    case = (3, 2, 8, (7, 7), 2, (True, False, True), False)
    feats, rois, g = pyramid_case(case, dtype, 17, img=(96, 128), k=30)
    scales = FPN_SCALES[:3]
    y, dxs = run(lambda xs: ops.multi_scale_roi_align(xs, rois, (7, 7), scales, 2), feats, g)
    levels = tv_levels(rois, *tv_level_range(scales)).cpu().numpy()
    r = rois.cpu().numpy()
    yn, gw, u = y.float().cpu().numpy(), g.float().cpu().numpy(), UNIT[dtype]
    for l, (f, s) in enumerate(zip(feats, scales)):
        idx = np.where(levels == l)[0]
        assert len(idx)
        want = align_ref(f.float().cpu().numpy(), r[idx], 7, 7, s, 2, False)
        e_fwd = rel(yn[idx], want)
        e_bwd = rel(dxs[l].float().cpu().numpy(), align_backward_ref(gw[idx], f.shape, r[idx], 7, 7, s, 2, False))
        print("multi_scale %s level %d: forward %.3e, backward %.3e" % (dtype, l, e_fwd, e_bwd))
        assert e_fwd <= 2e-7 + u
        assert e_bwd <= 2e-6 + u
    assert not yn[levels < 0].any()


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("channels_last,as_list", [(False, False), (True, True)])
def test_roi_pool_against_cpu_restatement(dtype, channels_last, as_list):
    rng = np.random.RandomState(18)
    n, c, h, w, scale, size = 2, 6, 20, 32, 1 / 16, (7, 3)
    xv = rng.randn(n, c, h, w).astype(F)
    xv[:, :, 3:9, 4:12] = 0.25                                          # ties: the first maximum in scan order
    x = half_input(xv, dtype, channels_last)
    boxes, rois_used = boxes_arg(make_rois(rng, 12, n, h, w, scale), n, as_list)
    want, arg = pool_ref(x.float().cpu().numpy(), rois_used, size[0], size[1], scale)
    g = half_input((rng.rand(*want.shape) + 0.5).astype(F), dtype, True)   # positive: no cancellation hides a cell
    y, (dx,) = run(lambda xs: ops.roi_pool(xs[0], boxes, size, scale), [x], g)
    assert np.array_equal(y.float().cpu().numpy(), want)
    d = np.zeros((n, c, h * w), np.float64)
    gw = g.float().cpu().numpy()
    for r in range(rois_used.shape[0]):
        if not (-1 < rois_used[r, 0] < n):
            continue
        for ch in range(c):
            a = arg[r, ch].ravel()
            np.add.at(d[int(rois_used[r, 0]), ch], a[a >= 0], gw[r, ch].ravel()[a >= 0].astype(np.float64))
    d = d.reshape(x.shape)
    dxn = dx.float().cpu().numpy()
    assert np.array_equal(dxn == 0, d == 0)
    assert rel(dxn, d) <= 1e-5 + UNIT[dtype]


# ---- 6. more than OPS_LIST = 1024 RoIs over one tile: the running sum must not pass through 16-bit memory ---------------------------
@pytest.mark.parametrize("dtype", HALF)
def test_more_than_1024_rois_over_one_tile_roi_align(dtype):
    rng = np.random.RandomState(19)
    x = half_input(rng.randn(2, 8, 16, 16).astype(F), dtype, True)
    k = 2600                                                            # three culling passes for the tiles under the boxes
    inset = np.linspace(0.0, 1.5, k).astype(F)                          # nested boxes of image 1 around the tile (6..7, 6..7)
    rois = np.stack([np.ones(k, F), 4 + inset, 4 + inset, 10 - inset, 10 - inset], 1)
    rois[::7] = rois[0]                                                 # and identical ones
    rois = torch.from_numpy(rois).to(DEV)
    g = half_input(rng.randn(k, 8, 7, 7).astype(F), dtype, True)
    fn = lambda xs: ops.roi_align(xs[0], rois, 7, 1.0, 2, True)        # noqa: E731
    _, (dx,) = assert_contract(fn, [x], g)
    assert float(dx[1].float().abs().max()) > 0 and not dx[0].any()
    assert_bits(run(fn, [x], g)[1][0], dx, "run to run")


@pytest.mark.parametrize("dtype", HALF)
def test_more_than_1024_rois_over_one_tile_multi_scale(dtype):
    rng = np.random.RandomState(20)
    feats = [half_input(rng.randn(1, 8, 256 >> (i + 2), 256 >> (i + 2)).astype(F), dtype, True) for i in range(4)]
    one = [[0, 40.25, 50.5, 100.75, 120.125], [0, 20, 20, 300, 280]]    # a level-0 and a level-2 RoI, 1500 copies each, interleaved
    rois = torch.tensor(one * 1500, dtype=torch.float32, device=DEV)
    g = half_input(rng.randn(3000, 8, 7, 7).astype(F), dtype, True)
    fn = lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2)      # noqa: E731
    _, dxs = assert_contract(fn, feats, g)
    assert dxs[0].any() and dxs[2].any() and not dxs[1].any() and not dxs[3].any()
    for a, b in zip(run(fn, feats, g)[1], dxs):
        assert_bits(a, b, "run to run")


@pytest.mark.parametrize("dtype", HALF)
def test_more_than_1024_rois_over_one_tile_roi_pool(dtype):
    rng = np.random.RandomState(21)
    x = half_input(rng.randn(1, 8, 12, 12).astype(F), dtype, False)
    rois = torch.tensor([[0, 2, 2, 9, 9], [0, 3, 1, 8, 10]] * 1300, dtype=torch.float32, device=DEV)
    g = half_input(rng.randn(2600, 8, 3, 3).astype(F), dtype, True)
    assert_contract(lambda xs: ops.roi_pool(xs[0], rois, 3, 1.0), [x], g)


# ---- 7. run to run ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF)
def test_backward_is_bit_identical_from_run_to_run(dtype):
    x, boxes, _, g = single_case(SINGLE[0], dtype, 22)
    feats, rois, gm = pyramid_case(MULTI[2], dtype, 22)
    for fn, xs, gg in ((lambda xs: ops.roi_align(xs[0], boxes, 7, 1 / 16, 2), [x], g),
                       (lambda xs: ops.roi_pool(xs[0], boxes, 7, 1 / 16), [x], g),
                       (lambda xs: ops.multi_scale_roi_align(xs, rois, 7, FPN_SCALES[:4], 2), feats, gm)):
        ya, da = run(fn, xs, gg)
        yb, db = run(fn, xs, gg)
        assert_bits(ya, yb)
        for a, b in zip(da, db):
            assert_bits(a, b)


# ---- 8. the autocast call pattern of an FPN detector ------------------------------------------------------------------------------------
class TinyFPNHead(torch.nn.Module):
    """conv -> two-level pyramid -> pooler -> linear head; `pool` maps (features, boxes, image_shapes) to the pooled tensor."""

    def __init__(self, pool):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.fc = torch.nn.Linear(8 * 5 * 5, 4)
        self.pool = pool
        self.pooled_dtype = None

    def forward(self, images, boxes):
        f0 = torch.nn.functional.max_pool2d(torch.relu(self.conv(images)), 4)
        feats = OrderedDict([("0", f0), ("1", torch.nn.functional.max_pool2d(f0, 2))])
        pooled = self.pool(feats, boxes, [tuple(images.shape[2:])] * images.shape[0])
        self.pooled_dtype = pooled.dtype
        return self.fc(pooled.flatten(1))


@pytest.mark.parametrize("dtype", HALF)
def test_autocast_call_pattern(dtype):
    rng = np.random.RandomState(23)
    images = torch.from_numpy(rng.randn(2, 3, 64, 96).astype(F)).to(DEV)
    boxes = [torch.tensor([[4, 6, 40, 50], [10, 2, 90, 60], [30, 30, 44, 41]], dtype=torch.float32, device=DEV),
             torch.tensor([[0, 0, 95, 63], [50, 20, 70, 45]], dtype=torch.float32, device=DEV)]
    scales = [1 / 4, 1 / 8]

    def composed(feats, bxs, image_shapes):                             # what a user had to write before: widen, float32 op, round
        fs = list(feats.values())
        return ops.multi_scale_roi_align([f.float() for f in fs], bxs, 5, scales, 2).to(fs[0].dtype)

    grads = []
    for pool in (ops.MultiScaleRoIAlign(["0", "1"], 5, 2), composed):
        torch.manual_seed(0)
        model = TinyFPNHead(pool).to(DEV)
        with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            with torch.autocast("cuda", dtype=dtype):
                out = model(images, boxes)
                loss = out.float().square().mean()
            loss.backward()
        assert model.pooled_dtype == dtype
        if isinstance(pool, ops.MultiScaleRoIAlign):
            assert pool.scales == scales
        gs = [p.grad for p in model.parameters()]
        assert all(g is not None and torch.isfinite(g).all() for g in gs)
        assert float(model.conv.weight.grad.abs().max()) > 0
        grads.append((out.detach(), gs))
    assert torch.equal(grads[0][0], grads[1][0])
    for a, b in zip(grads[0][1], grads[1][1]):
        assert torch.equal(a, b)


# ---- 9. opcheck -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF)
def test_opcheck_every_roi_op(dtype):
    rng = np.random.RandomState(24)
    x = half_input(rng.randn(2, 8, 10, 12).astype(F), dtype, False).requires_grad_(True)
    rois = torch.from_numpy(make_rois(rng, 6, 2, 10, 12, 0.5)).to(DEV)
    torch.library.opcheck(torch.ops.frcnn.roi_align.default, (x, rois, 0.5, 7, 3, 2, False), test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.roi_pool.default, (x, rois, 0.5, 7, 3), test_utils=OPCHECK)
    g = half_input(rng.randn(6, 8, 7, 3).astype(F), dtype, False)
    torch.library.opcheck(torch.ops.frcnn.roi_align_backward.default, (g, rois, 0.5, 7, 3, 2, False, 2, 8, 10, 12, True),
                          test_utils=OPCHECK)
    _, argmax = torch.ops.frcnn.roi_pool.default(x.detach(), rois, 0.5, 7, 3)
    torch.library.opcheck(torch.ops.frcnn.roi_pool_backward.default, (g, rois, argmax, 0.5, 7, 3, 2, 8, 10, 12, False),
                          test_utils=OPCHECK)
    feats = [half_input(rng.randn(2, 6, 96 >> (i + 2), 128 >> (i + 2)).astype(F), dtype, i == 1).requires_grad_(True) for i in range(3)]
    boxes = make_boxes(rng, 20, 2, 96, 128)
    torch.library.opcheck(torch.ops.frcnn.multi_scale_roi_align.default, (feats, boxes, FPN_SCALES[:3], 7, 3, 2, 224.0, 4.0, 2, 4),
                          test_utils=OPCHECK)
    gm = half_input(rng.randn(20, 6, 7, 3).astype(F), dtype, False)
    torch.library.opcheck(torch.ops.frcnn.multi_scale_roi_align_backward.default,
                          (gm, boxes, FPN_SCALES[:3], 7, 3, 2, 224.0, 4.0, 2, 4, 2, 6, [f.shape[2] for f in feats],
                           [f.shape[3] for f in feats], [False, True, False]), test_utils=OPCHECK)
