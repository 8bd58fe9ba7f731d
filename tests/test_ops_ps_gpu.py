"""fasterrcnn_amd.ops.ps_roi_align / ps_roi_pool on the GPU against the numpy restatements of torchvision (tests/ps_roi_cases.py).

Bounds are the project's RoI bounds (tests/test_roialign_gpu.py, tests/test_ops_gpu.py): ps_roi_align forward (float32, the restatement's
operation order) <= 2e-7 of max|y| with the NaN positions of the degenerate RoIs coinciding; both backward passes against the float64
accumulation of the same plan <= 2e-6 of max|d| and bit-identical from run to run.  ps_roi_pool's kernel keeps torchvision's scan-order
float32 sum, so its forward is compared exactly with the float32 restatement.  16-bit maps: op(x_T) == op(x_T.float()).to(T) bit for
bit, forward and backward."""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import ops

from tests import ps_roi_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CL = torch.channels_last


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def gpu(x, channels_last=False):
    t = torch.from_numpy(x).to(DEV)
    return t.contiguous(memory_format=CL) if channels_last else t


def boxes_arg(rois, n_img, as_list):
    """rois as the op's boxes argument, and the rows in the order the op sees them (a list cannot name an image out of range)."""
    if not as_list:
        return torch.from_numpy(rois).to(DEV), rois
    keep = (rois[:, 0] >= 0) & (rois[:, 0] < n_img) & (rois[:, 0] == np.floor(rois[:, 0]))
    order = np.argsort(rois[:, 0] + (~keep) * 1e9, kind="stable")[: int(keep.sum())]
    lst = [torch.from_numpy(rois[order][rois[order][:, 0] == i, 1:].copy()).to(DEV) for i in range(n_img)]
    return lst, rois[order]


def diagonal(y, oh, ow):
    k, c = y.shape[:2]
    co = c // (oh * ow)
    ph, pw = torch.meshgrid(torch.arange(oh, device=y.device), torch.arange(ow, device=y.device), indexing="ij")
    ci = (torch.arange(co, device=y.device)[:, None, None] * oh + ph[None]) * ow + pw[None]
    return y[:, ci, ph[None], pw[None]]


# (output size, output channels, images, scale, map height, map width)
SHAPES = [((7, 7), 2, 1, 1 / 16, 12, 17), ((3, 5), 3, 3, 1 / 16, 13, 11), ((1, 1), 5, 3, 1.0, 9, 14), ((7, 7), 1, 3, 1.0, 15, 10),
          ((2, 3), 4, 1, 1.0, 10, 12)]
ALIGN_CASES = [(size, co, n, scale, h, w, sr, bool((i + j) % 2), bool(i % 2))
               for i, (size, co, n, scale, h, w) in enumerate(SHAPES) for j, sr in enumerate((-1, 1, 2))]


# ---- 1. ps_roi_align forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,co,n_img,scale,h,w,sr,as_list,channels_last", ALIGN_CASES)
def test_ps_roi_align_forward(size, co, n_img, scale, h, w, sr, as_list, channels_last):
    oh, ow = size
    rng = np.random.RandomState(oh * 31 + ow * 7 + sr + n_img)
    x = rng.randn(n_img, co * oh * ow, h, w).astype(F)
    boxes, rois = boxes_arg(P.make_rois(rng, 48, n_img, h, w, scale), n_img, as_list)
    y = ops.ps_roi_align(gpu(x, channels_last), boxes, size, scale, sr)
    assert y.shape == (rois.shape[0], co, oh, ow) and y.is_contiguous() and y.dtype == torch.float32
    got = y.cpu().numpy()
    want = P.ps_roi_align(x, rois, oh, ow, scale, sr)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)                           # 0.0f / 0 of the degenerate RoIs, nowhere else
    assert nan.any() == (sr <= 0)
    err = rel(np.where(nan, 0, got), np.where(nan, 0, want))
    print("ps_roi_align forward %s sr %d: %.3g of max|y|" % (size, sr, err))
    assert err <= 2e-7
    bad = ~((rois[:, 0] > -1) & (rois[:, 0] < n_img))
    assert bad.any() == (not as_list) and not got[bad].any()
    # beside roi_align(aligned=True) on the diagonal, on the GPU: the same values wherever the RoI has a width and a height
    keep = P.nondegenerate(rois, scale)
    share = keep.mean()
    print("compared with ops.roi_align(aligned=True) on the diagonal: %.1f %% of the RoIs" % (100 * share))
    assert share >= 0.9
    ref = diagonal(ops.roi_align(gpu(x), torch.from_numpy(rois[keep]).to(DEV), size, scale, sr, aligned=True), oh, ow)
    assert rel(got[keep], ref.cpu().numpy()) <= 2e-7


# ---- 2. ps_roi_pool forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,co,n_img,scale,h,w", SHAPES)
@pytest.mark.parametrize("as_list", [False, True])
def test_ps_roi_pool_forward_is_the_scan_order_sum(size, co, n_img, scale, h, w, as_list):
    oh, ow = size
    rng = np.random.RandomState(oh * 13 + ow + n_img)
    x = rng.randn(n_img, co * oh * ow, h, w).astype(F)
    boxes, rois = boxes_arg(P.make_rois(rng, 48, n_img, h, w, scale), n_img, as_list)
    y = ops.ps_roi_pool(gpu(x, as_list), boxes, size, scale)
    assert y.shape == (rois.shape[0], co, oh, ow) and y.is_contiguous()
    got = y.cpu().numpy()
    want = P.ps_roi_pool(x, rois, oh, ow, scale)
    assert np.array_equal(got, want)
    empty = np.zeros(want.shape, bool)
    for r in range(rois.shape[0]):
        for (ph, pw), (hs, he, ws, we) in P.pool_windows(h, w, rois[r, 1:], oh, ow, scale).items():
            empty[r, :, ph, pw] = he <= hs or we <= ws or P.image_of(rois[r], n_img) is None
    assert empty.any() and not got[empty].any() and not np.signbit(got[empty]).any()
    assert np.abs(got[~empty]).max() > 0.1


# ---- 3. the backward passes -------------------------------------------------------------------------------------------------------------
BWD_CASES = [(size, co, n, scale, h, w, (-1, 2, 1)[i % 3], bool(i % 2)) for i, (size, co, n, scale, h, w) in enumerate(SHAPES)]


@pytest.mark.parametrize("size,co,n_img,scale,h,w,sr,channels_last", BWD_CASES)
def test_ps_roi_align_backward(size, co, n_img, scale, h, w, sr, channels_last):
    oh, ow = size
    rng = np.random.RandomState(oh * 5 + ow * 3 + sr + 100)
    x = rng.randn(n_img, co * oh * ow, h, w).astype(F)
    rois = P.make_rois(rng, 48, n_img, h, w, scale)
    g = rng.randn(rois.shape[0], co, oh, ow).astype(F)
    xt = gpu(x, channels_last).requires_grad_(True)
    boxes = torch.from_numpy(rois).to(DEV)
    grads = []
    for _ in range(2):
        xt.grad = None
        ops.ps_roi_align(xt, boxes, size, scale, sr).backward(gpu(g))
        grads.append(xt.grad.clone())
    assert torch.equal(grads[0], grads[1])                               # a gather in a fixed order: the same bits every run
    assert grads[0].stride() == xt.stride() and grads[0].dtype == torch.float32
    got = grads[0].cpu().numpy()
    assert np.isfinite(got).all()                                        # a degenerate RoI (NaN forward) sends nothing
    want = P.ps_roi_align_backward(g, x.shape, rois, oh, ow, scale, sr)
    err = rel(got, want)
    print("ps_roi_align backward %s sr %d: %.3g of max|d|" % (size, sr, err))
    assert err <= 2e-6 and np.abs(want).max() > 0.1
    # only the RoIs that send anything: a bad batch index, and under an adaptive grid the degenerate RoIs, change nothing
    sends = (rois[:, 0] > -1) & (rois[:, 0] < n_img)
    if sr <= 0:
        sends &= P.nondegenerate(rois, scale)
    assert not sends.all()
    xt.grad = None
    ops.ps_roi_align(xt, boxes[torch.from_numpy(sends).to(DEV)], size, scale, sr).backward(gpu(g[sends]))
    assert torch.equal(xt.grad, grads[0])


@pytest.mark.parametrize("size,co,n_img,scale,h,w,sr,channels_last", BWD_CASES)
def test_ps_roi_pool_backward(size, co, n_img, scale, h, w, sr, channels_last):
    oh, ow = size
    rng = np.random.RandomState(oh * 5 + ow * 3 + 200)
    x = rng.randn(n_img, co * oh * ow, h, w).astype(F)
    rois = P.make_rois(rng, 48, n_img, h, w, scale)
    g = rng.randn(rois.shape[0], co, oh, ow).astype(F)
    xt = gpu(x, channels_last).requires_grad_(True)
    boxes = torch.from_numpy(rois).to(DEV)
    grads = []
    for _ in range(2):
        xt.grad = None
        ops.ps_roi_pool(xt, boxes, size, scale).backward(gpu(g))
        grads.append(xt.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert grads[0].stride() == xt.stride()
    got = grads[0].cpu().numpy()
    want = P.ps_roi_pool_backward(g, x.shape, rois, oh, ow, scale)
    err = rel(got, want)
    print("ps_roi_pool backward %s: %.3g of max|d|" % (size, err))
    assert err <= 2e-6 and np.abs(want).max() > 0.1
    assert not got[want == 0].any()                                      # nothing outside the windows; the last row and column get none
    assert not got[:, :, h - 1, :].any() and not got[:, :, :, w - 1].any()
    good = (rois[:, 0] > -1) & (rois[:, 0] < n_img)
    xt.grad = None
    ops.ps_roi_pool(xt, boxes[torch.from_numpy(good).to(DEV)], size, scale).backward(gpu(g[good]))
    assert torch.equal(xt.grad, grads[0])


@pytest.mark.parametrize("op", ["ps_roi_align", "ps_roi_pool"])
def test_double_backward_raises(op):
    x = torch.randn((1, 8, 6, 6), device=DEV, requires_grad=True)
    boxes = torch.tensor([[0, 0, 0, 4, 4]], dtype=torch.float32, device=DEV)
    y = getattr(ops, op)(x, boxes, 2)
    v = torch.ones_like(y, requires_grad=True)                           # the backward is differentiable only in the output gradient
    dx, = torch.autograd.grad(y, x, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        dx.sum().backward()


# ---- 4. 16-bit maps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("op", ["ps_roi_align", "ps_roi_pool"])
@pytest.mark.parametrize("size,co", [((7, 7), 2), ((3, 1), 7), ((1, 1), 13)])        # 98, 21 and 13 channels: 21 and 13 hold no run of 8
@pytest.mark.parametrize("channels_last", [False, True])
def test_16_bit_maps_are_the_float32_op_rounded_once(dtype, op, size, co, channels_last):
    oh, ow = size
    n_img, h, w, scale = 3, 11, 13, 0.25
    rng = np.random.RandomState(oh + ow + co)
    x = torch.from_numpy(rng.randn(n_img, co * oh * ow, h, w).astype(F)).to(DEV).to(dtype)
    if channels_last:
        x = x.contiguous(memory_format=CL)
    rois = P.make_rois(rng, 48, n_img, h, w, scale)
    boxes = torch.from_numpy(rois).to(DEV)
    g = torch.from_numpy(rng.randn(rois.shape[0], co, oh, ow).astype(F)).to(DEV).to(dtype)
    f = (lambda t: ops.ps_roi_align(t, boxes, size, scale, -1)) if op == "ps_roi_align" else (lambda t: ops.ps_roi_pool(t, boxes, size, scale))
    x16 = x.clone().requires_grad_(True)
    x32 = x.float().requires_grad_(True)
    y16, y32 = f(x16), f(x32)
    assert y16.dtype == dtype and y16.is_contiguous()
    want = y32.detach().to(dtype)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(y16), nan) and nan.any() == (op == "ps_roi_align")
    assert torch.equal(torch.where(nan, 0, y16.detach()).view(torch.int16), torch.where(nan, 0, want).view(torch.int16))
    y16.backward(g)
    y32.backward(g.float())
    assert x16.grad.dtype == dtype and x16.grad.stride() == x16.stride()
    assert torch.equal(x16.grad.view(torch.int16), x32.grad.to(dtype).view(torch.int16))
    assert x32.grad.abs().max() > 0.1
    # boxes in the map's own dtype are widened before the launch
    assert torch.equal(torch.nan_to_num(f(x)), torch.nan_to_num(f(x))) and f(x).dtype == dtype
    b16 = boxes.to(dtype)
    y_b16 = ops.ps_roi_pool(x, b16, size, scale)
    assert torch.equal(y_b16, ops.ps_roi_pool(x, b16.float(), size, scale))


# ---- 5. sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["ps_roi_align", "ps_roi_pool"])
def test_empty_and_large_calls(op):
    f = getattr(ops, op)
    x = torch.randn((2, 18, 9, 8), device=DEV, requires_grad=True)
    y = f(x, torch.zeros((0, 5), device=DEV), 3, 0.5)                   # K == 0
    assert y.shape == (0, 2, 3, 3)
    y.sum().backward()
    assert x.grad.shape == x.shape and not x.grad.any()
    assert f(x, [], 3).shape == (0, 2, 3, 3)
    boxes = torch.tensor([[0, 0, 0, 4, 4], [1, 1, 1, 3, 3]], dtype=torch.float32, device=DEV)
    for shape in ((0, 18, 9, 8), (2, 18, 0, 8), (2, 18, 9, 0)):         # N * H * W == 0
        xe = torch.zeros(shape, device=DEV, requires_grad=True)
        y = f(xe, boxes, 3, 0.5)
        assert y.shape == (2, 2, 3, 3) and not y.any()
        y.sum().backward()
        assert xe.grad.shape == xe.shape
    assert f(torch.zeros((2, 0, 9, 8), device=DEV), boxes, 3).shape == (2, 0, 3, 3)
    k = 4096                                                            # a large K, over three images
    rng = np.random.RandomState(5)
    xl = torch.randn((3, 27, 20, 25), device=DEV, requires_grad=True)
    x1, y1 = rng.uniform(0, 300, k), rng.uniform(0, 240, k)
    rois = np.stack([rng.randint(0, 3, k), x1, y1, x1 + rng.uniform(8, 200, k), y1 + rng.uniform(8, 200, k)], 1).astype(F)
    y = f(xl, torch.from_numpy(rois).to(DEV), 3, 1 / 16)
    assert y.shape == (k, 3, 3, 3) and torch.isfinite(y).all() and y.abs().max() > 0.1
    y.backward(torch.ones_like(y))
    assert xl.grad.shape == xl.shape and torch.isfinite(xl.grad).all()
    # every non-empty bin hands on exactly its gradient: ps_roi_align's weights sum to 1 per sample inside the map
    if op == "ps_roi_pool":
        full = sum(1 for r in rois[:64] for (hs, he, ws, we) in P.pool_windows(20, 25, r[1:], 3, 3, 1 / 16).values() if he > hs and we > ws)
        xl.grad = None
        f(xl, torch.from_numpy(rois[:64]).to(DEV), 3, 1 / 16).sum().backward()
        assert float(xl.grad.double().sum()) == pytest.approx(3 * full, rel=1e-5)
