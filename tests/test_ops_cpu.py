"""fasterrcnn_amd.ops without a GPU: shapes, dtypes and strides from meta / fake tensors, the documented argument errors, and the
frcnn_ops_* C entry points rejecting bad arguments before they touch a device."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import ShapeEnv

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

CL = torch.channels_last


def cl_strides(k, c, oh, ow):
    return torch.empty((k, c, oh, ow), device="meta", memory_format=CL).stride()


@pytest.mark.parametrize("fn", ["roi_align", "roi_pool", "RoIAlign", "RoIPool"])
@pytest.mark.parametrize("output_size", [7, (7, 3), (1, 1), (64, 64)])
@pytest.mark.parametrize("k", [0, 1, 5])
@pytest.mark.parametrize("as_list", [False, True])
def test_roi_ops_meta_shapes(fn, output_size, k, as_list):
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    x = torch.empty((2, 6, 9, 11), device="meta")
    boxes = [torch.empty((k, 4), device="meta"), torch.empty((2, 4), device="meta")] if as_list else torch.empty((k, 5), device="meta")
    kk = k + 2 if as_list else k
    call = {"roi_align": lambda: ops.roi_align(x, boxes, output_size, 0.5, 2),
            "roi_pool": lambda: ops.roi_pool(x, boxes, output_size, 0.5),
            "RoIAlign": lambda: ops.RoIAlign(output_size, 0.5, -1, aligned=True)(x, boxes),
            "RoIPool": lambda: ops.RoIPool(output_size, 0.5)(x, boxes)}[fn]
    y = call()
    assert y.shape == (kk, 6, oh, ow) and y.dtype == torch.float32
    assert y.stride() == cl_strides(kk, 6, oh, ow)


@pytest.mark.parametrize("fn", ["roi_align", "roi_pool"])
@pytest.mark.parametrize("channels_last", [False, True])
def test_roi_ops_fake_and_meta_autograd(fn, channels_last):
    def run(device):
        x = torch.empty((3, 5, 12, 10), device=device)
        if channels_last:
            x = x.contiguous(memory_format=CL)
        x.requires_grad_(True)
        boxes = torch.empty((4, 5), device=device)
        y = ops.roi_align(x, boxes, (7, 3), 0.25, 2) if fn == "roi_align" else ops.roi_pool(x, boxes, (7, 3), 0.25)
        assert y.shape == (4, 5, 7, 3) and y.device.type == device and y.stride() == cl_strides(4, 5, 7, 3)
        assert y.requires_grad
        return x, y
    with FakeTensorMode():
        run("cuda")
    x, y = run("meta")                       # the autograd engine needs a real device type: the backward's fake on meta tensors
    y.sum().backward()
    assert x.grad.shape == x.shape and x.grad.stride() == x.stride()
    x, y = run("meta")
    v = torch.empty(y.shape, device="meta", requires_grad=True)
    g, = torch.autograd.grad(y, x, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        g.sum().backward()


def test_nms_fake_output_is_data_dependent():
    with FakeTensorMode(shape_env=ShapeEnv()):
        for dt in (torch.float32, torch.float64):
            boxes = torch.empty((10, 4), device="cuda", dtype=dt)
            scores = torch.empty((10,), device="cuda", dtype=dt)
            k = ops.nms(boxes, scores, 0.5)
            assert k.dim() == 1 and k.dtype == torch.int64
            k = ops.batched_nms(boxes, scores, torch.empty((10,), device="cuda", dtype=torch.int64), 0.5)
            assert k.dim() == 1 and k.dtype == torch.int64


def test_roi_ops_argument_errors():
    x = torch.empty((1, 4, 8, 8), device="meta")
    b = torch.empty((3, 5), device="meta")
    with pytest.raises(ValueError, match="GPU"):
        ops.roi_align(torch.zeros(1, 4, 8, 8), torch.zeros(3, 5), 7)
    with pytest.raises(ValueError, match="GPU"):
        ops.roi_pool(torch.zeros(1, 4, 8, 8), torch.zeros(3, 5), 7)
    with pytest.raises(TypeError, match="float32"):
        ops.roi_align(x.double(), b, 7)
    with pytest.raises(TypeError, match="float32"):
        ops.roi_pool(x, b.double(), 7)
    with pytest.raises(TypeError, match="float32"):
        ops.roi_pool(x, [torch.empty((2, 4), device="meta", dtype=torch.float16)], 7)
    with pytest.raises(ValueError, match=r"Tensor\[K, 5\]"):
        ops.roi_align(x, torch.empty((3, 4), device="meta"), 7)
    with pytest.raises(ValueError, match=r"\[L, 4\]"):
        ops.roi_align(x, [torch.empty((3, 5), device="meta")], 7)
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        ops.roi_pool(torch.empty((4, 8, 8), device="meta"), b, 7)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.roi_align(x, [[0, 0, 1, 1]], 7)
    with pytest.raises(ValueError, match="output_size"):
        ops.roi_align(x, b, 65)
    with pytest.raises(ValueError, match="output_size"):
        ops.roi_pool(x, b, (7, 0))
    with pytest.raises(TypeError, match="output_size"):
        ops.roi_pool(x, b, (7, 7, 7))
    with pytest.raises(ValueError, match="sampling_ratio"):
        ops.roi_align(x, b, 7, 1.0, 17)


def test_nms_argument_errors():
    b = torch.empty((5, 4), device="meta")
    s = torch.empty((5,), device="meta")
    with pytest.raises(ValueError, match="GPU"):
        ops.nms(torch.zeros(5, 4), torch.zeros(5), 0.5)
    with pytest.raises(TypeError, match="float32 or float64"):
        ops.nms(b.half(), s, 0.5)
    with pytest.raises(TypeError, match="float32 or float64"):
        ops.nms(b, s.to(torch.int64), 0.5)
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        ops.nms(torch.empty((5, 5), device="meta"), s, 0.5)
    with pytest.raises(ValueError, match=r"scores must be \[N\]"):
        ops.nms(b, torch.empty((4,), device="meta"), 0.5)
    with pytest.raises(TypeError, match="integer"):
        ops.batched_nms(b, s, torch.empty((5,), device="meta"), 0.5)
    with pytest.raises(ValueError, match=r"idxs must be \[N\]"):
        ops.batched_nms(b, s, torch.empty((6,), device="meta", dtype=torch.int64), 0.5)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.nms([[0, 0, 1, 1]], s, 0.5)


def test_ops_entry_points_reject_bad_arguments():
    lib = nv.lib()
    EINVAL = -1
    # roi_align: C % 4, C < 4, output 0 / 65, sampling ratio 17, no images, null pointers with k > 0
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 6, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 0, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 4, None, 1, 0, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 4, None, 1, 7, 65, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 4, None, 1, 7, 7, 1.0, 17, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 0, 8, 8, 4, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 4, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 4, None, -1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align(None, 1, 8, 8, 4, None, 0, 7, 7, 1.0, 2, 0, None, None) == 0       # k == 0: nothing to do
    assert lib.frcnn_ops_roi_align_backward(None, 1, 1, 8, 8, 4, 7, 7, 1.0, 2, 0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_backward(None, 0, 1, 8, 8, 6, 7, 7, 1.0, 2, 0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_backward(None, 0, 1, 8, 8, 4, 7, 7, 1.0, 17, 0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_backward(None, 0, 1, 8, 8, 4, 7, 7, 1.0, 2, 0, None, None, None) == EINVAL   # no d_dx
    # roi_pool
    assert lib.frcnn_ops_roi_pool(None, 1, 8, 8, 4, None, 1, 7, 7, 1.0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool(None, 1, 8, 8, 3, None, 1, 7, 7, 1.0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool(None, 1, 0, 8, 4, None, 1, 7, 7, 1.0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool(None, 1, 8, 8, 4, None, 0, 7, 7, 1.0, None, None, None) == 0
    assert lib.frcnn_ops_roi_pool_backward(None, 1, 1, 8, 8, 4, 7, 7, 1.0, None, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool_backward(None, 0, 1, 8, 8, 4, 7, 65, 1.0, None, None, None, None) == EINVAL
    # nms: dtype flag, n out of range, missing pointers / workspace
    assert lib.frcnn_ops_nms_workspace_bytes(0) == 0
    assert lib.frcnn_ops_nms_workspace_bytes(1) == 8
    assert lib.frcnn_ops_nms_workspace_bytes(12000) == 12000 * 188 * 8
    assert lib.frcnn_ops_nms_workspace_bytes(524289) == 0
    assert lib.frcnn_ops_nms(None, 0, None, None, 0, 0.5, None, None, 0, None) == 0
    assert lib.frcnn_ops_nms(None, 2, None, None, 10, 0.5, None, None, 0, None) == EINVAL
    assert lib.frcnn_ops_nms(None, 0, None, None, -1, 0.5, None, None, 0, None) == EINVAL
    assert lib.frcnn_ops_nms(None, 0, None, None, 524289, 0.5, None, None, 0, None) == EINVAL
    assert lib.frcnn_ops_nms(None, 1, None, None, 10, 0.5, None, None, 80, None) == EINVAL
    assert lib.frcnn_ops_nms(8, 0, 8, None, 10, 0.5, 8, 8, 79, None) == EINVAL      # workspace one byte short (no device access)
