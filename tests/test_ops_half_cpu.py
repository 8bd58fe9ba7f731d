"""fasterrcnn_amd.ops on float16 / bfloat16 maps without a GPU: meta / FakeTensor shapes, dtypes and strides through autograd, the argument
rules (which dtype combinations are taken, which keep raising TypeError), and the frcnn_ops_*_16 entry points' validation (ABI 21)."""
import ctypes as C

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

CL = torch.channels_last
HALF = [torch.float16, torch.bfloat16]
SCALES = [1 / 4, 1 / 8, 1 / 16]
EINVAL = -1


def cl_strides(k, c, oh, ow):
    return torch.empty((k, c, oh, ow), device="meta", memory_format=CL).stride()


def pyramid(device, dtype, n=2, c=6, channels_last=False, requires_grad=False):
    feats = []
    for i in range(3):
        f = torch.empty((n, c, 64 >> i, 96 >> i), device=device, dtype=dtype)
        if channels_last:
            f = f.contiguous(memory_format=CL)
        feats.append(f.requires_grad_(requires_grad))
    return feats


def run_op(op, device, dtype, channels_last=False, requires_grad=False, box_dtype=torch.float32, as_list=False):
    """One call of op on empty tensors: (inputs, output), output [4, 6, 7, 3]."""
    boxes = ([torch.empty((3, 4), device=device, dtype=box_dtype), torch.empty((1, 4), device=device, dtype=box_dtype)] if as_list
             else torch.empty((4, 5), device=device, dtype=box_dtype))
    if op == "multi_scale_roi_align":
        xs = pyramid(device, dtype, channels_last=channels_last, requires_grad=requires_grad)
        return xs, ops.multi_scale_roi_align(xs, boxes, (7, 3), SCALES, 2)
    x = torch.empty((2, 6, 12, 10), device=device, dtype=dtype)
    if channels_last:
        x = x.contiguous(memory_format=CL)
    x.requires_grad_(requires_grad)
    y = ops.roi_align(x, boxes, (7, 3), 0.25, 2) if op == "roi_align" else ops.roi_pool(x, boxes, (7, 3), 0.25)
    return [x], y


OPS = ["roi_align", "roi_pool", "multi_scale_roi_align"]


# ---- 1. meta / FakeTensor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("channels_last", [False, True])
def test_fake_and_meta_follow_the_inputs_dtype(op, dtype, channels_last):
    with FakeTensorMode():
        _, y = run_op(op, "cuda", dtype, channels_last, requires_grad=True)
        assert y.shape == (4, 6, 7, 3) and y.dtype == dtype and y.stride() == cl_strides(4, 6, 7, 3) and y.requires_grad
    xs, y = run_op(op, "meta", dtype, channels_last, requires_grad=True)
    assert y.shape == (4, 6, 7, 3) and y.dtype == dtype and y.stride() == cl_strides(4, 6, 7, 3)
    y.sum().backward()
    for x in xs:
        assert x.grad.dtype == dtype and x.grad.shape == x.shape and x.grad.stride() == x.stride()


@pytest.mark.parametrize("dtype", HALF)
def test_module_classes_and_empty_cases_keep_the_dtype(dtype):
    x = torch.empty((2, 6, 12, 10), device="meta", dtype=dtype)
    for boxes in (torch.empty((0, 5), device="meta"), [], torch.empty((5, 5), device="meta")):
        k = 5 if isinstance(boxes, torch.Tensor) and boxes.shape[0] else 0
        for y in (ops.RoIAlign(7, 0.5, 2)(x, boxes), ops.RoIPool((7, 7), 0.5)(x, boxes),
                  ops.multi_scale_roi_align([x], boxes, 7, [0.5], 2)):
            assert y.shape == (k, 6, 7, 7) and y.dtype == dtype
    y = ops.roi_align(torch.empty((2, 0, 12, 10), device="meta", dtype=dtype), torch.empty((3, 5), device="meta"), 7)
    assert y.shape == (3, 0, 7, 7) and y.dtype == dtype


@pytest.mark.parametrize("dtype", HALF)
def test_roi_pool_argmax_stays_int32(dtype):
    x = torch.empty((2, 6, 12, 10), device="meta", dtype=dtype)
    y, argmax = torch.ops.frcnn.roi_pool(x, torch.empty((4, 5), device="meta"), 0.25, 7, 3)
    assert y.dtype == dtype and argmax.dtype == torch.int32 and argmax.shape == y.shape and argmax.stride() == y.stride()
    dx = torch.ops.frcnn.roi_pool_backward(torch.empty_like(y), torch.empty((4, 5), device="meta"), argmax, 0.25, 7, 3, 2, 6, 12, 10, True)
    assert dx.dtype == dtype and dx.shape == x.shape and dx.stride() == x.contiguous(memory_format=CL).stride()


# ---- 2. argument rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("as_list", [False, True])
def test_boxes_float32_or_the_maps_own_dtype(op, dtype, as_list):
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    for box_dtype in (torch.float32, dtype):
        _, y = run_op(op, "meta", dtype, box_dtype=box_dtype, as_list=as_list)
        assert y.shape == (4, 6, 7, 3) and y.dtype == dtype
    for box_dtype in (other, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            run_op(op, "meta", dtype, box_dtype=box_dtype, as_list=as_list)
    with pytest.raises(TypeError, match="float32"):                     # 16-bit boxes go with a map of their own dtype only
        run_op(op, "meta", torch.float32, box_dtype=dtype, as_list=as_list)
    with pytest.raises(TypeError, match="float32"):
        run_op(op, "meta", torch.float64, as_list=as_list)


def test_a_pyramid_has_one_dtype():
    boxes = torch.empty((4, 5), device="meta")
    for a, b in ((torch.float16, torch.float32), (torch.float16, torch.bfloat16), (torch.float32, torch.bfloat16)):
        feats = pyramid("meta", a)
        feats[1] = feats[1].to(b)
        with pytest.raises(TypeError, match="one dtype"):
            ops.multi_scale_roi_align(feats, boxes, 7, SCALES, 2)
    with pytest.raises(TypeError, match="float32"):
        ops.multi_scale_roi_align(pyramid("meta", torch.float64), boxes, 7, SCALES, 2)


def test_nms_still_refuses_16_bit_boxes():
    b = torch.empty((5, 4), device="meta")
    s = torch.empty((5,), device="meta")
    for dtype in HALF:
        with pytest.raises(TypeError, match="float32 or float64"):
            ops.nms(b.to(dtype), s, 0.5)


# ---- 3. the C entry points --------------------------------------------------------------------------------------------------------------
def test_abi_21_and_type_codes():
    lib = nv.lib()
    assert nv.ABI_VERSION == 21 and lib.frcnn_abi_version() == 21
    assert (nv.OPS_F16, nv.OPS_BF16) == (1, 2)
    assert lib.frcnn_ops_half_run() in (4, 8)


@pytest.mark.parametrize("t", [nv.OPS_F16, nv.OPS_BF16])
def test_16_bit_entry_points_reject_what_their_float32_siblings_reject(t):
    lib = nv.lib()
    c = lib.frcnn_ops_half_run()
    # roi_align: C not a multiple of the run, C == 0, output 0 / 65, sampling ratio 17, no images, null pointers with k > 0, k < 0
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c + 2, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, 0, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, 1, 0, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, 1, 7, 65, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, 1, 7, 7, 1.0, 17, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 0, 8, 8, c, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, 1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, -1, 7, 7, 1.0, 2, 0, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, 0, 7, 7, 1.0, 2, 0, None, None) == 0       # k == 0: nothing to do
    assert lib.frcnn_ops_roi_align_backward_16(t, None, 1, 1, 8, 8, c, 7, 7, 1.0, 2, 0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_backward_16(t, None, 0, 1, 8, 8, c + 2, 7, 7, 1.0, 2, 0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_backward_16(t, None, 0, 1, 8, 8, c, 7, 7, 1.0, 17, 0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_align_backward_16(t, None, 0, 1, 8, 8, c, 7, 7, 1.0, 2, 0, None, None, None) == EINVAL   # no d_dx
    # roi_pool
    assert lib.frcnn_ops_roi_pool_16(t, None, 1, 8, 8, c, None, 1, 7, 7, 1.0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool_16(t, None, 1, 8, 8, c - 1, None, 1, 7, 7, 1.0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool_16(t, None, 1, 0, 8, c, None, 1, 7, 7, 1.0, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool_16(t, None, 1, 8, 8, c, None, 0, 7, 7, 1.0, None, None, None) == 0
    assert lib.frcnn_ops_roi_pool_backward_16(t, None, 1, 1, 8, 8, c, 7, 7, 1.0, None, None, None, None) == EINVAL
    assert lib.frcnn_ops_roi_pool_backward_16(t, None, 0, 1, 8, 8, c, 7, 65, 1.0, None, None, None, None) == EINVAL
    # multi-scale: levels 0 / 9, missing level arrays, C, output, sampling ratio, null pointers with k > 0, a short workspace
    hs, ws, sc = (C.c_int * 2)(16, 8), (C.c_int * 2)(16, 8), (C.c_float * 2)(0.25, 0.125)
    ms = lambda levels=2, ch=c, k=1, oh=7, sr=2, h=hs: lib.frcnn_ops_ms_roi_align_16(  # noqa: E731
        t, None, h, ws, sc, levels, 1, ch, None, k, oh, 7, sr, 224.0, 4.0, 2, 3, None, None)
    assert ms(levels=0) == EINVAL and ms(levels=9) == EINVAL and ms(h=None) == EINVAL
    assert ms(ch=c + 2) == EINVAL and ms(ch=0) == EINVAL and ms(oh=65) == EINVAL and ms(sr=17) == EINVAL
    assert ms() == EINVAL and ms(k=-1) == EINVAL
    assert ms(k=0) == 0
    need = lib.frcnn_ops_ms_roi_align_workspace_bytes(0, 2, 1)
    bw = lambda levels=2, ch=c, k=0, nbytes=need, dx=None: lib.frcnn_ops_ms_roi_align_backward_16(  # noqa: E731
        t, None, k, hs, ws, sc, levels, 1, ch, 7, 7, 2, 224.0, 4.0, 2, 3, None, dx, 8, nbytes, None)
    ptrs = (C.c_void_p * 2)(8, 8)
    assert bw() == EINVAL                                              # no d_dx
    assert bw(dx=ptrs, nbytes=need - 1) == EINVAL and bw(dx=ptrs, ch=c + 2) == EINVAL and bw(dx=ptrs, levels=9) == EINVAL
    assert bw(dx=ptrs, k=1) == EINVAL                                  # k > 0 without RoIs and gradient
    assert bw(dx=(C.c_void_p * 2)(8, None)) == EINVAL                  # a level without a gradient buffer


def test_16_bit_entry_points_reject_an_unknown_type_code():
    lib = nv.lib()
    c = lib.frcnn_ops_half_run()
    hs, ws, sc = (C.c_int * 1)(8), (C.c_int * 1)(8), (C.c_float * 1)(0.25)
    for t in (0, 3, -1, 16):
        assert lib.frcnn_ops_roi_align_16(t, None, 1, 8, 8, c, None, 0, 7, 7, 1.0, 2, 0, None, None) == EINVAL
        assert lib.frcnn_ops_roi_align_backward_16(t, None, 0, 1, 8, 8, c, 7, 7, 1.0, 2, 0, None, 8, None) == EINVAL
        assert lib.frcnn_ops_roi_pool_16(t, None, 1, 8, 8, c, None, 0, 7, 7, 1.0, None, None, None) == EINVAL
        assert lib.frcnn_ops_roi_pool_backward_16(t, None, 0, 1, 8, 8, c, 7, 7, 1.0, None, None, 8, None) == EINVAL
        assert lib.frcnn_ops_ms_roi_align_16(t, None, hs, ws, sc, 1, 1, c, None, 0, 7, 7, 2, 224.0, 4.0, 2, 2, None, None) == EINVAL
        assert lib.frcnn_ops_ms_roi_align_backward_16(t, None, 0, hs, ws, sc, 1, 1, c, 7, 7, 2, 224.0, 4.0, 2, 2, None,
                                                      (C.c_void_p * 1)(8), 8, 64, None) == EINVAL
