"""fasterrcnn_amd.ops.masked_conv2d / MaskedConv2d without a GPU: the argument checks, the fake implementation (on meta tensors), the
missing autograd formula, the module's nn.Conv2d behaviour, the mirrored tile constants and masked_conv2d_pytorch against the float64
truth of tests/mconv_cases.py."""
import pytest
import torch
import torch.nn.functional as F

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import mconv_cases as M

F32, F64 = torch.float32, torch.float64


def meta_call(n=2, c=3, h=5, w=6, co=4, k=(3, 3), pad=1, dtype=F32, channels_last=False, mask_shape=None, bias=True, **kw):
    """masked_conv2d on meta tensors: every check of the public function and the op's fake run, no kernel does."""
    x = torch.empty((n, c, h, w), dtype=dtype, device="meta")
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    wt = torch.empty((co, c) + tuple(k), dtype=kw.pop("weight_dtype", dtype), device="meta")
    b = torch.empty((co,), dtype=kw.pop("bias_dtype", dtype), device="meta") if bias else None
    p = (pad, pad) if isinstance(pad, int) else pad
    shape = (n, h + 2 * p[0] - k[0] + 1, w + 2 * p[1] - k[1] + 1) if mask_shape is None else mask_shape
    mask = torch.empty(shape, dtype=kw.pop("mask_dtype", F32), device="meta")
    return ops.masked_conv2d(x, mask, wt, b, pad, **kw)


def test_constants_mirror_the_library():
    lib = nv.lib()
    assert ops.MASKED_CONV_TILE_PIXELS == lib.frcnn_ops_masked_conv2d_tile_pixels()
    assert ops.MASKED_CONV_TILE_CHANNELS == lib.frcnn_ops_masked_conv2d_tile_channels()
    assert ops.MASKED_CONV_K_CHUNK == lib.frcnn_ops_masked_conv2d_k_chunk()
    assert ops.MAX_MASKED_CONV_INDEX == lib.frcnn_ops_masked_conv2d_max_index()
    assert nv.OPS_F32 not in (nv.OPS_F16, nv.OPS_BF16)
    assert {"masked_conv2d", "MaskedConv2d", "masked_conv2d_pytorch"} <= set(ops.__all__)


def test_library_validates_before_touching_the_gpu():
    lib = nv.lib()
    assert lib.frcnn_ops_masked_conv2d_workspace_bytes(2, 5, 6) >= 4 * (1 + 60)                # the count and an int32 per output pixel
    assert lib.frcnn_ops_masked_conv2d_workspace_bytes(0, 5, 6) == 0
    assert lib.frcnn_ops_masked_conv2d_workspace_bytes(65536, 65536, 1) == 0                  # N oh ow past 2^31
    import ctypes as C
    strides = (C.c_int64 * 4)(90, 30, 6, 1)
    args = [nv.OPS_F32, None, strides, 2, 3, 5, 6, None, None, 4, 3, 3, 1, 1, None, None, strides, None, 0, None]
    assert lib.frcnn_ops_masked_conv2d(*args) == -1                                           # NULL pointers
    args[0] = 7
    assert lib.frcnn_ops_masked_conv2d(*args) == -1                                           # unknown element type


@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("channels_last", (False, True))
def test_fake_shape_dtype_and_format(dtype, channels_last):
    out = meta_call(dtype=dtype, channels_last=channels_last, pad=(2, 0))
    assert out.shape == (2, 4, 7, 4) and out.dtype == dtype and out.device.type == "meta"
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert out.is_contiguous(memory_format=fmt) and out.stride() == torch.empty((2, 4, 7, 4), memory_format=fmt).stride()
    assert meta_call(bias=False).shape == (2, 4, 5, 6)                                        # bias=None is a zero bias
    for mask_dtype in (torch.bool, torch.uint8, torch.int64, torch.float16, F64):
        assert meta_call(mask_dtype=mask_dtype).shape == (2, 4, 5, 6)


def test_type_errors():
    for kw in (dict(weight_dtype=torch.float16), dict(bias_dtype=torch.bfloat16), dict(dtype=torch.float16, weight_dtype=F32),
               dict(dtype=torch.bfloat16, bias_dtype=torch.float16), dict(dtype=F64), dict(dtype=torch.int32),
               dict(mask_dtype=torch.complex64), dict(stride="1"), dict(pad=1.0)):
        with pytest.raises(TypeError):
            meta_call(**kw)
    x, mask, wt, b = M.case("kernel_3x3_p1")
    with pytest.raises(TypeError):
        ops.masked_conv2d(x.numpy(), mask, wt, b, 1)
    with pytest.raises(TypeError):
        ops.masked_conv2d_pytorch(x, mask, wt.double(), b, 1)
    with pytest.raises(TypeError):
        ops.masked_conv2d_pytorch(x, mask.numpy(), wt, b, 1)


def test_value_errors():
    for kw in (dict(stride=2), dict(stride=(1, 2)), dict(pad=-1), dict(mask_shape=(2, 5, 5)), dict(mask_shape=(1, 5, 6)),
               dict(mask_shape=(2, 1, 5, 6)), dict(pad=0, mask_shape=(2, 5, 6)),             # mmcv's mask on the map's grid: refused
               dict(h=2, w=2, pad=0), dict(c=0), dict(co=0)):
        with pytest.raises(ValueError):
            meta_call(**kw)
    x, mask, wt, b = M.case("kernel_3x3_p1")
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.masked_conv2d(x, mask, wt, b, 1)
    for call in (lambda: ops.masked_conv2d_pytorch(x, mask, wt[:, :2], b, 1), lambda: ops.masked_conv2d_pytorch(x, mask, wt, b[:3], 1),
                 lambda: ops.masked_conv2d_pytorch(x[0], mask, wt, b, 1), lambda: ops.masked_conv2d_pytorch(x, mask, wt[0], b, 1),
                 lambda: ops.masked_conv2d_pytorch(x, mask, wt, b, 1, stride=2), lambda: ops.masked_conv2d_pytorch(x, mask, wt, b, 0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="32-bit"):
        meta_call(n=1, c=1, h=46341, w=46341, co=1, k=(1, 1), pad=0)                          # N oh ow = 46341^2 > 2^31


def test_backward_through_the_op_raises():
    x = torch.empty((1, 2, 4, 4), device="meta", requires_grad=True)
    out = ops.masked_conv2d(x, torch.empty((1, 4, 4), device="meta"), torch.empty((3, 2, 1, 1), device="meta"), None)
    assert out.requires_grad
    with pytest.raises((RuntimeError, NotImplementedError)):
        out.sum().backward()


def test_module_without_a_mask_is_conv2d_and_trains():
    torch.manual_seed(0)
    m = ops.MaskedConv2d(3, 5, 3, stride=2, padding=1, dilation=2, groups=1)
    ref = torch.nn.Conv2d(3, 5, 3, stride=2, padding=1, dilation=2)
    assert isinstance(m, torch.nn.Conv2d) and sorted(m.state_dict()) == ["bias", "weight"]
    m.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(2, 3, 9, 8, requires_grad=True)
    y = m(x)
    assert torch.equal(y, ref(x))
    y.sum().backward()
    assert m.weight.grad is not None and m.bias.grad is not None and x.grad is not None
    nb = ops.MaskedConv2d(3, 5, 1, bias=False)
    nb.load_state_dict(torch.nn.Conv2d(3, 5, 1, bias=False).state_dict(), strict=True)
    assert nb.bias is None


def test_module_with_a_mask_refuses_what_it_cannot_do():
    x, mask = torch.zeros(1, 4, 5, 5), torch.ones(1, 5, 5)
    for kw in (dict(dilation=2, padding=2), dict(groups=2), dict(stride=2)):
        with pytest.raises(ValueError):
            ops.MaskedConv2d(4, 4, 3, **{"padding": 1, **kw})(x, mask)
    m = ops.MaskedConv2d(3, 4, 3, padding=1).to("meta")
    out = m(torch.empty((2, 3, 5, 6), device="meta"), torch.empty((2, 5, 6), dtype=torch.bool, device="meta"))
    assert out.shape == (2, 4, 5, 6)


@pytest.mark.parametrize("name", M.VALUE_CASES)
def test_pytorch_form_against_the_truth_in_float64(name):
    """Both sides are float64 sums of K + 1 <= 51 terms of order 1 / sqrt(K): 1e-12 of the largest output is hundreds of roundings."""
    x, mask, wt, b = (t.double() for t in M.case(name))
    got = ops.masked_conv2d_pytorch(x, mask, wt, b, M.CASES[name]["pad"])
    want = M.truth(name)
    assert got.dtype == F64 and got.shape == want.shape
    assert M.rel_err(got, want) <= 1e-12
    assert torch.equal(got == 0, want == 0) and not bool(torch.signbit(got[want == 0]).any())


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_pytorch_form_contract_details(dtype):
    x, mask, wt, b = M.case("n3", dtype)
    got = ops.masked_conv2d_pytorch(x, mask, wt, b, 1)
    assert got.dtype == dtype and M.rel_err(got, M.truth("n3", dtype)) <= 4 * max(M.rel_err(M.restated("n3", dtype), M.truth("n3", dtype)), 2.0 ** -24)
    assert torch.equal(got[0], torch.zeros_like(got[0])) and not bool(torch.signbit(got[0]).any())
    nob = ops.masked_conv2d_pytorch(x, mask, wt, None, 1)
    assert M.rel_err(nob, M.dense(x, mask, wt, None, 1, F64)) <= 2.0 ** -7
    cl = ops.masked_conv2d_pytorch(x.contiguous(memory_format=torch.channels_last), mask, wt, b, 1)
    assert cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl, got)
    nan_mask = mask.clone()
    nan_mask[2, 0, 0] = float("nan")
    assert bool((ops.masked_conv2d_pytorch(x, nan_mask, wt, b, 1)[2, :, 0, 0] == 0).all())   # NaN is inactive
    for other in (mask > 0, (mask > 0).to(torch.uint8), (mask > 0).long() - (mask < 0).long()):
        assert torch.equal(ops.masked_conv2d_pytorch(x, other, wt, b, 1), got)


def test_cases_cover_what_they_claim():
    assert M.COUNT_W * 5 >= 2 * M.T + 1 > (M.COUNT_W - 1) * 5
    for cnt in M.COUNTS:
        assert int((M.case("count_%d" % cnt)[1] > 0).sum()) == cnt
    _, mask, _, _ = M.case("n3")
    assert not bool((mask[0] > 0).any()) and bool((mask[1] > 0).all()) and 0 < int((mask[2] > 0).sum()) < mask[2].numel()
    assert bool((mask < 0).any()) and bool((mask == 0).any())
    assert M.KC + 1 in M.K_SHAPES and M.CO + 1 in M.C_OUTS
    for name in M.VALUE_CASES:
        assert float(M.truth(name).abs().max()) > 0.1
