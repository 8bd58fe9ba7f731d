"""fasterrcnn_amd.ops.deform_conv2d / DeformConv2d without a GPU: the torch restatement (tests/deform_conv_cases.py) against
torch's own convolution and against autograd, the argument rules on meta tensors, the module's parameters, and the validation of the
frcnn_ops_deform_* entry points (additive: the ABI number stays 21)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import deform_conv_cases as D

CL = torch.channels_last
EINVAL = -1
F64 = torch.float64
IDS = ["g%d" % i for i in range(len(D.GEOMETRIES))]


def conv_args(geometry):
    _, c, _, groups, _, _, stride, padding, dilation, _, _ = geometry
    return {"stride": stride, "padding": padding, "dilation": dilation, "groups": groups}


# ---- 1. the restatement against torch's convolution -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=IDS)
def test_zero_offsets_and_a_mask_of_ones_are_conv2d(geometry):
    case = D.cast(D.make_case(geometry, 3), F64)
    zero, ones = torch.zeros_like(case["offset"]), torch.ones_like(case["mask"])
    want = F.conv2d(case["input"], case["weight"], case["bias"], **conv_args(geometry))
    got = D.deform_conv2d_ref(case["input"], zero, case["weight"], case["bias"], mask=ones, **case["kw"])
    assert got.shape == want.shape and want.abs().max() > 0.1
    assert D.rel_err(got, want) <= 1e-12
    assert torch.equal(got, D.deform_conv2d_ref(case["input"], zero, case["weight"], case["bias"], mask=None, **case["kw"]))


@pytest.mark.parametrize("shift", [(1, 0), (0, -2), (-3, 2), (40, 0)])
@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=IDS)
def test_integer_offsets_are_a_convolution_of_the_shifted_zero_filled_map(geometry, shift):
    case = D.cast(D.make_case(geometry, 4, with_mask=False), F64)
    x = case["input"]
    h, w = x.shape[2:]
    (ph, pw), (dy, dx), b = case["kw"]["padding"], shift, 48
    offset = torch.zeros_like(case["offset"])
    offset[:, 0::2], offset[:, 1::2] = dy, dx
    big = F.pad(x, (b, b, b, b))
    moved = big[:, :, b - ph + dy:b - ph + dy + h + 2 * ph, b - pw + dx:b - pw + dx + w + 2 * pw]
    args = dict(conv_args(geometry), padding=(0, 0))
    want = F.conv2d(moved, case["weight"], case["bias"], **args)
    got = D.deform_conv2d_ref(x, offset, case["weight"], case["bias"], **case["kw"])
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=IDS)
def test_no_mask_is_a_mask_of_ones(geometry):
    case = D.make_case(geometry, 5, with_mask=False)
    ones = torch.ones((case["offset"].shape[0], case["offset"].shape[1] // 2) + tuple(case["offset"].shape[2:]))
    for dtype in (torch.float32, F64):
        c = D.cast(case, dtype)
        assert torch.equal(D.forward_ref(c, dtype), D.deform_conv2d_ref(c["input"], c["offset"], c["weight"], c["bias"],
                                                                        mask=ones.to(dtype), **c["kw"]))


def test_the_cases_exercise_the_border():
    for geometry in D.GEOMETRIES:
        case = D.make_case(geometry, 7)
        assert 0.10 <= case["rejected"] <= 0.40 and 0.10 <= case["straddling"] <= 0.40, (geometry, case["rejected"], case["straddling"])


# ---- 2. the explicit gradients against autograd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=IDS)
def test_explicit_gradients_are_autograds(geometry, with_mask):
    case = D.make_case(geometry, 11, with_mask=with_mask)
    explicit, auto = D.grads_ref(case, F64), D.autograd_ref(case, F64)
    for name, e, a in zip(D.ARGS, explicit, auto):
        assert (e is None) == (a is None), name
        if e is not None:
            assert a.abs().max() > 0.1 and D.rel_err(e, a) <= 1e-10, name


def test_offset_gradient_at_y_equal_minus_one_counts_row_zero():
    h = w = 4
    x = torch.arange(1.0, h * w + 1, dtype=F64).reshape(1, 1, h, w)
    offset = torch.zeros((1, 2, h, w), dtype=F64)
    offset[0, 0] = -1.0 - torch.arange(h, dtype=F64)[:, None]            # y == -1 exactly at every output
    offset[0, 1] = 0.25
    weight, grad = torch.ones((1, 1, 1, 1), dtype=F64), torch.ones((1, 1, h, w), dtype=F64)
    assert not D.deform_conv2d_ref(x, offset, weight).any()              # y <= -1: the sample is rejected
    _, d_offset, _, _, _ = D.deform_conv2d_grads_ref(x, offset, weight, None, (1, 1), (0, 0), (1, 1), None, grad)
    # d/dy = (1 - lw) * x[0, xl] + lw * x[0, xl + 1], the corner row -1 counting 0
    want = 0.75 * x[0, 0, 0, :3] + 0.25 * x[0, 0, 0, 1:]
    assert torch.allclose(d_offset[0, 0, :, :3], want.expand(h, 3), rtol=0, atol=1e-12) and d_offset[0, 0].abs().min() > 0.5


# ---- 3. the interface --------------------------------------------------------------------------------------------------------------------
def meta_args(geometry=D.GEOMETRIES[0], device="meta", dtype=torch.float32, mask=True, bias=True):
    n, c, co, groups, g, (kh, kw), stride, padding, dilation, h, w = geometry
    oh, ow = D.output_size(h, w, (kh, kw), stride, padding, dilation)
    e = lambda *shape: torch.empty(shape, device=device, dtype=dtype)    # noqa: E731
    return {"input": e(n, c, h, w), "offset": e(n, 2 * g * kh * kw, oh, ow), "weight": e(co, c // groups, kh, kw),
            "bias": e(co) if bias else None, "stride": stride, "padding": padding, "dilation": dilation,
            "mask": e(n, g * kh * kw, oh, ow) if mask else None}


def test_the_names_are_exported():
    for name in ("deform_conv2d", "DeformConv2d"):
        assert name in ops.__all__ and hasattr(ops, name)
    for name in ("deform_conv2d", "deform_conv2d_backward"):
        assert hasattr(torch.ops.frcnn, name)
    assert ops.DEFORM_CHUNK_IMAGES == 32


@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=IDS)
@pytest.mark.parametrize("channels_last", [False, True])
def test_meta_and_fake_results_are_contiguous_float32(geometry, channels_last):
    n, co = geometry[0], geometry[2]
    for device in ("meta", "fake"):
        mode = FakeTensorMode() if device == "fake" else None
        if mode:
            mode.__enter__()
        try:
            a = meta_args(geometry, "cuda" if mode else "meta")
            leaves = {}
            for k in D.ARGS:
                t = a[k].contiguous(memory_format=CL) if channels_last and a[k].dim() == 4 else a[k]
                leaves[k] = a[k] = t.requires_grad_(True)
            y = ops.deform_conv2d(**a)
            assert y.shape == (n, co) + tuple(a["offset"].shape[2:]) and y.dtype == torch.float32 and y.is_contiguous() and y.requires_grad
            if not mode:
                y.sum().backward()
                for k, t in leaves.items():
                    assert t.grad.shape == t.shape and t.grad.stride() == t.stride() and t.grad.dtype == torch.float32, k
        finally:
            if mode:
                mode.__exit__(None, None, None)


def test_int_and_pair_arguments_agree():
    a = meta_args(D.GEOMETRIES[0])
    a.update(stride=1, padding=1, dilation=1)
    assert ops.deform_conv2d(**a).shape == (3, 6, 9, 11)
    a = meta_args(D.GEOMETRIES[0], mask=False, bias=False)
    assert ops.deform_conv2d(a["input"], a["offset"], a["weight"], padding=(1, 1)).shape == (3, 6, 9, 11)


def test_argument_errors():
    good = meta_args(D.GEOMETRIES[0])                                    # N 3, C 8 -> 6, groups 2, G 2, 3x3, pad 1, 9 x 11
    e = lambda *shape: torch.empty(shape, device="meta")                 # noqa: E731

    def bad(match, **changes):
        with pytest.raises(ValueError, match=match):
            ops.deform_conv2d(**dict(good, **changes))

    bad("input must be", input=e(8, 9, 11))
    bad("weight must be", weight=e(6, 4, 3))
    bad("offset must be", offset=e(36, 9, 11))
    bad("mask must be", mask=e(18, 9, 11))
    bad("multiple of 2 \\* kh \\* kw", offset=e(3, 35, 9, 11))
    bad("multiple of 2 \\* kh \\* kw", offset=e(3, 0, 9, 11))
    bad("multiple of weight.shape\\[1\\]", weight=e(6, 3, 3, 3))         # C_in % (C_in / groups)
    bad("multiple of groups", weight=e(5, 4, 3, 3), bias=e(5))           # C_out % groups
    bad("multiple of the offset groups", offset=e(3, 2 * 3 * 9, 9, 11), mask=e(3, 27, 9, 11))   # C_in = 8, G = 3
    bad("offset must be \\[N", offset=e(3, 36, 9, 10))
    bad("offset must be \\[N", offset=e(2, 36, 9, 11))
    bad("mask must be \\[N", mask=e(3, 18, 8, 11))
    bad("mask must be \\[N", mask=e(1, 18, 9, 11))
    bad("mask must be \\[N", mask=e(3, 36, 9, 11))                       # the wrong number of mask channels
    bad("bias must be", bias=e(5))
    bad("bias must be", bias=e(6, 1))
    bad("stride must be >= 1", stride=(0, 1))
    bad("dilation must be >= 1", dilation=0)
    bad("padding must be >= 0", padding=(0, -1))
    bad("output would be empty", padding=0, dilation=5, offset=e(3, 36, 1, 1), mask=e(3, 18, 1, 1))
    with pytest.raises(TypeError, match="stride"):
        ops.deform_conv2d(**dict(good, stride=1.5))
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.deform_conv2d(**meta_args(D.GEOMETRIES[0], device="cpu"))
    with FakeTensorMode():                                               # tensors on different devices
        for name in ("offset", "weight", "bias", "mask"):
            with pytest.raises(ValueError, match="input and %s must be on the same device" % name):
                ops.deform_conv2d(**dict(meta_args(D.GEOMETRIES[0], device="cuda"), **{name: good[name]}))


def test_the_index_limit_is_a_named_constant():
    assert ops.MAX_DEFORM_INDEX == 2 ** 31 - 1 - 1024
    e = lambda *shape: torch.empty(shape, device="meta")                 # noqa: E731
    with pytest.raises(ValueError, match="MAX_DEFORM_INDEX"):            # 32 images x 4 corners x 9 taps x 2^21 outputs
        ops.deform_conv2d(e(32, 1, 2048, 1024), e(32, 18, 2048, 1024), e(1, 1, 3, 3), padding=1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_other_dtypes_are_a_type_error_that_names_float(dtype):
    good = meta_args(D.GEOMETRIES[0])
    other = meta_args(D.GEOMETRIES[0], dtype=dtype)
    for name in D.ARGS:
        with pytest.raises(TypeError, match="%s must be float32.*\\.float\\(\\)" % name):
            ops.deform_conv2d(**dict(good, **{name: other[name]}))


def test_empty_calls_on_meta():
    a = meta_args((0,) + D.GEOMETRIES[0][1:])
    assert ops.deform_conv2d(**a).shape == (0, 6, 9, 11)
    a = meta_args(D.GEOMETRIES[1][:2] + (0,) + D.GEOMETRIES[1][3:])
    assert ops.deform_conv2d(**a).shape == (2, 0, 10, 3)


def test_module_matches_torchvisions():
    torch.manual_seed(0)
    m = ops.DeformConv2d(16, 12, (3, 5), stride=2, padding=(1, 2), dilation=1, groups=4)
    sd = m.state_dict()
    assert list(sd) == ["weight", "bias"] and sd["weight"].shape == (12, 4, 3, 5) and sd["bias"].shape == (12,)
    ref = torch.nn.Conv2d(16, 12, (3, 5), stride=2, padding=(1, 2), groups=4)
    m.load_state_dict(ref.state_dict(), strict=True)
    fan_in = 4 * 3 * 5
    # kaiming_uniform_(a = sqrt(5)): gain sqrt(2 / 6), bound gain * sqrt(3 / fan_in) = 1 / sqrt(fan_in); the bias has the same bound
    bound = 1 / math.sqrt(fan_in)
    m.reset_parameters()
    for t in (m.weight, m.bias):
        assert 0.5 * bound < float(t.detach().abs().max()) <= bound
    assert repr(m) == "DeformConv2d(16, 12, kernel_size=(3, 5), stride=(2, 2), padding=(1, 2), groups=4)"
    plain = ops.DeformConv2d(3, 2, 3, dilation=2, bias=False)
    assert repr(plain) == "DeformConv2d(3, 2, kernel_size=(3, 3), stride=(1, 1), dilation=(2, 2), bias=False)"
    assert plain.bias is None and list(plain.state_dict()) == ["weight"]
    for cin, cout in ((6, 8), (8, 6)):
        with pytest.raises(ValueError, match="divisible by groups"):
            ops.DeformConv2d(cin, cout, 3, groups=4)
    a = meta_args(D.GEOMETRIES[0])
    mod = ops.DeformConv2d(8, 6, 3, padding=1, groups=2).to("meta")
    assert mod(a["input"], a["offset"], a["mask"]).shape == mod(a["input"], a["offset"]).shape == (3, 6, 9, 11)


# ---- 4. the C entry points -----------------------------------------------------------------------------------------------------------------
def geom(**changes):
    g = dict(c_in=8, height=9, width=11, c_out=6, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dilation_h=1,
             dilation_w=1, groups=2, offset_groups=2)
    g.update(changes)
    return nv.DeformGeom(**g)


BAD_GEOMETRIES = [dict(c_in=0), dict(c_out=0), dict(height=0), dict(width=0), dict(kernel_h=0), dict(kernel_w=0), dict(stride_h=0),
                  dict(stride_w=-1), dict(pad_h=-1), dict(pad_w=-1), dict(dilation_h=0), dict(dilation_w=0), dict(groups=0),
                  dict(offset_groups=0), dict(groups=3), dict(c_out=5), dict(offset_groups=3), dict(pad_h=0, dilation_h=5),
                  dict(height=1 << 16, width=1 << 16), dict(kernel_h=1 << 16, kernel_w=1 << 16, pad_h=1 << 20, pad_w=1 << 20)]


def test_entry_points_validate_before_touching_a_gpu():
    lib = nv.lib()
    P8 = 4096                                 # any aligned non-null pointer: every call below returns before a launch
    big = 1 << 40

    def calls(g, n, p=P8, ws=big):
        r = C.byref(g) if g is not None else None
        return [lib.frcnn_ops_deform_forward(r, n, p, p, None, p, None, p, p, ws, None),
                lib.frcnn_ops_deform_backward_columns(r, n, p, p, p, p, ws, None),
                lib.frcnn_ops_deform_backward_offset(r, n, p, p, None, p, p, p, None),
                lib.frcnn_ops_deform_input_plan(r, n, p, None, p, p, None),
                lib.frcnn_ops_deform_backward_input(r, n, p, p, p, p, p, p, ws, None),
                lib.frcnn_ops_deform_backward_weight(r, n, p, p, None, p, p, 0, p, ws, None)]

    for changes in BAD_GEOMETRIES:
        assert calls(geom(**changes), 1) == [EINVAL] * 6, changes
        assert lib.frcnn_ops_deform_workspace_bytes(C.byref(geom(**changes)), 1, nv.DEFORM_WS_FORWARD) == 0, changes
    assert calls(None, 1) == [EINVAL] * 6 and calls(geom(), 0) == [EINVAL] * 6 and calls(geom(), -1) == [EINVAL] * 6
    assert calls(geom(), 1 << 30) == [EINVAL] * 6                                     # columns beyond 32 bits
    assert calls(geom(), 1, p=None) == [EINVAL] * 6                                   # null pointers
    g = geom()
    stages = (nv.DEFORM_WS_FORWARD, nv.DEFORM_WS_BACKWARD_COLUMNS, nv.DEFORM_WS_BACKWARD_INPUT, nv.DEFORM_WS_BACKWARD_WEIGHT)
    need = [lib.frcnn_ops_deform_workspace_bytes(C.byref(g), 3, s) for s in stages]
    assert all(b > 0 and b % 16 == 0 for b in need)
    assert lib.frcnn_ops_deform_workspace_bytes(C.byref(g), 3, nv.DEFORM_WS_COLUMNS) == 8 * 9 * 3 * 100 * 4     # Pp = 100 for P = 99
    assert lib.frcnn_ops_deform_workspace_bytes(C.byref(g), 3, 5) == 0 and lib.frcnn_ops_deform_workspace_bytes(None, 3, 0) == 0
    r = C.byref(g)
    # a workspace one byte short, and a misaligned one
    assert lib.frcnn_ops_deform_forward(r, 3, P8, P8, None, P8, None, P8, P8, need[0] - 1, None) == EINVAL
    assert lib.frcnn_ops_deform_backward_columns(r, 3, P8, P8, P8, P8, need[1] - 1, None) == EINVAL
    assert lib.frcnn_ops_deform_backward_input(r, 3, P8, P8, P8, P8, P8, P8, need[2] - 1, None) == EINVAL
    assert lib.frcnn_ops_deform_backward_weight(r, 3, P8, P8, None, P8, P8, 0, P8, need[3] - 1, None) == EINVAL
    assert lib.frcnn_ops_deform_forward(r, 3, P8, P8, None, P8, None, P8, P8 + 4, big, None) == EINVAL
    assert lib.frcnn_ops_deform_backward_columns(r, 3, P8, P8, P8 + 8, P8, big, None) == EINVAL
    assert lib.frcnn_ops_deform_backward_offset(r, 3, P8, P8, None, P8, None, None, None) == EINVAL               # neither gradient


def test_the_abi_number_stays_21():
    assert nv.ABI_VERSION == 21 and nv.lib().frcnn_abi_version() == 21
    assert all(n in nv.SYMBOLS for n in ("frcnn_ops_deform_forward", "frcnn_ops_deform_backward_weight", "frcnn_ops_deform_workspace_bytes"))
