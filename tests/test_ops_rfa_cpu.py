"""fasterrcnn_amd.ops.rotated_feature_align without a GPU: the names exist (this file fails on a tree without the operator), the library
exports the entry points under ABI 21 and refuses bad arguments before it touches a GPU; the wrapper checks its arguments; the fake
implementations give the shapes, dtypes and formats; rotated_feature_align_pytorch (the composition from index gathers, the CPU route)
equals the float64 restatement of tests/rfa_cases.py; and the cases meet the conditions their tolerance tests rely on.

Bounds.  In float64 the composition forms every sample with the restatement's own expressions in the restatement's order, so its output
agrees to a few ulps of float64 (8 * 2**-53 relative to max|truth| is asked) and d_features, the same terms summed per cell in
another order, to 1e-12.  In float32 it is held to the rule the kernels are held to: err <= 4 * max(err_ref, 2**-24) with err_ref the
float32 mirror's own error."""
import ctypes
import os
import re

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import rfa_cases as A

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = 8 * 2.0 ** -53
SAME_SUMS = 1e-12
MARGIN = 4.0
FLOOR = 2.0 ** -24
OURS = {"frcnn_ops_rotated_feature_align", "frcnn_ops_rotated_feature_align_plan", "frcnn_ops_rotated_feature_align_backward",
        "frcnn_ops_rotated_feature_align_16", "frcnn_ops_rotated_feature_align_backward_16"}


def compose(case, dtype):
    x = case["input"].to(dtype).clone().requires_grad_(True)          # the cases are shared: never the tensor itself
    out = ops.rotated_feature_align_pytorch(x, case["boxes"].to(dtype), case["spatial_scale"], case["points"])
    out.backward(case["grad"].to(dtype))
    return out.detach(), x.grad


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_the_names_exist():
    for name in ("rotated_feature_align", "RotatedFeatureAlign", "rotated_feature_align_pytorch"):
        assert name in ops.__all__ and hasattr(ops, name), name
    for name in OURS:
        assert name in nv.SYMBOLS and hasattr(nv.lib(), name), name
    for name in ("rotated_feature_align", "rotated_feature_align_backward"):
        assert hasattr(torch.ops.frcnn, name), name


def test_the_library_exports_the_entry_points_under_abi_21():
    text = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert re.search(r"#define FRCNN_ABI_VERSION (\d+)", text).group(1) == "21"
    assert nv.ABI_VERSION == 21 == nv.lib().frcnn_abi_version()
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert OURS <= declared and declared == set(nv.SYMBOLS)


def test_the_argument_types_are_the_declared_ones():
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    lib = nv.lib()
    forward, plan, backward = [p, p, i, i, i, i, f, i, p, p], [p, i, i, i, f, i, p, p, p], [p, p, p, p, i, i, i, i, i, p, p]
    assert lib.frcnn_ops_rotated_feature_align.argtypes == forward and lib.frcnn_ops_rotated_feature_align_16.argtypes == [i] + forward
    assert lib.frcnn_ops_rotated_feature_align_plan.argtypes == plan
    assert lib.frcnn_ops_rotated_feature_align_backward.argtypes == backward
    assert lib.frcnn_ops_rotated_feature_align_backward_16.argtypes == [i] + backward
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    for name, types in (("frcnn_ops_rotated_feature_align", forward), ("frcnn_ops_rotated_feature_align_plan", plan),
                        ("frcnn_ops_rotated_feature_align_backward", backward)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(params.split(",")) == len(types), name


def test_the_constants():
    assert ops.RFA_POINTS == (1, 5) and ops.MAX_RFA_INDEX == 2 ** 31 - 1 - 1024
    assert ops.MSDA_SEGMENT == A.SEGMENT == nv.lib().frcnn_ops_msda_segment()
    assert A.LONG_SIDE ** 2 > A.SEGMENT                                # the long-segment case is past one segment


PTR = 4096                                         # a non-NULL pointer that no refused call dereferences
GOOD = {"n_img": 2, "fh": 5, "fw": 6, "c": 8, "points": 5}
BAD = [{"n_img": -1}, {"fh": 0}, {"fw": 0}, {"c": 0}, {"c": 6}, {"points": 3}, {"points": 0}, {"points": 4}, {"fh": 2 ** 16, "fw": 2 ** 16},
       {"n_img": 2 ** 10, "fh": 2 ** 10, "fw": 2 ** 10}]


def forward(lib, half, a, x=PTR, boxes=PTR, out=PTR, elem=nv.OPS_F16):
    args = (x, boxes, a["n_img"], a["fh"], a["fw"], a["c"], 0.125, a["points"], out, None)
    return lib.frcnn_ops_rotated_feature_align_16(elem, *args) if half else lib.frcnn_ops_rotated_feature_align(*args)


def backward(lib, half, a, keys=PTR, order=PTR, wts=PTR, dout=PTR, dx=PTR, elem=nv.OPS_BF16):
    args = (keys, order, wts, dout, a["n_img"], a["fh"], a["fw"], a["c"], a["points"], dx, None)
    return lib.frcnn_ops_rotated_feature_align_backward_16(elem, *args) if half else lib.frcnn_ops_rotated_feature_align_backward(*args)


def plan(lib, a, boxes=PTR, keys=PTR, wts=PTR):
    return lib.frcnn_ops_rotated_feature_align_plan(boxes, a["n_img"], a["fh"], a["fw"], 0.125, a["points"], keys, wts, None)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "16"])
def test_the_entry_points_refuse_bad_arguments_before_touching_a_gpu(half):
    lib = nv.lib()
    for bad in BAD:
        a = dict(GOOD, **bad)
        assert forward(lib, half, a) == -1, bad
        assert backward(lib, half, a) == -1, bad
        if "c" not in bad:
            assert plan(lib, a) == -1, bad
    for null in ("x", "boxes", "out"):
        assert forward(lib, half, GOOD, **{null: None}) == -1, null
    for null in ("keys", "order", "wts", "dout", "dx"):
        assert backward(lib, half, GOOD, **{null: None}) == -1, null
    for null in ("boxes", "keys", "wts"):
        assert plan(lib, GOOD, **{null: None}) == -1, null
    empty = dict(GOOD, n_img=0)                                        # nothing to do: no launch
    assert forward(lib, half, empty, None, None, None) == 0 and plan(lib, empty, None, None, None) == 0
    assert backward(lib, half, empty, None, None, None, None, None) == 0
    if half:
        assert forward(lib, True, dict(GOOD, c=12)) == -1 and backward(lib, True, dict(GOOD, c=12)) == -1      # whole runs of 8
        assert forward(lib, True, GOOD, elem=7) == -1 and backward(lib, True, GOOD, elem=7) == -1


# ---- the wrapper's argument checks ---------------------------------------------------------------------------------------------------------
def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("args, error, message", [
    ((None, meta(1, 5, 6, 5)), TypeError, "features must be a torch.Tensor, got NoneType"),
    ((meta(1, 8, 5, 6, dtype=F64), meta(1, 5, 6, 5)), TypeError, "features must be float32, float16 or bfloat16, got torch.float64"),
    ((meta(1, 8, 5, 6), meta(1, 5, 6, 5, dtype=F64)), TypeError, "best_bboxes must be float32, got torch.float64"),
    ((meta(8, 5, 6), meta(1, 5, 6, 5)), ValueError, "features must be [N, C, H, W], got shape (8, 5, 6)"),
    ((meta(1, 8, 5, 6), meta(1, 5, 6, 4)), ValueError, "best_bboxes must be [N, H, W, 5] = (1, 5, 6, 5)"),
    ((meta(1, 8, 5, 6), meta(1, 6, 5, 5)), ValueError, "got shape (1, 6, 5, 5)"),
    ((meta(2, 8, 5, 6), meta(1, 5, 6, 5)), ValueError, "best_bboxes must be [N, H, W, 5] = (2, 5, 6, 5)"),
    ((meta(1, 8, 5, 6), meta(1, 5, 6, 5), 0.125, 3), ValueError, "points must be 1 or 5, got 3"),
    ((meta(1, 8, 5, 6), meta(1, 5, 6, 5), 0.125, 5.0), TypeError, "points must be an int, got 5.0"),
    ((meta(2 ** 10, 4, 2 ** 10, 2 ** 10), meta(2 ** 10, 2 ** 10, 2 ** 10, 5), 0.125, 5), ValueError,
     "N H W points 4 = 21474836480 exceeds 2147482623"),
])
def test_argument_errors_name_the_argument(args, error, message):
    with pytest.raises(error) as info:
        ops.rotated_feature_align(*args)
    assert message in str(info.value)
    if error is ValueError and "features must be" not in message:
        with pytest.raises(ValueError):                                # the composition shares the shape rules
            ops.rotated_feature_align_pytorch(*(torch.empty(a.shape) if isinstance(a, torch.Tensor) and a.numel() < 10 ** 6 else a
                                                for a in args))


def test_cpu_tensors_are_pointed_to_the_composition():
    with pytest.raises(ValueError, match="rotated_feature_align_pytorch runs on any device"):
        ops.rotated_feature_align(torch.zeros(1, 8, 5, 6), torch.zeros(1, 5, 6, 5))
    with pytest.raises(ValueError, match="points must be 1 or 5"):
        ops.RotatedFeatureAlign(points=3)


def test_meta_shapes_and_the_module():
    for dtype in (F32, torch.float16, torch.bfloat16):
        for cl in (False, True):
            x = meta(2, 12, 6, 7, dtype=dtype)
            x = x.contiguous(memory_format=torch.channels_last) if cl else x
            out = ops.rotated_feature_align(x, meta(2, 6, 7, 5), 0.125, 5)
            assert out.shape == x.shape and out.dtype == dtype
            assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    dx = torch.ops.frcnn.rotated_feature_align_backward(meta(2, 12, 6, 7), meta(2, 6, 7, 5), 0.125, 5, True)
    assert dx.shape == (2, 12, 6, 7) and dx.is_contiguous(memory_format=torch.channels_last)
    m = ops.RotatedFeatureAlign(spatial_scale=0.25, points=5)
    assert (m.spatial_scale, m.points) == (0.25, 5) and m(meta(1, 4, 3, 3), meta(1, 3, 3, 5)).shape == (1, 4, 3, 3)
    assert ops.RotatedFeatureAlign().points == 1 and ops.RotatedFeatureAlign().spatial_scale == 0.125


# ---- the cases and the composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.TOLERANCE_CASES)
def test_the_cases_meet_their_conditions(name):
    case, truth, mirror = A.make_case(name)
    A.check_conditions(case, truth)
    assert truth[2] >= 1e-3                                             # no sample within 1e-3 of an integer coordinate
    assert A.rel_err(mirror[0], truth[0]) < 1e-5 and A.rel_err(mirror[1], truth[1]) < 1e-5


@pytest.mark.parametrize("name", A.TOLERANCE_CASES)
def test_the_composition_equals_the_restatement(name):
    case, truth, mirror = A.make_case(name)
    out, dx = compose(case, F64)
    assert out.dtype == F64 and A.rel_err(out, truth[0]) <= ULPS and A.rel_err(dx, truth[1]) <= SAME_SUMS
    out, dx = compose(case, F32)
    for label, got, t, m in (("output", out, truth[0], mirror[0]), ("d_features", dx, truth[1], mirror[1])):
        err, err_ref = A.rel_err(got, t), A.rel_err(m, t)
        print("%s %-10s err %.3e err_ref %.3e" % (name, label, err, err_ref))
        assert got.dtype == F32 and err <= MARGIN * max(err_ref, FLOOR), (name, label, err, err_ref)


def test_the_composition_on_the_special_cases():
    case, counted, total = A.range_case()
    out, dx = compose(case, F64)
    want = A.reference(case, F64)
    assert A.rel_err(out, want[0]) <= ULPS and A.rel_err(dx, want[1]) <= SAME_SUMS
    flat = (out - case["input"].double()).flatten(2)[0]                 # what the samples added, per pixel
    assert bool(flat[:, :counted].abs().amax(0).gt(0).all()) and not bool(flat[:, counted:total].any())
    for points in (1, 5):
        case, rows = A.bad_rows_case(points)
        out, dx = compose(case, F64)
        want = A.reference(case, F64)
        assert bool(torch.isfinite(out).all()) and A.rel_err(out, want[0]) <= ULPS and A.rel_err(dx, want[1]) <= SAME_SUMS
    case = A.dyadic_case()
    out, dx = compose(case, F32)
    want = A.reference(case, F64)
    assert torch.equal(out.double(), want[0]) and torch.equal(dx.double(), want[1])
    half = ops.rotated_feature_align_pytorch(case["input"].half(), case["boxes"], 0.5, 5)
    assert half.dtype == torch.float16
