"""fasterrcnn_amd.ops.riroi_align_rotated without a GPU: the names exist (this file fails on a tree without the operator), the library
exports the entry points under ABI 21 and refuses bad arguments before it touches a GPU; the wrapper checks its arguments; the fake
implementations give the shapes, dtypes and formats; riroi_align_rotated_pytorch (the blend from torch operations) equals the float64
restatement of tests/riroi_cases.py around the restatement's own pooled values; and the cases meet the conditions their tolerance
tests rely on.

Bounds.  In float64 the composition forms the blend with the restatement's own two products and one sum, so it agrees to a few ulps of
float64 (8 * 2**-53 relative to max|truth| is asked); in float32 it is held to 4 * 2**-24 relative to max|truth|, the rounding of
r = 1 - l, of two products and of one sum."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import riroi_cases as R

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = 8 * 2.0 ** -53
OURS = {"frcnn_ops_riroi_align_rotated", "frcnn_ops_riroi_align_rotated_backward", "frcnn_ops_riroi_align_rotated_16",
        "frcnn_ops_riroi_align_rotated_backward_16", "frcnn_ops_riroi_align_rotated_max_orientations"}


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_the_names_exist():
    for name in ("riroi_align_rotated", "RiRoIAlignRotated", "riroi_align_rotated_pytorch"):
        assert name in ops.__all__ and hasattr(ops, name), name
    for name in OURS:
        assert name in nv.SYMBOLS and hasattr(nv.lib(), name), name
    for name in ("riroi_align_rotated", "riroi_align_rotated_backward"):
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
    forward = [p, i, i, i, i, i, p, i, i, i, f, i, i, i, p, p]
    backward = [p, i, i, i, i, i, i, i, i, f, i, i, i, p, p, p]
    assert lib.frcnn_ops_riroi_align_rotated.argtypes == forward and lib.frcnn_ops_riroi_align_rotated_16.argtypes == [i] + forward
    assert lib.frcnn_ops_riroi_align_rotated_backward.argtypes == backward
    assert lib.frcnn_ops_riroi_align_rotated_backward_16.argtypes == [i] + backward
    assert lib.frcnn_ops_riroi_align_rotated_max_orientations.argtypes == []
    # the header's prototypes carry as many parameters
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    for name, types in (("frcnn_ops_riroi_align_rotated", forward), ("frcnn_ops_riroi_align_rotated_backward", backward)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(params.split(",")) == len(types), name


def test_the_constants():
    assert ops.MAX_RIROI_ORIENTATIONS == R.MAX_ORIENTATIONS == nv.lib().frcnn_ops_riroi_align_rotated_max_orientations() == 64
    assert ops.ROI_ALIGN_ROTATED_CULL_LIST == R.CULL_LIST == nv.lib().frcnn_ops_roi_align_rotated_cull_list()


PTR = 4096                                         # a non-NULL pointer that no refused call dereferences
GOOD = {"n_img": 2, "fh": 5, "fw": 6, "c": 16, "c_real": 16, "k": 3, "oh": 3, "ow": 2, "ns": 2, "n": 8}
BAD = [{"n_img": 0}, {"fh": 0}, {"fw": 0}, {"c": 0}, {"c": 6}, {"k": -1}, {"oh": 0}, {"ow": 65}, {"ns": 17}, {"n": 0}, {"n": 65}, {"n": 3},
       {"c_real": 0}, {"c_real": 24}, {"c_real": 12}, {"fh": 2 ** 16, "fw": 2 ** 16}, {"fh": 131072}]


def forward(lib, half, a, x=PTR, rois=PTR, out=PTR, elem=nv.OPS_F16):
    args = (x, a["n_img"], a["fh"], a["fw"], a["c"], a["c_real"], rois, a["k"], a["oh"], a["ow"], 0.5, a["ns"], a["n"], 0, out, None)
    return lib.frcnn_ops_riroi_align_rotated_16(elem, *args) if half else lib.frcnn_ops_riroi_align_rotated(*args)


def backward(lib, half, a, rois=PTR, dout=PTR, dx=PTR, elem=nv.OPS_BF16):
    args = (rois, a["k"], a["n_img"], a["fh"], a["fw"], a["c"], a["c_real"], a["oh"], a["ow"], 0.5, a["ns"], a["n"], 1, dout, dx, None)
    return lib.frcnn_ops_riroi_align_rotated_backward_16(elem, *args) if half else lib.frcnn_ops_riroi_align_rotated_backward(*args)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "16"])
def test_the_entry_points_refuse_bad_arguments_before_touching_a_gpu(half):
    lib = nv.lib()
    for bad in BAD:
        a = dict(GOOD, **bad)
        assert forward(lib, half, a) == -1, bad
        assert backward(lib, half, a) == -1, bad
    for null in ("x", "rois", "out"):
        assert forward(lib, half, GOOD, **{null: None}) == -1, null
    for null in ("rois", "dout", "dx"):
        assert backward(lib, half, GOOD, **{null: None}) == -1, null
    assert backward(lib, half, dict(GOOD, k=0), dx=None) == -1
    assert forward(lib, half, dict(GOOD, k=0), None, None, None) == 0                   # nothing to do: no launch
    if half:
        assert forward(lib, True, dict(GOOD, c=12, c_real=8)) == -1                     # whole runs of 8
        assert forward(lib, True, GOOD, elem=7) == -1 and backward(lib, True, GOOD, elem=7) == -1


# ---- the wrapper's argument checks ---------------------------------------------------------------------------------------------------------
def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("args, kwargs, error, message", [
    ((None, meta(3, 6), 3), {}, TypeError, "input must be a torch.Tensor, got NoneType"),
    ((meta(1, 16, 5, 6, dtype=F64), meta(3, 6), 3), {}, TypeError, "input must be float32, float16 or bfloat16, got torch.float64"),
    ((meta(1, 16, 5, 6), meta(3, 6, dtype=F64), 3), {}, TypeError, "rois must be float32, got torch.float64"),
    ((meta(16, 5, 6), meta(3, 6), 3), {}, ValueError, "input must be [N, C * num_orientations, H, W], got shape (16, 5, 6)"),
    ((meta(1, 16, 5, 6), meta(3, 5), 3), {}, ValueError, "rois must be a Tensor[K, 6] (batch index, cx, cy, w, h, angle), got shape (3, 5)"),
    ((meta(1, 16, 5, 6), meta(3, 6), 65), {}, ValueError, "output_size must lie in [1, 64], got (65, 65)"),
    ((meta(1, 16, 5, 6), meta(3, 6), 3), {"num_samples": 17}, ValueError, "num_samples must be <= 16, got 17"),
    ((meta(1, 16, 5, 6), meta(3, 6), 3), {"num_samples": 2.0}, TypeError, "num_samples must be an int, got 2.0"),
    ((meta(1, 12, 5, 6), meta(3, 6), 3), {}, ValueError, "num_orientations = 8 must divide the channel count, got 12 channels"),
    ((meta(1, 12, 5, 6), meta(3, 6), 3), {"num_orientations": 5}, ValueError, "num_orientations = 5 must divide the channel count, got 12 channels"),
    ((meta(1, 16, 5, 6), meta(3, 6), 3), {"num_orientations": 0}, ValueError, "num_orientations must lie in [1, 64], got 0"),
    ((meta(1, 130, 5, 6), meta(3, 6), 3), {"num_orientations": 65}, ValueError, "num_orientations must lie in [1, 64], got 65"),
    ((meta(1, 16, 5, 6), meta(3, 6), 3), {"num_orientations": True}, TypeError, "num_orientations must be an int, got True"),
])
def test_argument_errors_name_the_argument(args, kwargs, error, message):
    with pytest.raises(error) as info:
        ops.riroi_align_rotated(*args, **kwargs)
    assert message in str(info.value)


def test_cpu_tensors_are_pointed_to_the_composition():
    with pytest.raises(ValueError, match="riroi_align_rotated_pytorch"):
        ops.riroi_align_rotated(torch.zeros(1, 16, 5, 6), torch.zeros(3, 6), 3)
    with pytest.raises(ValueError, match="same K RoIs"):
        ops.riroi_align_rotated_pytorch(torch.zeros(2, 16, 3, 3), torch.zeros(3, 6), 8)
    with pytest.raises(ValueError, match="must divide the channel count"):
        ops.riroi_align_rotated_pytorch(torch.zeros(3, 12, 3, 3), torch.zeros(3, 6), 8)


def test_meta_shapes_and_the_module():
    for dtype in (F32, torch.float16, torch.bfloat16):
        out = ops.riroi_align_rotated(meta(2, 24, 12, 10, dtype=dtype), meta(6, 6), (3, 2), 0.5, 2, 8, True)
        assert out.shape == (6, 24, 3, 2) and out.dtype == dtype and out.is_contiguous(memory_format=torch.channels_last)
    dx = torch.ops.frcnn.riroi_align_rotated_backward(meta(6, 24, 3, 2), meta(6, 6), 0.5, 3, 2, 2, 8, False, 2, 24, 12, 10, True)
    assert dx.shape == (2, 24, 12, 10) and dx.is_contiguous(memory_format=torch.channels_last)
    m = ops.RiRoIAlignRotated(7, 0.25, num_samples=2, num_orientations=4, clockwise=True)
    assert (m.out_size, m.spatial_scale, m.num_samples, m.num_orientations, m.clockwise) == ((7, 7), 0.25, 2, 4, True)
    assert m(meta(1, 8, 9, 9), meta(5, 6)).shape == (5, 8, 7, 7)
    assert "num_orientations=4" in repr(m)


# ---- the cases and the composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.TOLERANCE_CASES)
def test_the_cases_meet_their_conditions(name):
    case, truth, mirror = R.make_case(name)
    R.check_conditions(case, truth)
    for angle in case["rois"][:, 5].tolist():
        left = float(R.blend(angle, case["num_orientations"])[0])
        assert 1e-3 < left < 1 - 1e-3
    assert R.plan_of(case, F64)[1] >= 1e-3
    assert R.rel_err(mirror[0], truth[0]) < 1e-5 and R.rel_err(mirror[1], truth[1]) < 1e-5


def test_the_blend_factors_of_the_wrap_angles():
    got = [R.blend(a, 8) for a in R.WRAP_ANGLES]
    assert got[0][2] == 7 and float(got[0][0]) > 0.99                                   # ind = -1: k = n - 1, l near 1
    assert got[1][2] == 0 and got[2][2] == (math.floor(-7.0 * 8 / (2 * math.pi)) % 8) == 7
    assert [g[2] for g in got[3:]] in ([0, 1, 1], [0, 0, 1], [1, 1, 1], [0, 0, 0])        # f next to 1 from either side
    assert R.blend(R.NAN, 8) is None and R.blend(R.INF, 8) is None and R.blend(2.0 ** 24, 8) is None
    assert R.blend(0.0, 8) == (0.0, 1.0, 0)


def test_the_restatements_grid_is_the_published_one():
    """x = xx cos t - yy sin t + cx, y = xx sin t + yy cos t + cy with t = clockwise ? -angle : angle, against plan_of's expressions."""
    for clockwise in (False, True):
        a, yy, xx = 0.7, 1.25, -0.5
        t = -a if clockwise else a
        tp = a if clockwise else -a                                                      # what plan_of takes
        x, y = xx * math.cos(t) - yy * math.sin(t), xx * math.sin(t) + yy * math.cos(t)
        assert abs((yy * math.sin(tp) + xx * math.cos(tp)) - x) < 1e-15 and abs((yy * math.cos(tp) - xx * math.sin(tp)) - y) < 1e-15


@pytest.mark.parametrize("name", ["n8-c2", "n8-c2-adaptive-clockwise", "n1-c5", "n3-c3", "n3-c86"])
def test_the_composition_is_the_restatements_blend(name):
    case, truth, mirror = R.make_case(name)
    n = case["num_orientations"]
    s = truth[2].clone().requires_grad_(True)
    out = ops.riroi_align_rotated_pytorch(s, case["rois"].double(), n)
    assert out.dtype == F64 and R.rel_err(out.detach(), truth[0]) <= ULPS
    out.backward(case["grad"].double())
    assert torch.allclose(s.grad.float(), R.blended_grad(case), rtol=1e-6, atol=1e-6)
    out32 = ops.riroi_align_rotated_pytorch(truth[2].float(), case["rois"], n)
    assert out32.dtype == F32 and R.rel_err(out32, truth[0]) <= 4 * 2.0 ** -24
    half = ops.riroi_align_rotated_pytorch(truth[2].half(), case["rois"], n)
    assert half.dtype == torch.float16


def test_the_composition_skips_what_the_contract_skips():
    case = R.skipped_case()
    s = torch.ones((6, 16, 3, 2))
    out = ops.riroi_align_rotated_pytorch(s, case["rois"], 8)
    assert float((out[:3] - 1).abs().max()) <= 2.0 ** -23 and not bool(out[3:].any())     # r + l is 1 to a rounding; rows 3.. are zeros
    assert np.isfinite(out.numpy()).all()
