"""The rotated-box operators without a GPU: the restatements of tests/rotated_cases.py against independent facts, the conditions every
case must meet, the wrappers' argument checks, `meta` shapes and the C entry points' validation."""
import math

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import deform_roi_cases as D
from tests import rotated_cases as R

F32, F64 = torch.float32, torch.float64


def boxes(*rows):
    return torch.tensor(rows, dtype=F64)


# ---- 1. the IoU restatement ---------------------------------------------------------------------------------------------------------
def test_iou_restatement_is_symmetric():
    """iou(a, b) clips a in b's frame, iou(b, a) the other way round: two computations of one number."""
    b1, b2 = R.iou_case("130x65")
    m = R.iou_matrix(b1, b2)
    assert float(m.max()) > 0.5 and float((m > 0).double().mean()) > 0.05
    assert float((m - R.iou_matrix(b2, b1).t()).abs().max()) < 1e-13


def test_iou_restatement_at_angle_zero_is_the_axis_aligned_formula():
    gen = torch.Generator().manual_seed(3)
    a, b = R.random_boxes(gen, 40).double(), R.random_boxes(gen, 50).double()
    a[:, 4], b[:, 4] = 0.0, 0.0
    ca, cb = R.rotated_to_corners(a)[:, None], R.rotated_to_corners(b)[None]
    wh = (torch.minimum(ca[..., 2:], cb[..., 2:]) - torch.maximum(ca[..., :2], cb[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area_a, area_b = (a[:, 2] * a[:, 3])[:, None], (b[:, 2] * b[:, 3])[None]
    assert float(inter.max()) > 100
    assert float((R.iou_matrix(a, b) - inter / (area_a + area_b - inter)).abs().max()) < 1e-13
    assert float((R.iou_matrix(a, b, "iof") - inter / area_a).abs().max()) < 1e-13


def test_iou_restatement_on_closed_forms():
    one = lambda a, b, mode="iou": float(R.iou_pairs(boxes(a), boxes(b), mode)[0])     # noqa: E731
    # two concentric equal squares at 45 degrees: a regular octagon of area 2 (sqrt 2 - 1) s^2
    inter = 2 * (math.sqrt(2) - 1)
    assert abs(one((3, 4, 10, 10, 0.2), (3, 4, 10, 10, 0.2 + math.pi / 4)) - inter / (2 - inter)) < 1e-13
    assert abs(one((3, 4, 10, 10, 0.2), (3, 4, 10, 10, 0.2 + math.pi / 4), "iof") - inter) < 1e-13
    assert abs(inter / (2 - inter) - 1 / math.sqrt(2)) < 1e-13
    # a contained box: the area ratio
    assert abs(one((5, 5, 4, 2, 1.0), (5.5, 4.5, 20, 30, -0.4)) - 8 / 600) < 1e-14
    assert abs(one((5, 5, 4, 2, 1.0), (5.5, 4.5, 20, 30, -0.4), "iof") - 1.0) < 1e-14
    # disjoint, and touching along an edge
    assert one((0, 0, 4, 4, 0.3), (20, 0, 4, 4, 1.0)) == 0.0
    assert one((0, 0, 4, 4, 0.0), (4, 0, 4, 4, 0.0)) == 0.0
    # the same rectangle written two ways; a box against itself is exactly 1 in both precisions
    assert abs(one((20, 20, 30, 10, 0.3), (20, 20, 10, 30, 0.3 + math.pi / 2)) - 1.0) < 1e-13
    b = R.iou_case("130x130")[0]
    for dtype in (F32, F64):
        assert bool((R.iou_pairs(b, b, dtype=dtype) == 1).all())


def test_zero_rule_and_clockwise_convention_of_the_restatement():
    b, _ = R.iou_case("special")
    m = R.iou_matrix(b, b)
    rows = list(R.ZERO_RULE_ROWS)
    assert not bool(m[rows].any()) and not bool(m[:, rows].any()) and bool(torch.isfinite(m).all())
    assert bool((m[0, :2] == 1).all()) and float(m[0, 2]) > 1 - 1e-5         # row 2: the angle rounded to float32
    assert float(m[19:21, :19].max()) == 0.0 and float(m[19, 20]) == 0.0
    assert float(m[21, 22]) > 0.05
    # clockwise: the long side of (w = 10, h = 2) at +45 degrees points towards (+x, +y)
    assert float(R.iou_pairs(boxes((0, 0, 10, 2, math.pi / 4)), boxes((3, 3, 1, 1, 0)), "iof")[0]) < 1e-12 + 1 / 20
    assert float(R.iou_pairs(boxes((3, 3, 1, 1, 0)), boxes((0, 0, 10, 2, math.pi / 4)), "iof")[0]) > 0.99
    assert float(R.iou_pairs(boxes((3, -3, 1, 1, 0)), boxes((0, 0, 10, 2, math.pi / 4)), "iof")[0]) == 0.0


@pytest.mark.parametrize("name", R.IOU_CASES)
def test_iou_cases_are_finite_and_overlap(name):
    b1, b2 = R.iou_case(name)
    truth, single = R.iou_matrix(b1, b2), R.iou_matrix(b1, b2, dtype=F32)
    assert bool(torch.isfinite(truth).all()) and bool(torch.isfinite(single).all())
    if name != "1x1":
        assert float(truth.max()) > 0.1
    assert R.rel_err(single, truth) < 1e-4 if float(truth.max()) > 0 else True


# ---- 2. the NMS cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.NMS_CASES))
def test_nms_cases_keep_their_margin(name):
    case = R.nms_case(name)
    assert not bool(R.near_threshold(case["boxes"], case["thr"]).any())
    keep = R.nms_ref(case)
    n = case["boxes"].shape[0]
    assert 1 <= keep.numel() <= n and (n < 60 or keep.numel() < n)          # something is suppressed
    if case["labels"] is not None and n >= 129:
        assert len(set(case["labels"].tolist())) == 3


# ---- 3. the pooling restatement and its cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_pool_cases_meet_their_conditions(name):
    case = R.pool_case(name)
    fraction = R.check_conditions(case)
    print(name, "marked", fraction)
    if name == "2x2-cull":
        assert case["rois"].shape[0] == ops.ROI_ALIGN_ROTATED_CULL_LIST + 1
    if R.POOL_CASES[name][7] == "mixed" and case["rois"].shape[0] >= 16:
        assert [float(v) for v in case["rois"][:7, 5]] == [R.f32(v) for v in R.ANGLES]
        out = R.forward_ref(case, F64)
        assert not bool(out[list(R.INVALID_ROWS)].any()) and not bool(out[10].any()) and float(out.abs().max()) > 0.1


@pytest.mark.parametrize("name", ["13x17-c6-7x7", "13x17-c8-2x3-adaptive", "5x4-c6-adaptive", "1x1-c4-7x7-adaptive", "2x2-cull"])
def test_explicit_gradient_is_autograd_of_the_restated_forward(name):
    case = R.pool_case(name)
    x = case["input"].double().requires_grad_(True)
    R.forward_ref(case, F64, input=x).backward(case["grad"].double())
    want = R.grad_ref(case, F64)
    assert float(want.abs().max()) > 0.1
    assert float((x.grad - want).abs().max()) < 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("clockwise", [False, True])
def test_restatement_at_angle_zero_is_aligned_roi_align(clockwise):
    case = dict(R.pool_case("13x17-c6-7x7"), clockwise=clockwise)
    rois = case["rois"].clone()
    rois[:, 5] = 0.0
    case["rois"] = rois
    want = D.roi_align_ref(R.as_corner_case(case), F64)
    got = R.forward_ref(case, F64)
    assert float(want.abs().max()) > 0.1 and float((got - want).abs().max()) < 1e-12


def test_restatement_rotates_the_way_the_box_convention_says():
    """clockwise=True: the bin row at local +v of a RoI at +90 degrees lies towards -x of the image."""
    x = torch.zeros((1, 4, 9, 9))
    x[0, :, 4, 1] = 1.0                                                      # a dot left of the centre (4, 4)
    case = {"name": "dot", "input": x, "output_size": (3, 1), "sampling_ratio": 1, "aligned": False, "clockwise": True,
            "spatial_scale": 1.0, "rois": torch.tensor([[0.0, 4.0, 4.0, 2.0, 9.0, math.pi / 2]])}
    out = R.forward_ref(case, F64)[0, 0, :, 0]
    assert abs(float(out[2]) - 1.0) < 1e-6 and abs(float(out[0])) < 1e-6 and abs(float(out[1])) < 1e-6     # the angle is a float32
    assert abs(float(R.forward_ref(dict(case, clockwise=False), F64)[0, 0, 0, 0]) - 1.0) < 1e-6


# ---- 4. wrappers, modules, meta tensors ------------------------------------------------------------------------------------------------
def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_meta_shapes():
    assert ops.box_iou_rotated(meta(3, 5), meta(4, 5)).shape == (3, 4)
    assert ops.box_iou_rotated(meta(3, 5), meta(3, 5), mode="iof", aligned=True, clockwise=False).shape == (3,)
    assert ops.box_iou_rotated(meta(0, 5), meta(4, 5)).shape == (0, 4)
    for dtype in (F32, torch.float16, torch.bfloat16):
        out = ops.roi_align_rotated(meta(2, 6, 5, 4, dtype=dtype), meta(3, 6), (2, 3), 0.5, 2)
        assert out.shape == (3, 6, 2, 3) and out.dtype == dtype
    assert ops.RoIAlignRotated(7, 0.25)(meta(2, 8, 5, 4), meta(0, 6)).shape == (0, 8, 7, 7)
    x = meta(2, 6, 5, 4).requires_grad_(True)
    assert ops.roi_align_rotated(x, meta(3, 6), 2).requires_grad
    for name in ("box_iou_rotated", "nms_rotated", "roi_align_rotated", "RoIAlignRotated"):
        assert name in ops.__all__


def test_module_keeps_its_arguments():
    m = ops.RoIAlignRotated((2, 3), 0.5, sampling_ratio=2, aligned=False, clockwise=True)
    assert "output_size=(2, 3), spatial_scale=0.5, sampling_ratio=2, aligned=False, clockwise=True" in repr(m)
    d = ops.RoIAlignRotated(7, 1.0)
    assert (d.sampling_ratio, d.aligned, d.clockwise) == (0, True, False)


def test_argument_errors_name_the_argument():
    b = meta(3, 5)
    with pytest.raises(TypeError, match="boxes1"):
        ops.box_iou_rotated(meta(3, 5, dtype=F64), b)
    with pytest.raises(TypeError, match="boxes2"):
        ops.box_iou_rotated(b, [1, 2])
    with pytest.raises(ValueError, match="boxes2"):
        ops.box_iou_rotated(b, meta(3, 4))
    with pytest.raises(ValueError, match="mode"):
        ops.box_iou_rotated(b, b, mode="giou")
    with pytest.raises(ValueError, match="aligned"):
        ops.box_iou_rotated(b, meta(4, 5), aligned=True)
    with pytest.raises(ValueError, match="boxes1"):
        ops.box_iou_rotated(torch.zeros(3, 5), torch.zeros(3, 5))           # CPU tensors
    s = meta(3)
    with pytest.raises(TypeError, match="boxes"):
        ops.nms_rotated(meta(3, 5, dtype=F64), s, 0.5)
    with pytest.raises(TypeError, match="scores"):
        ops.nms_rotated(b, meta(3, dtype=F64), 0.5)
    with pytest.raises(ValueError, match="boxes"):
        ops.nms_rotated(meta(3, 4), s, 0.5)
    with pytest.raises(ValueError, match="scores"):
        ops.nms_rotated(b, meta(4), 0.5)
    with pytest.raises(TypeError, match="labels"):
        ops.nms_rotated(b, s, 0.5, labels=meta(3))
    with pytest.raises(ValueError, match="labels"):
        ops.nms_rotated(b, s, 0.5, labels=meta(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="at most"):
        ops.nms_rotated(meta(ops.MAX_NMS_BOXES + 1, 5), meta(ops.MAX_NMS_BOXES + 1), 0.5)
    x = meta(2, 6, 5, 4)
    with pytest.raises(TypeError, match="input"):
        ops.roi_align_rotated(meta(2, 6, 5, 4, dtype=F64), meta(3, 6), 2)
    with pytest.raises(ValueError, match="input"):
        ops.roi_align_rotated(meta(6, 5, 4), meta(3, 6), 2)
    with pytest.raises(TypeError, match="rois"):
        ops.roi_align_rotated(x, meta(3, 6, dtype=torch.float16), 2)
    with pytest.raises(ValueError, match="rois"):
        ops.roi_align_rotated(x, meta(3, 5), 2)
    with pytest.raises(TypeError, match="output_size"):
        ops.roi_align_rotated(x, meta(3, 6), 2.5)
    with pytest.raises(ValueError, match="output_size"):
        ops.roi_align_rotated(x, meta(3, 6), 65)
    with pytest.raises(ValueError, match="sampling_ratio"):
        ops.roi_align_rotated(x, meta(3, 6), 2, sampling_ratio=17)
    with pytest.raises(ValueError, match="output_size"):
        ops.RoIAlignRotated(0, 1.0)


# ---- 5. the C entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_invalid_arguments_without_a_gpu():
    lib = nv.lib()
    assert lib.frcnn_ops_roi_align_rotated_cull_list() == ops.ROI_ALIGN_ROTATED_CULL_LIST == R.CULL_LIST
    p = 4096                                                                  # a non-null pointer that is never dereferenced
    assert lib.frcnn_ops_box_iou_rotated(None, 3, None, 4, 0, 0, None, None) == -1
    assert lib.frcnn_ops_box_iou_rotated(p, 3, p, 4, 2, 0, p, None) == -1          # mode
    assert lib.frcnn_ops_box_iou_rotated(p, 3, p, 4, 0, 1, p, None) == -1          # aligned, n != m
    assert lib.frcnn_ops_box_iou_rotated(p, -1, p, 4, 0, 0, p, None) == -1
    assert lib.frcnn_ops_box_iou_rotated(p, ops.MAX_ROTATED_IOU_ROWS + 1, p, 4, 0, 0, p, None) == -1
    assert lib.frcnn_ops_box_iou_rotated(None, 0, None, 4, 0, 0, None, None) == 0  # empty: nothing to do
    assert lib.frcnn_ops_nms_rotated(None, None, None, 5, 0.5, None, None, 0, None) == -1
    assert lib.frcnn_ops_nms_rotated(p, p, None, 5, 0.5, p, p, lib.frcnn_ops_nms_workspace_bytes(5) - 1, None) == -1
    assert lib.frcnn_ops_nms_rotated(p, p, None, ops.MAX_NMS_BOXES + 1, 0.5, p, p, 1 << 40, None) == -1
    assert lib.frcnn_ops_nms_rotated(p, p, None, -1, 0.5, p, p, 1 << 40, None) == -1
    assert lib.frcnn_ops_nms_rotated(None, None, None, 0, 0.5, None, None, 0, None) == 0
    fwd, bwd = lib.frcnn_ops_roi_align_rotated, lib.frcnn_ops_roi_align_rotated_backward
    assert fwd(None, 1, 5, 4, 8, None, 3, 2, 3, 1.0, 2, 1, 0, None, None) == -1
    assert fwd(p, 1, 5, 4, 6, p, 3, 2, 3, 1.0, 2, 1, 0, p, None) == -1             # c % 4
    assert fwd(p, 1, 5, 4, 8, p, 3, 65, 3, 1.0, 2, 1, 0, p, None) == -1            # out_h
    assert fwd(p, 1, 5, 4, 8, p, 3, 2, 3, 1.0, 17, 1, 0, p, None) == -1            # sampling_ratio
    assert fwd(p, 0, 5, 4, 8, p, 3, 2, 3, 1.0, 2, 1, 0, p, None) == -1             # n_img
    assert fwd(p, 1, 5, 4, 8, p, -1, 2, 3, 1.0, 2, 1, 0, p, None) == -1            # k
    assert fwd(None, 1, 5, 4, 8, None, 0, 2, 3, 1.0, 2, 1, 0, None, None) == 0     # k == 0
    assert bwd(None, 3, 1, 5, 4, 8, 2, 3, 1.0, 2, 1, 0, None, None, None) == -1
    assert bwd(p, 3, 1, 5, 4, 8, 2, 0, 1.0, 2, 1, 0, p, p, None) == -1             # out_w
    assert bwd(p, 3, 1, 131072, 4, 8, 2, 3, 1.0, 2, 1, 0, p, p, None) == -1        # fh beyond the grid
    assert bwd(p, 3, 1, 5, 4, 8, 2, 3, 1.0, 2, 1, 0, p, None, None) == -1          # no d_dx
    f16, b16 = lib.frcnn_ops_roi_align_rotated_16, lib.frcnn_ops_roi_align_rotated_backward_16
    assert f16(nv.OPS_F16, p, 1, 5, 4, 12, p, 3, 2, 3, 1.0, 2, 1, 0, p, None) == -1    # c % 8
    assert f16(7, p, 1, 5, 4, 8, p, 3, 2, 3, 1.0, 2, 1, 0, p, None) == -1              # element type
    assert b16(nv.OPS_BF16, p, 3, 1, 5, 4, 12, 2, 3, 1.0, 2, 1, 0, p, p, None) == -1
    assert b16(9, p, 3, 1, 5, 4, 8, 2, 3, 1.0, 2, 1, 0, p, p, None) == -1
