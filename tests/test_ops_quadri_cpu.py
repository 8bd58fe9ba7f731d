"""fasterrcnn_amd.ops.box_iou_quadri / nms_quadri / points_in_polygons without a GPU: the conditions of the cases (tests/quadri_cases.py),
the two restatements against independent facts and against each other, the torch compositions against the float64 truth, the argument
rules of the public functions, shapes and dtypes on meta and fake tensors, the header's ABI line and the validation of the C entry points.

Measured here: analytic(float64) agrees with the truth to 2.7e-15 (iou and iof, aligned and matrix cases), near x = 4096 to 9.9e-14 (the
truth clips on raw coordinates); the float64 compositions agree with the truth to 3e-14."""
import itertools
import os

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import ShapeEnv

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import quadri_cases as Q

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("box_iou_quadri", "nms_quadri", "points_in_polygons", "box_iou_quadri_pytorch", "points_in_polygons_pytorch")


def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def quad(*coords):
    return [(float(coords[i]), float(coords[i + 1])) for i in range(0, 8, 2)]


# ---- 1. the cases and the restatements ----------------------------------------------------------------------------------------------------
def test_conditions_of_the_cases():
    Q.check_conditions()
    assert Q.TILE_ROWS == ops.QUADRI_IOU_TILE_ROWS and Q.POINT_ROWS == ops.POINTS_IN_POLYGONS_TILE_ROWS
    assert Q.MIN_AREA == ops.CONVEX_MIN_AREA
    assert len(Q.NMS_CASES) == 30


def test_truth_against_independent_facts():
    square, shifted = quad(0, 0, 4, 0, 4, 4, 0, 4), quad(2, 1, 6, 1, 6, 5, 2, 5)
    iou, iof = Q.truth_pair(square, shifted)                                 # the axis-aligned closed form: 2 x 3 of 16 + 16 - 6
    assert iou == 6 / 26 and iof == 6 / 16
    assert Q.truth_pair(square, square) == (1.0, 1.0)
    assert Q.truth_pair(quad(1, 1, 3, 1, 3, 2, 1, 2), square) == (2 / 16, 1.0)                 # inside: iof 1
    assert Q.truth_pair(square, quad(4, 0, 8, 0, 8, 4, 4, 4)) == (0.0, 0.0)                    # a shared edge only
    assert Q.truth_pair(square, quad(0, 0, 1, 1, 2, 2, 3, 3)) == (0.0, 0.0)                    # collinear: dead
    diamond = quad(2, -1, 5, 2, 2, 5, -1, 2)                                 # the square's octagon: 16 - 4 * 0.5
    assert Q.truth_pair(square, diamond)[0] == 14 / (16 + 18 - 14)
    arrow = quad(0, 0, 6, 0, 2, 1, 0, 6)                                     # (2, 1) lies inside the triangle of the other three
    assert Q.truth_hull(arrow) == [(0.0, 0.0), (6.0, 0.0), (0.0, 6.0)]
    assert Q.truth_pair(arrow, square) == Q.truth_pair(quad(0, 0, 6, 0, 0, 6, 0, 6), square)
    for name in ("65", "near4096"):                                          # symmetry of iou, and every vertex order gives one value
        a, b = Q.case(name)
        back = [Q.truth_pair(q, p)[0] for p, q in zip(Q._rows(a), Q._rows(b))]
        assert float((torch.tensor(back, dtype=F64) - Q.truth(name)["iou"]).abs().max()) <= 1e-12
    p, q = Q._rows(Q.case("65")[0])[3], Q._rows(Q.case("65")[1])[3]
    want = Q.truth_pair(p, q)
    for perm in itertools.permutations(range(4)):
        got = Q.truth_pair([p[i] for i in perm], q)
        assert abs(got[0] - want[0]) <= 1e-14 and abs(got[1] - want[1]) <= 1e-14


@pytest.mark.parametrize("name", Q.ALIGNED_CASES)
def test_restatement_in_float64_is_the_truth(name):
    a, b = Q.case(name)
    bound = 1e-12 if name == "near4096" else 1e-13                         # the truth clips on raw coordinates: 4096 / 40 times the rounding
    for mode in Q.MODES:
        got = Q.analytic(a, b, mode, F64)
        worst = float((got - Q.truth(name)[mode]).abs().max())
        print(name, mode, worst)
        assert worst <= bound and torch.equal(got == 0, Q.truth(name)[mode] == 0)


@pytest.mark.parametrize("name", ("65", "near4096"))
def test_the_array_restatement_is_the_scalar_one_bit_for_bit(name):
    a, b = Q.case(name)
    for mode in Q.MODES:
        for dtype in (F32, F64):
            assert torch.equal(Q.analytic(a, b, mode, dtype), Q.analytic_scalar(a, b, mode, dtype)), (mode, dtype)
    rows, cols = Q.matrix_case("7x130")
    assert torch.equal(Q.analytic_matrix(rows, cols, "iou", F32)[:, :7].diagonal(), Q.analytic_scalar(rows, cols[:7], "iou", F32))


@pytest.mark.parametrize("name", ("63x65", "130x7", "%dx9" % (Q.TILE_ROWS + 1)))
def test_matrix_restatement_in_float64_is_the_truth(name):
    rows, cols = Q.matrix_case(name)
    for mode in Q.MODES:
        got, want = Q.analytic_matrix(rows, cols, mode, F64), Q.matrix_truth(name)[mode]
        assert float((got - want).abs().max()) <= 1e-13 and torch.equal(got == 0, want == 0)


def test_restatement_takes_the_arrow_as_its_hull_in_any_vertex_order():
    T = np.float32
    square = Q.analytic_hull([0, 0, 4, 0, 4, 4, 0, 4], T)
    arrow, triangle = [0, 0, 6, 0, 2, 1, 0, 6], [0, 0, 6, 0, 0, 6, 0, 6]
    assert list(zip(Q.analytic_hull(arrow, T)["x"], Q.analytic_hull(arrow, T)["y"])) == [(0, 0), (6, 0), (0, 6)]
    want = Q.analytic_pair(Q.analytic_hull(triangle, T), square, "iou", T)
    assert want > 0
    pts = [arrow[2 * i:2 * i + 2] for i in range(4)]
    for perm in itertools.permutations(range(4)):
        row = [c for i in perm for c in pts[i]]
        assert Q.analytic_pair(Q.analytic_hull(row, T), square, "iou", T) == want
        assert Q.analytic_pair(square, Q.analytic_hull(row, T), "iof", T) == Q.analytic_pair(square, Q.analytic_hull(triangle, T), "iof", T)
    assert Q.analytic_pair(square, square, "iou", T) == 1 and Q.analytic_pair(square, square, "iof", T) == 1
    for dead in ([0, 0, 1, 1, 2, 2, 3, 3], [5, 5] * 4, [float("nan"), 0, 4, 0, 4, 4, 0, 4], [0, 0, float("inf"), 0, 4, 4, 0, 4]):
        assert Q.analytic_hull(dead, T) is None


def test_points_restatements_on_exact_coordinates():
    polys = torch.tensor([[0, 0, 4, 0, 4, 4, 0, 4], [4, 4, 0, 0, 0, 4, 4, 0], [0, 0, 1, 1, 2, 2, 3, 3]], dtype=F32)
    points = torch.tensor([[2, 2], [0, 0], [4, 2], [2, 4], [5, 2], [2, -1], [-1, -1], [float("nan"), 2], [2, float("inf")]], dtype=F32)
    want = torch.tensor([[1, 1, 0]] * 4 + [[0, 0, 0]] * 5, dtype=F64)
    assert torch.equal(Q.truth_inside(points, polys), want)
    assert torch.equal(Q.analytic_inside(points, polys, F32).double(), want)
    assert torch.equal(Q.analytic_inside(points, polys, F64), want)


# ---- 2. the torch compositions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("65", "130", "near4096"))
def test_compositions_against_the_truth(name):
    a, b = Q.case(name)
    for mode in Q.MODES:
        got = ops.box_iou_quadri_pytorch(a.double(), b.double(), mode, aligned=True)
        assert got.dtype == F64 and got.shape == (a.shape[0],)
        assert float((got - Q.truth(name)[mode]).abs().max()) <= 1e-11 and torch.equal(got == 0, Q.truth(name)[mode] == 0)
        single = ops.box_iou_quadri_pytorch(a, b, mode, aligned=True)
        assert single.dtype == F32 and Q.rel_err(single, Q.truth(name)[mode]) <= 1e-4


def test_matrix_and_points_compositions_against_the_truth():
    rows, cols = Q.matrix_case("65x63")
    for mode in Q.MODES:
        got = ops.box_iou_quadri_pytorch(rows.double(), cols.double(), mode)
        assert float((got - Q.matrix_truth("65x63")[mode]).abs().max()) <= 1e-11
    assert torch.equal(ops.box_iou_quadri_pytorch(rows.double(), cols.double()).diagonal(),
                       ops.box_iou_quadri_pytorch(rows[:63].double(), cols.double(), aligned=True))
    for name in ("65x63", "%dx5" % (Q.POINT_ROWS + 1)):
        points, polys, _ = Q.point_case(name)
        want = Q.truth_inside(points, polys)
        assert torch.equal(ops.points_in_polygons_pytorch(points.double(), polys.double()), want)
        assert torch.equal(ops.points_in_polygons_pytorch(points, polys).double(), want)
    dead = torch.tensor([[0, 0, 1, 1, 2, 2, 3, 3], [float("nan"), 0, 4, 0, 4, 4, 0, 4]], dtype=F64)
    assert not bool(ops.box_iou_quadri_pytorch(dead, cols.double()).any()) and not bool(ops.box_iou_quadri_pytorch(rows.double(), dead).any())
    assert not bool(ops.points_in_polygons_pytorch(torch.tensor([[1.0, 1.0]], dtype=F64), dead).any())
    assert not bool(ops.points_in_polygons_pytorch(torch.tensor([[float("inf"), 1.0]]), cols).any())


def test_compositions_arguments_and_empty_inputs():
    a, b = Q.case("63")
    assert ops.box_iou_quadri_pytorch(a[:0], b).shape == (0, 63) and ops.box_iou_quadri_pytorch(a, b[:0]).shape == (63, 0)
    assert ops.box_iou_quadri_pytorch(a[:0], b[:0], aligned=True).shape == (0,)
    assert ops.points_in_polygons_pytorch(a[:0, :2], b).shape == (0, 63) and ops.points_in_polygons_pytorch(a[:, :2], b[:0]).shape == (63, 0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.box_iou_quadri_pytorch(a, [1.0])
    with pytest.raises(TypeError, match="float16"):
        ops.points_in_polygons_pytorch(a[:, :2].half(), b)
    with pytest.raises(ValueError, match=r"\(63, 7\)"):
        ops.box_iou_quadri_pytorch(a[:, :7], b)
    with pytest.raises(ValueError, match=r"points must be \[N, 2\].*\(63, 8\)"):
        ops.points_in_polygons_pytorch(a, b)
    with pytest.raises(ValueError, match="63 and 60"):
        ops.box_iou_quadri_pytorch(a, b[:60], aligned=True)
    with pytest.raises(ValueError, match="'giou'"):
        ops.box_iou_quadri_pytorch(a, b, mode="giou")


# ---- 3. the public functions: names, errors, meta -------------------------------------------------------------------------------------------
def test_names_are_exported_and_documented():
    for name in NAMES:
        assert name in ops.__all__ and callable(getattr(ops, name)) and name in ops.__doc__ and getattr(ops, name).__doc__
    for name in NAMES[3:]:
        assert "GENERAL POSITION" in getattr(ops, name).__doc__, name
    assert "from fasterrcnn_amd.ops import box_iou_quadri, nms_quadri, points_in_polygons" in ops.__doc__
    assert "deliberate deviation from mmcv" in ops.__doc__ and "half-open" in ops.__doc__
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in NAMES[:3]:
        assert name in integration and name in readme, name
    assert "ops_quadri.hip" in open(os.path.join(ROOT, "fasterrcnn_amd", "csrc", "Makefile")).read()


def test_constants_mirror_the_library_and_the_header_keeps_abi_21():
    lib = nv.lib()
    assert ops.QUADRI_IOU_TILE_ROWS == lib.frcnn_ops_box_iou_quadri_tile_rows()
    assert ops.POINTS_IN_POLYGONS_TILE_ROWS == lib.frcnn_ops_points_in_polygons_tile_rows()
    assert ops.MAX_QUADRI_ROWS == lib.frcnn_ops_quadri_max_rows() == ops.MAX_CONVEX_ROWS
    assert ops.MAX_QUADRI_COLUMNS == lib.frcnn_ops_quadri_max_columns()
    assert lib.frcnn_abi_version() == 21
    header = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert "#define FRCNN_ABI_VERSION 21" in " ".join(header.split())
    assert "still 21 (additions only): frcnn_ops_box_iou_quadri" in header
    for text in ("frcnn_ops_nms_quadri", "frcnn_ops_points_in_polygons", "ONE DELIBERATE DEVIATION", "half-open", "five copies"):
        assert text in header, text


def test_argument_errors():
    quads, points = meta(5, 8), meta(5, 2)
    calls = {"box_iou_quadri": (lambda a, b: ops.box_iou_quadri(a, b), "bboxes1", "bboxes2", quads),
             "points_in_polygons": (lambda a, b: ops.points_in_polygons(a, b), "points", "polygons", points)}
    for name, (fn, first, second, good) in calls.items():
        width = good.shape[1]
        with pytest.raises(TypeError, match="%s must be a torch.Tensor" % first):
            fn([[0.0] * width], quads)
        with pytest.raises(TypeError, match="%s must be float32.*float64" % first):
            fn(good.double(), quads)
        for dtype in (torch.float16, torch.bfloat16):
            with pytest.raises(TypeError, match=r"\.float\(\)"):
                fn(meta(5, width, dtype=dtype), quads)
        with pytest.raises(ValueError, match=r"%s must be \[N, %d\].*\(5, 6\)" % (first, width)):
            fn(meta(5, 6), quads)
        with pytest.raises(ValueError, match=r"\(8,\)"):
            fn(meta(8), quads)
        with pytest.raises(ValueError, match="no CPU implementation.*%s_pytorch runs on any device" % name):
            fn(torch.zeros(5, width), torch.zeros(5, 8))
        with pytest.raises(TypeError, match="%s must be a torch.Tensor" % second):
            fn(good, None)
        with pytest.raises(TypeError, match="%s must be float32" % second):
            fn(good, quads.double())
        with pytest.raises(ValueError, match=r"%s must be \[N, 8\].*\(5, 10\)" % second):
            fn(good, meta(5, 10))
        with pytest.raises(ValueError, match="cpu"):
            fn(good, torch.zeros(5, 8))                                       # one on meta, one on the CPU
        with FakeTensorMode():
            with pytest.raises(ValueError, match="same device"):
                fn(torch.empty((5, width), device="cuda:0"), torch.empty((5, 8), device="cuda:1"))
        with pytest.raises(ValueError, match="MAX_QUADRI_ROWS = %d rows, got %d" % (ops.MAX_QUADRI_ROWS, ops.MAX_QUADRI_ROWS + 1)):
            fn(meta(ops.MAX_QUADRI_ROWS + 1, width), quads)
        with pytest.raises(ValueError, match="MAX_QUADRI_COLUMNS = %d rows, got %d" % (ops.MAX_QUADRI_COLUMNS, ops.MAX_QUADRI_COLUMNS + 1)):
            fn(good, meta(ops.MAX_QUADRI_COLUMNS + 1, 8))
    with pytest.raises(ValueError, match="mode must be 'iou' or 'iof', got 'giou'"):
        ops.box_iou_quadri(quads, quads, mode="giou")
    with pytest.raises(ValueError, match="aligned=True needs bboxes1 and bboxes2 of one length, got 5 and 4"):
        ops.box_iou_quadri(quads, meta(4, 8), aligned=True)
    assert ops.box_iou_quadri(meta(ops.MAX_QUADRI_COLUMNS + 1, 8), meta(ops.MAX_QUADRI_COLUMNS + 1, 8), aligned=True).dim() == 1
    scores = meta(5)
    with pytest.raises(TypeError, match="dets must be a torch.Tensor"):
        ops.nms_quadri(None, scores, 0.5)
    with pytest.raises(TypeError, match="dets must be float32.*float64"):
        ops.nms_quadri(quads.double(), scores, 0.5)
    with pytest.raises(ValueError, match=r"dets must be \[N, 8\].*\(5, 5\)"):
        ops.nms_quadri(meta(5, 5), scores, 0.5)
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.nms_quadri(torch.zeros(5, 8), torch.zeros(5), 0.5)
    with pytest.raises(TypeError, match="scores must be float32"):
        ops.nms_quadri(quads, scores.double(), 0.5)
    with pytest.raises(ValueError, match=r"scores must be \[N\] with N = 5, got shape \(4,\)"):
        ops.nms_quadri(quads, meta(4), 0.5)
    with FakeTensorMode():
        with pytest.raises(ValueError, match="dets and scores must be on the same device"):
            ops.nms_quadri(torch.empty((5, 8), device="cuda:0"), torch.empty((5,), device="cuda:1"), 0.5)
        with pytest.raises(ValueError, match="dets and labels must be on the same device"):
            ops.nms_quadri(torch.empty((5, 8), device="cuda:0"), torch.empty((5,), device="cuda:0"), 0.5,
                           labels=torch.empty((5,), dtype=torch.int64, device="cuda:1"))
    with pytest.raises(TypeError, match="labels must be an integer tensor"):
        ops.nms_quadri(quads, scores, 0.5, labels=meta(5))
    with pytest.raises(ValueError, match=r"labels must be \[N\] with N = 5, got shape \(4,\)"):
        ops.nms_quadri(quads, scores, 0.5, labels=meta(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="nms_quadri takes at most %d boxes, got %d" % (ops.MAX_NMS_BOXES, ops.MAX_NMS_BOXES + 1)):
        ops.nms_quadri(meta(ops.MAX_NMS_BOXES + 1, 8), meta(ops.MAX_NMS_BOXES + 1), 0.5)
    with pytest.raises(ValueError, match="nms_rotated takes at most %d boxes" % ops.MAX_NMS_BOXES):     # the shared checks keep its wording
        ops.nms_rotated(meta(ops.MAX_NMS_BOXES + 1, 5), meta(ops.MAX_NMS_BOXES + 1), 0.5)


def test_meta_and_fake_shapes_and_dtypes():
    for n, m in ((5, 3), (0, 3), (5, 0), (70, 130)):
        for mode in Q.MODES:
            out = ops.box_iou_quadri(meta(n, 8).requires_grad_(True), meta(m, 8), mode)
            assert out.shape == (n, m) and out.dtype == F32 and not out.requires_grad
        hit = ops.points_in_polygons(meta(n, 2).requires_grad_(True), meta(m, 8))
        assert hit.shape == (n, m) and hit.dtype == F32 and not hit.requires_grad
    for n in (0, 1, 70):
        assert ops.box_iou_quadri(meta(n, 8), meta(n, 8), aligned=True).shape == (n,)
    with FakeTensorMode(shape_env=ShapeEnv()):
        quads = torch.empty((6, 8), device="cuda")
        assert ops.box_iou_quadri(quads, torch.empty((9, 8), device="cuda")).shape == (6, 9)
        assert ops.box_iou_quadri(quads, quads, "iof", True).shape == (6,)
        assert ops.points_in_polygons(torch.empty((4, 2), device="cuda"), quads).shape == (4, 6)
        dets, keep = ops.nms_quadri(quads, torch.empty((6,), device="cuda"), 0.5, labels=torch.empty((6,), dtype=torch.int64, device="cuda"))
        assert dets.dim() == 2 and dets.shape[1] == 9 and keep.dtype == torch.int64 and keep.dim() == 1 and dets.device.type == "cuda"


# ---- 4. FRCNN_EINVAL of the entry points, with null pointers and no device --------------------------------------------------------------------
def test_entry_points_validate_before_touching_the_gpu():
    lib, p = nv.lib(), 0x1000                                              # never dereferenced: every call below fails validation first
    iou, nms, pip = lib.frcnn_ops_box_iou_quadri, lib.frcnn_ops_nms_quadri, lib.frcnn_ops_points_in_polygons
    rows, cols = ops.MAX_QUADRI_ROWS + 1, ops.MAX_QUADRI_COLUMNS + 1
    assert iou(p, -1, p, 3, 0, 0, p, None) == -1 and iou(p, 3, p, -1, 0, 0, p, None) == -1
    assert iou(p, 3, p, 3, 2, 0, p, None) == -1 and iou(p, 3, p, 3, -1, 0, p, None) == -1           # mode outside {0, 1}
    assert iou(p, 3, p, 4, 0, 1, p, None) == -1                                                   # aligned with n != m
    assert iou(p, rows, p, 3, 0, 0, p, None) == -1 and iou(p, 2 ** 31 - 1, p, 2 ** 31 - 1, 0, 1, p, None) == -1
    assert iou(p, 3, p, cols, 0, 0, p, None) == -1
    assert iou(None, 3, p, 3, 0, 0, p, None) == -1 and iou(p, 3, None, 3, 1, 0, p, None) == -1 and iou(p, 3, p, 3, 0, 1, None, None) == -1
    assert iou(None, 0, None, 3, 0, 0, None, None) == 0 and iou(None, 3, None, 0, 1, 0, None, None) == 0
    assert iou(None, 0, None, 0, 0, 1, None, None) == 0
    assert pip(p, -1, p, 3, p, None) == -1 and pip(p, 3, p, -1, p, None) == -1 and pip(p, rows, p, 3, p, None) == -1
    assert pip(p, 3, p, cols, p, None) == -1
    assert pip(None, 3, p, 3, p, None) == -1 and pip(p, 3, None, 3, p, None) == -1 and pip(p, 3, p, 3, None, None) == -1
    assert pip(None, 0, None, 3, None, None) == 0 and pip(None, 3, None, 0, None, None) == 0
    ws = lib.frcnn_ops_nms_workspace_bytes(100)
    assert nms(p, p, None, -1, 0.5, p, p, ws, None) == -1 and nms(p, p, None, ops.MAX_NMS_BOXES + 1, 0.5, p, p, 1 << 40, None) == -1
    assert nms(p, p, None, 100, 0.5, p, p, ws - 1, None) == -1                                    # a workspace that is too small
    for null in (0, 1, 5, 6):
        args = [p, p, None, 100, 0.5, p, p, ws, None]
        args[null] = None
        assert nms(*args) == -1, null
    assert nms(None, None, None, 0, 0.5, None, None, 0, None) == 0
