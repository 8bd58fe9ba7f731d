"""fasterrcnn_amd.ops.convex_iou / convex_giou / min_area_polygons without a GPU: the conditions of the cases (tests/convex_cases.py), the
kernels' closed form in float64 against the float64 truth (hull, Sutherland-Hodgman, shoelace, autograd), the torch compositions against
that truth, the argument rules of the public functions, shapes and dtypes on meta and fake tensors, and the validation of the C entry
points.

Measured here: analytic(float64) agrees with the truth to 1.9e-15 (iou), 8.9e-16 (giou), 3.5e-15 of a gradient component on the pairs not
near a seam and 2.8e-14 px (the rectangle's corners); near x = 4096 to 7.5e-14, 3.2e-14, 9.6e-15 and 9.1e-13 (the truth forms its areas
relative to a vertex, its clip on raw coordinates).  Pairs near a seam: 0, 0, 1, 2, 1, 9 and 0 of the cases "1", "63", "64", "65", "130",
"1000" and "near4096".  The float32 compositions on all seven cases: values within 4.5e-7, gradients within 5.9e-5 of the truth."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import convex_cases as C

F32, F64 = torch.float32, torch.float64
NAMES = ("convex_iou", "convex_giou", "min_area_polygons", "convex_iou_pytorch", "convex_giou_pytorch", "min_area_polygons_pytorch")


def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def keep(name):
    return (~C.seam(name))[:, None]


# ---- 1. the cases and the closed form -----------------------------------------------------------------------------------------------------
def test_conditions_of_the_cases():
    C.check_conditions()
    sets, polys, names = C.special()
    t = C.truth("special")
    assert len(names) == sets.shape[0] == polys.shape[0] == 15
    row = names.index
    for name in ("triangle-on-edge", "triangle-repeated"):                   # Q's hull has three vertices
        assert len(C.hull_indices(polys[row(name)].double().view(4, 2).tolist())) == 3 and 0.4 < float(t["iou"][row(name)]) < 0.6
    assert float(t["giou"][row("triangle-on-edge")]) == float(t["giou"][row("triangle-repeated")])
    assert float(t["iou"][row("same")]) == 1.0 and float(t["giou"][row("same")]) == 1.0
    assert not bool(t["iou"][list(C.DEAD_ROWS)].any()) and not bool(t["grad"][list(C.DEAD_ROWS)].any())
    assert t["vertex"][row("grid")].tolist() == [True, False, True, False, False, False, True, False, True]
    assert float(t["iou"][row("clockwise")]) == float(t["iou"][row("crossing")]) > 0.4
    assert float(t["iou"][row("set-inside")]) == 0.0625 and 0 < float(t["iou"][row("polygon-inside")]) < 1
    assert float(t["iou"][row("disjoint")]) == 0 and float(t["giou"][row("disjoint")]) < 0
    for name in ("equal", "collinear"):                                       # degenerate, not dead: I = 0, the gradient goes through C
        assert float(t["iou"][row(name)]) == 0
    assert float(t["giou"][row("collinear")]) < 0 and bool(t["grad"][row("collinear")].any())


@pytest.mark.parametrize("name", C.RANDOM_CASES + ("special",))
def test_closed_form_in_float64_is_the_truth(name):
    sets, polys = C.case(name)
    t, a = C.truth(name), C.analytic(sets, polys, F64)
    scale = 100.0 if name == "near4096" else 1.0                           # the truth clips on raw coordinates: 4096 / 40 times the rounding
    k = keep(name) if name != "special" else torch.ones(sets.shape[0], 1, dtype=torch.bool)
    worst = {key: float((a[key] - t[key]).abs().max()) for key in ("iou", "giou", "rect")}
    worst["grad"] = float(((a["grad"] - t["grad"]) * k).abs().max())
    print(name, worst)
    assert worst["iou"] <= 1e-12 * scale and worst["giou"] <= 1e-12 * scale and worst["grad"] <= 1e-12 * scale and worst["rect"] <= 1e-11
    assert not bool((a["grad"][~t["vertex"].repeat_interleave(2, 1)]).any())       # a point that is no vertex of P: exactly zero


@pytest.mark.parametrize("name", C.MATRIX_CASES)
def test_matrix_closed_form_in_float64_is_the_truth(name):
    sets, polys = C.matrix_case(name)
    t = C.matrix_truth(name)
    assert float((C.analytic_matrix(sets, polys, F64) - t).abs().max()) <= 1e-12
    assert float(t.max()) > 0.3 and float((t == 0).double().mean()) > 0.1 or name == "1x1"


def test_seam_rule_sees_hull_changes_and_coincident_edges():
    square = [(0.0, 0.0), (8.0, 0.0), (8.0, 6.0), (0.0, 6.0)]
    sets, polys, names = C.special()
    pairs = dict(zip(names, zip(sets.double().view(-1, 9, 2).tolist(), polys.double().view(-1, 4, 2).tolist())))
    assert C.near_seam_pair(*pairs["grid"]) and C.near_seam_pair(*pairs["same"]) and C.near_seam_pair(*pairs["duplicates"])
    assert not C.near_seam_pair(*pairs["clockwise"]) and not C.near_seam_pair(*pairs["polygon-inside"])
    shifted = [(x + 1e-5, y) for x, y in pairs["clockwise"][0]]
    assert not C.near_seam_pair(shifted, square)


# ---- 2. the compositions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.RANDOM_CASES)
def test_compositions_against_the_truth(name):
    """float32: an area is a sum of at most 26 cross products of origin-relative coordinates of the pair's extent s, each with two
    roundings of 2^-24 s^2, and the recipe keeps s^2 / area below 20: 52 * 6e-8 * 20 = 6e-5 if every rounding had one sign, 9e-6 with
    sqrt(52) for independent ones.  The bound for a value is 2e-5, the same near x = 4096 (the composition subtracts the common origin
    first; without it the bound would be missed by a factor of 100), and ten times that for the gradient, whose terms are divided by
    U^2 and C^2."""
    sets, polys = C.case(name)
    t, k = C.truth(name), keep(name)
    for dtype, tol in ((F64, 1e-9), (F32, 2e-5)):
        s = sets.to(dtype).requires_grad_(True)
        giou, grad = ops.convex_giou_pytorch(s, polys.to(dtype))
        assert giou.dtype == grad.dtype == dtype and giou.requires_grad and not grad.requires_grad
        assert C.rel_err(giou.detach(), t["giou"]) <= tol and C.rel_err(grad * k, t["grad"] * k) <= 10 * tol
        g = C.upstream(name).to(dtype)
        (giou * g).sum().backward()
        assert torch.equal(s.grad, g[:, None] * grad)
        iou = ops.convex_iou_pytorch(sets.to(dtype), polys.to(dtype))
        assert iou.shape == (sets.shape[0],) * 2 and C.rel_err(iou.diagonal(), t["iou"]) <= tol
        assert C.rel_err(ops.min_area_polygons_pytorch(sets.to(dtype)), t["rect"]) <= tol


def test_composition_matrix_against_the_truth():
    for name in ("65x63", "7x130"):
        sets, polys = C.matrix_case(name)
        assert C.rel_err(ops.convex_iou_pytorch(sets.double(), polys.double()), C.matrix_truth(name)) <= 1e-9
        assert C.rel_err(ops.convex_iou_pytorch(sets, polys), C.matrix_truth(name)) <= 2e-5


def test_compositions_on_the_special_rows_in_general_position():
    sets, polys, names = C.special()
    rows = [names.index(r) for r in C.GENERAL_POSITION_ROWS]
    t = C.truth("special")
    s, q = sets[rows].double(), polys[rows].double()
    giou, grad = ops.convex_giou_pytorch(s, q)
    assert float((giou - t["giou"][rows]).abs().max()) <= 1e-12 and float((grad - t["grad"][rows]).abs().max()) <= 1e-12
    assert float((ops.convex_iou_pytorch(s, q).diagonal() - t["iou"][rows]).abs().max()) <= 1e-12
    assert float((ops.min_area_polygons_pytorch(s) - t["rect"][rows]).abs().max()) <= 1e-11
    dead = list(C.DEAD_ROWS)                                                   # dead rows need no general position
    giou, grad = ops.convex_giou_pytorch(sets[dead], polys[dead])
    assert not bool(giou.any()) and not bool(grad.any()) and not bool(ops.convex_iou_pytorch(sets[dead], polys[dead]).diagonal().any())
    assert not bool(ops.min_area_polygons_pytorch(sets[[names.index("nan")]]).any())


def test_compositions_empty_and_argument_rules():
    s, q = C.case("63")
    assert ops.convex_iou_pytorch(s[:0], q).shape == (0, 63) and ops.convex_iou_pytorch(s, q[:0]).shape == (63, 0)
    giou, grad = ops.convex_giou_pytorch(s[:0], q[:0])
    assert giou.shape == (0,) and grad.shape == (0, 18) and ops.min_area_polygons_pytorch(s[:0]).shape == (0, 8)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.convex_iou_pytorch(s, [1.0])
    with pytest.raises(TypeError, match="float16"):
        ops.convex_giou_pytorch(s.half(), q.half())
    with pytest.raises(ValueError, match=r"\(63, 17\)"):
        ops.min_area_polygons_pytorch(s[:, :17])
    with pytest.raises(ValueError, match="63 and 60"):
        ops.convex_giou_pytorch(s, q[:60])


# ---- 3. the public functions: names, errors, meta -------------------------------------------------------------------------------------------
def test_names_are_exported_and_documented():
    for name in NAMES:
        assert name in ops.__all__ and callable(getattr(ops, name)) and name in ops.__doc__ and getattr(ops, name).__doc__
    for name in NAMES[3:]:
        assert "GENERAL POSITION" in getattr(ops, name).__doc__, name
    assert ops.CONVEX_IOU_TILE_ROWS == nv.lib().frcnn_ops_convex_iou_tile_rows()
    assert ops.CONVEX_RECT_TIE == C.RECT_TIE and ops.CONVEX_MIN_AREA == C.MIN_AREA


def test_argument_errors():
    sets, polys = meta(5, 18), meta(5, 8)
    calls = {"convex_iou": lambda s, q: ops.convex_iou(s, q), "convex_giou": lambda s, q: ops.convex_giou(s, q),
             "min_area_polygons": lambda s, q: ops.min_area_polygons(s)}
    for name, fn in calls.items():
        with pytest.raises(TypeError, match="pointsets must be a torch.Tensor"):
            fn([[0.0] * 18], polys)
        with pytest.raises(TypeError, match="float64"):
            fn(sets.double(), polys)
        for dtype in (torch.float16, torch.bfloat16):
            with pytest.raises(TypeError, match=r"\.float\(\)"):
                fn(meta(5, 18, dtype=dtype), polys)
        with pytest.raises(ValueError, match=r"pointsets must be \[N, 18\].*\(5, 16\)"):
            fn(meta(5, 16), polys)
        with pytest.raises(ValueError, match=r"\(18,\)"):
            fn(meta(18), polys)
        with pytest.raises(ValueError, match="no CPU implementation.*%s_pytorch runs on any device" % name):
            fn(torch.zeros(5, 18), torch.zeros(5, 8))
    for name in ("convex_iou", "convex_giou"):
        fn = calls[name]
        with pytest.raises(TypeError, match="polygons must be a torch.Tensor"):
            fn(sets, None)
        with pytest.raises(TypeError, match="polygons must be float32"):
            fn(sets, polys.double())
        with pytest.raises(ValueError, match=r"polygons must be \[N, 8\].*\(5, 10\)"):
            fn(sets, meta(5, 10))
        with pytest.raises(ValueError, match="cpu"):
            fn(sets, torch.zeros(5, 8))                                       # one on meta, one on the CPU
        with FakeTensorMode():
            with pytest.raises(ValueError, match="same device"):
                fn(torch.empty((5, 18), device="cuda:0"), torch.empty((5, 8), device="cuda:1"))
    with pytest.raises(ValueError, match="5 and 4 rows"):
        ops.convex_giou(sets, meta(4, 8))
    with pytest.raises(ValueError, match=str(ops.MAX_CONVEX_POLYGONS + 1)):
        ops.convex_iou(sets, meta(ops.MAX_CONVEX_POLYGONS + 1, 8))
    for name, fn in calls.items():
        with pytest.raises(ValueError, match="MAX_CONVEX_ROWS = %d rows, got %d" % (ops.MAX_CONVEX_ROWS, ops.MAX_CONVEX_ROWS + 1)):
            fn(meta(ops.MAX_CONVEX_ROWS + 1, 18), polys)


def test_meta_and_fake_shapes_dtypes_and_autograd():
    for n, k in ((5, 3), (0, 3), (5, 0), (70, 130)):
        out = ops.convex_iou(meta(n, 18).requires_grad_(True), meta(k, 8))
        assert out.shape == (n, k) and out.dtype == F32 and not out.requires_grad
    for n in (0, 1, 70):
        s = meta(n, 18).requires_grad_(True)
        giou, grad = ops.convex_giou(s, meta(n, 8).requires_grad_(True))
        assert giou.shape == (n,) and grad.shape == (n, 18) and giou.dtype == grad.dtype == F32
        assert giou.requires_grad and not grad.requires_grad
        (1 - giou).sum().backward()
        assert s.grad.shape == (n, 18) and s.grad.dtype == F32
        rect = ops.min_area_polygons(s)
        assert rect.shape == (n, 8) and rect.dtype == F32 and not rect.requires_grad
    assert not ops.convex_giou(meta(4, 18), meta(4, 8))[0].requires_grad
    with FakeTensorMode():
        s = torch.empty((6, 18), device="cuda").requires_grad_(True)
        giou, grad = ops.convex_giou(s, torch.empty((6, 8), device="cuda"))
        assert giou.shape == (6,) and grad.shape == (6, 18) and giou.device.type == "cuda" and giou.requires_grad
        assert ops.convex_iou(s, torch.empty((9, 8), device="cuda")).shape == (6, 9)
        assert ops.min_area_polygons(s).shape == (6, 8)


# ---- 4. FRCNN_EINVAL of the entry points, with null pointers and no device --------------------------------------------------------------------
def test_entry_points_validate_before_touching_the_gpu():
    lib, p = nv.lib(), 0x1000                                              # never dereferenced: every call below fails validation first
    iou, giou, rect = lib.frcnn_ops_convex_iou, lib.frcnn_ops_convex_giou, lib.frcnn_ops_min_area_polygons
    assert iou(p, -1, p, 3, p, None) == -1 and iou(p, 3, p, -1, p, None) == -1 and iou(p, 3, p, ops.MAX_CONVEX_POLYGONS + 1, p, None) == -1
    assert iou(None, 3, p, 3, p, None) == -1 and iou(p, 3, None, 3, p, None) == -1 and iou(p, 3, p, 3, None, None) == -1
    assert iou(None, 0, None, 3, None, None) == 0 and iou(None, 3, None, 0, None, None) == 0
    rows = ops.MAX_CONVEX_ROWS + 1                                          # the grids' ceilings are formed in int
    assert iou(p, rows, p, 3, p, None) == -1 and giou(p, p, rows, p, p, None) == -1 and rect(p, rows, p, None) == -1
    assert iou(p, 2 ** 31 - 1, p, 3, p, None) == -1 and rect(p, 2 ** 31 - 1, p, None) == -1
    assert giou(p, p, -1, p, p, None) == -1
    for null in (0, 1, 3, 4):
        args = [p, p, 3, p, p, None]
        args[null] = None
        assert giou(*args) == -1, null
    assert giou(None, None, 0, None, None, None) == 0
    assert rect(p, -1, p, None) == -1 and rect(None, 3, p, None) == -1 and rect(p, 3, None, None) == -1 and rect(None, 0, None, None) == 0
