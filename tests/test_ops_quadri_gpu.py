"""fasterrcnn_amd.ops.box_iou_quadri / nms_quadri / points_in_polygons on the GPU against the float64 truth of tests/quadri_cases.py (hull,
Sutherland-Hodgman, shoelace; the greedy pass; the sign of every edge's cross product), and the properties the kernels promise: the
aligned form is the matrix's diagonal, mode "iou" has convex_iou's bits, a quadrilateral against itself gives 1, any vertex order gives
the same bits, dead rows give exact zeros, tiles do not show, two runs agree, strides do not matter, empty inputs give empty outputs.

The bound of every IoU comparison is measured in the same test, as in tests/test_ops_convex_gpu.py: err(a) = max|a - truth| / max|truth|
over the case, err_ref is the error of the kernels' arithmetic evaluated in float32 on the CPU (quadri_cases.analytic), and
err_gpu <= 4 * max(err_ref, 2**-24) must hold.  The NMS and points_in_polygons results are exact: the cases keep every IoU MARGIN away
from its threshold and every point DELTA away from every edge's line.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: 1.000, iou and iof, aligned and matrix cases -- on
every case err_gpu equals err_ref to the printed digits, so the kernels and the float32 restatement run the same arithmetic.  The largest
errors themselves: 5.2e-7 (iou, case "1000") and 6.6e-7 (iof, case "63x65")."""
import functools
import itertools

import pytest
import torch

from fasterrcnn_amd import ops

from tests import quadri_cases as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
BOUND = 4.0
FLOOR = 2.0 ** -24
NAN, INF = float("nan"), float("inf")


def check_bound(label, got, truth, single):
    """err_gpu <= 4 * max(err_ref, 2**-24); prints both errors; returns the ratio."""
    assert got.shape == truth.shape and got.dtype == F32 and single.dtype == F32, label
    assert float(truth.abs().max()) > 0, label
    err_gpu, err_ref = Q.rel_err(got.cpu(), truth), Q.rel_err(single, truth)
    ratio = err_gpu / max(err_ref, FLOOR)
    print("%s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, err_gpu, err_ref, ratio))
    assert err_gpu <= BOUND * max(err_ref, FLOOR), (label, err_gpu, err_ref)
    return ratio


@functools.lru_cache(maxsize=None)
def on_gpu(name):
    return tuple(t.to(DEV) for t in Q.case(name))


def quads(*rows):
    return torch.tensor(rows, dtype=F32, device=DEV)


def permuted(rows, perm):
    """rows [n, 8] with the four vertices of every row in the order perm."""
    return rows.view(-1, 4, 2)[:, list(perm)].reshape(-1, 8)


# ---- 1. IoU values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("name", Q.ALIGNED_CASES)
def test_aligned_values_against_the_truth(name, mode):
    a, b = on_gpu(name)
    got = ops.box_iou_quadri(a, b, mode, aligned=True)
    assert got.shape == (a.shape[0],) and bool(torch.isfinite(got).all()) and float(got.min()) >= 0
    want = Q.truth(name)[mode]
    check_bound("%s %s" % (name, mode), got, want, Q.analytic(*Q.case(name), mode, F32))
    assert torch.equal(got.cpu() == 0, want == 0)


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("name", Q.MATRIX_CASES)
def test_matrix_values_against_the_truth(name, mode):
    rows, cols = Q.matrix_case(name)
    got = ops.box_iou_quadri(rows.to(DEV), cols.to(DEV), mode)
    want = Q.matrix_truth(name)[mode]
    check_bound("%s %s" % (name, mode), got, want, Q.analytic_matrix(rows, cols, mode, F32))
    assert torch.equal(got.cpu() == 0, want == 0)                             # the pairs that do not meet are exactly 0


# ---- 2. IoU properties, all exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("65", "130", "near4096"))
def test_aligned_is_the_diagonal_and_iou_has_the_bits_of_convex_iou(name):
    a, b = on_gpu(name)
    for mode in Q.MODES:
        assert torch.equal(ops.box_iou_quadri(a, b, mode, aligned=True), ops.box_iou_quadri(a, b, mode).diagonal())
    padded = torch.cat([a, a[:, :2].repeat(1, 5)], 1)                        # the four vertices, then five copies of the first
    assert torch.equal(ops.box_iou_quadri(a, b), ops.convex_iou(padded, b))


def test_itself_inside_and_a_shared_edge():
    for name in ("130", "near4096"):
        a, b = on_gpu(name)
        for rows in (a, b):
            for mode in Q.MODES:
                assert bool((ops.box_iou_quadri(rows, rows, mode, aligned=True) == 1).all())
                assert bool((ops.box_iou_quadri(rows, rows, mode).diagonal() == 1).all())
    outer = quads([0, 0, 8, 0, 8, 6, 0, 6], [10, 10, 30, 12, 28, 30, 8, 26])
    inner = quads([2, 1, 5, 2, 6, 4, 1, 5], [14, 14, 24, 16, 22, 24, 12, 22])   # small integers: every product is exact
    assert torch.equal(ops.box_iou_quadri(inner, outer, "iof", aligned=True), torch.ones(2, device=DEV))
    assert bool((ops.box_iou_quadri(outer, inner, "iof", aligned=True) < 1).all())
    left, right, above = [0, 0, 4, 0, 4, 4, 0, 4], [4, 0, 8, 0, 8, 4, 4, 4], [0, 4, 4, 4, 4, 8, 0, 8]
    touch = ops.box_iou_quadri(quads(left), quads(right, above, [4, 4, 8, 4, 8, 8, 4, 8]))
    assert not bool(touch.any()) and not bool(ops.box_iou_quadri(quads(right, above), quads(left), "iof").any())


@pytest.mark.parametrize("name", ("65", "near4096"))
def test_no_vertex_order_changes_a_bit(name):
    a, b = on_gpu(name)
    want = {mode: ops.box_iou_quadri(a, b, mode) for mode in Q.MODES}
    for perm in itertools.permutations(range(4)):                            # both windings and the self-crossing orders among them
        for mode in Q.MODES:
            assert torch.equal(ops.box_iou_quadri(permuted(a, perm), b, mode), want[mode]), perm
            assert torch.equal(ops.box_iou_quadri(a, permuted(b, perm), mode), want[mode]), perm
    g = torch.Generator().manual_seed(3)
    perms = torch.stack([torch.randperm(4, generator=g) for _ in range(a.shape[0])]).to(DEV)      # one order per row
    mixed = a.view(-1, 4, 2).gather(1, perms[..., None].expand(-1, -1, 2)).reshape(-1, 8)
    assert torch.equal(ops.box_iou_quadri(mixed, b, "iou", aligned=True), want["iou"].diagonal())


def test_an_arrow_is_its_hull():
    arrow, triangle = [0, 0, 6, 0, 2, 1, 0, 6], [0, 0, 6, 0, 0, 6, 0, 6]     # (2, 1) lies inside the triangle of the other three
    others = torch.cat([quads([0, 0, 4, 0, 4, 4, 0, 4], [1, 1, 9, 2, 8, 7, 2, 9]), on_gpu("65")[0] * 0.1])
    for perm in itertools.permutations(range(4)):
        rows = permuted(quads(arrow), perm)
        for mode in Q.MODES:
            assert torch.equal(ops.box_iou_quadri(rows, others, mode), ops.box_iou_quadri(quads(triangle), others, mode))
            assert torch.equal(ops.box_iou_quadri(others, rows, mode), ops.box_iou_quadri(others, quads(triangle), mode))
    assert float(ops.box_iou_quadri(quads(arrow), quads(triangle))) == 1
    square = [0, 0, 4, 0, 4, 4, 0, 4]                                        # the triangle cuts a corner of area 2 off it: 14 / (18 + 16 - 14)
    assert abs(float(ops.box_iou_quadri(quads(arrow), quads(square))) - 0.7) <= 1e-6
    assert abs(float(ops.box_iou_quadri(quads(square), quads(arrow), "iof")) - 14 / 16) <= 1e-6


def test_dead_rows_give_zero_rows_and_columns():
    a, b = on_gpu("65")
    dead = quads([NAN, 0, 8, 0, 8, 6, 0, 6], [0, 0, 8, 0, INF, 6, 0, 6], [0, 0, 8, -INF, 8, 6, 0, 6], [5, 5] * 4, [0, 0, 1, 1, 2, 2, 3, 3],
                 [0, 0, 4, 2, 2, 1, 6, 3])
    rows, cols = a.clone(), b.clone()
    at = [3, 17, 31, 32, 63, 64]
    rows[at], cols[at] = dead, dead
    for mode in Q.MODES:
        got, clean = ops.box_iou_quadri(rows, cols, mode), ops.box_iou_quadri(a, b, mode)
        assert bool(torch.isfinite(got).all())
        assert not bool(got[at].any()) and not bool(got[:, at].any())
        live = torch.ones(65, dtype=torch.bool, device=DEV)
        live[at] = False
        assert torch.equal(got[live][:, live], clean[live][:, live])          # whatever else the matrix holds
        assert not bool(ops.box_iou_quadri(rows, b, mode, aligned=True)[at].any())
        assert not bool(ops.box_iou_quadri(a, cols, mode, aligned=True)[at].any())
        assert not bool(ops.box_iou_quadri(dead, dead, mode).any())


def test_tiles_do_not_show_two_runs_agree_and_strides_do_not_matter():
    a, b = on_gpu("130")
    rows = ops.QUADRI_IOU_TILE_ROWS
    for mode in Q.MODES:
        whole = ops.box_iou_quadri(a, b, mode)
        assert torch.equal(whole, ops.box_iou_quadri(a, b, mode))
        for j in (0, 63, 64, 65, 127, 128, 129):
            assert torch.equal(whole[:, j], ops.box_iou_quadri(a, b[j:j + 1], mode)[:, 0]), j
        for i in (0, rows - 1, rows, rows + 1, 63, 64, 65, 4 * rows, 129):
            assert torch.equal(whole[i], ops.box_iou_quadri(a[i:i + 1], b, mode)[0]), i
        assert torch.equal(whole[40:100, 60:70], ops.box_iou_quadri(a[40:100], b[60:70], mode))
    big = on_gpu("1000")
    assert torch.equal(ops.box_iou_quadri(*big, aligned=True), ops.box_iou_quadri(*big, aligned=True))
    wide_a, wide_b = torch.zeros(260, 20, device=DEV), torch.zeros(130, 16, device=DEV)
    wide_a[::2, 1:17:2], wide_b[:, ::2] = a, b
    sa, sb = wide_a[::2, 1:17:2], wide_b[:, ::2]
    assert not sa.is_contiguous() and not sb.is_contiguous()
    assert torch.equal(ops.box_iou_quadri(sa, sb), ops.box_iou_quadri(a, b))
    assert torch.equal(ops.box_iou_quadri(sa, sb, "iof", aligned=True), ops.box_iou_quadri(a, b, "iof", aligned=True))
    assert not ops.box_iou_quadri(a.clone().requires_grad_(True), b).requires_grad


# ---- 3. NMS ----------------------------------------------------------------------------------------------------------------------------------
def run_nms(c, labels):
    return ops.nms_quadri(c["quads"].to(DEV), c["scores"].to(DEV), c["thr"], None if labels is None else labels.to(DEV))


@pytest.mark.parametrize("name", Q.NMS_CASES)
def test_nms_keeps_exactly_the_truth(name):
    c = Q.nms_case(name)
    dets, keep = run_nms(c, c["labels"])
    want = Q.nms_ref(name)
    assert keep.dtype == torch.int64 and torch.equal(keep.cpu(), want)
    expect = torch.cat([c["quads"][want], c["scores"][want, None]], 1)
    assert dets.shape == (want.numel(), 9) and torch.equal(dets.cpu().nan_to_num(nan=-1.0), expect.nan_to_num(nan=-1.0))
    again = run_nms(c, c["labels"])
    assert torch.equal(again[1], keep) and torch.equal(again[0].nan_to_num(nan=-1.0), dets.nan_to_num(nan=-1.0))
    assert 0 < want.numel() and (c["quads"].shape[0] < 64 or want.numel() < c["quads"].shape[0])


@pytest.mark.parametrize("geometry", Q.NMS_GEOMETRIES)
def test_nms_with_one_label_is_nms_without_labels(geometry):
    c = Q.nms_case("n%d-t%s-none" % geometry)
    n = c["quads"].shape[0]
    plain = run_nms(c, None)
    for labels in (torch.full((n,), 5, dtype=torch.int64), torch.zeros(n, dtype=torch.int32)):
        same = run_nms(c, labels)
        assert torch.equal(same[1], plain[1]) and torch.equal(same[0].nan_to_num(nan=-1.0), plain[0].nan_to_num(nan=-1.0))


def test_nms_ties_nan_scores_strides_and_empty_input():
    c = Q.nms_case("n200-t0.5-none")
    q = c["quads"].to(DEV)
    flat = torch.full((200,), 0.25, device=DEV)                               # equal scores: ties go by ascending index
    keep = ops.nms_quadri(q, flat, c["thr"])[1]
    want = Q.nms_keep(dict(c, scores=flat.cpu()), None)
    assert torch.equal(keep.cpu(), want) and bool((keep[1:] > keep[:-1]).all())
    nan = torch.full((200,), NAN, device=DEV)                                 # NaN scores rank among themselves by index
    assert torch.equal(ops.nms_quadri(q, nan, c["thr"])[1], keep)
    wide = torch.zeros(200, 16, device=DEV)
    wide[:, ::2] = q
    assert torch.equal(ops.nms_quadri(wide[:, ::2], flat, c["thr"])[1], keep)
    dets, none = ops.nms_quadri(q[:0], flat[:0], 0.5)
    assert dets.shape == (0, 9) and none.shape == (0,) and none.dtype == torch.int64
    dead = q.clone()
    dead[::3] = NAN                                                           # a dead quadrilateral suppresses nothing and is never suppressed
    kept = ops.nms_quadri(dead, flat, c["thr"])[1]
    assert set(range(0, 200, 3)) <= set(kept.tolist())


def test_opcheck():
    a, b = on_gpu("65")
    scores = torch.rand(65, device=DEV)
    labels = torch.arange(65, device=DEV) % 3
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.frcnn.box_iou_quadri, (a, b, 0, False), test_utils=tests)
    torch.library.opcheck(torch.ops.frcnn.box_iou_quadri, (a, b, 1, True), test_utils=tests)
    torch.library.opcheck(torch.ops.frcnn.nms_quadri, (a, scores, None, 0.5), test_utils=tests)
    torch.library.opcheck(torch.ops.frcnn.nms_quadri, (a, scores, labels, 0.1), test_utils=tests)
    torch.library.opcheck(torch.ops.frcnn.points_in_polygons, (a[:, :2].contiguous(), b), test_utils=tests)


# ---- 4. points_in_polygons ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q.POINT_CASES)
def test_points_are_placed_exactly_as_the_truth_places_them(name):
    points, polys, _ = Q.point_case(name)
    got = ops.points_in_polygons(points.to(DEV), polys.to(DEV))
    assert got.dtype == F32 and torch.equal(got.cpu().double(), Q.truth_inside(points, polys))
    assert torch.equal(got, ops.points_in_polygons(points.to(DEV), polys.to(DEV)))


def test_points_on_the_boundary_are_inside_and_one_unit_outside_is_not():
    poly = [2, 1, 8, 3, 9, 9, 1, 7]                                          # small integers: every product is exact
    on = [[2, 1], [8, 3], [9, 9], [1, 7], [5, 2], [5, 8], [4, 4], [3, 6]]    # the vertices, two edge points ((2,1)+(3,1), (1,7)+(4,1)), interior
    off = [[1, 1], [2, 0], [9, 3], [8, 2], [10, 9], [9, 10], [0, 7], [1, 8], [5, 1], [5, 9], [5, 10], [-3, 4], [12, 6]]
    pts = torch.tensor(on + off, dtype=F32, device=DEV)
    want = torch.tensor([1.0] * len(on) + [0.0] * len(off), device=DEV)
    for perm in itertools.permutations(range(4)):                            # every vertex order gives the same bits
        assert torch.equal(ops.points_in_polygons(pts, permuted(quads(poly), perm))[:, 0], want), perm
    for shift in (4096.0, -300.0):                                            # exact still: the differences are formed first
        assert torch.equal(ops.points_in_polygons(pts + shift, quads(poly) + shift)[:, 0], want)
    triangle = quads([0, 0, 6, 0, 2, 1, 0, 6], [0, 0, 6, 0, 0, 6, 0, 6])     # an arrow is its hull; a repeated vertex
    tri_pts = torch.tensor([[3, 3], [2, 1], [0, 0], [1, 1], [4, 3], [3, 4], [-1, 0], [0, 7]], dtype=F32, device=DEV)
    assert ops.points_in_polygons(tri_pts, triangle).tolist() == [[1, 1]] * 4 + [[0, 0]] * 4


def test_dead_polygons_dead_points_tiles_strides_and_empty_inputs():
    points, polys = (t.to(DEV) for t in Q.point_case("%dx5" % (Q.POINT_ROWS + 1))[:2])
    clean = ops.points_in_polygons(points, polys)
    cols = torch.cat([polys, quads([5, 5] * 4, [0, 0, 1, 1, 2, 2, 3, 3], [NAN, 0, 90, 0, 90, 90, 0, 90], [0, 0, 90, 0, INF, 90, 0, 90])])
    rows = points.clone()
    at = [0, 31, 32, Q.POINT_ROWS - 1, Q.POINT_ROWS]
    rows[at] = torch.tensor([[NAN, 50], [50, NAN], [INF, 50], [50, -INF], [NAN, NAN]], device=DEV)
    got = ops.points_in_polygons(rows, cols)
    assert not bool(got[:, 5:].any()) and not bool(got[at].any())            # a zero column, a zero row
    live = torch.ones(rows.shape[0], dtype=torch.bool, device=DEV)
    live[at] = False
    assert torch.equal(got[live][:, :5], clean[live])
    many = on_gpu("130")[1]                                                   # 130 polygons: three tile columns
    whole = ops.points_in_polygons(points, many)
    for j in (0, 63, 64, 65, 128, 129):
        assert torch.equal(whole[:, j], ops.points_in_polygons(points, many[j:j + 1])[:, 0]), j
    for i in (0, Q.POINT_ROWS - 1, Q.POINT_ROWS):
        assert torch.equal(whole[i], ops.points_in_polygons(points[i:i + 1], many)[0]), i
    wide_p, wide_q = torch.zeros(points.shape[0], 4, device=DEV), torch.zeros(5, 16, device=DEV)
    wide_p[:, ::2], wide_q[:, ::2] = points, polys
    assert torch.equal(ops.points_in_polygons(wide_p[:, ::2], wide_q[:, ::2]), clean)
    assert ops.points_in_polygons(points[:0], polys).shape == (0, 5) and ops.points_in_polygons(points, polys[:0]).shape == (Q.POINT_ROWS + 1, 0)
    assert ops.box_iou_quadri(polys[:0], polys).shape == (0, 5) and ops.box_iou_quadri(polys, polys[:0], "iof").shape == (5, 0)
    assert ops.box_iou_quadri(polys[:0], polys[:0], aligned=True).shape == (0,)
    assert not ops.points_in_polygons(points.clone().requires_grad_(True), polys).requires_grad
