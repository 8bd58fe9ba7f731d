"""fasterrcnn_amd.ops.convex_iou / convex_giou / min_area_polygons on the GPU against the float64 truth of tests/convex_cases.py (hull,
Sutherland-Hodgman, shoelace, autograd), and the properties the kernels promise: exact zeros for dead rows and for points that are no
hull vertices, IoU 1 for P = Q, tiles that do not show, bit-identical results under any permutation of a set's points or a polygon's
vertices, determinism, the autograd formula, strides, the rectangle's geometry, empty inputs.

The bound of every comparison with the truth is measured in the same test, as in tests/test_ops_diffiou_gpu.py:
err(a) = max|a - truth| / max|truth| over the case, err_ref is the error of the kernels' closed form evaluated in float32 on the CPU
(convex_cases.analytic), and err_gpu <= 4 * max(err_ref, 2**-24) must hold.  Pairs near a seam (convex_cases.near_seam_pair) are left out
of the gradient comparisons only.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: giou 1.000, iou 1.000 (aligned
and matrix cases), the rectangle's corners 1.000, the gradient 1.000 -- on every case err_gpu equals err_ref to the printed digits,
so the kernels and the float32 restatement run the same arithmetic.  The largest errors themselves: iou 4.4e-7 and the gradient 5.3e-7
(case "1000"), giou 3.1e-7, the corners 7.7e-8."""
import functools

import pytest
import torch

from fasterrcnn_amd import ops

from tests import convex_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
ALL_CASES = C.RANDOM_CASES + ("special",)


def check_bound(label, got, truth, single):
    """err_gpu <= 4 * max(err_ref, 2**-24); prints both errors; returns the ratio."""
    assert got.shape == truth.shape and got.dtype == F32 and single.dtype == F32, label
    assert float(truth.abs().max()) > 0, label
    err_gpu, err_ref = C.rel_err(got.cpu(), truth), C.rel_err(single, truth)
    ratio = err_gpu / max(err_ref, FLOOR)
    print("%s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, err_gpu, err_ref, ratio))
    assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, err_gpu, err_ref)
    return ratio


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case on the GPU, the float64 truth, the float32 closed form on the CPU and the mask of the pairs not near a seam."""
    sets, polys = C.case(name)
    keep = torch.ones(sets.shape[0], 1, dtype=torch.bool) if name == "special" else (~C.seam(name))[:, None]
    return sets.to(DEV), polys.to(DEV), C.truth(name), C.analytic(sets, polys, F32), keep


def permutations(n, width, seed):
    """One random permutation of range(width) per row, int64 [n, width] on the GPU."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(width, generator=g) for _ in range(n)]).to(DEV)


def permute(rows, perm):
    """rows [n, 2 w] of w points, the points of row i reordered by perm[i]."""
    n, w = perm.shape
    return rows.view(n, w, 2).gather(1, perm[..., None].expand(-1, -1, 2)).reshape(n, 2 * w)


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_values_against_the_truth(name):
    sets, polys, t, single, _ = reference(name)
    giou, grad = ops.convex_giou(sets, polys)
    assert bool(torch.isfinite(giou).all()) and bool(torch.isfinite(grad).all())
    check_bound("%s giou" % name, giou, t["giou"], single["giou"])
    iou = ops.convex_iou(sets, polys)
    assert iou.shape == (sets.shape[0],) * 2 and bool(torch.isfinite(iou).all()) and float(iou.min()) >= 0
    check_bound("%s iou" % name, iou.diagonal().contiguous(), t["iou"], single["iou"])
    check_bound("%s rect" % name, ops.min_area_polygons(sets), t["rect"], single["rect"])


@pytest.mark.parametrize("name", C.MATRIX_CASES)
def test_matrix_against_the_truth(name):
    sets, polys = C.matrix_case(name)
    got = ops.convex_iou(sets.to(DEV), polys.to(DEV))
    check_bound("%s iou" % name, got, C.matrix_truth(name), C.analytic_matrix(sets, polys, F32))
    assert torch.equal(got.cpu() == 0, C.matrix_truth(name) == 0)             # the pairs that do not meet are exactly 0


# ---- 2. the gradient -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.RANDOM_CASES)
def test_gradient_against_float64_autograd(name):
    sets, polys, t, single, keep = reference(name)
    grad = ops.convex_giou(sets, polys)[1]
    check_bound("%s grad" % name, grad * keep.to(DEV), t["grad"] * keep, single["grad"] * keep)
    assert not bool(grad.cpu()[~t["vertex"].repeat_interleave(2, 1)].any())    # no vertex of P: exactly zero


def test_autograd_is_grad_out_times_grad():
    sets, polys, _, _, _ = reference("130")
    g = C.upstream("130").to(DEV)
    s = sets.clone().requires_grad_(True)
    q = polys.clone().requires_grad_(True)
    giou, grad = ops.convex_giou(s, q)
    assert giou.requires_grad and not grad.requires_grad
    (giou * g).sum().backward()
    assert torch.equal(s.grad, g[:, None] * grad) and q.grad is None
    s.grad = None
    (1 - ops.convex_giou(s, polys)[0]).mean().backward()                     # the loss of the point-set heads, without a Function
    assert torch.equal(s.grad, (torch.full_like(g, -1.0 / 130))[:, None] * grad)
    assert not ops.convex_iou(s, polys).requires_grad and not ops.min_area_polygons(s).requires_grad
    torch.library.opcheck(torch.ops.frcnn.convex_giou, (sets[:5].clone().requires_grad_(True), polys[:5]),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


# ---- 3. the special rows -----------------------------------------------------------------------------------------------------------------------
def test_special_rows_zeros_ones_and_finiteness():
    sets, polys, t, single, _ = reference("special")
    names = C.SPECIAL_ROWS
    giou, grad = (v.cpu() for v in ops.convex_giou(sets, polys))
    iou, rect = ops.convex_iou(sets, polys).cpu(), ops.min_area_polygons(sets).cpu()
    assert all(bool(torch.isfinite(v).all()) for v in (giou, grad, iou, rect))
    dead = list(C.DEAD_ROWS)
    assert not bool(giou[dead].any()) and not bool(grad[dead].any()) and not bool(iou.diagonal()[dead].any())
    nan, inf, flat = names.index("nan"), names.index("inf"), names.index("dead-polygon")
    assert not bool(iou[nan].any()) and not bool(iou[:, inf].any()) and not bool(iou[:, flat].any()) and not bool(rect[nan].any())
    assert not bool(grad[~t["vertex"].repeat_interleave(2, 1)].any())        # the grid's mid-edge and centre points among them
    grid = names.index("grid")
    assert grad[grid].view(9, 2).abs().sum(1).ne(0).tolist() == [True, False, True, False, False, False, True, False, True]
    same = names.index("same")
    bound = MARGIN * max(C.rel_err(single["iou"], t["iou"]), FLOOR)
    assert abs(float(iou[same, same]) - 1) <= bound and abs(float(giou[same]) - 1) <= bound
    for name in ("equal", "collinear"):                                       # degenerate, not dead
        assert float(iou[names.index(name), 0]) == 0
    assert float(giou[names.index("collinear")]) < 0 and bool(grad[names.index("collinear")].any())
    assert float(giou[names.index("equal")]) == 0 and not bool(grad[names.index("equal")].any())      # U / C - 1 with C = U = A_Q
    assert torch.equal(giou[names.index("clockwise")], giou[names.index("crossing")])
    assert torch.equal(grad[names.index("clockwise")], grad[names.index("crossing")])
    on_edge, repeated = names.index("triangle-on-edge"), names.index("triangle-repeated")       # Q's hull has three vertices
    assert 0.4 < float(iou[on_edge, on_edge]) < 0.6 and torch.equal(iou[:, on_edge], iou[:, repeated])
    assert torch.equal(giou[on_edge], giou[repeated]) and torch.equal(grad[on_edge], grad[repeated]) and bool(grad[on_edge].any())


def test_range_of_the_coordinates():
    """Scaling by a power of two is exact, so inside the stated range (differences below 2^60) every result scales bit for bit; below
    the range, where squares underflow, the rectangle's unit vectors stay finite (the edge is scaled before its length is taken)."""
    sets, polys, _, _, _ = reference("special")
    rows = [C.SPECIAL_ROWS.index(r) for r in ("grid", "clockwise", "polygon-inside", "triangle-on-edge", "disjoint")]
    s, q = sets[rows], polys[rows]
    giou, grad = ops.convex_giou(s, q)
    for scale in (2.0 ** 55, 2.0 ** -10):                                   # areas of 2^-20 stay above the dead rule's 1e-14
        big = ops.convex_giou(s * scale, q * scale)
        assert torch.equal(big[0], giou) and torch.equal(big[1] * scale, grad) and bool(grad.any(1).all()), scale
        assert torch.equal(ops.convex_iou(s * scale, q * scale), ops.convex_iou(s, q))
        assert torch.equal(ops.min_area_polygons(s * scale), ops.min_area_polygons(s) * scale)
    tiny = ops.min_area_polygons(s * 2.0 ** -75)                             # distinct vertices whose squared distance underflows
    assert bool(torch.isfinite(tiny).all()) and float(tiny.abs().max()) <= 2 * float(s.abs().max()) * 2.0 ** -75
    dead = ops.convex_giou(s * 2.0 ** -75, q * 2.0 ** -75)                   # areas below 1e-14: dead by rule
    assert not bool(dead[0].any()) and not bool(dead[1].any())


# ---- 4. exact properties --------------------------------------------------------------------------------------------------------------------------
def test_tiles_do_not_show():
    sets, polys, _, _, _ = reference("130")
    whole = ops.convex_iou(sets, polys)
    rows = ops.CONVEX_IOU_TILE_ROWS
    for j in (0, 63, 64, 65, 127, 128, 129):
        assert torch.equal(whole[:, j], ops.convex_iou(sets, polys[j:j + 1])[:, 0]), j
    for i in (0, rows - 1, rows, rows + 1, 63, 64, 65, 4 * rows, 129):
        assert torch.equal(whole[i], ops.convex_iou(sets[i:i + 1], polys)[0]), i
    assert torch.equal(whole[40:100, 60:70], ops.convex_iou(sets[40:100], polys[60:70]))


@pytest.mark.parametrize("name", ("65", "1000", "near4096", "special"))
def test_permuting_points_or_vertices_changes_no_bit(name):
    sets, polys, _, _, _ = reference(name)
    n = sets.shape[0]
    giou, grad = ops.convex_giou(sets, polys)
    iou, rect = ops.convex_iou(sets[:70], polys[:70]), ops.min_area_polygons(sets)
    perm = permutations(n, 9, 1)
    shuffled = permute(sets, perm)
    if name == "special":                                                     # of equal points the smallest index is the vertex: compare
        mask = torch.tensor([r not in ("equal", "duplicates") for r in C.SPECIAL_ROWS], device=DEV)[:, None]     # the gradient elsewhere
    else:
        mask = torch.ones(n, 1, dtype=torch.bool, device=DEV)
    giou_p, grad_p = ops.convex_giou(shuffled, polys)
    assert torch.equal(giou_p, giou) and torch.equal(grad_p * mask, permute(grad, perm) * mask)
    assert torch.equal(ops.convex_iou(shuffled[:70], polys[:70]), iou) and torch.equal(ops.min_area_polygons(shuffled), rect)
    turned = permute(polys, permutations(n, 4, 2))
    giou_q, grad_q = ops.convex_giou(sets, turned)
    assert torch.equal(giou_q, giou) and torch.equal(grad_q, grad) and torch.equal(ops.convex_iou(sets[:70], turned[:70]), iou)


def test_two_runs_are_bit_identical_and_strides_do_not_matter():
    sets, polys, _, _, _ = reference("1000")
    first = (*ops.convex_giou(sets, polys), ops.convex_iou(sets, polys[:70]), ops.min_area_polygons(sets))
    again = (*ops.convex_giou(sets, polys), ops.convex_iou(sets, polys[:70]), ops.min_area_polygons(sets))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    wide_s, wide_q = torch.zeros(2000, 40, device=DEV), torch.zeros(1000, 16, device=DEV)
    wide_s[::2, 1:37:2] = sets
    wide_q[:, ::2] = polys
    s, q = wide_s[::2, 1:37:2], wide_q[:, ::2]
    assert not s.is_contiguous() and not q.is_contiguous()
    strided = (*ops.convex_giou(s, q), ops.convex_iou(s, q[:70]), ops.min_area_polygons(s))
    assert all(torch.equal(a, b) for a, b in zip(first, strided))


# ---- 5. the rectangle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("130", "near4096"))
def test_rectangle_geometry(name):
    sets, _, t, single, _ = reference(name)
    rect = ops.min_area_polygons(sets).cpu().double().view(-1, 4, 2)
    pts = sets.cpu().double().view(-1, 9, 2)
    # the value bound is relative to the largest coordinate of the case, the extent of its points from the origin: a corner is a float32
    # number of that size, so that is what a corner may be off by; a side rests on two corners
    slack = 2 * MARGIN * max(C.rel_err(single["rect"], t["rect"]), FLOOR) * float(t["rect"].abs().max())
    side = torch.roll(rect, -1, 1) - rect                                    # c0 -> c1 -> c2 -> c3 -> c0
    length = side.norm(dim=2)
    # counter-clockwise, right angles, opposite sides equal
    turn = side[:, :, 0] * torch.roll(side, -1, 1)[:, :, 1] - side[:, :, 1] * torch.roll(side, -1, 1)[:, :, 0]
    assert bool((turn > 0).all())
    assert bool(((side * torch.roll(side, -1, 1)).sum(2).abs() <= slack * (length + torch.roll(length, -1, 1))).all())
    assert float((length - torch.roll(length, 2, 1)).abs().max()) <= slack
    # every point of the set lies inside: on the left of each side, up to the value bound times the extent
    rel = pts[:, None, :, :] - rect[:, :, None, :]                           # [n, side, point, 2]
    left = (side[:, :, None, 0] * rel[..., 1] - side[:, :, None, 1] * rel[..., 0]) / length[:, :, None]
    assert float(left.min()) >= -slack, float(left.min())
    assert bool((left.amin(2).abs() <= slack).all())                      # and every side touches the set
    # the side c0 -> c1 lies on a hull edge: two of the set's points are on it, and they are hull neighbours in the truth
    on = left[:, 0].abs() <= slack
    assert bool((on.sum(1) >= 2).all())
    for i in range(pts.shape[0]):
        hull = C.hull_indices(pts[i].tolist())
        edges = {(hull[k], hull[(k + 1) % len(hull)]) for k in range(len(hull))}
        idx = on[i].nonzero()[:, 0].tolist()
        assert any((a, b) in edges for a in idx for b in idx), i
    # the corner order: c0 -> c1 runs along that edge, and the area is the truth's
    area = length[:, 0] * length[:, 1]
    want = t["rect"].view(-1, 4, 2)
    want_area = (want[:, 1] - want[:, 0]).norm(dim=1) * (want[:, 2] - want[:, 1]).norm(dim=1)
    assert bool(((area - want_area).abs() <= slack * (length[:, 0] + length[:, 1])).all())


# ---- 6. empty inputs ----------------------------------------------------------------------------------------------------------------------------
def test_empty_inputs():
    sets, polys, _, _, _ = reference("63")
    assert ops.convex_iou(sets[:0], polys).shape == (0, 63) and ops.convex_iou(sets, polys[:0]).shape == (63, 0)
    assert ops.convex_iou(sets[:0], polys[:0]).shape == (0, 0)
    s = sets[:0].clone().requires_grad_(True)
    giou, grad = ops.convex_giou(s, polys[:0])
    assert giou.shape == (0,) and grad.shape == (0, 18) and giou.dtype == grad.dtype == F32
    giou.sum().backward()
    assert s.grad.shape == (0, 18)
    assert ops.min_area_polygons(sets[:0]).shape == (0, 8)
