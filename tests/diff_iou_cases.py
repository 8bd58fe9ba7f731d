"""Cases and restatements of the differentiable rotated IoU (fasterrcnn_amd.ops.diff_iou_rotated_2d / _3d), shared by
tests/test_ops_diffiou_cpu.py and tests/test_ops_diffiou_gpu.py.  The definition is the one include/frcnn_hip.h states.

Two restatements, both one pair at a time with Python-level branches (no masked divisions):
  truth(name)     float64, torch scalars: box 1's corners in box 2's frame, Sutherland-Hodgman, the fan area, and the gradients of iou and
                  inter in the ten box parameters by autograd.
  analytic(...)   the kernel's closed form on numpy scalars of one dtype, in the kernel's order of operations: the clip carries per vertex
                  the tag of the boundary piece that leaves it, and the gradient is a sum over the final polygon's edges.  In float64 it is
                  checked against the truth; in float32 its error against the truth is err_ref, the measure of the GPU tests' bound.
They share the clip pass and nothing else: the truth differentiates the area, the closed form never forms a derivative of it.

The IoU has a kink where edges of the two boxes coincide, and float32 and float64 can then clip on different sides of it.  A pair is
near a seam -- and left out of gradient comparisons only -- when an edge of one box is within ANGLE_TOL = 2e-3 rad of parallel to an edge
of the other and the two lines come closer than DIST_TOL = 2e-3 times the longest side of the pair somewhere on the stretch the two
edges share.  check_conditions asserts that at most 2 % of the overlapping pairs of a random case are left out and none of "jitter".
"special" is made of seams: only values, finiteness and the zero rows are checked there."""
import functools
import math

import numpy as np
import torch

from tests import rotated_cases as R

F32, F64 = torch.float32, torch.float64
ANGLE_TOL = 2e-3
DIST_TOL = 2e-3
SEAM_CAP = 0.02
RANDOM_CASES = ("1", "63", "64", "65", "130", "near4096", "jitter")           # gradients are compared on these
SPECIAL_CASES = ("special", "special-shift")                                  # values, finiteness and zero rows only
BATCH = (2, 65)                                                               # "130" viewed as [2, 65, 5]


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(boxes1 [n, 5], boxes2 [n, 5]) float32, aligned pairs."""
    if name == "special":
        return R.iou_case("special")
    if name == "special-shift":                                               # every row against the next one
        b, _ = R.iou_case("special")
        return b, b.roll(-1, 0).clone()
    if name == "near4096":
        return R.iou_case("near4096")
    if name == "jitter":
        gen = torch.Generator().manual_seed(77)
        b = R.random_boxes(gen, 200).double()
        u = lambda lo, hi: torch.rand((200,), generator=gen, dtype=F64) * (hi - lo) + lo     # noqa: E731
        moved = torch.stack([b[:, 0] + u(-3, 3), b[:, 1] + u(-3, 3), b[:, 2] * torch.exp(u(math.log(0.8), math.log(1.25))),
                             b[:, 3] * torch.exp(u(math.log(0.8), math.log(1.25))), b[:, 4] + u(-0.3, 0.3)], 1)
        return b.to(F32), moved.to(F32)
    return R.iou_case("%sx%s" % (name, name))


@functools.lru_cache(maxsize=None)
def case_3d(name="jitter3d"):
    """(box3d1 [200, 7], box3d2 [200, 7]) float32 rows (x, y, z, w, h, l, alpha): "jitter" in the plane with random z and l; every
    fifth pair has no overlap along z, and pair 1 touches exactly."""
    b1, b2 = case("jitter")
    gen = torch.Generator().manual_seed(78)
    u = lambda lo, hi: torch.rand((200,), generator=gen, dtype=F64) * (hi - lo) + lo     # noqa: E731
    z1, l1, l2 = u(-5, 5), u(2, 6), u(2, 6)
    z2 = z1 + u(-1.5, 1.5)
    z2[::5] = z1[::5] + 0.5 * (l1[::5] + l2[::5]) + u(0.1, 2.0)[::5]
    z1[1], l1[1], z2[1], l2[1] = 0.0, 2.0, 3.0, 4.0                           # touching: z overlap exactly 0
    lift = lambda b, z, l: torch.stack([b[:, 0], b[:, 1], z.to(F32), b[:, 2], b[:, 3], l.to(F32), b[:, 4]], 1)     # noqa: E731
    return lift(b1, z1, l1), lift(b2, z2, l2)


# ---- one pair at a time ---------------------------------------------------------------------------------------------------------------
def _clip(poly, axis, sign, bound, line):
    """One Sutherland-Hodgman pass over poly, a list of (x, y, tag): keeps sign * coordinate[axis] <= bound.  A kept vertex keeps its
    tag, a crossing where the polygon leaves takes `line`, one where it enters takes the tag of the vertex it comes from."""
    out = []
    if not poly:
        return out
    px, py, ptag = poly[-1]
    pd = sign * (py if axis else px)
    pin = bool(pd <= bound)
    for qx, qy, qtag in poly:
        qd = sign * (qy if axis else qx)
        qin = bool(qd <= bound)
        if pin != qin and len(out) < 8:
            t = (bound - pd) / (qd - pd)
            out.append((px + t * (qx - px), sign * bound, line if pin else ptag) if axis else
                       (sign * bound, py + t * (qy - py), line if pin else ptag))
        if qin and len(out) < 8:
            out.append((qx, qy, qtag))
        px, py, ptag, pd, pin = qx, qy, qtag, qd, qin
    return out


def _polygon(a, b, cos, sin, num):
    """Box a = (cx, cy, w, h, angle) clipped to box b in b's frame: (poly, (ox, oy, cd, sd)); num makes a constant of the scalar type."""
    ca, sa, cb, sb = cos(a[4]), sin(a[4]), cos(b[4]), sin(b[4])
    dx, dy = a[0] - b[0], a[1] - b[1]
    ox, oy = dx * cb + dy * sb, dy * cb - dx * sb
    cd, sd = ca * cb + sa * sb, sa * cb - ca * sb
    if bool(sd == 0):
        cd = num(-1.0) if bool(cd < 0) else num(1.0)
    if bool(cd == 0):
        sd = num(-1.0) if bool(sd < 0) else num(1.0)
    hw, hh = num(0.5) * a[2], num(0.5) * a[3]
    ux, uy, vx, vy = hw * cd, hw * sd, -hh * sd, hh * cd
    poly = [((ox + ux) + vx, (oy + uy) + vy, 0), ((ox - ux) + vx, (oy - uy) + vy, 1), ((ox - ux) - vx, (oy - uy) - vy, 2),
            ((ox + ux) - vx, (oy + uy) - vy, 3)]
    bw, bh = num(0.5) * b[2], num(0.5) * b[3]
    for line, (axis, sign, bound) in enumerate(((0, 1.0, bw), (1, 1.0, bh), (0, -1.0, bw), (1, -1.0, bh))):
        poly = _clip(poly, axis, num(sign), bound, 4 + line)
    return poly, (ox, oy, cd, sd)


def _fan(poly, num):
    total = num(0.0)
    if len(poly) >= 3:
        x0, y0 = poly[0][:2]
        ex, ey = poly[1][0] - x0, poly[1][1] - y0
        for qx, qy, _ in poly[2:]:
            fx, fy = qx - x0, qy - y0
            total = total + (ex * fy - fx * ey)
            ex, ey = fx, fy
    return num(0.5) * abs(total)


def _row_ok(row):
    return all(math.isfinite(v) for v in row) and row[2] >= 0 and row[3] >= 0 and row[2] * row[3] >= R.MIN_AREA


def _truth_pair(row1, row2):
    """(iou, inter, d iou [10], d inter [10]) of one pair in float64 by autograd; zeros under the zero rule."""
    zero = torch.zeros((10,), dtype=F64)
    if not (_row_ok(row1) and _row_ok(row2)):
        return 0.0, 0.0, zero, zero
    leaf = torch.tensor(list(row1) + list(row2), dtype=F64, requires_grad=True)
    p = leaf.unbind()
    a, b = p[:5], p[5:]
    poly, _ = _polygon(a, b, torch.cos, torch.sin, lambda v: torch.tensor(v, dtype=F64))
    if len(poly) < 3:
        return 0.0, 0.0, zero, zero
    inter = _fan(poly, lambda v: torch.tensor(v, dtype=F64))
    iou = inter / ((a[2] * a[3] + b[2] * b[3]) - inter)
    d_iou, = torch.autograd.grad(iou, leaf, retain_graph=True)
    d_inter, = torch.autograd.grad(inter, leaf)
    return float(iou.detach()), float(inter.detach()), d_iou, d_inter


def _truth_of(b1, b2):
    rows = [_truth_pair(r1, r2) for r1, r2 in zip(b1.double().tolist(), b2.double().tolist())]
    return {"iou": torch.tensor([r[0] for r in rows], dtype=F64), "inter": torch.tensor([r[1] for r in rows], dtype=F64),
            "d_iou": torch.stack([r[2] for r in rows]), "d_inter": torch.stack([r[3] for r in rows])}


@functools.lru_cache(maxsize=None)
def truth(name):
    """The float64 truth of case(name): iou [n], inter [n], and the per-pair Jacobians d_iou, d_inter [n, 10] (box 1's five, box 2's)."""
    return _truth_of(*case(name))


def truth_grads(name, grad_iou, grad_inter):
    """(d_boxes1, d_boxes2) [n, 5] float64 of sum(grad_iou * iou + grad_inter * inter): the pairs are independent."""
    t = truth(name)
    d = grad_iou.double()[:, None] * t["d_iou"] + grad_inter.double()[:, None] * t["d_inter"]
    return d[:, :5], d[:, 5:]


def _analytic_pair(row1, row2, gi, gn, T):
    """The kernel's closed form for one pair on numpy scalars of type T: (iou, inter, d_box1 [5], d_box2 [5])."""
    z = [T(0.0)] * 5
    a, b = [T(v) for v in row1], [T(v) for v in row2]
    ok = lambda r: all(np.isfinite(v) for v in r) and r[2] >= 0 and r[3] >= 0 and r[2] * r[3] >= T(R.MIN_AREA)     # noqa: E731
    if not (ok(a) and ok(b)):
        return T(0.0), T(0.0), z, z
    with np.errstate(all="ignore"):
        poly, (ox, oy, cd, sd) = _polygon(a, b, np.cos, np.sin, T)
        area_a, area_b = a[2] * a[3], b[2] * b[3]
        inter = _fan(poly, T)
        iou = inter / ((area_a + area_b) - inter)
        if len(poly) < 3:
            return iou, inter, z, z
        length = [T(0.0)] * 8
        gd = T(0.0)
        normals = ((-sd, cd), (-cd, -sd), (sd, -cd), (cd, sd))
        px, py, tag = poly[-1]
        for qx, qy, qtag in poly:
            ex, ey = qx - px, qy - py
            ln = np.sqrt(ex * ex + ey * ey)
            if tag < 4:
                nx, ny = normals[tag]
                mx, my = T(0.5) * (px + qx) - ox, T(0.5) * (py + qy) - oy
                gd = gd + ln * (ny * mx - nx * my)
            length[tag] = length[tag] + ln
            px, py, tag = qx, qy, qtag
        l0, l1, l2, l3 = length[:4]
        lbw, lbh = length[4] + length[6], length[5] + length[7]
        gox, goy = sd * (l2 - l0) + cd * (l3 - l1), cd * (l0 - l2) + sd * (l3 - l1)
        u = (area_a + area_b) - inter
        g_inter = gn + gi * ((u + inter) / (u * u))
        g_area = -gi * (inter / (u * u))
        cb, sb = np.cos(b[4]), np.sin(b[4])
        gx, gy = g_inter * (gox * cb - goy * sb), g_inter * (gox * sb + goy * cb)
        half = T(0.5)
        d1 = [gx, gy, g_inter * (half * (l1 + l3)) + g_area * a[3], g_inter * (half * (l0 + l2)) + g_area * a[2], g_inter * gd]
        d2 = [-gx, -gy, g_inter * (half * lbw) + g_area * b[3], g_inter * (half * lbh) + g_area * b[2],
              g_inter * ((gox * oy - goy * ox) - gd)]
    return iou, inter, d1, d2


def analytic(b1, b2, grad_iou, grad_inter, dtype):
    """(iou [n], inter [n], d_boxes1 [n, 5], d_boxes2 [n, 5]) in dtype (float32 or float64) by the kernel's closed form."""
    T = np.float32 if dtype == F32 else np.float64
    conv = lambda t: t.to(dtype).tolist()     # noqa: E731
    rows = [_analytic_pair(r1, r2, T(gi), T(gn), T)
            for r1, r2, gi, gn in zip(conv(b1), conv(b2), conv(grad_iou), conv(grad_inter))]
    pick = lambda k: torch.tensor(np.array([r[k] for r in rows], dtype=T).reshape((len(rows),) + ((5,) if k > 1 else ())))     # noqa: E731
    return pick(0), pick(1), pick(2), pick(3)


def upstream(name, seed=0):
    """Random upstream gradients (grad_iou, grad_inter) [n] float32 for case(name)."""
    gen = torch.Generator().manual_seed(1000 + seed + len(name))
    n = case(name)[0].shape[0]
    return torch.randn((n,), generator=gen, dtype=F32), torch.randn((n,), generator=gen, dtype=F32)


# ---- seams ----------------------------------------------------------------------------------------------------------------------------
def _edges(b):
    """The four edges of boxes b [n, 5] float64 as (start [n, 4, 2], unit direction [n, 4, 2], length [n, 4])."""
    c, s = torch.cos(b[:, 4]), torch.sin(b[:, 4])
    u = torch.stack([c, s], 1)[:, None] * (0.5 * b[:, 2])[:, None, None]
    v = torch.stack([-s, c], 1)[:, None] * (0.5 * b[:, 3])[:, None, None]
    o = b[:, None, :2]
    corners = torch.cat([o + u + v, o - u + v, o - u - v, o + u - v], 1)
    d = corners.roll(-1, 1) - corners
    length = d.norm(dim=2)
    return corners, d / length[..., None], length


def near_seam(b1, b2):
    """bool [n]: the pairs with an edge of box 1 within ANGLE_TOL of parallel to an edge of box 2, the two lines closer than DIST_TOL
    times the pair's longest side somewhere on the stretch that both edges cover."""
    a, b = b1.double(), b2.double()
    ok = R.box_ok(a) & R.box_ok(b)
    unit = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0], dtype=F64)
    a, b = torch.where(ok[:, None], a, unit), torch.where(ok[:, None], b, unit)
    tol = DIST_TOL * torch.maximum(a[:, 2:4].max(1).values, b[:, 2:4].max(1).values)
    pa, da, la = _edges(a)
    pb, db, lb = _edges(b)
    mark = torch.zeros_like(ok)
    for i in range(4):
        for j in range(4):
            di, dj = da[:, i], db[:, j]
            parallel = (di[:, 0] * dj[:, 1] - di[:, 1] * dj[:, 0]).abs() < math.sin(ANGLE_TOL)
            nj = torch.stack([-dj[:, 1], dj[:, 0]], 1)
            rel0, rel1 = pa[:, i] - pb[:, j], pa[:, i] + di * la[:, i, None] - pb[:, j]
            s0, s1 = (rel0 * dj).sum(1), (rel1 * dj).sum(1)                     # edge i's end points along edge j
            h0, h1 = (rel0 * nj).sum(1), (rel1 * nj).sum(1)                     # and their signed distances from its line
            lo, hi = torch.minimum(s0, s1).clamp(min=0), torch.minimum(torch.maximum(s0, s1), lb[:, j])
            span = torch.where((s1 - s0).abs() > 0, s1 - s0, torch.ones_like(s0))
            at = lambda s: h0 + (h1 - h0) * (s - s0) / span                    # noqa: E731
            e0, e1 = at(lo), at(hi)
            dist = torch.where(e0 * e1 <= 0, torch.zeros_like(e0), torch.minimum(e0.abs(), e1.abs()))
            mark |= parallel & (hi >= lo) & (dist < tol)
    return mark & ok


@functools.lru_cache(maxsize=None)
def seam(name):
    return near_seam(*case(name))


def check_conditions(name):
    """The cap on the pairs left out; returns (overlapping pairs, pairs left out)."""
    t, s = truth(name), seam(name)
    over = t["inter"] > 0
    left_out = int((s & over).sum())
    assert left_out <= SEAM_CAP * max(int(over.sum()), 1), (name, left_out, int(over.sum()))
    if name == "jitter":
        assert left_out == 0 and bool(over.all()), (name, left_out)
    return int(over.sum()), left_out


# ---- 3-D ------------------------------------------------------------------------------------------------------------------------------
BEV = [0, 1, 3, 4, 6]                                                         # the columns (x, y, w, h, alpha) of a 3-D row


def _compose_3d(b1, b2, inter2d, grad):
    """mmcv's 3-D definition around a given inter2d: (iou3d, d iou3d / d inter2d, d_box3d1, d_box3d2 without the path through inter2d)
    under the upstream gradient grad, by autograd in the dtype of the arguments."""
    b1, b2, inter2d = (t.clone().requires_grad_(True) for t in (b1, b2, inter2d))
    z_overlap = (torch.minimum(b1[:, 2] + b1[:, 5] / 2, b2[:, 2] + b2[:, 5] / 2)
                 - torch.maximum(b1[:, 2] - b1[:, 5] / 2, b2[:, 2] - b2[:, 5] / 2)).clamp_min(0)
    inter3d = inter2d * z_overlap
    vol1, vol2 = b1[:, 3] * b1[:, 4] * b1[:, 5], b2[:, 3] * b2[:, 4] * b2[:, 5]
    iou = inter3d / (vol1 + vol2 - inter3d)
    g_inter, g1, g2 = torch.autograd.grad(iou, (inter2d, b1, b2), grad.to(iou.dtype))
    return iou.detach(), g_inter, g1, g2


def truth_3d(grad, name="jitter3d"):
    """(iou3d [n], d_box3d1 [n, 7], d_box3d2 [n, 7]) float64: the definition around the truth's inter2d, the chain rule through inter2d
    written out with the truth's Jacobian."""
    t = truth("jitter")
    iou, g_inter, g1, g2 = _compose_3d(*(b.double() for b in case_3d(name)), t["inter"], grad)
    g1[:, BEV] += g_inter[:, None] * t["d_inter"][:, :5]
    g2[:, BEV] += g_inter[:, None] * t["d_inter"][:, 5:]
    return iou, g1, g2


def single_3d(grad, name="jitter3d"):
    """The same in float32 around the float32 closed form: the err_ref of the 3-D comparison."""
    p1, p2 = case("jitter")
    n = p1.shape[0]
    inter = analytic(p1, p2, torch.zeros(n), torch.ones(n), F32)[1]
    iou, g_inter, g1, g2 = _compose_3d(*case_3d(name), inter, grad)
    _, _, d1, d2 = analytic(p1, p2, torch.zeros(n), g_inter, F32)
    g1[:, BEV] += d1
    g2[:, BEV] += d2
    return iou, g1, g2
