"""fasterrcnn_amd.ops.diff_iou_rotated_2d / _3d / _2d_pytorch without a GPU: the self-checks of the restatements in
tests/diff_iou_cases.py (the closed-form gradient against float64 autograd, the cap on the pairs left out near seams), the torch
composition against the per-pair truth, the argument rules of the public functions, shapes and dtypes on meta and fake tensors, the
validation of the C entry points and the ABI.

Measured here: the closed form in float64 agrees with autograd through the per-pair clip to 3.0e-15 of the largest gradient on every pair
of every random case (bound 1e-9); diff_iou_rotated_2d_pytorch in float64 agrees in value exactly (bound 1e-12) and in gradient, on
the pairs away from seams, to 1.3e-15 of the largest gradient (bound 1e-6: it differentiates the clip's own t, which is ill-conditioned
for nearly parallel crossings)."""
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import diff_iou_cases as D
from tests import rotated_cases as R

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("diff_iou_rotated_2d", "diff_iou_rotated_3d", "diff_iou_rotated_2d_pytorch")
ENTRY_POINTS = {"frcnn_ops_diff_iou_rotated", "frcnn_ops_diff_iou_rotated_backward"}


def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def worst(got, want, keep=None):
    """max |got - want| over the kept rows of the tensors, relative to the largest |want| of the case."""
    scale = max(float(w.abs().max()) for w in want)
    pick = (lambda t: t) if keep is None else (lambda t: t[keep])
    return max(float(pick(g.double() - w).abs().max()) if pick(g).numel() else 0.0 for g, w in zip(got, want)) / scale


# ---- 1. the restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.RANDOM_CASES + D.SPECIAL_CASES)
def test_truth_values_are_the_vectorised_restatements(name):
    b1, b2 = D.case(name)
    t = D.truth(name)
    assert b1.shape == b2.shape and b1.dtype == F32 and t["iou"].shape == (b1.shape[0],) and t["d_iou"].shape == (b1.shape[0], 10)
    assert float((t["iou"] - R.iou_pairs(b1, b2)).abs().max()) <= 1e-12
    assert all(bool(torch.isfinite(v).all()) for v in t.values())


@pytest.mark.parametrize("name", D.RANDOM_CASES)
def test_seam_cap_and_overlap_of_the_random_cases(name):
    over, left_out = D.check_conditions(name)
    assert over >= 1
    if name == "jitter":
        iou = D.truth(name)["iou"]
        assert 0.35 < float(iou.min()) and float(iou.max()) < 0.95


def test_special_is_made_of_seams_and_zero_rows():
    b, _ = D.case("special")
    assert bool(D.seam("special")[R.box_ok(b)].all())
    t = D.truth("special")
    rows = list(R.ZERO_RULE_ROWS)
    assert not bool(t["iou"][rows].any()) and not bool(t["d_iou"][rows].any()) and bool((t["iou"][R.box_ok(b)] == 1).all())
    assert bool((D.truth("special-shift")["inter"] > 0).sum() >= 8)


@pytest.mark.parametrize("name", D.RANDOM_CASES)
def test_closed_form_agrees_with_autograd_in_float64(name):
    b1, b2 = D.case(name)
    gi, gn = D.upstream(name)
    iou, inter, d1, d2 = D.analytic(b1, b2, gi, gn, F64)
    t = D.truth(name)
    assert float((iou - t["iou"]).abs().max()) <= 1e-12 and float((inter - t["inter"]).abs().max()) <= 1e-12 * float(t["inter"].max())
    err = worst((d1, d2), D.truth_grads(name, gi, gn))                       # nothing excluded
    print("%s closed form against autograd: %.3e" % (name, err))
    assert err <= 1e-9


def test_closed_form_in_float32_is_a_few_ulps_away():
    for name in ("130", "jitter"):
        b1, b2 = D.case(name)
        gi, gn = D.upstream(name)
        _, _, d1, d2 = D.analytic(b1, b2, gi, gn, F32)
        assert d1.dtype == F32 and worst((d1, d2), D.truth_grads(name, gi, gn), ~D.seam(name)) < 2e-5


def test_3d_truth_is_the_definition():
    """The hand-written chain rule of truth_3d against central differences of the definition, and the axis-aligned closed form."""
    grad = torch.ones((200,), dtype=F64)
    iou, g1, g2 = D.truth_3d(grad)
    b1, b2 = (t.double() for t in D.case_3d())
    assert float(iou[1]) == 0.0 and not bool(iou[::5].any()) and int((iou > 0).sum()) >= 150 and float(iou.max()) < 1.0
    assert not bool(g1[::5].any()) and not bool(g2[::5].any())

    def value(r1, r2):
        inter2d = D._truth_pair([r1[c] for c in D.BEV], [r2[c] for c in D.BEV])[1]
        z = max(min(r1[2] + r1[5] / 2, r2[2] + r2[5] / 2) - max(r1[2] - r1[5] / 2, r2[2] - r2[5] / 2), 0.0)
        return inter2d * z / (r1[3] * r1[4] * r1[5] + r2[3] * r2[4] * r2[5] - inter2d * z)

    step = 1e-6
    for p in (2, 3, 7, 11):
        r1, r2 = b1[p].tolist(), b2[p].tolist()
        assert abs(value(r1, r2) - float(iou[p])) <= 1e-14
        for k in range(14):
            hi, lo = list(r1 + r2), list(r1 + r2)
            hi[k] += step
            lo[k] -= step
            numeric = (value(hi[:7], hi[7:]) - value(lo[:7], lo[7:])) / (2 * step)
            assert abs(numeric - float((g1[p].tolist() + g2[p].tolist())[k])) <= 1e-7, (p, k)
    a = [1.0, 2.0, 0.5, 4.0, 6.0, 2.0, 0.0]
    b = [2.0, 1.0, 1.0, 4.0, 4.0, 3.0, 0.0]
    assert abs(value(a, b) - (3.0 * 4.0 * 2.0) / (48.0 + 48.0 - 24.0)) <= 1e-15     # overlaps 3 x 4 x 2 of two volumes of 48


# ---- 2. the torch composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.RANDOM_CASES + D.SPECIAL_CASES)
def test_pytorch_composition_in_float64_against_the_truth(name):
    b1, b2 = (t.double().requires_grad_(True) for t in D.case(name))
    gi, _ = D.upstream(name)
    iou = ops.diff_iou_rotated_2d_pytorch(b1, b2)
    t = D.truth(name)
    assert iou.dtype == F64 and iou.shape == t["iou"].shape and float((iou.detach() - t["iou"]).abs().max()) <= 1e-12
    (iou * gi.double()).sum().backward()
    assert bool(torch.isfinite(b1.grad).all()) and bool(torch.isfinite(b2.grad).all())       # on the NaN / inf rows of special too
    if name in D.SPECIAL_CASES:
        rows = list(R.ZERO_RULE_ROWS)
        assert not bool(b1.grad[rows].any())
        return
    err = worst((b1.grad, b2.grad), D.truth_grads(name, gi, torch.zeros_like(gi)), ~D.seam(name))
    print("%s composition against autograd truth: %.3e" % (name, err))
    assert err <= 1e-6


def test_pytorch_composition_shapes_dtypes_and_errors():
    b1, b2 = D.case("130")
    flat = ops.diff_iou_rotated_2d_pytorch(b1, b2)
    assert flat.dtype == F32 and flat.shape == (130,)
    assert torch.equal(ops.diff_iou_rotated_2d_pytorch(b1.view(2, 65, 5), b2.view(2, 65, 5)), flat.view(2, 65))
    assert float((flat.double() - D.truth("130")["iou"]).abs().max()) < 1e-5
    b = D.case("special")[0].clone().requires_grad_(True)                  # float32: finite gradients on every input
    ops.diff_iou_rotated_2d_pytorch(b, b.detach().roll(1, 0)).sum().backward()
    assert bool(torch.isfinite(b.grad).all())
    assert ops.diff_iou_rotated_2d_pytorch(b1[:0], b2[:0]).shape == (0,)
    with pytest.raises(TypeError):
        ops.diff_iou_rotated_2d_pytorch(b1, [1.0])
    with pytest.raises(TypeError, match="float16"):
        ops.diff_iou_rotated_2d_pytorch(b1.half(), b2.half())
    with pytest.raises(ValueError, match=r"\(130, 4\)"):
        ops.diff_iou_rotated_2d_pytorch(b1[:, :4], b2[:, :4])
    with pytest.raises(ValueError):
        ops.diff_iou_rotated_2d_pytorch(b1, b2[:65])
    with pytest.raises(ValueError):
        ops.diff_iou_rotated_2d_pytorch(b1, b2.double())


# ---- 3. the public functions: names, errors, meta --------------------------------------------------------------------------------------
def test_names_are_exported_and_documented():
    for name in NAMES:
        assert name in ops.__all__ and callable(getattr(ops, name)) and name in ops.__doc__ and getattr(ops, name).__doc__
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "diff_iou_rotated_2d" in open(os.path.join(ROOT, doc)).read(), doc
    assert "MAX_ROTATED_IOU_ROWS" in ops.__doc__


def test_abi_number_and_the_two_entry_points():
    text = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert re.search(r"#define FRCNN_ABI_VERSION (\d+)", text).group(1) == "21"
    assert nv.ABI_VERSION == 21 == nv.lib().frcnn_abi_version()
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert ENTRY_POINTS <= declared and declared == set(nv.SYMBOLS)
    assert {s for s in nv.SYMBOLS if "diff_iou" in s} == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(nv.lib(), name), name


def test_wrappers_reject_bad_arguments():
    for fn, last in ((ops.diff_iou_rotated_2d, 5), (ops.diff_iou_rotated_3d, 7)):
        good = meta(2, 3, last)
        with pytest.raises(TypeError, match="torch.Tensor"):
            fn(good, [[0.0] * last])
        with pytest.raises(TypeError, match="float64"):
            fn(good.double(), good.double())
        for dtype in (torch.float16, torch.bfloat16):
            with pytest.raises(TypeError, match=r"\.float\(\)"):
                fn(good, meta(2, 3, last, dtype=dtype))
        with pytest.raises(ValueError, match=r"\(2, 4, %d\)" % last):
            fn(good, meta(2, 4, last))
        with pytest.raises(ValueError, match=r"\(2, 3, %d\)" % (last + 1)):
            fn(meta(2, 3, last + 1), meta(2, 3, last + 1))
        with pytest.raises(ValueError, match=r"\(%d,\)" % last):
            fn(meta(last), meta(last))
        with pytest.raises(ValueError, match=r"\(1, 2, 3, %d\)" % last):
            fn(meta(1, 2, 3, last), meta(1, 2, 3, last))
        with pytest.raises(ValueError, match="no CPU implementation"):
            fn(torch.zeros(3, last), torch.zeros(3, last))
        with pytest.raises(ValueError, match="cpu"):
            fn(good, torch.zeros(2, 3, last))                               # one on meta, one on the CPU
        n = ops.MAX_ROTATED_IOU_ROWS + 1
        with pytest.raises(ValueError, match=str(n)):
            fn(meta(n, last), meta(n, last))
    with pytest.raises(ValueError, match="diff_iou_rotated_2d_pytorch"):
        ops.diff_iou_rotated_2d(torch.zeros(3, 5), torch.zeros(3, 5))
    with FakeTensorMode():
        with pytest.raises(ValueError, match="same device"):
            ops.diff_iou_rotated_2d(torch.empty((3, 5), device="cuda:0"), torch.empty((3, 5), device="cuda:1"))


def test_meta_and_fake_shapes_and_dtypes():
    for shape in ((2, 3), (7,), (0,), (2, 0)):
        a, b = meta(*shape, 5).requires_grad_(True), meta(*shape, 5).requires_grad_(True)
        out = ops.diff_iou_rotated_2d(a, b)
        assert out.shape == shape and out.dtype == F32 and out.requires_grad
        out.sum().backward()
        assert a.grad.shape == a.shape and b.grad.shape == b.shape and a.grad.dtype == F32
        a3, b3 = meta(*shape, 7).requires_grad_(True), meta(*shape, 7)
        out = ops.diff_iou_rotated_3d(a3, b3)
        assert out.shape == shape and out.dtype == F32
        out.sum().backward()
        assert a3.grad.shape == a3.shape and b3.grad is None
    iou, inter = torch.ops.frcnn.diff_iou_rotated(meta(6, 5), meta(6, 5))
    assert iou.shape == inter.shape == (6,) and iou.dtype == inter.dtype == F32
    with FakeTensorMode():
        a = torch.empty((4, 5), device="cuda").requires_grad_(True)
        out = ops.diff_iou_rotated_2d(a, torch.empty((4, 5), device="cuda"))
        assert out.shape == (4,) and out.device.type == "cuda" and out.requires_grad
        assert ops.diff_iou_rotated_3d(torch.empty((2, 4, 7), device="cuda"), torch.empty((2, 4, 7), device="cuda")).shape == (2, 4)
    assert not ops.box_iou_rotated(meta(3, 5).requires_grad_(True), meta(3, 5), aligned=True).requires_grad     # still no autograd


def test_backward_on_meta_skips_what_is_not_needed_and_double_backward_raises():
    a, b, g = meta(6, 5), meta(6, 5), meta(6)
    for needs in ([True, True], [True, False], [False, True], [False, False]):
        got = torch.ops.frcnn.diff_iou_rotated_backward(g, g, a, b, needs)
        assert [tuple(t.shape) for t in got] == [(6, 5) if need else (0,) for need in needs]
    a.requires_grad_(True)
    d, = torch.autograd.grad(ops.diff_iou_rotated_2d(a, b).sum(), a, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        d.sum().backward()


# ---- 4. FRCNN_EINVAL of the entry points, with null pointers and no device ------------------------------------------------------------------
def test_entry_points_validate_before_touching_the_gpu():
    lib, p = nv.lib(), 0x1000                                              # never dereferenced: every call below fails validation first
    fwd, bwd = lib.frcnn_ops_diff_iou_rotated, lib.frcnn_ops_diff_iou_rotated_backward
    too_many = ops.MAX_ROTATED_IOU_ROWS + 1
    assert fwd(p, p, -1, p, p, None) == -1 and fwd(p, p, too_many, p, p, None) == -1
    for null in range(4):
        args = [p, p, 3, p, p, None]
        args[null if null < 2 else null + 1] = None
        assert fwd(*args) == -1, null
    assert fwd(None, None, 0, None, None, None) == 0                        # no pairs: nothing to do
    assert bwd(p, p, p, p, -1, p, p, None) == -1 and bwd(p, p, p, p, too_many, p, p, None) == -1
    assert bwd(None, p, p, p, 3, p, p, None) == -1 and bwd(p, None, p, p, 3, p, p, None) == -1
    assert bwd(p, p, None, None, 3, p, p, None) == -1                       # no upstream gradient at all
    assert bwd(p, p, p, p, 3, None, None, None) == -1                       # nothing to compute
    assert bwd(None, None, None, None, 0, None, None, None) == 0
