"""fasterrcnn_amd.ops.prroi_pool without a GPU: the two float64 restatements of tests/prroi_cases.py agree with each other and with the
properties of an exact integral of the bilinear surface; prroi_pool_pytorch (the composition from torch operations) equals them in the
output and in both gradients, bin edges on integers included; and the wrapper, the module and the C entry points check their arguments.

Bounds.  Float64 quantities that are the same sums in another order agree to 1e-12 relative (2**-53 times a few hundred terms, and for
the `narrow` case times the 1 / bin ~ 100 by which a weight's rounding is amplified).  The central differences of restatement B have the
error STEP * |second derivative| (the operator is C1 with a piecewise continuous second derivative, so the second-order term does not
cancel at a kink) plus 2**-53 / STEP rounding; with STEP = 2**-20 and a second derivative taken to be below 64 times the largest
gradient (the shortest length in any case is a bin of 1 / 64 of a cell) that is 64 * STEP relative to max|d_rois|."""
import os
import re

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import prroi_cases as P

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME_SUMS = 1e-12
DIFFERENCES = 64 * P.STEP


@pytest.fixture(scope="module", params=list(P.CASES))
def truth(request):
    case = P.make_case(request.param)
    return case, (P.forward_ref(case, F64),) + P.grads_ref(case, F64)


# ---- the restatements -----------------------------------------------------------------------------------------------------------------------
def test_the_two_restatements_agree(truth):
    case, (out, dx, drois) = truth
    P.check_conditions(case, (out, dx, drois))
    assert P.rel_err(P.forward_direct(case), out) <= SAME_SUMS
    assert P.rel_err(P.input_grad_direct(case), dx) <= SAME_SUMS
    err = P.rel_err(P.roi_grad_direct(case), drois)
    print("%s: analytic d_rois against central differences %.2e (bound %.2e)" % (case["name"], err, DIFFERENCES))
    assert err <= DIFFERENCES
    assert not bool(drois[:, 0].any())


def test_a_box_beyond_the_margin_pools_to_zeros_with_a_zero_gradient():
    case = P.make_case("beyond")
    out, (dx, drois) = P.forward_ref(case, F64), P.grads_ref(case, F64)
    assert not bool(out[P.BEYOND_ROW].any()) and not bool(drois[P.BEYOND_ROW].any())
    assert not bool(P.forward_direct(case)[P.BEYOND_ROW].any())


def test_degenerate_rois_pool_to_zeros_in_every_restatement():
    """The definition is a float32 one (an area that overflows float32 is not pooled), so the float32 evaluations are asked; the float64
    ones are asked for every row but the overflowing one."""
    case = dict(P.make_case("beyond"))
    case["rois"], names = P.degenerate_rois(case["input"].shape[0])
    case["grad"] = torch.ones((len(names), 4, 2, 3))
    alone = dict(case, rois=case["rois"][:1], grad=case["grad"][:1])
    assert torch.equal(P.geometry(case, F32)["valid"], torch.tensor([True] + [False] * (len(names) - 1)))
    for dtype, rows in ((F32, list(range(1, len(names)))), (F64, [i for i, name in enumerate(names) if i and name != "1e30"])):
        out, (dx, drois) = P.forward_ref(case, dtype), P.grads_ref(case, dtype)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(drois).all())
        assert float(out[0].abs().max()) > 0.1 and not bool(out[rows].any()) and not bool(drois[rows].any())
        if dtype == F32:
            assert torch.equal(dx, P.grads_ref(alone, dtype)[0]) and torch.equal(drois[:1], P.grads_ref(alone, dtype)[1])
            x = case["input"].clone().requires_grad_(True)
            r = case["rois"].clone().requires_grad_(True)
            py = ops.prroi_pool_pytorch(x, r, case["output_size"], case["spatial_scale"])
            py.backward(case["grad"])
            assert not bool(py[1:].any()) and not bool(r.grad[1:].any()) and bool(torch.isfinite(x.grad).all())
            assert P.rel_err(py[:1].detach(), out[:1]) <= 1e-5 and P.rel_err(x.grad, dx) <= 1e-5
        else:
            assert not bool(P.forward_direct(case)[rows].any())


@pytest.mark.parametrize("name", ["c6-7x7", "borders", "1x1"])
def test_midpoint_quadrature_of_the_surface_converges_to_the_output(name):
    """The midpoint rule on m x m pieces per bin has an O(1 / m**2) error on a piecewise bilinear surface: 4 times the pieces per axis
    must cut it by about 16 (at least 8 is asked), and at m = 64 it is below 1e-3 of the largest output."""
    case = P.make_case(name)
    out = P.forward_ref(case, F64)
    g = P.geometry(case, F64)
    errs = []
    for m in (16, 64):
        t = (torch.arange(m, dtype=F64) + 0.5) / m
        x = g["xs"][:, :, None] + t * g["bw"][:, None, None]                                      # [K, ow, m]
        y = g["ys"][:, :, None] + t * g["bh"][:, None, None]                                      # [K, oh, m]
        quad = torch.zeros_like(out)
        for k in range(out.shape[0]):
            yy, xx = y[k][:, None, :, None].expand(-1, x.shape[1], -1, m), x[k][None, :, None, :].expand(y.shape[1], -1, m, -1)
            quad[k] = P.surface(case, int(g["image"][k]), xx, yy).mean((3, 4))
        errs.append(P.rel_err(quad, out))
    print("%s: midpoint rule %.2e (m = 16), %.2e (m = 64)" % (name, errs[0], errs[1]))
    assert errs[1] <= errs[0] / 8 and errs[1] <= 1e-3


def test_a_unit_bin_between_four_cells_gives_their_mean():
    case = dict(P.make_case("c6-7x7"), output_size=(1, 1))
    x = case["input"].double()
    for j, i in ((0, 0), (3, 5), (7, 9)):
        case["rois"] = torch.tensor([[0.0, i, j, i + 1, j + 1]], dtype=F32)
        want = x[0, :, j:j + 2, i:i + 2].mean((1, 2))
        assert float((P.forward_ref(case, F64)[0, :, 0, 0] - want).abs().max()) <= 1e-14
        assert float((P.forward_direct(case)[0, :, 0, 0] - want).abs().max()) <= 1e-14


def test_an_affine_map_gives_the_value_at_the_bin_centre():
    base = P.make_case("c6-7x7")
    n, c, h, w = base["input"].shape
    coeff = torch.tensor([[0.3, -1.2, 0.7], [1.1, 0.4, -0.5], [-2.0, 0.25, 0.125], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [5.0, 0.0, 0.0]], dtype=F64)
    jj, ii = torch.arange(h, dtype=F64)[:, None], torch.arange(w, dtype=F64)[None, :]
    plane = coeff[:, 0, None, None] + coeff[:, 1, None, None] * ii + coeff[:, 2, None, None] * jj
    case = dict(base, input=plane[None])
    g = P.geometry(case, F64)
    assert float(g["x1"].min()) >= 0 and float(g["y1"].min()) >= 0
    assert float((g["xe"][:, -1]).max()) <= w - 1 and float((g["ye"][:, -1]).max()) <= h - 1
    cx, cy = (g["xs"] + g["xe"]) / 2, (g["ys"] + g["ye"]) / 2
    want = coeff[None, :, 0, None, None] + coeff[None, :, 1, None, None] * cx[:, None, None, :] + coeff[None, :, 2, None, None] * cy[:, None, :, None]
    assert P.rel_err(P.forward_ref(case, F64), want) <= SAME_SUMS
    assert P.rel_err(P.forward_direct(case), want) <= SAME_SUMS


@pytest.mark.parametrize("name", ["c6-7x7", "borders", "narrow"])
def test_one_bin_is_the_mean_of_its_two_by_two_bins(name):
    case = P.make_case(name)
    one = P.forward_ref(dict(case, output_size=(1, 1)), F64)
    four = P.forward_ref(dict(case, output_size=(2, 2)), F64)
    assert float(one.abs().max()) > 0.1
    assert P.rel_err(four.mean((2, 3), keepdim=True), one) <= SAME_SUMS


# ---- the composition from torch operations ------------------------------------------------------------------------------------------------
def test_the_torch_composition_equals_the_restatement_with_both_gradients(truth):
    case, (out, dx, drois) = truth
    x = case["input"].double().requires_grad_(True)
    r = case["rois"].double().requires_grad_(True)
    got = ops.prroi_pool_pytorch(x, r, case["output_size"], case["spatial_scale"])
    assert got.dtype == F64 and got.shape == out.shape
    got.backward(case["grad"].double())
    # the antiderivative form cancels where a bin is narrow: the `narrow` bins are 1 / 100 of a cell, two orders more rounding
    tol = SAME_SUMS * (100 if case["name"] == "narrow" else 1)
    assert P.rel_err(got.detach(), out) <= tol and P.rel_err(x.grad, dx) <= tol and P.rel_err(r.grad, drois) <= tol
    assert not bool(r.grad[:, 0].any())


def test_the_torch_composition_takes_lists_and_16_bit_maps():
    case = P.make_case("c260-two-images")
    rois = case["rois"]
    order = torch.cat([(rois[:, 0] == b).nonzero()[:, 0] for b in (0, 1)])
    boxes = [rois[rois[:, 0] == b, 1:].clone().requires_grad_(True) for b in (0, 1)]
    x = case["input"]
    got = ops.prroi_pool_pytorch(x, boxes, case["output_size"], case["spatial_scale"])
    want = ops.prroi_pool_pytorch(x, rois[order], case["output_size"], case["spatial_scale"])
    assert got.dtype == F32 and torch.equal(got, want)
    got.sum().backward()
    assert boxes[0].grad.shape == boxes[0].shape and bool(boxes[1].grad.any())
    half = ops.prroi_pool_pytorch(x.bfloat16(), rois, case["output_size"], case["spatial_scale"])
    assert half.dtype == torch.bfloat16
    assert torch.equal(half, ops.prroi_pool_pytorch(x.bfloat16().float(), rois, case["output_size"], case["spatial_scale"]).bfloat16())
    assert ops.prroi_pool_pytorch(x, rois[:0], 2).shape == (0, 260, 2, 2)
    with pytest.raises(ValueError):
        ops.prroi_pool_pytorch(x, rois[:, :4], 2)
    with pytest.raises(ValueError):
        ops.prroi_pool_pytorch(x[0], rois, 2)
    with pytest.raises(TypeError):
        ops.prroi_pool_pytorch(x.long(), rois, 2)


# ---- registrations, shapes and dtypes on meta -----------------------------------------------------------------------------------------------
def test_ops_are_registered_with_fake_implementations():
    x = torch.empty((2, 6, 5, 4), device="meta").requires_grad_(True)
    rois = torch.empty((3, 5), device="meta").requires_grad_(True)
    out = ops.prroi_pool(x, rois, (3, 5), 0.5)
    assert out.shape == (3, 6, 3, 5) and out.dtype == F32 and out.is_contiguous(memory_format=torch.channels_last)
    out.sum().backward()
    assert x.grad.shape == x.shape and rois.grad.shape == rois.shape and rois.grad.dtype == F32
    for dtype in (torch.float16, torch.bfloat16):
        xh = torch.empty((2, 6, 5, 4), device="meta", dtype=dtype).requires_grad_(True)
        rh = torch.empty((3, 5), device="meta", dtype=dtype).requires_grad_(True)
        out = ops.prroi_pool(xh, rh, 7)
        assert out.shape == (3, 6, 7, 7) and out.dtype == dtype
        out.sum().backward()
        assert xh.grad.dtype == dtype and rh.grad.dtype == dtype and rh.grad.shape == (3, 5)
        assert ops.prroi_pool(xh, rois, 7).dtype == dtype                   # float32 RoIs with a 16-bit map
    boxes = [torch.empty((2, 4), device="meta").requires_grad_(True), torch.empty((1, 4), device="meta").requires_grad_(True)]
    out = ops.PrRoIPool((2, 3), 0.25)(x, boxes)
    assert out.shape == (3, 6, 2, 3)
    out.sum().backward()
    assert boxes[0].grad.shape == (2, 4) and boxes[1].grad.shape == (1, 4)
    xc = torch.empty((2, 6, 5, 4), device="meta").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ops.prroi_pool(xc, rois, 2).sum().backward()
    assert xc.grad.is_contiguous(memory_format=torch.channels_last)
    assert ops.prroi_pool(x, torch.empty((0, 5), device="meta"), 2).shape == (0, 6, 2, 2)
    assert ops.PRROI_CULL_LIST == P.CULL_LIST == nv.lib().frcnn_ops_prroi_pool_cull_list()
    for name in ("prroi_pool", "PrRoIPool", "prroi_pool_pytorch"):
        assert name in ops.__all__
    assert repr(ops.PrRoIPool(7, 0.0625)) == "PrRoIPool(output_size=(7, 7), spatial_scale=0.0625)"
    assert not list(ops.PrRoIPool(7).parameters())


# ---- the wrapper's argument checks -----------------------------------------------------------------------------------------------------
def test_wrapper_rejects_cpu_tensors_and_bad_arguments():
    x = torch.zeros((1, 4, 5, 4), device="meta")
    rois = torch.zeros((3, 5), device="meta")
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.prroi_pool(torch.zeros((1, 4, 5, 4)), torch.zeros((3, 5)), 2)
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.prroi_pool(x, torch.zeros((3, 5)), 2)
    with pytest.raises(TypeError, match="float64"):
        ops.prroi_pool(x.double(), rois, 2)
    with pytest.raises(TypeError, match="float64"):
        ops.prroi_pool(x, rois.double(), 2)
    with pytest.raises(TypeError):
        ops.prroi_pool(x, rois.half(), 2)                                  # 16-bit RoIs go with a map of their dtype only
    with pytest.raises(TypeError):
        ops.prroi_pool(x.half(), rois.bfloat16(), 2)
    with pytest.raises(TypeError):
        ops.prroi_pool(x, [[0.0, 0.0, 1.0, 1.0]], 2)
    with pytest.raises(TypeError):
        ops.prroi_pool(x, rois, 2.5)
    with pytest.raises(TypeError):
        ops.prroi_pool(x, rois, (2, 2, 2))
    with pytest.raises(ValueError, match=r"\(0, 2\)"):
        ops.prroi_pool(x, rois, (0, 2))
    with pytest.raises(ValueError, match="65"):
        ops.prroi_pool(x, rois, ops.MAX_OUTPUT + 1)
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        ops.prroi_pool(x, torch.zeros((3, 4), device="meta"), 2)
    with pytest.raises(ValueError, match=r"\(2, 5\)"):
        ops.prroi_pool(x, [torch.zeros((2, 5), device="meta")], 2)
    with pytest.raises(ValueError, match=r"\(4, 5, 4\)"):
        ops.prroi_pool(x[0], rois, 2)
    with pytest.raises(ValueError):
        ops.PrRoIPool(0)
    with pytest.raises(TypeError):
        ops.PrRoIPool("7")


# ---- FRCNN_EINVAL of the entry points, with null pointers and no device ------------------------------------------------------------------
PTR = 0x1000        # a non-null pointer that is never dereferenced: every call below fails its validation first
GOOD = dict(n_img=1, fh=5, fw=4, c=8, k=3, out_h=2, out_w=2)
BAD = [dict(out_h=0), dict(out_h=65), dict(out_w=0), dict(out_w=65), dict(k=-1), dict(n_img=0), dict(fh=0), dict(fw=0), dict(c=0),
       dict(c=6), dict(fh=65536, fw=65536), dict(k=2 ** 30, out_h=2, out_w=2), dict(n_img=65536), dict(fh=131071, fw=1)]


def forward(lib, half, a, x=PTR, rois=PTR, out=PTR, elem=nv.OPS_F16):
    args = (x, a["n_img"], a["fh"], a["fw"], a["c"], rois, a["k"], a["out_h"], a["out_w"], 0.5, out, None)
    return lib.frcnn_ops_prroi_pool_16(elem, *args) if half else lib.frcnn_ops_prroi_pool(*args)


def backward(lib, half, a, x=PTR, rois=PTR, dout=PTR, dx=PTR, drois=PTR, ws=PTR, ws_bytes=1 << 40, elem=nv.OPS_BF16):
    args = (x, rois, a["k"], a["n_img"], a["fh"], a["fw"], a["c"], a["out_h"], a["out_w"], 0.5, dout, dx, drois, ws, ws_bytes, None)
    return lib.frcnn_ops_prroi_pool_backward_16(elem, *args) if half else lib.frcnn_ops_prroi_pool_backward(*args)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "16"])
def test_entry_points_validate_before_touching_the_gpu(half):
    lib = nv.lib()
    for bad in BAD:
        a = dict(GOOD, **bad)
        assert forward(lib, half, a) == -1, bad
        assert backward(lib, half, a) == -1, bad
    if half:
        assert forward(lib, True, dict(GOOD, c=4)) == -1                   # 16-bit runs are 8 channels
        assert forward(lib, True, GOOD, elem=0) == -1 and forward(lib, True, GOOD, elem=3) == -1
        assert backward(lib, True, GOOD, elem=0) == -1 and backward(lib, True, GOOD, elem=3) == -1
    for null in ("x", "rois", "out"):
        assert forward(lib, half, GOOD, **{null: None}) == -1, null
    for null in ("rois", "dout", "x", "ws"):
        assert backward(lib, half, GOOD, **{null: None}) == -1, null
    assert backward(lib, half, GOOD, dx=None, drois=None) == -1             # nothing to compute
    assert backward(lib, half, GOOD, ws=PTR + 4) == -1                      # a misaligned workspace
    need = lib.frcnn_ops_prroi_pool_workspace_bytes(GOOD["k"], GOOD["out_h"], GOOD["out_w"])
    assert need == 3 * 4 * 16
    assert backward(lib, half, GOOD, ws_bytes=need - 1) == -1
    assert forward(lib, half, dict(GOOD, k=0), x=None, rois=None, out=None) == 0          # nothing to pool: no launch
    for args in ((-1, 2, 2), (3, 0, 2), (3, 2, 65), (2 ** 30, 2, 2)):
        assert lib.frcnn_ops_prroi_pool_workspace_bytes(*args) == 0, args
    assert lib.frcnn_ops_prroi_pool_workspace_bytes(0, 2, 2) == 0


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_number_and_symbol_table_still_agree_with_the_header():
    text = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert re.search(r"#define FRCNN_ABI_VERSION (\d+)", text).group(1) == "21"
    assert nv.ABI_VERSION == 21 == nv.lib().frcnn_abi_version()
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    ours = {"frcnn_ops_prroi_pool", "frcnn_ops_prroi_pool_backward", "frcnn_ops_prroi_pool_16", "frcnn_ops_prroi_pool_backward_16",
            "frcnn_ops_prroi_pool_workspace_bytes", "frcnn_ops_prroi_pool_cull_list"}
    assert ours <= declared and declared == set(nv.SYMBOLS)
    for name in ours:
        assert hasattr(nv.lib(), name), name
