"""fasterrcnn_amd.ops.prroi_pool and PrRoIPool on the GPU against the float64 restatement (tests/prroi_cases.py) and on the properties the
kernels promise: degenerate boxes, the 16-bit contract, determinism, layouts, flags, lists of boxes.

The bound of every comparison with the float64 truth is measured in the same test, as in tests/test_ops_droi_gpu.py:
err(a) = max|a - truth| / max|truth|, err_ref is the error of the same restatement run in float32 on the CPU, and
err_gpu <= 4 * max(err_ref, 2**-24) must hold, with max|truth| > 0.1 (prroi_cases.check_conditions).  No bin is masked: the operator is
C1 in the box, integer coordinates are not seams.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: output 1.01, d_input 3.01 (narrow), d_rois 1.48
(out64); prroi_pool_pytorch on the GPU under the same rule, on the cases it is held to: 1.51.  The largest of all, 3.01, is inside the
margin of 4.  On `narrow` (exact bin edges) the float32 composition, whose weights are differences of antiderivatives, has ratio 170:
the case tells a cancelling weight formula from the kernels' one."""
import functools

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import prroi_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
HALF = [torch.float16, torch.bfloat16]


def run(case, dtype=F32, needs=(True, True), x_cl=False, grad_cl=True, rois=None, roi_dtype=F32, fn=None):
    """The operator on the GPU, forward and backward: (output, d_input or None, d_rois or None; for a list of boxes a list)."""
    x = case["input"].to(DEV).to(dtype)
    x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(needs[0])
    if rois is None:
        rois = case["rois"].to(DEV).to(roi_dtype).requires_grad_(needs[1])
    out = (ops.prroi_pool if fn is None else fn)(x, rois, case["output_size"], case["spatial_scale"])
    if out.requires_grad:
        grad = case["grad"].to(DEV).to(dtype)
        out.backward(grad.contiguous(memory_format=CL) if grad_cl else grad.contiguous())
    return out.detach(), x.grad, [b.grad for b in rois] if isinstance(rois, list) else rois.grad


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case with its float64 truth and the float32 restatement's results (output, d_input, d_rois), computed once."""
    case = P.make_case(name)
    truth = (P.forward_ref(case, F64),) + P.grads_ref(case, F64)
    single = (P.forward_ref(case, F32),) + P.grads_ref(case, F32)
    P.check_conditions(case, truth)
    return case, truth, single


def check_against_truth(label, got, truth, single, names=("output", "d_input", "d_rois")):
    """err_gpu <= 4 * max(err_ref, 2**-24) for every quantity; prints both errors; returns the ratios."""
    ratios = {}
    for name, g, t, s in zip(names, got, truth, single):
        assert g.shape == t.shape and g.dtype == F32, name
        assert float(t.abs().max()) > 0.1, (label, name)
        err_gpu, err_ref = P.rel_err(g.cpu(), t), P.rel_err(s, t)
        ratios[name] = err_gpu / max(err_ref, FLOOR)
        print("%s %-8s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, ratios[name]))
        assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, name, err_gpu, err_ref)
    return ratios


# ---- 1. output, d_input and d_rois against the float64 restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_forward_and_gradients_against_float64(name):
    case, truth, single = reference(name)
    out, dx, drois = run(case)
    assert out.is_contiguous(memory_format=CL) or out.shape[1] == 1 or out.shape[2] * out.shape[3] == 1
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(drois).all())
    assert not bool(drois[:, 0].any())
    if name == "beyond":                                                   # wholly beyond the one-cell margin: exact zeros
        assert not bool(out[P.BEYOND_ROW].any()) and not bool(drois[P.BEYOND_ROW].any())
    check_against_truth(name, (out, dx, drois), truth, single)


@pytest.mark.parametrize("name", ["6x7-integer-edges", "borders", "c260-two-images", "narrow"])
def test_the_torch_composition_on_the_gpu_agrees_with_the_kernel(name):
    """prroi_pool_pytorch on the GPU: in float64 it is the truth to rounding (the bound of tests/test_ops_prroi_cpu.py: 1e-12, times 100
    where the `narrow` bins make its antiderivative form cancel); in float32 it is held to the rule the kernel is held to (the float32
    restatement's own error, margin 4), so the two agree to within that -- except on `narrow`, whose exact bin edges are there to
    make a difference of antiderivatives miss that rule: there the float32 composition is asked to miss it, which shows that the case
    tells the two weight formulas apart."""
    case, truth, single = reference(name)
    got64 = run(case, dtype=F64, roi_dtype=F64, fn=ops.prroi_pool_pytorch)
    tol = 1e-12 * (100 if name == "narrow" else 1)
    for g, t in zip(got64, truth):
        assert g.dtype == F64 and P.rel_err(g.cpu(), t) <= tol
    composed = run(case, fn=ops.prroi_pool_pytorch)
    if name == "narrow":
        err_py, err_ref = P.rel_err(composed[0].cpu(), truth[0]), P.rel_err(single[0], truth[0])
        print("narrow (composition) output   err %.3e err_ref %.3e ratio %.3f" % (err_py, err_ref, err_py / max(err_ref, FLOOR)))
        assert err_py > MARGIN * max(err_ref, FLOOR)
        return
    check_against_truth(name + " (composition)", composed, truth, single)


# ---- 2. degenerate RoIs ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_rois_pool_to_zeros_beside_an_unchanged_normal_roi():
    base = P.make_case("beyond")
    rois, names = P.degenerate_rois(base["input"].shape[0])
    gen = torch.Generator().manual_seed(5)
    case = dict(base, rois=rois, grad=torch.randn((len(names), 4, 2, 3), generator=gen))
    alone = dict(case, rois=rois[:1], grad=case["grad"][:1])
    out, dx, drois = run(case)
    out_a, dx_a, drois_a = run(alone)
    assert float(out_a.abs().max()) > 0.1 and float(dx_a.abs().max()) > 0.1 and float(drois_a.abs().max()) > 0.1
    assert torch.equal(out[:1], out_a) and torch.equal(dx, dx_a) and torch.equal(drois[:1], drois_a)
    for row, name in enumerate(names[1:], 1):
        assert not bool(out[row].any()) and not bool(drois[row].any()), name
    for dtype in HALF:
        out_h, dx_h, drois_h = run(case, dtype=dtype)
        assert not bool(out_h[1:].any()) and not bool(drois_h[1:].any()) and bool(torch.isfinite(dx_h).all())


def test_a_huge_finite_box_is_pooled_with_finite_results():
    """x2 = 1e30 alone, or a box of 2e15 x 2e15 around the map, leaves a finite float32 bin area (1e30 and 7e29): both RoIs are pooled,
    every cell range is clamped in float, the results are finite and tiny."""
    base = P.make_case("beyond")
    rois = torch.tensor([[0.0, 1.2, 0.9, 5.1, 4.3], [0.0, 1.0, 1.0, 1e30, 4.0], [0.0, -1e15, -1e15, 1e15, 1e15]], dtype=F32)
    case = dict(base, rois=rois, grad=base["grad"][:3])
    assert bool(P.geometry(case, F32)["valid"].all())
    out, dx, drois = run(case)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(drois).all())
    assert float(out[0].abs().max()) > 0.1 and float(out[1:].abs().max()) < 1e-20
    alone = run(dict(case, rois=rois[:1], grad=case["grad"][:1]))
    assert torch.equal(out[:1], alone[0]) and float((dx - alone[1]).abs().max()) < 1e-20


# ---- 3. the 16-bit contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["c6-7x7", "c260-two-images", "borders", "narrow"])
def test_16_bit_maps_equal_the_float32_operator_rounded_once(name, dtype):
    case = dict(P.make_case(name))
    case["input"] = case["input"].to(dtype).float()                      # the 16-bit values, exactly
    case["grad"] = case["grad"].to(dtype).float()
    out32, dx32, drois32 = run(case)
    out16, dx16, drois16 = run(case, dtype=dtype)
    assert out16.dtype == dtype and dx16.dtype == dtype and drois16.dtype == F32
    assert float(out32.abs().max()) > 0.1 and float(dx32.abs().max()) > 0.1 and float(drois32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(dtype)) and torch.equal(dx16, dx32.to(dtype))
    assert torch.equal(drois16, drois32)
    # RoIs in the map's dtype are widened for the kernels; their gradient is the float32 run's, rounded once
    case["rois"] = case["rois"].to(dtype).float()
    out32, dx32, drois32 = run(case)
    out_b, dx_b, drois_b = run(case, dtype=dtype, roi_dtype=dtype)
    assert drois_b.dtype == dtype and torch.equal(drois_b, drois32.to(dtype))
    assert torch.equal(out_b, out32.to(dtype)) and torch.equal(dx_b, dx32.to(dtype))


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cull", "c260-two-images", "out64"])
def test_two_runs_are_bit_identical(name):
    case = P.make_case(name)
    first, second = run(case), run(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert float(first[1].abs().max()) > 0.1 and float(first[2].abs().max()) > 0.1


def test_the_gather_needs_its_second_cull_pass_and_keeps_ascending_order():
    """The PRROI_CULL_LIST + 6 boxes of `cull` lie all over one 3 x 3 map, whose tiles list more RoIs than one pass holds.  With one bin
    per RoI a cell gets one term per RoI, so d_input is the sum over the first PRROI_CULL_LIST RoIs with the last six RoIs' terms added
    one by one in ascending order, bit for bit."""
    case = P.make_case("cull")
    k = case["rois"].shape[0]
    assert k == ops.PRROI_CULL_LIST + 6 == nv.lib().frcnn_ops_prroi_pool_cull_list() + 6
    _, dx, _ = run(case)
    part = lambda a, b: run(dict(case, rois=case["rois"][a:b], grad=case["grad"][a:b]), needs=(True, False))[1]   # noqa: E731
    want = part(0, ops.PRROI_CULL_LIST)
    assert float(want.abs().max()) > 0.1
    for r in range(ops.PRROI_CULL_LIST, k):
        term = part(r, r + 1)
        assert bool(term.any())
        want = want + term
    assert torch.equal(dx, want)


# ---- 5. other behaviour -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c6-7x7", "c260-two-images"])
def test_layouts_give_the_same_bits_and_d_input_keeps_its_format(name):
    case = P.make_case(name)
    out, dx, drois = run(case)
    assert dx.is_contiguous()
    out_cl, dx_cl, drois_cl = run(case, x_cl=True, grad_cl=False)
    assert dx_cl.is_contiguous(memory_format=CL) and out_cl.is_contiguous(memory_format=CL)
    assert torch.equal(out, out_cl) and torch.equal(dx, dx_cl) and torch.equal(drois, drois_cl)


def test_needs_flags_skip_work():
    case = P.make_case("c6-7x7")
    out, dx, drois = run(case)
    out_a, dx_a, drois_a = run(case, needs=(True, False))
    out_b, dx_b, drois_b = run(case, needs=(False, True))
    assert drois_a is None and dx_b is None
    assert torch.equal(out, out_a) and torch.equal(out, out_b) and torch.equal(dx, dx_a) and torch.equal(drois, drois_b)
    out_c, dx_c, drois_c = run(case, needs=(False, False))
    assert dx_c is None and drois_c is None and torch.equal(out, out_c)
    x, rois, grad = (case[k].to(DEV) for k in ("input", "rois", "grad"))
    res = torch.ops.frcnn.prroi_pool_backward(grad, x, rois, case["spatial_scale"], 7, 7, [False, True], False)
    assert res[0].numel() == 0 and torch.equal(res[1], drois)
    res = torch.ops.frcnn.prroi_pool_backward(grad, x, rois, case["spatial_scale"], 7, 7, [True, False], False)
    assert res[1].numel() == 0 and torch.equal(res[0], dx)


def test_a_list_of_boxes_equals_the_tensor_form_and_gets_its_gradient():
    case = P.make_case("c260-two-images")
    rois = case["rois"]
    order = torch.cat([(rois[:, 0] == b).nonzero()[:, 0] for b in (0, 1)])
    sub = dict(case, rois=rois[order], grad=case["grad"][order])
    out, dx, drois = run(sub)
    boxes = [sub["rois"][sub["rois"][:, 0] == b, 1:].to(DEV).requires_grad_(True) for b in (0, 1)]
    out_l, dx_l, grads = run(sub, rois=boxes)
    assert torch.equal(out, out_l) and torch.equal(dx, dx_l)
    assert float(drois.abs().max()) > 0.1 and torch.equal(torch.cat(grads), drois[:, 1:])
    assert [tuple(g.shape) for g in grads] == [tuple(b.shape) for b in boxes]


def test_no_rois_give_empty_results_and_a_zero_d_input():
    case = P.make_case("c6-7x7")
    empty = dict(case, rois=case["rois"][:0], grad=case["grad"][:0])
    out, dx, drois = run(empty)
    assert out.shape == (0, 6, 7, 7) and drois.shape == (0, 5)
    assert dx.shape == case["input"].shape and not bool(dx.any())
    for shape in ((0, 6, 9, 11), (1, 0, 9, 11), (1, 6, 0, 11)):           # N == 0, C == 0, an empty map: no launch
        x = torch.zeros(shape, device=DEV, requires_grad=True)
        rois = case["rois"].to(DEV).requires_grad_(True)
        out = ops.prroi_pool(x, rois, 2)
        assert out.shape == (rois.shape[0], shape[1], 2, 2) and not bool(out.any())
        out.sum().backward()
        assert x.grad.shape == x.shape and not bool(rois.grad.any())
    # the C entry point: OK after zero-filling a NaN-prefilled d_dx
    buf = torch.full((1, 5, 4, 8), float("nan"), device=DEV)
    rc = nv.lib().frcnn_ops_prroi_pool_backward(None, None, 0, 1, 5, 4, 8, 3, 5, 1.0, None, buf.data_ptr(), None, None, 0,
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(buf.any())


def test_the_module_equals_the_function():
    case = P.make_case("borders")
    x, rois = case["input"].to(DEV), case["rois"].to(DEV)
    want = ops.prroi_pool(x, rois, case["output_size"], case["spatial_scale"])
    assert float(want.abs().max()) > 0.1
    assert torch.equal(ops.PrRoIPool(case["output_size"], case["spatial_scale"])(x, rois), want)


def test_c_abi_overwrites_nan_prefilled_buffers():
    """The entry points called directly on NaN-prefilled output and gradient buffers: every element is written."""
    case = P.make_case("c6-7x7")
    lib = nv.lib()
    n, c, h, w = case["input"].shape
    cp = 8
    oh, ow = case["output_size"]
    k = case["rois"].shape[0]
    x = torch.zeros((n, h, w, cp), device=DEV)
    x[..., :c] = case["input"].to(DEV).permute(0, 2, 3, 1)
    g = torch.zeros((k, oh, ow, cp), device=DEV)
    g[..., :c] = case["grad"].to(DEV).permute(0, 2, 3, 1)
    rois = case["rois"].to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)              # noqa: E731
    out, dx, drois = nan(k, oh, ow, cp), nan(n, h, w, cp), nan(k, 5)
    ws = torch.empty((lib.frcnn_ops_prroi_pool_workspace_bytes(k, oh, ow),), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    scale = case["spatial_scale"]
    assert lib.frcnn_ops_prroi_pool(x.data_ptr(), n, h, w, cp, rois.data_ptr(), k, oh, ow, scale, out.data_ptr(), stream) == 0
    assert lib.frcnn_ops_prroi_pool_backward(x.data_ptr(), rois.data_ptr(), k, n, h, w, cp, oh, ow, scale, g.data_ptr(), dx.data_ptr(),
                                             drois.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    torch.cuda.synchronize()
    want = run(case)
    assert torch.equal(out[..., :c].permute(0, 3, 1, 2), want[0]) and not bool(out[..., c:].any())
    assert torch.equal(dx[..., :c].permute(0, 3, 1, 2), want[1]) and not bool(dx[..., c:].any())
    assert torch.equal(drois, want[2])


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes_on_both_ops():
    case = P.make_case("6x7-integer-edges")
    x, rois, grad = (case[k].to(DEV) for k in ("input", "rois", "grad"))
    oh, ow = case["output_size"]
    tail = (case["spatial_scale"], oh, ow)
    torch.library.opcheck(torch.ops.frcnn.prroi_pool.default, (x.clone().requires_grad_(True), rois.clone().requires_grad_(True)) + tail,
                          test_utils=OPCHECK)
    for needs in ([True, True], [True, False], [False, True]):
        torch.library.opcheck(torch.ops.frcnn.prroi_pool_backward.default, (grad, x, rois) + tail + (needs, False), test_utils=OPCHECK)


def test_double_backward_raises():
    case = P.make_case("6x7-integer-edges")
    x = case["input"].to(DEV).requires_grad_(True)
    rois = case["rois"].to(DEV).requires_grad_(True)
    out = ops.prroi_pool(x, rois, case["output_size"], case["spatial_scale"])
    gx, gr = torch.autograd.grad(out, (x, rois), case["grad"].to(DEV), create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        (gx.sum() + gr.sum()).backward()
