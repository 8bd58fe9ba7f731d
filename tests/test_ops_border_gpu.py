"""fasterrcnn_amd.ops.border_align and BorderAlign on the GPU against the float64 restatement (tests/border_align_cases.py) and on the
properties the kernels promise: the argmax, boxes on and beyond the sample range, degenerate and non-finite boxes, NaN pixels, the 16-bit
contract, determinism and the cull passes, layouts, the C entry points.

The bound of every comparison with the float64 truth is measured in the same test, as in tests/test_ops_prroi_gpu.py:
err(a) = max|a - truth| / max|truth|, err_ref is the error of the float32 mirror of the restatement on the CPU, and
err_gpu <= 4 * max(err_ref, 2**-24) must hold, with max|truth| > 0.1.  No element is masked: border_align_cases.check_conditions asserts
that no case has a runner-up within 1e-3 max|truth| of its best sample unless the two are exactly equal by construction, and the GPU's
argmax must equal the truth's exactly.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: output 1.000, d_input 1.000 (the
kernels' results equal the float32 mirror's in every case, to the printed digits; the dyadic cases' outputs are exact, ratio 0);
border_align_pytorch on the GPU under the same rule, on the cases it is held to: 1.000."""

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import border_align_cases as B

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
HALF = [torch.float16, torch.bfloat16]


def run(case, dtype=F32, x_cl=False, grad_cl=True, boxes=None, fn=None, backward=True):
    """The operator on the GPU, forward and backward: (output, d_input or None)."""
    x = case["input"].to(DEV).to(dtype)
    x = (x.contiguous(memory_format=CL) if x_cl else x.contiguous()).clone().requires_grad_(backward)
    if boxes is None:
        boxes = case["boxes"].to(DEV)
    out = (ops.border_align if fn is None else fn)(x, boxes, case["pool_size"])
    if backward:
        grad = case["grad"].to(DEV).to(dtype)
        out.backward(grad.contiguous(memory_format=CL) if grad_cl else grad.contiguous())
    return out.detach(), x.grad


def argmax_of(case, dtype=F32):
    x = case["input"].to(DEV).to(dtype)
    return torch.ops.frcnn.border_align(x, case["boxes"].to(DEV), case["pool_size"])[1]


def check_against_truth(label, got, truth, mirror):
    """err_gpu <= 4 * max(err_ref, 2**-24) for the output and d_input; prints both errors; returns the ratios."""
    ratios = {}
    for name, g, t, m in zip(("output", "d_input"), got, (truth[0], truth[2]), (mirror[0], mirror[2])):
        assert g.shape == t.shape and g.dtype == F32, name
        assert float(t.abs().max()) > 0.1, (label, name)
        err_gpu, err_ref = B.rel_err(g.cpu(), t), B.rel_err(m, t)
        ratios[name] = err_gpu / max(err_ref, FLOOR)
        print("%s %-8s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, ratios[name]))
        assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, name, err_gpu, err_ref)
    return ratios


# ---- 1. output, argmax and d_input against the float64 restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("name", B.TOLERANCE_CASES)
def test_forward_argmax_and_gradient_against_float64(name):
    case, truth, mirror = B.make_case(name)
    B.check_conditions(case, truth, mirror)
    out, dx = run(case)
    assert (out.is_contiguous(memory_format=CL) or out.shape[1] == 1) and dx.is_contiguous()
    arg = argmax_of(case)
    assert arg.dtype == torch.int32 and torch.equal(arg.cpu().long(), truth[1])
    check_against_truth(name, (out, dx), truth, mirror)


@pytest.mark.parametrize("name", ["c3-two-images-random", "edges", "c260-two-images", "c9-pool64"])
def test_the_torch_composition_on_the_gpu_agrees_with_the_kernel(name):
    """border_align_pytorch on the GPU is held to the rule the kernel is held to, so the two agree to within that."""
    case, truth, mirror = B.make_case(name)
    check_against_truth(name + " (composition)", run(case, fn=ops.border_align_pytorch), truth, mirror)


# ---- 2. known answers and special boxes ----------------------------------------------------------------------------------------------------
def test_a_constant_map_ties_everywhere_argmax_0():
    case, truth, _ = B.make_case("constant")
    out, _ = run(case)
    assert bool((out == 1.5).all()) and not bool(argmax_of(case).any())


def test_a_single_maximum_at_the_last_sample():
    case, truth, _ = B.make_case("last-maximum")
    out, dx = run(case)
    assert out[0, 0, 0].tolist() == [2.0, 0.0, 0.0, 2.0] and argmax_of(case)[0, 0, 0].tolist() == [10, 0, 0, 10]
    assert torch.equal(dx.cpu().double(), truth[2])                          # every weight is 0, 0.5 or 1: exact


def test_zero_stride_edges_send_their_whole_gradient_to_sample_0():
    case, truth, _ = B.make_case("degenerate")
    arg = argmax_of(case)
    for row, edges in B.ZERO_STRIDE["degenerate"].items():
        for e in edges:
            assert not bool(arg[0, :, row, e].any())
    alone = dict(case, boxes=case["boxes"][:, 4:5], grad=case["grad"][:, :, 4:5].contiguous())     # the zero-area box
    _, dx = run(alone)
    x, y = float(case["boxes"][0, 4, 0]), float(case["boxes"][0, 4, 1])
    cells = torch.zeros_like(dx, dtype=torch.bool)
    cells[:, :, int(y):int(y) + 2, int(x):int(x) + 2] = True
    assert not bool(dx[~cells].any()) and abs(float(dx.double().sum()) - float(alone["grad"].double().sum())) < 1e-5


def test_non_finite_boxes_give_zeros_beside_an_unchanged_normal_box():
    case = B.nonfinite_case()
    alone = dict(case, boxes=case["boxes"][:, :1].contiguous(), grad=case["grad"][:, :, :1].contiguous())
    for dtype in [F32] + HALF:
        out, dx = run(case, dtype=dtype)
        out_a, dx_a = run(alone, dtype=dtype)
        assert float(out_a.abs().max()) > 0.1 and float(dx_a.abs().max()) > 0.1
        assert torch.equal(out[:, :, :1], out_a) and torch.equal(dx, dx_a)
        assert not bool(out[:, :, 1:].any()) and not bool(argmax_of(case, dtype)[:, :, 1:].any())
    want = B.reference(case, F64)
    assert torch.equal(argmax_of(case).cpu().long(), want[1])


def test_a_nan_pixel_stays_at_sample_0_and_never_wins_later():
    case = B.nan_pixel_case()
    want_out, want_arg, want_dx, _ = B.reference(case, F64)
    out, dx = run(case)
    assert torch.equal(argmax_of(case).cpu().long(), want_arg)
    assert torch.equal(torch.isnan(out).cpu(), torch.isnan(want_out)) and bool(torch.isnan(out[0, :, 0, :2]).all())
    assert not bool(torch.isnan(out[0, :, 1:]).any())
    assert torch.allclose(out.cpu().double(), want_out, rtol=1e-6, atol=1e-6, equal_nan=True)
    assert torch.allclose(dx.cpu().double(), want_dx, rtol=1e-6, atol=1e-6, equal_nan=True)


# ---- 3. the 16-bit contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["c3-two-images-random", "c260-two-images", "Hx1-c5", "c9-pool64", "edges"])
def test_16_bit_maps_equal_the_float32_operator_rounded_once(name, dtype):
    case = dict(B.make_case(name)[0])
    case["input"] = case["input"].to(dtype).float()                      # the 16-bit values, exactly
    case["grad"] = case["grad"].to(dtype).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=dtype)
    assert out16.dtype == dtype and dx16.dtype == dtype
    assert float(out32.abs().max()) > 0.1 and float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(dtype)) and torch.equal(dx16, dx32.to(dtype))
    assert torch.equal(argmax_of(case, dtype), argmax_of(case))
    # boxes in the map's dtype are widened for the kernels
    boxes16 = case["boxes"].to(dtype)
    wide = dict(case, boxes=boxes16.float())
    out_b, dx_b = run(case, dtype=dtype, boxes=boxes16.to(DEV))
    out_w, dx_w = run(wide)
    assert torch.equal(out_b, out_w.to(dtype)) and torch.equal(dx_b, dx_w.to(dtype))


# ---- 4. determinism and the cull passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cull", "c260-two-images", "c3-two-images-random"])
def test_two_runs_are_bit_identical(name):
    case = B.make_case(name)[0]
    first, second = run(case), run(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert float(first[1].abs().max()) > 0.1


def test_the_gather_needs_its_second_cull_pass_and_keeps_ascending_order():
    """16 BORDER_ALIGN_CULL_LIST + 1 boxes on one 3 x 3 map, every one with all four edges across both tile columns and within a cell of
    both tile rows, so every tile's waves take every box of sixteen full groups and one box of a seventeenth.  d_input must be the sum
    over the first sixteen groups with the last box's term added after it, bit for bit; and the sum over the first group with the
    second group's sum added box by box."""
    case = dict(B.make_case("cull")[0])
    k = case["boxes"].shape[1]
    assert k == B.CULL_BOXES == 16 * ops.BORDER_ALIGN_CULL_LIST + 1 and ops.BORDER_ALIGN_CULL_LIST == nv.lib().frcnn_ops_border_align_cull_list()
    case["boxes"] = case["boxes"].clone()
    case["boxes"][0, :-1] = torch.tensor([0.25, 0.5, 1.75, 1.5])             # every edge of every listed box crosses all four tiles
    case["boxes"][0, -1] = torch.tensor([0.5, 0.25, 1.5, 1.75])
    _, dx = run(case)
    part = lambda a, b: run(dict(case, boxes=case["boxes"][:, a:b].contiguous(), grad=case["grad"][:, :, a:b].contiguous()))[1]   # noqa: E731
    want, term = part(0, k - 1), part(k - 1, k)
    assert float(want.abs().max()) > 0.1 and bool(term.any())
    assert int((term != 0).sum()) >= 8                                       # the last box reaches cells of several tiles
    assert torch.equal(dx, want + term)
    group = ops.BORDER_ALIGN_CULL_LIST
    want = part(0, group)
    for r in range(group, group + 3):                                        # the second group's first boxes, one by one
        want = want + part(r, r + 1)
    assert torch.equal(part(0, group + 3), want)


# ---- 5. other behaviour -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3-two-images-random", "c260-two-images"])
def test_layouts_give_the_same_bits_and_d_input_keeps_its_format(name):
    case = B.make_case(name)[0]
    for dtype in [F32] + HALF:
        out, dx = run(case, dtype=dtype)
        assert dx.is_contiguous()
        out_cl, dx_cl = run(case, dtype=dtype, x_cl=True, grad_cl=False)
        assert dx_cl.is_contiguous(memory_format=CL) and out_cl.is_contiguous(memory_format=CL)
        assert torch.equal(out, out_cl) and torch.equal(dx, dx_cl)


def test_non_contiguous_boxes_give_the_same_bits():
    case = B.make_case("c3-two-images-random")[0]
    out, dx = run(case)
    n, k, _ = case["boxes"].shape
    wide = torch.zeros((n, k, 2, 8), device=DEV)
    wide[:, :, 1, 2:6] = case["boxes"].to(DEV)
    strided = wide[:, :, 1, 2:6]
    assert not strided.is_contiguous()
    out_s, dx_s = run(case, boxes=strided)
    assert torch.equal(out, out_s) and torch.equal(dx, dx_s)
    transposed = case["boxes"].to(DEV).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not transposed.is_contiguous()
    assert torch.equal(run(case, boxes=transposed)[0], out)


def test_boxes_get_no_gradient():
    case = B.make_case("c3-two-images-random")[0]
    boxes = case["boxes"].to(DEV).requires_grad_(True)
    x = case["input"].to(DEV).requires_grad_(True)
    ops.border_align(x, boxes, case["pool_size"]).backward(case["grad"].to(DEV))
    assert boxes.grad is None and x.grad is not None


def test_the_module_equals_the_function():
    case = B.make_case("c3-two-images-random")[0]
    x, boxes = case["input"].to(DEV), case["boxes"].to(DEV)
    want = ops.border_align(x, boxes, case["pool_size"])
    assert float(want.abs().max()) > 0.1
    assert torch.equal(ops.BorderAlign(case["pool_size"])(x, boxes), want)


def test_empty_inputs_give_empty_results_and_a_zero_d_input():
    case = B.make_case("c3-two-images-random")[0]
    n, c4, h, w = case["input"].shape
    empty = dict(case, boxes=case["boxes"][:, :0], grad=case["grad"][:, :, :0])
    out, dx = run(empty)
    assert out.shape == (n, c4 // 4, 0, 4) and dx.shape == case["input"].shape and not bool(dx.any())
    for shape in ((0, 12, 5, 6), (2, 0, 5, 6)):                            # N == 0, C == 0: no launch
        x = torch.zeros(shape, device=DEV, requires_grad=True)
        out = ops.border_align(x, torch.zeros((shape[0], 3, 4), device=DEV), 10)
        assert out.shape == (shape[0], shape[1] // 4, 3, 4)
        out.sum().backward()
        assert x.grad.shape == x.shape and not bool(x.grad.any())
    # the C entry point: OK after zero-filling a NaN-prefilled d_dx
    buf = torch.full((1, 4, 8, 16), float("nan"), device=DEV)
    rc = nv.lib().frcnn_ops_border_align_backward(None, 0, 1, 4, 8, 4, 10, None, None, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(buf.any())


def test_c_abi_overwrites_nan_prefilled_buffers():
    """The entry points called directly on NaN-prefilled output, argmax and gradient buffers: every element is written."""
    case = B.make_case("c3-two-images-random")[0]
    lib = nv.lib()
    n, c4, h, w = case["input"].shape
    c, cp, k, pool = c4 // 4, 4, case["boxes"].shape[1], case["pool_size"]
    x = torch.zeros((n, h, w, 4, cp), device=DEV)
    x[..., :c] = case["input"].to(DEV).unflatten(1, (4, c)).permute(0, 3, 4, 1, 2)
    g = torch.zeros((n, k, 4, cp), device=DEV)
    g[..., :c] = case["grad"].to(DEV).permute(0, 2, 3, 1)
    boxes = case["boxes"].to(DEV).contiguous()
    out = torch.full((n, k, 4, cp), float("nan"), device=DEV)
    argmax = torch.full((n, k, 4, cp), -7, dtype=torch.int32, device=DEV)
    dx = torch.full((n, h, w, 4, cp), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.frcnn_ops_border_align(x.data_ptr(), n, h, w, cp, boxes.data_ptr(), k, pool, out.data_ptr(), argmax.data_ptr(), stream) == 0
    assert lib.frcnn_ops_border_align_backward(boxes.data_ptr(), k, n, h, w, cp, pool, argmax.data_ptr(), g.data_ptr(), dx.data_ptr(),
                                               stream) == 0
    torch.cuda.synchronize()
    want_out, want_dx = run(case)
    assert torch.equal(out[..., :c].permute(0, 3, 1, 2), want_out) and not bool(out[..., c:].any())
    assert torch.equal(argmax[..., :c].permute(0, 3, 1, 2), argmax_of(case)) and bool((argmax >= 0).all())
    assert torch.equal(dx[..., :c].permute(0, 3, 4, 1, 2).flatten(1, 2), want_dx) and not bool(dx[..., c:].any())


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes_on_both_ops():
    case = B.make_case("c3-two-images-random")[0]
    x, boxes, grad = (case[k].to(DEV) for k in ("input", "boxes", "grad"))
    pool = case["pool_size"]
    torch.library.opcheck(torch.ops.frcnn.border_align.default, (x.clone().requires_grad_(True), boxes, pool), test_utils=OPCHECK)
    argmax = torch.ops.frcnn.border_align(x, boxes, pool)[1]
    for channels_last in (False, True):
        torch.library.opcheck(torch.ops.frcnn.border_align_backward.default, (grad, boxes, argmax, pool, x.shape[2], x.shape[3], channels_last),
                              test_utils=OPCHECK)


def test_double_backward_raises():
    case = B.make_case("c3-two-images-random")[0]
    x = case["input"].to(DEV).requires_grad_(True)
    out = ops.border_align(x, case["boxes"].to(DEV), case["pool_size"])
    v = case["grad"].to(DEV).requires_grad_(True)                        # the backward op's only differentiable argument
    gx, = torch.autograd.grad(out, (x,), v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()
