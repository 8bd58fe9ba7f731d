"""fasterrcnn_amd.ops.rotated_feature_align and RotatedFeatureAlign on the GPU against the float64 restatement (tests/rfa_cases.py) and on
the properties the kernels promise: channel counts with pad runs and past the 256-channel chunk, the range rule, bad box rows, points = 1
never reading components 2..4, exact dyadic results, a cell's segment past MSDA_SEGMENT entries, the 16-bit contract, layouts and
non-contiguous boxes, the C entry points.

The bound of every comparison with the float64 truth is measured in the same test: err(a) = max|a - truth| / max|truth|, err_ref is the
error of the float32 mirror of the restatement on the CPU, and err_gpu <= 4 * max(err_ref, 2**-24) must hold, with max|truth| > 0.1 and
no element masked (rfa_cases.check_conditions keeps the generic cases' samples 1e-3 away from every integer coordinate).

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: output 1.000, d_features 1.000;
rotated_feature_align_pytorch on the GPU under the same rule: 1.007."""
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import rfa_cases as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
HALF = [torch.float16, torch.bfloat16]


def run(case, dtype=F32, x_cl=False, grad_cl=False, boxes=None, fn=None, backward=True):
    """The operator on the GPU, forward and backward: (output, d_features or None)."""
    x = case["input"].to(DEV).to(dtype)
    x = (x.contiguous(memory_format=CL) if x_cl else x.contiguous()).clone().requires_grad_(backward)
    if boxes is None:
        boxes = case["boxes"].to(DEV)
    out = (ops.rotated_feature_align if fn is None else fn)(x, boxes, case["spatial_scale"], case["points"])
    if backward:
        grad = case["grad"].to(DEV).to(dtype)
        out.backward(grad.contiguous(memory_format=CL) if grad_cl else grad.contiguous())
    return out.detach(), x.grad


def check_against_truth(label, got, truth, mirror):
    ratios = {}
    for name, g, t, m in zip(("output", "d_features"), got, truth[:2], mirror[:2]):
        assert g.shape == t.shape and g.dtype == F32, name
        assert float(t.abs().max()) > 0.1, (label, name)
        err_gpu, err_ref = A.rel_err(g.cpu(), t), A.rel_err(m, t)
        ratios[name] = err_gpu / max(err_ref, FLOOR)
        print("%s %-10s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, ratios[name]))
        assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, name, err_gpu, err_ref)
    return ratios


# ---- 1. against the float64 restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.TOLERANCE_CASES)
def test_forward_and_gradient_against_float64(name):
    case, truth, mirror = A.make_case(name)
    A.check_conditions(case, truth)
    out, dx = run(case)
    assert out.is_contiguous() and dx.is_contiguous()
    check_against_truth(name, (out, dx), truth, mirror)


@pytest.mark.parametrize("name", ["c1-p5-eighth", "c4-p5", "c12-p1", "c260-p5"])
def test_the_torch_composition_on_the_gpu_agrees_with_the_kernel(name):
    """rotated_feature_align_pytorch on the GPU is held to the rule the kernel is held to, so the two agree to within that."""
    case, truth, mirror = A.make_case(name)
    check_against_truth(name + " (composition)", run(case, fn=ops.rotated_feature_align_pytorch), truth, mirror)


# ---- 2. the range rule, bad rows, known answers ---------------------------------------------------------------------------------------------
def test_centres_on_the_range_count_and_centres_beyond_it_do_not():
    case, counted, total = A.range_case()
    want = A.reference(case, F64)
    out, dx = run(case)
    added = (out.cpu().double() - case["input"].double()).flatten(2)[0]   # what the samples added, per pixel of image 0
    assert bool(added[:, :counted].abs().amax(0).gt(0).all()) and not bool(added[:, counted:total].any())
    check_against_truth("range", (out, dx), want, A.reference(case, F32))
    # a pixel whose sample counts nothing keeps its value, and its gradient goes to itself alone
    h, w = case["input"].shape[2:]
    for i in range(counted, total):
        assert torch.equal(out[0, :, i // w, i % w].cpu(), case["input"][0, :, i // w, i % w])


@pytest.mark.parametrize("points", [1, 5])
def test_nan_and_infinite_rows_add_nothing_and_leave_the_rest_unchanged(points):
    case, rows = A.bad_rows_case(points)
    want = A.reference(case, F64)
    for dtype in [F32] + HALF:
        out, dx = run(case, dtype=dtype)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
    out, dx = run(case)
    check_against_truth("bad rows, points %d" % points, (out, dx), want, A.reference(case, F32))
    w = case["input"].shape[3]
    for i in range(3):                                                    # a NaN row, an infinite row, a row at -inf: the pixel's own value
        assert torch.equal(out[0, :, i // w, i % w].cpu(), case["input"][0, :, i // w, i % w])


def test_points_1_never_reads_components_2_to_4():
    case = dict(A.make_case("c4-p1-eighth")[0])
    out, dx = run(case)
    boxes = case["boxes"].clone()
    boxes[..., 2:] = A.NAN
    boxes[0, 0, 0, 2:] = A.INF
    out_n, dx_n = run(dict(case, boxes=boxes))
    assert float(out.abs().max()) > 0.1 and torch.equal(out, out_n) and torch.equal(dx, dx_n)


def test_the_dyadic_case_is_exact():
    case = A.dyadic_case()
    want = A.reference(case, F64)
    assert float(want[0].abs().max()) > 0.1 and float(want[1].abs().max()) > 0.1
    for x_cl in (False, True):
        out, dx = run(case, x_cl=x_cl)
        assert torch.equal(out.cpu().double(), want[0]) and torch.equal(dx.cpu().double(), want[1])      # ratio 0
    for dtype in HALF:                                                    # small integers and dyadic weights: exact in 16 bits too
        out, dx = run(case, dtype=dtype)
        assert torch.equal(out, want[0].to(DEV).to(dtype)) and torch.equal(dx, want[1].to(DEV).to(dtype))


def test_a_segment_past_msda_segment_entries():
    """576 entries on each of four cells: both runs give the same bits, and the sum is the restatement's."""
    case = A.long_segment_case()
    assert case["input"].shape[2] * case["input"].shape[3] > ops.MSDA_SEGMENT == nv.lib().frcnn_ops_msda_segment()
    first, second = run(case), run(case)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    truth, mirror = A.reference(case, F64), A.reference(case, F32)
    check_against_truth("long", first, truth, mirror)
    assert torch.equal(first[1].cpu(), mirror[1])                         # ascending entry order after the identity term, as the mirror sums
    cells = torch.zeros((A.LONG_SIDE, A.LONG_SIDE), dtype=torch.bool)
    cells[11:13, 11:13] = True
    assert torch.equal(first[1][0][:, ~cells].cpu(), case["grad"][0][:, ~cells])     # every other cell keeps dout alone


# ---- 3. the 16-bit contract, determinism, layouts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["c1-p1", "c4-p5", "c12-p5-eighth", "c260-p5", "c260-p1-eighth"])
def test_16_bit_maps_equal_the_float32_operator_rounded_once(name, dtype):
    case = dict(A.make_case(name)[0])
    case["input"] = case["input"].to(dtype).float()                      # the 16-bit values, exactly
    case["grad"] = case["grad"].to(dtype).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=dtype)
    assert out16.dtype == dtype and dx16.dtype == dtype
    assert float(out32.abs().max()) > 0.1 and float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(dtype)) and torch.equal(dx16, dx32.to(dtype))
    boxes16 = case["boxes"].to(dtype)                                    # boxes in the map's dtype are widened for the kernels
    out_b, dx_b = run(case, dtype=dtype, boxes=boxes16.to(DEV))
    out_w, dx_w = run(dict(case, boxes=boxes16.float()))
    assert torch.equal(out_b, out_w.to(dtype)) and torch.equal(dx_b, dx_w.to(dtype))


def test_16_bit_backward_in_wide_runs():
    """C = 512: the gather walks runs of 8 channels (below that, of 4)."""
    gen = torch.Generator().manual_seed(51)
    case = dict(A.make_case("c4-p5")[0])
    case["input"] = torch.randn((2, 512, 6, 7), generator=gen).to(torch.bfloat16).float()
    case["grad"] = torch.randn((2, 512, 6, 7), generator=gen).to(torch.bfloat16).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=torch.bfloat16)
    assert float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(torch.bfloat16)) and torch.equal(dx16, dx32.to(torch.bfloat16))


@pytest.mark.parametrize("name", ["c4-p5", "c260-p5", "c12-p1"])
def test_two_runs_are_bit_identical(name):
    case = A.make_case(name)[0]
    first, second = run(case), run(case)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert float(first[1].abs().max()) > 0.1


@pytest.mark.parametrize("name", ["c1-p5-eighth", "c12-p5-eighth", "c260-p5"])
def test_layouts_and_non_contiguous_boxes_give_the_same_bits(name):
    case = A.make_case(name)[0]
    for dtype in [F32] + HALF:
        out, dx = run(case, dtype=dtype)
        assert out.is_contiguous() and dx.is_contiguous()
        out_cl, dx_cl = run(case, dtype=dtype, x_cl=True, grad_cl=True)
        c = case["input"].shape[1]
        assert c == 1 or (out_cl.is_contiguous(memory_format=CL) and dx_cl.is_contiguous(memory_format=CL))
        assert torch.equal(out, out_cl) and torch.equal(dx, dx_cl)
    out, dx = run(case)
    n, h, w, _ = case["boxes"].shape
    wide = torch.zeros((n, h, w, 2, 8), device=DEV)
    wide[:, :, :, 1, 2:7] = case["boxes"].to(DEV)
    strided = wide[:, :, :, 1, 2:7]
    assert not strided.is_contiguous()
    out_s, dx_s = run(case, boxes=strided)
    assert torch.equal(out, out_s) and torch.equal(dx, dx_s)
    transposed = case["boxes"].to(DEV).permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
    assert not transposed.is_contiguous() and torch.equal(run(case, boxes=transposed)[0], out)


# ---- 4. other behaviour -------------------------------------------------------------------------------------------------------------------
def test_best_bboxes_get_no_gradient_and_the_module_equals_the_function():
    case = A.make_case("c4-p5")[0]
    boxes = case["boxes"].to(DEV).requires_grad_(True)
    x = case["input"].to(DEV).requires_grad_(True)
    out = ops.rotated_feature_align(x, boxes, case["spatial_scale"], case["points"])
    out.backward(case["grad"].to(DEV))
    assert boxes.grad is None and x.grad is not None
    m = ops.RotatedFeatureAlign(case["spatial_scale"], case["points"])
    out = out.detach()
    assert float(out.abs().max()) > 0.1 and torch.equal(m(case["input"].to(DEV), case["boxes"].to(DEV)), out)


def test_empty_inputs_give_empty_results():
    for shape in ((0, 4, 6, 7), (2, 0, 6, 7)):                             # N == 0, C == 0: no launch
        x = torch.zeros(shape, device=DEV, requires_grad=True)
        out = ops.rotated_feature_align(x, torch.zeros((shape[0], 6, 7, 5), device=DEV), 1.0, 5)
        assert out.shape == shape
        out.sum().backward()
        assert x.grad.shape == x.shape
    assert ops.rotated_feature_align_pytorch(torch.zeros((0, 4, 6, 7), device=DEV), torch.zeros((0, 6, 7, 5), device=DEV)).shape == (0, 4, 6, 7)


def test_c_abi_overwrites_nan_prefilled_buffers():
    """The entry points called directly on NaN-prefilled output, plan and gradient buffers: every element is written."""
    case = A.make_case("c1-p5-eighth")[0]
    lib = nv.lib()
    n, c, h, w = case["input"].shape
    cp, points, scale = 4, case["points"], case["spatial_scale"]
    x = torch.zeros((n, h, w, cp), device=DEV)
    x[..., :c] = case["input"].to(DEV).permute(0, 2, 3, 1)
    g = torch.zeros((n, h, w, cp), device=DEV)
    g[..., :c] = case["grad"].to(DEV).permute(0, 2, 3, 1)
    boxes = case["boxes"].to(DEV).contiguous()
    out, dx = torch.full((n, h, w, cp), float("nan"), device=DEV), torch.full((n, h, w, cp), float("nan"), device=DEV)
    entries = n * h * w * points * 4
    keys = torch.full((entries,), -7, dtype=torch.int64, device=DEV)
    wts = torch.full((entries,), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.frcnn_ops_rotated_feature_align(x.data_ptr(), boxes.data_ptr(), n, h, w, cp, scale, points, out.data_ptr(), stream) == 0
    assert lib.frcnn_ops_rotated_feature_align_plan(boxes.data_ptr(), n, h, w, scale, points, keys.data_ptr(), wts.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert bool(((keys >= 0) & (keys <= n * h * w)).all()) and bool(torch.isfinite(wts).all())
    assert bool((keys == n * h * w).any()) and not bool(wts[keys == n * h * w].any())          # the sentinel carries weight 0
    skeys, order = torch.sort(keys, stable=True)
    assert lib.frcnn_ops_rotated_feature_align_backward(skeys.data_ptr(), order.data_ptr(), wts.data_ptr(), g.data_ptr(), n, h, w, cp, points,
                                                        dx.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    want = run(case)
    assert torch.equal(out[..., :c].permute(0, 3, 1, 2), want[0]) and not bool(out[..., c:].any())
    assert torch.equal(dx[..., :c].permute(0, 3, 1, 2), want[1]) and not bool(dx[..., c:].any())


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes_on_both_ops():
    case = A.make_case("c4-p5")[0]
    x, boxes, grad = (case[k].to(DEV) for k in ("input", "boxes", "grad"))
    tail = (case["spatial_scale"], case["points"])
    torch.library.opcheck(torch.ops.frcnn.rotated_feature_align.default, (x.clone().requires_grad_(True), boxes) + tail, test_utils=OPCHECK)
    for channels_last in (False, True):
        torch.library.opcheck(torch.ops.frcnn.rotated_feature_align_backward.default, (grad, boxes) + tail + (channels_last,),
                              test_utils=OPCHECK)


def test_double_backward_raises():
    case = A.make_case("c4-p5")[0]
    x = case["input"].to(DEV).requires_grad_(True)
    out = ops.rotated_feature_align(x, case["boxes"].to(DEV), case["spatial_scale"], case["points"])
    v = case["grad"].to(DEV).requires_grad_(True)                           # the backward is linear in v: a second-order graph exists
    gx, = torch.autograd.grad(out, x, v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()
