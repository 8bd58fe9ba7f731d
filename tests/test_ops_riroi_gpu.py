"""fasterrcnn_amd.ops.riroi_align_rotated and RiRoIAlignRotated on the GPU against the float64 restatement (tests/riroi_cases.py) and on the
properties the kernels promise: pool-then-blend bit for bit with roi_align_rotated, the index wrap, group sizes that straddle runs and
the 64-run boundary, skipped RoIs, the backward's bits, the second cull pass, the 16-bit contract, determinism, layouts, the C entry
points.

The bound of every comparison with the float64 truth is measured in the same test: err(a) = max|a - truth| / max|truth|, err_ref is the
error of the float32 mirror of the restatement on the CPU, and err_gpu <= 4 * max(err_ref, 2**-24) must hold, with max|truth| > 0.1 and
no element masked (riroi_cases.check_conditions keeps the cases away from the contract's jumps).

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: output 1.284, d_input 1.000 (the
d_input of every case equals the float32 mirror's to the printed digits)."""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import riroi_cases as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
HALF = [torch.float16, torch.bfloat16]


def args_of(case):
    return case["output_size"], case["spatial_scale"], case["num_samples"], case["num_orientations"], case["clockwise"]


def run(case, dtype=F32, x_cl=False, grad_cl=True, backward=True):
    """The operator on the GPU, forward and backward: (output, d_input or None)."""
    x = case["input"].to(DEV).to(dtype)
    x = (x.contiguous(memory_format=CL) if x_cl else x.contiguous()).clone().requires_grad_(backward)
    out = ops.riroi_align_rotated(x, case["rois"].to(DEV), *args_of(case))
    if backward:
        grad = case["grad"].to(DEV).to(dtype)
        out.backward(grad.contiguous(memory_format=CL) if grad_cl else grad.contiguous())
    return out.detach(), x.grad


def pooled(case, x=None, grad=None):
    """ops.roi_align_rotated under the contract's flags on the float32 map: (S, d_input for `grad` or None)."""
    x = (case["input"] if x is None else x).to(DEV).float().clone().requires_grad_(grad is not None)
    s = ops.roi_align_rotated(x, case["rois"].to(DEV), case["output_size"], case["spatial_scale"], case["num_samples"], aligned=False,
                              clockwise=not case["clockwise"])
    if grad is not None:
        s.backward(grad.to(DEV))
    return s.detach(), x.grad


def two_step(case, x=None):
    return ops.riroi_align_rotated_pytorch(pooled(case, x)[0], case["rois"].to(DEV), case["num_orientations"])


def check_against_truth(label, got, truth, mirror):
    ratios = {}
    for name, g, t, m in zip(("output", "d_input"), got, truth[:2], mirror[:2]):
        assert g.shape == t.shape and g.dtype == F32, name
        assert float(t.abs().max()) > 0.1, (label, name)
        err_gpu, err_ref = R.rel_err(g.cpu(), t), R.rel_err(m, t)
        ratios[name] = err_gpu / max(err_ref, FLOOR)
        print("%s %-8s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, ratios[name]))
        assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, name, err_gpu, err_ref)
    return ratios


# ---- 1. against the float64 restatement; pool-then-blend --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.TOLERANCE_CASES)
def test_forward_and_gradient_against_float64(name):
    case, truth, mirror = R.make_case(name)
    R.check_conditions(case, truth)
    out, dx = run(case)
    assert out.is_contiguous(memory_format=CL) and dx.is_contiguous()
    check_against_truth(name, (out, dx), truth, mirror)


@pytest.mark.parametrize("name", R.TOLERANCE_CASES)
def test_the_operator_is_the_blend_of_roi_align_rotated_bit_for_bit(name):
    case = R.make_case(name)[0]
    out, dx = run(case)
    assert float(out.abs().max()) > 0.1 and torch.equal(out, two_step(case))
    # the backward: roi_align_rotated's own backward of the float32 blend of the gradient, formed in numpy
    want = pooled(case, grad=R.blended_grad(case))[1]
    assert float(want.abs().max()) > 0.1 and torch.equal(dx, want)


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["n8-c2", "n8-c2-adaptive-clockwise", "n1-c5", "n3-c3", "n4-c4", "n3-c86", "n64-c1", "n6-c11"])
def test_16_bit_maps_equal_the_float32_operator_rounded_once(name, dtype):
    case = dict(R.make_case(name)[0])
    case["input"] = case["input"].to(dtype).float()                      # the 16-bit values, exactly
    case["grad"] = case["grad"].to(dtype).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=dtype)
    assert out16.dtype == dtype and dx16.dtype == dtype
    assert float(out32.abs().max()) > 0.1 and float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(dtype)) and torch.equal(dx16, dx32.to(dtype))
    # S stays float32 until after the blend: the blend of the float32 pooling, rounded once
    assert torch.equal(out16, two_step(case).to(dtype))
    rois16 = case["rois"].to(dtype)                                      # RoIs in the map's dtype are widened for the kernels
    got = ops.riroi_align_rotated(case["input"].to(DEV).to(dtype), rois16.to(DEV), *args_of(case))
    assert torch.equal(got, run(dict(case, rois=rois16.float()), backward=False)[0].to(dtype))


def test_16_bit_backward_in_wide_runs():
    """C n = 512: the backward walks runs of 8 channels (below that, of 4)."""
    gen = torch.Generator().manual_seed(41)
    case = dict(R.make_case("n8-c2")[0])
    case["input"] = torch.randn((2, 512, 12, 10), generator=gen).to(torch.bfloat16).float()
    case["grad"] = torch.randn((6, 512, 3, 2), generator=gen).to(torch.bfloat16).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=torch.bfloat16)
    assert float(dx32.abs().max()) > 0.1 and torch.equal(out32, two_step(case))
    assert torch.equal(out16, out32.to(torch.bfloat16)) and torch.equal(dx16, dx32.to(torch.bfloat16))


# ---- 2. the blend's seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n8-c2", "n8-c2-adaptive-clockwise", "n3-c3", "n1-c5"])
def test_at_angle_zero_the_operator_is_roi_align_rotated_itself(name):
    case = dict(R.make_case(name)[0])
    case = R.with_angles(case, [0.0] * case["rois"].shape[0])
    out, dx = run(case)
    s, ds = pooled(case, grad=case["grad"])
    assert float(s.abs().max()) > 0.1 and torch.equal(out, s) and torch.equal(dx, ds)


@pytest.mark.parametrize("name", ["n8-c2", "n8-c2-clockwise", "n3-c3", "n64-c1"])
def test_the_index_wraps(name):
    case = R.with_angles(R.make_case(name)[0], R.WRAP_ANGLES)
    out, dx = run(case)
    assert torch.equal(out, two_step(case))
    assert torch.equal(dx, pooled(case, grad=R.blended_grad(case))[1])
    if case["num_orientations"] == 8:
        assert R.blend(R.WRAP_ANGLES[0], 8)[2] == 7                       # ind = -1
        s = pooled(case)[0]
        left, right, k = (float(v) for v in R.blend(R.WRAP_ANGLES[0], 8))
        want = np.float32(right) * s[0, 1].cpu().numpy() + np.float32(left) * s[0, 2].cpu().numpy()     # o = 0: sources 0 - 7 = 1, 2 mod 8
        assert np.array_equal(out[0, 0].cpu().numpy(), want)


def test_a_nan_in_the_neighbouring_orientation_propagates_even_when_l_is_zero():
    case = R.with_angles(R.make_case("n8-c2")[0], [0.0] * 6)
    x = case["input"].clone()
    x[:, 1] = R.NAN                                                       # orientation 1 of group 0
    case = dict(case, input=x)
    out, _ = run(case, backward=False)
    assert torch.equal(torch.isnan(out), torch.isnan(two_step(case)))
    touched = torch.isnan(pooled(case)[0][:, 1])                          # where the pooling read the NaN channel
    assert bool(touched.any()) and bool(torch.isnan(out[:, 0])[touched].all()) and bool(torch.isnan(out[:, 1])[touched].all())
    assert not bool(torch.isnan(out[:, 2:]).any())


def test_skipped_rois_give_zero_rows_beside_an_unchanged_normal_roi():
    case = R.skipped_case()
    alone = dict(case, rois=case["rois"][:1].contiguous(), grad=case["grad"][:1].contiguous())
    for dtype in [F32] + HALF:
        out, dx = run(case, dtype=dtype)
        out_a, dx_a = run(alone, dtype=dtype)
        assert float(out_a.abs().max()) > 0.1 and float(dx_a.abs().max()) > 0.1
        assert torch.equal(out[:1], out_a) and not bool(out[1:].any()) and torch.equal(dx, dx_a)


# ---- 3. determinism, the cull passes, layouts -------------------------------------------------------------------------------------------
def cull_case():
    """ROI_ALIGN_ROTATED_CULL_LIST + 3 small RoIs around the centre of a 4 x 4 map, all of them on the middle tiles."""
    k = nv.lib().frcnn_ops_roi_align_rotated_cull_list() + 3
    gen = torch.Generator().manual_seed(42)
    u = lambda lo, hi: torch.rand((k,), generator=gen) * (hi - lo) + lo     # noqa: E731
    rois = torch.stack([torch.zeros(k), u(1.2, 1.8), u(1.2, 1.8), u(1.0, 1.5), u(1.0, 1.5), u(-3.0, 3.0)], 1)
    return {"name": "cull", "input": torch.randn((1, 8, 4, 4), generator=gen), "rois": rois, "output_size": (2, 2), "num_samples": 1,
            "clockwise": False, "spatial_scale": 1.0, "num_orientations": 4, "grad": torch.randn((k, 8, 2, 2), generator=gen)}


def test_the_gather_needs_its_second_cull_pass_and_keeps_ascending_order():
    case = cull_case()
    k = case["rois"].shape[0]
    assert k == ops.ROI_ALIGN_ROTATED_CULL_LIST + 3
    _, dx = run(case)
    assert torch.equal(dx, pooled(case, grad=R.blended_grad(case))[1])      # the same passes, the same order
    part = lambda a, b: run(dict(case, rois=case["rois"][a:b].contiguous(), grad=case["grad"][a:b].contiguous()))[1]   # noqa: E731
    first, rest = part(0, k - 3), part(k - 3, k)
    assert float(rest.abs().max()) > 1e-3 and not torch.equal(dx, first)
    # the last three RoIs' terms are added after the sum over the first CULL_LIST: at most 3 RoIs x 4 bins more roundings per cell
    want = first.double() + rest.double()
    assert float((dx.double() - want).abs().max()) <= 12 * 2.0 ** -23 * float(want.abs().max())
    tile = dx[0, :, 1:3, 1:3]
    assert float(tile.abs().min()) > 0                                     # every cell of the middle tile collects from every pass


@pytest.mark.parametrize("name", ["n8-c2", "n3-c86", "cull"])
def test_two_runs_are_bit_identical(name):
    case = cull_case() if name == "cull" else R.make_case(name)[0]
    first, second = run(case), run(case)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert float(first[1].abs().max()) > 0.1


@pytest.mark.parametrize("name", ["n8-c2", "n3-c3", "n3-c86"])
def test_layouts_give_the_same_bits_and_d_input_keeps_its_format(name):
    case = R.make_case(name)[0]
    for dtype in [F32] + HALF:
        out, dx = run(case, dtype=dtype)
        assert dx.is_contiguous()
        out_cl, dx_cl = run(case, dtype=dtype, x_cl=True, grad_cl=False)
        assert dx_cl.is_contiguous(memory_format=CL) and out_cl.is_contiguous(memory_format=CL)
        assert torch.equal(out, out_cl) and torch.equal(dx, dx_cl)


# ---- 4. other behaviour -------------------------------------------------------------------------------------------------------------------
def test_rois_get_no_gradient_and_the_module_equals_the_function():
    case = R.make_case("n8-c2")[0]
    rois = case["rois"].to(DEV).requires_grad_(True)
    x = case["input"].to(DEV).requires_grad_(True)
    out = ops.riroi_align_rotated(x, rois, *args_of(case))
    out.backward(case["grad"].to(DEV))
    assert rois.grad is None and x.grad is not None
    size, scale, ns, n, cw = args_of(case)
    m = ops.RiRoIAlignRotated(size, scale, num_samples=ns, num_orientations=n, clockwise=cw)
    out = out.detach()
    assert float(out.abs().max()) > 0.1 and torch.equal(m(case["input"].to(DEV), case["rois"].to(DEV)), out)


def test_no_rois_give_an_empty_result_and_a_zero_d_input():
    case = dict(R.make_case("n8-c2")[0])
    case["rois"], case["grad"] = case["rois"][:0], case["grad"][:0]
    out, dx = run(case)
    assert out.shape == (0, 16, 3, 2) and dx.shape == case["input"].shape and not bool(dx.any())
    buf = torch.full((1, 5, 4, 8), float("nan"), device=DEV)
    rc = nv.lib().frcnn_ops_riroi_align_rotated_backward(None, 0, 1, 5, 4, 8, 8, 2, 3, 1.0, 2, 4, 0, None, buf.data_ptr(),
                                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(buf.any())


@pytest.mark.parametrize("name", ["n3-c3", "n1-c5"])
def test_c_abi_overwrites_nan_prefilled_buffers(name):
    """The entry points called directly on NaN-prefilled buffers: every element is written, the pad channels of no group as zeros."""
    case = R.make_case(name)[0]
    lib = nv.lib()
    n, c, h, w = case["input"].shape
    cp = (c + 3) // 4 * 4
    assert cp > c
    oh, ow = case["output_size"]
    k = case["rois"].shape[0]
    x = torch.full((n, h, w, cp), 3.0, device=DEV)                        # the pad channels hold values: they belong to no group
    x[..., :c] = case["input"].to(DEV).permute(0, 2, 3, 1)
    g = torch.full((k, oh, ow, cp), 5.0, device=DEV)
    g[..., :c] = case["grad"].to(DEV).permute(0, 2, 3, 1)
    rois = case["rois"].to(DEV)
    out, dx = torch.full((k, oh, ow, cp), float("nan"), device=DEV), torch.full((n, h, w, cp), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    tail = (case["spatial_scale"], case["num_samples"], case["num_orientations"], int(case["clockwise"]))
    assert lib.frcnn_ops_riroi_align_rotated(x.data_ptr(), n, h, w, cp, c, rois.data_ptr(), k, oh, ow, *tail, out.data_ptr(), stream) == 0
    assert lib.frcnn_ops_riroi_align_rotated_backward(rois.data_ptr(), k, n, h, w, cp, c, oh, ow, *tail, g.data_ptr(), dx.data_ptr(),
                                                      stream) == 0
    torch.cuda.synchronize()
    want = run(case)
    assert torch.equal(out[..., :c].permute(0, 3, 1, 2), want[0]) and not bool(out[..., c:].any())
    assert torch.equal(dx[..., :c].permute(0, 3, 1, 2), want[1]) and not bool(dx[..., c:].any())


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes_on_both_ops():
    case = R.make_case("n3-c3")[0]
    x, rois, grad = (case[k].to(DEV) for k in ("input", "rois", "grad"))
    oh, ow = case["output_size"]
    tail = (case["spatial_scale"], oh, ow, case["num_samples"], case["num_orientations"], case["clockwise"])
    torch.library.opcheck(torch.ops.frcnn.riroi_align_rotated.default, (x.clone().requires_grad_(True), rois) + tail, test_utils=OPCHECK)
    for channels_last in (False, True):
        torch.library.opcheck(torch.ops.frcnn.riroi_align_rotated_backward.default, (grad, rois) + tail + tuple(x.shape) + (channels_last,),
                              test_utils=OPCHECK)


def test_double_backward_raises():
    case = R.make_case("n3-c3")[0]
    x = case["input"].to(DEV).requires_grad_(True)
    out = ops.riroi_align_rotated(x, case["rois"].to(DEV), *args_of(case))
    v = case["grad"].to(DEV).requires_grad_(True)                           # the backward is linear in v: a second-order graph exists
    gx, = torch.autograd.grad(out, x, v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()
