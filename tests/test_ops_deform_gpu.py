"""fasterrcnn_amd.ops.deform_conv2d / DeformConv2d on the GPU against the float64 restatement (tests/deform_conv_cases.py), against
torch's own convolution, and on the properties the kernels promise: determinism, independence of the chunking, layouts, flags.

The bound of every comparison with the float64 truth is measured in the same test: err(a) = max|a - truth| / max|truth|, err_ref is the
error of the same restatement run in float32 on the CPU, and err_gpu <= 4 * max(err_ref, 2**-24) must hold -- both sides are float32
sums of the same few hundred products, or fewer, taken in different orders with differently associated bilinear weights, while a wrong
tap, corner, group or layout gives errors five orders of magnitude larger.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: against the float64 restatement output 1.00,
d_input 1.43, d_offset 1.00, d_weight 1.25, d_bias 1.37, d_mask 1.06; against torch's conv2d output 1.15, d_input 1.75, d_weight 1.22;
d_weight of the chunked calls 1.09.  The largest of all, 1.75, is well inside the margin of 4."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fasterrcnn_amd import ops

from tests import deform_conv_cases as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F64 = torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
IDS = ["g%d" % i for i in range(len(D.GEOMETRIES))]
NAMES = ("output",) + tuple("d_" + k for k in D.ARGS)


def to_dev(t):
    return None if t is None else t.to(DEV)


def run(case, needs=D.ARGS, channels_last=(), backward=True, chunk=None):
    """The operator on the GPU: (output, {name: gradient})."""
    leaves = {}
    for k in D.ARGS:
        t = to_dev(case[k])
        if t is not None:
            if k in channels_last:
                t = t.contiguous(memory_format=CL)
            t.requires_grad_(k in needs)
        leaves[k] = t
    kw = case["kw"]
    if chunk is None:
        out = ops.deform_conv2d(leaves["input"], leaves["offset"], leaves["weight"], leaves["bias"], mask=leaves["mask"], **kw)
    else:
        out = torch.ops.frcnn.deform_conv2d(leaves["input"], leaves["offset"], leaves["weight"], leaves["bias"], leaves["mask"],
                                            *kw["stride"], *kw["padding"], *kw["dilation"], chunk)
    if not backward:
        return out, {}
    grad = to_dev(case["grad"])
    if "grad" in channels_last:
        grad = grad.contiguous(memory_format=CL)
    out.backward(grad)
    return out.detach(), {k: (None if t is None or t.grad is None else t.grad) for k, t in leaves.items()}


@functools.lru_cache(maxsize=None)
def reference(index, with_mask, with_bias):
    """The case of geometry `index` with its float64 truth and the float32 restatement's results, computed once."""
    case = D.make_case(D.GEOMETRIES[index], 100 + index, with_mask=with_mask, with_bias=with_bias)
    truth = (D.forward_ref(case, F64),) + tuple(D.grads_ref(case, F64))
    single = (D.forward_ref(case, torch.float32),) + tuple(D.grads_ref(case, torch.float32))
    return case, truth, single


def check_against_truth(label, got, truth, single):
    """err_gpu <= 4 * max(err_ref, 2**-24) for every quantity; prints both errors."""
    worst = 0.0
    for name, g, t, s in zip(NAMES, got, truth, single):
        assert (g is None) == (t is None), name
        if t is None:
            continue
        assert g.shape == t.shape and float(t.abs().max()) > 0.1, name
        err_gpu, err_ref = D.rel_err(g.cpu(), t), D.rel_err(s, t)
        bound = MARGIN * max(err_ref, FLOOR)
        print("%s %-9s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, err_gpu / max(err_ref, FLOOR)))
        worst = max(worst, err_gpu / max(err_ref, FLOOR))
        assert err_gpu <= bound, (label, name, err_gpu, err_ref)
    return worst


# ---- forward and all five gradients against the float64 restatement ------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("index", range(len(D.GEOMETRIES)), ids=IDS)
def test_forward_and_gradients_against_float64(index, with_mask, with_bias):
    case, truth, single = reference(index, with_mask, with_bias)
    assert 0.10 <= case["rejected"] <= 0.40 and 0.10 <= case["straddling"] <= 0.40, (case["rejected"], case["straddling"])
    out, grads = run(case)
    assert out.is_contiguous() and out.dtype == torch.float32
    check_against_truth("g%d mask=%d bias=%d" % (index, with_mask, with_bias), (out,) + tuple(grads[k] for k in D.ARGS), truth, single)


# ---- against torch's own convolution on the GPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(D.GEOMETRIES)), ids=IDS)
def test_zero_offsets_and_a_mask_of_ones_are_torchs_conv2d(index):
    geometry = D.GEOMETRIES[index]
    case = dict(D.make_case(geometry, 200 + index))
    case["offset"], case["mask"] = torch.zeros_like(case["offset"]), torch.ones_like(case["mask"])
    conv = {"stride": geometry[6], "padding": geometry[7], "dilation": geometry[8], "groups": geometry[3]}
    # the float32 restatement's own error against the float64 convolution: the measured bound
    c64 = D.cast(case, F64)
    x64, w64 = c64["input"].requires_grad_(True), c64["weight"].requires_grad_(True)
    truth = F.conv2d(x64, w64, c64["bias"], **conv)
    truth.backward(c64["grad"])
    single = (D.forward_ref(case, torch.float32),) + tuple(D.grads_ref(case, torch.float32))
    x, w = to_dev(case["input"]).requires_grad_(True), to_dev(case["weight"]).requires_grad_(True)
    want = F.conv2d(x, w, to_dev(case["bias"]), **conv)
    want.backward(to_dev(case["grad"]))
    out, grads = run(case, needs=("input", "weight"))
    for name, got, ref, t, s in (("output", out, want.detach(), truth.detach(), single[0]), ("d_input", grads["input"], x.grad, x64.grad, single[1]),
                                 ("d_weight", grads["weight"], w.grad, w64.grad, single[3])):
        err_ref = D.rel_err(s, t)
        err_gpu = D.rel_err(got.cpu(), ref.cpu())
        print("g%d conv2d %-9s err_gpu %.3e err_ref %.3e ratio %.3f" % (index, name, err_gpu, err_ref, err_gpu / max(err_ref, FLOOR)))
        assert float(t.abs().max()) > 0.1 and err_gpu <= MARGIN * max(err_ref, FLOOR), (name, err_gpu, err_ref)


@pytest.mark.parametrize("index", range(len(D.GEOMETRIES)), ids=IDS)
def test_no_mask_is_a_mask_of_ones_bit_for_bit(index):
    case = dict(D.make_case(D.GEOMETRIES[index], 300 + index, with_mask=False))
    out, grads = run(case)
    n, ch = case["offset"].shape[:2]
    case["mask"] = torch.ones((n, ch // 2) + tuple(case["offset"].shape[2:]))
    out1, grads1 = run(case)
    assert torch.equal(out, out1)
    for k in ("input", "offset", "weight", "bias"):
        assert torch.equal(grads[k], grads1[k]), k


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("index", [0, 3], ids=["g0", "g3"])
def test_samples_far_outside_give_the_bias_and_no_gradient(index, with_bias):
    case = dict(D.make_case(D.GEOMETRIES[index], 400 + index, with_bias=with_bias))
    case["offset"] = torch.full_like(case["offset"], 1000.0)
    out, grads = run(case)
    want = to_dev(case["bias"])[None, :, None, None].expand_as(out) if with_bias else torch.zeros_like(out)
    assert torch.equal(out, want)
    for k in ("input", "offset", "mask", "weight"):
        assert grads[k].shape == case[k].shape and not grads[k].any(), k


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 3], ids=["g0", "g3"])
def test_backward_is_bit_identical_and_writes_every_cell(index):
    case, _, _ = reference(index, True, True)
    _, first = run(case)
    # poison the allocator: freed blocks of NaNs of the size of d_input (and of the other 4-d gradients) are what torch.empty hands out next
    for k in ("input", "offset", "mask", "weight"):
        poison = torch.full(case[k].shape, float("nan"), device=DEV)
        del poison
    _, second = run(case)
    for k in D.ARGS:
        assert torch.equal(first[k], second[k]), k
        assert not torch.isnan(second[k]).any(), k
    # cells no sample reaches are written too: with every sample far outside, d_input is exactly zero over poisoned memory
    far = dict(case, offset=torch.full_like(case["offset"], -1000.0))
    poison = torch.full(case["input"].shape, float("nan"), device=DEV)
    del poison
    _, grads = run(far, needs=("input",))
    assert not grads["input"].any() and not torch.isnan(grads["input"]).any()


# ---- chunking --------------------------------------------------------------------------------------------------------------------------------
def per_image(case, i):
    return {k: (v[i:i + 1] if k in ("input", "offset", "mask", "grad") and v is not None else v) for k, v in case.items()}


def check_chunking(case, chunk, label):
    n = case["input"].shape[0]
    out, grads = run(case, chunk=chunk)
    parts = [run(per_image(case, i), chunk=chunk) for i in range(n)]
    assert torch.equal(out, torch.cat([p[0] for p in parts]))
    for k in ("input", "offset", "mask"):
        assert torch.equal(grads[k], torch.cat([p[1][k] for p in parts])), k
    truth = D.grads_ref(case, F64)[2]
    err_ref = D.rel_err(D.grads_ref(case, torch.float32)[2], truth)
    summed = torch.stack([p[1]["weight"] for p in parts]).sum(0)
    for name, g in (("chunked", grads["weight"]), ("per-image sum", summed)):
        err = D.rel_err(g.cpu(), truth)
        print("%s d_weight %-13s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err, err_ref, err / max(err_ref, FLOOR)))
        assert float(truth.abs().max()) > 0.1 and err <= MARGIN * max(err_ref, FLOOR), (name, err, err_ref)


def test_more_images_than_the_chunk_cap_equal_per_image_calls():
    n = ops.DEFORM_CHUNK_IMAGES + 1                                      # a chunk of 32 and a chunk of 1, on a tiny map
    case = D.make_case((n, 2, 3, 1, 1, (3, 3), (1, 1), (1, 1), (1, 1), 5, 6), 500, offset_sigma=1.0)
    check_chunking(case, None, "N=33")


def test_a_lower_cap_through_the_private_op_changes_nothing():
    case, _, _ = reference(0, True, True)                                # N = 3: chunks of 2 + 1
    check_chunking(case, 2, "chunk=2")
    out, grads = run(case)
    out2, grads2 = run(case, chunk=2)
    assert torch.equal(out, out2)
    for k in ("input", "offset", "mask", "bias"):
        assert torch.equal(grads[k], grads2[k]), k


# ---- layouts and flags -------------------------------------------------------------------------------------------------------------------------
def test_channels_last_arguments_and_gradients():
    case, _, _ = reference(0, True, True)
    out, grads = run(case)
    out_cl, grads_cl = run(case, channels_last=("input", "offset", "weight", "mask", "grad"))
    assert torch.equal(out, out_cl) and out_cl.is_contiguous()
    for k in D.ARGS:
        assert torch.equal(grads[k], grads_cl[k]), k
        assert grads[k].is_contiguous(), k
        if k != "bias":
            assert grads_cl[k].is_contiguous(memory_format=CL) and not grads_cl[k].is_contiguous(), k
    out_in, grads_in = run(case, channels_last=("input",))
    assert torch.equal(out, out_in) and grads_in["input"].is_contiguous(memory_format=CL) and grads_in["offset"].is_contiguous()


@pytest.mark.parametrize("only", ["offset", "weight", "input", "mask", "bias"])
def test_a_single_gradient_equals_the_full_backward(only):
    case, _, _ = reference(3, True, True)
    _, full = run(case)
    _, one = run(case, needs=(only,))
    assert torch.equal(one[only], full[only])
    assert all(one[k] is None for k in D.ARGS if k != only)


# ---- the module ----------------------------------------------------------------------------------------------------------------------------------
def test_module_equals_the_function_and_double_backward_raises():
    n, c, co, groups, g, kernel, stride, padding, dilation, h, w = D.GEOMETRIES[0]
    case, _, _ = reference(0, True, True)
    m = ops.DeformConv2d(c, co, kernel, stride=stride, padding=padding, dilation=dilation, groups=groups).to(DEV)
    with torch.no_grad():
        m.weight.copy_(to_dev(case["weight"]))
        m.bias.copy_(to_dev(case["bias"]))
    x, off, mask = (to_dev(case[k]).requires_grad_(True) for k in ("input", "offset", "mask"))
    y = m(x, off, mask)
    y.backward(to_dev(case["grad"]))
    out, grads = run(case)
    assert torch.equal(y.detach(), out)
    for got, k in ((x.grad, "input"), (off.grad, "offset"), (mask.grad, "mask"), (m.weight.grad, "weight"), (m.bias.grad, "bias")):
        assert torch.equal(got, grads[k]), k
    x = to_dev(case["input"]).requires_grad_(True)
    y = ops.deform_conv2d(x, to_dev(case["offset"]), to_dev(case["weight"]), **case["kw"])
    v = torch.ones_like(y, requires_grad=True)
    gx, = torch.autograd.grad(y, x, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()


# ---- meta checks -----------------------------------------------------------------------------------------------------------------------------------
def test_opcheck_both_ops():
    case, _, _ = reference(0, True, True)
    x, off, w, b, mask, grad = (to_dev(case[k]) for k in ("input", "offset", "weight", "bias", "mask", "grad"))
    checks = ("test_schema", "test_faketensor")
    for args in ((x, off, w, b, mask, 1, 1, 1, 1, 1, 1, 32), (x, off, w, None, None, 1, 1, 1, 1, 1, 1, 2)):
        torch.library.opcheck(torch.ops.frcnn.deform_conv2d.default, args, test_utils=checks)
    for m, needs, cl in ((mask, [True] * 5, [False] * 4), (mask, [False, True, False, False, False], [False] * 4),
                         (None, [True, False, True, True, False], [True, False, False, False])):
        torch.library.opcheck(torch.ops.frcnn.deform_conv2d_backward.default, (grad, x, off, w, m, 1, 1, 1, 1, 1, 1, 32, needs, cl),
                              test_utils=checks)


# ---- empty calls -------------------------------------------------------------------------------------------------------------------------------------
def test_empty_calls():
    base = D.GEOMETRIES[0]
    for geometry in ((0,) + base[1:], base[:2] + (0,) + base[3:]):
        n, c, co = geometry[:3]
        case = D.make_case(geometry, 600)
        out, grads = run(case)
        assert out.shape == (n, co, 9, 11) and out.device.type == "cuda"
        for k in D.ARGS:
            assert grads[k].shape == case[k].shape and not grads[k].any(), k
