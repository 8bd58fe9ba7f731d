"""fasterrcnn_amd.ops.deform_conv2d / DeformConv2d on float16 and bfloat16 tensors on the GPU, against the contract of
fasterrcnn_amd/ops.py (tests/deform16_cases.py restates it).  T is the 16-bit dtype, p its significant bits (11 / 8).

Every bound is derived, none is tuned.  "2^-p |truth|" below is one rounding of the truth to T (deform16_cases.rounding_error): 2^-p |truth|
in T's normal range and half of the subnormal spacing (float16: 2^-25) below it, where a rounding error is absolute -- the exactly rounded
float64 truth itself misses the plain 2^-p |truth| there.
  columns   bit for bit the float32 operator's columns of the widened tensors, rounded to T (one-hot weights make both products exact);
  forward   |out - truth| <= 2^-p |truth| + (K + 2) 2^-24 (sum_k |w| |col| + |bias|): one rounding to T and the standard bound of a float32
            sum of K exact products and a bias; truth is the float64 product of the weights with col16;
  d_weight  the same form with R = N oh ow terms; d_bias likewise;
  d_input, d_offset, d_mask   |got - truth| <= 2^-p |truth| + 4 E32, truth the float64 restatement's gradient of the widened tensors and E32
            the largest error of the float32 operator on them (floored at 2^-24 max |truth|), measured in the test: the margin of 4 is the
            one tests/test_ops_deform_gpu.py gives.
Route of the columns: EVERY case takes col16 from the one-hot probe of the FLOAT32 operator (C_in kh kw <= 360 output channels), rounded
to T -- code this suite does not put under test; the first test pins the 16-bit operator's own columns to it.  No case needs CPU columns.

The block tile of csrc/gemm_nt16.hip is 128 x 128, so shape a keeps C_out = 130.

Largest ratios measured on an MI355X over every case below (each test prints its own): error / bound of the forward 0.996 (g2, bfloat16:
an output of two products sits on its rounding), of d_weight 0.995, of d_bias below both; (|got - truth| - 2^-p |truth|) / E32 of d_input,
d_offset and d_mask at most 0.07 against the bound of 4: the 16-bit gradients are one rounding away from the float32 operator's."""
import functools

import pytest
import torch

from fasterrcnn_amd import ops

from tests import deform16_cases as H
from tests import deform_conv_cases as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
dtypes = pytest.mark.parametrize("dtype", H.DTYPES, ids=H.DTYPE_IDS)
shapes = pytest.mark.parametrize("index", range(len(H.GEOMETRIES)), ids=H.IDS)
full = pytest.mark.parametrize("full", [True, False], ids=["mask+bias", "plain"])
A = H.GEOMETRIES.index(H.SHAPE_A)


def poison():
    """Freed blocks of 0xFF bytes (NaN in float16, bfloat16 and float32) of every size up to 4 MB: what torch.empty hands the operator's
    workspaces next, so that a pad nobody writes is a NaN in the product."""
    blocks = [torch.full((2 ** k,), 255, dtype=torch.uint8, device=DEV) for k in range(9, 23)]
    torch.cuda.synchronize()
    del blocks


def on_device(case):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def one_hot(c, dtype):
    cin = c["input"].shape[1]
    kh, kw = c["weight"].shape[2:]
    rows = cin * kh * kw
    return torch.eye(rows, dtype=dtype, device=DEV).reshape(rows, cin, kh, kw)


def probe(c, dtype):
    """The columns through one-hot weights (groups = 1, weight[r] = e_r): [N, C_in kh kw, oh, ow] of `dtype`; every product is exact."""
    x, off, m = (None if c[k] is None else c[k].to(dtype) for k in ("input", "offset", "mask"))
    return ops.deform_conv2d(x, off, one_hot(c, dtype), mask=m, **c["kw"])


@functools.lru_cache(maxsize=None)
def reference(index, dtype, with_all):
    """(the case on the CPU, on the GPU, col16 [N, groups, K, P] on the CPU from the float32 operator's probe), computed once."""
    case = H.make_case16(H.GEOMETRIES[index], 800 + index, dtype, with_mask=with_all, with_bias=with_all)
    c = on_device(case)
    groups = c["input"].shape[1] // c["weight"].shape[1]
    col16 = probe(c, torch.float32).to(dtype)
    n, rows = col16.shape[:2]
    return case, c, col16.reshape(n, groups, rows // groups, -1).cpu()


def run(c, needs=D.ARGS, backward=True):
    """The operator on the GPU in the dtype of c's tensors: (output, {name: gradient})."""
    leaves = {k: (None if c[k] is None else c[k].clone().requires_grad_(k in needs)) for k in D.ARGS}
    out = ops.deform_conv2d(leaves["input"], leaves["offset"], leaves["weight"], leaves["bias"], mask=leaves["mask"], **c["kw"])
    if not backward:
        return out.detach(), {}
    out.backward(c["grad"])
    return out.detach(), {k: (None if t is None else t.grad) for k, t in leaves.items()}


def private(c, chunk, needs=(True,) * 5):
    """(output, [d_input, d_offset, d_weight, d_bias, d_mask]) through the private ops with a chunk of `chunk` images."""
    kw = c["kw"]
    geometry = (*kw["stride"], *kw["padding"], *kw["dilation"])
    out = torch.ops.frcnn.deform_conv2d(c["input"], c["offset"], c["weight"], c["bias"], c["mask"], *geometry, chunk)
    grads = torch.ops.frcnn.deform_conv2d_backward(c["grad"], c["input"], c["offset"], c["weight"], c["mask"], *geometry, chunk,
                                                   list(needs), [False] * 4)
    return out, grads


def assert_within(label, got, truth, bound):
    err = (got.double().cpu().reshape(truth.shape) - truth).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s max err / bound %.3f" % (label, ratio))
    assert float(truth.abs().max()) > 0.1 and bool((err <= bound).all()), (label, ratio)
    return ratio


# ---- 1. the column seam, bit for bit ---------------------------------------------------------------------------------------------------
@dtypes
@full
@pytest.mark.parametrize("index", [0, 1], ids=["g0", "g1"])
def test_columns_are_the_float32_operators_rounded_once(index, full, dtype):
    _, c, _ = reference(index, dtype, full)
    poison()
    got = probe(c, dtype)
    want = probe(c, torch.float32).to(dtype)
    assert got.dtype == dtype and got.is_contiguous() and torch.equal(got, want)
    assert float(want.float().abs().max()) > 0.5 and float((want == 0).float().mean()) > 0.05        # samples, and rejected ones


# ---- 2. the forward product ---------------------------------------------------------------------------------------------------------------
@dtypes
@full
@shapes
def test_forward_is_one_rounding_of_a_float32_sum(index, full, dtype):
    case, c, col16 = reference(index, dtype, full)
    poison()
    out, _ = run(c, backward=False)
    assert out.dtype == dtype and out.is_contiguous() and out.shape[:2] == (case["input"].shape[0], case["weight"].shape[0])
    truth, mass = H.product(case["weight"], col16, case["bias"])
    terms = col16.shape[2]
    bound = H.rounding_error(truth, dtype) + H.sum_bound(terms, mass)
    assert_within("%s %s forward (probe route, K = %d)" % (H.IDS[index], dtype, terms), out, truth, bound)
    assert bool(torch.isfinite(out.float()).all())


# ---- 3. d_weight and d_bias ---------------------------------------------------------------------------------------------------------------
@dtypes
@full
@shapes
def test_weight_and_bias_gradients(index, full, dtype):
    case, c, col16 = reference(index, dtype, full)
    poison()
    _, grads = run(c, needs=("weight", "bias"))
    terms = case["grad"].shape[0] * case["grad"].shape[2] * case["grad"].shape[3]                     # R = N oh ow
    truth, mass = H.weight_product(case["grad"], col16)
    assert grads["weight"].dtype == dtype and grads["weight"].shape == case["weight"].shape
    bound = H.rounding_error(truth, dtype) + H.sum_bound(terms, mass)
    assert_within("%s %s d_weight (R = %d)" % (H.IDS[index], dtype, terms), grads["weight"], truth, bound)
    if full:
        g = case["grad"].double()
        truth, mass = g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))
        assert grads["bias"].dtype == dtype
        assert_within("%s %s d_bias" % (H.IDS[index], dtype), grads["bias"], truth, H.rounding_error(truth, dtype) + H.sum_bound(terms, mass))


# ---- 4. d_input, d_offset, d_mask -----------------------------------------------------------------------------------------------------------
@dtypes
@full
@shapes
def test_sampling_gradients_against_float64_with_the_float32_operator_as_yardstick(index, full, dtype):
    case, c, _ = reference(index, dtype, full)
    truth = dict(zip(D.ARGS, D.grads_ref(H.widen(case, F64), F64)))
    _, single = run(H.widen(c, torch.float32), needs=("input", "offset", "mask"))
    _, grads = run(c, needs=("input", "offset", "mask"))
    for k in ("input", "offset", "mask"):
        if truth[k] is None:
            assert grads[k] is None
            continue
        t = truth[k]
        assert grads[k].dtype == dtype and grads[k].shape == t.shape and float(t.abs().max()) > 0.1
        e32 = max(float((single[k].double().cpu() - t).abs().max()), 2.0 ** -24 * float(t.abs().max()))
        err = (grads[k].double().cpu() - t).abs()
        excess = float(((err - H.rounding_error(t, dtype)) / e32).max())
        print("%s %s d_%-6s E32 %.3e (err - 2^-p |truth|) / E32 %.3f" % (H.IDS[index], dtype, k, e32, excess))
        assert bool((err <= H.rounding_error(t, dtype) + 4.0 * e32).all()), (k, excess)


# ---- 5. chunking ----------------------------------------------------------------------------------------------------------------------------
@dtypes
def test_chunking_changes_only_the_order_of_the_weight_gradients_sum(dtype):
    case, c, col16 = reference(A, dtype, True)
    out1, grads1 = private(c, 1)
    out32, grads32 = private(c, 32)
    assert torch.equal(out1, out32)
    for i, k in ((0, "input"), (1, "offset"), (4, "mask"), (3, "bias")):
        assert torch.equal(grads1[i], grads32[i]), k
    terms = case["grad"].shape[0] * case["grad"].shape[2] * case["grad"].shape[3]
    truth, mass = H.weight_product(case["grad"], col16)
    bound = H.rounding_error(truth, dtype) + H.sum_bound(terms, mass)
    for chunk, grads in ((1, grads1), (32, grads32)):
        assert_within("a %s d_weight chunk = %d" % (dtype, chunk), grads[2], truth, bound)


@dtypes
def test_weight_gradient_chunks_are_added_in_float32_and_rounded_once(dtype):
    """Three equal images in chunks of one: every chunk's d_weight is the same value v, exact in float32 (small integers times multiples
    of 2^-6, zero offsets, no mask), so the contract gives round_T((v + v) + v) -- and adding the chunks in T would give something else."""
    n, cin, co, groups, g, kernel, stride, padding, dilation, h, w = H.SHAPE_A
    gen = torch.Generator().manual_seed(900)
    oh, ow = D.output_size(h, w, kernel, stride, padding, dilation)
    image = torch.randint(-4, 5, (1, cin, h, w), generator=gen).float()
    grad = torch.randint(-128, 129, (1, co, oh, ow), generator=gen).float() / 64
    case = {"input": image.expand(n, -1, -1, -1).contiguous(), "offset": torch.zeros((n, 2 * g * 9, oh, ow)),
            "weight": torch.zeros((co, cin // groups) + kernel), "bias": None, "mask": None, "grad": grad.expand(n, -1, -1, -1).contiguous(),
            "kw": {"stride": stride, "padding": padding, "dilation": dilation}}
    case = D.cast(case, dtype)
    assert all(torch.equal(case[k].float(), v) for k, v in (("input", image.expand(n, -1, -1, -1)), ("grad", grad.expand(n, -1, -1, -1))))
    col = H.columns(case, F64)
    v, _ = H.weight_product(case["grad"][:1], col[:1])
    assert torch.equal(v.float().double(), v) and torch.equal((3 * v).float().double(), 3 * v)       # exact in float32
    parts = [v.float()] * n
    want, stepwise = H.f32_accumulate(parts, dtype), H.t_accumulate(parts, dtype)
    differing = int((want != stepwise).sum())
    print("%s: %d of %d elements tell the float32 accumulation from the T accumulation" % (dtype, differing, want.numel()))
    assert differing > 20                                                # checked on the CPU first
    _, grads = private(on_device(case), 1, needs=(False, False, True, False, False))
    got = grads[2].cpu().reshape(want.shape)
    assert got.dtype == dtype and torch.equal(got, want)
    assert not torch.equal(got, stepwise)


# ---- 6. determinism and `needs` -------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("index", [3, A], ids=["g3", "a"])
def test_two_runs_agree_and_a_single_gradient_equals_the_full_backward(index, dtype):
    _, c, _ = reference(index, dtype, True)
    out1, first = run(c)
    poison()
    out2, second = run(c)
    assert torch.equal(out1, out2)
    for k in D.ARGS:
        assert torch.equal(first[k], second[k]) and not torch.isnan(second[k].float()).any(), k
    for only in D.ARGS:
        _, one = run(c, needs=(only,))
        assert torch.equal(one[only], first[only]), only
        assert all(one[k] is None for k in D.ARGS if k != only)


# ---- 7. the module under autocast -----------------------------------------------------------------------------------------------------------
@dtypes
def test_module_under_autocast_casts_its_float32_parameters(dtype):
    n, cin, co, groups, g, kernel, stride, padding, dilation, h, w = H.GEOMETRIES[0]
    case, c, _ = reference(0, dtype, True)
    m = ops.DeformConv2d(cin, co, kernel, stride=stride, padding=padding, dilation=dilation, groups=groups).to(DEV)
    assert m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32
    x = c["input"].clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        y = m(x, c["offset"].float(), c["mask"].float())                # float32 offset and mask: the module casts them
    assert y.dtype == dtype
    y.backward(c["grad"])
    assert m.weight.grad.dtype == torch.float32 and m.bias.grad.dtype == torch.float32 and x.grad.dtype == dtype
    w16, b16 = m.weight.detach().to(dtype).requires_grad_(True), m.bias.detach().to(dtype).requires_grad_(True)
    x2 = c["input"].clone().requires_grad_(True)
    y2 = ops.deform_conv2d(x2, c["offset"], w16, b16, mask=c["mask"], **c["kw"])
    y2.backward(c["grad"])
    assert torch.equal(y.detach(), y2.detach()) and torch.equal(x.grad, x2.grad)
    assert torch.equal(m.weight.grad, w16.grad.float()) and torch.equal(m.bias.grad, b16.grad.float())


# ---- 8. opcheck -----------------------------------------------------------------------------------------------------------------------------
def test_opcheck_both_ops_in_float16():
    _, c, _ = reference(0, torch.float16, True)
    x, off, w, b, mask, grad = (c[k] for k in ("input", "offset", "weight", "bias", "mask", "grad"))
    checks = ("test_schema", "test_faketensor")
    for args in ((x, off, w, b, mask, 1, 1, 1, 1, 1, 1, 32), (x, off, w, None, None, 1, 1, 1, 1, 1, 1, 2)):
        torch.library.opcheck(torch.ops.frcnn.deform_conv2d.default, args, test_utils=checks)
    for m, needs, cl in ((mask, [True] * 5, [False] * 4), (None, [True, False, True, True, False], [True, False, False, False])):
        torch.library.opcheck(torch.ops.frcnn.deform_conv2d_backward.default, (grad, x, off, w, m, 1, 1, 1, 1, 1, 1, 32, needs, cl),
                              test_utils=checks)


# ---- empty calls ------------------------------------------------------------------------------------------------------------------------------
@dtypes
def test_empty_calls(dtype):
    base = D.GEOMETRIES[0]
    for geometry in ((0,) + base[1:], base[:2] + (0,) + base[3:]):
        case = H.make_case16(geometry, 600, dtype)
        out, grads = run(on_device(case))
        assert out.shape == (geometry[0], geometry[2], 9, 11) and out.dtype == dtype and out.device.type == "cuda"
        for k in D.ARGS:
            assert grads[k].shape == case[k].shape and grads[k].dtype == dtype and not grads[k].any(), k
