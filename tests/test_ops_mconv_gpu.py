"""fasterrcnn_amd.ops.masked_conv2d / MaskedConv2d on the GPU against the float64 truth of tests/mconv_cases.py (F.conv2d in float64 on
the CPU, times the mask), and the properties the kernels promise: an active pixel's bits do not depend on the rest of the mask, on the
number of images or on the memory format; inactive outputs are +0.0 without the bias; padding taps are zeros and never the neighbouring
row or image; two runs agree; nothing synchronises with the host.

The bound of every value comparison is measured in the same test, as in tests/test_ops_quadri_gpu.py: err(a) = max|a - truth| /
max|truth| over the case, err_ref is the error of the same sum evaluated in float32 on the CPU (for a 16-bit case: on the 16-bit-valued
inputs, rounded once to the dtype), and err_gpu <= 4 * max(err_ref, 2**-24) must hold.  The MFMA's sum order is not the CPU's, so no
bits are claimed against the CPU.  A 16-bit result differs from the float32 operator on the widened tensors by at most one rounding of
the 16-bit type plus that float32 bound.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: 1.396 (float32, case "n3": err_gpu 1.88e-7 against
err_ref 1.35e-7; then 1.378 on "kernel_3x3_p0" and 1.320 on "K_2"); every float16 and bfloat16 case gave 1.000 to the printed digits,
the one rounding to the dtype being the whole error.  Against the float32 operator on the widened tensors the largest
|y_T - y_32| / (u (|y_32| + B) + B) over the active outputs was 0.984 (bfloat16 "K_50" and "kernel_3x3_p1", float16 "kernel_1x3_p01"),
and the inactive outputs were equal."""
import functools

import pytest
import torch

from fasterrcnn_amd import ops

from tests import mconv_cases as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
CL = torch.channels_last
BOUND = 4.0
FLOOR = 2.0 ** -24
IDS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
dtypes = pytest.mark.parametrize("dtype", M.DTYPES, ids=IDS.values())


def check_bound(label, got, name, dtype):
    """err_gpu <= 4 * max(err_ref, 2**-24); prints both errors; returns the ratio."""
    want, single = M.truth(name, dtype), M.restated(name, dtype)
    assert got.shape == want.shape and got.dtype == dtype and single.dtype == dtype, label
    err_gpu, err_ref = M.rel_err(got.cpu(), want), M.rel_err(single, want)
    ratio = err_gpu / max(err_ref, FLOOR)
    print("%s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, err_gpu, err_ref, ratio))
    assert err_gpu <= BOUND * max(err_ref, FLOOR), (label, err_gpu, err_ref)
    return ratio


@functools.lru_cache(maxsize=None)
def on_gpu(name, dtype=F32):
    return tuple(t.to(DEV) for t in M.case(name, dtype))


def run(name, dtype=F32, **kw):
    x, mask, wt, b = on_gpu(name, dtype)
    return ops.masked_conv2d(x, mask, wt, b, M.CASES[name]["pad"], **kw)


def plus_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("name", M.VALUE_CASES)
def test_values_against_the_truth(name, dtype):
    got = run(name, dtype)
    check_bound("%s %s" % (name, IDS[dtype]), got, name, dtype)
    inactive = ~(on_gpu(name, dtype)[1] > 0)[:, None].expand_as(got)
    assert plus_zero(got[inactive])                                           # the bias of every case is non-zero: none of it here


@dtypes
def test_no_active_pixel_gives_plus_zero(dtype):
    got = run("count_0", dtype)
    assert got.shape == M.truth("count_0").shape and got.dtype == dtype and plus_zero(got)


@pytest.mark.parametrize("dtype", M.HALF, ids=("f16", "bf16"))
@pytest.mark.parametrize("name", M.VALUE_CASES)
def test_16_bit_is_one_rounding_from_the_float32_operator(name, dtype):
    """|y_T - y_32| <= u (|y_32| + B) + B: y_T rounds a float32 accumulator that lies within B of y_32, u = half an ulp of T, and B is the
    float32 operator's own bound, 4 max(err_ref, 2**-24) max|truth|, on the widened tensors."""
    x, mask, wt, b = on_gpu(name, dtype)
    pad = M.CASES[name]["pad"]
    wide = ops.masked_conv2d(x.float(), mask, wt.float(), b.float(), pad)
    got = ops.masked_conv2d(x, mask, wt, b, pad).float()
    want = M.truth(name, dtype)
    single = M.dense(*M.case(name, dtype), pad, F32)
    bound32 = BOUND * max(M.rel_err(single, want), FLOOR) * float(want.abs().max())
    active = (mask > 0)[:, None].expand_as(got)
    limit = M.ROUNDING[dtype] * (wide.abs().double() + bound32) + bound32
    ratio = float(((got - wide).abs().double()[active] / limit[active]).max())
    print("%s %s largest |y_T - y_32| / limit over the active outputs %.3f (bound32 %.3e)" % (name, IDS[dtype], ratio, bound32))
    assert ratio <= 1 and torch.equal(got[~active], wide[~active])


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("k,pad", (((3, 3), (1, 1)), ((5, 5), (2, 2)), ((1, 3), (0, 1)), ((3, 3), (2, 2))))
def test_ones_count_the_taps_inside_the_map(k, pad, dtype):
    """Features and weights all ones, zero bias, the four corners and the edge midpoints active: the output is C_in times the number of
    taps inside the map, a small integer, exact in all three dtypes.  A tap that wraps into the neighbouring row would be counted."""
    n, c, h, w, co = 2, 3, 6, 7, 5
    oh, ow = h + 2 * pad[0] - k[0] + 1, w + 2 * pad[1] - k[1] + 1
    mask = torch.zeros((n, oh, ow), device=DEV)
    ys, xs = (0, oh // 2, oh - 1), (0, ow // 2, ow - 1)
    for y in ys:
        for x in xs:
            if (y, x) != (oh // 2, ow // 2):
                mask[:, y, x] = 1
    x = torch.ones((n, c, h, w), dtype=dtype, device=DEV)
    wt = torch.ones((co, c) + k, dtype=dtype, device=DEV)
    got = ops.masked_conv2d(x, mask, wt, torch.zeros((co,), dtype=dtype, device=DEV), pad)
    inside_y = torch.tensor([sum(0 <= y - pad[0] + i < h for i in range(k[0])) for y in range(oh)], device=DEV)
    inside_x = torch.tensor([sum(0 <= x - pad[1] + j < w for j in range(k[1])) for x in range(ow)], device=DEV)
    want = (c * inside_y[:, None] * inside_x[None, :] * (mask > 0)).to(dtype)[:, None].expand(n, co, oh, ow)
    assert torch.equal(got, want)
    assert torch.equal(ops.masked_conv2d(x.contiguous(memory_format=CL), mask, wt, None, pad), want)


@dtypes
def test_nan_images_behind_empty_masks_reach_nothing(dtype):
    """An image of NaNs with an empty mask before and after a normal image: a tap that wraps into the neighbouring image would bring a
    NaN, and an inactive pixel that multiplied anything would too."""
    x, mask, wt, b = on_gpu("kernel_3x3_p2", dtype)
    nan = torch.full_like(x[:1], float("nan"))
    x3 = torch.cat([nan, x[:1], nan])
    m3 = torch.cat([torch.zeros_like(mask[:1]), torch.ones_like(mask[:1]), torch.zeros_like(mask[:1])])
    for xin in (x3, x3.contiguous(memory_format=CL)):
        got = ops.masked_conv2d(xin, m3, wt, b, M.CASES["kernel_3x3_p2"]["pad"])
        assert bool(torch.isfinite(got).all()) and plus_zero(got[0]) and plus_zero(got[2])
        assert torch.equal(got[1], ops.masked_conv2d(x[:1], mask[:1] * 0 + 1, wt, b, M.CASES["kernel_3x3_p2"]["pad"])[0])


@dtypes
@pytest.mark.parametrize("channels_last", (False, True), ids=("nchw", "cl"))
def test_inactive_outputs_are_plus_zero_under_a_bias(channels_last, dtype):
    x, mask, wt, _ = on_gpu("Cout_33", dtype)
    b = torch.linspace(-3, 3, wt.shape[0], device=DEV).to(dtype) - 0.125      # no zero among them
    assert bool((b != 0).all())
    got = ops.masked_conv2d(x.contiguous(memory_format=CL) if channels_last else x, mask, wt, b, 1)
    inactive = ~(mask > 0)[:, None].expand_as(got)
    assert int(inactive.sum()) > 0 and plus_zero(got[inactive])
    assert bool((got[~inactive] != 0).all())


# ---- 3. bit properties, GPU against GPU ----------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("name", ("count_%d" % (M.T + 1), "kernel_3x3_p2", "K_%d" % (M.KC + 1), "Cout_%d" % (M.CO + 1)))
def test_an_active_pixel_does_not_see_the_rest_of_the_mask(name, dtype):
    x, mask, wt, b = on_gpu(name, dtype)
    pad = M.CASES[name]["pad"]
    got = ops.masked_conv2d(x, mask, wt, b, pad)
    full = ops.masked_conv2d(x, torch.ones_like(mask), wt, b, pad)
    active = (mask > 0)[:, None].expand_as(got)
    assert torch.equal(got[active], full[active])
    where = torch.nonzero(mask > 0)
    for i in (0, len(where) // 2, len(where) - 1):                           # a mask of that pixel alone
        bi, y, xx = where[i].tolist()
        alone = torch.zeros_like(mask)
        alone[bi, y, xx] = 1
        one = ops.masked_conv2d(x, alone, wt, b, pad)
        assert torch.equal(one[bi, :, y, xx], got[bi, :, y, xx]) and int((one != 0).sum()) <= wt.shape[0]


@dtypes
def test_an_n_image_call_equals_the_single_image_calls(dtype):
    x, mask, wt, b = on_gpu("n3", dtype)
    got = ops.masked_conv2d(x, mask, wt, b, 1)
    for i in range(x.shape[0]):
        assert torch.equal(got[i:i + 1], ops.masked_conv2d(x[i:i + 1], mask[i:i + 1], wt, b, 1))


@dtypes
@pytest.mark.parametrize("name", ("n3", "kernel_5x5_p2", "Cout_80", "K_1"))
def test_memory_formats_agree_each_in_its_own_format(name, dtype):
    x, mask, wt, b = on_gpu(name, dtype)
    pad = M.CASES[name]["pad"]
    a = ops.masked_conv2d(x, mask, wt, b, pad)
    c = ops.masked_conv2d(x.contiguous(memory_format=CL), mask, wt.contiguous(memory_format=CL), b, pad)
    assert a.is_contiguous() and torch.equal(a, c)
    if x.shape[1] > 1:
        assert c.is_contiguous(memory_format=CL) and not c.is_contiguous()
    sliced = torch.cat([x, x], 3)[..., :x.shape[3]]                           # neither contiguous nor channels_last: made contiguous first
    assert not sliced.is_contiguous() and torch.equal(ops.masked_conv2d(sliced, mask, wt, b, pad), a)


@dtypes
def test_two_runs_agree_and_nothing_synchronises(dtype):
    x, mask, wt, b = on_gpu("count_%d" % (2 * M.T + 1), dtype)
    xc = x.contiguous(memory_format=CL)
    module = ops.MaskedConv2d(x.shape[1], wt.shape[0], 3, padding=1).to(DEV, dtype)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            outs = [ops.masked_conv2d(t, mask, wt, b, 1) for t in (x, x, xc)]
            mods = [module(x, mask), module(x, mask > 0)]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.equal(mods[0], mods[1])
    check_bound("no-sync %s" % IDS[dtype], outs[0], "count_%d" % (2 * M.T + 1), dtype)


# ---- 4. the mask, the interface ------------------------------------------------------------------------------------------------------------
@dtypes
def test_mask_dtypes_and_nan(dtype):
    x, mask, wt, b = on_gpu("n3", dtype)
    assert bool((mask < 0).any())
    want = ops.masked_conv2d(x, mask, wt, b, 1)
    active = mask > 0
    for other in (active, active.to(torch.uint8), active.long() - (mask < 0).long(), mask.double(), mask.half()):
        assert torch.equal(ops.masked_conv2d(x, other, wt, b, 1), want)
    nan_mask = torch.where(active, mask, torch.full_like(mask, float("nan")))  # NaN is inactive
    assert torch.equal(ops.masked_conv2d(x, nan_mask, wt, b, 1), want)
    assert torch.equal(ops.masked_conv2d(x, mask.expand(2, *mask.shape)[1].transpose(1, 2).contiguous().transpose(1, 2), wt, b, 1), want)


@dtypes
def test_no_bias_is_a_zero_bias(dtype):
    x, mask, wt, b = on_gpu("Cout_31", dtype)
    assert torch.equal(ops.masked_conv2d(x, mask, wt, None, 1), ops.masked_conv2d(x, mask, wt, torch.zeros_like(b), 1))


@dtypes
def test_module_with_a_mask(dtype):
    x, mask, wt, b = on_gpu("kernel_3x3_p1", dtype)
    ref = torch.nn.Conv2d(x.shape[1], wt.shape[0], 3, padding=1).to(DEV, dtype)
    with torch.no_grad():
        ref.weight.copy_(wt)
        ref.bias.copy_(b)
    m = ops.MaskedConv2d(x.shape[1], wt.shape[0], 3, padding=1).to(DEV, dtype)
    m.load_state_dict(ref.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(m(x, mask), ops.masked_conv2d(x, mask, wt, b, 1))
        assert torch.equal(m(x), ref(x))
    y = m(x.clone().requires_grad_(True), mask)                               # no autograd formula: the backward raises
    with pytest.raises((RuntimeError, NotImplementedError)):
        y.sum().backward()
    empty = ops.masked_conv2d(x[:0], mask[:0], wt, b, 1)
    assert empty.shape == (0,) + tuple(y.shape[1:])
    with pytest.raises(ValueError):
        ops.masked_conv2d(x, mask.cpu(), wt, b, 1)


@pytest.mark.parametrize("pytorch_dtype", (F32, F64), ids=("f32", "f64"))
def test_pytorch_form_on_the_gpu(pytorch_dtype):
    x, mask, wt, b = (t.to(pytorch_dtype) if t.is_floating_point() else t for t in on_gpu("kernel_3x3_p2"))
    got = ops.masked_conv2d_pytorch(x, mask, wt, b, 2)
    assert got.device.type == "cuda" and got.dtype == pytorch_dtype
    assert M.rel_err(got.cpu(), M.truth("kernel_3x3_p2")) <= (1e-12 if pytorch_dtype == F64 else
                                                             BOUND * max(M.rel_err(M.restated("kernel_3x3_p2"), M.truth("kernel_3x3_p2")), FLOOR))


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


@dtypes
@pytest.mark.parametrize("channels_last", (False, True), ids=("nchw", "cl"))
def test_opcheck(channels_last, dtype):
    x, mask, wt, b = on_gpu("kernel_1x3_p01", dtype)
    x = x.contiguous(memory_format=CL) if channels_last else x
    m8 = (mask > 0).view(torch.uint8)
    torch.library.opcheck(torch.ops.frcnn.masked_conv2d.default, (x, m8, wt, b, 0, 1), test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.masked_conv2d.default, (x, m8, wt, None, 0, 1), test_utils=OPCHECK)
