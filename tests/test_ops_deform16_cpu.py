"""fasterrcnn_amd.ops.deform_conv2d / DeformConv2d on float16 and bfloat16 tensors, without a GPU: shapes and dtypes on `meta`, the
dtype rule (all float32, all float16 or all bfloat16; every mix is the TypeError it was), the module's AMP rule, and the CPU
restatement of the 16-bit contract that the GPU tests lean on (tests/deform16_cases.py)."""
import pytest
import torch

from fasterrcnn_amd import ops

from tests import deform16_cases as H
from tests import deform_conv_cases as D

IDS = ["g%d" % i for i in range(len(D.GEOMETRIES))]
dtypes = pytest.mark.parametrize("dtype", H.DTYPES, ids=H.DTYPE_IDS)


def meta_case(geometry, dtype, seed=0):
    case = H.make_case16(geometry, seed, dtype)
    return {k: (v.to("meta") if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


# ---- meta shapes and dtypes ----------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("index", range(len(D.GEOMETRIES)), ids=IDS)
def test_meta_shape_and_dtype(index, dtype):
    geometry = D.GEOMETRIES[index]
    c = meta_case(geometry, dtype)
    n, co = geometry[0], geometry[2]
    for bias, mask in ((c["bias"], c["mask"]), (None, None)):
        out = ops.deform_conv2d(c["input"], c["offset"], c["weight"], bias, mask=mask, **c["kw"])
        assert out.shape == (n, co) + tuple(c["offset"].shape[2:]) and out.dtype == dtype and out.device.type == "meta"
        assert out.is_contiguous()


@dtypes
def test_meta_empty_calls(dtype):
    base = D.GEOMETRIES[0]
    for geometry in ((0,) + base[1:], base[:2] + (0,) + base[3:]):
        c = meta_case(geometry, dtype)
        out = ops.deform_conv2d(c["input"], c["offset"], c["weight"], c["bias"], mask=c["mask"], **c["kw"])
        assert out.shape == (geometry[0], geometry[2], 9, 11) and out.dtype == dtype


@dtypes
def test_meta_backward_shapes_and_dtypes(dtype):
    c = meta_case(D.GEOMETRIES[0], dtype)
    grads = torch.ops.frcnn.deform_conv2d_backward(c["grad"], c["input"], c["offset"], c["weight"], c["mask"], 1, 1, 1, 1, 1, 1, 32,
                                                   [True] * 5, [False] * 4)
    for g, k in zip(grads, ("input", "offset", "weight", "bias", "mask")):
        assert g.shape == c[k].shape and g.dtype == dtype, k


# ---- mixes still raise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.ARGS)
@pytest.mark.parametrize("base, other", [(torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.float32, torch.float16),
                                         (torch.float32, torch.bfloat16), (torch.float16, torch.float32), (torch.float16, torch.float64),
                                         (torch.float32, torch.float64)],
                         ids=["f16+bf16", "bf16+f16", "f32+f16", "f32+bf16", "f16+f32", "f16+f64", "f32+f64"])
def test_a_mix_of_dtypes_is_a_type_error_that_names_a_tensor(name, base, other):
    c = meta_case(D.GEOMETRIES[0], base)
    c[name] = c[name].to(other)
    with pytest.raises(TypeError, match=r"(input|offset|weight|bias|mask) must be float32.*\.float\(\)"):
        ops.deform_conv2d(c["input"], c["offset"], c["weight"], c["bias"], mask=c["mask"], **c["kw"])


@dtypes
def test_one_16_bit_tensor_among_float32_names_that_tensor(dtype):
    for name in D.ARGS:
        c = meta_case(D.GEOMETRIES[0], torch.float32)
        c[name] = c[name].to(dtype)
        with pytest.raises(TypeError, match=r"%s must be float32.*\.float\(\)" % name):
            ops.deform_conv2d(c["input"], c["offset"], c["weight"], c["bias"], mask=c["mask"], **c["kw"])


# ---- the module under AMP ----------------------------------------------------------------------------------------------------------------
@dtypes
def test_module_casts_to_a_16_bit_input_and_leaves_float32_alone(dtype):
    n, c, co, groups, g, kernel, stride, padding, dilation, h, w = D.GEOMETRIES[0]
    m = ops.DeformConv2d(c, co, kernel, stride=stride, padding=padding, dilation=dilation, groups=groups).to("meta")
    case = meta_case(D.GEOMETRIES[0], torch.float32)
    assert m.weight.dtype == torch.float32
    out = m(case["input"].to(dtype), case["offset"], case["mask"])              # float32 offset and mask, float32 parameters
    assert out.dtype == dtype and out.shape == (n, co, 9, 11)
    assert m(case["input"].to(dtype), case["offset"]).dtype == dtype
    out = m(case["input"], case["offset"], case["mask"])
    assert out.dtype == torch.float32
    with pytest.raises(TypeError, match=r"offset must be float32.*\.float\(\)"):   # a float32 input casts nothing
        m(case["input"], case["offset"].to(dtype), case["mask"])


# ---- the case helpers -------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("index", range(len(H.GEOMETRIES)), ids=H.IDS)
def test_deform16_ref_is_the_float64_operator_within_the_column_rounding(index, with_mask, dtype):
    """deform16_ref differs from the float64 operator on the widened tensors only by the rounding of the columns to T: 2^-p of each
    column's magnitude, so 2^-p sum |w col| of an output, with the absolute half-spacing in place of 2^-p |col| for a column in T's
    subnormal range (deform16_cases.column_rounding_bound; measured without it: g2, float16, mask: 1.038 times 2^-p sum |w col| on an
    output of two columns of which one is rejected and the other below 2^-14) -- and by its last rounding, checked for itself."""
    case = H.make_case16(H.GEOMETRIES[index], 700 + index, dtype, with_mask=with_mask)
    wide = H.widen(case, torch.float64)
    truth = D.deform_conv2d_ref(wide["input"], wide["offset"], wide["weight"], wide["bias"], mask=wide["mask"], **wide["kw"])
    exact = H.deform16_ref(case, dtype, rounded=False)
    bound = H.column_rounding_bound(case["weight"], H.columns(case, torch.float64), dtype).reshape(truth.shape)
    err = (exact - truth).abs()
    print("%s %s max err / bound %.3f" % (H.IDS[index], dtype, float((err / bound.clamp_min(1e-300)).max())))
    assert float(truth.abs().max()) > 0.1 and bool((err <= bound).all())
    rounded = H.deform16_ref(case, dtype)
    assert rounded.dtype == dtype and torch.equal(rounded, exact.to(dtype))
    assert bool(torch.isfinite(rounded.float()).all()) and float(truth.abs().max()) < 6.0e4          # nothing near float16's 65504


@dtypes
def test_t_accumulation_differs_from_the_float32_accumulation(dtype):
    """The two ways to add chunks that the d_weight test of the GPU suite tells apart do differ, and on many values."""
    parts = [torch.linspace(1.0, 2.0, 4097)] * 3                       # multiples of 2^-12: every sum below is exact in float32
    once, stepwise = H.f32_accumulate(parts, dtype), H.t_accumulate(parts, dtype)
    assert torch.equal(once, (3.0 * parts[0]).to(dtype))
    assert int((once != stepwise).sum()) > 300                        # 341 (float16) and 473 (bfloat16) of 4097
