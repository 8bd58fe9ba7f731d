"""The float16 / bfloat16 contract of fasterrcnn_amd.ops.deform_conv2d restated on the CPU, for tests/test_ops_deform16_cpu.py and
tests/test_ops_deform16_gpu.py: the cases (tests/deform_conv_cases.py's, rounded to the 16-bit dtype T, plus two shapes that straddle
the tile edges of the 16-bit product), the column matrix, the operator from its contract, and the derived bounds.

Contract (fasterrcnn_amd/ops.py, include/frcnn_hip.h): the column value is the float32 operator's column of the widened tensors, rounded
once to T; out = round_T(float32 sum of the exact products w * col + float(bias)).  P_BITS[T] = p is the number of significant bits of T,
so rounding to nearest changes a value by at most 2^-p of its magnitude."""
import torch

from tests import deform_conv_cases as D

P_BITS = {torch.float16: 11, torch.bfloat16: 8}
DTYPES = (torch.float16, torch.bfloat16)
DTYPE_IDS = ("f16", "bf16")

TILE = 128              # rows and columns of the block tile of csrc/gemm_nt16.hip
# (N, C_in, C_out, groups, G, kernel, stride, padding, dilation, H, W)
SHAPE_A = (3, 4, TILE + 2, 1, 1, (3, 3), (1, 1), (1, 1), (1, 1), 9, 11)    # M = 130 crosses a 128-row tile, K = 36 (two whole MFMA steps
#                                                                             and a masked one of 4 + 4 pad); 297 columns cross the images
SHAPE_B = (1, 40, 8, 1, 2, (3, 3), (1, 1), (0, 0), (1, 1), 7, 7)           # K = 360: 22 reduction steps and a tail; P = 25: a short tail
GEOMETRIES = list(D.GEOMETRIES) + [SHAPE_A, SHAPE_B]
IDS = ["g%d" % i for i in range(len(D.GEOMETRIES))] + ["a", "b"]


def make_case16(geometry, seed, dtype, with_mask=True, with_bias=True, offset_sigma=2.0):
    """deform_conv_cases.make_case with every tensor rounded to `dtype` (and kept in it).  The values are randn, so |out| is of the
    order sqrt(K) <= 20 and a few hundred at most: nothing comes near float16's 65504."""
    return D.cast(D.make_case(geometry, seed, with_mask=with_mask, with_bias=with_bias, offset_sigma=offset_sigma), dtype)


def widen(case, dtype=torch.float32):
    return D.cast(case, dtype)


def columns(case, dtype):
    """The column matrix of the widened case computed in `dtype` on the CPU: [N, groups, K, P], K = (C_in / groups) kh kw."""
    c = widen(case, dtype)
    co, cg, kh, kw = c["weight"].shape
    n, cin = c["input"].shape[:2]
    kwargs = c["kw"]
    _, _, col = D._columns(c["input"], c["offset"], c["mask"], (kh, kw), kwargs["stride"], kwargs["padding"], kwargs["dilation"])
    return col.reshape(n, cin // cg, cg * kh * kw, -1)


def product(weight, col, bias):
    """(sum_k w col + bias, sum_k |w| |col| + |bias|) in float64: [N, C_out, P] each; weight [C_out, C_in / groups, kh, kw], col
    [N, groups, K, P]."""
    groups = col.shape[1]
    co = weight.shape[0]
    w = weight.double().reshape(groups, co // groups, -1)
    value = torch.einsum("gok,ngkp->ngop", w, col.double()).reshape(col.shape[0], co, -1)
    mass = torch.einsum("gok,ngkp->ngop", w.abs(), col.double().abs()).reshape(col.shape[0], co, -1)
    if bias is not None:
        value = value + bias.double()[None, :, None]
        mass = mass + bias.double().abs()[None, :, None]
    return value, mass


def weight_product(grad, col):
    """(d_weight, its mass sum |dout| |col|) in float64, flattened to [C_out, K]: grad [N, C_out, oh, ow], col [N, groups, K, P]."""
    n, groups = col.shape[:2]
    co = grad.shape[1]
    g = grad.double().reshape(n, groups, co // groups, -1)
    value = torch.einsum("ngop,ngkp->gok", g, col.double()).reshape(co, -1)
    mass = torch.einsum("ngop,ngkp->gok", g.abs(), col.double().abs()).reshape(co, -1)
    return value, mass


def deform16_ref(case, dtype, rounded=True):
    """The 16-bit operator from its contract: float32 columns of the widened tensors, rounded to T, the product and the bias in float64,
    rounded to T ([N, C_out, oh, ow]); rounded=False: the float64 value before that last rounding."""
    col16 = columns(case, torch.float32).to(dtype)
    value, _ = product(case["weight"], col16, case["bias"])
    n, _, oh, ow = case["offset"].shape
    value = value.reshape(n, -1, oh, ow)
    return value.to(dtype) if rounded else value


def rounding_unit(dtype):
    return 2.0 ** -P_BITS[dtype]


def rounding_error(value, dtype):
    """One rounding of `value` (float64) to T: at most 2^-p |value| in T's normal range, and half of the subnormal spacing below it, where
    the rounding error is absolute (float16: a value below 2^-14 rounds to a multiple of 2^-24, up to 2^-25 away whatever it is.  The
    exactly rounded float64 truth of g2, float16, without mask and bias has such an output, -4.33e-6, and misses 2^-p |truth| plus the
    float32 sum's term by a factor of 1.49)."""
    tiny = torch.finfo(dtype).tiny
    mag = value.double().abs()
    return torch.where(mag >= tiny, rounding_unit(dtype) * mag, torch.full_like(mag, tiny * rounding_unit(dtype)))


def column_rounding_bound(weight, col, dtype):
    """sum_k |w| e(col): what rounding the columns to T can change an output by, [N, C_out, P] in float64.  e(c) = 2^-p |c| for a column
    in T's normal range -- the whole of the bound 2^-p sum |w col| -- and half of T's subnormal spacing below it, where a rounding error
    is absolute (float16: columns below 2^-14 round to multiples of 2^-24, an error of up to 2^-25 whatever the column; a mask times a
    bilinear sample comes arbitrarily close to zero, and with K = 2 an output can consist of such columns alone)."""
    err = rounding_error(col, dtype)
    groups = col.shape[1]
    co = weight.shape[0]
    w = weight.double().abs().reshape(groups, co // groups, -1)
    return torch.einsum("gok,ngkp->ngop", w, err).reshape(col.shape[0], co, -1)


def sum_bound(terms, mass):
    """The standard bound of a float32 sum of `terms` exact products and a bias (terms + 1 additions, one spare): (terms + 2) 2^-24 mass."""
    return (terms + 2) * 2.0 ** -24 * mass


def t_accumulate(parts, dtype):
    """What adding the parts in T would give: the running sum rounded to T after every addition."""
    acc = parts[0].to(dtype)
    for part in parts[1:]:
        acc = (acc.float() + part.float()).to(dtype)
    return acc


def f32_accumulate(parts, dtype):
    """The contract: the parts added in ascending order in float32, rounded to T once."""
    acc = parts[0].float()
    for part in parts[1:]:
        acc = acc + part.float()
    return acc.to(dtype)
