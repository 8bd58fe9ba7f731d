"""fasterrcnn_amd.ops.border_align without a GPU: the library exports the entry points under ABI 21 and refuses bad arguments before it
touches a GPU; the wrapper checks its arguments; the fake implementations give the shapes, dtypes and formats; border_align_pytorch (the
composition from torch operations, the CPU route) equals the float64 restatement of tests/border_align_cases.py; and the known answers
hold by hand.

Bounds.  In float64 the composition forms every sample with the restatement's own expressions in the restatement's order, so its output
agrees to a few ulps of float64 (8 * 2**-53 relative to max|truth| is asked; 0 is measured) and d_input, the same terms summed per cell
in another order, to 1e-12.  In float32 it is held to the rule the kernels are held to: err <= 4 * max(err_ref, 2**-24) with err_ref
the float32 mirror's own error."""
import os
import re

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import border_align_cases as B

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = 8 * 2.0 ** -53
SAME_SUMS = 1e-12
MARGIN = 4.0
FLOOR = 2.0 ** -24


def compose(case, dtype):
    x = case["input"].to(dtype).clone().requires_grad_(True)          # the cases are shared: never the tensor itself
    out = ops.border_align_pytorch(x, case["boxes"].to(dtype), case["pool_size"])
    out.backward(case["grad"].to(dtype))
    return out.detach(), x.grad


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_points_under_abi_21():
    text = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert re.search(r"#define FRCNN_ABI_VERSION (\d+)", text).group(1) == "21"
    assert nv.ABI_VERSION == 21 == nv.lib().frcnn_abi_version()
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    ours = {"frcnn_ops_border_align", "frcnn_ops_border_align_backward", "frcnn_ops_border_align_16", "frcnn_ops_border_align_backward_16",
            "frcnn_ops_border_align_cull_list"}
    assert ours <= declared and declared == set(nv.SYMBOLS)
    for name in ours:
        assert hasattr(nv.lib(), name), name


def test_the_constants():
    assert ops.MAX_BORDER_POOL == 64 and ops.MAX_BORDER_SIDE == 2 ** 24 and ops.MAX_BORDER_INDEX == 2 ** 31 - 1 - 1024
    assert ops.BORDER_ALIGN_CULL_LIST == B.CULL_LIST == nv.lib().frcnn_ops_border_align_cull_list()
    for name in ("border_align", "BorderAlign", "border_align_pytorch"):
        assert name in ops.__all__


PTR = 4096                                         # a non-NULL pointer that no refused call dereferences
GOOD = {"n_img": 2, "fh": 5, "fw": 6, "c": 8, "k": 3, "pool": 10}
BAD = [{"n_img": 0}, {"fh": 0}, {"fw": 0}, {"fh": 2 ** 24 + 1}, {"fw": 2 ** 24 + 1}, {"c": 0}, {"c": 6}, {"k": -1}, {"pool": 0}, {"pool": 65},
       {"fh": 2 ** 16, "fw": 2 ** 16}]


def forward(lib, half, a, x=PTR, boxes=PTR, out=PTR, argmax=PTR, elem=nv.OPS_F16):
    args = (x, a["n_img"], a["fh"], a["fw"], a["c"], boxes, a["k"], a["pool"], out, argmax, None)
    return lib.frcnn_ops_border_align_16(elem, *args) if half else lib.frcnn_ops_border_align(*args)


def backward(lib, half, a, boxes=PTR, argmax=PTR, dout=PTR, dx=PTR, elem=nv.OPS_BF16):
    args = (boxes, a["k"], a["n_img"], a["fh"], a["fw"], a["c"], a["pool"], argmax, dout, dx, None)
    return lib.frcnn_ops_border_align_backward_16(elem, *args) if half else lib.frcnn_ops_border_align_backward(*args)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "16"])
def test_the_entry_points_refuse_bad_arguments_before_touching_a_gpu(half):
    lib = nv.lib()
    for bad in BAD:
        a = dict(GOOD, **bad)
        assert forward(lib, half, a) == -1, bad
        assert backward(lib, half, a) == -1, bad
    for null in ("x", "boxes", "out", "argmax"):
        assert forward(lib, half, GOOD, **{null: None}) == -1, null
    for null in ("boxes", "argmax", "dout", "dx"):
        assert backward(lib, half, GOOD, **{null: None}) == -1, null
    assert backward(lib, half, dict(GOOD, k=0), dx=None) == -1
    assert forward(lib, half, dict(GOOD, k=0), None, None, None, None) == 0            # nothing to do: no launch
    # the flat launch grids: lanes n k 4 (c / run) and blocks n ceil(c / run / 64) ceil(fh / 2) ceil(fw / 2)
    assert forward(lib, half, dict(GOOD, n_img=2 ** 15, k=2 ** 15, c=8)) == -1
    assert backward(lib, half, dict(GOOD, n_img=2 ** 10, fh=2 ** 12, fw=2 ** 12)) == -1
    if half:
        assert forward(lib, True, dict(GOOD, c=12)) == -1 and backward(lib, True, dict(GOOD, c=12)) == -1      # whole runs of 8
        assert forward(lib, True, GOOD, elem=7) == -1 and backward(lib, True, GOOD, elem=7) == -1


# ---- the wrapper's argument checks ---------------------------------------------------------------------------------------------------------
def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("args, error, message", [
    ((None, meta(1, 3, 4), 10), TypeError, "input must be a torch.Tensor, got NoneType"),
    ((meta(1, 8, 5, 6, dtype=F64), meta(1, 3, 4), 10), TypeError, "input must be float32, float16 or bfloat16, got torch.float64"),
    ((meta(1, 8, 5, 6), [[1, 2, 3, 4]], 10), TypeError, "boxes must be a torch.Tensor, got list"),
    ((meta(1, 8, 5, 6), meta(1, 3, 4, dtype=F64), 10), TypeError, "boxes must be float32, got torch.float64"),
    ((meta(1, 8, 5, 6), meta(1, 3, 4, dtype=torch.float16), 10), TypeError, "boxes must be float32, got torch.float16"),
    ((meta(1, 8, 5, 6, dtype=torch.float16), meta(1, 3, 4, dtype=torch.bfloat16), 10), TypeError,
     "boxes must be float32 or the input's torch.float16, got torch.bfloat16"),
    ((meta(8, 5, 6), meta(1, 3, 4), 10), ValueError, "input must be [N, 4 C, H, W], got shape (8, 5, 6)"),
    ((meta(1, 6, 5, 6), meta(1, 3, 4), 10), ValueError, "input must have 4 C channels (top, left, bottom, right groups of C), got 6"),
    ((meta(2, 8, 5, 6), meta(1, 3, 4), 10), ValueError, "boxes must be [N, K, 4] (x1, y1, x2, y2) with N = 2, got shape (1, 3, 4)"),
    ((meta(1, 8, 5, 6), meta(1, 3, 5), 10), ValueError, "boxes must be [N, K, 4] (x1, y1, x2, y2) with N = 1, got shape (1, 3, 5)"),
    ((meta(1, 8, 5, 6), meta(3, 4), 10), ValueError, "boxes must be [N, K, 4] (x1, y1, x2, y2) with N = 1, got shape (3, 4)"),
    ((meta(1, 8, 5, 6), meta(1, 3, 4), 10.0), TypeError, "pool_size must be an int, got 10.0"),
    ((meta(1, 8, 5, 6), meta(1, 3, 4), True), TypeError, "pool_size must be an int, got True"),
    ((meta(1, 8, 5, 6), meta(1, 3, 4), 0), ValueError, "pool_size must lie in [1, 64], got 0"),
    ((meta(1, 8, 5, 6), meta(1, 3, 4), 65), ValueError, "pool_size must lie in [1, 64], got 65"),
    ((meta(1, 4, 2 ** 24 + 1, 1), meta(1, 3, 4), 10), ValueError, "input: H and W must be <= 16777216, got 16777217 x 1"),
    ((meta(2 ** 15, 8, 5, 6), meta(2 ** 15, 2 ** 15, 4), 10), ValueError,
     "N K 4 ceil(C / 4) = 4294967296 exceeds 2147482623 (the forward's launch grid)"),
    ((meta(2 ** 10, 4, 2 ** 12, 2 ** 12), meta(2 ** 10, 3, 4), 10), ValueError,
     "N ceil(C / 256) ceil(H / 2) ceil(W / 2) = 4294967296 exceeds 2147482623 (the backward's launch grid)"),
])
def test_every_validation_error_and_its_message(args, error, message):
    with pytest.raises(error) as info:
        ops.border_align(*args)
    assert str(info.value) == message


def test_a_cpu_tensor_names_the_fallback_and_devices_must_match():
    with pytest.raises(ValueError) as info:
        ops.border_align(torch.zeros(1, 8, 5, 6), torch.zeros(1, 3, 4), 10)
    assert str(info.value) == ("input must be a tensor on the GPU, got device cpu: fasterrcnn_amd.ops has no CPU implementation "
                               "(border_align_pytorch runs on any device)")
    with pytest.raises(ValueError, match="boxes must be a tensor on the GPU.*border_align_pytorch runs on any device"):
        ops.border_align(meta(1, 8, 5, 6), torch.zeros(1, 3, 4), 10)
    with pytest.raises(ValueError, match="pool_size must lie in"):
        ops.BorderAlign(0)
    for bad, error in (((torch.zeros(1, 8, 5, 6).long(), torch.zeros(1, 3, 4), 10), TypeError),
                       ((torch.zeros(1, 6, 5, 6), torch.zeros(1, 3, 4), 10), ValueError),
                       ((torch.zeros(1, 8, 5, 6), torch.zeros(2, 3, 4), 10), ValueError),
                       ((torch.zeros(1, 8, 5, 6), torch.zeros(1, 3, 4), 0), ValueError)):
        with pytest.raises(error):
            ops.border_align_pytorch(*bad)


def test_the_module_has_mmcvs_repr():
    assert repr(ops.BorderAlign(10)) == "BorderAlign(pool_size=10)"
    assert ops.BorderAlign(7).pool_size == 7


# ---- fake and meta shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, torch.float16, torch.bfloat16])
def test_fake_and_meta_shapes_dtypes_and_formats(dtype):
    x, boxes = meta(2, 12, 5, 6, dtype=dtype), meta(2, 7, 4)
    out = ops.border_align(x, boxes, 10)
    assert out.shape == (2, 3, 7, 4) and out.dtype == dtype and out.is_contiguous(memory_format=torch.channels_last)
    out, argmax = torch.ops.frcnn.border_align(x, boxes, 10)
    assert argmax.shape == (2, 3, 7, 4) and argmax.dtype == torch.int32 and out.dtype == dtype
    assert ops.border_align(x, meta(2, 7, 4, dtype=dtype), 10).dtype == dtype          # boxes in the map's own 16-bit dtype
    for channels_last in (False, True):
        dx = torch.ops.frcnn.border_align_backward(out, boxes, argmax, 10, 5, 6, channels_last)
        assert dx.shape == (2, 12, 5, 6) and dx.dtype == dtype
        assert dx.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert ops.border_align(meta(2, 12, 5, 6, dtype=dtype), meta(2, 0, 4), 10).shape == (2, 3, 0, 4)


# ---- the composition against the truth --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.TOLERANCE_CASES)
def test_the_cases_meet_the_argmax_condition(name):
    case, truth, mirror = B.make_case(name)
    B.check_conditions(case, truth, mirror)
    assert torch.equal(truth[0], truth[3].gather(-1, truth[1][..., None])[..., 0])     # the output is the sample the argmax names


@pytest.mark.parametrize("name", B.TOLERANCE_CASES)
def test_the_composition_equals_the_truth_in_float64(name):
    case, truth, _ = B.make_case(name)
    out, dx = compose(case, F64)
    assert out.dtype == F64 and out.shape == truth[0].shape and dx.shape == truth[2].shape
    assert B.rel_err(out, truth[0]) <= ULPS and B.rel_err(dx, truth[2]) <= SAME_SUMS


@pytest.mark.parametrize("name", B.TOLERANCE_CASES)
def test_the_composition_meets_the_tolerance_rule_in_float32(name):
    case, truth, mirror = B.make_case(name)
    got = compose(case, F32)
    for what, g, t, m in zip(("output", "d_input"), got, (truth[0], truth[2]), (mirror[0], mirror[2])):
        assert g.dtype == F32 and float(t.abs().max()) > 0.1
        err, err_ref = B.rel_err(g, t), B.rel_err(m, t)
        print("%s %-8s err %.3e err_ref %.3e ratio %.3f" % (name, what, err, err_ref, err / max(err_ref, FLOOR)))
        assert err <= MARGIN * max(err_ref, FLOOR), (name, what, err, err_ref)


def test_16_bit_maps_compute_in_float32_and_round_once():
    case, _, _ = B.make_case("c3-two-images-random")
    for dtype in (torch.float16, torch.bfloat16):
        x = case["input"].to(dtype)
        want = ops.border_align_pytorch(x.float(), case["boxes"], case["pool_size"]).to(dtype)
        got = ops.border_align_pytorch(x, case["boxes"].to(dtype).float(), case["pool_size"])
        assert got.dtype == dtype
        assert torch.equal(ops.border_align_pytorch(x, case["boxes"], case["pool_size"]), want)


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
def test_a_constant_map_ties_everywhere_argmax_0():
    case, truth, _ = B.make_case("constant")
    out, arg, dx, vals = truth
    assert bool((out == 1.5).all()) and not bool(arg.any())
    got, got_dx = compose(case, F64)
    assert bool((got == 1.5).all())
    assert abs(float(got_dx.sum()) - float(case["grad"].double().sum())) < 1e-9      # every box inside the map: the weights sum to 1
    assert torch.allclose(got_dx, dx, rtol=0, atol=1e-12)


def test_a_single_maximum_at_the_last_sample():
    """Box (1, 2, 6, 4.5), pool_size 10, the map 2.0 at (y 2, x 6) and 0 elsewhere: the top edge's samples are x = 1, 1.5, .., 6 at y = 2 and
    only the last one, exactly on the cell, sees 2.0 (x = 5.5 sees half of it): out 2.0, argmax 10, the whole gradient on that cell.  The
    right edge starts at (6, 4.5) and steps up to (6, 2): its last sample is the same point.  Left and bottom never meet it: 0, argmax 0."""
    case, truth, _ = B.make_case("last-maximum")
    out, arg, dx, _ = truth
    got, got_dx = compose(case, F64)
    for o in (out, got):
        assert o[0, 0, 0].tolist() == [2.0, 0.0, 0.0, 2.0]
    assert arg[0, 0, 0].tolist() == [10, 0, 0, 10]
    g = case["grad"][0, 0, 0].double()
    want = torch.zeros_like(dx)
    want[0, 0, B.PEAK[0], B.PEAK[1]] = g[0]
    want[0, 3, B.PEAK[0], B.PEAK[1]] = g[3]
    want[0, 1, 2, 1] = g[1]                          # left: sample 0 at (1, 2), exactly on a cell
    want[0, 2, 4, 6] = g[2] * 0.5                    # bottom: sample 0 at (6, 4.5), between rows 4 and 5 of the last column
    want[0, 2, 5, 6] = g[2] * 0.5
    assert torch.equal(dx, want) and torch.allclose(got_dx, want, rtol=0, atol=1e-15)


def test_zero_stride_edges_keep_sample_0_and_an_inverted_box_is_simply_sampled():
    case, truth, _ = B.make_case("degenerate")
    out, arg, dx, vals = truth
    for row, edges in B.ZERO_STRIDE["degenerate"].items():
        for e in edges:
            assert not bool(arg[0, :, row, e].any())
            assert bool((vals[0, :, row, e] == vals[0, :, row, e, :1]).all())
    assert bool(arg[0, :, 1].any())                                                  # the inverted box: sampled backwards, not rejected
    # the zero-area box: all four edges sit on one point, whose four cells get the whole gradient of the box's group channels
    alone = dict(case, boxes=case["boxes"][:, 4:5], grad=case["grad"][:, :, 4:5])
    _, dx_alone = compose(alone, F64)
    x, y = float(case["boxes"][0, 4, 0]), float(case["boxes"][0, 4, 1])
    cells = torch.zeros_like(dx_alone, dtype=torch.bool)
    cells[:, :, int(y):int(y) + 2, int(x):int(x) + 2] = True
    assert not bool(dx_alone[~cells].any())
    assert abs(float(dx_alone.sum()) - float(alone["grad"].double().sum())) < 1e-12


def test_non_finite_boxes_give_zeros_beside_an_unchanged_normal_box():
    case = B.nonfinite_case()
    out, arg, dx, _ = B.reference(case, F64)
    alone = dict(case, boxes=case["boxes"][:, :1], grad=case["grad"][:, :, :1])
    out_a, _, dx_a, _ = B.reference(alone, F64)
    assert float(out_a.abs().max()) > 0.1 and float(dx_a.abs().max()) > 0.1
    assert torch.equal(out[:, :, :1], out_a) and torch.equal(dx, dx_a) and not bool(out[:, :, 1:].any()) and not bool(arg[:, :, 1:].any())
    got, got_dx = compose(case, F64)
    assert torch.equal(got, out) and B.rel_err(got_dx, dx) <= SAME_SUMS


def test_a_nan_pixel_stays_at_sample_0_and_never_wins_later():
    case = B.nan_pixel_case()
    out, arg, dx, vals = B.reference(case, F64)
    assert bool(torch.isnan(out[0, :, 0, :2]).all()) and not bool(arg[0, :, 0, :2].any())      # i = 0 of box 0's top and left edges
    assert bool(torch.isnan(vals[0, :, 1, 0, 2]).all()) and not bool(torch.isnan(out[0, :, 1:]).any())
    assert not bool((arg[0, :, 1, 0] == 2).any())
    got, got_dx = compose(case, F64)
    assert torch.equal(torch.isnan(got), torch.isnan(out)) and torch.equal(got.nan_to_num(7.0), out.nan_to_num(7.0))
    assert torch.allclose(got_dx, dx, rtol=0, atol=1e-12, equal_nan=True)


def test_empty_inputs_give_empty_results_and_a_zero_gradient():
    for shape, k in (((2, 8, 5, 6), 0), ((0, 8, 5, 6), 3), ((2, 0, 5, 6), 3)):
        x = torch.zeros(shape, requires_grad=True)
        out = ops.border_align_pytorch(x, torch.zeros((shape[0], k, 4)), 10)
        assert out.shape == (shape[0], shape[1] // 4, k, 4)
        out.sum().backward()
        assert x.grad.shape == x.shape and not bool(x.grad.any())
