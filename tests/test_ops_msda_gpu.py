"""fasterrcnn_amd.ops.multi_scale_deformable_attn / MultiScaleDeformableAttention on the GPU against the float64 truth of
tests/msda_cases.py and on the exact properties the kernels promise: the sampling rule at its edges, memory safety whatever the shape
tensors hold, determinism, independence of im2col_step, the 16-bit contract, layouts and empty inputs.

The bound of every comparison with the float64 truth is measured in the same test, as tests/test_ops_deform_gpu.py does:
err(a) = max|a - truth| / max|truth|, err_ref is the error of the explicit restatement run in float32 on the CPU, and
err_gpu <= 4 * max(err_ref, 2**-24) must hold -- both sides are short float32 sums taken in a different order.  max|truth| > 0.1 is
asserted, so nothing is compared against noise.  Each test prints err_gpu, err_ref and their ratio.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: out 1.000 (base, d1-block, d72, chunks), d_value 0.993
(base), d_loc 1.000 (d1-block), d_attn 1.000 (base, d70-scalar); the module against its composition 0.907."""
import functools

import pytest
import torch

from fasterrcnn_amd import ops

from tests import msda_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
HALF = [torch.float16, torch.bfloat16]
MARGIN, FLOOR = 4.0, 2.0 ** -24
LABELS = ("out", "d_value", "d_loc", "d_attn")


def run(value, shapes, starts, loc, attn, grad=None, need=(True, True, True), im2col_step=64, dtype=F32, loc_dtype=F32):
    """(out, d_value, d_loc, d_attn) of the operator on the GPU (a gradient that is not asked for is None); shapes and starts lists."""
    v = value.to(dtype).to(DEV).requires_grad_(need[0])
    lo = loc.to(loc_dtype).to(DEV).requires_grad_(need[1])
    a = attn.to(loc_dtype).to(DEV).requires_grad_(need[2])
    shp = torch.tensor(shapes, dtype=torch.int64, device=DEV).view(-1, 2)
    st = torch.tensor(starts, dtype=torch.int64, device=DEV)
    out = ops.multi_scale_deformable_attn(v, shp, st, lo, a, im2col_step)
    if grad is not None and any(need):
        out.backward(grad.to(dtype).to(DEV))
    return out.detach(), v.grad, lo.grad, a.grad


@functools.lru_cache(maxsize=None)
def gpu_result(name):
    """The float32 GPU result of a case, shared by the tests that compare against it.  Cached: do not modify."""
    return run(*K.case(name))


def within_measured_bound(label, got, truths, singles, names=LABELS):
    worst = 0.0
    for name, g, t, s in zip(names, got, truths, singles):
        assert g.shape == t.shape and float(t.abs().max()) > 0.1, (label, name)
        err_gpu, err_ref = K.rel_err(g.cpu(), t), K.rel_err(s, t)
        ratio = err_gpu / max(err_ref, FLOOR)
        print("%s %-8s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, ratio))
        worst = max(worst, ratio)
        assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, name, err_gpu, err_ref)
    return worst


# ---- 1. against the float64 truth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_forward_and_gradients_against_float64(name):
    truths, singles = K.reference(name)
    got = gpu_result(name)
    assert all(g.dtype == F32 and g.is_contiguous() for g in got)
    within_measured_bound(name, got, truths, singles)


# ---- 2. exact properties ---------------------------------------------------------------------------------------------------------------------
# Small-integer values, power-of-two H and W, coordinates on quarters and power-of-two weights: every product and sum is exact in
# float32, so the GPU must EQUAL the float64 restatement.
EXACT_SHAPES = [(2, 4), (4, 8)]                       # H != W on both levels
EXACT_STARTS = [0, 8]


def exact_case(points, d=4, m=2, seed=0):
    """points: a list of queries, each a list over the two levels of lists of (x, y, weight) in pixel coordinates (one P for all)."""
    gen = torch.Generator().manual_seed(seed)
    q, p = len(points), len(points[0][0])
    value = torch.randint(-8, 9, (1, 40, m, d), generator=gen).to(F64)
    loc = torch.zeros((1, q, m, 2, p, 2), dtype=F64)
    attn = torch.zeros((1, q, m, 2, p), dtype=F64)
    for qi, levels in enumerate(points):
        for l, ((h, w), samples) in enumerate(zip(EXACT_SHAPES, levels)):
            for pi, (x, y, weight) in enumerate(samples):
                loc[0, qi, :, l, pi, 0] = (x + 0.5) / w               # exact: w is a power of two
                loc[0, qi, :, l, pi, 1] = (y + 0.5) / h
                attn[0, qi, :, l, pi] = weight
    attn[:, :, 1] *= 0.5                                              # the second head differs from the first
    grad = torch.randint(-4, 5, (1, q, m * d), generator=gen).to(F64)
    return value, EXACT_SHAPES, EXACT_STARTS, loc, attn, grad


def assert_equals_truth(case, d_loc_too=True):
    truth = K.msda_explicit(case[0], case[1], case[2], case[3], case[4], case[5])
    got = run(*case)
    for name, g, t in zip(LABELS, got, truth):
        if name == "d_loc" and not d_loc_too:
            continue
        assert torch.equal(g.cpu().to(F64), t), name
    return got, truth


def test_a_sample_at_a_cell_centre_returns_that_cell():
    pts = [[[(float(j), float(i), 1.0)], [(float(2 * j + 1), float(i + 2), 2.0)]] for i in range(2) for j in range(4)]
    case = exact_case(pts)
    (out, dv, dloc, dattn), _ = assert_equals_truth(case)
    value = case[0]
    for qi, (i, j) in enumerate((i, j) for i in range(2) for j in range(4)):
        want = value[0, i * 4 + j] + 2.0 * value[0, 8 + (i + 2) * 8 + 2 * j + 1]             # [M, D]
        want[1] *= 0.5
        assert torch.equal(out[0, qi].cpu().to(F64), want.flatten())


def test_the_edges_of_the_sample_test():
    w = 4
    pts = [[[(-1.0, 0.0, 1.0), (float(w), 1.0, 1.0), (w - 0.5, 1.0, 1.0), (-0.5, 0.0, 2.0)], [(0.0, -1.0, 1.0), (3.0, 4.0, 1.0), (2.0, 3.5, 1.0), (7.5, 3.0, 4.0)]]]
    case = exact_case(pts, d=3)                                        # D = 3: the scalar body
    (out, dv, dloc, dattn), _ = assert_equals_truth(case)
    value = case[0]
    # level 0: x = -1 and x = W give 0; x = W - 0.5 counts only its left corner; x = -0.5 only its right corner (cell 0)
    # level 1: y = -1 and y = H give 0; y = H - 0.5 only the upper corner; x = W - 0.5 only the left corner, weight 4
    want = 0.5 * value[0, 1 * 4 + 3] + 2.0 * 0.5 * value[0, 0] + 0.5 * value[0, 8 + 3 * 8 + 2] + 4.0 * 0.5 * value[0, 8 + 3 * 8 + 7]
    want[1] *= 0.5
    assert torch.equal(out[0, 0].cpu().to(F64), want.flatten())
    assert not bool(dattn[0, 0, :, 0, :2].any()) and not bool(dattn[0, 0, :, 1, :2].any()) and not bool(dloc[0, 0, :, :, :2].any())


def test_a_nan_location_gives_zero_and_a_zero_value_gradient():
    case = list(exact_case([[[(1.0, 1.0, 1.0)], [(2.0, 2.0, 1.0)]]]))
    for axis in (0, 1):
        loc = case[3].clone()
        loc[..., axis] = float("nan")
        out, dv, dloc, dattn = run(case[0], case[1], case[2], loc, case[4], case[5])
        assert not bool(out.any()) and not bool(dv.any()) and not bool(dloc.any()) and not bool(dattn.any())
        assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dv).any())


def test_x_and_y_are_not_swapped():
    case = exact_case([[[(2.25, 0.5, 1.0)], [(6.75, 1.25, 2.0)]], [[(0.25, 0.75, 1.0)], [(1.5, 2.5, 1.0)]]])
    (out, _, _, _), truth = assert_equals_truth(case)
    swapped = K.msda_explicit(case[0], case[1], case[2], case[3].flip(-1), case[4])[0]
    assert float((swapped - truth[0]).abs().max()) > 0.5               # the test can tell


def test_zero_weights_on_one_head_zero_exactly_its_channels():
    case = list(exact_case([[[(1.25, 0.5, 1.0)], [(3.5, 1.75, 1.0)]], [[(2.0, 1.0, 1.0)], [(5.25, 2.0, 2.0)]]], m=3, d=5, seed=3))
    case[4][:, :, 1] = 0.0
    (out, dv, _, _), _ = assert_equals_truth(tuple(case))
    out = out.view(1, 2, 3, 5)
    assert not bool(out[:, :, 1].any()) and bool(out[:, :, 0].any()) and bool(out[:, :, 2].any())
    assert not bool(dv[:, :, 1].any()) and bool(dv[:, :, 0].any())


def test_a_level_reads_only_its_own_cells():
    base = exact_case([[[(x + 0.25, y + 0.5, 1.0) for x in (-1, 1, 3)], [(2 * x + 0.75, y + 1.25, 1.0) for x in (-1, 1, 3)]] for y in (-1, 0, 1)])
    for level, (lo, hi) in enumerate(((0, 8), (8, 40))):
        case = list(base)
        case[4] = base[4].clone()
        case[4][:, :, :, 1 - level] = 0.0                             # only `level` counts
        (out, dv, _, _), _ = assert_equals_truth(tuple(case))
        assert bool(dv[:, lo:hi].any()) and not bool(dv[:, :lo].any()) and not bool(dv[:, hi:].any())
        other = case[0].clone()
        other[:, :lo] += 3.0
        other[:, hi:] -= 5.0
        assert torch.equal(run(other, *case[1:5])[0], out)


# ---- 3. memory safety of the shape tensors ---------------------------------------------------------------------------------------------------
def test_more_cells_than_the_levels_cover():
    value, shapes, starts, loc, attn, grad = K.case("base")
    extra = torch.randn((value.shape[0], 7) + tuple(value.shape[2:]), generator=torch.Generator().manual_seed(5), dtype=F32).to(F64)
    got = run(torch.cat([value, extra], 1), shapes, starts, loc, attn, grad)
    ref = gpu_result("base")
    s = value.shape[1]
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    assert torch.equal(got[1][:, :s], ref[1]) and got[1].shape[1] == s + 7 and not bool(got[1][:, s:].any())


def test_one_row_of_cells_short():
    value, shapes, starts, loc, attn, grad = K.case("base")
    short = value[:, :-shapes[-1][1]].contiguous()                    # the last level lacks its last row
    truths = K.msda_explicit(short, shapes, starts, loc.to(F64), attn, grad)
    singles = K.msda_explicit(short.to(F32), shapes, starts, loc, attn.to(F32), grad.to(F32))
    extended = value.clone()
    extended[:, short.shape[1]:] = 0.0
    full = K.msda_explicit(extended, shapes, starts, loc.to(F64), attn, grad)
    assert torch.equal(full[0], truths[0]) and torch.equal(full[1][:, :short.shape[1]], truths[1])    # what "safe" means
    assert float((full[0] - K.reference("base")[0][0]).abs().max()) > 0.01                           # the missing row was in use
    within_measured_bound("base, one row short", run(short, shapes, starts, loc, attn, grad), truths, singles)


def test_shape_tensors_of_garbage_touch_nothing():
    value, shapes, starts, loc, attn, grad = K.case("base")
    for bad_shapes, bad_starts in (([(4, 5), (2 ** 40, 3), (2, 7)], starts), ([(4, 5), (-3, 3), (0, 7)], starts),
                                   (shapes, [0, 2 ** 62, -2 ** 62]), (shapes, [0, value.shape[1] - 2, -3])):
        ok = [h in range(1, 2 ** 24 + 1) and w in range(1, 2 ** 24 + 1) and -2 ** 50 <= st < value.shape[1]
              for (h, w), st in zip(bad_shapes, bad_starts)]
        keep = [l for l in range(len(shapes)) if ok[l]]                # a level the kernels refuse contributes nothing
        truths = K.msda_explicit(value, [bad_shapes[l] for l in keep], [bad_starts[l] for l in keep], loc[:, :, :, keep].to(F64),
                                 attn[:, :, :, keep], grad)
        out, dv, dloc, dattn = run(value, bad_shapes, bad_starts, loc, attn, grad)
        drop = [l for l in range(len(shapes)) if not ok[l]]
        assert not bool(dloc[:, :, :, drop].any()) and not bool(dattn[:, :, :, drop].any())
        assert float((out.cpu().to(F64) - truths[0]).abs().max()) <= 1e-5 * float(truths[0].abs().max())
        assert float((dv.cpu().to(F64) - truths[1]).abs().max()) <= 1e-5 * float(truths[1].abs().max())


# ---- 4. determinism and chunking ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_on_the_long_segment():
    first, again = gpu_result("one-cell"), run(*K.case("one-cell"))
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_im2col_step_changes_no_bit():
    case = K.case("chunks")
    assert case[0].shape[0] == 3
    whole = run(*case, im2col_step=3)
    for step in (1, 2):
        for a, b in zip(whole, run(*case, im2col_step=step)):
            assert torch.equal(a, b), step
    for a, b in zip(whole, gpu_result("chunks")):                      # the default step of 64 is above B
        assert torch.equal(a, b)
    # long segments: image 1's pieces sit at other positions of the sorted plan when it is planned alone
    for a, b in zip(gpu_result("one-cell"), run(*K.case("one-cell"), im2col_step=1)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (True, False, True)])
def test_a_gradient_that_is_not_needed_is_none_and_the_others_are_unchanged(need):
    full = gpu_result("d32-levels")
    got = run(*K.case("d32-levels"), need=need)
    assert torch.equal(got[0], full[0])
    for wanted, g, f in zip(need, got[1:], full[1:]):
        assert (g is None) if not wanted else torch.equal(g, f)


# ---- 5. the 16-bit contract ------------------------------------------------------------------------------------------------------------------
def reordered(got, want, d):
    """d_loc / d_attn of the two element widths: the same float32 terms summed over D in another lane order (8 channels a lane against
    4), so they differ by the rounding of at most D float32 additions: D * 2**-23 of the largest entry is generous."""
    return float((got.to(F64) - want.to(F64)).abs().max()) <= d * 2.0 ** -23 * float(want.abs().max())


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("name", ["base", "d32-levels", "d72"])
def test_the_16_bit_contract_bit_for_bit(name, dtype):
    value, shapes, starts, loc, attn, grad = K.case(name)
    d = value.shape[3]
    v, g = value.to(dtype), grad.to(dtype)
    half = run(v, shapes, starts, loc, attn, g, dtype=dtype)
    wide = run(v.to(F64), shapes, starts, loc, attn, g.to(F64))        # the same 16-bit values, widened
    assert half[0].dtype == dtype and half[1].dtype == dtype and half[2].dtype == F32 and half[3].dtype == F32
    assert torch.equal(half[0], wide[0].to(dtype)) and torch.equal(half[1], wide[1].to(dtype))
    assert reordered(half[2], wide[2], d) and reordered(half[3], wide[3], d)
    assert bool((half[0].float() != wide[0]).any())                    # the store does round
    # locations and weights in the value's own dtype: widened before the launch, their gradients rounded once to that dtype
    lo, a = loc.to(dtype), attn.to(dtype)
    half = run(v, shapes, starts, lo, a, g, dtype=dtype, loc_dtype=dtype)
    wide = run(v.to(F64), shapes, starts, lo.to(F32), a.to(F64), g.to(F64))
    assert [t.dtype for t in half] == [dtype] * 4
    assert torch.equal(half[0], wide[0].to(dtype)) and torch.equal(half[1], wide[1].to(dtype))
    eps = torch.finfo(dtype).eps                                       # one rounding to T (eps / 2) on top of the reordering
    for h, w_ in zip(half[2:], wide[2:]):
        assert float((h.to(F64) - w_.to(F64)).abs().max()) <= (eps / 2 + d * 2.0 ** -23) * float(w_.abs().max())


# ---- 6. layouts, empty inputs, the interface --------------------------------------------------------------------------------------------------
def strided(t):
    """t on the GPU as a non-contiguous view: a slice of a tensor one wider along the last axis."""
    wide = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype, device=DEV)
    view = wide[..., 1:]
    view.copy_(t)
    assert not view.is_contiguous()
    return view


def test_non_contiguous_arguments():
    value, shapes, starts, loc, attn, grad = K.case("d32-levels")
    v = strided(value.to(F32)).requires_grad_(True)
    lo = strided(loc).requires_grad_(True)
    a = strided(attn.to(F32)).requires_grad_(True)
    shp = strided(torch.tensor(shapes, dtype=torch.int64))
    st = torch.tensor(starts, dtype=torch.int64, device=DEV).repeat_interleave(2)[::2]
    assert not st.is_contiguous()
    out = ops.multi_scale_deformable_attn(v, shp, st, lo, a)
    out.backward(strided(grad.to(F32)))
    for got, want in zip((out.detach(), v.grad, lo.grad, a.grad), gpu_result("d32-levels")):
        assert torch.equal(got, want)


@pytest.mark.parametrize("axis", ["B", "Q", "S"])
def test_empty_inputs(axis):
    value, shapes, starts, loc, attn, grad = K.case("chunks")
    if axis == "B":
        value, loc, attn, grad = value[:0], loc[:0], attn[:0], grad[:0]
    elif axis == "Q":
        loc, attn, grad = loc[:, :0], attn[:, :0], grad[:, :0]
    else:
        value = value[:, :0]
    out, dv, dloc, dattn = run(value, shapes, starts, loc, attn, grad)
    assert out.shape == (value.shape[0], loc.shape[1], value.shape[2] * value.shape[3]) and not bool(out.any())
    for g, t in zip((dv, dloc, dattn), (value, loc, attn)):
        assert g.shape == t.shape and not bool(g.any())


def test_apply_takes_mmcvs_positional_arguments_and_double_backward_raises():
    value, shapes, starts, loc, attn, grad = K.case("chunks")
    v = value.to(F32).to(DEV).requires_grad_(True)
    shp, st = (t.to(DEV) for t in K.levels_of(shapes))
    out = ops.MultiScaleDeformableAttnFunction.apply(v, shp, st, loc.to(DEV), attn.to(F32).to(DEV), 2)
    assert torch.equal(out.detach(), gpu_result("chunks")[0])
    dv, = torch.autograd.grad(out, v, grad.to(F32).to(DEV), create_graph=True)
    assert torch.equal(dv.detach(), gpu_result("chunks")[1])
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        dv.sum().backward()


def test_the_module_on_the_gpu_against_its_composition():
    torch.manual_seed(4)
    shapes = [(5, 7), (3, 4), (2, 2)]
    spatial, starts = K.levels_of(shapes)
    mod = ops.MultiScaleDeformableAttention(embed_dims=32, num_heads=4, num_levels=3, num_points=4, dropout=0.0, batch_first=True)
    torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.2)
    torch.nn.init.normal_(mod.attention_weights.weight, std=0.2)
    bs, nq, nv = 2, 11, 51
    query, value = torch.randn(bs, nq, 32), torch.randn(bs, nv, 32)
    mask = torch.zeros(bs, nv, dtype=torch.bool)
    mask[0, :3] = True
    ref = torch.rand(bs, nq, 3, 2)
    call = lambda m, t: m(t(query), value=t(value), key_padding_mask=mask.to(t(query).device), reference_points=t(ref),   # noqa: E731
                          spatial_shapes=spatial.to(t(query).device), level_start_index=starts.to(t(query).device)).detach()
    single = call(mod, lambda t: t)                                    # float32 on the CPU: multi_scale_deformable_attn_pytorch
    got = call(mod.to(DEV), lambda t: t.to(DEV))
    mod = mod.cpu().double()
    truth = call(mod, lambda t: t.double())
    within_measured_bound("module", (got,), (truth,), (single,), names=("out",))
