"""fasterrcnn_amd.ops.dcnv3 / DCNv3Function / DCNv3 on the GPU against the float64 truth of tests/dcnv3_cases.py and on the exact properties
the kernels promise: the sampling rule at its seams, offsets that are not numbers, the box filter and the identity, determinism,
independence of im2col_step, the 16-bit contract, layouts and empty inputs.

The bound of every comparison with the float64 truth is measured in the same test, as tests/test_ops_msda_gpu.py does:
err(a) = max|a - truth| / max|truth|, err_ref is the error of the explicit restatement run in float32 on the CPU, and
err_gpu <= 4 * max(err_ref, 2**-24) must hold -- both sides are short float32 sums taken in a different order.  max|truth| > 0.1 is
asserted, so nothing is compared against noise.  Each test prints err_gpu, err_ref and their ratio.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: out 1.000 (every case), d_input 2.817 (one-cell: 1296
entries on one cell, summed in pieces of the gather's segment), d_offset 2.483 (gc70), d_mask 1.050 (gc32); the module against its
composition 0.639.

Times from one run of tools/ops_bench.py --only dcnv3 on an MI355X (2 x 100 x 160 x 128, G 8, Gc 16, 3 x 3, pad 1; microseconds, ops.dcnv3 /
dcnv3_core_pytorch): float32 forward 62.0 / 590.2, forward + backward 1431.9 / 4428.5; bfloat16 forward 97.2 / 580.7, forward + backward
1590.5 / 14539.9.  Not measured: the backward's split between the plan, the sort and the gather, and any roofline.
"""
import functools

import pytest
import torch

from fasterrcnn_amd import ops

from tests import dcnv3_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
HALF = [torch.float16, torch.bfloat16]
MARGIN, FLOOR = 4.0, 2.0 ** -24
LABELS = K.LABELS


def run(input, offset, mask, geom, grad=None, need=(True, True, True), im2col_step=256, dtype=F32, off_dtype=F32):
    """(out, d_input, d_offset, d_mask) of the operator on the GPU (a gradient that is not asked for is None)."""
    x = input.to(dtype).to(DEV).requires_grad_(need[0])
    off = offset.to(off_dtype).to(DEV).requires_grad_(need[1])
    m = mask.to(off_dtype).to(DEV).requires_grad_(need[2])
    out = ops.DCNv3Function.apply(x, off, m, *geom, im2col_step)
    if grad is not None and any(need):
        out.backward(grad.to(dtype).to(DEV))
    return out.detach(), x.grad, off.grad, m.grad


def run_case(name, **kw):
    input, offset, mask, grad = K.case(name)
    return run(input, offset, mask, K.geom_of(name), grad, **kw)


@functools.lru_cache(maxsize=None)
def gpu_result(name):
    """The float32 GPU result of a case, shared by the tests that compare against it.  Cached: do not modify."""
    return run_case(name)


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


# ---- 2. exact seams ------------------------------------------------------------------------------------------------------------------------------
# Small-integer values, power-of-two masks and scales, coordinates on quarters: every product and sum is exact in float32, so the GPU
# must EQUAL the float64 restatement, gradients included.
EXACT_H, EXACT_W = 4, 8


def exact_case(targets, gc=4, group=2, scale=1.0, seed=0):
    """A 1 x 1 kernel on a 4 x 8 map, so output pixel (oy, ox) owns one sample per group: the first len(targets) pixels, row-major, are
    aimed at the given (x, y, weight); the others keep their own centre with weight 1."""
    gen = torch.Generator().manual_seed(seed)
    input = torch.randint(-8, 9, (1, EXACT_H, EXACT_W, group * gc), generator=gen).to(F64)
    offset = torch.zeros((1, EXACT_H, EXACT_W, group, 1, 2), dtype=F64)
    mask = torch.ones((1, EXACT_H, EXACT_W, group, 1), dtype=F64)
    for i, (x, y, weight) in enumerate(targets):
        oy, ox = divmod(i, EXACT_W)
        offset[0, oy, ox, :, 0, 0] = (x - ox) / scale
        offset[0, oy, ox, :, 0, 1] = (y - oy) / scale
        mask[0, oy, ox, :, 0] = weight
    mask[:, :, :, 1] *= 0.5                                               # the second group differs from the first
    assert torch.equal(offset.to(F32).to(F64), offset)
    grad = torch.randint(-4, 5, (1, EXACT_H, EXACT_W, group * gc), generator=gen).to(F64)
    return input, offset.reshape(1, EXACT_H, EXACT_W, -1), mask.reshape(1, EXACT_H, EXACT_W, -1), \
        K.geometry((1, 1), group=group, gc=gc, scale=scale), grad


def assert_equals_truth(case):
    input, offset, mask, geom, grad = case
    truth = K.with_gradients(K.dcnv3_explicit, input, offset, mask, geom, grad)
    got = run(input, offset, mask, geom, grad)
    for name, g, t in zip(LABELS, got, truth):
        assert torch.equal(g.cpu().to(F64), t), name
    return got


@pytest.mark.parametrize("gc, scale", [(4, 1.0), (3, 0.5), (8, 2.0)])
def test_the_seams_of_the_sample_test(gc, scale):
    w, h = EXACT_W, EXACT_H
    near = -1.0 + 2.0 ** -16                                              # just inside -1: the right corner with weight 2**-16
    targets = [(-1.0, 0.0, 1.0), (float(w), 1.0, 1.0), (w - 1.0, 1.0, 2.0), (-0.75, 0.0, 2.0), (near, 2.0, 4.0), (w - 0.25, 1.0, 1.0),
               (2.0, -1.0, 1.0), (3.0, float(h), 1.0), (2.25, h - 0.5, 1.0), (1.5, -0.25, 4.0), (near, 3.0, 1.0), (w - 1.0, h - 1.0, 1.0),
               (2.75, 1.25, 0.5), (-2.0, 1.0, 1.0), (w + 0.25, 2.0, 1.0)]
    case = exact_case(targets, gc=gc, scale=scale)
    out, dx, doff, dmask = assert_equals_truth(case)
    x = case[0][0].view(h, w, 2, gc)
    o = out[0].cpu().to(F64).view(h, w, 2, gc)
    rejected = [0, 1, 6, 7, 13, 14]                                       # x = -1, x = W, y = -1, y = H and beyond: nothing
    for i in rejected:
        assert not bool(o[divmod(i, w)].any())
        assert not bool(doff.view(h, w, 2, 2)[divmod(i, w)].any()) and not bool(dmask.view(h, w, 2)[divmod(i, w)].any())
    half = torch.tensor([1.0, 0.5], dtype=F64).view(2, 1)
    assert torch.equal(o[0, 2], 2.0 * half * x[1, w - 1])                  # x = W - 1 counts: the left corner whole, the right one 0
    assert torch.equal(o[0, 3], 2.0 * half * 0.25 * x[0, 0])               # x = -0.75: only the right corner, a quarter of cell 0
    assert torch.equal(o[0, 4], 4.0 * half * 2.0 ** -16 * x[2, 0])         # just inside -1
    assert torch.equal(o[0, 5], half * 0.25 * x[1, w - 1])                 # x = W - 0.25: only the left corner
    assert torch.equal(o[1, 2], half * 2.0 ** -16 * x[3, 0]) and bool(o[1, 2].any())
    assert torch.equal(o[1, 3], half * x[h - 1, w - 1])
    assert bool(dmask.view(h, w, 2)[0, 2].any()) and bool(dmask.view(h, w, 2)[0, 4].any())


def test_x_and_y_and_the_point_order_are_not_swapped():
    """A 2 x 3 kernel (kh 2, kw 3) with a one-hot mask on each point in turn, and the offset pair stored as (dx, dy)."""
    input = torch.arange(40, dtype=F64).view(1, 4, 5, 2)
    geom = K.geometry((2, 3), group=1, gc=2)
    for p, (y0, x0) in ((0, (0, 0)), (1, (1, 0)), (2, (0, 1)), (5, (1, 2))):
        mask = torch.zeros((1, 3, 3, 6), dtype=F64)
        mask[..., p] = 1.0
        offset = torch.zeros((1, 3, 3, 6, 2), dtype=F64)
        assert torch.equal(run(input, offset.view(1, 3, 3, 12), mask, geom)[0].cpu().to(F64), input[:, y0:y0 + 3, x0:x0 + 3])
        offset[..., p, 0] = 1.0                                           # one pixel along x
        got = run(input, offset.view(1, 3, 3, 12), mask, geom)[0].cpu().to(F64)
        want = torch.zeros_like(got)
        cols = min(3, 5 - (x0 + 1))
        want[:, :, :cols] = input[:, y0:y0 + 3, x0 + 1:x0 + 1 + cols]
        assert torch.equal(got, want), p


# ---- 3. offsets that are not numbers ---------------------------------------------------------------------------------------------------------
def test_nan_infinite_and_huge_offsets_contribute_nothing_and_keep_the_gradients_finite():
    input, offset, mask, grad = K.case("base")
    geom = K.geom_of("base")
    n, ho, wo = offset.shape[:3]
    bad_off, zero_mask = offset.clone().view(n, ho, wo, 2, 9, 2), mask.clone().view(n, ho, wo, 2, 9)
    values = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30]
    touched = []
    for i, v in enumerate(values):
        for axis in (0, 1):
            at = (i % n, (2 * i + axis) % ho, (3 * i + 1) % wo, axis, (i + 4 * axis) % 9)
            bad_off[at + (axis,)] = v
            zero_mask[at] = 0.0
            touched.append(at)
    bad = run(input, bad_off.view_as(offset), mask, geom, grad)
    ref = run(input, offset, zero_mask.view_as(mask), geom, grad)          # the same samples switched off by their masks
    assert all(bool(torch.isfinite(t).all()) for t in bad)
    assert torch.equal(bad[0], ref[0]) and torch.equal(bad[1], ref[1])
    assert not torch.equal(bad[0], gpu_result("base")[0])                  # the samples were in use
    doff, dmask = bad[2].view(n, ho, wo, 2, 9, 2), bad[3].view(n, ho, wo, 2, 9)
    keep = torch.ones((n, ho, wo, 2, 9), dtype=torch.bool)
    for at in touched:
        assert not bool(doff[at].any()) and float(dmask[at]) == 0.0
        keep[at] = False
    keep = keep.to(DEV)
    assert torch.equal(doff[keep], ref[2].view_as(doff)[keep]) and torch.equal(dmask[keep], ref[3].view_as(dmask)[keep])


# ---- 4. the box filter and the identity, bitwise -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel, stride, pad, dil", K.BOX)
def test_zero_offsets_and_unit_masks_give_the_box_filter_exactly(kernel, stride, pad, dil):
    for gc in (3, 4):
        input, offset, mask, geom, want = K.box_filter_case(kernel, stride, pad, dil, gc=gc)
        assert torch.equal(run(input, offset, mask, geom)[0].cpu().to(F64), want), gc


@pytest.mark.parametrize("kernel, dil", K.IDENTITY)
def test_a_one_hot_centre_mask_returns_the_input_bit_for_bit(kernel, dil):
    for gc in (5, 8):
        input, offset, mask, geom = K.identity_case(kernel, dil, gc=gc)
        assert torch.equal(run(input, offset, mask, geom)[0].cpu(), input), gc
        for dtype in HALF:
            assert torch.equal(run(input, offset, mask, geom, dtype=dtype)[0].cpu(), input.to(dtype)), (gc, dtype)


# ---- 5. determinism and chunking ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "one-cell"])
def test_two_runs_are_bit_identical(name):
    for a, b in zip(gpu_result(name), run_case(name)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["base", "strided", "one-cell"])
def test_im2col_step_changes_no_bit(name):
    n = K.case(name)[0].shape[0]
    assert n == 2
    whole = run_case(name, im2col_step=n)
    for a, b in zip(whole, run_case(name, im2col_step=1)):
        assert torch.equal(a, b)
    for a, b in zip(whole, gpu_result(name)):                              # the default step of 256 is above N
        assert torch.equal(a, b)


def test_three_images_in_chunks_of_two():
    input, offset, mask, grad = (torch.cat([t, t[:1]]) for t in K.case("base"))
    geom = K.geom_of("base")
    whole = run(input, offset, mask, geom, grad)
    for a, b, c in zip(whole, run(input, offset, mask, geom, grad, im2col_step=2), gpu_result("base")):
        assert torch.equal(a, b) and torch.equal(a[:2], c) and torch.equal(a[2], c[0])


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (True, False, True)])
def test_a_gradient_that_is_not_needed_is_none_and_the_others_are_unchanged(need):
    full = gpu_result("strided")
    got = run_case("strided", need=need)
    assert torch.equal(got[0], full[0])
    for wanted, g, f in zip(need, got[1:], full[1:]):
        assert (g is None) if not wanted else torch.equal(g, f)


# ---- 6. the 16-bit contract ------------------------------------------------------------------------------------------------------------------
def reordered(got, want, gc):
    """d_offset / d_mask of the two element widths: the same float32 terms summed over Gc in another lane order (8 channels a lane
    against 4), so they differ by the rounding of at most Gc float32 additions: Gc * 2**-23 of the largest entry is generous."""
    return float((got.to(F64) - want.to(F64)).abs().max()) <= gc * 2.0 ** -23 * float(want.abs().max())


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("name", ["base", "gc6", "gc32", "gc72", "one-cell"])
def test_the_16_bit_contract_bit_for_bit(name, dtype):
    input, offset, mask, grad = K.case(name)
    geom, gc = K.geom_of(name), K.CASES[name][4]
    x, g = input.to(dtype), grad.to(dtype)
    half = run(x, offset, mask, geom, g, dtype=dtype)
    wide = run(x.to(F64), offset, mask, geom, g.to(F64))                   # the same 16-bit values, widened
    assert half[0].dtype == dtype and half[1].dtype == dtype and half[2].dtype == F32 and half[3].dtype == F32
    assert torch.equal(half[0], wide[0].to(dtype)) and torch.equal(half[1], wide[1].to(dtype))
    assert reordered(half[2], wide[2], gc) and reordered(half[3], wide[3], gc)
    assert bool((half[0].float() != wide[0]).any())                        # the store does round


@pytest.mark.parametrize("dtype", HALF)
def test_offsets_and_masks_in_the_inputs_16_bit_dtype(dtype):
    """Widened before the launch, their gradients rounded once to that dtype."""
    input, offset, mask, grad = K.case("base")
    geom, gc = K.geom_of("base"), 8
    x, g, off, m = input.to(dtype), grad.to(dtype), offset.to(dtype), mask.to(dtype)
    half = run(x, off, m, geom, g, dtype=dtype, off_dtype=dtype)
    wide = run(x.to(F64), off.to(F32), m.to(F64), geom, g.to(F64))
    assert [t.dtype for t in half] == [dtype] * 4
    assert torch.equal(half[0], wide[0].to(dtype)) and torch.equal(half[1], wide[1].to(dtype))
    eps = torch.finfo(dtype).eps                                           # one rounding to T (eps / 2) on top of the reordering
    for h, w_ in zip(half[2:], wide[2:]):
        assert float((h.to(F64) - w_.to(F64)).abs().max()) <= (eps / 2 + gc * 2.0 ** -23) * float(w_.abs().max())


# ---- 7. layouts, empty inputs, the interface --------------------------------------------------------------------------------------------------
def strided(t):
    """t on the GPU as a non-contiguous view: a slice of a tensor one wider along the last axis."""
    wide = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype, device=DEV)
    view = wide[..., 1:]
    view.copy_(t)
    assert not view.is_contiguous()
    return view


def test_non_contiguous_arguments():
    input, offset, mask, grad = K.case("strided")
    x = strided(input.to(F32)).requires_grad_(True)
    off = strided(offset).requires_grad_(True)
    m = strided(mask.to(F32)).requires_grad_(True)
    out = ops.dcnv3(x, off, m, (3, 2), (2, 1), (1, 0), (2, 1), 3, 0.5)
    out.backward(strided(grad.to(F32)))
    for got, want in zip((out.detach(), x.grad, off.grad, m.grad), gpu_result("strided")):
        assert torch.equal(got, want)
    # an NCHW tensor seen as channels last: the layout a convolution hands over
    nchw = input.to(F32).permute(0, 3, 1, 2).contiguous().to(DEV)
    assert torch.equal(ops.dcnv3(nchw.permute(0, 2, 3, 1), offset.to(DEV), mask.to(F32).to(DEV), (3, 2), (2, 1), (1, 0), (2, 1), 3, 0.5),
                       gpu_result("strided")[0])


@pytest.mark.parametrize("axis", ["N", "Ho", "Wo"])
def test_empty_inputs(axis):
    n, h, w, pad = {"N": (0, 5, 6, (1, 1)), "Ho": (2, 2, 6, (0, 1)), "Wo": (2, 5, 2, (1, 0))}[axis]
    ho, wo = K.out_size(h, 3, 1, pad[0], 1), K.out_size(w, 3, 1, pad[1], 1)
    assert n * ho * wo == 0
    x = torch.randn(n, h, w, 8, device=DEV, requires_grad=True)
    off = torch.randn(n, ho, wo, 36, device=DEV, requires_grad=True)
    m = torch.randn(n, ho, wo, 18, device=DEV, requires_grad=True)
    out = ops.dcnv3(x, off, m, 3, 1, pad, 1, 2)
    assert out.shape == (n, ho, wo, 8)
    out.sum().backward()
    for t in (x, off, m):
        assert t.grad.shape == t.shape and not bool(t.grad.any())


def test_apply_takes_upstreams_positional_arguments_and_double_backward_raises():
    input, offset, mask, grad = K.case("even")
    x = input.to(F32).to(DEV).requires_grad_(True)
    out = ops.DCNv3Function.apply(x, offset.to(DEV), mask.to(F32).to(DEV), 2, 4, 1, 2, 0, 2, 1, 1, 2, 8, 1.5, 256)
    assert torch.equal(out.detach(), gpu_result("even")[0])
    assert torch.equal(ops.dcnv3(x, offset.to(DEV), mask.to(F32).to(DEV), (2, 4), (1, 2), (0, 2), 1, 2, 1.5).detach(), out.detach())
    dx, = torch.autograd.grad(out, x, grad.to(F32).to(DEV), create_graph=True)
    assert torch.equal(dx.detach(), gpu_result("even")[1])
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        dx.sum().backward()


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes_on_both_ops():
    input, offset, mask, grad = (t.to(F32).to(DEV) for t in K.case("gc3"))
    tail = K.geom_of("gc3") + (256,)
    torch.library.opcheck(torch.ops.frcnn.dcnv3.default, tuple(t.clone().requires_grad_(True) for t in (input, offset, mask)) + tail,
                          test_utils=OPCHECK)
    for needs in ([True, True, True], [True, False, False], [False, True, True]):
        torch.library.opcheck(torch.ops.frcnn.dcnv3_backward.default, (grad, input, offset, mask) + tail + (needs,), test_utils=OPCHECK)


def test_the_module_on_the_gpu_against_its_composition():
    torch.manual_seed(4)
    mod = ops.DCNv3(channels=32, kernel_size=3, pad=1, group=4, offset_scale=1.5)
    torch.nn.init.normal_(mod.offset.weight, std=0.3)
    torch.nn.init.normal_(mod.mask.weight, std=0.3)
    x = torch.randn(2, 7, 9, 32)
    single = mod(x).detach()                                               # float32 on the CPU: dcnv3_core_pytorch
    got = mod.to(DEV)(x.to(DEV)).detach()
    truth = mod.cpu().double()(x.double()).detach()
    within_measured_bound("module", (got,), (truth,), (single,), names=("out",))
