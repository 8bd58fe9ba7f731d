"""fasterrcnn_amd.ops.box_iou_rotated, nms_rotated and roi_align_rotated on the GPU against the float64 restatements of
tests/rotated_cases.py, against ops.nms and ops.roi_align at angle 0, and on the properties the kernels promise: exact zeros and ones,
one IoU for the pairwise and the NMS kernels, the 16-bit contract, determinism, layouts, flags.

The bound of every comparison with the float64 truth is measured in the same test, as in tests/test_ops_droi_gpu.py:
err(a) = max|a - truth| / max|truth|, err_ref is the error of the same restatement run in float32 on the CPU, and
err_gpu <= 4 * max(err_ref, 2**-24) must hold.  Pooling bins near a seam (rotated_cases.near_seam) send no gradient and are left out of
the output comparisons.  NMS results are exact: the cases keep every pair's float64 IoU 1e-4 away from the threshold.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: IoU 1.41 (near4096), pooled output 1.65, d_input
1.17; at angle 0 against ops.roi_align 1.60.  The largest of all, 1.65, is well inside the margin of 4."""
import functools

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import rotated_cases as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
HALF = [torch.float16, torch.bfloat16]
POOL_NAMES = [n for n in R.POOL_CASES if n != "k0"]


def check_bound(label, got, truth, single):
    """err_gpu <= 4 * max(err_ref, 2**-24); prints both errors; returns the ratio."""
    assert got.shape == truth.shape and got.dtype == F32, label
    assert float(truth.abs().max()) > 0.1, (label, float(truth.abs().max()))
    err_gpu, err_ref = R.rel_err(got.cpu(), truth), R.rel_err(single, truth)
    ratio = err_gpu / max(err_ref, FLOOR)
    print("%s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, err_gpu, err_ref, ratio))
    assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, err_gpu, err_ref)
    return ratio


# ---- 1. box_iou_rotated -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def iou_reference(name, mode):
    b1, b2 = R.iou_case(name)
    return b1, b2, R.iou_matrix(b1, b2, mode, F64), R.iou_matrix(b1, b2, mode, F32)


@pytest.mark.parametrize("mode", ["iou", "iof"])
@pytest.mark.parametrize("name", [n for n in R.IOU_CASES if n != "1x1"])
def test_iou_against_float64(name, mode):
    b1, b2, truth, single = iou_reference(name, mode)
    got = ops.box_iou_rotated(b1.to(DEV), b2.to(DEV), mode=mode)
    assert bool(torch.isfinite(got).all())
    check_bound("%s %s" % (name, mode), got, truth, single)


def test_iou_of_one_pair():
    b1, b2, truth, single = iou_reference("1x1", "iou")
    got = ops.box_iou_rotated(b1.to(DEV), b2.to(DEV))
    assert got.shape == (1, 1) and abs(float(got) - float(truth)) <= MARGIN * max(abs(float(single) - float(truth)), FLOOR)


@pytest.mark.parametrize("name", ["63x63", "64x64", "65x65", "130x130", "special"])
def test_aligned_is_the_diagonal_bit_for_bit(name):
    b1, b2 = (t.to(DEV) for t in R.iou_case(name))
    for mode in ("iou", "iof"):
        full = ops.box_iou_rotated(b1, b2, mode=mode)
        got = ops.box_iou_rotated(b1, b2, mode=mode, aligned=True)
        assert got.shape == (b1.shape[0],) and torch.equal(got, full.diagonal())
    assert float(full.max()) > 0.1


def test_zero_rule_pairs_are_exactly_zero_and_identical_boxes_exactly_one():
    b, _ = R.iou_case("special")
    for mode in ("iou", "iof"):
        m = ops.box_iou_rotated(b.to(DEV), b.to(DEV), mode=mode).cpu()
        rows = list(R.ZERO_RULE_ROWS)
        assert bool(torch.isfinite(m).all()) and not bool(m[rows].any()) and not bool(m[:, rows].any())
        ok = R.box_ok(b)
        assert bool((m.diagonal()[ok] == 1).all()) and float(m[0, 1]) == 1.0 and float(m[3, 4]) == 1.0
        assert float(m[19:21, :19].max()) == 0.0                              # centres 1e4 apart
    for name in ("130x130", "near4096"):
        b = R.iou_case(name)[0].to(DEV)
        assert bool((ops.box_iou_rotated(b, b, aligned=True) == 1).all())


def test_counter_clockwise_is_negated_angles_bit_for_bit():
    b1, b2 = (t.to(DEV) for t in R.iou_case("130x65"))
    flip = lambda b: torch.cat([b[:, :4], -b[:, 4:]], 1)                      # noqa: E731
    want = ops.box_iou_rotated(b1, b2)
    assert torch.equal(ops.box_iou_rotated(flip(b1), flip(b2), clockwise=False), want)
    assert torch.equal(ops.box_iou_rotated(flip(b1), flip(b2), aligned=False, clockwise=False, mode="iof"),
                       ops.box_iou_rotated(b1, b2, mode="iof"))
    # the two conventions differ on boxes that are not symmetric under the flip
    assert not torch.equal(ops.box_iou_rotated(b1, b2, clockwise=False), want)


def test_empty_inputs_give_empty_outputs():
    b = R.iou_case("63x63")[0].to(DEV)
    e = b[:0]
    assert ops.box_iou_rotated(e, b).shape == (0, 63) and ops.box_iou_rotated(b, e).shape == (63, 0)
    assert ops.box_iou_rotated(e, e, aligned=True).shape == (0,)
    assert not ops.box_iou_rotated(b.requires_grad_(True), b).requires_grad


# ---- 2. nms_rotated -------------------------------------------------------------------------------------------------------------------
def run_nms(case, **kw):
    labels = None if case["labels"] is None else case["labels"].to(DEV)
    return ops.nms_rotated(case["boxes"].to(DEV), case["scores"].to(DEV), case["thr"], labels, **kw)


@pytest.mark.parametrize("name", list(R.NMS_CASES))
def test_nms_keeps_what_the_float64_greedy_pass_keeps(name):
    case = R.nms_case(name)
    dets, keep = run_nms(case)
    want = R.nms_ref(case)
    assert keep.dtype == torch.int64 and torch.equal(keep.cpu(), want)
    # dets: the kept boxes with their scores (NaN scores compare as bits)
    assert dets.shape == (want.numel(), 6) and dets.dtype == F32
    assert torch.equal(dets[:, :5].cpu(), case["boxes"][want])
    assert torch.equal(dets[:, 5].cpu().view(torch.int32), case["scores"][want].view(torch.int32))


@pytest.mark.parametrize("name", list(R.NMS_CASES))
def test_nms_is_the_greedy_pass_over_the_gpus_own_iou_matrix(name):
    """No tolerance: the mask kernel and the pairwise kernel share one IoU function and one argument order."""
    case = R.nms_case(name)
    _, keep = run_nms(case)
    order = R.score_order(case["scores"])
    b = case["boxes"][order].to(DEV)
    over = (ops.box_iou_rotated(b, b) > case["thr"]).cpu()
    labels = None if case["labels"] is None else case["labels"][order]
    kept_sorted = R.greedy(over, range(len(order)), labels)
    assert torch.equal(keep.cpu(), torch.tensor(order, dtype=torch.int64)[kept_sorted])


@pytest.mark.parametrize("name", ["n65-angle0", "n300-angle0-labels"])
def test_nms_at_angle_zero_is_ops_nms_on_the_corner_boxes(name):
    case = R.nms_case(name)
    _, keep = run_nms(case)
    corners, scores = R.rotated_to_corners(case["boxes"]).to(DEV), case["scores"].to(DEV)
    if case["labels"] is None:
        want = ops.nms(corners, scores, case["thr"])
    else:
        want = ops.batched_nms(corners, scores, case["labels"].to(DEV), case["thr"])
    assert torch.equal(keep, want)


@pytest.mark.parametrize("name", ["n129-labels", "n300-labels"])
def test_nms_with_labels_is_the_per_label_loop(name):
    case = R.nms_case(name)
    _, keep = run_nms(case)
    parts = []
    for label in case["labels"].unique().tolist():
        idx = (case["labels"] == label).nonzero()[:, 0]
        _, k = ops.nms_rotated(case["boxes"][idx].to(DEV), case["scores"][idx].to(DEV), case["thr"])
        parts.append(idx[k.cpu()])
    merged = torch.cat(parts).sort().values
    merged = merged[torch.tensor(R.score_order(case["scores"][merged]), dtype=torch.int64)]
    assert torch.equal(keep.cpu(), merged)


def test_nms_counter_clockwise_and_empty():
    case = R.nms_case("n129-labels")
    _, keep = run_nms(case)
    flipped = dict(case, boxes=torch.cat([case["boxes"][:, :4], -case["boxes"][:, 4:]], 1))
    dets, keep_ccw = run_nms(flipped, clockwise=False)
    assert torch.equal(keep, keep_ccw) and torch.equal(dets[:, :5].cpu(), flipped["boxes"][keep.cpu()])
    e = torch.empty((0, 5), device=DEV)
    dets, keep = ops.nms_rotated(e, torch.empty((0,), device=DEV), 0.5)
    assert dets.shape == (0, 6) and keep.shape == (0,) and keep.dtype == torch.int64
    dets, keep = ops.nms_rotated(e, torch.empty((0,), device=DEV), 0.5, labels=torch.empty((0,), dtype=torch.int64, device=DEV))
    assert dets.shape == (0, 6) and keep.shape == (0,)


# ---- 3. roi_align_rotated ---------------------------------------------------------------------------------------------------------------
def args_of(case):
    return case["output_size"], case["spatial_scale"], case["sampling_ratio"], case["aligned"], case["clockwise"]


def run(case, dtype=F32, need=True, x_cl=False, grad_cl=True):
    """The operator on the GPU, forward and backward: (output, d_input or None)."""
    x = case["input"].to(DEV).to(dtype)
    x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(need)
    out = ops.roi_align_rotated(x, case["rois"].to(DEV), *args_of(case))
    if out.requires_grad:
        grad = case["grad"].to(DEV).to(dtype)
        out.backward(grad.contiguous(memory_format=CL) if grad_cl else grad.contiguous())
    return out.detach(), x.grad


@functools.lru_cache(maxsize=None)
def pool_reference(name):
    """The case with its float64 truth and the float32 restatement's results (output, d_input), computed once."""
    case = R.pool_case(name)
    return case, (R.forward_ref(case, F64), R.grad_ref(case, F64)), (R.forward_ref(case, F32), R.grad_ref(case, F32))


@pytest.mark.parametrize("name", POOL_NAMES)
def test_pooling_and_gradient_against_float64(name):
    case, truth, single = pool_reference(name)
    R.check_conditions(case)
    out, dx = run(case)
    assert out.is_contiguous(memory_format=CL) or out.shape[1] == 1 or out.shape[2] * out.shape[3] == 1
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
    check_bound(name + " output", R.masked(out, case), R.masked(truth[0], case), R.masked(single[0], case))
    check_bound(name + " d_input", dx, truth[1], single[1])


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("name", ["13x17-c6-7x7", "5x4-c6-adaptive"])
def test_angle_zero_is_roi_align_on_the_corner_boxes(name, aligned):
    case = dict(R.pool_case(name), aligned=aligned)
    rois = case["rois"].clone()
    rois[:, 5] = 0.0
    case["rois"] = rois
    case["seam"] = R.near_seam(case)
    R.check_conditions(case)
    truth, single = R.forward_ref(case, F64), R.forward_ref(case, F32)
    corner = torch.cat([rois[:, :1].double(), R.rotated_to_corners(rois[:, 1:].double())], 1).to(F32)
    # sampling_ratio 0 is adaptive here, -1 in roi_align
    sr = case["sampling_ratio"] if case["sampling_ratio"] > 0 else -1
    for clockwise in (False, True):
        got = ops.roi_align_rotated(case["input"].to(DEV), rois.to(DEV), case["output_size"], case["spatial_scale"],
                                    case["sampling_ratio"], aligned, clockwise)
        check_bound("%s aligned=%s rotated" % (name, aligned), R.masked(got, case), R.masked(truth, case), R.masked(single, case))
    plain = ops.roi_align(case["input"].to(DEV), corner.to(DEV), case["output_size"], case["spatial_scale"], sr, aligned)
    # aligned=False raises a size below one pixel to 1: around the centre here, from x1 / y1 in roi_align -- two different windows, so
    # those RoIs are left out; an adaptive grid may round differently from corner boxes: fixed grids only
    rows = torch.ones((rois.shape[0],), dtype=torch.bool)
    if not aligned:
        rows = (rois[:, 3].double() * case["spatial_scale"] >= 1) & (rois[:, 4].double() * case["spatial_scale"] >= 1)
    assert int(rows.sum()) >= rois.shape[0] // 2
    if case["sampling_ratio"] > 0:
        pick = lambda t: R.masked(t.cpu(), case)[rows]                        # noqa: E731
        check_bound("%s aligned=%s roi_align" % (name, aligned), pick(plain), pick(truth), pick(single))


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["13x17-c6-7x7", "13x17-c8-2x3-adaptive", "5x4-c6-adaptive", "2x2-cull"])
def test_16_bit_maps_equal_the_float32_operator_rounded_once(name, dtype):
    case = dict(R.pool_case(name))
    case["input"] = case["input"].to(dtype).float()                      # the 16-bit values, exactly
    case["grad"] = case["grad"].to(dtype).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=dtype)
    assert out16.dtype == dtype and dx16.dtype == dtype
    assert float(out32.abs().max()) > 0.1 and float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(dtype)) and torch.equal(dx16, dx32.to(dtype))


def test_16_bit_backward_in_wide_runs():
    """C = 512: the backward walks runs of 8 channels (below that, of 4)."""
    gen = torch.Generator().manual_seed(31)
    case = dict(R.pool_case("5x4-c6-adaptive"), input=torch.randn((2, 512, 5, 4), generator=gen).to(torch.bfloat16).float())
    case["grad"] = torch.where(case["seam"][:, None], torch.zeros(()), torch.randn((37, 512, 2, 3), generator=gen)).to(torch.bfloat16).float()
    out32, dx32 = run(case)
    out16, dx16 = run(case, dtype=torch.bfloat16)
    assert float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(torch.bfloat16)) and torch.equal(dx16, dx32.to(torch.bfloat16))


@pytest.mark.parametrize("name", ["2x2-cull", "13x17-c6-7x7"])
def test_two_runs_are_bit_identical(name):
    case = R.pool_case(name)
    first, second = run(case), run(case)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert float(first[1].abs().max()) > 0.1


def test_the_gather_needs_its_second_cull_pass():
    """Every RoI of 2x2-cull reaches the map's one tile, so it lists CULL_LIST RoIs, then one more: the last RoI alone changes d_input."""
    case = R.pool_case("2x2-cull")
    assert case["rois"].shape[0] == ops.ROI_ALIGN_ROTATED_CULL_LIST + 1
    _, dx = run(case)
    _, dx_short = run(dict(case, rois=case["rois"][:-1], grad=case["grad"][:-1]))
    _, dx_last = run(dict(case, rois=case["rois"][-1:], grad=case["grad"][-1:]))
    assert float(dx_last.abs().max()) > 1e-3 and not torch.equal(dx, dx_short)
    # the last RoI's terms are added last, after the sum over the first CULL_LIST: at most one term per (cell, bin), four bins
    want = dx_short.double() + dx_last.double()
    assert float((dx.double() - want).abs().max()) <= 4 * 2.0 ** -23 * float(want.abs().max())


def test_results_do_not_depend_on_the_roi_order_beyond_the_summation_order():
    case = R.pool_case("13x17-c6-7x7")
    out, dx = run(case)
    gen = torch.Generator().manual_seed(7)
    perm = torch.randperm(case["rois"].shape[0], generator=gen)
    out_p, dx_p = run(dict(case, rois=case["rois"][perm], grad=case["grad"][perm]))
    assert torch.equal(out_p, out[perm.to(DEV)])                             # a RoI's row depends on nothing else
    assert float((dx_p - dx).abs().max()) <= 1e-5 * float(dx.abs().max())   # the same terms in another order
    # grouping the RoIs by image keeps every image's ascending order: the same sums, bit for bit
    b = case["rois"][:, 0]
    group = torch.sort(torch.where(torch.isnan(b), torch.full_like(b, 9.0), b), stable=True).indices
    out_g, dx_g = run(dict(case, rois=case["rois"][group], grad=case["grad"][group]))
    assert torch.equal(out_g, out[group.to(DEV)]) and torch.equal(dx_g, dx)


@pytest.mark.parametrize("name", ["13x17-c6-7x7", "13x17-c8-2x3-adaptive"])
def test_layouts_give_the_same_bits_and_gradients_keep_their_format(name):
    case = R.pool_case(name)
    out, dx = run(case)
    assert dx.is_contiguous()
    out_cl, dx_cl = run(case, x_cl=True, grad_cl=False)
    assert dx_cl.is_contiguous(memory_format=CL)
    assert torch.equal(out, out_cl) and torch.equal(dx, dx_cl)


def test_no_gradient_is_computed_for_an_input_that_needs_none():
    case = R.pool_case("13x17-c6-7x7")
    out, dx = run(case)
    out_n, dx_n = run(case, need=False)
    assert dx_n is None and not out_n.requires_grad and torch.equal(out, out_n)
    m = ops.RoIAlignRotated(*args_of(case))
    assert torch.equal(m(case["input"].to(DEV), case["rois"].to(DEV)), out)


def test_invalid_batch_indices_pool_to_zeros_with_zero_gradients():
    case = R.pool_case("13x17-c6-7x7")
    out, dx = run(case)
    for r in R.INVALID_ROWS:
        assert not bool(out[r].any())
    valid = dict(case, grad=case["grad"].clone())
    for r in R.INVALID_ROWS:
        valid["grad"][r] = 0
    assert torch.equal(run(valid)[1], dx)                                  # they send nothing


def test_no_rois_give_an_empty_result_and_a_zero_gradient():
    case = R.pool_case("k0")
    out, dx = run(case)
    assert out.shape == (0, 4, 2, 3) and dx.shape == case["input"].shape and not bool(dx.any())
    lib = nv.lib()
    buf = torch.full((1, 5, 4, 8), float("nan"), device=DEV)
    rc = lib.frcnn_ops_roi_align_rotated_backward(None, 0, 1, 5, 4, 8, 2, 3, 1.0, 2, 1, 0, None, buf.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(buf.any())


def test_c_abi_overwrites_nan_prefilled_buffers():
    """The entry points called directly on NaN-prefilled output and gradient buffers: every element is written, padding included."""
    case = R.pool_case("5x4-c6-adaptive")
    lib = nv.lib()
    n, c, h, w = case["input"].shape
    cp = 8
    oh, ow = case["output_size"]
    k = case["rois"].shape[0]
    x = torch.zeros((n, h, w, cp), device=DEV)
    x[..., :c] = case["input"].to(DEV).permute(0, 2, 3, 1)
    g = torch.zeros((k, oh, ow, cp), device=DEV)
    g[..., :c] = case["grad"].to(DEV).permute(0, 2, 3, 1)
    rois = case["rois"].to(DEV)
    out, dx = torch.full((k, oh, ow, cp), float("nan"), device=DEV), torch.full((n, h, w, cp), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    tail = (case["spatial_scale"], case["sampling_ratio"], int(case["aligned"]), int(case["clockwise"]))
    assert lib.frcnn_ops_roi_align_rotated(x.data_ptr(), n, h, w, cp, rois.data_ptr(), k, oh, ow, *tail, out.data_ptr(), stream) == 0
    assert lib.frcnn_ops_roi_align_rotated_backward(rois.data_ptr(), k, n, h, w, cp, oh, ow, *tail, g.data_ptr(), dx.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    want = run(case)
    assert torch.equal(out[..., :c].permute(0, 3, 1, 2), want[0]) and not bool(out[..., c:].any())
    assert torch.equal(dx[..., :c].permute(0, 3, 1, 2), want[1]) and not bool(dx[..., c:].any())


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes():
    case = R.pool_case("5x4-c6-adaptive")
    x, rois, grad = (case[k].to(DEV) for k in ("input", "rois", "grad"))
    oh, ow = case["output_size"]
    tail = (case["spatial_scale"], oh, ow, case["sampling_ratio"], case["aligned"], case["clockwise"])
    torch.library.opcheck(torch.ops.frcnn.roi_align_rotated.default, (x.clone().requires_grad_(True), rois) + tail, test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.roi_align_rotated_backward.default, (grad, rois) + tail + tuple(x.shape) + (False,),
                          test_utils=OPCHECK)
    b1, b2 = (t.to(DEV) for t in R.iou_case("63x130"))
    torch.library.opcheck(torch.ops.frcnn.box_iou_rotated.default, (b1, b2, 0, False), test_utils=OPCHECK)


def test_double_backward_raises():
    case = R.pool_case("5x4-c6-adaptive")
    x = case["input"].to(DEV).requires_grad_(True)
    out = ops.roi_align_rotated(x, case["rois"].to(DEV), *args_of(case))
    v = case["grad"].to(DEV).requires_grad_(True)                           # the backward is linear in v: a second-order graph exists
    gx, = torch.autograd.grad(out, x, v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()
