"""fasterrcnn_amd.ops.deform_roi_pool and its modules on the GPU against the float64 restatement (tests/deform_roi_cases.py), against
ops.roi_align(aligned=True), and on the properties the kernels promise: the 16-bit contract, determinism, layouts, flags.

The bound of every comparison with the float64 truth is measured in the same test, as in tests/test_ops_deform_gpu.py:
err(a) = max|a - truth| / max|truth|, err_ref is the error of the same restatement run in float32 on the CPU, and
err_gpu <= 4 * max(err_ref, 2**-24) must hold, with max|truth| > 0.1.  Bins near a seam (deform_roi_cases.near_seam) send no gradient and
are left out of the output and d_offset comparisons.  On a 1 x 1 map the four corners of every sample are one cell, the published
d_offset is identically zero and a relative error has no meaning: there the kernel's d_offset must be exactly zero.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over every case below: output 1.00, d_x 1.14, d_offset 1.05; the Pack
modules' outputs 1.73.  The largest of all, 1.73, is well inside the margin of 4."""
import functools

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import deform_roi_cases as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
FLOOR = 2.0 ** -24
NAMES = [n for n in D.CASES if n != "k0"]
HALF = [torch.float16, torch.bfloat16]


def args_of(case):
    return case["output_size"], case["spatial_scale"], case["sampling_ratio"], case["gamma"]


def run(case, dtype=F32, needs=(True, True), x_cl=False, off_cl=False, grad_cl=True, offset="case", off_dtype=F32, rois=None):
    """The operator on the GPU, forward and backward: (output, d_x or None, d_offset or None)."""
    x = case["input"].to(DEV).to(dtype)
    x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(needs[0])
    off = case["offset"] if isinstance(offset, str) else offset
    if off is not None:
        off = off.to(DEV).to(off_dtype)
        off = (off.contiguous(memory_format=CL) if off_cl else off).requires_grad_(needs[1])
    out = ops.deform_roi_pool(x, case["rois"].to(DEV) if rois is None else rois, off, *args_of(case))
    if out.requires_grad:
        grad = case["grad"].to(DEV).to(dtype)
        out.backward(grad.contiguous(memory_format=CL) if grad_cl else grad.contiguous())
    return out.detach(), x.grad, None if off is None else off.grad


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case with its float64 truth and the float32 restatement's results (output, d_x, d_offset), computed once."""
    case = D.make_case(name)
    truth = (D.forward_ref(case, F64),) + D.grads_ref(case, F64)
    single = (D.forward_ref(case, F32),) + D.grads_ref(case, F32)
    return case, truth, single


def check_against_truth(label, case, got, truth, single, names=("output", "d_x", "d_offset")):
    """err_gpu <= 4 * max(err_ref, 2**-24) for every quantity; prints both errors; returns the ratios."""
    ratios = {}
    one_cell = case["input"].shape[2] * case["input"].shape[3] == 1
    for name, g, t, s in zip(names, got, truth, single):
        assert (g is None) == (t is None), name
        if t is None:
            continue
        assert g.shape == t.shape and g.dtype == F32, name
        g = g.cpu()
        if name != "d_x":
            g, t, s = D.masked(g, case), D.masked(t, case), D.masked(s, case)
        if name == "d_offset" and one_cell:
            assert not bool(t.any()) and not bool(g.any()), label
            continue
        assert float(t.abs().max()) > 0.1, (label, name, float(t.abs().max()))
        err_gpu, err_ref = D.rel_err(g, t), D.rel_err(s, t)
        ratios[name] = err_gpu / max(err_ref, FLOOR)
        print("%s %-9s err_gpu %.3e err_ref %.3e ratio %.3f" % (label, name, err_gpu, err_ref, ratios[name]))
        assert err_gpu <= MARGIN * max(err_ref, FLOOR), (label, name, err_gpu, err_ref)
    return ratios


# ---- 1. output, d_x and d_offset against the float64 restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_gradients_against_float64(name):
    case, truth, single = reference(name)
    D.check_conditions(case)
    out, dx, doff = run(case)
    assert out.is_contiguous(memory_format=CL) or out.shape[1] == 1 or out.shape[2] * out.shape[3] == 1
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
    check_against_truth(name, case, (out, dx, doff), truth, single)


# ---- 2. zero / absent offset is roi_align(aligned=True), bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32] + HALF, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["13x17-none", "13x17-zeros", "5x4-c6-adaptive", "c260-two-images", "1x1-adaptive"])
def test_zero_or_absent_offset_is_aligned_roi_align_bit_for_bit(name, dtype):
    case = D.make_case(name)
    x, rois = case["input"].to(DEV).to(dtype), case["rois"].to(DEV)
    out_size, scale, sr, gamma = args_of(case)
    want = ops.roi_align(x, rois, out_size, scale, sr, aligned=True)
    assert float(want.float().abs().max()) > 0.1
    zeros = torch.zeros((rois.shape[0], 2) + out_size, device=DEV)
    for off in (None, zeros, torch.empty((0,), device=DEV), zeros.to(dtype)):
        got = ops.deform_roi_pool(x, rois, off, out_size, scale, sr, gamma)
        assert got.dtype == dtype and torch.equal(got, want)


# ---- 3. the 16-bit contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["13x17-border", "c260-two-images", "5x4-c6-adaptive", "nonfinite"])
def test_16_bit_maps_equal_the_float32_operator_rounded_once(name, dtype):
    case = dict(D.make_case(name))
    case["input"] = case["input"].to(dtype).float()                      # the 16-bit values, exactly
    case["grad"] = case["grad"].to(dtype).float()
    out32, dx32, doff32 = run(case)
    out16, dx16, doff16 = run(case, dtype=dtype)
    assert out16.dtype == dtype and dx16.dtype == dtype and doff16.dtype == F32
    assert float(out32.abs().max()) > 0.1 and float(dx32.abs().max()) > 0.1
    assert torch.equal(out16, out32.to(dtype)) and torch.equal(dx16, dx32.to(dtype))
    assert torch.equal(doff16, doff32)
    # an offset in the map's dtype is widened for the kernels; its gradient is the float32 run's, rounded once
    case["offset"] = case["offset"].to(dtype).float()
    _, _, doff32 = run(case)
    out_b, dx_b, doff_b = run(case, dtype=dtype, off_dtype=dtype)
    assert doff_b.dtype == dtype and torch.equal(doff_b, doff32.to(dtype))


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c260-cull", "13x17-border"])
def test_two_runs_are_bit_identical(name):
    case = D.make_case(name)
    first, second = run(case), run(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert float(first[1].abs().max()) > 0.1 and float(first[2].abs().max()) > 0.1


def test_the_gather_needs_its_second_cull_pass():
    """Every RoI of c260-cull reaches every tile, so a tile lists CULL_LIST RoIs, then one more: the last RoI alone changes d_x."""
    case = D.make_case("c260-cull")
    assert case["rois"].shape[0] == ops.DEFORM_ROI_CULL_LIST + 1
    _, dx, _ = run(case)
    short = dict(case, rois=case["rois"][:-1], offset=case["offset"][:-1], grad=case["grad"][:-1])
    _, dx_short, _ = run(short)
    last = dict(case, rois=case["rois"][-1:], offset=case["offset"][-1:], grad=case["grad"][-1:])
    _, dx_last, _ = run(last)
    assert float(dx_last.abs().max()) > 0.1
    # one bin per RoI: the sum over all RoIs is the sum over the first CULL_LIST plus the last RoI's one term per cell
    assert torch.equal(dx, dx_short + dx_last)


# ---- 5. other behaviour -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["13x17-border", "c260-two-images"])
def test_layouts_give_the_same_bits_and_gradients_keep_their_format(name):
    case = D.make_case(name)
    out, dx, doff = run(case)
    assert dx.is_contiguous() and doff.is_contiguous()
    out_cl, dx_cl, doff_cl = run(case, x_cl=True, off_cl=True, grad_cl=False)
    assert dx_cl.is_contiguous(memory_format=CL) and doff_cl.is_contiguous(memory_format=CL)
    assert torch.equal(out, out_cl) and torch.equal(dx, dx_cl) and torch.equal(doff, doff_cl)


def test_needs_flags_skip_work():
    case = D.make_case("13x17-border")
    out, dx, doff = run(case)
    out_a, dx_a, doff_a = run(case, needs=(True, False))
    out_b, dx_b, doff_b = run(case, needs=(False, True))
    assert doff_a is None and dx_b is None
    assert torch.equal(out, out_a) and torch.equal(out, out_b) and torch.equal(dx, dx_a) and torch.equal(doff, doff_b)
    out_c, dx_c, doff_c = run(case, needs=(False, False))
    assert dx_c is None and doff_c is None and torch.equal(out, out_c)
    x, rois, off, grad = (case[k].to(DEV) for k in ("input", "rois", "offset", "grad"))
    res = torch.ops.frcnn.deform_roi_pool_backward(grad, x, rois, off, case["spatial_scale"], 7, 7, 2, case["gamma"], [False, True],
                                                   [False, False])
    assert res[0].numel() == 0 and torch.equal(res[1], doff)
    res = torch.ops.frcnn.deform_roi_pool_backward(grad, x, rois, None, case["spatial_scale"], 7, 7, 2, case["gamma"], [True, True],
                                                   [False, False])
    assert res[1].numel() == 0 and res[0].shape == x.shape


def test_roi_list_and_tensor_forms_agree():
    case = D.make_case("13x17-border")
    rois = case["rois"]
    keep = torch.tensor([i for i in range(rois.shape[0]) if float(rois[i, 0]) in (0.0, 1.0)])
    order = torch.cat([keep[rois[keep, 0] == 0], keep[rois[keep, 0] == 1]])
    sub = dict(case, rois=rois[order], offset=case["offset"][order], grad=case["grad"][order])
    out, dx, doff = run(sub)
    boxes = [sub["rois"][sub["rois"][:, 0] == i, 1:].to(DEV) for i in (0, 1)]
    out_l, dx_l, doff_l = run(sub, rois=boxes)
    assert torch.equal(out, out_l) and torch.equal(dx, dx_l) and torch.equal(doff, doff_l)


def test_invalid_batch_indices_pool_to_zeros_with_zero_gradients():
    case = D.make_case("13x17-border")
    out, dx, doff = run(case)
    for r in (9, 11, 13):
        assert not bool(out[r].any()) and not bool(doff[r].any())
    valid = dict(case, grad=case["grad"].clone())
    for r in (9, 11, 13):
        valid["grad"][r] = 0
    assert torch.equal(run(valid)[1], dx)                                  # they send nothing either


def test_no_rois_give_empty_results_and_a_zero_d_x():
    case = D.make_case("k0")
    out, dx, doff = run(case)
    assert out.shape == (0, 4, 3, 5) and doff.shape == (0, 2, 3, 5)
    assert dx.shape == case["input"].shape and not bool(dx.any())
    # the C entry point: OK after zero-filling a NaN-prefilled d_x
    lib = nv.lib()
    buf = torch.full((1, 5, 4, 8), float("nan"), device=DEV)
    rc = lib.frcnn_ops_deform_roi_pool_backward(None, None, None, 0, 1, 5, 4, 8, 3, 5, 1.0, 2, 0.1, None, buf.data_ptr(), None, None, 0,
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(buf.any())


def test_non_finite_offsets_zero_their_bins_and_nothing_else():
    case = D.make_case("nonfinite")
    clean = dict(case, offset=case["offset"].clone(), grad=case["grad"].clone())
    for r, ch, ph, pw in D.NONFINITE_BINS:
        clean["offset"][r, ch, ph, pw] = 0.0
        clean["grad"][r, :, ph, pw] = 0.0
    out, dx, doff = run(case)
    out_c, dx_c, doff_c = run(clean)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(doff).all())
    for r, ch, ph, pw in D.NONFINITE_BINS:
        assert not bool(out[r, :, ph, pw].any()) and not bool(doff[r, :, ph, pw].any())
        out_c[r, :, ph, pw] = 0
        doff_c[r, :, ph, pw] = 0
    assert torch.equal(out, out_c) and torch.equal(dx, dx_c) and torch.equal(doff, doff_c)


def test_c_abi_overwrites_nan_prefilled_buffers():
    """The entry points called directly on NaN-prefilled output and gradient buffers: every element is written."""
    case = D.make_case("5x4-c6-adaptive")
    lib = nv.lib()
    n, c, h, w = case["input"].shape
    cp = 8
    oh, ow = case["output_size"]
    k = case["rois"].shape[0]
    x = torch.zeros((n, h, w, cp), device=DEV)
    x[..., :c] = case["input"].to(DEV).permute(0, 2, 3, 1)
    g = torch.zeros((k, oh, ow, cp), device=DEV)
    g[..., :c] = case["grad"].to(DEV).permute(0, 2, 3, 1)
    rois, off = case["rois"].to(DEV), case["offset"].to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)              # noqa: E731
    out, dx, doff = nan(k, oh, ow, cp), nan(n, h, w, cp), nan(k, 2, oh, ow)
    ws = torch.empty((lib.frcnn_ops_deform_roi_pool_workspace_bytes(k, oh, ow),), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    sr, scale, gamma = case["sampling_ratio"], case["spatial_scale"], case["gamma"]
    assert lib.frcnn_ops_deform_roi_pool(x.data_ptr(), n, h, w, cp, rois.data_ptr(), off.data_ptr(), k, oh, ow, scale, sr, gamma,
                                         out.data_ptr(), stream) == 0
    assert lib.frcnn_ops_deform_roi_pool_backward(x.data_ptr(), rois.data_ptr(), off.data_ptr(), k, n, h, w, cp, oh, ow, scale, sr, gamma,
                                                  g.data_ptr(), dx.data_ptr(), doff.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    torch.cuda.synchronize()
    want = run(case)
    assert torch.equal(out[..., :c].permute(0, 3, 1, 2), want[0]) and not bool(out[..., c:].any())
    assert torch.equal(dx[..., :c].permute(0, 3, 1, 2), want[1]) and not bool(dx[..., c:].any())
    assert torch.equal(doff, want[2])


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes_on_both_ops():
    case = D.make_case("5x4-c6-adaptive")
    x, rois, off, grad = (case[k].to(DEV) for k in ("input", "rois", "offset", "grad"))
    oh, ow = case["output_size"]
    tail = (case["spatial_scale"], oh, ow, case["sampling_ratio"], case["gamma"])
    torch.library.opcheck(torch.ops.frcnn.deform_roi_pool.default, (x.clone().requires_grad_(True), rois, off.clone().requires_grad_(True)) + tail,
                          test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.deform_roi_pool.default, (x, rois, None) + tail, test_utils=OPCHECK)
    for needs in ([True, True], [True, False], [False, True]):
        torch.library.opcheck(torch.ops.frcnn.deform_roi_pool_backward.default, (grad, x, rois, off) + tail + (needs, [False, False]),
                              test_utils=OPCHECK)


def test_double_backward_raises():
    case = D.make_case("5x4-c6-adaptive")
    x = case["input"].to(DEV).requires_grad_(True)
    off = case["offset"].to(DEV).requires_grad_(True)
    out = ops.deform_roi_pool(x, case["rois"].to(DEV), off, *args_of(case))
    gx, = torch.autograd.grad(out, x, case["grad"].to(DEV), create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()


# ---- 6. the Pack modules -----------------------------------------------------------------------------------------------------------------
def pack_case():
    case = D.make_case("13x17-border")
    return case, case["input"].to(DEV), case["rois"].to(DEV)


@pytest.mark.parametrize("cls", [ops.DeformRoIPoolPack, ops.ModulatedDeformRoIPoolPack], ids=["v1", "v2"])
def test_pack_modules_start_as_plain_pooling_and_learn(cls):
    case, x, rois = pack_case()
    out_size, scale, sr, gamma = args_of(case)
    torch.manual_seed(1)
    m = cls(out_size, x.shape[1], deform_fc_channels=32, spatial_scale=scale, sampling_ratio=sr, gamma=gamma).to(DEV)
    plain = ops.roi_align(x, rois, out_size, scale, sr, aligned=True)
    got = m(x, rois)
    assert float(plain.abs().max()) > 0.1
    assert torch.equal(got, plain * 0.5 if cls is ops.ModulatedDeformRoIPoolPack else plain)
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    weight = torch.randn(got.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2))

    def sgd_step():
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        opt.zero_grad()
        (m(x, rois) * weight).sum().backward()
        opt.step()
        return {k for k, v in m.named_parameters() if not torch.equal(v.detach(), before[k])}
    # From the initial state one step moves exactly the zero-initialised last layers: the gradient of every layer before them passes
    # through their weights, which are zero (the chain rule, not the kernels).
    last = {"offset_fc.4.weight", "offset_fc.4.bias"} | ({"mask_fc.2.weight", "mask_fc.2.bias"} if hasattr(m, "mask_fc") else set())
    assert sgd_step() == last
    # From any state with non-zero last layers -- this one -- one SGD step on a random loss changes every parameter.
    assert sgd_step() == {k for k, _ in m.named_parameters()}


@pytest.mark.parametrize("cls", [ops.DeformRoIPoolPack, ops.ModulatedDeformRoIPoolPack], ids=["v1", "v2"])
def test_pack_modules_match_the_restatement_with_the_same_layers(cls):
    case, x, rois = pack_case()
    out_size, scale, sr, gamma = args_of(case)
    oh, ow = out_size
    torch.manual_seed(3)
    m = cls(out_size, x.shape[1], deform_fc_channels=32, spatial_scale=scale, sampling_ratio=sr, gamma=gamma)
    for p in list(m.offset_fc[4].parameters()) + (list(m.mask_fc[2].parameters()) if hasattr(m, "mask_fc") else []):
        torch.nn.init.normal_(p, std=0.05)
    got = m.to(DEV)(x, rois).detach().cpu()
    results = []
    for dtype in (F64, F32):
        ref = m.cpu().to(dtype)
        with torch.no_grad():
            flat = D.forward_ref(dict(case, offset=None), dtype).reshape(rois.shape[0], -1)
            offset = ref.offset_fc(flat).view(-1, 2, oh, ow)
            out = D.forward_ref(dict(case, offset=offset), dtype)
            if hasattr(ref, "mask_fc"):
                out = out * ref.mask_fc(flat).view(-1, 1, oh, ow)
        results.append((out, offset))
    (truth, off64), (single, _) = results
    # the learned offsets move the seams: leave out the bins near one under them
    seam = D.near_seam(dict(case, offset=off64.float()))[:, None]
    assert float(seam.double().mean()) <= 0.05
    zero = torch.zeros(())
    g, t, s = (torch.where(seam, zero.to(v.dtype), v) for v in (got, truth, single))
    assert float(t.abs().max()) > 0.1
    err_gpu, err_ref = D.rel_err(g, t), D.rel_err(s, t)
    print("%s output err_gpu %.3e err_ref %.3e ratio %.3f" % (cls.__name__, err_gpu, err_ref, err_gpu / max(err_ref, FLOOR)))
    assert err_gpu <= MARGIN * max(err_ref, FLOOR), (err_gpu, err_ref)
