"""fasterrcnn_amd.ops.deform_roi_pool without a GPU: the restatement of tests/deform_roi_cases.py checks itself (its explicit gradients
against autograd of its own forward, zero offsets against aligned RoIAlign, the near-seam conditions of every case), and the wrapper,
the modules and the C entry points check their arguments."""
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import deform_roi_cases as D

F64 = torch.float64
NAMES = [n for n in D.CASES if n != "k0"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.CASES))
def test_near_seam_conditions_hold(name):
    case = D.make_case(name)
    fraction = D.check_conditions(case)
    print("%s: %.2f %% of the bins are near a seam" % (name, 100 * fraction))
    assert not bool(case["grad"][case["seam"][:, None].expand_as(case["grad"])].any())


@pytest.mark.parametrize("name", NAMES)
def test_explicit_gradients_equal_autograd_of_the_restated_forward(name):
    case = D.make_case(name)
    x = case["input"].to(F64).requires_grad_(True)
    off = None if case["offset"] is None else case["offset"].to(F64).requires_grad_(True)
    D.forward_ref(case, F64, offset=off, input=x).backward(case["grad"].to(F64))
    dx, doff = D.grads_ref(case, F64)
    assert float(dx.abs().max()) > 0.1
    assert D.rel_err(dx, x.grad) < 1e-12
    if off is None:
        assert doff is None
        return
    # the published formula is the derivative where no sample is clamped: strictly inside (0, size - 1); the non-finite bins have none
    inner = D.interior(case) & ~case["seam"]
    if case["input"].shape[2] * case["input"].shape[3] == 1:
        assert not bool(inner.any()) and not bool(doff.any())              # a 1 x 1 map: all four corners are one cell
        return
    assert int(inner.sum()) >= 5, int(inner.sum())
    sel = inner[:, None].expand_as(doff)
    got, want = doff[sel], torch.nan_to_num(off.grad)[sel]
    assert float(want.abs().max()) > 0.01
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name", ["13x17-zeros", "13x17-none", "5x4-c6-adaptive", "1x1-adaptive"])
def test_zero_offset_is_the_restated_aligned_roi_align(name):
    """forward_ref at a zero / absent offset against aligned RoIAlign restated on its own (one product grid of samples per RoI, no
    per-bin start): the same products, summed per bin over the same samples, so the two agree to a few roundings."""
    case = D.make_case(name)
    zero = dict(case, offset=None if case["offset"] is None else torch.zeros_like(case["offset"]))
    for dtype, tol in ((F64, 2.0 ** -48), (torch.float32, 2.0 ** -20)):
        got, want = D.forward_ref(zero, dtype), D.roi_align_ref(case, dtype)
        assert got.shape == want.shape and float(want.abs().max()) > 0.1
        assert D.rel_err(got, want) <= tol, (name, dtype, D.rel_err(got, want))
    assert not bool(D.roi_align_ref(case, F64)[[9, 11, 13]].any())          # invalid batch indices pool to zeros


def test_non_finite_offsets_zero_their_bins_only():
    case = D.make_case("nonfinite")
    clean = dict(case, offset=case["offset"].clone())
    for r, ch, ph, pw in D.NONFINITE_BINS:
        clean["offset"][r, ch, ph, pw] = 0.0
    out, ref = D.forward_ref(case, F64), D.forward_ref(clean, F64)
    (dx, doff), (dx_ref, doff_ref) = D.grads_ref(case, F64), D.grads_ref(clean, F64)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(doff).all())
    for r, ch, ph, pw in D.NONFINITE_BINS:
        assert not bool(out[r, :, ph, pw].any()) and not bool(doff[r, :, ph, pw].any())
        ref[r, :, ph, pw] = 0
        doff_ref[r, :, ph, pw] = 0
    assert torch.equal(out, ref) and torch.equal(doff, doff_ref)


# ---- modules ------------------------------------------------------------------------------------------------------------------------------
def test_pack_modules_parameters_initialisation_repr_and_state_dict():
    torch.manual_seed(0)
    m = ops.DeformRoIPoolPack((3, 5), 6, deform_fc_channels=16, spatial_scale=1 / 16, sampling_ratio=2, gamma=0.2)
    names = [k for k, _ in m.named_parameters()]
    assert names == ["offset_fc.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias")]
    assert m.offset_fc[0].weight.shape == (16, 3 * 5 * 6) and m.offset_fc[4].weight.shape == (3 * 5 * 2, 16)
    assert not bool(m.offset_fc[4].weight.any()) and not bool(m.offset_fc[4].bias.any()) and bool(m.offset_fc[2].weight.any())
    text = repr(m)
    for part in ("DeformRoIPoolPack(", "output_size=(3, 5)", "spatial_scale=0.0625", "sampling_ratio=2", "gamma=0.2", "output_channels=6",
                 "deform_fc_channels=16", "offset_fc"):
        assert part in text, (part, text)
    v2 = ops.ModulatedDeformRoIPoolPack(7, 4, deform_fc_channels=8)
    names = [k for k, _ in v2.named_parameters()]
    assert names == ["offset_fc.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias")] + \
        ["mask_fc.%d.%s" % (i, p) for i in (0, 2) for p in ("weight", "bias")]
    assert v2.output_size == (7, 7) and v2.mask_fc[2].weight.shape == (49, 8) and isinstance(v2.mask_fc[3], torch.nn.Sigmoid)
    assert not bool(v2.mask_fc[2].weight.any()) and not bool(v2.mask_fc[2].bias.any()) and not bool(v2.offset_fc[4].weight.any())
    assert "ModulatedDeformRoIPoolPack(" in repr(v2) and "mask_fc" in repr(v2) and "gamma=0.1" in repr(v2)
    plain = ops.DeformRoIPool((2, 3), 0.25, 2, 0.5)
    assert repr(plain) == "DeformRoIPool(output_size=(2, 3), spatial_scale=0.25, sampling_ratio=2, gamma=0.5)"
    assert not list(plain.parameters())
    # state_dict round trip, strict
    for p in v2.parameters():
        torch.nn.init.normal_(p)
    other = ops.ModulatedDeformRoIPoolPack(7, 4, deform_fc_channels=8)
    result = other.load_state_dict(v2.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for (ka, a), (kb, b) in zip(v2.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(a, b)


def test_ops_are_registered_with_fake_implementations():
    x = torch.empty((2, 6, 5, 4), device="meta").requires_grad_(True)
    rois = torch.empty((3, 5), device="meta")
    off = torch.empty((3, 2, 3, 5), device="meta").requires_grad_(True)
    out = ops.deform_roi_pool(x, rois, off, (3, 5), 0.5, 2, 0.1)
    assert out.shape == (3, 6, 3, 5) and out.is_contiguous(memory_format=torch.channels_last)
    out.sum().backward()
    assert x.grad.shape == x.shape and off.grad.shape == off.shape
    assert ops.deform_roi_pool(x, rois, None, (3, 5)).shape == (3, 6, 3, 5)
    assert ops.deform_roi_pool(x, rois, torch.empty((0,), device="meta"), (3, 5)).shape == (3, 6, 3, 5)
    assert ops.DEFORM_ROI_CULL_LIST == D.CULL_LIST == nv.lib().frcnn_ops_deform_roi_pool_cull_list()
    assert "deform_roi_pool" in ops.__all__ and "ModulatedDeformRoIPoolPack" in ops.__all__


# ---- the wrapper's argument checks -----------------------------------------------------------------------------------------------------
def test_wrapper_rejects_cpu_tensors_and_bad_arguments():
    x = torch.zeros((1, 4, 5, 4), device="meta")
    rois = torch.zeros((3, 5), device="meta")
    off = torch.zeros((3, 2, 2, 2), device="meta")
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.deform_roi_pool(torch.zeros((1, 4, 5, 4)), torch.zeros((3, 5)), None, 2)
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.deform_roi_pool(x, rois, torch.zeros((3, 2, 2, 2)), 2)
    with pytest.raises(TypeError):
        ops.deform_roi_pool(x, rois, [0.0], 2)
    with pytest.raises(TypeError):
        ops.deform_roi_pool(x, rois, off.double(), 2)
    with pytest.raises(TypeError):
        ops.deform_roi_pool(x, rois, off.half(), 2)                        # a 16-bit offset goes with a map of its dtype only
    with pytest.raises(TypeError):
        ops.deform_roi_pool(x.double(), rois, off, 2)
    with pytest.raises(TypeError):
        ops.deform_roi_pool(x, rois, off, 2.5)
    assert ops.deform_roi_pool(x.half(), rois, off.half(), 2).dtype == torch.float16
    assert ops.deform_roi_pool(x.bfloat16(), rois, off, 2).dtype == torch.bfloat16
    for bad in (torch.zeros((3, 2, 2, 3), device="meta"), torch.zeros((2, 2, 2, 2), device="meta"), torch.zeros((3, 1, 2, 2), device="meta"),
                torch.zeros((3, 8), device="meta")):
        with pytest.raises(ValueError, match="offset must be"):
            ops.deform_roi_pool(x, rois, bad, 2)
    with pytest.raises(ValueError):
        ops.deform_roi_pool(x, rois, None, 0)
    with pytest.raises(ValueError):
        ops.deform_roi_pool(x, rois, None, ops.MAX_OUTPUT + 1)
    with pytest.raises(ValueError, match="sampling_ratio"):
        ops.deform_roi_pool(x, rois, off, 2, sampling_ratio=ops.MAX_SAMPLING_RATIO + 1)
    with pytest.raises(ValueError):
        ops.deform_roi_pool(x, torch.zeros((3, 4), device="meta"), None, 2)
    with pytest.raises(ValueError):
        ops.deform_roi_pool(x[0], rois, None, 2)
    with pytest.raises(ValueError, match="output_channels"):
        ops.DeformRoIPoolPack(2, 8, deform_fc_channels=4)(x, rois)


# ---- FRCNN_EINVAL of the entry points, with null pointers and no device ------------------------------------------------------------------
P = 0x1000          # a non-null pointer that is never dereferenced: every call below fails its validation first
GOOD = dict(n_img=1, fh=5, fw=4, c=8, k=3, out_h=2, out_w=2, sampling_ratio=2)
BAD = [dict(out_h=0), dict(out_h=65), dict(out_w=0), dict(out_w=65), dict(sampling_ratio=17), dict(k=-1), dict(n_img=0), dict(fh=0),
       dict(fw=0), dict(c=0), dict(c=6), dict(fh=65536, fw=65536), dict(k=2 ** 30, out_h=2, out_w=2), dict(n_img=65536),
       dict(fh=131071, fw=1)]


def forward(lib, half, a, x=P, rois=P, offset=None, out=P, elem=nv.OPS_F16):
    args = (x, a["n_img"], a["fh"], a["fw"], a["c"], rois, offset, a["k"], a["out_h"], a["out_w"], 0.5, a["sampling_ratio"], 0.1, out, None)
    return lib.frcnn_ops_deform_roi_pool_16(elem, *args) if half else lib.frcnn_ops_deform_roi_pool(*args)


def backward(lib, half, a, x=P, rois=P, offset=P, dout=P, dx=P, doffset=P, ws=P, ws_bytes=1 << 40, elem=nv.OPS_BF16):
    args = (x, rois, offset, a["k"], a["n_img"], a["fh"], a["fw"], a["c"], a["out_h"], a["out_w"], 0.5, a["sampling_ratio"], 0.1, dout, dx,
            doffset, ws, ws_bytes, None)
    return lib.frcnn_ops_deform_roi_pool_backward_16(elem, *args) if half else lib.frcnn_ops_deform_roi_pool_backward(*args)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "16"])
def test_entry_points_validate_before_touching_the_gpu(half):
    lib = nv.lib()
    for bad in BAD:
        a = dict(GOOD, **bad)
        assert forward(lib, half, a) == -1, bad
        assert backward(lib, half, a) == -1, bad
    if half:
        assert forward(lib, True, dict(GOOD, c=4)) == -1                   # 16-bit runs are 8 channels
        assert forward(lib, True, GOOD, elem=0) == -1 and forward(lib, True, GOOD, elem=3) == -1
        assert backward(lib, True, GOOD, elem=0) == -1 and backward(lib, True, GOOD, elem=3) == -1
    for null in ("x", "rois", "out"):
        assert forward(lib, half, GOOD, **{null: None}) == -1, null
    for null in ("rois", "dout", "ws"):
        assert backward(lib, half, GOOD, **{null: None}) == -1, null
    assert backward(lib, half, GOOD, dx=None, doffset=None) == -1           # nothing to compute
    assert backward(lib, half, GOOD, offset=None) == -1                     # d_offset without an offset
    assert backward(lib, half, GOOD, x=None) == -1                          # d_offset reads the map
    assert backward(lib, half, GOOD, ws=P + 4) == -1                        # a misaligned workspace
    need = lib.frcnn_ops_deform_roi_pool_workspace_bytes(GOOD["k"], GOOD["out_h"], GOOD["out_w"])
    assert need == 3 * 4 * (16 + 8) + 3 * 32
    assert backward(lib, half, GOOD, ws_bytes=need - 1) == -1
    assert forward(lib, half, dict(GOOD, k=0), x=None, rois=None, out=None) == 0          # nothing to pool: no launch
    for args in ((-1, 2, 2), (3, 0, 2), (3, 2, 65), (2 ** 30, 2, 2)):
        assert lib.frcnn_ops_deform_roi_pool_workspace_bytes(*args) == 0, args
    assert lib.frcnn_ops_deform_roi_pool_workspace_bytes(0, 2, 2) == 0
