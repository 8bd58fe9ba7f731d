"""fasterrcnn_amd.ops.dcnv4 / DCNv4Function / dcnv4_core_pytorch / DCNv4 without a GPU: the self-checks of the restatements in
tests/dcnv4_cases.py, dcnv4_core_pytorch against both, the point order without the centre, the argument rules of the public functions,
shapes and dtypes on meta and fake tensors, the validation of the C entry points, and the module's parameters, init and CPU forward."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import dcnv4_cases as K

F32, F64 = torch.float32, torch.float64


# ---- 1. the restatements -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in K.CASES if n != "split"])     # "split" is sized by the library: see the seams test
def test_the_two_restatements_agree_and_every_case_is_non_trivial(name):
    truth, single = K.reference(name)                                      # asserts the agreement, the pad gradient and the positions
    input, om, grad = K.case(name)
    n, h, w, g, gc, kernel, stride, pad, dil, scale, rc, mode = K.CASES[name]
    p = K.points_of(name)
    assert [tuple(t.shape) for t in truth] == [tuple(grad.shape), tuple(input.shape), tuple(om.shape)]
    assert om.shape[3] == K.record(g, p) and om.shape[3] % 8 == 0 and 0 <= om.shape[3] - 3 * g * p < 8
    assert bool((om[..., 3 * g * p:] == K.PAD_VALUE).all())
    (tp, _), (sp, _) = K.parts(truth, g, p), K.parts(single, g, p)
    for t, s in zip(tp, sp):
        assert t.dtype == F64 and s.dtype == F32 and float(t.abs().max()) > 0.1
        assert K.rel_err(s, t) < 2e-6                                      # a float32 evaluation is a few ulps away
    xs, ys = K.coordinates(om.to(F64), h, w, *K.geom_of(name)[:8], g, scale, rc)
    outside = (xs <= -1) | (xs >= w) | (ys <= -1) | (ys >= h)
    mask = K.unpack(om, g, p)[1]
    if mode == "spread":                                                   # a share of the samples outside the map, most of them inside
        assert 0.1 < float(outside.double().mean()) < 0.8
        assert bool((mask < -0.5).any()) and bool((mask > 1.5).any())      # signed, not normalised
    else:
        assert not bool(outside.any())


def test_pack_and_unpack_are_inverse_and_lay_the_record_out_as_stated():
    off = torch.arange(2 * 3 * 2 * 5 * 2, dtype=F64).view(2, 3, 1, 20) + 1000
    mask = torch.arange(2 * 3 * 2 * 5, dtype=F64).view(2, 3, 1, 10)
    om = K.pack(off, mask, 2, 5, fill=-1.0)
    assert om.shape == (2, 3, 1, 32) and K.record(2, 5) == 32
    o, m, pad = K.unpack(om, 2, 5)
    assert torch.equal(o, off) and torch.equal(m, mask) and bool((pad == -1).all()) and pad.shape[-1] == 2
    rec = om[1, 2, 0]
    assert torch.equal(rec[0:10], off[1, 2, 0, 0:10]) and torch.equal(rec[10:15], mask[1, 2, 0, 0:5])      # group 0: 2 P offsets, P masks
    assert torch.equal(rec[15:25], off[1, 2, 0, 10:20]) and torch.equal(rec[25:30], mask[1, 2, 0, 5:10])
    assert [K.record(g, p) for g, p in ((2, 9), (3, 8), (1, 24), (3, 9), (2, 8), (5, 8), (3, 1))] == [56, 72, 72, 88, 48, 120, 16]


@pytest.mark.parametrize("name", [n for n in K.CASES if n != "split"])
def test_dcnv4_core_pytorch_against_both_restatements(name):
    truth, _ = K.reference(name)
    input, om, grad = K.case(name)
    geom, g, p = K.geom_of(name), K.CASES[name][3], K.points_of(name)
    got = K.with_gradients(ops.dcnv4_core_pytorch, input, om.to(F64), geom, grad)
    other = K.with_gradients(K.dcnv4_composition, input, om.to(F64), geom, grad)
    (gp, gpad), (tp, _), (op, _) = K.parts(got, g, p), K.parts(truth, g, p), K.parts(other, g, p)
    for i, (a, t, o) in enumerate(zip(gp, tp, op)):
        assert a.shape == t.shape and a.dtype == F64
        assert K.rel_err(a, t) <= (1e-13 if i == 0 else 1e-12) and K.rel_err(a, o) <= 1e-13
    assert not bool(gpad.any())


def test_dcnv4_core_pytorch_never_reads_the_pad_lanes():
    input, om, grad = K.case("pad7")
    geom = K.geom_of("pad7")
    bad = om.to(F64).clone()
    bad[..., 81:] = float("nan")
    for fn in (ops.dcnv4_core_pytorch, K.dcnv4_explicit, K.dcnv4_composition):
        a, b = K.with_gradients(fn, input, bad, geom, grad), K.with_gradients(fn, input, om.to(F64), geom, grad)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), fn.__name__


def test_the_point_order_without_the_centre():
    """3 x 3 without its centre, a one-hot mask on each of the 8 points in turn: points 0..3 are grid points 0..3, points 4..7 grid
    points 5..8; x is the outer index."""
    assert K.points(3, 3, True) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]
    assert K.points(2, 3, False) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    input = torch.arange(30, dtype=F64).view(1, 5, 6, 1)
    geom = K.geometry((3, 3), remove_center=True)
    for p, (i, j) in enumerate(K.points(3, 3, True)):
        mask = torch.zeros((1, 3, 4, 8), dtype=F64)
        mask[..., p] = 1.0
        om = K.pack(torch.zeros((1, 3, 4, 16), dtype=F64), mask, 1, 8)
        for fn in (K.dcnv4_explicit, K.dcnv4_composition, ops.dcnv4_core_pytorch):
            assert float((fn(input, om, *geom)[0] - input[0, j:j + 3, i:i + 4]).abs().max()) < 1e-12, (fn.__name__, p)


def test_without_remove_center_the_restatement_is_dcnv3s():
    from tests import dcnv3_cases as K3
    input, om, grad = K.case("pad7")
    off, mask, _ = K.unpack(om.to(F64), 3, 9)
    geom = K.geom_of("pad7")
    assert torch.equal(K.dcnv4_explicit(input, om.to(F64), *geom), K3.dcnv3_explicit(input, off, mask, *geom[:-1]))


def test_the_cases_sit_on_the_kernels_seams():
    lib = nv.lib()
    # frcnn_ops_dcnv4_record: the table of the cases, and 0 for bad arguments
    for name, want in (("base", 56), ("rc3", 72), ("rc5", 72), ("pad7", 88), ("even", 48), ("g5rc", 120), ("k1", 16), ("k7rc", 144)):
        n, h, w, g, gc, kernel, stride, pad, dil, scale, rc, mode = K.CASES[name]
        assert lib.frcnn_ops_dcnv4_record(g, kernel[0], kernel[1], int(rc)) == want == K.record(g, K.points_of(name)), name
    for bad in ((0, 3, 3, 0), (2, 0, 3, 0), (2, 3, 8, 0), (2, 3, 3, 2), (2, 3, 3, -1), (2, 1, 1, 1), (2, 3, 5, 1), (2, 4, 4, 1), (2, 2, 2, 1),
                (2 ** 30, 3, 3, 0)):
        assert lib.frcnn_ops_dcnv4_record(*bad) == 0, bad
    # the mapping the getter reports: dcnv3's with P samples an item
    assert K.block_items(8, 3, 3) == 113 == lib.frcnn_ops_dcnv3_block_items(8, 3, 3, 0) and K.block_items(8, 3, 3, True) == 128
    assert K.block_items(4, 7, 7, True) == 21 and K.block_items(4, 7, 7) == 20 and K.block_items(16, 3, 3, False, nv.OPS_BF16) == 113
    assert K.block_items(256, 3, 3) == 4 and K.block_items(3, 3, 3, True) == 64 and K.block_items(2, 3, 3, True) == 128
    for bad in ((0, 3, 3, 0, 0), (257, 3, 3, 0, 0), (8, 8, 3, 0, 0), (8, 3, 0, 0, 0), (8, 3, 3, 0, 3), (8, 3, 3, 2, 0), (8, 1, 1, 1, 0),
                (8, 3, 5, 1, 0), (8, 4, 4, 1, 0)):
        assert lib.frcnn_ops_dcnv4_block_items(*bad) == 0, bad
    for name in ("base", "rc3", "k7rc", "one-cell", "split"):             # more than one block, the last one partly filled
        n, h, w, g, gc, kernel = K.CASES[name][:6]
        items, ipb = K.case(name)[2].numel() // gc, K.block_items(gc, kernel[0], kernel[1], K.CASES[name][10])
        assert items > ipb and items % ipb != 0, name
    # blocks that begin inside a record: the items of a block are no multiple of G
    for name in ("base", "rc3", "split"):
        n, h, w, g, gc, kernel = K.CASES[name][:6]
        assert K.block_items(gc, kernel[0], kernel[1], K.CASES[name][10]) % g != 0, name
    n, h, w, g, gc = K.shape_of("split")[:5]
    ipb = K.block_items(gc, 3, 3)
    assert (g, gc, w) == (3, 8, ipb // 3 + 1) and h * w * g > 2 * ipb and K.record(3, 9) - 81 == 7
    K.reference("split")                                                   # the self-checks of the case the library sizes
    # the long segment: every sample of an image lands in cell (1, 1), so four cells own Ho Wo P entries each
    n, h, w, g, gc, kernel = K.CASES["one-cell"][:6]
    per_cell = h * w * 9
    assert per_cell > 2 * K.segment() and (4 * per_cell) % K.segment() != 0 and n == 2
    xs, ys = K.coordinates(K.case("one-cell")[1].to(F64), h, w, *K.geom_of("one-cell")[:8], g, 1.0, False)
    assert bool(((xs > 1) & (xs < 2) & (ys > 1) & (ys < 2)).all())
    assert {K.CASES[c][4] for c in K.CASES} >= {3, 70, 72, 256} and K.CASES["gc3"][10]


# ---- 2. the interface ----------------------------------------------------------------------------------------------------------------------
def args(n=2, h=5, w=6, group=2, gc=4, kernel=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), rc=False, device="meta", dtype=F32, om_dtype=None):
    ho, wo = K.out_size(h, kernel[0], stride[0], pad[0], dil[0]), K.out_size(w, kernel[1], stride[1], pad[1], dil[1])
    p = kernel[0] * kernel[1] - int(rc)
    e = lambda shape, dt: torch.empty(shape, device=device, dtype=dt)       # noqa: E731
    return [e((n, h, w, group * gc), dtype), e((n, max(ho, 0), max(wo, 0), K.record(group, p)), om_dtype or dtype)]


def test_the_names_are_exported():
    for name in ("dcnv4", "DCNv4Function", "dcnv4_core_pytorch", "DCNv4"):
        assert name in ops.__all__ and hasattr(ops, name)
    for name in ("dcnv4", "dcnv4_backward"):
        assert hasattr(torch.ops.frcnn, name)
    assert "dcnv4(" in ops.__doc__ and "DCNv4(" in ops.__doc__ and "DCNv4Function.apply(" in ops.__doc__
    assert nv.ABI_VERSION == 21 and nv.lib().frcnn_abi_version() == 21


def test_the_header_and_the_symbol_table_agree_on_the_new_entry_points():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frcnn_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(frcnn_ops_dcnv4_\w+)\(", header, re.M))
    want = {"frcnn_ops_dcnv4_" + n for n in ("record", "block_items", "workspace_bytes", "forward", "backward_offset_mask", "plan",
                                              "backward_input", "forward_16", "backward_offset_mask_16", "backward_input_16")}
    assert declared == want == {s for s in nv.SYMBOLS if s.startswith("frcnn_ops_dcnv4_")}
    for name in want:
        assert hasattr(nv.lib(), name)


def test_argument_errors():
    e = lambda *shape, dtype=F32: torch.empty(shape, device="meta", dtype=dtype)    # noqa: E731

    def bad(match, error=ValueError, a=None, **kw):
        call = dict(kernel_size=3, padding=1, group=2)
        call.update(kw)
        with pytest.raises(error, match=match):
            ops.dcnv4(*(a or args()), **call)

    bad("input must be \\[N, H, W, C\\] \\(channels last\\), got shape \\(2, 5, 24\\)", a=[e(2, 5, 24), args()[1]])
    bad("input's 8 channels must be divisible by group, got 3", group=3)
    bad("group must be at least 1, got 0", group=0)
    bad("group must be an int, got 2.0", TypeError, group=2.0)
    bad("offset_mask must be \\[N, Ho, Wo, L\\] = \\[2, 5, 6, 56\\] with L = ceil\\(G P 3 / 8\\) 8 for G = 2 groups of P = 9 points "
        "\\(2 P offsets, then P masks; the record padded to a multiple of 8\\), got shape \\(2, 5, 6, 54\\)", a=[args()[0], e(2, 5, 6, 54)])
    bad("offset_mask must be \\[N, Ho, Wo, L\\] = \\[2, 5, 6, 48\\] with L = .* G = 2 groups of P = 8 points", remove_center=True)
    bad("offset_mask must be \\[N, Ho, Wo, L\\] = \\[2, 3, 4, 56\\]", padding=0)                 # Ho, Wo follow the geometry
    bad("remove_center requires a square kernel of odd size >= 3, got \\(3, 5\\)", kernel_size=(3, 5), remove_center=True)
    bad("remove_center requires a square kernel of odd size >= 3, got \\(4, 4\\)", kernel_size=4, remove_center=True)
    bad("remove_center requires a square kernel of odd size >= 3, got \\(1, 1\\)", kernel_size=1, padding=0, remove_center=True)
    bad("remove_center must be False or True \\(0 or 1\\), got 2", remove_center=2)
    bad("remove_center must be False or True \\(0 or 1\\), got -1", remove_center=-1)
    bad("remove_center must be a bool, got None", TypeError, remove_center=None)
    bad("kernel_size must lie in \\[1, MAX_DCNV3_KERNEL = 7\\], got \\(8, 3\\)", kernel_size=(8, 3))
    bad("kernel_size must be >= 1, got \\(0, 3\\)", kernel_size=(0, 3))
    bad("kernel_size must be an int or a pair of ints", TypeError, kernel_size=3.0)
    bad("stride must be >= 1, got \\(0, 0\\)", stride=0)
    bad("dilation must be >= 1, got \\(1, 0\\)", dilation=(1, 0))
    bad("padding must be >= 0, got \\(-1, -1\\)", padding=-1)
    bad("stride must lie in \\[1, MAX_DCNV3_STEP = 65536\\], got \\(65537, 1\\)", stride=(65537, 1))
    bad("group_channels must lie in \\[1, MAX_DCNV3_CHANNELS = 256\\], got 257", a=args(group=1, gc=257), group=1)
    bad("offset_scale must be finite, got nan", offset_scale=float("nan"))
    bad("offset_scale must be a float, got '1'", TypeError, offset_scale="1")
    bad("im2col_step must be an int, got 2.0", TypeError, im2col_step=2.0)
    bad("im2col_step must be at least 1, got 0", im2col_step=0)
    bad("input must be float32, float16 or bfloat16, got torch.float64", TypeError, a=args(dtype=F64))
    bad("offset_mask must be float32, got torch.float16", TypeError, a=args(om_dtype=torch.float16))
    bad("offset_mask must be float32 or the input's torch.float16, got torch.bfloat16", TypeError,
        a=args(dtype=torch.float16, om_dtype=torch.bfloat16))
    bad("input must be a torch.Tensor", TypeError, a=[None, args()[1]])
    with pytest.raises(ValueError, match="input must be a tensor on the GPU.*no CPU implementation"):
        ops.dcnv4(*args(device="cpu"), 3, padding=1, group=2)
    with pytest.raises(ValueError, match="group \\* group_channels must equal input's 8 channels, got group 2 and group_channels 3"):
        ops.DCNv4Function.apply(*args(), 3, 3, 1, 1, 1, 1, 1, 1, 2, 3, 1.0, 256, False)
    with FakeTensorMode():
        with pytest.raises(ValueError, match="input and offset_mask must be on the same device"):
            ops.dcnv4(args(device="cuda")[0], args()[1], 3, padding=1, group=2)


def test_the_index_limits_are_named_count_the_points_and_follow_im2col_step():
    a = args(n=4, h=2 ** 14, w=2 ** 14, group=2, gc=1, kernel=(1, 1), stride=(2 ** 14, 2 ** 14), pad=(0, 0))      # 4 * 2^28 * 2 cells
    with pytest.raises(ValueError, match="32-bit cell indices: 4 images x H x W x G = 2147483648 > MAX_MSDA_INDEX = 2147482623"):
        ops.dcnv4(*a, 1, stride=2 ** 14, group=2)
    assert ops.dcnv4(*a, 1, stride=2 ** 14, group=2, im2col_step=3).shape == (4, 1, 1, 2)
    a = args(n=2, h=2896, w=2896, group=1, gc=1, kernel=(7, 7), pad=(3, 3), rc=True)                             # 2 * 2896^2 * 48 * 4 entries
    with pytest.raises(ValueError, match="32-bit plan indices: 2 images x Ho x Wo x G x P x 4 = 3220537344 > MAX_MSDA_INDEX"):
        ops.dcnv4(*a, 7, padding=3, remove_center=True)
    assert ops.dcnv4(*a, 7, padding=3, im2col_step=1, remove_center=True).shape == (2, 2896, 2896, 1)
    # 1 x 3344^2 x 48 x 4 entries fit, x 49 do not: the entries are counted with P
    assert ops.dcnv4(*args(n=1, h=3344, w=3344, group=1, gc=1, kernel=(7, 7), pad=(3, 3), rc=True), 7, padding=3, remove_center=True).shape[1] == 3344
    with pytest.raises(ValueError, match="32-bit plan indices"):
        ops.dcnv4(*args(n=1, h=3344, w=3344, group=1, gc=1, kernel=(7, 7), pad=(3, 3)), 7, padding=3)
    assert ops.dcnv4(*args(group=1, gc=256, kernel=(7, 7), pad=(3, 3)), 7, padding=3).shape == (2, 5, 6, 256)     # the limits are served


@pytest.mark.parametrize("dtype, om_dtype", [(F32, F32), (torch.float16, F32), (torch.float16, torch.float16), (torch.bfloat16, F32),
                                             (torch.bfloat16, torch.bfloat16)])
def test_meta_and_fake_shapes_and_dtypes(dtype, om_dtype):
    for device in ("meta", "fake"):
        mode = FakeTensorMode() if device == "fake" else None
        if mode:
            mode.__enter__()
        try:
            a = args(device="cuda" if mode else "meta", dtype=dtype, om_dtype=om_dtype, kernel=(3, 3), stride=(2, 1), pad=(1, 0), dil=(2, 1),
                     rc=True)
            for t in a:
                t.requires_grad_(True)
            a[1] = a[1].transpose(1, 2).contiguous().transpose(1, 2)                 # a non-contiguous argument
            y = ops.dcnv4(*a, 3, (2, 1), (1, 0), (2, 1), 2, 0.5, 1, True)
            assert y.shape == (2, 2, 4, 8) and y.dtype == dtype and y.is_contiguous() and y.requires_grad
            assert ops.DCNv4Function.apply(*a, 3, 3, 2, 1, 1, 0, 2, 1, 2, 4, 0.5, 256, True).shape == y.shape
            if not mode:
                dx, dom = torch.autograd.grad(y.sum(), a)
                assert (dx.shape, dx.dtype) == (a[0].shape, dtype) and (dom.shape, dom.dtype) == (a[1].shape, om_dtype)
        finally:
            if mode:
                mode.__exit__(None, None, None)


def test_backward_on_meta_skips_what_is_not_needed_and_double_backward_raises():
    a = args()
    grad = torch.empty((2, 5, 6, 8), device="meta")
    tail = (3, 3, 1, 1, 1, 1, 1, 1, 2, 4, 1.0, 256, False)
    for needs in ([True, False], [False, True], [True, True], [False, False]):
        got = torch.ops.frcnn.dcnv4_backward(grad, *a, *tail, needs)
        assert [tuple(g.shape) for g in got] == [tuple(t.shape) if need else (0,) for t, need in zip(a, needs)]
    a[0].requires_grad_(True)
    y = ops.dcnv4(*a, 3, padding=1, group=2)
    dx, = torch.autograd.grad(y.sum(), a[0], create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        dx.sum().backward()


def test_empty_calls_on_meta():
    for changes, call in ((dict(n=0), dict(padding=1)), (dict(h=1, pad=(0, 0)), dict(padding=0)), (dict(w=2, pad=(1, 0)), dict(padding=(1, 0)))):
        a = args(**changes)
        for t in a:
            t.requires_grad_(True)
        y = ops.dcnv4(*a, 3, group=2, **call)
        assert y.numel() == 0 and y.shape == tuple(a[1].shape[:3]) + (8,)
        y.sum().backward()
        assert all(t.grad.shape == t.shape for t in a)


def test_an_empty_input_map_with_a_non_empty_output_on_meta():
    """H W == 0 with Ho Wo > 0: padding alone carries the kernel, so every sample lies outside the (empty) map."""
    for changes, call, shape in ((dict(h=0, pad=(2, 1)), dict(padding=(2, 1)), (2, 2, 6, 8)), (dict(w=0, pad=(1, 2)), dict(padding=(1, 2)), (2, 5, 2, 8))):
        a = args(**changes)
        assert a[0].numel() == 0 and a[1].numel() > 0
        for t in a:
            t.requires_grad_(True)
        y = ops.dcnv4(*a, 3, group=2, **call)
        assert y.shape == shape and y.numel() > 0
        y.sum().backward()
        assert all(t.grad.shape == t.shape and t.grad.dtype == t.dtype for t in a)
        for needs in ([True, False], [False, True], [True, True]):
            got = torch.ops.frcnn.dcnv4_backward(torch.empty(shape, device="meta"), *a, 3, 3, 1, 1, *call["padding"], 1, 1, 2, 4, 1.0, 256, False, needs)
            assert [tuple(g.shape) for g in got] == [tuple(t.shape) if need else (0,) for t, need in zip(a, needs)]


# ---- 3. the C entry points -----------------------------------------------------------------------------------------------------------------
GOOD = dict(n=2, h=5, w=6, g=2, gc=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
BAD = [dict(n=0), dict(h=0), dict(w=0), dict(g=0), dict(gc=0), dict(gc=257), dict(kh=0), dict(kh=8), dict(kw=0), dict(kw=8), dict(sh=0),
       dict(sw=0), dict(dh=0), dict(dw=0), dict(ph=-1), dict(pw=-1), dict(sh=65537), dict(pw=65537), dict(dh=65537), dict(n=-1),
       dict(h=2 ** 24 + 1), dict(h=2, ph=0), dict(w=4, pw=0, dw=2, kw=3), dict(n=4, h=2 ** 14, w=2 ** 14, g=2),
       dict(n=2, h=2 ** 12, w=2 ** 12, g=1, kh=7, kw=7, ph=3, pw=3),
       dict(rc=2), dict(rc=-1), dict(rc=1, kh=1, kw=1, ph=0, pw=0), dict(rc=1, kh=3, kw=5), dict(rc=1, kh=2, kw=2), dict(rc=1, kh=4, kw=4),
       dict(rc=1, n=2, h=2 ** 12, w=2 ** 12, g=1, kh=7, kw=7, ph=3, pw=3)]


def test_entry_points_validate_before_touching_a_gpu():
    lib = nv.lib()
    P = 4096                                  # any aligned non-null pointer: every call below returns before a launch

    def dims(changes, with_gc=True):
        a = dict(GOOD, **changes)
        return tuple(a[k] for k in GOOD if with_gc or k != "gc"), a.get("rc", 0)

    def forward(elem, ptrs, scale=1.0, **changes):
        d, rc = dims(changes)
        tail = tuple(ptrs[:2]) + d + (scale, rc, ptrs[2], None)
        return lib.frcnn_ops_dcnv4_forward(*tail) if elem is None else lib.frcnn_ops_dcnv4_forward_16(elem, *tail)

    def backward_om(elem, ptrs, scale=1.0, **changes):
        d, rc = dims(changes)
        tail = tuple(ptrs[:3]) + d + (scale, rc, ptrs[3], None)
        return lib.frcnn_ops_dcnv4_backward_offset_mask(*tail) if elem is None else lib.frcnn_ops_dcnv4_backward_offset_mask_16(elem, *tail)

    def plan(ptrs, scale=1.0, **changes):
        d, rc = dims(changes, with_gc=False)
        return lib.frcnn_ops_dcnv4_plan(ptrs[0], *d, scale, rc, ptrs[1], ptrs[2], None)

    def backward_input(elem, ptrs, ws=P, ws_bytes=1 << 20, **changes):
        d, rc = dims(changes)
        tail = tuple(ptrs[:4]) + d + (rc, ptrs[4], ws, ws_bytes, None)
        return lib.frcnn_ops_dcnv4_backward_input(*tail) if elem is None else lib.frcnn_ops_dcnv4_backward_input_16(elem, *tail)

    def workspace(**changes):
        d, rc = dims(changes)
        return lib.frcnn_ops_dcnv4_workspace_bytes(*d, rc)

    def nulls(n):
        for i in range(n):
            yield [None if j == i else P for j in range(n)]

    need = workspace()
    assert need == lib.frcnn_ops_dcnv3_workspace_bytes(*dims({})[0]) and need % 256 == 0
    assert workspace(rc=1) == lib.frcnn_ops_msda_workspace_bytes(2, 30, 2, 4, 30, 1, 8)        # the gather's: L = 1, P = 8, M = G, D = Gc
    for changes in BAD:
        assert workspace(**changes) == 0, changes
    for elem in (None, nv.OPS_F16, nv.OPS_BF16):
        for rc in (0, 1):
            for ptrs in nulls(3):
                assert forward(elem, ptrs, rc=rc) == -1
            for ptrs in nulls(4):
                assert backward_om(elem, ptrs, rc=rc) == -1
            for ptrs in nulls(5):
                assert backward_input(elem, ptrs, rc=rc) == -1
        assert backward_input(elem, [P] * 5, ws=None) == -1
        assert backward_input(elem, [P] * 5, ws=P + 4) == -1               # a misaligned workspace
        assert backward_input(elem, [P] * 5, ws_bytes=need - 1) == -1      # too small a workspace
        for scale in (float("nan"), float("inf"), -float("inf")):
            assert forward(elem, [P] * 3, scale=scale) == -1 and backward_om(elem, [P] * 4, scale=scale) == -1
        for changes in BAD:
            assert forward(elem, [P] * 3, **changes) == -1, changes
            assert backward_om(elem, [P] * 4, **changes) == -1, changes
            assert backward_input(elem, [P] * 5, ws_bytes=1 << 62, **changes) == -1, changes
    for ptrs in nulls(3):
        assert plan(ptrs) == -1
    assert plan([P] * 3, scale=float("nan")) == -1
    for changes in BAD:
        if "gc" not in changes:
            assert plan([P] * 3, **changes) == -1, changes
    for elem in (0, 3, -1):
        assert forward(elem, [P] * 3) == -1 and backward_om(elem, [P] * 4) == -1 and backward_input(elem, [P] * 5) == -1


# ---- 4. the module -------------------------------------------------------------------------------------------------------------------------
def test_module_owns_upstreams_parameters_and_loads_strict():
    torch.manual_seed(0)
    mod = ops.DCNv4()
    names = ["offset_mask.weight", "offset_mask.bias", "value_proj.weight", "value_proj.bias", "output_proj.weight", "output_proj.bias"]
    shapes = [(112, 64), (112,), (64, 64), (64,), (64, 64), (64,)]          # 4 groups x 9 points x 3 = 108 -> 112
    sd = mod.state_dict()
    assert list(sd) == names and [tuple(sd[k].shape) for k in names] == shapes

    def layout(**kw):
        return {k: tuple(v.shape) for k, v in ops.DCNv4(**kw).state_dict().items()}

    assert layout(channels=12, kernel_size=5, pad=2, group=3, remove_center=True, dw_kernel_size=3) == {
        "offset_mask_dw.weight": (12, 1, 3, 3), "offset_mask_dw.bias": (12,), "offset_mask.weight": (216, 12), "offset_mask.bias": (216,),
        "value_proj.weight": (12, 12), "value_proj.bias": (12,), "output_proj.weight": (12, 12), "output_proj.bias": (12,)}
    assert layout(channels=16, group=2, without_pointwise=True) == {"offset_mask.weight": (56, 16), "offset_mask.bias": (56,)}
    assert layout(channels=16, group=2, remove_center=True, output_bias=False) == {
        "offset_mask.weight": (48, 16), "offset_mask.bias": (48,), "value_proj.weight": (16, 16), "value_proj.bias": (16,),
        "output_proj.weight": (16, 16)}
    assert layout(channels=6, group=3, kernel_size=1, pad=0) == {                                       # Gc = 2: no Gc % 16 rule here
        "offset_mask.weight": (16, 6), "offset_mask.bias": (16,), "value_proj.weight": (6, 6), "value_proj.bias": (6,),
        "output_proj.weight": (6, 6), "output_proj.bias": (6,)}
    gen = torch.Generator().manual_seed(1)
    theirs = {k: torch.randn(shape, generator=gen) for k, shape in zip(names, shapes)}       # a hand-built upstream-named checkpoint
    mod.load_state_dict(theirs, strict=True)
    assert all(torch.equal(mod.state_dict()[k], theirs[k]) for k in names)
    with pytest.raises(RuntimeError, match="offset_mask_dw"):
        mod.load_state_dict(dict(theirs, **{"offset_mask_dw.weight": torch.zeros(64, 1, 3, 3)}), strict=True)
    with pytest.raises(ValueError, match="channels must be divisible by group, got 10 and 4"):
        ops.DCNv4(channels=10)
    with pytest.raises(NotImplementedError, match="center_feature_scale"):
        ops.DCNv4(center_feature_scale=True)
    with pytest.raises(ValueError, match="remove_center requires a square kernel of odd size >= 3, got \\(4, 4\\)"):
        ops.DCNv4(kernel_size=4, remove_center=True)
    with pytest.raises(NotImplementedError, match="remove_center"):        # DCNv3 keeps refusing the flag
        ops.DCNv3(remove_center=True)
    assert "group=4" in repr(mod) and "remove_center=False" in repr(mod) and mod.K == 36 and ops.DCNv4(remove_center=True).K == 32


def test_module_init_is_upstreams_and_a_fresh_module_outputs_its_bias():
    torch.manual_seed(0)
    mod = ops.DCNv4(channels=64, group=4)
    assert not bool(mod.offset_mask.weight.any()) and not bool(mod.offset_mask.bias.any())
    bound = (6.0 / (64 + 64)) ** 0.5                                       # Xavier-uniform
    for proj in (mod.value_proj, mod.output_proj):
        w = proj.weight.detach()
        assert not bool(proj.bias.any())
        assert 0.98 * bound < float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) < 0.03 * bound
    # a zero mask zeroes the core: the freshly built module outputs exactly output_proj.bias
    torch.nn.init.normal_(mod.output_proj.bias)
    x = torch.randn(2, 30, 64)
    out = mod(x, shape=(5, 6))
    assert out.shape == (2, 30, 64) and torch.equal(out.detach(), mod.output_proj.bias.detach().expand(2, 30, 64))
    dw = ops.DCNv4(channels=8, group=2, dw_kernel_size=5)
    assert dw.offset_mask_dw.groups == 8 and dw.offset_mask_dw.padding == (2, 2) and dw.offset_mask_dw.kernel_size == (5, 5)


def test_module_forward_takes_its_shape_or_a_perfect_square():
    mod = ops.DCNv4(channels=8, group=2)
    assert mod(torch.randn(1, 36, 8)).shape == (1, 36, 8)                  # 6 x 6
    assert mod(torch.randn(1, 35, 8), shape=(5, 7)).shape == (1, 35, 8)
    with pytest.raises(ValueError, match="input's length 35 is not H W"):
        mod(torch.randn(1, 35, 8))
    with pytest.raises(ValueError, match="input's length 35 is not H W"):
        mod(torch.randn(1, 35, 8), shape=(6, 6))


@pytest.mark.parametrize("kw", [dict(), dict(remove_center=True), dict(dw_kernel_size=3), dict(without_pointwise=True),
                                dict(output_bias=False, remove_center=True, dw_kernel_size=5)])
def test_module_cpu_forward_is_the_restatement(kw):
    torch.manual_seed(2)
    mod = ops.DCNv4(channels=12, kernel_size=3, pad=1, group=3, offset_scale=1.5, **kw).double()
    torch.nn.init.normal_(mod.offset_mask.weight, std=0.5)
    torch.nn.init.normal_(mod.offset_mask.bias, std=0.5)
    x = torch.randn(2, 30, 12, dtype=F64)
    out = mod(x, (5, 6))
    assert out.shape == x.shape
    head = x.view(2, 5, 6, 12)
    if "dw_kernel_size" in kw:
        head = mod.offset_mask_dw(head.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    om = mod.offset_mask(head)
    assert float(om.detach().abs().max()) > 0.5 and om.shape[-1] == K.record(3, 8 if kw.get("remove_center") else 9)
    value = x if kw.get("without_pointwise") else mod.value_proj(x)
    core = K.dcnv4_explicit(value.view(2, 5, 6, 12), om, *K.geometry((3, 3), (1, 1), (1, 1), (1, 1), 3, 4, 1.5, bool(kw.get("remove_center"))))
    want = core.view(2, 30, 12) if kw.get("without_pointwise") else mod.output_proj(core.view(2, 30, 12))
    assert float(want.detach().abs().max()) > 0.5 and float((want - out).detach().abs().max()) < 1e-12
    assert hasattr(mod, "output_proj") != bool(kw.get("without_pointwise"))
    if kw.get("output_bias") is False:
        assert mod.output_proj.bias is None
