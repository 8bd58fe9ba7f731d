"""fasterrcnn_amd.ops.dcnv3 / DCNv3Function / dcnv3_core_pytorch / DCNv3 without a GPU: the self-checks of the restatements in
tests/dcnv3_cases.py, dcnv3_core_pytorch against both, the exact properties of the rule (box filter, identity), the argument rules of
the public functions, shapes and dtypes on meta and fake tensors, the validation of the C entry points, and the module's parameters,
init and CPU forward."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import dcnv3_cases as K

F32, F64 = torch.float32, torch.float64


# ---- 1. the restatements -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_the_two_restatements_agree_and_every_case_is_non_trivial(name):
    truth, single = K.reference(name)                                      # asserts the agreement; K.case the positions of the samples
    input, offset, mask, grad = K.case(name)
    assert [tuple(t.shape) for t in truth] == [tuple(grad.shape), tuple(input.shape), tuple(offset.shape), tuple(mask.shape)]
    for t, s in zip(truth, single):
        assert t.dtype == F64 and s.dtype == F32 and float(t.abs().max()) > 0.1
        assert K.rel_err(s, t) < 2e-6                                      # a float32 evaluation is a few ulps away
    n, h, w, g, gc, kernel, stride, pad, dil, scale, mode = K.CASES[name]
    xs, ys = K.coordinates(offset.to(F64), h, w, *K.geom_of(name)[:8], g, scale)
    outside = (xs <= -1) | (xs >= w) | (ys <= -1) | (ys >= h)
    if mode == "spread":                                                   # a share of the samples outside the map, most of them inside
        assert 0.1 < float(outside.double().mean()) < 0.8
        assert bool(((xs > -1) & (xs < 0) & ~outside).any()) or bool(((ys > -1) & (ys < 0) & ~outside).any())
    else:
        assert not bool(outside.any())


def test_the_self_check_geometries_agree_as_tightly_as_stated():
    for name in ("base", "strided", "even", "gc6"):                        # even kernels, kh != kw, stride 2, dilation 2, unequal padding
        truth, _ = K.reference(name)
        input, offset, mask, grad = K.case(name)
        other = K.dcnv3_composition(input, offset.to(F64), mask, *K.geom_of(name))
        assert float((truth[0] - other).abs().max()) <= 6e-15


@pytest.mark.parametrize("name", list(K.CASES))
def test_dcnv3_core_pytorch_against_both_restatements(name):
    truth, _ = K.reference(name)
    input, offset, mask, grad = K.case(name)
    geom = K.geom_of(name)
    got = K.with_gradients(ops.dcnv3_core_pytorch, input, offset.to(F64), mask, geom, grad)
    other = K.with_gradients(K.dcnv3_composition, input, offset.to(F64), mask, geom, grad)
    for i, (g, t, o) in enumerate(zip(got, truth, other)):
        assert g.shape == t.shape and g.dtype == F64
        assert K.rel_err(g, t) <= (1e-13 if i == 0 else 1e-12) and K.rel_err(g, o) <= 1e-13


def test_the_cases_sit_on_the_kernels_seams():
    lib = nv.lib()
    assert (lib.frcnn_ops_dcnv3_max_kernel(), lib.frcnn_ops_dcnv3_max_channels()) == (ops.MAX_DCNV3_KERNEL, ops.MAX_DCNV3_CHANNELS) == (7, 256)
    gcs = {c[4] for c in K.CASES.values()}
    assert gcs >= {3, 6, 70, 8, 32, 72, 256} and {c[3] for c in K.CASES.values()} >= {1, 2, 3}
    assert K.CASES["k7"][5] == (7, 7) and K.CASES["even"][5] == (2, 4) and K.CASES["strided"][5] == (3, 2)
    # the mapping the getter reports: Gc / 4 float32 runs (Gc / 8 16-bit ones) rounded up to a power of two lanes, 256 lanes a block,
    # at most 1024 staged samples
    assert K.block_items(8, 3, 3) == 113 and K.block_items(16, 3, 3) == 64 and K.block_items(16, 3, 3, nv.OPS_BF16) == 113
    assert K.block_items(256, 3, 3) == 4 and K.block_items(4, 7, 7) == 20 and K.block_items(3, 3, 3) == 64 and K.block_items(70, 1, 3) == 4
    assert lib.frcnn_ops_dcnv3_block_items(0, 3, 3, 0) == 0 and lib.frcnn_ops_dcnv3_block_items(8, 8, 3, 0) == 0
    assert lib.frcnn_ops_dcnv3_block_items(8, 3, 0, 0) == 0 and lib.frcnn_ops_dcnv3_block_items(8, 3, 3, 3) == 0
    for name in ("base", "k7", "one-cell"):                                # more than one block, the last one partly filled
        n, h, w, g, gc, kernel = K.CASES[name][:6]
        items = K.case(name)[3].numel() // gc
        assert items > K.block_items(gc, *kernel) and items % K.block_items(gc, *kernel) != 0
    # the long segment: every sample of an image lands in cell (1, 1), so four cells own Ho Wo K entries each
    n, h, w, g, gc, kernel = K.CASES["one-cell"][:6]
    per_cell = h * w * kernel[0] * kernel[1]
    assert per_cell > 2 * K.segment() and (4 * per_cell) % K.segment() != 0 and n == 2
    xs, ys = K.coordinates(K.case("one-cell")[1].to(F64), h, w, *K.geom_of("one-cell")[:8], g, 1.0)
    assert bool(((xs > 1) & (xs < 2) & (ys > 1) & (ys < 2)).all())


# ---- 2. exact properties of the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel, stride, pad, dil", K.BOX)
def test_zero_offsets_and_unit_masks_give_the_box_filter_exactly(kernel, stride, pad, dil):
    input, offset, mask, geom, want = K.box_filter_case(kernel, stride, pad, dil)
    assert float(want.abs().max()) >= 8
    for dtype in (F64, F32):                                               # the rule forms integer coordinates exactly
        assert torch.equal(K.dcnv3_explicit(input.to(dtype), offset.to(dtype), mask.to(dtype), *geom).to(F64), want), dtype
    for fn in (K.dcnv3_composition, ops.dcnv3_core_pytorch):               # the compositions round them through normalised locations
        assert float((fn(input, offset, mask, *geom) - want).abs().max()) < 1e-12, fn.__name__


@pytest.mark.parametrize("kernel, dil", K.IDENTITY)
def test_a_one_hot_centre_mask_returns_the_input_bit_for_bit(kernel, dil):
    input, offset, mask, geom = K.identity_case(kernel, dil)
    assert torch.equal(K.dcnv3_explicit(input, offset, mask, *geom), input)
    assert torch.equal(K.dcnv3_explicit(input.to(F64), offset.to(F64), mask.to(F64), *geom), input.to(F64))
    assert float((ops.dcnv3_core_pytorch(input.to(F64), offset.to(F64), mask.to(F64), *geom) - input).abs().max()) < 1e-13


def test_x_is_the_outer_index_of_a_point():
    """A 2 x 3 kernel (kh 2, kw 3): point 1 is one step along y from point 0, point 2 one step along x."""
    input = torch.arange(20, dtype=F64).view(1, 4, 5, 1)
    geom = K.geometry((2, 3), (1, 1), (0, 0), (1, 1), 1, 1, 1.0)
    offset = torch.zeros((1, 3, 3, 12), dtype=F64)
    for p, want in ((0, input[0, 0:3, 0:3]), (1, input[0, 1:4, 0:3]), (2, input[0, 0:3, 1:4]), (5, input[0, 1:4, 2:5])):
        mask = torch.zeros((1, 3, 3, 6), dtype=F64)
        mask[..., p] = 1.0
        for fn in (K.dcnv3_explicit, K.dcnv3_composition, ops.dcnv3_core_pytorch):
            assert float((fn(input, offset, mask, *geom)[0] - want).abs().max()) < 1e-12, (fn.__name__, p)


# ---- 3. the interface ----------------------------------------------------------------------------------------------------------------------
def args(n=2, h=5, w=6, group=2, gc=4, kernel=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), device="meta", dtype=F32, off_dtype=None):
    ho, wo = K.out_size(h, kernel[0], stride[0], pad[0], dil[0]), K.out_size(w, kernel[1], stride[1], pad[1], dil[1])
    k = kernel[0] * kernel[1]
    e = lambda shape, dt: torch.empty(shape, device=device, dtype=dt)       # noqa: E731
    off_dtype = off_dtype or dtype
    return [e((n, h, w, group * gc), dtype), e((n, max(ho, 0), max(wo, 0), group * k * 2), off_dtype),
            e((n, max(ho, 0), max(wo, 0), group * k), off_dtype)]


def test_the_names_are_exported():
    for name in ("dcnv3", "DCNv3Function", "dcnv3_core_pytorch", "DCNv3"):
        assert name in ops.__all__ and hasattr(ops, name)
    for name in ("dcnv3", "dcnv3_backward"):
        assert hasattr(torch.ops.frcnn, name)
    assert "dcnv3(" in ops.__doc__ and "DCNv3(" in ops.__doc__ and "DCNv3Function.apply(" in ops.__doc__


def test_argument_errors():
    e = lambda *shape, dtype=F32: torch.empty(shape, device="meta", dtype=dtype)    # noqa: E731

    def bad(match, error=ValueError, a=None, **kw):
        call = dict(kernel_size=3, padding=1, group=2)
        call.update(kw)
        with pytest.raises(error, match=match):
            ops.dcnv3(*(a or args()), **call)

    bad("input must be \\[N, H, W, C\\] \\(channels last\\), got shape \\(2, 5, 24\\)", a=[e(2, 5, 24)] + args()[1:])
    bad("input's 8 channels must be divisible by group, got 3", group=3)
    bad("group must be at least 1, got 0", group=0)
    bad("group must be an int, got 2.0", TypeError, group=2.0)
    bad("offset must be \\[N, Ho, Wo, G K 2\\] = \\[2, 5, 6, 36\\], got shape \\(2, 5, 6, 18\\)", a=[args()[0], e(2, 5, 6, 18), args()[2]])
    bad("mask must be \\[N, Ho, Wo, G K\\] = \\[2, 5, 6, 18\\], got shape \\(2, 5, 5, 18\\)", a=args()[:2] + [e(2, 5, 5, 18)])
    bad("offset must be \\[N, Ho, Wo, G K 2\\] = \\[2, 3, 4, 36\\]", padding=0)         # Ho, Wo follow the geometry
    bad("kernel_size must lie in \\[1, MAX_DCNV3_KERNEL = 7\\], got \\(8, 3\\)", kernel_size=(8, 3))
    bad("kernel_size must be >= 1, got \\(0, 3\\)", kernel_size=(0, 3))
    bad("kernel_size must be an int or a pair of ints", TypeError, kernel_size=3.0)
    bad("stride must be >= 1, got \\(0, 0\\)", stride=0)
    bad("dilation must be >= 1, got \\(1, 0\\)", dilation=(1, 0))
    bad("padding must be >= 0, got \\(-1, -1\\)", padding=-1)
    bad("stride must lie in \\[1, MAX_DCNV3_STEP = 65536\\], got \\(65537, 1\\)", stride=(65537, 1))
    bad("group_channels must lie in \\[1, MAX_DCNV3_CHANNELS = 256\\], got 257", a=args(group=1, gc=257), group=1)
    bad("offset_scale must be finite, got nan", offset_scale=float("nan"))
    bad("offset_scale must be finite, got inf", offset_scale=float("inf"))
    bad("offset_scale must be a float, got '1'", TypeError, offset_scale="1")
    bad("im2col_step must be an int, got 2.0", TypeError, im2col_step=2.0)
    bad("im2col_step must be at least 1, got 0", im2col_step=0)
    bad("input must be float32, float16 or bfloat16, got torch.float64", TypeError, a=args(dtype=F64))
    bad("offset must be float32, got torch.float16", TypeError, a=args(off_dtype=torch.float16))
    bad("mask must be float32 or the input's torch.float16, got torch.bfloat16", TypeError,
        a=args(dtype=torch.float16)[:2] + [args(dtype=torch.bfloat16)[2]])
    bad("input must be a torch.Tensor", TypeError, a=[None] + args()[1:])
    with pytest.raises(ValueError, match="input must be a tensor on the GPU.*no CPU implementation"):
        ops.dcnv3(*args(device="cpu"), 3, padding=1, group=2)
    with pytest.raises(ValueError, match="group \\* group_channels must equal input's 8 channels, got group 2 and group_channels 3"):
        ops.DCNv3Function.apply(*args(), 3, 3, 1, 1, 1, 1, 1, 1, 2, 3, 1.0, 256)
    with FakeTensorMode():
        with pytest.raises(ValueError, match="input and mask must be on the same device"):
            a = args(device="cuda")
            a[2] = args()[2]
            ops.dcnv3(*a, 3, padding=1, group=2)


def test_the_index_limits_are_named_and_follow_im2col_step():
    a = args(n=4, h=2 ** 14, w=2 ** 14, group=2, gc=1, kernel=(1, 1), stride=(2 ** 14, 2 ** 14), pad=(0, 0))      # 4 * 2^28 * 2 cells
    with pytest.raises(ValueError, match="32-bit cell indices: 4 images x H x W x G = 2147483648 > MAX_MSDA_INDEX = 2147482623"):
        ops.dcnv3(*a, 1, stride=2 ** 14, group=2)
    assert ops.dcnv3(*a, 1, stride=2 ** 14, group=2, im2col_step=3).shape == (4, 1, 1, 2)
    a = args(n=2, h=2896, w=2896, group=1, gc=1, kernel=(7, 7), pad=(3, 3))                                      # 2 * 2896^2 * 49 * 4 entries
    with pytest.raises(ValueError, match="32-bit plan indices: 2 images x Ho x Wo x G x K x 4 = 3287631872 > MAX_MSDA_INDEX"):
        ops.dcnv3(*a, 7, padding=3)
    assert ops.dcnv3(*a, 7, padding=3, im2col_step=1).shape == (2, 2896, 2896, 1)
    assert ops.dcnv3(*args(group=1, gc=256, kernel=(7, 7), pad=(3, 3)), 7, padding=3).shape == (2, 5, 6, 256)     # the limits are served


@pytest.mark.parametrize("dtype, off_dtype", [(F32, F32), (torch.float16, F32), (torch.float16, torch.float16), (torch.bfloat16, F32),
                                              (torch.bfloat16, torch.bfloat16)])
def test_meta_and_fake_shapes_and_dtypes(dtype, off_dtype):
    for device in ("meta", "fake"):
        mode = FakeTensorMode() if device == "fake" else None
        if mode:
            mode.__enter__()
        try:
            a = args(device="cuda" if mode else "meta", dtype=dtype, off_dtype=off_dtype, kernel=(3, 2), stride=(2, 1), pad=(1, 0), dil=(2, 1))
            for t in a:
                t.requires_grad_(True)
            a[1] = a[1].transpose(1, 2).contiguous().transpose(1, 2)                 # a non-contiguous argument
            y = ops.dcnv3(*a, (3, 2), (2, 1), (1, 0), (2, 1), 2, 0.5, 1)
            assert y.shape == (2, 2, 5, 8) and y.dtype == dtype and y.is_contiguous() and y.requires_grad
            assert ops.DCNv3Function.apply(*a, 3, 2, 2, 1, 1, 0, 2, 1, 2, 4, 0.5, 256).shape == y.shape
            if not mode:
                dx, do, dm = torch.autograd.grad(y.sum(), a)
                assert (dx.shape, dx.dtype) == (a[0].shape, dtype)
                assert (do.shape, do.dtype) == (a[1].shape, off_dtype) and (dm.shape, dm.dtype) == (a[2].shape, off_dtype)
        finally:
            if mode:
                mode.__exit__(None, None, None)


def test_backward_on_meta_skips_what_is_not_needed_and_double_backward_raises():
    a = args()
    grad = torch.empty((2, 5, 6, 8), device="meta")
    tail = (3, 3, 1, 1, 1, 1, 1, 1, 2, 4, 1.0, 256)
    for needs in ([True, False, False], [False, True, False], [False, False, True], [True, True, True], [False, False, False]):
        got = torch.ops.frcnn.dcnv3_backward(grad, *a, *tail, needs)
        assert [tuple(g.shape) for g in got] == [tuple(t.shape) if need else (0,) for t, need in zip(a, needs)]
    a[0].requires_grad_(True)
    y = ops.dcnv3(*a, 3, padding=1, group=2)
    dx, = torch.autograd.grad(y.sum(), a[0], create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        dx.sum().backward()


def test_empty_calls_on_meta():
    for changes, call in ((dict(n=0), dict(padding=1)), (dict(h=1, pad=(0, 0)), dict(padding=0)), (dict(w=2, pad=(1, 0)), dict(padding=(1, 0)))):
        a = args(**changes)
        for t in a:
            t.requires_grad_(True)
        y = ops.dcnv3(*a, 3, group=2, **call)
        assert y.numel() == 0 and y.shape == tuple(a[1].shape[:3]) + (8,)
        y.sum().backward()
        assert all(t.grad.shape == t.shape for t in a)


# ---- 4. the C entry points -----------------------------------------------------------------------------------------------------------------
GOOD = dict(n=2, h=5, w=6, g=2, gc=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
BAD = [dict(n=0), dict(h=0), dict(w=0), dict(g=0), dict(gc=0), dict(gc=257), dict(kh=0), dict(kh=8), dict(kw=0), dict(kw=8), dict(sh=0),
       dict(sw=0), dict(dh=0), dict(dw=0), dict(ph=-1), dict(pw=-1), dict(sh=65537), dict(pw=65537), dict(dh=65537), dict(n=-1),
       dict(h=2 ** 24 + 1), dict(h=2, ph=0), dict(w=4, pw=0, dw=2, kw=3), dict(n=4, h=2 ** 14, w=2 ** 14, g=2),
       dict(n=2, h=2 ** 12, w=2 ** 12, g=1, kh=7, kw=7, ph=3, pw=3)]


def test_entry_points_validate_before_touching_a_gpu():
    lib = nv.lib()
    P = 4096                                  # any aligned non-null pointer: every call below returns before a launch

    def dims(changes, with_gc=True):
        a = dict(GOOD, **changes)
        return tuple(a[k] for k in GOOD if with_gc or k != "gc")

    def forward(elem, ptrs, scale=1.0, **changes):
        tail = tuple(ptrs[:3]) + dims(changes) + (scale, ptrs[3], None)
        return lib.frcnn_ops_dcnv3_forward(*tail) if elem is None else lib.frcnn_ops_dcnv3_forward_16(elem, *tail)

    def backward_offset(elem, ptrs, scale=1.0, **changes):
        tail = tuple(ptrs[:4]) + dims(changes) + (scale, ptrs[4], ptrs[5], None)
        return lib.frcnn_ops_dcnv3_backward_offset(*tail) if elem is None else lib.frcnn_ops_dcnv3_backward_offset_16(elem, *tail)

    def plan(ptrs, scale=1.0, **changes):
        return lib.frcnn_ops_dcnv3_plan(*ptrs[:2], *dims(changes, with_gc=False), scale, ptrs[2], ptrs[3], None)

    def backward_input(elem, ptrs, ws=P, ws_bytes=1 << 20, **changes):
        tail = tuple(ptrs[:4]) + dims(changes) + (ptrs[4], ws, ws_bytes, None)
        return lib.frcnn_ops_dcnv3_backward_input(*tail) if elem is None else lib.frcnn_ops_dcnv3_backward_input_16(elem, *tail)

    def nulls(n, optional=()):
        for i in range(n):
            if i not in optional:
                yield [None if j == i else P for j in range(n)]

    need = lib.frcnn_ops_dcnv3_workspace_bytes(*dims({}))
    windows = -(-2 * 5 * 6 * 2 * 9 * 4 // K.segment())                     # of the plan's entries: two rows of gc sums each
    assert need >= (2 * 5 * 6 * 2 + 1) * 4 + windows * 2 * 4 * 4 and need % 256 == 0
    assert need == lib.frcnn_ops_msda_workspace_bytes(2, 30, 2, 4, 30, 1, 9)         # the gather's: L = 1, P = K, M = G, D = Gc
    for changes in BAD:
        assert lib.frcnn_ops_dcnv3_workspace_bytes(*dims(changes)) == 0, changes
    for elem in (None, nv.OPS_F16, nv.OPS_BF16):
        for ptrs in nulls(4):
            assert forward(elem, ptrs) == -1
        for ptrs in nulls(6, optional=(4, 5)):
            assert backward_offset(elem, ptrs) == -1
        assert backward_offset(elem, [P] * 4 + [None, None]) == -1         # neither gradient asked for
        for ptrs in nulls(5):
            assert backward_input(elem, ptrs) == -1
        assert backward_input(elem, [P] * 5, ws=None) == -1
        assert backward_input(elem, [P] * 5, ws=P + 4) == -1               # a misaligned workspace
        assert backward_input(elem, [P] * 5, ws_bytes=need - 1) == -1      # too small a workspace
        for scale in (float("nan"), float("inf"), -float("inf")):
            assert forward(elem, [P] * 4, scale=scale) == -1 and backward_offset(elem, [P] * 6, scale=scale) == -1
        for changes in BAD:
            assert forward(elem, [P] * 4, **changes) == -1, changes
            assert backward_offset(elem, [P] * 6, **changes) == -1, changes
            assert backward_input(elem, [P] * 5, ws_bytes=1 << 62, **changes) == -1, changes
    for ptrs in nulls(4):
        assert plan(ptrs) == -1
    assert plan([P] * 4, scale=float("nan")) == -1
    for changes in BAD:
        if "gc" not in changes:
            assert plan([P] * 4, **changes) == -1, changes
    for elem in (0, 3, -1):
        assert forward(elem, [P] * 4) == -1 and backward_offset(elem, [P] * 6) == -1 and backward_input(elem, [P] * 5) == -1


# ---- 5. the module -------------------------------------------------------------------------------------------------------------------------
NAMES = ["dw_conv.0.weight", "dw_conv.0.bias", "dw_conv.1.1.weight", "dw_conv.1.1.bias", "offset.weight", "offset.bias", "mask.weight",
         "mask.bias", "input_proj.weight", "input_proj.bias", "output_proj.weight", "output_proj.bias"]


def test_module_owns_upstreams_parameters_and_loads_strict():
    torch.manual_seed(0)
    mod = ops.DCNv3()
    shapes = [(64, 1, 3, 3), (64,), (64,), (64,), (72, 64), (72,), (36, 64), (36,), (64, 64), (64,), (64, 64), (64,)]
    sd = mod.state_dict()
    assert list(sd) == NAMES and [tuple(sd[k].shape) for k in NAMES] == shapes
    small = ops.DCNv3(channels=12, kernel_size=5, dw_kernel_size=3, pad=2, group=3)
    assert [tuple(v.shape) for v in small.state_dict().values()] == [(12, 1, 3, 3), (12,), (12,), (12,), (150, 12), (150,), (75, 12), (75,),
                                                                      (12, 12), (12,), (12, 12), (12,)]
    gen = torch.Generator().manual_seed(1)
    theirs = {k: torch.randn(shape, generator=gen) for k, shape in zip(NAMES, shapes)}       # a hand-built upstream-named checkpoint
    mod.load_state_dict(theirs, strict=True)
    assert all(torch.equal(mod.state_dict()[k], theirs[k]) for k in NAMES)
    with pytest.raises(ValueError, match="channels must be divisible by group, got 10 and 4"):
        ops.DCNv3(channels=10)
    for flag in ("center_feature_scale", "remove_center"):
        with pytest.raises(NotImplementedError, match=flag):
            ops.DCNv3(**{flag: True})
    assert "group=4" in repr(mod) and mod.dw_conv[1][1].eps == 1e-6 and mod.dw_conv[0].groups == 64


def test_module_init_is_upstreams():
    torch.manual_seed(0)
    mod = ops.DCNv3(channels=64, group=4)
    for head in (mod.offset, mod.mask):
        assert not bool(head.weight.any()) and not bool(head.bias.any())
    bound = (6.0 / (64 + 64)) ** 0.5                                       # Xavier-uniform
    for proj in (mod.input_proj, mod.output_proj):
        w = proj.weight.detach()
        assert not bool(proj.bias.any())
        assert 0.98 * bound < float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) < 0.03 * bound
    # zero offsets and a uniform softmax: the freshly built module is a 3 x 3 mean filter between its projections
    x = torch.randn(2, 5, 6, 64)
    want = mod.output_proj(torch.nn.functional.avg_pool2d(mod.input_proj(x).permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1))
    assert float((mod(x) - want).detach().abs().max()) < 1e-5


def test_module_cpu_forward_is_the_restatement():
    torch.manual_seed(2)
    mod = ops.DCNv3(channels=12, kernel_size=3, dw_kernel_size=5, pad=1, group=3, offset_scale=1.5).double()
    torch.nn.init.normal_(mod.offset.weight, std=0.5)
    torch.nn.init.normal_(mod.mask.weight, std=0.5)
    x = torch.randn(2, 5, 6, 12, dtype=F64)
    out = mod(x)
    assert out.shape == x.shape
    x1 = torch.nn.functional.gelu(torch.nn.functional.layer_norm(mod.dw_conv[0](x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1), (12,),
                                                                 mod.dw_conv[1][1].weight, mod.dw_conv[1][1].bias, 1e-6))
    offset = mod.offset(x1)
    mask = mod.mask(x1).view(2, 5, 6, 3, 9).softmax(-1).view(2, 5, 6, 27)
    assert float(offset.detach().abs().max()) > 0.5
    want = mod.output_proj(K.dcnv3_explicit(mod.input_proj(x), offset, mask, *K.geometry((3, 3), (1, 1), (1, 1), (1, 1), 3, 4, 1.5)))
    assert float((want - out).detach().abs().max()) < 1e-12
