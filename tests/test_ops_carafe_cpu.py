"""fasterrcnn_amd.ops.carafe / CARAFE / CARAFEPack without a GPU: the self-checks of the restatements in tests/carafe_cases.py, the
argument rules of the public function, shapes, dtypes and memory formats on meta and fake tensors, the validation of the C entry
points, and CARAFEPack's parameters."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import carafe_cases as K

F32, F64 = torch.float32, torch.float64
CL = torch.channels_last
CHECKED = ("edges-2x3-k5", "edges-1x1-k3", "k1-g2", "k3-s3-c5", "k5-s1-g3", "k7-g2", "n2", "denormals")


# ---- 1. the restatements -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHECKED)
def test_the_two_restatements_agree_in_float64(name):
    x, m, grad, k, G, s = K.case(name)
    a, b = K.carafe_ref(x, m, k, G, s), K.carafe_unfold(x, m, k, G, s)
    assert a.shape == (x.shape[0], x.shape[1], s * x.shape[2], s * x.shape[3]) and a.dtype == F64
    assert float((a - b).abs().max()) <= 1e-12
    for ga, gb in zip(K.gradients(K.carafe_ref, x, m, grad, k, G, s), K.gradients(K.carafe_unfold, x, m, grad, k, G, s)):
        assert ga.shape == gb.shape and float((ga - gb).abs().max()) <= 1e-12


def test_the_hand_computed_example():
    x, m, want = K.hand_example()
    for fn in (K.carafe_ref, K.carafe_unfold):
        assert torch.equal(fn(x, m, 3, 1, 2), want)


def test_the_gradient_restatements_are_the_autograd_gradients():
    x, m, grad, k, G, s = K.case("k3-s3-c5")
    dx, dm = K.gradients(K.carafe_ref, x, m, grad, k, G, s)
    assert torch.equal(K.d_features_ref(grad, m, x.shape[1], k, G, s), dx) and torch.equal(K.d_masks_ref(grad, x, k, G, s), dm)
    # d_masks of a tap outside the map is 0: pixel (0, 0) of a k = 3 window has its first row and column outside
    assert not bool(dm.view(1, 9, 12, 15)[0, [0, 1, 2, 3, 6], 0, 0].any()) and bool(dm.view(1, 9, 12, 15)[0, 4, 0, 0] != 0)


@pytest.mark.parametrize("name", list(K.CASES))
def test_every_case_is_non_trivial_and_its_bounds_are_small(name):
    (out, dx, dm), bounds = K.reference(name)
    for truth, bound in zip((out, dx, dm), bounds):
        assert truth.shape == bound.shape and float(truth.abs().max()) > 0.1
        assert bool((bound >= 0).all()) and float(bound.max()) < 1e-3 * float(truth.abs().max())
        assert K.ratio(truth.to(F32), truth, bound) <= 1.0                 # rounding the truth once is far inside the bound
    x, m, grad, k, G, s = K.case(name)
    wrong = K.carafe_ref(x, m.roll(1, dims=1), k, G, s)                     # an indexing mistake (the taps off by one) lands far outside
    assert K.ratio(wrong, out, bounds[0]) > 1e3


def test_the_cases_sit_on_the_kernels_seams():
    assert (K.MAX_KERNEL, K.CHUNK, K.TILE_W, K.TILE_H) == (7, 64, 64, 4) and ops.MAX_CARAFE_KERNEL == K.MAX_KERNEL
    shapes = {name: c for name, c in K.CASES.items()}
    assert {c[4] for c in shapes.values()} == {1, 3, 5, 7} and {c[6] for c in shapes.values()} >= {1, 2, 3}
    assert {c[5] for c in shapes.values()} >= {1, 2, 3}
    assert {c[6] * c[3] for c in shapes.values()} >= {K.TILE_W - 1, K.TILE_W + 1}
    assert {c[6] * c[2] for c in shapes.values()} >= {K.TILE_H - 1, K.TILE_H + 1}
    assert {c[1] for c in shapes.values()} >= {K.CHUNK - 1, K.CHUNK + 1}
    x = K.case("denormals")[0]
    tiny = (x != 0) & (x.abs() < torch.finfo(F32).tiny)
    assert int(tiny.sum()) >= 6 and bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())


# ---- 2. the interface ----------------------------------------------------------------------------------------------------------------------
def args(n=2, c=6, h=3, w=4, k=3, g=3, s=2, device="meta", dtype=F32):
    e = lambda *shape: torch.empty(shape, device=device, dtype=dtype)       # noqa: E731
    return [e(n, c, h, w), e(n, g * k * k, s * h, s * w), k, g, s]


def test_the_names_are_exported():
    for name in ("carafe", "CARAFE", "CARAFEPack"):
        assert name in ops.__all__ and hasattr(ops, name)
    for name in ("carafe", "carafe_backward"):
        assert hasattr(torch.ops.frcnn, name)
    assert ops.MAX_CARAFE_KERNEL == 7 and ops.MAX_CARAFE_SCALE == 8 and ops.MAX_CARAFE_PLANE == 2 ** 31 - 1 - 1024


def test_argument_errors():
    e = lambda *shape: torch.empty(shape, device="meta")                    # noqa: E731

    def bad(match, error=ValueError, **changes):
        a = dict(zip(("features", "masks", "kernel_size", "group_size", "scale_factor"), args()))
        a.update(changes)
        with pytest.raises(error, match=match):
            ops.carafe(**a)

    bad("kernel_size must be odd, got 4", kernel_size=4, masks=e(2, 48, 6, 8))
    bad("kernel_size must lie in \\[1, 7\\].*got 9", kernel_size=9, masks=e(2, 243, 6, 8))
    bad("kernel_size must lie in \\[1, 7\\].*got 0", kernel_size=0)
    bad("kernel_size must be an int", TypeError, kernel_size=3.0)
    bad("group_size must divide.*group_size 4 for 6 channels", group_size=4, masks=e(2, 36, 6, 8))
    bad("group_size must lie in.*got 0", group_size=0)
    bad("scale_factor must lie in \\[1, 8\\].*got 9", scale_factor=9, masks=e(2, 27, 27, 36))
    bad("scale_factor must lie in \\[1, 8\\].*got 0", scale_factor=0)
    bad("masks must be \\[N.*= \\[2, 27, 6, 8\\], got shape \\(2, 18, 6, 8\\)", masks=e(2, 18, 6, 8))       # the wrong mask channels
    bad("masks must be \\[N.*got shape \\(2, 27, 3, 4\\)", masks=e(2, 27, 3, 4))                            # the low-resolution size
    bad("masks must be \\[N.*got shape \\(2, 27, 6, 9\\)", masks=e(2, 27, 6, 9))
    bad("masks must be \\[N.*got shape \\(1, 27, 6, 8\\)", masks=e(1, 27, 6, 8))
    bad("masks must be \\[N", masks=e(27, 6, 8))
    bad("features must be \\[N, C, H, W\\]", features=e(6, 3, 4))
    bad("at least one cell", features=e(2, 6, 0, 4), masks=e(2, 27, 0, 8))
    bad("one dtype.*torch.float32 and torch.float16", TypeError, masks=args(dtype=torch.float16)[1])
    bad("one dtype", TypeError, features=args(dtype=torch.bfloat16)[0])
    bad("features must be float32, float16 or bfloat16, got torch.float64", TypeError, features=args(dtype=F64)[0], masks=args(dtype=F64)[1])
    bad("masks must be float32, float16 or bfloat16, got torch.float64", TypeError, masks=args(dtype=F64)[1])
    bad("features must be a torch.Tensor", TypeError, features=None)
    with pytest.raises(ValueError, match="features must be a tensor on the GPU.*no CPU implementation"):
        ops.carafe(*args(device="cpu"))
    with FakeTensorMode():
        with pytest.raises(ValueError, match="features and masks must be on the same device"):
            ops.carafe(args(device="cuda")[0], *args()[1:])


def test_the_index_limits_are_named():
    e = lambda *shape: torch.empty(shape, device="meta")                    # noqa: E731
    with pytest.raises(ValueError, match="MAX_CARAFE_PLANE"):               # 2 * 32768 * 2 * 16384 = 2^31
        ops.carafe(e(1, 1, 32768, 16384), e(1, 1, 65536, 32768), 1, 1, 2)
    with pytest.raises(ValueError, match="at most 65535 images"):
        ops.carafe(e(65536, 1, 1, 1), e(65536, 1, 1, 1), 1, 1, 1)
    with pytest.raises(ValueError, match="at most 65535 runs"):
        ops.carafe(e(1, 65536, 1, 1), e(1, 65536, 1, 1), 1, 65536, 1)
    assert ops.carafe(e(1, 4 * 65535, 1, 1), e(1, 1, 1, 1), 1, 1, 1).shape == (1, 4 * 65535, 1, 1)


@pytest.mark.parametrize("dtype", [F32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("x_cl, m_cl", [(False, False), (True, False), (False, True), (True, True)])
def test_meta_and_fake_shapes_dtypes_and_memory_formats(dtype, x_cl, m_cl):
    for device in ("meta", "fake"):
        mode = FakeTensorMode() if device == "fake" else None
        if mode:
            mode.__enter__()
        try:
            x, m, k, g, s = args(device="cuda" if mode else "meta", dtype=dtype)
            x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(True)
            m = (m.contiguous(memory_format=CL) if m_cl else m).requires_grad_(True)
            y = ops.carafe(x, m, k, g, s)
            assert y.shape == (2, 6, 6, 8) and y.dtype == dtype and y.is_contiguous() and y.requires_grad
            assert ops.CARAFE(k, g, s)(x, m).shape == y.shape
            if not mode:
                y.sum().backward()
                for t in (x, m):
                    assert t.grad.shape == t.shape and t.grad.stride() == t.stride() and t.grad.dtype == dtype
        finally:
            if mode:
                mode.__exit__(None, None, None)


def test_backward_on_meta_skips_what_is_not_needed():
    x, m, k, g, s = args()
    grad = torch.empty((2, 6, 6, 8), device="meta")
    dx, dm = torch.ops.frcnn.carafe_backward(grad, x, m, k, g, s, [True, False], [True, False])
    assert dx.shape == x.shape and dx.is_contiguous(memory_format=CL) and dm.shape == (0,)
    dx, dm = torch.ops.frcnn.carafe_backward(grad, x, m, k, g, s, [False, True], [False, False])
    assert dx.shape == (0,) and dm.shape == m.shape and dm.is_contiguous()


def test_empty_calls_on_meta():
    for n, c in ((0, 6), (2, 0)):
        x, m, k, g, s = args(n=n, c=c, g=3)
        x.requires_grad_(True), m.requires_grad_(True)
        y = ops.carafe(x, m, k, g, s)
        assert y.shape == (n, c, 6, 8)
        y.sum().backward()
        assert x.grad.shape == x.shape and m.grad.shape == m.shape


# ---- 3. the C entry points -----------------------------------------------------------------------------------------------------------------
GOOD = dict(n=2, c=6, h=3, w=4, k=3, g=3, s=2)
BAD = [dict(n=0), dict(n=65536), dict(c=0), dict(h=0), dict(w=0), dict(k=0), dict(k=2), dict(k=9), dict(k=-1), dict(g=0), dict(g=4),
       dict(s=0), dict(s=9), dict(h=32768, w=16384), dict(c=4 * 65536, g=1), dict(c=65536, g=65536)]


def test_entry_points_validate_before_touching_a_gpu():
    lib = nv.lib()
    P = 4096                                  # any aligned non-null pointer: every call below returns before a launch

    def forward(elem, x, m, out, **changes):
        a = dict(GOOD, **changes)
        tail = (x, m, a["n"], a["c"], a["h"], a["w"], a["k"], a["g"], a["s"], out, None)
        return lib.frcnn_ops_carafe(*tail) if elem is None else lib.frcnn_ops_carafe_16(elem, *tail)

    def backward(elem, x, m, grad, dx, dm, **changes):
        a = dict(GOOD, **changes)
        tail = (x, m, grad, a["n"], a["c"], a["h"], a["w"], a["k"], a["g"], a["s"], dx, dm, None)
        return lib.frcnn_ops_carafe_backward(*tail) if elem is None else lib.frcnn_ops_carafe_backward_16(elem, *tail)

    for elem in (None, nv.OPS_F16, nv.OPS_BF16):
        for ptrs in ((None, P, P), (P, None, P), (P, P, None)):
            assert forward(elem, *ptrs) == -1
        for ptrs in ((P, P, None, P, P), (None, P, P, P, P), (P, None, P, P, P), (None, P, P, None, P), (P, None, P, P, None)):
            assert backward(elem, *ptrs) == -1                             # no gradient; d_masks without features; d_features without masks
        for changes in BAD:
            assert forward(elem, P, P, P, **changes) == -1, changes
            assert backward(elem, P, P, P, P, P, **changes) == -1, changes
    for elem in (0, 3, -1):
        assert forward(elem, P, P, P) == -1 and backward(elem, P, P, P, P, P) == -1


# ---- 4. CARAFEPack -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config, shapes", [
    (dict(channels=256, scale_factor=2), [(64, 256, 1, 1), (64,), (100, 64, 3, 3), (100,)]),
    (dict(channels=12, scale_factor=3, up_kernel=3, up_group=2, encoder_kernel=5, encoder_dilation=2, compressed_channels=8),
     [(8, 12, 1, 1), (8,), (162, 8, 5, 5), (162,)])])
def test_pack_owns_mmcvs_parameters(config, shapes):
    torch.manual_seed(0)
    mod = ops.CARAFEPack(**config)
    sd = mod.state_dict()
    names = ["channel_compressor.weight", "channel_compressor.bias", "content_encoder.weight", "content_encoder.bias"]
    assert list(sd) == names and [tuple(sd[k].shape) for k in names] == shapes
    gen = torch.Generator().manual_seed(1)
    theirs = {k: torch.randn(shape, generator=gen) for k, shape in zip(names, shapes)}       # a hand-built mmcv-named checkpoint
    mod.load_state_dict(theirs, strict=True)
    assert all(torch.equal(mod.state_dict()[k], theirs[k]) for k in names)
    enc = mod.content_encoder
    kernel, dilation = config.get("encoder_kernel", 3), config.get("encoder_dilation", 1)
    assert enc.padding == (int((kernel - 1) * dilation / 2),) * 2 and enc.dilation == (dilation,) * 2
    x = torch.empty((2, config["channels"], 5, 7), device="meta")
    s = config["scale_factor"]
    assert mod.to("meta")(x).shape == (2, config["channels"], 5 * s, 7 * s)


def test_pack_init_is_mmcvs():
    torch.manual_seed(0)
    mod = ops.CARAFEPack(256, 2)
    w = mod.content_encoder.weight.detach()                                # 57600 samples of normal(0, 0.001)
    assert abs(float(w.std()) - 1e-3) < 5e-5 and abs(float(w.mean())) < 2e-5
    assert not bool(mod.content_encoder.bias.any()) and not bool(mod.channel_compressor.bias.any())
    w = mod.channel_compressor.weight.detach()                             # Xavier-uniform: bound sqrt(6 / (256 + 64))
    bound = (6.0 / (256 + 64)) ** 0.5
    assert 0.99 * bound < float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) < 0.02 * bound
    assert "up_kernel=5" in repr(mod) and repr(ops.CARAFE(5, 1, 2)) == "CARAFE(kernel_size=5, group_size=1, scale_factor=2)"
