"""fasterrcnn_amd.ops.carafe / CARAFEPack on the GPU against the float64 truth of tests/carafe_cases.py and on the exact properties
the kernels promise: shifted copies, group isolation, determinism, the 16-bit contract, layouts, empty inputs.

Every comparison with the truth runs under the derived bound of tests/carafe_cases.py, |got - truth| <= (n + 1) * 2**-23 * S
elementwise (n = k k for the forward, k k s s for d_features, C / G for d_masks; S the restatement on absolute values), and an element
whose bound is 0 must be exactly 0.  Each test prints the largest err / bound it saw.

Largest err / bound measured on an MI355X over every case below: out 0.237 (k1-g2), d_features 0.142 (k1-g2), d_masks 0.291
(tile+1-s1), CARAFEPack's average pooling 0.032.  Information, not a gate."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fasterrcnn_amd import ops

from tests import carafe_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
F32, F64 = torch.float32, torch.float64
HALF = [torch.float16, torch.bfloat16]


def on_gpu(t):
    """t on the GPU in its own layout: a tensor that is dense in neither format arrives as a slice of a wider one."""
    if t.is_contiguous() or t.is_contiguous(memory_format=CL):
        return t.to(DEV)
    view = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype, device=DEV)[..., 1:]
    view.copy_(t)
    assert not view.is_contiguous()
    return view


def run(x, m, grad, k, G, s, need=(True, True)):
    """(out, d_features or None, d_masks or None) of ops.carafe on the GPU, keeping the arguments' layouts."""
    x = on_gpu(x).requires_grad_(need[0])
    m = on_gpu(m).requires_grad_(need[1])
    out = ops.carafe(x, m, k, G, s)
    if any(need):
        out.backward(grad.to(DEV))
    return out.detach(), x.grad, m.grad


@functools.lru_cache(maxsize=None)
def gpu_result(name):
    """The float32 GPU result of a case, shared by the tests that compare against it.  Cached: do not modify."""
    return run(*K.case(name))


def logical(t):
    """The CPU copy of a tensor by its logical index, whatever its memory format."""
    return t.detach().cpu().contiguous()


# ---- 1. against the float64 truth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_forward_and_gradients_against_float64(name):
    truths, bounds = K.reference(name)
    got = gpu_result(name)
    ratios = []
    for label, g, truth, bound in zip(("out", "d_features", "d_masks"), got, truths, bounds):
        assert g.shape == truth.shape and g.dtype == F32, label
        assert float(truth.abs().max()) > 0.1, label
        ratios.append(K.ratio(g, truth, bound))
    print("%s err / bound: out %.3f d_features %.3f d_masks %.3f" % ((name,) + tuple(ratios)))
    assert max(ratios) <= 1.0, (name, ratios)


# ---- 2. exact properties -----------------------------------------------------------------------------------------------------------------------
def one_hot_masks(n, G, k, i, j, oh, ow):
    m = torch.zeros((n, G, k * k, oh, ow))
    m[:, :, i * k + j] = 1.0
    return m.view(n, G * k * k, oh, ow)


@pytest.mark.parametrize("k, s, i, j", [(3, 2, 1, 1), (5, 2, 2, 2), (5, 2, 0, 3), (5, 3, 4, 1), (7, 1, 6, 2), (3, 2, 2, 0)])
def test_one_hot_masks_give_the_zero_padded_shifted_copy(k, s, i, j):
    """Tap (i, j) alone reads features[ph // s - r + i, pw // s - r + j]: the centre tap is nearest-neighbour upsampling, any other the
    same copy shifted, zeros moving in at the border.  The asymmetric taps fail a kernel that swaps its axes."""
    n, c, G, h, w, r = 2, 4, 2, 5, 7, (k - 1) // 2
    x = torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(7))
    out = ops.carafe(x.to(DEV), one_hot_masks(n, G, k, i, j, s * h, s * w).to(DEV), k, G, s)
    shifted = F.pad(x, (r, r, r, r))[:, :, i:i + h, j:j + w]
    want = shifted.repeat_interleave(s, dim=2).repeat_interleave(s, dim=3)
    if (i, j) == (r, r):
        assert torch.equal(want, F.interpolate(x, scale_factor=s, mode="nearest"))
    assert torch.equal(out.cpu(), want)


def test_k1_s1_with_masks_of_ones_returns_the_features():
    x = torch.randn((2, 5, 9, 70), generator=torch.Generator().manual_seed(8)).to(DEV)
    assert torch.equal(ops.carafe(x, torch.ones((2, 1, 9, 70), device=DEV), 1, 1, 1), x)


def test_zeroing_one_groups_masks_zeroes_exactly_its_channels():
    x, m, grad, k, G, s = K.case("k7-g2")
    c = x.shape[1]
    full = ops.carafe(x.to(DEV), m.to(DEV), k, G, s)
    m0 = m.clone()
    m0[:, k * k:] = 0.0
    out = ops.carafe(x.to(DEV), m0.to(DEV), k, G, s)
    assert torch.equal(out[:, :c // 2], full[:, :c // 2]) and bool(full[:, c // 2:].abs().min() > 0)
    assert not bool(out[:, c // 2:].any())


@pytest.mark.parametrize("name", ["two-tiles-s2", "chunk+1-g2", "k7-g2"])
def test_two_runs_are_bit_identical(name):
    a, b = run(*K.case(name)), gpu_result(name)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name", ["k3-s3-c5", "chunk+1-g2", "x-channels-last"])
def test_a_gradient_does_not_depend_on_whether_the_other_is_needed(name):
    both = gpu_result(name)
    out, dx, none = run(*K.case(name), need=(True, False))
    assert none is None and torch.equal(dx, both[1]) and dx.stride() == both[1].stride() and torch.equal(out, both[0])
    out, none, dm = run(*K.case(name), need=(False, True))
    assert none is None and torch.equal(dm, both[2]) and dm.stride() == both[2].stride()


# ---- 3. the 16-bit contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", K.HALF_CASES)
def test_16_bit_tensors_equal_the_float32_operator_rounded_once(name, dtype):
    """op(x_T, m_T) == op(x_T.float(), m_T.float()).to(T) and d_T == backward(grad_T.float(), ...).to(T), bit for bit."""
    x, m, grad, k, G, s = K.case(name)
    x, m, grad = x.to(dtype), m.to(dtype), grad.to(dtype)
    got = run(x, m, grad, k, G, s)
    want = run(x.float(), m.float(), grad.float(), k, G, s)
    for label, g, w in zip(("out", "d_features", "d_masks"), got, want):
        assert g.dtype == dtype and w.dtype == F32, label
        assert torch.equal(g, w.to(dtype)), label
    assert float(got[0].float().abs().max()) > 0.1


@pytest.mark.parametrize("k", K.TIE_KERNELS)
@pytest.mark.parametrize("name", list(K.TIES))
def test_float16_forward_rounds_the_float32_sum_at_a_tie(name, k):
    """tests/carafe_cases.py: the float32 sum of pixel (r, r) is a float16 midpoint and the exact sum lies a quarter of a float32 ulp
    off it.  Rounding the float32 sum gives the even neighbour, `want`; a conversion fused with the last multiply-add gives the other
    one (a library with that fusion returned 1 + 2**-10 for down and up and -(1 + 2**-10) for down-negative, at every k)."""
    x, m, want = K.tie_case(name, k)
    r = (k - 1) // 2
    got = ops.carafe(x.to(DEV), m.to(DEV), k, 1, 1)
    rounded = ops.carafe(x.float().to(DEV), m.float().to(DEV), k, 1, 1).to(torch.float16)
    values = "pixel (r, r) %r, float32 operator rounded %r, want %r" % (float(got[0, 0, r, r]), float(rounded[0, 0, r, r]), want)
    assert got.dtype == torch.float16 and got.shape == (1, 1, k, k)
    assert torch.equal(got, rounded), values
    assert float(got[0, 0, r, r]) == want, values


# ---- 4. layouts and empty inputs ---------------------------------------------------------------------------------------------------------------
def test_layouts_give_the_same_bits_and_gradients_keep_their_format():
    for name in ("x-channels-last", "m-channels-last"):
        x, m, grad, k, G, s = K.case(name)
        out, dx, dm = gpu_result(name)
        assert out.is_contiguous()
        assert dx.stride() == x.stride() and dm.stride() == m.stride()
        assert dx.is_contiguous(memory_format=CL) == (name == "x-channels-last")
        assert dm.is_contiguous(memory_format=CL) == (name == "m-channels-last")
        same = run(x.contiguous(), m.contiguous(), grad, k, G, s)
        assert all(t.is_contiguous() for t in same)
        assert all(torch.equal(logical(a), logical(b)) for a, b in zip((out, dx, dm), same))
    x, m, grad, k, G, s = K.case("slices")
    got = gpu_result("slices")
    assert all(t.is_contiguous() for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, run(x.contiguous(), m.contiguous(), grad, k, G, s)))
    x, m, grad, k, G, s = K.case("x-channels-last")
    cl_grad = run(x, m, grad.contiguous(memory_format=CL), k, G, s)          # a channels_last output gradient is read by logical index too
    assert all(torch.equal(a, b) for a, b in zip(cl_grad, gpu_result("x-channels-last")))


@pytest.mark.parametrize("n, c", [(0, 6), (2, 0)])
def test_empty_n_and_empty_c(n, c):
    x = torch.zeros((n, c, 3, 4), device=DEV, requires_grad=True)
    m = torch.ones((n, 27, 6, 8), device=DEV, requires_grad=True)
    out = ops.carafe(x, m, 3, 3, 2)
    assert out.shape == (n, c, 6, 8) and out.dtype == F32
    out.sum().backward()
    assert x.grad.shape == x.shape and m.grad.shape == m.shape and not bool(m.grad.any()) and not bool(x.grad.any())


def test_double_backward_raises():
    x, m, grad, k, G, s = K.case("n2")
    x = x.to(DEV).requires_grad_(True)
    out = ops.carafe(x, m.to(DEV).requires_grad_(True), k, G, s)
    v = grad.to(DEV).requires_grad_(True)                                   # the backward is linear in v: a second-order graph exists
    gx, = torch.autograd.grad(out, x, v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gx.sum().backward()


OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")


def test_opcheck_passes():
    x, m, grad, k, G, s = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in K.case("n2"))
    torch.library.opcheck(torch.ops.frcnn.carafe.default, (x.clone().requires_grad_(True), m.clone().requires_grad_(True), k, G, s),
                          test_utils=OPCHECK)
    for needs in ([True, True], [True, False], [False, True]):
        torch.library.opcheck(torch.ops.frcnn.carafe_backward.default, (grad, x, m, k, G, s, needs, [False, True]), test_utils=OPCHECK)


# ---- 5. CARAFEPack -----------------------------------------------------------------------------------------------------------------------------
def pack(**config):
    torch.manual_seed(3)
    mod = ops.CARAFEPack(**config)
    torch.nn.init.normal_(mod.content_encoder.weight, std=0.5)             # masks far from uniform
    return mod.to(DEV)


@pytest.mark.parametrize("config", [dict(channels=16, scale_factor=2, compressed_channels=8),
                                    dict(channels=6, scale_factor=3, up_kernel=3, up_group=2, encoder_kernel=5, encoder_dilation=2,
                                         compressed_channels=4)])
def test_pack_is_carafe_on_the_masks_of_its_own_convolutions(config):
    mod = pack(**config)
    x = torch.randn((2, config["channels"], 5, 7), generator=torch.Generator().manual_seed(4)).to(DEV)
    k, G, s = mod.up_kernel, mod.up_group, mod.scale_factor
    with torch.no_grad():
        mod(x)                                                             # the convolutions have chosen their algorithms
        out = mod(x)
        logits = F.pixel_shuffle(mod.content_encoder(mod.channel_compressor(x)), s)
        masks = torch.softmax(logits.view(2, G, k * k, 5 * s, 7 * s), dim=2).view(2, G * k * k, 5 * s, 7 * s)
        assert out.shape == (2, config["channels"], 5 * s, 7 * s)
        assert torch.equal(out, ops.carafe(x, masks, k, G, s))
        assert float((masks.view(2, G, k * k, -1).sum(2) - 1).abs().max()) < 1e-5 and float(masks.max()) > 2.0 / (k * k)


def test_pack_with_a_zeroed_encoder_is_average_pooling():
    """Uniform masks 1 / k k: the output is avg_pool2d(k, stride 1, padding r, count_include_pad=True), nearest-upsampled, under the
    derived forward bound (the rounding of 1 / 25 to float32 is one more relative 2**-24, inside the bound's slack over gamma_25)."""
    mod = pack(channels=5, scale_factor=2, compressed_channels=4)
    torch.nn.init.zeros_(mod.content_encoder.weight)
    x = torch.randn((2, 5, 6, 9), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        out = mod(x.to(DEV))
    truth = F.interpolate(F.avg_pool2d(x.to(F64), 5, stride=1, padding=2, count_include_pad=True), scale_factor=2, mode="nearest")
    uniform = torch.full((2, 25, 12, 18), 1.0 / 25.0, dtype=F64)
    bound = 26 * K.UNIT * K.carafe_ref(x.abs(), uniform, 5, 1, 2)
    assert float(truth.abs().max()) > 0.1
    ratio = K.ratio(out, truth, bound)
    print("pack average pooling err / bound %.3f" % ratio)
    assert ratio <= 1.0


def test_one_sgd_step_changes_both_convolutions():
    mod = pack(channels=8, scale_factor=2, compressed_channels=4)
    gen = torch.Generator().manual_seed(6)
    x, target = torch.randn((2, 8, 5, 6), generator=gen).to(DEV), torch.randn((2, 8, 10, 12), generator=gen).to(DEV)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    opt = torch.optim.SGD(mod.parameters(), lr=0.1)
    loss = (mod(x) * target).sum()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) for p in mod.parameters())
    opt.step()
    for name, value in mod.state_dict().items():
        assert not torch.equal(value, before[name]), name
