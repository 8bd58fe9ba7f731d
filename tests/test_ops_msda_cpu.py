"""fasterrcnn_amd.ops.multi_scale_deformable_attn / MultiScaleDeformableAttnFunction / MultiScaleDeformableAttention without a GPU: the
self-checks of the restatements in tests/msda_cases.py, the argument rules of the public function, shapes and dtypes on meta and fake
tensors, the validation of the C entry points, and the module's parameters, init and CPU forward."""
import math

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import msda_cases as K

F32, F64, I64 = torch.float32, torch.float64, torch.int64


# ---- 1. the restatements -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_the_two_restatements_agree_and_every_case_is_non_trivial(name):
    truth, single = K.reference(name)                                      # asserts the agreement and the positions of the samples
    value, shapes, starts, loc, attn, grad = K.case(name)
    b, q, m, d = value.shape[0], loc.shape[1], value.shape[2], value.shape[3]
    assert [tuple(t.shape) for t in truth] == [(b, q, m * d), tuple(value.shape), tuple(loc.shape), tuple(attn.shape)]
    for t, s in zip(truth, single):
        assert t.dtype == F64 and s.dtype == F32 and float(t.abs().max()) > 0.1
        assert K.rel_err(s, t) < 2e-6                                      # a float32 evaluation is a few ulps away
    for axis in (0, 1):                                                    # a share of the samples outside the map on each side
        size = torch.tensor([hw[1 - axis] for hw in shapes], dtype=F64).view(1, 1, 1, -1, 1)
        c = loc[..., axis].to(F64) * size - 0.5
        if K.CASES[name][6] != "spread":
            assert not bool(((c <= -1) | (c >= size)).any())
        elif c.numel() >= 100:                                             # (the smallest cases hold too few samples to say)
            assert bool((c <= -1).any()) and bool((c >= size).any()) and bool(((c > -1) & (c < 0)).any())
            assert 0.05 < float(((c <= -1) | (c >= size)).double().mean()) < 0.6


def test_the_self_check_case_agrees_as_tightly_as_stated():
    value, shapes, starts, loc, attn, grad = K.case("base")
    assert (value.shape, loc.shape) == ((2, 43, 3, 5), (2, 9, 3, 3, 4, 2))
    a = K.msda_explicit(value, shapes, starts, loc.to(F64), attn, grad)
    c = (K.msda_grid_sample(value, shapes, loc.to(F64), attn),) + K.grid_sample_gradients(value, shapes, loc.to(F64), attn, grad)
    assert float((a[0] - c[0]).abs().max()) <= 1e-15
    for x, y in zip(a[1:], c[1:]):
        assert float((x - y).abs().max()) <= 1e-14 * max(1.0, float(x.abs().max()))


def test_the_hand_computed_example():
    value, shapes, starts, loc, attn, want = K.hand_example()
    assert torch.equal(K.msda_explicit(value, shapes, starts, loc, attn)[0], want)
    assert torch.equal(K.msda_grid_sample(value, shapes, loc, attn), want)
    assert torch.equal(ops.multi_scale_deformable_attn_pytorch(value, torch.tensor(shapes), loc, attn), want)
    # the published gradients by hand: d_weight = the samples; the centre point's slope along x is ((2 - 1) + (4 - 3)) / 2 times W = 2
    out, dv, dloc, dattn = K.msda_explicit(value, shapes, starts, loc, attn, torch.ones((1, 1, 1), dtype=F64))
    assert dattn.flatten().tolist() == [2.5, 2.0] and dloc[0, 0, 0, 0, 0].tolist() == [0.5 * 2 * 1.0, 0.5 * 2 * 2.0]
    assert dv.flatten().tolist() == [0.125, 0.125 + 2.0, 0.125, 0.125]


def test_the_cases_sit_on_the_kernels_seams():
    lib = nv.lib()
    assert (lib.frcnn_ops_msda_max_levels(), lib.frcnn_ops_msda_max_points(), lib.frcnn_ops_msda_max_channels()) == (
        ops.MAX_MSDA_LEVELS, ops.MAX_MSDA_POINTS, ops.MAX_MSDA_CHANNELS) == (8, 16, 256)
    shapes = {name: K.case(name) for name in K.CASES}
    dims = {name: (v[0].shape, v[3].shape) for name, v in shapes.items()}
    assert {vs[3] for vs, _ in dims.values()} >= {1, 5, 32, 72, 70}                  # D: scalar, below a run, whole runs, past a wave's
    assert {ls[4] for _, ls in dims.values()} >= {1, 2, 4} and {ls[3] for _, ls in dims.values()} >= {1, 4}
    assert {vs[2] for vs, _ in dims.values()} >= {1, 3}
    assert [1, 2] in [list(hw) for hw in shapes["d32-levels"][1]] and [1, 1] in [list(hw) for hw in shapes["d32-levels"][1]]
    assert any(w % 2 == 1 for _, w in shapes["base"][1])
    assert dims["d1-block"][1][1] == K.block_items(1, 1, 1) + 1                      # one item more than a block serves
    assert dims["chunks"][0][0] == 3
    per_cell = dims["one-cell"][1][1] * dims["one-cell"][1][4]                       # entries on each of the four cells of an image
    assert K.segment() == ops.MSDA_SEGMENT == 512 and per_cell > 2 * K.segment() and (4 * per_cell) % K.segment() != 0
    assert dims["one-cell"][0][0] == 2
    # the mapping the getter reports: D / 4 float32 runs (D / 8 16-bit ones) rounded up to a power of two lanes, 256 lanes a block
    assert K.block_items(32, 4, 4) == 32 and K.block_items(32, 4, 4, nv.OPS_F16) == 64 and K.block_items(256, 1, 1) == 4
    assert K.block_items(5, 1, 1) == 32 and K.block_items(70, 1, 1) == 4 and K.block_items(1, 8, 16) == 8     # 1024 staged samples
    assert lib.frcnn_ops_msda_block_items(0, 1, 1, 0) == 0 and lib.frcnn_ops_msda_block_items(8, 9, 1, 0) == 0
    assert lib.frcnn_ops_msda_block_items(8, 1, 17, 0) == 0 and lib.frcnn_ops_msda_block_items(8, 1, 1, 3) == 0


# ---- 2. the interface ----------------------------------------------------------------------------------------------------------------------
NAMES = ("value", "value_spatial_shapes", "value_level_start_index", "sampling_locations", "attention_weights")


def args(b=2, s=11, m=3, d=5, q=4, levels=2, points=3, device="meta", dtype=F32, loc_dtype=None):
    e = lambda shape, dt: torch.empty(shape, device=device, dtype=dt)       # noqa: E731
    loc_dtype = loc_dtype or dtype
    return [e((b, s, m, d), dtype), e((levels, 2), I64), e((levels,), I64), e((b, q, m, levels, points, 2), loc_dtype),
            e((b, q, m, levels, points), loc_dtype)]


def test_the_names_are_exported():
    for name in ("multi_scale_deformable_attn", "multi_scale_deformable_attn_pytorch", "MultiScaleDeformableAttnFunction",
                 "MultiScaleDeformableAttention"):
        assert name in ops.__all__ and hasattr(ops, name)
    for name in ("ms_deform_attn", "ms_deform_attn_backward"):
        assert hasattr(torch.ops.frcnn, name)
    assert ops.MAX_MSDA_INDEX == 2 ** 31 - 1 - 1024
    assert "multi_scale_deformable_attn(" in ops.__doc__ and "MultiScaleDeformableAttention(" in ops.__doc__


def test_argument_errors():
    e = lambda *shape, dtype=F32: torch.empty(shape, device="meta", dtype=dtype)    # noqa: E731

    def bad(match, error=ValueError, im2col_step=64, **changes):
        a = dict(zip(NAMES, args()))
        a.update(changes)
        with pytest.raises(error, match=match):
            ops.multi_scale_deformable_attn(**a, im2col_step=im2col_step)

    bad("value must be \\[B, S, M, D\\], got shape \\(2, 11, 15\\)", value=e(2, 11, 15))
    bad("sampling_locations must be \\[B, Q, M, L, P, 2\\], got shape \\(2, 4, 3, 2, 3\\)", sampling_locations=e(2, 4, 3, 2, 3))
    bad("sampling_locations must be \\[B, Q, M, L, P, 2\\], got shape \\(2, 4, 3, 2, 3, 3\\)", sampling_locations=e(2, 4, 3, 2, 3, 3))
    bad("with value's B = 2 and M = 3, got shape \\(1, 4, 3, 2, 3, 2\\)", sampling_locations=e(1, 4, 3, 2, 3, 2))
    bad("with value's B = 2 and M = 3, got shape \\(2, 4, 2, 2, 3, 2\\)", sampling_locations=e(2, 4, 2, 2, 3, 2))
    bad("attention_weights must be .* = \\[2, 4, 3, 2, 3\\], got shape \\(2, 4, 3, 2, 4\\)", attention_weights=e(2, 4, 3, 2, 4))
    bad("attention_weights must be .*got shape \\(2, 4, 3, 3, 3\\)", attention_weights=e(2, 4, 3, 3, 3))
    bad("value_spatial_shapes must be \\[L, 2\\] = \\[2, 2\\], got shape \\(3, 2\\)", value_spatial_shapes=e(3, 2, dtype=I64))
    bad("value_level_start_index must be \\[L\\] = \\[2\\], got shape \\(3,\\)", value_level_start_index=e(3, dtype=I64))
    bad("value_spatial_shapes must be int64, got torch.int32", TypeError, value_spatial_shapes=e(2, 2, dtype=torch.int32))
    bad("value_level_start_index must be int64, got torch.float32", TypeError, value_level_start_index=e(2))
    bad("value must be float32, float16 or bfloat16, got torch.float64", TypeError, value=e(2, 11, 3, 5, dtype=F64))
    bad("sampling_locations must be float32, got torch.float64", TypeError, sampling_locations=e(2, 4, 3, 2, 3, 2, dtype=F64))
    bad("attention_weights must be float32, got torch.float16", TypeError, attention_weights=e(2, 4, 3, 2, 3, dtype=torch.float16))
    bad("sampling_locations must be float32 or the value's torch.float16, got torch.bfloat16", TypeError,
        value=e(2, 11, 3, 5, dtype=torch.float16), sampling_locations=e(2, 4, 3, 2, 3, 2, dtype=torch.bfloat16))
    bad("value must be a torch.Tensor", TypeError, value=None)
    bad("im2col_step must be an int, got 2.0", TypeError, im2col_step=2.0)
    bad("im2col_step must be at least 1, got 0", im2col_step=0)
    big = dict(zip(NAMES, args(levels=9)))
    bad("at most MAX_MSDA_LEVELS = 8 levels, got 9", **big)
    bad("at most MAX_MSDA_POINTS = 16 points per level, got 17", **dict(zip(NAMES, args(points=17))))
    bad("at most MAX_MSDA_CHANNELS = 256 channels per head, got 257", **dict(zip(NAMES, args(d=257))))
    with pytest.raises(ValueError, match="value must be a tensor on the GPU.*no CPU implementation"):
        ops.multi_scale_deformable_attn(*args(device="cpu"))
    with FakeTensorMode():
        with pytest.raises(ValueError, match="value and sampling_locations must be on the same device"):
            a = args(device="cuda")
            a[3] = args()[3]
            ops.multi_scale_deformable_attn(*a)


def test_the_index_limits_are_named_and_follow_im2col_step():
    a = args(b=4, s=2 ** 28, m=2, d=1, q=1, levels=1, points=1)                      # 4 * 2^28 * 2 = 2^31 cells
    with pytest.raises(ValueError, match="32-bit cell indices: 4 images x S x M = 2147483648 > MAX_MSDA_INDEX = 2147482623"):
        ops.multi_scale_deformable_attn(*a)
    assert ops.multi_scale_deformable_attn(*a, im2col_step=3).shape == (4, 1, 2)    # chunks of 3 images fit
    a = args(b=2, s=1, m=1, d=1, q=2 ** 21, levels=8, points=16)                     # 2 * 2^21 * 128 * 4 = 2^31 plan entries
    with pytest.raises(ValueError, match="32-bit plan indices: 2 images x Q x M x L x P x 4 = 2147483648 > MAX_MSDA_INDEX"):
        ops.multi_scale_deformable_attn(*a)
    assert ops.multi_scale_deformable_attn(*a, im2col_step=1).shape == (2, 2 ** 21, 1)
    assert ops.multi_scale_deformable_attn(*args(levels=8, points=16, d=256)).shape == (2, 4, 768)     # the limits themselves are served


@pytest.mark.parametrize("dtype, loc_dtype", [(F32, F32), (torch.float16, F32), (torch.float16, torch.float16), (torch.bfloat16, F32),
                                              (torch.bfloat16, torch.bfloat16)])
def test_meta_and_fake_shapes_and_dtypes(dtype, loc_dtype):
    for device in ("meta", "fake"):
        mode = FakeTensorMode() if device == "fake" else None
        if mode:
            mode.__enter__()
        try:
            a = args(device="cuda" if mode else "meta", dtype=dtype, loc_dtype=loc_dtype)
            for i in (0, 3, 4):
                a[i].requires_grad_(True)
            a[3] = a[3].transpose(1, 2).contiguous().transpose(1, 2)                 # a non-contiguous argument
            y = ops.multi_scale_deformable_attn(*a, im2col_step=1)
            assert y.shape == (2, 4, 15) and y.dtype == dtype and y.is_contiguous() and y.requires_grad
            assert ops.MultiScaleDeformableAttnFunction.apply(*a, 64).shape == y.shape
            if not mode:
                value, _, _, loc, attn = a
                dv, dl, da = torch.autograd.grad(y.sum(), (value, loc, attn))
                assert (dv.shape, dv.dtype) == (value.shape, dtype)
                assert (dl.shape, dl.dtype) == (loc.shape, loc_dtype) and (da.shape, da.dtype) == (attn.shape, loc_dtype)
        finally:
            if mode:
                mode.__exit__(None, None, None)


def test_backward_on_meta_skips_what_is_not_needed_and_double_backward_raises():
    a = args()
    grad = torch.empty((2, 4, 15), device="meta")
    for needs in ([True, False, False], [False, True, False], [False, False, True], [True, True, True], [False, False, False]):
        got = torch.ops.frcnn.ms_deform_attn_backward(grad, *a, 64, needs)
        assert [tuple(g.shape) for g in got] == [tuple(t.shape) if need else (0,) for t, need in zip((a[0], a[3], a[4]), needs)]
    a[0].requires_grad_(True)
    y = ops.multi_scale_deformable_attn(*a)
    dv, = torch.autograd.grad(y.sum(), a[0], create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        dv.sum().backward()


def test_empty_calls_on_meta():
    for changes in (dict(b=0), dict(q=0), dict(s=0), dict(m=0), dict(d=0)):
        a = args(**changes)
        for i in (0, 3, 4):
            a[i].requires_grad_(True)
        y = ops.multi_scale_deformable_attn(*a)
        assert y.shape == (a[0].shape[0], a[3].shape[1], a[0].shape[2] * a[0].shape[3])
        y.sum().backward()
        assert all(a[i].grad.shape == a[i].shape for i in (0, 3, 4))


# ---- 3. the C entry points -----------------------------------------------------------------------------------------------------------------
GOOD = dict(n=2, s=11, m=3, d=5, q=4, levels=2, points=3)
BAD = [dict(n=0), dict(s=0), dict(m=0), dict(d=0), dict(d=257), dict(q=0), dict(levels=0), dict(levels=9), dict(points=0), dict(points=17),
       dict(n=-1), dict(n=4, s=2 ** 28, m=2), dict(n=2, q=2 ** 21, m=1, levels=8, points=16), dict(s=2 ** 31 - 1, m=2 ** 31 - 1)]


def test_entry_points_validate_before_touching_a_gpu():
    lib = nv.lib()
    P = 4096                                  # any aligned non-null pointer: every call below returns before a launch

    def dims(changes, with_d=True):
        a = dict(GOOD, **changes)
        return (a["n"], a["s"], a["m"]) + ((a["d"],) if with_d else ()) + (a["q"], a["levels"], a["points"])

    def forward(elem, ptrs, **changes):
        tail = tuple(ptrs[:5]) + dims(changes) + (ptrs[5], None)
        return lib.frcnn_ops_msda_forward(*tail) if elem is None else lib.frcnn_ops_msda_forward_16(elem, *tail)

    def backward_loc(elem, ptrs, **changes):
        tail = tuple(ptrs[:6]) + dims(changes) + (ptrs[6], ptrs[7], None)
        return lib.frcnn_ops_msda_backward_loc(*tail) if elem is None else lib.frcnn_ops_msda_backward_loc_16(elem, *tail)

    def plan(ptrs, **changes):
        return lib.frcnn_ops_msda_plan(*ptrs[:4], *dims(changes, with_d=False), ptrs[4], ptrs[5], None)

    def backward_value(elem, ptrs, ws=P, ws_bytes=1 << 20, **changes):
        tail = tuple(ptrs[:4]) + dims(changes) + (ptrs[4], ws, ws_bytes, None)
        return lib.frcnn_ops_msda_backward_value(*tail) if elem is None else lib.frcnn_ops_msda_backward_value_16(elem, *tail)

    def nulls(n, optional=()):
        for i in range(n):
            if i not in optional:
                yield [None if j == i else P for j in range(n)]

    need = lib.frcnn_ops_msda_workspace_bytes(*dims({}))
    windows = -(-2 * 4 * 3 * 2 * 3 * 4 // K.segment())                     # of the plan's entries: two rows of d sums each
    assert need >= (2 * 11 * 3 + 1) * 4 + windows * 2 * 5 * 4 and need % 256 == 0
    for changes in BAD:
        assert lib.frcnn_ops_msda_workspace_bytes(*dims(changes)) == 0, changes
    for elem in (None, nv.OPS_F16, nv.OPS_BF16):
        for ptrs in nulls(6):
            assert forward(elem, ptrs) == -1
        for ptrs in nulls(8, optional=(6, 7)):
            assert backward_loc(elem, ptrs) == -1
        assert backward_loc(elem, [P] * 6 + [None, None]) == -1            # neither gradient asked for
        for ptrs in nulls(5):
            assert backward_value(elem, ptrs) == -1
        assert backward_value(elem, [P] * 5, ws=None) == -1
        assert backward_value(elem, [P] * 5, ws=P + 4) == -1               # a misaligned workspace
        assert backward_value(elem, [P] * 5, ws_bytes=need - 1) == -1      # too small a workspace
        for changes in BAD:
            assert forward(elem, [P] * 6, **changes) == -1, changes
            assert backward_loc(elem, [P] * 8, **changes) == -1, changes
            assert backward_value(elem, [P] * 5, ws_bytes=1 << 62, **changes) == -1, changes
    for ptrs in nulls(6):
        assert plan(ptrs) == -1
    for changes in BAD:
        if "d" not in changes:
            assert plan([P] * 6, **changes) == -1, changes
    for elem in (0, 3, -1):
        assert forward(elem, [P] * 6) == -1 and backward_loc(elem, [P] * 8) == -1 and backward_value(elem, [P] * 5) == -1


# ---- 4. the module -------------------------------------------------------------------------------------------------------------------------
def test_module_owns_mmcvs_parameters_and_loads_strict():
    torch.manual_seed(0)
    mod = ops.MultiScaleDeformableAttention()
    names = ["sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias",
             "value_proj.weight", "value_proj.bias", "output_proj.weight", "output_proj.bias"]
    shapes = [(256, 256), (256,), (128, 256), (128,), (256, 256), (256,), (256, 256), (256,)]
    sd = mod.state_dict()
    assert list(sd) == names and [tuple(sd[k].shape) for k in names] == shapes
    small = ops.MultiScaleDeformableAttention(embed_dims=12, num_heads=3, num_levels=2, num_points=5, value_proj_ratio=0.5)
    assert [tuple(v.shape) for v in small.state_dict().values()] == [(60, 12), (60,), (30, 12), (30,), (6, 12), (6,), (12, 6), (12,)]
    gen = torch.Generator().manual_seed(1)
    theirs = {k: torch.randn(shape, generator=gen) for k, shape in zip(names, shapes)}       # a hand-built mmcv-named checkpoint
    mod.load_state_dict(theirs, strict=True)
    assert all(torch.equal(mod.state_dict()[k], theirs[k]) for k in names)
    with pytest.raises(ValueError, match="embed_dims must be divisible by num_heads, got 10 and 3"):
        ops.MultiScaleDeformableAttention(embed_dims=10, num_heads=3)
    assert "num_levels=4" in repr(mod)


def test_module_init_is_mmcvs():
    torch.manual_seed(0)
    mod = ops.MultiScaleDeformableAttention(embed_dims=64, num_heads=8, num_levels=3, num_points=4)
    assert not bool(mod.sampling_offsets.weight.any()) and not bool(mod.attention_weights.weight.any())
    assert not bool(mod.attention_weights.bias.any()) and not bool(mod.value_proj.bias.any()) and not bool(mod.output_proj.bias.any())
    bias = mod.sampling_offsets.bias.detach().view(8, 3, 4, 2)
    for head in range(8):
        t = head * 2 * math.pi / 8
        unit = torch.tensor([math.cos(t), math.sin(t)]) / max(abs(math.cos(t)), abs(math.sin(t)))     # the direction, largest entry 1
        for point in range(4):
            assert torch.allclose(bias[head, :, point], (unit * (point + 1)).expand(3, 2), atol=1e-6)
    assert bias[0, 0, 0].tolist() == [1.0, 0.0] and bias[0, 2, 3].tolist() == [4.0, 0.0]
    bound = (6.0 / (64 + 64)) ** 0.5                                       # Xavier-uniform
    for proj in (mod.value_proj, mod.output_proj):
        w = proj.weight.detach()
        assert 0.98 * bound < float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) < 0.03 * bound


@pytest.mark.parametrize("ref_dim, batch_first", [(2, False), (4, True)])
def test_module_cpu_forward_is_the_restatement(ref_dim, batch_first):
    torch.manual_seed(2)
    shapes = [(3, 4), (2, 3)]
    spatial, starts = K.levels_of(shapes)
    mod = ops.MultiScaleDeformableAttention(embed_dims=12, num_heads=3, num_levels=2, num_points=2, dropout=0.0,
                                            batch_first=batch_first).double()
    torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.3)
    torch.nn.init.normal_(mod.attention_weights.weight, std=0.3)
    bs, nq, nv_ = 2, 5, 18
    query, value, pos = torch.randn(bs, nq, 12, dtype=F64), torch.randn(bs, nv_, 12, dtype=F64), torch.randn(bs, nq, 12, dtype=F64)
    mask = torch.zeros(bs, nv_, dtype=torch.bool)
    mask[1, -4:] = True
    ref = torch.rand(bs, nq, 2, ref_dim, dtype=F64) * 0.8 + 0.1
    lay = (lambda t: t) if batch_first else (lambda t: t.transpose(0, 1))  # noqa: E731
    out = mod(lay(query), value=lay(value), query_pos=lay(pos), key_padding_mask=mask, reference_points=ref, spatial_shapes=spatial,
              level_start_index=starts)
    assert out.shape == lay(query).shape
    # the same by hand on the explicit restatement
    qp = query + pos
    v = mod.value_proj(value).masked_fill(mask[..., None], 0.0).view(bs, nv_, 3, 4)
    off = mod.sampling_offsets(qp).view(bs, nq, 3, 2, 2, 2)
    w = mod.attention_weights(qp).view(bs, nq, 3, 4).softmax(-1).view(bs, nq, 3, 2, 2)
    if ref_dim == 2:
        norm = torch.tensor([[w_, h_] for h_, w_ in shapes], dtype=F64)
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + off / 2 * ref[:, :, None, :, None, 2:] * 0.5
    want = mod.output_proj(K.msda_explicit(v, shapes, starts.tolist(), loc, w)[0]) + query
    assert float((lay(want) - out).detach().abs().max()) < 1e-12
    with pytest.raises(ValueError, match="reference_points must hold 2 or 4 entries, got 3"):
        mod(lay(query), value=lay(value), reference_points=torch.rand(bs, nq, 2, 3, dtype=F64), spatial_shapes=spatial,
            level_start_index=starts)
