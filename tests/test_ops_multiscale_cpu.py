"""fasterrcnn_amd.ops.multi_scale_roi_align / MultiScaleRoIAlign without a GPU: shapes and strides from meta / fake tensors, the
argument errors, and the host side of torchvision's MultiScaleRoIAlign (ops/poolers.py) -- featmap_names filtering, the scale and
k_min / k_max inference, first-call caching -- against a restatement of it written here."""
from collections import OrderedDict

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

CL = torch.channels_last


def cl_strides(k, c, oh, ow):
    return torch.empty((k, c, oh, ow), device="meta", memory_format=CL).stride()


def pyramid(device, n=2, c=6, h=64, w=96, levels=4, channels_last=False, requires_grad=False):
    feats = []
    for i in range(levels):
        f = torch.empty((n, c, max(h >> i, 1), max(w >> i, 1)), device=device)
        if channels_last:
            f = f.contiguous(memory_format=CL)
        feats.append(f.requires_grad_(requires_grad))
    return feats


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("output_size", [7, (7, 3), (64, 64)])
@pytest.mark.parametrize("as_list", [False, True])
def test_meta_shapes(levels, output_size, as_list):
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    feats = pyramid("meta", levels=levels)
    boxes = [torch.empty((3, 4), device="meta"), torch.empty((4, 4), device="meta")] if as_list else torch.empty((7, 5), device="meta")
    y = ops.multi_scale_roi_align(feats, boxes, output_size, [2.0 ** -(i + 2) for i in range(levels)], 2)
    assert y.shape == (7, 6, oh, ow) and y.dtype == torch.float32 and y.stride() == cl_strides(7, 6, oh, ow)


@pytest.mark.parametrize("levels", [1, 3, 8])
@pytest.mark.parametrize("channels_last", [False, True])
def test_fake_and_meta_autograd(levels, channels_last):
    scales = [2.0 ** -(i + 2) for i in range(levels)]

    def run(device):
        feats = pyramid(device, n=3, c=5, levels=levels, channels_last=channels_last, requires_grad=True)
        y = ops.multi_scale_roi_align(feats, torch.empty((4, 5), device=device), (7, 3), scales, 2)
        assert y.shape == (4, 5, 7, 3) and y.device.type == device and y.stride() == cl_strides(4, 5, 7, 3) and y.requires_grad
        return feats, y
    with FakeTensorMode():
        run("cuda")
    feats, y = run("meta")
    y.sum().backward()
    for f in feats:
        assert f.grad.shape == f.shape and f.grad.stride() == f.stride()
    feats, y = run("meta")
    v = torch.empty(y.shape, device="meta", requires_grad=True)
    g = torch.autograd.grad(y, feats, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        sum(t.sum() for t in g).backward()


def test_mixed_layouts_keep_each_levels_gradient_format():
    feats = pyramid("meta", levels=3, requires_grad=True)
    feats[1] = torch.empty(feats[1].shape, device="meta").contiguous(memory_format=CL).requires_grad_(True)
    ops.multi_scale_roi_align(feats, torch.empty((2, 5), device="meta"), 7, [0.25, 0.125, 0.0625]).sum().backward()
    assert [f.grad.is_contiguous(memory_format=CL) and not f.grad.is_contiguous() for f in feats] == [False, True, False]


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    b = torch.empty((3, 5), device="meta")
    feats = pyramid("meta", levels=2)
    s2 = [0.25, 0.125]
    with pytest.raises(ValueError, match="same N and C"):
        ops.multi_scale_roi_align([feats[0], torch.empty((3, 6, 32, 48), device="meta")], b, 7, s2)
    with pytest.raises(ValueError, match="same N and C"):
        ops.multi_scale_roi_align([feats[0], torch.empty((2, 5, 32, 48), device="meta")], b, 7, s2)
    with pytest.raises(TypeError, match="float32"):
        ops.multi_scale_roi_align([feats[0], feats[1].double()], b, 7, s2)
    with pytest.raises(ValueError, match="GPU"):
        ops.multi_scale_roi_align([feats[0], torch.empty((2, 6, 32, 48))], b, 7, s2)
    with FakeTensorMode():
        with pytest.raises(ValueError, match="same device"):
            ops.multi_scale_roi_align([torch.empty((2, 6, 8, 8), device="cuda"), torch.empty((2, 6, 4, 4), device="meta")],
                                      torch.empty((3, 5), device="cuda"), 7, s2)
    with pytest.raises(ValueError, match="1 to 8"):
        ops.multi_scale_roi_align(pyramid("meta", levels=9), b, 7, [2.0 ** -i for i in range(9)])
    with pytest.raises(ValueError, match="1 to 8"):
        ops.multi_scale_roi_align([], b, 7, [])
    with pytest.raises(TypeError, match="list"):
        ops.multi_scale_roi_align(feats[0], b, 7, [0.25])
    with pytest.raises(ValueError, match="one scale per feature map"):
        ops.multi_scale_roi_align(feats, b, 7, [0.25])
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        ops.multi_scale_roi_align([torch.empty((6, 8, 8), device="meta")], b, 7, [0.25])
    with pytest.raises(ValueError, match="output_size"):
        ops.multi_scale_roi_align(feats, b, 65, s2)
    with pytest.raises(ValueError, match="output_size"):
        ops.multi_scale_roi_align(feats, b, (7, 0), s2)
    with pytest.raises(ValueError, match="sampling_ratio"):
        ops.multi_scale_roi_align(feats, b, 7, s2, 17)
    with pytest.raises(ValueError, match=r"Tensor\[K, 5\]"):
        ops.multi_scale_roi_align(feats, torch.empty((3, 4), device="meta"), 7, s2)
    with pytest.raises(ValueError, match="image_shapes"):
        ops.MultiScaleRoIAlign(["0", "1"], 7, 2)(OrderedDict(zip("01", feats)), [torch.empty((2, 4), device="meta")], [])
    with pytest.raises(ValueError, match="featmap_names"):
        ops.MultiScaleRoIAlign(["a"], 7, 2)(OrderedDict(zip("01", feats)), [torch.empty((2, 4), device="meta")], [(64, 96)])


def test_entry_points_reject_bad_arguments():
    import ctypes as C
    lib = nv.lib()
    EINVAL = -1

    def levels(hs, ws, ss):
        n = len(hs)
        return (C.c_int * n)(*hs), (C.c_int * n)(*ws), (C.c_float * n)(*ss)
    h, w, s = levels([8, 4], [8, 4], [0.25, 0.125])
    none2 = (C.c_void_p * 2)(None, None)
    fwd = lib.frcnn_ops_ms_roi_align
    assert fwd(none2, h, w, s, 2, 1, 4, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == 0              # k == 0: nothing to do
    assert fwd(none2, h, w, s, 0, 1, 4, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL         # no level
    assert fwd(none2, h, w, s, 9, 1, 4, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL         # 9 levels
    assert fwd(none2, h, w, s, 2, 1, 6, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL         # c % 4
    assert fwd(none2, h, w, s, 2, 0, 4, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL         # no image
    assert fwd(none2, h, w, s, 2, 1, 4, None, 0, 65, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL        # output 65
    assert fwd(none2, h, w, s, 2, 1, 4, None, 0, 7, 7, 17, 224.0, 4.0, 2, 3, None, None) == EINVAL        # sampling ratio 17
    assert fwd(none2, None, w, s, 2, 1, 4, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL      # no level sizes
    hn, wn, sn = levels([8, -1], [8, 4], [0.25, 0.125])
    assert fwd(none2, hn, wn, sn, 2, 1, 4, None, 0, 7, 7, 2, 224.0, 4.0, 2, 3, None, None) == EINVAL      # negative height
    assert fwd(none2, h, w, s, 2, 1, 4, 8, 1, 7, 7, 2, 224.0, 4.0, 2, 3, 8, None) == EINVAL               # null map, k > 0
    assert lib.frcnn_ops_ms_roi_align_workspace_bytes(10, 4, 2) == (10 + 2 * 4 * 2) * 4
    assert lib.frcnn_ops_ms_roi_align_workspace_bytes(0, 1, 1) == 8
    assert lib.frcnn_ops_ms_roi_align_workspace_bytes(10, 9, 2) == 0
    assert lib.frcnn_ops_ms_roi_align_workspace_bytes(-1, 4, 2) == 0
    bwd = lib.frcnn_ops_ms_roi_align_backward
    d2 = (C.c_void_p * 2)(8, 8)
    assert bwd(None, 0, h, w, s, 2, 1, 4, 7, 7, 2, 224.0, 4.0, 2, 3, None, d2, None, 0, None) == EINVAL       # no workspace
    assert bwd(None, 0, h, w, s, 2, 1, 4, 7, 7, 2, 224.0, 4.0, 2, 3, None, d2, 8, 15, None) == EINVAL        # one byte short
    assert bwd(None, 0, h, w, s, 2, 1, 4, 7, 7, 2, 224.0, 4.0, 2, 3, None, none2, 8, 16, None) == EINVAL     # no gradient maps
    assert bwd(None, 5, h, w, s, 2, 1, 4, 7, 7, 2, 224.0, 4.0, 2, 3, None, d2, 8, 64, None) == EINVAL        # k > 0, no RoIs
    assert bwd(None, 0, h, w, s, 2, 1, 4, 7, 7, 17, 224.0, 4.0, 2, 3, None, d2, 8, 16, None) == EINVAL      # sampling ratio 17


# ---- torchvision's host side, restated ----------------------------------------------------------------------------------------------
def tv_setup_scales(features, image_shapes):
    """torchvision ops/poolers.py _setup_scales + _infer_scale, as written there."""
    if not image_shapes:
        raise ValueError("images list should not be empty")
    max_x = 0
    max_y = 0
    for shape in image_shapes:
        max_x = max(shape[0], max_x)
        max_y = max(shape[1], max_y)
    original_input_shape = (max_x, max_y)
    scales = []
    for feature in features:
        possible_scales = []
        for s1, s2 in zip(feature.shape[-2:], original_input_shape):
            approx_scale = float(s1) / float(s2)
            possible_scales.append(2 ** float(torch.tensor(approx_scale).log2().round()))
        scales.append(possible_scales[0])
    lvl_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
    lvl_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
    return scales, (int(lvl_min), int(lvl_max))


def meta_maps(shapes, n=2, c=4):
    return [torch.empty((n, c, h, w), device="meta") for h, w in shapes]


SCALE_CASES = [
    # torchvision's FPN on two 800 x 1216 images
    ([(200, 304), (100, 152), (50, 76), (25, 38)], [(800, 1216), (800, 1216)]),
    # several image shapes: the largest H and the largest W come from different images
    ([(200, 304), (100, 152), (50, 76), (25, 38)], [(800, 1000), (640, 1216), (797, 1100)]),
    # non-square images, H decides: a wide image whose W ratio would round differently
    ([(60, 500), (30, 250), (15, 125)], [(240, 333)]),
    # round half to even in log2: ratios 2 ** -2.5 and 2 ** -1.5 sit at the .5 points only approximately; 3 / 8 and 3 / 16 do not
    ([(3, 3), (6, 6), (12, 12)], [(8, 8)]),
    ([(181, 100), (362, 200), (91, 50)], [(1024, 512)]),
    # coarsest first: k_min > k_max
    ([(25, 38), (50, 76), (100, 152), (200, 304)], [(800, 1216)]),
    # one level
    ([(100, 152)], [(800, 1216)]),
    # maps that do not divide the image (ceil-mode strides)
    ([(201, 305), (101, 153), (51, 77), (26, 39), (13, 20)], [(801, 1217), (700, 1100)]),
]


@pytest.mark.parametrize("shapes,image_shapes", SCALE_CASES)
def test_scale_inference_matches_torchvision(shapes, image_shapes):
    feats = meta_maps(shapes)
    want_scales, want_range = tv_setup_scales(feats, image_shapes)
    assert ops._infer_scales(feats, image_shapes) == want_scales
    assert ops._level_range(want_scales) == want_range
    m = ops.MultiScaleRoIAlign([str(i) for i in range(len(feats))], 7, 2)
    x = OrderedDict((str(i), f) for i, f in enumerate(feats))
    y = m(x, [torch.empty((3, 4), device="meta")] * 2, image_shapes)
    assert y.shape == (6, 4, 7, 7)
    assert m.scales == want_scales and m._k_range == want_range


def test_round_half_even_and_float32_log2():
    # H / max_h = 0.5 ** 0.5 (log2 = -0.5 in float32: rounds to -0 -> scale 1) vs the neighbouring cases, and exact half points
    for h, max_h, want in [(1, 4, 0.25), (3, 4, 1.0), (1, 2, 0.5), (5, 16, 0.25), (3, 8, 0.5), (2, 1, 2.0), (6, 1, 8.0)]:
        got = ops._infer_scales(meta_maps([(h, 7)]), [(max_h, 9)])
        assert got == [2 ** float(torch.tensor(h / max_h).log2().round())] == [want], (h, max_h)
    assert float(torch.tensor(-2.5).round()) == -2.0 and float(torch.tensor(-1.5).round()) == -2.0


def test_featmap_names_filtering_in_dict_order():
    feats = meta_maps([(64, 96), (32, 48), (16, 24), (8, 12)])
    pool = torch.empty((2, 4, 4, 6), device="meta")
    x = OrderedDict([("3", feats[3]), ("pool", pool), ("0", feats[0]), ("1", feats[1]), ("2", feats[2])])
    m = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    m(x, [torch.empty((2, 4), device="meta")], [(256, 384)])
    assert m.scales == [1 / 32, 1 / 4, 1 / 8, 1 / 16]                  # x's own order, 'pool' ignored
    assert m._k_range == (5, 4)
    m = ops.MultiScaleRoIAlign(["1", "pool"], (5, 3), 2)
    y = m(x, torch.empty((3, 5), device="meta"), [(256, 384)])
    assert m.scales == [1 / 64, 1 / 8] and y.shape == (3, 4, 5, 3)


def test_scales_are_cached_on_the_first_call():
    feats = meta_maps([(200, 304), (100, 152), (50, 76), (25, 38)])
    x = OrderedDict((str(i), f) for i, f in enumerate(feats))
    m = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    boxes = [torch.empty((2, 4), device="meta")]
    m(x, boxes, [(800, 1216)])
    assert m.scales == [1 / 4, 1 / 8, 1 / 16, 1 / 32] and m._k_range == (2, 5)
    m(x, boxes, [(400, 608)])                                             # torchvision keeps the first call's scales
    assert m.scales == [1 / 4, 1 / 8, 1 / 16, 1 / 32] and m._k_range == (2, 5)
    m(x, boxes, [])                                                       # not inferred again: an empty list is not an error now
    fresh = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    fresh(x, boxes, [(400, 608)])
    assert fresh.scales == [1 / 2, 1 / 4, 1 / 8, 1 / 16] and fresh._k_range == (1, 4)


def test_module_defaults_and_repr():
    m = ops.MultiScaleRoIAlign(["feat1", "feat3"], 3, 2)
    assert m.output_size == (3, 3) and m.canonical_scale == 224 and m.canonical_level == 4 and m.scales is None
    assert "featmap_names=['feat1', 'feat3']" in repr(m)
    m = ops.MultiScaleRoIAlign(["0"], (7, 5), -1, canonical_scale=112, canonical_level=3)
    assert m.output_size == (7, 5) and m.canonical_scale == 112 and m.canonical_level == 3
    assert "multi_scale_roi_align" in ops.__all__ and "MultiScaleRoIAlign" in ops.__all__
