"""fasterrcnn_amd.ops.heatmaps_to_keypoints and friends without a GPU: the float32 mirror of tests/keypoint_cases.py against its float64
truth, the _pytorch twin against the same truth and its defined cases, keypoints_to_heatmap against a literal per-element loop,
keypointrcnn_inference's split, the fake (on meta tensors), the C entry point's argument validation, every Python-side message, and that
the cases hold what they claim (the share of near-tied pairs among them)."""
import re

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import keypoint_cases as C

F32, F64 = torch.float32, torch.float64
META = "meta"
NAN, INF = C.NAN, C.INF


def raises(kind, message, call):
    with pytest.raises(kind, match="^" + re.escape(message) + "$"):
        call()


def meta(shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device=META)


# ---- the library and the constants ------------------------------------------------------------------------------------------------------
def test_constants_mirror_the_library():
    lib = nv.lib()
    assert ops.MAX_KEYPOINT_MAP_SIDE == lib.frcnn_ops_keypoint_max_map_side() >= 112
    assert ops.MAX_KEYPOINT_ROI_SIDE == lib.frcnn_ops_keypoint_max_roi_side() >= 1344          # an 800 x 1333 image fits
    assert ops.KEYPOINT_BLOCK_THREADS == lib.frcnn_ops_keypoint_block_threads() and ops.KEYPOINT_BLOCK_THREADS % 64 == 0
    assert {"heatmaps_to_keypoints", "heatmaps_to_keypoints_scored", "keypointrcnn_inference", "keypoints_to_heatmap",
            "heatmaps_to_keypoints_pytorch", "heatmaps_to_keypoints_scored_pytorch"} <= set(ops.__all__)


def test_library_validates_before_touching_the_gpu():
    f = nv.lib().frcnn_ops_heatmaps_to_keypoints
    side = ops.MAX_KEYPOINT_MAP_SIDE
    assert f(nv.OPS_F32, None, None, 0, 3, 7, 7, None, None) == 0              # R = 0: nothing to do
    assert f(nv.OPS_F16, None, None, 5, 0, 7, 7, None, None) == 0              # K = 0: nothing to do
    assert f(nv.OPS_F32, None, None, 2, 3, 7, 7, None, None) == -1             # NULL pointers
    assert f(7, None, None, 0, 3, 7, 7, None, None) == -1                      # unknown element type
    assert f(nv.OPS_BF16, None, None, -1, 3, 7, 7, None, None) == -1
    assert f(nv.OPS_BF16, None, None, 2, -3, 7, 7, None, None) == -1
    assert f(nv.OPS_F32, None, None, 0, 3, 0, 7, None, None) == -1
    assert f(nv.OPS_F32, None, None, 0, 3, 7, 0, None, None) == -1
    assert f(nv.OPS_F32, None, None, 0, 3, side + 1, 7, None, None) == -1
    assert f(nv.OPS_F32, None, None, 0, 3, 7, side + 1, None, None) == -1
    assert f(nv.OPS_F32, None, None, 0, 3, side, side, None, None) == 0
    assert f(nv.OPS_F32, None, None, 65536, 32768, 7, 7, None, None) == -1     # R K past 2^31 - 1


# ---- the fake -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F32,) + C.HALF)
def test_fake_shapes_and_dtypes(dtype):
    out = ops.heatmaps_to_keypoints_scored(meta((5, 17, 56, 56), dtype), meta((5, 4)))
    assert out.shape == (5, 17, 4) and out.dtype == F32 and out.device.type == META
    xy, scores = ops.heatmaps_to_keypoints(meta((5, 17, 7, 9), dtype), meta((5, 4), torch.float16))
    assert xy.shape == (5, 17, 3) and scores.shape == (5, 17) and xy.dtype == scores.dtype == F32
    assert ops.heatmaps_to_keypoints_scored(meta((0, 17, 7, 7), dtype), meta((0, 4))).shape == (0, 17, 4)
    assert ops.heatmaps_to_keypoints_scored(meta((5, 0, 7, 7), dtype), meta((5, 4))).shape == (5, 0, 4)
    xys, scs = ops.keypointrcnn_inference(meta((5, 17, 7, 7), dtype), [meta((2, 4)), meta((0, 4)), meta((3, 4))])
    assert [tuple(t.shape) for t in xys] == [(2, 17, 3), (0, 17, 3), (3, 17, 3)]
    assert [tuple(t.shape) for t in scs] == [(2, 17), (0, 17), (3, 17)]


def test_no_autograd():
    """A map or box tensor that requires grad is accepted and the result does not."""
    assert not ops.heatmaps_to_keypoints_scored(meta((2, 3, 7, 7)).requires_grad_(), meta((2, 4)).requires_grad_()).requires_grad
    maps, rois = torch.randn(2, 3, 7, 7, requires_grad=True), torch.tensor([[1.0, 1, 6, 7], [0, 2, 5, 5]], requires_grad=True)
    assert not ops.heatmaps_to_keypoints_scored_pytorch(maps, rois).requires_grad
    assert not ops.heatmaps_to_keypoints(maps, rois)[0].requires_grad


# ---- every error message ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", (ops.heatmaps_to_keypoints, ops.heatmaps_to_keypoints_scored, ops.heatmaps_to_keypoints_pytorch,
                               ops.heatmaps_to_keypoints_scored_pytorch), ids=lambda f: f.__name__)
def test_heatmaps_to_keypoints_errors(f):
    good, b = meta((3, 17, 7, 7)), meta((3, 4))
    raises(TypeError, "maps must be a torch.Tensor, got ndarray", lambda: f(np.zeros((3, 17, 7, 7), np.float32), b))
    raises(TypeError, "rois must be a torch.Tensor, got list", lambda: f(good, [[0, 0, 1, 1]] * 3))
    raises(TypeError, "maps must be float32, float16 or bfloat16 (or float64: the _pytorch twin), got torch.int32",
           lambda: f(meta((3, 17, 7, 7), torch.int32), b))
    raises(TypeError, "rois must be a float dtype, got torch.int64", lambda: f(good, meta((3, 4), torch.int64)))
    raises(ValueError, "maps and rois must be on the same device, got meta and cpu", lambda: f(good, torch.zeros(3, 4)))
    raises(ValueError, "maps must be [R, K, Mh, Mw], got shape (3, 7, 7)", lambda: f(meta((3, 7, 7)), b))
    raises(ValueError, "rois must be [R, 4], got shape (3, 5)", lambda: f(good, meta((3, 5))))
    raises(ValueError, "rois must be [R, 4], got shape (12,)", lambda: f(good, meta((12,))))
    raises(ValueError, "maps and rois must have the same R, got 3 maps and 2 rois", lambda: f(good, meta((2, 4))))
    side = ops.MAX_KEYPOINT_MAP_SIDE
    raises(ValueError, "maps must be Mh x Mw with 1 <= Mh, Mw <= MAX_KEYPOINT_MAP_SIDE = %d, got 7 x %d" % (side, side + 1),
           lambda: f(meta((3, 17, 7, side + 1)), b))
    raises(ValueError, "maps must be Mh x Mw with 1 <= Mh, Mw <= MAX_KEYPOINT_MAP_SIDE = %d, got 0 x 7" % side, lambda: f(meta((3, 17, 0, 7)), b))


def test_other_errors():
    raises(TypeError, "boxes must be a list of Tensor[R_i, 4], one per image, got Tensor",
           lambda: ops.keypointrcnn_inference(meta((3, 17, 7, 7)), meta((3, 4))))
    raises(ValueError, "maps and rois must have the same R, got 3 maps and 4 rois",
           lambda: ops.keypointrcnn_inference(meta((3, 17, 7, 7)), [meta((2, 4)), meta((2, 4))]))
    k, r = torch.zeros(3, 17, 3), torch.zeros(3, 4)
    raises(TypeError, "keypoints must be a torch.Tensor, got list", lambda: ops.keypoints_to_heatmap([], r, 56))
    raises(ValueError, "keypoints must be [R, K, 3], got shape (3, 17, 2)", lambda: ops.keypoints_to_heatmap(torch.zeros(3, 17, 2), r, 56))
    raises(ValueError, "rois must be [R, 4] with the keypoints' R = 3, got shape (2, 4)", lambda: ops.keypoints_to_heatmap(k, torch.zeros(2, 4), 56))
    raises(ValueError, "heatmap_size must be a positive int, got 0", lambda: ops.keypoints_to_heatmap(k, r, 0))
    raises(ValueError, "heatmap_size must be a positive int, got 56.0", lambda: ops.keypoints_to_heatmap(k, r, 56.0))


# ---- the cases hold what they claim -------------------------------------------------------------------------------------------------------
def test_cases_hold_what_they_claim():
    """The near-tied share of the truth alone: 6 of 150 pairs (the two RoIs of "side": 7 pixels stretched over 4096)."""
    tied = total = 0
    for name, ((mh, mw), boxes) in C.CASES.items():
        assert len(boxes) <= 12 and max(mh, mw) <= C.MAX_MAP
        for row in C.truth(name):
            for p in row:
                assert p.image is not None and p.image.size <= 300 * 411 and np.isfinite(p.image).all()
                total += 1
                tied += p.bound > 0 and not p.gap > 2 * p.bound
                assert p.bound == 0 or 0 < p.bound < 2e-3                      # maps of magnitude ~10: a few 1e-4
    print("near-tied pairs of the truth: %d of %d" % (tied, total))
    assert total >= 100 and tied <= C.LEFT_OUT_SHARE * total
    sz = {name: [C.sizes(np.float32(b))[2:] for b in boxes] for name, (_, boxes) in C.CASES.items()}
    assert sz["m7"][:10] == [(1, 1), (20, 1), (1, 20), (13, 5), (13, 6), (14, 5), (1, 1), (1, 9), (9, 1), (3, 4)]
    assert sz["seams"][:3] == [(63, 3), (64, 4), (65, 5)] and sz["side"] == [(4096, 2), (3, 4096)]
    assert sz["m56"] == [(20, 20), (57, 200), (300, 411), (134, 81)]
    assert all(C.sizes(np.float32(b)) is None for b in C.refused_rois()[:-1].numpy()) and C.sizes(C.refused_rois()[-1].numpy()) is not None
    assert all(p.constant for row in C.truth("m1") for p in row) and not any(p.constant for row in C.truth("m2") for p in row)


def test_truth_is_torch_s_bicubic():
    """The float64 formula against F.interpolate(bicubic) in float64 on the same map: the same function."""
    maps, _ = C.case("m7")
    for (h, w) in ((13, 5), (3, 4), (1, 1), (40, 33)):
        want = torch.nn.functional.interpolate(maps[0].double()[:, None], size=(h, w), mode="bicubic", align_corners=False)[:, 0]
        for j in range(C.K):
            iy, cy = C.taps64(7, h)
            ix, cx = C.taps64(7, w)
            got = C.resize64(maps[0, j].double().numpy(), iy, cy, ix, cx)
            assert float(np.abs(got - want[j].numpy()).max()) <= 1e-12


# ---- the mirror and the twin against the truth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASES)
def test_mirror_against_the_truth(name):
    maps, rois = C.case(name)
    worst, worst_prob, left_out, total = C.judge(C.mirror(maps, rois), maps, rois, C.truth(name))
    print("%s: largest error / bound %.4f, prob %.4f, left out %d of %d" % (name, worst, worst_prob, left_out, total))
    assert worst <= 1 and worst_prob <= 1


@pytest.mark.parametrize("name", C.CASES)
def test_twin_against_the_truth(name):
    maps, rois = C.case(name)
    got = ops.heatmaps_to_keypoints_scored_pytorch(maps, rois)
    assert got.shape == (len(rois), C.K, 4) and got.dtype == F32
    worst, worst_prob, left_out, total = C.judge(got, maps, rois, C.truth(name))
    print("%s: largest error / bound %.4f, prob %.4f, left out %d of %d" % (name, worst, worst_prob, left_out, total))
    assert worst <= 1 and worst_prob <= 1
    # CPU tensors are served by the twin, in either shape
    assert torch.equal(ops.heatmaps_to_keypoints_scored(maps, rois), got)
    xy, scores = ops.heatmaps_to_keypoints(maps, rois)
    assert torch.equal(xy[..., :2], got[..., :2]) and bool((xy[..., 2] == 1).all()) and torch.equal(scores, got[..., 2])


def test_twin_float64_and_16_bit():
    maps, rois = C.case("m7")
    got = ops.heatmaps_to_keypoints_scored(maps.double(), rois.double())
    assert got.dtype == F64
    for i, row in enumerate(C.truth("m7")):
        for j, p in enumerate(row):
            assert C.position_of(got[i, j, :2].numpy(), rois[i].numpy(), p.sizes) == p.pos
            assert abs(float(got[i, j, 2]) - p.value) <= 1e-12 and abs(float(got[i, j, 3]) - p.prob) <= 1e-12 * p.prob
    for dtype in C.HALF:
        m16, _ = C.case("m7", dtype)
        assert torch.equal(ops.heatmaps_to_keypoints_scored_pytorch(m16, rois), ops.heatmaps_to_keypoints_scored_pytorch(m16.float(), rois))
        assert torch.equal(ops.heatmaps_to_keypoints_scored_pytorch(maps, rois.to(dtype)),
                           ops.heatmaps_to_keypoints_scored_pytorch(maps, rois.to(dtype).float()))


def test_twin_defined_cases():
    C.check_defined_cases(ops.heatmaps_to_keypoints_scored_pytorch, "cpu", False)


def test_twin_non_contiguous_inputs():
    maps, rois = C.case("rect")
    want = ops.heatmaps_to_keypoints_scored_pytorch(maps, rois)
    m = maps.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    b = torch.stack([rois, rois], 2)[:, :, 0]
    assert not m.is_contiguous() and not b.is_contiguous()
    assert torch.equal(ops.heatmaps_to_keypoints_scored_pytorch(m, b), want)


# ---- keypointrcnn_inference ----------------------------------------------------------------------------------------------------------------
def test_keypointrcnn_inference_splits_per_image():
    maps, rois = C.case("m7")
    xy, scores = ops.heatmaps_to_keypoints(maps, rois)
    counts = [5, 0, 4, 3]
    xys, scs = ops.keypointrcnn_inference(maps, list(rois.split(counts)))
    assert [len(t) for t in xys] == counts and [len(t) for t in scs] == counts
    assert torch.equal(torch.cat(xys), xy) and torch.equal(torch.cat(scs), scores)
    assert ops.keypointrcnn_inference(maps[:0], []) == ([], [])


# ---- keypoints_to_heatmap -------------------------------------------------------------------------------------------------------------------
def heatmap_loop(keypoints, rois, size):
    """torchvision's keypoints_to_heatmap, one element at a time, in float32."""
    f = np.float32
    kp, rs = keypoints.numpy(), rois.numpy()
    heat, valid = np.zeros(kp.shape[:2], np.int64), np.zeros(kp.shape[:2], np.int64)
    for i in range(kp.shape[0]):
        x1, y1, x2, y2 = rs[i]
        with np.errstate(all="ignore"):
            sx, sy = f(size) / f(x2 - x1), f(size) / f(y2 - y1)
        for j in range(kp.shape[1]):
            x, y, v = kp[i, j]
            xi = size - 1 if x == x2 else int(np.floor(f(f(x - x1) * sx)))
            yi = size - 1 if y == y2 else int(np.floor(f(f(y - y1) * sy)))
            ok = xi >= 0 and yi >= 0 and xi < size and yi < size and v > 0
            valid[i, j] = int(ok)
            heat[i, j] = (yi * size + xi) * int(ok)
    return torch.from_numpy(heat), torch.from_numpy(valid)


@pytest.mark.parametrize("size", (56, 7, 1))
def test_keypoints_to_heatmap_against_the_loop(size):
    g = torch.Generator().manual_seed(11)
    rois = torch.tensor([[10.0, 20, 110, 220], [0, 0, 33.5, 17.25], [-5.5, -7, 40, 3], [3, 3, 4, 4]])
    wh = (rois[:, 2:] - rois[:, :2])[:, None]
    kp = torch.cat([rois[:, None, :2] + wh * (torch.rand((4, 12, 2), generator=g) * 1.3 - 0.15), torch.randint(0, 3, (4, 12, 1), generator=g).float()], 2)
    kp[:, (0, 1, 5, 6), :2] = ((rois[:, :2] + rois[:, 2:]) * 0.5)[:, None]     # inside, before one coordinate is moved
    kp[:, 0, 0], kp[:, 0, 2] = rois[:, 2], 1                                   # exactly on the right edge
    kp[:, 1, 1], kp[:, 1, 2] = rois[:, 3], 2                                   # exactly on the bottom edge
    kp[:, 2, :2], kp[:, 2, 2] = rois[:, 2:], 1                                 # the corner
    kp[:, 3, :2], kp[:, 3, 2] = rois[:, 2:], 0                                 # the corner, invisible
    kp[:, 4, :2], kp[:, 4, 2] = rois[:, :2], 1                                 # the first cell
    kp[:, 5, 0], kp[:, 5, 2] = rois[:, 0] - 0.01, 1                            # outside, left
    kp[:, 6, 1], kp[:, 6, 2] = rois[:, 3] + 0.01, 1                            # outside, below
    heat, valid = ops.keypoints_to_heatmap(kp, rois, size)
    want_heat, want_valid = heatmap_loop(kp, rois, size)
    assert heat.dtype == valid.dtype == torch.int64 and heat.shape == valid.shape == (4, 12)
    assert torch.equal(valid, want_valid) and torch.equal(heat, want_heat)
    assert valid[:, :3].all() and not valid[:, 3].any() and valid[:, 4].all() and not valid[:, 5:7].any()
    assert bool((heat[:, 2] == size * size - 1).all()) and bool((heat[:, 4] == 0).all()) and bool((heat[:, 0] % size == size - 1).all())
    assert 0 < int(valid[:, 7:].sum()) < valid[:, 7:].numel()
    h2, v2 = ops.keypoints_to_heatmap(meta((4, 12, 3)), meta((4, 4)), size)
    assert h2.shape == v2.shape == (4, 12) and h2.dtype == torch.int64
