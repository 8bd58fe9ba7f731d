"""fasterrcnn_amd.ops.heatmaps_to_keypoints on the GPU against tests/keypoint_cases.py: the float32 mirror bit for bit (x, y, logit), the
float64 truth under the derived per-pair bound (optimality, logit, position where the truth's top-two gap exceeds twice the bound, prob),
the _pytorch twin on the GPU under the same rules, the 16-bit identities, the defined cases and two runs bit for bit.

Every test prints the figure it asserts on.  Measured on an MI355X: no x, y or logit differs from the mirror in a bit; the largest
error is 0.091 of the derived bound ("m7"; 0.031 on "m56", 0.019 on "m_max") and 0.087 of prob's tolerance; the twin's is 0.038; 6 of
150 pairs are left out of the position comparison (the two RoIs of "side": 7 source pixels stretched over 4096), and no position
differs outside them; the 16-bit identities and the run-to-run comparisons hold without a differing element.  The kernel has one
path: one block per (RoI, keypoint) whatever the RoI's size (no multi-block form), so the seams are a wave's step of 64 pixels, a pass
of 4 rows, and the stated caps."""
import functools

import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import keypoint_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
half = pytest.mark.parametrize("dtype", C.HALF, ids=("f16", "bf16"))


@functools.lru_cache(maxsize=None)
def on_gpu(name, dtype=F32):
    maps, rois = C.case(name, dtype)
    return maps.to(DEV), rois.to(DEV)


@functools.lru_cache(maxsize=None)
def result(name):
    return ops.heatmaps_to_keypoints_scored(*on_gpu(name)).cpu()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", C.CASES)
def test_x_y_and_logit_are_the_mirror_s_bit_for_bit(name):
    maps, rois = C.case(name)
    got, want = result(name), C.mirror(maps, rois)
    assert got.shape == (len(rois), C.K, 4) and got.dtype == F32
    differing = int((got[..., :3].view(torch.int32) != want[..., :3].contiguous().view(torch.int32)).sum())
    print("%s: differing x / y / logit elements %d of %d" % (name, differing, got[..., :3].numel()))
    assert differing == 0


@pytest.mark.parametrize("name", C.CASES)
def test_against_the_truth(name):
    maps, rois = C.case(name)
    worst, worst_prob, left_out, total = C.judge(result(name), maps, rois, C.truth(name))
    print("%s: largest error / bound %.4f, largest prob error / tolerance %.4f, left out %d of %d" % (name, worst, worst_prob, left_out, total))
    assert worst <= 1 and worst_prob <= 1


def test_left_out_share():
    left_out = total = 0
    for name in C.CASES:
        _, _, n, t = C.judge(result(name), *C.case(name), C.truth(name))
        left_out, total = left_out + n, total + t
    print("left out of the position comparison: %d of %d pairs" % (left_out, total))
    assert left_out <= C.LEFT_OUT_SHARE * total


@pytest.mark.parametrize("name", C.CASES)
def test_twin_on_the_gpu_under_the_same_rules(name):
    maps, rois = C.case(name)
    got = ops.heatmaps_to_keypoints_scored_pytorch(*on_gpu(name))
    assert got.device.type == DEV and got.dtype == F32
    worst, worst_prob, left_out, total = C.judge(got.cpu(), maps, rois, C.truth(name))
    print("%s (twin): largest error / bound %.4f, prob %.4f, left out %d of %d" % (name, worst, worst_prob, left_out, total))
    assert worst <= 1 and worst_prob <= 1


@half
@pytest.mark.parametrize("name", ("m7", "seams", "m56", "m_max"))
def test_16_bit_maps_are_the_widened_map_s_result_bit_for_bit(name, dtype):
    maps, rois = on_gpu(name, dtype)
    got, want = ops.heatmaps_to_keypoints_scored(maps, rois), ops.heatmaps_to_keypoints_scored(maps.float(), rois)
    print("%s %s: differing elements %d" % (name, dtype, int((got.view(torch.int32) != want.view(torch.int32)).sum())))
    assert same_bits(got, want)
    worst, worst_prob, _, _ = C.judge(got.cpu(), *C.case(name, dtype), C.truth(name, dtype))
    assert worst <= 1 and worst_prob <= 1


@pytest.mark.parametrize("name", ("m7", "m56", "side"))
def test_two_runs_agree_bit_for_bit(name):
    maps, rois = on_gpu(name)
    assert same_bits(ops.heatmaps_to_keypoints_scored(maps, rois).cpu(), result(name))
    assert same_bits(ops.heatmaps_to_keypoints_scored(maps.clone(), rois.clone()).cpu(), result(name))


def test_defined_cases():
    C.check_defined_cases(ops.heatmaps_to_keypoints_scored, DEV, True)


def test_twin_defined_cases_on_the_gpu():
    C.check_defined_cases(ops.heatmaps_to_keypoints_scored_pytorch, DEV, False)


def test_non_contiguous_inputs_and_other_box_dtypes():
    maps, rois = on_gpu("rect")
    want = result("rect")
    m = maps.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    b = torch.stack([rois, rois], 2)[:, :, 0]
    assert not m.is_contiguous() and not b.is_contiguous()
    assert same_bits(ops.heatmaps_to_keypoints_scored(m, b).cpu(), want)
    assert same_bits(ops.heatmaps_to_keypoints_scored(maps[:, :, ::2, 1:], rois).cpu(),
                     ops.heatmaps_to_keypoints_scored(maps[:, :, ::2, 1:].contiguous(), rois).cpu())
    assert same_bits(ops.heatmaps_to_keypoints_scored(maps, rois.double()).cpu(), want)       # the boxes are float32-valued
    b16 = rois.to(torch.bfloat16)
    assert same_bits(ops.heatmaps_to_keypoints_scored(maps, b16), ops.heatmaps_to_keypoints_scored(maps, b16.float()))
    assert not ops.heatmaps_to_keypoints_scored(maps.clone().requires_grad_(), rois.clone().requires_grad_()).requires_grad
    got64 = ops.heatmaps_to_keypoints_scored(maps.double(), rois)                              # float64 maps: the twin, in float64
    assert got64.dtype == torch.float64 and got64.device.type == DEV


def test_torchvision_s_return_and_the_per_image_split():
    maps, rois = on_gpu("m7")
    want = result("m7")
    xy, scores = ops.heatmaps_to_keypoints(maps, rois)
    assert xy.shape == (len(rois), C.K, 3) and scores.shape == (len(rois), C.K)
    assert same_bits(xy[..., :2].cpu(), want[..., :2]) and bool((xy[..., 2] == 1).all()) and same_bits(scores.cpu(), want[..., 2])
    counts = [5, 0, 4, 3]
    xys, scs = ops.keypointrcnn_inference(maps, list(rois.split(counts)))
    assert [len(t) for t in xys] == counts and [len(t) for t in scs] == counts
    assert same_bits(torch.cat(xys), xy) and same_bits(torch.cat(scs), scores)


def test_library_rejects_on_the_gpu_too():
    maps, rois = on_gpu("m7")
    out = torch.empty((len(rois), C.K, 4), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    f = nv.lib().frcnn_ops_heatmaps_to_keypoints
    assert f(3, maps.data_ptr(), rois.data_ptr(), len(rois), C.K, 7, 7, out.data_ptr(), s) == -1
    assert f(nv.OPS_F32, maps.data_ptr(), rois.data_ptr(), len(rois), C.K, 7, ops.MAX_KEYPOINT_MAP_SIDE + 1, out.data_ptr(), s) == -1
    assert f(nv.OPS_F32, maps.data_ptr(), None, len(rois), C.K, 7, 7, out.data_ptr(), s) == -1
    assert f(nv.OPS_F32, maps.data_ptr(), rois.data_ptr(), len(rois), C.K, 7, 7, out.data_ptr(), s) == 0
    assert same_bits(out.cpu(), result("m7"))
