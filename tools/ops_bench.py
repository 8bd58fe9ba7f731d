"""
Times of fasterrcnn_amd.ops (torch custom ops over csrc/ops.hip) at the reference's shapes, beside the model's own kernels on the same
input, and at an FPN-like shape.  Device events around `--reps` calls after `--warmup` calls; median of 5 windows, in microseconds.

    python tools/ops_bench.py [--reps 50] [--warmup 10]

  * one image, C = 512, 37 x 62 (VGG-16's map of a 600 x 1000 image), 128 and 300 RoIs, 7 x 7:
      ops.roi_pool / ops.roi_align on an NCHW input (the layout conversion included) and on a channels_last input,
      frcnn_roi_pool / frcnn_roi_align (sampling_ratio 2) on the NHWC map, and the backward passes (ops via autograd, with the
      forward) beside frcnn_roi_pool_backward / frcnn_roi_align_backward;
  * FPN-like: 2 images, 256 x 200 x 336, 1000 RoIs, 7 x 7, sampling_ratio 2: roi_align forward, forward + backward;
  * nms on 12000 float32 boxes and 2000 float64 boxes (the sort included);
  * multi-scale: torchvision's FPN pooler (2 images, 256 x {200 x 304, 100 x 152, 50 x 76, 25 x 38}, 7 x 7, sampling_ratio 2), 512 and
    1000 RoIs per image with sizes log-uniform over 16 .. 800 px (every level gets RoIs): ops.multi_scale_roi_align beside torchvision's
    composition (LevelMapper, then torch.where + ops.roi_align + index_put per level), forward and forward + backward, the two timed in
    alternating windows of the same call.

  * half: float16 and bfloat16 maps on the FPN pooler shape above (ops.multi_scale_roi_align, 512 and 1000 RoIs per image) and on the
    VGG-16 map (1 x 512 x 37 x 62, 300 RoIs: ops.roi_align sampling_ratio 2 and ops.roi_pool), forward and forward + backward: the
    native 16-bit op, the float32 op on the same values, and the composition op(x.float()).to(T) -- the only way before the 16-bit
    kernels --, the three timed in alternating windows of the same process.

  * ps: R-FCN's position-sensitive pooling at its VOC shape (1 x 1029 x 38 x 63 = 7 * 7 * 21 score maps, 300 RoIs, 7 x 7, scale 1 / 16,
    sampling_ratio 2), float32 and bfloat16: ops.ps_roi_align beside the only composition there was before it -- ops.roi_align(aligned =
    True) of all 1029 channels, then the diagonal gather [k, (c * 7 + ph) * 7 + pw, ph, pw] --, forward and forward + backward, in
    alternating windows; and ops.ps_roi_pool alone.

  * deform: deformable convolution at a DCN stage (2 x 256 -> 256, 3 x 3, padding 1, 50 x 68 maps), 1 and 4 offset groups, with and
    without a mask, offsets N(0, 2 px): ops.deform_conv2d beside the same operator composed from torch operations on the GPU (the
    restatement of tests/deform_conv_cases.py: floor, index gathers and einsum), forward and forward + backward of all five gradients,
    in alternating windows.  The same shapes in float16 and bfloat16: the 16-bit operator (16-bit columns, the products on the
    16-bit matrix pipe) beside the float32 operator on the widened tensors, forward and forward + backward.

  * droi: deformable RoI pooling on a C4 map (2 x 256 x 50 x 68, 512 RoIs, 7 x 7, scale 1 / 16, sampling_ratio 2), with offsets N(0, 0.5)
    and without, float32 and bfloat16: ops.deform_roi_pool beside the same operator composed from torch operations on the GPU (the
    restatement of tests/deform_roi_cases.py: floor, index gathers and sums), forward and forward + backward, in alternating windows.

  * rot: rotated boxes.  ops.nms_rotated on 12000 boxes (threshold 0.5, the sort included) beside ops.nms on the same boxes at angle
    0, and ops.roi_align_rotated on a C4 map (2 x 256 x 50 x 68, 512 RoIs with uniform angles, 7 x 7, scale 1 / 16, sampling_ratio 2),
    float32 and bfloat16, forward and forward + backward, beside ops.roi_align on the RoIs' axis-aligned boxes.  Informational.

  * carafe: CARAFE upsampling in an FPN top-down path (2 x 256 x 100 x 168 -> 200 x 336, k = 5, G = 1, masks a softmax over the 25
    taps), float32 and float16: ops.carafe beside the torch composition (unfold, nearest upsample, multiply, sum over the taps, with
    autograd's backward), forward and forward + backward of both gradients, in alternating windows; and the forward's algorithmic
    bytes (features + masks + result, each once) per second as a share of the 8 TB/s HBM peak.

  * msda: multi-scale deformable attention in a Deformable-DETR encoder layer (B 2; levels 100 x 134, 50 x 67, 25 x 34, 13 x 17, so
    S = 17821; M 8, D 32, P 4; Q = S, every query's reference point its own cell's centre on every level, offsets N(0, 2 px), weights a
    softmax over the 16 samples), float32 and float16: ops.multi_scale_deformable_attn beside ops.multi_scale_deformable_attn_pytorch
    (one grid_sample per level, autograd's backward), forward and forward + backward of all three gradients, in alternating windows;
    and the forward's algorithmic bytes (value + locations + weights + result, each once) per second as a share of the HBM peak.

  * prroi: Precise RoI Pooling on a C4 map (2 x 256 x 50 x 68, 512 RoIs, 7 x 7, scale 1 / 16), float32 and bfloat16:
    ops.prroi_pool beside ops.prroi_pool_pytorch (the weight matrices and one einsum per image, autograd's backward), forward and
    forward + backward of both gradients (the map's and the boxes'), in alternating windows.  Informational: no speed bound is set.

  * dcnv3: DCNv3 in an InternImage-T stage at detection size (2 x 100 x 160 x 128, G 8, Gc 16, 3 x 3, pad 1, offsets N(0, 2 px), masks
    a softmax over the 9 points), float32 and bfloat16: ops.dcnv3 beside ops.dcnv3_core_pytorch (pad, one grid_sample, autograd's
    backward), forward and forward + backward of all three gradients, in alternating windows.  Informational: no speed bound is set.

  * dcnv4: DCNv4 at the same size (2 x 100 x 160 x 128, G 8, Gc 16, 3 x 3, pad 1, offsets N(0, 2 px), masks N(0, 1), one packed
    offset_mask tensor of 216 values a pixel), float32 and bfloat16: ops.dcnv4 beside ops.dcnv4_core_pytorch and beside ops.dcnv3 fed the
    unpacked tensors, with the two unpacking copies (and, backward, autograd's re-packing of the gradients) inside the timed region;
    forward and forward + backward of both gradients, in alternating windows.  Informational: no speed bound is set.

  * diffiou: the differentiable rotated IoU of 2^20 aligned pairs (boxes of 8 to 30 px against jittered copies of themselves, every
    pair overlapping): ops.diff_iou_rotated_2d beside ops.diff_iou_rotated_2d_pytorch (the clip from torch operations, autograd's
    backward), forward and forward + backward of both gradients, in alternating windows.  Informational: no speed bound is set.

  * softnms: Soft-NMS on clustered detections (about N / 12 clusters in a 600-px frame, sides 30-120 px, scores uniform in [0.02, 1);
    thr 0.3, sigma 0.5, min_score 0.05): 1000 and 4000 boxes in one problem, and 80 labels x 250 boxes, linear and gaussian:
    ops.soft_nms beside ops.soft_nms_pytorch on the same GPU tensors, and beside what users of mmcv's CPU-only soft_nms do today --
    ops.soft_nms_pytorch on CPU copies, with the two copies inside the timed region.  Wall-clock milliseconds per call, synchronised,
    medians of 5 (the fallbacks: of 3 single calls).  Informational: no speed bound is set.  Measured on an MI355X:
      1000 boxes, one problem, linear      kept   169   ops.soft_nms  0.534   soft_nms_pytorch on the GPU    57.7 (  108x)   copies + soft_nms_pytorch on the CPU   10.5 (  20x)
      1000 boxes, one problem, gaussian    kept   179   ops.soft_nms  0.567   soft_nms_pytorch on the GPU    61.0 (  108x)   copies + soft_nms_pytorch on the CPU   10.7 (  19x)
      4000 boxes, one problem, linear      kept   459   ops.soft_nms  1.711   soft_nms_pytorch on the GPU   158.6 (   93x)   copies + soft_nms_pytorch on the CPU   52.3 (  31x)
      4000 boxes, one problem, gaussian    kept   420   ops.soft_nms  1.821   soft_nms_pytorch on the GPU   143.4 (   79x)   copies + soft_nms_pytorch on the CPU   52.5 (  29x)
      80 labels x 250 boxes, linear        kept  3852   ops.soft_nms  0.405   soft_nms_pytorch on the GPU  1082.4 ( 2673x)   copies + soft_nms_pytorch on the CPU  191.0 ( 472x)
      80 labels x 250 boxes, gaussian      kept  4410   ops.soft_nms  0.392   soft_nms_pytorch on the GPU  1216.9 ( 3104x)   copies + soft_nms_pytorch on the CPU  211.2 ( 539x)

  * border: BorderAlign in a BorderDet head (2 x (4 x 256) x 100 x 152, the P3 map of an 800 x 1216 image; one box per location,
    K = H W = 15200, its four sides log-uniform in 1 to 24 cells from the location; pool_size 10), float32 and float16:
    ops.border_align beside ops.border_align_pytorch (index gathers and torch.max, autograd's backward), forward and forward + backward,
    in alternating windows.  Informational: no speed bound is set.

  * riroi: RiRoIAlignRotated in a ReDet head (2 x (32 x 8) x 128 x 128, 512 RoIs, 7 x 7, num_samples 2), float32 and float16:
    ops.riroi_align_rotated beside the two-step route (ops.roi_align_rotated, then ops.riroi_align_rotated_pytorch's torch blend) and
    beside plain ops.roi_align_rotated on the same shapes (the fused forward does its loads plus one LDS exchange, so the ratio to it
    is what the blend costs), forward and forward + backward, in alternating windows.  Informational: no speed bound is set.

  * rfa: rotated_feature_align in an R3Det head (2 x 256 x 128 x 128, points 5, spatial_scale 1 / 8), float32 and float16:
    ops.rotated_feature_align beside ops.rotated_feature_align_pytorch (index gathers, autograd's backward), forward and
    forward + backward, in alternating windows.  Informational: no speed bound is set.

  * convex: the point-set operators of Oriented RepPoints / CFA / SASM on a 1024 x 1024 image, float32: ops.convex_iou of 20000 point
    sets against 64 polygons (the assigner: half of the sets lie around a polygon, half anywhere), ops.convex_giou of 4096 aligned
    pairs, forward and forward + backward (the loss), and ops.min_area_polygons of the 20000 sets, each beside its _pytorch
    composition on the same GPU, in alternating windows.  Informational: no speed bound is set.

  * quadri: the quadrilateral operators on a 1024 x 1024 image, float32: ops.box_iou_quadri of 20000 quadrilaterals against 64 (the
    assigner: half of them lie around one of the 64, half anywhere), ops.nms_quadri of 4096 clustered quadrilaterals at threshold 0.1
    with and without 15 labels, and ops.points_in_polygons of 20000 points against 64 polygons, each beside its _pytorch composition on
    the same GPU (for NMS: ops.box_iou_quadri_pytorch's matrix, then a greedy pass on the host).  Informational: no speed bound is set.

  * mconv: ops.masked_conv2d at GA-RetinaNet's two head shapes (256 -> 80 and 256 -> 4, 1 x 1) and one 3 x 3, 256 -> 256 shape, on a
    100 x 152 map, one image, at 5 %, 25 % and 100 % active pixels, in float32 and bfloat16, NCHW and channels_last, beside what a head
    does without the operator (dense F.conv2d, then * mask) and beside ops.masked_conv2d_pytorch on the same GPU (mmcv's composition,
    its nonzero synchronisation included), in alternating windows.  Informational: no speed bound is set.

  * mask: the mask operators of a Mask R-CNN's last step at K = 100 masks of 28 x 28 on an 800 x 1333 image (boxes of 30 to 400 pixels a
    side, some over the image's sides): ops.paste_masks_in_image (padding 1; float32 and float16) beside its _pytorch twin and beside
    torchvision's loop restated (per mask four host reads, F.interpolate, zeros and a slice copy); ops.paste_masks_aligned (bool at 0.5,
    uint8) beside its twin and beside the grid_sample composition of detectron2 / mmdetection in one chunk; ops.masks_to_boxes on the
    pasted bool masks beside its twin.  Each operator's row also holds the bytes it writes (reads, for masks_to_boxes), the rate, and
    that rate as a share of the 8 TB/s HBM peak.  Informational: no speed bound is set.

  * keypoint: the last step of a Keypoint R-CNN at R = 100 detections of an 800 x 1333 image (boxes of 30 to 400 pixels a side), K = 17
    keypoints, 56 x 56 maps: ops.heatmaps_to_keypoints_scored (float32 and float16 maps) beside its _pytorch twin on the same device,
    which is upstream's loop (two host reads, F.interpolate(bicubic), argmax and a gather per detection); and one case of R = 4
    image-sized boxes, where a block walks a million pixels: the case that says whether a large box should be split over several
    blocks.  Each row also holds the pixels of the resized images and the operator's rate over them.  Informational: no speed bound
    is set.

    python tools/ops_bench.py --only keypoint        # just the keypoint leg
    python tools/ops_bench.py --only mask            # just the mask leg
    python tools/ops_bench.py --only mconv           # just the masked-convolution leg
    python tools/ops_bench.py --only quadri          # just the quadrilateral leg
    python tools/ops_bench.py --only convex          # just the point-set leg
    python tools/ops_bench.py --only rfa             # just the rotated_feature_align leg
    python tools/ops_bench.py --only riroi           # just the RiRoIAlignRotated leg
    python tools/ops_bench.py --only border          # just the BorderAlign leg
    python tools/ops_bench.py --only softnms         # just the Soft-NMS leg
    python tools/ops_bench.py --only diffiou         # just the differentiable-IoU leg
    python tools/ops_bench.py --only dcnv4           # just the DCNv4 leg
    python tools/ops_bench.py --only dcnv3           # just the DCNv3 leg
    python tools/ops_bench.py --only prroi           # just the Precise-RoI-Pooling leg
    python tools/ops_bench.py --only msda            # just the deformable-attention leg
    python tools/ops_bench.py --only carafe          # just the CARAFE leg
    python tools/ops_bench.py --only rot             # just the rotated-box leg
    python tools/ops_bench.py --only multiscale      # just the multi-scale leg
    python tools/ops_bench.py --only droi            # just the deformable-RoI-pooling leg
    python tools/ops_bench.py --only deform          # just the deformable-convolution leg
    python tools/ops_bench.py --only ps              # just the position-sensitive leg
    python tools/ops_bench.py --only half            # just the 16-bit leg
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fasterrcnn_amd import _native as nv          # noqa: E402
from fasterrcnn_amd import ops                    # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / reps)
    return float(np.median(ts))


def timed_pair(fa, fb, reps, warmup):
    """timed() of two callables in alternating windows (a, b, a, b, ...): medians of 5 each"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(5):
        for fn, t in ((fa, ts[0]), (fb, ts[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1000.0 / reps)
    return float(np.median(ts[0])), float(np.median(ts[1]))


def timed_group(fns, reps, warmup):
    """timed_pair for any number of callables: windows in the order a, b, c, a, b, c, ...; medians of 5 each"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(5):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1000.0 / reps)
    return [float(np.median(t)) for t in ts]


def tv_multiscale(features, rois, scales, k_min, k_max):
    """torchvision's _multiscale_roi_align over ops.roi_align (7 x 7, sampling_ratio 2): LevelMapper, then per level torch.where (a host
    sync each), roi_align and index_put"""
    b = rois[:, 1:]
    s = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    levels = torch.clamp(torch.floor(4 + torch.log2(s / 224) + torch.tensor(1e-6, dtype=s.dtype)), min=k_min, max=k_max)
    levels = levels.to(torch.int64) - k_min
    result = torch.zeros((rois.shape[0], features[0].shape[1], 7, 7), device=rois.device)
    for level, (f, sc) in enumerate(zip(features, scales)):
        idx = torch.where(levels == level)[0]
        result[idx] = ops.roi_align(f, rois[idx], 7, sc, 2)
    return result


def multiscale_leg(rng, reps, warmup):
    n, c = 2, 256
    shapes = [(200, 304), (100, 152), (50, 76), (25, 38)]
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    feats = [torch.randn((n, c, h, w), device=DEV).contiguous(memory_format=torch.channels_last) for h, w in shapes]
    feats_g = [f.clone().requires_grad_(True) for f in feats]
    res = {}
    for per_img in (512, 1000):
        k = n * per_img
        side = np.exp(rng.uniform(np.log(16), np.log(800), (k, 2)))
        x1, y1 = rng.uniform(0, 1216 - 16, k), rng.uniform(0, 800 - 16, k)
        rois = np.stack([np.repeat(np.arange(n), per_img), x1, y1, np.minimum(x1 + side[:, 0], 1216), np.minimum(y1 + side[:, 1], 800)], 1)
        rois = torch.from_numpy(rois.astype(np.float32)).to(DEV)
        g = torch.randn((k, c, 7, 7), device=DEV)
        b = rois[:, 1:]
        lv = (torch.clamp(torch.floor(4 + torch.log2(torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224) + 1e-6), 2, 5) - 2).long()
        r = {"rois per level": torch.bincount(lv, minlength=4).tolist()}
        fwd = timed_pair(lambda: ops.multi_scale_roi_align(feats, rois, 7, scales, 2), lambda: tv_multiscale(feats, rois, scales, 2, 5),
                         reps, warmup)
        fb = timed_pair(lambda: ops.multi_scale_roi_align(feats_g, rois, 7, scales, 2).backward(g),
                        lambda: tv_multiscale(feats_g, rois, scales, 2, 5).backward(g), reps, warmup)
        r["ops.multi_scale_roi_align fwd"], r["composition fwd"] = fwd
        r["ops.multi_scale_roi_align fwd+bwd"], r["composition fwd+bwd"] = fb
        r["ops.roi_align fwd, all RoIs on level 0"] = timed(lambda: ops.roi_align(feats[0], rois, 7, 0.25, 2), reps, warmup)
        res["multi-scale fpn 2 x 256 x 200 x 304 .. 25 x 38, %d RoIs per image, 7 x 7, sr 2" % per_img] = r
    return res


def half_rows(op, x16, g, reps, warmup):
    """op(list of maps) -> pooled, on the 16-bit maps x16: microseconds of the native op, of the float32 op on the same values and of the
    composition op(x.float()).to(T), forward and forward + backward (gradient g in the maps' dtype), with the ratios to the native op"""
    dtype = x16[0].dtype
    x32 = [x.float() for x in x16]
    x16g = [x.clone().requires_grad_(True) for x in x16]
    x32g = [x.clone().requires_grad_(True) for x in x32]
    g32 = g.float()

    def composed(xs):
        return op([x.float() for x in xs]).to(dtype)
    r = {}
    for name, fns in (("fwd", (lambda: op(x16), lambda: op(x32), lambda: composed(x16))),
                      ("fwd+bwd", (lambda: op(x16g).backward(g), lambda: op(x32g).backward(g32), lambda: composed(x16g).backward(g)))):
        native, f32, comp = timed_group(fns, reps, warmup)
        r[name] = {"native 16-bit": round(native, 1), "float32 op": round(f32, 1), "op(x.float()).to(T)": round(comp, 1),
                   "float32 / native": round(f32 / native, 2), "composition / native": round(comp / native, 2)}
    return r


def half_leg(rng, reps, warmup):
    res = {}
    n, c = 2, 256
    shapes = [(200, 304), (100, 152), (50, 76), (25, 38)]
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    feats = [torch.randn((n, c, h, w), device=DEV).contiguous(memory_format=torch.channels_last) for h, w in shapes]
    vgg = torch.relu(torch.randn((1, 512, 37, 62), device=DEV)).contiguous(memory_format=torch.channels_last)
    fpn_rois = {}
    for per_img in (512, 1000):
        k = n * per_img
        side = np.exp(rng.uniform(np.log(16), np.log(800), (k, 2)))
        x1, y1 = rng.uniform(0, 1216 - 16, k), rng.uniform(0, 800 - 16, k)
        rois = np.stack([np.repeat(np.arange(n), per_img), x1, y1, np.minimum(x1 + side[:, 0], 1216), np.minimum(y1 + side[:, 1], 800)], 1)
        fpn_rois[per_img] = torch.from_numpy(rois.astype(np.float32)).to(DEV)
    props = torch.from_numpy(proposals(rng, 300, 600, 1000)).to(DEV)
    vgg_rois = torch.cat([torch.zeros((300, 1), device=DEV), props[:, [1, 0, 3, 2]]], 1)
    for dtype in (torch.float16, torch.bfloat16):
        name = str(dtype).split(".")[-1]
        for per_img, rois in fpn_rois.items():
            g = torch.randn((rois.shape[0], c, 7, 7), device=DEV).to(dtype)
            res["%s multi_scale_roi_align fpn 2 x 256 x 200 x 304 .. 25 x 38, %d RoIs per image" % (name, per_img)] = half_rows(
                lambda xs: ops.multi_scale_roi_align(xs, rois, 7, scales, 2), [f.to(dtype) for f in feats], g, reps, warmup)
        g = torch.randn((300, 512, 7, 7), device=DEV).to(dtype)
        res["%s roi_align vgg16 map 512 x 37 x 62, 300 RoIs" % name] = half_rows(
            lambda xs: ops.roi_align(xs[0], vgg_rois, 7, 1 / 16, 2), [vgg.to(dtype)], g, reps, warmup)
        res["%s roi_pool vgg16 map 512 x 37 x 62, 300 RoIs" % name] = half_rows(
            lambda xs: ops.roi_pool(xs[0], vgg_rois, 7, 1 / 16), [vgg.to(dtype)], g, reps, warmup)
    return res


def ps_leg(rng, reps, warmup):
    oh = ow = 7
    classes, k, h, w, scale, sr = 21, 300, 38, 63, 1 / 16, 2
    c = oh * ow * classes
    props = torch.from_numpy(proposals(rng, k, 600, 1000)).to(DEV)
    rois = torch.cat([torch.zeros((k, 1), device=DEV), props[:, [1, 0, 3, 2]]], 1)
    ph, pw = torch.meshgrid(torch.arange(oh, device=DEV), torch.arange(ow, device=DEV), indexing="ij")
    ci = (torch.arange(classes, device=DEV)[:, None, None] * oh + ph[None]) * ow + pw[None]

    def composed(x):
        return ops.roi_align(x, rois, (oh, ow), scale, sr, aligned=True)[:, ci, ph[None], pw[None]]
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((1, c, h, w), device=DEV).to(dtype)
        xg = x.clone().requires_grad_(True)
        g = torch.randn((k, classes, oh, ow), device=DEV).to(dtype)
        y, yc = ops.ps_roi_align(x, rois, (oh, ow), scale, sr), composed(x)
        r = {"max |ps_roi_align - composition|": float((y.float() - yc.float()).abs().max())}
        for name, fns in (("fwd", (lambda: ops.ps_roi_align(x, rois, (oh, ow), scale, sr), lambda: composed(x))),
                          ("fwd+bwd", (lambda: ops.ps_roi_align(xg, rois, (oh, ow), scale, sr).backward(g), lambda: composed(xg).backward(g)))):
            native, comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.ps_roi_align": round(native, 1), "roi_align(aligned) + diagonal gather": round(comp, 1),
                       "composition / ps_roi_align": round(comp / native, 2)}
        r["ops.ps_roi_pool fwd"] = round(timed(lambda: ops.ps_roi_pool(x, rois, (oh, ow), scale), reps, warmup), 1)
        r["ops.ps_roi_pool fwd+bwd"] = round(timed(lambda: ops.ps_roi_pool(xg, rois, (oh, ow), scale).backward(g), reps, warmup), 1)
        res["%s r-fcn voc 1 x %d x %d x %d, %d RoIs, 7 x 7, sr 2" % (str(dtype).split(".")[-1], c, h, w, k)] = r
    return res


def deform_leg(rng, reps, warmup):
    from tests import deform_conv_cases as D
    n, c, co, h, w = 2, 256, 256, 50, 68
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((n, c, h, w), generator=gen).to(DEV)
    weight = (torch.randn((co, c, 3, 3), generator=gen) / 48).to(DEV)
    bias = torch.randn((co,), generator=gen).to(DEV)
    g = torch.randn((n, co, h, w), generator=gen).to(DEV)
    res = {}
    for groups in (1, 4):
        offset = (torch.randn((n, 2 * groups * 9, h, w), generator=gen) * 2).to(DEV)
        for with_mask in (False, True):
            mask = torch.rand((n, groups * 9, h, w), generator=gen).to(DEV) if with_mask else None
            leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, offset, weight, bias, mask)]

            def native(a=(x, offset, weight, bias, mask)):
                return ops.deform_conv2d(a[0], a[1], a[2], a[3], padding=1, mask=a[4])

            def composed(a=(x, offset, weight, bias, mask)):
                return D.deform_conv2d_ref(a[0], a[1], a[2], a[3], padding=(1, 1), mask=a[4])
            y, yc = native(), composed()
            r = {"max |deform_conv2d - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
            for name, fns in (("fwd", (native, composed)),
                              ("fwd+bwd", (lambda: native(leaves).backward(g), lambda: composed(leaves).backward(g)))):
                t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
                r[name] = {"ops.deform_conv2d": round(t_native, 1), "torch composition": round(t_comp, 1),
                           "composition / deform_conv2d": round(t_comp / t_native, 2)}
            res["deform 2 x 256 -> 256, 3 x 3, pad 1, 50 x 68, G %d, %s" % (groups, "mask" if with_mask else "no mask")] = r
            # float16 / bfloat16: the 16-bit operator beside the float32 operator on the widened tensors (the only way to run the call before)
            for dtype in (torch.float16, torch.bfloat16):
                half = [t.to(dtype) if t is not None else None for t in (x, offset, weight, bias, mask)]
                wide = [t.float() if t is not None else None for t in half]
                leaves16 = [t.clone().requires_grad_(True) if t is not None else None for t in half]
                leaves32 = [t.clone().requires_grad_(True) if t is not None else None for t in wide]
                g16 = g.to(dtype)
                y16, y32 = native(half).float(), native(wide)
                r = {"max |16-bit - float32 of the widened tensors| / max |float32|": float((y16 - y32).abs().max() / y32.abs().max())}
                for name, fns in (("fwd", (lambda: native(half), lambda: native(wide))),
                                  ("fwd+bwd", (lambda: native(leaves16).backward(g16), lambda: native(leaves32).backward(g16.float())))):
                    t_half, t_wide = timed_pair(fns[0], fns[1], reps, warmup)
                    r[name] = {"ops.deform_conv2d %s" % str(dtype).split(".")[-1]: round(t_half, 1),
                               "ops.deform_conv2d float32 (widened)": round(t_wide, 1), "float32 / 16-bit": round(t_wide / t_half, 2)}
                res["deform %s 2 x 256 -> 256, 3 x 3, pad 1, 50 x 68, G %d, %s" % (str(dtype).split(".")[-1], groups,
                                                                                  "mask" if with_mask else "no mask")] = r
    return res


def droi_leg(rng, reps, warmup):
    from tests import deform_roi_cases as D
    n, c, h, w, k, out, scale, sr, gamma = 2, 256, 50, 68, 512, (7, 7), 1 / 16, 2, 0.1
    gen = torch.Generator().manual_seed(0)
    props = proposals(rng, k, 800, 1088)
    rois = torch.from_numpy(np.concatenate([(np.arange(k) % n).astype(np.float32)[:, None], props[:, [1, 0, 3, 2]]], 1)).to(DEV)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((n, c, h, w), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        g = torch.randn((k, c) + out, generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        for with_offset in (False, True):
            offset = (torch.randn((k, 2) + out, generator=gen) * 0.5).to(DEV) if with_offset else None
            case = {"rois": rois, "output_size": out, "sampling_ratio": sr, "gamma": D.f32(gamma), "spatial_scale": D.f32(scale),
                    "input": x, "offset": offset}
            leaves = [x.clone().requires_grad_(True), offset.clone().requires_grad_(True) if with_offset else None]

            def native(a=(x, offset)):
                return ops.deform_roi_pool(a[0], rois, a[1], out, scale, sr, gamma)

            def composed(a=(x, offset)):
                return D.forward_ref(dict(case, offset=a[1]), torch.float32, input=a[0]).to(dtype)     # float32 arithmetic, as the op's
            y, yc = native().float(), composed().float()
            r = {"max |deform_roi_pool - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
            for name, fns in (("fwd", (native, composed)),
                              ("fwd+bwd", (lambda: native(leaves).backward(g), lambda: composed(leaves).backward(g)))):
                t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
                r[name] = {"ops.deform_roi_pool": round(t_native, 1), "torch composition": round(t_comp, 1),
                           "composition / deform_roi_pool": round(t_comp / t_native, 2)}
            res["droi %s 2 x 256 x 50 x 68, 512 RoIs, 7 x 7, sr 2, %s" % (str(dtype).split(".")[-1], "offset" if with_offset else "no offset")] = r
    return res


def rot_leg(rng, reps, warmup):
    res = {}
    nb = 12000
    b = proposals(rng, nb, 600, 1000)[:, [1, 0, 3, 2]]
    corners = torch.from_numpy(b).to(DEV)
    angle = torch.from_numpy(rng.uniform(-np.pi, np.pi, nb).astype(np.float32)).to(DEV)
    centre, size = (corners[:, :2] + corners[:, 2:]) / 2, corners[:, 2:] - corners[:, :2]
    boxes = torch.cat([centre, size, angle[:, None]], 1)
    scores = torch.rand((nb,), device=DEV)
    kept = len(ops.nms_rotated(boxes, scores, 0.5)[1])
    t_rot, t_plain = timed_pair(lambda: ops.nms_rotated(boxes, scores, 0.5), lambda: ops.nms(corners, scores, 0.5), reps, warmup)
    res["nms_rotated %d boxes (0.5), %d kept" % (nb, kept)] = {"ops.nms_rotated": round(t_rot, 1), "ops.nms at angle 0": round(t_plain, 1)}
    n, c, h, w, k, out, scale, sr = 2, 256, 50, 68, 512, (7, 7), 1 / 16, 2
    props = proposals(rng, k, 800, 1088)[:, [1, 0, 3, 2]]
    img = (np.arange(k) % n).astype(np.float32)[:, None]
    plain = torch.from_numpy(np.concatenate([img, props], 1)).to(DEV)
    rot = np.concatenate([img, (props[:, :2] + props[:, 2:]) / 2, props[:, 2:] - props[:, :2],
                          rng.uniform(-np.pi, np.pi, (k, 1)).astype(np.float32)], 1)
    rois = torch.from_numpy(rot.astype(np.float32)).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((n, c, h, w), device=DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        g = torch.randn((k, c) + out, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        xg = x.clone().requires_grad_(True)
        r = {}
        for name, fns in (("fwd", (lambda: ops.roi_align_rotated(x, rois, out, scale, sr), lambda: ops.roi_align(x, plain, out, scale, sr, True))),
                          ("fwd+bwd", (lambda: ops.roi_align_rotated(xg, rois, out, scale, sr).backward(g),
                                       lambda: ops.roi_align(xg, plain, out, scale, sr, True).backward(g)))):
            t_rot, t_plain = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.roi_align_rotated": round(t_rot, 1), "ops.roi_align, axis-aligned": round(t_plain, 1),
                       "rotated / axis-aligned": round(t_rot / t_plain, 2)}
        res["rot %s 2 x 256 x 50 x 68, 512 RoIs, 7 x 7, sr 2" % str(dtype).split(".")[-1]] = r
    return res


HBM_PEAK = 8.0e12        # bytes / s, the MI355X's specified HBM3E peak


def carafe_leg(rng, reps, warmup):
    import torch.nn.functional as F
    n, c, h, w, k, G, s = 2, 256, 100, 168, 5, 1, 2
    gen = torch.Generator().manual_seed(0)

    def composed(x, m):
        cols = F.unfold(x, k, padding=(k - 1) // 2).view(n, c * k * k, h, w)
        cols = F.interpolate(cols, scale_factor=s, mode="nearest").view(n, G, c // G, k * k, s * h, s * w)
        return (cols * m.view(n, G, 1, k * k, s * h, s * w)).sum(3).view(n, c, s * h, s * w)
    res = {}
    for dtype in (torch.float32, torch.float16):
        x = torch.randn((n, c, h, w), generator=gen).to(DEV).to(dtype)
        m = torch.softmax(torch.randn((n, G, k * k, s * h, s * w), generator=gen).to(DEV), dim=2).view(n, G * k * k, s * h, s * w).to(dtype)
        g = torch.randn((n, c, s * h, s * w), generator=gen).to(DEV).to(dtype)
        xg, mg = x.clone().requires_grad_(True), m.clone().requires_grad_(True)
        y, yc = ops.carafe(x, m, k, G, s).float(), composed(x, m).float()
        r = {"max |carafe - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
        del y, yc
        for name, fns in (("fwd", (lambda: ops.carafe(x, m, k, G, s), lambda: composed(x, m))),
                          ("fwd+bwd", (lambda: ops.carafe(xg, mg, k, G, s).backward(g), lambda: composed(xg, mg).backward(g)))):
            t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.carafe": round(t_native, 1), "torch composition": round(t_comp, 1),
                       "composition / carafe": round(t_comp / t_native, 2)}
        nbytes = (x.numel() + m.numel() + g.numel()) * x.element_size()
        r["fwd algorithmic bytes (features + masks + result)"] = nbytes
        r["fwd bytes / s over the 8 TB/s HBM peak"] = round(nbytes / (r["fwd"]["ops.carafe"] * 1e-6) / HBM_PEAK, 3)
        res["carafe %s 2 x 256 x 100 x 168 -> 200 x 336, k 5, G 1" % str(dtype).split(".")[-1]] = r
    return res


def msda_leg(rng, reps, warmup):
    b, m, d, p = 2, 8, 32, 4
    shapes = [(100, 134), (50, 67), (25, 34), (13, 17)]
    gen = torch.Generator().manual_seed(0)
    spatial = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    starts = torch.tensor([sum(h * w for h, w in shapes[:l]) for l in range(len(shapes))], dtype=torch.int64, device=DEV)
    s = q = sum(h * w for h, w in shapes)
    # the encoder's reference points: the centre of the query's own cell, normalised, the same on every level
    centres = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij"), -1).view(-1, 2)
                         for h, w in shapes])[:, [1, 0]]                                    # (x, y)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)
    loc = (centres.view(1, q, 1, 1, 1, 2) + 2.0 * torch.randn((b, q, m, len(shapes), p, 2), generator=gen) / norm.view(1, 1, 1, -1, 1, 2))
    res = {}
    for dtype in (torch.float32, torch.float16):
        v = torch.randn((b, s, m, d), generator=gen).to(DEV).to(dtype)
        lo = loc.to(DEV).to(dtype)
        a = torch.softmax(torch.randn((b, q, m, len(shapes) * p), generator=gen), -1).view(b, q, m, len(shapes), p).to(DEV).to(dtype)
        g = torch.randn((b, q, m * d), generator=gen).to(DEV).to(dtype)
        vg, lg, ag = (t.clone().requires_grad_(True) for t in (v, lo, a))
        native = lambda *t: ops.multi_scale_deformable_attn(t[0], spatial, starts, t[1], t[2])          # noqa: E731
        composed = lambda *t: ops.multi_scale_deformable_attn_pytorch(t[0], spatial, t[1], t[2])       # noqa: E731
        y, yc = native(v, lo, a).float(), composed(v, lo, a).float()
        r = {"max |ops - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
        del y, yc
        for name, fns in (("fwd", (lambda: native(v, lo, a), lambda: composed(v, lo, a))),
                          ("fwd+bwd", (lambda: native(vg, lg, ag).backward(g), lambda: composed(vg, lg, ag).backward(g)))):
            t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.multi_scale_deformable_attn": round(t_native, 1), "multi_scale_deformable_attn_pytorch": round(t_comp, 1),
                       "composition / ops": round(t_comp / t_native, 2)}
        nbytes = (v.numel() + lo.numel() + a.numel() + g.numel()) * v.element_size()
        r["fwd algorithmic bytes (value + locations + weights + result)"] = nbytes
        r["fwd bytes / s over the 8 TB/s HBM peak"] = round(nbytes / (r["fwd"]["ops.multi_scale_deformable_attn"] * 1e-6) / HBM_PEAK, 3)
        res["msda %s encoder layer B 2, S = Q = 17821 over 4 levels, M 8, D 32, P 4" % str(dtype).split(".")[-1]] = r
    return res


def dcnv3_leg(rng, reps, warmup):
    n, h, w, group, gc, k = 2, 100, 160, 8, 16, 3
    geom = (k, k, 1, 1, 1, 1, 1, 1, group, gc, 1.0)
    gen = torch.Generator().manual_seed(0)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((n, h, w, group * gc), generator=gen).to(DEV).to(dtype)
        off = (2.0 * torch.randn((n, h, w, group * k * k * 2), generator=gen)).to(DEV).to(dtype)
        m = torch.softmax(torch.randn((n, h, w, group, k * k), generator=gen), -1).view(n, h, w, -1).to(DEV).to(dtype)
        g = torch.randn((n, h, w, group * gc), generator=gen).to(DEV).to(dtype)
        xg, og, mg = (t.clone().requires_grad_(True) for t in (x, off, m))
        native = lambda *t: ops.DCNv3Function.apply(*t, *geom, 256)              # noqa: E731
        composed = lambda *t: ops.dcnv3_core_pytorch(*t, *geom)                  # noqa: E731
        y, yc = native(x, off, m).float(), composed(x, off, m).float()
        r = {"max |ops - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
        del y, yc
        for name, fns in (("fwd", (lambda: native(x, off, m), lambda: composed(x, off, m))),
                          ("fwd+bwd", (lambda: native(xg, og, mg).backward(g), lambda: composed(xg, og, mg).backward(g)))):
            t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.dcnv3": round(t_native, 1), "dcnv3_core_pytorch": round(t_comp, 1), "composition / ops": round(t_comp / t_native, 2)}
        res["dcnv3 %s InternImage-T stage 2 x 100 x 160 x 128, G 8, Gc 16, 3 x 3, pad 1" % str(dtype).split(".")[-1]] = r
    return res


def dcnv4_leg(rng, reps, warmup):
    n, h, w, group, gc, k = 2, 100, 160, 8, 16, 3
    p = k * k
    geom = (k, k, 1, 1, 1, 1, 1, 1, group, gc, 1.0)
    length = (group * p * 3 + 7) // 8 * 8
    gen = torch.Generator().manual_seed(0)
    res = {}

    def unpack(om):
        rec = om[..., :group * p * 3].reshape(n, h, w, group, p * 3)
        return rec[..., :2 * p].reshape(n, h, w, group * p * 2), rec[..., 2 * p:].reshape(n, h, w, group * p)       # two strided copies

    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((n, h, w, group * gc), generator=gen).to(DEV).to(dtype)
        rec = torch.cat([2.0 * torch.randn((n, h, w, group, 2 * p), generator=gen), torch.randn((n, h, w, group, p), generator=gen)], -1)
        om = torch.nn.functional.pad(rec.reshape(n, h, w, group * p * 3), [0, length - group * p * 3]).to(DEV).to(dtype)
        g = torch.randn((n, h, w, group * gc), generator=gen).to(DEV).to(dtype)
        xg, omg = (t.clone().requires_grad_(True) for t in (x, om))
        native = lambda a, b: ops.DCNv4Function.apply(a, b, *geom, 256, False)       # noqa: E731
        composed = lambda a, b: ops.dcnv4_core_pytorch(a, b, *geom, False)           # noqa: E731
        via_v3 = lambda a, b: ops.DCNv3Function.apply(a, *unpack(b), *geom, 256)     # noqa: E731
        y, yc, y3 = native(x, om), composed(x, om).float(), via_v3(x, om)
        r = {"max |ops - composition| / max |composition|": float((y.float() - yc).abs().max() / yc.abs().max()),
             "ops.dcnv4 == ops.dcnv3 on the unpacked tensors": bool(torch.equal(y, y3))}
        del y, yc, y3
        for name, fns in (("fwd", (lambda: native(x, om), lambda: composed(x, om), lambda: via_v3(x, om))),
                          ("fwd+bwd", (lambda: native(xg, omg).backward(g), lambda: composed(xg, omg).backward(g),
                                       lambda: via_v3(xg, omg).backward(g)))):
            t_native, t_comp, t_v3 = timed_group(fns, reps, warmup)
            r[name] = {"ops.dcnv4": round(t_native, 1), "dcnv4_core_pytorch": round(t_comp, 1), "ops.dcnv3 with the copies": round(t_v3, 1),
                       "composition / ops": round(t_comp / t_native, 2), "dcnv3 with the copies / ops": round(t_v3 / t_native, 2)}
        res["dcnv4 %s 2 x 100 x 160 x 128, G 8, Gc 16, 3 x 3, pad 1, L %d" % (str(dtype).split(".")[-1], length)] = r
    return res


def prroi_leg(rng, reps, warmup):
    n, c, h, w, k, out, scale = 2, 256, 50, 68, 512, (7, 7), 1 / 16
    gen = torch.Generator().manual_seed(0)
    props = proposals(rng, k, 800, 1088)
    rois = torch.from_numpy(np.concatenate([(np.arange(k) % n).astype(np.float32)[:, None], props[:, [1, 0, 3, 2]]], 1)).to(DEV)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((n, c, h, w), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        g = torch.randn((k, c) + out, generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        leaves = (x.clone().requires_grad_(True), rois.clone().requires_grad_(True))

        def native(a=(x, rois)):
            return ops.prroi_pool(a[0], a[1], out, scale)

        def composed(a=(x, rois)):
            return ops.prroi_pool_pytorch(a[0], a[1], out, scale)
        y, yc = native().float(), composed().float()
        r = {"max |prroi_pool - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
        for name, fns in (("fwd", (native, composed)),
                          ("fwd+bwd (d_input and d_rois)", (lambda: native(leaves).backward(g), lambda: composed(leaves).backward(g)))):
            t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.prroi_pool": round(t_native, 1), "ops.prroi_pool_pytorch": round(t_comp, 1),
                       "composition / prroi_pool": round(t_comp / t_native, 2)}
        res["prroi %s 2 x 256 x 50 x 68, 512 RoIs, 7 x 7" % str(dtype).split(".")[-1]] = r
    return res


def border_leg(rng, reps, warmup):
    n, c, h, w, pool = 2, 256, 100, 152, 10
    gen = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    sides = torch.exp(torch.rand((n, h * w, 4), generator=gen) * float(np.log(24.0)))            # left, top, right, bottom
    centre = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)[None]
    boxes = torch.cat([centre - sides[..., :2], centre + sides[..., 2:]], 2).to(DEV)
    res = {}
    for dtype in (torch.float32, torch.float16):
        x = torch.randn((n, 4 * c, h, w), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        g = torch.randn((n, c, h * w, 4), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        leaf = x.clone().requires_grad_(True)

        def native(a=x):
            return ops.border_align(a, boxes, pool)

        def composed(a=x):
            return ops.border_align_pytorch(a, boxes, pool)
        y, yc = native().float(), composed().float()
        r = {"max |border_align - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
        for name, fns in (("fwd", (native, composed)),
                          ("fwd+bwd", (lambda: native(leaf).backward(g), lambda: composed(leaf).backward(g)))):
            t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.border_align": round(t_native, 1), "ops.border_align_pytorch": round(t_comp, 1),
                       "composition / border_align": round(t_comp / t_native, 2)}
        res["border %s 2 x (4 x 256) x 100 x 152, K 15200, pool_size 10" % str(dtype).split(".")[-1]] = r
    return res


def riroi_leg(rng, reps, warmup):
    n, groups, orient, h, w, k, out, ns, scale = 2, 32, 8, 128, 128, 512, (7, 7), 2, 0.25
    c = groups * orient
    gen = torch.Generator().manual_seed(0)
    u = lambda lo, hi: torch.rand((k,), generator=gen) * (hi - lo) + lo     # noqa: E731
    rois = torch.stack([(torch.arange(k) % n).float(), u(0, w / scale), u(0, h / scale), u(16, 160), u(16, 160), u(-np.pi, np.pi)], 1).to(DEV)
    res = {}
    for dtype in (torch.float32, torch.float16):
        x = torch.randn((n, c, h, w), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        g = torch.randn((k, c) + out, generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        leaf = x.clone().requires_grad_(True)

        def fused(a=x):
            return ops.riroi_align_rotated(a, rois, out, scale, ns, orient, False)

        def plain(a=x):
            return ops.roi_align_rotated(a, rois, out, scale, ns, False, True)

        def two_step(a=x):
            return ops.riroi_align_rotated_pytorch(plain(a), rois, orient)
        y, yc = fused().float(), two_step().float()
        r = {"max |riroi_align_rotated - two-step| / max |two-step|": float((y - yc).abs().max() / yc.abs().max())}
        for name, fns in (("fwd", (fused, two_step, plain)),
                          ("fwd+bwd", (lambda: fused(leaf).backward(g), lambda: two_step(leaf).backward(g), lambda: plain(leaf).backward(g)))):
            t_fused, t_two, t_plain = timed_group(fns, reps, warmup)
            r[name] = {"ops.riroi_align_rotated": round(t_fused, 1), "roi_align_rotated + torch blend": round(t_two, 1),
                       "plain ops.roi_align_rotated": round(t_plain, 1), "two-step / riroi_align_rotated": round(t_two / t_fused, 2),
                       "riroi_align_rotated / plain roi_align_rotated": round(t_fused / t_plain, 2)}
        res["riroi %s 2 x (32 x 8) x 128 x 128, 512 RoIs, 7 x 7, num_samples 2" % str(dtype).split(".")[-1]] = r
    return res


def rfa_leg(rng, reps, warmup):
    n, c, h, w, points, scale = 2, 256, 128, 128, 5, 1 / 8
    gen = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    u = lambda lo, hi: torch.rand((n, h, w), generator=gen) * (hi - lo) + lo     # noqa: E731
    # refined boxes around their own locations, in input coordinates: (y, x, w, h, angle) rows
    boxes = torch.stack([(ys[None] + u(-2, 2)) / scale, (xs[None] + u(-2, 2)) / scale, u(2, 24) / scale, u(2, 24) / scale,
                         u(-np.pi / 2, np.pi / 2)], 3).to(DEV)
    res = {}
    for dtype in (torch.float32, torch.float16):
        x = torch.randn((n, c, h, w), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        g = torch.randn((n, c, h, w), generator=gen).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        leaf = x.clone().requires_grad_(True)

        def native(a=x):
            return ops.rotated_feature_align(a, boxes, scale, points)

        def composed(a=x):
            return ops.rotated_feature_align_pytorch(a, boxes, scale, points)
        y, yc = native().float(), composed().float()
        r = {"max |rotated_feature_align - composition| / max |composition|": float((y - yc).abs().max() / yc.abs().max())}
        for name, fns in (("fwd", (native, composed)),
                          ("fwd+bwd", (lambda: native(leaf).backward(g), lambda: composed(leaf).backward(g)))):
            t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
            r[name] = {"ops.rotated_feature_align": round(t_native, 1), "ops.rotated_feature_align_pytorch": round(t_comp, 1),
                       "composition / rotated_feature_align": round(t_comp / t_native, 2)}
        res["rfa %s 2 x 256 x 128 x 128, points 5, spatial_scale 1/8" % str(dtype).split(".")[-1]] = r
    return res


def convex_leg(rng, reps, warmup):
    n, k, pairs = 20000, 64, 4096

    def rot(a):
        return np.stack([np.stack([np.cos(a), -np.sin(a)], -1), np.stack([np.sin(a), np.cos(a)], -1)], -2)

    def boxes(m):
        return rng.uniform(0, 1024, (m, 2)), np.exp(rng.uniform(np.log(16), np.log(256), (m, 2))), rng.uniform(-np.pi / 2, np.pi / 2, m)

    def polygons(c, wh, a):
        corners = np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]])[None] * wh[:, None]
        return (np.einsum("nij,nkj->nki", rot(a), corners) + c[:, None]).reshape(-1, 8)

    def pointsets(c, wh, a):
        m = c.shape[0]
        p = rng.uniform(-0.7, 0.7, (m, 9, 2)) * wh[:, None]
        return (np.einsum("nij,nkj->nki", rot(a + rng.uniform(-0.3, 0.3, m)), p) + (rng.uniform(-0.2, 0.2, (m, 2)) * wh + c)[:, None]).reshape(-1, 18)

    to = lambda v: torch.from_numpy(v.astype(np.float32)).to(DEV)     # noqa: E731
    c, wh, a = boxes(k)
    polys = to(polygons(c, wh, a))
    pick = np.arange(n) % k
    cs = np.where((np.arange(n) % 2 == 0)[:, None], c[pick], rng.uniform(0, 1024, (n, 2)))
    sets = to(pointsets(cs, wh[pick], a[pick]))
    c, wh, a = boxes(pairs)
    pair_sets, pair_polys, g = to(pointsets(c, wh, a)), to(polygons(c, wh, a)), to(rng.uniform(-1, 1, pairs))
    leaf = pair_sets.clone().requires_grad_(True)
    iou, iou_c = ops.convex_iou(sets, polys), ops.convex_iou_pytorch(sets, polys)
    giou, giou_c = ops.convex_giou(pair_sets, pair_polys), ops.convex_giou_pytorch(pair_sets, pair_polys)
    res = {"max |convex_iou - composition|": float((iou - iou_c).abs().max()), "share of pairs with IoU > 0": float((iou > 0).float().mean()),
           "max |giou - composition|": float((giou[0] - giou_c[0]).abs().max()), "mean giou": float(giou[0].mean()),
           "median |grad - composition| / max |grad|": float((giou[1] - giou_c[1]).abs().amax(1).median() / giou_c[1].abs().max()),
           "median |min_area_polygons - composition|": float((ops.min_area_polygons(sets) - ops.min_area_polygons_pytorch(sets)).abs().amax(1).median())}
    for name, native, comp in (
            ("convex_iou %d x %d" % (n, k), lambda: ops.convex_iou(sets, polys), lambda: ops.convex_iou_pytorch(sets, polys)),
            ("convex_giou %d fwd" % pairs, lambda: ops.convex_giou(pair_sets, pair_polys), lambda: ops.convex_giou_pytorch(pair_sets, pair_polys)),
            ("convex_giou %d fwd+bwd" % pairs, lambda: ops.convex_giou(leaf, pair_polys)[0].backward(g),
             lambda: ops.convex_giou_pytorch(leaf, pair_polys)[0].backward(g)),
            ("min_area_polygons %d" % n, lambda: ops.min_area_polygons(sets), lambda: ops.min_area_polygons_pytorch(sets))):
        t_native, t_comp = timed_pair(native, comp, reps, warmup)
        res[name] = {"ops": round(t_native, 1), "_pytorch composition": round(t_comp, 1), "composition / ops": round(t_comp / t_native, 2)}
    return {"convex float32 (microseconds)": res}


def quadri_leg(rng, reps, warmup):
    import time
    n, k, boxes, n_labels, thr = 20000, 64, 4096, 15, 0.1

    def rot(a):
        return np.stack([np.stack([np.cos(a), -np.sin(a)], -1), np.stack([np.sin(a), np.cos(a)], -1)], -2)

    def quads(c, wh, a):
        corners = (np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]])[None] + rng.uniform(-0.15, 0.15, (c.shape[0], 4, 2))) * wh[:, None]
        return (np.einsum("nij,nkj->nki", rot(a), corners) + c[:, None]).reshape(-1, 8)

    to = lambda v: torch.from_numpy(v.astype(np.float32)).to(DEV)     # noqa: E731
    c, wh, a = rng.uniform(0, 1024, (k, 2)), np.exp(rng.uniform(np.log(16), np.log(256), (k, 2))), rng.uniform(-np.pi / 2, np.pi / 2, k)
    gts = to(quads(c, wh, a))
    pick = np.arange(n) % k
    around = (np.arange(n) % 2 == 0)[:, None]
    cs = np.where(around, c[pick] + rng.uniform(-0.3, 0.3, (n, 2)) * wh[pick], rng.uniform(0, 1024, (n, 2)))
    rows = to(quads(cs, wh[pick] * np.exp(rng.uniform(-0.3, 0.3, (n, 1))), a[pick] + rng.uniform(-0.3, 0.3, n)))
    points = to(np.where(around, c[pick] + np.einsum("nij,nj->ni", rot(a[pick]), rng.uniform(-0.8, 0.8, (n, 2)) * wh[pick]),
                         rng.uniform(0, 1024, (n, 2))))
    groups = boxes // 8                                                        # clusters of eight around one base quadrilateral
    gc, gwh, ga = rng.uniform(0, 1024, (groups, 2)), np.exp(rng.uniform(np.log(16), np.log(128), (groups, 2))), rng.uniform(-np.pi / 2, np.pi / 2, groups)
    g = np.arange(boxes) % groups
    dets = to(quads(gc[g] + rng.uniform(-0.3, 0.3, (boxes, 2)) * gwh[g], gwh[g] * np.exp(rng.uniform(-0.3, 0.3, (boxes, 1))),
                    ga[g] + rng.uniform(-0.3, 0.3, boxes)))
    scores = to(rng.uniform(0.02, 1.0, boxes))
    labels = torch.from_numpy(rng.randint(0, n_labels, boxes)).to(DEV)

    def composed_nms(lab):
        """The IoU matrix of the composition, then the greedy pass on the host; the kept indices."""
        order = torch.sort(scores, descending=True, stable=True).indices
        d = dets[order]
        over = ops.box_iou_quadri_pytorch(d, d) > thr
        if lab is not None:
            over &= lab[order][:, None] == lab[order][None, :]
        over = over.cpu().numpy()
        gone = np.zeros(boxes, dtype=bool)
        kept = []
        for i in range(boxes):
            if not gone[i]:
                kept.append(i)
                gone[i + 1:] |= over[i, i + 1:]
        return order[torch.tensor(kept, device=DEV)]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    iou, iou_c = ops.box_iou_quadri(rows, gts), ops.box_iou_quadri_pytorch(rows, gts)
    hit, hit_c = ops.points_in_polygons(points, gts), ops.points_in_polygons_pytorch(points, gts)
    res = {"max |box_iou_quadri - composition|": float((iou - iou_c).abs().max()), "share of pairs with IoU > 0": float((iou > 0).float().mean()),
           "points_in_polygons: pairs that differ from the composition": int((hit != hit_c).sum()), "share of pairs inside": float(hit.mean())}
    for name, native, comp in (
            ("box_iou_quadri %d x %d" % (n, k), lambda: ops.box_iou_quadri(rows, gts), lambda: ops.box_iou_quadri_pytorch(rows, gts)),
            ("points_in_polygons %d x %d" % (n, k), lambda: ops.points_in_polygons(points, gts), lambda: ops.points_in_polygons_pytorch(points, gts))):
        t_native, t_comp = timed_pair(native, comp, reps, warmup)
        res[name] = {"ops": round(t_native, 1), "_pytorch composition": round(t_comp, 1), "composition / ops": round(t_comp / t_native, 2)}
    for name, lab in (("nms_quadri %d, thr %s" % (boxes, thr), None), ("nms_quadri %d, thr %s, %d labels" % (boxes, thr, n_labels), labels)):
        keep = ops.nms_quadri(dets, scores, thr, lab)[1]
        keep_c = composed_nms(lab)
        t_native = timed(lambda: ops.nms_quadri(dets, scores, thr, lab), reps, warmup)
        t_comp = float(np.median([wall(lambda: composed_nms(lab)) for _ in range(3)]))
        res[name] = {"kept": int(keep.numel()), "kept by the composition": int(keep_c.numel()),
                     "kept by both": int(np.intersect1d(keep.cpu().numpy(), keep_c.cpu().numpy()).size),
                     "ops": round(t_native, 1), "matrix composition + host greedy pass": round(t_comp, 1),
                     "composition / ops": round(t_comp / t_native, 2)}
    return {"quadri float32 (microseconds)": res}


def mconv_leg(rng, reps, warmup):
    import torch.nn.functional as F
    h, w, c = 100, 152, 256
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.from_numpy(rng.randn(1, c, h, w).astype(np.float32)).to(DEV).to(dtype)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        for co, k in ((80, 1), (4, 1), (256, 3)):
            wt = (torch.from_numpy(rng.randn(co, c, k, k).astype(np.float32)) / (c * k * k) ** 0.5).to(DEV).to(dtype)
            b = torch.from_numpy(rng.randn(co).astype(np.float32)).to(DEV).to(dtype)
            for share in (0.05, 0.25, 1.0):
                mask = torch.from_numpy((rng.rand(1, h, w) < share).astype(np.float32)).to(DEV)
                mask_t = mask[:, None].to(dtype)
                fns = [lambda: ops.masked_conv2d(x, mask, wt, b, k // 2), lambda: ops.masked_conv2d(x_cl, mask, wt, b, k // 2),
                       lambda: F.conv2d(x, wt, b, padding=k // 2) * mask_t, lambda: ops.masked_conv2d_pytorch(x, mask, wt, b, k // 2)]
                dense, native = fns[2]().float(), fns[0]().float()
                t = timed_group(fns, reps, warmup)
                res["%s %d -> %d, %d x %d, %g %% active" % (str(dtype).split(".")[-1], c, co, k, k, 100 * share)] = {
                    "active pixels": int(mask.sum()), "max |ops - dense conv2d * mask|": float((native - dense).abs().max()),
                    "ops": round(t[0], 1), "ops channels_last": round(t[1], 1), "dense conv2d * mask": round(t[2], 1),
                    "_pytorch composition": round(t[3], 1), "dense / ops": round(t[2] / t[0], 2), "composition / ops": round(t[3] / t[0], 2)}
    return {"masked_conv2d, 1 x 256 x 100 x 152 (microseconds)": res}


def mask_leg(rng, reps, warmup):
    import torch.nn.functional as F
    k, m, h, w = 100, 28, 800, 1333
    cx, cy = rng.uniform(0, w, k), rng.uniform(0, h, k)
    bw, bh = rng.uniform(30, 400, k), rng.uniform(30, 400, k)
    boxes = torch.from_numpy(np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(np.float32)).to(DEV)
    masks = torch.from_numpy(rng.uniform(0, 1, (k, 1, m, m)).astype(np.float32)).to(DEV)

    def tv_loop(masks, boxes, pad=1):
        """torchvision's paste_masks_in_image restated: expand_masks / expand_boxes, then its loop"""
        scale = (m + 2 * pad) / m
        mk = F.pad(masks, (pad,) * 4)
        w_half, h_half = (boxes[:, 2] - boxes[:, 0]) * 0.5 * scale, (boxes[:, 3] - boxes[:, 1]) * 0.5 * scale
        x_c, y_c = (boxes[:, 2] + boxes[:, 0]) * 0.5, (boxes[:, 3] + boxes[:, 1]) * 0.5
        ib = torch.stack([x_c - w_half, y_c - h_half, x_c + w_half, y_c + h_half], 1).to(torch.int64)
        res = []
        for mask, box in zip(mk, ib):
            x0, y0, x1, y1 = (int(v) for v in box)                                     # four host reads
            bw_, bh_ = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
            mask = F.interpolate(mask.expand((1, 1, -1, -1)), size=(bh_, bw_), mode="bilinear", align_corners=False)[0][0]
            im = torch.zeros((h, w), dtype=mask.dtype, device=mask.device)
            xa, xb, ya, yb = max(x0, 0), min(x1 + 1, w), max(y0, 0), min(y1 + 1, h)
            im[ya:yb, xa:xb] = mask[(ya - y0):(yb - y0), (xa - x0):(xb - x0)]
            res.append(im)
        return torch.stack(res, 0)[:, None]

    def grid_sample_paste(masks, boxes, thr):
        """detectron2's _do_paste_mask (one chunk, no skip_empty) and its threshold"""
        x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
        ys = (torch.arange(0, h, device=DEV, dtype=torch.float32) + 0.5 - y0) / (y1 - y0) * 2 - 1
        xs = (torch.arange(0, w, device=DEV, dtype=torch.float32) + 0.5 - x0) / (x1 - x0) * 2 - 1
        grid = torch.stack([xs[:, None, :].expand(k, h, w), ys[:, :, None].expand(k, h, w)], dim=3)
        img = F.grid_sample(masks, grid, align_corners=False)[:, 0]
        return img >= thr if thr >= 0 else (img * 255).to(torch.uint8)

    res = {}

    def row(name, fns, labels, nbytes):
        t = timed_group(fns, reps, warmup)
        r = {lab: round(v, 1) for lab, v in zip(labels, t)}
        for lab, v in zip(labels[1:], t[1:]):
            r["%s / ops" % lab] = round(v / t[0], 1)
        r["bytes"] = nbytes
        r["ops TB/s"] = round(nbytes / t[0] / 1e6, 3)
        r["share of the 8 TB/s peak"] = round(nbytes / t[0] / 1e6 / 8.0, 3)
        res[name] = r

    half = masks.half()
    row("paste_masks_in_image float32, padding 1", [lambda: ops.paste_masks_in_image(masks, boxes, (h, w), 1),
        lambda: ops.paste_masks_in_image_pytorch(masks, boxes, (h, w), 1), lambda: tv_loop(masks, boxes)],
        ["ops", "_pytorch twin", "torchvision's loop"], k * h * w * 4)
    row("paste_masks_in_image float16, padding 1", [lambda: ops.paste_masks_in_image(half, boxes, (h, w), 1),
        lambda: ops.paste_masks_in_image_pytorch(half, boxes, (h, w), 1), lambda: tv_loop(half, boxes)],
        ["ops", "_pytorch twin", "torchvision's loop"], k * h * w * 2)
    for name, thr in (("bool, threshold 0.5", 0.5), ("uint8", -1.0)):
        row("paste_masks_aligned " + name, [lambda: ops.paste_masks_aligned(masks, boxes, (h, w), thr),
            lambda: ops.paste_masks_aligned_pytorch(masks, boxes, (h, w), thr), lambda: grid_sample_paste(masks, boxes, thr)],
            ["ops", "_pytorch twin", "grid_sample composition"], k * h * w)
    pasted = ops.paste_masks_aligned(masks, boxes, (h, w), 0.5)
    row("masks_to_boxes bool", [lambda: ops.masks_to_boxes(pasted), lambda: ops.masks_to_boxes_pytorch(pasted)], ["ops", "_pytorch twin"], k * h * w)
    pasted32 = pasted.float()
    row("masks_to_boxes float32", [lambda: ops.masks_to_boxes(pasted32), lambda: ops.masks_to_boxes_pytorch(pasted32)], ["ops", "_pytorch twin"],
        k * h * w * 4)
    a, b = ops.paste_masks_in_image(masks, boxes, (h, w), 1), tv_loop(masks, boxes)
    res["max |ops - torchvision's loop| (float32)"] = float((a - b).abs().max())
    res["pixels where ops.paste_masks_aligned(0.5) differs from the grid_sample composition"] = int((pasted != grid_sample_paste(masks, boxes, 0.5)).sum())
    return {"mask operators, K = 100, M = 28, 800 x 1333 (microseconds)": res}


def keypoint_leg(rng, reps, warmup):
    k, m, h, w = 17, 56, 800, 1333
    res = {}

    def row(name, boxes, dtype):
        r = len(boxes)
        maps = (torch.from_numpy(rng.standard_normal((r, k, m, m)).astype(np.float32)) * 3).to(DEV).to(dtype)
        rois = torch.from_numpy(boxes.astype(np.float32)).to(DEV)
        t = timed_group([lambda: ops.heatmaps_to_keypoints_scored(maps, rois), lambda: ops.heatmaps_to_keypoints_scored_pytorch(maps, rois)],
                        reps, warmup)
        size = (rois[:, 2:] - rois[:, :2]).clamp(min=1).ceil().double()
        pixels = int((size[:, 0] * size[:, 1]).sum()) * k
        a, b = ops.heatmaps_to_keypoints_scored(maps, rois), ops.heatmaps_to_keypoints_scored_pytorch(maps, rois)
        res[name] = {"ops": round(t[0], 1), "_pytorch twin (upstream's loop)": round(t[1], 1), "twin / ops": round(t[1] / t[0], 1),
                     "pixels of the resized images": pixels, "ops Gpixel/s": round(pixels / t[0] / 1e3, 2),
                     "pairs whose position differs from the twin's": int(((a[..., :2] != b[..., :2]).any(2)).sum()),
                     "max |logit - twin's|": float((a[..., 2] - b[..., 2]).abs().max())}

    r = 100
    cx, cy = rng.uniform(0, w, r), rng.uniform(0, h, r)
    bw, bh = rng.uniform(30, 400, r), rng.uniform(30, 400, r)
    detections = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    row("R = 100 detections, float32 maps", detections, torch.float32)
    row("R = 100 detections, float16 maps", detections, torch.float16)
    image_sized = np.array([[0, 0, w, h], [10.5, 20.25, w - 30, h - 7.5], [0, 0, w, h / 2], [w / 3, 0, w, h]])
    row("R = 4 image-sized boxes, float32 maps", image_sized, torch.float32)
    return {"heatmaps_to_keypoints, K = 17, 56 x 56 maps, 800 x 1333 (microseconds)": res}


def diffiou_leg(rng, reps, warmup):
    n = 1 << 20
    u = lambda lo, hi, *shape: torch.from_numpy(rng.uniform(lo, hi, (n,) + shape).astype(np.float32))     # noqa: E731
    b1 = torch.cat([u(0, 1000, 2), u(8, 30, 2), u(-np.pi, np.pi, 1)], 1)
    b2 = torch.cat([b1[:, :2] + u(-3, 3, 2), b1[:, 2:4] * u(0.8, 1.25, 2), b1[:, 4:] + u(-0.3, 0.3, 1)], 1)
    b1, b2, g = b1.to(DEV), b2.to(DEV), u(-1, 1).to(DEV)
    leaves = (b1.clone().requires_grad_(True), b2.clone().requires_grad_(True))
    y, yc = ops.diff_iou_rotated_2d(b1, b2), ops.diff_iou_rotated_2d_pytorch(b1, b2)
    r = {"max |diff_iou_rotated_2d - composition|": float((y - yc).abs().max()), "mean IoU": float(y.mean())}
    for name, fns in (("fwd", (lambda: ops.diff_iou_rotated_2d(b1, b2), lambda: ops.diff_iou_rotated_2d_pytorch(b1, b2))),
                      ("fwd+bwd (both boxes)", (lambda: ops.diff_iou_rotated_2d(*leaves).backward(g),
                                                lambda: ops.diff_iou_rotated_2d_pytorch(*leaves).backward(g)))):
        t_native, t_comp = timed_pair(fns[0], fns[1], reps, warmup)
        r[name] = {"ops.diff_iou_rotated_2d": round(t_native, 1), "ops.diff_iou_rotated_2d_pytorch": round(t_comp, 1),
                   "composition / diff_iou_rotated_2d": round(t_comp / t_native, 2)}
    return {"diffiou float32, %d aligned pairs" % n: r}


def softnms_leg(rng, reps, warmup):
    import time

    def clustered(n):
        k = max(1, n // 12)
        c = rng.randint(0, k, n)
        ctr = rng.uniform(70, 530, (k, 2))[c] + rng.uniform(-5, 5, (n, 2))
        sd = rng.uniform(30, 120, (k, 2))[c] * rng.uniform(0.85, 1.15, (n, 2))
        return (torch.from_numpy(np.concatenate([ctr - sd / 2, ctr + sd / 2], 1).astype(np.float32)),
                torch.from_numpy(rng.uniform(0.02, 1.0, n).astype(np.float32)))

    def wall(fn, calls, windows):
        ts = []
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / calls)
        return float(np.median(ts))

    res = {}
    for name, n, n_labels in (("1000 boxes, one problem", 1000, 0), ("4000 boxes, one problem", 4000, 0),
                              ("80 labels x 250 boxes", 20000, 80)):
        if n_labels:                                                           # every label its own clustered 250 boxes, then shuffled
            parts = [clustered(n // n_labels) for _ in range(n_labels)]
            perm = torch.from_numpy(rng.permutation(n))
            boxes, scores = torch.cat([p[0] for p in parts])[perm], torch.cat([p[1] for p in parts])[perm]
            labels = torch.arange(n_labels).repeat_interleave(n // n_labels)[perm]
        else:
            boxes, scores = clustered(n)
            labels = None
        b, s, lab = boxes.to(DEV), scores.to(DEV), labels.to(DEV) if n_labels else None
        for method in ("linear", "gaussian"):
            args = (0.3, 0.5, 0.05, method, 0)

            def on_cpu():
                dets, inds = ops.soft_nms_pytorch(b.cpu(), s.cpu(), *args, lab.cpu() if n_labels else None)
                return dets.to(DEV), inds.to(DEV)

            native = lambda: ops.soft_nms(b, s, *args, lab)                    # noqa: E731
            for _ in range(warmup):
                native()
            kept = int(native()[1].numel())
            same = bool(torch.equal(native()[1], ops.soft_nms_pytorch(b, s, *args, lab)[1]))
            t_native = wall(native, reps, 5)
            t_gpu = wall(lambda: ops.soft_nms_pytorch(b, s, *args, lab), 1, 3)
            t_cpu = wall(on_cpu, 1, 3)
            res["softnms %s, %s" % (name, method)] = {
                "kept": kept, "inds equal the fallback's": same, "ops.soft_nms ms": round(t_native, 3),
                "ops.soft_nms_pytorch (same GPU tensors) ms": round(t_gpu, 1), "copies + ops.soft_nms_pytorch on the CPU ms": round(t_cpu, 1),
                "GPU fallback / soft_nms": round(t_gpu / t_native, 1), "CPU route / soft_nms": round(t_cpu / t_native, 1)}
    return res


def proposals(rng, k, H, W):
    y1 = rng.uniform(0, H - 64, k); x1 = rng.uniform(0, W - 64, k)
    return np.stack([y1, x1, np.minimum(y1 + rng.uniform(32, 400, k), H), np.minimum(x1 + rng.uniform(32, 600, k), W)], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["multiscale", "half", "ps", "deform", "droi", "rot", "carafe", "msda", "prroi", "dcnv3", "dcnv4", "diffiou", "softnms", "border", "riroi", "rfa", "convex", "quadri", "mconv", "mask", "keypoint"], default=None)
    a = ap.parse_args()
    nv.require_gpu()
    lib = nv.lib()
    S = nv.stream_ptr
    rng = np.random.RandomState(0)
    res = {}
    if a.only == "multiscale":
        print(json.dumps(multiscale_leg(rng, 10, 3), indent=1))
        return
    if a.only == "half":
        print(json.dumps(half_leg(rng, 10, 3), indent=1))
        return
    if a.only == "ps":
        print(json.dumps(ps_leg(rng, 10, 3), indent=1))
        return
    if a.only == "deform":
        print(json.dumps(deform_leg(rng, 5, 2), indent=1))
        return
    if a.only == "droi":
        print(json.dumps(droi_leg(rng, 5, 2), indent=1))
        return
    if a.only == "rot":
        print(json.dumps(rot_leg(rng, 5, 2), indent=1))
        return
    if a.only == "carafe":
        print(json.dumps(carafe_leg(rng, 5, 2), indent=1))
        return
    if a.only == "msda":
        print(json.dumps(msda_leg(rng, 5, 2), indent=1))
        return
    if a.only == "prroi":
        print(json.dumps(prroi_leg(rng, 5, 2), indent=1))
        return
    if a.only == "dcnv3":
        print(json.dumps(dcnv3_leg(rng, 5, 2), indent=1))
        return
    if a.only == "diffiou":
        print(json.dumps(diffiou_leg(rng, 5, 2), indent=1))
        return
    if a.only == "softnms":
        print(json.dumps(softnms_leg(rng, 20, 3), indent=1))
        return
    if a.only == "dcnv4":
        print(json.dumps(dcnv4_leg(rng, 5, 2), indent=1))
        return
    if a.only == "border":
        print(json.dumps(border_leg(rng, 5, 2), indent=1))
        return
    if a.only == "riroi":
        print(json.dumps(riroi_leg(rng, 5, 2), indent=1))
        return
    if a.only == "rfa":
        print(json.dumps(rfa_leg(rng, 5, 2), indent=1))
        return
    if a.only == "convex":
        print(json.dumps(convex_leg(rng, 5, 2), indent=1))
        return
    if a.only == "quadri":
        print(json.dumps(quadri_leg(rng, 5, 2), indent=1))
        return
    if a.only == "mconv":
        print(json.dumps(mconv_leg(rng, 50, 5), indent=1))
        return
    if a.only == "mask":
        print(json.dumps(mask_leg(rng, 10, 2), indent=1))
        return
    if a.only == "keypoint":
        print(json.dumps(keypoint_leg(rng, 5, 2), indent=1))
        return
    c, fh, fw = 512, 37, 62
    x = torch.relu(torch.randn((1, c, fh, fw), device=DEV))
    x_cl = x.contiguous(memory_format=torch.channels_last)
    fm_hwc = x[0].permute(1, 2, 0).contiguous()
    for k in (128, 300):
        props = torch.from_numpy(proposals(rng, k, 600, 1000)).to(DEV)              # (y1, x1, y2, x2)
        rois = torch.cat([torch.zeros((k, 1), device=DEV), props[:, [1, 0, 3, 2]]], 1)
        cnt = torch.tensor([k], dtype=torch.int32, device=DEV)
        out = torch.empty((k, 7, 7, c), device=DEV)
        g = torch.randn((k, c, 7, 7), device=DEV)
        g_hwc = g.permute(0, 2, 3, 1).contiguous()
        dfm = torch.empty((fh, fw, c), device=DEV)
        wsb = int(lib.frcnn_roi_pool_backward_workspace_bytes(k, 7, c))
        ws = torch.empty((wsb // 4,), device=DEV)
        r = {}
        r["ops.roi_pool nchw"] = timed(lambda: ops.roi_pool(x, rois, 7, 1 / 16), a.reps, a.warmup)
        r["ops.roi_pool channels_last"] = timed(lambda: ops.roi_pool(x_cl, rois, 7, 1 / 16), a.reps, a.warmup)
        r["frcnn_roi_pool"] = timed(lambda: lib.frcnn_roi_pool(nv.ptr(fm_hwc), fh, fw, c, nv.ptr(props), nv.ptr(cnt), k, 7, 1 / 16,
                                                               nv.ptr(out), S()), a.reps, a.warmup)
        r["ops.roi_align nchw"] = timed(lambda: ops.roi_align(x, rois, 7, 1 / 16, 2), a.reps, a.warmup)
        r["ops.roi_align channels_last"] = timed(lambda: ops.roi_align(x_cl, rois, 7, 1 / 16, 2), a.reps, a.warmup)
        r["frcnn_roi_align"] = timed(lambda: lib.frcnn_roi_align(nv.ptr(fm_hwc), fh, fw, c, nv.ptr(props), nv.ptr(cnt), k, 7, 1 / 16, 2,
                                                                 0, nv.ptr(out), S()), a.reps, a.warmup)
        xg = x_cl.clone().requires_grad_(True)

        def pool_fb():
            ops.roi_pool(xg, rois, 7, 1 / 16).backward(g)

        def align_fb():
            ops.roi_align(xg, rois, 7, 1 / 16, 2).backward(g)
        r["ops.roi_pool fwd+bwd channels_last"] = timed(pool_fb, a.reps, a.warmup)
        r["frcnn_roi_pool_backward (argmax + gather)"] = timed(
            lambda: lib.frcnn_roi_pool_backward(nv.ptr(fm_hwc), fh, fw, c, nv.ptr(props), k, 7, 1 / 16, nv.ptr(g_hwc), nv.ptr(dfm), 0,
                                                nv.ptr(ws), wsb, S()), a.reps, a.warmup)
        r["ops.roi_align fwd+bwd channels_last"] = timed(align_fb, a.reps, a.warmup)
        r["frcnn_roi_align_backward"] = timed(
            lambda: lib.frcnn_roi_align_backward(nv.ptr(props), k, fh, fw, c, 7, 1 / 16, 2, 0, nv.ptr(g_hwc), nv.ptr(dfm), 0, S()),
            a.reps, a.warmup)
        res["vgg16 map, %d RoIs" % k] = r
    # FPN-like
    n, c, h, w, k = 2, 256, 200, 336, 1000
    xf = torch.randn((n, c, h, w), device=DEV).contiguous(memory_format=torch.channels_last)
    bx = proposals(rng, k, h * 4, w * 4)
    rois = torch.from_numpy(np.concatenate([rng.randint(0, n, (k, 1)).astype(np.float32), bx[:, [1, 0, 3, 2]]], 1)).to(DEV)
    gf = torch.randn((k, c, 7, 7), device=DEV)
    xfg = xf.clone().requires_grad_(True)
    res["fpn-like 2x256x200x336, 1000 RoIs, sr 2"] = {
        "ops.roi_align fwd": timed(lambda: ops.roi_align(xf, rois, 7, 0.25, 2), 10, 3),
        "ops.roi_align fwd+bwd": timed(lambda: ops.roi_align(xfg, rois, 7, 0.25, 2).backward(gf), 10, 3),
    }
    # nms
    r = {}
    for dt, nb in ((torch.float32, 12000), (torch.float64, 2000)):
        b = proposals(rng, nb, 600, 1000)
        boxes = torch.from_numpy(b[:, [1, 0, 3, 2]]).to(DEV).to(dt)
        scores = torch.rand((nb,), device=DEV, dtype=dt)
        r["nms %d %s (0.7), %d kept" % (nb, str(dt).split(".")[-1], len(ops.nms(boxes, scores, 0.7)))] = timed(
            lambda: ops.nms(boxes, scores, 0.7), 20, 3)
    res["nms"] = r
    res.update(multiscale_leg(rng, 10, 3))
    res.update(half_leg(rng, 10, 3))
    res.update(ps_leg(rng, 10, 3))
    res.update(deform_leg(rng, 5, 2))
    res.update(droi_leg(rng, 5, 2))
    res.update(rot_leg(rng, 5, 2))
    res.update(carafe_leg(rng, 5, 2))
    res.update(msda_leg(rng, 5, 2))
    res.update(prroi_leg(rng, 5, 2))
    res.update(dcnv3_leg(rng, 5, 2))
    res.update(dcnv4_leg(rng, 5, 2))
    res.update(border_leg(rng, 5, 2))
    res.update(riroi_leg(rng, 5, 2))
    res.update(rfa_leg(rng, 5, 2))
    res.update(convex_leg(rng, 5, 2))
    res.update(quadri_leg(rng, 5, 2))
    res.update(mconv_leg(rng, 50, 5))
    res.update(mask_leg(rng, 10, 2))
    res.update(keypoint_leg(rng, 5, 2))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
