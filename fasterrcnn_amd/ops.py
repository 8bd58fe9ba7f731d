"""
torchvision.ops-style operators on the project's HIP kernels (csrc/ops.hip), as torch custom ops with autograd.

    from fasterrcnn_amd.ops import nms, batched_nms, roi_pool, roi_align, RoIPool, RoIAlign, multi_scale_roi_align, MultiScaleRoIAlign
    from fasterrcnn_amd.ops import ps_roi_pool, ps_roi_align, PSRoIPool, PSRoIAlign
    from fasterrcnn_amd.ops import deform_conv2d, DeformConv2d
    from fasterrcnn_amd.ops import deform_roi_pool, DeformRoIPool, DeformRoIPoolPack, ModulatedDeformRoIPoolPack
    from fasterrcnn_amd.ops import box_iou_rotated, nms_rotated, roi_align_rotated, RoIAlignRotated
    from fasterrcnn_amd.ops import diff_iou_rotated_2d, diff_iou_rotated_3d, diff_iou_rotated_2d_pytorch
    from fasterrcnn_amd.ops import soft_nms, soft_nms_pytorch
    from fasterrcnn_amd.ops import carafe, CARAFE, CARAFEPack
    from fasterrcnn_amd.ops import multi_scale_deformable_attn, MultiScaleDeformableAttnFunction, MultiScaleDeformableAttention
    from fasterrcnn_amd.ops import prroi_pool, PrRoIPool, prroi_pool_pytorch
    from fasterrcnn_amd.ops import dcnv3, DCNv3Function, dcnv3_core_pytorch, DCNv3
    from fasterrcnn_amd.ops import dcnv4, DCNv4Function, dcnv4_core_pytorch, DCNv4
    from fasterrcnn_amd.ops import border_align, BorderAlign, border_align_pytorch
    from fasterrcnn_amd.ops import riroi_align_rotated, RiRoIAlignRotated, riroi_align_rotated_pytorch
    from fasterrcnn_amd.ops import rotated_feature_align, RotatedFeatureAlign, rotated_feature_align_pytorch
    from fasterrcnn_amd.ops import convex_iou, convex_giou, min_area_polygons
    from fasterrcnn_amd.ops import convex_iou_pytorch, convex_giou_pytorch, min_area_polygons_pytorch
    from fasterrcnn_amd.ops import box_iou_quadri, nms_quadri, points_in_polygons, box_iou_quadri_pytorch, points_in_polygons_pytorch
    from fasterrcnn_amd.ops import masked_conv2d, MaskedConv2d, masked_conv2d_pytorch
    from fasterrcnn_amd.ops import paste_masks_in_image, paste_masks_aligned, masks_to_boxes
    from fasterrcnn_amd.ops import paste_masks_in_image_pytorch, paste_masks_aligned_pytorch, masks_to_boxes_pytorch
    from fasterrcnn_amd.ops import heatmaps_to_keypoints, heatmaps_to_keypoints_scored, keypointrcnn_inference, keypoints_to_heatmap
    from fasterrcnn_amd.ops import heatmaps_to_keypoints_pytorch, heatmaps_to_keypoints_scored_pytorch

Signatures and semantics are torchvision's (oracle/frcnn_oracle.py restates them):
  nms(boxes, scores, iou_threshold) -> int64[K]     boxes (x1, y1, x2, y2) float32 or float64; visited in a stable descending sort of
                                                     the scores; box j goes iff inter / union > float32(iou_threshold), computed in the
                                                     boxes' dtype.  Any n (up to 524288: the n x n / 64 bit mask), no cap on K.
  batched_nms(boxes, scores, idxs, iou_threshold)   NMS within each category, one pass over all of them; kept indices by descending
                                                     score, ties by ascending index (torchvision's per-category loop, no coordinate offset).
  roi_pool(input, boxes, output_size, spatial_scale=1.0)
  roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False)
      input float32, float16 or bfloat16 [N, C, H, W]; boxes float32 Tensor[K, 5] (batch index, x1, y1, x2, y2) or list[Tensor[L_i, 4]];
      output_size int or (oh, ow), each <= 64; sampling_ratio <= 16.  The result is [K, C, oh, ow] in the input's dtype and channels_last
      memory ([K, oh, ow, C]).  A batch
      index outside [0, N) pools to zeros and receives no gradient.  Backward passes are deterministic gathers (no atomics):
      RoIPool sends each bin's gradient to its first maximum in scan order, an empty bin sends none.  Double backward raises.
  MultiScaleRoIAlign(featmap_names, output_size, sampling_ratio, *, canonical_scale=224, canonical_level=4)(x, boxes, image_shapes)
  multi_scale_roi_align(features, boxes, output_size, spatial_scales, sampling_ratio=-1, canonical_scale=224, canonical_level=4)
      torchvision's FPN pooler (ops/poolers.py): 1 to 8 maps of the same N, C and dtype; each RoI's level by LevelMapper in float32 as
      torch computes it on the GPU, then roi_align(aligned=False) on that level, bit-identical to the per-level torch.where loop (forward
      and backward) in one launch each way and without a host sync.  A RoI without a level (negative or NaN area) pools to zeros.
  ps_roi_pool(input, boxes, output_size, spatial_scale=1.0)
  ps_roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1)
      R-FCN's position-sensitive pooling (csrc/ops_ps.hip; torchvision's ps_roi_pool_kernel.cu / ps_roi_align_kernel.cu restated,
      unpinned): inputs and limits as roi_pool / roi_align, C a multiple of oh * ow (else ValueError).  The result is
      [K, C / (oh * ow), oh, ow] in the input's dtype, contiguous NCHW (torchvision's layout: the usual consumer is a mean over (oh, ow));
      output channel c of bin (ph, pw) pools input channel (c * oh + ph) * ow + pw.  ps_roi_pool: start = roundf(coord * scale),
      end = roundf((coord + 1) * scale), window bounds clamped to [0, size - 1], the window's mean, 0 for an empty window.
      ps_roi_align: always aligned (coord * scale - 0.5), count = grid_h * grid_w without a lower bound, so an adaptive grid on a RoI
      of no height or width gives 0.0 / count (NaN when count is 0), as torchvision does; such a RoI receives no gradient.  A
      contiguous NCHW input is read as it is (every output element owns one plane of it: there is no layout copy); a channels_last
      input is made contiguous by one copy.  Backward: deterministic gathers, input gradients in the input's memory format.
  deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None)
  DeformConv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True).forward(input, offset, mask=None)
      Deformable convolution v1, and v2 when a mask is given (csrc/ops_deform.hip; torchvision's ops/deform_conv.py and
      deform_conv2d_kernel.cu restated, unpinned).  input [N, C_in, H, W]; weight [C_out, C_in / groups, kh, kw], groups =
      C_in // weight.shape[1]; offset [N, 2 G kh kw, oh, ow], G = offset.shape[1] // (2 kh kw) offset groups; mask [N, G kh kw, oh, ow]
      or None (a mask of ones); bias [C_out] or None; stride, padding, dilation an int or a pair;
      oh = (H + 2 pad_h - (dil_h (kh - 1) + 1)) // stride_h + 1, likewise ow.  Channel 2 (g kh kw + i kw + j) of offset is the y
      displacement of tap (i, j) of offset group g, the next channel its x displacement; channel g kh kw + i kw + j of mask is the
      tap's modulation; input channel c belongs to offset group c // (C_in / G) and to weight group c // (C_in / groups).  Tap (i, j)
      at output (oy, ox) samples y = oy stride_h - pad_h + i dil_h + off_y, x = ox stride_w - pad_w + j dil_w + off_x: 0 when
      y <= -1 or y >= H or x <= -1 or x >= W (a NaN coordinate too), else the bilinear value on floor / floor + 1 with the weights
      hh hw, hh lw, lh hw, lh lw, a corner outside [0, H - 1] x [0, W - 1] counting 0.  The column value is mask * sample and
      out[n, co, oy, ox] = bias[co] + the sum over (c in co's weight group, i, j) of weight[co, c', i, j] * column.
      Gradients for input, offset, mask, weight and bias are torchvision's: the offset gradient uses get_coordinate_weight (the
      difference of the validly indexed corner values weighted by the other axis's fractions: the right-hand slope at an integer
      coordinate, without an early-out, so at exactly y == -1 the corner row 0 still counts while the forward sample is 0); d_mask is
      the sum over c of dcol * sample; d_bias is grad.sum((0, 2, 3)).  The backward is deterministic and free of atomics -- the input
      gradient sums, per cell, the sorted plan of the samples that reach it -- so two runs agree bit for bit, which torchvision's own
      GPU backward does not promise; it skips the work of every argument that needs no gradient.  Double backward raises.
      All tensors are float32, or all float16, or all bfloat16 (below); any other mix, and float64, is the TypeError that names the
      first tensor that is not float32 (pass .float()).  Tensors live on the GPU or on `meta`.  Contiguous NCHW is the native layout, a channels_last argument is made contiguous by
      one copy, gradients come back in each argument's own memory format, the result is contiguous NCHW.  The float32 products run on the
      exact-float32 MFMA kernel of csrc/gemm_tn.hip over chunks of DEFORM_CHUNK_IMAGES images (the bound of the column workspace);
      the forward, d_input, d_offset and d_mask do not depend on the chunking, d_weight sums the chunks in ascending order.  N == 0
      or C_out == 0 return empty tensors (zero gradients).  The 32-bit indices of the kernels bound the sizes (MAX_DEFORM_INDEX).
      float16 / bfloat16 (T; the frcnn_ops_deform_*_16 kernels, csrc/gemm_nt16.hip).  Columns: input, offset and mask are widened to
      float32 on read; the sample coordinate, the bilinear value and mask * sample are computed in float32 by the device functions of
      the float32 kernels (csrc/ops_deform.h); the column value is rounded ONCE to T, to nearest even -- bit for bit the float32
      operator's column of the widened tensors, rounded.  Forward: the products of two T values are exact in float32 and are summed in
      float32 accumulators on v_mfma_f32_32x32x16_{f16,bf16}, both operands 16-bit in memory, without a split reduction, so an output
      does not depend on the chunking; out = round_T(acc + float(bias)) is the one rounding; a float16 result beyond 65504 is inf, as
      for any half convolution.  Backward: dcol = W^T dout on the same kernel, no split, kept in float32; d_offset, d_mask and d_input
      are the float32 gathers (T input, offset and mask, float32 dcol, the same order of summation, d_input through the same plan,
      stable sort and ascending sum), rounded once to T on the store; d_weight samples the columns again to T (the forward's values),
      multiplies on the same kernel with a deterministic split reduction, adds the chunks of DEFORM_CHUNK_IMAGES images in ascending
      order in a FLOAT32 buffer and rounds it to T once after the last chunk (never in T); d_bias =
      grad.sum((0, 2, 3), dtype=float32).to(T).  Deterministic, no atomics; the forward, d_input, d_offset and d_mask do not depend
      on the chunking.  The result and the gradients have dtype T.  DeformConv2d.forward follows mmcv's AMP rule: when input is 16-bit,
      offset, mask, weight and bias are cast to input.dtype by differentiable .to calls, so float32 parameters receive float32
      gradients; a float32 input casts nothing.
  deform_roi_pool(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1)
  DeformRoIPool(output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1).forward(input, rois, offset=None)
  DeformRoIPoolPack / ModulatedDeformRoIPoolPack(output_size, output_channels, deform_fc_channels=1024, spatial_scale=1.0,
                                                 sampling_ratio=0, gamma=0.1).forward(input, rois)
      Deformable RoI pooling of DCN v1 / v2 (csrc/ops_droi.hip; mmcv's deform_roi_pool restated, unpinned: where the two differ
      include/frcnn_hip.h holds).  Inputs, limits, dtypes and layouts as roi_align; offset [K, 2, oh, ow] in float32 or the map's
      dtype, channel 0 the x (width) offset, channel 1 the y offset; None or an empty tensor: no offset.  Bin (ph, pw) of RoI k is
      roi_align(aligned=True)'s bin with its window shifted by gamma * roi_w * offset[k, 0, ph, pw] along x and gamma * roi_h *
      offset[k, 1, ph, pw] along y; a sample outside [-1, size] or at a NaN / infinite coordinate contributes nothing.  With no offset
      or an all-zero one the result is roi_align(input, rois, output_size, spatial_scale, sampling_ratio, aligned=True) bit for bit
      (sampling_ratio 0 is adaptive, as roi_align's -1).  Gradients for input and offset (the published offset formula: the sample
      coordinate before the bilinear clamp); both are deterministic and free of atomics, each is skipped when its argument needs none;
      RoIs get no gradient; double backward raises.  16-bit maps under the contract below for the output and d_input; the kernels read
      the offset and write its gradient in float32, and the gradient is rounded once to the offset's dtype.  The Pack modules own
      mmcv's offset_fc (and mask_fc) stacks with zero-initialised last layers, so mmcv / mmdetection checkpoints load strict.
  box_iou_rotated(boxes1, boxes2, mode="iou", aligned=False, clockwise=True) -> float32 [N, M], or [N] when aligned (N == M)
  nms_rotated(boxes, scores, iou_threshold, labels=None, clockwise=True) -> (dets [K, 6], keep int64 [K])
  roi_align_rotated(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True, clockwise=False)
  RoIAlignRotated(output_size, spatial_scale, sampling_ratio=0, aligned=True, clockwise=False).forward(input, rois)
      Rotated boxes for oriented detection (csrc/ops_rot.hip; mmcv's box_iou_rotated, nms_rotated and roi_align_rotated restated,
      unpinned: where the two differ include/frcnn_hip.h holds).  A box is float32 (cx, cy, w, h, angle), angle in radians.  With
      clockwise=True a local point (u, v) of the box, |u| <= w / 2, |v| <= h / 2, lies at the image point (cx + u cos a - v sin a,
      cy + u sin a + v cos a); clockwise=False means the same with a replaced by -a (the wrapper negates the column: the kernels know
      one convention).  IoU: inter is the area of the intersection of the two rectangles; mode "iou": inter / (w1 h1 + w2 h2 - inter),
      mode "iof": inter / (w1 h1).  A pair gives exactly 0 if either box has w h < 1e-14, a negative w or h, or a non-finite component;
      a box against itself gives exactly 1.  Empty inputs give empty outputs; there is no autograd (mmcv's has none).
      nms_rotated: boxes are visited in a stable descending sort of the scores, NaN scores last; sorted box j goes iff a kept box i
      before it, with the same label when labels are given, has iou(i, j) > float32(iou_threshold) -- box_iou_rotated's value, in that
      argument order.  keep is ordered by descending score, ties by ascending index, as in batched_nms; dets =
      cat(boxes[keep], scores[keep, None]).  N <= MAX_NMS_BOXES.  Boxes and scores are float32 only (float64 is a TypeError).
      roi_align_rotated: rois float32 [K, 6] rows (batch index, cx, cy, w, h, angle).  off = 0.5 if aligned else 0; centre =
      (cx, cy) * scale - off; rw = w * scale, rh = h * scale, each raised to >= 1 only when not aligned; bins rh / oh x rw / ow; grid =
      sampling_ratio if sampling_ratio > 0 else ceil(rh / oh) (likewise w); count = max(grid_h * grid_w, 1); t = -angle if clockwise
      else angle.  Sample (ph, iy, pw, ix) has local yy = -rh / 2 + ph * bin_h + (iy + .5) * bin_h / grid_h, xx likewise, and lies at
      x = yy sin t + xx cos t + centre_x, y = yy cos t - xx sin t + centre_y, so clockwise=True agrees with the box convention above.
      The value is roi_align's bilinear rule (nothing outside [-1, size] or at a NaN coordinate), the output the mean over count.
      Limits, layouts ([K, C, oh, ow] channels_last), channel padding and the batch-index rule are roi_align's; 16-bit maps run under
      the contract below, forward and backward, with RoIs in float32.  The gradient goes to input only; it is a deterministic gather
      without atomics (RoIs ascending, ROI_ALIGN_ROTATED_CULL_LIST per pass, then bins in (ph, pw) order).  Double backward raises.
  diff_iou_rotated_2d(box1, box2) -> float32 [B, N] or [N]
  diff_iou_rotated_3d(box3d1, box3d2) -> float32 [B, N] or [N]
  diff_iou_rotated_2d_pytorch(box1, box2)
      The differentiable IoU of aligned pairs of rotated boxes, what mmrotate's RotatedIoULoss and mmdet3d's 3-D IoU losses are built on
      (csrc/ops_rot.hip; mmcv's diff_iou_rotated_2d / _3d, signatures kept).  box1 and box2 are float32, of one shape [B, N, 5] or
      [N, 5], rows (cx, cy, w, h, angle in radians); there is no clockwise flag: the IoU of a pair does not depend on the convention as
      long as both boxes use one.  The value is box_iou_rotated(box1.view(-1, 5), box2.view(-1, 5), aligned=True) bit for bit -- the
      same device function -- so the zero rule holds (exactly 0 for a non-finite component, a negative side or w h < 1e-14) and
      identical boxes give exactly 1.  This is where it differs from mmcv, which intersects the edges pairwise into 24 candidate points,
      sorts them around their mean and takes the hull's area, with epsilons, in dozens of small launches differentiated by autograd:
      here the forward is one launch and the whole backward is one launch with the closed-form gradient of the clipped polygon
      (include/frcnn_hip.h states it: the length of the polygon's edges on each boundary line, chained to the ten box parameters).
      Where edges of the two boxes coincide the IoU has a kink, and the gradient is the one-sided value of the polygon the clip
      produced (a vertex on a line counts as inside: identical boxes get the gradient of box1 inside box2).  A pair under the zero
      rule, or one that does not overlap, gets exact zeros in all ten slots, whatever NaNs it holds.  Deterministic, no atomics; each
      gradient is skipped when its argument needs none; double backward raises.  3d: rows (x, y, z, w, h, l, alpha), [B, N, 7] or
      [N, 7], mmcv's definition: inter2d of the columns (0, 1, 3, 4, 6), z_overlap = clamp_min(min(z1 + l1 / 2, z2 + l2 / 2) -
      max(z1 - l1 / 2, z2 - l2 / 2), 0), inter3d = inter2d z_overlap, vol = w h l, inter3d / (vol1 + vol2 - inter3d); inter2d and
      its gradient come from the kernels, the rest is torch's.  float64 or 16-bit boxes are a TypeError (pass .float()), differing
      shapes or devices, CPU tensors and more than MAX_ROTATED_IOU_ROWS pairs a ValueError; no pairs give empty results and zero
      gradients without a launch.  diff_iou_rotated_2d_pytorch is the same clip from torch operations (8 vertex slots per pair, four
      passes, the fan area), differentiable by autograd, on any device and in float64 too: the fallback, with finite gradients for
      every input (each division sees a safe denominator before torch.where selects).
  soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method="linear", offset=0, labels=None)
      -> (dets [K, 5] float32, inds int64 [K])
  soft_nms_pytorch(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method="linear", offset=0, labels=None)
      Soft-NMS (Bodla et al., 2017), what mmdetection reaches with nms=dict(type='soft_nms', ...) (csrc/ops_softnms.hip; mmcv's soft_nms,
      which runs on the CPU only, restated, unpinned: where the two differ include/frcnn_hip.h holds; the signature is mmcv's plus
      `labels`, as nms_rotated has it).  boxes float32 [N, 4] rows (x1, y1, x2, y2); scores float32 [N]; method "naive", "linear" or
      "gaussian"; offset 0 or 1; sigma > 0; labels None or an integer tensor [N] of any int64 values.  The contract: all arithmetic is
      float32, every operation rounded on its own, the division IEEE; iou_threshold (thr), sigma and min_score are first rounded to
      float32; min / max ignore a NaN operand (fmin / fmax).  Each label is an independent problem (no labels: one problem).  Every box
      has a working score s_j = scores[j]; the live set starts as all of the problem's boxes; while it is not empty: (1) pick the live
      box i with the largest s, ties to the smaller index, NaN scores after every number and in index order (as nms orders its
      visits); i leaves the live set and is kept with its current s_i whatever that is -- the first pick of a problem is kept even
      below min_score; (2) for every live j: area = (x2 - x1 + offset) * (y2 - y1 + offset), w = max(0, min(x2_i, x2_j) -
      max(x1_i, x1_j) + offset), h likewise, inter = w * h, ovr = inter / ((area_i + area_j) - inter), a NaN ovr (0 / 0) counting as 0;
      (3) weight = naive: 0 if ovr >= thr else 1; linear: 1 - ovr if ovr >= thr else 1; gaussian: expf(-(ovr * ovr) / sigma);
      (4) s_j = s_j * weight, and j is dropped from the live set if s_j < min_score (a NaN s_j never is).  inds: the kept boxes of all
      problems by descending final score, ties by ascending index, NaN last, as batched_nms merges -- within one problem of
      non-negative scores that is exactly the pick order (the header proves it), so the kernel emits no rank; dets =
      cat(boxes[inds], final_scores[inds, None]).  No autograd (mmcv has none): the results are detached.  It differs from upstream in
      three places: the tie rule (mmcv's depends on its in-place swaps), a NaN ovr (0 here), and labels -- mmdetection's
      coordinate-offset trick lets a pick of one class drop a box of another class that is already below min_score, here a box is only
      ever touched by picks of its own label.  One launch: one workgroup owns one problem from its first pick to its last (the picks
      are a dependent chain), labels run side by side; the state of a problem lives in LDS up to 4096 boxes, in registers up to 64.
      N == 0 gives ([0, 5], [0]) without a launch; N <= MAX_SOFT_NMS_BOXES = 65536, else a ValueError naming N (one label may hold every
      box; one workgroup then runs N dependent picks).  float64 or 16-bit boxes or scores and non-integer labels are a TypeError (pass
      .float(), or use soft_nms_pytorch); wrong shapes, an unknown method, an offset outside {0, 1}, sigma <= 0 or not finite, a NaN
      iou_threshold or min_score, differing devices and CPU tensors a ValueError.  soft_nms_pytorch is the same contract from torch
      operations, one vectorised rescoring per pick, on any device, in float32 and in float64 (the boxes' dtype): the fallback, and the
      CPU reference users can read.
  carafe(features, masks, kernel_size, group_size, scale_factor) -> Tensor [N, C, s H, s W]
  CARAFE(kernel_size, group_size, scale_factor).forward(features, masks)
  CARAFEPack(channels, scale_factor, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1, compressed_channels=64).forward(x)
      CARAFE, content-aware reassembly of features: the learned upsampler of mmdetection's FPN_CARAFE necks (csrc/ops_carafe.hip; mmcv's
      carafe / CARAFE / CARAFEPack restated, unpinned: where the two differ include/frcnn_hip.h holds).  features [N, C, H, W]; masks
      [N, G k k, s H, s W]; k = kernel_size odd, 1 <= k <= MAX_CARAFE_KERNEL = 7 (a thread keeps the k k mask values of its pixel in
      registers); G = group_size >= 1 divides C; s = scale_factor in [1, MAX_CARAFE_SCALE = 8]; a violated limit is a ValueError that
      names the value.  With r = (k - 1) / 2 and g = c // (C / G),
          out[n, c, ph, pw] = sum over i, j in [0, k) of features[n, c, ph // s - r + i, pw // s - r + j] * masks[n, (g k + i) k + j, ph, pw]
      where a tap outside the map contributes nothing (zero padding).  Gradients go to both tensors: d_features[n, c, y, x] sums
      grad * mask over the k k s s output pixels whose window holds (y, x); d_masks[n, (g k + i) k + j, ph, pw] sums grad * feature over
      the C / G channels of group g and is exactly 0 for a tap outside the map.  Both are gathers, deterministic and free of atomics
      (two runs agree bit for bit); each is skipped when its argument needs none; double backward raises.  float32, and float16 /
      bfloat16 under the contract below, forward and both gradients (sums in float32, one rounding on store); features and masks share
      one dtype, else TypeError; float64 is a TypeError.  Contiguous NCHW is the native layout of features, masks and the result (what
      torch's convolutions, pixel_shuffle and softmax produce); a channels_last argument is made contiguous by one copy; gradients come
      back in each argument's own memory format.  N == 0 or C == 0 give empty tensors and zero gradients.  The kernels index a plane
      with 32 bits: s H s W <= MAX_CARAFE_PLANE, N <= 65535, G ceil(C / G / 4) <= 65535 (the launch grid), else ValueError.
      CARAFEPack owns mmcv's channel_compressor (1 x 1) and content_encoder convolutions under mmcv's names and init (Xavier-uniform,
      then normal(0, 0.001) on content_encoder, zero biases), so mmcv / mmdetection checkpoints load strict; its forward is
      content_encoder(channel_compressor(x)), pixel_shuffle(s), softmax over the k k taps of each group, then carafe: the convolutions,
      the shuffle and the softmax are torch's.
  multi_scale_deformable_attn(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                              im2col_step=64) -> Tensor [B, Q, M * D]
  MultiScaleDeformableAttnFunction.apply(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                                         im2col_step)
  multi_scale_deformable_attn_pytorch(value, value_spatial_shapes, sampling_locations, attention_weights)
  MultiScaleDeformableAttention(embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1, batch_first=False,
                                value_proj_ratio=1.0)
      Multi-scale deformable attention, the sampling core of Deformable DETR, DINO and Mask2Former (csrc/ops_msda.hip; mmcv's
      ms_deform_attn restated, unpinned: where the two differ include/frcnn_hip.h holds).  value [B, S, M, D]: S cells over all levels,
      M heads, D channels per head; value_spatial_shapes int64 [L, 2] rows (H_l, W_l); value_level_start_index int64 [L];
      sampling_locations [B, Q, M, L, P, 2], last axis (x, y) with [0, 1] spanning the level; attention_weights [B, Q, M, L, P].
      Sample (b, q, m, l, p) lies at x = fmaf(loc_x, W_l, -0.5), y = fmaf(loc_y, H_l, -0.5) in float32 (grid_sample's
      align_corners=False); it counts only if x > -1 and y > -1 and x < W_l and y < H_l (a NaN coordinate fails); its value is the bilinear
      mix of the corners floor / floor + 1, a corner outside the level counting 0; corner (yy, xx) is cell start_l + yy W_l + xx of
      value[b, :, m, :]; out[b, q, m D + d] = the sum over (l, p) of attention_weights * sample_d, in float32 in ascending (l, p).
      Gradients go to value, sampling_locations and attention_weights (the published ones: d_loc from the validly indexed corners, the
      right-hand slope at an integer coordinate, times W_l or H_l; d_weight = sum over d of grad * sample); all three are deterministic
      and free of atomics (d_value sums, per cell, the stably sorted plan of the corners that reach it, as deform_conv2d's input
      gradient does, a cell with more than MSDA_SEGMENT = 512 entries in pieces of 512 summed in order; the sums over D are fixed-order
      lane reductions), so two runs agree bit for bit; each is skipped when its argument
      needs none; double backward raises.  The shape tensors get no gradient, stay on the GPU and are read by the kernels: there is no
      host sync in the forward or the backward, and the kernels are memory-safe whatever the shape tensors hold (a corner whose cell
      falls outside [0, S) contributes nothing and receives nothing; a cell no level covers gets a zero gradient).  im2col_step bounds
      the images per launch and per plan, chunks of min(B, im2col_step) images; it need not divide B and no bit of any result depends
      on it.  float32, and float16 / bfloat16 value under the contract below (output and d_value); sampling_locations and
      attention_weights are float32 or the value's own 16-bit dtype (widened before the launch, their gradients rounded once to that
      dtype); anything else, float64 included, is a TypeError.  Limits, each a ValueError naming the value: L <= MAX_MSDA_LEVELS = 8,
      P <= MAX_MSDA_POINTS = 16, 1 <= D <= MAX_MSDA_CHANNELS = 256, and for a chunk of n images n S M <= MAX_MSDA_INDEX and
      n Q M L P 4 <= MAX_MSDA_INDEX (the kernels' 32-bit cell and plan-entry indices).  B, Q, S, M or D equal to 0 give empty or zero
      results and zero gradients without a launch.  multi_scale_deformable_attn_pytorch is mmcv's grid_sample composition, the fallback
      users know: any device, S must equal the sum of H_l W_l.  The module has mmcv's parameter names (sampling_offsets,
      attention_weights, value_proj, output_proj) and init (zero weights and the per-head directional grid bias scaled by point index
      on sampling_offsets, zeros on attention_weights, Xavier-uniform with zero bias on the projections), so mmdetection checkpoints load
      strict; forward(query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None, reference_points=None,
      spatial_shapes=None, level_start_index=None) serves reference points with 2 or 4 last-axis entries (else ValueError); the linear
      layers, the softmax over L P and the dropout are torch's; on the GPU the sampler is this operator, elsewhere the composition.
  prroi_pool(input, rois, output_size, spatial_scale=1.0) -> Tensor [K, C, oh, ow]
  PrRoIPool(output_size, spatial_scale=1.0).forward(input, rois)
  prroi_pool_pytorch(input, rois, output_size, spatial_scale=1.0)
      Precise RoI Pooling, the pooler of IoU-Net and of the ATOM / DiMP trackers, the one RoI pooler with a gradient for the boxes
      (csrc/ops_prroi.hip; mmcv's prroi_pool restated, unpinned: where the two differ include/frcnn_hip.h holds).  Inputs, limits, dtypes
      and layouts as roi_align.  The map is extended to the surface f(x, y) = sum of hat(y - j) hat(x - i) input[b, c, j, i], hat(t) =
      max(0, 1 - |t|): cell (j, i) at the integer point (i, j), no half-pixel shift, zero beyond one cell outside the map.  In float32,
      with s = spatial_scale: X1 = x1 s (likewise Y1, X2, Y2), bw = max(X2 - X1, 0) / ow, bh = max(Y2 - Y1, 0) / oh, A = bw bh; bin
      (ph, pw) spans xs = X1 + pw bw .. xe = xs + bw and ys = Y1 + ph bh .. ye = ys + bh, and out[k, c, ph, pw] is the exact integral of f
      over the bin divided by A = (sum of Wy(j) Wx(i) input[b, c, j, i]) / A with Wx(i) the integral of hat(x - i) over [xs, xe], formed
      on the two unit pieces either side of i (no difference of antiderivatives: a bin much narrower than a cell does not cancel).  There
      is no sampling grid.  A RoI is pooled iff 0 < A < +inf and its batch index lies in [0, N): a box of no or negative width or
      height, a NaN or infinite coordinate, or an area that overflows float32 pools to exact zeros and sends and receives no gradient;
      the kernels are memory-safe for any box.  Gradients go to input (roi_align's culled, ordered gather) and to rois: the analytic
      derivative d out / d xs = (-Lx(xs) + out bh) / A, d out / d xe = (Lx(xe) - out bh) / A with the line integral Lx(t) of f along
      x = t over [ys, ye] (likewise in y), chained to (x1, y1, x2, y2); column 0 of the RoI gradient is 0.  The operator is C1 in the box
      wherever A > 0: integer coordinates are no seams.  The box gradient is recomputed from the map, not from the saved output.  Both
      gradients are deterministic and free of atomics (two runs agree bit for bit), each is skipped when its argument needs none; a
      list of boxes gets its gradient in the list's tensors; double backward raises.  16-bit maps under the contract below for the
      output and d_input; the kernels compute the box gradient in float32 (bit for bit that of the widened map) and it is rounded once
      to the RoIs' dtype.  K == 0, N == 0 and C == 0 give empty or zero results without a launch.  prroi_pool_pytorch is the same
      operator from torch operations with autograd to input and rois, on any device and in float64 too: the weight matrices
      Wy [K, oh, H] and Wx [K, ow, W] in the clamped antiderivative form (C1, so autograd gives the analytic box gradient at integer
      coordinates too; it does cancel for very narrow bins) and two einsums per image, rows then columns.  It decides which RoIs are
      pooled in the dtype it computes in: a float64 map pools a box whose area overflows only float32, which the kernels do not.
  dcnv3(input, offset, mask, kernel_size, stride=1, padding=0, dilation=1, group=1, offset_scale=1.0, im2col_step=256)
  DCNv3Function.apply(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                      group_channels, offset_scale, im2col_step)
  dcnv3_core_pytorch(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                     group_channels, offset_scale)
  DCNv3(channels=64, kernel_size=3, dw_kernel_size=None, stride=1, pad=1, dilation=1, group=4, offset_scale=1.0)
      DCNv3, the deformable convolution v3 of the InternImage backbones (csrc/ops_dcnv3.hip; InternImage's DCNv3 restated, unpinned:
      where the two differ include/frcnn_hip.h holds): a grouped, weight-free deformable sampling on channels-last maps.  input
      [N, H, W, G Gc]; offset [N, Ho, Wo, G K 2], the pair of (g, p) at (g K + p) 2 as (dx, dy); mask [N, Ho, Wo, G K]; the result is
      [N, Ho, Wo, G Gc], contiguous, in the input's dtype.  K = kh kw, Ho = (H + 2 pad_h - (dil_h (kh - 1) + 1)) // stride_h + 1 (Wo
      likewise); kernel_size, stride, padding and dilation are ints or pairs (h, w); Gc = input.shape[-1] // group.  Point p = i kh + j has
      i in [0, kw) along x as the outer index and j in [0, kh) along y.  With bx = dil_w (kw - 1) // 2 and by = dil_h (kh - 1) // 2 the
      sample (n, oy, ox, g, p) lies at x = (ox stride_w - pad_w + bx) + ((i dil_w - bx) + dx) * offset_scale, y likewise, the integer parts
      in integers and the rest in float32, in pixels of the unpadded map; it counts only if x > -1 and y > -1 and x < W and y < H (a NaN
      coordinate fails); its value is the bilinear mix of the corners floor / floor + 1, a corner outside the map counting 0;
      out[n, oy, ox, g Gc + c] = the sum over p ascending of mask * sample_c in float32.  Gradients go to input, offset and mask (d_offset
      over the forward's accepted range and corners, the right-hand slope at an integer coordinate, times offset_scale; d_mask = sum over c
      of grad * sample); all three are deterministic and free of atomics (d_input sums, per cell and group, the stably sorted plan of the
      corners that reach it with multi_scale_deformable_attn's gather, every cell written), so two runs agree bit for bit; each is
      skipped when its argument needs none; double backward raises.  im2col_step bounds the images per launch and per plan; it need not
      divide N and no bit of any result depends on it.  float32, and float16 / bfloat16 input under the contract below (output and
      d_input); offset and mask are float32 or the input's own 16-bit dtype (widened before the launch, their gradients rounded once to
      that dtype); anything else is a TypeError.  Limits, each a ValueError naming the argument: 1 <= kh, kw <= MAX_DCNV3_KERNEL = 7,
      1 <= Gc <= MAX_DCNV3_CHANNELS = 256, stride and dilation in [1, MAX_DCNV3_STEP], padding in [0, MAX_DCNV3_STEP], a finite
      offset_scale, H, W <= 2 ** 24, and for a chunk of n images n H W G <= MAX_MSDA_INDEX and n Ho Wo G K 4 <= MAX_MSDA_INDEX.  N == 0 or
      Ho Wo == 0 give empty results and zero gradients without a launch.  dcnv3_core_pytorch is InternImage's grid_sample composition,
      the fallback users know, on any device: pad, reference points and the dilated grid in normalised coordinates of the padded map,
      one grid_sample, the masked sum over K (it materialises an [N G, Gc, Ho Wo, K] tensor).  The module has InternImage's parameter
      names (dw_conv.0, dw_conv.1.1, offset, mask, input_proj, output_proj) and init (zeros on offset and mask, Xavier-uniform with zero
      bias on the projections), so InternImage checkpoints load strict; the depthwise convolution, LayerNorm, GELU, the linear layers
      and the softmax over K are torch's; on the GPU the sampler is this operator, elsewhere the composition.  center_feature_scale
      and remove_center are not implemented (NotImplementedError).
  dcnv4(input, offset_mask, kernel_size, stride=1, padding=0, dilation=1, group=1, offset_scale=1.0, im2col_step=256, remove_center=False)
  DCNv4Function.apply(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                      group_channels, offset_scale, im2col_step, remove_center)
  dcnv4_core_pytorch(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                     group_channels, offset_scale, remove_center)
  DCNv4(channels=64, kernel_size=3, stride=1, pad=1, dilation=1, group=4, offset_scale=1.0, dw_kernel_size=None,
        center_feature_scale=False, remove_center=False, output_bias=True, without_pointwise=False)
      DCNv4, the deformable convolution v4 of the FlashInternImage backbones (csrc/ops_dcnv4.hip; restated, unpinned: where upstream
      differs include/frcnn_hip.h holds): dcnv3's sampling on ONE packed tensor, with masks that are not soft-maxed (unbounded, signed)
      and optionally without the centre point.  input [N, H, W, G Gc]; offset_mask [N, Ho, Wo, L], the raw output of one nn.Linear: the
      record of a pixel holds one slice per group g at [3 P g, 3 P (g + 1)), inside it (dx, dy) of point p at [2 p, 2 p + 1] and its mask
      value at [2 P + p]; L = ceil(3 G P / 8) 8, and the last L - 3 G P values are padding, never read (a NaN there changes nothing),
      their gradient 0.  P = kh kw, points enumerated as dcnv3's (x the outer index); with remove_center (kh == kw, odd, >= 3, else a
      ValueError) the point (kw // 2, kh // 2) is skipped, the later points move down by one and P = kh kw - 1.  Ho, Wo, the coordinate of
      a sample, the sample test, corners, weights and every sum are dcnv3's, by the same kernels: with remove_center=False
      dcnv4(x, pack(offset, mask)) equals dcnv3(x, offset, mask) bit for bit, forward and all gradients.  Gradients go to input and to
      offset_mask as ONE tensor laid out as offset_mask, every element written once by one launch (pad lanes zeros); deterministic, no
      atomics; d_input by dcnv3's plan, sort and gather; each is skipped when not needed; double backward raises.  im2col_step, the
      16-bit contract (input, output, d_input; offset_mask float32 or the input's 16-bit dtype, widened before the launch -- the kernels
      do not read 16-bit records -- its gradient rounded once to that dtype) and the limits are dcnv3's with K = P.
      dcnv4_core_pytorch is the grid_sample composition on any device (it unpacks the record, drops the centre location when asked,
      applies no softmax): the CPU fallback.  The module takes [N, L, C] with shape=(H, W) (or L a perfect square) and has upstream's
      parameter names (offset_mask, and value_proj / output_proj unless without_pointwise; offset_mask_dw, a depthwise Conv2d, only with
      dw_kernel_size) and init (zeros on offset_mask, Xavier-uniform with zero bias on the projections), so checkpoints load strict; any
      Gc in [1, 256] works (upstream's Gc % 16 == 0 is not required); center_feature_scale is not implemented (NotImplementedError).
  border_align(input, boxes, pool_size) -> Tensor [N, C, K, 4]
  BorderAlign(pool_size).forward(input, boxes)
  border_align_pytorch(input, boxes, pool_size)
      BorderAlign, the border pooling of BorderDet's heads (csrc/ops_border.hip; mmcv's border_align restated, unpinned: where the two
      differ include/frcnn_hip.h holds).  input [N, 4 C, H, W], channels [0, C) for the top edge, [C, 2 C) left, [2 C, 3 C) bottom,
      [3 C, 4 C) right; boxes [N, K, 4] as (x1, y1, x2, y2) in map coordinates, float32 or the input's own 16-bit dtype, any strides; K
      need not be H W.  The result is [N, C, K, 4] (channels_last memory), last axis top, left, bottom, right, in the input's dtype.  All
      arithmetic is float32.  Edge e starts at (x1, y1) (top, left) or (x2, y2) (bottom, right) and steps by s = (x2 - x1) / pool_size
      along x (top: +s, bottom: -s) or (y2 - y1) / pool_size along y (left: +s, right: -s); sample i = 0 .. pool_size lies at
      (x0 + (float)i dx, y0 + (float)i dy), the product first, in both directions (mmcv accumulates x += stride forwards and multiplies
      backwards).  A sample counts iff -1 <= y <= H and -1 <= x <= W, with roi_align's bilinear value (coordinates <= 0 go to 0, a low
      index >= size - 1 collapses to the last cell); otherwise, NaN included, it is exactly 0 and receives nothing.  No box is rejected
      as a whole: inverted, empty and non-finite boxes are sampled by that rule.  out[n, c, k, e] is the maximum over i under
      val > best from i = 0: ties go to the smallest i, a NaN sample never replaces the running value, a NaN at i = 0 stays.  The int32
      argmax is saved and the backward sends dout[n, c, k, e] to the four cells of that sample: roi_align's 2 x 2 tile gather with one
      wave per edge group, which tests BORDER_ALIGN_CULL_LIST = 64 boxes at once and walks the ballot's bits, each lane re-deriving its
      channels' samples from their argmax; ascending box order, no atomics (two runs agree bit for bit; mmcv's is an atomic scatter).
      boxes get no gradient (None), as in mmcv; double backward raises.  16-bit maps under the contract below (output and d_input; the
      argmax is the widened map's).  Limits:
      pool_size in [1, MAX_BORDER_POOL = 64], H, W <= MAX_BORDER_SIDE = 2 ** 24, and the flat launch grids N K 4 ceil(C / 4) and
      N ceil(C / 256) ceil(H / 2) ceil(W / 2) <= MAX_BORDER_INDEX.  N == 0, K == 0 or C == 0 give empty results and a zero d_input
      without a launch.  border_align_pytorch is the same contract from torch operations (index gathers and torch.max), on any device,
      differentiable by autograd, in float64 for a float64 map and float32 otherwise: the CPU route, and what tools/ops_bench.py
      measures the kernels against.
  riroi_align_rotated(input, rois, output_size, spatial_scale=1.0, num_samples=0, num_orientations=8, clockwise=False)
  RiRoIAlignRotated(out_size, spatial_scale, num_samples=0, num_orientations=8, clockwise=False).forward(input, rois)
  riroi_align_rotated_pytorch(pooled, rois, num_orientations=8)
      ReDet's rotation-invariant RoI pooling (csrc/ops_rot.hip; mmcv's riroi_align_rotated restated, unpinned: where the two differ
      include/frcnn_hip.h holds).  input [N, C n, H, W], n = num_orientations in [1, MAX_RIROI_ORIENTATIONS = 64] dividing the channel
      count (else ValueError), channel c n + o being orientation o of group c; rois [K, 6] (batch index, cx, cy, w, h, angle), float32 or
      the input's own 16-bit dtype; the other limits are roi_align_rotated's, num_samples playing sampling_ratio's part.  The result is
      [K, C n, oh, ow] (channels_last memory).  Pool, then blend: S = roi_align_rotated(input, rois, output_size, spatial_scale,
      num_samples, aligned=False, clockwise=not clockwise) in float32, then per RoI f = float32(float64(angle) n / (2 pi)), ind = floor(f),
      l = f - ind, r = 1 - l, k = ind mod n >= 0 and out[c n + o] = r S[c n + (o - k) mod n] + l S[c n + (o - k + 1) mod n], two products
      and a sum, each rounded.  mmcv blends per sample; pooling each source channel once and blending the pooled values is the same sum
      in another order at half the loads, and makes the result bit-identical to riroi_align_rotated_pytorch(S, rois, n).  One launch each
      way: the forward exchanges the pooled runs through LDS, the backward is roi_align_rotated's culled tile gather that blends dS where it
      loads a bin's gradient (deterministic, no atomics; mmcv's is an atomic scatter).  A RoI with a batch index outside (-1, N), a
      non-finite angle or |f| >= 2 ** 24 pools to zeros and sends no gradient.  rois get no gradient; double backward raises.  16-bit
      maps: S and the blend stay float32, one rounding (op(x) == op(x.float()).to(x.dtype)).  riroi_align_rotated_pytorch is the blend
      alone, from torch operations around any pooled S, on any device, differentiable by autograd in S.
  rotated_feature_align(features, best_bboxes, spatial_scale=1 / 8, points=1)
  RotatedFeatureAlign(spatial_scale=1 / 8, points=1).forward(features, best_bboxes)
  rotated_feature_align_pytorch(features, best_bboxes, spatial_scale=1 / 8, points=1)
      R3Det's feature refinement module (csrc/ops_rfa.hip; mmcv's rotated_feature_align restated, unpinned).  features [N, C, H, W];
      best_bboxes [N, H, W, 5], one row per pixel, float32 (or the map's 16-bit dtype), any strides.  COMPONENT 0 OF A ROW IS THE ROW
      (y) COORDINATE: the row is (y, x, w, h, angle) in input coordinates, although mmcv's docstring names it (x, y, w, h, a); swap the
      first two columns of (x, y, ...) boxes.  y0 = b0 s, x0 = b1 s, w2 = b2 s / 2, h2 = b3 s / 2, (wx, wy) = (cos a, sin a) w2,
      (hx, hy) = (-sin a, cos a) h2; the sample points are the centre (x0, y0) and, for points = 5, the corners (x0 + wx + hx, y0 + wy +
      hy), (x0 - wx + hx, y0 - wy + hy), (x0 - wx - hx, y0 - wy - hy), (x0 + wx - hx, y0 + wy - hy).  out[n, :, h, w] = features[n, :, h, w]
      + the bilinear samples of features[n] at the pixel's points, added in that order in float32, by roi_align's rule (nothing outside
      [-1, size] or at a non-finite coordinate).  points is 1 or 5 (else ValueError); with points = 1 components 2..4 are never read.  The
      result has the input's dtype and memory format.  Backward for features only: d_features[cell] = dout[cell], then + weight *
      dout[pixel] over the sample corners that land on the cell in ascending (pixel, point, corner) order, through the sorted plan of
      multi_scale_deformable_attn (one plan and one stable sort, 64 channel runs per block): deterministic, no atomics.  N H W points 4
      <= MAX_RFA_INDEX.  rotated_feature_align_pytorch is the same contract from index gathers, on any device, float64 for a float64 map.
  convex_iou(pointsets, polygons) -> float32 [N, K]
  convex_giou(pointsets, polygons) -> (giou float32 [N], grad float32 [N, 18])
  min_area_polygons(pointsets) -> float32 [N, 8]
  convex_iou_pytorch(pointsets, polygons), convex_giou_pytorch(pointsets, polygons), min_area_polygons_pytorch(pointsets)
      The point-set operators of Oriented RepPoints, CFA and SASM (csrc/ops_convex.hip; mmcv has operators of these names and
      signatures, but the contract is the mathematical one of include/frcnn_hip.h: mmcv's epsilons, hull tie-breaks and the scaling of
      its gradient output are not followed).  Everything is float32.  pointsets [N, 18], rows (x1, y1, ..., x9, y9); polygons [K, 8]
      (convex_giou: [N, 8], aligned pairs), four vertices in any order.  P is the convex hull of the nine points, Q of the four
      vertices, H of all thirteen: strictly convex vertices, counter-clockwise from the smallest (x, y); a point inside a hull edge is
      no vertex, of equal points the smallest index is.  Turns and crossings are decided on coordinates relative to an origin (a set's
      own smallest point for its own hull, Q's smallest vertex for everything about a pair), so boxes near x = 4096 behave as boxes near
      0, and the hull is a function of the set: permuting the nine points or the four vertices changes no bit of any result (grad is
      permuted alike; the header names the one exception, three nearly collinear candidates whose rounded products tie).  A_P, A_Q and C = area(H) are shoelace sums, I = area(P n Q) (Sutherland-Hodgman) is clamped at 0, U = A_P +
      A_Q - I.  A row is dead when a coordinate is not finite, a polygon also when A_Q < 1e-14; a pair when a row of it is, or U <
      1e-14 or C < 1e-14.  A degenerate set (A_P = 0) is not dead: I = 0 and the gradient goes through C.  convex_iou is I / U, 0 for a
      dead pair, not differentiable (detached); a workgroup forms each hull of its CONVEX_IOU_TILE_ROWS x 64 tile once.  convex_giou
      is I / U + U / C - 1 and its closed-form derivative in the 18 coordinates (the header states it: N / 2 of each hull edge's
      scaled normal to both ends for the areas, N (s1 - s2) and N s2 for the part of P's edge inside Q), from ONE launch; a dead pair
      gives 0 and a zero row, points that are no vertices of P exactly 0.  giou is differentiable by autograd too -- its backward is
      grad_out[:, None] * grad, so (1 - giou).mean().backward() works --, grad is not; polygons get no gradient.  min_area_polygons:
      over P's edges in hull order, u the edge's unit direction and v its left normal, the extents [u_min, u_max] x [0, v_max] of the
      hull's vertices relative to the edge's start; the smallest (u_max - u_min) v_max wins, ties to the first edge (exact ties are
      structural -- every edge of an acute triangle gives twice its area -- so a later edge wins only with an area < (1 - 2^-18)
      times the best so far: CONVEX_RECT_TIE); corners (u_min, 0),
      (u_max, 0), (u_max, v_max), (u_min, v_max), counter-clockwise; two hull vertices a, b give (a, b, b, a), one gives it four
      times, a non-finite row zeros; not differentiable.  N = 0 or K = 0 gives empty tensors without a launch; K <=
      MAX_CONVEX_POLYGONS, N <= MAX_CONVEX_ROWS; coordinate differences below 2^60 (beyond, products overflow).  Other dtypes are a
      TypeError, CPU tensors, other shapes and differing devices a ValueError.  The _pytorch
      forms are the same contract from torch operations (hull edges by the all-pairs left-of test, areas by the boundary sum over the
      clipped edge pieces), on any device, float32 or float64, convex_giou_pytorch's gradient from autograd; they serve point sets in
      GENERAL POSITION only: no duplicate points, no three collinear hull points, no coincident edges.
  box_iou_quadri(bboxes1, bboxes2, mode="iou", aligned=False) -> float32 [N, M], or [N] when aligned
  nms_quadri(dets, scores, iou_threshold, labels=None) -> (dets [K, 9], keep int64 [K])
  points_in_polygons(points, polygons) -> float32 [N, M]
  box_iou_quadri_pytorch(bboxes1, bboxes2, mode="iou", aligned=False), points_in_polygons_pytorch(points, polygons)
      The quadrilateral operators of the heads that predict four free corners and of the point-set assigners (csrc/ops_quadri.hip, on
      the device functions of convex_iou; mmcv has operators of these names and signatures, the contract is include/frcnn_hip.h's).
      Everything is float32.  A quadrilateral is a row (x1, y1, ..., x4, y4): four vertices in ANY order and either winding, and it
      stands for Q, the convex hull of its vertices under convex_iou's hull rules, so permuting the four vertices changes no bit of any
      result.  A non-convex or self-crossing row therefore counts as its hull: the one deliberate deviation from mmcv, whose kernels walk
      the vertices in the order given; for a convex quadrilateral given in order, which is every use in mmrotate, the two agree.  A row
      with a non-finite coordinate is dead, and so is a quadrilateral whose hull area is below 1e-14 (CONVEX_MIN_AREA).
      box_iou_quadri: A1, A2 the hull areas, I the area of hull 1 clipped against hull 2's half-planes (Sutherland-Hodgman, a vertex on
      the line inside) on coordinates relative to hull 2's smallest vertex, clamped at 0; mode "iou" is I / (A1 + A2 - I), "iof" is I /
      A1; exactly 0 for a dead row or a denominator below 1e-14, and without a clip when the bounding boxes are apart; a live
      quadrilateral against its own bits gives exactly 1 in both modes; aligned=True needs N == M and gives the matrix's diagonal bit
      for bit.  In mode "iou" the result has the bits of convex_iou(s, bboxes2), s[i] being bboxes1[i]'s four vertices followed by five
      copies of the first.  A workgroup forms each hull of its QUADRI_IOU_TILE_ROWS x 64 tile once.  nms_quadri: nms_rotated on
      quadrilaterals -- the same ordering (stable descending scores, NaN scores last), labels, bit mask and greedy pass; sorted
      quadrilateral j goes iff a kept quadrilateral i before it, of the same label, has box_iou_quadri(i, j) > float32(iou_threshold);
      dets is cat(dets[keep], scores[keep, None]).  N <= MAX_NMS_BOXES.  points_in_polygons: 1.0 when point i [N, 2] lies in the CLOSED
      hull Q_j of polygon j [M, 8] -- for every hull edge a -> b, (b_x - a_x) (p_y - a_y) >= (b_y - a_y) (p_x - a_x) on coordinates
      relative to Q_j's smallest vertex, the two rounded products compared --, else 0.0; 0.0 for a dead polygon and a non-finite point.
      A point on an edge or a vertex is inside (mmcv's crossing-number loop is half-open on the boundary instead).  A workgroup owns
      POINTS_IN_POLYGONS_TILE_ROWS points x 64 polygons.  None is differentiable (inputs are detached; mmcv has no autograd either).
      Empty inputs give empty outputs without a launch; rows <= MAX_QUADRI_ROWS, columns of a matrix <= MAX_QUADRI_COLUMNS.  Other
      dtypes are a TypeError, CPU tensors, other shapes and differing devices a ValueError.  The _pytorch forms are the same contract
      from torch operations (convex_iou_pytorch's hull list and boundary sum), on any device, float32 or float64, for quadrilaterals in
      GENERAL POSITION only: no duplicate vertices, no three collinear vertices, no coincident edges, no point on an edge's line.
  masked_conv2d(features, mask, weight, bias, padding=0, stride=1) -> [N, C_out, oh, ow]
  MaskedConv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True).forward(input, mask=None)
  masked_conv2d_pytorch(features, mask, weight, bias, padding=0, stride=1)
      The sparse convolution of Guided Anchoring's heads (GA-RPN, GA-Faster R-CNN, GA-RetinaNet evaluate conv_cls and conv_reg only
      where the location map passed its threshold; csrc/ops_mconv.hip; mmcv has operators of these names and signatures, the contract
      is include/frcnn_hip.h's).  features [N, C_in, H, W], weight [C_out, C_in, kh, kw] and bias [C_out] (or None: a zero bias) are
      all float32, all float16 or all bfloat16; every mix is a TypeError.  padding is an int or a pair, stride must be 1 (mmcv's rule;
      else ValueError).  mask [N, oh, ow] lies on the OUTPUT grid oh = H + 2 pad_h - kh + 1, ow = W + 2 pad_w - kw + 1, in any real
      dtype or bool; a pixel is active iff mask > 0, so NaN is inactive.  At an active pixel out[b, co, y, x] = bias[co] + sum over (c,
      i, j) of weight[co, c, i, j] features[b, c, y - pad_h + i, x - pad_w + j], taps outside the map counting as zero; everywhere
      else out is +0.0, without the bias.  The sum runs in float32 in ascending (c, i, j) -- on the exact-float32 matrix instruction,
      or for 16-bit tensors on the 16-bit one with float32 accumulators, bias added in float32, one rounding on the store -- in an
      order that depends on (C_in, kh, kw) alone: an active pixel's bits do not depend on the rest of the mask, on N, or on the memory
      format.  The output has the features' dtype and memory format; NCHW-contiguous and channels_last maps are read in place, any
      other layout is made contiguous first.  A compaction kernel lists the active pixels on the device and a fused gather-and-
      multiply kernel works through tiles of MASKED_CONV_TILE_PIXELS listed pixels x MASKED_CONV_TILE_CHANNELS channels in chunks of
      MASKED_CONV_K_CHUNK reduction indices; its grid holds the worst case and surplus blocks return at once, so the active count
      never reaches the host: no host synchronisation anywhere in the call.  Deviations from mmcv, all deliberate: N >= 1 (mmcv
      asserts 1), the mask on the output grid (mmcv asserts the map's size and scatters out of bounds when they differ), bias=None
      allowed, MaskedConv2d.forward with a mask and dilation != 1 or groups != 1 a ValueError (mmcv ignores the dilation).  Inference
      only, like mmcv (whose backward returns None for every input): no autograd formula is registered, so a backward through the op
      raises torch's not-implemented error.  MaskedConv2d is an nn.Conv2d -- parameters weight and bias, so mmdet checkpoints load
      strict --; without a mask it is nn.Conv2d.forward and trains.  Sizes up to MAX_MASKED_CONV_INDEX (N oh ow, C_out C_in kh kw and
      each tensor's elements).  masked_conv2d_pytorch keeps the same contract from torch operations (mmcv's nonzero / gather / addmm /
      scatter composition, one image at a time, which synchronises on a GPU), on any device, float64 too.
  paste_masks_in_image(masks, boxes, img_shape, padding=1) -> [K, 1, H, W]            paste_masks_in_image_pytorch(...)
  paste_masks_aligned(masks, boxes, image_shape, threshold=0.5) -> bool / uint8 [K, H, W]    paste_masks_aligned_pytorch(...)
  masks_to_boxes(masks) -> float32 [N, 4]                                                 masks_to_boxes_pytorch(masks)
      The last step of a Mask R-CNN's mask head and the box of a mask (csrc/ops_mask.hip; the contracts are include/frcnn_hip.h's,
      restated from torchvision and detectron2 / mmdetection, unpinned).  No autograd (upstream's paste is never differentiated): a
      mask or box tensor that requires grad is accepted and the result does not.  Nothing synchronises with the host, every output
      element is written by the one launch (no memset in front of it), two runs agree bit for bit.
      paste_masks_in_image is torchvision's roi_heads.paste_masks_in_image without its Python loop (4 host reads and ~6 launches per
      mask): masks [K, 1, M, M] float32 / float16 / bfloat16, square (else ValueError), M <= MAX_PASTE_MASK_SIDE; boxes [K, 4] float32
      (x1, y1, x2, y2); img_shape (H, W); padding an int in [0, MAX_PASTE_PADDING].  With M' = M + 2 padding and s = float32(M' / M)
      (the division in double), per box IN FLOAT32 AND IN THIS ORDER, no fused multiply-add: w_half = (x2 - x1) * 0.5, x_c =
      (x2 + x1) * 0.5, w_half = w_half * s, X0 = trunc(x_c - w_half), X1 = trunc(x_c + w_half), likewise in y; trunc is toward zero and
      saturates to [-PASTE_CORNER, PASTE_CORNER].  bw = max(X1 - X0 + 1, 1), bh likewise.  Pixel (y, x) is non-zero only if X0 <= x <
      X0 + bw, X0 <= X1, Y0 <= y < Y0 + bh, Y0 <= Y1; there r = float32(M') / float32(bw), sx = max(r * (dx + 0.5) - 0.5, 0) with dx =
      x - X0, ix = min((int)sx, M' - 1), ix1 = ix + (ix < M' - 1), lx = sx - ix, likewise y, and value = (1 - ly) * ((1 - lx) * P[iy][ix]
      + lx * P[iy][ix1]) + ly * ((1 - lx) * P[iy1][ix] + lx * P[iy1][ix1]), P the mask padded by `padding` zeros (never materialised).
      float32 arithmetic on widened masks, one rounding on the store: op(x_T) == op(x_T.float()).to(T) bit for bit.  Deviations
      (torchvision raises or is undefined there): a non-finite coordinate, an inverted integer box or a box wholly outside the image
      give an all-zero image; corners saturate; a huge box costs nothing extra; K == 0 gives an empty [0, 1, H, W].
      paste_masks_aligned is detectron2's paste_masks_in_image / mmdet's _do_paste_mask plus its threshold, without the K x H x W x 2
      grid, the float image and the 1 GB chunking: masks [K, Mh, Mw] or [K, 1, Mh, Mw] (rectangular allowed, each side <=
      MAX_PASTE_MASK_SIDE), boxes [K, 4] float32 (x0, y0, x1, y1), threshold a float.  Sample coordinates in pixels, float32, in this
      order: sx = ((x + 0.5) - x0) / (x1 - x0) * Mw - 0.5, sy likewise with Mh; value is the blend above on floor / floor + 1 of the
      unpadded mask with a corner outside it counting 0 (grid_sample(align_corners=False, padding_mode="zeros")), never rounded to a
      16-bit type.  threshold >= 0: torch.bool, value >= float32(threshold); threshold < 0: torch.uint8, trunc(value * 255) saturated
      to [0, 255], NaN giving 0.  Deviations: a row with a non-finite coordinate, x1 <= x0 or y1 <= y0 gives all False / 0 (upstream
      flips or smears such a mask); decisions may differ from upstream's within the float32 error of the threshold.
      masks_to_boxes is torchvision.ops.masks_to_boxes without its loop (a torch.where and a host read per mask): masks [N, H, W]
      bool, uint8, float32, float16 or bfloat16 with any strides (made contiguous by one copy); (x_min, y_min, x_max, y_max) over the
      pixels != 0, maxima inclusive; NaN counts as non-zero, -0.0 as zero; an all-zero mask gives (0, 0, 0, 0), detectron2's convention
      (torchvision raises there); N == 0 gives [0, 4].  H W of one image up to MAX_MASK_PLANE; K H W may exceed 2^31.
      The _pytorch twins state the same contracts, deviations included, from torch operations on any device, float64 masks too (then
      the arithmetic after the float32 integer box is float64).
      Measured on an MI355X (tools/ops_bench.py --only mask; K = 100, M = 28, 800 x 1333; MASK_BENCH below):
      paste_masks_in_image float32 82 us (38 x its twin, 96 x torchvision's loop; 5.2 TB/s written), float16 58 us;
      paste_masks_aligned bool 68 us, uint8 60 us (28-36 x the grid_sample composition; 1.6-1.8 TB/s: the evaluation inside the boxes
      bounds the byte forms, not the store); masks_to_boxes bool 28 us (15 x its twin), float32 74 us (5.8 TB/s read).
  heatmaps_to_keypoints(maps, rois) -> (xy_preds [R, K, 3], end_scores [R, K])             heatmaps_to_keypoints_pytorch(maps, rois)
  heatmaps_to_keypoints_scored(maps, rois) -> [R, K, 4] = (x, y, logit, prob)               heatmaps_to_keypoints_scored_pytorch(maps, rois)
  keypointrcnn_inference(x, boxes) -> (list of xy_preds, list of end_scores)
  keypoints_to_heatmap(keypoints, rois, heatmap_size) -> (heatmaps int64 [R, K], valid int64 [R, K])
      The last step of a Keypoint R-CNN's keypoint head (csrc/ops_keypoint.hip; the contract is include/frcnn_hip.h's, restated from
      torchvision's roi_heads and detectron2's structures/keypoints, unpinned).  Upstream loops over the detections: two host reads, a
      [K, ceil(h), ceil(w)] float image from F.interpolate(bicubic), an argmax and a gather per detection.  Here one launch does all
      of them, a block per (RoI, keypoint) with the map in LDS; the image never exists, nothing synchronises with the host, two runs
      agree bit for bit.  No autograd: a tensor that requires grad is accepted and the result does not.
      maps [R, K, Mh, Mw] float32 / float16 / bfloat16 (a 16-bit map gives, bit for bit, the result of maps.float()), each side <=
      MAX_KEYPOINT_MAP_SIDE; rois [R, 4] (x1, y1, x2, y2) of any float dtype, converted to float32.  Per RoI w = max(x2 - x1, 1), h
      likewise, W = ceil(w), H = ceil(h); the logit image is torch's upsample_bicubic2d(align_corners=False) of the map to [H, W]
      (A = -0.75, the source coordinate scale * (d + 0.5) - 0.5 not clamped, tap indices clamped), in float32 in the header's stated
      order without fused multiply-adds, rows combined first.  The maximum's (xi, yi) -- ties to the smallest yi * W + xi, a NaN above
      every number and the first NaN winning -- gives x = (xi + 0.5) * (w / W) + x1, y likewise, logit = the maximum, prob = 1 /
      sum(exp(map - logit)) (detectron2's score).  Defined where upstream is not: a constant map gives (xi, yi) = (0, 0) and its own
      value as the logit (an all -inf map among them: logit -inf, prob NaN); a RoI with a non-finite coordinate or with W or H above
      MAX_KEYPOINT_ROI_SIDE is refused: four NaNs per keypoint (torchvision's shape: NaN, NaN, 1 and a NaN score), no work; R == 0
      or K == 0 launch nothing.  heatmaps_to_keypoints is torchvision's signature and return, heatmaps_to_keypoints_scored
      detectron2's; keypointrcnn_inference is torchvision's wrapper over per-image box lists: one launch for all images, then the
      split.  CPU tensors and float64 maps are served by the _pytorch twins: the per-RoI loop upstream runs (F.interpolate, argmax,
      gather; two host reads per RoI) with the defined cases carried, float64 maps computed and returned in float64.
      keypoints_to_heatmap is torchvision's training-target encoder (keypoints [R, K, 3] = (x, y, visibility) -> the flat index
      y * S + x of each keypoint's cell in its RoI's S x S heatmap and whether it is valid): a handful of elementwise torch operations
      that never read the host, so it is plain torch on any device and has no kernel.
      Measured on an MI355X (tools/ops_bench.py --only keypoint; KEYPOINT_BENCH below): R = 100 detections of an
      800 x 1333 image, K = 17, 56 x 56 maps: 292 us, 56 x the twin's loop (16.3 ms), float16 maps the same; R = 4 image-sized boxes:
      927 us, 1.6 x the loop.

Mixed precision.  For T in {float16, bfloat16} the RoI operators run natively on 16-bit maps (the frcnn_ops_*_16 kernels), with
torchvision's autocast definition as the contract, bit for bit:
      op(x_T, boxes)  ==  op(x_T.float(), boxes).to(T)          backward:  dx_T  ==  op_backward(grad_T.float()).to(T)
Values are widened exactly on load; geometry, weights and sums are the float32 kernels' (one shared body); the result is rounded once, to
nearest even, on store, and backward sums never pass through 16-bit memory.  RoIPool's maximum and argmax are those of the float32 op.
Boxes stay float32; boxes in the map's own 16-bit dtype are accepted too (torchvision requires equal dtypes outside autocast) and widened
before the launch, so the kernels and the level mapper only ever see float32 RoIs.  Any other combination is a TypeError, as is a pyramid
of mixed dtypes.  No autocast registration is needed: under torch.autocast the backbone hands the ops 16-bit maps and float32 boxes, which
they take as they are.  nms / batched_nms keep float32 or float64 boxes (widen 16-bit boxes at the call).

Inputs must be CUDA (HIP) tensors; there is no CPU implementation.  channels_last inputs go to the NHWC kernels as they are, contiguous
NCHW inputs are converted once, a channel count that is not a multiple of 4 (of the 16-bit kernels' run of 8 for 16-bit maps) goes through
a zero-padded copy; input gradients come back in the input's dtype and memory format.
"""
import ctypes as C
import math
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _native as nv

__all__ = ["nms", "batched_nms", "roi_pool", "roi_align", "RoIPool", "RoIAlign", "multi_scale_roi_align", "MultiScaleRoIAlign",
           "ps_roi_pool", "ps_roi_align", "PSRoIPool", "PSRoIAlign", "deform_conv2d", "DeformConv2d", "deform_roi_pool", "DeformRoIPool",
           "DeformRoIPoolPack", "ModulatedDeformRoIPoolPack", "box_iou_rotated", "nms_rotated", "roi_align_rotated", "RoIAlignRotated",
           "diff_iou_rotated_2d", "diff_iou_rotated_3d", "diff_iou_rotated_2d_pytorch", "soft_nms", "soft_nms_pytorch",
           "carafe", "CARAFE", "CARAFEPack", "multi_scale_deformable_attn", "multi_scale_deformable_attn_pytorch",
           "MultiScaleDeformableAttnFunction", "MultiScaleDeformableAttention", "prroi_pool", "PrRoIPool", "prroi_pool_pytorch",
           "dcnv3", "DCNv3Function", "dcnv3_core_pytorch", "DCNv3", "dcnv4", "DCNv4Function", "dcnv4_core_pytorch", "DCNv4",
           "border_align", "BorderAlign", "border_align_pytorch", "riroi_align_rotated", "RiRoIAlignRotated",
           "riroi_align_rotated_pytorch", "rotated_feature_align", "RotatedFeatureAlign", "rotated_feature_align_pytorch",
           "convex_iou", "convex_giou", "min_area_polygons", "convex_iou_pytorch", "convex_giou_pytorch", "min_area_polygons_pytorch",
           "box_iou_quadri", "nms_quadri", "points_in_polygons", "box_iou_quadri_pytorch", "points_in_polygons_pytorch",
           "masked_conv2d", "MaskedConv2d", "masked_conv2d_pytorch",
           "paste_masks_in_image", "paste_masks_aligned", "masks_to_boxes",
           "paste_masks_in_image_pytorch", "paste_masks_aligned_pytorch", "masks_to_boxes_pytorch",
           "heatmaps_to_keypoints", "heatmaps_to_keypoints_scored", "keypointrcnn_inference", "keypoints_to_heatmap",
           "heatmaps_to_keypoints_pytorch", "heatmaps_to_keypoints_scored_pytorch"]

_CL = torch.channels_last
MAX_OUTPUT = 64
DEFORM_ROI_CULL_LIST = 256                # RoIs that deform_roi_pool's input-gradient gather lists per pass (DROI_LIST of csrc/ops_droi.hip)
ROI_ALIGN_ROTATED_CULL_LIST = 1024        # RoIs that roi_align_rotated's backward gather lists per pass (OPS_LIST of csrc/ops_run.h)
PRROI_CULL_LIST = 1024                    # RoIs that prroi_pool's input-gradient gather lists per pass (OPS_LIST of csrc/ops_run.h)
MAX_SAMPLING_RATIO = 16
MAX_NMS_BOXES = 524288
MAX_ROTATED_IOU_ROWS = 65535 * 64         # rows of box_iou_rotated's matrix (the tile rows of its launch grid)
MAX_CONVEX_POLYGONS = 65535 * 64          # columns of convex_iou's matrix (the tile columns of its launch grid)
MAX_CONVEX_ROWS = 2 ** 31 - 1 - 1024      # point sets of one call (CVX_MAX_ROWS of csrc/ops_convex.hip: the grids' ceilings are formed in int)
CONVEX_IOU_TILE_ROWS = 32                 # rows of convex_iou's tile (CVX_TILE_ROWS of csrc/ops_convex.hip); its columns: 64
CONVEX_MIN_AREA = 1e-14                   # below it a polygon, a union or an enclosing hull is dead (CVX_MIN_AREA)
CONVEX_RECT_TIE = 1 - 2.0 ** -18          # min_area_polygons: a later edge wins only with an area below this times the best (CVX_RECT_TIE)
MAX_QUADRI_ROWS = 2 ** 31 - 1 - 1024      # quadrilaterals or points of one call (frcnn_ops_quadri_max_rows: the grids' ceilings are formed in int)
MAX_QUADRI_COLUMNS = 65535 * 64           # columns of box_iou_quadri's and points_in_polygons' matrix (frcnn_ops_quadri_max_columns)
QUADRI_IOU_TILE_ROWS = 32                 # rows of box_iou_quadri's tile (QUAD_TILE_ROWS of csrc/ops_quadri.hip); its columns: 64
POINTS_IN_POLYGONS_TILE_ROWS = 256        # points of points_in_polygons' tile (QUAD_POINT_ROWS of csrc/ops_quadri.hip); its columns: 64
MASKED_CONV_TILE_PIXELS = 64              # listed pixels of masked_conv2d's tile (frcnn_ops_masked_conv2d_tile_pixels(): MC_T of csrc/ops_mconv.hip)
MASKED_CONV_TILE_CHANNELS = 64            # output channels of that tile (frcnn_ops_masked_conv2d_tile_channels())
MASKED_CONV_K_CHUNK = 32                  # reduction indices (c, i, j) of one of its LDS stages (frcnn_ops_masked_conv2d_k_chunk())
MAX_MASKED_CONV_INDEX = 2 ** 31 - 1 - 1024    # what its 32-bit indices hold: N oh ow, C_out C_in kh kw, a tensor's elements (frcnn_ops_masked_conv2d_max_index())
MAX_PASTE_MASK_SIDE = 112                 # M, Mh, Mw of the paste operators: the mask lies in LDS as float32 (frcnn_ops_paste_masks_max_side())
MAX_PASTE_PADDING = 65536                 # paste_masks_in_image's padding (frcnn_ops_paste_masks_max_padding())
PASTE_CORNER = 2 ** 29                    # its integer corners saturate to [-2^29, 2^29] (frcnn_ops_paste_masks_max_corner())
MAX_MASK_PLANE = 2 ** 31 - 1 - 1024       # H W of one image of the mask operators (frcnn_ops_mask_max_plane()); K H W is 64-bit
MAX_KEYPOINT_MAP_SIDE = 112               # Mh, Mw of heatmaps_to_keypoints: the map lies in LDS as float32 (frcnn_ops_keypoint_max_map_side())
MAX_KEYPOINT_ROI_SIDE = 4096              # ceil(w), ceil(h) of one of its RoIs: one block walks the resized image (frcnn_ops_keypoint_max_roi_side())
KEYPOINT_BLOCK_THREADS = 256              # its block: 4 waves, an output row each per pass, 64 pixels a step (frcnn_ops_keypoint_block_threads())
MAX_SOFT_NMS_BOXES = 65536                # soft_nms: one label may hold every box, and one workgroup then runs N dependent picks.  Measured on
                                          # an MI355X at N = 65536 in one problem (clustered boxes, thr 0.3): 43 ms linear and 48 ms gaussian at
                                          # min_score 0.05 (1503 / 1104 picks), 7 ms naive; 2.06 s in the worst case, min_score = 0, where all
                                          # 65536 boxes are picked one after the other (16384 boxes: 157 ms, 4096: 14 ms)
SOFT_NMS_METHODS = {"naive": 0, "linear": 1, "gaussian": 2}     # mmcv's method codes
MAX_LEVELS = 8
DEFORM_CHUNK_IMAGES = 32                  # images per chunk of deform_conv2d's column workspace (torchvision processes 32 at a time too)
MAX_DEFORM_INDEX = 2 ** 31 - 1 - 1024     # what the 32-bit indices of csrc/ops_deform.hip hold: columns, cells and plan entries of a chunk
MAX_CARAFE_KERNEL = 7                     # carafe's kernel_size: k k mask values in a thread's registers (CARAFE_MAX_KERNEL of csrc/ops_carafe.hip)
MAX_CARAFE_SCALE = 8                      # carafe's scale_factor
MAX_CARAFE_PLANE = 2 ** 31 - 1 - 1024     # elements of one upsampled plane, s H s W: the 32-bit indices inside a plane of csrc/ops_carafe.hip
MAX_MSDA_LEVELS = 8                       # multi_scale_deformable_attn: levels, points per level and channels per head (MSDA_MAX_* of
MAX_MSDA_POINTS = 16                      # csrc/ops_msda.hip: the L P samples of a block's items are staged in LDS, a lane's channel runs
MAX_MSDA_CHANNELS = 256                   # live in registers)
MSDA_SEGMENT = 512                        # entries of one piece of a long d_value segment (frcnn_ops_msda_segment())
MAX_MSDA_INDEX = 2 ** 31 - 1 - 1024       # what the 32-bit indices of csrc/ops_msda.hip hold: cells n S M and plan entries n Q M L P 4 of a chunk
MAX_DCNV3_KERNEL = 7                      # dcnv3: kh and kw (frcnn_ops_dcnv3_max_kernel(): the K samples of a block's items are staged in LDS)
MAX_DCNV3_CHANNELS = 256                  # dcnv3: channels of one group (frcnn_ops_dcnv3_max_channels())
MAX_DCNV3_STEP = 65536                    # dcnv3: stride, dilation and padding (the integer part of a coordinate stays far inside 32 bits)
MAX_DCNV3_SIDE = 2 ** 24                  # dcnv3: H and W, exact in float32
MAX_BORDER_POOL = 64                      # border_align: pool_size (BorderDet uses 10)
MAX_BORDER_SIDE = 2 ** 24                 # border_align: H and W, exact in float32
MAX_BORDER_INDEX = 2 ** 31 - 1 - 1024     # border_align's flat launch grids (csrc/ops_border.hip): the forward's lanes N K 4 ceil(C / 4) and the
                                          # backward's blocks N ceil(C / 256) ceil(H / 2) ceil(W / 2)
BORDER_ALIGN_CULL_LIST = 64               # boxes a wave of border_align's input-gradient gather tests at once (BORDER_GROUP of csrc/ops_border.hip)
MAX_RIROI_ORIENTATIONS = 64               # riroi_align_rotated: num_orientations (frcnn_ops_riroi_align_rotated_max_orientations(): a group lies
                                          # inside the 64 channel runs of one wave)
RFA_POINTS = (1, 5)                       # rotated_feature_align: the centre, or the centre and the four corners
MAX_RFA_INDEX = 2 ** 31 - 1 - 1024        # rotated_feature_align: the plan entries N H W points 4 of one call (csrc/ops_rfa.hip)
CARAFE_RUN = 4                            # channels a thread of carafe's d_features gather owns: G ceil(C / G / 4) blocks along the grid's y


# ---- argument checks (the public functions; the custom ops assume them) -----------------------------------------------------------
def _check_tensor(name, t, dtypes, what, fallback=None):
    """fallback: the name of the torch composition that serves other devices, for the message."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in dtypes:
        raise TypeError("%s must be %s, got %s" % (name, what, t.dtype))
    if t.device.type not in ("cuda", "meta"):
        raise ValueError("%s must be a tensor on the GPU, got device %s: fasterrcnn_amd.ops has no CPU implementation%s"
                         % (name, t.device, " (%s runs on any device)" % fallback if fallback else ""))


def _check_same_device(a, b, na, nb):
    if a.device != b.device:
        raise ValueError("%s and %s must be on the same device, got %s and %s" % (na, nb, a.device, b.device))


def _output_size(output_size):
    if isinstance(output_size, int):
        oh = ow = output_size
    elif isinstance(output_size, (tuple, list)) and len(output_size) == 2 and all(isinstance(v, int) for v in output_size):
        oh, ow = output_size
    else:
        raise TypeError("output_size must be an int or a pair of ints, got %r" % (output_size,))
    if not (1 <= oh <= MAX_OUTPUT and 1 <= ow <= MAX_OUTPUT):
        raise ValueError("output_size must lie in [1, %d], got (%d, %d)" % (MAX_OUTPUT, oh, ow))
    return oh, ow


_HALF = (torch.float16, torch.bfloat16)
_MAP_DTYPES = (torch.float32,) + _HALF
_MAP_WHAT = "float32, float16 or bfloat16"


def _box_dtypes(input):
    """Boxes are float32; with a 16-bit map, also that map's own dtype (widened before the launch)."""
    if input.dtype in _HALF:
        return (torch.float32, input.dtype), "float32 or the input's %s" % input.dtype
    return (torch.float32,), "float32"


def _roi_input(input, boxes):
    """Checks the RoI ops' inputs; returns boxes as a float32 Tensor[K, 5] (torchvision's convert_boxes_to_roi_format)."""
    _check_tensor("input", input, _MAP_DTYPES, _MAP_WHAT)
    if input.dim() != 4:
        raise ValueError("input must be [N, C, H, W], got shape %s" % (tuple(input.shape),))
    dtypes, what = _box_dtypes(input)
    if isinstance(boxes, (list, tuple)):
        for i, b in enumerate(boxes):
            _check_tensor("boxes[%d]" % i, b, dtypes, what)
            _check_same_device(input, b, "input", "boxes[%d]" % i)
            if b.dim() != 2 or b.shape[1] != 4:
                raise ValueError("boxes[%d] must be [L, 4], got shape %s" % (i, tuple(b.shape)))
        if not boxes:
            return input.new_zeros((0, 5), dtype=torch.float32)
        boxes = [b.float() for b in boxes]
        return torch.cat([torch.cat([torch.full_like(b[:, :1], float(i)), b], dim=1) for i, b in enumerate(boxes)], dim=0)
    _check_tensor("boxes", boxes, dtypes, what)
    _check_same_device(input, boxes, "input", "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 5:
        raise ValueError("boxes must be a Tensor[K, 5] (batch index, x1, y1, x2, y2) or a list of Tensor[L, 4], got shape %s"
                         % (tuple(boxes.shape),))
    return boxes.float()


def _input_is_channels_last(x):
    return x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=_CL)


# ---- layout helpers of the real implementations ------------------------------------------------------------------------------------
def _elem(dtype):
    """The frcnn_ops_*_16 element-type code of a 16-bit dtype; None for float32 (the frcnn_ops_* entry points)."""
    return {torch.float16: nv.OPS_F16, torch.bfloat16: nv.OPS_BF16}.get(dtype)


def _call(name, like, *args):
    """frcnn_ops_<name> on float32 tensors, frcnn_ops_<name>_16 with the element-type code first on 16-bit ones."""
    e = _elem(like.dtype)
    if e is None:
        nv.check(getattr(nv.lib(), "frcnn_ops_" + name)(*args), "frcnn_ops_" + name)
    else:
        nv.check(getattr(nv.lib(), "frcnn_ops_%s_16" % name)(e, *args), "frcnn_ops_%s_16" % name)


def _padded_channels(c, dtype):
    """c rounded up to the channels a lane of the dtype's kernels owns: 4 floats, frcnn_ops_half_run() 16-bit values."""
    v = nv.lib().frcnn_ops_half_run() if dtype in _HALF else 4
    return (c + v - 1) // v * v


def _nhwc(x, fill=0, like=None):
    """x [A, C, B, D] as a channels_last tensor with C padded for the kernels of like's dtype (x's own by default); no copy when x
    already is one."""
    c = x.shape[1]
    cp = _padded_channels(c, (x if like is None else like).dtype)
    if cp == c:
        return x.contiguous(memory_format=_CL)
    xp = torch.full((x.shape[0], cp) + tuple(x.shape[2:]), fill, dtype=x.dtype, device=x.device).contiguous(memory_format=_CL)
    xp[:, :c].copy_(x)
    return xp


def _empty_cl(shape, like, dtype=None):
    return torch.empty(shape, dtype=like.dtype if dtype is None else dtype, device=like.device, memory_format=_CL)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _format(t, channels_last):
    return t.contiguous(memory_format=_CL if channels_last else torch.contiguous_format)


def _grad_layout(dx, c, channels_last):
    return _format(dx[:, :c], channels_last)


def _grad_empty(shape, like, channels_last):
    return torch.empty(shape, dtype=like.dtype, device=like.device, memory_format=_CL if channels_last else torch.contiguous_format)


# ---- the host-side scaffolds the operators share ------------------------------------------------------------------------------------
def _register_autograd(name, backward, setup):
    """frcnn::<name> differentiates through `backward`; frcnn::<name>_backward is not differentiable."""
    def double_backward(ctx, *grads):
        raise RuntimeError("frcnn::%s: double backward is not supported (the backward of frcnn::%s is not differentiable)" % (name, name))
    torch.library.register_autograd("frcnn::" + name, backward, setup_context=setup)
    torch.library.register_autograd("frcnn::%s_backward" % name, double_backward, setup_context=lambda ctx, inputs, output: None)


def _workspace(getter, like, *args):
    """A buffer of frcnn_ops_<getter>_workspace_bytes(*args) on like's device (the allocator's alignment covers the kernels'); a size
    of 0 is the library refusing the arguments."""
    name = "frcnn_ops_%s_workspace_bytes" % getter
    size = getattr(nv.lib(), name)(*args)
    if size == 0:
        raise nv.FrcnnError(-1, name)
    return torch.empty((size,), dtype=torch.uint8, device=like.device)


def _placeholder(grad):
    """What a `needs`-style backward returns for a gradient that is not wanted: it costs nothing."""
    return grad.new_empty((0,))


def _needs_fake(grad, tensors, needs):
    """The fake result of a `needs`-style backward whose gradients are contiguous and in their arguments' dtypes."""
    return [torch.empty(t.shape, dtype=t.dtype, device=t.device) if need else _placeholder(grad) for t, need in zip(tensors, needs)]


def _chunks(n, step):
    """(first image, images) of each chunk of at most `step` of n images."""
    nb = min(n, step)
    for i0 in range(0, n, nb):
        yield i0, min(nb, n - i0)


def _sorted_gather(plan, gather, entries, device):
    """The deterministic scatter of the sampler backwards: plan(keys, weights) fills `entries` int64 keys and float32 weights, the keys
    are sorted stably, gather(sorted keys, order, weights) sums each cell's run.  All arguments of the two call-backs are pointers.
    Returns the four buffers: the caller holds them until its next chunk or its end, so that the allocator does not hand pieces of
    these large blocks to the small tensors the caller makes next."""
    keys = torch.empty((entries,), dtype=torch.int64, device=device)
    wts = torch.empty((entries,), dtype=torch.float32, device=device)
    plan(keys.data_ptr(), wts.data_ptr())
    sorted_keys, order = torch.sort(keys, stable=True)
    gather(sorted_keys.data_ptr(), order.data_ptr(), wts.data_ptr())
    return keys, wts, sorted_keys, order


# ---- frcnn::roi_align -------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("frcnn::roi_align", mutates_args=())
def _roi_align(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, sampling_ratio: int,
               aligned: bool) -> Tensor:
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), input)
    if k == 0 or c == 0:
        return out
    if n * h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x = _nhwc(input)
        r = rois.contiguous()
        cp = x.shape[1]
        dst = out if cp == c else _empty_cl((k, cp, pooled_height, pooled_width), input)
        _call("roi_align", input, x.data_ptr(), n, h, w, cp, r.data_ptr(), k, pooled_height, pooled_width, spatial_scale, sampling_ratio,
              int(aligned), dst.data_ptr(), _stream(input))
        if dst is not out:
            out.copy_(dst[:, :c])
    return out


@_roi_align.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, aligned):
    return _empty_cl((rois.shape[0], input.shape[1], pooled_height, pooled_width), input)


@torch.library.custom_op("frcnn::roi_align_backward", mutates_args=())
def _roi_align_backward(grad: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, sampling_ratio: int,
                        aligned: bool, batch_size: int, channels: int, height: int, width: int, channels_last: bool) -> Tensor:
    k = rois.shape[0]
    if channels == 0 or batch_size * height * width == 0:
        return _grad_layout(grad.new_zeros((batch_size, channels, height, width)), channels, channels_last)
    with torch.cuda.device(grad.device):
        cp = _padded_channels(channels, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        dx = _empty_cl((batch_size, cp, height, width), grad)
        _call("roi_align_backward", grad, r.data_ptr() if k else None, k, batch_size, height, width, cp, pooled_height, pooled_width,
              spatial_scale, sampling_ratio, int(aligned), g.data_ptr() if k else None, dx.data_ptr(), _stream(grad))
        return _grad_layout(dx, channels, channels_last)


@_roi_align_backward.register_fake
def _(grad, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, aligned, batch_size, channels, height, width, channels_last):
    return _grad_empty((batch_size, channels, height, width), grad, channels_last)


def _roi_setup(ctx, inputs, output):
    """Of an op (input, rois, *args) whose one gradient is the map's: what its backward op takes after (grad, rois)."""
    ctx.save_for_backward(inputs[1])
    ctx.args = tuple(inputs[2:])
    ctx.shape = tuple(inputs[0].shape)
    ctx.channels_last = _input_is_channels_last(inputs[0])


def _roi_align_bwd(ctx, grad):
    rois, = ctx.saved_tensors
    return (_roi_align_backward(grad, rois, *ctx.args, *ctx.shape, ctx.channels_last),) + (None,) * 6


_register_autograd("roi_align", _roi_align_bwd, _roi_setup)


# ---- frcnn::multi_scale_roi_align -------------------------------------------------------------------------------------------------
def _ms_levels(heights, widths, scales):
    n = len(scales)
    return (C.c_int * n)(*heights), (C.c_int * n)(*widths), (C.c_float * n)(*scales)


@torch.library.custom_op("frcnn::multi_scale_roi_align", mutates_args=())
def _ms_roi_align(features: List[Tensor], rois: Tensor, scales: List[float], pooled_height: int, pooled_width: int, sampling_ratio: int,
                  canonical_scale: float, canonical_level: float, k_min: int, k_max: int) -> Tensor:
    x0 = features[0]
    n, c = x0.shape[:2]
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), x0)
    if k == 0 or c == 0:
        return out
    if n == 0:
        return out.zero_()
    with torch.cuda.device(x0.device):
        xs = [_nhwc(f) for f in features]
        r = rois.contiguous()
        cp = xs[0].shape[1]
        dst = out if cp == c else _empty_cl((k, cp, pooled_height, pooled_width), x0)
        hs, ws, sc = _ms_levels([f.shape[2] for f in features], [f.shape[3] for f in features], scales)
        ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        _call("ms_roi_align", x0, ptrs, hs, ws, sc, len(xs), n, cp, r.data_ptr(), k, pooled_height, pooled_width, sampling_ratio,
              canonical_scale, canonical_level, k_min, k_max, dst.data_ptr(), _stream(x0))
        if dst is not out:
            out.copy_(dst[:, :c])
    return out


@_ms_roi_align.register_fake
def _(features, rois, scales, pooled_height, pooled_width, sampling_ratio, canonical_scale, canonical_level, k_min, k_max):
    return _empty_cl((rois.shape[0], features[0].shape[1], pooled_height, pooled_width), features[0])


@torch.library.custom_op("frcnn::multi_scale_roi_align_backward", mutates_args=())
def _ms_roi_align_backward(grad: Tensor, rois: Tensor, scales: List[float], pooled_height: int, pooled_width: int, sampling_ratio: int,
                           canonical_scale: float, canonical_level: float, k_min: int, k_max: int, batch_size: int, channels: int,
                           heights: List[int], widths: List[int], channels_last: List[bool]) -> List[Tensor]:
    if channels == 0 or batch_size == 0:
        return [_grad_layout(grad.new_zeros((batch_size, channels, h, w)), channels, cl)
                for h, w, cl in zip(heights, widths, channels_last)]
    k = rois.shape[0]
    with torch.cuda.device(grad.device):
        cp = _padded_channels(channels, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        dxs = [_empty_cl((batch_size, cp, h, w), grad) for h, w in zip(heights, widths)]
        lib = nv.lib()
        ws = torch.empty((lib.frcnn_ops_ms_roi_align_workspace_bytes(k, len(scales), batch_size),), dtype=torch.uint8, device=grad.device)
        hs, wd, sc = _ms_levels(heights, widths, scales)
        ptrs = (C.c_void_p * len(dxs))(*[d.data_ptr() for d in dxs])
        _call("ms_roi_align_backward", grad, r.data_ptr() if k else None, k, hs, wd, sc, len(scales), batch_size, cp, pooled_height,
              pooled_width, sampling_ratio, canonical_scale, canonical_level, k_min, k_max, g.data_ptr() if k else None, ptrs,
              ws.data_ptr(), ws.numel(), _stream(grad))
        return [_grad_layout(d, channels, cl) for d, cl in zip(dxs, channels_last)]


@_ms_roi_align_backward.register_fake
def _(grad, rois, scales, pooled_height, pooled_width, sampling_ratio, canonical_scale, canonical_level, k_min, k_max, batch_size, channels,
      heights, widths, channels_last):
    return [_grad_empty((batch_size, channels, h, w), grad, cl) for h, w, cl in zip(heights, widths, channels_last)]


def _ms_roi_align_setup(ctx, inputs, output):
    features, rois = inputs[:2]
    ctx.save_for_backward(rois)
    ctx.args = tuple(inputs[2:])
    ctx.shape = tuple(features[0].shape[:2])
    ctx.heights = [f.shape[2] for f in features]
    ctx.widths = [f.shape[3] for f in features]
    ctx.channels_last = [_input_is_channels_last(f) for f in features]


def _ms_roi_align_bwd(ctx, grad):
    rois, = ctx.saved_tensors
    n, c = ctx.shape
    dxs = _ms_roi_align_backward(grad, rois, *ctx.args, n, c, ctx.heights, ctx.widths, ctx.channels_last)
    return (list(dxs),) + (None,) * 9


_register_autograd("multi_scale_roi_align", _ms_roi_align_bwd, _ms_roi_align_setup)


# ---- frcnn::roi_pool --------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("frcnn::roi_pool", mutates_args=())
def _roi_pool(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int) -> tuple[Tensor, Tensor]:
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), input)
    argmax = _empty_cl((k, c, pooled_height, pooled_width), input, torch.int32)
    if k == 0 or c == 0:
        return out, argmax
    if n * h * w == 0:
        return out.zero_(), argmax.fill_(-1)
    with torch.cuda.device(input.device):
        x = _nhwc(input)
        r = rois.contiguous()
        cp = x.shape[1]
        padded = cp != c
        dst = _empty_cl((k, cp, pooled_height, pooled_width), input) if padded else out
        am = _empty_cl((k, cp, pooled_height, pooled_width), input, torch.int32) if padded else argmax
        _call("roi_pool", input, x.data_ptr(), n, h, w, cp, r.data_ptr(), k, pooled_height, pooled_width, spatial_scale, dst.data_ptr(),
              am.data_ptr(), _stream(input))
        if padded:
            out.copy_(dst[:, :c])
            argmax.copy_(am[:, :c])
    return out, argmax


@_roi_pool.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width):
    shape = (rois.shape[0], input.shape[1], pooled_height, pooled_width)
    return _empty_cl(shape, input), _empty_cl(shape, input, torch.int32)


@torch.library.custom_op("frcnn::roi_pool_backward", mutates_args=())
def _roi_pool_backward(grad: Tensor, rois: Tensor, argmax: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int,
                       batch_size: int, channels: int, height: int, width: int, channels_last: bool) -> Tensor:
    k = rois.shape[0]
    if channels == 0 or batch_size * height * width == 0:
        return _grad_layout(grad.new_zeros((batch_size, channels, height, width)), channels, channels_last)
    with torch.cuda.device(grad.device):
        cp = _padded_channels(channels, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        am = _nhwc(argmax, fill=-1, like=grad)
        dx = _empty_cl((batch_size, cp, height, width), grad)
        _call("roi_pool_backward", grad, r.data_ptr() if k else None, k, batch_size, height, width, cp, pooled_height, pooled_width,
              spatial_scale, am.data_ptr() if k else None, g.data_ptr() if k else None, dx.data_ptr(), _stream(grad))
        return _grad_layout(dx, channels, channels_last)


@_roi_pool_backward.register_fake
def _(grad, rois, argmax, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width, channels_last):
    return _grad_empty((batch_size, channels, height, width), grad, channels_last)


def _roi_pool_setup(ctx, inputs, output):
    input, rois, spatial_scale, pooled_height, pooled_width = inputs
    ctx.save_for_backward(rois, output[1])
    ctx.args = (spatial_scale, pooled_height, pooled_width)
    ctx.shape = tuple(input.shape)
    ctx.channels_last = _input_is_channels_last(input)


def _roi_pool_bwd(ctx, grad, grad_argmax):
    rois, argmax = ctx.saved_tensors
    n, c, h, w = ctx.shape
    dx = _roi_pool_backward(grad, rois, argmax, *ctx.args, n, c, h, w, ctx.channels_last)
    return dx, None, None, None, None


_register_autograd("roi_pool", _roi_pool_bwd, _roi_pool_setup)


# ---- frcnn::ps_roi_pool, frcnn::ps_roi_align (plain NCHW in and out) --------------------------------------------------------------
def _ps_forward(name, input, rois, pooled_height, pooled_width, *args):
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = torch.empty((k, c // (pooled_height * pooled_width), pooled_height, pooled_width), dtype=input.dtype, device=input.device)
    if k == 0 or c == 0:
        return out
    if n * h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x = input.contiguous()
        r = rois.contiguous()
        _call(name, input, x.data_ptr(), n, h, w, c, r.data_ptr(), k, pooled_height, pooled_width, *args, out.data_ptr(), _stream(input))
    return out


def _ps_backward(name, grad, rois, pooled_height, pooled_width, batch_size, channels, height, width, channels_last, *args):
    k = rois.shape[0]
    if channels == 0 or batch_size * height * width == 0:
        return _grad_layout(grad.new_zeros((batch_size, channels, height, width)), channels, channels_last)
    with torch.cuda.device(grad.device):
        g = grad.contiguous()
        r = rois.contiguous()
        dx = torch.empty((batch_size, channels, height, width), dtype=grad.dtype, device=grad.device)
        _call(name, grad, r.data_ptr() if k else None, k, batch_size, height, width, channels, pooled_height, pooled_width, *args,
              g.data_ptr() if k else None, dx.data_ptr(), _stream(grad))
        return _grad_layout(dx, channels, channels_last)


def _ps_fake(input, rois, pooled_height, pooled_width):
    return input.new_empty((rois.shape[0], input.shape[1] // (pooled_height * pooled_width), pooled_height, pooled_width))


@torch.library.custom_op("frcnn::ps_roi_pool", mutates_args=())
def _ps_roi_pool(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int) -> Tensor:
    return _ps_forward("ps_roi_pool", input, rois, pooled_height, pooled_width, spatial_scale)


@_ps_roi_pool.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width):
    return _ps_fake(input, rois, pooled_height, pooled_width)


@torch.library.custom_op("frcnn::ps_roi_pool_backward", mutates_args=())
def _ps_roi_pool_backward(grad: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, batch_size: int,
                          channels: int, height: int, width: int, channels_last: bool) -> Tensor:
    return _ps_backward("ps_roi_pool_backward", grad, rois, pooled_height, pooled_width, batch_size, channels, height, width, channels_last,
                        spatial_scale)


@_ps_roi_pool_backward.register_fake
def _(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width, channels_last):
    return _grad_empty((batch_size, channels, height, width), grad, channels_last)


@torch.library.custom_op("frcnn::ps_roi_align", mutates_args=())
def _ps_roi_align(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, sampling_ratio: int) -> Tensor:
    return _ps_forward("ps_roi_align", input, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio)


@_ps_roi_align.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    return _ps_fake(input, rois, pooled_height, pooled_width)


@torch.library.custom_op("frcnn::ps_roi_align_backward", mutates_args=())
def _ps_roi_align_backward(grad: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, sampling_ratio: int,
                           batch_size: int, channels: int, height: int, width: int, channels_last: bool) -> Tensor:
    return _ps_backward("ps_roi_align_backward", grad, rois, pooled_height, pooled_width, batch_size, channels, height, width,
                        channels_last, spatial_scale, sampling_ratio)


@_ps_roi_align_backward.register_fake
def _(grad, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, batch_size, channels, height, width, channels_last):
    return _grad_empty((batch_size, channels, height, width), grad, channels_last)


def _ps_roi_pool_bwd(ctx, grad):
    rois, = ctx.saved_tensors
    return (_ps_roi_pool_backward(grad, rois, *ctx.args, *ctx.shape, ctx.channels_last),) + (None,) * 4


def _ps_roi_align_bwd(ctx, grad):
    rois, = ctx.saved_tensors
    return (_ps_roi_align_backward(grad, rois, *ctx.args, *ctx.shape, ctx.channels_last),) + (None,) * 5


_register_autograd("ps_roi_pool", _ps_roi_pool_bwd, _roi_setup)
_register_autograd("ps_roi_align", _ps_roi_align_bwd, _roi_setup)


# ---- frcnn::deform_conv2d (plain NCHW; csrc/ops_deform.hip) ------------------------------------------------------------------------
def _deform_output_size(h, w, kh, kw, stride, padding, dilation):
    oh = (h + 2 * padding[0] - (dilation[0] * (kh - 1) + 1)) // stride[0] + 1
    ow = (w + 2 * padding[1] - (dilation[1] * (kw - 1) + 1)) // stride[1] + 1
    return oh, ow


def _deform_geom(input, offset, weight, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w):
    c, h, w = input.shape[1:]
    co, cg, kh, kw = weight.shape
    return nv.DeformGeom(c, h, w, co, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, c // cg,
                         offset.shape[1] // (2 * kh * kw))


def _opt_ptr(t, i0=0):
    return None if t is None else t[i0:].data_ptr()


def _deform_call(like):
    """call(name, *args): frcnn_ops_deform_<name> for float32 tensors, frcnn_ops_deform_<name>_16 with the element-type code first for
    16-bit ones; the value comes back (a status, checked, or workspace bytes)."""
    e = _elem(like.dtype)
    lib = nv.lib()

    def call(name, *args):
        full = "frcnn_ops_deform_" + name + ("" if e is None else "_16")
        rc = getattr(lib, full)(*(args if e is None else (e,) + args))
        if name != "workspace_bytes":
            nv.check(rc, full)
        elif rc == 0:
            raise nv.FrcnnError(-1, full)
        return rc
    return call


def _deform_buffer(call, like, ref, images, stage):
    return torch.empty((call("workspace_bytes", ref, images, stage),), dtype=torch.uint8, device=like.device)


def _opt_contiguous(t):
    return None if t is None else t.contiguous()


@torch.library.custom_op("frcnn::deform_conv2d", mutates_args=())
def _deform_conv2d(input: Tensor, offset: Tensor, weight: Tensor, bias: Optional[Tensor], mask: Optional[Tensor], stride_h: int,
                   stride_w: int, pad_h: int, pad_w: int, dilation_h: int, dilation_w: int, chunk: int) -> Tensor:
    n = input.shape[0]
    co = weight.shape[0]
    out = torch.empty((n, co) + tuple(offset.shape[2:]), dtype=input.dtype, device=input.device)
    if n == 0 or co == 0:
        return out
    with torch.cuda.device(input.device):
        geom = _deform_geom(input, offset, weight, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w)
        x, off, wgt, b, m = input.contiguous(), offset.contiguous(), weight.contiguous(), _opt_contiguous(bias), _opt_contiguous(mask)
        nb = min(n, chunk)
        call = _deform_call(input)
        ws = _deform_buffer(call, input, C.byref(geom), nb, nv.DEFORM_WS_FORWARD)
        for i0 in range(0, n, nb):
            call("forward", C.byref(geom), min(nb, n - i0), x[i0:].data_ptr(), off[i0:].data_ptr(), _opt_ptr(m, i0), wgt.data_ptr(),
                 _opt_ptr(b), out[i0:].data_ptr(), ws.data_ptr(), ws.numel(), _stream(input))
    return out


@_deform_conv2d.register_fake
def _(input, offset, weight, bias, mask, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, chunk):
    return input.new_empty((input.shape[0], weight.shape[0]) + tuple(offset.shape[2:]))


def _deform_grad_shapes(grad, input, offset, weight, mask, needs, channels_last):
    """(shape or None, channels_last) of d_input, d_offset, d_weight, d_bias, d_mask; None: not asked for (an empty placeholder)."""
    shapes = [tuple(input.shape), tuple(offset.shape), tuple(weight.shape), (weight.shape[0],), None if mask is None else tuple(mask.shape)]
    formats = [channels_last[0], channels_last[1], channels_last[2], False, channels_last[3]]
    return [(s if need else None, cl) for s, need, cl in zip(shapes, needs, formats)]


@torch.library.custom_op("frcnn::deform_conv2d_backward", mutates_args=())
def _deform_conv2d_backward(grad: Tensor, input: Tensor, offset: Tensor, weight: Tensor, mask: Optional[Tensor], stride_h: int,
                            stride_w: int, pad_h: int, pad_w: int, dilation_h: int, dilation_w: int, chunk: int, needs: List[bool],
                            channels_last: List[bool]) -> List[Tensor]:
    """[d_input, d_offset, d_weight, d_bias, d_mask]; needs: which of them are wanted (the others come back as empty placeholders and
    cost nothing); channels_last: the memory format of input, offset, weight and mask, which their gradients take."""
    plan = _deform_grad_shapes(grad, input, offset, weight, mask, needs, channels_last)
    n = input.shape[0]
    co, _, kh, kw = weight.shape
    if n == 0 or co == 0:
        return [_placeholder(grad) if s is None else _grad_layout(grad.new_zeros(s), s[1], cl) if len(s) == 4 else grad.new_zeros(s)
                for s, cl in plan]
    want_input, want_offset, want_weight, want_bias, want_mask = [s is not None for s, _ in plan]
    with torch.cuda.device(grad.device):
        geom = _deform_geom(input, offset, weight, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w)
        g, x, off, wgt, m = grad.contiguous(), input.contiguous(), offset.contiguous(), weight.contiguous(), _opt_contiguous(mask)
        new = lambda want, like: torch.empty(like.shape, dtype=like.dtype, device=like.device) if want else None   # noqa: E731
        dx, doff, dm = new(want_input, x), new(want_offset, off), new(want_mask, m)
        # the 16-bit kernels add the chunks of d_weight in a float32 buffer, rounded once after the last chunk
        dw = torch.empty(wgt.shape, dtype=torch.float32, device=wgt.device) if want_weight else None
        call, stream, ref = _deform_call(grad), _stream(grad), C.byref(geom)
        stage = lambda which: _deform_buffer(call, grad, ref, min(n, chunk), which)                                  # noqa: E731
        want_columns = want_input or want_offset or want_mask
        if want_columns:
            dcol = stage(nv.DEFORM_WS_COLUMNS)
            ws_col = stage(nv.DEFORM_WS_BACKWARD_COLUMNS)
        if want_input:
            ws_in = stage(nv.DEFORM_WS_BACKWARD_INPUT)
        if want_weight:
            ws_w = stage(nv.DEFORM_WS_BACKWARD_WEIGHT)
        samples = geom.offset_groups * kh * kw * offset.shape[2] * offset.shape[3]          # per image
        for i0, k in _chunks(n, chunk):
            if want_columns:
                call("backward_columns", ref, k, wgt.data_ptr(), g[i0:].data_ptr(), dcol.data_ptr(), ws_col.data_ptr(), ws_col.numel(), stream)
            if want_offset or want_mask:
                call("backward_offset", ref, k, x[i0:].data_ptr(), off[i0:].data_ptr(), _opt_ptr(m, i0), dcol.data_ptr(), _opt_ptr(doff, i0),
                     _opt_ptr(dm, i0), stream)
            if want_input:
                def fill(keys, wts):
                    call("input_plan", ref, k, off[i0:].data_ptr(), _opt_ptr(m, i0), keys, wts, stream)

                def gather(keys, order, wts):
                    call("backward_input", ref, k, keys, order, wts, dcol.data_ptr(), dx[i0:].data_ptr(), ws_in.data_ptr(), ws_in.numel(),
                         stream)
                held = _sorted_gather(fill, gather, k * samples * 4, grad.device)       # noqa: F841 (kept alive)
            if want_weight:
                call("backward_weight", ref, k, x[i0:].data_ptr(), off[i0:].data_ptr(), _opt_ptr(m, i0), g[i0:].data_ptr(), dw.data_ptr(),
                     int(i0 > 0), ws_w.data_ptr(), ws_w.numel(), stream)
        if want_weight:
            dw = dw.to(grad.dtype)
        db = g.sum((0, 2, 3), dtype=torch.float32).to(grad.dtype) if want_bias else None
        return [_placeholder(grad) if t is None else _grad_layout(t, t.shape[1], cl) if t.dim() == 4 else t
                for t, (_, cl) in zip((dx, doff, dw, db, dm), plan)]


@_deform_conv2d_backward.register_fake
def _(grad, input, offset, weight, mask, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, chunk, needs, channels_last):
    return [_placeholder(grad) if s is None else _grad_empty(s, grad, cl) if len(s) == 4 else grad.new_empty(s)
            for s, cl in _deform_grad_shapes(grad, input, offset, weight, mask, needs, channels_last)]


def _deform_setup(ctx, inputs, output):
    input, offset, weight, bias, mask = inputs[:5]
    ctx.save_for_backward(input, offset, weight, mask)
    ctx.args = tuple(inputs[5:])
    ctx.channels_last = [_input_is_channels_last(t) if t is not None else False for t in (input, offset, weight, mask)]


def _deform_bwd(ctx, grad):
    input, offset, weight, mask = ctx.saved_tensors
    needs = [bool(v) for v in ctx.needs_input_grad[:5]]                     # input, offset, weight, bias, mask
    grads = _deform_conv2d_backward(grad, input, offset, weight, mask, *ctx.args, needs, ctx.channels_last)
    return tuple(g if need else None for g, need in zip(grads, needs)) + (None,) * 7


_register_autograd("deform_conv2d", _deform_bwd, _deform_setup)


# ---- frcnn::deform_roi_pool (NHWC as roi_align; csrc/ops_droi.hip) -----------------------------------------------------------------
def _droi_offset(offset):
    """The offset as the kernels read it: float32, contiguous [K, 2, oh, ow]; None stays None."""
    return None if offset is None else offset.float().contiguous()


@torch.library.custom_op("frcnn::deform_roi_pool", mutates_args=())
def _deform_roi_pool(input: Tensor, rois: Tensor, offset: Optional[Tensor], spatial_scale: float, pooled_height: int, pooled_width: int,
                     sampling_ratio: int, gamma: float) -> Tensor:
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), input)
    if k == 0 or c == 0:
        return out
    if n * h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x = _nhwc(input)
        r = rois.contiguous()
        off = _droi_offset(offset)
        cp = x.shape[1]
        dst = out if cp == c else _empty_cl((k, cp, pooled_height, pooled_width), input)
        _call("deform_roi_pool", input, x.data_ptr(), n, h, w, cp, r.data_ptr(), _opt_ptr(off), k, pooled_height, pooled_width,
              spatial_scale, sampling_ratio, gamma, dst.data_ptr(), _stream(input))
        if dst is not out:
            out.copy_(dst[:, :c])
    return out


@_deform_roi_pool.register_fake
def _(input, rois, offset, spatial_scale, pooled_height, pooled_width, sampling_ratio, gamma):
    return _empty_cl((rois.shape[0], input.shape[1], pooled_height, pooled_width), input)


@torch.library.custom_op("frcnn::deform_roi_pool_backward", mutates_args=())
def _deform_roi_pool_backward(grad: Tensor, input: Tensor, rois: Tensor, offset: Optional[Tensor], spatial_scale: float,
                              pooled_height: int, pooled_width: int, sampling_ratio: int, gamma: float, needs: List[bool],
                              channels_last: List[bool]) -> List[Tensor]:
    """[d_input, d_offset]; needs: which of them are wanted (the other comes back as an empty placeholder and costs nothing);
    channels_last: the memory format of input and offset, which their gradients take.  d_offset is in the offset's dtype."""
    n, c, h, w = input.shape
    k = rois.shape[0]
    want_input, want_offset = needs[0], needs[1] and offset is not None
    if k == 0 or c == 0 or n * h * w == 0:
        return [_grad_layout(grad.new_zeros((n, c, h, w)), c, channels_last[0]) if want_input else _placeholder(grad),
                _format(torch.zeros_like(offset), channels_last[1]) if want_offset else _placeholder(grad)]
    if not (want_input or want_offset):
        return [_placeholder(grad), _placeholder(grad)]
    with torch.cuda.device(grad.device):
        cp = _padded_channels(c, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        off = _droi_offset(offset)
        x = _nhwc(input) if want_offset else None
        dx = _empty_cl((n, cp, h, w), grad) if want_input else None
        doff = torch.empty_like(off) if want_offset else None
        ws = _workspace("deform_roi_pool", grad, k, pooled_height, pooled_width) if want_input else None
        _call("deform_roi_pool_backward", grad, _opt_ptr(x), r.data_ptr(), _opt_ptr(off), k, n, h, w, cp, pooled_height, pooled_width,
              spatial_scale, sampling_ratio, gamma, g.data_ptr(), _opt_ptr(dx), _opt_ptr(doff), _opt_ptr(ws), 0 if ws is None else ws.numel(),
              _stream(grad))
        return [_grad_layout(dx, c, channels_last[0]) if want_input else _placeholder(grad),
                _format(doff.to(offset.dtype), channels_last[1]) if want_offset else _placeholder(grad)]


@_deform_roi_pool_backward.register_fake
def _(grad, input, rois, offset, spatial_scale, pooled_height, pooled_width, sampling_ratio, gamma, needs, channels_last):
    return [_grad_empty(tuple(input.shape), grad, channels_last[0]) if needs[0] else _placeholder(grad),
            _format(torch.empty_like(offset), channels_last[1]) if needs[1] and offset is not None else _placeholder(grad)]


def _deform_roi_pool_setup(ctx, inputs, output):
    input, rois, offset = inputs[:3]
    ctx.save_for_backward(input, rois, offset)
    ctx.args = tuple(inputs[3:])
    ctx.channels_last = [_input_is_channels_last(input), offset is not None and _input_is_channels_last(offset)]


def _deform_roi_pool_bwd(ctx, grad):
    input, rois, offset = ctx.saved_tensors
    needs = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[2]) and offset is not None]
    dx, doff = _deform_roi_pool_backward(grad, input, rois, offset, *ctx.args, needs, ctx.channels_last)
    return (dx if needs[0] else None, None, doff if needs[1] else None) + (None,) * 5


_register_autograd("deform_roi_pool", _deform_roi_pool_bwd, _deform_roi_pool_setup)


# ---- frcnn::prroi_pool (NHWC as roi_align; csrc/ops_prroi.hip) ----------------------------------------------------------------------
@torch.library.custom_op("frcnn::prroi_pool", mutates_args=())
def _prroi_pool(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int) -> Tensor:
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), input)
    if k == 0 or c == 0:
        return out
    if n * h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x = _nhwc(input)
        r = rois.contiguous()
        cp = x.shape[1]
        dst = out if cp == c else _empty_cl((k, cp, pooled_height, pooled_width), input)
        _call("prroi_pool", input, x.data_ptr(), n, h, w, cp, r.data_ptr(), k, pooled_height, pooled_width, spatial_scale, dst.data_ptr(),
              _stream(input))
        if dst is not out:
            out.copy_(dst[:, :c])
    return out


@_prroi_pool.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width):
    return _empty_cl((rois.shape[0], input.shape[1], pooled_height, pooled_width), input)


@torch.library.custom_op("frcnn::prroi_pool_backward", mutates_args=())
def _prroi_pool_backward(grad: Tensor, input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int,
                         needs: List[bool], channels_last: bool) -> List[Tensor]:
    """[d_input, d_rois]; needs: which of them are wanted (the other comes back as an empty placeholder and costs nothing);
    channels_last: the memory format of input, which its gradient takes.  d_rois is float32 [K, 5] with a zero column 0."""
    n, c, h, w = input.shape
    k = rois.shape[0]
    if k == 0 or c == 0 or n * h * w == 0:
        return [_grad_layout(grad.new_zeros((n, c, h, w)), c, channels_last) if needs[0] else _placeholder(grad),
                torch.zeros_like(rois) if needs[1] else _placeholder(grad)]
    if not (needs[0] or needs[1]):
        return [_placeholder(grad), _placeholder(grad)]
    with torch.cuda.device(grad.device):
        cp = _padded_channels(c, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        x = _nhwc(input) if needs[1] else None
        dx = _empty_cl((n, cp, h, w), grad) if needs[0] else None
        drois = torch.empty_like(r) if needs[1] else None
        ws = _workspace("prroi_pool", grad, k, pooled_height, pooled_width) if needs[1] else None
        _call("prroi_pool_backward", grad, _opt_ptr(x), r.data_ptr(), k, n, h, w, cp, pooled_height, pooled_width, spatial_scale,
              g.data_ptr(), _opt_ptr(dx), _opt_ptr(drois), _opt_ptr(ws), 0 if ws is None else ws.numel(), _stream(grad))
        return [_grad_layout(dx, c, channels_last) if needs[0] else _placeholder(grad), drois if needs[1] else _placeholder(grad)]


@_prroi_pool_backward.register_fake
def _(grad, input, rois, spatial_scale, pooled_height, pooled_width, needs, channels_last):
    return [_grad_empty(tuple(input.shape), grad, channels_last) if needs[0] else _placeholder(grad),
            torch.empty_like(rois, memory_format=torch.contiguous_format) if needs[1] else _placeholder(grad)]


def _prroi_pool_setup(ctx, inputs, output):
    input, rois = inputs[:2]
    ctx.save_for_backward(input, rois)
    ctx.args = tuple(inputs[2:])
    ctx.channels_last = _input_is_channels_last(input)


def _prroi_pool_bwd(ctx, grad):
    input, rois = ctx.saved_tensors
    needs = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
    dx, drois = _prroi_pool_backward(grad, input, rois, *ctx.args, needs, ctx.channels_last)
    return (dx if needs[0] else None, drois if needs[1] else None, None, None, None)


_register_autograd("prroi_pool", _prroi_pool_bwd, _prroi_pool_setup)


# ---- frcnn::border_align (the map NHWC with each edge group padded to whole runs; csrc/ops_border.hip) ------------------------------
def _border_groups(x, cp, fill=0):
    """x [A, 4 c, B, D] as a channels_last [A, 4 cp, B, D] tensor, each of the four edge groups padded to cp channels; no copy when x
    already is one."""
    c = x.shape[1] // 4
    if cp == c:
        return x.contiguous(memory_format=_CL)
    xp = torch.full((x.shape[0], 4 * cp) + tuple(x.shape[2:]), fill, dtype=x.dtype, device=x.device).contiguous(memory_format=_CL)
    xp.unflatten(1, (4, cp))[:, :, :c].copy_(x.unflatten(1, (4, c)))
    return xp


@torch.library.custom_op("frcnn::border_align", mutates_args=())
def _border_align(input: Tensor, boxes: Tensor, pool_size: int) -> tuple[Tensor, Tensor]:
    """(output, int32 argmax), both [N, C, K, 4] in channels_last memory ([N, K, 4, C])."""
    n, c4, h, w = input.shape
    c, k = c4 // 4, boxes.shape[1]
    out = _empty_cl((n, c, k, 4), input)
    argmax = _empty_cl((n, c, k, 4), input, torch.int32)
    if n * c * k == 0:
        return out, argmax
    if h * w == 0:
        return out.zero_(), argmax.zero_()
    with torch.cuda.device(input.device):
        cp = _padded_channels(c, input.dtype)
        x = _border_groups(input, cp)
        b = boxes.contiguous()
        padded = cp != c
        dst = _empty_cl((n, cp, k, 4), input) if padded else out
        am = _empty_cl((n, cp, k, 4), input, torch.int32) if padded else argmax
        _call("border_align", input, x.data_ptr(), n, h, w, cp, b.data_ptr(), k, pool_size, dst.data_ptr(), am.data_ptr(), _stream(input))
        if padded:
            out.copy_(dst[:, :c])
            argmax.copy_(am[:, :c])
    return out, argmax


@_border_align.register_fake
def _(input, boxes, pool_size):
    shape = (input.shape[0], input.shape[1] // 4, boxes.shape[1], 4)
    return _empty_cl(shape, input), _empty_cl(shape, input, torch.int32)


@torch.library.custom_op("frcnn::border_align_backward", mutates_args=())
def _border_align_backward(grad: Tensor, boxes: Tensor, argmax: Tensor, pool_size: int, height: int, width: int,
                           channels_last: bool) -> Tensor:
    n, c, k, _ = grad.shape
    if n * c * height * width == 0:
        return _format(grad.new_zeros((n, 4 * c, height, width)), channels_last)
    with torch.cuda.device(grad.device):
        cp = _padded_channels(c, grad.dtype)
        g = _nhwc(grad)
        am = _nhwc(argmax, like=grad)
        b = boxes.contiguous()
        dx = _empty_cl((n, 4 * cp, height, width), grad)
        _call("border_align_backward", grad, b.data_ptr() if k else None, k, n, height, width, cp, pool_size, am.data_ptr() if k else None,
              g.data_ptr() if k else None, dx.data_ptr(), _stream(grad))
        if cp != c:
            dx = dx.unflatten(1, (4, cp))[:, :, :c].flatten(1, 2)
        return _format(dx, channels_last)


@_border_align_backward.register_fake
def _(grad, boxes, argmax, pool_size, height, width, channels_last):
    return _grad_empty((grad.shape[0], 4 * grad.shape[1], height, width), grad, channels_last)


def _border_align_setup(ctx, inputs, output):
    input, boxes, pool_size = inputs
    ctx.save_for_backward(boxes, output[1])
    ctx.args = (pool_size, input.shape[2], input.shape[3])
    ctx.channels_last = _input_is_channels_last(input)


def _border_align_bwd(ctx, grad, grad_argmax):
    boxes, argmax = ctx.saved_tensors
    return _border_align_backward(grad, boxes, argmax, *ctx.args, ctx.channels_last), None, None


_register_autograd("border_align", _border_align_bwd, _border_align_setup)


# ---- frcnn::nms, frcnn::batched_nms -----------------------------------------------------------------------------------------------
def _score_order(scores):
    """The oracle's argsort(-scores, "stable"): descending score, ties in input order, NaN scores last in input order."""
    nan = torch.isnan(scores)
    order = torch.sort(torch.where(nan, 0.0, -scores), stable=True).indices
    return order[torch.sort(nan[order].to(torch.uint8), stable=True).indices]


def _nms(boxes, scores, idxs, iou_threshold, rotated=False, quadri=False):
    """The kept indices of greedy NMS, within each category of idxs when given: the sorting and merging around frcnn_ops_nms, around
    frcnn_ops_nms_rotated on boxes in the kernels' (clockwise) convention, or around frcnn_ops_nms_quadri on rows of 8 floats."""
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    with torch.cuda.device(boxes.device):
        order = _score_order(scores)
        cats = None
        if idxs is not None:
            cats = idxs.to(torch.int64).contiguous()
            order = order[torch.sort(cats[order], stable=True).indices]       # each category one run, by score inside it
        lib = nv.lib()
        ws = torch.empty((lib.frcnn_ops_nms_workspace_bytes(n),), dtype=torch.uint8, device=boxes.device)
        keep = torch.empty((n,), dtype=torch.uint8, device=boxes.device)
        b = boxes.contiguous()
        tail = (order.data_ptr(), cats.data_ptr() if cats is not None else None, n, iou_threshold, keep.data_ptr(), ws.data_ptr(), ws.numel(),
                _stream(boxes))
        if rotated:
            nv.check(lib.frcnn_ops_nms_rotated(b.data_ptr(), *tail), "frcnn_ops_nms_rotated")
        elif quadri:
            nv.check(lib.frcnn_ops_nms_quadri(b.data_ptr(), *tail), "frcnn_ops_nms_quadri")
        else:
            nv.check(lib.frcnn_ops_nms(b.data_ptr(), int(b.dtype == torch.float64), *tail), "frcnn_ops_nms")
        kept = order[keep.bool()]
        if idxs is not None:                                                   # merge: descending score, ties by ascending index
            kept = torch.sort(kept).values
            kept = kept[_score_order(scores[kept])]
        return kept


def _nms_fake_result(boxes):
    k = torch.library.get_ctx().new_dynamic_size()
    return boxes.new_empty((k,), dtype=torch.int64)


@torch.library.custom_op("frcnn::nms", mutates_args=())
def _nms_op(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    return _nms(boxes, scores, None, iou_threshold)


@_nms_op.register_fake
def _(boxes, scores, iou_threshold):
    return _nms_fake_result(boxes)


@torch.library.custom_op("frcnn::batched_nms", mutates_args=())
def _batched_nms_op(boxes: Tensor, scores: Tensor, idxs: Tensor, iou_threshold: float) -> Tensor:
    return _nms(boxes, scores, idxs, iou_threshold)


@_batched_nms_op.register_fake
def _(boxes, scores, idxs, iou_threshold):
    return _nms_fake_result(boxes)


def _nms_input(boxes, scores):
    _check_tensor("boxes", boxes, (torch.float32, torch.float64), "float32 or float64")
    _check_tensor("scores", scores, (torch.float32, torch.float64), "float32 or float64")
    _check_same_device(boxes, scores, "boxes", "scores")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("boxes must be [N, 4] (x1, y1, x2, y2), got shape %s" % (tuple(boxes.shape),))
    if scores.dim() != 1 or scores.shape[0] != boxes.shape[0]:
        raise ValueError("scores must be [N] with N = %d, got shape %s" % (boxes.shape[0], tuple(scores.shape)))
    if boxes.shape[0] > MAX_NMS_BOXES:
        raise ValueError("nms takes at most %d boxes, got %d" % (MAX_NMS_BOXES, boxes.shape[0]))


# ---- frcnn::box_iou_rotated, frcnn::nms_rotated, frcnn::roi_align_rotated (csrc/ops_rot.hip) --------------------------------------
@torch.library.custom_op("frcnn::box_iou_rotated", mutates_args=())
def _box_iou_rotated(boxes1: Tensor, boxes2: Tensor, mode: int, aligned: bool) -> Tensor:
    n, m = boxes1.shape[0], boxes2.shape[0]
    out = torch.empty((n,) if aligned else (n, m), dtype=torch.float32, device=boxes1.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(boxes1.device):
        a, b = boxes1.contiguous(), boxes2.contiguous()
        nv.check(nv.lib().frcnn_ops_box_iou_rotated(a.data_ptr(), n, b.data_ptr(), m, mode, int(aligned), out.data_ptr(), _stream(boxes1)),
                 "frcnn_ops_box_iou_rotated")
    return out


@_box_iou_rotated.register_fake
def _(boxes1, boxes2, mode, aligned):
    n, m = boxes1.shape[0], boxes2.shape[0]
    return boxes1.new_empty((n,) if aligned else (n, m), dtype=torch.float32)


@torch.library.custom_op("frcnn::diff_iou_rotated", mutates_args=())
def _diff_iou_rotated(boxes1: Tensor, boxes2: Tensor) -> Tuple[Tensor, Tensor]:
    """(iou [n], inter [n]) of the aligned pairs boxes1[i], boxes2[i] ([n, 5] each, the kernels' convention)."""
    n = boxes1.shape[0]
    iou, inter = boxes1.new_empty((n,)), boxes1.new_empty((n,))
    if n == 0:
        return iou, inter
    with torch.cuda.device(boxes1.device):
        a, b = boxes1.contiguous(), boxes2.contiguous()
        nv.check(nv.lib().frcnn_ops_diff_iou_rotated(a.data_ptr(), b.data_ptr(), n, iou.data_ptr(), inter.data_ptr(), _stream(boxes1)),
                 "frcnn_ops_diff_iou_rotated")
    return iou, inter


@_diff_iou_rotated.register_fake
def _(boxes1, boxes2):
    n = boxes1.shape[0]
    return boxes1.new_empty((n,)), boxes1.new_empty((n,))


@torch.library.custom_op("frcnn::diff_iou_rotated_backward", mutates_args=())
def _diff_iou_rotated_backward(grad_iou: Tensor, grad_inter: Tensor, boxes1: Tensor, boxes2: Tensor, needs: List[bool]) -> List[Tensor]:
    """[d_boxes1, d_boxes2] of sum(grad_iou * iou + grad_inter * inter); needs: which of them are wanted (the other comes back as an
    empty placeholder and is not written)."""
    n = boxes1.shape[0]
    if n == 0:
        return [torch.zeros_like(t, memory_format=torch.contiguous_format) if need else _placeholder(grad_iou)
                for t, need in zip((boxes1, boxes2), needs)]
    if not any(needs):
        return [_placeholder(grad_iou), _placeholder(grad_iou)]
    with torch.cuda.device(boxes1.device):
        a, b, gi, gn = boxes1.contiguous(), boxes2.contiguous(), grad_iou.contiguous(), grad_inter.contiguous()
        d1 = torch.empty_like(a) if needs[0] else None
        d2 = torch.empty_like(b) if needs[1] else None
        nv.check(nv.lib().frcnn_ops_diff_iou_rotated_backward(a.data_ptr(), b.data_ptr(), gi.data_ptr(), gn.data_ptr(), n, _opt_ptr(d1),
                                                              _opt_ptr(d2), _stream(boxes1)), "frcnn_ops_diff_iou_rotated_backward")
    return [_placeholder(grad_iou) if d is None else d for d in (d1, d2)]


@_diff_iou_rotated_backward.register_fake
def _(grad_iou, grad_inter, boxes1, boxes2, needs):
    return _needs_fake(grad_iou, (boxes1, boxes2), needs)


def _diff_iou_rotated_bwd(ctx, grad_iou, grad_inter):
    needs = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
    d1, d2 = _diff_iou_rotated_backward(grad_iou, grad_inter, *ctx.saved_tensors, needs)
    return (d1 if needs[0] else None, d2 if needs[1] else None)


_register_autograd("diff_iou_rotated", _diff_iou_rotated_bwd, lambda ctx, inputs, output: ctx.save_for_backward(*inputs))


@torch.library.custom_op("frcnn::nms_rotated", mutates_args=())
def _nms_rotated_op(boxes: Tensor, scores: Tensor, labels: Optional[Tensor], iou_threshold: float) -> Tensor:
    """The kept indices; boxes in the kernels' (clockwise) convention."""
    return _nms(boxes, scores, labels, iou_threshold, rotated=True)


@_nms_rotated_op.register_fake
def _(boxes, scores, labels, iou_threshold):
    return _nms_fake_result(boxes)


# ---- frcnn::soft_nms (csrc/ops_softnms.hip) ------------------------------------------------------------------------------------------
@torch.library.custom_op("frcnn::soft_nms", mutates_args=())
def _soft_nms_op(boxes: Tensor, scores: Tensor, labels: Optional[Tensor], iou_threshold: float, sigma: float, min_score: float,
                 method: int, offset: int) -> Tuple[Tensor, Tensor]:
    """(the final scores of the kept boxes [K], their indices int64 [K]): by descending final score, ties by ascending index, NaN last."""
    n = boxes.shape[0]
    if n == 0:
        return scores.new_empty((0,)), torch.empty((0,), dtype=torch.int64, device=boxes.device)
    with torch.cuda.device(boxes.device):
        cats = None
        if labels is not None:
            cats = labels.to(torch.int64).contiguous()
            order = torch.sort(cats, stable=True).indices                     # each label one run, ascending in the index inside it
        else:
            order = torch.arange(n, dtype=torch.int64, device=boxes.device)
        ws = _workspace("soft_nms", boxes, n)
        keep = torch.empty((n,), dtype=torch.uint8, device=boxes.device)
        out = torch.empty((n,), dtype=torch.float32, device=boxes.device)
        b, s = boxes.contiguous(), scores.contiguous()
        nv.check(nv.lib().frcnn_ops_soft_nms(b.data_ptr(), s.data_ptr(), order.data_ptr(), _opt_ptr(cats), n, iou_threshold, sigma,
                                             min_score, method, offset, out.data_ptr(), keep.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _stream(boxes)), "frcnn_ops_soft_nms")
        kept = keep.bool()
        inds, final = order[kept], out[kept]
        if cats is not None:                                                   # merge the labels: ascending index first
            inds, by_index = torch.sort(inds)
            final = final[by_index]
        rank = _score_order(final)                                             # a problem's picks already are in this order
        return final[rank], inds[rank]


@_soft_nms_op.register_fake
def _(boxes, scores, labels, iou_threshold, sigma, min_score, method, offset):
    k = torch.library.get_ctx().new_dynamic_size()
    return scores.new_empty((k,), dtype=torch.float32), boxes.new_empty((k,), dtype=torch.int64)


@torch.library.custom_op("frcnn::roi_align_rotated", mutates_args=())
def _roi_align_rotated(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, sampling_ratio: int,
                       aligned: bool, clockwise: bool) -> Tensor:
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), input)
    if k == 0 or c == 0:
        return out
    if n * h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x = _nhwc(input)
        r = rois.contiguous()
        cp = x.shape[1]
        dst = out if cp == c else _empty_cl((k, cp, pooled_height, pooled_width), input)
        _call("roi_align_rotated", input, x.data_ptr(), n, h, w, cp, r.data_ptr(), k, pooled_height, pooled_width, spatial_scale,
              sampling_ratio, int(aligned), int(clockwise), dst.data_ptr(), _stream(input))
        if dst is not out:
            out.copy_(dst[:, :c])
    return out


@_roi_align_rotated.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, aligned, clockwise):
    return _empty_cl((rois.shape[0], input.shape[1], pooled_height, pooled_width), input)


@torch.library.custom_op("frcnn::roi_align_rotated_backward", mutates_args=())
def _roi_align_rotated_backward(grad: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int,
                                sampling_ratio: int, aligned: bool, clockwise: bool, batch_size: int, channels: int, height: int,
                                width: int, channels_last: bool) -> Tensor:
    k = rois.shape[0]
    if channels == 0 or batch_size * height * width == 0:
        return _grad_layout(grad.new_zeros((batch_size, channels, height, width)), channels, channels_last)
    with torch.cuda.device(grad.device):
        cp = _padded_channels(channels, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        dx = _empty_cl((batch_size, cp, height, width), grad)
        _call("roi_align_rotated_backward", grad, r.data_ptr() if k else None, k, batch_size, height, width, cp, pooled_height,
              pooled_width, spatial_scale, sampling_ratio, int(aligned), int(clockwise), g.data_ptr() if k else None, dx.data_ptr(),
              _stream(grad))
        return _grad_layout(dx, channels, channels_last)


@_roi_align_rotated_backward.register_fake
def _(grad, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, aligned, clockwise, batch_size, channels, height, width,
      channels_last):
    return _grad_empty((batch_size, channels, height, width), grad, channels_last)


def _roi_align_rotated_bwd(ctx, grad):
    rois, = ctx.saved_tensors
    return (_roi_align_rotated_backward(grad, rois, *ctx.args, *ctx.shape, ctx.channels_last),) + (None,) * 7


_register_autograd("roi_align_rotated", _roi_align_rotated_bwd, _roi_setup)


# ---- frcnn::riroi_align_rotated (csrc/ops_rot.hip: the kernels get the padded channel count and the real one) -----------------------
@torch.library.custom_op("frcnn::riroi_align_rotated", mutates_args=())
def _riroi_align_rotated(input: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int, num_samples: int,
                         num_orientations: int, clockwise: bool) -> Tensor:
    n, c, h, w = input.shape
    k = rois.shape[0]
    out = _empty_cl((k, c, pooled_height, pooled_width), input)
    if k == 0 or c == 0:
        return out
    if n * h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x = _nhwc(input)
        r = rois.contiguous()
        cp = x.shape[1]
        dst = out if cp == c else _empty_cl((k, cp, pooled_height, pooled_width), input)
        _call("riroi_align_rotated", input, x.data_ptr(), n, h, w, cp, c, r.data_ptr(), k, pooled_height, pooled_width, spatial_scale,
              num_samples, num_orientations, int(clockwise), dst.data_ptr(), _stream(input))
        if dst is not out:
            out.copy_(dst[:, :c])
    return out


@_riroi_align_rotated.register_fake
def _(input, rois, spatial_scale, pooled_height, pooled_width, num_samples, num_orientations, clockwise):
    return _empty_cl((rois.shape[0], input.shape[1], pooled_height, pooled_width), input)


@torch.library.custom_op("frcnn::riroi_align_rotated_backward", mutates_args=())
def _riroi_align_rotated_backward(grad: Tensor, rois: Tensor, spatial_scale: float, pooled_height: int, pooled_width: int,
                                  num_samples: int, num_orientations: int, clockwise: bool, batch_size: int, channels: int, height: int,
                                  width: int, channels_last: bool) -> Tensor:
    k = rois.shape[0]
    if channels == 0 or batch_size * height * width == 0:
        return _grad_layout(grad.new_zeros((batch_size, channels, height, width)), channels, channels_last)
    with torch.cuda.device(grad.device):
        cp = _padded_channels(channels, grad.dtype)
        g = _nhwc(grad)
        r = rois.contiguous()
        dx = _empty_cl((batch_size, cp, height, width), grad)
        _call("riroi_align_rotated_backward", grad, r.data_ptr() if k else None, k, batch_size, height, width, cp, channels, pooled_height,
              pooled_width, spatial_scale, num_samples, num_orientations, int(clockwise), g.data_ptr() if k else None, dx.data_ptr(),
              _stream(grad))
        return _grad_layout(dx, channels, channels_last)


@_riroi_align_rotated_backward.register_fake
def _(grad, rois, spatial_scale, pooled_height, pooled_width, num_samples, num_orientations, clockwise, batch_size, channels, height, width,
      channels_last):
    return _grad_empty((batch_size, channels, height, width), grad, channels_last)


def _riroi_align_rotated_bwd(ctx, grad):
    rois, = ctx.saved_tensors
    return (_riroi_align_rotated_backward(grad, rois, *ctx.args, *ctx.shape, ctx.channels_last),) + (None,) * 7


_register_autograd("riroi_align_rotated", _riroi_align_rotated_bwd, _roi_setup)


# ---- frcnn::rotated_feature_align (csrc/ops_rfa.hip) ---------------------------------------------------------------------------------
@torch.library.custom_op("frcnn::rotated_feature_align", mutates_args=())
def _rotated_feature_align(features: Tensor, best_bboxes: Tensor, spatial_scale: float, points: int) -> Tensor:
    n, c, h, w = features.shape
    channels_last = _input_is_channels_last(features)
    if features.numel() == 0:
        return _grad_empty((n, c, h, w), features, channels_last)
    with torch.cuda.device(features.device):
        x = _nhwc(features)
        b = best_bboxes.contiguous()
        out = _empty_cl(tuple(x.shape), features)
        _call("rotated_feature_align", features, x.data_ptr(), b.data_ptr(), n, h, w, x.shape[1], spatial_scale, points, out.data_ptr(),
              _stream(features))
        return _grad_layout(out, c, channels_last)


@_rotated_feature_align.register_fake
def _(features, best_bboxes, spatial_scale, points):
    return _grad_empty(tuple(features.shape), features, _input_is_channels_last(features))


@torch.library.custom_op("frcnn::rotated_feature_align_backward", mutates_args=())
def _rotated_feature_align_backward(grad: Tensor, best_bboxes: Tensor, spatial_scale: float, points: int, channels_last: bool) -> Tensor:
    n, c, h, w = grad.shape
    if grad.numel() == 0:
        return _grad_empty((n, c, h, w), grad, channels_last)
    with torch.cuda.device(grad.device):
        g = _nhwc(grad)
        b = best_bboxes.contiguous()
        cp = g.shape[1]
        dx = _empty_cl((n, cp, h, w), grad)
        stream, lib = _stream(grad), nv.lib()

        def plan(keys, wts):
            nv.check(lib.frcnn_ops_rotated_feature_align_plan(b.data_ptr(), n, h, w, spatial_scale, points, keys, wts, stream),
                     "frcnn_ops_rotated_feature_align_plan")

        def gather(keys, order, wts):
            _call("rotated_feature_align_backward", grad, keys, order, wts, g.data_ptr(), n, h, w, cp, points, dx.data_ptr(), stream)
        held = _sorted_gather(plan, gather, n * h * w * points * 4, grad.device)       # noqa: F841 (kept alive)
        return _grad_layout(dx, c, channels_last)


@_rotated_feature_align_backward.register_fake
def _(grad, best_bboxes, spatial_scale, points, channels_last):
    return _grad_empty(tuple(grad.shape), grad, channels_last)


def _rotated_feature_align_setup(ctx, inputs, output):
    features, best_bboxes, spatial_scale, points = inputs
    ctx.save_for_backward(best_bboxes)
    ctx.args = (spatial_scale, points)
    ctx.channels_last = _input_is_channels_last(features)


def _rotated_feature_align_bwd(ctx, grad):
    best_bboxes, = ctx.saved_tensors
    return _rotated_feature_align_backward(grad, best_bboxes, *ctx.args, ctx.channels_last), None, None, None


_register_autograd("rotated_feature_align", _rotated_feature_align_bwd, _rotated_feature_align_setup)


# ---- frcnn::carafe (plain NCHW; csrc/ops_carafe.hip) --------------------------------------------------------------------------------
@torch.library.custom_op("frcnn::carafe", mutates_args=())
def _carafe(features: Tensor, masks: Tensor, kernel_size: int, group_size: int, scale_factor: int) -> Tensor:
    n, c, h, w = features.shape
    out = torch.empty((n, c, h * scale_factor, w * scale_factor), dtype=features.dtype, device=features.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(features.device):
        x, m = features.contiguous(), masks.contiguous()
        _call("carafe", features, x.data_ptr(), m.data_ptr(), n, c, h, w, kernel_size, group_size, scale_factor, out.data_ptr(),
              _stream(features))
    return out


@_carafe.register_fake
def _(features, masks, kernel_size, group_size, scale_factor):
    n, c, h, w = features.shape
    return features.new_empty((n, c, h * scale_factor, w * scale_factor))


@torch.library.custom_op("frcnn::carafe_backward", mutates_args=())
def _carafe_backward(grad: Tensor, features: Tensor, masks: Tensor, kernel_size: int, group_size: int, scale_factor: int,
                     needs: List[bool], channels_last: List[bool]) -> List[Tensor]:
    """[d_features, d_masks]; needs: which of them are wanted (the other comes back as an empty placeholder and costs nothing);
    channels_last: the memory format of features and masks, which their gradients take."""
    n, c, h, w = features.shape
    if grad.numel() == 0:
        return [_format(torch.zeros_like(t, memory_format=torch.contiguous_format), cl) if need else _placeholder(grad)
                for t, need, cl in zip((features, masks), needs, channels_last)]
    if not (needs[0] or needs[1]):
        return [_placeholder(grad), _placeholder(grad)]
    with torch.cuda.device(grad.device):
        g = grad.contiguous()
        x = features.contiguous() if needs[1] else None
        m = masks.contiguous() if needs[0] else None
        dx = torch.empty(features.shape, dtype=grad.dtype, device=grad.device) if needs[0] else None
        dm = torch.empty(masks.shape, dtype=grad.dtype, device=grad.device) if needs[1] else None
        _call("carafe_backward", grad, _opt_ptr(x), _opt_ptr(m), g.data_ptr(), n, c, h, w, kernel_size, group_size, scale_factor,
              _opt_ptr(dx), _opt_ptr(dm), _stream(grad))
        return [_format(t, cl) if need else _placeholder(grad) for t, need, cl in zip((dx, dm), needs, channels_last)]


@_carafe_backward.register_fake
def _(grad, features, masks, kernel_size, group_size, scale_factor, needs, channels_last):
    return [_grad_empty(tuple(t.shape), grad, cl) if need else _placeholder(grad)
            for t, need, cl in zip((features, masks), needs, channels_last)]


def _carafe_setup(ctx, inputs, output):
    features, masks = inputs[:2]
    ctx.save_for_backward(features, masks)
    ctx.args = tuple(inputs[2:])
    ctx.channels_last = [_input_is_channels_last(features), _input_is_channels_last(masks)]


def _carafe_bwd(ctx, grad):
    features, masks = ctx.saved_tensors
    needs = [bool(v) for v in ctx.needs_input_grad[:2]]
    dx, dm = _carafe_backward(grad, features, masks, *ctx.args, needs, ctx.channels_last)
    return (dx if needs[0] else None, dm if needs[1] else None, None, None, None)


_register_autograd("carafe", _carafe_bwd, _carafe_setup)


# ---- frcnn::ms_deform_attn (csrc/ops_msda.hip) ---------------------------------------------------------------------------------------
def _msda_float(t):
    """sampling_locations / attention_weights as the kernels read them: float32, contiguous."""
    return t.float().contiguous()


def _msda_dims(value, sampling_locations):
    b, s, m, d = value.shape
    q, levels, points = sampling_locations.shape[1], sampling_locations.shape[3], sampling_locations.shape[4]
    return b, s, m, d, q, levels, points


@torch.library.custom_op("frcnn::ms_deform_attn", mutates_args=())
def _ms_deform_attn(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, sampling_locations: Tensor,
                    attention_weights: Tensor, im2col_step: int) -> Tensor:
    b, s, m, d, q, levels, points = _msda_dims(value, sampling_locations)
    out = torch.empty((b, q, m * d), dtype=value.dtype, device=value.device)
    if out.numel() == 0:
        return out
    if s == 0 or levels * points == 0:
        return out.zero_()
    with torch.cuda.device(value.device):
        v, shp, st = value.contiguous(), spatial_shapes.contiguous(), level_start_index.contiguous()
        loc, attn = _msda_float(sampling_locations), _msda_float(attention_weights)
        nb, stream = min(b, im2col_step), _stream(value)
        for i0 in range(0, b, nb):
            _call("msda_forward", value, v[i0:].data_ptr(), shp.data_ptr(), st.data_ptr(), loc[i0:].data_ptr(), attn[i0:].data_ptr(),
                  min(nb, b - i0), s, m, d, q, levels, points, out[i0:].data_ptr(), stream)
    return out


@_ms_deform_attn.register_fake
def _(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step):
    return value.new_empty((value.shape[0], sampling_locations.shape[1], value.shape[2] * value.shape[3]))


@torch.library.custom_op("frcnn::ms_deform_attn_backward", mutates_args=())
def _ms_deform_attn_backward(grad: Tensor, value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, sampling_locations: Tensor,
                             attention_weights: Tensor, im2col_step: int, needs: List[bool]) -> List[Tensor]:
    """[d_value, d_sampling_locations, d_attention_weights], each in its argument's dtype; needs: which of them are wanted (the others
    come back as empty placeholders and cost nothing)."""
    b, s, m, d, q, levels, points = _msda_dims(value, sampling_locations)
    if grad.numel() == 0 or s == 0 or levels * points == 0:
        return [torch.zeros_like(t, memory_format=torch.contiguous_format) if need else _placeholder(grad)
                for t, need in zip((value, sampling_locations, attention_weights), needs)]
    if not any(needs):
        return [_placeholder(grad) for _ in needs]
    with torch.cuda.device(grad.device):
        g, shp, st = grad.contiguous().view(b, q, m, d), spatial_shapes.contiguous(), level_start_index.contiguous()
        loc, attn = _msda_float(sampling_locations), _msda_float(attention_weights)
        v = value.contiguous() if needs[1] or needs[2] else None
        dv = torch.empty(value.shape, dtype=value.dtype, device=grad.device) if needs[0] else None
        dloc = torch.empty_like(loc) if needs[1] else None
        dattn = torch.empty_like(attn) if needs[2] else None
        stream, lib = _stream(grad), nv.lib()
        if needs[0]:
            ws = _workspace("msda", grad, min(b, im2col_step), s, m, d, q, levels, points)
        for i0, k in _chunks(b, im2col_step):
            if needs[1] or needs[2]:
                _call("msda_backward_loc", value, v[i0:].data_ptr(), shp.data_ptr(), st.data_ptr(), loc[i0:].data_ptr(), attn[i0:].data_ptr(),
                      g[i0:].data_ptr(), k, s, m, d, q, levels, points, _opt_ptr(dloc, i0), _opt_ptr(dattn, i0), stream)
            if needs[0]:
                def plan(keys, wts):
                    nv.check(lib.frcnn_ops_msda_plan(shp.data_ptr(), st.data_ptr(), loc[i0:].data_ptr(), attn[i0:].data_ptr(), k, s, m, q,
                                                     levels, points, keys, wts, stream), "frcnn_ops_msda_plan")

                def gather(keys, order, wts):
                    _call("msda_backward_value", value, keys, order, wts, g[i0:].data_ptr(), k, s, m, d, q, levels, points,
                          dv[i0:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
                held = _sorted_gather(plan, gather, k * q * m * levels * points * 4, grad.device)       # noqa: F841 (kept alive)
        return [dv if needs[0] else _placeholder(grad),
                dloc.to(sampling_locations.dtype) if needs[1] else _placeholder(grad),
                dattn.to(attention_weights.dtype) if needs[2] else _placeholder(grad)]


@_ms_deform_attn_backward.register_fake
def _(grad, value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step, needs):
    return _needs_fake(grad, (value, sampling_locations, attention_weights), needs)


def _msda_setup(ctx, inputs, output):
    value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step = inputs
    ctx.save_for_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights)
    ctx.im2col_step = im2col_step


def _msda_bwd(ctx, grad):
    needs = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[3]), bool(ctx.needs_input_grad[4])]
    dv, dloc, dattn = _ms_deform_attn_backward(grad, *ctx.saved_tensors, ctx.im2col_step, needs)
    return (dv if needs[0] else None, None, None, dloc if needs[1] else None, dattn if needs[2] else None, None)


_register_autograd("ms_deform_attn", _msda_bwd, _msda_setup)


# ---- frcnn::dcnv3, frcnn::dcnv4 (csrc/ops_dcnv3.hip, csrc/ops_dcnv4.hip: one sampler, two layouts of the learned tensors) -----------
def _dcnv3_out_size(size, kernel, stride, pad, dil):
    return max((size + 2 * pad - (dil * (kernel - 1) + 1)) // stride + 1, 0)


def _dcnv4_points(kernel_h, kernel_w, remove_center):
    return kernel_h * kernel_w - (1 if remove_center else 0)


def _dcnv4_record(group, points):
    """L: the 3 G P values of a pixel's record padded to a multiple of 8 (frcnn_ops_dcnv4_record())."""
    return (group * points * 3 + 7) // 8 * 8


def _dcn_backward(op, grad, input, learned, geom, group, group_channels, offset_scale, im2col_step, needs, remove_center=False):
    """The backward of op "dcnv3" on learned = (offset, mask), or of op "dcnv4" on learned = (offset_mask,) with its remove_center, which
    dcnv4's entry points take after the geometry; geom = (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w).
    Returns [d_input, then the gradient of each learned tensor], each in its argument's dtype; needs: which of them are wanted (the
    others come back as empty placeholders and cost nothing)."""
    tail = (int(remove_center),) if op == "dcnv4" else ()
    n, h, w, _ = input.shape
    ho, wo = learned[0].shape[1], learned[0].shape[2]
    points = _dcnv4_points(geom[0], geom[1], remove_center)
    if grad.numel() == 0 or h * w == 0:
        return [torch.zeros_like(t, memory_format=torch.contiguous_format) if need else _placeholder(grad)
                for t, need in zip((input,) + learned, needs)]
    if not any(needs):
        return [_placeholder(grad) for _ in needs]
    with torch.cuda.device(grad.device):
        g, fs = grad.contiguous(), [_msda_float(t) for t in learned]
        x = input.contiguous() if any(needs[1:]) else None
        dx = torch.empty(input.shape, dtype=input.dtype, device=grad.device) if needs[0] else None
        dfs = [torch.empty_like(f) if need else None for f, need in zip(fs, needs[1:])]     # dcnv4's kernel writes the pad lanes too
        stream, plan_entry = _stream(grad), getattr(nv.lib(), "frcnn_ops_%s_plan" % op)
        learned_backward = op + ("_backward_offset_mask" if op == "dcnv4" else "_backward_offset")
        if needs[0]:
            ws = _workspace(op, grad, min(n, im2col_step), h, w, group, group_channels, *geom, *tail)
        for i0, c in _chunks(n, im2col_step):
            if any(needs[1:]):
                _call(learned_backward, input, x[i0:].data_ptr(), *[f[i0:].data_ptr() for f in fs], g[i0:].data_ptr(), c, h, w, group,
                      group_channels, *geom, offset_scale, *tail, *[_opt_ptr(d, i0) for d in dfs], stream)
            if needs[0]:
                def plan(keys, wts):
                    nv.check(plan_entry(*[f[i0:].data_ptr() for f in fs], c, h, w, group, *geom, offset_scale, *tail, keys, wts, stream),
                             "frcnn_ops_%s_plan" % op)

                def gather(keys, order, wts):
                    _call(op + "_backward_input", input, keys, order, wts, g[i0:].data_ptr(), c, h, w, group, group_channels, *geom, *tail,
                          dx[i0:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
                held = _sorted_gather(plan, gather, c * ho * wo * group * points * 4, grad.device)       # noqa: F841 (kept alive)
        return [dx if needs[0] else _placeholder(grad)] + [d.to(t.dtype) if need else _placeholder(grad)
                                                           for d, t, need in zip(dfs, learned, needs[1:])]


@torch.library.custom_op("frcnn::dcnv3", mutates_args=())
def _dcnv3(input: Tensor, offset: Tensor, mask: Tensor, kernel_h: int, kernel_w: int, stride_h: int, stride_w: int, pad_h: int, pad_w: int,
           dilation_h: int, dilation_w: int, group: int, group_channels: int, offset_scale: float, im2col_step: int) -> Tensor:
    n, h, w, _ = input.shape
    ho, wo = offset.shape[1], offset.shape[2]
    out = torch.empty((n, ho, wo, group * group_channels), dtype=input.dtype, device=input.device)
    if out.numel() == 0:
        return out
    if h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x, off, msk = input.contiguous(), _msda_float(offset), _msda_float(mask)
        nb, stream = min(n, im2col_step), _stream(input)
        for i0 in range(0, n, nb):
            _call("dcnv3_forward", input, x[i0:].data_ptr(), off[i0:].data_ptr(), msk[i0:].data_ptr(), min(nb, n - i0), h, w, group,
                  group_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, offset_scale,
                  out[i0:].data_ptr(), stream)
    return out


@_dcnv3.register_fake
def _(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
      offset_scale, im2col_step):
    return input.new_empty((input.shape[0], offset.shape[1], offset.shape[2], group * group_channels))


@torch.library.custom_op("frcnn::dcnv3_backward", mutates_args=())
def _dcnv3_backward(grad: Tensor, input: Tensor, offset: Tensor, mask: Tensor, kernel_h: int, kernel_w: int, stride_h: int, stride_w: int,
                    pad_h: int, pad_w: int, dilation_h: int, dilation_w: int, group: int, group_channels: int, offset_scale: float,
                    im2col_step: int, needs: List[bool]) -> List[Tensor]:
    """[d_input, d_offset, d_mask], each in its argument's dtype; needs: which of them are wanted (the others come back as empty
    placeholders and cost nothing)."""
    return _dcn_backward("dcnv3", grad, input, (offset, mask), (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w),
                         group, group_channels, offset_scale, im2col_step, needs)


@_dcnv3_backward.register_fake
def _(grad, input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
      offset_scale, im2col_step, needs):
    return _needs_fake(grad, (input, offset, mask), needs)


def _dcnv3_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:3])
    ctx.args = tuple(inputs[3:])


def _dcnv3_bwd(ctx, grad):
    needs = [bool(v) for v in ctx.needs_input_grad[:3]]
    dx, doff, dmsk = _dcnv3_backward(grad, *ctx.saved_tensors, *ctx.args, needs)
    return (dx if needs[0] else None, doff if needs[1] else None, dmsk if needs[2] else None) + (None,) * 12


_register_autograd("dcnv3", _dcnv3_bwd, _dcnv3_setup)


@torch.library.custom_op("frcnn::dcnv4", mutates_args=())
def _dcnv4(input: Tensor, offset_mask: Tensor, kernel_h: int, kernel_w: int, stride_h: int, stride_w: int, pad_h: int, pad_w: int,
           dilation_h: int, dilation_w: int, group: int, group_channels: int, offset_scale: float, im2col_step: int,
           remove_center: bool) -> Tensor:
    n, h, w, _ = input.shape
    ho, wo = offset_mask.shape[1], offset_mask.shape[2]
    out = torch.empty((n, ho, wo, group * group_channels), dtype=input.dtype, device=input.device)
    if out.numel() == 0:
        return out
    if h * w == 0:
        return out.zero_()
    with torch.cuda.device(input.device):
        x, om = input.contiguous(), _msda_float(offset_mask)
        nb, stream = min(n, im2col_step), _stream(input)
        for i0 in range(0, n, nb):
            _call("dcnv4_forward", input, x[i0:].data_ptr(), om[i0:].data_ptr(), min(nb, n - i0), h, w, group, group_channels, kernel_h,
                  kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, offset_scale, int(remove_center), out[i0:].data_ptr(),
                  stream)
    return out


@_dcnv4.register_fake
def _(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
      offset_scale, im2col_step, remove_center):
    return input.new_empty((input.shape[0], offset_mask.shape[1], offset_mask.shape[2], group * group_channels))


@torch.library.custom_op("frcnn::dcnv4_backward", mutates_args=())
def _dcnv4_backward(grad: Tensor, input: Tensor, offset_mask: Tensor, kernel_h: int, kernel_w: int, stride_h: int, stride_w: int,
                    pad_h: int, pad_w: int, dilation_h: int, dilation_w: int, group: int, group_channels: int, offset_scale: float,
                    im2col_step: int, remove_center: bool, needs: List[bool]) -> List[Tensor]:
    """[d_input, d_offset_mask], each in its argument's dtype; needs: which of them are wanted (the other comes back as an empty
    placeholder and costs nothing)."""
    return _dcn_backward("dcnv4", grad, input, (offset_mask,), (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w),
                         group, group_channels, offset_scale, im2col_step, needs, remove_center)


@_dcnv4_backward.register_fake
def _(grad, input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
      offset_scale, im2col_step, remove_center, needs):
    return _needs_fake(grad, (input, offset_mask), needs)


def _dcnv4_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:2])
    ctx.args = tuple(inputs[2:])


def _dcnv4_bwd(ctx, grad):
    needs = [bool(v) for v in ctx.needs_input_grad[:2]]
    dx, dom = _dcnv4_backward(grad, *ctx.saved_tensors, *ctx.args, needs)
    return (dx if needs[0] else None, dom if needs[1] else None) + (None,) * 13


_register_autograd("dcnv4", _dcnv4_bwd, _dcnv4_setup)


# ---- public interface -------------------------------------------------------------------------------------------------------------
def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: int64 indices of the kept boxes, by descending score."""
    _nms_input(boxes, scores)
    return _nms_op(boxes, scores, float(iou_threshold))


def batched_nms(boxes, scores, idxs, iou_threshold):
    """torchvision.ops.batched_nms: NMS within each category of idxs; kept indices by descending score, ties by ascending index."""
    _nms_input(boxes, scores)
    _check_tensor("idxs", idxs, (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8), "an integer tensor")
    _check_same_device(boxes, idxs, "boxes", "idxs")
    if idxs.dim() != 1 or idxs.shape[0] != boxes.shape[0]:
        raise ValueError("idxs must be [N] with N = %d, got shape %s" % (boxes.shape[0], tuple(idxs.shape)))
    return _batched_nms_op(boxes, scores, idxs, float(iou_threshold))


def roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
    """torchvision.ops.roi_align: [K, C, oh, ow] (channels_last memory)."""
    rois = _roi_input(input, boxes)
    oh, ow = _output_size(output_size)
    if int(sampling_ratio) > MAX_SAMPLING_RATIO:
        raise ValueError("sampling_ratio must be <= %d, got %d" % (MAX_SAMPLING_RATIO, sampling_ratio))
    return _roi_align(input, rois, float(spatial_scale), oh, ow, int(sampling_ratio), bool(aligned))


def roi_pool(input, boxes, output_size, spatial_scale=1.0):
    """torchvision.ops.roi_pool: [K, C, oh, ow] (channels_last memory)."""
    rois = _roi_input(input, boxes)
    oh, ow = _output_size(output_size)
    return _roi_pool(input, rois, float(spatial_scale), oh, ow)[0]


def _ps_output_size(input, output_size):
    oh, ow = _output_size(output_size)
    if input.shape[1] % (oh * ow) != 0:
        raise ValueError("input channels must be a multiple of pooling height * pooling width, got %d channels for (%d, %d)"
                         % (input.shape[1], oh, ow))
    return oh, ow


def ps_roi_pool(input, boxes, output_size, spatial_scale=1.0):
    """torchvision.ops.ps_roi_pool: [K, C / (oh * ow), oh, ow], contiguous."""
    rois = _roi_input(input, boxes)
    oh, ow = _ps_output_size(input, output_size)
    return _ps_roi_pool(input, rois, float(spatial_scale), oh, ow)


def ps_roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1):
    """torchvision.ops.ps_roi_align: [K, C / (oh * ow), oh, ow], contiguous."""
    rois = _roi_input(input, boxes)
    oh, ow = _ps_output_size(input, output_size)
    if int(sampling_ratio) > MAX_SAMPLING_RATIO:
        raise ValueError("sampling_ratio must be <= %d, got %d" % (MAX_SAMPLING_RATIO, sampling_ratio))
    return _ps_roi_align(input, rois, float(spatial_scale), oh, ow, int(sampling_ratio))


_F32_ONLY = ("float32 (deform_conv2d takes all-float32 tensors, or all-float16 / all-bfloat16 ones for the 16-bit kernels, and no mix: "
             "pass .float())")


def _check_int(name, v):
    """An int, and no bool (True would pass for 1)."""
    if not isinstance(v, int) or isinstance(v, bool):
        raise TypeError("%s must be an int, got %r" % (name, v))


def _int_pair(name, v, low):
    if isinstance(v, int) and not isinstance(v, bool):
        v = (v, v)
    if not (isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, int) and not isinstance(e, bool) for e in v)):
        raise TypeError("%s must be an int or a pair of ints, got %r" % (name, v))
    if v[0] < low or v[1] < low:
        raise ValueError("%s must be >= %d, got %r" % (name, low, tuple(v)))
    return int(v[0]), int(v[1])


def deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    """torchvision.ops.deform_conv2d: deformable convolution v1, v2 with a mask; [N, C_out, oh, ow], contiguous."""
    tensors = [("input", input), ("offset", offset), ("weight", weight)] + [(k, t) for k, t in (("bias", bias), ("mask", mask)) if t is not None]
    if all(isinstance(t, torch.Tensor) and t.dtype == torch.float16 for _, t in tensors):
        allowed = (torch.float16,)
    elif all(isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 for _, t in tensors):
        allowed = (torch.bfloat16,)
    else:
        allowed = (torch.float32,)                      # a mix is refused at its first tensor that is not float32
    for name, t in tensors:
        _check_tensor(name, t, allowed, _F32_ONLY)
    for name, t in tensors[1:]:
        _check_same_device(input, t, "input", name)
    if input.dim() != 4:
        raise ValueError("input must be [N, C_in, H, W], got shape %s" % (tuple(input.shape),))
    if weight.dim() != 4:
        raise ValueError("weight must be [C_out, C_in / groups, kh, kw], got shape %s" % (tuple(weight.shape),))
    if offset.dim() != 4:
        raise ValueError("offset must be [N, 2 * offset_groups * kh * kw, oh, ow], got shape %s" % (tuple(offset.shape),))
    if mask is not None and mask.dim() != 4:
        raise ValueError("mask must be [N, offset_groups * kh * kw, oh, ow], got shape %s" % (tuple(mask.shape),))
    stride, padding, dilation = _int_pair("stride", stride, 1), _int_pair("padding", padding, 0), _int_pair("dilation", dilation, 1)
    n, c, h, w = input.shape
    co, cg, kh, kw = weight.shape
    if cg < 1 or kh < 1 or kw < 1 or h < 1 or w < 1:
        raise ValueError("weight must have at least one input channel and one tap and input at least one cell, got weight %s, input %s"
                         % (tuple(weight.shape), tuple(input.shape)))
    if c % cg != 0:
        raise ValueError("input channels must be a multiple of weight.shape[1] (C_in / groups), got %d and %d" % (c, cg))
    groups = c // cg
    if co % groups != 0:
        raise ValueError("output channels must be a multiple of groups, got %d for %d groups" % (co, groups))
    if offset.shape[1] == 0 or offset.shape[1] % (2 * kh * kw) != 0:
        raise ValueError("offset.shape[1] must be a positive multiple of 2 * kh * kw = %d, got %d" % (2 * kh * kw, offset.shape[1]))
    og = offset.shape[1] // (2 * kh * kw)
    if c % og != 0:
        raise ValueError("input channels must be a multiple of the offset groups, got %d for %d offset groups" % (c, og))
    oh, ow = _deform_output_size(h, w, kh, kw, stride, padding, dilation)
    if oh < 1 or ow < 1:
        raise ValueError("the output would be empty: (%d, %d) for input %s, kernel (%d, %d), stride %s, padding %s, dilation %s"
                         % (oh, ow, tuple(input.shape), kh, kw, stride, padding, dilation))
    if tuple(offset.shape) != (n, 2 * og * kh * kw, oh, ow):
        raise ValueError("offset must be [N, 2 * offset_groups * kh * kw, oh, ow] = [%d, %d, %d, %d], got shape %s"
                         % (n, 2 * og * kh * kw, oh, ow, tuple(offset.shape)))
    if mask is not None and tuple(mask.shape) != (n, og * kh * kw, oh, ow):
        raise ValueError("mask must be [N, offset_groups * kh * kw, oh, ow] = [%d, %d, %d, %d], got shape %s"
                         % (n, og * kh * kw, oh, ow, tuple(mask.shape)))
    if bias is not None and tuple(bias.shape) != (co,):
        raise ValueError("bias must be [C_out] = [%d], got shape %s" % (co, tuple(bias.shape)))
    nb = max(1, min(n, DEFORM_CHUNK_IMAGES))
    run = 8 if input.dtype in _HALF else 4               # what the kernels pad a row of the column matrix to
    pp = (oh * ow + run - 1) // run * run
    largest = max(nb * pp, c * kh * kw + (8 * groups if input.dtype in _HALF else 0), nb * og * h * w, nb * og * kh * kw * oh * ow * 4, h + padding[0] + dilation[0] * (kh - 1) + 1,
                  w + padding[1] + dilation[1] * (kw - 1) + 1)
    if largest > MAX_DEFORM_INDEX:
        raise ValueError("deform_conv2d is too large for the kernels' 32-bit indices: %d > MAX_DEFORM_INDEX = %d (columns, cells or "
                         "sample corners of %d images)" % (largest, MAX_DEFORM_INDEX, nb))
    return _deform_conv2d(input, offset, weight, bias, mask, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                          DEFORM_CHUNK_IMAGES)


def deform_roi_pool(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1):
    """Deformable RoI pooling (mmcv's deform_roi_pool, restated, unpinned): [K, C, oh, ow] (channels_last memory).  offset [K, 2, oh, ow],
    channel 0 the x offset, channel 1 the y offset, in float32 or the input's dtype; None or an empty tensor: no offset."""
    r = _roi_input(input, rois)
    oh, ow = _output_size(output_size)
    if int(sampling_ratio) > MAX_SAMPLING_RATIO:
        raise ValueError("sampling_ratio must be <= %d, got %d" % (MAX_SAMPLING_RATIO, sampling_ratio))
    if offset is not None:
        what = "float32" if input.dtype == torch.float32 else "float32 or the input's %s" % input.dtype
        _check_tensor("offset", offset, (torch.float32, input.dtype), what)
        _check_same_device(input, offset, "input", "offset")
        if tuple(offset.shape) != (r.shape[0], 2, oh, ow) and offset.numel() == 0:
            offset = None
        elif tuple(offset.shape) != (r.shape[0], 2, oh, ow):
            raise ValueError("offset must be [K, 2, oh, ow] = [%d, 2, %d, %d] (x offsets, then y offsets), got shape %s"
                             % (r.shape[0], oh, ow, tuple(offset.shape)))
    return _deform_roi_pool(input, r, offset, float(spatial_scale), oh, ow, int(sampling_ratio), float(gamma))


def prroi_pool(input, rois, output_size, spatial_scale=1.0):
    """Precise RoI Pooling (IoU-Net's PrRoIPool; mmcv's prroi_pool, restated, unpinned): [K, C, oh, ow] (channels_last memory), the exact
    integral of the bilinear surface over each bin divided by the bin's area; differentiable in input and in rois."""
    r = _roi_input(input, rois)
    oh, ow = _output_size(output_size)
    return _prroi_pool(input, r, float(spatial_scale), oh, ow)


def _prroi_antiderivative(t):
    """The integral of hat from -inf to t: C1, so autograd through the clamp gives hat(t) everywhere, ties included."""
    u = t.clamp(-1.0, 1.0)
    return torch.where(u < 0, (u + 1) ** 2 / 2, 1 - (1 - u) ** 2 / 2)


def _prroi_axis_weights(start, size, n_out, cells):
    """[K, n_out, cells]: the integral of hat(x - i) over bin p = [start + p size, start + (p + 1) size] of each RoI."""
    p = torch.arange(n_out, dtype=start.dtype, device=start.device)[None, :]
    i = torch.arange(cells, dtype=start.dtype, device=start.device)
    s = start[:, None] + p * size[:, None]
    e = s + size[:, None]
    return _prroi_antiderivative(e[..., None] - i) - _prroi_antiderivative(s[..., None] - i)


def prroi_pool_pytorch(input, rois, output_size, spatial_scale=1.0):
    """prroi_pool from torch operations, on any device, with autograd to input and rois: the fallback, and what tools/ops_bench.py
    measures the kernels against.  input [N, C, H, W] of any floating dtype (16-bit maps compute in float32, float64 in float64);
    rois a Tensor[K, 5] or a list of Tensor[L_i, 4] of any floating dtype.  Returns [K, C, oh, ow] in the input's dtype.  The rule
    0 < A < +inf is applied in the computing dtype, so with a float64 map a box whose area overflows only float32 (1e30 x 1e30) is pooled,
    where the kernels and the float32 composition return zeros."""
    if not isinstance(input, torch.Tensor) or not input.is_floating_point():
        raise TypeError("input must be a floating-point torch.Tensor, got %s" % (input.dtype if isinstance(input, torch.Tensor)
                                                                                 else type(input).__name__))
    if input.dim() != 4:
        raise ValueError("input must be [N, C, H, W], got shape %s" % (tuple(input.shape),))
    oh, ow = _output_size(output_size)
    dtype = torch.float64 if input.dtype == torch.float64 else torch.float32
    if isinstance(rois, (list, tuple)):
        for j, b in enumerate(rois):
            if not isinstance(b, torch.Tensor) or not b.is_floating_point() or b.dim() != 2 or b.shape[1] != 4:
                raise ValueError("rois[%d] must be a floating-point Tensor[L, 4]" % j)
        parts = [torch.cat([torch.full_like(b[:, :1], float(j)), b], dim=1).to(dtype) for j, b in enumerate(rois)]
        r = torch.cat(parts, dim=0) if parts else input.new_zeros((0, 5), dtype=dtype)
    elif isinstance(rois, torch.Tensor) and rois.is_floating_point() and rois.dim() == 2 and rois.shape[1] == 5:
        r = rois.to(dtype)
    else:
        raise ValueError("rois must be a floating-point Tensor[K, 5] (batch index, x1, y1, x2, y2) or a list of Tensor[L, 4]")
    n, c, h, w = input.shape
    k = r.shape[0]
    scale = float(torch.tensor(spatial_scale, dtype=torch.float32))         # as the kernels receive it
    def bins(rows):
        x1, y1, x2, y2 = (rows[:, j] * scale for j in (1, 2, 3, 4))
        return x1, y1, (x2 - x1).clamp(min=0) / ow, (y2 - y1).clamp(min=0) / oh

    # which RoIs are pooled is decided without autograd, and only their rows are computed on: a NaN never meets a gradient
    with torch.no_grad():
        _, _, bw, bh = bins(r)
        valid = (bw * bh > 0) & torch.isfinite(bw * bh) & (r[:, 0] > -1) & (r[:, 0] < n)
        image = torch.where(valid, r[:, 0], torch.zeros_like(r[:, 0])).long()
    out = torch.zeros((k, c, oh, ow), dtype=dtype, device=input.device)
    for b in range(n):
        pick = (valid & (image == b)).nonzero()[:, 0]
        if pick.numel() == 0:
            continue
        x1, y1, bw, bh = bins(r[pick])
        wy = _prroi_axis_weights(y1, bh, oh, h)
        wx = _prroi_axis_weights(x1, bw, ow, w)
        rows = torch.einsum("kph,chw->kcpw", wy, input[b].to(dtype))
        vals = torch.einsum("kcpw,kqw->kcpq", rows, wx) / (bw * bh)[:, None, None, None]
        out = out.index_add(0, pick, vals)
    return out.to(input.dtype)


def _border_pool_size(pool_size):
    _check_int("pool_size", pool_size)
    if not 1 <= pool_size <= MAX_BORDER_POOL:
        raise ValueError("pool_size must lie in [1, %d], got %d" % (MAX_BORDER_POOL, pool_size))
    return pool_size


def _border_shapes(input, boxes):
    """The shape rules border_align and border_align_pytorch share."""
    if input.dim() != 4:
        raise ValueError("input must be [N, 4 C, H, W], got shape %s" % (tuple(input.shape),))
    if input.shape[1] % 4 != 0:
        raise ValueError("input must have 4 C channels (top, left, bottom, right groups of C), got %d" % input.shape[1])
    if boxes.dim() != 3 or boxes.shape[0] != input.shape[0] or boxes.shape[2] != 4:
        raise ValueError("boxes must be [N, K, 4] (x1, y1, x2, y2) with N = %d, got shape %s" % (input.shape[0], tuple(boxes.shape)))


def border_align(input, boxes, pool_size):
    """BorderAlign (BorderDet's border pooling; mmcv's border_align, restated, unpinned): [N, C, K, 4] (channels_last memory), per box
    and edge (top, left, bottom, right) the per-channel maximum of pool_size + 1 bilinear samples along the edge, taken from that
    edge's group of the 4 C channels; differentiable in input."""
    _check_tensor("input", input, _MAP_DTYPES, _MAP_WHAT, "border_align_pytorch")
    dtypes, what = _box_dtypes(input)
    _check_tensor("boxes", boxes, dtypes, what, "border_align_pytorch")
    _check_same_device(input, boxes, "input", "boxes")
    _border_shapes(input, boxes)
    pool_size = _border_pool_size(pool_size)
    n, c4, h, w = input.shape
    c, k = c4 // 4, boxes.shape[1]
    if h > MAX_BORDER_SIDE or w > MAX_BORDER_SIDE:
        raise ValueError("input: H and W must be <= %d, got %d x %d" % (MAX_BORDER_SIDE, h, w))
    lanes = n * k * 4 * ((c + 3) // 4)
    blocks = n * ((c + 255) // 256) * ((h + 1) // 2) * ((w + 1) // 2)
    if lanes > MAX_BORDER_INDEX:
        raise ValueError("N K 4 ceil(C / 4) = %d exceeds %d (the forward's launch grid)" % (lanes, MAX_BORDER_INDEX))
    if blocks > MAX_BORDER_INDEX:
        raise ValueError("N ceil(C / 256) ceil(H / 2) ceil(W / 2) = %d exceeds %d (the backward's launch grid)" % (blocks, MAX_BORDER_INDEX))
    return _border_align(input, boxes.float(), pool_size)[0]


def _border_axis_pytorch(v, size):
    """roi_align's rule for one coordinate already known to lie in [-1, size]: (low index, high index, weight of low, weight of high)."""
    v = v.clamp(min=0)
    low = v.long()
    last = low >= size - 1
    low = torch.where(last, torch.full_like(low, size - 1), low)
    high = torch.where(last, low, low + 1)
    v = torch.where(last, low.to(v.dtype), v)
    wh = v - low.to(v.dtype)
    return low, high, 1 - wh, wh


def border_align_pytorch(input, boxes, pool_size):
    """border_align from torch operations, on any device, with autograd to input: the fallback, and what tools/ops_bench.py measures the
    kernels against.  input [N, 4 C, H, W] of any floating dtype (16-bit maps compute in float32, float64 in float64), boxes a
    floating-point [N, K, 4].  Returns [N, C, K, 4] in the input's dtype.  One edge at a time it gathers the four cells of every sample
    ([N, C, K, pool_size + 1] each) and takes torch.max over the samples, which keeps the first maximum; a NaN sample at i > 0 is
    replaced by -inf first, so that it never wins."""
    for name, t in (("input", input), ("boxes", boxes)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError("%s must be a floating-point torch.Tensor, got %s" % (name, t.dtype if isinstance(t, torch.Tensor)
                                                                                   else type(t).__name__))
    _check_same_device(input, boxes, "input", "boxes")
    _border_shapes(input, boxes)
    pool_size = _border_pool_size(pool_size)
    dtype = torch.float64 if input.dtype == torch.float64 else torch.float32
    n, c4, h, w = input.shape
    c, k = c4 // 4, boxes.shape[1]
    if n * c * k == 0 or h * w == 0:
        return input.new_zeros((n, c, k, 4)) + input.sum() * 0
    b = boxes.detach().to(dtype)
    x1, y1, x2, y2 = (b[..., j, None] for j in range(4))                    # [N, K, 1]
    i = torch.arange(pool_size + 1, dtype=dtype, device=input.device)      # [P + 1]
    sx, sy = (x2 - x1) / pool_size, (y2 - y1) / pool_size
    zero = torch.zeros_like(i)
    edges = ((x1, y1, i * sx, zero), (x1, y1, zero, i * sy), (x2, y2, i * -sx, zero), (x2, y2, zero, i * -sy))
    maps = input.to(dtype).reshape(n, 4, c, h * w)
    outs = []
    for e, (x0, y0, dx, dy) in enumerate(edges):
        x, y = x0 + dx, y0 + dy                                             # [N, K, P + 1]
        valid = (y >= -1) & (y <= h) & (x >= -1) & (x <= w)                 # a NaN fails
        yl, yh, wyl, wyh = _border_axis_pytorch(torch.where(valid, y, zero), h)
        xl, xh, wxl, wxh = _border_axis_pytorch(torch.where(valid, x, zero), w)

        def cells(row, col):
            index = (row * w + col).reshape(n, 1, -1).expand(n, c, -1)
            return maps[:, e].gather(2, index).reshape(n, c, k, pool_size + 1)

        w1, w2, w3, w4 = ((a * b)[:, None] for a, b in ((wyl, wxl), (wyl, wxh), (wyh, wxl), (wyh, wxh)))
        vals = ((cells(yl, xl) * w1 + cells(yl, xh) * w2) + cells(yh, xl) * w3) + cells(yh, xh) * w4
        vals = torch.where(valid[:, None], vals, torch.zeros_like(vals))
        late_nan = torch.isnan(vals) & (i > 0)
        vals = torch.where(late_nan, torch.full_like(vals, float("-inf")), vals)
        outs.append(vals.max(dim=3).values)
    return torch.stack(outs, dim=3).to(input.dtype)


def _rotated_boxes(name, boxes, clockwise):
    """Checks a Tensor[N, 5] of rotated boxes; returns it in the kernels' convention (angles negated for clockwise=False)."""
    _check_tensor(name, boxes, (torch.float32,), "float32 (rotated boxes are float32 only: pass .float())")
    if boxes.dim() != 2 or boxes.shape[1] != 5:
        raise ValueError("%s must be [N, 5] (cx, cy, w, h, angle), got shape %s" % (name, tuple(boxes.shape)))
    if clockwise:
        return boxes
    return torch.cat([boxes[:, :4], -boxes[:, 4:]], dim=1)


def box_iou_rotated(boxes1, boxes2, mode="iou", aligned=False, clockwise=True):
    """mmcv.ops.box_iou_rotated: the IoU (or, mode="iof", the intersection over the first box's area) of rotated boxes
    (cx, cy, w, h, angle in radians): float32 [N, M], or [N] when aligned.  No autograd."""
    if mode not in ("iou", "iof"):
        raise ValueError("mode must be 'iou' or 'iof', got %r" % (mode,))
    b1, b2 = _rotated_boxes("boxes1", boxes1, clockwise), _rotated_boxes("boxes2", boxes2, clockwise)
    _check_same_device(boxes1, boxes2, "boxes1", "boxes2")
    if aligned and b1.shape[0] != b2.shape[0]:
        raise ValueError("aligned=True needs boxes1 and boxes2 of one length, got %d and %d" % (b1.shape[0], b2.shape[0]))
    if b1.shape[0] > MAX_ROTATED_IOU_ROWS:
        raise ValueError("boxes1 holds at most %d boxes, got %d" % (MAX_ROTATED_IOU_ROWS, b1.shape[0]))
    return _box_iou_rotated(b1.detach(), b2.detach(), int(mode == "iof"), bool(aligned))


def _diff_iou_input(names, boxes, last, row, fallback=None):
    """Checks the two box tensors of a differentiable IoU: float32, one shape [B, N, last] or [N, last], one device, at most
    MAX_ROTATED_IOU_ROWS pairs."""
    for name, b in zip(names, boxes):
        _check_tensor(name, b, (torch.float32,), "float32 (rotated boxes are float32 only: pass .float())", fallback)
        if b.dim() not in (2, 3) or b.shape[-1] != last:
            raise ValueError("%s must be [B, N, %d] or [N, %d] %s, got shape %s" % (name, last, last, row, tuple(b.shape)))
    if boxes[0].shape != boxes[1].shape:
        raise ValueError("%s and %s must have one shape, got %s and %s" % (names + (tuple(boxes[0].shape), tuple(boxes[1].shape))))
    _check_same_device(boxes[0], boxes[1], *names)
    n = boxes[0].numel() // last
    if n > MAX_ROTATED_IOU_ROWS:
        raise ValueError("%s and %s hold at most MAX_ROTATED_IOU_ROWS = %d pairs, got %d" % (names + (MAX_ROTATED_IOU_ROWS, n)))


def diff_iou_rotated_2d(box1, box2):
    """mmcv.ops.diff_iou_rotated_2d: the IoU of the aligned pairs of rotated boxes (cx, cy, w, h, angle in radians), [B, N, 5] or [N, 5]
    -> [B, N] or [N], with gradients for both: box_iou_rotated(aligned=True)'s value bit for bit, a closed-form backward in one launch."""
    _diff_iou_input(("box1", "box2"), (box1, box2), 5, "(cx, cy, w, h, angle)", "diff_iou_rotated_2d_pytorch")
    return _diff_iou_rotated(box1.reshape(-1, 5), box2.reshape(-1, 5))[0].view(box1.shape[:-1])


def diff_iou_rotated_3d(box3d1, box3d2):
    """mmcv.ops.diff_iou_rotated_3d: the IoU of the aligned pairs of 3-D boxes (x, y, z, w, h, l, alpha), rotated by alpha about z,
    [B, N, 7] or [N, 7] -> [B, N] or [N]: the 2-D intersection of (x, y, w, h, alpha) times the overlap along z, over the union volume."""
    _diff_iou_input(("box3d1", "box3d2"), (box3d1, box3d2), 7, "(x, y, z, w, h, l, alpha)")
    a, b = box3d1.reshape(-1, 7), box3d2.reshape(-1, 7)
    bev = lambda t: torch.cat([t[:, 0:2], t[:, 3:5], t[:, 6:7]], dim=1)     # noqa: E731
    inter2d = _diff_iou_rotated(bev(a), bev(b))[1]
    z_overlap = (torch.min(a[:, 2] + a[:, 5] * 0.5, b[:, 2] + b[:, 5] * 0.5)
                 - torch.max(a[:, 2] - a[:, 5] * 0.5, b[:, 2] - b[:, 5] * 0.5)).clamp_min(0.0)
    inter3d = inter2d * z_overlap
    vol1, vol2 = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
    return (inter3d / (vol1 + vol2 - inter3d)).view(box3d1.shape[:-1])


def _diff_iou_clip(v, n, axis, sign, bound):
    """One Sutherland-Hodgman pass over polygons v [P, 8, 2] with n [P] vertices, keeping sign * coordinate[axis] <= bound [P]: out of
    place and free of host syncs; the division sees a denominator of 1 wherever the edge does not cross."""
    slots = torch.arange(8, device=v.device)
    out, m = torch.zeros_like(v), torch.zeros_like(n)
    prev = v.gather(1, (n - 1).clamp(min=0)[:, None, None].expand(-1, 1, 2))[:, 0]
    for i in range(8):
        q = v[:, i]
        act = i < n
        pd, qd = sign * prev[:, axis], sign * q[:, axis]
        pin, qin = pd <= bound, qd <= bound
        cross = act & (pin != qin) & (m < 8)
        t = (bound - pd) / torch.where(cross, qd - pd, torch.ones_like(qd))
        other = prev[:, 1 - axis] + t * (q[:, 1 - axis] - prev[:, 1 - axis])
        pt = torch.stack([sign * bound, other] if axis == 0 else [other, sign * bound], 1)
        out = torch.where(((slots == m[:, None]) & cross[:, None])[:, :, None], pt[:, None], out)
        m = m + cross
        keep = act & qin & (m < 8)
        out = torch.where(((slots == m[:, None]) & keep[:, None])[:, :, None], q[:, None], out)
        m = m + keep
        prev = torch.where(act[:, None], q, prev)
    return out, m


def diff_iou_rotated_2d_pytorch(box1, box2):
    """diff_iou_rotated_2d from torch operations, differentiable by autograd, on any device, in float32 or float64: box 1's corners in
    box 2's frame, four Sutherland-Hodgman passes over a fixed list of 8 vertices per pair, the fan area.  Every gradient is finite
    whatever the boxes hold (a pair under the zero rule gets zeros)."""
    for name, b in (("box1", box1), ("box2", box2)):
        if not isinstance(b, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(b).__name__))
        if b.dtype not in (torch.float32, torch.float64):
            raise TypeError("%s must be float32 or float64, got %s" % (name, b.dtype))
        if b.dim() not in (2, 3) or b.shape[-1] != 5:
            raise ValueError("%s must be [B, N, 5] or [N, 5] (cx, cy, w, h, angle), got shape %s" % (name, tuple(b.shape)))
    if box1.shape != box2.shape or box1.dtype != box2.dtype:
        raise ValueError("box1 and box2 must have one shape and dtype, got %s %s and %s %s"
                         % (tuple(box1.shape), box1.dtype, tuple(box2.shape), box2.dtype))
    _check_same_device(box1, box2, "box1", "box2")
    a, b = box1.reshape(-1, 5), box2.reshape(-1, 5)
    ok = lambda t: torch.isfinite(t).all(1) & (t[:, 2] >= 0) & (t[:, 3] >= 0) & (t[:, 2] * t[:, 3] >= 1e-14)     # noqa: E731
    valid = ok(a) & ok(b)
    unit = a.new_tensor([0.0, 0.0, 1.0, 1.0, 0.0])
    a, b = torch.where(valid[:, None], a, unit), torch.where(valid[:, None], b, unit)      # a NaN never meets a gradient
    ca, sa, cb, sb = torch.cos(a[:, 4]), torch.sin(a[:, 4]), torch.cos(b[:, 4]), torch.sin(b[:, 4])
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    ox, oy = dx * cb + dy * sb, dy * cb - dx * sb
    cd, sd = ca * cb + sa * sb, sa * cb - ca * sb
    one = torch.ones_like(cd)
    cd = torch.where(sd == 0, torch.where(cd < 0, -one, one), cd)
    sd = torch.where(cd == 0, torch.where(sd < 0, -one, one), sd)
    hw, hh = 0.5 * a[:, 2], 0.5 * a[:, 3]
    ux, uy, vx, vy = hw * cd, hw * sd, -hh * sd, hh * cd
    zero = torch.zeros_like(ox)
    corners = [((ox + ux) + vx, (oy + uy) + vy), ((ox - ux) + vx, (oy - uy) + vy), ((ox - ux) - vx, (oy - uy) - vy),
               ((ox + ux) - vx, (oy + uy) - vy)] + [(zero, zero)] * 4
    v = torch.stack([torch.stack(c, 1) for c in corners], 1)
    n = torch.full_like(valid, 4, dtype=torch.int64)
    bw, bh = 0.5 * b[:, 2], 0.5 * b[:, 3]
    for axis, sign, bound in ((0, 1.0, bw), (1, 1.0, bh), (0, -1.0, bw), (1, -1.0, bh)):
        v, n = _diff_iou_clip(v, n, axis, sign, bound)
    total = zero
    e = v[:, 1] - v[:, 0]
    for i in range(2, 8):
        f = v[:, i] - v[:, 0]
        act = (i < n) & (n >= 3)
        total = total + torch.where(act, e[:, 0] * f[:, 1] - f[:, 0] * e[:, 1], zero)
        e = torch.where(act[:, None], f, e)
    inter = 0.5 * total.abs()
    iou = inter / ((a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3]) - inter)
    return torch.where(valid, iou, zero).view(box1.shape[:-1])


def _nms_scores_labels(op, name, boxes, scores, labels):
    """The checks nms_rotated and nms_quadri share once their boxes (`name`) are checked: float32 scores [N], at most MAX_NMS_BOXES
    boxes, integer labels [N] or None, one device."""
    _check_tensor("scores", scores, (torch.float32,), "float32")
    _check_same_device(boxes, scores, name, "scores")
    if scores.dim() != 1 or scores.shape[0] != boxes.shape[0]:
        raise ValueError("scores must be [N] with N = %d, got shape %s" % (boxes.shape[0], tuple(scores.shape)))
    if boxes.shape[0] > MAX_NMS_BOXES:
        raise ValueError("%s takes at most %d boxes, got %d" % (op, MAX_NMS_BOXES, boxes.shape[0]))
    if labels is not None:
        _check_tensor("labels", labels, (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8), "an integer tensor")
        _check_same_device(boxes, labels, name, "labels")
        if labels.dim() != 1 or labels.shape[0] != boxes.shape[0]:
            raise ValueError("labels must be [N] with N = %d, got shape %s" % (boxes.shape[0], tuple(labels.shape)))


def nms_rotated(boxes, scores, iou_threshold, labels=None, clockwise=True):
    """mmcv.ops.nms_rotated: greedy NMS on box_iou_rotated, within each label when labels are given.  Returns (dets [K, 6] =
    cat(boxes[keep], scores[keep, None]), keep int64 [K]), by descending score, ties by ascending index."""
    b = _rotated_boxes("boxes", boxes, clockwise)
    _nms_scores_labels("nms_rotated", "boxes", boxes, scores, labels)
    keep = _nms_rotated_op(b.detach(), scores.detach(), labels, float(iou_threshold))
    return torch.cat([boxes[keep], scores[keep, None]], dim=1), keep


def _f32(v):
    """v rounded to float32, as the kernels receive it."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _soft_nms_args(boxes, scores, iou_threshold, sigma, min_score, method, offset, labels):
    """The checks soft_nms and soft_nms_pytorch share (dtypes and devices are each one's own); returns (thr, sigma, min_score) rounded
    to float32, the method's code and the offset."""
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("boxes must be [N, 4] (x1, y1, x2, y2), got shape %s" % (tuple(boxes.shape),))
    if scores.dim() != 1 or scores.shape[0] != boxes.shape[0]:
        raise ValueError("scores must be [N] with N = %d, got shape %s" % (boxes.shape[0], tuple(scores.shape)))
    _check_same_device(boxes, scores, "boxes", "scores")
    if labels is not None:
        if not isinstance(labels, torch.Tensor):
            raise TypeError("labels must be a torch.Tensor, got %s" % type(labels).__name__)
        if labels.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise TypeError("labels must be an integer tensor, got %s" % labels.dtype)
        _check_same_device(boxes, labels, "boxes", "labels")
        if labels.dim() != 1 or labels.shape[0] != boxes.shape[0]:
            raise ValueError("labels must be [N] with N = %d, got shape %s" % (boxes.shape[0], tuple(labels.shape)))
    if method not in SOFT_NMS_METHODS:
        raise ValueError("method must be 'naive', 'linear' or 'gaussian', got %r" % (method,))
    if isinstance(offset, bool) or offset not in (0, 1):
        raise ValueError("offset must be 0 or 1, got %r" % (offset,))
    thr, sig, low = _f32(iou_threshold), _f32(sigma), _f32(min_score)
    if not (sig > 0 and math.isfinite(sig)):
        raise ValueError("sigma must be positive and finite, got %r" % (sigma,))
    if math.isnan(thr):
        raise ValueError("iou_threshold must not be NaN, got %r" % (iou_threshold,))
    if math.isnan(low):
        raise ValueError("min_score must not be NaN, got %r" % (min_score,))
    return thr, sig, low, SOFT_NMS_METHODS[method], int(offset)


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method="linear", offset=0, labels=None):
    """mmcv.ops.soft_nms on the GPU, within each label when labels are given: Soft-NMS with naive, linear or gaussian rescoring under the
    contract of the module docstring (float32, ties to the smaller index, a box only ever touched by picks of its own label).  Returns
    (dets [K, 5] = cat(boxes[inds], final_scores[inds, None]), inds int64 [K]), by descending final score, ties by ascending index,
    NaN last.  No autograd."""
    what = "float32 (soft_nms is float32 only: pass .float(), or use soft_nms_pytorch)"
    _check_tensor("boxes", boxes, (torch.float32,), what, "soft_nms_pytorch")
    _check_tensor("scores", scores, (torch.float32,), what, "soft_nms_pytorch")
    thr, sig, low, code, off = _soft_nms_args(boxes, scores, iou_threshold, sigma, min_score, method, offset, labels)
    if boxes.shape[0] > MAX_SOFT_NMS_BOXES:
        raise ValueError("soft_nms takes at most MAX_SOFT_NMS_BOXES = %d boxes, got N = %d" % (MAX_SOFT_NMS_BOXES, boxes.shape[0]))
    final, inds = _soft_nms_op(boxes.detach(), scores.detach(), labels, thr, sig, low, code, off)
    return torch.cat([boxes.detach()[inds], final[:, None]], dim=1), inds


def _soft_nms_problem(boxes, scores, thr, sig, low, code, off):
    """One problem of soft_nms_pytorch: (the final scores, live-or-kept mask) of its boxes."""
    m = boxes.shape[0]
    x1, y1, x2, y2 = boxes.unbind(1)
    area = (x2 - x1 + off) * (y2 - y1 + off)
    s = scores.clone()
    live = torch.ones((m,), dtype=torch.bool, device=boxes.device)
    kept = torch.zeros_like(live)
    index = torch.arange(m, device=boxes.device)
    for _ in range(m):
        if not bool(live.any()):
            break
        number = live & ~torch.isnan(s)
        if bool(number.any()):
            cand = number & (s == s[number].max())
        else:
            cand = live                                                        # NaN scores only: in index order
        i = int(torch.where(cand, index, m).min())
        live[i] = False
        kept[i] = True
        zero = torch.zeros_like(s)
        w = torch.fmax(zero, torch.fmin(x2[i], x2) - torch.fmax(x1[i], x1) + off)
        h = torch.fmax(zero, torch.fmin(y2[i], y2) - torch.fmax(y1[i], y1) + off)
        inter = w * h
        ovr = inter / ((area[i] + area) - inter)
        ovr = torch.where(torch.isnan(ovr), zero, ovr)
        if code == 2:
            weight = torch.exp(-(ovr * ovr) / sig)
        elif code == 1:
            weight = torch.where(ovr >= thr, 1 - ovr, torch.ones_like(ovr))
        else:
            weight = torch.where(ovr >= thr, torch.zeros_like(ovr), torch.ones_like(ovr))
        s = torch.where(live, s * weight, s)
        live = live & ~(s < low)
    return s, kept


def soft_nms_pytorch(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method="linear", offset=0, labels=None):
    """soft_nms from torch operations under the same contract, one vectorised rescoring per pick (and a few host syncs): the fallback
    and the reference users can read, on any device, in float32 or float64 (the boxes' dtype; iou_threshold, sigma and min_score are
    rounded to float32 first either way).  Returns (dets [K, 5] in the boxes' dtype, inds int64 [K])."""
    for name, t in (("boxes", boxes), ("scores", scores)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError("%s must be float32 or float64, got %s" % (name, t.dtype))
    if boxes.dtype != scores.dtype:
        raise TypeError("boxes and scores must have one dtype, got %s and %s" % (boxes.dtype, scores.dtype))
    thr, sig, low, code, off = _soft_nms_args(boxes, scores, iou_threshold, sigma, min_score, method, offset, labels)
    boxes, scores = boxes.detach(), scores.detach()
    n = boxes.shape[0]
    final = scores.clone()
    kept = torch.zeros((n,), dtype=torch.bool, device=boxes.device)
    if labels is None:
        problems = [torch.arange(n, device=boxes.device)] if n else []
    else:
        problems = [(labels == v).nonzero()[:, 0] for v in torch.unique(labels)]
    for rows in problems:
        s, k = _soft_nms_problem(boxes[rows], scores[rows], thr, sig, low, code, off)
        final[rows] = s
        kept[rows] = k
    inds = kept.nonzero()[:, 0]
    inds = inds[_score_order(final[inds])]
    return torch.cat([boxes[inds], final[inds, None]], dim=1), inds


def roi_align_rotated(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True, clockwise=False):
    """mmcv.ops.roi_align_rotated: RoIAlign on the rotated sampling grid of rois [K, 6] (batch index, cx, cy, w, h, angle in radians):
    [K, C, oh, ow] (channels_last memory)."""
    _check_tensor("input", input, _MAP_DTYPES, _MAP_WHAT)
    if input.dim() != 4:
        raise ValueError("input must be [N, C, H, W], got shape %s" % (tuple(input.shape),))
    dtypes, what = _box_dtypes(input)
    _check_tensor("rois", rois, dtypes, what)
    _check_same_device(input, rois, "input", "rois")
    if rois.dim() != 2 or rois.shape[1] != 6:
        raise ValueError("rois must be a Tensor[K, 6] (batch index, cx, cy, w, h, angle), got shape %s" % (tuple(rois.shape),))
    oh, ow = _output_size(output_size)
    if int(sampling_ratio) > MAX_SAMPLING_RATIO:
        raise ValueError("sampling_ratio must be <= %d, got %d" % (MAX_SAMPLING_RATIO, sampling_ratio))
    return _roi_align_rotated(input, rois.float(), float(spatial_scale), oh, ow, int(sampling_ratio), bool(aligned), bool(clockwise))


def _riroi_orientations(num_orientations, channels):
    _check_int("num_orientations", num_orientations)
    if not 1 <= num_orientations <= MAX_RIROI_ORIENTATIONS:
        raise ValueError("num_orientations must lie in [1, %d], got %d" % (MAX_RIROI_ORIENTATIONS, num_orientations))
    if channels % num_orientations != 0:
        raise ValueError("num_orientations = %d must divide the channel count, got %d channels" % (num_orientations, channels))
    return num_orientations


def _riroi_rois(rois):
    if rois.dim() != 2 or rois.shape[1] != 6:
        raise ValueError("rois must be a Tensor[K, 6] (batch index, cx, cy, w, h, angle), got shape %s" % (tuple(rois.shape),))


def riroi_align_rotated(input, rois, output_size, spatial_scale=1.0, num_samples=0, num_orientations=8, clockwise=False):
    """mmcv.ops.riroi_align_rotated (ReDet's rotation-invariant RoI pooling): roi_align_rotated's pooled values of input [N, C n, H, W]
    (aligned off) with the n = num_orientations channels of every group rotated by the RoI's angle and blended between the two nearest
    orientations: [K, C n, oh, ow] (channels_last memory); differentiable in input."""
    _check_tensor("input", input, _MAP_DTYPES, _MAP_WHAT, "riroi_align_rotated_pytorch around a pooled tensor")
    if input.dim() != 4:
        raise ValueError("input must be [N, C * num_orientations, H, W], got shape %s" % (tuple(input.shape),))
    dtypes, what = _box_dtypes(input)
    _check_tensor("rois", rois, dtypes, what, "riroi_align_rotated_pytorch around a pooled tensor")
    _check_same_device(input, rois, "input", "rois")
    _riroi_rois(rois)
    oh, ow = _output_size(output_size)
    _check_int("num_samples", num_samples)
    if num_samples > MAX_SAMPLING_RATIO:
        raise ValueError("num_samples must be <= %d, got %d" % (MAX_SAMPLING_RATIO, num_samples))
    n = _riroi_orientations(num_orientations, input.shape[1])
    return _riroi_align_rotated(input, rois.float(), float(spatial_scale), oh, ow, num_samples, n, bool(clockwise))


def riroi_align_rotated_pytorch(pooled, rois, num_orientations=8):
    """riroi_align_rotated's blend from torch operations, on any device: pooled is S [K, C n, oh, ow], the result of roi_align_rotated
    (aligned=False, the opposite clockwise flag) or of any other pooling, rois [K, 6] the rows it was pooled with.  Per RoI
    f = float32(float64(angle) n / (2 pi)), ind = floor(f), l = f - ind, r = 1 - l, k = ind mod n, and out[c n + o] =
    r S[c n + (o - k) mod n] + l S[c n + (o - k + 1) mod n]; a RoI whose angle is not finite or whose |f| >= 2 ** 24 gives zeros.  Computed
    in float32 (float64 for a float64 S), returned in S's dtype; differentiable by autograd in S."""
    for name, t in (("pooled", pooled), ("rois", rois)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError("%s must be a floating-point torch.Tensor, got %s" % (name, t.dtype if isinstance(t, torch.Tensor)
                                                                                   else type(t).__name__))
    _check_same_device(pooled, rois, "pooled", "rois")
    if pooled.dim() != 4:
        raise ValueError("pooled must be [K, C * num_orientations, oh, ow], got shape %s" % (tuple(pooled.shape),))
    _riroi_rois(rois)
    if rois.shape[0] != pooled.shape[0]:
        raise ValueError("pooled and rois must hold the same K RoIs, got %d and %d" % (pooled.shape[0], rois.shape[0]))
    n = _riroi_orientations(num_orientations, pooled.shape[1])
    dtype = torch.float64 if pooled.dtype == torch.float64 else torch.float32
    k_rois, channels = pooled.shape[:2]
    if pooled.numel() == 0:
        return pooled.new_zeros(tuple(pooled.shape)) + pooled.sum() * 0
    angle = rois.detach()[:, 5].double()
    f = (angle * n / (2 * math.pi)).float()
    ok = torch.isfinite(angle) & (f.abs() < 2.0 ** 24)
    f = torch.where(ok, f, torch.zeros_like(f))
    ind = torch.floor(f)
    left = (f - ind).to(dtype)
    right = 1 - left
    k = torch.remainder(ind.long(), n)                                               # non-negative
    ch = torch.arange(channels, device=pooled.device)
    base, o = ch // n * n, ch % n
    first = base[None] + torch.remainder(o[None] - k[:, None], n)                    # [K, C n]
    second = base[None] + torch.remainder(o[None] - k[:, None] + 1, n)
    s = pooled.to(dtype)
    shape = (k_rois, channels) + tuple(pooled.shape[2:])
    a = s.gather(1, first[:, :, None, None].expand(shape)) * right[:, None, None, None]
    b = s.gather(1, second[:, :, None, None].expand(shape)) * left[:, None, None, None]
    out = torch.where(ok[:, None, None, None], a + b, torch.zeros_like(a))
    return out.to(pooled.dtype)


def _rfa_args(features, best_bboxes, points):
    """The shape rules rotated_feature_align and rotated_feature_align_pytorch share."""
    if features.dim() != 4:
        raise ValueError("features must be [N, C, H, W], got shape %s" % (tuple(features.shape),))
    n, _, h, w = features.shape
    if tuple(best_bboxes.shape) != (n, h, w, 5):
        raise ValueError("best_bboxes must be [N, H, W, 5] = %s (one (y, x, w, h, angle) row per pixel), got shape %s"
                         % ((n, h, w, 5), tuple(best_bboxes.shape)))
    _check_int("points", points)
    if points not in RFA_POINTS:
        raise ValueError("points must be 1 or 5, got %d" % points)
    if n * h * w * points * 4 > MAX_RFA_INDEX:
        raise ValueError("N H W points 4 = %d exceeds %d (the plan entries of the backward)" % (n * h * w * points * 4, MAX_RFA_INDEX))


def rotated_feature_align(features, best_bboxes, spatial_scale=1 / 8, points=1):
    """mmcv.ops.rotated_feature_align (R3Det's feature refinement module): every pixel adds to its own value the bilinear samples of its
    image at the centre (points=1) or the centre and the four corners (points=5) of its box row best_bboxes[n, h, w] =
    (y, x, w, h, angle): component 0 is the ROW coordinate.  [N, C, H, W] in the input's memory format; differentiable in features."""
    _check_tensor("features", features, _MAP_DTYPES, _MAP_WHAT, "rotated_feature_align_pytorch")
    dtypes, what = _box_dtypes(features)
    _check_tensor("best_bboxes", best_bboxes, dtypes, what, "rotated_feature_align_pytorch")
    _check_same_device(features, best_bboxes, "features", "best_bboxes")
    _rfa_args(features, best_bboxes, points)
    return _rotated_feature_align(features, best_bboxes.float(), float(spatial_scale), points)


def rotated_feature_align_pytorch(features, best_bboxes, spatial_scale=1 / 8, points=1):
    """rotated_feature_align from torch operations (index gathers), on any device, with autograd to features: the fallback, and what
    tools/ops_bench.py measures the kernels against.  features [N, C, H, W] of any floating dtype (16-bit maps compute in float32,
    float64 in float64), best_bboxes a floating-point [N, H, W, 5] of (y, x, w, h, angle) rows.  Returns [N, C, H, W] in the input's
    dtype."""
    for name, t in (("features", features), ("best_bboxes", best_bboxes)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError("%s must be a floating-point torch.Tensor, got %s" % (name, t.dtype if isinstance(t, torch.Tensor)
                                                                                   else type(t).__name__))
    _check_same_device(features, best_bboxes, "features", "best_bboxes")
    _rfa_args(features, best_bboxes, points)
    dtype = torch.float64 if features.dtype == torch.float64 else torch.float32
    n, c, h, w = features.shape
    if features.numel() == 0:
        return features.new_zeros((n, c, h, w)) + features.sum() * 0
    b = best_bboxes.detach().to(dtype)
    scale = float(spatial_scale)
    y0, x0 = b[..., 0] * scale, b[..., 1] * scale                          # [N, H, W]
    pts = [(x0, y0)]
    if points == 5:
        w2, h2, a = b[..., 2] * scale / 2, b[..., 3] * scale / 2, b[..., 4]
        ca, sa = torch.cos(a), torch.sin(a)
        wx, wy, hx, hy = ca * w2, sa * w2, -sa * h2, ca * h2
        pts += [((x0 + wx) + hx, (y0 + wy) + hy), ((x0 - wx) + hx, (y0 - wy) + hy), ((x0 - wx) - hx, (y0 - wy) - hy),
                ((x0 + wx) - hx, (y0 + wy) - hy)]
    x = features.to(dtype)
    flat = x.reshape(n, c, h * w)
    out = x
    zero = torch.zeros_like(y0)
    for px, py in pts:
        valid = (py >= -1) & (py <= h) & (px >= -1) & (px <= w)             # a NaN fails
        yl, yh, wyl, wyh = _border_axis_pytorch(torch.where(valid, py, zero), h)
        xl, xh, wxl, wxh = _border_axis_pytorch(torch.where(valid, px, zero), w)

        def cells(row, col):
            index = (row * w + col).reshape(n, 1, -1).expand(n, c, -1)
            return flat.gather(2, index).reshape(n, c, h, w)

        w1, w2_, w3, w4 = ((p * q)[:, None] for p, q in ((wyl, wxl), (wyl, wxh), (wyh, wxl), (wyh, wxh)))
        val = ((cells(yl, xl) * w1 + cells(yl, xh) * w2_) + cells(yh, xl) * w3) + cells(yh, xh) * w4
        out = out + torch.where(valid[:, None], val, torch.zeros_like(val))
    return out.to(features.dtype)


def _carafe_int(name, v, low, high, what=""):
    _check_int(name, v)
    if not low <= v <= high:
        raise ValueError("%s must lie in [%d, %d]%s, got %d" % (name, low, high, what, v))
    return v


def carafe(features, masks, kernel_size, group_size, scale_factor):
    """mmcv.ops.carafe: content-aware reassembly of features [N, C, H, W] with the per-pixel kernels masks [N, G * k * k, s * H, s * W]
    (normally a softmax over each group's k * k taps): [N, C, s * H, s * W], contiguous."""
    _check_tensor("features", features, _MAP_DTYPES, _MAP_WHAT)
    _check_tensor("masks", masks, _MAP_DTYPES, _MAP_WHAT)
    if features.dtype != masks.dtype:
        raise TypeError("features and masks must have one dtype (float32, float16 or bfloat16), got %s and %s" % (features.dtype, masks.dtype))
    _check_same_device(features, masks, "features", "masks")
    if features.dim() != 4:
        raise ValueError("features must be [N, C, H, W], got shape %s" % (tuple(features.shape),))
    if masks.dim() != 4:
        raise ValueError("masks must be [N, group_size * kernel_size ** 2, s * H, s * W], got shape %s" % (tuple(masks.shape),))
    k = _carafe_int("kernel_size", kernel_size, 1, MAX_CARAFE_KERNEL, " (MAX_CARAFE_KERNEL)")
    if k % 2 == 0:
        raise ValueError("kernel_size must be odd, got %d" % k)
    s = _carafe_int("scale_factor", scale_factor, 1, MAX_CARAFE_SCALE, " (MAX_CARAFE_SCALE)")
    n, c, h, w = features.shape
    g = _carafe_int("group_size", group_size, 1, 2 ** 31 - 1)
    if c % g != 0:
        raise ValueError("group_size must divide the channels of features, got group_size %d for %d channels" % (g, c))
    if h < 1 or w < 1:
        raise ValueError("features must have at least one cell, got shape %s" % (tuple(features.shape),))
    if tuple(masks.shape) != (n, g * k * k, s * h, s * w):
        raise ValueError("masks must be [N, group_size * kernel_size ** 2, s * H, s * W] = [%d, %d, %d, %d], got shape %s"
                         % (n, g * k * k, s * h, s * w, tuple(masks.shape)))
    if s * h * s * w > MAX_CARAFE_PLANE:
        raise ValueError("carafe is too large for the kernels' 32-bit indices inside a plane: s * H * s * W = %d > MAX_CARAFE_PLANE = %d"
                         % (s * h * s * w, MAX_CARAFE_PLANE))
    if n > 65535:
        raise ValueError("carafe takes at most 65535 images (the launch grid), got %d" % n)
    if g * ((c // g + CARAFE_RUN - 1) // CARAFE_RUN) > 65535:
        raise ValueError("carafe takes at most 65535 runs of %d channels over the groups (the launch grid), got %d for %d channels in %d "
                         "groups" % (CARAFE_RUN, g * ((c // g + CARAFE_RUN - 1) // CARAFE_RUN), c, g))
    return _carafe(features, masks, k, g, s)


def multi_scale_deformable_attn(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                                im2col_step=64):
    """mmcv.ops.multi_scale_deformable_attn: value [B, S, M, D] sampled at sampling_locations [B, Q, M, L, P, 2] on the L levels
    value_spatial_shapes [L, 2] / value_level_start_index [L] and mixed with attention_weights [B, Q, M, L, P]: [B, Q, M * D]."""
    _check_tensor("value", value, _MAP_DTYPES, _MAP_WHAT)
    dtypes, what = _box_dtypes(value)
    what = what.replace("input's", "value's")
    _check_tensor("sampling_locations", sampling_locations, dtypes, what)
    _check_tensor("attention_weights", attention_weights, dtypes, what)
    _check_tensor("value_spatial_shapes", value_spatial_shapes, (torch.int64,), "int64")
    _check_tensor("value_level_start_index", value_level_start_index, (torch.int64,), "int64")
    for name, t in (("value_spatial_shapes", value_spatial_shapes), ("value_level_start_index", value_level_start_index),
                    ("sampling_locations", sampling_locations), ("attention_weights", attention_weights)):
        _check_same_device(value, t, "value", name)
    if value.dim() != 4:
        raise ValueError("value must be [B, S, M, D], got shape %s" % (tuple(value.shape),))
    if sampling_locations.dim() != 6 or sampling_locations.shape[5] != 2:
        raise ValueError("sampling_locations must be [B, Q, M, L, P, 2], got shape %s" % (tuple(sampling_locations.shape),))
    b, s, m, d = value.shape
    q, levels, points = sampling_locations.shape[1], sampling_locations.shape[3], sampling_locations.shape[4]
    if tuple(sampling_locations.shape) != (b, q, m, levels, points, 2):
        raise ValueError("sampling_locations must be [B, Q, M, L, P, 2] with value's B = %d and M = %d, got shape %s"
                         % (b, m, tuple(sampling_locations.shape)))
    if tuple(attention_weights.shape) != (b, q, m, levels, points):
        raise ValueError("attention_weights must be [B, Q, M, L, P] = [%d, %d, %d, %d, %d], got shape %s"
                         % (b, q, m, levels, points, tuple(attention_weights.shape)))
    if tuple(value_spatial_shapes.shape) != (levels, 2):
        raise ValueError("value_spatial_shapes must be [L, 2] = [%d, 2], got shape %s" % (levels, tuple(value_spatial_shapes.shape)))
    if tuple(value_level_start_index.shape) != (levels,):
        raise ValueError("value_level_start_index must be [L] = [%d], got shape %s" % (levels, tuple(value_level_start_index.shape)))
    _check_int("im2col_step", im2col_step)
    if im2col_step < 1:
        raise ValueError("im2col_step must be at least 1, got %d" % im2col_step)
    if levels > MAX_MSDA_LEVELS:
        raise ValueError("multi_scale_deformable_attn takes at most MAX_MSDA_LEVELS = %d levels, got %d" % (MAX_MSDA_LEVELS, levels))
    if points > MAX_MSDA_POINTS:
        raise ValueError("multi_scale_deformable_attn takes at most MAX_MSDA_POINTS = %d points per level, got %d" % (MAX_MSDA_POINTS, points))
    if d > MAX_MSDA_CHANNELS:
        raise ValueError("multi_scale_deformable_attn takes at most MAX_MSDA_CHANNELS = %d channels per head, got %d" % (MAX_MSDA_CHANNELS, d))
    nb = min(b, im2col_step)
    if nb * s * m > MAX_MSDA_INDEX:
        raise ValueError("multi_scale_deformable_attn is too large for the kernels' 32-bit cell indices: %d images x S x M = %d > "
                         "MAX_MSDA_INDEX = %d (lower im2col_step)" % (nb, nb * s * m, MAX_MSDA_INDEX))
    if nb * q * m * levels * points * 4 > MAX_MSDA_INDEX:
        raise ValueError("multi_scale_deformable_attn is too large for the kernels' 32-bit plan indices: %d images x Q x M x L x P x 4 = %d "
                         "> MAX_MSDA_INDEX = %d (lower im2col_step)" % (nb, nb * q * m * levels * points * 4, MAX_MSDA_INDEX))
    return _ms_deform_attn(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step)


def multi_scale_deformable_attn_pytorch(value, value_spatial_shapes, sampling_locations, attention_weights):
    """mmcv.ops.multi_scale_deform_attn.multi_scale_deformable_attn_pytorch: the same operator composed from one F.grid_sample per
    level, on any device (S must equal the sum of H_l * W_l; the shapes are read on the host)."""
    bs, _, num_heads, embed_dims = value.shape
    _, num_queries, num_heads, num_levels, num_points, _ = sampling_locations.shape
    shapes = [(int(h), int(w)) for h, w in value_spatial_shapes.tolist()]
    value_list = value.split([h * w for h, w in shapes], dim=1)
    sampling_grids = 2 * sampling_locations - 1
    sampling_value_list = []
    for level, (h, w) in enumerate(shapes):
        value_l = value_list[level].flatten(2).transpose(1, 2).reshape(bs * num_heads, embed_dims, h, w)
        grid_l = sampling_grids[:, :, :, level].transpose(1, 2).flatten(0, 1)
        sampling_value_list.append(torch.nn.functional.grid_sample(value_l, grid_l, mode="bilinear", padding_mode="zeros",
                                                                   align_corners=False))
    attention_weights = attention_weights.transpose(1, 2).reshape(bs * num_heads, 1, num_queries, num_levels * num_points)
    output = (torch.stack(sampling_value_list, dim=-2).flatten(-2) * attention_weights).sum(-1)
    return output.view(bs, num_heads * embed_dims, num_queries).transpose(1, 2).contiguous()


_DCN_NAMES = ("kernel_size", "stride", "padding", "dilation")                                                      # of dcnv3(), dcnv4()
_DCN_APPLY_NAMES = ("kernel_h, kernel_w", "stride_h, stride_w", "pad_h, pad_w", "dilation_h, dilation_w")          # of the Functions


def _dcn_pairs(names, kernel, stride, pad, dil):
    """kernel, stride, pad and dil as pairs (h, w) of ints, under the caller's names for them."""
    return _int_pair(names[0], kernel, 1), _int_pair(names[1], stride, 1), _int_pair(names[2], pad, 0), _int_pair(names[3], dil, 1)


def _dcn_group_channels(input, group):
    """The group rules of dcnv3() and dcnv4(), which have no group_channels argument: it follows from input."""
    _check_int("group", group)
    if group < 1:
        raise ValueError("group must be at least 1, got %d" % group)
    if isinstance(input, torch.Tensor) and input.dim() == 4 and input.shape[3] % group != 0:
        raise ValueError("input's %d channels must be divisible by group, got %d" % (input.shape[3], group))
    return input.shape[3] // group if isinstance(input, torch.Tensor) and input.dim() == 4 else 1


def _dcn_args(op, input, learned, kernel, stride, pad, dil, group, group_channels, offset_scale, im2col_step, remove_center=False):
    """The argument rules of op "dcnv3" (dcnv3 / DCNv3Function, learned = (offset, mask)) or "dcnv4" (dcnv4 / DCNv4Function, learned =
    (offset_mask,), with its remove_center), kernel, stride, pad and dil pairs (h, w) of ints; returns what the custom op takes after
    its tensors."""
    v4 = op == "dcnv4"
    names = ("offset_mask",) if v4 else ("offset", "mask")
    _check_tensor("input", input, _MAP_DTYPES, _MAP_WHAT)
    dtypes, what = _box_dtypes(input)
    for name, t in zip(names, learned):
        _check_tensor(name, t, dtypes, what)
    for name, t in zip(names, learned):
        _check_same_device(input, t, "input", name)
    if input.dim() != 4:
        raise ValueError("input must be [N, H, W, C] (channels last), got shape %s" % (tuple(input.shape),))
    for name, v in (("group", group), ("group_channels", group_channels), ("im2col_step", im2col_step)):
        _check_int(name, v)
    if v4 and not isinstance(remove_center, (bool, int)):
        raise TypeError("remove_center must be a bool, got %r" % (remove_center,))
    if v4 and remove_center not in (0, 1):
        raise ValueError("remove_center must be False or True (0 or 1), got %r" % (remove_center,))
    if isinstance(offset_scale, bool) or not isinstance(offset_scale, (int, float)):
        raise TypeError("offset_scale must be a float, got %r" % (offset_scale,))
    if not math.isfinite(offset_scale):
        raise ValueError("offset_scale must be finite, got %r" % (offset_scale,))
    if im2col_step < 1:
        raise ValueError("im2col_step must be at least 1, got %d" % im2col_step)
    if group < 1:
        raise ValueError("group must be at least 1, got %d" % group)
    n, h, w, c = input.shape
    if group * group_channels != c:
        raise ValueError("group * group_channels must equal input's %d channels, got group %d and group_channels %d"
                         % (c, group, group_channels))
    if not 1 <= group_channels <= MAX_DCNV3_CHANNELS:
        raise ValueError("group_channels must lie in [1, MAX_DCNV3_CHANNELS = %d], got %d" % (MAX_DCNV3_CHANNELS, group_channels))
    if not (1 <= kernel[0] <= MAX_DCNV3_KERNEL and 1 <= kernel[1] <= MAX_DCNV3_KERNEL):
        raise ValueError("kernel_size must lie in [1, MAX_DCNV3_KERNEL = %d], got %r" % (MAX_DCNV3_KERNEL, tuple(kernel)))
    if v4 and remove_center and (kernel[0] != kernel[1] or kernel[0] % 2 == 0 or kernel[0] < 3):
        raise ValueError("remove_center requires a square kernel of odd size >= 3, got %r" % (tuple(kernel),))
    for name, v, low in (("stride", stride, 1), ("padding", pad, 0), ("dilation", dil, 1)):
        if not (low <= v[0] <= MAX_DCNV3_STEP and low <= v[1] <= MAX_DCNV3_STEP):
            raise ValueError("%s must lie in [%d, MAX_DCNV3_STEP = %d], got %r" % (name, low, MAX_DCNV3_STEP, tuple(v)))
    if h > MAX_DCNV3_SIDE or w > MAX_DCNV3_SIDE:
        raise ValueError("input must have H and W of at most MAX_DCNV3_SIDE = %d, got shape %s" % (MAX_DCNV3_SIDE, tuple(input.shape)))
    p = _dcnv4_points(kernel[0], kernel[1], v4 and remove_center)
    ho, wo = _dcnv3_out_size(h, kernel[0], stride[0], pad[0], dil[0]), _dcnv3_out_size(w, kernel[1], stride[1], pad[1], dil[1])
    if v4:
        rec = _dcnv4_record(group, p)
        if tuple(learned[0].shape) != (n, ho, wo, rec):
            raise ValueError("offset_mask must be [N, Ho, Wo, L] = [%d, %d, %d, %d] with L = ceil(G P 3 / 8) 8 for G = %d groups of P = %d "
                             "points (2 P offsets, then P masks; the record padded to a multiple of 8), got shape %s"
                             % (n, ho, wo, rec, group, p, tuple(learned[0].shape)))
    else:
        for name, t, what, last in zip(names, learned, ("G K 2", "G K"), (group * p * 2, group * p)):
            if tuple(t.shape) != (n, ho, wo, last):
                raise ValueError("%s must be [N, Ho, Wo, %s] = [%d, %d, %d, %d], got shape %s" % (name, what, n, ho, wo, last, tuple(t.shape)))
    nb = min(n, im2col_step)
    if nb * h * w * group > MAX_MSDA_INDEX:
        raise ValueError("input is too large for the kernels' 32-bit cell indices: %d images x H x W x G = %d > MAX_MSDA_INDEX = %d "
                         "(lower im2col_step)" % (nb, nb * h * w * group, MAX_MSDA_INDEX))
    if nb * ho * wo * group * p * 4 > MAX_MSDA_INDEX:
        raise ValueError("%s is too large for the kernels' 32-bit plan indices: %d images x Ho x Wo x G x %s x 4 = %d > MAX_MSDA_INDEX = "
                         "%d (lower im2col_step)" % (names[0], nb, "P" if v4 else "K", nb * ho * wo * group * p * 4, MAX_MSDA_INDEX))
    return (kernel[0], kernel[1], stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], group, group_channels, float(offset_scale),
            im2col_step) + ((bool(remove_center),) if v4 else ())


def dcnv3(input, offset, mask, kernel_size, stride=1, padding=0, dilation=1, group=1, offset_scale=1.0, im2col_step=256):
    """DCNv3's sampling core: input [N, H, W, G Gc] sampled at kh kw learned positions per output pixel and group (offset
    [N, Ho, Wo, G K 2], pairs (dx, dy)), the samples weighted by mask [N, Ho, Wo, G K] and summed: [N, Ho, Wo, G Gc]."""
    pairs = _dcn_pairs(_DCN_NAMES, kernel_size, stride, padding, dilation)
    return _dcnv3(input, offset, mask, *_dcn_args("dcnv3", input, (offset, mask), *pairs, group, _dcn_group_channels(input, group),
                                                  offset_scale, im2col_step))


def dcnv3_core_pytorch(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                       group_channels, offset_scale):
    """InternImage's dcnv3_core_pytorch: the same operator composed from F.pad and one F.grid_sample, on any device.  It materialises an
    [N G, Gc, Ho Wo, K] tensor."""
    n, ho, wo, k = input.shape[0], offset.shape[1], offset.shape[2], kernel_h * kernel_w
    return _dcn_core_pytorch(input, offset.view(n, ho, wo, group, k, 2), mask.view(n, ho * wo, group, k), None, kernel_h, kernel_w,
                             stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels, offset_scale)


def _dcn_core_pytorch(input, offset, mask, points, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                      group_channels, offset_scale):
    """The composition behind dcnv3_core_pytorch and dcnv4_core_pytorch: offset [N, Ho, Wo, G, P, 2] and mask [N, Ho Wo, G, P], views of
    the callers' tensors.  points: None for all kh kw grid points, laid out on the device as dcnv3_core_pytorch always has; dcnv4's list
    of the (i, j) it keeps, whose P integer parts come from the host as dcnv4_core_pytorch's always have."""
    F = torch.nn.functional
    x = F.pad(input, [0, 0, pad_w, pad_w, pad_h, pad_h])
    n, hp, wp, _ = x.shape
    ho, wo, p = offset.shape[1], offset.shape[2], offset.shape[4]
    bx, by = (dilation_w * (kernel_w - 1)) // 2, (dilation_h * (kernel_h - 1)) // 2
    new = lambda v: torch.as_tensor(v, dtype=x.dtype, device=x.device)     # noqa: E731
    steps = lambda count: torch.arange(count, dtype=x.dtype, device=x.device)   # noqa: E731
    ref = torch.stack(torch.broadcast_tensors(((steps(wo) * stride_w + bx + 0.5) / wp).view(1, wo),
                                              ((steps(ho) * stride_h + by + 0.5) / hp).view(ho, 1)), -1)           # [Ho, Wo, 2] (x, y)
    if points is None:
        grid = torch.stack([((steps(kernel_w) * dilation_w - bx) / wp).repeat_interleave(kernel_h),                 # x: the outer index
                            ((steps(kernel_h) * dilation_h - by) / hp).repeat(kernel_w)], -1) * offset_scale        # [K, 2]
    else:
        grid = torch.stack([new([float(i * dilation_w - bx) for i, j in points]) / wp,
                            new([float(j * dilation_h - by) for i, j in points]) / hp], -1) * offset_scale          # [P, 2]
    loc = ref.view(1, ho, wo, 1, 1, 2) + grid.view(1, 1, 1, 1, p, 2) + offset * offset_scale / new([wp, hp])
    maps = x.reshape(n, hp * wp, group, group_channels).permute(0, 2, 3, 1).reshape(n * group, group_channels, hp, wp)
    grids = (2 * loc - 1).view(n, ho * wo, group, p, 2).transpose(1, 2).flatten(0, 1)                               # [N G, Q, P, 2]
    sampled = F.grid_sample(maps, grids, mode="bilinear", padding_mode="zeros", align_corners=False)                # [N G, Gc, Q, P]
    weights = mask.transpose(1, 2).reshape(n * group, 1, ho * wo, p)
    out = (sampled * weights).sum(-1).view(n, group * group_channels, ho * wo)
    return out.transpose(1, 2).reshape(n, ho, wo, group * group_channels).contiguous()


def dcnv4(input, offset_mask, kernel_size, stride=1, padding=0, dilation=1, group=1, offset_scale=1.0, im2col_step=256,
          remove_center=False):
    """DCNv4's sampling core: input [N, H, W, G Gc] sampled at P learned positions per output pixel and group, the samples weighted by
    unnormalised masks and summed: [N, Ho, Wo, G Gc].  offset_mask [N, Ho, Wo, L] holds, per pixel and group, the 2 P offsets (pairs
    (dx, dy)) and then the P masks, the record padded to L = ceil(G P 3 / 8) 8; P = kh kw, less the centre point with remove_center."""
    pairs = _dcn_pairs(_DCN_NAMES, kernel_size, stride, padding, dilation)
    return _dcnv4(input, offset_mask, *_dcn_args("dcnv4", input, (offset_mask,), *pairs, group, _dcn_group_channels(input, group),
                                                 offset_scale, im2col_step, remove_center))


def dcnv4_core_pytorch(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                       group_channels, offset_scale, remove_center):
    """The same operator composed from F.pad and one F.grid_sample, on any device, differentiable to input and offset_mask: it unpacks
    the record, drops the centre location when asked and applies no softmax.  It materialises an [N G, Gc, Ho Wo, P] tensor."""
    n, ho, wo = input.shape[0], offset_mask.shape[1], offset_mask.shape[2]
    points = [(i, j) for i in range(kernel_w) for j in range(kernel_h)]                                             # x: the outer index
    if remove_center:
        points.remove((kernel_w // 2, kernel_h // 2))
    p = len(points)
    rec = offset_mask[..., :group * p * 3].reshape(n, ho, wo, group, p * 3)
    return _dcn_core_pytorch(input, rec[..., :2 * p].reshape(n, ho, wo, group, p, 2), rec[..., 2 * p:].reshape(n, ho * wo, group, p),
                             points, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
                             offset_scale)


def _ms_features(features):
    if not isinstance(features, (list, tuple)):
        raise TypeError("features must be a list of tensors, got %s" % type(features).__name__)
    if not 1 <= len(features) <= MAX_LEVELS:
        raise ValueError("features must hold 1 to %d feature maps, got %d" % (MAX_LEVELS, len(features)))
    for i, f in enumerate(features):
        _check_tensor("features[%d]" % i, f, _MAP_DTYPES, _MAP_WHAT)
        if f.dtype != features[0].dtype:
            raise TypeError("every feature map must have one dtype (float32, float16 or bfloat16): features[0] is %s, features[%d] is %s"
                            % (features[0].dtype, i, f.dtype))
        if f.dim() != 4:
            raise ValueError("features[%d] must be [N, C, H, W], got shape %s" % (i, tuple(f.shape)))
        _check_same_device(features[0], f, "features[0]", "features[%d]" % i)
        if f.shape[:2] != features[0].shape[:2]:
            raise ValueError("every feature map must have the same N and C: features[0] is %s, features[%d] is %s"
                             % (tuple(features[0].shape), i, tuple(f.shape)))


def _level_range(scales):
    """torchvision's _setup_scales: k_min, k_max = int(-log2(scale)) of the first and the last level, log2 in float32."""
    k_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
    k_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
    return int(k_min), int(k_max)


def _infer_scales(features, image_shapes):
    """torchvision's _setup_scales / _infer_scale: per level 2 ** round(log2(H_l / max_h)) (float32 log2, round half to even), max_h the
    largest image height; only H decides."""
    if not image_shapes:
        raise ValueError("image_shapes must not be empty")
    max_h = max(int(s[0]) for s in image_shapes)
    return [2 ** float(torch.tensor(float(f.shape[2]) / float(max_h)).log2().round()) for f in features]


def _multi_scale_roi_align(features, boxes, output_size, scales, sampling_ratio, canonical_scale, canonical_level, k_range):
    _ms_features(features)
    rois = _roi_input(features[0], boxes)
    oh, ow = _output_size(output_size)
    if int(sampling_ratio) > MAX_SAMPLING_RATIO:
        raise ValueError("sampling_ratio must be <= %d, got %d" % (MAX_SAMPLING_RATIO, sampling_ratio))
    if len(scales) != len(features):
        raise ValueError("spatial_scales must hold one scale per feature map: %d scales, %d maps" % (len(scales), len(features)))
    k_min, k_max = _level_range(scales) if k_range is None else k_range
    return _ms_roi_align(list(features), rois, [float(s) for s in scales], oh, ow, int(sampling_ratio), float(canonical_scale),
                         float(canonical_level), k_min, k_max)


def multi_scale_roi_align(features, boxes, output_size, spatial_scales, sampling_ratio=-1, canonical_scale=224, canonical_level=4):
    """torchvision.ops.MultiScaleRoIAlign's pooling on explicit levels: [K, C, oh, ow] (channels_last memory).  features: 1 to 8
    maps [N, C, H_l, W_l] (the same N, C and dtype: float32, float16 or bfloat16), finest first; spatial_scales: one per map.  Each RoI goes to level
    floor(canonical_level + log2(sqrt(area) / canonical_scale) + 1e-6), clamped to [k_min, k_max] = int(-log2) of the first and the last
    scale, minus k_min, and is pooled there by roi_align(aligned=False); a RoI without a level (negative or NaN area, an index outside the
    maps) pools to zeros.  One map: every RoI is pooled on it."""
    return _multi_scale_roi_align(features, boxes, output_size, list(spatial_scales), sampling_ratio, canonical_scale, canonical_level,
                                  None)


class MultiScaleRoIAlign(torch.nn.Module):
    """torchvision.ops.MultiScaleRoIAlign: forward(x, boxes, image_shapes) pools boxes (list[Tensor[L_i, 4]] or Tensor[K, 5]) from the
    maps of the dict x named in featmap_names (in x's order).  The scales are inferred from the maps and image_shapes on the first call
    and kept, as torchvision does."""

    def __init__(self, featmap_names, output_size, sampling_ratio, *, canonical_scale=224, canonical_level=4):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size)
        self.featmap_names = featmap_names
        self.sampling_ratio = sampling_ratio
        self.output_size = tuple(output_size)
        self.scales = None
        self.canonical_scale = canonical_scale
        self.canonical_level = canonical_level
        self._k_range = None

    def forward(self, x, boxes, image_shapes):
        features = [v for k, v in x.items() if k in self.featmap_names]
        if not features:
            raise ValueError("none of featmap_names %r is a key of x" % (list(self.featmap_names),))
        if self.scales is None or self._k_range is None:
            scales = _infer_scales(features, image_shapes)
            self._k_range = _level_range(scales)
            self.scales = scales
        return _multi_scale_roi_align(features, boxes, self.output_size, self.scales, self.sampling_ratio, self.canonical_scale,
                                      self.canonical_level, self._k_range)

    def extra_repr(self):
        return "featmap_names=%s, output_size=%s, sampling_ratio=%s" % (self.featmap_names, self.output_size, self.sampling_ratio)


class RoIAlign(torch.nn.Module):
    """torchvision.ops.RoIAlign."""

    def __init__(self, output_size, spatial_scale, sampling_ratio, aligned=False):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio
        self.aligned = aligned

    def forward(self, input, rois):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.aligned)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s, sampling_ratio=%s, aligned=%s" % (
            self.output_size, self.spatial_scale, self.sampling_ratio, self.aligned)


class RoIAlignRotated(torch.nn.Module):
    """mmcv.ops.RoIAlignRotated."""

    def __init__(self, output_size, spatial_scale, sampling_ratio=0, aligned=True, clockwise=False):
        super().__init__()
        self.output_size = _output_size(output_size)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)
        self.aligned = bool(aligned)
        self.clockwise = bool(clockwise)

    def forward(self, input, rois):
        return roi_align_rotated(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.aligned, self.clockwise)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s, sampling_ratio=%s, aligned=%s, clockwise=%s" % (
            self.output_size, self.spatial_scale, self.sampling_ratio, self.aligned, self.clockwise)


class RiRoIAlignRotated(torch.nn.Module):
    """mmcv.ops.RiRoIAlignRotated (ReDet): its argument names; input [N, C * num_orientations, H, W] and rois [K, 6]."""

    def __init__(self, out_size, spatial_scale, num_samples=0, num_orientations=8, clockwise=False):
        super().__init__()
        self.out_size = _output_size(out_size)
        self.spatial_scale = float(spatial_scale)
        self.num_samples = int(num_samples)
        self.num_orientations = int(num_orientations)
        self.clockwise = bool(clockwise)

    def forward(self, features, rois):
        return riroi_align_rotated(features, rois, self.out_size, self.spatial_scale, self.num_samples, self.num_orientations,
                                   self.clockwise)

    def extra_repr(self):
        return "out_size=%s, spatial_scale=%s, num_samples=%s, num_orientations=%s, clockwise=%s" % (
            self.out_size, self.spatial_scale, self.num_samples, self.num_orientations, self.clockwise)


class RotatedFeatureAlign(torch.nn.Module):
    """rotated_feature_align as a module: features [N, C, H, W] and best_bboxes [N, H, W, 5] of (y, x, w, h, angle) rows."""

    def __init__(self, spatial_scale=1 / 8, points=1):
        super().__init__()
        if points not in RFA_POINTS:
            raise ValueError("points must be 1 or 5, got %r" % (points,))
        self.spatial_scale = float(spatial_scale)
        self.points = points

    def forward(self, features, best_bboxes):
        return rotated_feature_align(features, best_bboxes, self.spatial_scale, self.points)

    def extra_repr(self):
        return "spatial_scale=%s, points=%d" % (self.spatial_scale, self.points)


class RoIPool(torch.nn.Module):
    """torchvision.ops.RoIPool."""

    def __init__(self, output_size, spatial_scale):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale

    def forward(self, input, rois):
        return roi_pool(input, rois, self.output_size, self.spatial_scale)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s" % (self.output_size, self.spatial_scale)


class PSRoIPool(torch.nn.Module):
    """torchvision.ops.PSRoIPool."""

    def __init__(self, output_size, spatial_scale):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale

    def forward(self, input, rois):
        return ps_roi_pool(input, rois, self.output_size, self.spatial_scale)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s" % (self.output_size, self.spatial_scale)


class PSRoIAlign(torch.nn.Module):
    """torchvision.ops.PSRoIAlign."""

    def __init__(self, output_size, spatial_scale, sampling_ratio):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio

    def forward(self, input, rois):
        return ps_roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s, sampling_ratio=%s" % (self.output_size, self.spatial_scale, self.sampling_ratio)


class DeformConv2d(torch.nn.Module):
    """torchvision.ops.DeformConv2d: parameters weight [out, in / groups, kh, kw] and bias [out] (or None), initialised as nn.Conv2d's."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        if in_channels % groups != 0:
            raise ValueError("in_channels must be divisible by groups")
        if out_channels % groups != 0:
            raise ValueError("out_channels must be divisible by groups")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _int_pair("kernel_size", kernel_size, 1)
        self.stride = _int_pair("stride", stride, 1)
        self.padding = _int_pair("padding", padding, 0)
        self.dilation = _int_pair("dilation", dilation, 1)
        self.groups = groups
        self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels // groups, self.kernel_size[0], self.kernel_size[1]))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.weight.shape[1] * self.weight.shape[2] * self.weight.shape[3]
            bound = 1 / math.sqrt(fan_in)
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input, offset, mask=None):
        weight, bias = self.weight, self.bias
        if isinstance(input, torch.Tensor) and input.dtype in _HALF:
            # mmcv's AMP rule: a 16-bit input takes the other tensors to its dtype; the casts are differentiable, so the float32
            # parameters receive float32 gradients
            weight = weight.to(input.dtype)
            bias = None if bias is None else bias.to(input.dtype)
            offset = offset.to(input.dtype) if isinstance(offset, torch.Tensor) else offset
            mask = mask.to(input.dtype) if isinstance(mask, torch.Tensor) else mask
        return deform_conv2d(input, offset, weight, bias, stride=self.stride, padding=self.padding, dilation=self.dilation, mask=mask)

    def __repr__(self):
        s = "%s(%s, %s, kernel_size=%s, stride=%s" % (self.__class__.__name__, self.in_channels, self.out_channels, self.kernel_size,
                                                        self.stride)
        s += ", padding=%s" % (self.padding,) if self.padding != (0, 0) else ""
        s += ", dilation=%s" % (self.dilation,) if self.dilation != (1, 1) else ""
        s += ", groups=%s" % self.groups if self.groups != 1 else ""
        s += ", bias=False" if self.bias is None else ""
        return s + ")"


class DeformRoIPool(torch.nn.Module):
    """mmcv.ops.DeformRoIPool: deformable RoI pooling with the offset given by the caller (None: aligned RoIAlign)."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1):
        super().__init__()
        self.output_size = _output_size(output_size)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)
        self.gamma = float(gamma)

    def forward(self, input, rois, offset=None):
        return deform_roi_pool(input, rois, offset, self.output_size, self.spatial_scale, self.sampling_ratio, self.gamma)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s, sampling_ratio=%s, gamma=%s" % (
            self.output_size, self.spatial_scale, self.sampling_ratio, self.gamma)


class PrRoIPool(torch.nn.Module):
    """mmcv.ops.PrRoIPool: Precise RoI Pooling, differentiable in the map and in the boxes."""

    def __init__(self, output_size, spatial_scale=1.0):
        super().__init__()
        self.output_size = _output_size(output_size)
        self.spatial_scale = float(spatial_scale)

    def forward(self, input, rois):
        return prroi_pool(input, rois, self.output_size, self.spatial_scale)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%s" % (self.output_size, self.spatial_scale)


class BorderAlign(torch.nn.Module):
    """mmcv.ops.BorderAlign: BorderDet's border pooling, input [N, 4 C, H, W] and boxes [N, K, 4] to [N, C, K, 4]."""

    def __init__(self, pool_size):
        super().__init__()
        self.pool_size = _border_pool_size(pool_size)

    def forward(self, input, boxes):
        return border_align(input, boxes, self.pool_size)

    def __repr__(self):
        return "%s(pool_size=%d)" % (self.__class__.__name__, self.pool_size)


def _zero_last(stack, index):
    torch.nn.init.zeros_(stack[index].weight)
    torch.nn.init.zeros_(stack[index].bias)


class DeformRoIPoolPack(DeformRoIPool):
    """mmcv.ops.DeformRoIPoolPack (DCN v1): pools without offset, computes the offset from the pooled features (flattened in the logical
    (C, oh, ow) order) with offset_fc, whose last layer starts at zero, and pools again with it."""

    def __init__(self, output_size, output_channels, deform_fc_channels=1024, spatial_scale=1.0, sampling_ratio=0, gamma=0.1):
        super().__init__(output_size, spatial_scale, sampling_ratio, gamma)
        self.output_channels = output_channels
        self.deform_fc_channels = deform_fc_channels
        oh, ow = self.output_size
        nn = torch.nn
        self.offset_fc = nn.Sequential(nn.Linear(oh * ow * output_channels, deform_fc_channels), nn.ReLU(inplace=True),
                                       nn.Linear(deform_fc_channels, deform_fc_channels), nn.ReLU(inplace=True),
                                       nn.Linear(deform_fc_channels, oh * ow * 2))
        _zero_last(self.offset_fc, 4)

    def _pool(self, input, rois):
        """(the pooled features without offset flattened [K, C * oh * ow], the pooled features with the learned offset)"""
        if input.dim() != 4 or input.shape[1] != self.output_channels:
            raise ValueError("input must be [N, %d, H, W] (output_channels), got shape %s" % (self.output_channels, tuple(input.shape)))
        oh, ow = self.output_size
        x = deform_roi_pool(input, rois, None, self.output_size, self.spatial_scale, self.sampling_ratio, self.gamma)
        flat = x.reshape(x.shape[0], -1)                                   # logical (C, oh, ow) order, whatever the memory format
        offset = self.offset_fc(flat).view(x.shape[0], 2, oh, ow)
        return flat, deform_roi_pool(input, rois, offset, self.output_size, self.spatial_scale, self.sampling_ratio, self.gamma)

    def forward(self, input, rois):
        return self._pool(input, rois)[1]

    def extra_repr(self):
        return "%s, output_channels=%s, deform_fc_channels=%s" % (super().extra_repr(), self.output_channels, self.deform_fc_channels)


class ModulatedDeformRoIPoolPack(DeformRoIPoolPack):
    """mmcv.ops.ModulatedDeformRoIPoolPack (DCN v2): DeformRoIPoolPack times a learned per-bin mask [K, 1, oh, ow] in (0, 1), which is
    sigmoid(mask_fc(.)) with a zero-initialised last layer: 0.5 at the start."""

    def __init__(self, output_size, output_channels, deform_fc_channels=1024, spatial_scale=1.0, sampling_ratio=0, gamma=0.1):
        super().__init__(output_size, output_channels, deform_fc_channels, spatial_scale, sampling_ratio, gamma)
        oh, ow = self.output_size
        nn = torch.nn
        self.mask_fc = nn.Sequential(nn.Linear(oh * ow * output_channels, deform_fc_channels), nn.ReLU(inplace=True),
                                     nn.Linear(deform_fc_channels, oh * ow), nn.Sigmoid())
        _zero_last(self.mask_fc, 2)

    def forward(self, input, rois):
        flat, pooled = self._pool(input, rois)
        oh, ow = self.output_size
        return pooled * self.mask_fc(flat).view(flat.shape[0], 1, oh, ow)


class CARAFE(torch.nn.Module):
    """mmcv.ops.CARAFE: carafe with the masks given by the caller."""

    def __init__(self, kernel_size, group_size, scale_factor):
        super().__init__()
        self.kernel_size = int(kernel_size)
        self.group_size = int(group_size)
        self.scale_factor = int(scale_factor)

    def forward(self, features, masks):
        return carafe(features, masks, self.kernel_size, self.group_size, self.scale_factor)

    def extra_repr(self):
        return "kernel_size=%s, group_size=%s, scale_factor=%s" % (self.kernel_size, self.group_size, self.scale_factor)


class CARAFEPack(torch.nn.Module):
    """mmcv.ops.CARAFEPack: the upsampler with its kernel predictor.  channel_compressor (1 x 1) and content_encoder predict
    up_group * up_kernel ** 2 * scale_factor ** 2 channels at the low resolution; pixel_shuffle spreads them over the s x s sub-pixels, a
    softmax over the up_kernel ** 2 taps of each group normalises them, and carafe reassembles x with them."""

    def __init__(self, channels, scale_factor, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1, compressed_channels=64):
        super().__init__()
        self.channels = channels
        self.scale_factor = scale_factor
        self.up_kernel = up_kernel
        self.up_group = up_group
        self.encoder_kernel = encoder_kernel
        self.encoder_dilation = encoder_dilation
        self.compressed_channels = compressed_channels
        self.channel_compressor = torch.nn.Conv2d(channels, compressed_channels, 1)
        self.content_encoder = torch.nn.Conv2d(compressed_channels, up_kernel * up_kernel * up_group * scale_factor * scale_factor,
                                               encoder_kernel, padding=int((encoder_kernel - 1) * encoder_dilation / 2),
                                               dilation=encoder_dilation)
        self.init_weights()

    def init_weights(self):
        for m in (self.channel_compressor, self.content_encoder):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.zeros_(m.bias)
        torch.nn.init.normal_(self.content_encoder.weight, mean=0.0, std=0.001)
        torch.nn.init.zeros_(self.content_encoder.bias)

    def kernel_normalizer(self, mask):
        """pixel_shuffle to the high resolution, then a softmax over the up_kernel ** 2 taps of each group."""
        mask = torch.nn.functional.pixel_shuffle(mask, self.scale_factor)
        n, c, h, w = mask.shape
        k2 = self.up_kernel * self.up_kernel
        return torch.softmax(mask.view(n, c // k2, k2, h, w), dim=2).view(n, c, h, w).contiguous()

    def masks(self, x):
        return self.kernel_normalizer(self.content_encoder(self.channel_compressor(x)))

    def forward(self, x):
        return carafe(x, self.masks(x), self.up_kernel, self.up_group, self.scale_factor)

    def extra_repr(self):
        return "channels=%s, scale_factor=%s, up_kernel=%s, up_group=%s, encoder_kernel=%s, encoder_dilation=%s, compressed_channels=%s" % (
            self.channels, self.scale_factor, self.up_kernel, self.up_group, self.encoder_kernel, self.encoder_dilation,
            self.compressed_channels)


class MultiScaleDeformableAttnFunction:
    """mmcv.ops.MultiScaleDeformableAttnFunction: .apply(value, value_spatial_shapes, value_level_start_index, sampling_locations,
    attention_weights, im2col_step), mmcv's six positional arguments, on frcnn::ms_deform_attn (whose autograd is registered with
    the custom op)."""

    @staticmethod
    def apply(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step):
        return multi_scale_deformable_attn(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                                           im2col_step)


class MultiScaleDeformableAttention(torch.nn.Module):
    """mmcv.ops.MultiScaleDeformableAttention: the attention module of Deformable DETR.  sampling_offsets and attention_weights
    predict, from the query, P offsets per head and level around the reference points and a softmax over L * P weights; value_proj
    projects the value, the sampler mixes it, output_proj projects back; dropout and the identity residual close the layer."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1, batch_first=False,
                 value_proj_ratio=1.0):
        super().__init__()
        if embed_dims % num_heads != 0:
            raise ValueError("embed_dims must be divisible by num_heads, got %d and %d" % (embed_dims, num_heads))
        self.embed_dims = embed_dims
        self.num_heads = num_heads
        self.num_levels = num_levels
        self.num_points = num_points
        self.im2col_step = im2col_step
        self.batch_first = batch_first
        self.dropout = torch.nn.Dropout(dropout)
        self.sampling_offsets = torch.nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = torch.nn.Linear(embed_dims, num_heads * num_levels * num_points)
        value_proj_size = int(embed_dims * value_proj_ratio)
        self.value_proj = torch.nn.Linear(embed_dims, value_proj_size)
        self.output_proj = torch.nn.Linear(value_proj_size, embed_dims)
        self.init_weights()

    def init_weights(self):
        torch.nn.init.zeros_(self.sampling_offsets.weight)
        thetas = torch.arange(self.num_heads, dtype=torch.float32) * (2.0 * math.pi / self.num_heads)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(self.num_heads, 1, 1, 2).repeat(1, self.num_levels, self.num_points, 1)
        for i in range(self.num_points):
            grid[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias.copy_(grid.view(-1))
        torch.nn.init.zeros_(self.attention_weights.weight)
        torch.nn.init.zeros_(self.attention_weights.bias)
        for proj in (self.value_proj, self.output_proj):
            torch.nn.init.xavier_uniform_(proj.weight)
            torch.nn.init.zeros_(proj.bias)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None, reference_points=None,
                spatial_shapes=None, level_start_index=None):
        if value is None:
            value = query
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        bs, num_query, _ = query.shape
        num_value = value.shape[1]
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        value = value.view(bs, num_value, self.num_heads, -1)
        heads, levels, points = self.num_heads, self.num_levels, self.num_points
        offsets = self.sampling_offsets(query).view(bs, num_query, heads, levels, points, 2)
        weights = self.attention_weights(query).view(bs, num_query, heads, levels * points).softmax(-1)
        weights = weights.view(bs, num_query, heads, levels, points)
        if reference_points.shape[-1] == 2:
            normalizer = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)
            locations = reference_points[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
        elif reference_points.shape[-1] == 4:
            locations = (reference_points[:, :, None, :, None, :2]
                         + offsets / points * reference_points[:, :, None, :, None, 2:] * 0.5)
        else:
            raise ValueError("the last axis of reference_points must hold 2 or 4 entries, got %d" % reference_points.shape[-1])
        if value.device.type == "cuda":
            output = multi_scale_deformable_attn(value, spatial_shapes, level_start_index, locations, weights, self.im2col_step)
        else:
            output = multi_scale_deformable_attn_pytorch(value, spatial_shapes, locations, weights)
        output = self.output_proj(output)
        if not self.batch_first:
            output = output.permute(1, 0, 2)
        return self.dropout(output) + identity

    def extra_repr(self):
        return "embed_dims=%s, num_heads=%s, num_levels=%s, num_points=%s, im2col_step=%s, batch_first=%s" % (
            self.embed_dims, self.num_heads, self.num_levels, self.num_points, self.im2col_step, self.batch_first)


class DCNv3Function:
    """InternImage's DCNv3Function: .apply(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
    dilation_w, group, group_channels, offset_scale, im2col_step), upstream's fifteen positional arguments, on frcnn::dcnv3 (whose
    autograd is registered with the custom op)."""

    @staticmethod
    def apply(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
              offset_scale, im2col_step):
        pairs = _dcn_pairs(_DCN_APPLY_NAMES, (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w))
        return _dcnv3(input, offset, mask, *_dcn_args("dcnv3", input, (offset, mask), *pairs, group, group_channels, offset_scale,
                                                      im2col_step))


class _ToChannelsLast(torch.nn.Module):
    def forward(self, x):
        return x.permute(0, 2, 3, 1)


class DCNv3(torch.nn.Module):
    """InternImage's DCNv3 module on [N, H, W, C] input.  input_proj projects the input; a depthwise convolution, LayerNorm and GELU on
    the input feed the offset and mask heads (a softmax over the K points of each group); the sampler mixes the projected input;
    output_proj projects back."""

    def __init__(self, channels=64, kernel_size=3, dw_kernel_size=None, stride=1, pad=1, dilation=1, group=4, offset_scale=1.0,
                 center_feature_scale=False, remove_center=False):
        super().__init__()
        if center_feature_scale or remove_center:
            raise NotImplementedError("DCNv3: center_feature_scale and remove_center are not implemented")
        if channels % group != 0:
            raise ValueError("channels must be divisible by group, got %d and %d" % (channels, group))
        dw_kernel_size = dw_kernel_size if dw_kernel_size is not None else kernel_size
        nn = torch.nn
        self.offset_scale = offset_scale
        self.channels = channels
        self.kernel_size = kernel_size
        self.dw_kernel_size = dw_kernel_size
        self.stride = stride
        self.dilation = dilation
        self.pad = pad
        self.group = group
        self.group_channels = channels // group
        self.dw_conv = nn.Sequential(nn.Conv2d(channels, channels, dw_kernel_size, 1, (dw_kernel_size - 1) // 2, groups=channels),
                                     nn.Sequential(_ToChannelsLast(), nn.LayerNorm(channels, eps=1e-6)), nn.GELU())
        self.offset = nn.Linear(channels, group * kernel_size * kernel_size * 2)
        self.mask = nn.Linear(channels, group * kernel_size * kernel_size)
        self.input_proj = nn.Linear(channels, channels)
        self.output_proj = nn.Linear(channels, channels)
        self._reset_parameters()

    def _reset_parameters(self):
        for head in (self.offset, self.mask):
            torch.nn.init.zeros_(head.weight)
            torch.nn.init.zeros_(head.bias)
        for proj in (self.input_proj, self.output_proj):
            torch.nn.init.xavier_uniform_(proj.weight)
            torch.nn.init.zeros_(proj.bias)

    def forward(self, input):
        n, h, w, _ = input.shape
        x = self.input_proj(input)
        x1 = self.dw_conv(input.permute(0, 3, 1, 2))
        offset = self.offset(x1)
        mask = torch.softmax(self.mask(x1).reshape(n, h, w, self.group, -1), -1).reshape(n, h, w, -1)
        k, s, p, d = self.kernel_size, self.stride, self.pad, self.dilation
        if x.device.type == "cuda":
            x = DCNv3Function.apply(x, offset, mask, k, k, s, s, p, p, d, d, self.group, self.group_channels, self.offset_scale, 256)
        else:
            x = dcnv3_core_pytorch(x, offset, mask, k, k, s, s, p, p, d, d, self.group, self.group_channels, self.offset_scale)
        return self.output_proj(x)

    def extra_repr(self):
        return "channels=%s, kernel_size=%s, dw_kernel_size=%s, stride=%s, pad=%s, dilation=%s, group=%s, offset_scale=%s" % (
            self.channels, self.kernel_size, self.dw_kernel_size, self.stride, self.pad, self.dilation, self.group, self.offset_scale)


class DCNv4Function:
    """Upstream's DCNv4Function: .apply(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
    group, group_channels, offset_scale, im2col_step, remove_center), its fifteen positional arguments, on frcnn::dcnv4 (whose autograd
    is registered with the custom op)."""

    @staticmethod
    def apply(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, group_channels,
              offset_scale, im2col_step, remove_center):
        pairs = _dcn_pairs(_DCN_APPLY_NAMES, (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w))
        return _dcnv4(input, offset_mask, *_dcn_args("dcnv4", input, (offset_mask,), *pairs, group, group_channels, offset_scale,
                                                     im2col_step, remove_center))


class DCNv4(torch.nn.Module):
    """FlashInternImage's DCNv4 module on [N, L, C] input with L = H W.  value_proj projects the input; offset_mask, one linear layer on
    the input (after the depthwise convolution offset_mask_dw when dw_kernel_size is given), yields the packed offsets and masks -- no
    softmax; the sampler mixes the projected input; output_proj projects back.  without_pointwise drops both projections."""

    def __init__(self, channels=64, kernel_size=3, stride=1, pad=1, dilation=1, group=4, offset_scale=1.0, dw_kernel_size=None,
                 center_feature_scale=False, remove_center=False, output_bias=True, without_pointwise=False):
        super().__init__()
        if center_feature_scale:
            raise NotImplementedError("DCNv4: center_feature_scale is not implemented")
        if channels % group != 0:
            raise ValueError("channels must be divisible by group, got %d and %d" % (channels, group))
        if remove_center and (kernel_size % 2 == 0 or kernel_size < 3):
            raise ValueError("remove_center requires a square kernel of odd size >= 3, got %r" % ((kernel_size, kernel_size),))
        nn = torch.nn
        self.offset_scale = offset_scale
        self.channels = channels
        self.kernel_size = kernel_size
        self.dw_kernel_size = dw_kernel_size
        self.stride = stride
        self.dilation = dilation
        self.pad = pad
        self.group = group
        self.group_channels = channels // group
        self.remove_center = bool(remove_center)
        self.without_pointwise = without_pointwise
        self.K = group * _dcnv4_points(kernel_size, kernel_size, remove_center)
        if dw_kernel_size is not None:
            self.offset_mask_dw = nn.Conv2d(channels, channels, dw_kernel_size, stride=1, padding=(dw_kernel_size - 1) // 2, groups=channels)
        self.offset_mask = nn.Linear(channels, _dcnv4_record(group, self.K // group))
        if not without_pointwise:
            self.value_proj = nn.Linear(channels, channels)
            self.output_proj = nn.Linear(channels, channels, bias=output_bias)
        self._reset_parameters()

    def _reset_parameters(self):
        torch.nn.init.zeros_(self.offset_mask.weight)
        torch.nn.init.zeros_(self.offset_mask.bias)
        if not self.without_pointwise:
            for proj in (self.value_proj, self.output_proj):
                torch.nn.init.xavier_uniform_(proj.weight)
                if proj.bias is not None:
                    torch.nn.init.zeros_(proj.bias)

    def forward(self, input, shape=None):
        n, length, c = input.shape
        if shape is not None:
            h, w = shape
        else:
            h = w = math.isqrt(length)
        if h * w != length:
            raise ValueError("input's length %d is not H W: pass shape=(H, W) (got %r)" % (length, shape))
        x = input if self.without_pointwise else self.value_proj(input)
        x = x.reshape(n, h, w, c)
        if self.dw_kernel_size is not None:
            head = self.offset_mask_dw(input.reshape(n, h, w, c).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        else:
            head = input.reshape(n, h, w, c)
        offset_mask = self.offset_mask(head)
        k, s, p, d = self.kernel_size, self.stride, self.pad, self.dilation
        if x.device.type == "cuda":
            x = DCNv4Function.apply(x, offset_mask, k, k, s, s, p, p, d, d, self.group, self.group_channels, self.offset_scale, 256,
                                    self.remove_center)
        else:
            x = dcnv4_core_pytorch(x, offset_mask, k, k, s, s, p, p, d, d, self.group, self.group_channels, self.offset_scale,
                                   self.remove_center)
        x = x.reshape(n, -1, c)
        return x if self.without_pointwise else self.output_proj(x)

    def extra_repr(self):
        return ("channels=%s, kernel_size=%s, stride=%s, pad=%s, dilation=%s, group=%s, offset_scale=%s, dw_kernel_size=%s, "
                "remove_center=%s, without_pointwise=%s" % (self.channels, self.kernel_size, self.stride, self.pad, self.dilation, self.group,
                                                           self.offset_scale, self.dw_kernel_size, self.remove_center,
                                                           self.without_pointwise))


# ---- point-set operators: convex_iou, convex_giou, min_area_polygons (csrc/ops_convex.hip) --------------------------------------------
@torch.library.custom_op("frcnn::convex_iou", mutates_args=())
def _convex_iou(pointsets: Tensor, polygons: Tensor) -> Tensor:
    n, k = pointsets.shape[0], polygons.shape[0]
    out = pointsets.new_empty((n, k))
    if n == 0 or k == 0:
        return out
    with torch.cuda.device(pointsets.device):
        a, b = pointsets.contiguous(), polygons.contiguous()
        nv.check(nv.lib().frcnn_ops_convex_iou(a.data_ptr(), n, b.data_ptr(), k, out.data_ptr(), _stream(pointsets)),
                 "frcnn_ops_convex_iou")
    return out


@_convex_iou.register_fake
def _(pointsets, polygons):
    return pointsets.new_empty((pointsets.shape[0], polygons.shape[0]))


@torch.library.custom_op("frcnn::convex_giou", mutates_args=())
def _convex_giou(pointsets: Tensor, polygons: Tensor) -> Tuple[Tensor, Tensor]:
    """(giou [n], its derivative in the point sets [n, 18]) of the aligned pairs, from one launch."""
    n = pointsets.shape[0]
    giou, grad = pointsets.new_empty((n,)), pointsets.new_empty((n, 18))
    if n == 0:
        return giou, grad
    with torch.cuda.device(pointsets.device):
        a, b = pointsets.contiguous(), polygons.contiguous()
        nv.check(nv.lib().frcnn_ops_convex_giou(a.data_ptr(), b.data_ptr(), n, giou.data_ptr(), grad.data_ptr(), _stream(pointsets)),
                 "frcnn_ops_convex_giou")
    return giou, grad


@_convex_giou.register_fake
def _(pointsets, polygons):
    n = pointsets.shape[0]
    return pointsets.new_empty((n,)), pointsets.new_empty((n, 18))


def _convex_giou_bwd(ctx, grad_giou, grad_grad):
    (grad,) = ctx.saved_tensors
    return (grad_giou[:, None] * grad if ctx.needs_input_grad[0] else None), None


torch.library.register_autograd("frcnn::convex_giou", _convex_giou_bwd,
                                setup_context=lambda ctx, inputs, output: ctx.save_for_backward(output[1].detach()))


@torch.library.custom_op("frcnn::min_area_polygons", mutates_args=())
def _min_area_polygons(pointsets: Tensor) -> Tensor:
    n = pointsets.shape[0]
    out = pointsets.new_empty((n, 8))
    if n == 0:
        return out
    with torch.cuda.device(pointsets.device):
        a = pointsets.contiguous()
        nv.check(nv.lib().frcnn_ops_min_area_polygons(a.data_ptr(), n, out.data_ptr(), _stream(pointsets)), "frcnn_ops_min_area_polygons")
    return out


@_min_area_polygons.register_fake
def _(pointsets):
    return pointsets.new_empty((pointsets.shape[0], 8))


def _convex_input(name, t, width, row, fallback):
    _check_tensor(name, t, (torch.float32,), "float32 (the point-set operators are float32 only: pass .float())", fallback)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError("%s must be [N, %d] %s, got shape %s" % (name, width, row, tuple(t.shape)))
    if t.shape[0] > MAX_CONVEX_ROWS:
        raise ValueError("%s holds at most MAX_CONVEX_ROWS = %d rows, got %d" % (name, MAX_CONVEX_ROWS, t.shape[0]))


_CONVEX_SET_ROW, _CONVEX_POLY_ROW = "(x1, y1, ..., x9, y9)", "(x1, y1, ..., x4, y4)"


def convex_iou(pointsets, polygons):
    """mmcv.ops.convex_iou: the IoU of the convex hull of every point set [N, 18] with every polygon [K, 8] -> [N, K] (the module
    docstring states the contract).  Not differentiable."""
    _convex_input("pointsets", pointsets, 18, _CONVEX_SET_ROW, "convex_iou_pytorch")
    _convex_input("polygons", polygons, 8, _CONVEX_POLY_ROW, "convex_iou_pytorch")
    _check_same_device(pointsets, polygons, "pointsets", "polygons")
    if polygons.shape[0] > MAX_CONVEX_POLYGONS:
        raise ValueError("polygons holds at most MAX_CONVEX_POLYGONS = %d rows, got %d" % (MAX_CONVEX_POLYGONS, polygons.shape[0]))
    return _convex_iou(pointsets.detach(), polygons.detach())


def convex_giou(pointsets, polygons):
    """mmcv.ops.convex_giou: (giou [N], grad [N, 18]) of the aligned pairs of point sets [N, 18] and polygons [N, 8]: the generalised
    IoU of the sets' hulls and its closed-form derivative in the sets' coordinates, from one launch.  giou also carries that
    derivative through autograd (backward: grad_out[:, None] * grad); grad itself is not differentiable."""
    _convex_input("pointsets", pointsets, 18, _CONVEX_SET_ROW, "convex_giou_pytorch")
    _convex_input("polygons", polygons, 8, _CONVEX_POLY_ROW, "convex_giou_pytorch")
    if pointsets.shape[0] != polygons.shape[0]:
        raise ValueError("pointsets and polygons must hold one polygon per point set, got %d and %d rows"
                         % (pointsets.shape[0], polygons.shape[0]))
    _check_same_device(pointsets, polygons, "pointsets", "polygons")
    giou, grad = _convex_giou(pointsets, polygons.detach())
    return giou, grad.detach()


def min_area_polygons(pointsets):
    """mmcv.ops.min_area_polygons: the rectangle of the smallest area around each point set [N, 18] -> [N, 8], four corners
    counter-clockwise, one side on a hull edge (the module docstring states the contract).  Not differentiable."""
    _convex_input("pointsets", pointsets, 18, _CONVEX_SET_ROW, "min_area_polygons_pytorch")
    return _min_area_polygons(pointsets.detach())


def _convex_pytorch_input(name, t, width, row):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s must be float32 or float64, got %s" % (name, t.dtype))
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError("%s must be [N, %d] %s, got shape %s" % (name, width, row, tuple(t.shape)))


def _cross2(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _convex_hull_list(pts):
    """pts [B, n, 2] in general position -> the hull's vertices [B, n, 2], counter-clockwise from the smallest (x, y), the start repeated
    after the last one (a zero-length edge adds nothing to any sum below).  i -> j is a hull edge iff every other point lies strictly on
    its left; the decisions carry no gradient, the gathered vertices do."""
    n = pts.shape[1]
    with torch.no_grad():
        d = pts[:, None, :, :] - pts[:, :, None, :]                                  # d[b, i, j] = p_j - p_i
        left = d[:, :, :, None, 0] * d[:, :, None, :, 1] - d[:, :, :, None, 1] * d[:, :, None, :, 0] > 0     # [b, i, j, k]
        eye = torch.eye(n, dtype=torch.bool, device=pts.device)
        edge = (left | eye[:, None, :] | eye[None, :, :]).all(-1) & ~eye              # k == i or k == j does not vote
        vertex = edge.any(-1)
        nxt = edge.to(torch.uint8).argmax(-1)
        inf = torch.full_like(pts[..., 0], float("inf"))
        xs = torch.where(vertex, pts[..., 0], inf)
        first = vertex & (xs == xs.min(-1, keepdim=True).values)
        start = torch.where(first, pts[..., 1], inf).argmin(-1, keepdim=True)
        cur, done, order = start, torch.zeros_like(start, dtype=torch.bool), [start]
        for _ in range(n - 1):
            step = nxt.gather(1, cur)
            done = done | (step == start)
            cur = torch.where(done, start, step)
            order.append(cur)
        order = torch.cat(order, 1)
    return pts.gather(1, order[..., None].expand(-1, -1, 2))


def _convex_list_area(v):
    """The shoelace area of vertex lists [..., n, 2]: the fan from the first vertex."""
    r = v[..., 1:, :] - v[..., :1, :]
    return 0.5 * _cross2(r[..., :-1, :], r[..., 1:, :]).sum(-1)


def _convex_boundary_inside(a, w):
    """Half the sum of cross(start, end) over the pieces of polygon a's edges ([..., m, 2]) that lie inside the convex polygon w
    ([..., k, 2], counter-clockwise): Cyrus-Beck per edge, every division on a safe denominator."""
    b = torch.roll(a, -1, -2)
    wa = w[..., None, :, :]
    e = torch.roll(w, -1, -2)[..., None, :, :] - wa                                    # [..., 1, k, 2]
    da = _cross2(e, a[..., :, None, :] - wa)                                          # [..., m, k]
    db = _cross2(e, b[..., :, None, :] - wa)
    enter, leave = (da < 0) & (db >= 0), (da >= 0) & (db < 0)
    t = da / torch.where(enter | leave, da - db, torch.ones_like(da))
    t0 = torch.where(enter, t, torch.zeros_like(t)).max(-1).values
    t1 = torch.where(leave, t, torch.ones_like(t)).min(-1).values
    inside = ~((da < 0) & (db < 0)).any(-1) & (t1 > t0)
    d = b - a
    piece = _cross2(a + t0[..., None] * d, a + t1[..., None] * d)
    return 0.5 * torch.where(inside, piece, torch.zeros_like(piece)).sum(-1)


def _convex_inter(p, q):
    """area(P n Q) of hull lists p [..., 9, 2] and q [..., 4, 2] on one origin: the boundary of the intersection is P's edges inside Q
    and Q's edges inside P."""
    return (_convex_boundary_inside(p, q) + _convex_boundary_inside(q, p)).clamp_min(0)


def _convex_finite(t):
    return torch.isfinite(t).all(-1)


def convex_iou_pytorch(pointsets, polygons):
    """convex_iou from torch operations, on any device, float32 or float64 -> [N, K].  The hull edges come from the all-pairs left-of
    test and I from the boundary sum over the clipped edge pieces, so it serves point sets in GENERAL POSITION only: no duplicate
    points, no three collinear hull points, no edge of P on an edge of Q.  Not fast: rows go through in chunks."""
    _convex_pytorch_input("pointsets", pointsets, 18, _CONVEX_SET_ROW)
    _convex_pytorch_input("polygons", polygons, 8, _CONVEX_POLY_ROW)
    n, k = pointsets.shape[0], polygons.shape[0]
    out = pointsets.new_zeros((n, k))
    if n == 0 or k == 0:
        return out
    with torch.no_grad():
        polygons = polygons.to(pointsets.dtype)
        okq = _convex_finite(polygons)
        q = _convex_hull_list(torch.where(okq[:, None], polygons, torch.zeros_like(polygons)).view(k, 4, 2))
        origin = q[:, 0]
        q = q - origin[:, None]
        aq = _convex_list_area(q)
        okq = okq & (aq >= CONVEX_MIN_AREA)
        for i0 in range(0, n, 1024):
            rows = pointsets[i0:i0 + 1024]
            okp = _convex_finite(rows)
            p = _convex_hull_list(torch.where(okp[:, None], rows, torch.zeros_like(rows)).view(-1, 9, 2))
            ap = _convex_list_area(p - p[:, :1])
            inter = _convex_inter(p[:, None] - origin[None, :, None], q[None])
            union = ap[:, None] + aq[None] - inter
            ok = okp[:, None] & okq[None] & (union >= CONVEX_MIN_AREA)
            out[i0:i0 + 1024] = torch.where(ok, inter / torch.where(ok, union, torch.ones_like(union)), torch.zeros_like(union))
    return out


def _convex_giou_value(pointsets, polygons):
    n = pointsets.shape[0]
    ok = _convex_finite(pointsets) & _convex_finite(polygons)
    sets = torch.where(ok[:, None], pointsets, torch.zeros_like(pointsets)).view(n, 9, 2)
    quads = torch.where(ok[:, None], polygons, torch.zeros_like(polygons)).view(n, 4, 2)
    q = _convex_hull_list(quads)
    origin = q[:, :1]
    q = q - origin
    p = _convex_hull_list(sets)
    ap, aq = _convex_list_area(p - p[:, :1]), _convex_list_area(q)
    p = p - origin
    inter = _convex_inter(p, q)
    union = ap + aq - inter
    hull = _convex_list_area(_convex_hull_list(torch.cat([sets, quads], 1) - origin))
    ok = ok & (aq >= CONVEX_MIN_AREA) & (union >= CONVEX_MIN_AREA) & (hull >= CONVEX_MIN_AREA)
    one = torch.ones_like(union)
    union, hull = torch.where(ok, union, one), torch.where(ok, hull, one)
    return torch.where(ok, inter / union + union / hull - 1, torch.zeros_like(union))


class _ConvexGiouPytorch(torch.autograd.Function):
    """Hands giou out with the gradient that autograd already formed: backward is grad_out[:, None] * grad."""

    @staticmethod
    def forward(ctx, pointsets, giou, grad):
        ctx.save_for_backward(grad)
        return giou.clone()

    @staticmethod
    def backward(ctx, grad_out):
        return grad_out[:, None] * ctx.saved_tensors[0], None, None


def convex_giou_pytorch(pointsets, polygons):
    """convex_giou from torch operations, on any device, float32 or float64 -> (giou [N], grad [N, 18]); grad comes from autograd
    through the composition, and giou carries it as convex_giou's does.  For point sets in GENERAL POSITION only: no duplicate points, no
    three collinear hull points (of P, or of the thirteen points), no edge of P on an edge of Q."""
    _convex_pytorch_input("pointsets", pointsets, 18, _CONVEX_SET_ROW)
    _convex_pytorch_input("polygons", polygons, 8, _CONVEX_POLY_ROW)
    if pointsets.shape[0] != polygons.shape[0]:
        raise ValueError("pointsets and polygons must hold one polygon per point set, got %d and %d rows"
                         % (pointsets.shape[0], polygons.shape[0]))
    if pointsets.shape[0] == 0:
        return pointsets.new_zeros((0,)) + 0 * pointsets.sum(), pointsets.new_zeros((0, 18))
    with torch.enable_grad():
        leaf = pointsets.detach().requires_grad_(True)
        value = _convex_giou_value(leaf, polygons.detach().to(pointsets.dtype))
        (grad,) = torch.autograd.grad(value.sum(), leaf)
    return _ConvexGiouPytorch.apply(pointsets, value.detach(), grad), grad


def min_area_polygons_pytorch(pointsets):
    """min_area_polygons from torch operations, on any device, float32 or float64 -> [N, 8].  For point sets in GENERAL POSITION only: no
    duplicate points, no three collinear hull points; of edges whose rectangles tie (areas within a relative 2^-18 of the smallest) the
    first one wins."""
    _convex_pytorch_input("pointsets", pointsets, 18, _CONVEX_SET_ROW)
    n = pointsets.shape[0]
    if n == 0:
        return pointsets.new_zeros((0, 8))
    with torch.no_grad():
        ok = _convex_finite(pointsets)
        hull = _convex_hull_list(torch.where(ok[:, None], pointsets, torch.zeros_like(pointsets)).view(n, 9, 2))
        origin = hull[:, :1]
        v = hull - origin
        e = torch.roll(v, -1, 1) - v                                                  # [n, 9, 2]; zero for the repeated start
        length = e.norm(dim=-1)
        real = length > 0
        u = e / torch.where(real, length, torch.ones_like(length))[..., None]
        d = v[:, None, :, :] - v[:, :, None, :]                                      # d[b, k, w] = v_w - v_k
        pu = (d * u[:, :, None, :]).sum(-1)
        pv = d[..., 1] * u[:, :, None, 0] - d[..., 0] * u[:, :, None, 1]
        u0, u1, v1 = pu.min(-1).values, pu.max(-1).values, pv.max(-1).values
        area = torch.where(real, (u1 - u0) * v1, torch.full_like(length, float("inf")))
        tied = area * CONVEX_RECT_TIE <= area.min(-1, keepdim=True).values
        best = tied.to(torch.uint8).argmax(-1, keepdim=True)                          # the first of the tied
        pick = lambda t: t.gather(1, best)[:, 0]                                       # noqa: E731
        a = v.gather(1, best[..., None].expand(-1, -1, 2))[:, 0]
        ub = u.gather(1, best[..., None].expand(-1, -1, 2))[:, 0]
        u0, u1, v1 = pick(u0)[:, None], pick(u1)[:, None], pick(v1)[:, None]
        left = torch.stack([-ub[:, 1], ub[:, 0]], 1)
        c0, c1 = a + u0 * ub, a + u1 * ub
        out = torch.stack([c0, c1, c1 + v1 * left, c0 + v1 * left], 1) + origin
        return torch.where(ok[:, None], out.reshape(n, 8), torch.zeros_like(pointsets[:, :8]))


# ---- quadrilateral operators: box_iou_quadri, nms_quadri, points_in_polygons (csrc/ops_quadri.hip) ------------------------------------
@torch.library.custom_op("frcnn::box_iou_quadri", mutates_args=())
def _box_iou_quadri(bboxes1: Tensor, bboxes2: Tensor, mode: int, aligned: bool) -> Tensor:
    n, m = bboxes1.shape[0], bboxes2.shape[0]
    out = torch.empty((n,) if aligned else (n, m), dtype=torch.float32, device=bboxes1.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(bboxes1.device):
        a, b = bboxes1.contiguous(), bboxes2.contiguous()
        nv.check(nv.lib().frcnn_ops_box_iou_quadri(a.data_ptr(), n, b.data_ptr(), m, mode, int(aligned), out.data_ptr(), _stream(bboxes1)),
                 "frcnn_ops_box_iou_quadri")
    return out


@_box_iou_quadri.register_fake
def _(bboxes1, bboxes2, mode, aligned):
    n, m = bboxes1.shape[0], bboxes2.shape[0]
    return bboxes1.new_empty((n,) if aligned else (n, m), dtype=torch.float32)


@torch.library.custom_op("frcnn::nms_quadri", mutates_args=())
def _nms_quadri_op(dets: Tensor, scores: Tensor, labels: Optional[Tensor], iou_threshold: float) -> Tensor:
    """The kept indices."""
    return _nms(dets, scores, labels, iou_threshold, quadri=True)


@_nms_quadri_op.register_fake
def _(dets, scores, labels, iou_threshold):
    return _nms_fake_result(dets)


@torch.library.custom_op("frcnn::points_in_polygons", mutates_args=())
def _points_in_polygons(points: Tensor, polygons: Tensor) -> Tensor:
    n, m = points.shape[0], polygons.shape[0]
    out = points.new_empty((n, m))
    if n == 0 or m == 0:
        return out
    with torch.cuda.device(points.device):
        a, b = points.contiguous(), polygons.contiguous()
        nv.check(nv.lib().frcnn_ops_points_in_polygons(a.data_ptr(), n, b.data_ptr(), m, out.data_ptr(), _stream(points)),
                 "frcnn_ops_points_in_polygons")
    return out


@_points_in_polygons.register_fake
def _(points, polygons):
    return points.new_empty((points.shape[0], polygons.shape[0]))


_QUADRI_ROW, _POINT_ROW = "(x1, y1, ..., x4, y4)", "(x, y)"


def _quadri_input(name, t, width, row, fallback=None):
    _check_tensor(name, t, (torch.float32,), "float32 (the quadrilateral operators are float32 only: pass .float())", fallback)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError("%s must be [N, %d] %s, got shape %s" % (name, width, row, tuple(t.shape)))
    if t.shape[0] > MAX_QUADRI_ROWS:
        raise ValueError("%s holds at most MAX_QUADRI_ROWS = %d rows, got %d" % (name, MAX_QUADRI_ROWS, t.shape[0]))


def _quadri_mode(mode, bboxes1, bboxes2, aligned):
    if mode not in ("iou", "iof"):
        raise ValueError("mode must be 'iou' or 'iof', got %r" % (mode,))
    if aligned and bboxes1.shape[0] != bboxes2.shape[0]:
        raise ValueError("aligned=True needs bboxes1 and bboxes2 of one length, got %d and %d" % (bboxes1.shape[0], bboxes2.shape[0]))


def box_iou_quadri(bboxes1, bboxes2, mode="iou", aligned=False):
    """mmcv.ops.box_iou_quadri: the IoU (or, mode="iof", the intersection over the first one's area) of quadrilaterals [N, 8] and [M, 8]
    (x1, y1, ..., x4, y4): float32 [N, M], or [N] when aligned.  A row stands for the convex hull of its four vertices, in any order
    (the module docstring states the contract).  No autograd."""
    _quadri_input("bboxes1", bboxes1, 8, _QUADRI_ROW, "box_iou_quadri_pytorch")
    _quadri_input("bboxes2", bboxes2, 8, _QUADRI_ROW, "box_iou_quadri_pytorch")
    _quadri_mode(mode, bboxes1, bboxes2, aligned)
    _check_same_device(bboxes1, bboxes2, "bboxes1", "bboxes2")
    if not aligned and bboxes2.shape[0] > MAX_QUADRI_COLUMNS:
        raise ValueError("bboxes2 holds at most MAX_QUADRI_COLUMNS = %d rows, got %d" % (MAX_QUADRI_COLUMNS, bboxes2.shape[0]))
    return _box_iou_quadri(bboxes1.detach(), bboxes2.detach(), int(mode == "iof"), bool(aligned))


def nms_quadri(dets, scores, iou_threshold, labels=None):
    """mmcv.ops.nms_quadri: greedy NMS on box_iou_quadri, within each label when labels are given.  dets [N, 8] quadrilaterals, scores
    [N].  Returns (dets [K, 9] = cat(dets[keep], scores[keep, None]), keep int64 [K]), by descending score, ties by ascending index,
    NaN scores last (nms_rotated's rules)."""
    _quadri_input("dets", dets, 8, _QUADRI_ROW)
    _nms_scores_labels("nms_quadri", "dets", dets, scores, labels)
    keep = _nms_quadri_op(dets.detach(), scores.detach(), labels, float(iou_threshold))
    return torch.cat([dets[keep], scores[keep, None]], dim=1), keep


def points_in_polygons(points, polygons):
    """mmcv.ops.points_in_polygons: float32 [N, M], 1.0 where point i of points [N, 2] lies in the closed convex hull of polygon j of
    polygons [M, 8] (x1, y1, ..., x4, y4; vertices in any order), else 0.0 (the module docstring states the contract).  No autograd."""
    _quadri_input("points", points, 2, _POINT_ROW, "points_in_polygons_pytorch")
    _quadri_input("polygons", polygons, 8, _QUADRI_ROW, "points_in_polygons_pytorch")
    _check_same_device(points, polygons, "points", "polygons")
    if polygons.shape[0] > MAX_QUADRI_COLUMNS:
        raise ValueError("polygons holds at most MAX_QUADRI_COLUMNS = %d rows, got %d" % (MAX_QUADRI_COLUMNS, polygons.shape[0]))
    return _points_in_polygons(points.detach(), polygons.detach())


def _quadri_hulls(quads):
    """quads [n, 8] -> (the hull lists [n, 4, 2] of _convex_hull_list, their areas on coordinates relative to the smallest vertex, the
    mask of the live rows)."""
    ok = _convex_finite(quads)
    hull = _convex_hull_list(torch.where(ok[:, None], quads, torch.zeros_like(quads)).view(-1, 4, 2))
    area = _convex_list_area(hull - hull[:, :1])
    return hull, area, ok & (area >= CONVEX_MIN_AREA)


def box_iou_quadri_pytorch(bboxes1, bboxes2, mode="iou", aligned=False):
    """box_iou_quadri from torch operations, on any device, float32 or float64 -> [N, M], or [N] when aligned: convex_iou_pytorch's
    hull list and boundary sum, so it serves quadrilaterals in GENERAL POSITION only: no duplicate vertices, no three collinear
    vertices, no edge of one on an edge of the other.  Not fast: rows go through in chunks."""
    _convex_pytorch_input("bboxes1", bboxes1, 8, _QUADRI_ROW)
    _convex_pytorch_input("bboxes2", bboxes2, 8, _QUADRI_ROW)
    _quadri_mode(mode, bboxes1, bboxes2, aligned)
    n, m = bboxes1.shape[0], bboxes2.shape[0]
    out = bboxes1.new_zeros((n,) if aligned else (n, m))
    if out.numel() == 0:
        return out
    with torch.no_grad():
        q, aq, okq = _quadri_hulls(bboxes2.detach().to(bboxes1.dtype))
        origin = q[:, :1]
        q = q - origin
        for i0 in range(0, n, 1024):
            p, ap, okp = _quadri_hulls(bboxes1[i0:i0 + 1024].detach())
            if aligned:
                chunk = slice(i0, i0 + 1024)
                inter, a1, a2, ok = _convex_inter(p - origin[chunk], q[chunk]), ap, aq[chunk], okp & okq[chunk]
            else:
                inter, a1, a2, ok = _convex_inter(p[:, None] - origin[None], q[None]), ap[:, None], aq[None], okp[:, None] & okq[None]
            den = a1.expand_as(inter) if mode == "iof" else a1 + a2 - inter
            ok = ok & (den >= CONVEX_MIN_AREA)
            out[i0:i0 + 1024] = torch.where(ok, inter / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
    return out


def points_in_polygons_pytorch(points, polygons):
    """points_in_polygons from torch operations, on any device, float32 or float64 -> [N, M]: the hull list of convex_iou_pytorch and
    the closed left-of test of every hull edge, so it serves polygons in GENERAL POSITION only: no duplicate vertices, no three
    collinear vertices."""
    _convex_pytorch_input("points", points, 2, _POINT_ROW)
    _convex_pytorch_input("polygons", polygons, 8, _QUADRI_ROW)
    n, m = points.shape[0], polygons.shape[0]
    out = points.new_zeros((n, m))
    if n == 0 or m == 0:
        return out
    with torch.no_grad():
        q, _, okq = _quadri_hulls(polygons.detach().to(points.dtype))
        origin = q[:, 0]
        a = q - origin[:, None]                                                        # [m, 4, 2]; the repeated start: an edge of length zero
        e = torch.roll(a, -1, 1) - a
        for i0 in range(0, n, 4096):
            pts = points[i0:i0 + 4096].detach()
            okp = _convex_finite(pts)
            d = torch.where(okp[:, None], pts, torch.zeros_like(pts))[:, None, None, :] - origin[None, :, None, :] - a[None]     # [n, m, 4, 2]
            inside = (e[None, ..., 0] * d[..., 1] >= e[None, ..., 1] * d[..., 0]).all(-1)
            out[i0:i0 + 4096] = (inside & okp[:, None] & okq[None]).to(out.dtype)
    return out


# ---- masked_conv2d / MaskedConv2d: the sparse convolution of Guided Anchoring's heads (csrc/ops_mconv.hip) ----------------------------
@torch.library.custom_op("frcnn::masked_conv2d", mutates_args=())
def _masked_conv2d(input: Tensor, mask: Tensor, weight: Tensor, bias: Optional[Tensor], pad_h: int, pad_w: int) -> Tensor:
    """mask: uint8 [N, oh, ow], active where not 0.  No autograd formula is registered: a backward through the op raises."""
    n, c, h, w = input.shape
    co, _, kh, kw = weight.shape
    oh, ow = h + 2 * pad_h - kh + 1, w + 2 * pad_w - kw + 1
    channels_last = _input_is_channels_last(input)
    out = _grad_empty((n, co, oh, ow), input, channels_last)
    if out.numel() == 0:
        return out
    with torch.cuda.device(input.device):
        x = input if channels_last else input.contiguous()        # both formats are read in place through their strides
        wt, m = weight.contiguous(), mask.contiguous()
        b = None if bias is None else bias.contiguous()
        ws = _workspace("masked_conv2d", input, n, oh, ow)
        e = _elem(input.dtype)
        nv.check(nv.lib().frcnn_ops_masked_conv2d(nv.OPS_F32 if e is None else e, x.data_ptr(), (C.c_int64 * 4)(*x.stride()), n, c, h, w,
                                                  wt.data_ptr(), None if b is None else b.data_ptr(), co, kh, kw, pad_h, pad_w,
                                                  m.data_ptr(), out.data_ptr(), (C.c_int64 * 4)(*out.stride()), ws.data_ptr(), ws.numel(),
                                                  _stream(input)), "frcnn_ops_masked_conv2d")
    return out


@_masked_conv2d.register_fake
def _(input, mask, weight, bias, pad_h, pad_w):
    n, _, h, w = input.shape
    co, _, kh, kw = weight.shape
    return _grad_empty((n, co, h + 2 * pad_h - kh + 1, w + 2 * pad_w - kw + 1), input, _input_is_channels_last(input))


_MCONV_WHAT = ("float32, float16 or bfloat16, the same for features, weight and bias (masked_conv2d takes no mix: cast the other tensors "
               "to the features' dtype)")


def _masked_conv2d_input(features, mask, weight, bias, padding, stride, dtypes, what, device_check):
    """The checks masked_conv2d and masked_conv2d_pytorch share; returns (pad_h, pad_w, oh, ow)."""
    tensors = [("features", features), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    allowed = (features.dtype,) if features.dtype in dtypes else dtypes[:1]      # a mix is refused at its first tensor of another dtype
    for name, t in tensors:
        if t.dtype not in allowed or t.dtype not in dtypes:
            raise TypeError("%s must be %s, got %s%s" % (name, what, t.dtype, "" if name == "features" else " beside features of %s" % features.dtype))
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor, got %s" % type(mask).__name__)
    if mask.dtype.is_complex:
        raise TypeError("mask must have a real dtype or bool, got %s" % mask.dtype)
    if device_check:
        for name, t in tensors + [("mask", mask)]:
            _check_tensor(name, t, (t.dtype,), "", "masked_conv2d_pytorch")
    for name, t in tensors[1:] + [("mask", mask)]:
        _check_same_device(features, t, "features", name)
    pad = _int_pair("padding", padding, 0)
    if _int_pair("stride", stride, 1) != (1, 1):
        raise ValueError("masked_conv2d supports stride 1 only (mmcv's rule), got %r" % (stride,))
    if features.dim() != 4:
        raise ValueError("features must be [N, C_in, H, W], got shape %s" % (tuple(features.shape),))
    if weight.dim() != 4:
        raise ValueError("weight must be [C_out, C_in, kh, kw], got shape %s" % (tuple(weight.shape),))
    n, c, h, w = features.shape
    co, cw, kh, kw = weight.shape
    if min(c, h, w, co, kh, kw) < 1:
        raise ValueError("features and weight must not be empty beyond N, got features %s, weight %s" % (tuple(features.shape), tuple(weight.shape)))
    if cw != c:
        raise ValueError("weight must be [C_out, C_in, kh, kw] with C_in = %d (no groups), got shape %s" % (c, tuple(weight.shape)))
    if bias is not None and tuple(bias.shape) != (co,):
        raise ValueError("bias must be [C_out] = [%d], got shape %s" % (co, tuple(bias.shape)))
    oh, ow = h + 2 * pad[0] - kh + 1, w + 2 * pad[1] - kw + 1
    if oh < 1 or ow < 1:
        raise ValueError("the output would be empty: (%d, %d) for features %s, kernel (%d, %d), padding %s" % (oh, ow, tuple(features.shape), kh, kw, pad))
    if tuple(mask.shape) != (n, oh, ow):
        raise ValueError("mask must lie on the output grid [N, oh, ow] = [%d, %d, %d], got shape %s" % (n, oh, ow, tuple(mask.shape)))
    return pad[0], pad[1], oh, ow


def masked_conv2d(features, mask, weight, bias, padding=0, stride=1):
    """mmcv.ops.masked_conv2d: the stride-1 convolution of features [N, C_in, H, W] with weight [C_out, C_in, kh, kw] and bias [C_out] (or
    None) at the pixels where mask [N, oh, ow] > 0, +0.0 (no bias) everywhere else -> [N, C_out, oh, ow] in the features' dtype and
    memory format.  Inference only: a backward through it raises."""
    ph, pw, oh, ow = _masked_conv2d_input(features, mask, weight, bias, padding, stride, _MAP_DTYPES, _MCONV_WHAT, True)
    n, c, h, w = features.shape
    co, _, kh, kw = weight.shape
    largest = max(n * oh * ow, co * c * kh * kw, n * c * h * w, n * co * oh * ow, h + ph + kh, w + pw + kw)
    if largest > MAX_MASKED_CONV_INDEX:
        raise ValueError("masked_conv2d is too large for the kernels' 32-bit indices: %d > MAX_MASKED_CONV_INDEX = %d (output pixels, "
                         "weights or a tensor's elements)" % (largest, MAX_MASKED_CONV_INDEX))
    return _masked_conv2d(features, (mask > 0).view(torch.uint8), weight, bias, ph, pw)


def masked_conv2d_pytorch(features, mask, weight, bias, padding=0, stride=1):
    """masked_conv2d from torch operations, on any device, float64 too: mmcv's composition, one image at a time -- nonzero (a host
    synchronisation on a GPU), the active pixels' taps gathered from the zero-padded map into a column matrix, addmm, scatter.  16-bit
    tensors multiply in float32 and round once."""
    dtypes = _MAP_DTYPES + (torch.float64,)
    ph, pw, oh, ow = _masked_conv2d_input(features, mask, weight, bias, padding, stride, dtypes, _MCONV_WHAT[:-1] + "; float64 too)", False)
    n, c = features.shape[:2]
    co, _, kh, kw = weight.shape
    math_dtype = torch.float32 if features.dtype in _HALF else features.dtype
    out = _grad_empty((n, co, oh, ow), features, _input_is_channels_last(features)).zero_()
    with torch.no_grad():
        wt = weight.detach().to(math_dtype).reshape(co, c * kh * kw)
        b = wt.new_zeros((co,)) if bias is None else bias.detach().to(math_dtype)
        padded = torch.nn.functional.pad(features.detach().to(math_dtype), (pw, pw, ph, ph))
        for i in range(n):
            y, x = torch.nonzero(mask[i] > 0, as_tuple=True)
            if y.numel() == 0:
                continue
            cols = torch.stack([padded[i][:, y + di, x + dj] for di in range(kh) for dj in range(kw)], dim=1)       # [C_in, kh kw, active]
            out[i][:, y, x] = torch.addmm(b[:, None], wt, cols.reshape(c * kh * kw, -1)).to(out.dtype)
    return out


class MaskedConv2d(torch.nn.Conv2d):
    """mmcv.ops.MaskedConv2d: an nn.Conv2d (same constructor, same parameters weight and bias, so a Conv2d or mmdet state dict loads
    strict) whose forward takes an optional mask.  Without one it is nn.Conv2d.forward and trains as usual; with one it is
    masked_conv2d(input, mask, weight, bias, padding), inference only.  A mask with a dilation or groups other than 1 is a ValueError
    (mmcv silently ignores the dilation), as is a stride other than 1."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)

    def forward(self, input, mask=None):
        if mask is None:
            return super().forward(input)
        if tuple(self.dilation) != (1, 1) or self.groups != 1:
            raise ValueError("MaskedConv2d with a mask supports dilation 1 and groups 1 only, got dilation %s, groups %d"
                             % (tuple(self.dilation), self.groups))
        return masked_conv2d(input, mask, self.weight, self.bias, self.padding, self.stride)


# ---- paste_masks_in_image / paste_masks_aligned / masks_to_boxes: a Mask R-CNN's last step (csrc/ops_mask.hip) ------------------------
# One run on an MI355X (tools/ops_bench.py --only mask; K = 100, M = 28, 800 x 1333, boxes of 30 to 400 px a side): microseconds of the
# operator, of its _pytorch twin and of upstream's composition (torchvision's loop restated; grid_sample in one chunk and the threshold),
# and the operator's rate over the bytes it writes (masks_to_boxes: reads).  No form is slower than its twin.  The float32 paste runs
# at 0.65 of the 8 TB/s HBM peak.  The byte forms do not reach the store's rate: with 16 pixels a lane they took 116 / 123 us (the few
# lanes of a wave that a box covers evaluated 16 pixels each), so a lane stores 4 pixels there; the evaluation inside the boxes remains.
MASK_BENCH = {
    "paste_masks_in_image float32, padding 1": {"ops": 81.8, "twin": 3091.9, "upstream": 7871.0, "TB/s": 5.22},
    "paste_masks_in_image float16, padding 1": {"ops": 58.1, "twin": 3203.2, "upstream": 7887.7, "TB/s": 3.67},
    "paste_masks_aligned bool, threshold 0.5": {"ops": 67.7, "twin": 3038.8, "upstream": 1869.4, "TB/s": 1.58},
    "paste_masks_aligned uint8": {"ops": 60.1, "twin": 3890.7, "upstream": 2148.8, "TB/s": 1.78},
    "masks_to_boxes bool": {"ops": 27.8, "twin": 411.3, "TB/s": 3.84},
    "masks_to_boxes float32": {"ops": 73.5, "twin": 343.0, "TB/s": 5.81},
}


def _mask_elem(dtype):
    e = _elem(dtype)
    return nv.OPS_F32 if e is None else e


@torch.library.custom_op("frcnn::paste_masks_in_image", mutates_args=())
def _paste_masks_in_image(masks: Tensor, boxes: Tensor, h: int, w: int, padding: int) -> Tensor:
    k, m = masks.shape[0], masks.shape[2]
    out = torch.empty((k, 1, h, w), dtype=masks.dtype, device=masks.device)
    if k == 0:
        return out
    with torch.cuda.device(masks.device):
        mk, bx = masks.contiguous(), boxes.contiguous()
        nv.check(nv.lib().frcnn_ops_paste_masks_in_image(_mask_elem(masks.dtype), mk.data_ptr(), bx.data_ptr(), k, m, padding, h, w,
                                                         out.data_ptr(), _stream(masks)), "frcnn_ops_paste_masks_in_image")
    return out


@_paste_masks_in_image.register_fake
def _(masks, boxes, h, w, padding):
    return torch.empty((masks.shape[0], 1, h, w), dtype=masks.dtype, device=masks.device)


@torch.library.custom_op("frcnn::paste_masks_aligned", mutates_args=())
def _paste_masks_aligned(masks: Tensor, boxes: Tensor, h: int, w: int, threshold: float, as_uint8: bool) -> Tensor:
    """masks [K, Mh, Mw]; bytes [K, H, W] as torch.uint8 (the public function views the comparison's bytes as bool)."""
    k, mh, mw = masks.shape
    out = torch.empty((k, h, w), dtype=torch.uint8, device=masks.device)
    if k == 0:
        return out
    with torch.cuda.device(masks.device):
        mk, bx = masks.contiguous(), boxes.contiguous()
        nv.check(nv.lib().frcnn_ops_paste_masks_aligned(_mask_elem(masks.dtype), mk.data_ptr(), bx.data_ptr(), k, mh, mw, h, w, threshold,
                                                        int(as_uint8), out.data_ptr(), _stream(masks)), "frcnn_ops_paste_masks_aligned")
    return out


@_paste_masks_aligned.register_fake
def _(masks, boxes, h, w, threshold, as_uint8):
    return torch.empty((masks.shape[0], h, w), dtype=torch.uint8, device=masks.device)


@torch.library.custom_op("frcnn::masks_to_boxes", mutates_args=())
def _masks_to_boxes(masks: Tensor) -> Tensor:
    """masks [N, H, W] of 1-, 2- or 4-byte elements (bool as uint8)."""
    n, h, w = masks.shape
    out = torch.empty((n, 4), dtype=torch.float32, device=masks.device)
    if n == 0:
        return out
    with torch.cuda.device(masks.device):
        mk = masks.contiguous()
        ws = _workspace("masks_to_boxes", masks, n, h, w, mk.element_size())
        nv.check(nv.lib().frcnn_ops_masks_to_boxes(mk.element_size(), mk.data_ptr(), n, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _stream(masks)), "frcnn_ops_masks_to_boxes")
    return out


@_masks_to_boxes.register_fake
def _(masks):
    return torch.empty((masks.shape[0], 4), dtype=torch.float32, device=masks.device)


_MASKS_TO_BOXES_DTYPES = (torch.bool, torch.uint8) + _MAP_DTYPES
_MASKS_TO_BOXES_WHAT = "bool, uint8, float32, float16 or bfloat16"


def _image_shape(name, shape):
    if not (isinstance(shape, (tuple, list, torch.Size)) and len(shape) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in shape)):
        raise TypeError("%s must be a pair of ints (H, W), got %r" % (name, shape))
    h, w = shape
    if h < 1 or w < 1:
        raise ValueError("%s must be at least (1, 1), got (%d, %d)" % (name, h, w))
    if h * w > MAX_MASK_PLANE:
        raise ValueError("%s (%d, %d) has more than MAX_MASK_PLANE = %d pixels (indices inside one image are 32-bit)" % (name, h, w, MAX_MASK_PLANE))
    return h, w


def _paste_input(masks, boxes, shape, shape_name, float64, fallback):
    """The checks the paste operators and their twins share (fallback: the twin's name for a GPU operator, None for the twin itself);
    returns (H, W)."""
    dtypes = _MAP_DTYPES + ((torch.float64,) if float64 else ())
    what = _MAP_WHAT + (" (or float64)" if float64 else "")
    if fallback is None:
        for name, t, d, wh in (("masks", masks, dtypes, what), ("boxes", boxes, (torch.float32,), "float32")):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
            if t.dtype not in d:
                raise TypeError("%s must be %s, got %s" % (name, wh, t.dtype))
    else:
        _check_tensor("masks", masks, dtypes, what, fallback)
        _check_tensor("boxes", boxes, (torch.float32,), "float32", fallback)
    _check_same_device(masks, boxes, "masks", "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("boxes must be [K, 4], got shape %s" % (tuple(boxes.shape),))
    return _image_shape(shape_name, shape)


def _paste_in_image_input(masks, boxes, img_shape, padding, float64, fallback):
    h, w = _paste_input(masks, boxes, img_shape, "img_shape", float64, fallback)
    if masks.dim() != 4 or masks.shape[1] != 1:
        raise ValueError("masks must be [K, 1, M, M], got shape %s" % (tuple(masks.shape),))
    if masks.shape[2] != masks.shape[3]:
        raise ValueError("masks must be square, [K, 1, M, M] (paste_masks_aligned takes rectangular ones), got shape %s" % (tuple(masks.shape),))
    if masks.shape[0] != boxes.shape[0]:
        raise ValueError("masks and boxes must have the same K, got %d masks and %d boxes" % (masks.shape[0], boxes.shape[0]))
    if not isinstance(padding, int) or isinstance(padding, bool):
        raise TypeError("padding must be an int, got %r" % (padding,))
    if not 0 <= padding <= MAX_PASTE_PADDING:
        raise ValueError("padding must lie in [0, %d], got %d" % (MAX_PASTE_PADDING, padding))
    if not 1 <= masks.shape[2] <= MAX_PASTE_MASK_SIDE:
        raise ValueError("masks must be M x M with 1 <= M <= MAX_PASTE_MASK_SIDE = %d, got M = %d" % (MAX_PASTE_MASK_SIDE, masks.shape[2]))
    return h, w


def _paste_aligned_input(masks, boxes, image_shape, threshold, float64, fallback):
    """Returns (H, W, masks as [K, Mh, Mw], float32(threshold), as_uint8)."""
    h, w = _paste_input(masks, boxes, image_shape, "image_shape", float64, fallback)
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3:
        raise ValueError("masks must be [K, Mh, Mw] or [K, 1, Mh, Mw], got shape %s" % (tuple(masks.shape),))
    if masks.shape[0] != boxes.shape[0]:
        raise ValueError("masks and boxes must have the same K, got %d masks and %d boxes" % (masks.shape[0], boxes.shape[0]))
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise TypeError("threshold must be a float, got %r" % (threshold,))
    if not (1 <= masks.shape[1] <= MAX_PASTE_MASK_SIDE and 1 <= masks.shape[2] <= MAX_PASTE_MASK_SIDE):
        raise ValueError("masks must be Mh x Mw with 1 <= Mh, Mw <= MAX_PASTE_MASK_SIDE = %d, got %d x %d"
                         % (MAX_PASTE_MASK_SIDE, masks.shape[1], masks.shape[2]))
    return h, w, masks, C.c_float(threshold).value, threshold < 0


def paste_masks_in_image(masks, boxes, img_shape, padding=1):
    """torchvision's roi_heads.paste_masks_in_image in one launch: masks [K, 1, M, M] (float32 / float16 / bfloat16) padded by `padding`
    zeros and resized bilinearly into the integer boxes of boxes [K, 4] float32 -> [K, 1, H, W] in the masks' dtype, zero elsewhere.
    No autograd (upstream's paste is never differentiated); no host synchronisation."""
    h, w = _paste_in_image_input(masks, boxes, img_shape, padding, False, "paste_masks_in_image_pytorch")
    return _paste_masks_in_image(masks.detach(), boxes.detach(), h, w, padding)


def paste_masks_aligned(masks, boxes, image_shape, threshold=0.5):
    """detectron2's paste_masks_in_image / mmdet's _do_paste_mask and its threshold in one launch: masks [K, Mh, Mw] or [K, 1, Mh, Mw]
    sampled bilinearly (zero padding) at every pixel centre of boxes [K, 4] float32 -> [K, H, W], torch.bool (value >= threshold) for
    threshold >= 0, else torch.uint8 (trunc(255 value), saturated).  No autograd; no host synchronisation."""
    h, w, mk, thr, as_uint8 = _paste_aligned_input(masks, boxes, image_shape, threshold, False, "paste_masks_aligned_pytorch")
    out = _paste_masks_aligned(mk.detach(), boxes.detach(), h, w, thr, as_uint8)
    return out if as_uint8 else out.view(torch.bool)


def _masks_to_boxes_input(masks, fallback):
    dtypes = _MASKS_TO_BOXES_DTYPES + ((torch.float64,) if fallback is None else ())
    what = _MASKS_TO_BOXES_WHAT + (" (or float64)" if fallback is None else "")
    if fallback is None:
        if not isinstance(masks, torch.Tensor):
            raise TypeError("masks must be a torch.Tensor, got %s" % type(masks).__name__)
        if masks.dtype not in dtypes:
            raise TypeError("masks must be %s, got %s" % (what, masks.dtype))
    else:
        _check_tensor("masks", masks, dtypes, what, fallback)
    if masks.dim() != 3:
        raise ValueError("masks must be [N, H, W], got shape %s" % (tuple(masks.shape),))
    _image_shape("the masks' (H, W)", tuple(masks.shape[1:]))


def masks_to_boxes(masks):
    """torchvision.ops.masks_to_boxes without its loop: masks [N, H, W] (bool, uint8, float32, float16, bfloat16) -> float32 [N, 4],
    (x_min, y_min, x_max, y_max) over the pixels != 0, maxima inclusive; an all-zero mask gives (0, 0, 0, 0) (detectron2's convention;
    torchvision raises).  No autograd; no host synchronisation."""
    _masks_to_boxes_input(masks, "masks_to_boxes_pytorch")
    m = masks.detach().contiguous()
    return _masks_to_boxes(m.view(torch.uint8) if m.dtype == torch.bool else m)


def _mask_blend(p, iy, iy1, ly, ix, ix1, lx):
    """(1 - ly) ((1 - lx) p[iy][ix] + lx p[iy][ix1]) + ly ((1 - lx) p[iy1][ix] + lx p[iy1][ix1]) for p [K, A, B], row terms [K, H] and
    column terms [K, W] -> [K, H, W]."""
    k, h, w = p.shape[0], iy.shape[1], ix.shape[1]
    rows0 = p.gather(1, iy[:, :, None].expand(k, h, p.shape[2]))
    rows1 = p.gather(1, iy1[:, :, None].expand(k, h, p.shape[2]))
    cx, cx1, lx, ly = ix[:, None, :].expand(k, h, w), ix1[:, None, :].expand(k, h, w), lx[:, None, :], ly[:, :, None]
    top = (1 - lx) * rows0.gather(2, cx) + lx * rows0.gather(2, cx1)
    bot = (1 - lx) * rows1.gather(2, cx) + lx * rows1.gather(2, cx1)
    return (1 - ly) * top + ly * bot


def _paste_integer_boxes(boxes, m, padding):
    """The integer boxes of paste_masks_in_image's contract, from float32 torch operations, each rounded on its own: (X0, Y0, X1, Y1)
    int64 [K] each, saturated to [-PASTE_CORNER, PASTE_CORNER] (a NaN row: 0; such rows are dead anyway)."""
    b = boxes.detach().to(torch.float32)
    s = torch.tensor((m + 2 * padding) / m, dtype=torch.float32, device=b.device)

    def corners(lo, hi):
        half = (hi - lo) * 0.5
        c = (hi + lo) * 0.5
        half = half * s
        return [torch.nan_to_num(v, nan=0.0).clamp(-PASTE_CORNER, PASTE_CORNER).to(torch.int64) for v in (c - half, c + half)]
    (x0, x1), (y0, y1) = corners(b[:, 0], b[:, 2]), corners(b[:, 1], b[:, 3])
    return x0, y0, x1, y1


def paste_masks_in_image_pytorch(masks, boxes, img_shape, padding=1):
    """paste_masks_in_image's contract, deviations included, from torch operations: any device, float64 masks too (the integer boxes are
    the float32 sequence's either way; everything after them is then float64).  16-bit masks compute in float32 and round once."""
    h, w = _paste_in_image_input(masks, boxes, img_shape, padding, True, None)
    k, m = masks.shape[0], masks.shape[2]
    mp = m + 2 * padding
    math = torch.float64 if masks.dtype == torch.float64 else torch.float32
    dev = masks.device
    with torch.no_grad():
        if k == 0:
            return masks.new_zeros((0, 1, h, w))
        x0, y0, x1, y1 = _paste_integer_boxes(boxes, m, padding)
        alive = torch.isfinite(boxes.detach()).all(1) & (x0 <= x1) & (y0 <= y1)
        p = torch.nn.functional.pad(masks.detach()[:, 0].to(math), (padding,) * 4)

        def axis(n, origin, size):
            d = torch.arange(n, device=dev)[None, :] - origin[:, None]
            r = torch.full((k,), float(mp), dtype=math, device=dev) / size.to(math)
            sc = (r[:, None] * (d.to(math) + 0.5) - 0.5).clamp(min=0)
            i0 = sc.to(torch.int64).clamp(max=mp - 1)
            return (d >= 0) & (d < size[:, None]), i0, i0 + (i0 < mp - 1).to(torch.int64), sc - i0.to(math)
        in_x, ix, ix1, lx = axis(w, x0, (x1 - x0 + 1).clamp(min=1))
        in_y, iy, iy1, ly = axis(h, y0, (y1 - y0 + 1).clamp(min=1))
        value = _mask_blend(p, iy, iy1, ly, ix, ix1, lx)
        keep = alive[:, None, None] & in_y[:, :, None] & in_x[:, None, :]
        return torch.where(keep, value, value.new_zeros(())).to(masks.dtype)[:, None]


def paste_masks_aligned_pytorch(masks, boxes, image_shape, threshold=0.5):
    """paste_masks_aligned's contract, deviations included, from torch operations: any device, float64 masks too (then the sample
    coordinates and the blend are float64 on the float32 boxes, compared with float32(threshold))."""
    h, w, mk, thr, as_uint8 = _paste_aligned_input(masks, boxes, image_shape, threshold, True, None)
    k, mh, mw = mk.shape
    math = torch.float64 if mk.dtype == torch.float64 else torch.float32
    dev = mk.device
    with torch.no_grad():
        if k == 0:
            return torch.zeros((0, h, w), dtype=torch.uint8 if as_uint8 else torch.bool, device=dev)
        b = boxes.detach()
        alive = torch.isfinite(b).all(1) & (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
        b = b.to(math)
        p = torch.nn.functional.pad(mk.detach().to(math), (1, 1, 1, 1))              # the zero padding: index i + 1 holds mask[i]

        def axis(n, c0, c1, m):
            c = torch.arange(n, dtype=math, device=dev) + 0.5
            sc = (c[None, :] - c0[:, None]) / (c1 - c0)[:, None] * m - 0.5
            ok = alive[:, None] & (sc > -1) & (sc < m)
            f = torch.where(ok, sc.floor(), sc.new_zeros(()))
            i0 = f.to(torch.int64) + 1
            return ok, i0, i0 + 1, torch.where(ok, sc - f, sc.new_zeros(()))
        ok_x, ix, ix1, lx = axis(w, b[:, 0], b[:, 2], mw)
        ok_y, iy, iy1, ly = axis(h, b[:, 1], b[:, 3], mh)
        value = _mask_blend(p, iy, iy1, ly, ix, ix1, lx)
        value = torch.where(ok_y[:, :, None] & ok_x[:, None, :], value, value.new_zeros(()))
        live = alive[:, None, None]
        if as_uint8:
            q = value * 255
            q = torch.where(q >= 255, q.new_full((), 255.0), torch.where(q > 0, q.trunc(), q.new_zeros(())))
            return q.to(torch.uint8) * live.to(torch.uint8)
        return (value >= torch.tensor(thr, dtype=torch.float32, device=dev).to(math)) & live


def masks_to_boxes_pytorch(masks):
    """masks_to_boxes' contract from torch operations: any device, float64 masks too."""
    _masks_to_boxes_input(masks, None)
    n, h, w = masks.shape
    with torch.no_grad():
        nz = masks.detach() != 0                                                      # NaN != 0, -0.0 == 0
        cols, rows = nz.any(1), nz.any(2)
        xs, ys = torch.arange(w, device=masks.device)[None, :], torch.arange(h, device=masks.device)[None, :]
        out = torch.stack([torch.where(cols, xs, w).amin(1), torch.where(rows, ys, h).amin(1),
                           torch.where(cols, xs, -1).amax(1), torch.where(rows, ys, -1).amax(1)], dim=1).to(torch.float32)
        return torch.where(cols.any(1)[:, None], out, out.new_zeros(()))


# ---- heatmaps_to_keypoints / keypointrcnn_inference / keypoints_to_heatmap: a Keypoint R-CNN's last step (csrc/ops_keypoint.hip) -------
# One run on an MI355X (tools/ops_bench.py --only keypoint; K = 17, 56 x 56 maps, boxes of an 800 x 1333 image): microseconds of the
# operator and of its _pytorch twin (upstream's loop) on the same device, and the operator's rate over the pixels of the resized images.
# The image-sized case is what a single block per (RoI, keypoint) costs when only 68 blocks exist: still ahead of the loop, so a large
# box is not split over several blocks.
KEYPOINT_BENCH = {
    "R = 100 detections, float32 maps": {"ops": 291.6, "twin": 16265.0, "Gpixel/s": 254.4},
    "R = 100 detections, float16 maps": {"ops": 291.3, "twin": 16160.1, "Gpixel/s": 254.7},
    "R = 4 image-sized boxes, float32 maps": {"ops": 927.4, "twin": 1466.3, "Gpixel/s": 60.7},
}


@torch.library.custom_op("frcnn::heatmaps_to_keypoints", mutates_args=())
def _heatmaps_to_keypoints(maps: Tensor, rois: Tensor) -> Tensor:
    """maps [R, K, Mh, Mw], rois [R, 4] float32 -> float32 [R, K, 4] = (x, y, logit, prob)."""
    r, k, mh, mw = maps.shape
    out = torch.empty((r, k, 4), dtype=torch.float32, device=maps.device)
    if r == 0 or k == 0:
        return out
    with torch.cuda.device(maps.device):
        mp, bx = maps.contiguous(), rois.contiguous()
        nv.check(nv.lib().frcnn_ops_heatmaps_to_keypoints(_mask_elem(maps.dtype), mp.data_ptr(), bx.data_ptr(), r, k, mh, mw, out.data_ptr(),
                                                          _stream(maps)), "frcnn_ops_heatmaps_to_keypoints")
    return out


@_heatmaps_to_keypoints.register_fake
def _(maps, rois):
    return torch.empty((maps.shape[0], maps.shape[1], 4), dtype=torch.float32, device=maps.device)


_KEYPOINT_BOX_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)


def _keypoint_input(maps, rois):
    """The checks heatmaps_to_keypoints and its twin share; returns rois as float32."""
    for name, t, d, what in (("maps", maps, _MAP_DTYPES + (torch.float64,), _MAP_WHAT + " (or float64: the _pytorch twin)"),
                             ("rois", rois, _KEYPOINT_BOX_DTYPES, "a float dtype")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.dtype not in d:
            raise TypeError("%s must be %s, got %s" % (name, what, t.dtype))
    _check_same_device(maps, rois, "maps", "rois")
    if maps.dim() != 4:
        raise ValueError("maps must be [R, K, Mh, Mw], got shape %s" % (tuple(maps.shape),))
    if rois.dim() != 2 or rois.shape[1] != 4:
        raise ValueError("rois must be [R, 4], got shape %s" % (tuple(rois.shape),))
    if maps.shape[0] != rois.shape[0]:
        raise ValueError("maps and rois must have the same R, got %d maps and %d rois" % (maps.shape[0], rois.shape[0]))
    if not (1 <= maps.shape[2] <= MAX_KEYPOINT_MAP_SIDE and 1 <= maps.shape[3] <= MAX_KEYPOINT_MAP_SIDE):
        raise ValueError("maps must be Mh x Mw with 1 <= Mh, Mw <= MAX_KEYPOINT_MAP_SIDE = %d, got %d x %d"
                         % (MAX_KEYPOINT_MAP_SIDE, maps.shape[2], maps.shape[3]))
    return rois.detach().to(torch.float32)


def _keypoints_torchvision(scored):
    """(x, y, logit, prob) [R, K, 4] as torchvision returns it: (x, y, 1) [R, K, 3] and the logits [R, K]."""
    return torch.cat([scored[..., :2], torch.ones_like(scored[..., :1])], dim=2), scored[..., 2]


def heatmaps_to_keypoints_scored(maps, rois):
    """detectron2's heatmaps_to_keypoints in one launch: maps [R, K, Mh, Mw] (float32 / float16 / bfloat16), rois [R, 4] -> float32
    [R, K, 4] = (x, y, logit, prob) of the maximum of each map resized bicubically to its RoI.  No autograd; no host synchronisation.
    CPU tensors and float64 maps are served by heatmaps_to_keypoints_scored_pytorch."""
    boxes = _keypoint_input(maps, rois)
    if maps.device.type == "cpu" or maps.dtype == torch.float64:
        return heatmaps_to_keypoints_scored_pytorch(maps, rois)
    return _heatmaps_to_keypoints(maps.detach(), boxes)


def heatmaps_to_keypoints(maps, rois):
    """torchvision's roi_heads.heatmaps_to_keypoints in one launch: (xy_preds [R, K, 3] = (x, y, 1), end_scores [R, K] = the logits)."""
    return _keypoints_torchvision(heatmaps_to_keypoints_scored(maps, rois))


def keypointrcnn_inference(x, boxes):
    """torchvision's roi_heads.keypointrcnn_inference: x [sum of R_i, K, Mh, Mw], boxes a list of [R_i, 4] per image -> (list of xy_preds
    [R_i, K, 3], list of end_scores [R_i, K]).  One launch for all images, then the split."""
    if not isinstance(boxes, (list, tuple)) or not all(isinstance(b, torch.Tensor) for b in boxes):
        raise TypeError("boxes must be a list of Tensor[R_i, 4], one per image, got %s" % type(boxes).__name__)
    if len(boxes) == 0:
        return [], []
    per_image = [b.shape[0] for b in boxes]
    xy, scores = heatmaps_to_keypoints(x, torch.cat(list(boxes), dim=0))
    return list(xy.split(per_image, dim=0)), list(scores.split(per_image, dim=0))


def heatmaps_to_keypoints_scored_pytorch(maps, rois):
    """heatmaps_to_keypoints_scored's contract, defined cases included, as the per-RoI loop upstream runs (two host reads, F.interpolate
    (bicubic), argmax and a gather per RoI): any device, float64 maps too (computed and returned in float64; else float32)."""
    boxes = _keypoint_input(maps, rois)
    r, k = maps.shape[:2]
    math = torch.float64 if maps.dtype == torch.float64 else torch.float32
    with torch.no_grad():
        out = torch.full((r, k, 4), float("nan"), dtype=math, device=maps.device)
        if r == 0 or k == 0:
            return out
        flat = maps.detach().to(math).reshape(r, k, -1)
        first = flat[:, :, 0]
        constant = (flat == first[:, :, None]).all(2)
        w, h = (boxes[:, 2] - boxes[:, 0]).clamp(min=1), (boxes[:, 3] - boxes[:, 1]).clamp(min=1)
        wc, hc = w.ceil(), h.ceil()
        ok = torch.isfinite(boxes).all(1) & (wc <= MAX_KEYPOINT_ROI_SIDE) & (hc <= MAX_KEYPOINT_ROI_SIDE)
        sizes = torch.stack([torch.where(ok, wc, wc.new_zeros(())), torch.where(ok, hc, hc.new_zeros(()))], 1).tolist()
        for i, (wi, hi) in enumerate(sizes):
            if wi == 0:                                                          # refused: four NaNs
                continue
            wi, hi = int(wi), int(hi)
            image = torch.nn.functional.interpolate(flat[i].reshape((k, 1) + tuple(maps.shape[2:])), size=(hi, wi), mode="bicubic",
                                                    align_corners=False).reshape(k, -1)
            pos = torch.where(constant[i], 0, image.argmax(1))                   # NaN is the largest, the first of equals wins
            v = torch.where(constant[i], first[i], image.gather(1, pos[:, None])[:, 0])
            xi, yi = pos % wi, pos // wi
            out[i, :, 0] = (xi.to(torch.float32) + 0.5) * (w[i] / wc[i]) + boxes[i, 0]
            out[i, :, 1] = (yi.to(torch.float32) + 0.5) * (h[i] / hc[i]) + boxes[i, 1]
            out[i, :, 2] = v
            out[i, :, 3] = 1 / (flat[i] - v[:, None]).exp().sum(1)
        return out


def heatmaps_to_keypoints_pytorch(maps, rois):
    """heatmaps_to_keypoints_scored_pytorch in torchvision's shape: (xy_preds [R, K, 3], end_scores [R, K])."""
    return _keypoints_torchvision(heatmaps_to_keypoints_scored_pytorch(maps, rois))


def keypoints_to_heatmap(keypoints, rois, heatmap_size):
    """torchvision's roi_heads.keypoints_to_heatmap, the training-target encoder: keypoints [R, K, 3] = (x, y, visibility), rois [R, 4],
    heatmap_size S -> (heatmaps int64 [R, K]: y * S + x of the keypoint's cell in its RoI's S x S map, 0 where not valid; valid int64
    [R, K]: inside the map and visibility > 0).  A keypoint exactly on the RoI's right or bottom edge belongs to the last cell.
    Plain torch operations on any device: a handful of elementwise operations that read nothing back to the host, so there is no
    kernel to write (the loss over it is F.cross_entropy)."""
    for name, t in (("keypoints", keypoints), ("rois", rois)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if keypoints.dim() != 3 or keypoints.shape[2] != 3:
        raise ValueError("keypoints must be [R, K, 3], got shape %s" % (tuple(keypoints.shape),))
    if rois.dim() != 2 or rois.shape[1] != 4 or rois.shape[0] != keypoints.shape[0]:
        raise ValueError("rois must be [R, 4] with the keypoints' R = %d, got shape %s" % (keypoints.shape[0], tuple(rois.shape)))
    if not isinstance(heatmap_size, int) or isinstance(heatmap_size, bool) or heatmap_size < 1:
        raise ValueError("heatmap_size must be a positive int, got %r" % (heatmap_size,))
    s = heatmap_size
    x, y = keypoints[..., 0], keypoints[..., 1]
    on_right, on_bottom = x == rois[:, 2, None], y == rois[:, 3, None]
    size = rois.new_full((), s)                                                  # S / extent as one division (int / Tensor is reciprocal * S)
    x = ((x - rois[:, 0, None]) * (size / (rois[:, 2] - rois[:, 0]))[:, None]).floor().long()
    y = ((y - rois[:, 1, None]) * (size / (rois[:, 3] - rois[:, 1]))[:, None]).floor().long()
    x, y = torch.where(on_right, s - 1, x), torch.where(on_bottom, s - 1, y)
    valid = ((x >= 0) & (y >= 0) & (x < s) & (y < s) & (keypoints[..., 2] > 0)).long()
    return (y * s + x) * valid, valid
