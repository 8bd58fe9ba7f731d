/*
 * frcnn_hip.h -- C ABI of libfrcnn_hip.so, the MI355X (gfx950) Faster R-CNN hot path: inference (forward / predict),
 * and the operators of the train step (section "Training path" below).
 *
 * The reference (trzy/FasterRCNN, pytorch tree) has no FFI: its hot path is Python calling
 * torch / torchvision native kernels.  Each entry point below replaces one of those call sites;
 * the reference file:line it stands in for is cited per function (paths relative to
 * /root/reference/pytorch/FasterRCNN/).  INTEGRATION.md shows how a maintainer of the reference
 * binds them (the torchvision.ops call sites through fasterrcnn_amd.ops, on the frcnn_ops_* entry points).
 *
 * Conventions (all functions):
 *   - return int: 0 = FRCNN_OK, negative = error code below; never throws, never aborts.
 *   - every pointer named d_* / marked "device" is a DEVICE pointer owned by the caller
 *     (e.g. a torch allocation); nothing is allocated behind the caller's back except inside
 *     an frcnn_ctx (frcnn_ctx_create / frcnn_ctx_destroy).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *     asynchronously on it, no host synchronisation unless stated.
 *   - activations are float32, NHWC ("pixel-major, channel-contiguous") unless stated; the
 *     network input is the reference's NCHW float32 image.
 *   - box layout is the reference's (y1, x1, y2, x2) in image pixels; anchors are
 *     (center_y, center_x, height, width).
 */
#ifndef FRCNN_HIP_H
#define FRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_OK            0
#define FRCNN_EINVAL       -1   /* bad argument (null pointer, shape not supported by the kernel) */
#define FRCNN_EHIP         -2   /* a HIP runtime call failed; see frcnn_last_hip_error() */
#define FRCNN_ENOMEM       -3   /* workspace allocation failed */
#define FRCNN_EUNSUPPORTED -4   /* valid request outside what this build implements */
#define FRCNN_ENODEVICE    -5   /* no gfx950 device visible */

#define FRCNN_ABI_VERSION 21  /* 2: training entry points, frcnn_forward_params.conv_blocks_target; 3: Winograd F(2x2,3x3) layers; 4: one-launch Winograd layers;
                                 5: bf16 gradient GEMMs (the *_math entry points); 6: x6t GEMM, x6 Winograd layers, frcnn_forward_params.winograd_x6_mask,
                                 timing classes 8 / 9; 7: batched feature extractor (frcnn_resnet_backbone, frcnn_resnet_forward_features,
                                 frcnn_ctx_create_backbone, frcnn_conv3x3_nhwc_winograd_fused_maps); 8: the f32x3 arithmetic (frcnn_*_x3t, frcnn_*_winograd_x3,
                                 frcnn_forward_params.winograd_x3_mask, FRCNN_FC_F32X3T, frcnn_bottleneck_weights.x3_mask); 9: one-launch f32x3 Winograd layers
                                 in the forward (frcnn_forward_params.winograd_x3f_mask, timing class 10), frcnn_roi_pool_x3t; 10: frcnn_conv3x3_c3_cmax, bits 1 (conv1_2)
                                 and 13 (RPN trunk) of winograd_x3f_mask; 11: frcnn_conv_nhwc_x3g, frcnn_tensor_absmax, frcnn_bottleneck_weights.g3 / .wmax;
                                 12: frcnn_x3_saturation_events, FRCNN_X3F_WAVES4 / FRCNN_X3F_WAVES8; 13: REMOVED the round-2 f32x6 kernels that no table has used since round 3
                                 (frcnn_pack_conv3x3_x6, frcnn_conv3x3_nhwc_x6, frcnn_split_rows_x6, frcnn_linear_x6(_workspace_bytes), math mode 1 =
                                 FRCNN_MATH_F32X6 and fc mode 1 = FRCNN_FC_F32X6 are FRCNN_EINVAL); the f32x6 arithmetic stays as gemm_x6t / wino_x6; 14: FRCNN_X3F_PAIR, frcnn_conv3x3_winograd_x3_pair_workspace_bytes, frcnn_forward_params.winograd_x3p_mask,
                                 frcnn_resnet_rpn_roipool / frcnn_ctx_create_head / frcnn_resnet_head; 15: frcnn_conv_nhwc_x3g_tickets (split reductions finished inside the kernel), frcnn_pack_conv_x3g_weights + FRCNN_X3G_WSPLIT + frcnn_bottleneck_weights.g3 == 2 (pre-split weight packs);
                                 16: frcnn_train_conv, frcnn_bottleneck_backward(_workspace_bytes): the backward of one trainable bottleneck as ONE call, weight gradients on a second stream;
                                 17: frcnn_dropout, frcnn_dropout_relu_backward (training-mode dropout of the VGG-16 head);
                                 18: REMOVED the eight-wave (round 5) and two-pass (round 6) forms of the one-launch f32x3 layer that no table has used (FRCNN_X3F_WAVES4 /
                                 FRCNN_X3F_WAVES8 / FRCNN_X3F_PAIR, frcnn_conv3x3_winograd_x3_pair_workspace_bytes, frcnn_forward_params.winograd_x3p_mask;
                                 measured in DESIGN.md section 5);
                                 19: frcnn_ops_* (torchvision.ops-style roi_align / roi_pool / nms over N images, no context: fasterrcnn_amd.ops);
                                 20: frcnn_ops_ms_roi_align(_backward / _workspace_bytes): torchvision.ops.MultiScaleRoIAlign (FPN pooling) in one launch
                                 per direction;
                                 21: frcnn_ops_*_16: the RoI operators on float16 / bfloat16 maps (widen, float32 arithmetic, one rounding);
                                 still 21 (round 7, additions only: no existing prototype or struct changed, and tests/test_ops_half_cpu.py pins the number):
                                 frcnn_predict_submit (one image enqueued natively: producer dependency only when the producer is busy, one packed
                                 D2H copy), frcnn_stream_depend, frcnn_output_block_layout, frcnn_ctx_submit_stats, frcnn_streams_share_queue;
                                 still 21 (additions only, the number stays pinned): frcnn_ops_ps_roi_pool / frcnn_ops_ps_roi_align, their _backward and
                                 _16 forms (torchvision.ops.ps_roi_pool / ps_roi_align, R-FCN's position-sensitive pooling, on NCHW maps);
                                 still 21 (additions only): frcnn_ops_deform_* and frcnn_deform_geom (torchvision.ops.deform_conv2d, deformable
                                 convolution v1 / v2, forward and backward on frcnn_gemm_tn's kernel);
                                 still 21 (additions only): frcnn_ops_deform_roi_pool, its _backward, _16, _workspace_bytes and _cull_list forms
                                 (deformable RoI pooling of DCN v1 / v2, mmcv's deform_roi_pool);
                                 still 21 (additions only): frcnn_ops_box_iou_rotated, frcnn_ops_nms_rotated, frcnn_ops_roi_align_rotated, its
                                 _backward, _16 and _cull_list forms (rotated boxes: mmcv's box_iou_rotated, nms_rotated, roi_align_rotated);
                                 still 21 (additions only): frcnn_ops_carafe, its _backward and _16 forms and the frcnn_ops_carafe_max_kernel /
                                 _channel_chunk / _tile_width / _tile_height getters (CARAFE upsampling: mmcv's carafe);
                                 still 21 (additions only): frcnn_ops_msda_forward, _backward_loc, _plan, _backward_value, _workspace_bytes, the _16
                                 forms and the frcnn_ops_msda_max_levels / _max_points / _max_channels / _block_items / _segment getters (multi-scale deformable
                                 attention: mmcv's ms_deform_attn);
                                 still 21 (additions only): frcnn_ops_prroi_pool, its _backward, _16, _workspace_bytes and _cull_list forms
                                 (Precise RoI Pooling with box gradients: IoU-Net's PrRoIPool, mmcv's prroi_pool);
                                 still 21 (additions only): frcnn_ops_dcnv3_forward, _backward_offset, _plan, _backward_input, _workspace_bytes, the
                                 _16 forms and the frcnn_ops_dcnv3_max_kernel / _max_channels / _block_items getters (DCNv3: InternImage's deformable
                                 convolution v3);
                                 still 21 (additions only): frcnn_ops_dcnv4_forward, _backward_offset_mask, _plan, _backward_input, _workspace_bytes,
                                 the _16 forms and the frcnn_ops_dcnv4_block_items / _record getters (DCNv4: FlashInternImage's deformable
                                 convolution v4, one packed offset_mask tensor, optionally without the centre point);
                                 still 21 (additions only): frcnn_ops_diff_iou_rotated and its _backward (the differentiable IoU of aligned
                                 rotated boxes: mmcv's diff_iou_rotated_2d / _3d);
                                 still 21 (additions only): frcnn_ops_soft_nms, its _workspace_bytes and the frcnn_ops_soft_nms_block_threads /
                                 _lds_boxes / _max_boxes getters (Soft-NMS, per label: mmcv's CPU-only soft_nms);
                                 still 21 (additions only): frcnn_ops_border_align, its _backward, _16 and _cull_list forms (BorderAlign, the
                                 border pooling of BorderDet: mmcv's border_align);
                                 still 21 (additions only): frcnn_ops_riroi_align_rotated, its _backward, _16 and _max_orientations forms
                                 (ReDet's rotation-invariant RoI pooling: mmcv's riroi_align_rotated) and frcnn_ops_rotated_feature_align, its
                                 _plan, _backward and _16 forms (R3Det's feature refinement: mmcv's rotated_feature_align);
                                 still 21 (additions only): frcnn_ops_convex_iou, its _tile_rows getter, frcnn_ops_convex_giou and
                                 frcnn_ops_min_area_polygons (the point-set operators of Oriented RepPoints, CFA and SASM: mmcv's convex_iou,
                                 convex_giou and min_area_polygons);
                                 still 21 (additions only): the frcnn_ops_deform_*_16 forms (deformable convolution on float16 / bfloat16 tensors,
                                 its products on the 16-bit matrix pipe);
                                 still 21 (no prototype or struct changed): frcnn_detections returns the documented FRCNN_EUNSUPPORTED for images past
                                 the limit stated with it (sides of about 3000 px at the 0.3 threshold; it accepted them without a proof before);
                                 still 21 (additions only): frcnn_ops_box_iou_quadri, frcnn_ops_nms_quadri, frcnn_ops_points_in_polygons and the
                                 frcnn_ops_box_iou_quadri_tile_rows / frcnn_ops_points_in_polygons_tile_rows / frcnn_ops_quadri_max_rows /
                                 _max_columns getters (the quadrilateral operators: mmcv's box_iou_quadri, nms_quadri and points_in_polygons);
                                 still 21 (additions only): frcnn_ops_masked_conv2d, frcnn_ops_masked_conv2d_workspace_bytes, the
                                 frcnn_ops_masked_conv2d_tile_pixels / _tile_channels / _k_chunk / _max_index getters and FRCNN_OPS_F32 (the sparse
                                 convolution of Guided Anchoring's heads: mmcv's masked_conv2d);
                                 still 21 (additions only): frcnn_ops_paste_masks_in_image, frcnn_ops_paste_masks_aligned, frcnn_ops_masks_to_boxes,
                                 frcnn_ops_masks_to_boxes_workspace_bytes and the frcnn_ops_paste_masks_max_side / _max_padding / _max_corner and
                                 frcnn_ops_mask_max_plane getters (a Mask R-CNN's last step: torchvision's and detectron2's paste_masks_in_image,
                                 torchvision's masks_to_boxes);
                                 still 21 (additions only): frcnn_ops_heatmaps_to_keypoints and the frcnn_ops_keypoint_max_map_side /
                                 _max_roi_side / _block_threads getters (a Keypoint R-CNN's last step: torchvision's and detectron2's
                                 heatmaps_to_keypoints) */

/* flags for frcnn_conv3x3_nhwc / frcnn_linear */
#define FRCNN_RELU   1u
#define FRCNN_POOL2  2u   /* fuse MaxPool2d(2, stride 2, floor) into the conv epilogue */
#define FRCNN_X3G_WSPLIT 0x800u   /* frcnn_conv_nhwc_x3g(_tickets): d_w_packed is the PRE-SPLIT image of the float32 pack (frcnn_pack_conv_x3g_weights, round 6) */

int         frcnn_abi_version(void);
const char* frcnn_error_string(int code);
/* hipGetErrorString of the last HIP failure seen by this thread ("" if none). */
const char* frcnn_last_hip_error(void);
/* Number of visible devices whose gcnArchName starts with "gfx950"; <0 on error. */
int         frcnn_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Anchors.  Replaces models/anchors.py:43-135 generate_anchor_maps (float64 math, one final
 * cast to float32 -- reproduced bit-exactly).
 *   d_anchor_map : float32 [fh][fw][9*4]  (cy, cx, h, w) per anchor, k = area-major/aspect-minor
 *   d_valid_map  : float32 [fh][fw][9]    1.0 if the anchor lies inside the image else 0.0
 * ---------------------------------------------------------------------------------------- */
int frcnn_anchors(int image_h, int image_w, int fh, int fw, int feature_pixels,
                  float* d_anchor_map, float* d_valid_map, void* stream);

/* Image preprocessing.  Replaces datasets/image.py:92-100 and :43-57: PIL
 * `Image.resize((out_w, out_h), BILINEAR)` of the decoded 8-bit RGB image (optionally after
 * FLIP_LEFT_RIGHT), reproduced bit for bit (22-bit fixed-point two-pass resampler), then channel
 * order / scaling / (x - mean) / std in float32 into the CHW tensor the model consumes.
 *   d_rgb    : uint8 [H][W][3] RGB (what imageio / PIL decode to)
 *   means, stds: HOST float[3] in OUTPUT channel order (PreprocessingParams.means / .stds)
 *   d_out    : float32 [3][out_h][out_w];  d_out_u8: optional uint8 [out_h][out_w][3] resized RGB
 *   d_ws     : scratch of frcnn_preprocess_workspace_bytes(H, W, out_h, out_w) bytes */
size_t frcnn_preprocess_workspace_bytes(int H, int W, int out_h, int out_w);
int frcnn_preprocess(const unsigned char* d_rgb, int H, int W, int out_h, int out_w, int bgr_order,
                     int horizontal_flip, float scaling, const float* means, const float* stds,
                     float* d_out, unsigned char* d_out_u8, void* d_ws, size_t ws_bytes, void* stream);

/* RPN ground-truth labelling (anchor <-> GT IoU matching).  Replaces models/anchors.py:137-262
 * generate_rpn_map: float64 IoU of every anchor with every ground-truth box (float32 corners
 * (y1,x1,y2,x2)), invalid anchors excluded; object if IoU >= object_thr or the anchor attains a
 * GT box's maximum IoU, background if max IoU < background_thr, ignored otherwise; float32
 * regression targets of the best-IoU box.
 *   d_rpn_map        : float32 [A][6] = (trainable, object, ty, tx, th, tw), A = fh*fw*9
 *   d_object_idx     : int32 [A] flat anchor indices of object anchors, ascending; d_counts[0] of them
 *   d_background_idx : int32 [A] likewise for background anchors; d_counts[1]
 *   d_ws             : scratch, at least 8*n_gt bytes.  n_gt >= 1 (the reference cannot label an
 *                      image without boxes either). */
int frcnn_rpn_targets(const float* d_anchor_map, const float* d_valid_map, int n_anchors,
                      const float* d_gt_boxes, int n_gt, double object_thr, double background_thr,
                      float* d_rpn_map, int32_t* d_object_idx, int32_t* d_background_idx, int32_t* d_counts,
                      void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight repacking (run once at load; device -> device).
 * ---------------------------------------------------------------------------------------- */
/* OIHW [cout][cin][3][3] -> tap-major [9][cout][cin] (cin contiguous) for frcnn_conv3x3_nhwc. */
int frcnn_pack_conv3x3(const float* d_w_oihw, float* d_w_packed, int cout, int cin, void* stream);
/* OIHW [cout][3][3][3] -> [27][cout] (k = ci*9 + r*3 + s major) for frcnn_conv3x3_c3. */
int frcnn_pack_conv3x3_c3(const float* d_w_oihw, float* d_w_packed, int cout, void* stream);
/* fc1 [out][c*ph*pw] (reference flatten order C,7,7: vgg16.py:129) -> [out][(p)*C + c]
 * so that it consumes the NHWC RoI-pool output directly. */
int frcnn_pack_fc_chw_to_hwc(const float* d_w, float* d_w_packed, int out_features, int channels,
                             int pooled_hw, void* stream);
/* Stack row-major matrices [n1][k] and [n2][k] into [n_pad][k] (rows >= n1+n2 zero) and the
 * biases into [n_pad].  Used for the RPN 1x1 heads (rpn.py:40-41) and the detector heads
 * (detector.py:29-30). */
int frcnn_pack_stack_rows(const float* d_w1, const float* d_b1, int n1,
                          const float* d_w2, const float* d_b2, int n2,
                          int k, int n_pad, float* d_w_out, float* d_b_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolutions.  Replace nn.Conv2d(3x3, stride 1, "same") + F.relu (+ nn.MaxPool2d(2,2)) at
 * models/vgg16.py:76-96 and models/rpn.py:88.
 * ---------------------------------------------------------------------------------------- */
/* First layer: Cin = 3, input NCHW float32 [3][H][W], output NHWC [H][W][cout]; cout % 16 == 0.
 * d_w_packed from frcnn_pack_conv3x3_c3. */
int frcnn_conv3x3_c3(const float* d_x_chw, const float* d_w_packed, const float* d_bias,
                     float* d_y, int H, int W, int cout, unsigned flags, void* stream);
/* The same layer (models/vgg16.py:76 conv1_1 + ReLU; cout = 64 only) that also leaves the per-pixel maximum |y| over the 64 output channels in d_cmax_out [H][W]: the scale
 * source of an f32x3 layer that consumes y (d_cmax_in of frcnn_conv3x3_nhwc_winograd_x3_chain).  A plain store per pixel from the lanes
 * that hold its channels (no atomics, nothing to zero); y is bit-identical to frcnn_conv3x3_c3's.  ABI 10. */
int frcnn_conv3x3_c3_cmax(const float* d_x_chw, const float* d_w_packed, const float* d_bias,
                          float* d_y, int H, int W, int cout, unsigned flags, float* d_cmax_out, void* stream);
/* General layer on the f32 MFMA pipe: x NHWC [H][W][cin], y NHWC [H][W][cout] or, with
 * FRCNN_POOL2, [H/2][W/2][cout].  Requires cin % 16 == 0, cout % 64 == 0.
 * d_w_packed from frcnn_pack_conv3x3.  Layers whose output grid cannot fill the chip (the 37x62
 * maps of block 5 / the RPN trunk) run split-K over input channels with a deterministic
 * fixed-order finish; `d_ws` is scratch of at least frcnn_conv3x3_workspace_bytes() bytes
 * (NULL or too small = no split, same results up to fp32 summation order). */
size_t frcnn_conv3x3_workspace_bytes(int H, int W, int cin, int cout);
int frcnn_conv3x3_nhwc(const float* d_x, const float* d_w_packed, const float* d_bias,
                       float* d_y, int H, int W, int cin, int cout, unsigned flags,
                       void* d_ws, size_t ws_bytes, void* stream);
/* The same layer (models/vgg16.py:36-47, models/rpn.py:39; with n_maps > 1 also the stride-1 3x3 of a ResNet
 * bottleneck on the per-RoI maps, models/resnet.py:110) as Winograd F(2x2,3x3) in float32: three launches
 * (input transform, 16 batched exact-f32 MFMA GEMMs over the channels, output transform + bias + ReLU +
 * optional 2x2 max-pool), 2.25x fewer multiplies than the direct form.  No reduced-precision operands: every
 * value is float32 (the filter transform G g G^T is evaluated in float64 and rounded once); results differ
 * from the direct kernel by fp32 rounding only (a few 1e-7 relative per layer).
 *   d_x    : float32 NHWC [n_maps][H][W][cin];  d_y : [n_maps][H][W][cout] ([n_maps][H/2][W/2][cout] with FRCNN_POOL2)
 *   d_u    : float32 [16][cout][cin] from frcnn_pack_conv3x3_winograd (OIHW weights in; d_row_scale, optional,
 *            multiplies filter row `cout` in float32 first = the frozen-BatchNorm fold of frcnn_fold_bn_pack)
 *   d_ws   : scratch of frcnn_conv3x3_winograd_workspace_bytes() = 16*n_maps*ceil(H/2)*ceil(W/2)*(cin+cout)*4 bytes
 * Requires cin % 16 == 0 and cout % 128 == 0 (FRCNN_EUNSUPPORTED otherwise).  The fused forwards use it in
 * math mode FRCNN_MATH_F32_WINOGRAD: VGG-16 / RPN trunk layers where frcnn_conv3x3_uses_winograd(cin, cout) != 0
 * (cin >= 128 and cout >= 256: for narrower layers the transformed tensors cost more HBM traffic than the
 * matrix pipe saves -- measured per VGG-16 layer) and ResNet bottlenecks where
 * frcnn_resnet_block_uses_winograd(width, stride) != 0 (the stride-1 blocks of layer3 and layer4: width >= 256). */
int frcnn_conv3x3_uses_winograd(int cin, int cout);
int frcnn_resnet_block_uses_winograd(int width, int stride);
int frcnn_pack_conv3x3_winograd(const float* d_w_oihw, const float* d_row_scale, float* d_u, int cout, int cin, void* stream);
/* The same filter bank from the direct kernels' tap-major pack [9][cout][cin] (frcnn_pack_conv3x3: the train step's master
 * weights).  data_gradient = 0: the layer's own bank [16][cout][cin]; data_gradient = 1: the bank [16][cin][cout] of the
 * convolution that maps the output gradient (cout channels) to the input gradient (cin channels), i.e. of the 180-degree rotated,
 * channel-transposed filter that frcnn_pack_conv3x3_dgrad builds for the direct kernel (autograd of models/vgg16.py:84-96). */
int frcnn_pack_conv3x3_winograd_taps(const float* d_w_packed, float* d_u, int cout, int cin, int data_gradient, void* stream);
size_t frcnn_conv3x3_winograd_workspace_bytes(int n_maps, int H, int W, int cin, int cout);
int frcnn_conv3x3_nhwc_winograd(const float* d_x, const float* d_u, const float* d_bias,
                                float* d_y, int n_maps, int H, int W, int cin, int cout, unsigned flags,
                                void* d_ws, size_t ws_bytes, void* stream);
/* The same Winograd F(2x2,3x3) float32 layer for ONE map as ONE launch with no V / M scratch (csrc/winofused.hip): a
 * block owns 2 x 16 tiles x 64 output channels and all 16 Winograd positions in MFMA accumulators
 * (v_mfma_f32_16x16x4_f32; the position rows are split over wave pairs); the input transform B^T d B is evaluated on the LDS-staged halo when the operand is formed
 * (same float32 operation order as the three-launch form), the output transform A^T M A + bias + ReLU + optional
 * 2x2 max-pool runs on the accumulators.  HBM traffic of a layer = its input, filter bank and output, so the form pays for
 * every 3x3 stride-1 layer with cin % 16 == 0 and cout % 64 == 0 (FRCNN_EUNSUPPORTED otherwise; H*W*cin*4 and 64*cin*cout < 2^31).
 *   d_u : float32 [cin/16][cout/64][16][64][16] (the 16 positions in the kernel's slab order) from frcnn_pack_conv3x3_winograd_fused (OIHW in; optional per-cout
 *         d_row_scale as above) or frcnn_pack_conv3x3_winograd_fused_taps (tap-major [9][cout][cin] in; data_gradient = 1
 *         packs the bank of the data-gradient convolution cout -> cin channels).  16*cout*cin floats, the values of
 *         frcnn_pack_conv3x3_winograd's bank in another order.
 * The fused forwards use it in math mode FRCNN_MATH_F32_WINOGRAD for every single-map 3x3 stride-1 layer
 * (frcnn_conv3x3_uses_winograd_fused(cin, cout) != 0); the three-launch form stays for ResNet's per-RoI 4 x 4 maps. */
int frcnn_conv3x3_uses_winograd_fused(int cin, int cout);
/* ResNet bottleneck 3x3 (width -> width, n_maps maps in one call): != 0 for ONE map, stride 1, width >= 64 -- the blocks of
 * layer1..3 at inference; frcnn_resnet_forward then expects frcnn_pack_conv3x3_winograd_fused's bank in w2 (frozen-BatchNorm
 * scale as d_row_scale).  The per-RoI maps of layer4 keep frcnn_resnet_block_uses_winograd / the three-launch form. */
int frcnn_resnet_block_uses_winograd_fused(int n_maps, int width, int stride);
int frcnn_pack_conv3x3_winograd_fused(const float* d_w_oihw, const float* d_row_scale, float* d_u, int cout, int cin, void* stream);
int frcnn_pack_conv3x3_winograd_fused_taps(const float* d_w_packed, float* d_u, int cout, int cin, int data_gradient, void* stream);
int frcnn_conv3x3_nhwc_winograd_fused(const float* d_x, const float* d_u, const float* d_bias, float* d_y,
                                      int H, int W, int cin, int cout, unsigned flags, void* stream);
/* The same launch over n_maps maps [n_maps][H][W][cin] -> [n_maps][Ho][Wo][cout] (a batch of images through one layer): the tile
 * blocks of the maps follow each other in ONE grid, every map's result is bit-identical to its own single-map call. */
int frcnn_conv3x3_nhwc_winograd_fused_maps(const float* d_x, const float* d_u, const float* d_bias, float* d_y, int n_maps,
                                           int H, int W, int cin, int cout, unsigned flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Round 3: the f32x6 arithmetic as a general batched GEMM on TILE records ("x6t", csrc/gemm_x6t.hip) and the Winograd layers built
 * on it (csrc/wino_x6.hip).  Replaces the multiply-accumulate of the 512-channel 3x3 convolutions, models/vgg16.py:89-96 and
 * models/rpn.py:88 (cuDNN fp32 in the reference), with fp32-class accuracy on the bf16 matrix pipe.
 *
 * x6t records of a row-major float32 matrix X[R][K], K % 16 == 0, rows padded to `rows_padded` (% 32 == 0):
 *   [K/16][rows_padded/32][3 = hi, mid, lo][1024 B], 1024 B = [k-half 2][row 32][8 bf16]; x = hi + mid + lo exactly.
 *   frcnn_x6t_record_bytes(rows_padded, K)  : bytes of one record array
 *   frcnn_split_rows_x6t                    : [batches][rows][lda] float32 -> [batches] record arrays (rows beyond `rows` zero)
 *   frcnn_gemm_x6t                          : C_b[m][n] = act(bias[n] + residual_b[m][n] + sum_k A_b[m][k] B_b[n][k]), b < batches
 *       (bias / residual may be NULL; the residual has C's layout); A records padded
 *       to a_rows (% FRCNN_X6T_ROW_TILE == 0, >= M), B records padded to b_rows (% FRCNN_X6T_COL_TILE == 0, >= N); batch strides
 *       of the record arrays in BYTES (0: shared by all batches), of C in floats; N % 4 == 0, ldc % 4 == 0; deterministic
 *       (fixed-order split-K when the grid would not cover the chip: d_ws >= frcnn_gemm_x6t_workspace_bytes(M, N, K, batches)).
 * Winograd F(2x2,3x3) layer in this arithmetic (three launches: input transform + exact split -> 16 batched GEMMs -> output
 * transform + bias + ReLU + optional fused 2x2 max-pool), NHWC float32 in and out, cin % 16 == 0, cout % 4 == 0:
 *   frcnn_pack_conv3x3_winograd_x6          : OIHW float32 (optional per-cout scale, as frcnn_pack_conv3x3_winograd) -> the
 *       transformed filter bank as x6t records, frcnn_conv3x3_winograd_x6_pack_bytes(cout, cin) bytes
 *   frcnn_conv3x3_nhwc_winograd_x6          : the layer over n_maps maps [n_maps][H][W][cin]; d_ws >= frcnn_conv3x3_winograd_x6_workspace_bytes(n_maps, H, W, cin, cout)
 *   frcnn_conv3x3_uses_winograd_x6(cin,cout): the layers the fused VGG-16 forward runs this way in math mode
 *       FRCNN_MATH_F32_WINOGRAD when frcnn_forward_params.winograd_x6 != 0 (cin >= 256, cout % 256 == 0).
 * ---------------------------------------------------------------------------------------- */
#define FRCNN_X6T_ROW_TILE 320
#define FRCNN_X6T_COL_TILE 256
size_t frcnn_x6t_record_bytes(int rows_padded, int K);
int frcnn_split_rows_x6t(const float* d_a, int lda, size_t a_batch_floats, void* d_rec, int rows, int rows_padded, int K, int batches,
                         void* stream);
size_t frcnn_gemm_x6t_workspace_bytes(int M, int N, int K, int batches);
int frcnn_gemm_x6t(const void* d_a_rec, int a_rows, size_t a_batch_bytes, const void* d_b_rec, int b_rows, size_t b_batch_bytes,
                   const float* d_bias, const float* d_residual, float* d_c, int ldc, size_t c_batch_floats, int M, int N, int K,
                   int batches, unsigned flags, void* d_ws, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * The same batched GEMM in the "f32x3" arithmetic (csrc/gemm_x3t.hip): HALF the matrix instructions of the f32x6 form.  Every operand
 * row carries a power-of-two scale that puts its largest magnitude into [2^14, 2^15); the scaled float32 value is split into two fp16
 * terms x 2^e = hi + lo (|remainder| <= 2^-22 |x 2^e|) and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with float32
 * accumulation; the epilogue multiplies by the two 2^-e (exact).  Operands are held to 22-23 bits relative to their ROW's largest
 * element -- a perturbation below the float32 accumulation error of either matrix pipe (tests/test_gemm_x3t_gpu.py: error against
 * float64 within the exact-f32 kernel's).
 * x3t records of X[R][K]: [K/16][rows_padded/32][2 = hi, lo][1024 B], 1024 B = [k-half 2][row 32][8 fp16]; scales: float32 2^-e per row.
 *   frcnn_rows_scale_x3t  : [batches][rows][lda] float32 -> d_inv_scale [batches][rows_padded] (2^-e; 1 for zero / padding rows)
 *   frcnn_split_rows_x3t  : the records of the rows scaled by 1 / d_inv_scale
 *   frcnn_gemm_x3t        : as frcnn_gemm_x6t, plus the two scale arrays (batch strides in floats, 0 = shared by all batches)
 * ---------------------------------------------------------------------------------------- */
/* A PACKED x3t operand ("blob") = its record arrays followed by its scale arrays: [batches][frcnn_x3t_record_bytes(rows_padded, K)] bytes, then
 * [batches][rows_padded] float32; frcnn_pack_rows_x3t = frcnn_rows_scale_x3t + frcnn_split_rows_x3t into one such allocation of
 * frcnn_x3t_blob_bytes(rows_padded, K, batches) bytes (weights: fc1_w / fc2_w with fc_math_mode FRCNN_FC_F32X3T, rows_padded = 4096).
 * Winograd F(2x2,3x3) layer in this arithmetic (csrc/wino_x3.hip: channel-maximum pass + input transform with one scale per tile,
 * 16 batched GEMMs, output transform), the f32x3 counterpart of the frcnn_*_winograd_x6 entries:
 *   frcnn_pack_conv3x3_winograd_x3 : d_u_f32 = the float32 bank [16][cout][cin] of frcnn_pack_conv3x3_winograd -> blob of
 *                                    frcnn_conv3x3_winograd_x3_pack_bytes(cout, cin) bytes
 *   frcnn_conv3x3_nhwc_winograd_x3 : the layer; d_ws >= frcnn_conv3x3_winograd_x3_workspace_bytes(n_maps, H, W, cin, cout) */
/* A-side producers for convolutions as f32x3 GEMMs (the f32x3 counterparts of frcnn_split_pixels_x6t / frcnn_split_patches3x3_x6t): the row
 * of an output pixel is scaled by the power of two that the channel maxima of its input pixel(s) give.
 *   frcnn_pixel_absmax           : x [pixels][c] -> d_cmax [pixels] = max_c |x|
 *   frcnn_split_pixels_x3t       : 1x1 convolution, stride 1 / 2: records + d_inv_scale [rows_padded]; d_cmax = NULL: the launch reduces the
 *                                  channel maxima of the rows it needs itself (one launch instead of two, the same bytes)
 *   frcnn_split_patches3x3_x3t   : 3x3 / padding 1, stride 1 / 2 (im2col rows, K = 9 c) */
int frcnn_pixel_absmax(const float* d_x, float* d_cmax, long long pixels, int c, void* stream);
int frcnn_split_pixels_x3t(const float* d_x, const float* d_cmax, void* d_rec, float* d_inv_scale, int n_maps, int H, int W, int c, int stride,
                           int rows_padded, void* stream);
int frcnn_split_patches3x3_x3t(const float* d_x, const float* d_cmax, void* d_rec, float* d_inv_scale, int n_maps, int H, int W, int c,
                               int stride, int rows_padded, void* stream);
size_t frcnn_x3t_blob_bytes(int rows_padded, int K, int batches);
int frcnn_pack_rows_x3t(const float* d_a, int lda, size_t a_batch_floats, void* d_blob, int rows, int rows_padded, int K, int batches,
                        void* stream);
size_t frcnn_conv3x3_winograd_x3_pack_bytes(int cout, int cin);
int frcnn_pack_conv3x3_winograd_x3(const float* d_u_f32, void* d_blob, int cout, int cin, void* stream);
size_t frcnn_conv3x3_winograd_x3_workspace_bytes(int n_maps, int H, int W, int cin, int cout);
int frcnn_conv3x3_nhwc_winograd_x3(const float* d_x, const void* d_blob, const float* d_bias, float* d_y, int n_maps, int H, int W, int cin,
                                   int cout, unsigned flags, void* d_ws, size_t ws_bytes, void* stream);
/* The same layer as ONE launch (csrc/wino_x3f.hip, round 4: 64 tiles x 64 output channels x all 16 positions per block; the operand formed in
 * registers from an LDS-staged halo, the filter fragments loaded straight from L2 into registers, output transform in the epilogue; no
 * V / M scratch), for the layers whose scratch does not fit the Infinity Cache (frcnn_forward_params.winograd_x3f_mask: conv2_2 .. conv3_3
 * of VGG-16; with several images in flight also the 512-channel layers).  The same operands, products and accumulation order as
 * frcnn_conv3x3_nhwc_winograd_x3 on the same blob; the output transform combines columns before rows, so the two forms differ by the
 * float32 rounding of that transform only (<= 2e-6 of max|y|, tests/test_gemm_x3t_gpu.py).  cin % 32 == 0, cout % 64 == 0;
 * d_ws >= frcnn_conv3x3_winograd_x3_fused_workspace_bytes (the channel maxima of the input).  Its eight-wave and two-pass forms were removed
 * in ABI 18 (measurements: DESIGN.md section 5); flag bits other than FRCNN_RELU / FRCNN_POOL2 are ignored. */
size_t frcnn_conv3x3_winograd_x3_fused_workspace_bytes(int n_maps, int H, int W);
int frcnn_conv3x3_nhwc_winograd_x3_fused(const float* d_x, const void* d_blob, const float* d_bias, float* d_y, int n_maps, int H, int W,
                                         int cin, int cout, unsigned flags, void* d_ws, size_t ws_bytes, void* stream);
/* The same two layers CHAINED (round 4): an f32x3 layer takes its scales from the per-pixel channel maximum of its INPUT.  d_cmax_in (optional):
 * those maxima [n_maps][H][W] if a producer already left them -- the layer then does not read its input once more (frcnn_pixel_absmax).
 * d_cmax_out (optional; FRCNN_RELU required, three-launch form: cout % 256 == 0): the channel maxima of the OUTPUT [n_maps][Ho][Wo],
 * accumulated with atomic maxima into a buffer the CALLER ZEROED -- the next layer's d_cmax_in.  Outputs are bit-identical with or
 * without either pointer.  one_launch != 0: csrc/wino_x3f.hip (d_ws as frcnn_conv3x3_nhwc_winograd_x3_fused), else the three-launch form.
 * frcnn_vgg16_forward chains conv2_2 ... conv5_3, the RPN trunk and the RoI pooling this way (11 of 12 channel-maximum passes disappear). */
int frcnn_conv3x3_nhwc_winograd_x3_chain(const float* d_x, const void* d_blob, const float* d_bias, float* d_y, int n_maps, int H, int W, int cin,
                                         int cout, unsigned flags, int one_launch, void* d_ws, size_t ws_bytes, const float* d_cmax_in,
                                         float* d_cmax_out, void* stream);
size_t frcnn_x3t_record_bytes(int rows_padded, int K);
int frcnn_rows_scale_x3t(const float* d_a, int lda, size_t a_batch_floats, float* d_inv_scale, int rows, int rows_padded, int K, int batches,
                         void* stream);
int frcnn_split_rows_x3t(const float* d_a, int lda, size_t a_batch_floats, const float* d_inv_scale, void* d_rec, int rows, int rows_padded,
                         int K, int batches, void* stream);
size_t frcnn_gemm_x3t_workspace_bytes(int M, int N, int K, int batches);
int frcnn_gemm_x3t(const void* d_a_rec, const float* d_a_inv, int a_rows, size_t a_batch_bytes, size_t a_inv_batch_floats,
                   const void* d_b_rec, const float* d_b_inv, int b_rows, size_t b_batch_bytes, size_t b_inv_batch_floats,
                   const float* d_bias, const float* d_residual, float* d_c, int ldc, size_t c_batch_floats, int M, int N, int K,
                   int batches, unsigned flags, void* d_ws, size_t ws_bytes, void* stream);

/* NHWC float32 [N][H][W][C] -> the x6t records of the [N Ho Wo][C] matrix of its pixels taken with `stride` in y and x
 * (Ho = (H - 1) / stride + 1): the A operand of a 1x1 convolution (stride 1 or 2) as a GEMM.  C % 16 == 0. */
int frcnn_split_pixels_x6t(const float* d_x, void* d_rec, int N, int H, int W, int C, int stride, int rows_padded, void* stream);
int frcnn_conv3x3_uses_winograd_x6(int cin, int cout);
size_t frcnn_conv3x3_winograd_x6_pack_bytes(int cout, int cin);
int frcnn_pack_conv3x3_winograd_x6(const float* d_w_oihw, const float* d_row_scale, void* d_u_rec, int cout, int cin, void* stream);
size_t frcnn_conv3x3_winograd_x6_workspace_bytes(int n_maps, int H, int W, int cin, int cout);
int frcnn_conv3x3_nhwc_winograd_x6(const float* d_x, const void* d_u_rec, const float* d_bias, float* d_y, int n_maps, int H, int W, int cin,
                                   int cout, unsigned flags, void* d_ws, size_t ws_bytes, void* stream);
/* NHWC float32 [N][H][W][C] -> the x6t records of the im2col matrix [N Ho Wo][9 C] of a 3x3 convolution with padding 1 and `stride`
 * (Ho = (H - 1) / stride + 1; column index = tap * C + c, tap = 3 r + s; zeros outside the map): the A operand of a strided 3x3
 * convolution as a GEMM against the records of the [cout][9 cin] filter matrix (ResNet layer4.0.conv2).  C % 16 == 0. */
int frcnn_split_patches3x3_x6t(const float* d_x, void* d_rec, int N, int H, int W, int C, int stride, int rows_padded, void* stream);
/* Stand-alone 2x2/stride-2 floor max-pool on NHWC (vgg16.py:78,82,87,92), c % 4 == 0. */
int frcnn_maxpool2x2_nhwc(const float* d_x, float* d_y, int H, int W, int c, void* stream);

/* ------------------------------------------------------------------------------------------
 * ResNet building blocks.  Replace what torchvision.models.resnet{50,101,152} executes under
 * models/resnet.py:33-118 (conv1/bn1/relu/maxpool/layer1-3 as feature extractor, layer4 + spatial
 * mean as the per-RoI head); BatchNorm is always in eval mode there (:58-77,:100-107) and is
 * folded into the preceding convolution at pack time.
 * ---------------------------------------------------------------------------------------- */
/* Fold a frozen BatchNorm2d(gamma, beta, running_mean, running_var, eps) into conv weights
 * OIHW [cout][cin][k][k]: d_w_packed is [k*k][cout][cin] (or [cin*k*k][cout] when cin == 3),
 * d_b_packed [cout]. */
int frcnn_fold_bn_pack(const float* d_w_oihw, const float* d_gamma, const float* d_beta,
                       const float* d_mean, const float* d_var, float eps, int cout, int cin, int ksize,
                       float* d_w_packed, float* d_b_packed, void* stream);
/* Generic NHWC convolution (gather implicit GEMM, f32 MFMA): x [N][H][W][cin] ->
 * y [N][Ho][Wo][cout], square kernel `ksize` (1 or 3), any stride / padding;
 * y = act(conv(x) + bias (+ residual)), residual [N][Ho][Wo][cout] or NULL (Bottleneck's
 * `out += identity`).  cin % 16 == 0, cout % 4 == 0.  d_ws: split-K scratch
 * (frcnn_conv_workspace_bytes; NULL = un-split). */
size_t frcnn_conv_workspace_bytes(int N, int H, int W, int cin, int cout, int ksize, int stride, int pad);
int frcnn_conv_nhwc(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual,
                    float* d_y, int N, int H, int W, int cin, int cout, int ksize, int stride, int pad,
                    unsigned flags, void* d_ws, size_t ws_bytes, void* stream);
/* Stem: 7x7 stride-2 pad-3 conv of the NCHW image [3][H][W] (+folded bn1, ReLU) -> NHWC
 * [(H-1)/2+1][(W-1)/2+1][cout]; d_w_packed [147][cout] from frcnn_fold_bn_pack(cin = 3). */
int frcnn_conv7x7_s2_c3(const float* d_x_chw, const float* d_w_packed, const float* d_bias, float* d_y,
                        int H, int W, int cout, unsigned flags, void* stream);
/* MaxPool2d(3, stride 2, padding 1) on NHWC; output [(H-1)/2+1][(W-1)/2+1][c]. */
int frcnn_maxpool3x3_s2_nhwc(const float* d_x, float* d_y, int H, int W, int c, void* stream);
/* y[n][c] = mean_y(mean_x(x[n][y][x][c]))  (models/resnet.py:117 `.mean(-1).mean(-1)`). */
int frcnn_spatial_mean_nhwc(const float* d_x, float* d_y, int N, int H, int W, int c, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense layers on the f32 MFMA pipe.  Replace nn.Linear (+ReLU) at models/vgg16.py:130-132,
 * models/detector.py:76,78 and the two 1x1 convolutions at models/rpn.py:89-90.
 *   y[m][n] = act( sum_k a[m*lda + k] * w[n*k_dim + k] + bias[n] ),  m < M, n < N
 * w is row-major [n_rows][K] with n_rows >= N rounded up to 128 (extra rows must be readable;
 * frcnn_pack_stack_rows zero-fills them).  K % 16 == 0.  `d_ws` is split-K scratch of at least
 * frcnn_linear_workspace_bytes(M, N, K) bytes (may be NULL if that returns 0).
 * ---------------------------------------------------------------------------------------- */
size_t frcnn_linear_workspace_bytes(int M, int N, int K);
int frcnn_linear(const float* d_a, int lda, const float* d_w, const float* d_bias,
                 float* d_y, int ldy, int M, int N, int K, unsigned flags,
                 void* d_ws, size_t ws_bytes, void* stream);
/* Row softmax over the first `ncls` columns of x[m*ldx ..] -> y[m*ncls ..] (detector.py:77). */
int frcnn_softmax_rows(const float* d_x, int ldx, float* d_y, int M, int ncls, void* stream);

/* ------------------------------------------------------------------------------------------
 * RPN proposal generation.  Replaces models/rpn.py:89 (sigmoid), :98-104 (_extract_valid),
 * :118-123 + models/math_utils.py:99-128 (decode), :129-132 (argsort/flip/top-N),
 * :135-144 (clip, >=16 px filter), :147-153 (torchvision.ops.nms 0.7, first N).
 *
 *   d_head      : float32 [fh*fw][ld_head]; columns 0..8 objectness logits, 9..44 box deltas
 *                 (ty,tx,th,tw per anchor) -- the fused 1x1 head output
 *   d_anchor_map: float32 [fh*fw*9][4];  d_valid_map: float32 [fh*fw*9] or NULL
 *                 (NULL == allow_edge_proposals=True, models/faster_rcnn.py:36)
 * Outputs (device):
 *   d_scores    : float32 [A]       sigmoid objectness per anchor (A = fh*fw*9), reference order
 *   d_sorted_idx: int32   [pre_nms] flat anchor index of the top-N, score-descending; ties are
 *                 broken by HIGHER anchor index first (what stable-ascending argsort + flip gives)
 *   d_props     : float32 [post_nms][4] kept proposals (y1,x1,y2,x2), rows >= *d_n_props zeroed
 *   d_counts    : int32 [4] = { n_candidates (<=pre_nms), n_after_size_filter, n_props, 0 }
 * `ctx` supplies scratch (keys, decoded boxes, NMS mask).  pre_nms <= 16384, post_nms <= 2048.
 * ---------------------------------------------------------------------------------------- */
typedef struct frcnn_ctx frcnn_ctx;

int frcnn_rpn_proposals(frcnn_ctx* ctx, const float* d_head, int ld_head,
                        const float* d_anchor_map, const float* d_valid_map,
                        int fh, int fw, int image_h, int image_w,
                        int pre_nms, int post_nms, float nms_threshold, float min_side,
                        float* d_scores, int32_t* d_sorted_idx, float* d_props, int32_t* d_counts,
                        void* stream);

/* Stand-alone greedy NMS, float32 boxes (any consistent corner order), replaces
 * torchvision.ops.nms as called at models/rpn.py:147-151: scores are sorted stably descending,
 * box j is suppressed by an earlier kept box i iff inter/(area_i+area_j-inter) > threshold.
 * d_keep receives up to max_keep indices into the INPUT order (score-descending), d_n_keep the
 * count.  0 <= n <= 16384 and 1 <= max_keep <= 2048, else FRCNN_EINVAL.  The order is that of a stable
 * argsort(-scores): ties keep the input order, -0.0 ties with +0.0, NaN scores go last (in input order).
 * Boxes of any sign: a box inverted along one axis has a negative area, and a pair whose union is not
 * positive is decided by the division itself, as torchvision does (0 / negative = -0.0: not suppressed). */
int frcnn_nms(frcnn_ctx* ctx, const float* d_boxes, const float* d_scores, int n, float threshold,
              int max_keep, int32_t* d_keep, int32_t* d_n_keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * RoI max pooling.  Replaces torchvision.ops.RoIPool((7,7), 1/16) at models/detector.py:27,72
 * including the (y1,x1,y2,x2)->(x1,y1,x2,y2) column swap at :65-69.
 *   d_fm   : float32 NHWC [fh][fw][c];   d_rois : float32 [max_rois][4] (y1,x1,y2,x2) pixels
 *   d_n_rois: device int32, rows >= *d_n_rois produce zeros
 *   d_out  : float32 [max_rois][pooled][pooled][c]  (NHWC per RoI)
 * ---------------------------------------------------------------------------------------- */
int frcnn_roi_pool(const float* d_fm, int fh, int fw, int c, const float* d_rois,
                   const int32_t* d_n_rois, int max_rois, int pooled, float spatial_scale,
                   float* d_out, void* stream);
/* The same pooling writing fc1's operand in the f32x3 arithmetic directly (csrc/roipool.hip: roi_scale_x3t_kernel, roi_pool_x3t_kernel; what
 * frcnn_vgg16_forward runs with fc_math_mode FRCNN_FC_F32X3T): x3t records of the matrix [rec_rows][pooled * pooled * c], k = (ph * pooled +
 * pw) * c + channel, one power-of-two scale per RoI taken from the maximum of |fm| over the UNION OF THE RoI'S BINS (the bins' own float32
 * floor / ceil edges, which can reach one cell past round(x2 / 16): tests/test_gemm_x3t_gpu.py).
 *   d_cmax : scratch, float32 [fh * fw] (per-cell channel maximum of |fm|, written here);  d_inv_scale : float32 [rec_rows] (2^-e, written)
 *   d_rec  : frcnn_x3t_record_bytes(rec_rows, pooled * pooled * c) bytes;  rec_rows % 32 == 0, >= max_rois;  c % 16 == 0 */
int frcnn_roi_pool_x3t(const float* d_fm, int fh, int fw, int c, const float* d_rois, const int32_t* d_n_rois, int max_rois, int pooled,
                       float spatial_scale, float* d_cmax, float* d_inv_scale, void* d_rec, int rec_rows, void* stream);
/* RoIAlign with torchvision.ops.roi_align's semantics (csrc/roialign.hip) -- the pooling BASELINE.json's north_star names; the
 * reference pools with RoIPool (models/detector.py:16,27), so this is an option beyond it (DetectorNetwork(pooling="align")).
 * Same tensors as frcnn_roi_pool; sampling_ratio = samples per bin and axis (1 or 2; <= 0: adaptive ceil(roi_size / pooled)),
 * aligned = the half-pixel shift of torchvision's `aligned=True`.  float32, the operation order of torchvision's kernel.
 * frcnn_roi_align_backward: d_dfm [fh][fw][c] (+)= gradient of d_dout [n_rois][pooled][pooled][c] with respect to the feature
 * map, gathered per cell in a fixed order (deterministic; torchvision scatters with atomicAdd).  pooled <= 14. */
int frcnn_roi_align(const float* d_fm, int fh, int fw, int c, const float* d_rois, const int32_t* d_n_rois, int max_rois,
                    int pooled, float spatial_scale, int sampling_ratio, int aligned, float* d_out, void* stream);
int frcnn_roi_align_backward(const float* d_rois, int n_rois, int fh, int fw, int c, int pooled, float spatial_scale,
                             int sampling_ratio, int aligned, const float* d_dout, float* d_dfm, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * torchvision.ops-style operators (csrc/ops.hip; Python: fasterrcnn_amd.ops, torch custom ops frcnn::*).  No context; float32 maps
 * (float16 / bfloat16 maps: the frcnn_ops_*_16 entry points below).
 *   d_x    : float32 NHWC [n_img][fh][fw][c] (a channels_last NCHW tensor), c % 4 == 0, c >= 4
 *   d_rois : float32 [k][5] torchvision rows (batch index, x1, y1, x2, y2); a batch index outside (-1, n_img) pools to zeros and
 *            receives no gradient (checked on the device: no host sync)
 *   d_out  : float32 [k][out_h][out_w][c];  1 <= out_h, out_w <= 64;  k >= 0 (k == 0: nothing to do)
 * frcnn_ops_roi_align: torchvision.ops.roi_align, the arithmetic of frcnn_roi_align; sampling_ratio <= 16 (<= 0: adaptive
 *   ceil(roi_size / out)), aligned = the half-pixel shift.
 * frcnn_ops_roi_align_backward: d_dx [n_img][fh][fw][c] = the gradient of d_dout (overwritten, every cell).  A gather per 2 x 2 tile of
 *   cells over the RoIs culled for it, in a fixed order: no atomics, bit-identical from run to run; no cap on out or sampling_ratio.
 * frcnn_ops_roi_pool: torchvision.ops.roi_pool; d_argmax int32 [k][out_h][out_w][c] receives each bin's first maximum in (h, w)
 *   scan order as h * fw + w (-1: empty bin, output 0).
 * frcnn_ops_roi_pool_backward: d_dx = each bin's gradient sent to its d_argmax cell (overwritten; deterministic gather).
 * frcnn_ops_nms: greedy NMS on d_boxes [n][4] (x1, y1, x2, y2), float32 (boxes_f64 = 0) or float64 (1), visited in the order d_order
 *   (int64 [n], a permutation: the stable score-descending sort).  Box j is suppressed by an earlier kept box i iff
 *   inter / (area_i + area_j - inter) > threshold, computed in the boxes' dtype (the threshold a float, as in torchvision's kernel);
 *   boxes of any sign are decided by the division itself (frcnn_nms).  d_categories (int64 [n], optional): batched NMS -- boxes
 *   interact only within a category, and d_order must list each category as one contiguous run; every run is reduced in parallel.
 *   d_keep uint8 [n]: d_keep[s] = 1 iff box d_order[s] is kept.  0 <= n <= 524288; d_ws of frcnn_ops_nms_workspace_bytes(n) bytes
 *   (the n x n / 64 bit mask). */
int frcnn_ops_roi_align(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                        float spatial_scale, int sampling_ratio, int aligned, float* d_out, void* stream);
int frcnn_ops_roi_align_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                 int sampling_ratio, int aligned, const float* d_dout, float* d_dx, void* stream);
/* frcnn_ops_ms_roi_align: torchvision.ops.MultiScaleRoIAlign's pooling (ops/poolers.py: LevelMapper + one roi_align per level,
 *   aligned = False) over n_levels (1..8) maps in ONE launch.  Level l: d_x[l] NHWC [n_img][fh[l]][fw[l]][c] (device pointer in a HOST
 *   array; fh[l] or fw[l] == 0: an empty map, its RoIs pool to zeros), spatial scale scales[l] (host arrays).  A RoI's level is
 *   floor(canonical_level + log2(sqrt(area) * (1 / canonical_scale)) + 1e-6) in float32, clamped to [k_min, k_max] as torch.clamp does
 *   (k_max when k_min > k_max), minus k_min; a NaN level (negative or NaN area) or one outside [0, n_levels) pools to zeros.
 *   n_levels == 1: every RoI is pooled on level 0 and no level is computed.  Each RoI's values are bit-identical to frcnn_ops_roi_align
 *   on its level.  d_out [k][out_h][out_w][c] as frcnn_ops_roi_align.
 * frcnn_ops_ms_roi_align_backward: d_dx[l] (device pointers in a host array) [n_img][fh[l]][fw[l]][c] = level l's gradient (overwritten,
 *   every cell: no zero fill), bit-identical to frcnn_ops_roi_align_backward over the RoIs of level l in ascending order.  Two launches:
 *   one lists the RoIs of every (level, image) in ascending order in d_ws (frcnn_ops_ms_roi_align_workspace_bytes(k, n_levels, n_img)
 *   bytes), then one grid over the 2 x 2 tiles of every level gathers, each tile culling only its (level, image) list.  No atomics. */
int frcnn_ops_ms_roi_align(const float* const* d_x, const int* fh, const int* fw, const float* scales, int n_levels, int n_img, int c,
                           const float* d_rois, int k, int out_h, int out_w, int sampling_ratio, float canonical_scale,
                           float canonical_level, int k_min, int k_max, float* d_out, void* stream);
size_t frcnn_ops_ms_roi_align_workspace_bytes(int k, int n_levels, int n_img);
int frcnn_ops_ms_roi_align_backward(const float* d_rois, int k, const int* fh, const int* fw, const float* scales, int n_levels, int n_img,
                                    int c, int out_h, int out_w, int sampling_ratio, float canonical_scale, float canonical_level,
                                    int k_min, int k_max, const float* d_dout, float* const* d_dx, void* d_ws, size_t ws_bytes,
                                    void* stream);
int frcnn_ops_roi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                       float spatial_scale, float* d_out, int32_t* d_argmax, void* stream);
int frcnn_ops_roi_pool_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                const int32_t* d_argmax, const float* d_dout, float* d_dx, void* stream);
size_t frcnn_ops_nms_workspace_bytes(int n);
int frcnn_ops_nms(const void* d_boxes, int boxes_f64, const int64_t* d_order, const int64_t* d_categories, int n, float iou_threshold,
                  uint8_t* d_keep, void* d_ws, size_t ws_bytes, void* stream);

/* The RoI operators on 16-bit maps (ABI 21): float16 or bfloat16 d_x / d_out / d_dout / d_dx (elem_type, one for the whole call), in the
 *   layouts of their float32 siblings above; d_rois and the level arithmetic stay float32, d_argmax int32.  Values are widened exactly
 *   on load, every weight and sum is float32 in the float32 kernels' order (one shared body), and the result is rounded once, to nearest
 *   even as torch's Tensor.to() rounds (bfloat16: every NaN becomes 0x7FC0), on store:
 *       op_16(x) == op(float(x)) rounded,   op_backward_16(dout) == op_backward(float(dout)) rounded,   bit for bit
 *   (torchvision's autocast definition); the backward sums live in registers over every culling pass, never in the 16-bit d_dx.
 *   c % frcnn_ops_half_run() == 0 (8: the 16-bit channels a lane loads at once, 16 bytes; the backward gathers walk the same tensors in
 *   runs of 4 while c / 8 would not fill a wave, c < 512).  Arguments are validated as by the float32
 *   entry points; an unknown elem_type is FRCNN_EINVAL.  The multi-scale workspace is frcnn_ops_ms_roi_align_workspace_bytes's. */
#define FRCNN_OPS_F16  1   /* IEEE binary16 (torch.float16) */
#define FRCNN_OPS_BF16 2   /* bfloat16 (torch.bfloat16) */
#define FRCNN_OPS_F32  0   /* float32: only where one entry point serves all three element types (frcnn_ops_masked_conv2d, frcnn_ops_paste_masks_*,
                              frcnn_ops_heatmaps_to_keypoints) */
int frcnn_ops_half_run(void);
int frcnn_ops_roi_align_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                           int out_w, float spatial_scale, int sampling_ratio, int aligned, void* d_out, void* stream);
int frcnn_ops_roi_align_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                    float spatial_scale, int sampling_ratio, int aligned, const void* d_dout, void* d_dx, void* stream);
int frcnn_ops_roi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                          int out_w, float spatial_scale, void* d_out, int32_t* d_argmax, void* stream);
int frcnn_ops_roi_pool_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                   float spatial_scale, const int32_t* d_argmax, const void* d_dout, void* d_dx, void* stream);
int frcnn_ops_ms_roi_align_16(int elem_type, const void* const* d_x, const int* fh, const int* fw, const float* scales, int n_levels,
                              int n_img, int c, const float* d_rois, int k, int out_h, int out_w, int sampling_ratio,
                              float canonical_scale, float canonical_level, int k_min, int k_max, void* d_out, void* stream);
int frcnn_ops_ms_roi_align_backward_16(int elem_type, const float* d_rois, int k, const int* fh, const int* fw, const float* scales,
                                       int n_levels, int n_img, int c, int out_h, int out_w, int sampling_ratio, float canonical_scale,
                                       float canonical_level, int k_min, int k_max, const void* d_dout, void* const* d_dx, void* d_ws,
                                       size_t ws_bytes, void* stream);

/* Position-sensitive RoI pooling (R-FCN; csrc/ops_ps.hip): torchvision.ops.ps_roi_pool and ps_roi_align, restated from the published
 *   algorithm of torchvision/csrc/ops/cuda/ps_roi_pool_kernel.cu and ps_roi_align_kernel.cu (third party, absent here: restated,
 *   unpinned, like nms / roi_align).  Unlike the operators above these read and write plain NCHW, with no layout copy:
 *     d_x    : [n_img][c][fh][fw], c % (out_h * out_w) == 0, c >= out_h * out_w
 *     d_out  : [k][c / (out_h * out_w)][out_h][out_w]; output channel co of bin (ph, pw) pools input plane (co * out_h + ph) * out_w + pw
 *     d_rois, out_h, out_w, k, sampling_ratio: as above (a batch index outside (-1, n_img) pools to zeros and receives no gradient)
 *   All arithmetic is float32.
 * frcnn_ops_ps_roi_pool: start = roundf(coord * scale), end = roundf((coord + 1) * scale), integer size max(end - start, 1); bin p covers
 *   [floor(p * bin), ceil((p + 1) * bin)) + start with every bound clamped to [0, size - 1] (torchvision's clamp for this operator); the
 *   output is the (h, w) scan-order sum of the window divided by its area, 0 for an empty window.
 * frcnn_ops_ps_roi_align: always aligned (coord * scale - 0.5), size = end - start unclamped, grid = sampling_ratio > 0 ? sampling_ratio
 *   : ceil(size / out), count = grid_h * grid_w with no lower bound: samples and bilinear_interpolate are frcnn_ops_roi_align's (one
 *   shared body), out = sum / count -- so an adaptive grid on a RoI of no height or width gives 0.0f / count (NaN for count == 0).
 * The backwards overwrite every element of d_dx [n_img][c][fh][fw] (no zero fill).  Deterministic gathers, no atomics: one thread per
 *   element of d_dx visits, in ascending order, the RoIs of its image whose bin (ph, pw) of its plane reaches it (each block first
 *   lists those bins' windows in LDS), so the result is bit-identical from run to run.  ps_roi_pool sends dout / area to every cell of
 *   a non-empty window; ps_roi_align sends dout * (the cell's summed sample weight) / count.
 * The _16 forms take float16 / bfloat16 d_x / d_out / d_dout / d_dx under the contract of the 16-bit operators above (widened exactly on
 *   load, float32 sums in registers, one rounding to nearest even on store); any c that the float32 forms take. */
int frcnn_ops_ps_roi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                          float spatial_scale, float* d_out, void* stream);
int frcnn_ops_ps_roi_pool_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                   const float* d_dout, float* d_dx, void* stream);
int frcnn_ops_ps_roi_align(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                           float spatial_scale, int sampling_ratio, float* d_out, void* stream);
int frcnn_ops_ps_roi_align_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                    int sampling_ratio, const float* d_dout, float* d_dx, void* stream);
int frcnn_ops_ps_roi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                             int out_w, float spatial_scale, void* d_out, void* stream);
int frcnn_ops_ps_roi_pool_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                      float spatial_scale, const void* d_dout, void* d_dx, void* stream);
int frcnn_ops_ps_roi_align_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                              int out_w, float spatial_scale, int sampling_ratio, void* d_out, void* stream);
int frcnn_ops_ps_roi_align_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                       float spatial_scale, int sampling_ratio, const void* d_dout, void* d_dx, void* stream);

/* Deformable convolution v1 / v2 (csrc/ops_deform.hip): torchvision.ops.deform_conv2d in both directions, restated from the published
 *   algorithm of torchvision/csrc/ops/cuda/deform_conv2d_kernel.cu (third party, absent here: restated, unpinned).  Float32 (the _16
 *   forms below: float16 / bfloat16), plain NCHW;
 *   every entry point works on one chunk of n_img images (the caller walks the chunks and owns every buffer):
 *     d_x      : [n_img][c_in][height][width]
 *     d_weight : [c_out][c_in / groups][kernel_h][kernel_w]
 *     d_offset : [n_img][2 * offset_groups * kh * kw][oh][ow]: channel 2 * (g * kh * kw + i * kw + j) is the y displacement of tap
 *                (i, j) of offset group g, the next channel its x displacement
 *     d_mask   : [n_img][offset_groups * kh * kw][oh][ow] or NULL (v1: a mask of ones)
 *     d_out    : [n_img][c_out][oh][ow], oh = (height + 2 pad_h - (dilation_h (kh - 1) + 1)) / stride_h + 1, likewise ow
 *   A sample at y = oy stride_h - pad_h + i dilation_h + off_y (likewise x) is 0 when y <= -1, y >= height, x <= -1 or x >= width (or
 *   NaN), else the bilinear value on floor / floor + 1 with the weights hh hw, hh lw, lh hw, lh lw, a corner outside the map counting 0;
 *   the column value is mask * sample and out = bias + sum over the weight group's (c, i, j) of weight * column.
 *   With P = oh * ow and Pp = P rounded up to a multiple of 4, the column matrix is [c_in * kh * kw][n_img * Pp] floats
 *   (frcnn_ops_deform_workspace_bytes(.., FRCNN_DEFORM_WS_COLUMNS)); the products run on the exact-float32 kernel of frcnn_gemm_tn.
 *   Every function validates its arguments before touching the GPU (FRCNN_EINVAL: a NULL geometry, sizes < 1, channels not divisible
 *   by groups / offset_groups, an empty output, an index beyond 32 bits, a NULL or misaligned pointer, a workspace that is too small);
 *   workspaces and d_dcol are 16-byte aligned.  Nothing allocates.
 * frcnn_ops_deform_forward: d_bias [c_out] or NULL.  The product is not split, so an output element does not depend on the chunking.
 * frcnn_ops_deform_backward_columns: d_dcol = W^T dout in the column layout (d_dout: [n_img][c_out][oh][ow]).
 * frcnn_ops_deform_backward_offset: d_doffset and / or d_dmask (either may be NULL, not both) by a gather over the channels of the
 *   offset group: (mask * coordinate_weight) * dcol for y and x -- torchvision's get_coordinate_weight: the difference of the validly
 *   indexed corner values, weighted by the other axis's fractions, without an early-out -- and dcol * sample for the mask.
 * frcnn_ops_deform_input_plan + frcnn_ops_deform_backward_input: the input gradient without atomics.  The plan writes one entry per
 *   sample and corner, e = (((b G + g) kh kw + tap) P + p) * 4 + corner (n_img * G * kh * kw * P * 4 entries): d_keys[e] = the cell
 *   ((b G + g) height + y) width + x, or n_img * G * height * width for a corner outside the map or a rejected sample, and
 *   d_weights[e] = corner weight * mask.  The caller sorts the keys stably; d_sorted_keys and d_order (the sort's permutation) come
 *   back, and every element of d_dx [n_img][c_in][height][width] is written as the sum, in ascending e, of
 *   d_weights[e] * dcol over the entries of its cell: bit-identical from run to run.
 * frcnn_ops_deform_backward_weight: d_dweight (= or, with accumulate != 0, +=) dout col^T per group, the columns sampled again;
 *   deterministic split reduction inside the chunk. */
typedef struct frcnn_deform_geom {
    int32_t c_in, height, width, c_out, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups,
            offset_groups;
} frcnn_deform_geom;
#define FRCNN_DEFORM_WS_FORWARD          0
#define FRCNN_DEFORM_WS_BACKWARD_COLUMNS 1
#define FRCNN_DEFORM_WS_BACKWARD_INPUT   2
#define FRCNN_DEFORM_WS_BACKWARD_WEIGHT  3
#define FRCNN_DEFORM_WS_COLUMNS          4   /* not a workspace: the bytes of the column matrix d_dcol itself */
size_t frcnn_ops_deform_workspace_bytes(const frcnn_deform_geom* g, int n_img, int stage);   /* 0 for a bad geometry or stage */
int frcnn_ops_deform_forward(const frcnn_deform_geom* g, int n_img, const float* d_x, const float* d_offset, const float* d_mask,
                             const float* d_weight, const float* d_bias, float* d_out, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_deform_backward_columns(const frcnn_deform_geom* g, int n_img, const float* d_weight, const float* d_dout, float* d_dcol,
                                      void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_deform_backward_offset(const frcnn_deform_geom* g, int n_img, const float* d_x, const float* d_offset, const float* d_mask,
                                     const float* d_dcol, float* d_doffset, float* d_dmask, void* stream);
int frcnn_ops_deform_input_plan(const frcnn_deform_geom* g, int n_img, const float* d_offset, const float* d_mask, int64_t* d_keys,
                                float* d_weights, void* stream);
int frcnn_ops_deform_backward_input(const frcnn_deform_geom* g, int n_img, const int64_t* d_sorted_keys, const int64_t* d_order,
                                    const float* d_weights, const float* d_dcol, float* d_dx, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_deform_backward_weight(const frcnn_deform_geom* g, int n_img, const float* d_x, const float* d_offset, const float* d_mask,
                                     const float* d_dout, float* d_dweight, int accumulate, void* d_ws, size_t ws_bytes, void* stream);

/* The same operator on float16 / bfloat16 tensors (elem_type: FRCNN_OPS_F16 / FRCNN_OPS_BF16; T below): every tensor of the float32
 *   forms above is of type T here, in the same layouts, EXCEPT d_dcol, the plan's d_weights and d_dweight, which stay float32.  The
 *   validation rules are the float32 forms', plus FRCNN_EINVAL (0 from _workspace_bytes_16) for an unknown elem_type.  Nothing allocates.
 *   Arithmetic contract:
 *   columns   input, offset and mask are widened to float32 on read (exact); the sample coordinate, the bilinear value and
 *             mask * sample are computed in float32 by the device functions of the float32 kernels (csrc/ops_deform.h); the column
 *             value is rounded ONCE to T, to nearest even: bit for bit the float32 operator's column of the widened tensors, rounded.
 *   forward   out = round_T(sum_k w col + float(bias)): the products w * col of two T values are exact in float32, the sum runs in
 *             float32 accumulators on v_mfma_f32_32x32x16_{f16,bf16} (csrc/gemm_nt16.hip) without a split reduction, so an output
 *             element does not depend on the chunking; the bias is added in float32 and the result rounded once.  A float16 result
 *             beyond 65504 is inf, as for any half convolution.
 *   backward  d_dcol = W^T dout on the same kernel, without a split, kept in float32 (the accumulators as they are), in the column
 *             layout with Pp = P rounded up to a multiple of 8: [c_in * kh * kw][n_img * Pp] floats (.._workspace_bytes_16(..,
 *             FRCNN_DEFORM_WS_COLUMNS)).  d_doffset, d_dmask and d_dx are the float32 forms' gathers: they read T input, offset and
 *             mask and the float32 d_dcol, sum in float32 in the same order (d_dx through the same plan, stable sort and ascending
 *             sum) and round once to T on the store; they do not depend on the chunking.
 *             frcnn_ops_deform_backward_weight_16: the columns are sampled again to T (the forward's values), dout col^T runs on the
 *             same kernel with a deterministic split reduction over the chunk's outputs (float32 planes added in ascending order), and
 *             d_dweight is a FLOAT32 [c_out][c_in / groups][kh][kw] buffer (= or, with accumulate != 0, +=): the caller adds the
 *             chunks in ascending order in float32 and rounds to T once after the last one; the chunks are never accumulated in T.
 *   Everything is deterministic and free of atomics. */
size_t frcnn_ops_deform_workspace_bytes_16(int elem_type, const frcnn_deform_geom* g, int n_img, int stage);
int frcnn_ops_deform_forward_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_x, const void* d_offset,
                                const void* d_mask, const void* d_weight, const void* d_bias, void* d_out, void* d_ws, size_t ws_bytes,
                                void* stream);
int frcnn_ops_deform_backward_columns_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_weight, const void* d_dout,
                                         float* d_dcol, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_deform_backward_offset_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_x, const void* d_offset,
                                        const void* d_mask, const float* d_dcol, void* d_doffset, void* d_dmask, void* stream);
int frcnn_ops_deform_input_plan_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_offset, const void* d_mask,
                                   int64_t* d_keys, float* d_weights, void* stream);
int frcnn_ops_deform_backward_input_16(int elem_type, const frcnn_deform_geom* g, int n_img, const int64_t* d_sorted_keys,
                                       const int64_t* d_order, const float* d_weights, const float* d_dcol, void* d_dx, void* d_ws,
                                       size_t ws_bytes, void* stream);
int frcnn_ops_deform_backward_weight_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_x, const void* d_offset,
                                        const void* d_mask, const void* d_dout, float* d_dweight, int accumulate, void* d_ws,
                                        size_t ws_bytes, void* stream);

/* Deformable RoI pooling (DCN v1 / v2; csrc/ops_droi.hip): mmcv's deform_roi_pool in both directions, restated from the published
 *   definition of mmcv/ops/csrc/common/cuda/deform_roi_pool_cuda_kernel.cuh (third party, absent here: restated, unpinned; where the two
 *   differ this text holds).  Layouts and element types as frcnn_ops_roi_align above (NHWC maps, c % 4 == 0; the _16 forms c % 8 == 0):
 *     d_x      : [n_img][fh][fw][c]
 *     d_rois   : [k][5] rows (b, x1, y1, x2, y2); a batch index outside (-1, n_img) pools to zeros and sends and receives no gradient
 *     d_offset : float32 [k][2][out_h][out_w], channel 0 the x (width) offset, channel 1 the y offset; NULL: no offset
 *     d_out    : [k][out_h][out_w][c]
 *   Bin (ph, pw) of a RoI is frcnn_ops_roi_align(aligned = 1)'s bin -- start = coord * scale - 0.5, size = end - start with no lower
 *   bound, bin = size / out, grid = sampling_ratio > 0 ? sampling_ratio : ceil(size / out), count = max(grid_h * grid_w, 1) -- with its
 *   window shifted: start_w += gamma * roi_w * offset[k][0][ph][pw], start_h += gamma * roi_h * offset[k][1][ph][pw]; bin and grid are
 *   unchanged.  out = (1 / count) * sum over iy (outer), ix (inner) of the bilinear sample, roi_align's expressions in roi_align's order:
 *   with a NULL or all-zero offset and finite RoIs the output is frcnn_ops_roi_align(aligned = 1) bit for bit.  A sample outside
 *   [-1, size] on either axis, or at a NaN or infinite coordinate (rejected before any conversion to an integer), contributes nothing.
 * frcnn_ops_deform_roi_pool_backward: with g = dout / count per accepted sample at (y, x), corners (yl, yh, xl, xh), weights w1..w4:
 *   d_dx (NULL: skipped; else every element overwritten) gets g w1 at (yl, xl), g w2 at (yl, xh), g w3 at (yh, xl), g w4 at (yh, xh);
 *   d_doffset (NULL: skipped; float32 [k][2][out_h][out_w], needs d_offset and d_x) gets
 *     [0] += gamma roi_w g (v(yh,xh) (y - yl) + v(yl,xh) (yh - y) + v(yh,xl) (yl - y) + v(yl,xl) (y - yh))
 *     [1] += gamma roi_h g (v(yh,xh) (x - xl) + v(yh,xl) (xh - x) + v(yl,xh) (xl - x) + v(yl,xl) (x - xh))
 *   summed over the channels, with y and x as computed, before the clamp of the bilinear weights (the published formula: the exact
 *   derivative in the interior, deliberately not in the clamped bands (-1, 0] and [size - 1, size]).  Both are deterministic and free of
 *   atomics: d_doffset by one wave per (RoI, bin) with a fixed cross-lane reduction; d_dx by a plan launch (per bin the shifted start
 *   and the window of cells its samples can touch, per RoI their union) and a gather per 2 x 2 tile that culls RoIs in ascending order,
 *   frcnn_ops_deform_roi_pool_cull_list() at a time, and sums in ascending (RoI, ph, pw) order into registers, stored once.  d_ws:
 *   frcnn_ops_deform_roi_pool_workspace_bytes(k, out_h, out_w) bytes, 16-byte aligned, needed with d_dx only (0: invalid sizes).
 *   At least one of d_dx and d_doffset is given.  k == 0 returns FRCNN_OK after zero-filling d_dx.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): out_h, out_w in [1, 64], sampling_ratio <= 16, k >= 0, sizes < 1,
 *   c not in whole runs, k * out_h * out_w or fh * fw beyond 32 bits, fh > 131070 or n_img * ceil(c / run / 64) > 65535 (the gather's
 *   launch grid), NULL pointers, a small workspace.
 * The _16 forms take float16 / bfloat16 d_x / d_out / d_dout / d_dx under the contract of the 16-bit operators above; offsets and
 *   d_doffset stay float32. */
int frcnn_ops_deform_roi_pool_cull_list(void);
size_t frcnn_ops_deform_roi_pool_workspace_bytes(int k, int out_h, int out_w);
int frcnn_ops_deform_roi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, const float* d_offset, int k,
                              int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma, float* d_out, void* stream);
int frcnn_ops_deform_roi_pool_backward(const float* d_x, const float* d_rois, const float* d_offset, int k, int n_img, int fh, int fw,
                                       int c, int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma,
                                       const float* d_dout, float* d_dx, float* d_doffset, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_deform_roi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois,
                                 const float* d_offset, int k, int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma,
                                 void* d_out, void* stream);
int frcnn_ops_deform_roi_pool_backward_16(int elem_type, const void* d_x, const float* d_rois, const float* d_offset, int k, int n_img,
                                          int fh, int fw, int c, int out_h, int out_w, float spatial_scale, int sampling_ratio,
                                          float gamma, const void* d_dout, void* d_dx, float* d_doffset, void* d_ws, size_t ws_bytes,
                                          void* stream);

/* Precise RoI Pooling (PrRoIPool of IoU-Net; csrc/ops_prroi.hip): mmcv's prroi_pool in both directions, with the gradient for the boxes,
 *   restated from the published definition (third party, absent here: restated, unpinned; where the two differ this text holds).
 *   Layouts and element types as frcnn_ops_roi_align above (NHWC maps, c % 4 == 0; the _16 forms c % 8 == 0):
 *     d_x    : [n_img][fh][fw][c]
 *     d_rois : float32 [k][5] rows (b, x1, y1, x2, y2)
 *     d_out  : [k][out_h][out_w][c]
 *   The map of image b, channel c is extended to the surface f(x, y) = sum over j, i of hat(y - j) hat(x - i) x[b][j][i][c] with
 *   hat(t) = max(0, 1 - |t|): cell (j, i) sits at the integer point (i, j), no half-pixel shift, zero beyond one cell outside the map.
 *   In float32: X1 = x1 * scale (likewise Y1, X2, Y2), rw = max(X2 - X1, 0), rh = max(Y2 - Y1, 0), bw = rw / out_w, bh = rh / out_h,
 *   A = bw * bh; bin (ph, pw): xs = X1 + pw * bw, xe = xs + bw, ys = Y1 + ph * bh, ye = ys + bh, and
 *     out[k][ph][pw][c] = (sum over j, i of Wy(j) Wx(i) x[b][j][i][c]) / A,   Wx(i) = the integral of hat(x - i) over [xs, xe],
 *   Wx(i) formed on the unit pieces [i - 1, i] and [i, i + 1] cut to [xs, xe]: a piece [p, q] with q > p and m = (p + q) / 2 gives
 *   (q - p) (m - i + 1) on the rising side, (q - p) (1 - (m - i)) on the falling side (never a difference of antiderivatives, which
 *   cancels for a bin much narrower than a cell); Wy(j) likewise with ys, ye.
 *   A RoI is pooled iff 0 < A < +inf and its batch index lies in (-1, n_img); any other -- no or negative width or height, a NaN or
 *   infinite coordinate, an area that overflows -- pools to exact zeros and sends and receives no gradient.  A pooled RoI has finite bin
 *   edges; every cell range is clamped to the map in float before it is converted: the kernels are memory-safe for any box.
 * frcnn_ops_prroi_pool_backward:
 *   d_dx (NULL: skipped; else every element overwritten) = sum over the RoIs of image b and their bins of dout Wy(j) Wx(i) / A: a gather
 *   per 2 x 2 tile that culls the RoIs in ascending order, frcnn_ops_prroi_pool_cull_list() at a time (a RoI is listed if its scaled box,
 *   grown by one cell and rounded outwards, meets the tile), sums in ascending (RoI, ph, pw) order into registers and stores once.
 *   d_drois (NULL: skipped; float32 [k][5], needs d_x and d_ws) is the analytic derivative.  With
 *   Lx(t) = sum_j Wy(j) sum_i hat(t - i) x[j][i] and Ly(t) = sum_i Wx(i) sum_j hat(t - j) x[j][i], per bin and channel:
 *     d out / d xs = (-Lx(xs) + out bh) / A,  d out / d xe = (Lx(xe) - out bh) / A,  d out / d ys = (-Ly(ys) + out bw) / A,
 *     d out / d ye = (Ly(ye) - out bw) / A;  d xs / d X1 = 1 - pw / out_w, d xs / d X2 = pw / out_w, d xe / d X1 = 1 - (pw + 1) / out_w,
 *     d xe / d X2 = (pw + 1) / out_w, the same in y; d_drois[k][1..4] = scale * (dX1, dY1, dX2, dY2), d_drois[k][0] = 0.
 *   It is recomputed from d_x (the saved output is not read: a 16-bit output has been rounded): one wave per (RoI, bin) sums dout times
 *   the five integrals over its channels in runs of 4 whatever the element type, with a fixed cross-lane reduction, into d_ws
 *   (frcnn_ops_prroi_pool_workspace_bytes(k, out_h, out_w) bytes, 16-byte aligned; 0: invalid sizes); one wave per RoI then sums the bins
 *   in a fixed order.  Both gradients are deterministic and free of atomics.  At least one of d_dx and d_drois is given.  k == 0 returns
 *   FRCNN_OK after zero-filling d_dx.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): out_h, out_w in [1, 64], k >= 0, sizes < 1, c not in whole runs,
 *   k * out_h * out_w or fh * fw beyond 32 bits, fh > 131070 or n_img * ceil(c / run / 64) > 65535 (the gather's launch grid), NULL
 *   pointers, a small or misaligned workspace.
 * The _16 forms take float16 / bfloat16 d_x / d_out / d_dout / d_dx under the contract of the 16-bit operators above; RoIs and d_drois
 *   stay float32, and d_drois of a 16-bit map equals that of the widened map bit for bit. */
int frcnn_ops_prroi_pool_cull_list(void);
size_t frcnn_ops_prroi_pool_workspace_bytes(int k, int out_h, int out_w);
int frcnn_ops_prroi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                         float spatial_scale, float* d_out, void* stream);
int frcnn_ops_prroi_pool_backward(const float* d_x, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                  float spatial_scale, const float* d_dout, float* d_dx, float* d_drois, void* d_ws, size_t ws_bytes,
                                  void* stream);
int frcnn_ops_prroi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                            int out_w, float spatial_scale, void* d_out, void* stream);
int frcnn_ops_prroi_pool_backward_16(int elem_type, const void* d_x, const float* d_rois, int k, int n_img, int fh, int fw, int c,
                                     int out_h, int out_w, float spatial_scale, const void* d_dout, void* d_dx, float* d_drois, void* d_ws,
                                     size_t ws_bytes, void* stream);

/* BorderAlign, the border pooling of BorderDet (csrc/ops_border.hip): mmcv's border_align in both directions, restated from the published
 *   definition (third party, absent here: restated, unpinned; where the two differ this text holds).
 *   Layouts (element types as frcnn_ops_roi_align above; c = the channels of ONE edge group, c % 4 == 0, the _16 forms c % 8 == 0):
 *     d_x      : [n_img][fh][fw][4 c], group e in channels [e c, (e + 1) c): e = 0 top, 1 left, 2 bottom, 3 right
 *     d_boxes  : float32 [n_img][k][4] rows (x1, y1, x2, y2) in map coordinates; box r of image b pools image b
 *     d_out    : [n_img][k][4][c];  d_argmax : int32 [n_img][k][4][c];  d_dout as d_out, d_dx as d_x
 *   The contract.  All arithmetic is float32, every operation rounded on its own.  With P = pool_size, edge e of a box starts at
 *   (x0, y0) and steps by (dx, dy):
 *     e = 0 top    : (x1, y1), s = (x2 - x1) / P, ( s, 0)        e = 1 left  : (x1, y1), s = (y2 - y1) / P, (0,  s)
 *     e = 2 bottom : (x2, y2), s = (x2 - x1) / P, (-s, 0)        e = 3 right : (x2, y2), s = (y2 - y1) / P, (0, -s)
 *   Sample i = 0 .. P lies at (x0 + (float)i * dx, y0 + (float)i * dy): the product is formed first, then one add, in the forward and in
 *   the backward, so the backward lands on the forward's sample exactly (mmcv accumulates x += stride forwards and multiplies backwards).
 *   A sample counts iff -1 <= y <= fh and -1 <= x <= fw; its value is then the bilinear one of frcnn_ops_roi_align: a coordinate <= 0
 *   goes to 0, low = (int)v, a low index >= size - 1 collapses to the last cell (low = high = size - 1, v = low), weights 1 - (v - low)
 *   and v - low, and value = ((w1 v1 + w2 v2) + w3 v3) + w4 v4 over (y low, x low), (y low, x high), (y high, x low), (y high, x high)
 *   with w = wy * wx.  Any other sample, a NaN coordinate included, is exactly 0 and receives no gradient.  No box is rejected as a
 *   whole: inverted and empty boxes are simply sampled (a zero stride makes every sample the same point) and non-finite coordinates
 *   fall under the sample rule.  No coordinate is converted to int before it has passed the range test.
 *   d_out[b][r][e][ch] = the maximum over i of the samples of channel e c + ch, found as best = sample 0, then for i = 1 .. P:
 *   if (val > best) take val and i.  So ties go to the smallest i, a NaN sample never replaces the running value, and a NaN at i = 0
 *   stays.  d_argmax holds the winning i.  Every element of both is written.
 * frcnn_ops_border_align_backward: d_dx (every element overwritten) gets, for every (b, r, e, ch), d_dout times the four bilinear weights
 *   of sample d_argmax[b][r][e][ch] on its four cells (a collapsed pair adds both weights to the one cell); a sample outside the range
 *   sends nothing, whatever the argmax holds.  A gather per 2 x 2 tile and 64 channel runs, one wave per edge group: the wave tests the
 *   boxes of its image frcnn_ops_border_align_cull_list() = 64 at a time, one per lane (a box is taken for edge e when that edge's
 *   segment, sample 0 to sample P, grown by one cell and rounded outwards, meets the tile) and walks the ballot's bits from the lowest;
 *   each lane re-derives its channels' samples from their argmax and adds, in ascending box order over all groups, into the registers of
 *   the tile's four cells, one store each.  Deterministic, no atomics.  k == 0 returns FRCNN_OK after
 *   zero-filling d_dx.  d_boxes gets no gradient.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): pool_size outside [1, 64], k < 0, sizes < 1, fh or fw > 2^24
 *   (coordinates up to the map's size are exact in float32), c not in whole runs, fh * fw beyond 32 bits, the flat launch grids
 *   n_img k 4 (c / run) lanes (forward) or n_img ceil(c / run / 64) ceil(fh / 2) ceil(fw / 2) blocks (backward) above 2^31 - 1 - 1024,
 *   NULL pointers.
 * The _16 forms take float16 / bfloat16 d_x / d_out / d_dout / d_dx under the contract of the 16-bit operators above; the boxes stay
 *   float32 and the argmax is that of the widened map. */
int frcnn_ops_border_align_cull_list(void);
int frcnn_ops_border_align(const float* d_x, int n_img, int fh, int fw, int c, const float* d_boxes, int k, int pool_size, float* d_out,
                           int* d_argmax, void* stream);
int frcnn_ops_border_align_backward(const float* d_boxes, int k, int n_img, int fh, int fw, int c, int pool_size, const int* d_argmax,
                                    const float* d_dout, float* d_dx, void* stream);
int frcnn_ops_border_align_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_boxes, int k,
                              int pool_size, void* d_out, int* d_argmax, void* stream);
int frcnn_ops_border_align_backward_16(int elem_type, const float* d_boxes, int k, int n_img, int fh, int fw, int c, int pool_size,
                                       const int* d_argmax, const void* d_dout, void* d_dx, void* stream);

/* Rotated boxes (oriented detection; csrc/ops_rot.hip): mmcv's box_iou_rotated, nms_rotated and roi_align_rotated, restated from their
 *   published definitions (third party, absent here: restated, unpinned; where the two differ this text holds).
 * Box: float32 (cx, cy, w, h, angle), angle in radians.  A local point (u, v) of the box, |u| <= w / 2, |v| <= h / 2, lies at the image
 *   point (cx + u cos a - v sin a, cy + u sin a + v cos a): mmcv's clockwise = True.  The kernels know this one convention; for the
 *   other the caller negates the angles.
 * IoU: inter = the area of the intersection of the two rectangles; mode 0 (iou): inter / (w1 h1 + w2 h2 - inter), mode 1 (iof):
 *   inter / (w1 h1).  A pair gives exactly 0 if either box has w h < 1e-14, a negative w or h, or a non-finite component.  Computed in
 *   float32: the centre difference first, box 1's corners in box 2's frame, clipped against box 2's four half-planes (Sutherland-Hodgman),
 *   the area as a fan of triangles.  A box against itself gives exactly 1.
 * frcnn_ops_box_iou_rotated: d_out [n][m] = IoU(d_boxes1[i], d_boxes2[j]), or with aligned != 0 (n == m required) d_out [n] =
 *   IoU(d_boxes1[i], d_boxes2[i]), bit-identical to the diagonal of the full matrix.  n or m == 0 returns FRCNN_OK.  n <= 4194240.
 * frcnn_ops_nms_rotated: frcnn_ops_nms on rotated boxes d_boxes [n][5]: the same order / categories / keep / workspace arguments
 *   (frcnn_ops_nms_workspace_bytes(n)), the same bit mask and the same greedy pass; sorted box j goes iff a kept box i before it, of
 *   the same category, has IoU(box i, box j) > iou_threshold, with the IoU, and the argument order, of frcnn_ops_box_iou_rotated.
 * frcnn_ops_roi_align_rotated: RoIAlign on a rotated sampling grid.  d_x [n_img][fh][fw][c], d_out [k][out_h][out_w][c] and the limits
 *   as frcnn_ops_roi_align; d_rois [k][6] rows (b, cx, cy, w, h, angle), a batch index outside (-1, n_img) pools to zeros and gets no
 *   gradient.  off = aligned ? 0.5 : 0; centre = (cx, cy) * scale - off; rw = w * scale, rh = h * scale, each raised to >= 1 only when
 *   !aligned; bins rh / out_h x rw / out_w; grid = sampling_ratio > 0 ? sampling_ratio : ceil(rh / out_h) (likewise w; 0 for a size that
 *   is not positive, NaN or gives more than 2^30 samples per bin); count = max(grid_h * grid_w, 1); t = clockwise ? -angle : angle.
 *   Sample (ph, iy, pw, ix) has local yy = -rh / 2 + ph * bin_h + (iy + .5) * bin_h / grid_h, xx likewise, and lies at
 *   x = yy sin t + xx cos t + centre_x, y = yy cos t - xx sin t + centre_y: clockwise != 0 agrees with the box convention above.  Its
 *   value is frcnn_ops_roi_align's bilinear rule; nothing outside [-1, size] on either axis or at a NaN coordinate.  The output is the
 *   sum over iy (outer), ix (inner) divided by count.
 * frcnn_ops_roi_align_rotated_backward: d_dx [n_img][fh][fw][c], every element overwritten (k == 0: zeros).  Deterministic, no atomics:
 *   a gather per 2 x 2 cell tile that culls RoIs in ascending order, frcnn_ops_roi_align_rotated_cull_list() at a time, against the
 *   rotated RoI's bounding box grown by two pixels; per cell and listed RoI the candidate samples are bounded analytically (a rotation
 *   is an isometry: a touching sample lies within sqrt(2) of the cell on both local axes) and each is tested exactly with the forward's
 *   expressions.  The sum runs over RoIs ascending, then bins (ph, pw) ascending, each bin sending dout * (the sum of its samples' weights
 *   in (iy, ix) order) / count; it stays in registers and is stored once.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): frcnn_ops_roi_align's limits, fh <= 131070, NULL pointers, mode
 *   outside {0, 1}, aligned with n != m, n beyond the limits, a small workspace.
 * The _16 forms take float16 / bfloat16 d_x / d_out / d_dout / d_dx under the contract of the 16-bit operators above; RoIs stay float32.
 * frcnn_ops_diff_iou_rotated: the differentiable IoU of n aligned pairs (mmcv's diff_iou_rotated_2d; mmcv builds it from 24 candidate
 *   points and a sorted hull with epsilons, this is the clipped polygon above).  d_iou [n] = IoU(d_boxes1[i], d_boxes2[i]), the bits of
 *   frcnn_ops_box_iou_rotated(mode 0, aligned) from the same device function, and d_inter [n] = the intersection area it divides (0 under
 *   the zero rule).  n == 0 returns FRCNN_OK; n <= 4194240.
 * frcnn_ops_diff_iou_rotated_backward: d_dboxes1 / d_dboxes2 [n][5] = the gradient of sum_i (grad_iou[i] iou[i] + grad_inter[i] inter[i])
 *   in the boxes.  d_grad_iou or d_grad_inter may be NULL (zeros), not both; d_dboxes1 or d_dboxes2 may be NULL (skipped), not both.  One
 *   launch, one lane per pair, no atomics, no workspace, every element of a wanted gradient written once; deterministic.  The lane
 *   repeats the clip and carries, per vertex, the tag of the boundary piece that leaves it: box 1's edges 0..3 in the order the corners
 *   are laid down (edge 0 the local +h/2 side, 1 the -w/2 side, 2 the -h/2 side, 3 the +w/2 side) or one of box 2's four lines; a kept
 *   vertex keeps its tag, a crossing where the polygon leaves the half-plane takes the clip line's, one where it enters takes that of
 *   the vertex it comes from.  With L_e the length of edge e of the final polygon, o box 1's centre in box 2's frame, d = angle1 - angle2,
 *   (cd, sd) its cosine and sine as the forward forms them, and n_k the outward normal of box 1's edge k -- (-sd, cd), (-cd, -sd),
 *   (sd, -cd), (cd, sd) --
 *     d inter / d (w2 / 2) = the sum of L_e over the edges on x = +-w2 / 2, d inter / d (h2 / 2) likewise,
 *     d inter / d (w1 / 2) = the sum over the edges tagged 1 or 3, d inter / d (h1 / 2) over those tagged 0 or 2,
 *     d inter / d o = the sum over box 1's edges of L_e n_k, d inter / d d = the sum over box 1's edges of L_e (n_k . perp(mid_e - o)),
 *   perp(x, y) = (-y, x), mid_e the edge's midpoint; chained by o = R(-angle2)(centre1 - centre2), so d o / d angle2 = (o_y, -o_x), and
 *   d d / d angle1 = 1, d d / d angle2 = -1.  With U = w1 h1 + w2 h2 - inter the adjoint of inter is grad_inter + grad_iou (U + inter) /
 *   U^2 and that of each area w h is -grad_iou inter / U^2.  Where edges of the two boxes coincide the function has a kink; the result
 *   is the one-sided derivative of the polygon the clip produced (a vertex on a line counts as inside).  A pair under the zero rule, or
 *   whose polygon has fewer than 3 vertices, gets exact zeros in all ten slots, whatever NaNs the boxes hold. */
int frcnn_ops_box_iou_rotated(const float* d_boxes1, int n, const float* d_boxes2, int m, int mode, int aligned, float* d_out,
                              void* stream);
int frcnn_ops_diff_iou_rotated(const float* d_boxes1, const float* d_boxes2, int n, float* d_iou, float* d_inter, void* stream);
int frcnn_ops_diff_iou_rotated_backward(const float* d_boxes1, const float* d_boxes2, const float* d_grad_iou, const float* d_grad_inter,
                                        int n, float* d_dboxes1, float* d_dboxes2, void* stream);
int frcnn_ops_nms_rotated(const float* d_boxes, const int64_t* d_order, const int64_t* d_categories, int n, float iou_threshold,
                          uint8_t* d_keep, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_roi_align_rotated_cull_list(void);
int frcnn_ops_roi_align_rotated(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                                float spatial_scale, int sampling_ratio, int aligned, int clockwise, float* d_out, void* stream);
int frcnn_ops_roi_align_rotated_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                         float spatial_scale, int sampling_ratio, int aligned, int clockwise, const float* d_dout,
                                         float* d_dx, void* stream);
int frcnn_ops_roi_align_rotated_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                                   int out_w, float spatial_scale, int sampling_ratio, int aligned, int clockwise, void* d_out,
                                   void* stream);
int frcnn_ops_roi_align_rotated_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h,
                                            int out_w, float spatial_scale, int sampling_ratio, int aligned, int clockwise,
                                            const void* d_dout, void* d_dx, void* stream);

/* RiRoIAlignRotated, the rotation-invariant RoI pooling of ReDet (csrc/ops_rot.hip): mmcv's riroi_align_rotated in both directions,
 *   restated from the published kernels (third party, absent here: restated, unpinned; where the two differ this text holds).
 *   Layouts and element types as frcnn_ops_roi_align_rotated: d_x [n_img][fh][fw][c], d_out [k][out_h][out_w][c], d_rois float32 [k][6]
 *   rows (b, cx, cy, w, h, angle).  The first c_real channels form c_real / n groups of n = num_orientations channels, channel g n + o
 *   being orientation o of group g; the channels from c_real to c (padding up to whole runs) belong to no group: the forward writes zeros
 *   there and the backward ignores them.
 *   The contract: pool, then blend.  Let S = frcnn_ops_roi_align_rotated(d_x, d_rois, spatial_scale, sampling_ratio = num_samples,
 *   aligned = 0, clockwise = !clockwise), in float32.  (mmcv's RiRoI grid is x = xx cos t - yy sin t + cx, y = xx sin t + yy cos t + cy
 *   with t = clockwise ? -angle : angle, which is the grid above under the opposite flag; sinf(-t) == -sinf(t) exactly.)  Per RoI
 *     f = (float)((double)angle * n / (2 pi)),  ind = floor(f),  l = f - ind,  r = 1 - l,  k = ind mod n taken non-negative,
 *     out[g n + o] = r * S[g n + (o - k) mod n] + l * S[g n + (o - k + 1) mod n]
 *   as two products and one sum, each rounded in float32 (no fma).  The second term is computed even when l == 0, so a NaN in the
 *   neighbouring orientation propagates, as in mmcv.  A RoI pools to zeros and sends no gradient if its batch index is outside
 *   (-1, n_img), its angle is not finite, or |f| >= 2^24.
 *   mmcv blends per sample: every sample's bilinear value is split between two output channels.  Here every source channel is pooled
 *   once and the pooled values are blended: the same sum in another order at half the loads, and the output is, bit for bit, the blend
 *   above applied to frcnn_ops_roi_align_rotated's own output.  One launch: a wave pools whole groups' runs, exchanges them through LDS
 *   and stores the blended runs once; S never reaches memory.
 * frcnn_ops_riroi_align_rotated_backward: d_dx [n_img][fh][fw][c], every element overwritten (k == 0: zeros), for d_x only.
 *     dS[g n + j] = r * dout[g n + (j + k) mod n] + l * dout[g n + (j + k - 1) mod n]     (rounded the same way)
 *   and then exactly frcnn_ops_roi_align_rotated_backward on dS -- the same launch grid, RoI order, bin order, w_sum / count and cull
 *   list (frcnn_ops_roi_align_rotated_cull_list()) -- in one launch: dS is blended where that gather loads a bin's gradient, is never
 *   rounded to 16 bits and never written to memory.  Deterministic, no atomics.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): frcnn_ops_roi_align_rotated's limits (num_samples as
 *   sampling_ratio), num_orientations outside [1, frcnn_ops_riroi_align_rotated_max_orientations() = 64] (a group must fit the 64
 *   channel runs of one wave wherever it starts in its run), c_real not a positive multiple of num_orientations or above c, NULL pointers.
 * The _16 forms take float16 / bfloat16 maps under the contract of the 16-bit operators above: S and the blend stay float32 and the
 *   result is rounded once. */
int frcnn_ops_riroi_align_rotated_max_orientations(void);
int frcnn_ops_riroi_align_rotated(const float* d_x, int n_img, int fh, int fw, int c, int c_real, const float* d_rois, int k, int out_h,
                                  int out_w, float spatial_scale, int num_samples, int num_orientations, int clockwise, float* d_out,
                                  void* stream);
int frcnn_ops_riroi_align_rotated_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int c_real, int out_h, int out_w,
                                           float spatial_scale, int num_samples, int num_orientations, int clockwise, const float* d_dout,
                                           float* d_dx, void* stream);
int frcnn_ops_riroi_align_rotated_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, int c_real, const float* d_rois,
                                     int k, int out_h, int out_w, float spatial_scale, int num_samples, int num_orientations,
                                     int clockwise, void* d_out, void* stream);
int frcnn_ops_riroi_align_rotated_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int c_real,
                                              int out_h, int out_w, float spatial_scale, int num_samples, int num_orientations,
                                              int clockwise, const void* d_dout, void* d_dx, void* stream);

/* rotated_feature_align, the feature refinement module of R3Det (csrc/ops_rfa.hip): mmcv's rotated_feature_align in both directions,
 *   restated from the published kernels (third party, absent here: restated, unpinned; where the two differ this text holds).
 *   Layouts (element types as frcnn_ops_roi_align above; c % 4 == 0, the _16 forms c % 8 == 0):
 *     d_x, d_out, d_dout, d_dx : [n_img][fh][fw][c];   d_boxes : float32 [n_img][fh][fw][5], one row b per pixel
 *   The box row.  COMPONENT 0 IS THE ROW (y) COORDINATE, component 1 the column (x): (y, x, w, h, angle), in input coordinates; a caller
 *   holding (x, y, w, h, a) rows swaps the first two columns.  With s = spatial_scale, all in float32, each operation rounded on its own:
 *     y0 = b[0] s,  x0 = b[1] s,  w2 = b[2] s / 2,  h2 = b[3] s / 2,  a = b[4],
 *     wx = cos a * w2,  wy = sin a * w2,  hx = -sin a * h2,  hy = cos a * h2,
 *     p0 = (x0, y0),  p1 = ((x0 + wx) + hx, (y0 + wy) + hy),  p2 = ((x0 - wx) + hx, (y0 - wy) + hy),
 *     p3 = ((x0 - wx) - hx, (y0 - wy) - hy),  p4 = ((x0 + wx) - hx, (y0 + wy) - hy)       as (x, y).
 *   d_out[n][h][w][:] = d_x[n][h][w][:] + sum over i < points of bilinear(d_x[n], p_i), the terms added to the pixel's own value in order
 *   i, in float32.  bilinear is frcnn_ops_roi_align's rule: value = ((w1 v1 + w2 v2) + w3 v3) + w4 v4 over (y low, x low), (y low, x high),
 *   (y high, x low), (y high, x high); nothing outside [-1, size] on either axis and nothing at a NaN or infinite coordinate; a
 *   coordinate <= 0 goes to 0 and a low index >= size - 1 collapses to the last cell.  points is 1 or 5; with points == 1 components
 *   2..4 are never read.  One launch, lanes along channels; a pixel's positions and weights are formed once per lane, not per channel.
 * The backward (for d_x only; the boxes get no gradient) is the sorted-plan gather of frcnn_ops_msda_plan / _backward_value for rows of
 *   any length, deterministic and free of atomics:
 *   frcnn_ops_rotated_feature_align_plan writes, for entry e = (pixel * points + i) * 4 + corner (pixel = (n fh + h) fw + w), the key
 *     n fh fw + cell of the cell that corner lands on and its weight; all four corners of a sample that counts nothing carry the
 *     sentinel key n_img fh fw and weight 0.  The caller sorts the keys stably and passes the sorted keys and the permutation.
 *   frcnn_ops_rotated_feature_align_backward: d_dx[cell] = d_dout[cell] FIRST (the identity term), then + weight[e] * d_dout[pixel of e]
 *     over the cell's entries in ascending e, each product and sum rounded in float32.  One group of lanes per cell and chunk of 64
 *     channel runs (256 float32 channels), all chunks over the one plan and sort; a cell's segment is found by bisection and summed by
 *     its group however long it is.  Every element of d_dx is written.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): points other than 1 or 5, fh or fw < 1, n_img < 0, c not in whole
 *   runs, n_img fh fw points 4 (the plan's entries) above 2^31 - 1 - 1024, NULL pointers.  n_img == 0 returns FRCNN_OK. */
int frcnn_ops_rotated_feature_align(const float* d_x, const float* d_boxes, int n_img, int fh, int fw, int c, float spatial_scale,
                                    int points, float* d_out, void* stream);
int frcnn_ops_rotated_feature_align_plan(const float* d_boxes, int n_img, int fh, int fw, float spatial_scale, int points, int64_t* d_keys,
                                         float* d_weights, void* stream);
int frcnn_ops_rotated_feature_align_backward(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                             const float* d_dout, int n_img, int fh, int fw, int c, int points, float* d_dx, void* stream);
int frcnn_ops_rotated_feature_align_16(int elem_type, const void* d_x, const float* d_boxes, int n_img, int fh, int fw, int c,
                                       float spatial_scale, int points, void* d_out, void* stream);
int frcnn_ops_rotated_feature_align_backward_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                                const void* d_dout, int n_img, int fh, int fw, int c, int points, void* d_dx, void* stream);

/* convex_iou, convex_giou and min_area_polygons, the point-set operators of Oriented RepPoints, CFA and SASM (csrc/ops_convex.hip).
 *   mmcv has operators of these names (third party, absent here); this text is the mathematical contract and holds where mmcv's
 *   kernels deviate from it: their epsilons, their hull tie-breaks and the scaling of their gradient output are not followed.
 *   Everything is float32.  A point set is a row of 18 floats (x1, y1, ..., x9, y9); a polygon a row of 8 floats, four vertices in ANY
 *   order.
 * Hulls.  P is the convex hull of the nine points, Q that of the polygon's four vertices, H that of all thirteen.  A hull is the list
 *   of its strictly convex vertices, counter-clockwise, starting at the vertex with the smallest x, ties to the smaller y.  A point
 *   in the interior of a hull edge is not a vertex; of exactly equal points only the one with the smallest index (a set's points
 *   before the polygon's) is a vertex.  Every product that decides a turn or a crossing is formed on coordinates relative to an
 *   origin: a set's or a polygon's own hull relative to its own smallest point, everything that involves a pair (the clip, H, the
 *   normals of the gradient) relative to Q's smallest vertex; boxes near x = 4096 behave as boxes near 0.  The hull is a function
 *   of the set, not of the order of its points: permuting the nine points, or the four vertices, changes no bit of any result
 *   (the gradient's rows are permuted alike).  The one exception: a turn is decided by comparing the two rounded products of its cross
 *   product, and where the products of points that are not truly collinear round to one value the farther point wins; among three
 *   such nearly collinear candidates that rule is no total order, and the winner can depend on the order of the points.
 * Range.  The results are specified for coordinates whose differences stay below 2^60 in magnitude: beyond, the products of the turns
 *   and the areas overflow.  Inside it, scaling every coordinate by a power of two scales every result exactly (no area is squared:
 *   I / U^2 and U / C^2 are two divisions each), as long as the areas stay above the 1e-14 of the dead rule, which is absolute.
 *   min_area_polygons has no such rule: where the products of differences underflow (differences below 2^-60) its hull may come out
 *   flat, but it scales an edge by its larger component before it takes the length, so its unit vectors are finite for any two
 *   distinct vertices.
 * Areas.  A_P, A_Q and C = area(H) are shoelace sums (the fan of triangles from the first hull vertex); I = area(P n Q) is the area of
 *   P's hull clipped against Q's half-planes (Sutherland-Hodgman, at most 13 vertices), clamped at 0 from below; U = A_P + A_Q - I.
 * Dead rows and pairs.  A row is dead when a coordinate is not finite, a polygon also when A_Q < 1e-14.  A pair is dead when either
 *   of its rows is, or when U < 1e-14 or C < 1e-14.  A degenerate point set (A_P = 0: coincident or collinear points) is NOT dead:
 *   it has I = 0 and a gradient through C.
 * frcnn_ops_convex_iou: d_out[n][k] = I / U of set i and polygon j, 0 for a dead pair.  One launch; a workgroup owns
 *   frcnn_ops_convex_iou_tile_rows() rows x 64 columns, forms the hull of each of its rows and columns once, in LDS, and sweeps
 *   them; a pair whose axis-aligned bounding boxes are apart is 0 without a clip.  (C plays no part: C >= U.)
 * frcnn_ops_convex_giou: aligned pairs, one launch writing both outputs.  d_giou[n] = I / U + U / C - 1;  d_grad[n][18] its derivative
 *   in the set's coordinates (the polygon is a target), in closed form.  For a hull edge a -> b let N = (b_y - a_y, a_x - b_x), the
 *   outward normal times the edge's length; clip the edge against Q's half-planes (Cyrus-Beck), [t0, t1] the parameter interval
 *   inside Q, s1 = t1 - t0, s2 = (t1^2 - t0^2) / 2.  Then
 *     dA_P: every edge of P adds N / 2 to a and to b;     dC: the same over H's edges, for those ends that are points of the set;
 *     dI: every edge of P with t1 > t0 adds N (s1 - s2) to a and N s2 to b;     dU = dA_P - dI;
 *     d giou = dI / U - I dU / U^2 + dU / C - U dC / C^2.
 *   Points that are not vertices of P get exactly 0; a dead pair gives giou = 0 and a zero row.  Where hull membership changes or
 *   edges coincide the function has a kink and the result is the one-sided derivative of the hulls that were formed.
 * frcnn_ops_min_area_polygons: d_out[n][8].  For every edge k of P in hull order, with u the edge's unit direction and v its left
 *   normal: the extents [u_min, u_max] x [0, v_max] of the hull's vertices relative to the edge's start vertex.  The result is the
 *   rectangle of the smallest area (u_max - u_min) v_max, ties to the first k, as four corners counter-clockwise: (u_min, 0),
 *   (u_max, 0), (u_max, v_max), (u_min, v_max).  A hull of two vertices a, b gives (a, b, b, a), one of a single vertex that vertex
 *   four times, a row with a non-finite coordinate zeros.  One launch.  Exact ties are structural (all edges of an acute triangle
 *   give twice its area; so does every hull whose rectangle rests on three vertices) and no float32 sum resolves them, so a tie
 *   has a width: walking k upwards, edge k replaces the best so far only when its area < (1 - 2^-18) * best.
 * No vertex list lives in scratch memory (LDS columns, one per lane); no atomics; every output element is written.  Arguments are
 *   validated before the GPU is touched (FRCNN_EINVAL): negative counts, more than 2^31 - 1 - 1024 rows (the grids' ceilings are formed
 *   in int), more than 65535 * 64 polygons in convex_iou, NULL pointers.
 *   n == 0 (or k == 0) returns FRCNN_OK without a launch. */
int frcnn_ops_convex_iou_tile_rows(void);
int frcnn_ops_convex_iou(const float* d_pointsets, int n, const float* d_polygons, int k, float* d_out, void* stream);
int frcnn_ops_convex_giou(const float* d_pointsets, const float* d_polygons, int n, float* d_giou, float* d_grad, void* stream);
int frcnn_ops_min_area_polygons(const float* d_pointsets, int n, float* d_out, void* stream);

/* box_iou_quadri, nms_quadri and points_in_polygons, the quadrilateral operators of the heads that predict four free corners and of the
 *   point-set assigners (csrc/ops_quadri.hip, on the device functions of csrc/ops_convex.h).  mmcv has operators of these names (third
 *   party, absent here); this text is the contract and holds where mmcv's kernels deviate from it.  Everything is float32.
 * The quadrilateral.  A row of 8 floats (x1, y1, ..., x4, y4): four vertices in ANY order and either winding.  It stands for Q, the
 *   convex hull of its four vertices under the hull rules stated above for convex_iou: strictly convex vertices, counter-clockwise from
 *   the smallest (x, y); of equal points the smallest index; a turn decided by comparing the two rounded products of its cross product,
 *   formed relative to the quadrilateral's own smallest point.  Permuting the four vertices changes no bit of any result.  A non-convex
 *   or self-crossing row therefore counts as its hull: THE ONE DELIBERATE DEVIATION from mmcv, whose kernels walk the vertices in the
 *   order given.  For a convex quadrilateral given in order -- every use in mmrotate -- the two definitions agree.
 * Dead rows.  A row with a coordinate that is not finite is dead; so is a quadrilateral whose hull area is below 1e-14.
 * frcnn_ops_box_iou_quadri: A1, A2 are the hull areas (the fan from the first hull vertex, on coordinates relative to the row's own
 *   smallest point); I is the area of hull 1 clipped against hull 2's half-planes (Sutherland-Hodgman, a vertex on the line counts as
 *   inside, at most 8 vertices), formed on coordinates relative to hull 2's smallest vertex and clamped at 0 from below.
 *   mode 0: I / (A1 + A2 - I);  mode 1 (iof): I / A1.  A pair is exactly 0 when either row is dead or the denominator is below 1e-14; a
 *   pair whose axis-aligned bounding boxes are apart is 0 without a clip.  A live quadrilateral against its own bits gives exactly 1 in
 *   both modes.  aligned == 0: d_out[n][m]; one launch, a workgroup owns frcnn_ops_box_iou_quadri_tile_rows() rows x 64 columns and
 *   forms the hull of each of its rows and columns once, in LDS.  aligned != 0 needs n == m and writes d_out[n], one lane per pair,
 *   bit-identical to the matrix's diagonal.  Consequence of the shared arithmetic: in mode 0, for a live row a[i],
 *   box_iou_quadri(a, b)[i][j] has the bits of convex_iou(s, b)[i][j], where s[i] is a[i]'s four vertices followed by five copies of
 *   its first vertex.
 * frcnn_ops_nms_quadri: frcnn_ops_nms_rotated on rows of 8 floats -- the same arguments, the same workspace
 *   (frcnn_ops_nms_workspace_bytes(n)), the same 64 x 64 bit tiles, tile skipping and greedy pass.  Sorted quadrilateral j goes iff a
 *   kept quadrilateral i before it, of the same category, has IoU(i, j) > iou_threshold; that IoU has the value and the argument order
 *   of frcnn_ops_box_iou_quadri mode 0 (quads1 = i, quads2 = j), from the same device function.
 * frcnn_ops_points_in_polygons: d_points[n][2], d_polygons[m][8], d_out[n][m].  d_out[i][j] = 1.0f when point i lies in the CLOSED hull
 *   Q_j: for every hull edge a -> b, (b_x - a_x) (p_y - a_y) >= (b_y - a_y) (p_x - a_x), every difference formed on coordinates
 *   relative to Q_j's smallest vertex and the two rounded products compared; otherwise 0.0f.  0.0f for a dead polygon and for a point
 *   with a coordinate that is not finite.  A point on an edge or on a vertex is inside, as a vertex on the line is in the clip; mmcv's
 *   crossing-number loop is half-open on the boundary instead.  One launch; a workgroup owns
 *   frcnn_ops_points_in_polygons_tile_rows() points x 64 polygons and forms each polygon's hull once.
 * No vertex list lives in scratch memory (LDS columns, one per lane); no atomics; every output element is written once; two runs agree
 *   bit for bit.  Arguments are validated before the GPU is touched (FRCNN_EINVAL): negative counts, more than
 *   frcnn_ops_quadri_max_rows() rows (2^31 - 1 - 1024: the grids' ceilings are formed in int), more than
 *   frcnn_ops_quadri_max_columns() (65535 * 64) columns of a matrix, mode outside {0, 1}, aligned with n != m, more boxes than
 *   frcnn_ops_nms takes, a workspace that is too small, NULL pointers with non-zero counts.  n == 0 (or m == 0) returns FRCNN_OK
 *   without a launch. */
int frcnn_ops_box_iou_quadri_tile_rows(void);
int frcnn_ops_points_in_polygons_tile_rows(void);
int frcnn_ops_quadri_max_rows(void);
int frcnn_ops_quadri_max_columns(void);
int frcnn_ops_box_iou_quadri(const float* d_quads1, int n, const float* d_quads2, int m, int mode, int aligned, float* d_out, void* stream);
int frcnn_ops_nms_quadri(const float* d_quads, const int64_t* d_order, const int64_t* d_categories, int n, float iou_threshold,
                         uint8_t* d_keep, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_points_in_polygons(const float* d_points, int n, const float* d_polygons, int m, float* d_out, void* stream);

/* masked_conv2d, the sparse convolution of Guided Anchoring's heads (GA-RPN, GA-Faster R-CNN, GA-RetinaNet; csrc/ops_mconv.hip): a
 *   stride-1 convolution evaluated only at the output pixels a mask marks.  mmcv has an operator of this name (third party, absent here:
 *   its published algorithm restated, unpinned; where the two differ this text holds).  Inference only: there is no backward.
 * Tensors.  T is float32, float16 or bfloat16 (elem_type FRCNN_OPS_F32 / _F16 / _BF16), one type for every tensor of a call.
 *   d_input  [n_img, c_in, h, w] elements of T read IN PLACE through in_stride[4], the element strides of (b, c, y, x): an NCHW-contiguous
 *            and a channels_last map are both legal, as is any other non-negative stride set whose extent stays below the index limit.
 *   d_weight [c_out, c_in, kh, kw] contiguous; d_bias [c_out] contiguous, or NULL for a zero bias.
 *   d_mask   [n_img, oh, ow] uint8, contiguous, on the OUTPUT grid oh = h + 2 pad_h - kh + 1, ow = w + 2 pad_w - kw + 1; a pixel is active
 *            iff its byte is not 0 (the caller forms it as mask > 0, so a NaN is inactive).
 *   d_out    [n_img, c_out, oh, ow] written through out_stride[4]; every element is written by this call.
 * Values.  At an active pixel
 *     out[b, co, y, x] = T(bias[co] + sum over (c, i, j) of weight[co, c, i, j] * input[b, c, y - pad_h + i, x - pad_w + j]),
 *   taps outside the map counting as zero; at every other pixel out is +0.0 (no bias there: mmcv's new_zeros).  The sum runs in float32
 *   in ascending r = (c kh + i) kw + j: for float32 an fma chain on v_mfma_f32_32x32x2_f32, for the 16-bit types exact products on
 *   v_mfma_f32_32x32x16_{f16,bf16} with float32 accumulators; the bias is widened and added last, in float32, and the store rounds once
 *   to nearest even.  The order depends on (c_in, kh, kw) alone: not on the pixel's place in the list or the tile, n_img, the strides or
 *   the rest of the mask, so an active pixel's bits are those it has under the all-ones mask, an n_img-image call equals n_img calls, the
 *   two memory formats agree, and two runs agree.
 * Deliberate deviations from mmcv: n_img >= 1 (mmcv asserts 1); the mask lives on the output grid (mmcv asserts the map's size and
 *   scatters out of bounds when the padding makes the output smaller); a NULL bias is a zero bias (mmcv fails); no host synchronisation
 *   (mmcv finds the active pixels with nonzero); the Python module refuses a dilation or groups other than 1 (mmcv ignores the dilation).
 * Kernels.  A compaction pass over the mask appends each active pixel's index b oh ow + p (int32) to a list in the workspace behind its
 *   count, and writes the zeros of each inactive pixel, once.  The list's order is not fixed (integer atomics on the count); no output
 *   bit depends on it.  The product is an implicit GEMM over tiles of frcnn_ops_masked_conv2d_tile_pixels() listed pixels by
 *   frcnn_ops_masked_conv2d_tile_channels() output channels, staged through LDS in chunks of frcnn_ops_masked_conv2d_k_chunk() reduction
 *   indices; its grid is sized for the worst case and a block whose tile starts at or past the device-side count returns at once.  Taps
 *   outside the map are zeros formed in registers; no address outside a tensor is formed.  No atomics on floating-point data.
 * Limits.  Indices are 32-bit.  FRCNN_EINVAL before the GPU is touched: an unknown elem_type, sizes < 1, a negative padding, an empty
 *   output grid, n_img oh ow, c_in kh kw, c_out c_in kh kw or a tensor's extent (1 + the largest element offset its strides reach) above
 *   frcnn_ops_masked_conv2d_max_index() = 2^31 - 1 - 1024, a negative stride, c_out above 65535 channel tiles, NULL pointers (d_bias
 *   excepted), a workspace smaller than frcnn_ops_masked_conv2d_workspace_bytes(n_img, oh, ow) (0 for sizes it refuses) or not 4-byte
 *   aligned.  in_stride and out_stride are HOST arrays, read before the call returns. */
int frcnn_ops_masked_conv2d_tile_pixels(void);
int frcnn_ops_masked_conv2d_tile_channels(void);
int frcnn_ops_masked_conv2d_k_chunk(void);
int frcnn_ops_masked_conv2d_max_index(void);
size_t frcnn_ops_masked_conv2d_workspace_bytes(int n_img, int oh, int ow);
int frcnn_ops_masked_conv2d(int elem_type, const void* d_input, const int64_t* in_stride, int n_img, int c_in, int h, int w,
                            const void* d_weight, const void* d_bias, int c_out, int kh, int kw, int pad_h, int pad_w,
                            const uint8_t* d_mask, void* d_out, const int64_t* out_stride, void* d_ws, size_t ws_bytes, void* stream);

/* The mask operators of a Mask R-CNN's last step (csrc/ops_mask.hip).  torchvision and detectron2 / mmdetection are third parties, absent
 *   here: their published algorithms restated, unpinned; where they differ from this text, this text holds.  No autograd (upstream's
 *   paste is never differentiated).  Nothing synchronises with the host; every output element is written by the call's own launches, no
 *   memset precedes them, no atomics: two runs agree bit for bit.
 *
 * frcnn_ops_paste_masks_in_image: torchvision's roi_heads.paste_masks_in_image (expand_masks, expand_boxes, .to(int64),
 *   paste_mask_in_image) without its loop over the masks and its four host reads per mask.
 *   d_masks [k, m, m] elements of T (elem_type FRCNN_OPS_F32 / _F16 / _BF16), contiguous; d_boxes [k, 4] float32 (x1, y1, x2, y2);
 *   d_out [k, h, w] elements of T, contiguous.  With M' = m + 2 padding and s = float32((double)M' / (double)m):
 *   The integer box, in float32, every operation rounded on its own (NO contraction into fused multiply-adds: a fused
 *   x_c - w_half * s changes the integer for real boxes), in this order:
 *       w_half = (x2 - x1) * 0.5    h_half = (y2 - y1) * 0.5    x_c = (x2 + x1) * 0.5    y_c = (y2 + y1) * 0.5
 *       w_half = w_half * s         h_half = h_half * s
 *       X0 = trunc(x_c - w_half)    X1 = trunc(x_c + w_half)    Y0 = trunc(y_c - h_half)    Y1 = trunc(y_c + h_half)
 *   trunc rounds toward zero (torch's .to(int64)) and SATURATES to [-C, C], C = frcnn_ops_paste_masks_max_corner() = 2^29.
 *   The target size: bw = max(X1 - X0 + 1, 1), bh = max(Y1 - Y0 + 1, 1).
 *   Pixel (y, x) of image i is non-zero only if X0 <= x < X0 + bw, X0 <= X1, Y0 <= y < Y0 + bh and Y0 <= Y1.  There, with dx = x - X0,
 *       r = float32(M') / float32(bw)    sx = max(r * (float32(dx) + 0.5) - 0.5, 0)
 *       ix = min((int)sx, M' - 1)        ix1 = ix + (ix < M' - 1)        lx = sx - ix
 *   likewise (iy, iy1, ly) from dy = y - Y0 and bh, and
 *       value = (1 - ly) * ((1 - lx) * P[iy][ix] + lx * P[iy][ix1]) + ly * ((1 - lx) * P[iy1][ix] + lx * P[iy1][ix1])
 *   where P is the mask padded by `padding` zeros on each side (never materialised) -- F.interpolate(bilinear, align_corners=False)
 *   to (bh, bw).  Masks are widened exactly, the arithmetic is float32 without contraction, and the store rounds once (ops_elem.h):
 *   op(x_T) == op(x_T.float()).to(T) bit for bit.  Everywhere else the pixel is +0.0.
 *   Stated deviations (torchvision raises or is undefined there): a row with a non-finite coordinate, an inverted integer box or a box
 *   wholly outside the image gives an all-zero image; integer corners saturate as above; a huge box costs nothing extra (only pixels of
 *   the image are evaluated); k == 0 is legal and launches nothing.
 *
 * frcnn_ops_paste_masks_aligned: detectron2's paste_masks_in_image / mmdetection's _do_paste_mask followed by the threshold.
 *   d_masks [k, mh, mw] elements of T, contiguous; d_boxes [k, 4] float32 (x0, y0, x1, y1); d_out [k, h, w] bytes.  The sample
 *   coordinates of pixel (y, x) are formed in pixels, in float32 and in this order (no normalised round trip):
 *       sx = ((float32(x) + 0.5) - x0) / (x1 - x0) * float32(mw) - 0.5        sy = ((float32(y) + 0.5) - y0) / (y1 - y0) * float32(mh) - 0.5
 *   and value is the blend above with ix = floor(sx), ix1 = ix + 1, lx = sx - ix (likewise y) on the UNPADDED mask, a corner outside
 *   it counting 0 (grid_sample(align_corners=False, padding_mode="zeros")); a sample with sx outside (-1, mw) or sy outside (-1, mh)
 *   is 0.  float32 on widened masks, never rounded to a 16-bit type.  The byte is value >= threshold (as_uint8 == 0; 0 or 1), or
 *   trunc(value * 255) saturated to [0, 255] with NaN giving 0 (as_uint8 != 0).
 *   Stated deviations: a row with a non-finite coordinate, x1 <= x0 or y1 <= y0 gives all 0 bytes, whatever the threshold (upstream
 *   flips or smears such a mask); decisions may differ from upstream's on values within the float32 error of the threshold.
 *
 * frcnn_ops_masks_to_boxes: torchvision.ops.masks_to_boxes.  d_masks [n, h, w] elements of elem_bytes = 1 (bool, uint8), 2 (float16,
 *   bfloat16) or 4 (float32) bytes, contiguous; d_out [n, 4] float32 (x_min, y_min, x_max, y_max) over the pixels != 0, maxima inclusive.
 *   A float is non-zero iff any bit but its sign is set: -0.0 is zero, every NaN is not.  A mask without such a pixel gives
 *   (0, 0, 0, 0) -- detectron2's convention for empty masks; torchvision raises there.  Two stages: integer extrema of bands of
 *   every mask into the workspace (every entry written, no initial value needed), then one wave per mask combines them.
 *
 * Limits, FRCNN_EINVAL before the GPU is touched: an unknown elem_type / elem_bytes; m, mh or mw outside [1,
 *   frcnn_ops_paste_masks_max_side()] (the mask is staged in LDS as float32; 112); padding outside [0,
 *   frcnn_ops_paste_masks_max_padding()]; h or w < 1 or h w above frcnn_ops_mask_max_plane() = 2^31 - 1 - 1024 (indices inside one image
 *   are 32-bit; the offset of an image is 64-bit, so k h w may exceed 2^31); k or n < 0; with k, n > 0 a NULL pointer, an output not
 *   aligned to its element, a workspace smaller than frcnn_ops_masks_to_boxes_workspace_bytes(n, h, w, elem_bytes) (0 for arguments it
 *   refuses) or not 16-byte aligned.  Inputs and outputs need no other alignment: heads and tails of an image around the aligned
 *   vectors are handled element by element. */
int frcnn_ops_paste_masks_max_side(void);
int frcnn_ops_paste_masks_max_padding(void);
int frcnn_ops_paste_masks_max_corner(void);
int frcnn_ops_mask_max_plane(void);
int frcnn_ops_paste_masks_in_image(int elem_type, const void* d_masks, const float* d_boxes, int k, int m, int padding, int h, int w,
                                   void* d_out, void* stream);
int frcnn_ops_paste_masks_aligned(int elem_type, const void* d_masks, const float* d_boxes, int k, int mh, int mw, int h, int w,
                                  float threshold, int as_uint8, uint8_t* d_out, void* stream);
size_t frcnn_ops_masks_to_boxes_workspace_bytes(int n, int h, int w, int elem_bytes);
int frcnn_ops_masks_to_boxes(int elem_bytes, const void* d_masks, int n, int h, int w, float* d_out, void* d_ws, size_t ws_bytes,
                             void* stream);

/* The keypoint operator of a Keypoint R-CNN's last step (csrc/ops_keypoint.hip): torchvision's roi_heads.heatmaps_to_keypoints and
 *   detectron2's structures.keypoints.heatmaps_to_keypoints without their loop over the detections, its two host reads and its
 *   [k, H, W] float image per detection.  Third parties, absent here: their published algorithm restated, unpinned; where they differ
 *   from this text, this text holds.  No autograd.  One launch, a block per (RoI, keypoint); nothing synchronises with the host, no
 *   workspace, no memset, no atomics; every output element is written once; two runs agree bit for bit.
 *
 * frcnn_ops_heatmaps_to_keypoints: d_maps [r, k, mh, mw] elements of T (elem_type FRCNN_OPS_F32 / _F16 / _BF16), contiguous, widened
 *   exactly once on the way into LDS (ops_elem.h), so that op(x_T) == op(x_T.float()) bit for bit; d_rois [r, 4] float32
 *   (x1, y1, x2, y2); d_out [r, k, 4] float32 (x, y, logit, prob).
 *   Per RoI, in float32:  w = max(x2 - x1, 1)   h = max(y2 - y1, 1)   W = ceil(w)   H = ceil(h).
 *   The logit image of keypoint j is the bicubic resize of map j to [H, W], torch's upsample_bicubic2d(align_corners=False): Keys'
 *   kernel with A = -0.75, the source coordinate not clamped, the four taps per axis on indices clamped to the map.  Its arithmetic is
 *   float32, every operation rounded on its own (NO contraction into fused multiply-adds), in THIS order (it need not be torch's:
 *   torch's CPU and CUDA kernels do not agree with each other either).  For output coordinate d of an axis of n source and N output
 *   pixels (n = mw, N = W for x; n = mh, N = H for y):
 *       scale = float32(n) / float32(N)        src = scale * (float32(d) + 0.5) - 0.5        f = floor(src)        t = src - f
 *       i_j = min(max(f - 1 + j, 0), n - 1),  j = 0 .. 3
 *       u0 = t + 1                  c_0 = ((-0.75 * u0 + 3.75) * u0 - 6) * u0 + 3
 *                                   c_1 = ((1.25 * t - 2.25) * t) * t + 1
 *       u2 = 1 - t                  c_2 = ((1.25 * u2 - 2.25) * u2) * u2 + 1
 *       u3 = u2 + 1                 c_3 = ((-0.75 * u3 + 3.75) * u3 - 6) * u3 + 3
 *   The rows are combined first, then the columns, each sum from the left:
 *       v[y][c] = ((cy_0 * M[iy_0][c] + cy_1 * M[iy_1][c]) + cy_2 * M[iy_2][c]) + cy_3 * M[iy_3][c]          for every column c of the map
 *       image[y][x] = ((cx_0 * v[y][ix_0] + cx_1 * v[y][ix_1]) + cx_2 * v[y][ix_2]) + cx_3 * v[y][ix_3]
 *   The answer is the image's maximum under a total order on (value, index = y * W + x): a NaN is larger than every number, then the
 *   larger value (+0.0 and -0.0 are equal), then the smaller index -- so ties go to the smallest y * W + x and the first NaN wins
 *   (torch's argmax rule), whatever the order of the reduction.  With the maximum v at (xi, yi), in float32 and in this order:
 *       x = (float32(xi) + 0.5) * (w / float32(W)) + x1        y = (float32(yi) + 0.5) * (h / float32(H)) + y1        logit = v
 *       prob = 1 / sum over the mh x mw map of exp(M - v)      (detectron2's roi_map_scores at the maximum)
 *   The sum's order is fixed (per lane, a butterfly, the waves in order) but not part of the contract; prob is accurate to the
 *   float32 error of its terms, not bit-exact against another implementation.
 *   Defined where upstream leaves it open:
 *     - A constant map (every element compares equal to the first; +0.0 == -0.0) IS its resized image, whose float32 evaluation would
 *       otherwise differ in the last bits from pixel to pixel: (xi, yi) = (0, 0), logit = the first element, prob by the formula
 *       (1 / (mh mw) for a finite constant).
 *     - A NaN in the map spreads to the pixels whose taps touch it; the first such pixel wins, logit and prob are NaN.
 *     - An all -inf map is a constant map: (0, 0), logit = -inf, and prob is NaN (exp(-inf - -inf)); so is an all +inf map.  A map that
 *       mixes -inf with numbers resizes to NaNs around each -inf (0 * inf, inf - inf in the taps) and falls under the NaN rule.
 *     - A RoI is REFUSED when a coordinate is not finite or when W or H exceeds frcnn_ops_keypoint_max_roi_side() = 4096 (one block
 *       walks the whole image: at most 2^24 pixels, 2^16 a lane, about ten milliseconds; x2 - x1 overflowing to +inf is refused by
 *       the same comparison).  A refused RoI gives four NaNs for each of its keypoints and costs no work: its blocks return before
 *       they read the map.
 *     - w or h under 1, an inverted box included, is clamped to 1 as upstream clamps it.
 *     - r == 0 or k == 0 is legal and launches nothing.
 * Limits, FRCNN_EINVAL before the GPU is touched: an unknown elem_type; mh or mw outside [1, frcnn_ops_keypoint_max_map_side()] (the map
 *   is staged in LDS as float32; 112); r or k < 0; r k above 2^31 - 1; with r k > 0 a NULL pointer.
 *   frcnn_ops_keypoint_block_threads() = 256: a block's waves of 64 lanes take one output row each per pass and 64 pixels of it per
 *   step (what the tests size their seams by). */
int frcnn_ops_keypoint_max_map_side(void);
int frcnn_ops_keypoint_max_roi_side(void);
int frcnn_ops_keypoint_block_threads(void);
int frcnn_ops_heatmaps_to_keypoints(int elem_type, const void* d_maps, const float* d_rois, int r, int k, int mh, int mw, float* d_out,
                                    void* stream);

/* Soft-NMS (Bodla et al., 2017), per label (csrc/ops_softnms.hip): mmcv's soft_nms, which exists on the CPU only, restated from its
 *   published loop (third party, absent here: restated, unpinned; where the two differ this text holds).
 * The contract.  All arithmetic is float32, every operation rounded on its own (no contraction), the division IEEE; min and max are
 *   fminf / fmaxf (a NaN operand gives the other one).  thr = iou_threshold, sigma and min_score arrive as float32; off = (float)offset.
 *   Each label (d_categories) is an independent problem; without labels there is one problem.  Within a problem every box j has a
 *   working score s_j = d_scores[j] and area_j = (x2_j - x1_j + off) * (y2_j - y1_j + off); the live set starts as all of the
 *   problem's boxes.  While the live set is not empty:
 *     1. pick the live box i with the largest s; ties (-0 == +0 is one) go to the smaller box index; NaN scores rank after every
 *        number, among themselves by index.  Box i leaves the live set and is KEPT with its current s_i, whatever that is: the first
 *        pick of a problem is kept even when its score is below min_score;
 *     2. for every live j: w = max(0, min(x2_i, x2_j) - max(x1_i, x1_j) + off), h likewise in y, inter = w * h,
 *        ovr = inter / ((area_i + area_j) - inter), and a NaN ovr (0 / 0) counts as 0;
 *     3. weight = method 0 (naive): ovr >= thr ? 0 : 1;  1 (linear): ovr >= thr ? 1 - ovr : 1;  2 (gaussian): expf(-(ovr * ovr) / sigma);
 *     4. s_j = s_j * weight; if s_j < min_score, j leaves the live set and is DROPPED (a NaN s_j never is).
 *   The final score of a kept box is the s it was picked with.
 *   The output order is (final score descending, ties by ascending index, NaN last) over the kept boxes of all problems.  Within one
 *   problem of non-negative scores and proper boxes that is exactly the pick order, so this entry point returns no rank and the
 *   caller sorts by that key, which also merges the problems.  Proof: picks are non-increasing -- pick t is the maximum of the live
 *   set, every live s_j <= s_t, and for ovr in [0, 1] all three weights lie in [0, 1], so s_j * weight <= s_j <= s_t when s_j >= 0:
 *   the maximum of the next live set is no larger; a NaN is picked only when no number is live, and no number becomes live later.
 *   And two picks t < u with equal final scores: u was live at pick t with s_u(then) >= s_u(final) = s_t, and s_u(then) <= s_t, so
 *   it tied with t there and t won by the smaller index.  (Negative scores, which a weight below 1 raises, or inverted boxes, whose
 *   ovr can leave [0, 1], can break the chain; the sort key is the definition of the output order either way.)
 * frcnn_ops_soft_nms: d_boxes float32 [n][4] rows (x1, y1, x2, y2), d_scores float32 [n].  d_order int64 [n]: a permutation of the box
 *   indices in which each label is one run, as frcnn_ops_nms expects, and ASCENDING in the index inside a run (the tie rule reads the
 *   position); d_categories int64 [n] by box index, any values, or NULL: one problem, d_order then ascending.  Outputs by POSITION s in
 *   d_order: d_keep[s] = 1 iff box d_order[s] is kept, d_scores_out[s] = the score it was picked with, or, for a dropped box, the
 *   rescored value that dropped it; every element of both is written.  0 <= n <= frcnn_ops_soft_nms_max_boxes() = 65536: one label may
 *   hold every box, and one workgroup then runs n dependent picks.  d_ws of frcnn_ops_soft_nms_workspace_bytes(n) bytes holds the state
 *   of problems longer than frcnn_ops_soft_nms_lds_boxes() = 4096 (shorter ones live in LDS, those of at most 64 boxes in the registers
 *   of one wave); a workgroup has frcnn_ops_soft_nms_block_threads() = 512 threads, thread i owning positions i, i + 512, ... of its
 *   problem.  One launch; deterministic (no atomics, and the argmax key is a total order).
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): n outside the range, method outside {0, 1, 2}, offset outside
 *   {0, 1}, sigma not positive and finite, a NaN iou_threshold or min_score, and for n > 0 NULL pointers (d_categories excepted) or a
 *   small workspace.  n == 0 returns FRCNN_OK. */
int frcnn_ops_soft_nms_block_threads(void);
int frcnn_ops_soft_nms_lds_boxes(void);
int frcnn_ops_soft_nms_max_boxes(void);
size_t frcnn_ops_soft_nms_workspace_bytes(int n);
int frcnn_ops_soft_nms(const float* d_boxes, const float* d_scores, const int64_t* d_order, const int64_t* d_categories, int n,
                       float iou_threshold, float sigma, float min_score, int method, int offset, float* d_scores_out, uint8_t* d_keep,
                       void* d_ws, size_t ws_bytes, void* stream);

/* CARAFE, content-aware reassembly of features (the learned upsampler of FPN_CARAFE necks; csrc/ops_carafe.hip): mmcv's carafe, restated
 *   from its published definition (third party, absent here: restated, unpinned; where the two differ this text holds).
 * Layouts: plain NCHW.  d_features [n][c][h][w], d_masks [n][group_size k k][s h][s w], d_out [n][c][s h][s w], with k = kernel_size odd,
 *   1 <= k <= frcnn_ops_carafe_max_kernel() = 7 (k k mask values, or mask-gradient sums, live in a thread's registers), group_size >= 1
 *   dividing c, s = scale_factor in [1, 8].  With r = (k - 1) / 2 and g = ch / (c / group_size):
 *     out[b][ch][ph][pw] = sum over i (outer), j (inner) in [0, k) of
 *         features[b][ch][ph / s - r + i][pw / s - r + j] * masks[b][(g k + i) k + j][ph][pw]
 *   in float32, products and sums rounded separately, starting from +0; a tap outside the map counts as a feature of +0 (zero padding).
 * frcnn_ops_carafe_backward: d_dfeatures [n][c][h][w] and d_dmasks [n][group_size k k][s h][s w], every element overwritten; either may
 *   be NULL: that gradient is skipped (d_masks may then be NULL for d_dmasks alone, d_features for d_dfeatures alone).
 *   d_dfeatures[b][ch][y][x] = the sum of dout * mask over the k k s s output pixels whose window holds (y, x), in the order
 *   low-resolution cell (qy, qx) of the pixel row-major, then its sub-pixel (sy, sx) row-major; cells outside the map are skipped.
 *   d_dmasks[b][(g k + i) k + j][ph][pw] = the sum of dout * feature over the c / group_size channels of group g ascending; exactly 0 for
 *   a tap outside the map.  Both are gathers: deterministic, no atomics, no workspace.
 * Tiling, exported because callers and tests place shapes on its seams: a forward block owns frcnn_ops_carafe_tile_height() = 4 rows of
 *   frcnn_ops_carafe_tile_width() = 64 output pixels and walks frcnn_ops_carafe_channel_chunk() = 64 channels of one group per load of
 *   its masks; the result does not depend on the tiling.
 * The _16 forms take float16 / bfloat16 tensors (elem_type, one for the whole call) under the contract of the 16-bit operators above:
 *   widened exactly on load, the float32 body, one rounding to nearest even on store.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): the limits above, n in [1, 65535], c, h, w >= 1,
 *   s h s w <= 2^31 - 1025 (32-bit indices inside a plane, 64-bit plane bases), group_size * ceil(c / group_size / 4) <= 65535 (the launch
 *   grid), NULL pointers, an elem_type other than FRCNN_OPS_F16 / FRCNN_OPS_BF16. */
int frcnn_ops_carafe_max_kernel(void);
int frcnn_ops_carafe_channel_chunk(void);
int frcnn_ops_carafe_tile_width(void);
int frcnn_ops_carafe_tile_height(void);
int frcnn_ops_carafe(const float* d_features, const float* d_masks, int n, int c, int h, int w, int kernel_size, int group_size,
                     int scale_factor, float* d_out, void* stream);
int frcnn_ops_carafe_backward(const float* d_features, const float* d_masks, const float* d_dout, int n, int c, int h, int w,
                              int kernel_size, int group_size, int scale_factor, float* d_dfeatures, float* d_dmasks, void* stream);
int frcnn_ops_carafe_16(int elem_type, const void* d_features, const void* d_masks, int n, int c, int h, int w, int kernel_size,
                        int group_size, int scale_factor, void* d_out, void* stream);
int frcnn_ops_carafe_backward_16(int elem_type, const void* d_features, const void* d_masks, const void* d_dout, int n, int c, int h,
                                 int w, int kernel_size, int group_size, int scale_factor, void* d_dfeatures, void* d_dmasks,
                                 void* stream);

/* Multi-scale deformable attention, the sampling core of Deformable DETR (csrc/ops_msda.hip): mmcv's ms_deform_attn, restated from the
 *   published algorithm (third party, absent here: restated, unpinned; where the two differ this text holds).
 * Tensors: d_value [n][s][m][d] (s cells over all levels, m heads, d channels per head); d_shapes int64 [levels][2] rows (H_l, W_l);
 *   d_starts int64 [levels]; d_loc float32 [n][q][m][levels][points][2], last axis (x, y) with [0, 1] spanning the level; d_attn float32
 *   [n][q][m][levels][points]; d_out and d_dout [n][q][m d].  Sample (b, q, m, l, p): x = fmaf(loc_x, W_l, -0.5f), y = fmaf(loc_y, H_l,
 *   -0.5f) in float32; it counts iff x > -1 && y > -1 && x < W_l && y < H_l (a NaN coordinate fails); its corners are (y0, x0), (y0, x1),
 *   (y1, x0), (y1, x1) with y0 = floor(y), y1 = y0 + 1, ly = y - y0, hy = 1 - ly (likewise x) and the weights hy hx, hy lx, ly hx, ly lx;
 *   corner (yy, xx) is cell start_l + yy W_l + xx of value[b][:][m][:] and counts 0 outside [0, H_l - 1] x [0, W_l - 1].
 *     out[b][q][m d + c] = sum over (l, p) ascending of attn * (w0 v0 + w1 v1 + w2 v2 + w3 v3)      (float32, rounded separately)
 * The shape tensors are device memory that the kernels read; no entry point copies them to the host.  They are not trusted: a level
 *   with H_l or W_l outside [1, 2^24] or start_l outside [-2^50, s) contributes nothing, a corner whose cell index falls outside [0, s)
 *   contributes nothing and receives nothing, a cell no sample reaches gets a zero gradient.
 * frcnn_ops_msda_backward_loc: d_dloc (shaped as d_loc) and d_dattn (as d_attn), every element overwritten, one store each; either may
 *   be NULL (not both).  d_dattn = sum over c of dout * sample; d_dloc x = W_l * sum over c of (dout * attn) * ((hy v1 - hy v0) + (ly v3
 *   - ly v2)) and y = H_l * sum of (dout * attn) * ((hx v2 - hx v0) + (lx v3 - lx v1)) over the validly indexed corners (a corner that
 *   counts 0 enters as 0): the right-hand slope at an integer coordinate; both 0 for a sample that does not count.  The sum over c is
 *   a lane's channels ascending, then an xor butterfly over the lanes of the item: a fixed order.
 * frcnn_ops_msda_plan + frcnn_ops_msda_backward_value: the value gradient without atomics.  The plan writes one entry per sample and
 *   corner, e = ((((b q_n + q) m_n + m) levels + l) points + p) 4 + corner: d_keys[e] = (b s + cell) m_n + m, or the sentinel n s m for a
 *   corner that counts 0, and d_weights[e] = corner weight * attn.  The caller sorts the keys STABLY (sorted keys + the permutation,
 *   int64 each) and passes them on; d_dvalue[b][cell][m][:] = the sum over the cell's entries in ascending e of weight *
 *   dout[b][q][m][:], every cell written.  A cell with more than frcnn_ops_msda_segment() = 512 entries (every query samples the
 *   few cells of a coarse level) is summed in pieces of 512 entries, cut from the segment's own start: each piece's sum ascending, then
 *   the pieces' sums in ascending order.  A cell's entries belong to its own image and the cuts depend on the segment alone: chunking
 *   the images changes no bit.  d_ws: frcnn_ops_msda_workspace_bytes(n, s, m, d, q, levels, points) bytes (the segment starts and the
 *   pieces' sums), 16-byte aligned.
 * Mapping, exported because callers and tests place shapes on its seams: a group of lanes serves one (b, q, m); a lane owns runs of 4
 *   float32 (8 16-bit) channels when d holds whole runs and the tensors are 16-byte aligned, else single channels;
 *   frcnn_ops_msda_block_items(d, levels, points, elem_type) (elem_type 0: float32) is the number of (b, q, m) a block serves for
 *   aligned tensors, 0 for arguments out of range.  The result does not depend on the mapping's block size.
 * The _16 forms take float16 / bfloat16 value, dout, out and d_value (elem_type) under the contract of the 16-bit operators above:
 *   widened exactly on load, the float32 body, one rounding to nearest even on store; loc, attn and their gradients stay float32.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): n, s, m, q >= 1, 1 <= d <= frcnn_ops_msda_max_channels() = 256,
 *   1 <= levels <= frcnn_ops_msda_max_levels() = 8, 1 <= points <= frcnn_ops_msda_max_points() = 16, n s m <= 2^31 - 1025 and
 *   n q m levels points 4 <= 2^31 - 1025 (32-bit cell and entry indices; element offsets are 64-bit), NULL pointers, a workspace that
 *   is NULL, misaligned or too small, an unknown elem_type. */
int frcnn_ops_msda_max_levels(void);
int frcnn_ops_msda_max_points(void);
int frcnn_ops_msda_max_channels(void);
int frcnn_ops_msda_block_items(int d, int levels, int points, int elem_type);
int frcnn_ops_msda_segment(void);
size_t frcnn_ops_msda_workspace_bytes(int n_img, int s, int m, int d, int q, int levels, int points);
int frcnn_ops_msda_forward(const float* d_value, const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc, const float* d_attn,
                           int n_img, int s, int m, int d, int q, int levels, int points, float* d_out, void* stream);
int frcnn_ops_msda_backward_loc(const float* d_value, const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc,
                                const float* d_attn, const float* d_dout, int n_img, int s, int m, int d, int q, int levels, int points,
                                float* d_dloc, float* d_dattn, void* stream);
int frcnn_ops_msda_plan(const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc, const float* d_attn, int n_img, int s, int m,
                        int q, int levels, int points, int64_t* d_keys, float* d_weights, void* stream);
int frcnn_ops_msda_backward_value(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                  int n_img, int s, int m, int d, int q, int levels, int points, float* d_dvalue, void* d_ws,
                                  size_t ws_bytes, void* stream);
int frcnn_ops_msda_forward_16(int elem_type, const void* d_value, const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc,
                              const float* d_attn, int n_img, int s, int m, int d, int q, int levels, int points, void* d_out,
                              void* stream);
int frcnn_ops_msda_backward_loc_16(int elem_type, const void* d_value, const int64_t* d_shapes, const int64_t* d_starts,
                                   const float* d_loc, const float* d_attn, const void* d_dout, int n_img, int s, int m, int d, int q,
                                   int levels, int points, float* d_dloc, float* d_dattn, void* stream);
int frcnn_ops_msda_backward_value_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                     const void* d_dout, int n_img, int s, int m, int d, int q, int levels, int points, void* d_dvalue,
                                     void* d_ws, size_t ws_bytes, void* stream);

/* DCNv3, the deformable convolution v3 of the InternImage backbones (csrc/ops_dcnv3.hip): a grouped, weight-free deformable sampling on
 *   channels-last maps, restated from the published operator (third party, absent here: restated, unpinned; where the two differ this
 *   text holds).
 * Tensors: d_input [n][h][w][g gc] (g groups of gc channels); d_offset float32 [n][ho][wo][g K 2], the pair of (group, point p) at
 *   (group K + p) 2 as (dx, dy); d_mask float32 [n][ho][wo][g K], that of (group, p) at group K + p; d_out and d_dout [n][ho][wo][g gc].
 *   K = kernel_h kernel_w; ho = (h + 2 pad_h - (dil_h (kernel_h - 1) + 1)) / stride_h + 1, wo likewise.  Point p = i kernel_h + j has i in
 *   [0, kernel_w) along x as the OUTER index and j in [0, kernel_h) along y (x-major).  With bx = dil_w (kernel_w - 1) / 2 and by =
 *   dil_h (kernel_h - 1) / 2 (integer division) the sample (b, oy, ox, group, p) lies at
 *       x = (ox stride_w - pad_w + bx) + ((i dil_w - bx) + dx) * offset_scale
 *       y = (oy stride_h - pad_h + by) + ((j dil_h - by) + dy) * offset_scale
 *   in pixels of the unpadded map: the two integer parts formed in int and converted exactly, the sum with the offset, the product and the
 *   final sum in float32, each rounded.  The sample counts iff x > -1 && y > -1 && x < w && y < h (a NaN coordinate fails, so no index is
 *   formed from it); its corners are (y0, x0), (y0, x1), (y1, x0), (y1, x1) with y0 = floor(y), y1 = y0 + 1, ly = y - y0, hy = 1 - ly
 *   (likewise x) and the weights hy hx, hy lx, ly hx, ly lx; a corner outside [0, h - 1] x [0, w - 1] counts 0.
 *     out[b][oy][ox][group gc + c] = sum over p ascending of mask * (((w0 v0 + w1 v1) + w2 v2) + w3 v3)     (float32, rounded separately)
 * frcnn_ops_dcnv3_backward_offset: d_doffset (shaped as d_offset) and d_dmask (as d_mask), every element overwritten, one store each;
 *   either may be NULL (not both).  d_dmask = sum over c of dout * sample; d_doffset dx = offset_scale * sum over c of (dout * mask) *
 *   ((hy v1 - hy v0) + (ly v3 - ly v2)) and dy = offset_scale * sum of (dout * mask) * ((hx v2 - hx v0) + (lx v3 - lx v1)), over the
 *   forward's accepted range and corners (a corner that counts 0 enters as 0): at an integer coordinate this is the RIGHT-HAND slope, the
 *   slope of the cell [x0, x0 + 1) that floor selects; all three are 0 for a sample that does not count (x == -1 included).  The sum over
 *   c is a lane's channels ascending, then an xor butterfly over the lanes of the item: a fixed order.
 * frcnn_ops_dcnv3_plan + frcnn_ops_dcnv3_backward_input: the input gradient without atomics.  The plan writes one entry per sample and
 *   corner, e = (((b ho wo + oy wo + ox) g_n + group) K + p) 4 + corner: d_keys[e] = (b h w + cell) g_n + group with cell = yy w + xx, or the
 *   sentinel n h w g for a corner that counts 0, and d_weights[e] = corner weight * mask.  The caller sorts the keys STABLY (sorted keys +
 *   the permutation, int64 each) and passes them on; d_dinput[b][yy][xx][group][:] = the sum over the cell's entries in ascending e of
 *   weight * dout[b][oy][ox][group][:], every cell written (zeros included), by the gather of frcnn_ops_msda_backward_value: a cell with
 *   more than frcnn_ops_msda_segment() entries is summed in pieces, cut from the segment's own start.  A cell's entries belong to its
 *   own image: chunking the images changes no bit.  d_ws: frcnn_ops_dcnv3_workspace_bytes(...) bytes, 16-byte aligned (0: invalid sizes).
 * Mapping, exported because callers and tests place shapes on its seams: a group of lanes serves one (b, oy, ox, group); a lane owns runs
 *   of 4 float32 (8 16-bit) channels when gc holds whole runs and the tensors are 16-byte aligned, else single channels;
 *   frcnn_ops_dcnv3_block_items(gc, kernel_h, kernel_w, elem_type) (elem_type 0: float32) is the number of items a block serves for
 *   aligned tensors, 0 for arguments out of range.  The result does not depend on the mapping's block size.
 * The _16 forms take float16 / bfloat16 input, dout, out and d_input (elem_type) under the contract of the 16-bit operators above:
 *   widened exactly on load, the float32 body, one rounding to nearest even on store; offset, mask and their gradients stay float32.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): n, g >= 1, 1 <= h, w <= 2^24, 1 <= gc <=
 *   frcnn_ops_dcnv3_max_channels() = 256, 1 <= kernel_h, kernel_w <= frcnn_ops_dcnv3_max_kernel() = 7, stride and dilation in [1, 65536],
 *   padding in [0, 65536], ho and wo >= 1, a finite offset_scale, n h w g <= 2^31 - 1025 and n ho wo g K 4 <= 2^31 - 1025 (32-bit cell and
 *   entry indices; element offsets are 64-bit), NULL pointers, a workspace that is NULL, misaligned or too small, an unknown elem_type. */
int frcnn_ops_dcnv3_max_kernel(void);
int frcnn_ops_dcnv3_max_channels(void);
int frcnn_ops_dcnv3_block_items(int gc, int kernel_h, int kernel_w, int elem_type);
size_t frcnn_ops_dcnv3_workspace_bytes(int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w);
int frcnn_ops_dcnv3_forward(const float* d_input, const float* d_offset, const float* d_mask, int n_img, int h, int w, int g, int gc,
                            int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                            float offset_scale, float* d_out, void* stream);
int frcnn_ops_dcnv3_backward_offset(const float* d_input, const float* d_offset, const float* d_mask, const float* d_dout, int n_img, int h,
                                    int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                    int dil_h, int dil_w, float offset_scale, float* d_doffset, float* d_dmask, void* stream);
int frcnn_ops_dcnv3_plan(const float* d_offset, const float* d_mask, int n_img, int h, int w, int g, int kernel_h, int kernel_w,
                         int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, int64_t* d_keys,
                         float* d_weights, void* stream);
int frcnn_ops_dcnv3_backward_input(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                   int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dil_h, int dil_w, float* d_dinput, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_ops_dcnv3_forward_16(int elem_type, const void* d_input, const float* d_offset, const float* d_mask, int n_img, int h, int w,
                               int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                               int dil_w, float offset_scale, void* d_out, void* stream);
int frcnn_ops_dcnv3_backward_offset_16(int elem_type, const void* d_input, const float* d_offset, const float* d_mask, const void* d_dout,
                                       int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, float* d_doffset, float* d_dmask,
                                       void* stream);
int frcnn_ops_dcnv3_backward_input_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                      const void* d_dout, int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h,
                                      int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, void* d_dinput, void* d_ws, size_t ws_bytes,
                                      void* stream);

/* DCNv4, the deformable convolution v4 of the FlashInternImage backbones (csrc/ops_dcnv4.hip): DCNv3's sampling on ONE packed tensor of
 *   offsets and masks, the masks not soft-maxed (unbounded, signed), optionally without the centre point.  Restated from the published
 *   operator (third party, absent here: restated, unpinned; where the two differ this text holds).
 * Tensors: d_input [n][h][w][g gc]; d_offset_mask float32 [n][ho][wo][L], one record for each output pixel, L = ceil(3 g P / 8) 8 =
 *   frcnn_ops_dcnv4_record(g, kernel_h, kernel_w, remove_center) (0 for bad arguments); d_out and d_dout [n][ho][wo][g gc]; ho and wo as for
 *   DCNv3.  The record of pixel (b, oy, ox) holds one slice for each group, at [3 P group, 3 P (group + 1)); inside a slice [2 p, 2 p + 1]
 *   is (dx, dy) of point p and [2 P + p] its mask value.  The last L - 3 g P values of a record are padding: never read (a NaN there
 *   changes nothing), their gradient 0.
 * Points: the grid points are enumerated as DCNv3's, i in [0, kernel_w) along x as the OUTER index and j in [0, kernel_h) along y.
 *   remove_center == 0: P = kernel_h kernel_w and point p is grid point p.  remove_center == 1 (it requires kernel_h == kernel_w, odd,
 *   >= 3): the grid point (kernel_w / 2, kernel_h / 2) is skipped and the later points move down by one, P = kernel_h kernel_w - 1.
 * Sampling: the coordinate of a sample, the test x > -1 && y > -1 && x < w && y < h (a NaN fails), the corners, the weights, the order of
 *   the four-corner sum and the ascending sum over p are exactly DCNv3's above (the integer parts in int, the rest in float32, in pixels
 *   of the unpadded map), by the same kernels: with remove_center == 0 and the same offsets and masks, d_out, d_dinput and the gradient
 *   of every offset and mask value EQUAL DCNv3's bit for bit.
 * frcnn_ops_dcnv4_backward_offset_mask: d_doffset_mask, shaped and laid out as d_offset_mask, every element written exactly once by one
 *   launch: the offset and mask parts by DCNv3's formulas (the right-hand slope at an integer coordinate, 0 for a sample that does not
 *   count), the pad lanes as zeros.  No atomics, a fixed summation order.
 * frcnn_ops_dcnv4_plan + frcnn_ops_dcnv4_backward_input: as DCNv3's, the plan read from the records: entry e = (((b ho wo + oy wo + ox) g_n +
 *   group) P + p) 4 + corner, keys, sentinel and weights as there; the gather is frcnn_ops_msda_backward_value's with P samples an item;
 *   every cell is written; chunking the images changes no bit.  d_ws: frcnn_ops_dcnv4_workspace_bytes(...) bytes, 16-byte aligned.
 * Mapping: DCNv3's, with P samples an item; frcnn_ops_dcnv4_block_items(gc, kernel_h, kernel_w, remove_center, elem_type) is the number of
 *   items (b, oy, ox, group) a block serves for aligned tensors, 0 for arguments out of range.  A block stages its items' slices in LDS
 *   from the records themselves (16-byte loads when d_offset_mask is 16-byte aligned), whether or not it begins or ends inside a record.
 * The _16 forms take float16 / bfloat16 input, dout, out and d_input (elem_type) under the contract of the 16-bit operators above;
 *   offset_mask and its gradient stay float32.
 * Arguments are validated before the GPU is touched (FRCNN_EINVAL): DCNv3's limits with K = P (kernel <= 7, gc <= 256, stride and
 *   dilation in [1, 65536], padding in [0, 65536], ho and wo >= 1, a finite offset_scale, n h w g <= 2^31 - 1025 and n ho wo g P 4 <=
 *   2^31 - 1025), remove_center outside {0, 1}, remove_center == 1 with kernel_h != kernel_w, an even kernel or a kernel below 3, NULL
 *   pointers, a workspace that is NULL, misaligned or too small, an unknown elem_type. */
int frcnn_ops_dcnv4_record(int g, int kernel_h, int kernel_w, int remove_center);
int frcnn_ops_dcnv4_block_items(int gc, int kernel_h, int kernel_w, int remove_center, int elem_type);
size_t frcnn_ops_dcnv4_workspace_bytes(int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w, int remove_center);
int frcnn_ops_dcnv4_forward(const float* d_input, const float* d_offset_mask, int n_img, int h, int w, int g, int gc, int kernel_h,
                            int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale,
                            int remove_center, float* d_out, void* stream);
int frcnn_ops_dcnv4_backward_offset_mask(const float* d_input, const float* d_offset_mask, const float* d_dout, int n_img, int h, int w,
                                         int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                         int dil_h, int dil_w, float offset_scale, int remove_center, float* d_doffset_mask, void* stream);
int frcnn_ops_dcnv4_plan(const float* d_offset_mask, int n_img, int h, int w, int g, int kernel_h, int kernel_w, int stride_h, int stride_w,
                         int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, int remove_center, int64_t* d_keys,
                         float* d_weights, void* stream);
int frcnn_ops_dcnv4_backward_input(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                   int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dil_h, int dil_w, int remove_center, float* d_dinput, void* d_ws,
                                   size_t ws_bytes, void* stream);
int frcnn_ops_dcnv4_forward_16(int elem_type, const void* d_input, const float* d_offset_mask, int n_img, int h, int w, int g, int gc,
                               int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                               float offset_scale, int remove_center, void* d_out, void* stream);
int frcnn_ops_dcnv4_backward_offset_mask_16(int elem_type, const void* d_input, const float* d_offset_mask, const void* d_dout, int n_img,
                                            int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                            int pad_w, int dil_h, int dil_w, float offset_scale, int remove_center, float* d_doffset_mask,
                                            void* stream);
int frcnn_ops_dcnv4_backward_input_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                      const void* d_dout, int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h,
                                      int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int remove_center, void* d_dinput,
                                      void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Final detections.  Replaces models/faster_rcnn.py:179-224 (the numpy float64 decode with
 * stds [.1,.1,.2,.2], clip to [0,H-1]/[0,W-1], score > threshold, per-class
 * torchvision.ops.nms(0.3) on float64 boxes) without the 20 host round trips.
 *   d_props  : float32 [max_rois][4]; d_classes: float32 [max_rois][ncls] (softmax);
 *   d_deltas : float32 [max_rois][(ncls-1)*4]; d_n_rois: device int32
 * Outputs:
 *   d_out    : float64 [(ncls-1)][max_rois][5]  rows (y1,x1,y2,x2,score) in NMS (score-desc) order
 *   d_out_cnt: int32   [(ncls-1)]               rows valid per class (class c -> index c-1)
 * 1 <= max_rois <= 512 and 2 <= ncls <= 128, else FRCNN_EINVAL.  nms_threshold in [0, 1].
 * Image limit: (max(image_h, image_w) - 1) * (1.25 + 5.25 * nms_threshold) <= 8388.608, else FRCNN_EUNSUPPORTED -- sides up to 2970 px
 * at the reference's 0.3 (2165 at 0.5, 1704 at 0.7, 1291 at 1.0, 6711 at 0.0).  Inside it the kernel's float32 pre-filter of the IoU test
 * is proven to agree with the float64 expression (csrc/detect.hip; the derivation is in tests/detection_cases.py); past it the float32
 * rounding of a pair of image-sized boxes can exceed the pre-filter's margin.
 * ---------------------------------------------------------------------------------------- */
int frcnn_detections(const float* d_props, const float* d_classes, const float* d_deltas,
                     const int32_t* d_n_rois, int max_rois, int ncls,
                     int image_h, int image_w, float score_threshold, float nms_threshold,
                     double* d_out, int32_t* d_out_cnt, void* stream);

/* ------------------------------------------------------------------------------------------
 * Context + fused VGG-16 forward.  Replaces FasterRCNNModel.forward
 * (models/faster_rcnn.py:80-132) for the VGG-16 backbone (models/vgg16.py:22-158): one call
 * enqueues every kernel of stage 1-3 on `stream`, no host round trip.
 * One ctx per in-flight image (it owns the activation ping-pong buffers and scratch);
 * a ctx is not re-entrant, different ctxs are independent.  The slab is allocated by
 * frcnn_ctx_create; the V / M scratch of the Winograd layers (FRCNN_MATH_F32_WINOGRAD) is added by the
 * first forward of the ctx that runs in that mode (one hipMalloc, sized for the ctx's largest image:
 * 307 MB at 600x1000) and counted by frcnn_ctx_bytes from then on.
 * ---------------------------------------------------------------------------------------- */
int  frcnn_ctx_create(frcnn_ctx** out, int max_image_h, int max_image_w, int max_rois);
/* A ctx that owns ONLY the proposal scratch (~50 MB: keys, decoded boxes, NMS bit matrix) for the stage-level entry points
 * frcnn_rpn_proposals / frcnn_nms; the fused forwards return FRCNN_EINVAL on it.  Not re-entrant: one per stream. */
int  frcnn_ctx_create_proposals(frcnn_ctx** out, int max_image_h, int max_image_w);
void frcnn_ctx_destroy(frcnn_ctx* ctx);
size_t frcnn_ctx_bytes(const frcnn_ctx* ctx);

typedef struct frcnn_vgg16_weights {
    const float* conv_w[13];   /* [0]: frcnn_pack_conv3x3_c3, [1..12]: frcnn_pack_conv3x3     */
    const float* conv_b[13];
    const float* rpn_conv_w;   /* frcnn_pack_conv3x3 of _rpn_conv1                            */
    const float* rpn_conv_b;
    const float* rpn_head_w;   /* frcnn_pack_stack_rows(_rpn_class, _rpn_boxes) -> [128][512] */
    const float* rpn_head_b;   /* [128]                                                       */
    const float* fc1_w;        /* frcnn_pack_fc_chw_to_hwc(_fc1) [4096][25088]; FRCNN_FC_F32X6T / _F32X3T: its records */
    const float* fc1_b;
    const float* fc2_w;        /* [4096][4096] as stored; FRCNN_FC_F32X6T / _F32X3T: its records */
    const float* fc2_b;
    const float* head_w;       /* frcnn_pack_stack_rows(_classifier, _regressor) -> [128][4096] */
    const float* head_b;       /* [128]                                                       */
    int32_t num_classes;       /* 21 for VOC                                                  */
} frcnn_vgg16_weights;

typedef struct frcnn_forward_params {
    int32_t pre_nms;            /* 6000  (models/faster_rcnn.py:124) */
    int32_t post_nms;           /* 300   (models/faster_rcnn.py:125) */
    float   rpn_nms_threshold;  /* 0.7   (models/rpn.py:150)         */
    float   min_side;           /* 16    (models/rpn.py:142)         */
    int32_t allow_edge_proposals; /* 1   (models/faster_rcnn.py:36)  */
    int32_t math_mode;          /* FRCNN_MATH_F32 (exact f32 MFMA, direct) or FRCNN_MATH_F32_WINOGRAD;
                                   selects how the 3x3 conv weight pointers of the weights struct are interpreted:
                                   FRCNN_MATH_F32: frcnn_pack_conv3x3; FRCNN_MATH_F32_WINOGRAD: layers with
                                   frcnn_conv3x3_uses_winograd_fused(cin, cout) (every 3x3 layer from conv1_2 on, the RPN trunk;
                                   ResNet: frcnn_resnet_block_uses_winograd_fused blocks) frcnn_pack_conv3x3_winograd_fused,
                                   ResNet layer4 blocks with frcnn_resnet_block_uses_winograd: frcnn_pack_conv3x3_winograd,
                                   frcnn_pack_conv3x3 otherwise */
    int32_t conv_blocks_target; /* split-K granularity of the 3x3 layers: blocks per launch to aim for.  0 = 1280 (best
                                   latency for one image on the chip); ~320 when many images are in flight on separate
                                   streams (other images' kernels fill the tail, longer work units win) */
    int32_t fc_math_mode;       /* VGG-16 detector fc1 / fc2: FRCNN_FC_F32 (exact f32 MFMA, fc1_w / fc2_w = float32 matrices), FRCNN_FC_F32X6T or
                                   FRCNN_FC_F32X3T (record operands, see the defines below) */
    int32_t roi_op;             /* FRCNN_ROI_POOL (the reference: torchvision RoIPool, models/detector.py:27) or FRCNN_ROI_ALIGN
                                   (torchvision roi_align semantics, aligned = 0) */
    int32_t roi_sampling_ratio; /* FRCNN_ROI_ALIGN: samples per bin and axis (1 or 2; <= 0 adaptive); ignored for FRCNN_ROI_POOL */
    int32_t winograd_tile_rows; /* three-launch Winograd form only (ResNet layer4): row count of the batched GEMM's block tile.  0 = 64 (64 x 128 tiles, five
                                   blocks per CU: best latency for one image on the chip); 128 with many images in flight (the chip
                                   is then at its power limit and the tile with fewer operand bytes per MFMA wins) */
    int32_t winograd_x6_mask;   /* FRCNN_MATH_F32_WINOGRAD only: bit i set = 3x3 layer i runs as an x6 Winograd layer (csrc/wino_x6.hip: the position
                                   GEMMs in the f32x6 arithmetic on the bf16 pipe) and its weight pointer is frcnn_pack_conv3x3_winograd_x6's record bank.
                                   VGG-16: bit i = conv_w[i] (1 .. 12: conv1_2 .. conv5_3), bit 13 = the RPN trunk.  ResNet: bit 13 = the RPN trunk only.
                                   A set bit on a layer with frcnn_conv3x3_uses_winograd_x6(cin, cout) == 0 is FRCNN_EINVAL.  0 = rounds 1-2's behaviour */
    int32_t x6_gemm_tiles;      /* block tile of the x6 Winograd layers' batched GEMM (csrc/gemm_x6t.hip): 0 = chosen per shape by the cost model (best
                                   latency for one image on the chip: 320 x 256 tiles, one 8-wave block per CU, where they cover the chip in one
                                   round), 1 = 320 x 256 always, 2 = 160 x 128 always (4-wave blocks that leave registers and LDS for a second kernel on
                                   the CU: with several images in flight the transforms, epilogues and proposal kernels of the other images then
                                   overlap the GEMM -- measured +3..8 % images/sec at 3 images in flight) */
    int32_t winograd_x3_mask;   /* a subset of winograd_x6_mask (VGG-16): the layers whose position GEMMs run in the f32x3 arithmetic instead (two
                                   fp16 terms per row-scaled operand, three MFMAs per product: csrc/wino_x3.hip); their weight pointers are
                                   frcnn_pack_conv3x3_winograd_x3's blobs.  ResNet: 0 */
    int32_t winograd_x3f_mask;  /* round 4 (ABI 9), VGG-16, FRCNN_MATH_F32_WINOGRAD only: bit i set = 3x3 layer i (1 = conv1_2 .. 12, 13 = the RPN trunk; disjoint from
                                   winograd_x6_mask) runs as a ONE-LAUNCH Winograd layer in the f32x3 arithmetic (csrc/wino_x3f.hip: operand formed in
                                   registers from the LDS-staged halo, filter fragments straight from L2, all 16 positions in accumulators, no V / M
                                   scratch; the three-launch f32x3 layer's arithmetic up to the rounding order of the output transform) and its weight
                                   pointer is frcnn_pack_conv3x3_winograd_x3's blob.  For the layers whose V + M scratch does not fit the Infinity
                                   Cache (conv2_1 .. conv3_3) and, when several images are in flight and the chip is full anyway, for the 512-channel
                                   layers too (one launch instead of three, no scratch traffic).  cin % 32 == 0, cout % 64 == 0 */
} frcnn_forward_params;
#define FRCNN_X6_RPN_TRUNK_BIT 13
/* capacity of the detector heads: classifier (n) + regressor (4 n - 4) rows are stacked into one zero-padded GEMM operand of
 * ceil((5 n - 4) / 128) * 128 rows (head_w / head_b of the weight structs), at most FRCNN_HEAD_LD_MAX */
#define FRCNN_HEAD_LD_MAX 512
#define FRCNN_MAX_NUM_CLASSES 103
#define FRCNN_MATH_F32   0
/* (1 was FRCNN_MATH_F32X6, the direct f32x6 convolution of round 2: removed in ABI 13) */
#define FRCNN_MATH_F32_WINOGRAD 2
#define FRCNN_ROI_POOL  0
#define FRCNN_ROI_ALIGN 1
#define FRCNN_FC_F32   0
/* (1 was FRCNN_FC_F32X6, round 2's chunk-major-record kernel: removed in ABI 13) */
#define FRCNN_FC_F32X6T 2     /* the f32x6 arithmetic (three bf16 terms per operand, six MFMAs per product) on csrc/gemm_x6t.hip (fc1_w / fc2_w = frcnn_split_rows_x6t records of the
                                 same matrices, rows padded to FRCNN_X6T_COL_TILE; any number of RoIs the ctx holds) */
#define FRCNN_FC_F32X3T 3     /* the f32x3 arithmetic on csrc/gemm_x3t.hip (two fp16 terms per row-scaled operand, three MFMAs per product):
                                 fc1_w / fc2_w = frcnn_pack_rows_x3t blobs of the same matrices (rows_padded = 4096) */

/* d_image: float32 NCHW [3][H][W] (preprocessed as models/vgg16.py:146 prescribes).
 * d_anchor_map / d_valid_map: optional caller-provided maps (faster_rcnn.py:113-115); NULL =
 * generate (and cache per shape) inside the ctx.
 * Outputs (device, caller-owned): d_props [post_nms][4], d_classes [post_nms][ncls],
 * d_deltas [post_nms][(ncls-1)*4], d_counts int32[4] as in frcnn_rpn_proposals. */
int frcnn_vgg16_forward(frcnn_ctx* ctx, const frcnn_vgg16_weights* w, const frcnn_forward_params* p,
                        const float* d_image, int H, int W,
                        const float* d_anchor_map, const float* d_valid_map,
                        float* d_props, float* d_classes, float* d_deltas, int32_t* d_counts,
                        void* stream);

/* Fused ResNet forward: FasterRCNNModel.forward (models/faster_rcnn.py:80-132) for the
 * ResNet-50/101/152 backbones (models/resnet.py:131-185): feature map [ceil(H/16)][ceil(W/16)][1024],
 * RPN on 1024 channels, RoIPool 7x7, layer4 per RoI + spatial mean -> 2048, heads. */
#define FRCNN_RESNET_MAX_BLOCKS 64
typedef struct frcnn_bottleneck_weights {
    const float *w1, *b1;      /* 1x1 cin->width    (bn folded), [1][width][cin]   */
    const float *w2, *b2;      /* 3x3 width->width, stride on this conv (v1.5), [9][width][width]; in math mode
                                  FRCNN_MATH_F32_WINOGRAD the blocks with frcnn_resnet_block_uses_winograd(width, stride)
                                  carry frcnn_pack_conv3x3_winograd's [16][width][width] instead */
    const float *w3, *b3;      /* 1x1 width->cout, [1][cout][width] */
    const float *wd, *bd;      /* downsample 1x1 cin->cout (stride), NULL when identity */
    int32_t cin, width, cout, stride;
    int32_t x6_mask;           /* round 3: bit 0 / 1 / 2 set = w1 / w3 / wd is NOT a float32 pack but the x6t record array of the folded
                                  [cout][cin] matrix (frcnn_split_rows_x6t, rows padded to FRCNN_X6T_COL_TILE): that 1x1 convolution runs as a
                                  GEMM in the f32x6 arithmetic on the bf16 pipe (csrc/gemm_x6t.hip; the activations are split on the fly by
                                  frcnn_split_pixels_x6t).  Needs cin % 16 == 0 and cout % 4 == 0; FRCNN_MATH_F32_WINOGRAD only */
    int32_t x3_mask;           /* a subset of x6_mask: those convolutions run in the f32x3 arithmetic instead (csrc/gemm_x3t.hip, csrc/wino_x3.hip) and
                                  their weight pointers are f32x3 blobs: frcnn_pack_rows_x3t of the [cout][K] matrix (1x1 and stride-2 3x3
                                  convolutions), frcnn_pack_conv3x3_winograd_x3's blob (stride-1 3x3) */
    const float* wmax;         /* round 4 (ABI 11), with g3 != 0: device float[4] = max |w1|, |w2|, |w3|, |wd| of the packs (upper bounds; [3] unused without wd) */
    int32_t g3;                /* != 0 (2, ABI 15: w1 / w2 / w3 / wd are frcnn_pack_conv_x3g_weights images of the float32 packs, same results): the block's four convolutions run in the f32x3 arithmetic under ONE scale per tensor (frcnn_conv_nhwc_x3g's kernel,
                                  csrc/conv_gather.hip): w1 / w2 / w3 / wd are the plain float32 packs ([1][width][cin], [9][width][width], ...) whatever the
                                  math mode, x6_mask must be 0.  The activation maxima travel from one convolution's epilogue to the next one's scale inside
                                  the context.  Reference: the same Bottleneck forward, models/resnet.py:38-46 / :66-90 */
    int32_t reserved0;
} frcnn_bottleneck_weights;
#define FRCNN_X6_CONV1 1
#define FRCNN_X6_CONV3 2
#define FRCNN_X6_DOWN  4
#define FRCNN_X6_CONV2 8     /* w2 = x6t records: stride 1 -> frcnn_pack_conv3x3_winograd_x6's bank (an x6 Winograd layer over the block's maps),
                                stride 2 -> the records of the folded [cout][9 cin] matrix (tap-major columns; an im2col GEMM) */

typedef struct frcnn_resnet_weights {
    const float* stem_w;       /* [147][64] */
    const float* stem_b;
    int32_t n_blocks[4];       /* layer1..layer4: (3,4,6,3) / (3,4,23,3) / (3,8,36,3) */
    frcnn_bottleneck_weights blocks[FRCNN_RESNET_MAX_BLOCKS];   /* layer1, layer2, layer3, layer4 in order */
    const float* rpn_conv_w;   /* frcnn_pack_conv3x3 (FRCNN_MATH_F32) / frcnn_pack_conv3x3_winograd (FRCNN_MATH_F32_WINOGRAD) of
                                  _rpn_conv1 (1024 -> 1024) */
    const float* rpn_conv_b;
    const float* rpn_head_w;   /* [128][1024] */
    const float* rpn_head_b;
    const float* head_w;       /* [128][2048] */
    const float* head_b;
    int32_t num_classes;
} frcnn_resnet_weights;

int frcnn_resnet_forward(frcnn_ctx* ctx, const frcnn_resnet_weights* w, const frcnn_forward_params* p,
                         const float* d_image, int H, int W,
                         const float* d_anchor_map, const float* d_valid_map,
                         float* d_props, float* d_classes, float* d_deltas, int32_t* d_counts,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * One in-flight image, submitted natively (round 7; additions within ABI 21).
 *
 * The packed output block of a slot: the three results the host reads after an image, as regions of ONE device allocation with ONE
 * pinned host mirror of the same layout, so that one hipMemcpyAsync brings them back:
 *   [FRCNN_OUT_COUNTS]  int32 [4]                          d_counts of the forward                      offset 0
 *   [FRCNN_OUT_DET_CNT] int32 [(ncls-1)]                   d_out_cnt of frcnn_detections
 *   [FRCNN_OUT_DET]     float64 [(ncls-1)][max_rois][5]    d_out of frcnn_detections
 * Every region starts on a 16-byte boundary (the float64 rows are therefore 8-byte aligned).  frcnn_output_block_layout writes the three
 * byte offsets and the block's size; no GPU needed. */
#define FRCNN_OUT_COUNTS  0
#define FRCNN_OUT_DET_CNT 1
#define FRCNN_OUT_DET     2
int frcnn_output_block_layout(int max_rois, int ncls, size_t offsets[3], size_t* total_bytes);

/* Do two streams of this process share a hardware queue?  A process has GPU_MAX_HW_QUEUES in-order hardware queues (HIP's default: 4), and
 * the runtime hands a new stream the least-used one once they are all taken; the default stream holds one.  Two in-flight slots whose streams
 * land on one queue run their images one behind the other.  The runtime does not say where a stream went, so this
 * measures it: a ~200 us wait kernel on stream_a, then an event on stream_b; *shared = 1 when that event completed only behind the kernel.
 * Synchronises both streams; a few hundred microseconds, meant for set-up (runtime.slot_stream), never for the per-image path. */
int frcnn_streams_share_queue(void* stream_a, void* stream_b, int* shared);

/* Makes `stream` wait for the work enqueued so far on `producer` -- only when there is some.  hipStreamQuery(producer) == hipSuccess:
 * everything enqueued there has completed, what it produced is in memory, and NOTHING is recorded on the producer (counted as skipped).
 * hipErrorNotReady: an event of the ctx's ring (created once, on first use) is recorded on the producer and `stream` waits for it, as
 * torch's Stream.wait_stream does (counted as taken).  Any other code is returned as FRCNN_EHIP.  producer == stream: nothing to do, not counted.
 * The decision is taken on the host at the time of the call; work enqueued on the producer afterwards is not covered (nor was it by
 * wait_stream).  Why it matters: a process has GPU_MAX_HW_QUEUES in-order hardware queues; with as many slot streams as queues, the
 * producer (usually the default stream) shares a queue with one slot's stream, and an event recorded on it sits behind the whole image
 * that slot has already enqueued -- every submission then waits for another slot's image for nothing.
 * Must not be called while either stream is capturing. */
int frcnn_stream_depend(frcnn_ctx* ctx, void* producer, void* stream);

/* dependencies taken / skipped by frcnn_stream_depend and frcnn_predict_submit on this ctx since it was created */
int frcnn_ctx_submit_stats(const frcnn_ctx* ctx, int64_t* taken, int64_t* skipped);

/* Everything of one image on the slot's stream, in one call: [frcnn_stream_depend(producer, stream) if depend != 0] ->
 * frcnn_vgg16_forward (backbone 0, `weights` = frcnn_vgg16_weights*) or frcnn_resnet_forward (backbone 1, frcnn_resnet_weights*) ->
 * [frcnn_detections if with_detections != 0] -> ONE device-to-host copy of the packed block -> [hipEventRecord(done_event, stream) if
 * done_event].  The launches, their order and their arguments are those of the separate calls: d_counts, d_out_cnt and d_out are the
 * regions of d_block (frcnn_output_block_layout(max_rois, weights->num_classes)), h_block is pinned host memory of the same size.
 * Without detections only the counts region is copied.  Inside a stream capture: depend = 0 and done_event = NULL (a stream query is not
 * allowed on a capturing stream); the caller takes the dependency with frcnn_stream_depend before it replays the graph. */
int frcnn_predict_submit(frcnn_ctx* ctx, int backbone, const void* weights, const frcnn_forward_params* p,
                         const float* d_image, int H, int W, const float* d_anchor_map, const float* d_valid_map,
                         float* d_props, float* d_classes, float* d_deltas, void* d_block, void* h_block, int max_rois,
                         int with_detections, float score_threshold, float nms_threshold,
                         int depend, void* producer, void* stream, void* done_event);

/* The same forward in two calls, for a true batch of images (BASELINE configs[2] "batch=8"; the reference asserts batch 1 at
 * models/faster_rcnn.py:108, SURVEY 8b allows lifting it):
 *   frcnn_resnet_backbone          conv1 / bn1 / relu / maxpool / layer1..3 (models/resnet.py:38-46) over n_images images
 *                                  [n][3][H][W] -> d_features [n][fh][fw][1024] (NHWC float32) with EVERY bottleneck launch covering
 *                                  the n maps: the 1x1 convolutions become GEMMs over n * h * w pixels (one map of 38 x 63 fills 38
 *                                  tiles of a 256-CU chip).  ctx: frcnn_ctx_create_backbone(max_h, max_w, max_images) -- only the
 *                                  activation rotation and the gather kernel's split-K scratch (the fused forwards refuse it) -- or any
 *                                  full ctx with n_images == 1.
 *   frcnn_resnet_forward_features  RPN + RoI pooling + layer4 + heads (models/faster_rcnn.py:116-132) of ONE image from its feature
 *                                  map (copied into the ctx's own map unless it already is frcnn_ctx_tensor(ctx, 0)); H, W = the image's
 *                                  size as in frcnn_resnet_forward.
 * frcnn_resnet_forward(image) == frcnn_resnet_backbone(1 image) + frcnn_resnet_forward_features bit for bit; with n > 1 the split-K
 * factors of the under-filled GEMMs differ (fewer splits are needed), so feature maps agree to float32 rounding (~1e-6 relative),
 * deterministically. */
int frcnn_ctx_create_backbone(frcnn_ctx** out, int max_image_h, int max_image_w, int max_images);
int frcnn_resnet_backbone(frcnn_ctx* ctx, const frcnn_resnet_weights* w, const frcnn_forward_params* p,
                          const float* d_images, int n_images, int H, int W, float* d_features, void* stream);
int frcnn_resnet_forward_features(frcnn_ctx* ctx, const frcnn_resnet_weights* w, const frcnn_forward_params* p,
                                  const float* d_feature_map, int H, int W,
                                  const float* d_anchor_map, const float* d_valid_map,
                                  float* d_props, float* d_classes, float* d_deltas, int32_t* d_counts,
                                  void* stream);
/* The same tail in THREE calls (round 6, ABI 14): frcnn_resnet_rpn_roipool = RPN + proposals + RoI pooling (models/rpn.py:88-153, detector.py:65-72) of ONE
 * image from its feature map, into d_roi_out = that image's slice [post_nms][7][7][C] of a batch buffer (its own ctx and stream, as
 * frcnn_resnet_forward_features); frcnn_resnet_head = layer4 + spatial mean + classifier / regressor (models/resnet.py:109-118, detector.py:75-78) over the
 * n_rois pooled RoIs of ALL images in one set of launches (ctx: frcnn_ctx_create_head(max_rois_total)): d_classes [n_rois][num_classes],
 * d_deltas [n_rois][4 (num_classes - 1)].  Rows are independent of each other; with the per-tensor-scaled f32x3 blocks (frcnn_bottleneck_weights.g3)
 * the scales are those of the batch, so a batch's rows differ from the per-image call's at the rounding level (as frcnn_resnet_backbone's). */
int frcnn_resnet_rpn_roipool(frcnn_ctx* ctx, const frcnn_resnet_weights* w, const frcnn_forward_params* p, const float* d_feature_map, int H,
                             int W, const float* d_anchor_map, const float* d_valid_map, float* d_props, int32_t* d_counts, float* d_roi_out,
                             void* stream);
int frcnn_ctx_create_head(frcnn_ctx** out, int max_rois_total);
int frcnn_resnet_head(frcnn_ctx* ctx, const frcnn_resnet_weights* w, const frcnn_forward_params* p, float* d_rois, int n_rois, float* d_classes,
                      float* d_deltas, void* stream);

/* ==========================================================================================
 * Training path (SURVEY.md section 8 rows f2 + f3): FasterRCNNModel.train_step,
 * models/faster_rcnn.py:228-362.  The reference relies on autograd over cuDNN/cuBLAS; here every
 * backward operator is an explicit entry point and fasterrcnn_amd/models/faster_rcnn.py chains them.
 * All arithmetic is float32 on the exact-f32 matrix pipe; loss sums are float64, rounded once.
 * ======================================================================================== */

/* models/faster_rcnn.py:421-510 _label_proposals.  Rows 0..n_props-1 are the RPN proposals
 * (n_props read from the device, clamped to max_props), followed by the n_gt ground-truth boxes
 * (:433).  For every row whose best IoU >= min_background_iou (order preserved, :476-480):
 *   d_out_props         float32 [K][4]
 *   d_out_class_idx     int32   [K]       0 = background (best IoU < min_object_iou, :483)
 *   d_out_gt_classes    float32 [K][num_classes]            one-hot (:486-488)
 *   d_out_gt_box_deltas float32 [K][2][4*(num_classes-1)]   [:,0,:] mask, [:,1,:] (ty,tx,th,tw) tiled (:497-510)
 *   d_out_count         int32   K
 * Output buffers hold max_props + n_gt rows.  IoU as math_utils.py:39-63 in float32 (eps 1e-7). */
int frcnn_label_proposals(const float* d_props, const int32_t* d_n_props, int max_props,
                          const float* d_gt_boxes, const int32_t* d_gt_class_idx, int n_gt, int num_classes,
                          float min_background_iou, float min_object_iou,
                          const float box_delta_means[4], const float box_delta_stds[4],
                          float* d_out_props, int32_t* d_out_class_idx, float* d_out_gt_classes,
                          float* d_out_gt_box_deltas, int32_t* d_out_count, void* stream);

/* dst[i][:] = src[idx[i]][:] -- the index selects of faster_rcnn.py:557-561 (_sample_proposals; the
 * random permutation itself is drawn on the host exactly as the reference draws it). */
int frcnn_gather_rows(const float* d_src, const int32_t* d_idx, int n, int row_floats, float* d_dst, void* stream);

/* models/rpn.py:176-272 class_loss + regression_loss over the anchor mini-batch, and the gradient of
 * (class_loss + regression_loss) with respect to the RPN head output.
 *   d_head    float32 [cells][ld_head]: [9 objectness logits | 36 box deltas | pad] per feature-map cell
 *   d_sample  int32 [n_sample]: flat anchor indices (y*fw + x)*9 + k marked trainable by
 *             faster_rcnn.py:364-419 _sample_rpn_minibatch (no duplicates)
 *   d_rpn_map float32 [A][6] (trainable, object, ty, tx, th, tw)  (frcnn_rpn_targets layout)
 *   d_losses  float32 [2] = (class, regression);  d_grad_head [cells][ld_head] or NULL (fully written). */
int frcnn_rpn_loss(const float* d_head, int ld_head, int cells, const int32_t* d_sample, int n_sample,
                   const float* d_rpn_map, float* d_losses, float* d_grad_head, void* stream);

/* models/detector.py:83-155 class_loss + regression_loss and the gradient with respect to the stacked
 * head output [class logits (num_classes) | regressor outputs (4*(num_classes-1)) | pad to ld_grad].
 *   d_classes [n][num_classes] softmax output, d_deltas [n][4*(num_classes-1)],
 *   d_gt_classes / d_gt_box_deltas as produced by frcnn_label_proposals. */
int frcnn_detector_loss(const float* d_classes, const float* d_deltas, const float* d_gt_classes,
                        const float* d_gt_box_deltas, int n, int num_classes, float* d_losses,
                        float* d_grad_logits, int ld_grad, void* stream);

/* C[m][n] = sum_r A[r][m] * B[r][n]  (m < M, n < N, r < R): autograd's linear backward
 * (weight gradient dY^T X; data gradient with A = dY^T).  lda, ldb multiples of 4, ldc even,
 * A/B 16-byte aligned; rows may be read up to their leading dimension.  Deterministic split-R
 * through d_ws (frcnn_gemm_tn_workspace_bytes; NULL = no split). */
size_t frcnn_gemm_tn_workspace_bytes(int M, int N, int R);
int frcnn_gemm_tn(const float* d_a, int lda, const float* d_b, int ldb, float* d_c, int ldc,
                  int M, int N, int R, void* d_ws, size_t ws_bytes, void* stream);

/* The reduced-precision train step (BASELINE configs[4]; the reference trains in float32: faster_rcnn.py:355, so this is
 * beyond it): the same three gradient GEMMs with `grad_math`
 *   FRCNN_GRAD_F32  : the entry points without the suffix (exact-f32 matrix pipe)
 *   FRCNN_GRAD_BF16 : both operands rounded to bfloat16 (round to nearest even) on their way to the bf16 matrix pipe, float32
 *                     accumulation; result = f32 GEMM of the rounded operands up to the accumulation order
 *                     (oracle/train_oracle.py grad_math="bf16").  Operand arrays < 4 GiB.
 * Workspace sizes: the functions without the suffix cover both. */
#define FRCNN_GRAD_F32  0
#define FRCNN_GRAD_BF16 1
int frcnn_gemm_tn_math(const float* d_a, int lda, const float* d_b, int ldb, float* d_c, int ldc,
                       int M, int N, int R, int grad_math, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_conv3x3_wgrad_math(const float* d_x, const float* d_dz, float* d_dwp, int H, int W, int cin, int cout,
                             int grad_math, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_conv_wgrad_math(const float* d_x, const float* d_dz, float* d_dwp, int N, int H, int W, int cin, int cout,
                          int ksize, int stride, int pad, int grad_math, void* d_ws, size_t ws_bytes, void* stream);
/* ABI 10: the FORWARD and DATA-GRADIENT convolutions of the ResNet train step (models/faster_rcnn.py:228-362 train_step over the Bottleneck
 * convolutions of models/resnet.py:38-46,110 and their autograd backward) with the same switch (BASELINE configs[4] as written:
 * "train step ... bf16"): frcnn_conv_nhwc / frcnn_conv_dgrad with `math` = FRCNN_GRAD_BF16 round both operands (activations or output
 * gradients, and the folded weight pack) to bfloat16 on their way into LDS and multiply on the bf16 matrix pipe (one
 * v_mfma_f32_32x32x16_bf16 per 16-channel stage where the float32 kernel issues eight float32 instructions), float32 accumulation,
 * bias / residual / ReLU in float32; master weights and every stored tensor stay float32.  Same arguments, shapes and workspace as the
 * entry points without the suffix. */
int frcnn_conv_nhwc_math(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual, float* d_y,
                         int N, int H, int W, int cin, int cout, int ksize, int stride, int pad, unsigned flags, int math,
                         void* d_ws, size_t ws_bytes, void* stream);
int frcnn_conv_dgrad_math(const float* d_dz, const float* d_wd, const float* d_residual, float* d_dx, int N, int H, int W,
                          int cin, int cout, int ksize, int stride, int pad, int math, void* d_ws, size_t ws_bytes, void* stream);

/* ABI 16: the backward of ONE trainable Bottleneck (models/resnet.py:38-46 with frozen BatchNorm folded into the convolutions; the reference
 * gets it from autograd: pytorch/FasterRCNN/__main__.py:147-152 `loss.total.backward()`) as one call instead of ~25:
 *   out = relu(conv3(t2) + identity), t2 = relu(conv2(t1)), t1 = relu(conv1(x)), identity = x or downsample(x)
 * d_g = dL/d out on entry (overwritten: the ReLU mask of `out` is applied in place).  Writes, per convolution, the gradient of its RAW
 * weight (the folded weight's gradient x the BatchNorm scale of the output channel) into frcnn_train_conv.grad, and, if d_dx is not NULL,
 * dL/dx.  d_dt2 [N][Ho][Wo][width], d_dt1 [N][H][W][width], d_dxid [N][H][W][cin] (downsample blocks) are scratch the caller owns;
 * frcnn_train_conv.wd is the convolution's data-gradient pack scratch ([k k][cin][cout] floats).  The chain ReLU mask -> data gradient ->
 * ReLU mask ... runs on `stream`; the four weight gradients (GEMM + split reduction + row scale) run on `side_stream` behind ONE event
 * recorded on `stream` after the chain (NULL: on `stream` too, each before its data gradient) -- they execute under the next block's
 * chain, and the caller orders whatever reads the gradients, or frees the scratch, behind `side_stream`.  The values are those
 * of the separate entry points (frcnn_relu_backward, frcnn_conv_wgrad_math + frcnn_scale_rows, frcnn_pack_conv_dgrad + frcnn_conv_dgrad_math)
 * bit for bit.  (H, W): the block input's size; (Ho, Wo): its output's (stride of conv2 / downsample).  math: FRCNN_GRAD_F32 / _BF16. */
typedef struct frcnn_train_conv {
    const float* folded;   /* [k k][cout][cin]: W x BN scale (what the forward convolves with) */
    const float* scale;    /* [cout] BatchNorm scale gamma / sqrt(var + eps) */
    float* grad;           /* out: [k k][cout][cin] gradient of the raw weight */
    float* wd;             /* scratch: [k k][cin][cout] */
    int32_t cin, cout, ksize, stride, pad, reserved0;
} frcnn_train_conv;
int frcnn_bottleneck_backward_workspace_bytes(const frcnn_train_conv* c1, const frcnn_train_conv* c2, const frcnn_train_conv* c3,
                                              const frcnn_train_conv* cd, int N, int H, int W, int Ho, int Wo, size_t* main_bytes,
                                              size_t* side_bytes);
int frcnn_bottleneck_backward(const frcnn_train_conv* c1, const frcnn_train_conv* c2, const frcnn_train_conv* c3, const frcnn_train_conv* cd,
                              const float* d_x, const float* d_t1, const float* d_t2, const float* d_out, float* d_g, float* d_dt2,
                              float* d_dt1, float* d_dxid, float* d_dx, int N, int H, int W, int Ho, int Wo, int math, void* d_ws_main,
                              size_t ws_main_bytes, void* d_ws_side, size_t ws_side_bytes, void* stream, void* side_stream);

/* ABI 11: the same convolution (frcnn_conv_nhwc: the frozen-BN Bottleneck convolutions of models/resnet.py:38-46, BN folded) in the f32x3
 * arithmetic under ONE power-of-two scale per tensor: every activation and weight value as two fp16 terms hi = fp16(v 2^e),
 * lo = fp16(v 2^e - hi) with max|tensor| 2^e in [2^14, 2^15), split on the way into LDS, three v_mfma_f32_32x32x16_f16 per product,
 * float32 accumulation, bias / residual / ReLU in float32.  About 22 bits per value relative to the value itself down to 2^-14 of the
 * tensor maximum, 2^-38 of the maximum absolute below.
 *   d_xmax, d_wmax : device floats, UPPER BOUNDS of max|x| and max|w_packed| (a bound below the true maximum overflows fp16 -> inf)
 *   d_ymax         : NULL, or a device float that receives max(*d_ymax, max|y|) by atomic maximum -- zero it (or leave an older maximum)
 *                    before the call; it is the next convolution's d_xmax
 * Other arguments, shapes and workspace (frcnn_conv_workspace_bytes) as frcnn_conv_nhwc. */
int frcnn_conv_nhwc_x3g(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual, float* d_y,
                        int N, int H, int W, int cin, int cout, int ksize, int stride, int pad, unsigned flags,
                        const float* d_xmax, const float* d_wmax, float* d_ymax, void* d_ws, size_t ws_bytes, void* stream);
/* ABI 15: the same call with the split reduction of a small convolution finished INSIDE the kernel, by the last block of every output tile
 * to arrive (round 6: what frcnn_resnet_forward / frcnn_resnet_backbone run; frcnn_conv_nhwc_x3g keeps the separate finishing pass).
 *   d_tile_counters : FRCNN_X3G_TILE_COUNTERS unsigned ints, ZERO before the first call; every call leaves them zero again.  They
 *                     belong to one stream at a time (two convolutions in flight on different streams need two arrays).
 * The partial planes are summed in ascending order like the separate pass: the results are the same bits (tests/test_conv_x3g_gpu.py).
 * Launches whose tile count exceeds the array, and launches that do not split, behave as frcnn_conv_nhwc_x3g. */
#define FRCNN_X3G_TILE_COUNTERS 16384
int frcnn_conv_nhwc_x3g_tickets(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual, float* d_y,
                                int N, int H, int W, int cin, int cout, int ksize, int stride, int pad, unsigned flags,
                                const float* d_xmax, const float* d_wmax, float* d_ymax, void* d_ws, size_t ws_bytes,
                                unsigned* d_tile_counters, void* stream);
/* ABI 15: the weight side of frcnn_conv_nhwc_x3g split ONCE, at pack time.  d_out (taps * cout * cin * 4 bytes, the size of the float32 pack
 * [taps][cout][cin]) receives every row in the kernel's own operand format -- per 32 input channels 128 bytes: [hi x 16 | lo x 16] fp16 of channels
 * 0..15, then of 16..31, hi = fp16(w 2^e), lo = fp16(w 2^e - hi) under the scale that *d_wmax gives -- so that a weight piece is a 16-byte copy
 * into LDS in every block of every launch instead of a split.  Pass it as d_w_packed with FRCNN_X3G_WSPLIT in `flags` (and the SAME d_wmax):
 * the results are the same bits as with the float32 pack.  cin % 32 == 0.  frcnn_bottleneck_weights.g3 == 2: the block's four packs are such images. */
int frcnn_pack_conv_x3g_weights(const float* d_w_packed, const float* d_wmax, void* d_out, int taps, int cout, int cin, void* stream);
/* ABI 12: frcnn_conv_nhwc_x3g CLAMPS an activation whose hi term would overflow fp16 under the tensor's scale (i.e. *d_xmax was not an
 * upper bound) instead of producing inf / NaN; every wave that clamped one adds 1 to a process-wide counter.  *out = that count since the
 * library was loaded (read it after synchronising the streams the convolutions ran on).  With the maxima the producers' epilogues leave
 * behind (frcnn_resnet_forward / frcnn_resnet_backbone chain them) the count stays 0: tests/test_stress_gpu.py asserts it on inputs built
 * against the per-tensor scale (models/resnet.py:38-46 has no such notion: its float32 convolutions cannot overflow). */
int frcnn_x3_saturation_events(unsigned long long* out);

/* d_out[0] = max(d_out[0], max_i |d_x[i]|), n floats, d_x 16-byte aligned (the scale source of a tensor no frcnn_conv_nhwc_x3g produced) */
int frcnn_tensor_absmax(const float* d_x, long long n, float* d_out, void* stream);

/* conv2d backward of the 3x3 "same" layers (vgg16.py:76-96, rpn.py:88):
 *   weight gradient  d_dwp [9][cout][cin] (the frcnn_pack_conv3x3 layout) from x [H][W][cin], dz [H][W][cout];
 *   data gradient    dx = frcnn_conv3x3_nhwc(dz, frcnn_pack_conv3x3_dgrad(wp), zero bias, flags 0). */
size_t frcnn_conv3x3_wgrad_workspace_bytes(int H, int W, int cin, int cout);
int frcnn_conv3x3_wgrad(const float* d_x, const float* d_dz, float* d_dwp, int H, int W, int cin, int cout,
                        void* d_ws, size_t ws_bytes, void* stream);
int frcnn_pack_conv3x3_dgrad(const float* d_wp, float* d_wd, int cout, int cin, void* stream);

/* General forms for the ResNet bottlenecks (models/resnet.py:38-46,110; BatchNorm frozen, so each conv+BN is one conv with a
 * folded weight): x [N][H][W][cin], y = conv(x) [N][Ho][Wo][cout], k x k taps, stride, pad.
 *   frcnn_conv_wgrad : d_dwp [k*k][cout][cin] = gradient with respect to the (folded) weight pack
 *   frcnn_conv_dgrad : d_dx [N][H][W][cin] = d_residual (or 0 if NULL) + gradient with respect to x, from d_dz [N][Ho][Wo][cout]
 *                      and d_wd = frcnn_pack_conv_dgrad(weight pack) ([tap][cin][cout]); cout % 16 == 0, cin % 4 == 0
 *   frcnn_scale_rows : dst[tap][co][ci] = src[tap][co][ci] * scale[co] (fold a frozen BN scale into a pack; chain rule back)
 *   frcnn_bn_scale_shift : scale = gamma / sqrt(var + eps), shift = beta - mean * scale (the eval-mode BatchNorm affine)
 *   frcnn_spatial_mean_backward : backward of `y.mean(-1).mean(-1)` (resnet.py:117). */
size_t frcnn_conv_wgrad_workspace_bytes(int N, int H, int W, int cin, int cout, int ksize, int stride, int pad);
int frcnn_conv_wgrad(const float* d_x, const float* d_dz, float* d_dwp, int N, int H, int W, int cin, int cout,
                     int ksize, int stride, int pad, void* d_ws, size_t ws_bytes, void* stream);
size_t frcnn_conv_dgrad_workspace_bytes(int N, int H, int W, int cin, int cout, int ksize, int stride, int pad);
int frcnn_conv_dgrad(const float* d_dz, const float* d_wd, const float* d_residual, float* d_dx, int N, int H, int W,
                     int cin, int cout, int ksize, int stride, int pad, void* d_ws, size_t ws_bytes, void* stream);
int frcnn_pack_conv_dgrad(const float* d_wp, float* d_wd, int taps, int cout, int cin, void* stream);
int frcnn_scale_rows(const float* d_src, const float* d_scale, float* d_dst, int taps, int cout, int cin, void* stream);
int frcnn_bn_scale_shift(const float* d_gamma, const float* d_beta, const float* d_mean, const float* d_var, float eps,
                         int c, float* d_scale, float* d_shift, void* stream);
int frcnn_spatial_mean_backward(const float* d_dy, float* d_dx, int N, int H, int W, int c, void* stream);

/* dy[i] = y[i] > 0 ? dy[i] : 0 (ReLU backward, in place); a[i] += b[i]. */
int frcnn_relu_backward(float* d_dy, const float* d_y, size_t n, void* stream);
int frcnn_add_inplace(float* d_a, const float* d_b, size_t n, void* stream);
/* ABI 17: nn.Dropout(p) in training mode (models/vgg16.py:129-133 with `--dropout p`), in place on n floats (d_x 16-byte aligned):
 *   keep[i] = (w >> 8) * 2^-24 < 1 - p (float32), w = word (i & 3) of Philox4x32-10 with key (seed lo32, seed hi32) and counter
 *             (i >> 2 lo32, i >> 2 hi32, stream_id, rank), seed = *d_seed (device memory: drawing it needs no host synchronisation);
 *   x[i]    = keep[i] ? x[i] * scale : 0, scale = (float)(1.0 / (1.0 - p)) computed in double by the caller.
 * p == 0 leaves x untouched, p == 1 zeroes it.  d_keep_out: NULL, or n bytes that receive keep[i] as 0 / 1 (tests).
 * FRCNN_EINVAL: p outside [0, 1] or NaN, scale not finite or below 1 while p < 1, d_x / d_seed NULL while n > 0, d_x misaligned.
 * frcnn_dropout_relu_backward: dy[i] = y[i] > 0 ? dy[i] * scale : 0 in place, y = the output of relu followed by frcnn_dropout: the
 * gradient of dropout(relu(z)) with respect to z without a stored mask (y > 0 exactly on kept elements with relu(z) > 0).
 * scale >= 1 (else FRCNN_EINVAL); d_dy, d_y 16-byte aligned. */
int frcnn_dropout(float* d_x, size_t n, float p, float scale, const uint64_t* d_seed, uint32_t stream_id, uint32_t rank,
                  uint8_t* d_keep_out, void* stream);
int frcnn_dropout_relu_backward(float* d_dy, const float* d_y, size_t n, float scale, void* stream);
/* MaxPool2d(2,2) backward: x [H][W][c] pool input, dy [H/2][W/2][c] -> dx [H][W][c] (first maximum wins). */
int frcnn_maxpool2x2_backward(const float* d_x, const float* d_dy, float* d_dx, int H, int W, int c, void* stream);
/* torchvision RoIPool backward (detector.py:72): dout [n][pooled][pooled][c] -> dfm [fh][fw][c] (gradient to
 * each bin's argmax cell).  Deterministic gather formulation; accumulate != 0 adds to dfm. */
size_t frcnn_roi_pool_backward_workspace_bytes(int n_rois, int pooled, int c);
int frcnn_roi_pool_backward(const float* d_fm, int fh, int fw, int c, const float* d_rois, int n_rois, int pooled,
                            float spatial_scale, const float* d_dout, float* d_dfm, int accumulate,
                            void* d_ws, size_t ws_bytes, void* stream);
/* y[c][r] = x[r][c]; y rows are ldo >= rows wide, the tail is zero filled. */
int frcnn_transpose(const float* d_x, int ldi, float* d_y, int ldo, int rows, int cols, void* stream);
/* torch.optim.SGD.step as built at __main__.py:98-105: g += weight_decay*w; buf = first_step ? g :
 * momentum*buf + g; w -= lr*buf (layout agnostic: applied to the packed weights). */
int frcnn_sgd_step(float* d_w, const float* d_grad, float* d_momentum_buf, size_t n, float lr, float momentum,
                   float weight_decay, int first_step, void* stream);
/* The same update (__main__.py:98-105 SGD) of a convolution master [taps][cout][cin] whose frozen BatchNorm (models/resnet.py:58-77) is folded into the convolution (ResNet bottlenecks),
 * with the folded pack rebuilt in the same launch: d_folded = w_new * d_scale[co] (frcnn_scale_rows' product; n = taps*cout*cin).  ABI 10. */
int frcnn_sgd_step_fold(float* d_w, const float* d_grad, float* d_momentum_buf, size_t n, float lr, float momentum,
                        float weight_decay, int first_step, const float* d_scale, float* d_folded, int cout, int cin, void* stream);

/* Introspection for parity tests: device pointers of intermediate tensors of the LAST forward
 * on this ctx.  which: 0 feature map NHWC [fh][fw][512], 1 RPN head [fh*fw][128],
 * 2 objectness scores [A], 3 sorted anchor indices int32 [pre_nms], 4 RoI-pool out
 * [post_nms][7][7][512], 5 fc2 output [post_nms][4096], 6 anchor map, 7 valid map,
 * 8 head logits [post_nms][128].  (ResNet: the feature map / RoI-pool tensors have 1024 channels,
 * id 5 is the pooled [post_nms][2048] vector.)  Returns FRCNN_EINVAL for unknown ids. */
int frcnn_ctx_tensor(frcnn_ctx* ctx, int which, void** d_ptr, size_t* bytes);

/* Per-kernel-class HIP-event timing for bench.py's roofline block: when enabled, every launch
 * of class `k` inside frcnn_vgg16_forward is bracketed by events on the launch stream.
 * classes: 0 conv3x3 MFMA (backbone+RPN), 1 conv first layer, 2 linear MFMA, 3 proposals,
 * 4 roi_pool, 5 other, 6 Winograd input / output transforms (three-launch float32 form), 7 float32 Winograd MFMA kernels
 * (wino_fused_kernel; the three-launch form's batched GEMM), 8 x6 Winograd input / output transforms, 9 x6 Winograd batched GEMM
 * (gemm_x6t_kernel / gemm_x3t_kernel), 10 one-launch f32x3 Winograd layers (wino_x3d_kernel + their channel-maximum pass).
 * frcnn_ctx_timing_read synchronises the recorded events and returns
 * accumulated milliseconds and launch counts since the last reset. */
#define FRCNN_NUM_KCLASS 11
int frcnn_ctx_timing_enable(frcnn_ctx* ctx, int enable);
int frcnn_ctx_timing_read(frcnn_ctx* ctx, double ms[FRCNN_NUM_KCLASS], int64_t launches[FRCNN_NUM_KCLASS],
                          int reset);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_H */
