// geometry.h -- device helpers shared by the RoIAlign kernels (roialign.hip, ops.hip) and the NMS kernels (proposals.hip, ops.hip).
#pragma once
#include "common.h"

namespace frcnn {

// RoIAlign's sampling plan of one RoI (torchvision.ops.roi_align; oracle/frcnn_oracle.py: roi_align_weights) for out_h x out_w bins.
struct RoiGeom { float start_h, start_w, bin_h, bin_w; int grid_h, grid_w; float count; };

__device__ __forceinline__ RoiGeom roi_align_geom(const f32x4 roi /* y1, x1, y2, x2 */, float scale, int out_h, int out_w,
                                                  int sampling_ratio, int aligned)
{
    RoiGeom g;
    const float offset = aligned ? 0.5f : 0.0f;
    g.start_w = roi[1] * scale - offset;
    g.start_h = roi[0] * scale - offset;
    const float end_w = roi[3] * scale - offset, end_h = roi[2] * scale - offset;
    float roi_w = end_w - g.start_w, roi_h = end_h - g.start_h;
    if (!aligned) { roi_w = fmaxf(roi_w, 1.0f); roi_h = fmaxf(roi_h, 1.0f); }
    g.bin_h = roi_h / (float)out_h;
    g.bin_w = roi_w / (float)out_w;
    g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(roi_h / (float)out_h);
    g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(roi_w / (float)out_w);
    const int cnt = g.grid_h * g.grid_w;
    g.count = (float)(cnt > 1 ? cnt : 1);
    return g;
}

// one coordinate of bilinear_interpolate: returns false when the sample contributes nothing
__device__ __forceinline__ bool axis_weights(float v, int n, int& low, int& high, float& wl, float& wh)
{
    if (v < -1.0f || v > (float)n) return false;
    if (v <= 0.f) v = 0.f;
    low = (int)v;
    if (low >= n - 1) { high = low = n - 1; v = (float)low; }
    else high = low + 1;
    wh = v - (float)low;
    wl = 1.0f - wh;
    return true;
}

// IoU exactly as torchvision's nms kernels compute it (fp32, no +1, no epsilon):
//   inter / (area_a + area_b - inter), suppression iff iou > thr.
__device__ __forceinline__ bool iou_gt(const f32x4 a, const f32x4 b, float thr)
{
    const float l0 = fmaxf(a[0], b[0]), l1 = fmaxf(a[1], b[1]);
    const float r0 = fminf(a[2], b[2]), r1 = fminf(a[3], b[3]);
    const float d0 = fmaxf(r0 - l0, 0.f), d1 = fmaxf(r1 - l1, 0.f);
    const float inter = d0 * d1;
    const float sa = (a[2] - a[0]) * (a[3] - a[1]);
    const float sb = (b[2] - b[0]) * (b[3] - b[1]);
    // The decision is torchvision's `inter / union > thr` to the last bit -- but the quotient (a ~10-instruction sequence, a third of this
    // function) is computed only for the pairs that need it: with t = fl(thr * union), inter > t (1 + 1e-6) implies
    // fl(inter / union) > thr and inter < t (1 - 1e-6) implies fl(inter / union) < thr (the two roundings involved are 6e-8 relative each);
    // only a pair inside that band of 2e-6 takes the division.  The bounds hold for union > 0 only: every other union divides
    // (0 / 0 is NaN, not greater; a box inverted along one axis has a negative area, and 0 / negative is -0.0, not greater either,
    // where the shortcut's t < 0 would say "suppress").
    const float uni = sa + sb - inter, t = thr * uni;
    if (uni > 0.f) {
        if (inter > t * 1.000001f) return true;
        if (inter < t * 0.999999f) return false;
    }
    return (inter / uni) > thr;
}

}  // namespace frcnn
