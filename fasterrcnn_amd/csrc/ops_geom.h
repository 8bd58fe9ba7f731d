// ops_geom.h -- device helpers shared by the torchvision.ops-style RoI kernels (ops.hip, ops_ps.hip).
#pragma once
#include "geometry.h"

namespace frcnn {

// torchvision's `int roi_batch_ind = rois[0]` with the range check the op contract adds (NaN fails it)
__device__ __forceinline__ bool roi_image(float v, int n_img, int& b)
{
    if (!(v > -1.0f && v < (float)n_img)) return false;
    b = (int)v;
    return true;
}

__device__ __forceinline__ RoiGeom ops_align_geom(const float* roi, float scale, int out_h, int out_w, int sampling_ratio, int aligned)
{
    return roi_align_geom(f32x4{roi[2], roi[1], roi[4], roi[3]}, scale, out_h, out_w, sampling_ratio, aligned);
}

// sample coordinate of bin p, sample i (roi_align_kernel's expression)
__device__ __forceinline__ float sample_coord(float start, float bin, int grid, int p, int i)
{
    return start + (float)p * bin + ((float)i + 0.5f) * bin / (float)grid;
}

// the weight of `cell` in a sample's bilinear footprint along one axis; false when the sample does not touch it
__device__ __forceinline__ bool cell_weight(float v, int n, int cell, float& w)
{
    int lo, hi; float wl, wh;
    if (!axis_weights(v, n, lo, hi, wl, wh)) return false;
    bool hit = false;
    if (lo == cell) { w = wl; hit = true; }
    if (hi == cell) { w = hit ? w + wh : wh; hit = true; }
    return hit;
}

}  // namespace frcnn
