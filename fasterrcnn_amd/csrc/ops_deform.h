// ops_deform.h -- the bilinear sample of deformable convolution, stated once for every kernel of ops_deform.hip (torchvision's
// deform_conv2d_kernel.cu: bilinear_interpolate and get_coordinate_weight, restated, unpinned), over the storage type E of the maps:
// float, or a 16-bit type of ops_elem.h that is widened exactly on load, so that the arithmetic is the float32 kernels' whatever E is.
#pragma once
#include "ops_elem.h"

namespace frcnn {

// Elem<E>::store, with the element's address formed before the value is rounded: the order in which ops_deform.hip's kernels compile
// to the instruction streams they were measured with
template <typename E> __device__ __forceinline__ void deform_store(E* p, size_t i, float v) { round_to(v, p[i]); }

// sample coordinate of tap i at output index o along one axis: the integer position first, then the float displacement
__device__ __forceinline__ float deform_coord(int o, int stride, int pad, int i, int dil, float off)
{
    return (float)(o * stride - pad + i * dil) + off;
}

// an accepted sample: its low corner (yl, xl) in [-1, H - 1] x [-1, W - 1] and the fractions lh = y - yl, hh = 1 - lh (likewise x)
struct DeformSample { int yl, xl; float lh, hh, lw, hw; };

// false: the sample is rejected (y <= -1, y >= H, x <= -1, x >= W; a NaN coordinate is rejected too, so no corner index is ever formed
// from a value outside the map)
__device__ __forceinline__ bool deform_sample(float y, float x, int H, int W, DeformSample& s)
{
    if (!(y > -1.0f && y < (float)H && x > -1.0f && x < (float)W)) return false;
    const float yf = floorf(y), xf = floorf(x);
    s.yl = (int)yf; s.xl = (int)xf;
    s.lh = y - yf; s.lw = x - xf;
    s.hh = 1.0f - s.lh; s.hw = 1.0f - s.lw;
    return true;
}

// the corners (yl, xl), (yl, xl + 1), (yl + 1, xl), (yl + 1, xl + 1): weights hh hw, hh lw, lh hw, lh lw and the cell index y W + x,
// -1 for a corner outside [0, H - 1] x [0, W - 1]
__device__ __forceinline__ void deform_corners(const DeformSample& s, int H, int W, float w[4], int cell[4])
{
    const bool y0 = s.yl >= 0, y1 = s.yl + 1 <= H - 1, x0 = s.xl >= 0, x1 = s.xl + 1 <= W - 1;
    w[0] = s.hh * s.hw; w[1] = s.hh * s.lw; w[2] = s.lh * s.hw; w[3] = s.lh * s.lw;
    cell[0] = (y0 && x0) ? s.yl * W + s.xl : -1;
    cell[1] = (y0 && x1) ? s.yl * W + s.xl + 1 : -1;
    cell[2] = (y1 && x0) ? (s.yl + 1) * W + s.xl : -1;
    cell[3] = (y1 && x1) ? (s.yl + 1) * W + s.xl + 1 : -1;
}

// bilinear_interpolate: 0 for a rejected sample, else w1 v1 + w2 v2 + w3 v3 + w4 v4 summed from the left
template <typename E>
__device__ __forceinline__ float deform_bilinear(const E* __restrict__ plane, int H, int W, float y, float x)
{
    DeformSample s;
    if (!deform_sample(y, x, H, W, s)) return 0.f;
    float w[4]; int cell[4];
    deform_corners(s, H, W, w, cell);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = cell[k] >= 0 ? Elem<E>::load(plane, cell[k]) : 0.f;
    return ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3];
}

// get_coordinate_weight: the derivative of the sample along y (y_direction) or x -- the difference of the validly indexed corner
// values weighted by the other axis's fractions; the right-hand slope at an integer coordinate.  It has no early-out: at y == -1 the
// corner row 0 still counts.  Outside [-1, H) x [-1, W) no corner is valid and the result is 0 (NaN coordinates included).
template <typename E>
__device__ __forceinline__ float deform_coordinate_weight(const E* __restrict__ plane, int H, int W, float y, float x,
                                                          bool y_direction)
{
    if (!(y >= -1.0f && y < (float)H && x >= -1.0f && x < (float)W)) return 0.f;
    const float yf = floorf(y), xf = floorf(x);
    const int yl = (int)yf, xl = (int)xf, yh = yl + 1, xh = xl + 1;
    const bool vyl = yl >= 0, vyh = yh < H, vxl = xl >= 0, vxh = xh < W;      // yl <= H - 1 and yh >= 0 hold in the accepted range
    const float v_yx = (vyl && vxl) ? Elem<E>::load(plane, yl * W + xl) : 0.f, v_yX = (vyl && vxh) ? Elem<E>::load(plane, yl * W + xh) : 0.f;
    const float v_Yx = (vyh && vxl) ? Elem<E>::load(plane, yh * W + xl) : 0.f, v_YX = (vyh && vxh) ? Elem<E>::load(plane, yh * W + xh) : 0.f;
    const float dx = x - xf, dy = y - yf;
    return y_direction ? dx * (v_YX - v_yX) + (1.0f - dx) * (v_Yx - v_yx) : dy * (v_YX - v_Yx) + (1.0f - dy) * (v_yX - v_yx);
}

}  // namespace frcnn
