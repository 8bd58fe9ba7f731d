// ops_rfa.hip -- rotated_feature_align of fasterrcnn_amd.ops (R3Det's feature refinement module; S2ANet-style heads that re-sample a map at
// their refined boxes): the frcnn_ops_rotated_feature_align* entry points of include/frcnn_hip.h.  Restated from the published definition of
// mmcv's rotated_feature_align (third party, absent here: restated, unpinned); where the two differ the header's text holds.
//
// Every pixel of a channels-last map owns one box row and adds to its own value the bilinear samples of its image at the box's centre
// (points == 1) or at the centre and the four corners (points == 5).  Forward: one launch, a group of T lanes per pixel, lanes along the
// channel runs (Run<E>); a lane forms the pixel's positions and weights once and walks its runs with them.  Backward: no atomics; the
// sorted-plan gather of ops_msda.h restated for rows of any length: a plan of ((pixel * points + i) * 4 + corner) entries keyed by the cell
// a corner lands on (the sentinel n_cells for a sample that counts nothing), sorted stably by the caller, and one group of lanes per
// (cell, 64 channel runs) that finds the cell's segment by bisection and sums it in ascending entry order after the cell's own dout.
#include "ops_run.h"

namespace frcnn {

static constexpr int RFA_MAX_POINTS = 5;
static constexpr long long RFA_MAX_INDEX = (long long)INT32_MAX - 1024;     // plan entries of one call: 32-bit positions in the sorted plan

struct RfaSample { int cell[4]; float w[4]; bool ok; };

// frcnn_ops_roi_align's bilinear rule at (y, x): the four cells (y low, x low), (y low, x high), (y high, x low), (y high, x high) and
// their weights; not ok outside [-1, size] on either axis or at a NaN or infinite coordinate, which never reaches the conversion to int
__device__ __forceinline__ RfaSample rfa_sample(float y, float x, int fh, int fw)
{
    RfaSample s;
    int yl = 0, yh = 0, xl = 0, xh = 0;
    float hy = 0.f, ly = 0.f, hx = 0.f, lx = 0.f;
    s.ok = y >= -1.0f && y <= (float)fh && x >= -1.0f && x <= (float)fw && axis_weights(y, fh, yl, yh, hy, ly) &&
           axis_weights(x, fw, xl, xh, hx, lx);
    s.cell[0] = yl * fw + xl; s.cell[1] = yl * fw + xh; s.cell[2] = yh * fw + xl; s.cell[3] = yh * fw + xh;
    s.w[0] = hy * hx; s.w[1] = hy * lx; s.w[2] = ly * hx; s.w[3] = ly * lx;
    return s;
}

// the sample positions of one box row (component 0 is the ROW coordinate); with points == 1 components 2..4 are never read
__device__ __forceinline__ void rfa_positions(const float* __restrict__ b, float scale, int points, float* px, float* py)
{
    const float y0 = b[0] * scale, x0 = b[1] * scale;
    px[0] = x0; py[0] = y0;
    if (points == 1) return;
    const float w2 = b[2] * scale / 2.0f, h2 = b[3] * scale / 2.0f, a = b[4];
    const float ca = cosf(a), sa = sinf(a);
    const float wx = ca * w2, wy = sa * w2, hx = -sa * h2, hy = ca * h2;
    px[1] = (x0 + wx) + hx; py[1] = (y0 + wy) + hy;
    px[2] = (x0 - wx) + hx; py[2] = (y0 - wy) + hy;
    px[3] = (x0 - wx) - hx; py[3] = (y0 - wy) - hy;
    px[4] = (x0 + wx) - hx; py[4] = (y0 + wy) - hy;
}

// out[pixel] = x[pixel] + the pixel's samples in order i: a group of T lanes (a power of two <= 64) per pixel, the lane's runs T apart
template <typename E>
__global__ __launch_bounds__(256)
void ops_rfa_kernel(const E* __restrict__ x, const float* __restrict__ boxes, long long n_pixels, int fh, int fw, int C, float scale,
                    int points, int T, E* __restrict__ out)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    const int C4 = C / R::V, grp = threadIdx.x / T, t = threadIdx.x - grp * T;
    const long long pix = (long long)blockIdx.x * (256 / T) + grp;
    if (pix >= n_pixels) return;
    const long long img = pix / ((long long)fh * fw);
    const E* fm = x + (size_t)img * fh * fw * C;
    float px[RFA_MAX_POINTS], py[RFA_MAX_POINTS];
    rfa_positions(boxes + (size_t)pix * 5, scale, points, px, py);
    RfaSample s[RFA_MAX_POINTS];
#pragma unroll
    for (int i = 0; i < RFA_MAX_POINTS; ++i) {
        s[i].ok = false;
        if (i < points) s[i] = rfa_sample(py[i], px[i], fh, fw);
    }
    for (int c4 = t; c4 < C4; c4 += T) {
        vec acc = R::load(x + (size_t)pix * C, c4);
#pragma unroll
        for (int i = 0; i < RFA_MAX_POINTS; ++i) {
            if (!s[i].ok) continue;
            const vec v1 = R::load(fm + (size_t)s[i].cell[0] * C, c4);
            const vec v2 = R::load(fm + (size_t)s[i].cell[1] * C, c4);
            const vec v3 = R::load(fm + (size_t)s[i].cell[2] * C, c4);
            const vec v4 = R::load(fm + (size_t)s[i].cell[3] * C, c4);
            acc = acc + (((v1 * s[i].w[0] + v2 * s[i].w[1]) + v3 * s[i].w[2]) + v4 * s[i].w[3]);
        }
        R::store(out + (size_t)pix * C, c4, acc);
    }
}

// entry ((pixel * points + i) * 4 + corner): the key image * fh * fw + cell and the weight of that corner; a sample that counts nothing
// carries the sentinel n_pixels and weight 0 on all four
__global__ __launch_bounds__(256)
void ops_rfa_plan_kernel(const float* __restrict__ boxes, long long n_pixels, int fh, int fw, float scale, int points,
                         long long* __restrict__ keys, float* __restrict__ wts)
{
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pixels) return;
    const long long first = pix / ((long long)fh * fw) * ((long long)fh * fw);      // the image's first cell
    float px[RFA_MAX_POINTS], py[RFA_MAX_POINTS];
    rfa_positions(boxes + (size_t)pix * 5, scale, points, px, py);
#pragma unroll
    for (int i = 0; i < RFA_MAX_POINTS; ++i) {
        if (i >= points) break;
        const RfaSample s = rfa_sample(py[i], px[i], fh, fw);
        const size_t e = ((size_t)pix * points + i) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            keys[e + k] = s.ok ? first + s.cell[k] : n_pixels;
            wts[e + k] = s.ok ? s.w[k] : 0.f;
        }
    }
}

// the first position of the sorted keys that holds a key >= c
__device__ __forceinline__ int rfa_lower_bound(const long long* __restrict__ sorted_keys, int n_entries, long long c)
{
    int lo = 0, hi = n_entries;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (sorted_keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// dx[cell] = dout[cell], then + wts[e] * dout[e / (4 points)] over the cell's entries e in ascending order (a stable sort keeps them so):
// a group of T lanes per cell, blockIdx.y the chunk of 64 channel runs
template <typename E>
__global__ __launch_bounds__(256)
void ops_rfa_backward_kernel(const long long* __restrict__ sorted_keys, const long long* __restrict__ order, const float* __restrict__ wts,
                             const E* __restrict__ dout, long long n_pixels, int n_entries, int points4, int C, int T, E* __restrict__ dx)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    const int C4 = C / R::V, grp = threadIdx.x / T, t = threadIdx.x - grp * T;
    const long long cell = (long long)blockIdx.x * (256 / T) + grp;
    const int c4 = blockIdx.y * 64 + t;
    if (cell >= n_pixels || c4 >= C4) return;
    const int i0 = rfa_lower_bound(sorted_keys, n_entries, cell), i1 = rfa_lower_bound(sorted_keys, n_entries, cell + 1);
    vec acc = R::load(dout + (size_t)cell * C, c4);
    for (int i = i0; i < i1; ++i) {
        const long long e = order[i];
        if (e < 0 || e >= n_entries) continue;                        // a permutation of [0, n_entries) by contract
        acc = acc + R::load(dout + (size_t)(e / points4) * C, c4) * wts[e];
    }
    R::store(dx + (size_t)cell * C, c4, acc);
}

static int pow2_lanes(int runs) { int t = 1; while (t < runs && t < 64) t <<= 1; return t; }

// n_img == 0 is an empty call; the plan of one call holds n_img fh fw points 4 entries
static bool rfa_args_ok(int n_img, int fh, int fw, int c, int points, int v)
{
    if (n_img < 0 || fh < 1 || fw < 1 || c < v || c % v != 0 || (points != 1 && points != RFA_MAX_POINTS)) return false;
    if ((long long)fh * fw > RFA_MAX_INDEX || (long long)n_img * fh * fw > RFA_MAX_INDEX / (4 * points)) return false;
    return cdiv(c / v, 64) <= 65535;                                   // the gather's grid y
}

template <typename E>
static int rfa_impl(const void* d_x, const float* d_boxes, int n_img, int fh, int fw, int c, float spatial_scale, int points, void* d_out,
                    void* stream)
{
    if (!rfa_args_ok(n_img, fh, fw, c, points, Run<E>::V)) return FRCNN_EINVAL;
    if (n_img == 0) return FRCNN_OK;
    if (!d_x || !d_boxes || !d_out) return FRCNN_EINVAL;
    const long long n_pixels = (long long)n_img * fh * fw;
    const int T = pow2_lanes(c / Run<E>::V);
    hipLaunchKernelGGL(ops_rfa_kernel<E>, dim3((unsigned)((n_pixels + 256 / T - 1) / (256 / T))), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const E*>(d_x), d_boxes, n_pixels, fh, fw, c, spatial_scale, points, T, static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int rfa_backward_impl(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const void* d_dout, int n_img,
                             int fh, int fw, int c, int points, void* d_dx, void* stream)
{
    if (!rfa_args_ok(n_img, fh, fw, c, points, Run<E>::V)) return FRCNN_EINVAL;
    if (n_img == 0) return FRCNN_OK;
    if (!d_sorted_keys || !d_order || !d_weights || !d_dout || !d_dx) return FRCNN_EINVAL;
    const long long n_pixels = (long long)n_img * fh * fw;
    const int C4 = c / Run<E>::V, T = pow2_lanes(C4);
    hipLaunchKernelGGL(ops_rfa_backward_kernel<E>, dim3((unsigned)((n_pixels + 256 / T - 1) / (256 / T)), cdiv(C4, 64)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const long long*>(d_sorted_keys), reinterpret_cast<const long long*>(d_order),
                       d_weights, static_cast<const E*>(d_dout), n_pixels, (int)(n_pixels * points * 4), points * 4, c, T,
                       static_cast<E*>(d_dx));
    return check_launch();
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_rotated_feature_align(const float* d_x, const float* d_boxes, int n_img, int fh, int fw, int c, float spatial_scale,
                                    int points, float* d_out, void* stream)
{
    return rfa_impl<float>(d_x, d_boxes, n_img, fh, fw, c, spatial_scale, points, d_out, stream);
}

int frcnn_ops_rotated_feature_align_plan(const float* d_boxes, int n_img, int fh, int fw, float spatial_scale, int points, int64_t* d_keys,
                                         float* d_weights, void* stream)
{
    if (!rfa_args_ok(n_img, fh, fw, 4, points, 4)) return FRCNN_EINVAL;
    if (n_img == 0) return FRCNN_OK;
    if (!d_boxes || !d_keys || !d_weights) return FRCNN_EINVAL;
    const long long n_pixels = (long long)n_img * fh * fw;
    hipLaunchKernelGGL(ops_rfa_plan_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_boxes, n_pixels,
                       fh, fw, spatial_scale, points, reinterpret_cast<long long*>(d_keys), d_weights);
    return check_launch();
}

int frcnn_ops_rotated_feature_align_backward(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                             const float* d_dout, int n_img, int fh, int fw, int c, int points, float* d_dx, void* stream)
{
    return rfa_backward_impl<float>(d_sorted_keys, d_order, d_weights, d_dout, n_img, fh, fw, c, points, d_dx, stream);
}

int frcnn_ops_rotated_feature_align_16(int elem_type, const void* d_x, const float* d_boxes, int n_img, int fh, int fw, int c,
                                       float spatial_scale, int points, void* d_out, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, OPS_HALF_RUN, rfa_impl, d_x, d_boxes, n_img, fh, fw, c, spatial_scale, points, d_out, stream);
}

int frcnn_ops_rotated_feature_align_backward_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                                const void* d_dout, int n_img, int fh, int fw, int c, int points, void* d_dx, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), rfa_backward_impl, d_sorted_keys, d_order, d_weights, d_dout, n_img, fh, fw, c, points,
                    d_dx, stream);
}

}  // extern "C"
