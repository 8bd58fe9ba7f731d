// ops_keypoint.hip -- the last step of a Keypoint R-CNN's keypoint head (include/frcnn_hip.h states the contract):
//
//   keypoint_kernel<E>   torchvision's / detectron2's heatmaps_to_keypoints: per (RoI, keypoint) the position and value of the maximum
//                        of the map resized bicubically to the RoI's [H, W] pixels, and detectron2's score there.
//
// One block per (RoI, keypoint); the [H, W] image never exists.  The map is staged once in LDS, widened to float32.  The resize is
// separable and the rows are combined first: wave q of a pass takes output row y = pass * KP_WAVES + q, forms that row's four source
// rows and weights once and blends them into a row of mw floats of its own in LDS (lane j on column j: consecutive words, no bank
// conflict); after the pass's one barrier its lanes walk the row's W pixels 64 at a time, four reads of that LDS row each (when the box
// is larger than the map, neighbouring lanes read the same or the next word: broadcasts; a shrinking resize reads at a stride and may
// conflict, on few pixels), and keep a running (value, index) maximum.  The row buffers alternate between passes, so a pass needs one
// barrier.  The maxima are compared as (value, index) pairs under a total order -- a NaN above every number, then the larger value, then
// the smaller index -- through an xor butterfly and then across the waves, so the result does not depend on who saw a pixel.  The sum
// of exp(map - maximum) runs over the LDS map afterwards, a fixed order per lane, a butterfly, the waves in order.  No atomics, no
// workspace, no memset, no host read.  A refused RoI returns before the map is read.
// All arithmetic is float32 in the header's order without contraction.
#include "ops_elem.h"

#pragma clang fp contract(off)

namespace frcnn {

static constexpr int KP_THREADS = 256;
static constexpr int KP_WAVES = KP_THREADS / 64;                     // output rows of one pass of a block
static constexpr int KP_MAX_MAP = 112;                               // the map in LDS as float32: 112 * 112 * 4 = 50176 B
static constexpr int KP_MAX_SIDE = 4096;                             // W, H of one RoI: a block walks at most 2^24 pixels, 2^16 a lane
static constexpr long long KP_MAX_ITEMS = 2147483647LL;              // r k: one block each on grid.x

// the four taps of one output coordinate d of an axis resized from n to n / scale: torch's upsample_bicubic2d, align_corners=False
struct KpTaps {
    int i0, i1, i2, i3;
    float w0, w1, w2, w3;
};

__device__ __forceinline__ KpTaps kp_taps(int d, float scale, int n)
{
    KpTaps a;
    const float src = scale * ((float)d + 0.5f) - 0.5f;
    const float f = floorf(src);
    const float t = src - f;
    const int i = (int)f;
    a.i0 = min(max(i - 1, 0), n - 1);
    a.i1 = min(max(i, 0), n - 1);
    a.i2 = min(max(i + 1, 0), n - 1);
    a.i3 = min(max(i + 2, 0), n - 1);
    const float u0 = t + 1.f, u2 = 1.f - t, u3 = u2 + 1.f;
    a.w0 = ((-0.75f * u0 + 3.75f) * u0 - 6.f) * u0 + 3.f;
    a.w1 = (1.25f * t - 2.25f) * t * t + 1.f;
    a.w2 = (1.25f * u2 - 2.25f) * u2 * u2 + 1.f;
    a.w3 = ((-0.75f * u3 + 3.75f) * u3 - 6.f) * u3 + 3.f;
    return a;
}

// (v, i) before (bv, bi) in the total order: a NaN above every number, then the larger value, then the smaller index
__device__ __forceinline__ bool kp_before(float v, int i, float bv, int bi)
{
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (!vn && v != bv) return v > bv;
    return i < bi;
}

static __device__ __forceinline__ bool kp_finite(const float* b)
{
    return fabsf(b[0]) <= 3.4028234e38f && fabsf(b[1]) <= 3.4028234e38f && fabsf(b[2]) <= 3.4028234e38f && fabsf(b[3]) <= 3.4028234e38f;
}

template <typename E>
__global__ __launch_bounds__(KP_THREADS)
void keypoint_kernel(const E* __restrict__ maps, const float* __restrict__ rois, float* __restrict__ out, int k, int mh, int mw)
{
    extern __shared__ __attribute__((aligned(16))) float s_map[];
    __shared__ float s_row[2][KP_WAVES][KP_MAX_MAP];
    __shared__ float s_val[KP_WAVES];
    __shared__ int s_idx[KP_WAVES];
    __shared__ float s_sum[KP_WAVES];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    const size_t item = blockIdx.x;
    const float* b = rois + 4 * (item / (size_t)k);
    float* o = out + 4 * item;

    const float x1 = b[0], y1 = b[1];
    const float w = fmaxf(b[2] - x1, 1.f), h = fmaxf(b[3] - y1, 1.f);
    const float wc = ceilf(w), hc = ceilf(h);
    if (!(kp_finite(b) && wc <= (float)KP_MAX_SIDE && hc <= (float)KP_MAX_SIDE)) {     // block-uniform: before any barrier
        if (t < 4) o[t] = __uint_as_float(0x7FC00000u);
        return;
    }
    const int W = (int)wc, H = (int)hc, n = mh * mw;

    const E* m = maps + item * (size_t)n;
    const float first = widen(m[0]);
    bool same = true;
    for (int i = t; i < n; i += KP_THREADS) {
        const float v = widen(m[i]);
        s_map[i] = v;
        same &= v == first;
    }
    const bool constant = __syncthreads_and(same) != 0;               // a constant map IS its resized image: (0, 0), the constant

    float bv = first;
    int bi = 0;
    if (!constant) {
        bv = -INFINITY;
        bi = 0x7fffffff;
        const float sx = (float)mw / wc, sy = (float)mh / hc;
        for (int y0 = 0, buf = 0; y0 < H; y0 += KP_WAVES, buf ^= 1) {
            const int y = y0 + q;
            float* row = s_row[buf][q];
            if (y < H) {
                const KpTaps a = kp_taps(y, sy, mh);
                const float *r0 = s_map + a.i0 * mw, *r1 = s_map + a.i1 * mw, *r2 = s_map + a.i2 * mw, *r3 = s_map + a.i3 * mw;
                for (int j = lane; j < mw; j += 64) row[j] = ((a.w0 * r0[j] + a.w1 * r1[j]) + a.w2 * r2[j]) + a.w3 * r3[j];
            }
            __syncthreads();
            if (y < H) {
                for (int x = lane; x < W; x += 64) {
                    const KpTaps c = kp_taps(x, sx, mw);
                    const float v = ((c.w0 * row[c.i0] + c.w1 * row[c.i1]) + c.w2 * row[c.i2]) + c.w3 * row[c.i3];
                    const int i = y * W + x;
                    if (kp_before(v, i, bv, bi)) { bv = v; bi = i; }
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(bv, d);
            const int oi = __shfl_xor(bi, d);
            if (kp_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_val[q] = bv; s_idx[q] = bi; }
        __syncthreads();
        bv = s_val[0]; bi = s_idx[0];
#pragma unroll
        for (int p = 1; p < KP_WAVES; ++p)
            if (kp_before(s_val[p], s_idx[p], bv, bi)) { bv = s_val[p]; bi = s_idx[p]; }
    }

    float s = 0.f;
    for (int i = t; i < n; i += KP_THREADS) s = s + expf(s_map[i] - bv);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d);
    if (lane == 0) s_sum[q] = s;
    __syncthreads();
    if (t == 0) {
        float total = s_sum[0];
#pragma unroll
        for (int p = 1; p < KP_WAVES; ++p) total = total + s_sum[p];
        const int yi = bi / W, xi = bi - yi * W;
        o[0] = ((float)xi + 0.5f) * (w / wc) + x1;
        o[1] = ((float)yi + 0.5f) * (h / hc) + y1;
        o[2] = bv;
        o[3] = 1.f / total;
    }
}

template <typename E>
static int keypoint_launch(const void* maps, const float* rois, float* out, int r, int k, int mh, int mw, hipStream_t s)
{
    hipLaunchKernelGGL(keypoint_kernel<E>, dim3((unsigned)((long long)r * k)), dim3(KP_THREADS), (size_t)mh * mw * sizeof(float), s,
                       static_cast<const E*>(maps), rois, out, k, mh, mw);
    return check_launch();
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_keypoint_max_map_side(void) { return KP_MAX_MAP; }
int frcnn_ops_keypoint_max_roi_side(void) { return KP_MAX_SIDE; }
int frcnn_ops_keypoint_block_threads(void) { return KP_THREADS; }

int frcnn_ops_heatmaps_to_keypoints(int elem_type, const void* d_maps, const float* d_rois, int r, int k, int mh, int mw, float* d_out,
                                    void* stream)
{
    if (elem_type != FRCNN_OPS_F32 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    if (r < 0 || k < 0 || mh < 1 || mh > KP_MAX_MAP || mw < 1 || mw > KP_MAX_MAP || (long long)r * k > KP_MAX_ITEMS) return FRCNN_EINVAL;
    if (r == 0 || k == 0) return FRCNN_OK;
    if (!d_maps || !d_rois || !d_out) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (elem_type == FRCNN_OPS_F32) return keypoint_launch<float>(d_maps, d_rois, d_out, r, k, mh, mw, s);
    OPS_ELEM_DISPATCH(elem_type, E, keypoint_launch<E>(d_maps, d_rois, d_out, r, k, mh, mw, s));
}

}  // extern "C"
