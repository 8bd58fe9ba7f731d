// ops_mask.hip -- the mask operators of a Mask R-CNN's last step (include/frcnn_hip.h states the contracts):
//
//   paste_kernel<E, O, PasteInImage>   torchvision's paste_masks_in_image: mask k, padded by p zeros and resized bilinearly to the integer
//                                      box of its row, written into image k of [K, 1, H, W]; O = E.
//   paste_kernel<E, uint8_t, PasteAligned>   detectron2's paste_masks_in_image / mmdet's _do_paste_mask and its threshold: every pixel
//                                      centre sampled bilinearly in the mask with zero padding, compared or quantised; [K, H, W] bytes.
//   mask_boxes_band_kernel<Z>, mask_boxes_combine_kernel   torchvision's masks_to_boxes: integer extrema of the non-zero pixels of bands
//                                      of every mask into a workspace, then one wave per mask combines its bands in a fixed order.
//
// A paste is a store stream of K H W elements, so the image of one mask is cut into pieces of MASK_THREADS * MASK_ITERS vectors (16
// bytes of a 32- or 16-bit image, 4 bytes of a byte image: see PASTE_BYTE_VECTOR), a block per piece (grid.y: the mask).  H W and W are
// arbitrary, so neither an image nor a row starts on a vector boundary in general: the elements of image k before its first boundary
// (the head) and after its last whole vector (the tail), fewer than 16 each, are stored one by one by lanes of block 0, everything
// else as aligned vectors, consecutive lanes on consecutive vectors.
// Every element of the output is stored exactly once; nothing is read from it and no memset precedes the launch.
// An operator states per mask a pixel window outside which every pixel is the fill value (exact for PasteInImage: the integer box
// clipped to the image; for PasteAligned a superset of the pixels whose sample touches the mask).  A block whose rows miss the window,
// or whose box is dead, never reads the mask: it stores fill vectors.  The others stage the mask once in LDS, widened to float32, and a
// vector that lies in one row beside the window is again a fill vector; only the remaining pixels are evaluated (four LDS reads each).
// All arithmetic is float32 without contraction; the only rounding to a 16-bit type is ops_elem.h's on the store.
#include "ops_elem.h"

#pragma clang fp contract(off)

namespace frcnn {

static constexpr int MASK_THREADS = 256;
static constexpr int MASK_ITERS = 4;                                 // vectors a lane of a block stores (or loads)
static constexpr int MASK_PIECE = MASK_THREADS * MASK_ITERS;         // vectors of a block's piece: 16 KB of 16-byte vectors
static constexpr int MASK_MAX_SIDE = 112;                            // the mask in LDS as float32: 112 * 112 * 4 = 50176 B
static constexpr int MASK_MAX_PADDING = 65536;
static constexpr float MASK_CORNER = 536870912.f;                    // 2^29: integer corners saturate to [-2^29, 2^29]
static constexpr long long MASK_MAX_PLANE = 2147483647LL - 1024;     // H W of one image
static constexpr int MASK_GRID_Y = 65535;                            // masks of one launch

struct PasteArgs {
    int mh, mw, pad, h, w, hw;
    float scale;         // PasteInImage: float32((M + 2 pad) / M)
    float threshold;     // PasteAligned
    int as_uint8;        // PasteAligned: trunc(255 value) saturated instead of value >= threshold
};

// the padded mask at (i, j): the staged mask with the index shifted by pad, zero outside it
__device__ __forceinline__ float mask_at(const float* s_mask, int i, int j, const PasteArgs& a)
{
    i -= a.pad; j -= a.pad;
    return ((unsigned)i < (unsigned)a.mh && (unsigned)j < (unsigned)a.mw) ? s_mask[i * a.mw + j] : 0.f;
}

__device__ __forceinline__ float mask_blend(const float* s_mask, int iy, int iy1, float ly, int ix, int ix1, float lx, const PasteArgs& a)
{
    const float top = (1.f - lx) * mask_at(s_mask, iy, ix, a) + lx * mask_at(s_mask, iy, ix1, a);
    const float bot = (1.f - lx) * mask_at(s_mask, iy1, ix, a) + lx * mask_at(s_mask, iy1, ix1, a);
    return (1.f - ly) * top + ly * bot;
}

__device__ __forceinline__ bool box_finite(const float* b)
{
    return fabsf(b[0]) <= 3.4028234e38f && fabsf(b[1]) <= 3.4028234e38f && fabsf(b[2]) <= 3.4028234e38f && fabsf(b[3]) <= 3.4028234e38f;
}

// torchvision's expand_boxes / .to(int64) / paste_mask_in_image, in the header's order
struct PasteInImage {
    int X0, Y0, mp;
    float rx, ry;
    int wx0, wx1, wy0, wy1;       // the window: the integer box clipped to the image
    bool alive;

    static __device__ __forceinline__ int corner(float v) { return (int)fminf(fmaxf(v, -MASK_CORNER), MASK_CORNER); }

    __device__ __forceinline__ void init(const float* b, const PasteArgs& a)
    {
        const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        float w_half = (x2 - x1) * 0.5f, h_half = (y2 - y1) * 0.5f;
        const float x_c = (x2 + x1) * 0.5f, y_c = (y2 + y1) * 0.5f;
        w_half = w_half * a.scale;
        h_half = h_half * a.scale;
        X0 = corner(x_c - w_half);
        Y0 = corner(y_c - h_half);
        const int X1 = corner(x_c + w_half), Y1 = corner(y_c + h_half);
        const int bw = max(X1 - X0 + 1, 1), bh = max(Y1 - Y0 + 1, 1);
        mp = a.mh + 2 * a.pad;
        rx = (float)mp / (float)bw;
        ry = (float)mp / (float)bh;
        wx0 = max(X0, 0); wx1 = min(X0 + bw, a.w);
        wy0 = max(Y0, 0); wy1 = min(Y0 + bh, a.h);
        alive = box_finite(b) && X0 <= X1 && Y0 <= Y1 && wx0 < wx1 && wy0 < wy1;
    }
    __device__ __forceinline__ void axis(int d, float r, int& i0, int& i1, float& l) const
    {
        const float s = fmaxf(r * ((float)d + 0.5f) - 0.5f, 0.f);
        i0 = min((int)s, mp - 1);
        i1 = i0 + (i0 < mp - 1);
        l = s - (float)i0;
    }
    // the pixel (y, x) inside the window
    __device__ __forceinline__ float value(const float* s_mask, int y, int x, const PasteArgs& a) const
    {
        int ix, ix1, iy, iy1;
        float lx, ly;
        axis(x - X0, rx, ix, ix1, lx);
        axis(y - Y0, ry, iy, iy1, ly);
        return mask_blend(s_mask, iy, iy1, ly, ix, ix1, lx, a);
    }
    template <typename O> __device__ __forceinline__ O finish(float v, const PasteArgs&) const { return narrow<O>(v); }
    template <typename O> __device__ __forceinline__ O fill(const PasteArgs&) const { return O{}; }
};

// detectron2's / mmdet's paste: the pixel centre mapped into the mask in pixels, grid_sample's zero padding
struct PasteAligned {
    float x0, y0, bw, bh;
    int wx0, wx1, wy0, wy1;       // a superset of the pixels whose sample lies inside (-1, M)
    bool alive;

    // [lo, hi) of the pixels c with c + 0.5 inside (c0 - e, c1 + e), e = half a mask cell in pixels, widened by a cell, a pixel and
    // 2^-20 of the coordinates' magnitude: far more than the float32 error of the sample coordinate
    static __device__ __forceinline__ void span(float c0, float c1, float d, int m, int n, int& lo, int& hi)
    {
        const float e = d / (float)m + 1.f + (fabsf(c0) + fabsf(c1)) * 9.5367431640625e-7f;
        lo = (int)fminf(fmaxf(floorf(c0 - e), 0.f), (float)n);
        hi = (int)fminf(fmaxf(ceilf(c1 + e), 0.f), (float)n);
    }
    __device__ __forceinline__ void init(const float* b, const PasteArgs& a)
    {
        x0 = b[0]; y0 = b[1];
        bw = b[2] - b[0]; bh = b[3] - b[1];
        alive = box_finite(b) && b[2] > b[0] && b[3] > b[1];
        wx0 = wx1 = wy0 = wy1 = 0;
        if (alive) {
            span(b[0], b[2], bw, a.mw, a.w, wx0, wx1);
            span(b[1], b[3], bh, a.mh, a.h, wy0, wy1);
        }
    }
    __device__ __forceinline__ float value(const float* s_mask, int y, int x, const PasteArgs& a) const
    {
        const float sx = (((float)x + 0.5f) - x0) / bw * (float)a.mw - 0.5f;
        const float sy = (((float)y + 0.5f) - y0) / bh * (float)a.mh - 0.5f;
        if (!(sx > -1.f && sx < (float)a.mw && sy > -1.f && sy < (float)a.mh)) return 0.f;
        const float fx = floorf(sx), fy = floorf(sy);
        const int ix = (int)fx, iy = (int)fy;
        return mask_blend(s_mask, iy, iy + 1, sy - fy, ix, ix + 1, sx - fx, a);
    }
    template <typename O> __device__ __forceinline__ O finish(float v, const PasteArgs& a) const
    {
        if (a.as_uint8) {
            const float q = v * 255.f;
            return (O)(q >= 255.f ? 255 : q > 0.f ? (int)q : 0);             // a NaN fails both comparisons: 0
        }
        return (O)(v >= a.threshold);
    }
    // a dead row is all False / 0; a live one holds finish(0) outside its window
    template <typename O> __device__ __forceinline__ O fill(const PasteArgs& a) const { return alive ? finish<O>(0.f, a) : (O)0; }
};

// the pieces of one image of hw elements of O at address p: head elements, nvec aligned vectors of B bytes, then the tail
template <typename O, int B = 16> struct Pieces {
    static constexpr int V = B / (int)sizeof(O);
    int head, nvec, tail0;
    __device__ __forceinline__ Pieces(const void* p, int hw)
    {
        head = min(hw, (int)((((unsigned)B - (unsigned)(reinterpret_cast<uintptr_t>(p) & (unsigned)(B - 1))) & (unsigned)(B - 1)) / sizeof(O)));
        nvec = (hw - head) / V;
        tail0 = head + nvec * V;
    }
};

template <typename O, int B = 16> struct alignas(B) Vec { O e[B / sizeof(O)]; };

// B: the bytes of a lane's vector.  16 for PasteInImage (4 floats, 8 halves).  PasteAligned stores PASTE_BYTE_VECTOR = 4 pixels a lane:
// with 16 pixels a lane only the few lanes of a wave that a box covers would evaluate 16 pixels each, and that divergence, not the
// store, bounded the byte forms (measured: 116 us at 16 bytes for K = 100, 800 x 1333); a wave's store is still 256 contiguous bytes.
static constexpr int PASTE_BYTE_VECTOR = 4;

template <typename E, typename O, typename Op, int B>
__global__ __launch_bounds__(MASK_THREADS)
void paste_kernel(const E* __restrict__ masks, const float* __restrict__ boxes, O* __restrict__ out, PasteArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_mask[];
    constexpr int V = Pieces<O, B>::V;
    const int t = threadIdx.x, k = blockIdx.y, b = blockIdx.x;
    O* o = out + (size_t)k * a.hw;
    const Pieces<O, B> pc(o, a.hw);
    const int v_lo = b * MASK_PIECE, v_hi = min(v_lo + MASK_PIECE, pc.nvec);
    if (b > 0 && v_lo >= v_hi) return;                               // block-uniform: before the barrier

    Op op;
    op.init(boxes + 4 * (size_t)k, a);
    // the block's rows against the window (block 0 also owns the head and the tail: it takes every live box)
    bool need = op.alive;
    if (need && b > 0) {
        const int y_lo = (pc.head + v_lo * V) / a.w, y_hi = (pc.head + v_hi * V - 1) / a.w;
        need = y_lo < op.wy1 && y_hi >= op.wy0;
    }
    if (need) {
        const E* m = masks + (size_t)k * (a.mh * a.mw);
        for (int i = t; i < a.mh * a.mw; i += MASK_THREADS) s_mask[i] = widen(m[i]);
        __syncthreads();
    }
    const O fill = op.template fill<O>(a);
    auto pixel = [&](int y, int x) -> O {
        if (!need || y < op.wy0 || y >= op.wy1 || x < op.wx0 || x >= op.wx1) return fill;
        return op.template finish<O>(op.value(s_mask, y, x, a), a);
    };

#pragma unroll
    for (int it = 0; it < MASK_ITERS; ++it) {
        const int vi = v_lo + it * MASK_THREADS + t;
        if (vi >= v_hi) break;
        const int p = pc.head + vi * V;
        int y = p / a.w, x = p - y * a.w;
        Vec<O, B> r;
        // one row, beside the window: nothing to evaluate
        if (!need || (x + V <= a.w && (y < op.wy0 || y >= op.wy1 || x + V <= op.wx0 || x >= op.wx1))) {
#pragma unroll
            for (int j = 0; j < V; ++j) r.e[j] = fill;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                r.e[j] = pixel(y, x);
                if (++x == a.w) { x = 0; ++y; }
            }
        }
        *reinterpret_cast<Vec<O, B>*>(o + p) = r;
    }
    if (b == 0) {
        if (t < pc.head) o[t] = pixel(t / a.w, t % a.w);
        const int p = pc.tail0 + t;
        if (p < a.hw) o[p] = pixel(p / a.w, p % a.w);
    }
}

template <typename E, typename O, typename Op, int B>
static int paste_launch(const void* masks, const float* boxes, void* out, int k, const PasteArgs& a, hipStream_t s)
{
    const int blocks = max(1, cdiv(a.hw / Pieces<O, B>::V, MASK_PIECE));
    const size_t lds = (size_t)a.mh * a.mw * sizeof(float);
    for (int k0 = 0; k0 < k; k0 += MASK_GRID_Y) {
        hipLaunchKernelGGL((paste_kernel<E, O, Op, B>), dim3(blocks, min(k - k0, MASK_GRID_Y)), dim3(MASK_THREADS), lds, s,
                           static_cast<const E*>(masks) + (size_t)k0 * a.mh * a.mw, boxes + 4 * (size_t)k0,
                           static_cast<O*>(out) + (size_t)k0 * a.hw, a);
        const int rc = check_launch();
        if (rc) return rc;
    }
    return FRCNN_OK;
}

// ---- masks_to_boxes -------------------------------------------------------------------------------------------------------------------
// Z: the unsigned integer of an element's size; KEEP: the bits that make it non-zero (all of a bool or uint8; all but the sign of a
// float, so that -0.0 is zero and every NaN is not)
template <typename Z, unsigned KEEP>
__global__ __launch_bounds__(MASK_THREADS)
void mask_boxes_band_kernel(const Z* __restrict__ masks, int hw, int w, int4* __restrict__ ws)
{
    constexpr int V = Pieces<Z>::V;
    __shared__ int s_red[MASK_THREADS / 64][4];
    const int t = threadIdx.x, n = blockIdx.y, b = blockIdx.x;
    const Z* m = masks + (size_t)n * hw;
    const Pieces<Z> pc(m, hw);
    const int v_lo = b * MASK_PIECE, v_hi = min(v_lo + MASK_PIECE, pc.nvec);
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    auto take = [&](int y, int x) { xmin = min(xmin, x); ymin = min(ymin, y); xmax = max(xmax, x); ymax = max(ymax, y); };

#pragma unroll
    for (int it = 0; it < MASK_ITERS; ++it) {
        const int vi = v_lo + it * MASK_THREADS + t;
        if (vi >= v_hi) break;
        const int p = pc.head + vi * V;
        const Vec<Z> r = *reinterpret_cast<const Vec<Z>*>(m + p);
        bool any = false;
#pragma unroll
        for (int j = 0; j < V; ++j) any |= (r.e[j] & (Z)KEEP) != 0;
        if (!any) continue;
        int y = p / w, x = p - y * w;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (r.e[j] & (Z)KEEP) take(y, x);
            if (++x == w) { x = 0; ++y; }
        }
    }
    if (b == 0) {
        if (t < pc.head && (m[t] & (Z)KEEP)) take(t / w, t % w);
        const int p = pc.tail0 + t;
        if (p < hw && (m[p] & (Z)KEEP)) take(p / w, p % w);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, d)); ymin = min(ymin, __shfl_xor(ymin, d));
        xmax = max(xmax, __shfl_xor(xmax, d)); ymax = max(ymax, __shfl_xor(ymax, d));
    }
    if ((t & 63) == 0) { s_red[t >> 6][0] = xmin; s_red[t >> 6][1] = ymin; s_red[t >> 6][2] = xmax; s_red[t >> 6][3] = ymax; }
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < MASK_THREADS / 64; ++q) {
            xmin = min(xmin, s_red[q][0]); ymin = min(ymin, s_red[q][1]); xmax = max(xmax, s_red[q][2]); ymax = max(ymax, s_red[q][3]);
        }
        ws[(size_t)n * gridDim.x + b] = make_int4(xmin, ymin, xmax, ymax);     // every band of every mask, a band without a pixel too
    }
}

__global__ __launch_bounds__(64)
void mask_boxes_combine_kernel(const int4* __restrict__ ws, int bands, float* __restrict__ out)
{
    const int n = blockIdx.x, t = threadIdx.x;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (int b = t; b < bands; b += 64) {
        const int4 r = ws[(size_t)n * bands + b];
        xmin = min(xmin, r.x); ymin = min(ymin, r.y); xmax = max(xmax, r.z); ymax = max(ymax, r.w);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, d)); ymin = min(ymin, __shfl_xor(ymin, d));
        xmax = max(xmax, __shfl_xor(xmax, d)); ymax = max(ymax, __shfl_xor(ymax, d));
    }
    if (t == 0) {
        const bool any = xmax >= 0;                                            // an all-zero mask: (0, 0, 0, 0)
        float* o = out + 4 * (size_t)n;
        o[0] = any ? (float)xmin : 0.f; o[1] = any ? (float)ymin : 0.f; o[2] = any ? (float)xmax : 0.f; o[3] = any ? (float)ymax : 0.f;
    }
}

static int mask_boxes_bands(int h, int w, int elem_bytes) { return max(1, cdiv((int)((long long)h * w / (16 / elem_bytes)), MASK_PIECE)); }

template <typename Z, unsigned KEEP>
static int mask_boxes_launch(const void* masks, int n, int h, int w, float* out, int4* ws, hipStream_t s)
{
    const int hw = h * w, bands = mask_boxes_bands(h, w, (int)sizeof(Z));
    for (int n0 = 0; n0 < n; n0 += MASK_GRID_Y) {
        const int nn = min(n - n0, MASK_GRID_Y);
        hipLaunchKernelGGL((mask_boxes_band_kernel<Z, KEEP>), dim3(bands, nn), dim3(MASK_THREADS), 0, s,
                           static_cast<const Z*>(masks) + (size_t)n0 * hw, hw, w, ws);
        int rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(mask_boxes_combine_kernel, dim3(nn), dim3(64), 0, s, ws, bands, out + 4 * (size_t)n0);
        rc = check_launch();
        if (rc) return rc;
    }
    return FRCNN_OK;
}

static bool mask_image_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * w <= MASK_MAX_PLANE; }

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_paste_masks_max_side(void) { return MASK_MAX_SIDE; }
int frcnn_ops_paste_masks_max_padding(void) { return MASK_MAX_PADDING; }
int frcnn_ops_paste_masks_max_corner(void) { return (int)MASK_CORNER; }
int frcnn_ops_mask_max_plane(void) { return (int)MASK_MAX_PLANE; }

int frcnn_ops_paste_masks_in_image(int elem_type, const void* d_masks, const float* d_boxes, int k, int m, int padding, int h, int w,
                                   void* d_out, void* stream)
{
    if (elem_type != FRCNN_OPS_F32 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    if (k < 0 || m < 1 || m > MASK_MAX_SIDE || padding < 0 || padding > MASK_MAX_PADDING || !mask_image_ok(h, w)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    const uintptr_t align = elem_type == FRCNN_OPS_F32 ? 3 : 1;
    if (!d_masks || !d_boxes || !d_out || (reinterpret_cast<uintptr_t>(d_out) & align)) return FRCNN_EINVAL;
    const PasteArgs a = {m, m, padding, h, w, h * w, (float)((double)(m + 2 * padding) / (double)m), 0.f, 0};
    const hipStream_t s = (hipStream_t)stream;
    if (elem_type == FRCNN_OPS_F32) return paste_launch<float, float, PasteInImage, 16>(d_masks, d_boxes, d_out, k, a, s);
    OPS_ELEM_DISPATCH(elem_type, E, paste_launch<E, E, PasteInImage, 16>(d_masks, d_boxes, d_out, k, a, s));
}

int frcnn_ops_paste_masks_aligned(int elem_type, const void* d_masks, const float* d_boxes, int k, int mh, int mw, int h, int w,
                                  float threshold, int as_uint8, uint8_t* d_out, void* stream)
{
    if (elem_type != FRCNN_OPS_F32 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    if (k < 0 || mh < 1 || mh > MASK_MAX_SIDE || mw < 1 || mw > MASK_MAX_SIDE || !mask_image_ok(h, w)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_masks || !d_boxes || !d_out) return FRCNN_EINVAL;
    const PasteArgs a = {mh, mw, 0, h, w, h * w, 1.f, threshold, as_uint8 != 0};
    const hipStream_t s = (hipStream_t)stream;
    if (elem_type == FRCNN_OPS_F32) return paste_launch<float, uint8_t, PasteAligned, PASTE_BYTE_VECTOR>(d_masks, d_boxes, d_out, k, a, s);
    OPS_ELEM_DISPATCH(elem_type, E, paste_launch<E, uint8_t, PasteAligned, PASTE_BYTE_VECTOR>(d_masks, d_boxes, d_out, k, a, s));
}

size_t frcnn_ops_masks_to_boxes_workspace_bytes(int n, int h, int w, int elem_bytes)
{
    if (n < 1 || !mask_image_ok(h, w) || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)) return 0;
    return (size_t)min(n, MASK_GRID_Y) * mask_boxes_bands(h, w, elem_bytes) * sizeof(int4);
}

int frcnn_ops_masks_to_boxes(int elem_bytes, const void* d_masks, int n, int h, int w, float* d_out, void* d_ws, size_t ws_bytes,
                             void* stream)
{
    if (n < 0 || !mask_image_ok(h, w) || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_masks || !d_out || !d_ws || (reinterpret_cast<uintptr_t>(d_ws) & 15) || (reinterpret_cast<uintptr_t>(d_masks) & (elem_bytes - 1)))
        return FRCNN_EINVAL;
    if (ws_bytes < frcnn_ops_masks_to_boxes_workspace_bytes(n, h, w, elem_bytes)) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    int4* ws = static_cast<int4*>(d_ws);
    if (elem_bytes == 1) return mask_boxes_launch<uint8_t, 0xFFu>(d_masks, n, h, w, d_out, ws, s);
    if (elem_bytes == 2) return mask_boxes_launch<uint16_t, 0x7FFFu>(d_masks, n, h, w, d_out, ws, s);
    return mask_boxes_launch<uint32_t, 0x7FFFFFFFu>(d_masks, n, h, w, d_out, ws, s);
}

}  // extern "C"
