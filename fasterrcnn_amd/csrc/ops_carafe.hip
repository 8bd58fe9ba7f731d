// ops_carafe.hip -- CARAFE, content-aware reassembly of features (the learned upsampler of mmdetection's FPN_CARAFE necks): mmcv's
// carafe forward and both gradients (the frcnn_ops_carafe* entry points of include/frcnn_hip.h).  Restated from the published
// definition (third party, absent here: restated, unpinned; where the two differ include/frcnn_hip.h holds).
//
//   out[n, c, ph, pw] = sum over i, j in [0, k) of x[n, c, ph / s - r + i, pw / s - r + j] * mask[n, (g k + i) k + j, ph, pw]
//   r = (k - 1) / 2, g = c / (C / G); a tap outside the map contributes nothing (zero padding).
//
// Layouts: plain NCHW -- x [n][C][h][w], masks [n][G k k][s h][s w], out [n][C][s h][s w] -- what torch's convolutions, pixel_shuffle
// and softmax produce and what the next convolution consumes.  The operator is a memory-bound gather: no atomics, no workspace.
//
// Forward: a block owns CARAFE_TILE_H rows of CARAFE_TILE_W output pixels, lanes along pw, so mask planes and result rows are coalesced
// 256-byte lines.  A thread loads the k k mask values of its pixel once into registers (k is a template argument: 1, 3, 5, 7 are all
// the odd sizes up to CARAFE_MAX_KERNEL) and walks CARAFE_CHUNK channels of its group.  The block stages the low-resolution cells its
// windows cover in LDS, CARAFE_STAGE channels at a time, widened to float32 and with the zero padding written in; a thread then reads
// its k x k window at immediate offsets from one LDS address (neighbouring lanes read the same or adjacent words: no bank conflict)
// and adds each tap with one fused multiply-add, rows outer, columns inner.  Grid: (pixel tiles, channel chunks x groups, n): the
// masks are read once per chunk of channels, not once per channel, and every map cell once per tile that covers it.
// d_masks: the same tiling with k k accumulators per pixel over ALL the channels of the group in ascending order (grid: pixel tiles,
// groups, n), each accumulator stored once; a tap outside the map stores 0.
// d_features: a thread owns CARAFE_RUN consecutive channels of one low-resolution cell (lanes along x) and gathers its k k s s
// contributions in a fixed order -- low-resolution neighbour (qy, qx) row-major, then sub-pixel (sy, sx) row-major; the mask value of a
// contribution is loaded once for the run.  Bit-identical from run to run.
//
// Element types: templates over the storage type E (float, float16, bfloat16: ops_elem.h): widened exactly on load, every product and
// sum in float32 in one shared body (each term one explicit fmaf), rounded once to nearest even on store as Tensor.to() rounds, so
// op(x_T, m_T) == op(x_T.float(), m_T.float()).to(T) bit for bit, forward and backward.
// Indices: 64-bit plane bases, 32-bit inside a plane (s h s w < 2^31, checked by the entry points).
#include "ops_elem.h"

namespace frcnn {

static constexpr int CARAFE_MAX_KERNEL = 7;   // k odd, 1 <= k <= 7: k k = 49 registers of masks (forward) or accumulators (d_masks)
static constexpr int CARAFE_MAX_SCALE = 8;
static constexpr int CARAFE_CHUNK = 64;       // channels a forward block walks with one load of its masks
static constexpr int CARAFE_STAGE = 8;        // channels whose low-resolution window a block stages in LDS at a time
static constexpr int CARAFE_RUN = 4;          // channels a d_features thread owns
static constexpr int CARAFE_TILE_W = 64;      // output pixels along pw: one wave
static constexpr int CARAFE_TILE_H = 4;       // rows of a block: one per wave
static constexpr int CARAFE_BLOCK = CARAFE_TILE_W * CARAFE_TILE_H;

// the cell of a thread in a tile of CARAFE_TILE_H rows of CARAFE_TILE_W cells: blockIdx.x = tile row * tiles_w + tile column
__device__ __forceinline__ bool carafe_pixel(int out_h, int out_w, int& ph, int& pw)
{
    const int tiles_w = (out_w + CARAFE_TILE_W - 1) / CARAFE_TILE_W;
    const int ty = blockIdx.x / tiles_w, tx = blockIdx.x - ty * tiles_w;
    pw = tx * CARAFE_TILE_W + (threadIdx.x & (CARAFE_TILE_W - 1));
    ph = ty * CARAFE_TILE_H + threadIdx.x / CARAFE_TILE_W;
    return ph < out_h && pw < out_w;
}

// The low-resolution window of a tile of output pixels, staged in LDS as float32 with the zero padding written into it: the cells
// [qy0, qy0 + th) x [qx0, qx0 + tw) that the windows of the tile's pixels cover (th <= CARAFE_TILE_H + K - 1 rows of pitch
// CARAFE_TILE_W + K - 1: both reached at s == 1), for CARAFE_STAGE channels at a time.  A thread's window starts at `base`; tap (i, j)
// is an immediate offset from it, so the k k reads of a channel need one address register.
template <int K> struct CarafeTile {
    static constexpr int R = (K - 1) / 2, P = CARAFE_TILE_W + K - 1, TH = CARAFE_TILE_H + K - 1;
    int qy0, qx0, th, tw, base, ph, pw;
    bool active;
    unsigned yok, xok;                       // the taps of the thread's window that lie inside the map, by row and by column

    __device__ __forceinline__ CarafeTile(int fh, int fw, int s)
    {
        const int out_h = fh * s, out_w = fw * s;
        active = carafe_pixel(out_h, out_w, ph, pw);
        const int ph0 = ph - (int)(threadIdx.x / CARAFE_TILE_W), pw0 = pw - (int)(threadIdx.x & (CARAFE_TILE_W - 1));
        const int cy0 = ph0 / s, cx0 = pw0 / s;
        qy0 = cy0 - R; qx0 = cx0 - R;
        th = min(ph0 + CARAFE_TILE_H - 1, out_h - 1) / s - cy0 + K;
        tw = min(pw0 + CARAFE_TILE_W - 1, out_w - 1) / s - cx0 + K;
        const int cy = ph / s, cx = pw / s;
        base = active ? (cy - cy0) * P + (cx - cx0) : 0;
        yok = xok = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (cy - R + i >= 0 && cy - R + i < fh) yok |= 1u << i;
            if (cx - R + i >= 0 && cx - R + i < fw) xok |= 1u << i;
        }
    }

    // channels [c0, c0 + nc) of image n into s_x: rows over the waves, cells over the lanes
    template <typename E>
    __device__ __forceinline__ void stage(float* s_x, const E* __restrict__ x, int n, int C, int fh, int fw, int c0, int nc) const
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int row = wave; row < nc * th; row += CARAFE_BLOCK / 64) {
            const int ch = row / th, ty = row - ch * th, y = qy0 + ty;
            const bool yin = y >= 0 && y < fh;
            const E* const xr = x + (((size_t)n * C + c0 + ch) * fh + (yin ? y : 0)) * fw;
            for (int tx = lane; tx < tw; tx += 64) {
                const int xx = qx0 + tx;
                s_x[(ch * TH + ty) * P + tx] = yin && xx >= 0 && xx < fw ? Elem<E>::load(xr, (size_t)xx) : 0.f;
            }
        }
    }
};

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <typename E, int K>
__global__ __launch_bounds__(CARAFE_BLOCK)
void ops_carafe_kernel(const E* __restrict__ x, const E* __restrict__ masks, int C, int fh, int fw, int G, int s, int chunks,
                       E* __restrict__ out)
{
    typedef CarafeTile<K> T;
    __shared__ float s_x[CARAFE_STAGE * T::TH * T::P];
    const T t(fh, fw, s);
    const int n = blockIdx.z, g = blockIdx.y / chunks, chunk = blockIdx.y - g * chunks;
    const int cg = C / G, c_lo = g * cg + chunk * CARAFE_CHUNK, c_hi = min(c_lo + CARAFE_CHUNK, (g + 1) * cg);
    const size_t plane = (size_t)fh * s * fw * s, pix = t.active ? (size_t)t.ph * (fw * s) + t.pw : 0;
    const E* const mp = masks + ((size_t)n * G + g) * (K * K) * plane + pix;
    float m[K * K];
#pragma unroll
    for (int k = 0; k < K * K; ++k) m[k] = t.active ? Elem<E>::load(mp, (size_t)k * plane) : 0.f;
    for (int c0 = c_lo; c0 < c_hi; c0 += CARAFE_STAGE) {
        const int nc = min(CARAFE_STAGE, c_hi - c0);
        __syncthreads();                                 // the previous channels have been read
        t.stage(s_x, x, n, C, fh, fw, c0, nc);
        __syncthreads();
        if (!t.active) continue;
        for (int ch = 0; ch < nc; ++ch) {
            const float* const w = s_x + ch * (T::TH * T::P) + t.base;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) acc = fmaf(w[i * T::P + j], m[i * K + j], acc);
            Elem<E>::store(out, ((size_t)n * C + c0 + ch) * plane + pix, acc);
        }
    }
}

// ---- d_masks -----------------------------------------------------------------------------------------------------------------------------
template <typename E, int K>
__global__ __launch_bounds__(CARAFE_BLOCK)
void ops_carafe_backward_masks_kernel(const E* __restrict__ x, const E* __restrict__ dout, int C, int fh, int fw, int G, int s,
                                      E* __restrict__ dmasks)
{
    typedef CarafeTile<K> T;
    __shared__ float s_x[CARAFE_STAGE * T::TH * T::P];
    const T t(fh, fw, s);
    const int n = blockIdx.z, g = blockIdx.y;
    const int cg = C / G, c_lo = g * cg, c_hi = c_lo + cg;
    const size_t plane = (size_t)fh * s * fw * s, pix = t.active ? (size_t)t.ph * (fw * s) + t.pw : 0;
    float acc[K * K];
#pragma unroll
    for (int k = 0; k < K * K; ++k) acc[k] = 0.f;
    for (int c0 = c_lo; c0 < c_hi; c0 += CARAFE_STAGE) {
        const int nc = min(CARAFE_STAGE, c_hi - c0);
        __syncthreads();                                 // the previous channels have been read
        t.stage(s_x, x, n, C, fh, fw, c0, nc);
        __syncthreads();
        if (!t.active) continue;
        for (int ch = 0; ch < nc; ++ch) {
            const float* const w = s_x + ch * (T::TH * T::P) + t.base;
            const float d = Elem<E>::load(dout, ((size_t)n * C + c0 + ch) * plane + pix);
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) acc[i * K + j] = fmaf(d, w[i * T::P + j], acc[i * K + j]);
        }
    }
    if (!t.active) return;
    E* const dp = dmasks + ((size_t)n * G + g) * (K * K) * plane + pix;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const bool ok = ((t.yok >> i) & (t.xok >> j) & 1u) != 0;     // exactly 0 outside the map, whatever the gradient holds
            Elem<E>::store(dp, (size_t)(i * K + j) * plane, ok ? acc[i * K + j] : 0.f);
        }
}

// ---- d_features ----------------------------------------------------------------------------------------------------------------------------
// grid: (cell tiles, runs of CARAFE_RUN channels x groups, n); a run never crosses its group: the channels past the group's end are
// computed on the group's last channel and not stored
template <typename E, int K>
__global__ __launch_bounds__(CARAFE_BLOCK)
void ops_carafe_backward_features_kernel(const E* __restrict__ masks, const E* __restrict__ dout, int C, int fh, int fw, int G, int s,
                                         int runs, E* __restrict__ dx)
{
    int y, xx;
    if (!carafe_pixel(fh, fw, y, xx)) return;
    const int n = blockIdx.z, g = blockIdx.y / runs, run = blockIdx.y - g * runs;
    const int cg = C / G, c0 = g * cg + run * CARAFE_RUN, c_end = (g + 1) * cg;
    constexpr int R = (K - 1) / 2;
    const int out_w = fw * s;
    const size_t plane = (size_t)fh * s * out_w;
    const E* const mp = masks + ((size_t)n * G + g) * (K * K) * plane;
    const E* dp[CARAFE_RUN];
#pragma unroll
    for (int u = 0; u < CARAFE_RUN; ++u) dp[u] = dout + ((size_t)n * C + min(c0 + u, c_end - 1)) * plane;
    float acc[CARAFE_RUN];
#pragma unroll
    for (int u = 0; u < CARAFE_RUN; ++u) acc[u] = 0.f;
    // the window of the output pixels of low-resolution cell (qy, qx) holds (y, xx) at tap (i, j) = (y - qy + R, xx - qx + R)
#pragma unroll
    for (int a = 0; a < K; ++a) {
        const int qy = y - R + a, i = K - 1 - a;
        if (qy < 0 || qy >= fh) continue;
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const int qx = xx - R + b, j = K - 1 - b;
            if (qx < 0 || qx >= fw) continue;
            const E* const mt = mp + (size_t)(i * K + j) * plane;
            for (int sy = 0; sy < s; ++sy) {
                const size_t row = (size_t)(qy * s + sy) * out_w + (size_t)qx * s;
                for (int sx = 0; sx < s; ++sx) {
                    const float m = Elem<E>::load(mt, row + sx);
#pragma unroll
                    for (int u = 0; u < CARAFE_RUN; ++u) acc[u] = fmaf(Elem<E>::load(dp[u], row + sx), m, acc[u]);
                }
            }
        }
    }
    const size_t cell = (size_t)y * fw + xx;
#pragma unroll
    for (int u = 0; u < CARAFE_RUN; ++u)
        if (c0 + u < c_end) Elem<E>::store(dx, ((size_t)n * C + c0 + u) * fh * fw + cell, acc[u]);
}

// ---- the entry points' bodies, one per element type ---------------------------------------------------------------------------------
// The limits of the launch grids: tiles in x, (chunks or runs) x groups in y, images in z; 32-bit indices inside one plane.
static bool carafe_args_ok(int n, int c, int h, int w, int k, int group, int s)
{
    if (n < 1 || n > 65535 || c < 1 || h < 1 || w < 1) return false;
    if (k < 1 || k > CARAFE_MAX_KERNEL || k % 2 == 0 || s < 1 || s > CARAFE_MAX_SCALE) return false;
    if (group < 1 || c % group != 0) return false;
    if ((size_t)h * s * (size_t)w * s > (size_t)INT32_MAX - 1024) return false;
    const size_t cg = (size_t)(c / group);
    return (size_t)group * ((cg + CARAFE_RUN - 1) / CARAFE_RUN) <= 65535;       // the runs: at least as many as the chunks
}

static unsigned carafe_tiles(int h, int w) { return (unsigned)cdiv(w, CARAFE_TILE_W) * (unsigned)cdiv(h, CARAFE_TILE_H); }

template <typename E, int K>
static int carafe_forward_launch(const E* x, const E* masks, int n, int c, int h, int w, int group, int s, E* out, hipStream_t stream)
{
    const int chunks = cdiv(c / group, CARAFE_CHUNK);
    hipLaunchKernelGGL((ops_carafe_kernel<E, K>), dim3(carafe_tiles(h * s, w * s), chunks * group, n), dim3(CARAFE_BLOCK), 0, stream,
                       x, masks, c, h, w, group, s, chunks, out);
    return check_launch();
}

template <typename E, int K>
static int carafe_backward_launch(const E* x, const E* masks, const E* dout, int n, int c, int h, int w, int group, int s, E* dx,
                                  E* dmasks, hipStream_t stream)
{
    if (dx) {
        const int runs = cdiv(c / group, CARAFE_RUN);
        hipLaunchKernelGGL((ops_carafe_backward_features_kernel<E, K>), dim3(carafe_tiles(h, w), runs * group, n), dim3(CARAFE_BLOCK), 0,
                           stream, masks, dout, c, h, w, group, s, runs, dx);
        const int rc = check_launch();
        if (rc != FRCNN_OK) return rc;
    }
    if (dmasks) {
        hipLaunchKernelGGL((ops_carafe_backward_masks_kernel<E, K>), dim3(carafe_tiles(h * s, w * s), group, n), dim3(CARAFE_BLOCK), 0,
                           stream, x, dout, c, h, w, group, s, dmasks);
        return check_launch();
    }
    return FRCNN_OK;
}

// k is one of 1, 3, 5, 7 (carafe_args_ok)
#define CARAFE_BY_KERNEL(k, launch, ...)                          \
    do {                                                          \
        if ((k) == 1) return launch<E, 1>(__VA_ARGS__);           \
        if ((k) == 3) return launch<E, 3>(__VA_ARGS__);           \
        if ((k) == 5) return launch<E, 5>(__VA_ARGS__);           \
        return launch<E, 7>(__VA_ARGS__);                         \
    } while (0)

template <typename E>
static int carafe_impl(const void* d_features, const void* d_masks, int n, int c, int h, int w, int k, int group, int s, void* d_out,
                       void* stream)
{
    if (!carafe_args_ok(n, c, h, w, k, group, s) || !d_features || !d_masks || !d_out) return FRCNN_EINVAL;
    CARAFE_BY_KERNEL(k, carafe_forward_launch, static_cast<const E*>(d_features), static_cast<const E*>(d_masks), n, c, h, w, group, s,
                     static_cast<E*>(d_out), (hipStream_t)stream);
}

template <typename E>
static int carafe_backward_impl(const void* d_features, const void* d_masks, const void* d_dout, int n, int c, int h, int w, int k,
                                int group, int s, void* d_dfeatures, void* d_dmasks, void* stream)
{
    if (!carafe_args_ok(n, c, h, w, k, group, s) || !d_dout) return FRCNN_EINVAL;
    if ((d_dfeatures && !d_masks) || (d_dmasks && !d_features)) return FRCNN_EINVAL;
    CARAFE_BY_KERNEL(k, carafe_backward_launch, static_cast<const E*>(d_features), static_cast<const E*>(d_masks),
                     static_cast<const E*>(d_dout), n, c, h, w, group, s, static_cast<E*>(d_dfeatures), static_cast<E*>(d_dmasks),
                     (hipStream_t)stream);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_carafe_max_kernel(void) { return CARAFE_MAX_KERNEL; }
int frcnn_ops_carafe_channel_chunk(void) { return CARAFE_CHUNK; }
int frcnn_ops_carafe_tile_width(void) { return CARAFE_TILE_W; }
int frcnn_ops_carafe_tile_height(void) { return CARAFE_TILE_H; }

int frcnn_ops_carafe(const float* d_features, const float* d_masks, int n, int c, int h, int w, int kernel_size, int group_size,
                     int scale_factor, float* d_out, void* stream)
{
    return carafe_impl<float>(d_features, d_masks, n, c, h, w, kernel_size, group_size, scale_factor, d_out, stream);
}

int frcnn_ops_carafe_backward(const float* d_features, const float* d_masks, const float* d_dout, int n, int c, int h, int w,
                              int kernel_size, int group_size, int scale_factor, float* d_dfeatures, float* d_dmasks, void* stream)
{
    return carafe_backward_impl<float>(d_features, d_masks, d_dout, n, c, h, w, kernel_size, group_size, scale_factor, d_dfeatures,
                                       d_dmasks, stream);
}

int frcnn_ops_carafe_16(int elem_type, const void* d_features, const void* d_masks, int n, int c, int h, int w, int kernel_size,
                        int group_size, int scale_factor, void* d_out, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E,
                      carafe_impl<E>(d_features, d_masks, n, c, h, w, kernel_size, group_size, scale_factor, d_out, stream));
}

int frcnn_ops_carafe_backward_16(int elem_type, const void* d_features, const void* d_masks, const void* d_dout, int n, int c, int h,
                                 int w, int kernel_size, int group_size, int scale_factor, void* d_dfeatures, void* d_dmasks,
                                 void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, carafe_backward_impl<E>(d_features, d_masks, d_dout, n, c, h, w, kernel_size, group_size, scale_factor,
                                                            d_dfeatures, d_dmasks, stream));
}

}  // extern "C"
