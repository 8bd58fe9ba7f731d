// ops_droi.hip -- deformable RoI pooling (DCN v1 / v2, mmcv's deform_roi_pool) over N images with deterministic backward passes: the
// frcnn_ops_deform_roi_pool* entry points of include/frcnn_hip.h.  Restated from the published definition of mmcv's deform_roi_pool
// (third party, absent here: restated, unpinned); where the two differ the header's text holds.
//
// The operator is aligned RoIAlign (roi_align_geom(.., aligned = 1)) whose bin (ph, pw) of RoI r samples a window shifted by a learned
// offset: start_w += gamma roi_w offset[r][0][ph][pw], start_h += gamma roi_h offset[r][1][ph][pw] (channel 0 is x); bin sizes and
// sampling grids are the RoI's own.  A sample outside [-1, size] or at a NaN / infinite coordinate contributes nothing (the range test
// fails for NaN, before any conversion to an integer).
//
// Layouts: ops.hip's.  The map is NHWC [n][h][w][c], the pooled output [k][out_h][out_w][c], a lane owns a run of channels (16 bytes: 4
// floats or 8 sixteen-bit values); offsets and their gradient are float32 [k][2][out_h][out_w].
// Forward: one block per (RoI, ph), lanes over (pw, channel run), with align_row's expressions in align_row's order: at a zero or
// absent offset the output is frcnn_ops_roi_align(aligned = 1) bit for bit.
// d_offset: one wave per (RoI, bin), lanes over channel runs; a lane sums its channels over the samples in (iy, ix) order, a fixed
// butterfly adds the 64 lanes, lane 0 scales by gamma roi and stores.  No atomics.
// d_x: no atomics.  With offsets the bins of a RoI no longer form one product grid, but the samples of one bin still do.  A plan launch
// writes per (RoI, bin) the shifted start and the inclusive window of cells its samples can touch, and per RoI the union of the windows
// and the image; the gather -- one block per 2 x 2 cells of one image and 64 channel runs -- culls the RoIs against the union (in
// ascending order, DROI_LIST at a time), each wave owns one cell and tests the bins of every listed RoI against their own windows, and
// a bin that holds the cell sends dout (sum of its row weights) (sum of its column weights) / count, in ascending (RoI, ph, pw) order.
// The sum stays in registers over every culling pass and is stored once: bit-identical from run to run, and a 16-bit d_x never holds a
// partial sum.  A window derived from a NaN coordinate lists nothing; an infinite one is clamped off the map.
// Known and unmeasured: a 16-bit gather always walks runs of 8 channels, so below C = 512 a wave (one cell's runs) is partly idle, where
// ops.hip narrows its runs to 4; and a wave reads all out_h x out_w windows of every listed RoI, with no cut finer than the RoI's union.
//
// Element types: templates over the storage type E of maps, outputs and their gradients (float, float16, bfloat16): widened exactly on
// load, geometry, weights and sums in float32 in one shared body, rounded once on store (ops_elem.h), so that
// op(x_T) == op(x_T.float()).to(T) bit for bit for the output and d_x.
#include "ops_geom.h"
#include "ops_elem.h"
#include <climits>
#include <cstdint>

namespace frcnn {

static constexpr int DROI_LIST = 256;          // RoIs culled per pass of a tile; >= 256, the RoIs one culling step examines
static constexpr int DROI_TILE = 2;            // backward tile: 2 x 2 cells, one per wave
static constexpr int DROI_MAX_OUT = 64;        // out_h, out_w <= 64
static constexpr int DROI_MAX_SAMPLING = 16;   // sampling_ratio <= 16
static_assert(DROI_LIST >= 256, "a culling step of 256 RoIs must fit an empty list");

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
// the aligned RoIAlign plan of a RoI with the sizes that scale its offsets
struct DroiGeom { RoiGeom g; float roi_h, roi_w; };

__device__ __forceinline__ DroiGeom droi_geom(const float* roi, float scale, int out_h, int out_w, int sampling_ratio)
{
    DroiGeom d;
    d.g = ops_align_geom(roi, scale, out_h, out_w, sampling_ratio, 1);
    d.roi_w = (roi[3] * scale - 0.5f) - d.g.start_w;       // roi_align_geom's end - start
    d.roi_h = (roi[4] * scale - 0.5f) - d.g.start_h;
    return d;
}

// the window start of bin `bin`; off: the RoI's offsets [2][bins] (x, then y), or null for none
__device__ __forceinline__ void droi_start(const DroiGeom& d, const float* __restrict__ off, int bins, int bin, float gamma, float& sh,
                                           float& sw)
{
    sh = d.g.start_h; sw = d.g.start_w;
    if (off) {
        sw = sw + gamma * d.roi_w * off[bin];
        sh = sh + gamma * d.roi_h * off[bins + bin];
    }
}

// axis_weights behind a range test that NaN fails: a NaN or infinite coordinate never reaches the conversion to an integer
__device__ __forceinline__ bool droi_axis(float v, int n, int& low, int& high, float& wl, float& wh)
{
    if (!(v >= -1.0f && v <= (float)n)) return false;
    return axis_weights(v, n, low, high, wl, wh);
}

__device__ __forceinline__ bool droi_cell_weight(float v, int n, int cell, float& w)
{
    if (!(v >= -1.0f && v <= (float)n)) return false;
    return cell_weight(v, n, cell, w);
}

// The cells [lo, hi] of an axis of `size` cells that a bin's samples can touch, from its first and last sample (the coordinates between
// them are monotone): one cell of margin on either side of their footprints, cut to the map.  lo > hi: none.  A NaN coordinate lists
// nothing (with a NaN at either end every sample of the bin is NaN or infinite); an infinite one is clamped in float first (the
// conversion of an out-of-range float is undefined) and ends off the map.  The gather tests each sample exactly.
__device__ __forceinline__ void droi_window(float start, float bin, int grid, int p, int size, int& lo, int& hi)
{
    const float a = sample_coord(start, bin, grid, p, 0), b = sample_coord(start, bin, grid, p, grid - 1);
    if (a != a || b != b) { lo = 1; hi = 0; return; }
    lo = (int)fminf(fmaxf(floorf(fminf(a, b)) - 1.0f, 0.0f), 2.0e9f);
    hi = min((int)fmaxf(fminf(ceilf(fmaxf(a, b)) + 1.0f, 2.0e9f), -1.0f), size - 1);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256)
void ops_droi_forward_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois,
                             const float* __restrict__ offset, int out_h, int out_w, float scale, int sampling_ratio, float gamma,
                             E* __restrict__ out)
{
    typedef ElemRun<E, ELEM_WIDE_RUN<E>> R;
    typedef typename R::vec vec;
    const int r = blockIdx.x, ph = blockIdx.y, C4 = C / R::V, bins = out_h * out_w;
    const float* roi = rois + (size_t)r * 5;
    E* orow = out + ((size_t)r * out_h + ph) * out_w * C;
    int b;
    if (!roi_image(roi[0], n_img, b)) {
        const vec z = 0.f;
        for (int i = threadIdx.x; i < out_w * C4; i += 256) R::store(orow, i, z);
        return;
    }
    const DroiGeom d = droi_geom(roi, scale, out_h, out_w, sampling_ratio);
    const RoiGeom& g = d.g;
    const E* fm = x + (size_t)b * fh * fw * C;
    const float* off = offset ? offset + (size_t)r * 2 * bins : nullptr;
    // align_row's body (ops.hip) with the bin's own start: the same expressions in the same order
    for (int i = threadIdx.x; i < out_w * C4; i += 256) {
        const int pw = i / C4, c4 = i - pw * C4;
        float sh, sw;
        droi_start(d, off, bins, ph * out_w + pw, gamma, sh, sw);
        vec acc = 0.f;
        for (int iy = 0; iy < g.grid_h; ++iy) {
            const float y = sample_coord(sh, g.bin_h, g.grid_h, ph, iy);
            int yl = 0, yh = 0; float hy = 0.f, ly = 0.f;
            const bool yok = droi_axis(y, fh, yl, yh, hy, ly);
            for (int ix = 0; ix < g.grid_w; ++ix) {
                const float xx = sample_coord(sw, g.bin_w, g.grid_w, pw, ix);
                int xl, xh; float hx, lx;
                if (!yok || !droi_axis(xx, fw, xl, xh, hx, lx)) continue;
                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                const vec v1 = R::load(fm + ((size_t)yl * fw + xl) * C, c4);
                const vec v2 = R::load(fm + ((size_t)yl * fw + xh) * C, c4);
                const vec v3 = R::load(fm + ((size_t)yh * fw + xl) * C, c4);
                const vec v4 = R::load(fm + ((size_t)yh * fw + xh) * C, c4);
                acc = acc + (((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4);
            }
        }
        R::store(orow, i, acc / g.count);
    }
}

// ---- d_offset --------------------------------------------------------------------------------------------------------------------------
// One wave per (RoI, bin).  Per accepted sample at (y, x) -- the coordinates as computed, before axis_weights clamps them: the published
// formula -- with corners v1 (yl, xl), v2 (yl, xh), v3 (yh, xl), v4 (yh, xh) and g = dout / count:
//   d_offset x += g (v4 (y - yl) + v2 (yh - y) + v3 (yl - y) + v1 (y - yh)),  d_offset y += g (v4 (x - xl) + v3 (xh - x) + v2 (xl - x) + v1 (x - xh)),
// summed over the channels and scaled by gamma roi_w / gamma roi_h once.  A lane owns the channels 4 (lane + 64 j) .. + 3 whatever the
// element type, so the 16-bit kernels' d_offset is the float32 kernel's on the widened values, bit for bit.
template <typename E>
__global__ __launch_bounds__(256)
void ops_droi_offset_grad_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois,
                                 const float* __restrict__ offset, int k, int out_h, int out_w, float scale, int sampling_ratio,
                                 float gamma, const E* __restrict__ dout, float* __restrict__ doffset)
{
    typedef ElemRun<E, 4> R;               // runs of 4 for every element type: the lanes' partial sums are those of the float32 kernel
    typedef typename R::vec vec;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = C / R::V, bins = out_h * out_w;
    const long long item = (long long)blockIdx.x * 4 + wave;                // wave-uniform
    if (item >= (long long)k * bins) return;
    const int r = (int)(item / bins), bin = (int)(item - (long long)r * bins);
    const int ph = bin / out_w, pw = bin - ph * out_w;
    const float* roi = rois + (size_t)r * 5;
    float gx = 0.f, gy = 0.f, scale_x = 0.f, scale_y = 0.f;
    int b;
    if (roi_image(roi[0], n_img, b)) {
        const DroiGeom d = droi_geom(roi, scale, out_h, out_w, sampling_ratio);
        const RoiGeom& g = d.g;
        scale_x = gamma * d.roi_w; scale_y = gamma * d.roi_h;
        const E* fm = x + (size_t)b * fh * fw * C;
        float sh, sw;
        droi_start(d, offset + (size_t)r * 2 * bins, bins, bin, gamma, sh, sw);
        for (int c4 = lane; c4 < C4; c4 += 64) {
            const vec gr = R::load(dout + ((size_t)r * bins + bin) * C, c4) / g.count;
            for (int iy = 0; iy < g.grid_h; ++iy) {
                const float y = sample_coord(sh, g.bin_h, g.grid_h, ph, iy);
                int yl = 0, yh = 0; float hy, ly;
                const bool yok = droi_axis(y, fh, yl, yh, hy, ly);
                for (int ix = 0; ix < g.grid_w; ++ix) {
                    const float xx = sample_coord(sw, g.bin_w, g.grid_w, pw, ix);
                    int xl, xh; float hx, lx;
                    if (!yok || !droi_axis(xx, fw, xl, xh, hx, lx)) continue;
                    const vec v1 = R::load(fm + ((size_t)yl * fw + xl) * C, c4);
                    const vec v2 = R::load(fm + ((size_t)yl * fw + xh) * C, c4);
                    const vec v3 = R::load(fm + ((size_t)yh * fw + xl) * C, c4);
                    const vec v4 = R::load(fm + ((size_t)yh * fw + xh) * C, c4);
                    const float fyl = (float)yl, fyh = (float)yh, fxl = (float)xl, fxh = (float)xh;
                    const vec tx = ((v4 * (y - fyl) + v2 * (fyh - y)) + v3 * (fyl - y)) + v1 * (y - fyh);
                    const vec ty = ((v4 * (xx - fxl) + v3 * (fxh - xx)) + v2 * (fxl - xx)) + v1 * (xx - fxh);
#pragma unroll
                    for (int j = 0; j < R::V; ++j) {
                        gx = gx + gr[j] * tx[j];
                        gy = gy + gr[j] * ty[j];
                    }
                }
            }
        }
    }
    // the 64 lanes in a fixed butterfly: every lane ends with the same sum
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        gx = gx + __shfl_xor(gx, o, 64);
        gy = gy + __shfl_xor(gy, o, 64);
    }
    if (lane == 0) {
        float* const dst = doffset + (size_t)r * 2 * bins;
        dst[bin] = scale_x * gx;
        dst[bins + bin] = scale_y * gy;
    }
}

// ---- d_x: the plan -----------------------------------------------------------------------------------------------------------------------
// Per (RoI, bin): win = (y_lo, y_hi, x_lo, x_hi) inclusive, y_lo > y_hi: the bin sends nothing; start = (start_h, start_w) shifted.
// Per RoI: rec[8] = (image or -1, union y_lo, y_hi, x_lo, x_hi, 0, 0, 0).  One block per RoI.
__global__ __launch_bounds__(256)
void ops_droi_plan_kernel(const float* __restrict__ rois, const float* __restrict__ offset, int n_img, int fh, int fw, int out_h, int out_w,
                          float scale, int sampling_ratio, float gamma, i32x4* __restrict__ win, int* __restrict__ rec,
                          f32x2* __restrict__ start)
{
    __shared__ int s_red[4][4];
    const int r = blockIdx.x, bins = out_h * out_w, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* roi = rois + (size_t)r * 5;
    int b = -1;
    bool ok = roi_image(roi[0], n_img, b);
    const DroiGeom d = droi_geom(roi, scale, out_h, out_w, sampling_ratio);
    ok = ok && d.g.grid_h > 0 && d.g.grid_w > 0;
    const float* off = offset ? offset + (size_t)r * 2 * bins : nullptr;
    int u0 = INT_MAX, u1 = -1, u2 = INT_MAX, u3 = -1;          // the union: min y_lo, max y_hi, min x_lo, max x_hi
    for (int bin = threadIdx.x; bin < bins; bin += 256) {
        i32x4 w = {1, 0, 1, 0};
        float sh = 0.f, sw = 0.f;
        if (ok) {
            const int ph = bin / out_w, pw = bin - ph * out_w;
            droi_start(d, off, bins, bin, gamma, sh, sw);
            int y_lo, y_hi, x_lo, x_hi;
            droi_window(sh, d.g.bin_h, d.g.grid_h, ph, fh, y_lo, y_hi);
            droi_window(sw, d.g.bin_w, d.g.grid_w, pw, fw, x_lo, x_hi);
            if (y_lo <= y_hi && x_lo <= x_hi) {
                w = i32x4{y_lo, y_hi, x_lo, x_hi};
                u0 = min(u0, y_lo); u1 = max(u1, y_hi); u2 = min(u2, x_lo); u3 = max(u3, x_hi);
            }
        }
        win[(size_t)r * bins + bin] = w;
        start[(size_t)r * bins + bin] = f32x2{sh, sw};
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        u0 = min(u0, __shfl_xor(u0, o, 64)); u1 = max(u1, __shfl_xor(u1, o, 64));
        u2 = min(u2, __shfl_xor(u2, o, 64)); u3 = max(u3, __shfl_xor(u3, o, 64));
    }
    if (lane == 0) { s_red[wave][0] = u0; s_red[wave][1] = u1; s_red[wave][2] = u2; s_red[wave][3] = u3; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            u0 = min(u0, s_red[w][0]); u1 = max(u1, s_red[w][1]); u2 = min(u2, s_red[w][2]); u3 = max(u3, s_red[w][3]);
        }
        int* const dst = rec + (size_t)r * 8;
        dst[0] = u0 <= u1 ? b : -1;
        dst[1] = u0; dst[2] = u1; dst[3] = u2; dst[4] = u3; dst[5] = 0; dst[6] = 0; dst[7] = 0;
    }
}

// ---- d_x: the gather ---------------------------------------------------------------------------------------------------------------------
// Ordered culling (the scheme of ops.hip's backward kernels): appends to s_list, in ascending order, the RoIs r >= r_begin for which
// touches(r) holds, until DROI_LIST are listed.  Returns the first RoI not examined (k when all were).  Block of 256 threads.
template <typename Touches>
__device__ int droi_cull(int r_begin, int k, Touches touches, int* s_list, int* s_cnt, int* s_n)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                     // the previous pass has finished reading s_list
    if (tid == 0) *s_n = 0;
    int r0 = r_begin;
    for (; r0 < k; r0 += 256) {
        const int r = r0 + tid;
        const bool hit = r < k && touches(r);
        const u64 m = __ballot(hit);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        const int base = *s_n;
        const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (base + total > DROI_LIST) break;             // uniform: the list is full; this group starts the next pass
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_cnt[w];
        if (hit) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        if (tid == 0) *s_n = base + total;
    }
    __syncthreads();
    return r0 < k ? r0 : k;
}

template <typename E>
__global__ __launch_bounds__(256)
void ops_droi_input_grad_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w, float scale,
                                int sampling_ratio, const i32x4* __restrict__ win, const int* __restrict__ rec,
                                const f32x2* __restrict__ start, const E* __restrict__ dout, E* __restrict__ dx)
{
    typedef ElemRun<E, ELEM_WIDE_RUN<E>> R;
    __shared__ int s_list[DROI_LIST];
    __shared__ int s_cnt[4];
    __shared__ int s_n;
    const int C4 = C / R::V, n_chunks = (C4 + 63) >> 6, bins = out_h * out_w;
    const int img = blockIdx.z / n_chunks, chunk = blockIdx.z - img * n_chunks;
    const int ty0 = blockIdx.y * DROI_TILE, tx0 = blockIdx.x * DROI_TILE;
    const int ty1 = min(ty0 + DROI_TILE, fh) - 1, tx1 = min(tx0 + DROI_TILE, fw) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = chunk * 64 + lane;
    const bool act = c4 < C4;
    const int cy = ty0 + wave / DROI_TILE, cx = tx0 + wave % DROI_TILE;       // this wave's cell, for every pass
    const bool cell_ok = cy <= ty1 && cx <= tx1;

    auto touches = [&](int r) {
        const int* u = rec + (size_t)r * 8;
        return u[0] == img && u[2] >= ty0 && u[1] <= ty1 && u[4] >= tx0 && u[3] <= tx1;
    };

    typename R::vec acc = 0.f;
    int r_next = 0;
    do {
        r_next = droi_cull(r_next, k, touches, s_list, s_cnt, &s_n);
        const int n_list = s_n;
        if (cell_ok)
            for (int li = 0; li < n_list; ++li) {
                const int r = __builtin_amdgcn_readfirstlane(s_list[li]);
                const RoiGeom g = ops_align_geom(rois + (size_t)r * 5, scale, out_h, out_w, sampling_ratio, 1);
                const E* const dr = dout + (size_t)r * bins * C;
                for (int bin = 0; bin < bins; ++bin) {
                    const i32x4 w = win[(size_t)r * bins + bin];
                    if (cy < w[0] || cy > w[1] || cx < w[2] || cx > w[3]) continue;
                    const f32x2 s = start[(size_t)r * bins + bin];
                    const int ph = bin / out_w, pw = bin - ph * out_w;
                    // the bin's samples form a grid_h x grid_w product, so the cell's weight in it is (the sum of its row weights) x
                    // (the sum of its column weights): one term per bin, as in ops.hip's align_cell_grad
                    float wy_sum = 0.f, wx_sum = 0.f;
                    bool y_hit = false, x_hit = false;
                    for (int iy = 0; iy < g.grid_h; ++iy) {
                        float wy;
                        if (droi_cell_weight(sample_coord(s[0], g.bin_h, g.grid_h, ph, iy), fh, cy, wy)) { wy_sum += wy; y_hit = true; }
                    }
                    if (!y_hit) continue;
                    for (int ix = 0; ix < g.grid_w; ++ix) {
                        float wx;
                        if (droi_cell_weight(sample_coord(s[1], g.bin_w, g.grid_w, pw, ix), fw, cx, wx)) { wx_sum += wx; x_hit = true; }
                    }
                    if (x_hit && act) acc = acc + (R::load(dr, (size_t)bin * C4 + c4) * (wy_sum * wx_sum)) / g.count;
                }
            }
    } while (r_next < k);
    if (cell_ok && act) R::store(dx + (size_t)img * fh * fw * C, ((size_t)cy * fw + cx) * C4 + c4, acc);
}

// ---- the entry points' bodies, one per element type ---------------------------------------------------------------------------------
// v: the channels of a lane's run.  The limits are those of the launch grids (the gather's: tile rows in y, image x channel chunk in z)
// and of the plan's 32-bit (RoI, bin) indices.
static bool droi_args_ok(int n_img, int fh, int fw, int c, int k, int out_h, int out_w, int sampling_ratio, int v)
{
    if (out_h < 1 || out_h > DROI_MAX_OUT || out_w < 1 || out_w > DROI_MAX_OUT || sampling_ratio > DROI_MAX_SAMPLING) return false;
    return n_img >= 1 && fh >= 1 && fw >= 1 && c >= v && c % v == 0 && k >= 0 && (size_t)fh * fw <= (size_t)INT32_MAX &&
           (size_t)n_img * cdiv(c / v, 64) <= 65535 && fh <= 65535 * DROI_TILE && (size_t)k * out_h * out_w <= (size_t)INT32_MAX;
}

static size_t droi_workspace_bytes(int k, int out_h, int out_w)
{
    return (size_t)k * out_h * out_w * (sizeof(i32x4) + sizeof(f32x2)) + (size_t)k * 8 * sizeof(int);
}

template <typename E>
static int droi_forward_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, const float* d_offset, int k,
                             int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma, void* d_out, void* stream)
{
    if (!droi_args_ok(n_img, fh, fw, c, k, out_h, out_w, sampling_ratio, ELEM_WIDE_RUN<E>)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_droi_forward_kernel<E>, dim3(k, out_h), dim3(256), 0, (hipStream_t)stream, static_cast<const E*>(d_x), n_img,
                       fh, fw, c, d_rois, d_offset, out_h, out_w, spatial_scale, sampling_ratio, gamma, static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int droi_backward_impl(const void* d_x, const float* d_rois, const float* d_offset, int k, int n_img, int fh, int fw, int c,
                              int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma, const void* d_dout, void* d_dx,
                              float* d_doffset, void* d_ws, size_t ws_bytes, void* stream)
{
    if (!droi_args_ok(n_img, fh, fw, c, k, out_h, out_w, sampling_ratio, ELEM_WIDE_RUN<E>)) return FRCNN_EINVAL;
    if (!d_dx && !d_doffset) return FRCNN_EINVAL;
    if (d_doffset && !d_offset) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (k == 0) {
        if (d_dx) FRCNN_HIP_TRY(hipMemsetAsync(d_dx, 0, (size_t)n_img * fh * fw * c * sizeof(E), s));
        return FRCNN_OK;
    }
    if (!d_rois || !d_dout || (d_doffset && !d_x)) return FRCNN_EINVAL;
    if (d_dx && (!d_ws || (uintptr_t)d_ws % 16 != 0 || ws_bytes < droi_workspace_bytes(k, out_h, out_w))) return FRCNN_EINVAL;
    const int bins = out_h * out_w;
    if (d_doffset) {
        hipLaunchKernelGGL(ops_droi_offset_grad_kernel<E>, dim3((unsigned)(((size_t)k * bins + 3) / 4)), dim3(256), 0, s,
                           static_cast<const E*>(d_x), n_img, fh, fw, c, d_rois, d_offset, k, out_h, out_w, spatial_scale, sampling_ratio,
                           gamma, static_cast<const E*>(d_dout), d_doffset);
        const int rc = check_launch();
        if (rc) return rc;
    }
    if (d_dx) {
        i32x4* const win = static_cast<i32x4*>(d_ws);
        int* const rec = reinterpret_cast<int*>(win + (size_t)k * bins);
        f32x2* const start = reinterpret_cast<f32x2*>(rec + (size_t)k * 8);
        hipLaunchKernelGGL(ops_droi_plan_kernel, dim3(k), dim3(256), 0, s, d_rois, d_offset, n_img, fh, fw, out_h, out_w, spatial_scale,
                           sampling_ratio, gamma, win, rec, start);
        const int rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(ops_droi_input_grad_kernel<E>,
                           dim3(cdiv(fw, DROI_TILE), cdiv(fh, DROI_TILE), n_img * cdiv(c / ELEM_WIDE_RUN<E>, 64)), dim3(256), 0, s, d_rois, k,
                           n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, win, rec, start, static_cast<const E*>(d_dout),
                           static_cast<E*>(d_dx));
        return check_launch();
    }
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_deform_roi_pool_cull_list(void) { return DROI_LIST; }

size_t frcnn_ops_deform_roi_pool_workspace_bytes(int k, int out_h, int out_w)
{
    if (k < 0 || out_h < 1 || out_h > DROI_MAX_OUT || out_w < 1 || out_w > DROI_MAX_OUT || (size_t)k * out_h * out_w > (size_t)INT32_MAX)
        return 0;
    return droi_workspace_bytes(k, out_h, out_w);
}

int frcnn_ops_deform_roi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, const float* d_offset, int k,
                              int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma, float* d_out, void* stream)
{
    return droi_forward_impl<float>(d_x, n_img, fh, fw, c, d_rois, d_offset, k, out_h, out_w, spatial_scale, sampling_ratio, gamma, d_out,
                                    stream);
}

int frcnn_ops_deform_roi_pool_backward(const float* d_x, const float* d_rois, const float* d_offset, int k, int n_img, int fh, int fw,
                                       int c, int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma,
                                       const float* d_dout, float* d_dx, float* d_doffset, void* d_ws, size_t ws_bytes, void* stream)
{
    return droi_backward_impl<float>(d_x, d_rois, d_offset, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, gamma, d_dout,
                                     d_dx, d_doffset, d_ws, ws_bytes, stream);
}

int frcnn_ops_deform_roi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois,
                                 const float* d_offset, int k, int out_h, int out_w, float spatial_scale, int sampling_ratio, float gamma,
                                 void* d_out, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, droi_forward_impl<E>(d_x, n_img, fh, fw, c, d_rois, d_offset, k, out_h, out_w, spatial_scale,
                                                         sampling_ratio, gamma, d_out, stream));
}

int frcnn_ops_deform_roi_pool_backward_16(int elem_type, const void* d_x, const float* d_rois, const float* d_offset, int k, int n_img,
                                          int fh, int fw, int c, int out_h, int out_w, float spatial_scale, int sampling_ratio,
                                          float gamma, const void* d_dout, void* d_dx, float* d_doffset, void* d_ws, size_t ws_bytes,
                                          void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, droi_backward_impl<E>(d_x, d_rois, d_offset, k, n_img, fh, fw, c, out_h, out_w, spatial_scale,
                                                          sampling_ratio, gamma, d_dout, d_dx, d_doffset, d_ws, ws_bytes, stream));
}

}  // extern "C"
