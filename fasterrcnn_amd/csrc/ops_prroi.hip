// ops_prroi.hip -- Precise RoI Pooling (PrRoIPool of IoU-Net; mmcv's prroi_pool) over N images with deterministic backward passes for the
// map AND the boxes: the frcnn_ops_prroi_pool* entry points of include/frcnn_hip.h.  Restated from the published definition (mmcv is
// third party, absent here: restated, unpinned); where the two differ the header's text holds.
//
// The operator integrates the bilinear surface of the map exactly over each bin: with hat(t) = max(0, 1 - |t|) and bin [xs, xe] x [ys, ye],
//   out = (sum over j, i of Wy(j) Wx(i) x[j][i]) / A,  Wx(i) = the integral of hat(x - i) over [xs, xe],  A = bin_w bin_h.
// Wx(i) is formed on the two unit pieces [i - 1, i] and [i, i + 1] cut to the bin, (length) x (value of hat at the midpoint): no
// difference of antiderivatives, which cancels for a bin much narrower than a cell (prroi_weight).  A RoI is pooled iff 0 < A < +inf in
// float32 and its batch index lies in [0, n_img): every NaN, infinite, empty or inverted box fails that, pools to zeros and sends and
// receives no gradient; a RoI that passes has finite bin edges, and every cell range is clamped in float before its conversion to int.
//
// Layouts: ops.hip's.  The map is NHWC [n][h][w][c], the pooled output [k][out_h][out_w][c], a lane owns a run of channels (16 bytes).
// Forward: one block per (RoI, ph), lanes over (pw, channel run).  The row weights Wy of the block's ph are computed once into LDS (a bin of
//   more than 256 rows: 256 rows at a time); a lane computes the column weights of its bin once per column and sums column by column.
// d_x: the 2 x 2-cell tile gather of ops.hip (cull_rois, OPS_LIST RoIs per pass): a RoI is listed if its scaled box, grown by one cell
//   and rounded outwards, meets the tile; a wave owns one cell, derives from it the few (ph, pw) whose bins can reach it, and adds
//   dout Wy Wx / A in ascending (RoI, ph, pw) order into registers over all passes; one store.  No atomics.
// d_rois: one wave per (RoI, bin), lanes over channel runs of 4 whatever the element type.  It recomputes what it needs from the map (it
//   does not read the saved output, which a 16-bit map has rounded): a lane walks the bin's cells once, column by column, and forms,
//   per channel, the integral S and the four line integrals Lx(xs), Lx(xe), Ly(ys), Ly(ye), multiplies by dout and sums its channels
//   (the row weights live one row per lane and are broadcast, the column weights are computed once per column); a fixed butterfly
//   adds the 64 lanes; lane 0 applies the analytic formulas and the chain to (X1, Y1, X2, Y2) and stores the bin's four terms in the
//   workspace.  A second kernel, one wave per RoI, sums the bins in a fixed order and scales by spatial_scale.  No atomics.
//
// Element types: templates over the storage type E (ops_run.h: float, float16, bfloat16): widened exactly on load, geometry, weights and
// sums in float32 in one shared body, rounded once on store, so that op(x_T) == op(x_T.float()).to(T) bit for bit for the output and
// d_x, and d_rois (float32) of a 16-bit map is that of the widened map bit for bit.
#include "ops_run.h"
#include <climits>
#include <cstdint>

namespace frcnn {

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
struct PrGeom { float x1, y1, x2, y2, bin_w, bin_h, area; int image; bool ok; };

__device__ __forceinline__ PrGeom prroi_geom(const float* roi, float scale, int n_img, int out_h, int out_w)
{
    PrGeom g;
    g.x1 = roi[1] * scale; g.y1 = roi[2] * scale; g.x2 = roi[3] * scale; g.y2 = roi[4] * scale;
    const float rw = fmaxf(g.x2 - g.x1, 0.0f), rh = fmaxf(g.y2 - g.y1, 0.0f);      // fmaxf(NaN, 0) is 0
    g.bin_w = rw / (float)out_w;
    g.bin_h = rh / (float)out_h;
    g.area = g.bin_w * g.bin_h;
    g.image = 0;
    g.ok = g.area > 0.0f && g.area < __builtin_inff() && roi_image(roi[0], n_img, g.image);
    return g;
}

// bin p of an axis: [s, e]
__device__ __forceinline__ void prroi_bin(float start, float bin, int p, float& s, float& e)
{
    s = start + (float)p * bin;
    e = s + bin;
}

// the cells [lo, hi] of an axis of `size` cells whose hat meets [s, e] (finite): floor(s) .. ceil(e), cut to the map in float first
__device__ __forceinline__ void prroi_cells(float s, float e, int size, int& lo, int& hi)
{
    lo = (int)fminf(fmaxf(floorf(s), 0.0f), 2.0e9f);
    hi = min((int)fmaxf(fminf(ceilf(e), 2.0e9f), -1.0f), size - 1);
}

// Wx(i): the integral of hat(x - i) over [s, e], on the rising piece [i - 1, i] and the falling piece [i, i + 1]
__device__ __forceinline__ float prroi_weight(float s, float e, int i)
{
    const float c = (float)i;
    float w = 0.0f;
    float p = fmaxf(s, c - 1.0f), q = fminf(e, c);
    if (q > p) w = (q - p) * (((p + q) * 0.5f - c) + 1.0f);
    p = fmaxf(s, c); q = fminf(e, c + 1.0f);
    if (q > p) w = w + (q - p) * (1.0f - ((p + q) * 0.5f - c));
    return w;
}

__device__ __forceinline__ float prroi_hat(float t) { return fmaxf(1.0f - fabsf(t), 0.0f); }

// lane `l`'s value of v for every lane; l is wave-uniform and every lane of the wave is active at the call
__device__ __forceinline__ float prroi_lane(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// the bins [lo, hi] of an axis whose [s, e] can meet (cell - 1, cell + 1), one bin of margin either side: the weights decide exactly
__device__ __forceinline__ void prroi_bins_of_cell(float start, float bin, int n_out, int cell, int& lo, int& hi)
{
    const float a = floorf((((float)cell - 1.0f) - start) / bin) - 1.0f, b = floorf((((float)cell + 1.0f) - start) / bin) + 1.0f;
    lo = (int)fminf(fmaxf(a, 0.0f), (float)n_out);
    hi = (int)fmaxf(fminf(b, (float)(n_out - 1)), -1.0f);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256)
void ops_prroi_forward_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, int out_h,
                              int out_w, float scale, E* __restrict__ out)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    __shared__ float s_wy[256];
    const int r = blockIdx.x, ph = blockIdx.y, C4 = C / R::V, n = out_w * C4, tid = threadIdx.x;
    E* orow = out + ((size_t)r * out_h + ph) * out_w * C;
    const PrGeom g = prroi_geom(rois + (size_t)r * 5, scale, n_img, out_h, out_w);
    if (!g.ok) { zero_row<E>(orow, n); return; }                                // block-uniform
    const E* fm = x + (size_t)g.image * fh * fw * C;
    float ys, ye;
    prroi_bin(g.y1, g.bin_h, ph, ys, ye);
    int y_lo, y_hi;
    prroi_cells(ys, ye, fh, y_lo, y_hi);
    const bool once = y_hi - y_lo < 256;                                        // the usual case: the row weights fit, computed once
    if (once) {
        if (y_lo + tid <= y_hi) s_wy[tid] = prroi_weight(ys, ye, y_lo + tid);
        __syncthreads();
    }
    for (int i0 = 0; i0 < n; i0 += 256) {                                      // uniform trip counts: the barriers below are safe
        const int i = i0 + tid;
        const bool act = i < n;
        const int pw = act ? i / C4 : 0, c4 = i - pw * C4;
        float xs, xe;
        prroi_bin(g.x1, g.bin_w, pw, xs, xe);
        int x_lo, x_hi;
        prroi_cells(xs, xe, fw, x_lo, x_hi);
        vec acc = 0.f;
        for (int j0 = y_lo; j0 <= y_hi; j0 += 256) {
            const int rows = min(256, y_hi - j0 + 1);
            if (!once) {
                __syncthreads();                                                // the previous rows have been read
                if (tid < rows) s_wy[tid] = prroi_weight(ys, ye, j0 + tid);
                __syncthreads();
            }
            if (act)
                for (int ix = x_lo; ix <= x_hi; ++ix) {
                    const float wx = prroi_weight(xs, xe, ix);
                    vec col = 0.f;
                    for (int jj = 0; jj < rows; ++jj) col = col + R::load(fm + ((size_t)(j0 + jj) * fw + ix) * C, c4) * s_wy[jj];
                    acc = acc + col * wx;
                }
        }
        if (act) R::store(orow, i, acc / g.area);
    }
}

// ---- d_x: the gather --------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256)
void ops_prroi_input_grad_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w,
                                 float scale, const E* __restrict__ dout, E* __restrict__ dx)
{
    typedef Run<E> R;
    __shared__ int s_list[OPS_LIST];
    __shared__ int s_cnt[4];
    __shared__ int s_n;
    const int C4 = C / R::V, n_chunks = (C4 + 63) >> 6;
    const int img = blockIdx.z / n_chunks, chunk = blockIdx.z - img * n_chunks;
    const int ty0 = blockIdx.y * OPS_TILE, tx0 = blockIdx.x * OPS_TILE;
    const int ty1 = min(ty0 + OPS_TILE, fh) - 1, tx1 = min(tx0 + OPS_TILE, fw) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = chunk * 64 + lane;
    const bool act = c4 < C4;
    const int cy = ty0 + wave / OPS_TILE, cx = tx0 + wave % OPS_TILE;       // this wave's cell, for every pass
    const bool cell_ok = cy <= ty1 && cx <= tx1;

    // the scaled box grown by one cell and rounded outwards (the last bin's end may lie a rounding beyond x2)
    auto touches = [&](int r) {
        const PrGeom g = prroi_geom(rois + (size_t)r * 5, scale, n_img, out_h, out_w);
        return g.ok && g.image == img && floorf(g.x1) - 1.0f <= (float)tx1 && ceilf(g.x2) + 1.0f >= (float)tx0 &&
               floorf(g.y1) - 1.0f <= (float)ty1 && ceilf(g.y2) + 1.0f >= (float)ty0;
    };

    typename R::vec acc = 0.f;
    int r_next = 0;
    do {
        r_next = cull_rois(r_next, k, touches, s_list, s_cnt, &s_n);
        const int n_list = s_n;
        if (cell_ok)
            for (int li = 0; li < n_list; ++li) {
                const int r = __builtin_amdgcn_readfirstlane(s_list[li]);
                const PrGeom g = prroi_geom(rois + (size_t)r * 5, scale, n_img, out_h, out_w);
                const E* const dr = dout + (size_t)r * out_h * out_w * C;
                int ph0, ph1, pw0, pw1;
                prroi_bins_of_cell(g.y1, g.bin_h, out_h, cy, ph0, ph1);
                prroi_bins_of_cell(g.x1, g.bin_w, out_w, cx, pw0, pw1);
                for (int ph = ph0; ph <= ph1; ++ph) {
                    float ys, ye;
                    prroi_bin(g.y1, g.bin_h, ph, ys, ye);
                    const float wy = prroi_weight(ys, ye, cy);
                    if (!(wy > 0.0f)) continue;
                    for (int pw = pw0; pw <= pw1; ++pw) {
                        float xs, xe;
                        prroi_bin(g.x1, g.bin_w, pw, xs, xe);
                        const float wx = prroi_weight(xs, xe, cx);
                        if (!(wx > 0.0f)) continue;
                        if (act) acc = acc + R::load(dr, ((size_t)ph * out_w + pw) * C4 + c4) * ((wy * wx) / g.area);
                    }
                }
            }
    } while (r_next < k);
    if (cell_ok && act) R::store(dx + (size_t)img * fh * fw * C, ((size_t)cy * fw + cx) * C4 + c4, acc);
}

// ---- d_rois ----------------------------------------------------------------------------------------------------------------------------
// Per bin, with S = sum Wy Wx x (so out = S / A), Lx(t) = sum_j Wy(j) sum_i hat(t - i) x[j][i], Ly(t) = sum_i Wx(i) sum_j hat(t - j) x[j][i]:
//   d out / d xs = (-Lx(xs) + out bin_h) / A,  d out / d xe = (Lx(xe) - out bin_h) / A,  likewise ys, ye with Ly and bin_w;
//   xs = X1 + pw bin_w, xe = xs + bin_w: d xs / d X1 = 1 - pw / out_w, d xs / d X2 = pw / out_w, d xe / d X1 = 1 - (pw + 1) / out_w, ...
// Every cell with a non-zero hat(xs - i) or hat(xe - i) lies in the bin's own range floor(xs) .. ceil(xe), so one walk serves all five
// sums.  A lane owns the channels 4 (lane + 64 j) .. + 3 whatever the element type, so a 16-bit map's d_rois is the widened map's bit for
// bit (a zero-padded run adds +0).  part: [k][bins][4] = the bin's terms for (X1, Y1, X2, Y2).
template <typename E4>
__global__ __launch_bounds__(256)
void ops_prroi_roi_grad_kernel(const E4* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, int k,
                               int out_h, int out_w, float scale, const E4* __restrict__ dout, f32x4* __restrict__ part)
{
    typedef Run<E4> R;
    typedef typename R::vec vec;
    static_assert(R::V == 4, "runs of 4 for every element type: the lanes' partial sums are those of the float32 kernel");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = C / 4, bins = out_h * out_w;
    const long long item = (long long)blockIdx.x * 4 + wave;                // wave-uniform
    if (item >= (long long)k * bins) return;
    const int r = (int)(item / bins), bin = (int)(item - (long long)r * bins);
    const int ph = bin / out_w, pw = bin - ph * out_w;
    const PrGeom g = prroi_geom(rois + (size_t)r * 5, scale, n_img, out_h, out_w);
    if (!g.ok) {
        if (lane == 0) part[item] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const E4* fm = x + (size_t)g.image * fh * fw * C;
    float xs, xe, ys, ye;
    prroi_bin(g.x1, g.bin_w, pw, xs, xe);
    prroi_bin(g.y1, g.bin_h, ph, ys, ye);
    int x_lo, x_hi, y_lo, y_hi;
    prroi_cells(xs, xe, fw, x_lo, x_hi);
    prroi_cells(ys, ye, fh, y_lo, y_hi);
    float g_s = 0.f, g_xs = 0.f, g_xe = 0.f, g_ys = 0.f, g_ye = 0.f;
    // Uniform loops (every lane takes every trip; loads are guarded): lane l holds the three row weights of row j0 + l, computed once
    // per 64 rows, and a row's weights reach all lanes by v_readlane; the column weights are computed once per column.
    for (int c0 = 0; c0 < C4; c0 += 64) {
        const int c4 = c0 + lane;
        const bool act = c4 < C4;
        vec s = 0.f, lxs = 0.f, lxe = 0.f, lys = 0.f, lye = 0.f;
        for (int j0 = y_lo; j0 <= y_hi; j0 += 64) {
            const int rows = min(64, y_hi - j0 + 1), jl = j0 + lane;
            const bool row = lane < rows;
            const float wy_l = row ? prroi_weight(ys, ye, jl) : 0.f;
            const float hys_l = row ? prroi_hat(ys - (float)jl) : 0.f, hye_l = row ? prroi_hat(ye - (float)jl) : 0.f;
            for (int i = x_lo; i <= x_hi; ++i) {
                vec col_s = 0.f, col_ys = 0.f, col_ye = 0.f;
                for (int jj = 0; jj < rows; ++jj) {
                    const float wy = prroi_lane(wy_l, jj), hys = prroi_lane(hys_l, jj), hye = prroi_lane(hye_l, jj);
                    vec v = 0.f;
                    if (act) v = R::load(fm + ((size_t)(j0 + jj) * fw + i) * C, c4);
                    col_s = col_s + v * wy;
                    col_ys = col_ys + v * hys;
                    col_ye = col_ye + v * hye;
                }
                const float wx = prroi_weight(xs, xe, i);
                s = s + col_s * wx;
                lxs = lxs + col_s * prroi_hat(xs - (float)i);
                lxe = lxe + col_s * prroi_hat(xe - (float)i);
                lys = lys + col_ys * wx;
                lye = lye + col_ye * wx;
            }
        }
        if (act) {
            const vec gr = R::load(dout + ((size_t)r * bins + bin) * C, c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                g_s = g_s + gr[j] * s[j];
                g_xs = g_xs + gr[j] * lxs[j];
                g_xe = g_xe + gr[j] * lxe[j];
                g_ys = g_ys + gr[j] * lys[j];
                g_ye = g_ye + gr[j] * lye[j];
            }
        }
    }
    // the 64 lanes in a fixed butterfly: every lane ends with the same sums
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        g_s = g_s + __shfl_xor(g_s, o, 64);
        g_xs = g_xs + __shfl_xor(g_xs, o, 64);
        g_xe = g_xe + __shfl_xor(g_xe, o, 64);
        g_ys = g_ys + __shfl_xor(g_ys, o, 64);
        g_ye = g_ye + __shfl_xor(g_ye, o, 64);
    }
    if (lane == 0) {
        const float g_out = g_s / g.area;                                   // sum over the channels of dout out
        const float d_xs = (g_out * g.bin_h - g_xs) / g.area, d_xe = (g_xe - g_out * g.bin_h) / g.area;
        const float d_ys = (g_out * g.bin_w - g_ys) / g.area, d_ye = (g_ye - g_out * g.bin_w) / g.area;
        const float ax = (float)pw / (float)out_w, bx = (float)(pw + 1) / (float)out_w;
        const float ay = (float)ph / (float)out_h, by = (float)(ph + 1) / (float)out_h;
        part[item] = f32x4{d_xs * (1.0f - ax) + d_xe * (1.0f - bx), d_ys * (1.0f - ay) + d_ye * (1.0f - by), d_xs * ax + d_xe * bx,
                           d_ys * ay + d_ye * by};
    }
}

// one wave per RoI: lane l sums the bins l, l + 64, .. in ascending order, a fixed butterfly adds the lanes; drois [k][5], column 0 is 0
__global__ __launch_bounds__(256)
void ops_prroi_roi_reduce_kernel(const f32x4* __restrict__ part, int k, int bins, float scale, float* __restrict__ drois)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= k) return;                                                     // wave-uniform
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b = lane; b < bins; b += 64) acc = acc + part[(size_t)r * bins + b];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], o, 64);
    if (lane == 0) {
        float* const dst = drois + (size_t)r * 5;
        dst[0] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[1 + j] = scale * acc[j];
    }
}

// ---- the entry points' bodies, one per element type ---------------------------------------------------------------------------------
// the element type walked in runs of 4 channels
template <typename E> struct PrNarrow { typedef E type; };
template <typename E, int N> struct PrNarrow<run_t<E, N>> { typedef run_t<E, 4> type; };

// roi_align's limits (roi_args_ok), the gather grid's tile rows and the 32-bit (RoI, bin) indices
static bool prroi_args_ok(int n_img, int fh, int fw, int c, int k, int out_h, int out_w, int v)
{
    return roi_args_ok(n_img, fh, fw, c, k, out_h, out_w, v) && fh <= 65535 * OPS_TILE && (size_t)k * out_h * out_w <= (size_t)INT32_MAX;
}

static size_t prroi_workspace_bytes(int k, int out_h, int out_w) { return (size_t)k * out_h * out_w * sizeof(f32x4); }

template <typename E>
static int prroi_forward_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                              float spatial_scale, void* d_out, void* stream)
{
    if (!prroi_args_ok(n_img, fh, fw, c, k, out_h, out_w, Run<E>::V)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_prroi_forward_kernel<E>, dim3(k, out_h), dim3(256), 0, (hipStream_t)stream, static_cast<const E*>(d_x), n_img,
                       fh, fw, c, d_rois, out_h, out_w, spatial_scale, static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int prroi_backward_impl(const void* d_x, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                               float spatial_scale, const void* d_dout, void* d_dx, float* d_drois, void* d_ws, size_t ws_bytes,
                               void* stream)
{
    typedef typename PrNarrow<E>::type E4;
    if (!prroi_args_ok(n_img, fh, fw, c, k, out_h, out_w, Run<E>::V)) return FRCNN_EINVAL;
    if (!d_dx && !d_drois) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (k == 0) {
        if (d_dx) FRCNN_HIP_TRY(hipMemsetAsync(d_dx, 0, (size_t)n_img * fh * fw * c * sizeof(E), s));
        return FRCNN_OK;
    }
    if (!d_rois || !d_dout) return FRCNN_EINVAL;
    if (d_drois && (!d_x || !d_ws || (uintptr_t)d_ws % 16 != 0 || ws_bytes < prroi_workspace_bytes(k, out_h, out_w))) return FRCNN_EINVAL;
    const int bins = out_h * out_w;
    if (d_drois) {
        f32x4* const part = static_cast<f32x4*>(d_ws);
        hipLaunchKernelGGL(ops_prroi_roi_grad_kernel<E4>, dim3((unsigned)(((size_t)k * bins + 3) / 4)), dim3(256), 0, s,
                           static_cast<const E4*>(d_x), n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale,
                           static_cast<const E4*>(d_dout), part);
        int rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(ops_prroi_roi_reduce_kernel, dim3(cdiv(k, 4)), dim3(256), 0, s, part, k, bins, spatial_scale, d_drois);
        rc = check_launch();
        if (rc) return rc;
    }
    if (d_dx) {
        hipLaunchKernelGGL(ops_prroi_input_grad_kernel<E>, dim3(cdiv(fw, OPS_TILE), cdiv(fh, OPS_TILE), n_img * cdiv(c / Run<E>::V, 64)),
                           dim3(256), 0, s, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, static_cast<const E*>(d_dout),
                           static_cast<E*>(d_dx));
        return check_launch();
    }
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_prroi_pool_cull_list(void) { return OPS_LIST; }

size_t frcnn_ops_prroi_pool_workspace_bytes(int k, int out_h, int out_w)
{
    if (k < 0 || out_h < 1 || out_h > OPS_MAX_OUT || out_w < 1 || out_w > OPS_MAX_OUT || (size_t)k * out_h * out_w > (size_t)INT32_MAX)
        return 0;
    return prroi_workspace_bytes(k, out_h, out_w);
}

int frcnn_ops_prroi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                         float spatial_scale, float* d_out, void* stream)
{
    return prroi_forward_impl<float>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, d_out, stream);
}

int frcnn_ops_prroi_pool_backward(const float* d_x, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                  float spatial_scale, const float* d_dout, float* d_dx, float* d_drois, void* d_ws, size_t ws_bytes,
                                  void* stream)
{
    return prroi_backward_impl<float>(d_x, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, d_dout, d_dx, d_drois, d_ws, ws_bytes,
                                      stream);
}

int frcnn_ops_prroi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                            int out_w, float spatial_scale, void* d_out, void* stream)
{
    if (c % OPS_HALF_RUN != 0) return FRCNN_EINVAL;
    // the forward always walks runs of OPS_HALF_RUN: only those two kernels are built
    OPS_ELEM_DISPATCH(elem_type, E, prroi_forward_impl<run_t<E, OPS_HALF_RUN>>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale,
                                                                               d_out, stream));
}

int frcnn_ops_prroi_pool_backward_16(int elem_type, const void* d_x, const float* d_rois, int k, int n_img, int fh, int fw, int c,
                                     int out_h, int out_w, float spatial_scale, const void* d_dout, void* d_dx, float* d_drois, void* d_ws,
                                     size_t ws_bytes, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), prroi_backward_impl, d_x, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale,
                    d_dout, d_dx, d_drois, d_ws, ws_bytes, stream);
}

}  // extern "C"
