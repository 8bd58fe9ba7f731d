// ops_ps.hip -- position-sensitive RoI pooling (R-FCN): torchvision.ops.ps_roi_pool and ps_roi_align over N images with deterministic
// backward passes (the frcnn_ops_ps_* entry points of include/frcnn_hip.h).  Restated from the published algorithm of torchvision's
// ps_roi_pool_kernel.cu / ps_roi_align_kernel.cu (third party, absent here: restated, unpinned, like nms / roi_align).
//
// Layouts: plain NCHW.  The map is [n][C][h][w], RoIs are torchvision's rows (b, x1, y1, x2, y2), the pooled output is
// [k][C / (out_h out_w)][out_h][out_w].  Output channel co of bin (ph, pw) pools input plane (co out_h + ph) out_w + pw -- which is the
// output element's own linear index inside its RoI: every output element owns one plane of the map, so channels on lanes (the NHWC
// design of ops.hip) has nothing to share and the map is read where it lies, without a layout copy.
//
// Forward: one thread per output element, in output order -- the stores of a wave are one 256-byte line, and its 64 lanes walk 64
// neighbouring planes, each over the few rows of its own bin (iy outer, ix inner: the two corners of a row are adjacent).  A map of
// R-FCN's size stays in L2 over the RoIs of an image.
// Backward: no atomics.  Plane c of dx receives only from bin (ph, pw) = c % (out_h out_w) of output channel c / (out_h out_w), so a
// block owns 256 cells of one plane of one image and its threads first list, 256 RoIs at a time and in ascending order, that one bin's
// window and gradient per RoI in LDS (a RoI of another image, or a bin that sends nothing, lists an empty window); then each thread
// tests its cell against the listed windows -- a broadcast LDS read and four compares for the many bins that miss it -- and adds what
// the few that hold it send, in ascending RoI order: bit-identical from run to run.  The sum stays in a register until it is stored once.
//
// Element types: templates over the storage type E of maps, outputs and gradients (float, float16, bfloat16: ops_elem.h); widened
// exactly on load, geometry and sums in float32 in one shared body, rounded once to nearest even on store as Tensor.to() rounds, so
// that op(x_T) == op(x_T.float()).to(T) bit for bit.  One element per lane: no constraint on C beyond C % (out_h out_w) == 0.
#include "ops_geom.h"
#include "ops_elem.h"

namespace frcnn {

static constexpr int PS_MAX_OUT = 64;        // out_h, out_w <= 64
static constexpr int PS_MAX_SAMPLING = 16;   // sampling_ratio <= 16
static constexpr int PS_BLOCK = 256;

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
// ps_roi_align's plan: roi_align's aligned plan with torchvision's count = grid_h * grid_w for this operator, which has no lower bound
// (0 for a RoI of no height or width under an adaptive grid: the forward is then 0.0f / 0.0f).
__device__ __forceinline__ RoiGeom ps_align_geom(const float* roi, float scale, int out_h, int out_w, int sampling_ratio)
{
    RoiGeom g = ops_align_geom(roi, scale, out_h, out_w, sampling_ratio, 1);
    g.count = (float)(g.grid_h * g.grid_w);
    return g;
}

// ps_roi_pool: start = roundf(c scale), end = roundf((c + 1) scale), integer size max(end - start, 1)
struct PsPoolGeom { int rs_h, rs_w; float bin_h, bin_w; };

__device__ __forceinline__ PsPoolGeom ps_pool_geom(const float* roi, float scale, int out_h, int out_w)
{
    PsPoolGeom g;
    g.rs_w = (int)roundf(roi[1] * scale); g.rs_h = (int)roundf(roi[2] * scale);
    const int re_w = (int)roundf((roi[3] + 1.0f) * scale), re_h = (int)roundf((roi[4] + 1.0f) * scale);
    const int roi_w = max(re_w - g.rs_w, 1), roi_h = max(re_h - g.rs_h, 1);
    g.bin_h = (float)roi_h / (float)out_h; g.bin_w = (float)roi_w / (float)out_w;
    return g;
}
// bin p's window [s, e) along an axis of `size` cells: both bounds clamped to [0, size - 1], as torchvision clamps them here
__device__ __forceinline__ void ps_pool_bin(int p, float bin, int rs, int size, int& s, int& e)
{
    const int a = (int)floorf((float)p * bin) + rs, b = (int)ceilf((float)(p + 1) * bin) + rs;
    s = min(max(a, 0), size - 1); e = min(max(b, 0), size - 1);
}

// the output element of a thread: RoI r and its linear index c inside the RoI, which is also its input plane; bin (ph, pw) = c % bins
__device__ __forceinline__ bool ps_element(size_t total, int C, int out_w, int bins, int& r, int& c, int& ph, int& pw)
{
    const size_t idx = (size_t)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (idx >= total) return false;
    r = (int)(idx / (size_t)C);
    c = (int)(idx - (size_t)r * C);
    const int b = c % bins;
    ph = b / out_w; pw = b - ph * out_w;
    return true;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(PS_BLOCK)
void ops_ps_roi_align_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, size_t total,
                             int out_h, int out_w, float scale, int sampling_ratio, E* __restrict__ out)
{
    int r, c, ph, pw;
    if (!ps_element(total, C, out_w, out_h * out_w, r, c, ph, pw)) return;
    const float* roi = rois + (size_t)r * 5;
    const size_t o = (size_t)r * C + c;
    int b;
    if (!roi_image(roi[0], n_img, b)) { Elem<E>::store(out, o, 0.f); return; }
    const RoiGeom g = ps_align_geom(roi, scale, out_h, out_w, sampling_ratio);
    const E* const plane = x + ((size_t)b * C + c) * fh * fw;
    float acc = 0.f;
    for (int iy = 0; iy < g.grid_h; ++iy) {
        const float y = sample_coord(g.start_h, g.bin_h, g.grid_h, ph, iy);
        int yl, yh; float hy, ly;
        const bool yok = axis_weights(y, fh, yl, yh, hy, ly);
        for (int ix = 0; ix < g.grid_w; ++ix) {
            const float xx = sample_coord(g.start_w, g.bin_w, g.grid_w, pw, ix);
            int xl, xh; float hx, lx;
            if (!yok || !axis_weights(xx, fw, xl, xh, hx, lx)) continue;
            const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
            const float v1 = Elem<E>::load(plane, (size_t)yl * fw + xl), v2 = Elem<E>::load(plane, (size_t)yl * fw + xh);
            const float v3 = Elem<E>::load(plane, (size_t)yh * fw + xl), v4 = Elem<E>::load(plane, (size_t)yh * fw + xh);
            acc = acc + (((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4);
        }
    }
    Elem<E>::store(out, o, acc / g.count);
}

template <typename E>
__global__ __launch_bounds__(PS_BLOCK)
void ops_ps_roi_pool_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, size_t total,
                            int out_h, int out_w, float scale, E* __restrict__ out)
{
    int r, c, ph, pw;
    if (!ps_element(total, C, out_w, out_h * out_w, r, c, ph, pw)) return;
    const float* roi = rois + (size_t)r * 5;
    const size_t o = (size_t)r * C + c;
    int b;
    if (!roi_image(roi[0], n_img, b)) { Elem<E>::store(out, o, 0.f); return; }
    const PsPoolGeom g = ps_pool_geom(roi, scale, out_h, out_w);
    int hs, he, ws, we;
    ps_pool_bin(ph, g.bin_h, g.rs_h, fh, hs, he);
    ps_pool_bin(pw, g.bin_w, g.rs_w, fw, ws, we);
    const E* const plane = x + ((size_t)b * C + c) * fh * fw;
    float sum = 0.f;                                     // torchvision's scan-order sum: h outer, w inner
    for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) sum += Elem<E>::load(plane, (size_t)h * fw + w);
    const bool empty = he <= hs || we <= ws;
    Elem<E>::store(out, o, empty ? 0.f : sum / (float)((he - hs) * (we - ws)));
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// the cell, plane and bin of a backward thread: grid (cells / 256, C, n_img)
struct PsCell { int img, c, ph, pw, cy, cx; bool ok; };

__device__ __forceinline__ PsCell ps_cell(int fh, int fw, int out_h, int out_w)
{
    PsCell t;
    t.img = blockIdx.z; t.c = blockIdx.y;
    const int b = t.c % (out_h * out_w);
    t.ph = b / out_w; t.pw = b - t.ph * out_w;
    const int p = blockIdx.x * PS_BLOCK + threadIdx.x;
    t.ok = p < fh * fw;
    t.cy = p / fw; t.cx = p - t.cy * fw;
    return t;
}

template <typename E>
__global__ __launch_bounds__(PS_BLOCK)
void ops_ps_roi_pool_backward_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w,
                                     float scale, const E* __restrict__ dout, E* __restrict__ dx)
{
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    __shared__ i32x4 s_win[PS_BLOCK];                    // hs, he, ws, we of the plane's bin; hs == he: sends nothing
    __shared__ float s_val[PS_BLOCK];                    // dout / area
    const PsCell t = ps_cell(fh, fw, out_h, out_w);
    float acc = 0.f;
    for (int r0 = 0; r0 < k; r0 += PS_BLOCK) {
        const int r = r0 + threadIdx.x;
        i32x4 win = {0, 0, 0, 0};
        float val = 0.f;
        int b;
        if (r < k && roi_image(rois[(size_t)r * 5], n_img, b) && b == t.img) {
            const PsPoolGeom g = ps_pool_geom(rois + (size_t)r * 5, scale, out_h, out_w);
            int hs, he, ws, we;
            ps_pool_bin(t.ph, g.bin_h, g.rs_h, fh, hs, he);
            ps_pool_bin(t.pw, g.bin_w, g.rs_w, fw, ws, we);
            if (he > hs && we > ws) {
                win = i32x4{hs, he, ws, we};
                val = Elem<E>::load(dout, (size_t)r * C + t.c) / (float)((he - hs) * (we - ws));
            }
        }
        __syncthreads();                                 // the previous group has been read
        s_win[threadIdx.x] = win;
        s_val[threadIdx.x] = val;
        __syncthreads();
        const int n_list = min(PS_BLOCK, k - r0);
        if (t.ok)
            for (int i = 0; i < n_list; ++i) {
                const i32x4 w = s_win[i];
                if (t.cy >= w[0] && t.cy < w[1] && t.cx >= w[2] && t.cx < w[3]) acc += s_val[i];
            }
    }
    if (t.ok) Elem<E>::store(dx, (((size_t)t.img * C + t.c) * fh + t.cy) * fw + t.cx, acc);
}

// the cells a bin's samples can touch along one axis, from its first and last sample (the coordinates between them are monotone):
// one cell of margin on either side of their footprints; a NaN coordinate lists every cell.  The gather tests each sample exactly.
__device__ __forceinline__ void ps_sample_window(float start, float bin, int grid, int p, int& lo, int& hi)
{
    const float a = sample_coord(start, bin, grid, p, 0), b = sample_coord(start, bin, grid, p, grid - 1);
    // clamped in float first (the conversion of an out-of-range float is undefined)
    lo = (int)fminf(fmaxf(floorf(fminf(a, b)) - 1.0f, -2.0f), 2.0e9f);
    hi = (int)fmaxf(fminf(ceilf(fmaxf(a, b)) + 1.0f, 2.0e9f), -2.0f);
}

template <typename E>
__global__ __launch_bounds__(PS_BLOCK)
void ops_ps_roi_align_backward_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w,
                                      float scale, int sampling_ratio, const E* __restrict__ dout, E* __restrict__ dx)
{
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    __shared__ i32x4 s_win[PS_BLOCK];                    // y_lo, y_hi, x_lo, x_hi (inclusive); y_lo > y_hi: sends nothing
    __shared__ f32x4 s_geom[PS_BLOCK];                   // start_h, start_w, bin_h, bin_w
    __shared__ f32x4 s_grad[PS_BLOCK];                   // dout, count, grid_h, grid_w (the grids as integer bits)
    const PsCell t = ps_cell(fh, fw, out_h, out_w);
    float acc = 0.f;
    for (int r0 = 0; r0 < k; r0 += PS_BLOCK) {
        const int r = r0 + threadIdx.x;
        i32x4 win = {1, 0, 1, 0};
        f32x4 geom = {0.f, 0.f, 0.f, 0.f}, grad = {0.f, 0.f, 0.f, 0.f};
        int b;
        if (r < k && roi_image(rois[(size_t)r * 5], n_img, b) && b == t.img) {
            const RoiGeom g = ps_align_geom(rois + (size_t)r * 5, scale, out_h, out_w, sampling_ratio);
            if (g.grid_h > 0 && g.grid_w > 0) {
                int y_lo, y_hi, x_lo, x_hi;
                ps_sample_window(g.start_h, g.bin_h, g.grid_h, t.ph, y_lo, y_hi);
                ps_sample_window(g.start_w, g.bin_w, g.grid_w, t.pw, x_lo, x_hi);
                win = i32x4{y_lo, y_hi, x_lo, x_hi};
                geom = f32x4{g.start_h, g.start_w, g.bin_h, g.bin_w};
                grad = f32x4{Elem<E>::load(dout, (size_t)r * C + t.c), g.count, __int_as_float(g.grid_h), __int_as_float(g.grid_w)};
            }
        }
        __syncthreads();                                 // the previous group has been read
        s_win[threadIdx.x] = win;
        s_geom[threadIdx.x] = geom;
        s_grad[threadIdx.x] = grad;
        __syncthreads();
        const int n_list = min(PS_BLOCK, k - r0);
        if (t.ok)
            for (int i = 0; i < n_list; ++i) {
                const i32x4 w = s_win[i];
                if (t.cy < w[0] || t.cy > w[1] || t.cx < w[2] || t.cx > w[3]) continue;
                const f32x4 g = s_geom[i], d = s_grad[i];
                const int grid_h = __float_as_int(d[2]), grid_w = __float_as_int(d[3]);
                // the bin's samples form a grid_h x grid_w product, so the cell's weight in it is (the sum of its row weights) x (the
                // sum of its column weights): one term per bin, as in ops.hip's align_cell_grad
                float wy_sum = 0.f, wx_sum = 0.f;
                bool y_hit = false, x_hit = false;
                for (int iy = 0; iy < grid_h; ++iy) {
                    float wy;
                    if (cell_weight(sample_coord(g[0], g[2], grid_h, t.ph, iy), fh, t.cy, wy)) { wy_sum += wy; y_hit = true; }
                }
                if (!y_hit) continue;
                for (int ix = 0; ix < grid_w; ++ix) {
                    float wx;
                    if (cell_weight(sample_coord(g[1], g[3], grid_w, t.pw, ix), fw, t.cx, wx)) { wx_sum += wx; x_hit = true; }
                }
                if (x_hit) acc = acc + (d[0] * (wy_sum * wx_sum)) / d[1];
            }
    }
    if (t.ok) Elem<E>::store(dx, (((size_t)t.img * C + t.c) * fh + t.cy) * fw + t.cx, acc);
}

// ---- the entry points' bodies, one per element type ---------------------------------------------------------------------------------
// c: input channels.  The limits of the launch grids: forward blocks in x; backward planes in y and images in z.
static bool ps_args_ok(int n_img, int fh, int fw, int c, int k, int out_h, int out_w)
{
    if (out_h < 1 || out_h > PS_MAX_OUT || out_w < 1 || out_w > PS_MAX_OUT) return false;
    const int bins = out_h * out_w;
    return n_img >= 1 && n_img <= 65535 && fh >= 1 && fw >= 1 && c >= bins && c % bins == 0 && c <= 65535 && k >= 0 &&
           (size_t)fh * fw <= (size_t)INT32_MAX - PS_BLOCK && ((size_t)k * c + PS_BLOCK - 1) / PS_BLOCK <= (size_t)INT32_MAX;
}

static unsigned ps_forward_blocks(int k, int c) { return (unsigned)(((size_t)k * c + PS_BLOCK - 1) / PS_BLOCK); }
static dim3 ps_backward_grid(int n_img, int fh, int fw, int c) { return dim3(cdiv(fh * fw, PS_BLOCK), c, n_img); }

template <typename E>
static int ps_roi_pool_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                            float spatial_scale, void* d_out, void* stream)
{
    if (!ps_args_ok(n_img, fh, fw, c, k, out_h, out_w)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_ps_roi_pool_kernel<E>, dim3(ps_forward_blocks(k, c)), dim3(PS_BLOCK), 0, (hipStream_t)stream,
                       static_cast<const E*>(d_x), n_img, fh, fw, c, d_rois, (size_t)k * c, out_h, out_w, spatial_scale,
                       static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int ps_roi_pool_backward_impl(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                     float spatial_scale, const void* d_dout, void* d_dx, void* stream)
{
    if (!ps_args_ok(n_img, fh, fw, c, k, out_h, out_w)) return FRCNN_EINVAL;
    if (!d_dx || (k > 0 && (!d_rois || !d_dout))) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_ps_roi_pool_backward_kernel<E>, ps_backward_grid(n_img, fh, fw, c), dim3(PS_BLOCK), 0, (hipStream_t)stream,
                       d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, static_cast<const E*>(d_dout), static_cast<E*>(d_dx));
    return check_launch();
}

template <typename E>
static int ps_roi_align_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                             float spatial_scale, int sampling_ratio, void* d_out, void* stream)
{
    if (!ps_args_ok(n_img, fh, fw, c, k, out_h, out_w) || sampling_ratio > PS_MAX_SAMPLING) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_ps_roi_align_kernel<E>, dim3(ps_forward_blocks(k, c)), dim3(PS_BLOCK), 0, (hipStream_t)stream,
                       static_cast<const E*>(d_x), n_img, fh, fw, c, d_rois, (size_t)k * c, out_h, out_w, spatial_scale, sampling_ratio,
                       static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int ps_roi_align_backward_impl(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                      float spatial_scale, int sampling_ratio, const void* d_dout, void* d_dx, void* stream)
{
    if (!ps_args_ok(n_img, fh, fw, c, k, out_h, out_w) || sampling_ratio > PS_MAX_SAMPLING) return FRCNN_EINVAL;
    if (!d_dx || (k > 0 && (!d_rois || !d_dout))) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_ps_roi_align_backward_kernel<E>, ps_backward_grid(n_img, fh, fw, c), dim3(PS_BLOCK), 0, (hipStream_t)stream,
                       d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, static_cast<const E*>(d_dout),
                       static_cast<E*>(d_dx));
    return check_launch();
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_ps_roi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                          float spatial_scale, float* d_out, void* stream)
{
    return ps_roi_pool_impl<float>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, d_out, stream);
}

int frcnn_ops_ps_roi_pool_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                   const float* d_dout, float* d_dx, void* stream)
{
    return ps_roi_pool_backward_impl<float>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, d_dout, d_dx, stream);
}

int frcnn_ops_ps_roi_align(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                           float spatial_scale, int sampling_ratio, float* d_out, void* stream)
{
    return ps_roi_align_impl<float>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, sampling_ratio, d_out, stream);
}

int frcnn_ops_ps_roi_align_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                    int sampling_ratio, const float* d_dout, float* d_dx, void* stream)
{
    return ps_roi_align_backward_impl<float>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, d_dout, d_dx, stream);
}

int frcnn_ops_ps_roi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                             int out_w, float spatial_scale, void* d_out, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, ps_roi_pool_impl<E>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, d_out, stream));
}

int frcnn_ops_ps_roi_pool_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                      float spatial_scale, const void* d_dout, void* d_dx, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E,
                      ps_roi_pool_backward_impl<E>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, d_dout, d_dx, stream));
}

int frcnn_ops_ps_roi_align_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                              int out_w, float spatial_scale, int sampling_ratio, void* d_out, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, ps_roi_align_impl<E>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, sampling_ratio,
                                                         d_out, stream));
}

int frcnn_ops_ps_roi_align_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                       float spatial_scale, int sampling_ratio, const void* d_dout, void* d_dx, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, ps_roi_align_backward_impl<E>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio,
                                                                  d_dout, d_dx, stream));
}

}  // extern "C"
