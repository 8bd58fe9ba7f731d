// ops.hip -- the kernels behind fasterrcnn_amd.ops: torchvision.ops-style roi_align, roi_pool, nms and batched_nms over N images,
// with deterministic backward passes (the frcnn_ops_* entry points of include/frcnn_hip.h).
//
// Layouts: the feature map is NHWC [n][h][w][c] (a channels_last NCHW tensor), RoIs are torchvision's rows (b, x1, y1, x2, y2), the
// pooled output is [k][out_h][out_w][c] (a channels_last [k][c][out_h][out_w] tensor).  c % 4 == 0: a pixel is float4 runs.
// Element types: the RoI kernels are templates over the storage type E of maps, outputs and gradients -- float, or float16 / bfloat16
// (the frcnn_ops_*_16 entry points).  A lane owns a Run<E> of V channels (4 floats; 8, or in a narrow backward 4, 16-bit values): widened exactly on load,
// every sum, weight and coordinate in float32 in one shared body, rounded once (to nearest even, as Tensor.to() rounds) on store -- so
// op(x_T) == op(x_T.float()).to(T) bit for bit, the definition of torchvision's autocast wrappers.  RoIs are always float32.
// A RoI whose batch index b is outside (-1, n) -- truncated to an int as torchvision truncates it -- pools to zeros and gets no gradient.
//
// RoIAlign forward: the arithmetic of roi_align_kernel (csrc/roialign.hip), one block per (roi, ph), lanes over (pw, channel quad).
// Backwards: no atomics.  One block per 2 x 2 cells of one image and 64 channel quads; its threads first cull the RoIs whose footprint
// can touch the tile (in ascending order, up to OPS_LIST at a time), then each wave owns one cell and sums, RoI by RoI, the samples /
// bins that hold it in a fixed order: bit-identical from run to run.  The sum stays in registers over every culling pass and is stored
// once (a 16-bit dx never holds a partial sum).  RoIAlign finds the samples of a cell analytically -- the sample rows within one
// pixel of the cell, from the RoI's sample spacing, each then tested exactly -- so there is no cap on out_h / out_w or sampling_ratio.
// Multi-scale RoIAlign (torchvision's MultiScaleRoIAlign): the RoIAlign forward with the level picked per RoI, and the RoIAlign backward
// on a grid over the tiles of every level, each tile culling only the RoIs of its (level, image), listed once by a bucketing launch.
// RoIPool's backward sends each bin's gradient to the argmax cell its forward wrote (the first maximum in (h, w) scan order, -1 for an
// empty bin), the design of roi_pool_argmax_kernel / roi_pool_scatter_kernel (csrc/train.hip).
//
// NMS: the caller sorts (torch.sort, stable) and passes the permutation; for batched NMS the permutation groups each category into
// one contiguous segment.  ops_nms_mask_kernel writes 64 x 64 IoU bit tiles (only tiles on or above the diagonal whose rows and
// columns can share a category), ops_nms_reduce_kernel runs the greedy pass of every segment in its own wave, in parallel, with the
// segment's removed-bits in LDS.  float32 decides with iou_gt (csrc/geometry.h), float64 with the division in float64.
#include "ops_run.h"
#include <cfloat>

namespace frcnn {

// Output row ph of one RoI (out_w x C / V runs at orow) pooled from the image map fm [fh][fw][C]: the loop body of ops_roi_align_kernel,
// shared with ops_ms_roi_align_kernel so that the two stay bit-identical.  Block of 256 threads.
template <typename E>
__device__ __forceinline__ void align_row(const E* __restrict__ fm, int fh, int fw, int C, const RoiGeom& g, int ph, int out_w,
                                          E* __restrict__ orow)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    const int C4 = C / R::V;
    for (int i = threadIdx.x; i < out_w * C4; i += 256) {
        const int pw = i / C4, c4 = i - pw * C4;
        vec acc = 0.f;
        for (int iy = 0; iy < g.grid_h; ++iy) {
            const float y = sample_coord(g.start_h, g.bin_h, g.grid_h, ph, iy);
            int yl, yh; float hy, ly;
            const bool yok = axis_weights(y, fh, yl, yh, hy, ly);
            for (int ix = 0; ix < g.grid_w; ++ix) {
                const float xx = sample_coord(g.start_w, g.bin_w, g.grid_w, pw, ix);
                int xl, xh; float hx, lx;
                if (!yok || !axis_weights(xx, fw, xl, xh, hx, lx)) continue;
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

template <typename E>
__global__ __launch_bounds__(256)
void ops_roi_align_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, int out_h,
                          int out_w, float scale, int sampling_ratio, int aligned, E* __restrict__ out)
{
    const int r = blockIdx.x, ph = blockIdx.y;
    const float* roi = rois + (size_t)r * 5;
    E* orow = out + ((size_t)r * out_h + ph) * out_w * C;
    int b;
    if (!roi_image(roi[0], n_img, b)) {
        zero_row(orow, out_w * (C / Run<E>::V));
        return;
    }
    align_row(x + (size_t)b * fh * fw * C, fh, fw, C, ops_align_geom(roi, scale, out_h, out_w, sampling_ratio, aligned), ph, out_w, orow);
}

// The sample positions s = p * grid + i (0 <= s < n_out * grid) whose coordinate can lie within one pixel of `cell`: the linear model
// of the positions, widened by one sample and a relative margin for rounding; every candidate is then evaluated exactly by the caller.
__device__ __forceinline__ void sample_range(int cell, float start, float bin, int grid, int n_out, int& s_lo, int& s_hi)
{
    const long long last = min((long long)n_out * grid, (long long)INT32_MAX) - 1;      // grid >= 1 here
    const float step = bin / (float)grid;
    if (!(step > 0.f)) { s_lo = 0; s_hi = (int)last; return; }              // zero-size or inverted RoI (aligned): every sample
    const float pad = 1.0f + 1e-4f * (fabsf(start) + fabsf(bin) * (float)n_out + 2.0f) / step;
    const float a = ((float)cell - 1.0f - start) / step - 0.5f - pad;
    const float e = ((float)cell + 1.0f - start) / step - 0.5f + pad;
    // clamped in float first (the conversion of an out-of-range float is undefined), then exactly in integers
    s_lo = (int)fminf(fmaxf(floorf(a), 0.f), 2.0e9f);
    s_hi = (int)min((long long)fmaxf(fminf(ceilf(e), 2.0e9f), -1.0f), last);
}

// whether a RoI's samples can touch the tile of cells [ty0, ty1] x [tx0, tx1]: conservative, the gather tests each sample exactly
__device__ __forceinline__ bool align_touches_tile(const RoiGeom& g, int out_h, int out_w, int ty0, int ty1, int tx0, int tx1)
{
    if (g.grid_h <= 0 || g.grid_w <= 0) return false;
    // every sample lies between start and start + out * bin; its footprint within one cell of it (two: margin for rounding)
    const float ey = g.start_h + g.bin_h * (float)out_h, ex = g.start_w + g.bin_w * (float)out_w;
    return fmaxf(g.start_h, ey) + 2.f >= (float)ty0 && fminf(g.start_h, ey) - 2.f <= (float)ty1 &&
           fmaxf(g.start_w, ex) + 2.f >= (float)tx0 && fminf(g.start_w, ex) - 2.f <= (float)tx1;
}

// Adds to acc the gradient that one RoI (plan g, output gradient rows dr [out_h][out_w][C4] runs) sends to cell (cy, cx), channel run c4
// (act: c4 < C4): the per-RoI body of the gather, shared by ops_roi_align_backward_kernel and ops_ms_roi_align_backward_kernel.
template <typename E>
__device__ __forceinline__ void align_cell_grad(const RoiGeom& g, const E* __restrict__ dr, int fh, int fw, int cy, int cx, int out_h,
                                                int out_w, int C4, int c4, bool act, typename Run<E>::vec& acc)
{
    int ys0, ys1, xs0, xs1;
    sample_range(cy, g.start_h, g.bin_h, g.grid_h, out_h, ys0, ys1);
    sample_range(cx, g.start_w, g.bin_w, g.grid_w, out_w, xs0, xs1);
    // a bin's samples form a grid_h x grid_w product, so the cell's weight in bin (ph, pw) is (sum of its row weights
    // in ph) x (sum of its column weights in pw): one term per bin, not per sample (256 float32 terms per bin at
    // sampling_ratio 16 drift ~4e-6 from the float64 sum)
    for (int sy = ys0; sy <= ys1; ) {
        const int ph = sy / g.grid_h, y_end = min(ys1, (ph + 1) * g.grid_h - 1);
        float wy_sum = 0.f;
        bool y_hit = false;
        for (; sy <= y_end; ++sy) {
            float wy;
            if (cell_weight(sample_coord(g.start_h, g.bin_h, g.grid_h, ph, sy - ph * g.grid_h), fh, cy, wy)) {
                wy_sum += wy;
                y_hit = true;
            }
        }
        if (!y_hit) continue;
        for (int sx = xs0; sx <= xs1; ) {
            const int pw = sx / g.grid_w, x_end = min(xs1, (pw + 1) * g.grid_w - 1);
            float wx_sum = 0.f;
            bool x_hit = false;
            for (; sx <= x_end; ++sx) {
                float wx;
                if (cell_weight(sample_coord(g.start_w, g.bin_w, g.grid_w, pw, sx - pw * g.grid_w), fw, cx, wx)) {
                    wx_sum += wx;
                    x_hit = true;
                }
            }
            if (x_hit && act) acc = acc + (Run<E>::load(dr, ((size_t)ph * out_w + pw) * C4 + c4) * (wy_sum * wx_sum)) / g.count;
        }
    }
}

template <typename E>
__global__ __launch_bounds__(256)
void ops_roi_align_backward_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w,
                                   float scale, int sampling_ratio, int aligned, const E* __restrict__ dout, E* __restrict__ dx)
{
    __shared__ int s_list[OPS_LIST];
    __shared__ int s_cnt[4];
    __shared__ int s_n;
    const int C4 = C / Run<E>::V, n_chunks = (C4 + 63) >> 6;
    const int img = blockIdx.z / n_chunks, chunk = blockIdx.z - img * n_chunks;
    const int ty0 = blockIdx.y * OPS_TILE, tx0 = blockIdx.x * OPS_TILE;
    const int ty1 = min(ty0 + OPS_TILE, fh) - 1, tx1 = min(tx0 + OPS_TILE, fw) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = chunk * 64 + lane;
    const bool act = c4 < C4;
    const int cy = ty0 + wave / OPS_TILE, cx = tx0 + wave % OPS_TILE;       // this wave's cell, for every pass
    const bool cell_ok = cy <= ty1 && cx <= tx1;

    auto touches = [&](int r) {
        const float* roi = rois + (size_t)r * 5;
        int b;
        if (!roi_image(roi[0], n_img, b) || b != img) return false;
        return align_touches_tile(ops_align_geom(roi, scale, out_h, out_w, sampling_ratio, aligned), out_h, out_w, ty0, ty1, tx0, tx1);
    };

    typename Run<E>::vec acc = 0.f;
    int r_next = 0;
    do {
        r_next = cull_rois(r_next, k, touches, s_list, s_cnt, &s_n);
        const int n_list = s_n;
        if (cell_ok)
            for (int li = 0; li < n_list; ++li) {
                const int r = s_list[li];
                align_cell_grad<E>(ops_align_geom(rois + (size_t)r * 5, scale, out_h, out_w, sampling_ratio, aligned),
                                   dout + (size_t)r * out_h * out_w * C, fh, fw, cy, cx, out_h, out_w, C4, c4, act, acc);
            }
    } while (r_next < k);
    if (cell_ok && act) Run<E>::store(dx + (size_t)img * fh * fw * C, ((size_t)cy * fw + cx) * C4 + c4, acc);
}

// ---- multi-scale RoIAlign (torchvision.ops.MultiScaleRoIAlign) ------------------------------------------------------------------
// Every level's descriptor travels in one by-value argument.  block0: the level's first block in the backward grid, which is flattened
// over (image, channel chunk, tile row, tile column) of every level in turn.
struct OpsMsLevel {
    const void* x;                            // maps and gradients of the launch's element type
    void* dx;
    int fh, fw, tiles_y, tiles_x, block0;
    float scale;
};
struct OpsMsArgs {
    OpsMsLevel lv[OPS_MS_MAX_LEVELS];
    int n_levels, n_img, C, out_h, out_w, sampling_ratio, k_min, k_max;
    float canonical_level, inv_canonical_scale;
};

template <typename T> __device__ __forceinline__ T uniform(T v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T> __device__ __forceinline__ T* uniform(T* p)
{
    const u64 v = (u64)p;
    return (T*)(((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v));
}

// a.lv[l] for a block-uniform l, as scalar selects: each field is read into a register first, else the compiler folds the selects
// into a dynamic index over a private copy of the argument (scratch)
__device__ __forceinline__ OpsMsLevel ms_level(const OpsMsArgs& a, int l)
{
    OpsMsLevel d = a.lv[0];
#pragma unroll
    for (int i = 1; i < OPS_MS_MAX_LEVELS; ++i) {
        const OpsMsLevel& s = a.lv[i];
        const void* x = uniform(s.x);
        void* dx = uniform(s.dx);
        const int fh = uniform(s.fh), fw = uniform(s.fw), ty = uniform(s.tiles_y), tx = uniform(s.tiles_x), b0 = uniform(s.block0);
        const float sc = __int_as_float(uniform(__float_as_int(s.scale)));
        if (l == i) d = OpsMsLevel{x, dx, fh, fw, ty, tx, b0, sc};
    }
    return d;
}

// torchvision's LevelMapper on one RoI row, in float32 and in its order of operations, on the GPU as torch evaluates it (s / s0 is
// s * (1 / s0) there):  floor(canonical_level + log2(sqrt(area) / canonical_scale) + 1e-6), torch.clamp to [k_min, k_max] (k_max when
// k_min > k_max), minus k_min.  -1 for a NaN level (negative or NaN area: no level, as on torchvision's CPU path) and for an index
// outside [0, n_levels).  One level: every RoI is on it, as in torchvision's num_levels == 1 branch.
__device__ __forceinline__ int ms_roi_level(const float* roi, const OpsMsArgs& a)
{
    if (a.n_levels == 1) return 0;
    const float area = (roi[3] - roi[1]) * (roi[4] - roi[2]);
    const float v = floorf((a.canonical_level + log2f(sqrtf(area) * a.inv_canonical_scale)) + 1e-6f);
    if (v != v) return -1;
    float t = v < (float)a.k_min ? (float)a.k_min : v;
    t = t > (float)a.k_max ? (float)a.k_max : t;
    const int l = (int)t - a.k_min;
    return l >= 0 && l < a.n_levels ? l : -1;
}

// the (level, image) bucket of a RoI; -1: no level or an image outside [0, n_img)
__device__ __forceinline__ int ms_bucket(const float* roi, const OpsMsArgs& a)
{
    int b;
    if (!roi_image(roi[0], a.n_img, b)) return -1;
    const int l = ms_roi_level(roi, a);
    return l < 0 ? -1 : l * a.n_img + b;
}

// One block per (roi, ph), as ops_roi_align_kernel: the RoI's level (uniform over the block) picks the map and the scale.
template <typename E>
__global__ __launch_bounds__(256)
void ops_ms_roi_align_kernel(const OpsMsArgs a, const float* __restrict__ rois, E* __restrict__ out)
{
    const int r = blockIdx.x, ph = blockIdx.y;
    const float* roi = rois + (size_t)r * 5;
    E* orow = out + ((size_t)r * a.out_h + ph) * a.out_w * a.C;
    const int l = __builtin_amdgcn_readfirstlane(ms_roi_level(roi, a));      // uniform: one RoI per block
    const OpsMsLevel d = ms_level(a, l);
    int b;
    if (l < 0 || d.fh == 0 || d.fw == 0 || !roi_image(roi[0], a.n_img, b)) {
        zero_row(orow, a.out_w * (a.C / Run<E>::V));
        return;
    }
    align_row(static_cast<const E*>(d.x) + (size_t)b * d.fh * d.fw * a.C, d.fh, d.fw, a.C,
              ops_align_geom(roi, d.scale, a.out_h, a.out_w, a.sampling_ratio, 0), ph, a.out_w, orow);
}

// One block per (level, image) bucket: ids[span[2 q] .. span[2 q + 1]) = the RoIs of bucket q in ascending order; the buckets follow
// one another in bucket order.  Two passes over the RoIs: count those of lower buckets and of this one, then list this one's.
__global__ __launch_bounds__(256)
void ops_ms_bucket_kernel(const OpsMsArgs a, const float* __restrict__ rois, int k, int* __restrict__ ids, int* __restrict__ span)
{
    __shared__ int s_lo[4], s_own[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo = 0, own = 0;
    for (int r = tid; r < k; r += 256) {
        const int qr = ms_bucket(rois + (size_t)r * 5, a);
        lo += qr >= 0 && qr < q;
        own += qr == q;
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo += __shfl_xor(lo, o);
        own += __shfl_xor(own, o);
    }
    if (lane == 0) { s_lo[wave] = lo; s_own[wave] = own; }
    __syncthreads();
    const int begin = s_lo[0] + s_lo[1] + s_lo[2] + s_lo[3];
    if (tid == 0) {
        span[2 * q] = begin;
        span[2 * q + 1] = begin + s_own[0] + s_own[1] + s_own[2] + s_own[3];
    }
    int base = begin;
    for (int r0 = 0; r0 < k; r0 += 256) {
        const int r = r0 + tid;
        const bool hit = r < k && ms_bucket(rois + (size_t)r * 5, a) == q;
        const u64 m = __ballot(hit);
        __syncthreads();                                 // the previous group has read s_own
        if (lane == 0) s_own[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_own[w];
        if (hit) ids[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
        base += s_own[0] + s_own[1] + s_own[2] + s_own[3];
    }
}

// The backward of ops_ms_roi_align_kernel: ops_roi_align_backward_kernel's gather on every level in one grid, each block culling only
// the RoIs of its (level, image) bucket, in ascending order -- the RoIs, and the order, of that level's ops_roi_align_backward_kernel.
template <typename E>
__global__ __launch_bounds__(256)
void ops_ms_roi_align_backward_kernel(const OpsMsArgs a, const float* __restrict__ rois, const int* __restrict__ ids,
                                      const int* __restrict__ span, const E* __restrict__ dout)
{
    __shared__ int s_list[OPS_LIST];
    __shared__ int s_cnt[4];
    __shared__ int s_n;
    const int bid = blockIdx.x;
    int l = 0;
#pragma unroll
    for (int i = 1; i < OPS_MS_MAX_LEVELS; ++i)
        if (i < a.n_levels && bid >= a.lv[i].block0) l = i;
    const OpsMsLevel d = ms_level(a, l);
    const int fh = d.fh, fw = d.fw, C = a.C, out_h = a.out_h, out_w = a.out_w;
    const int C4 = C / Run<E>::V, n_chunks = (C4 + 63) >> 6;
    int t = bid - d.block0;
    const int tx = t % d.tiles_x;
    t /= d.tiles_x;
    const int ty = t % d.tiles_y;
    t /= d.tiles_y;
    const int img = t / n_chunks, chunk = t - img * n_chunks;
    const int ty0 = ty * OPS_TILE, tx0 = tx * OPS_TILE;
    const int ty1 = min(ty0 + OPS_TILE, fh) - 1, tx1 = min(tx0 + OPS_TILE, fw) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = chunk * 64 + lane;
    const bool act = c4 < C4;
    const int cy = ty0 + wave / OPS_TILE, cx = tx0 + wave % OPS_TILE;
    const bool cell_ok = cy <= ty1 && cx <= tx1;
    const int q = l * a.n_img + img;
    const int* const bucket = ids + span[2 * q];
    const int n_bucket = span[2 * q + 1] - span[2 * q];

    auto touches = [&](int i) {
        return align_touches_tile(ops_align_geom(rois + (size_t)bucket[i] * 5, d.scale, out_h, out_w, a.sampling_ratio, 0), out_h, out_w,
                                  ty0, ty1, tx0, tx1);
    };

    typename Run<E>::vec acc = 0.f;
    int i_next = 0;
    do {
        i_next = cull_rois(i_next, n_bucket, touches, s_list, s_cnt, &s_n);
        const int n_list = s_n;
        if (cell_ok)
            for (int li = 0; li < n_list; ++li) {
                const int r = bucket[s_list[li]];
                align_cell_grad<E>(ops_align_geom(rois + (size_t)r * 5, d.scale, out_h, out_w, a.sampling_ratio, 0),
                                   dout + (size_t)r * out_h * out_w * C, fh, fw, cy, cx, out_h, out_w, C4, c4, act, acc);
            }
    } while (i_next < n_bucket);
    if (cell_ok && act) Run<E>::store(static_cast<E*>(d.dx) + (size_t)img * fh * fw * C, ((size_t)cy * fw + cx) * C4 + c4, acc);
}

// ---- RoIPool ------------------------------------------------------------------------------------------------------------------------
// torchvision's roi_pool geometry (oracle/frcnn_oracle.py: roi_pool) for out_h x out_w bins
struct PoolGeom { int rs_h, rs_w; float bin_h, bin_w; };

__device__ __forceinline__ PoolGeom ops_pool_geom(const float* roi, float scale, int out_h, int out_w)
{
    PoolGeom g;
    g.rs_w = (int)roundf(roi[1] * scale); g.rs_h = (int)roundf(roi[2] * scale);
    const int re_w = (int)roundf(roi[3] * scale), re_h = (int)roundf(roi[4] * scale);
    const int roi_w = max(re_w - g.rs_w + 1, 1), roi_h = max(re_h - g.rs_h + 1, 1);
    g.bin_h = (float)roi_h / (float)out_h; g.bin_w = (float)roi_w / (float)out_w;
    return g;
}
__device__ __forceinline__ void pool_bin(int p, float bin, int rs, int limit, int& s, int& e)
{
    const int a = (int)floorf((float)p * bin) + rs, b = (int)ceilf((float)(p + 1) * bin) + rs;
    s = min(max(a, 0), limit); e = min(max(b, 0), limit);
}

// One block per bin (roi, ph, pw), one thread per channel run: the max and the argmax cell (h * fw + w; -1 for an empty bin) per
// channel, first maximum in (h, w) scan order with torchvision's strict '>' from -FLT_MAX.
template <typename E>
__global__ __launch_bounds__(128)
void ops_roi_pool_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, int out_h,
                         int out_w, float scale, E* __restrict__ out, int32_t* __restrict__ argmax)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    typedef typename R::ivec ivec;
    const int r = blockIdx.x, ph = blockIdx.y, pw = blockIdx.z;
    const int C4 = C / R::V;
    const float* roi = rois + (size_t)r * 5;
    const size_t o = (((size_t)r * out_h + ph) * out_w + pw) * C4;
    ivec* const ap = reinterpret_cast<ivec*>(argmax) + o;
    int b, hs = 0, he = 0, ws = 0, we = 0;
    if (roi_image(roi[0], n_img, b)) {
        const PoolGeom g = ops_pool_geom(roi, scale, out_h, out_w);
        pool_bin(ph, g.bin_h, g.rs_h, fh, hs, he);
        pool_bin(pw, g.bin_w, g.rs_w, fw, ws, we);
    } else {
        b = 0;
    }
    const bool empty = he <= hs || we <= ws;
    const E* const fm = x + (size_t)b * fh * fw * C;
    for (int c4 = threadIdx.x; c4 < C4; c4 += 128) {
        vec m = empty ? 0.f : -FLT_MAX;
        ivec am = -1;
        for (int h = hs; h < he; ++h)
            for (int w = ws; w < we; ++w) {
                const int cell = h * fw + w;
                const vec v = R::load(fm, (size_t)cell * C4 + c4);
#pragma unroll
                for (int j = 0; j < R::V; ++j)
                    if (v[j] > m[j]) { m[j] = v[j]; am[j] = cell; }
            }
        R::store(out, o + c4, m);
        ap[c4] = am;
    }
}

template <typename E>
__global__ __launch_bounds__(256)
void ops_roi_pool_backward_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w,
                                  float scale, const int32_t* __restrict__ argmax, const E* __restrict__ dout, E* __restrict__ dx)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    typedef typename R::ivec ivec;
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
    const int cy = ty0 + wave / OPS_TILE, cx = tx0 + wave % OPS_TILE;
    const bool cell_ok = cy <= ty1 && cx <= tx1;
    const int cell = cy * fw + cx;

    auto touches = [&](int r) {
        const float* roi = rois + (size_t)r * 5;
        int b;
        if (!roi_image(roi[0], n_img, b) || b != img) return false;
        const PoolGeom g = ops_pool_geom(roi, scale, out_h, out_w);
        // the bins cover [rs, rs + ceil(out * bin)) along each axis, out * bin = the RoI's size
        const float eh = (float)g.rs_h + g.bin_h * (float)out_h + 1.f, ew = (float)g.rs_w + g.bin_w * (float)out_w + 1.f;
        return eh >= (float)ty0 && (float)g.rs_h <= (float)ty1 && ew >= (float)tx0 && (float)g.rs_w <= (float)tx1;
    };

    vec acc = 0.f;
    int r_next = 0;
    do {
        r_next = cull_rois(r_next, k, touches, s_list, s_cnt, &s_n);
        const int n_list = s_n;
        if (cell_ok)
            for (int li = 0; li < n_list; ++li) {
                const int r = s_list[li];
                const PoolGeom g = ops_pool_geom(rois + (size_t)r * 5, scale, out_h, out_w);
                // bin p holds offset t iff floor(p bin) <= t < ceil((p + 1) bin): p in (t / bin - 1, (t + 1) / bin), widened by one
                const int th = cy - g.rs_h, tw = cx - g.rs_w;
                const int ph0 = max((int)floorf((float)th / g.bin_h) - 2, 0), ph1 = min((int)ceilf((float)(th + 1) / g.bin_h) + 1, out_h - 1);
                const int pw0 = max((int)floorf((float)tw / g.bin_w) - 2, 0), pw1 = min((int)ceilf((float)(tw + 1) / g.bin_w) + 1, out_w - 1);
                const size_t rb = (size_t)r * out_h * out_w * C4;
                for (int ph = ph0; ph <= ph1; ++ph) {
                    int hs, he;
                    pool_bin(ph, g.bin_h, g.rs_h, fh, hs, he);
                    if (cy < hs || cy >= he) continue;
                    for (int pw = pw0; pw <= pw1; ++pw) {
                        int ws, we;
                        pool_bin(pw, g.bin_w, g.rs_w, fw, ws, we);
                        if (cx < ws || cx >= we || !act) continue;
                        const size_t o = rb + ((size_t)ph * out_w + pw) * C4 + c4;
                        const ivec am = reinterpret_cast<const ivec*>(argmax)[o];
                        const vec gv = R::load(dout, o);
#pragma unroll
                        for (int j = 0; j < R::V; ++j)
                            if (am[j] == cell) acc[j] += gv[j];
                    }
                }
            }
    } while (r_next < k);
    if (cell_ok && act) R::store(dx + (size_t)img * fh * fw * C, (size_t)cell * C4 + c4, acc);
}

// ---- NMS ----------------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ bool ops_iou_gt(const T* a, const T* b, float thr);
template <> __device__ __forceinline__ bool ops_iou_gt<float>(const float* a, const float* b, float thr)
{
    return iou_gt(f32x4{a[0], a[1], a[2], a[3]}, f32x4{b[0], b[1], b[2], b[3]}, thr);
}
// torchvision's devIoU for double: the whole decision in float64 against the float threshold
template <> __device__ __forceinline__ bool ops_iou_gt<double>(const double* a, const double* b, float thr)
{
    const double l0 = fmax(a[0], b[0]), l1 = fmax(a[1], b[1]);
    const double r0 = fmin(a[2], b[2]), r1 = fmin(a[3], b[3]);
    const double d0 = fmax(r0 - l0, 0.0), d1 = fmax(r1 - l1, 0.0);
    const double inter = d0 * d1;
    const double sa = (a[2] - a[0]) * (a[3] - a[1]);
    const double sb = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / (sa + sb - inter) > (double)thr;
}

// grid (nw, nw), one wave per 64 x 64 tile of the sorted order; bit j of word bx of row i: sorted box 64 bx + j (> i, same category)
// is suppressed by sorted box i.  Tiles below the diagonal, and tiles whose rows and columns cannot share a category, are not written.
template <typename T>
__global__ __launch_bounds__(64)
void ops_nms_mask_kernel(const T* __restrict__ boxes, const int64_t* __restrict__ order, const int64_t* __restrict__ cats, int n,
                         int nw, float thr, u64* __restrict__ mask)
{
    const int by = blockIdx.y, bx = blockIdx.x;
    if (bx < by) return;
    if (cats && cats[order[bx * 64]] > cats[order[min(by * 64 + 63, n - 1)]]) return;
    __shared__ T colb[64][4];
    __shared__ int64_t colc[64];
    const int t = threadIdx.x;
    const int jn = bx * 64 + t;
    if (jn < n) {
        const T* p = boxes + (size_t)order[jn] * 4;
        colb[t][0] = p[0]; colb[t][1] = p[1]; colb[t][2] = p[2]; colb[t][3] = p[3];
        colc[t] = cats ? cats[order[jn]] : 0;
    }
    __syncthreads();
    const int i = by * 64 + t;
    if (i >= n) return;
    const T* p = boxes + (size_t)order[i] * 4;
    const T a[4] = {p[0], p[1], p[2], p[3]};
    const int64_t ca = cats ? cats[order[i]] : 0;
    u64 bits = 0ull;
    const int jmax = min(n - bx * 64, 64);
    for (int j = 0; j < jmax; ++j)
        if (bx * 64 + j > i && colc[j] == ca && ops_iou_gt<T>(a, colb[j], thr)) bits |= 1ull << j;
    mask[(size_t)i * nw + bx] = bits;
}

// One wave per segment of the sorted order (a category of batched NMS; the whole list otherwise): block s works iff sorted position s
// starts a segment.  The segment's removed-bits live in LDS; per 64-box chunk the kept boxes are resolved serially on the chunk's
// diagonal words, then their rows are OR-ed into the words of the chunks after it.  keep[s] = 1 iff sorted box s is kept.
__global__ __launch_bounds__(64)
void ops_nms_reduce_kernel(const u64* __restrict__ mask, const int64_t* __restrict__ order, const int64_t* __restrict__ cats, int n,
                           int nw, uint8_t* __restrict__ keep)
{
    extern __shared__ __attribute__((aligned(16))) u64 ops_rem[];
    const int s0 = blockIdx.x, lane = threadIdx.x;
    int s1 = n;
    if (cats) {
        const int64_t cat = cats[order[s0]];
        if (s0 > 0 && cats[order[s0 - 1]] == cat) return;
        for (int base = s0 + 1; base < n; base += 64) {
            const int j = base + lane;
            const u64 m = __ballot(j < n && cats[order[j]] != cat);
            if (m) { s1 = base + __ffsll((long long)m) - 1; break; }
        }
    }
    const int w0 = s0 >> 6, w1 = (s1 - 1) >> 6;
    for (int w = lane; w <= w1 - w0; w += 64) ops_rem[w] = 0ull;
    __syncthreads();
    for (int c = w0; c <= w1; ++c) {
        const int row = c * 64 + lane;
        const bool in = row >= s0 && row < s1;
        const u64 diag = in ? mask[(size_t)row * nw + c] : 0ull;
        u64 alive = __ballot(in) & ~ops_rem[c - w0];
        u64 kept = 0ull;
        while (alive) {
            const int b = __ffsll((long long)alive) - 1;
            kept |= 1ull << b;
            alive &= ~(1ull << b);
            alive &= ~__shfl(diag, b);
        }
        if (in) keep[row] = (uint8_t)((kept >> lane) & 1ull);
        // the rows kept here remove from the later chunks of the segment: sixteen rows' loads in flight at a time
        for (u64 kk = c < w1 ? kept : 0ull; kk; ) {
            int rb[16];
            int cnt = 0;
            for (int q = 0; q < 16; ++q) {
                rb[q] = kk ? __ffsll((long long)kk) - 1 : rb[0];
                if (kk) { kk &= kk - 1ull; ++cnt; }
            }
            for (int w = c + 1 + lane; w <= w1; w += 64) {
                u64 v = 0ull;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q < cnt) v |= mask[(size_t)(c * 64 + rb[q]) * nw + w];
                ops_rem[w - w0] |= v;
            }
        }
        __syncthreads();
    }
}

// the greedy pass over a finished bit mask (frcnn_ops_nms here, frcnn_ops_nms_rotated in ops_rot.hip)
int launch_ops_nms_reduce(const u64* mask, const int64_t* order, const int64_t* cats, int n, int nw, uint8_t* keep, hipStream_t s)
{
    hipLaunchKernelGGL(ops_nms_reduce_kernel, dim3(cats ? n : 1), dim3(64), (size_t)nw * sizeof(u64), s, mask, order, cats, n, nw, keep);
    return check_launch();
}

// Fills the multi-scale argument (without map pointers) and the size of the backward grid; false on an invalid request.
static bool ms_args_ok(OpsMsArgs& a, long long& blocks, const int* fh, const int* fw, const float* scales, int n_levels, int n_img, int c,
                       int k, int out_h, int out_w, int sampling_ratio, float canonical_scale, float canonical_level, int k_min, int k_max,
                       int v)
{
    if (n_levels < 1 || n_levels > OPS_MS_MAX_LEVELS || !fh || !fw || !scales || n_img < 1 || c < v || c % v != 0 || k < 0 ||
        out_h < 1 || out_h > OPS_MAX_OUT || out_w < 1 || out_w > OPS_MAX_OUT || sampling_ratio > OPS_MAX_SAMPLING ||
        (long long)n_levels * n_img > INT32_MAX / 2)
        return false;
    a = OpsMsArgs{};
    a.n_levels = n_levels; a.n_img = n_img; a.C = c; a.out_h = out_h; a.out_w = out_w; a.sampling_ratio = sampling_ratio;
    a.k_min = k_min; a.k_max = k_max; a.canonical_level = canonical_level;
    a.inv_canonical_scale = 1.0f / canonical_scale;              // torch's tensor / scalar on the GPU: a * (1 / b), 1 / b in float32
    blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (fh[l] < 0 || fw[l] < 0 || (long long)fh[l] * fw[l] > INT32_MAX) return false;
        OpsMsLevel& d = a.lv[l];
        d.fh = fh[l]; d.fw = fw[l]; d.scale = scales[l];
        d.tiles_y = cdiv(fh[l], OPS_TILE); d.tiles_x = cdiv(fw[l], OPS_TILE);
        d.block0 = (int)min(blocks, (long long)INT32_MAX);
        blocks += (long long)d.tiles_y * d.tiles_x * n_img * cdiv(c / v, 64);
    }
    return blocks <= INT32_MAX;
}

// ---- the entry points' bodies, one per element type ---------------------------------------------------------------------------------
template <typename E>
static int roi_align_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                          float spatial_scale, int sampling_ratio, int aligned, void* d_out, void* stream)
{
    if (!roi_args_ok(n_img, fh, fw, c, k, out_h, out_w, Run<E>::V) || sampling_ratio > OPS_MAX_SAMPLING) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_roi_align_kernel<E>, dim3(k, out_h), dim3(256), 0, (hipStream_t)stream, static_cast<const E*>(d_x), n_img, fh,
                       fw, c, d_rois, out_h, out_w, spatial_scale, sampling_ratio, aligned ? 1 : 0, static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int roi_align_backward_impl(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                   int sampling_ratio, int aligned, const void* d_dout, void* d_dx, void* stream)
{
    if (!roi_args_ok(n_img, fh, fw, c, k, out_h, out_w, Run<E>::V) || sampling_ratio > OPS_MAX_SAMPLING) return FRCNN_EINVAL;
    if (!d_dx || (k > 0 && (!d_rois || !d_dout))) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_roi_align_backward_kernel<E>, dim3(cdiv(fw, OPS_TILE), cdiv(fh, OPS_TILE), n_img * cdiv(c / Run<E>::V, 64)),
                       dim3(256), 0, (hipStream_t)stream, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio,
                       aligned ? 1 : 0, static_cast<const E*>(d_dout), static_cast<E*>(d_dx));
    return check_launch();
}

template <typename E>
static int roi_pool_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                         float spatial_scale, void* d_out, int32_t* d_argmax, void* stream)
{
    if (!roi_args_ok(n_img, fh, fw, c, k, out_h, out_w, Run<E>::V)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out || !d_argmax) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_roi_pool_kernel<E>, dim3(k, out_h, out_w), dim3(128), 0, (hipStream_t)stream, static_cast<const E*>(d_x), n_img,
                       fh, fw, c, d_rois, out_h, out_w, spatial_scale, static_cast<E*>(d_out), d_argmax);
    return check_launch();
}

template <typename E>
static int roi_pool_backward_impl(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                  const int32_t* d_argmax, const void* d_dout, void* d_dx, void* stream)
{
    if (!roi_args_ok(n_img, fh, fw, c, k, out_h, out_w, Run<E>::V)) return FRCNN_EINVAL;
    if (!d_dx || (k > 0 && (!d_rois || !d_argmax || !d_dout))) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_roi_pool_backward_kernel<E>, dim3(cdiv(fw, OPS_TILE), cdiv(fh, OPS_TILE), n_img * cdiv(c / Run<E>::V, 64)),
                       dim3(256), 0, (hipStream_t)stream, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, d_argmax,
                       static_cast<const E*>(d_dout), static_cast<E*>(d_dx));
    return check_launch();
}

template <typename E>
static int ms_roi_align_impl(const void* const* d_x, const int* fh, const int* fw, const float* scales, int n_levels, int n_img, int c,
                             const float* d_rois, int k, int out_h, int out_w, int sampling_ratio, float canonical_scale,
                             float canonical_level, int k_min, int k_max, void* d_out, void* stream)
{
    OpsMsArgs a;
    long long blocks;
    if (!ms_args_ok(a, blocks, fh, fw, scales, n_levels, n_img, c, k, out_h, out_w, sampling_ratio, canonical_scale, canonical_level,
                    k_min, k_max, Run<E>::V))
        return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    for (int l = 0; l < n_levels; ++l) {
        if (!d_x[l] && fh[l] * fw[l] > 0) return FRCNN_EINVAL;
        a.lv[l].x = d_x[l];
    }
    hipLaunchKernelGGL(ops_ms_roi_align_kernel<E>, dim3(k, out_h), dim3(256), 0, (hipStream_t)stream, a, d_rois, static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int ms_roi_align_backward_impl(const float* d_rois, int k, const int* fh, const int* fw, const float* scales, int n_levels,
                                      int n_img, int c, int out_h, int out_w, int sampling_ratio, float canonical_scale,
                                      float canonical_level, int k_min, int k_max, const void* d_dout, void* const* d_dx, void* d_ws,
                                      size_t ws_bytes, void* stream)
{
    OpsMsArgs a;
    long long blocks;
    if (!ms_args_ok(a, blocks, fh, fw, scales, n_levels, n_img, c, k, out_h, out_w, sampling_ratio, canonical_scale, canonical_level,
                    k_min, k_max, Run<E>::V))
        return FRCNN_EINVAL;
    if (!d_dx || !d_ws || ws_bytes < frcnn_ops_ms_roi_align_workspace_bytes(k, n_levels, n_img) || (k > 0 && (!d_rois || !d_dout)))
        return FRCNN_EINVAL;
    for (int l = 0; l < n_levels; ++l) {
        if (!d_dx[l] && fh[l] * fw[l] > 0) return FRCNN_EINVAL;
        a.lv[l].dx = d_dx[l];
    }
    if (blocks == 0) return FRCNN_OK;
    int* const span = static_cast<int*>(d_ws);
    int* const ids = span + 2 * n_levels * n_img;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ops_ms_bucket_kernel, dim3(n_levels * n_img), dim3(256), 0, s, a, d_rois, k, ids, span);
    const int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(ops_ms_roi_align_backward_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, s, a, d_rois, ids, span,
                       static_cast<const E*>(d_dout));
    return check_launch();
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_roi_align(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                        float spatial_scale, int sampling_ratio, int aligned, float* d_out, void* stream)
{
    return roi_align_impl<float>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, sampling_ratio, aligned, d_out, stream);
}

int frcnn_ops_roi_align_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                 int sampling_ratio, int aligned, const float* d_dout, float* d_dx, void* stream)
{
    return roi_align_backward_impl<float>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, aligned, d_dout, d_dx,
                                          stream);
}

int frcnn_ops_roi_pool(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                       float spatial_scale, float* d_out, int32_t* d_argmax, void* stream)
{
    return roi_pool_impl<float>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, d_out, d_argmax, stream);
}

int frcnn_ops_roi_pool_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w, float spatial_scale,
                                const int32_t* d_argmax, const float* d_dout, float* d_dx, void* stream)
{
    return roi_pool_backward_impl<float>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, d_argmax, d_dout, d_dx, stream);
}

size_t frcnn_ops_ms_roi_align_workspace_bytes(int k, int n_levels, int n_img)
{
    if (k < 0 || n_levels < 1 || n_levels > OPS_MS_MAX_LEVELS || n_img < 1 || (long long)n_levels * n_img > INT32_MAX / 2) return 0;
    return ((size_t)k + 2 * (size_t)n_levels * n_img) * sizeof(int);
}

int frcnn_ops_ms_roi_align(const float* const* d_x, const int* fh, const int* fw, const float* scales, int n_levels, int n_img, int c,
                           const float* d_rois, int k, int out_h, int out_w, int sampling_ratio, float canonical_scale,
                           float canonical_level, int k_min, int k_max, float* d_out, void* stream)
{
    return ms_roi_align_impl<float>(reinterpret_cast<const void* const*>(d_x), fh, fw, scales, n_levels, n_img, c, d_rois, k, out_h, out_w,
                                    sampling_ratio, canonical_scale, canonical_level, k_min, k_max, d_out, stream);
}

int frcnn_ops_ms_roi_align_backward(const float* d_rois, int k, const int* fh, const int* fw, const float* scales, int n_levels, int n_img,
                                    int c, int out_h, int out_w, int sampling_ratio, float canonical_scale, float canonical_level,
                                    int k_min, int k_max, const float* d_dout, float* const* d_dx, void* d_ws, size_t ws_bytes,
                                    void* stream)
{
    return ms_roi_align_backward_impl<float>(d_rois, k, fh, fw, scales, n_levels, n_img, c, out_h, out_w, sampling_ratio, canonical_scale,
                                             canonical_level, k_min, k_max, d_dout, reinterpret_cast<void* const*>(d_dx), d_ws, ws_bytes,
                                             stream);
}

int frcnn_ops_half_run(void) { return OPS_HALF_RUN; }

int frcnn_ops_roi_align_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                           int out_w, float spatial_scale, int sampling_ratio, int aligned, void* d_out, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, OPS_HALF_RUN, roi_align_impl, d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, sampling_ratio, aligned,
                    d_out, stream);
}

int frcnn_ops_roi_align_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                    float spatial_scale, int sampling_ratio, int aligned, const void* d_dout, void* d_dx, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), roi_align_backward_impl, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, aligned,
                    d_dout, d_dx, stream);
}

int frcnn_ops_roi_pool_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                          int out_w, float spatial_scale, void* d_out, int32_t* d_argmax, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, OPS_HALF_RUN, roi_pool_impl, d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, d_out, d_argmax, stream);
}

int frcnn_ops_roi_pool_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                   float spatial_scale, const int32_t* d_argmax, const void* d_dout, void* d_dx, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), roi_pool_backward_impl, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, d_argmax, d_dout, d_dx,
                    stream);
}

int frcnn_ops_ms_roi_align_16(int elem_type, const void* const* d_x, const int* fh, const int* fw, const float* scales, int n_levels,
                              int n_img, int c, const float* d_rois, int k, int out_h, int out_w, int sampling_ratio,
                              float canonical_scale, float canonical_level, int k_min, int k_max, void* d_out, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, OPS_HALF_RUN, ms_roi_align_impl, d_x, fh, fw, scales, n_levels, n_img, c, d_rois, k, out_h, out_w, sampling_ratio,
                    canonical_scale, canonical_level, k_min, k_max, d_out, stream);
}

int frcnn_ops_ms_roi_align_backward_16(int elem_type, const float* d_rois, int k, const int* fh, const int* fw, const float* scales,
                                       int n_levels, int n_img, int c, int out_h, int out_w, int sampling_ratio, float canonical_scale,
                                       float canonical_level, int k_min, int k_max, const void* d_dout, void* const* d_dx, void* d_ws,
                                       size_t ws_bytes, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), ms_roi_align_backward_impl, d_rois, k, fh, fw, scales, n_levels, n_img, c, out_h, out_w, sampling_ratio,
                    canonical_scale, canonical_level, k_min, k_max, d_dout, d_dx, d_ws, ws_bytes, stream);
}

size_t frcnn_ops_nms_workspace_bytes(int n)
{
    if (n <= 0 || n > 64 * OPS_NMS_MAX_WORDS) return 0;
    return (size_t)n * (size_t)cdiv(n, 64) * sizeof(u64);
}

int frcnn_ops_nms(const void* d_boxes, int boxes_f64, const int64_t* d_order, const int64_t* d_categories, int n, float iou_threshold,
                  uint8_t* d_keep, void* d_ws, size_t ws_bytes, void* stream)
{
    if (n < 0 || n > 64 * OPS_NMS_MAX_WORDS || (boxes_f64 != 0 && boxes_f64 != 1)) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_boxes || !d_order || !d_keep || !d_ws || ws_bytes < frcnn_ops_nms_workspace_bytes(n)) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    const int nw = cdiv(n, 64);
    u64* mask = static_cast<u64*>(d_ws);
    if (boxes_f64)
        hipLaunchKernelGGL(ops_nms_mask_kernel<double>, dim3(nw, nw), dim3(64), 0, s, static_cast<const double*>(d_boxes), d_order,
                           d_categories, n, nw, iou_threshold, mask);
    else
        hipLaunchKernelGGL(ops_nms_mask_kernel<float>, dim3(nw, nw), dim3(64), 0, s, static_cast<const float*>(d_boxes), d_order,
                           d_categories, n, nw, iou_threshold, mask);
    const int rc = check_launch();
    if (rc) return rc;
    return launch_ops_nms_reduce(mask, d_order, d_categories, n, nw, d_keep, s);
}

}  // extern "C"
