// ops_dcnv3.hip -- DCNv3, the deformable convolution v3 of the InternImage backbones, in both directions: the frcnn_ops_dcnv3* entry
// points of include/frcnn_hip.h.  Restated from the published operator (third party, absent here: restated, unpinned, like the other
// operators of fasterrcnn_amd.ops; where the two differ include/frcnn_hip.h holds).
//
//   Channels-last tensors: input [n][H][W][G Gc], offset float32 [n][Ho][Wo][G K 2] pairs (dx, dy), mask float32 [n][Ho][Wo][G K],
//   out [n][Ho][Wo][G Gc]; K = kh kw, point p = i kh + j with i in [0, kw) along x (the outer index) and j in [0, kh) along y.  With
//   bx = dil_w (kw - 1) / 2 and by = dil_h (kh - 1) / 2 (integer division) the sample (b, oy, ox, g, p) lies at
//       x = (ox stride_w - pad_w + bx) + ((i dil_w - bx) + dx) * offset_scale,   y likewise with (oy, j, h, dy):
//   the integer parts in int, the rest in float32, in pixels of the unpadded map; there is no normalised location in between.  The sample
//   counts iff x > -1 && y > -1 && x < W && y < H (ops_deform.h: deform_sample, a NaN fails); its corners and weights are deform_corners'.
//   out[b][oy][ox][g Gc + c] = sum over p ascending of mask * (((w0 v0 + w1 v1) + w2 v2) + w3 v3), every product and sum in float32.
//
// Mapping (forward and d_offset / d_mask), that of ops_msda.hip with one level of K points: an item is one (b, oy, ox, g); a group of T
// lanes (a power of two <= 64) serves it, lanes along Gc, so a corner read is one contiguous run of input[b][cell][g][:]: R = 4 floats or
// 8 16-bit values per lane (16 B) when Gc holds whole runs and the tensors are 16-byte aligned, else the scalar body.  256 / T items share
// a block, fewer when their K samples would not fit MSDA_LDS_SAMPLES; the block's offsets and masks are one contiguous piece of offset /
// mask, staged once in LDS by coalesced loads (consecutive lanes write consecutive words: no bank conflict; the lanes of a group read
// one word: a broadcast).
// d_offset / d_mask: per sample, a lane's partial sums over its channels, then an xor butterfly over the T lanes (a fixed order), one
// store per (b, oy, ox, g, p) by the group's lane 0.
// d_input: the plan writes one entry per sample and corner, e = (((b Q + q) G + g) K + p) 4 + corner with Q = Ho Wo, the key
// (b S + cell) G + g with S = H W, or the sentinel n S G for a corner that counts 0, and the weight corner weight * mask.  The caller sorts
// the keys stably and ops_msda.hip's gather (msda_gather: it uses an item's samples only as their number) sums each cell's entries in
// ascending e: no atomics, every cell written, no bit depends on how the images are chunked.
#include "ops_msda.h"
#include "ops_deform.h"

#include <cmath>

namespace frcnn {

static constexpr int DCNV3_MAX_KERNEL = 7;
static constexpr int DCNV3_MAX_STEP = 1 << 16;           // stride, dilation and padding: the integer parts of a coordinate stay far inside int

static_assert(DCNV3_MAX_KERNEL * DCNV3_MAX_KERNEL <= MSDA_LDS_SAMPLES, "one item's samples fit the staging buffer");

struct DcGeom { int H, W, Ho, Wo, G, K, kh, sh, sw, ph, pw, dh, dw, bx, by; float scale; };

// the tensors of one call as the sampling kernels see them
struct DcDims { long long items; DcGeom s; int Gc, T, nruns, ipb; };

// item ((b Q + q) G + g): its image, output pixel and group
struct DcItem { long long b; int oy, ox, g; };

__device__ __forceinline__ DcItem dc_item(const DcGeom& s, long long item)
{
    DcItem it;
    const long long pix = item / s.G;
    it.g = (int)(item - pix * s.G);
    const long long row = pix / s.Wo;
    it.ox = (int)(pix - row * s.Wo);
    it.b = row / s.Ho;
    it.oy = (int)(row - it.b * s.Ho);
    return it;
}

// valid: the sample counts.  cell[k] >= 0: corner k lies inside the map (y W + x); w[k]: its bilinear weight; hh, lh, hw, lw: the fractions
struct DcSample { int cell[4]; float w[4]; float hh, lh, hw, lw; bool valid; };

__device__ __forceinline__ DcSample dc_sample(const DcGeom& s, int oy, int ox, int p, float dx, float dy)
{
    DcSample r;
    const int i = p / s.kh, j = p - i * s.kh;
    const float x = (float)(ox * s.sw - s.pw + s.bx) + ((float)(i * s.dw - s.bx) + dx) * s.scale;
    const float y = (float)(oy * s.sh - s.ph + s.by) + ((float)(j * s.dh - s.by) + dy) * s.scale;
    DeformSample d;
    r.valid = deform_sample(y, x, s.H, s.W, d);
    if (!r.valid) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { r.cell[k] = -1; r.w[k] = 0.f; }
        r.hh = r.lh = r.hw = r.lw = 0.f;
        return r;
    }
    deform_corners(d, s.H, s.W, r.w, r.cell);
    r.hh = d.hh; r.lh = d.lh; r.hw = d.hw; r.lw = d.lw;
    return r;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
template <typename E, int R, int PASSES>
__global__ __launch_bounds__(MSDA_BLOCK)
void dcnv3_forward_kernel(const E* __restrict__ input, const float* __restrict__ offset, const float* __restrict__ mask, DcDims g,
                          E* __restrict__ out)
{
    __shared__ float s_off[2 * MSDA_LDS_SAMPLES];
    __shared__ float s_w[MSDA_LDS_SAMPLES];
    const int K = g.s.K;
    const long long item0 = (long long)blockIdx.x * g.ipb;
    const long long left = g.items - item0;
    const int n_here = left < g.ipb ? (int)left : g.ipb;
    for (int i = threadIdx.x; i < n_here * K * 2; i += blockDim.x) s_off[i] = offset[item0 * K * 2 + i];
    for (int i = threadIdx.x; i < n_here * K; i += blockDim.x) s_w[i] = mask[item0 * K + i];
    __syncthreads();
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    if (grp >= n_here) return;
    const long long item = item0 + grp;
    const DcItem at = dc_item(g.s, item);
    const size_t cell_stride = (size_t)g.s.G * g.Gc;
    const E* const vb = input + ((size_t)at.b * g.s.H * g.s.W * g.s.G + at.g) * g.Gc;
    MsVec<R> acc[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[it].v[j] = 0.f;
    for (int p = 0; p < K; ++p) {
        const int si = grp * K + p;
        const DcSample s = dc_sample(g.s, at.oy, at.ox, p, s_off[2 * si], s_off[2 * si + 1]);
        if (!s.valid) continue;
        const float aw = s_w[si];
#pragma unroll
        for (int it = 0; it < PASSES; ++it) {
            const int run = t + it * g.T;
            if (run >= g.nruns) continue;
            MsVec<R> v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (s.cell[k] >= 0) {
                    v[k] = ms_load<E, R>(vb + (size_t)s.cell[k] * cell_stride + (size_t)run * R);
                } else {
#pragma unroll
                    for (int j = 0; j < R; ++j) v[k].v[j] = 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float val = ((s.w[0] * v[0].v[j] + s.w[1] * v[1].v[j]) + s.w[2] * v[2].v[j]) + s.w[3] * v[3].v[j];
                acc[it].v[j] += aw * val;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int run = t + it * g.T;
        if (run < g.nruns) ms_store<E, R>(out + (size_t)item * g.Gc + (size_t)run * R, acc[it]);
    }
}

// ---- d_offset, d_mask ------------------------------------------------------------------------------------------------------------------
template <typename E, int R, int PASSES>
__global__ __launch_bounds__(MSDA_BLOCK)
void dcnv3_backward_offset_kernel(const E* __restrict__ input, const float* __restrict__ offset, const float* __restrict__ mask,
                                  const E* __restrict__ dout, DcDims g, float* __restrict__ doffset, float* __restrict__ dmask)
{
    __shared__ float s_off[2 * MSDA_LDS_SAMPLES];
    __shared__ float s_w[MSDA_LDS_SAMPLES];
    const int K = g.s.K;
    const long long item0 = (long long)blockIdx.x * g.ipb;
    const long long left = g.items - item0;
    const int n_here = left < g.ipb ? (int)left : g.ipb;
    for (int i = threadIdx.x; i < n_here * K * 2; i += blockDim.x) s_off[i] = offset[item0 * K * 2 + i];
    for (int i = threadIdx.x; i < n_here * K; i += blockDim.x) s_w[i] = mask[item0 * K + i];
    __syncthreads();
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    const bool active = grp < n_here;                     // an idle group still takes part in the butterflies of its wave
    const long long item = active ? item0 + grp : item0;
    const DcItem at = dc_item(g.s, item);
    const size_t cell_stride = (size_t)g.s.G * g.Gc;
    const E* const vb = input + ((size_t)at.b * g.s.H * g.s.W * g.s.G + at.g) * g.Gc;
    MsVec<R> gr[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int run = t + it * g.T;
        if (active && run < g.nruns) {
            gr[it] = ms_load<E, R>(dout + (size_t)item * g.Gc + (size_t)run * R);
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) gr[it].v[j] = 0.f;
        }
    }
    for (int p = 0; p < K; ++p) {
        const int si = active ? grp * K + p : 0;
        const DcSample s = dc_sample(g.s, at.oy, at.ox, p, s_off[2 * si], s_off[2 * si + 1]);
        const float aw = s_w[si];
        float pw = 0.f, px = 0.f, py = 0.f;
        if (active && s.valid) {
#pragma unroll
            for (int it = 0; it < PASSES; ++it) {
                const int run = t + it * g.T;
                if (run >= g.nruns) continue;
                MsVec<R> v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (s.cell[k] >= 0) {
                        v[k] = ms_load<E, R>(vb + (size_t)s.cell[k] * cell_stride + (size_t)run * R);
                    } else {
#pragma unroll
                        for (int j = 0; j < R; ++j) v[k].v[j] = 0.f;
                    }
                }
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float val = ((s.w[0] * v[0].v[j] + s.w[1] * v[1].v[j]) + s.w[2] * v[2].v[j]) + s.w[3] * v[3].v[j];
                    // the slopes over the validly indexed corners (a corner that counts 0 enters as 0): the right-hand slope at an integer
                    const float gx = (s.hh * v[1].v[j] - s.hh * v[0].v[j]) + (s.lh * v[3].v[j] - s.lh * v[2].v[j]);
                    const float gy = (s.hw * v[2].v[j] - s.hw * v[0].v[j]) + (s.lw * v[3].v[j] - s.lw * v[1].v[j]);
                    const float ga = gr[it].v[j] * aw;
                    pw += gr[it].v[j] * val;
                    px += ga * gx;
                    py += ga * gy;
                }
            }
        }
        for (int off = g.T >> 1; off > 0; off >>= 1) {
            pw += __shfl_xor(pw, off);
            px += __shfl_xor(px, off);
            py += __shfl_xor(py, off);
        }
        if (active && t == 0) {
            const size_t o = (size_t)item * K + p;
            if (dmask) dmask[o] = pw;
            if (doffset) { doffset[2 * o] = g.s.scale * px; doffset[2 * o + 1] = g.s.scale * py; }
        }
    }
}

// ---- d_input: the plan -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MSDA_BLOCK)
void dcnv3_plan_kernel(const float* __restrict__ offset, const float* __restrict__ mask, long long total, DcGeom s, long long sentinel,
                       long long* __restrict__ keys, float* __restrict__ wts)
{
    const long long S = (long long)s.H * s.W;
    for (long long idx = (long long)blockIdx.x * MSDA_BLOCK + threadIdx.x; idx < total; idx += (long long)gridDim.x * MSDA_BLOCK) {
        const long long item = idx / s.K;
        const int p = (int)(idx - item * s.K);
        const DcItem at = dc_item(s, item);
        const DcSample c = dc_sample(s, at.oy, at.ox, p, offset[2 * idx], offset[2 * idx + 1]);
        const float aw = mask[idx];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            keys[4 * idx + k] = c.cell[k] >= 0 ? (at.b * S + c.cell[k]) * s.G + at.g : sentinel;
            wts[4 * idx + k] = c.cell[k] >= 0 ? c.w[k] * aw : 0.f;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// the arguments of one call, checked; false: FRCNN_EINVAL
static bool dcnv3_geom(int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                       float offset_scale, DcGeom& s)
{
    if (n_img < 1 || h < 1 || h > MSDA_MAX_SIDE || w < 1 || w > MSDA_MAX_SIDE || g < 1 || gc < 1 || gc > MSDA_MAX_CHANNELS) return false;
    if (kh < 1 || kh > DCNV3_MAX_KERNEL || kw < 1 || kw > DCNV3_MAX_KERNEL) return false;
    if (sh < 1 || sh > DCNV3_MAX_STEP || sw < 1 || sw > DCNV3_MAX_STEP || dh < 1 || dh > DCNV3_MAX_STEP || dw < 1 || dw > DCNV3_MAX_STEP)
        return false;
    if (ph < 0 || ph > DCNV3_MAX_STEP || pw < 0 || pw > DCNV3_MAX_STEP || !std::isfinite(offset_scale)) return false;
    const long long span_h = (long long)h + 2LL * ph - ((long long)dh * (kh - 1) + 1);
    const long long span_w = (long long)w + 2LL * pw - ((long long)dw * (kw - 1) + 1);
    if (span_h < 0 || span_w < 0) return false;                                               // no output pixel
    const long long ho = span_h / sh + 1, wo = span_w / sw + 1;
    if ((long long)n_img * h * w > MSDA_MAX_INDEX / g) return false;                          // cells: n H W G
    if ((long long)n_img * ho * wo > MSDA_MAX_INDEX / g / (4LL * kh * kw)) return false;      // plan entries: n Ho Wo G K 4
    s.H = h; s.W = w; s.Ho = (int)ho; s.Wo = (int)wo; s.G = g; s.K = kh * kw; s.kh = kh; s.sh = sh; s.sw = sw; s.ph = ph; s.pw = pw;
    s.dh = dh; s.dw = dw; s.bx = dw * (kw - 1) / 2; s.by = dh * (kh - 1) / 2; s.scale = offset_scale;
    return true;
}

static inline long long dcnv3_items(int n_img, const DcGeom& s) { return (long long)n_img * s.Ho * s.Wo * s.G; }

template <typename E>
static int dcnv3_forward_impl(const void* input, const float* offset, const float* mask, int n_img, int h, int w, int g, int gc, int kh,
                              int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale, void* out, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, s) || !input || !offset || !mask || !out)
        return FRCNN_EINVAL;
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = gc % RUN == 0 && aligned16(input) && aligned16(out);
    const MsMap mp = ms_map(gc, s.K, RUN, vector);
    const DcDims d = {dcnv3_items(n_img, s), s, gc, mp.T, mp.nruns, mp.ipb};
    const dim3 grid((unsigned)((d.items + mp.ipb - 1) / mp.ipb)), block(mp.threads);
    if (vector)
        hipLaunchKernelGGL((dcnv3_forward_kernel<E, RUN, 1>), grid, block, 0, (hipStream_t)stream, static_cast<const E*>(input), offset,
                           mask, d, static_cast<E*>(out));
    else
        hipLaunchKernelGGL((dcnv3_forward_kernel<E, 1, MSDA_SCALAR_PASSES>), grid, block, 0, (hipStream_t)stream,
                           static_cast<const E*>(input), offset, mask, d, static_cast<E*>(out));
    return check_launch();
}

template <typename E>
static int dcnv3_backward_offset_impl(const void* input, const float* offset, const float* mask, const void* dout, int n_img, int h, int w,
                                      int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale,
                                      float* doffset, float* dmask, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, s) || !input || !offset || !mask || !dout)
        return FRCNN_EINVAL;
    if (!doffset && !dmask) return FRCNN_EINVAL;
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = gc % RUN == 0 && aligned16(input) && aligned16(dout);
    const MsMap mp = ms_map(gc, s.K, RUN, vector);
    const DcDims d = {dcnv3_items(n_img, s), s, gc, mp.T, mp.nruns, mp.ipb};
    const dim3 grid((unsigned)((d.items + mp.ipb - 1) / mp.ipb)), block(mp.threads);
    if (vector)
        hipLaunchKernelGGL((dcnv3_backward_offset_kernel<E, RUN, 1>), grid, block, 0, (hipStream_t)stream, static_cast<const E*>(input),
                           offset, mask, static_cast<const E*>(dout), d, doffset, dmask);
    else
        hipLaunchKernelGGL((dcnv3_backward_offset_kernel<E, 1, MSDA_SCALAR_PASSES>), grid, block, 0, (hipStream_t)stream,
                           static_cast<const E*>(input), offset, mask, static_cast<const E*>(dout), d, doffset, dmask);
    return check_launch();
}

static int dcnv3_backward_input(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout,
                                int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                void* dinput, void* ws, size_t ws_bytes, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, 1.0f, s)) return FRCNN_EINVAL;
    return msda_gather(elem_type, sorted_keys, order, wts, dout, n_img * h * w * g, (int)(dcnv3_items(n_img, s) * s.K * 4), s.K * 4, gc,
                       dinput, ws, ws_bytes, (hipStream_t)stream);
}

}  // namespace frcnn

using namespace frcnn;

// a 16-bit entry point's body by element-type code
#define DCNV3_DISPATCH_16(elem_type, impl, ...)                                \
    do {                                                                       \
        if ((elem_type) == FRCNN_OPS_F16) return impl<ms_f16>(__VA_ARGS__);    \
        if ((elem_type) == FRCNN_OPS_BF16) return impl<ms_bf16>(__VA_ARGS__);  \
        return FRCNN_EINVAL;                                                   \
    } while (0)

extern "C" {

int frcnn_ops_dcnv3_max_kernel(void) { return DCNV3_MAX_KERNEL; }
int frcnn_ops_dcnv3_max_channels(void) { return MSDA_MAX_CHANNELS; }

int frcnn_ops_dcnv3_block_items(int gc, int kernel_h, int kernel_w, int elem_type)
{
    if (gc < 1 || gc > MSDA_MAX_CHANNELS || kernel_h < 1 || kernel_h > DCNV3_MAX_KERNEL || kernel_w < 1 || kernel_w > DCNV3_MAX_KERNEL)
        return 0;
    if (elem_type != 0 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return 0;
    const int run = elem_type == 0 ? MsElem<float>::RUN : MsElem<ms_f16>::RUN;
    return ms_map(gc, kernel_h * kernel_w, run, gc % run == 0).ipb;
}

size_t frcnn_ops_dcnv3_workspace_bytes(int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, 1.0f, s)) return 0;
    return msda_gather_workspace(n_img * h * w * g, (int)(dcnv3_items(n_img, s) * s.K * 4), gc);
}

int frcnn_ops_dcnv3_forward(const float* d_input, const float* d_offset, const float* d_mask, int n_img, int h, int w, int g, int gc,
                            int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                            float offset_scale, float* d_out, void* stream)
{
    return dcnv3_forward_impl<float>(d_input, d_offset, d_mask, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                     dil_h, dil_w, offset_scale, d_out, stream);
}

int frcnn_ops_dcnv3_backward_offset(const float* d_input, const float* d_offset, const float* d_mask, const float* d_dout, int n_img, int h,
                                    int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                    int dil_h, int dil_w, float offset_scale, float* d_doffset, float* d_dmask, void* stream)
{
    return dcnv3_backward_offset_impl<float>(d_input, d_offset, d_mask, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                                             pad_h, pad_w, dil_h, dil_w, offset_scale, d_doffset, d_dmask, stream);
}

int frcnn_ops_dcnv3_plan(const float* d_offset, const float* d_mask, int n_img, int h, int w, int g, int kernel_h, int kernel_w,
                         int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, int64_t* d_keys,
                         float* d_weights, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, 1, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, s) || !d_offset ||
        !d_mask || !d_keys || !d_weights)
        return FRCNN_EINVAL;
    const long long total = dcnv3_items(n_img, s) * s.K;
    hipLaunchKernelGGL(dcnv3_plan_kernel, dim3(msda_blocks(total)), dim3(MSDA_BLOCK), 0, (hipStream_t)stream, d_offset, d_mask, total, s,
                       (long long)n_img * h * w * g, reinterpret_cast<long long*>(d_keys), d_weights);
    return check_launch();
}

int frcnn_ops_dcnv3_backward_input(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                   int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dil_h, int dil_w, float* d_dinput, void* d_ws, size_t ws_bytes, void* stream)
{
    return dcnv3_backward_input(0, d_sorted_keys, d_order, d_weights, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                                pad_h, pad_w, dil_h, dil_w, d_dinput, d_ws, ws_bytes, stream);
}

int frcnn_ops_dcnv3_forward_16(int elem_type, const void* d_input, const float* d_offset, const float* d_mask, int n_img, int h, int w,
                               int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                               int dil_w, float offset_scale, void* d_out, void* stream)
{
    DCNV3_DISPATCH_16(elem_type, dcnv3_forward_impl, d_input, d_offset, d_mask, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                      pad_h, pad_w, dil_h, dil_w, offset_scale, d_out, stream);
}

int frcnn_ops_dcnv3_backward_offset_16(int elem_type, const void* d_input, const float* d_offset, const float* d_mask, const void* d_dout,
                                       int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, float* d_doffset, float* d_dmask,
                                       void* stream)
{
    DCNV3_DISPATCH_16(elem_type, dcnv3_backward_offset_impl, d_input, d_offset, d_mask, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w,
                      stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, d_doffset, d_dmask, stream);
}

int frcnn_ops_dcnv3_backward_input_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                      const void* d_dout, int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h,
                                      int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, void* d_dinput, void* d_ws, size_t ws_bytes,
                                      void* stream)
{
    if (elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    return dcnv3_backward_input(elem_type, d_sorted_keys, d_order, d_weights, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h,
                                stride_w, pad_h, pad_w, dil_h, dil_w, d_dinput, d_ws, ws_bytes, stream);
}

}  // extern "C"
