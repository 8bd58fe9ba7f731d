// ops_dcn.h -- the sampling kernels that DCNv3 (ops_dcnv3.hip) and DCNv4 (ops_dcnv4.hip) share: one sampling rule, one mapping, one
// forward, one offset / mask gradient and one plan kernel, each a template over WHERE a call's offsets and masks lie:
//   DcPlanar  DCNv3's two tensors, offset [n][Ho][Wo][G K 2] and mask [n][Ho][Wo][G K];
//   DcPacked  DCNv4's one tensor of records, offset_mask [n][Ho][Wo][L]: per group the 2 K offsets and then the K masks, the record padded
//             to L = ceil(3 G K / 8) 8 values.
// Here K is the number of points an item SAMPLES: kh kw, or kh kw - 1 when the centre point is removed (DcGeom::skip).
//
//   Channels-last tensors: input [n][H][W][G Gc], out [n][Ho][Wo][G Gc].  Point p of the kh kw grid is i kh + j with i in [0, kw) along x
//   (the outer index) and j in [0, kh) along y; with the centre removed the points after it move down by one.  With bx = dil_w (kw - 1) / 2
//   and by = dil_h (kh - 1) / 2 (integer division) the sample (b, oy, ox, g, p) lies at
//       x = (ox stride_w - pad_w + bx) + ((i dil_w - bx) + dx) * offset_scale,   y likewise with (oy, j, h, dy):
//   the integer parts in int, the rest in float32, in pixels of the unpadded map; there is no normalised location in between.  The sample
//   counts iff x > -1 && y > -1 && x < W && y < H (ops_deform.h: deform_sample, a NaN fails); its corners and weights are deform_corners'.
//   out[b][oy][ox][g Gc + c] = sum over p ascending of mask * (((w0 v0 + w1 v1) + w2 v2) + w3 v3), every product and sum in float32.
//
// Mapping (forward and the offset / mask gradient), that of ops_msda.hip with one level of K points: an item is one (b, oy, ox, g); a group
// of T lanes (a power of two <= 64) serves it, lanes along Gc, so a corner read is one contiguous run of input[b][cell][g][:]: R = 4 floats
// or 8 16-bit values per lane (16 B) when Gc holds whole runs and the tensors are 16-byte aligned, else the scalar body.  256 / T items
// share a block, fewer when their K samples would not fit MSDA_LDS_SAMPLES; the block's offsets and masks are staged once in LDS, 3 K words
// an item, by coalesced loads (the lanes of a group then read one word: a broadcast).
// Offset / mask gradient: per sample, a lane's partial sums over its channels, then an xor butterfly over the T lanes (a fixed order), one
// store per (b, oy, ox, g, p) by the group's lane 0.
// d_input: the plan writes one entry per sample and corner, e = (((b Q + q) G + g) K + p) 4 + corner with Q = Ho Wo, the key
// (b S + cell) G + g with S = H W, or the sentinel n S G for a corner that counts 0, and the weight corner weight * mask.  The caller sorts
// the keys stably and ops_msda.hip's gather (msda_gather: it uses an item's samples only as their number) sums each cell's entries in
// ascending e: no atomics, every cell written, no bit depends on how the images are chunked.
#pragma once
#include "ops_msda.h"
#include "ops_deform.h"

#include <climits>
#include <cmath>

namespace frcnn {

static constexpr int DCN_MAX_KERNEL = 7;
static constexpr int DCN_MAX_STEP = 1 << 16;             // stride, dilation and padding: the integer parts of a coordinate stay far inside int

static_assert(DCN_MAX_KERNEL * DCN_MAX_KERNEL <= MSDA_LDS_SAMPLES, "one item's samples fit the staging buffer");

// K: the points an item samples; skip: the grid point that is left out (INT_MAX: none)
struct DcGeom { int H, W, Ho, Wo, G, K, kh, sh, sw, ph, pw, dh, dw, bx, by, skip; float scale; };

// the tensors of one call as the sampling kernels see them
struct DcDims { long long items; DcGeom s; int Gc, T, nruns, ipb; };

// item ((b Q + q) G + g): its output pixel b Q + q, image, row, column and group
struct DcItem { long long pix, b; int oy, ox, g; };

__device__ __forceinline__ DcItem dc_item(const DcGeom& s, long long item)
{
    DcItem it;
    it.pix = item / s.G;
    it.g = (int)(item - it.pix * s.G);
    const long long row = it.pix / s.Wo;
    it.ox = (int)(it.pix - row * s.Wo);
    it.b = row / s.Ho;
    it.oy = (int)(row - it.b * s.Ho);
    return it;
}

// valid: the sample counts.  cell[k] >= 0: corner k lies inside the map (y W + x); w[k]: its bilinear weight; hh, lh, hw, lw: the fractions
struct DcSample { int cell[4]; float w[4]; float hh, lh, hw, lw; bool valid; };

__device__ __forceinline__ DcSample dc_sample(const DcGeom& s, int oy, int ox, int p, float dx, float dy)
{
    DcSample r;
    const int q = p + (p >= s.skip ? 1 : 0);             // the grid point of sample p
    const int i = q / s.kh, j = q - i * s.kh;
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

// ---- where the offsets and masks lie ---------------------------------------------------------------------------------------------------
// A layout stages a block's items in LDS (3 MSDA_LDS_SAMPLES words: 12 KB), says where item `grp` of the block finds its pairs (off_at:
// (dx, dy) of point p at + 2 p) and its masks (mask_at: + p), reads one sample for the plan, and stores the gradients.
static constexpr int DC_LDS_WORDS = 3 * MSDA_LDS_SAMPLES;

struct DcPlanar {
    const float* offset; const float* mask; float* doffset; float* dmask;   // the gradients: NULL outside the gradient kernel, either may be

    __device__ __forceinline__ void stage(float* s, long long item0, int n_here, const DcGeom& g) const
    {
        // the block's offsets and masks are one contiguous piece of each tensor
        for (int i = threadIdx.x; i < n_here * g.K * 2; i += blockDim.x) s[i] = offset[item0 * g.K * 2 + i];
        for (int i = threadIdx.x; i < n_here * g.K; i += blockDim.x) s[2 * MSDA_LDS_SAMPLES + i] = mask[item0 * g.K + i];
    }
    __device__ __forceinline__ static int off_at(int grp, int K) { return 2 * grp * K; }
    __device__ __forceinline__ static int mask_at(int grp, int K) { return 2 * MSDA_LDS_SAMPLES + grp * K; }
    __device__ __forceinline__ void fetch(const DcGeom& g, long long item, const DcItem&, int p, float& dx, float& dy, float& aw) const
    {
        const long long idx = item * g.K + p;
        dx = offset[2 * idx]; dy = offset[2 * idx + 1]; aw = mask[idx];
    }
    __device__ __forceinline__ void store(const DcGeom& g, long long item, const DcItem&, int p, float pw, float px, float py) const
    {
        const size_t o = (size_t)item * g.K + p;
        if (dmask) dmask[o] = pw;
        if (doffset) { doffset[2 * o] = px; doffset[2 * o + 1] = py; }
    }
    __device__ __forceinline__ void finish(const DcGeom&, const DcItem&, int, int) const {}
};

struct DcPacked {
    const float* om; float* dom; int L, vec;             // vec: om is 16-byte aligned (a record is a multiple of 32 bytes)

    // One word of the block's span: `rel` counts from the first word of the block's first pixel's record, inside record `pix_rel`
    // at place `r`.  Words of the pad, of the items before the block's first and after its last are dropped; the others land at
    // 3 K (item - item0) + place in the slice, so LDS holds the items' slices back to back whatever lies between them in memory.
    __device__ __forceinline__ static void place(float* s, int r, int pix_rel, int g0, int n_here, int slice, int G, float v)
    {
        if (r >= slice * G) return;
        const int gg = r / slice;
        const int local = pix_rel * G + gg - g0;
        if (local >= 0 && local < n_here) s[local * slice + (r - gg * slice)] = v;
    }
    __device__ __forceinline__ void stage(float* s, long long item0, int n_here, const DcGeom& g) const
    {
        const int slice = 3 * g.K;
        const long long pix0 = item0 / g.G;
        const int g0 = (int)(item0 - pix0 * g.G);
        const int last = g0 + n_here - 1;                                  // the block's last item, counted in groups from pix0's first
        // the span [first, end) in words from pix0's record: it ends inside the second record at the latest when G exceeds a block's
        // items, and records are short otherwise, so 32 unsigned bits hold it (3 G K < 2^31: dc_geom's bound on the plan)
        const unsigned ul = (unsigned)L, first = (unsigned)(g0 * slice), end = (unsigned)(last / g.G) * ul + (unsigned)((last % g.G + 1) * slice);
        const float* const base = om + pix0 * L;
        if (vec) {
            // 16-byte loads: L is a multiple of 8, so a run of 4 words from a multiple of 4 lies inside one record
            for (unsigned rel = (first & ~3u) + 4 * threadIdx.x; rel < end; rel += 4 * blockDim.x) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(base + rel);
                const unsigned pix_rel = rel / ul;
                const int r = (int)(rel - pix_rel * ul);
#pragma unroll
                for (int j = 0; j < 4; ++j) place(s, r + j, (int)pix_rel, g0, n_here, slice, g.G, t[j]);
            }
        } else {
            for (unsigned rel = first + threadIdx.x; rel < end; rel += blockDim.x) {
                const unsigned pix_rel = rel / ul;
                place(s, (int)(rel - pix_rel * ul), (int)pix_rel, g0, n_here, slice, g.G, base[rel]);
            }
        }
    }
    __device__ __forceinline__ static int off_at(int grp, int K) { return 3 * grp * K; }
    __device__ __forceinline__ static int mask_at(int grp, int K) { return 3 * grp * K + 2 * K; }
    __device__ __forceinline__ size_t slice_at(const DcGeom& g, const DcItem& at) const { return (size_t)at.pix * L + (size_t)at.g * 3 * g.K; }
    __device__ __forceinline__ void fetch(const DcGeom& g, long long, const DcItem& at, int p, float& dx, float& dy, float& aw) const
    {
        const float* const rec = om + slice_at(g, at);
        dx = rec[2 * p]; dy = rec[2 * p + 1]; aw = rec[2 * g.K + p];
    }
    __device__ __forceinline__ void store(const DcGeom& g, long long, const DcItem& at, int p, float pw, float px, float py) const
    {
        float* const rec = dom + slice_at(g, at);
        rec[2 * p] = px; rec[2 * p + 1] = py; rec[2 * g.K + p] = pw;
    }
    // the pad lanes of a record: zeros, by the lanes of the record's last group
    __device__ __forceinline__ void finish(const DcGeom& g, const DcItem& at, int t, int T) const
    {
        if (at.g != g.G - 1) return;
        for (int k = 3 * g.G * g.K + t; k < L; k += T) dom[(size_t)at.pix * L + k] = 0.f;
    }
};

// ---- forward -------------------------------------------------------------------------------------------------------------------------
template <typename E, int R, int PASSES, typename A>
__global__ __launch_bounds__(MSDA_BLOCK)
void dc_forward_kernel(const E* __restrict__ input, A a, DcDims g, E* __restrict__ out)
{
    __shared__ float s_rec[DC_LDS_WORDS];
    const int K = g.s.K;
    const long long item0 = (long long)blockIdx.x * g.ipb;
    const long long left = g.items - item0;
    const int n_here = left < g.ipb ? (int)left : g.ipb;
    a.stage(s_rec, item0, n_here, g.s);
    __syncthreads();
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    if (grp >= n_here) return;
    const long long item = item0 + grp;
    const DcItem at = dc_item(g.s, item);
    const size_t cell_stride = (size_t)g.s.G * g.Gc;
    const E* const vb = input + ((size_t)at.b * g.s.H * g.s.W * g.s.G + at.g) * g.Gc;
    const float* const s_off = s_rec + A::off_at(grp, K);
    const float* const s_w = s_rec + A::mask_at(grp, K);
    MsVec<R> acc[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[it].v[j] = 0.f;
    for (int p = 0; p < K; ++p) {
        const DcSample s = dc_sample(g.s, at.oy, at.ox, p, s_off[2 * p], s_off[2 * p + 1]);
        if (!s.valid) continue;
        const float aw = s_w[p];
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

// ---- the offset and mask gradients -------------------------------------------------------------------------------------------------------
template <typename E, int R, int PASSES, typename A>
__global__ __launch_bounds__(MSDA_BLOCK)
void dc_backward_offset_kernel(const E* __restrict__ input, const E* __restrict__ dout, A a, DcDims g)
{
    __shared__ float s_rec[DC_LDS_WORDS];
    const int K = g.s.K;
    const long long item0 = (long long)blockIdx.x * g.ipb;
    const long long left = g.items - item0;
    const int n_here = left < g.ipb ? (int)left : g.ipb;
    a.stage(s_rec, item0, n_here, g.s);
    __syncthreads();
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    const bool active = grp < n_here;                     // an idle group still takes part in the butterflies of its wave
    const long long item = active ? item0 + grp : item0;
    const DcItem at = dc_item(g.s, item);
    const size_t cell_stride = (size_t)g.s.G * g.Gc;
    const E* const vb = input + ((size_t)at.b * g.s.H * g.s.W * g.s.G + at.g) * g.Gc;
    const float* const s_off = s_rec + A::off_at(active ? grp : 0, K);
    const float* const s_w = s_rec + A::mask_at(active ? grp : 0, K);
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
        const DcSample s = dc_sample(g.s, at.oy, at.ox, p, s_off[2 * p], s_off[2 * p + 1]);
        const float aw = s_w[p];
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
        if (active && t == 0) a.store(g.s, item, at, p, pw, g.s.scale * px, g.s.scale * py);
    }
    if (active) a.finish(g.s, at, t, g.T);
}

// ---- d_input: the plan -----------------------------------------------------------------------------------------------------------------
template <typename A>
__global__ __launch_bounds__(MSDA_BLOCK)
void dc_plan_kernel(A a, long long total, DcGeom s, long long sentinel, long long* __restrict__ keys, float* __restrict__ wts)
{
    const long long S = (long long)s.H * s.W;
    for (long long idx = (long long)blockIdx.x * MSDA_BLOCK + threadIdx.x; idx < total; idx += (long long)gridDim.x * MSDA_BLOCK) {
        const long long item = idx / s.K;
        const int p = (int)(idx - item * s.K);
        const DcItem at = dc_item(s, item);
        float dx, dy, aw;
        a.fetch(s, item, at, p, dx, dy, aw);
        const DcSample c = dc_sample(s, at.oy, at.ox, p, dx, dy);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            keys[4 * idx + k] = c.cell[k] >= 0 ? (at.b * S + c.cell[k]) * s.G + at.g : sentinel;
            wts[4 * idx + k] = c.cell[k] >= 0 ? c.w[k] * aw : 0.f;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// the arguments of one call, checked; false: FRCNN_EINVAL.  remove_center (0 or 1, else false) leaves out the grid point
// (kw / 2, kh / 2) and needs kh == kw, odd, >= 3.
static inline bool dc_geom(int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                           float offset_scale, int remove_center, DcGeom& s)
{
    if (n_img < 1 || h < 1 || h > MSDA_MAX_SIDE || w < 1 || w > MSDA_MAX_SIDE || g < 1 || gc < 1 || gc > MSDA_MAX_CHANNELS) return false;
    if (kh < 1 || kh > DCN_MAX_KERNEL || kw < 1 || kw > DCN_MAX_KERNEL) return false;
    if (remove_center != 0 && (remove_center != 1 || kh != kw || kh % 2 == 0 || kh < 3)) return false;
    if (sh < 1 || sh > DCN_MAX_STEP || sw < 1 || sw > DCN_MAX_STEP || dh < 1 || dh > DCN_MAX_STEP || dw < 1 || dw > DCN_MAX_STEP)
        return false;
    if (ph < 0 || ph > DCN_MAX_STEP || pw < 0 || pw > DCN_MAX_STEP || !std::isfinite(offset_scale)) return false;
    const long long span_h = (long long)h + 2LL * ph - ((long long)dh * (kh - 1) + 1);
    const long long span_w = (long long)w + 2LL * pw - ((long long)dw * (kw - 1) + 1);
    if (span_h < 0 || span_w < 0) return false;                                               // no output pixel
    const long long ho = span_h / sh + 1, wo = span_w / sw + 1;
    const int k = kh * kw - remove_center;
    if ((long long)n_img * h * w > MSDA_MAX_INDEX / g) return false;                          // cells: n H W G
    if ((long long)n_img * ho * wo > MSDA_MAX_INDEX / g / (4LL * k)) return false;            // plan entries: n Ho Wo G K 4
    s.H = h; s.W = w; s.Ho = (int)ho; s.Wo = (int)wo; s.G = g; s.K = k; s.kh = kh; s.sh = sh; s.sw = sw; s.ph = ph; s.pw = pw;
    s.dh = dh; s.dw = dw; s.bx = dw * (kw - 1) / 2; s.by = dh * (kh - 1) / 2; s.scale = offset_scale;
    s.skip = remove_center ? (kw / 2) * kh + kh / 2 : INT_MAX;
    return true;
}

static inline long long dc_items(int n_img, const DcGeom& s) { return (long long)n_img * s.Ho * s.Wo * s.G; }

template <typename E, typename A>
static int dc_forward(const void* input, const A& a, int n_img, const DcGeom& s, int gc, void* out, void* stream)
{
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = gc % RUN == 0 && aligned16(input) && aligned16(out);
    const MsMap mp = ms_map(gc, s.K, RUN, vector);
    const DcDims d = {dc_items(n_img, s), s, gc, mp.T, mp.nruns, mp.ipb};
    const dim3 grid((unsigned)((d.items + mp.ipb - 1) / mp.ipb)), block(mp.threads);
    if (vector)
        hipLaunchKernelGGL((dc_forward_kernel<E, RUN, 1, A>), grid, block, 0, (hipStream_t)stream, static_cast<const E*>(input), a, d,
                           static_cast<E*>(out));
    else
        hipLaunchKernelGGL((dc_forward_kernel<E, 1, MSDA_SCALAR_PASSES, A>), grid, block, 0, (hipStream_t)stream,
                           static_cast<const E*>(input), a, d, static_cast<E*>(out));
    return check_launch();
}

template <typename E, typename A>
static int dc_backward_offset(const void* input, const void* dout, const A& a, int n_img, const DcGeom& s, int gc, void* stream)
{
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = gc % RUN == 0 && aligned16(input) && aligned16(dout);
    const MsMap mp = ms_map(gc, s.K, RUN, vector);
    const DcDims d = {dc_items(n_img, s), s, gc, mp.T, mp.nruns, mp.ipb};
    const dim3 grid((unsigned)((d.items + mp.ipb - 1) / mp.ipb)), block(mp.threads);
    if (vector)
        hipLaunchKernelGGL((dc_backward_offset_kernel<E, RUN, 1, A>), grid, block, 0, (hipStream_t)stream, static_cast<const E*>(input),
                           static_cast<const E*>(dout), a, d);
    else
        hipLaunchKernelGGL((dc_backward_offset_kernel<E, 1, MSDA_SCALAR_PASSES, A>), grid, block, 0, (hipStream_t)stream,
                           static_cast<const E*>(input), static_cast<const E*>(dout), a, d);
    return check_launch();
}

template <typename A>
static int dc_plan(const A& a, int n_img, int h, int w, const DcGeom& s, int64_t* keys, float* wts, void* stream)
{
    const long long total = dc_items(n_img, s) * s.K;
    hipLaunchKernelGGL(dc_plan_kernel<A>, dim3(msda_blocks(total)), dim3(MSDA_BLOCK), 0, (hipStream_t)stream, a, total, s,
                       (long long)n_img * h * w * s.G, reinterpret_cast<long long*>(keys), wts);
    return check_launch();
}

static inline int dc_backward_input(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout,
                                    int n_img, int h, int w, const DcGeom& s, int gc, void* dinput, void* ws, size_t ws_bytes, void* stream)
{
    return msda_gather(elem_type, sorted_keys, order, wts, dout, n_img * h * w * s.G, (int)(dc_items(n_img, s) * s.K * 4), s.K * 4, gc,
                       dinput, ws, ws_bytes, (hipStream_t)stream);
}

}  // namespace frcnn
