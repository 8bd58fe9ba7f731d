// ops_deform.hip -- deformable convolution v1 / v2 (torchvision.ops.deform_conv2d) in both directions: the frcnn_ops_deform_* entry
// points of include/frcnn_hip.h.  Restated from the published algorithm of torchvision's deform_conv2d_kernel.cu (third party, absent
// here: restated, unpinned, like the other operators of fasterrcnn_amd.ops).
//
// The operator is three sampling kernels around three dense products, and the products are gemm_tn.hip's exact-float32 MFMA kernel
// (C[m][n] = sum_r A[r][m] B[r][n]).  Every entry point works on one chunk of n_img images; the caller walks the chunks.
//
// Layouts: plain NCHW.  With P = oh ow outputs per image, Pp = P rounded up to 4 and ld = n_img Pp, the column matrix is
//   col[(c, i, j)][b Pp + p]     rows (c kh + i) kw + j over ALL input channels, row stride ld, the columns p >= P of an image zero
// so that the rows of weight group w are the contiguous block [w K, (w + 1) K), K = (C_in / groups) kh kw, and every leading dimension
// is a multiple of 4 floats whatever P is.
//
// Forward:   col = mask * bilinear sample (one thread per element, p fastest: coalesced stores);  per weight group
//            tmp[co][b Pp + p] = sum_k Wt[k][co] col[k][b Pp + p]  (Wt: the group's weights transposed by train.hip's transpose);
//            out[b][co][p] = tmp + bias strips the padding.  The product runs WITHOUT a split reduction: every output element is one
//            sequential dot product over k inside one block, so the result does not depend on how the images are chunked.
// Backward:  dcol = W^T dout per group (weights padded to a row stride of 4, dout packed to [co][b Pp + p]; again no split).
//   offset / mask: a gather -- one thread per (b, g, tap, p) sums over the channels of offset group g
//            (mask * coordinate_weight) * dcol for y and x, and dcol * sample for the mask.
//   input:   deterministic and without atomics.  Which samples reach a cell depends on the offsets, so a plan is built first: one
//            entry per sample and corner, e = ((((b G + g) kk + tap) P + p) 4 + corner, with the key ((b G + g) H + y) W + x of the
//            cell the corner lands on -- or the sentinel n_img G H W for a corner outside the map or a rejected sample -- and the
//            weight corner weight * mask.  The caller sorts the keys stably (torch.sort: plumbing); a binary search per cell finds
//            the segment starts; then one thread per (b, c, y, x) sums its cell's entries in ascending e:
//            (corner weight * mask) * dcol[(c, tap)][b Pp + p].  The plan is shared by the C_in / G channels of the group; every
//            cell is written, zeros included (no zero fill), and the result is bit-identical from run to run and from chunking to
//            chunking (a cell's entries all belong to its own image).
//   weight:  dW[co][k] = sum over (b, p) of dout^T[(b, p)][co] col^T[(b, p)][k] per group: the columns are sampled again, both
//            operands transposed to reduction-major form, deterministic split reduction through the workspace; chunks are added in
//            ascending order by the caller's accumulate flag.
//
// float16 / bfloat16 (the frcnn_ops_deform_*_16 entry points): the same kernels, templates over the storage type E of the tensors
// (ops_elem.h widens on load, rounds once on store; dcol and the plan's weights stay float32), around gemm_nt16.hip's product of
// 16-bit operands; see "the 16-bit operator" below for the operand layouts and include/frcnn_hip.h for the arithmetic contract.
#include "ops_deform.h"

namespace frcnn {

static constexpr int DF_BLOCK = 256;
static constexpr int DF_MAX_BLOCKS = 16384;                   // grid-stride beyond

// the geometry as the kernels use it
struct DeformGeom {
    int C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, G;
    int oh, ow, P, Pp, kk, cpo;                                // cpo: channels per offset group
};

static inline int round4(int v) { return (v + 3) & ~3; }
static inline int round8(int v) { return (v + 7) & ~7; }

// validates the public geometry and the sizes the 32-bit indices of the kernels and of the products can hold; fills the kernel form.
// pad: what P is rounded up to in the column rows (4 floats for gemm_tn, 8 elements for the 16-bit product)
static bool deform_geom(const frcnn_deform_geom* g, int n_img, DeformGeom& d, int& c_out, int& groups, int pad = 4)
{
    if (!g || n_img < 1) return false;
    if (g->c_in < 1 || g->c_out < 1 || g->height < 1 || g->width < 1 || g->kernel_h < 1 || g->kernel_w < 1) return false;
    if (g->stride_h < 1 || g->stride_w < 1 || g->pad_h < 0 || g->pad_w < 0 || g->dilation_h < 1 || g->dilation_w < 1) return false;
    if (g->groups < 1 || g->offset_groups < 1 || g->c_in % g->groups || g->c_out % g->groups || g->c_in % g->offset_groups) return false;
    const long long lim = INT32_MAX - 4 * DF_BLOCK;
    const long long eh = (long long)g->dilation_h * (g->kernel_h - 1) + 1, ew = (long long)g->dilation_w * (g->kernel_w - 1) + 1;
    const long long oh = ((long long)g->height + 2LL * g->pad_h - eh) / g->stride_h + 1;
    const long long ow = ((long long)g->width + 2LL * g->pad_w - ew) / g->stride_w + 1;
    if ((long long)g->height + 2LL * g->pad_h < eh || (long long)g->width + 2LL * g->pad_w < ew || oh < 1 || ow < 1) return false;
    const long long kk = (long long)g->kernel_h * g->kernel_w, P = oh * ow;
    if (kk > lim || P > lim || (long long)g->height * g->width > lim) return false;
    if ((long long)g->height + g->pad_h + eh > lim || (long long)g->width + g->pad_w + ew > lim) return false;   // o stride - pad + i dil
    const long long Pp = (P + pad - 1) / pad * pad;
    if (n_img * Pp > lim || g->c_in * kk + (pad == 8 ? 8LL * g->groups : 0) > lim || (long long)n_img * g->offset_groups * g->height * g->width > lim) return false;
    if ((long long)n_img * g->offset_groups * kk > lim / 4 / P) return false;                                    // plan entries
    d.C = g->c_in; d.H = g->height; d.W = g->width; d.kh = g->kernel_h; d.kw = g->kernel_w; d.sh = g->stride_h; d.sw = g->stride_w;
    d.ph = g->pad_h; d.pw = g->pad_w; d.dh = g->dilation_h; d.dw = g->dilation_w; d.G = g->offset_groups;
    d.oh = (int)oh; d.ow = (int)ow; d.P = (int)P; d.Pp = (int)Pp; d.kk = (int)kk; d.cpo = g->c_in / g->offset_groups;
    c_out = g->c_out; groups = g->groups;
    return true;
}

static inline unsigned df_blocks(size_t total)
{
    const size_t b = (total + DF_BLOCK - 1) / DF_BLOCK;
    return (unsigned)(b < (size_t)DF_MAX_BLOCKS ? (b ? b : 1) : (size_t)DF_MAX_BLOCKS);
}

// offset and mask of sample t = (b G + g) kk + tap at output p
template <typename E>
__device__ __forceinline__ void deform_read(const DeformGeom& g, const E* __restrict__ offset, const E* __restrict__ mask,
                                            size_t t, int p, int tap, float& y, float& x, float& m)
{
    const int i = tap / g.kw, j = tap - i * g.kw, oy = p / g.ow, ox = p - oy * g.ow;
    y = deform_coord(oy, g.sh, g.ph, i, g.dh, Elem<E>::load(offset, (2 * t) * g.P + p));
    x = deform_coord(ox, g.sw, g.pw, j, g.dw, Elem<E>::load(offset, (2 * t + 1) * g.P + p));
    m = mask ? Elem<E>::load(mask, t * g.P + p) : 1.0f;
}

// the column value of input channel c, tap `tap`, image b of the chunk, output p: mask * bilinear sample, in float32
template <typename E>
__device__ __forceinline__ float deform_column(const DeformGeom& g, const E* __restrict__ x, const E* __restrict__ offset,
                                               const E* __restrict__ mask, int b, int c, int tap, int p)
{
    const size_t t = ((size_t)b * g.G + c / g.cpo) * g.kk + tap;
    float sy, sx, m;
    deform_read(g, offset, mask, t, p, tap, sy, sx, m);
    return m * deform_bilinear(x + ((size_t)b * g.C + c) * g.H * g.W, g.H, g.W, sy, sx);
}

// ---- deformable im2col -----------------------------------------------------------------------------------------------------------
// col[(c, tap)][b Pp + p], rounded once to E on the store (float: as it is)
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_columns_kernel(const E* __restrict__ x, const E* __restrict__ offset, const E* __restrict__ mask, DeformGeom g,
                           int n_img, size_t total, E* __restrict__ col)
{
    const size_t ld = (size_t)n_img * g.Pp;
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int row = (int)(idx / ld), cn = (int)(idx - (size_t)row * ld);
        const int b = cn / g.Pp, p = cn - b * g.Pp;
        float v = 0.f;
        if (p < g.P) {
            const int c = row / g.kk;
            v = deform_column(g, x, offset, mask, b, c, row - c * g.kk, p);
        }
        deform_store(col, idx, v);
    }
}

// The same values in the forward product's layout (16-bit E only): col[b P + p][w Kp + kl], kl = (c - w cg) kk + tap the index inside
// weight group w (cg = C / groups channels, K = cg kk, Kp = K rounded up to 8, the pad kl >= K written as zeros).  A thread owns eight
// consecutive kl of one output, one 16-byte store; a wave owns 64 consecutive outputs (the offset and mask reads coalesce as in the
// kernel above) and the waves that follow it take the next kl of the same outputs, so a row's cache lines fill while they are hot.
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_columns_nk_kernel(const E* __restrict__ x, const E* __restrict__ offset, const E* __restrict__ mask, DeformGeom g, int n_img,
                              int cg, int Kp, int groups, size_t total, E* __restrict__ col)
{
    static_assert(sizeof(E) == 2, "eight elements are one 16-byte store");
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int K = cg * g.kk, runs = groups * (Kp / 8), N = n_img * g.P;
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const size_t q = idx >> 6;
        const int run = (int)(q % runs), n = (int)(q / runs) * 64 + (int)(idx & 63);
        if (n >= N) continue;
        const int b = n / g.P, p = n - b * g.P, w = run / (Kp / 8), kl0 = (run - w * (Kp / 8)) * 8;
        union { E e[8]; u32x4 v; } r;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kl = kl0 + j;
            float v = 0.f;
            if (kl < K) {
                const int cl = kl / g.kk;
                v = deform_column(g, x, offset, mask, b, w * cg + cl, kl - cl * g.kk, p);
            }
            round_to(v, r.e[j]);
        }
        *reinterpret_cast<u32x4*>(col + (size_t)n * groups * Kp + (size_t)run * 8) = r.v;
    }
}

// ---- layout glue -----------------------------------------------------------------------------------------------------------------
// out[b][co][p] = tmp[co][b Pp + p] (+ bias[co])
__global__ __launch_bounds__(DF_BLOCK)
void deform_output_kernel(const float* __restrict__ tmp, const float* __restrict__ bias, int n_img, int c_out, int P, int Pp, size_t total,
                          float* __restrict__ out)
{
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int p = (int)(idx % P);
        const size_t bc = idx / P;
        const int co = (int)(bc % c_out), b = (int)(bc / c_out);
        const float v = tmp[((size_t)co * n_img + b) * Pp + p];
        out[idx] = bias ? v + bias[co] : v;
    }
}

// gt[co][b Pp + p] = dout[b][co][p], zero for p >= P
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_pack_grad_kernel(const E* __restrict__ dout, int n_img, int c_out, int P, int Pp, size_t total, E* __restrict__ gt)
{
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int p = (int)(idx % Pp);
        const size_t cb = idx / Pp;
        const int b = (int)(cb % n_img), co = (int)(cb / n_img);
        gt[idx] = p < P ? dout[((size_t)b * c_out + co) * P + p] : E{};
    }
}

// gT[b Pp + p][w cogp + col] = dout[b][w cog + col][p], zero for p >= P and for col >= cog (cogp: cog rounded up to 8)
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_pack_grad_t_kernel(const E* __restrict__ dout, int c_out, int cog, int cogp, int groups, int P, int Pp, size_t total,
                               E* __restrict__ gT)
{
    const int ld = groups * cogp;
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int j = (int)(idx % ld), w = j / cogp, col = j - w * cogp;
        const size_t n = idx / ld;
        const int p = (int)(n % Pp);
        const size_t b = n / Pp;
        gT[idx] = p < P && col < cog ? dout[(b * c_out + w * cog + col) * P + p] : E{};
    }
}

// wt[w][k][col] (row stride cogp) = weight[w cog + col][k], zero for col >= cog
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_pack_weight_t_kernel(const E* __restrict__ weight, int cog, int cogp, int K, size_t total, E* __restrict__ wt)
{
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int col = (int)(idx % cogp);
        const size_t wk = idx / cogp;
        const int k = (int)(wk % K);
        const size_t w = wk / K;
        wt[idx] = col < cog ? weight[(w * cog + col) * K + k] : E{};
    }
}

// dst[r][c] (row stride ldd, c < ldd) = src[r][c] for c < cols, else zero
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_pad_rows_kernel(const E* __restrict__ src, int cols, E* __restrict__ dst, int ldd, size_t total)
{
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int c = (int)(idx % ldd);
        const size_t r = idx / ldd;
        dst[idx] = c < cols ? src[r * cols + c] : E{};
    }
}

// dst[r][c] (dense, cols wide) = (accumulate ? dst[r][c] : 0) + src[r][c] (row stride lds)
__global__ __launch_bounds__(DF_BLOCK)
void deform_add_rows_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int cols, int accumulate, size_t total)
{
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int c = (int)(idx % cols);
        const size_t r = idx / cols;
        const float v = src[r * lds + c];
        dst[idx] = accumulate ? dst[idx] + v : v;
    }
}

// ---- offset and mask gradient ------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_offset_grad_kernel(const E* __restrict__ x, const E* __restrict__ offset, const E* __restrict__ mask,
                               const float* __restrict__ dcol, DeformGeom g, int n_img, size_t total, E* __restrict__ doffset,
                               E* __restrict__ dmask)
{
    const size_t ld = (size_t)n_img * g.Pp;
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int p = (int)(idx % g.P);
        const size_t t = idx / g.P;                             // (b G + og) kk + tap
        const int tap = (int)(t % g.kk);
        const size_t bg = t / g.kk;
        const int og = (int)(bg % g.G), b = (int)(bg / g.G);
        float sy, sx, m;
        deform_read(g, offset, mask, t, p, tap, sy, sx, m);
        float gy = 0.f, gx = 0.f, gm = 0.f;
        for (int cc = 0; cc < g.cpo; ++cc) {
            const int c = og * g.cpo + cc;
            const E* plane = x + ((size_t)b * g.C + c) * g.H * g.W;
            const float dc = dcol[((size_t)c * g.kk + tap) * ld + (size_t)b * g.Pp + p];
            if (doffset) {
                gy += (m * deform_coordinate_weight(plane, g.H, g.W, sy, sx, true)) * dc;
                gx += (m * deform_coordinate_weight(plane, g.H, g.W, sy, sx, false)) * dc;
            }
            if (dmask) gm += dc * deform_bilinear(plane, g.H, g.W, sy, sx);
        }
        if (doffset) { deform_store(doffset, (2 * t) * g.P + p, gy); deform_store(doffset, (2 * t + 1) * g.P + p, gx); }
        if (dmask) deform_store(dmask, idx, gm);
    }
}

// ---- input gradient: plan, segment starts, gather ------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_plan_kernel(const E* __restrict__ offset, const E* __restrict__ mask, DeformGeom g, int n_img, size_t total,
                        long long* __restrict__ keys, float* __restrict__ wts)
{
    const long long cells = (long long)g.H * g.W, sentinel = (long long)n_img * g.G * cells;
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int p = (int)(idx % g.P);
        const size_t t = idx / g.P;
        const int tap = (int)(t % g.kk);
        const long long bg = (long long)(t / g.kk);             // b G + og
        float sy, sx, m;
        deform_read(g, offset, mask, t, p, tap, sy, sx, m);
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        int cell[4] = {-1, -1, -1, -1};
        DeformSample s;
        if (deform_sample(sy, sx, g.H, g.W, s)) deform_corners(s, g.H, g.W, w, cell);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            keys[4 * idx + k] = cell[k] >= 0 ? bg * cells + cell[k] : sentinel;
            wts[4 * idx + k] = w[k] * m;
        }
    }
}

// start[q] = the first position of the sorted keys that holds a key >= q, for q in [0, n_cells]
__global__ __launch_bounds__(DF_BLOCK)
void deform_segments_kernel(const long long* __restrict__ sorted_keys, int n_entries, int n_cells, int* __restrict__ start)
{
    for (long long q = (long long)blockIdx.x * DF_BLOCK + threadIdx.x; q <= n_cells; q += (long long)gridDim.x * DF_BLOCK) {
        int lo = 0, hi = n_entries;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (sorted_keys[mid] < q) lo = mid + 1; else hi = mid;
        }
        start[q] = lo;
    }
}

template <typename E>
__global__ __launch_bounds__(DF_BLOCK)
void deform_input_grad_kernel(const int* __restrict__ start, const long long* __restrict__ order, const float* __restrict__ wts,
                              const float* __restrict__ dcol, DeformGeom g, int n_img, size_t total, E* __restrict__ dx)
{
    const size_t ld = (size_t)n_img * g.Pp;
    const int cells = g.H * g.W;
    for (size_t idx = (size_t)blockIdx.x * DF_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * DF_BLOCK) {
        const int cell = (int)(idx % cells);
        const size_t bc = idx / cells;
        const int c = (int)(bc % g.C), b = (int)(bc / g.C);
        const int q = (b * g.G + c / g.cpo) * cells + cell;
        const int s1 = start[q + 1];
        const float* const rows = dcol + (size_t)c * g.kk * ld + (size_t)b * g.Pp;
        float acc = 0.f;
        for (int i = start[q]; i < s1; ++i) {
            const long long e = order[i];
            const long long smp = e >> 2;                        // ((b G + og) kk + tap) P + p
            const int p = (int)(smp % g.P), tap = (int)((smp / g.P) % g.kk);
            acc += wts[e] * rows[(size_t)tap * ld + p];
        }
        deform_store(dx, idx, acc);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct DeformSizes { int K, Kp, cog, cogp, ld; size_t col, gt, wt, wp, gtT, colT, tmpw, gemm; };

static DeformSizes deform_sizes(const DeformGeom& d, int c_out, int groups, int n_img)
{
    DeformSizes z;
    z.K = d.C / groups * d.kk; z.Kp = round4(z.K); z.cog = c_out / groups; z.cogp = round4(z.cog); z.ld = n_img * d.Pp;
    z.col = align256((size_t)d.C * d.kk * z.ld * sizeof(float));
    z.gt = align256((size_t)c_out * z.ld * sizeof(float));
    z.wt = align256((size_t)z.K * z.cogp * sizeof(float));
    z.wp = align256((size_t)c_out * z.Kp * sizeof(float));
    z.gtT = align256((size_t)z.ld * z.cogp * sizeof(float));
    z.colT = align256((size_t)z.ld * z.Kp * sizeof(float));
    z.tmpw = align256((size_t)z.cog * z.Kp * sizeof(float));
    z.gemm = align256(gemm_tn_workspace_bytes(z.cog, z.K, z.ld, 1));
    return z;
}

static size_t deform_input_workspace(const DeformGeom& d, int n_img)
{
    return align256(((size_t)n_img * d.G * d.H * d.W + 1) * sizeof(int));
}

static size_t deform_workspace(const DeformGeom& d, const DeformSizes& z, int n_img, int stage)
{
    switch (stage) {
    case FRCNN_DEFORM_WS_FORWARD: return z.col + z.gt + z.wt;
    case FRCNN_DEFORM_WS_BACKWARD_COLUMNS: return z.wp + z.gt;
    case FRCNN_DEFORM_WS_BACKWARD_INPUT: return deform_input_workspace(d, n_img);
    case FRCNN_DEFORM_WS_BACKWARD_WEIGHT: return z.col + z.gt + z.gtT + z.colT + z.tmpw + z.gemm;
    case FRCNN_DEFORM_WS_COLUMNS: return (size_t)d.C * d.kk * z.ld * sizeof(float);
    default: return 0;
    }
}

template <typename E>
static int deform_launch_columns(const DeformGeom& d, int n_img, const E* x, const E* offset, const E* mask, E* col, hipStream_t s)
{
    const size_t total = (size_t)d.C * d.kk * n_img * d.Pp;
    hipLaunchKernelGGL(deform_columns_kernel<E>, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, s, x, offset, mask, d, n_img, total, col);
    return check_launch();
}

template <typename E>
static int deform_launch_pack_grad(int n_img, int c_out, const DeformGeom& d, const E* dout, E* gt, hipStream_t s)
{
    const size_t total = (size_t)c_out * n_img * d.Pp;
    hipLaunchKernelGGL(deform_pack_grad_kernel<E>, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, s, dout, n_img, c_out, d.P, d.Pp, total, gt);
    return check_launch();
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define DF_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)

// ---- the gathers' entry points, for every element type (pad: deform_geom's) ---------------------------------------------------------
template <typename E>
static int deform_backward_offset_impl(const frcnn_deform_geom* g, int n_img, int pad, const E* d_x, const E* d_offset, const E* d_mask,
                                       const float* d_dcol, E* d_doffset, E* d_dmask, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups, pad)) return FRCNN_EINVAL;
    if (!d_x || !d_offset || !d_dcol || (!d_doffset && !d_dmask)) return FRCNN_EINVAL;
    const size_t total = (size_t)n_img * d.G * d.kk * d.P;
    hipLaunchKernelGGL(deform_offset_grad_kernel<E>, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, (hipStream_t)stream, d_x, d_offset, d_mask,
                       d_dcol, d, n_img, total, d_doffset, d_dmask);
    return check_launch();
}

template <typename E>
static int deform_input_plan_impl(const frcnn_deform_geom* g, int n_img, int pad, const E* d_offset, const E* d_mask, int64_t* d_keys,
                                  float* d_weights, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups, pad)) return FRCNN_EINVAL;
    if (!d_offset || !d_keys || !d_weights) return FRCNN_EINVAL;
    const size_t total = (size_t)n_img * d.G * d.kk * d.P;
    hipLaunchKernelGGL(deform_plan_kernel<E>, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, (hipStream_t)stream, d_offset, d_mask, d, n_img,
                       total, reinterpret_cast<long long*>(d_keys), d_weights);
    return check_launch();
}

template <typename E>
static int deform_backward_input_impl(const frcnn_deform_geom* g, int n_img, int pad, const int64_t* d_sorted_keys, const int64_t* d_order,
                                      const float* d_weights, const float* d_dcol, E* d_dx, void* d_ws, size_t ws_bytes, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups, pad)) return FRCNN_EINVAL;
    if (!d_sorted_keys || !d_order || !d_weights || !d_dcol || !d_dx || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform_input_workspace(d, n_img)) return FRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int* start = static_cast<int*>(d_ws);
    const int n_cells = n_img * d.G * d.H * d.W, n_entries = n_img * d.G * d.kk * d.P * 4;
    hipLaunchKernelGGL(deform_segments_kernel, dim3(df_blocks((size_t)n_cells + 1)), dim3(DF_BLOCK), 0, s,
                       reinterpret_cast<const long long*>(d_sorted_keys), n_entries, n_cells, start);
    DF_TRY(check_launch());
    const size_t total = (size_t)n_img * d.C * d.H * d.W;
    hipLaunchKernelGGL(deform_input_grad_kernel<E>, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, s, start,
                       reinterpret_cast<const long long*>(d_order), d_weights, d_dcol, d, n_img, total, d_dx);
    return check_launch();
}

// ---- the 16-bit operator (frcnn_ops_deform_*_16): the same sampling kernels on 16-bit tensors around gemm_nt16.hip's product ----------
// Every operand of that product is reduction-contiguous with a row stride that is a multiple of 8 elements and zeros in the pad:
//   forward   out[co][n]  = sum_k  wp[co][k] colNK[n][k]        wp: the weights with rows padded to Kp; colNK: deform_columns_nk_kernel
//   dcol      dcol[k][n]  = sum_co wt[k][co] gT[n][co]          wt, gT: deform_pack_weight_t_kernel, deform_pack_grad_t_kernel
//   d_weight  dW[co][k]   = sum_n  gt[co][n] col[k][n]          gt: deform_pack_grad_kernel; col: deform_columns_kernel, Pp = P up to 8
struct Deform16Sizes { int K, Kp, cog, cogp, ld, N; size_t colnk, wp, wt, gT, col, gt, part; };

static Deform16Sizes deform16_sizes(const DeformGeom& d, int c_out, int groups, int n_img)
{
    Deform16Sizes z;
    z.K = d.C / groups * d.kk; z.Kp = round8(z.K); z.cog = c_out / groups; z.cogp = round8(z.cog); z.ld = n_img * d.Pp; z.N = n_img * d.P;
    z.colnk = align256((size_t)z.N * groups * z.Kp * 2);
    z.wp = align256((size_t)c_out * z.Kp * 2);
    z.wt = align256((size_t)groups * z.K * z.cogp * 2);
    z.gT = align256((size_t)z.ld * groups * z.cogp * 2);
    z.col = align256((size_t)d.C * d.kk * z.ld * 2);
    z.gt = align256((size_t)c_out * z.ld * 2);
    z.part = align256(gemm_nt16_workspace_bytes(z.cog, z.K, z.ld));
    return z;
}

static size_t deform16_workspace(const DeformGeom& d, const Deform16Sizes& z, int n_img, int stage)
{
    switch (stage) {
    case FRCNN_DEFORM_WS_FORWARD: return z.colnk + z.wp;
    case FRCNN_DEFORM_WS_BACKWARD_COLUMNS: return z.wt + z.gT;
    case FRCNN_DEFORM_WS_BACKWARD_INPUT: return deform_input_workspace(d, n_img);
    case FRCNN_DEFORM_WS_BACKWARD_WEIGHT: return z.col + z.gt + z.part;
    case FRCNN_DEFORM_WS_COLUMNS: return (size_t)d.C * d.kk * z.ld * sizeof(float);
    default: return 0;
    }
}

template <typename E>
static int deform16_forward(int elem_type, const DeformGeom& d, const Deform16Sizes& z, int c_out, int groups, int n_img, const E* x,
                            const E* offset, const E* mask, const E* weight, const E* bias, E* out, char* ws, hipStream_t s)
{
    E* col = reinterpret_cast<E*>(ws);
    E* wp = reinterpret_cast<E*>(ws + z.colnk);
    const size_t total = (size_t)cdiv(z.N, 64) * 64 * groups * (z.Kp / 8);
    hipLaunchKernelGGL(deform_columns_nk_kernel<E>, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, s, x, offset, mask, d, n_img, d.C / groups,
                       z.Kp, groups, total, col);
    DF_TRY(check_launch());
    const size_t wtotal = (size_t)c_out * z.Kp;
    hipLaunchKernelGGL(deform_pad_rows_kernel<E>, dim3(df_blocks(wtotal)), dim3(DF_BLOCK), 0, s, weight, z.K, wp, z.Kp, wtotal);
    DF_TRY(check_launch());
    for (int w = 0; w < groups; ++w)
        DF_TRY(launch_gemm_nt16_nchw(elem_type, wp + (size_t)w * z.cog * z.Kp, z.Kp, col + (size_t)w * z.Kp, groups * z.Kp, z.cog, z.N,
                                     z.Kp, bias, out, d.P, c_out, w * z.cog, s));
    return FRCNN_OK;
}

template <typename E>
static int deform16_backward_columns(int elem_type, const DeformGeom& d, const Deform16Sizes& z, int c_out, int groups, int n_img,
                                     const E* weight, const E* dout, float* dcol, char* ws, hipStream_t s)
{
    E* wt = reinterpret_cast<E*>(ws);
    E* gT = reinterpret_cast<E*>(ws + z.wt);
    const size_t wtotal = (size_t)groups * z.K * z.cogp;
    hipLaunchKernelGGL(deform_pack_weight_t_kernel<E>, dim3(df_blocks(wtotal)), dim3(DF_BLOCK), 0, s, weight, z.cog, z.cogp, z.K, wtotal, wt);
    DF_TRY(check_launch());
    const size_t gtotal = (size_t)z.ld * groups * z.cogp;
    hipLaunchKernelGGL(deform_pack_grad_t_kernel<E>, dim3(df_blocks(gtotal)), dim3(DF_BLOCK), 0, s, dout, c_out, z.cog, z.cogp, groups, d.P,
                       d.Pp, gtotal, gT);
    DF_TRY(check_launch());
    for (int w = 0; w < groups; ++w)
        DF_TRY(launch_gemm_nt16(elem_type, wt + (size_t)w * z.K * z.cogp, z.cogp, gT + (size_t)w * z.cogp, groups * z.cogp,
                                dcol + (size_t)w * z.K * z.ld, z.ld, z.K, z.ld, z.cogp, s));
    return FRCNN_OK;
}

template <typename E>
static int deform16_backward_weight(int elem_type, const DeformGeom& d, const Deform16Sizes& z, int c_out, int groups, int n_img, const E* x,
                                    const E* offset, const E* mask, const E* dout, float* dweight, int accumulate, char* ws, hipStream_t s)
{
    E* col = reinterpret_cast<E*>(ws);
    E* gt = reinterpret_cast<E*>(ws + z.col);
    void* part = ws + z.col + z.gt;
    DF_TRY(deform_launch_columns(d, n_img, x, offset, mask, col, s));
    DF_TRY(deform_launch_pack_grad(n_img, c_out, d, dout, gt, s));
    for (int w = 0; w < groups; ++w)
        DF_TRY(launch_gemm_nt16_split(elem_type, gt + (size_t)w * z.cog * z.ld, z.ld, col + (size_t)w * z.K * z.ld, z.ld,
                                      dweight + (size_t)w * z.cog * z.K, z.K, z.cog, z.K, z.ld, accumulate, part, z.part, s));
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

size_t frcnn_ops_deform_workspace_bytes(const frcnn_deform_geom* g, int n_img, int stage)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups)) return 0;
    return deform_workspace(d, deform_sizes(d, c_out, groups, n_img), n_img, stage);
}

int frcnn_ops_deform_forward(const frcnn_deform_geom* g, int n_img, const float* d_x, const float* d_offset, const float* d_mask,
                             const float* d_weight, const float* d_bias, float* d_out, void* d_ws, size_t ws_bytes, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups)) return FRCNN_EINVAL;
    const DeformSizes z = deform_sizes(d, c_out, groups, n_img);
    if (!d_x || !d_offset || !d_weight || !d_out || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform_workspace(d, z, n_img, FRCNN_DEFORM_WS_FORWARD)) return FRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(d_ws);
    float* col = reinterpret_cast<float*>(ws);
    float* tmp = reinterpret_cast<float*>(ws + z.col);
    float* wt = reinterpret_cast<float*>(ws + z.col + z.gt);
    DF_TRY(deform_launch_columns(d, n_img, d_x, d_offset, d_mask, col, s));
    for (int w = 0; w < groups; ++w) {
        DF_TRY(launch_transpose(d_weight + (size_t)w * z.cog * z.K, z.K, wt, z.cogp, z.cog, z.K, s));
        DF_TRY(launch_gemm_tn(wt, z.cogp, col + (size_t)w * z.K * z.ld, z.ld, tmp + (size_t)w * z.cog * z.ld, z.ld, z.cog, z.ld, z.K,
                              nullptr, 0, s));
    }
    const size_t total = (size_t)n_img * c_out * d.P;
    hipLaunchKernelGGL(deform_output_kernel, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, s, tmp, d_bias, n_img, c_out, d.P, d.Pp, total,
                       d_out);
    return check_launch();
}

int frcnn_ops_deform_backward_columns(const frcnn_deform_geom* g, int n_img, const float* d_weight, const float* d_dout, float* d_dcol,
                                      void* d_ws, size_t ws_bytes, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups)) return FRCNN_EINVAL;
    const DeformSizes z = deform_sizes(d, c_out, groups, n_img);
    if (!d_weight || !d_dout || !d_dcol || !aligned16(d_dcol) || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform_workspace(d, z, n_img, FRCNN_DEFORM_WS_BACKWARD_COLUMNS)) return FRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(d_ws);
    float* wp = reinterpret_cast<float*>(ws);
    float* gt = reinterpret_cast<float*>(ws + z.wp);
    const size_t wtotal = (size_t)c_out * z.Kp;
    hipLaunchKernelGGL(deform_pad_rows_kernel<float>, dim3(df_blocks(wtotal)), dim3(DF_BLOCK), 0, s, d_weight, z.K, wp, z.Kp, wtotal);
    DF_TRY(check_launch());
    DF_TRY(deform_launch_pack_grad(n_img, c_out, d, d_dout, gt, s));
    for (int w = 0; w < groups; ++w)
        DF_TRY(launch_gemm_tn(wp + (size_t)w * z.cog * z.Kp, z.Kp, gt + (size_t)w * z.cog * z.ld, z.ld, d_dcol + (size_t)w * z.K * z.ld,
                              z.ld, z.K, z.ld, z.cog, nullptr, 0, s));
    return FRCNN_OK;
}

int frcnn_ops_deform_backward_offset(const frcnn_deform_geom* g, int n_img, const float* d_x, const float* d_offset, const float* d_mask,
                                     const float* d_dcol, float* d_doffset, float* d_dmask, void* stream)
{
    return deform_backward_offset_impl<float>(g, n_img, 4, d_x, d_offset, d_mask, d_dcol, d_doffset, d_dmask, stream);
}

int frcnn_ops_deform_input_plan(const frcnn_deform_geom* g, int n_img, const float* d_offset, const float* d_mask, int64_t* d_keys,
                                float* d_weights, void* stream)
{
    return deform_input_plan_impl<float>(g, n_img, 4, d_offset, d_mask, d_keys, d_weights, stream);
}

int frcnn_ops_deform_backward_input(const frcnn_deform_geom* g, int n_img, const int64_t* d_sorted_keys, const int64_t* d_order,
                                    const float* d_weights, const float* d_dcol, float* d_dx, void* d_ws, size_t ws_bytes, void* stream)
{
    return deform_backward_input_impl<float>(g, n_img, 4, d_sorted_keys, d_order, d_weights, d_dcol, d_dx, d_ws, ws_bytes, stream);
}

int frcnn_ops_deform_backward_weight(const frcnn_deform_geom* g, int n_img, const float* d_x, const float* d_offset, const float* d_mask,
                                     const float* d_dout, float* d_dweight, int accumulate, void* d_ws, size_t ws_bytes, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform_geom(g, n_img, d, c_out, groups)) return FRCNN_EINVAL;
    const DeformSizes z = deform_sizes(d, c_out, groups, n_img);
    if (!d_x || !d_offset || !d_dout || !d_dweight || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform_workspace(d, z, n_img, FRCNN_DEFORM_WS_BACKWARD_WEIGHT)) return FRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(d_ws);
    float* col = reinterpret_cast<float*>(ws);
    float* gt = reinterpret_cast<float*>(ws + z.col);
    float* gtT = reinterpret_cast<float*>(ws + z.col + z.gt);
    float* colT = reinterpret_cast<float*>(ws + z.col + z.gt + z.gtT);
    float* tmpw = reinterpret_cast<float*>(ws + z.col + z.gt + z.gtT + z.colT);
    void* gemm_ws = z.gemm ? ws + z.col + z.gt + z.gtT + z.colT + z.tmpw : nullptr;
    DF_TRY(deform_launch_columns(d, n_img, d_x, d_offset, d_mask, col, s));
    DF_TRY(deform_launch_pack_grad(n_img, c_out, d, d_dout, gt, s));
    for (int w = 0; w < groups; ++w) {
        DF_TRY(launch_transpose(gt + (size_t)w * z.cog * z.ld, z.ld, gtT, z.cogp, z.cog, z.ld, s));
        DF_TRY(launch_transpose(col + (size_t)w * z.K * z.ld, z.ld, colT, z.Kp, z.K, z.ld, s));
        DF_TRY(launch_gemm_tn(gtT, z.cogp, colT, z.Kp, tmpw, z.Kp, z.cog, z.K, z.ld, gemm_ws, z.gemm, s));
        const size_t total = (size_t)z.cog * z.K;
        hipLaunchKernelGGL(deform_add_rows_kernel, dim3(df_blocks(total)), dim3(DF_BLOCK), 0, s, tmpw, z.Kp,
                           d_dweight + (size_t)w * z.cog * z.K, z.K, accumulate, total);
        DF_TRY(check_launch());
    }
    return FRCNN_OK;
}

// ---- float16 / bfloat16 (elem_type: FRCNN_OPS_F16 / FRCNN_OPS_BF16) ------------------------------------------------------------------
static bool deform16_elem(int elem_type) { return elem_type == FRCNN_OPS_F16 || elem_type == FRCNN_OPS_BF16; }

size_t frcnn_ops_deform_workspace_bytes_16(int elem_type, const frcnn_deform_geom* g, int n_img, int stage)
{
    DeformGeom d; int c_out, groups;
    if (!deform16_elem(elem_type) || !deform_geom(g, n_img, d, c_out, groups, 8)) return 0;
    return deform16_workspace(d, deform16_sizes(d, c_out, groups, n_img), n_img, stage);
}

int frcnn_ops_deform_forward_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_x, const void* d_offset,
                                const void* d_mask, const void* d_weight, const void* d_bias, void* d_out, void* d_ws, size_t ws_bytes,
                                void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform16_elem(elem_type) || !deform_geom(g, n_img, d, c_out, groups, 8)) return FRCNN_EINVAL;
    const Deform16Sizes z = deform16_sizes(d, c_out, groups, n_img);
    if (!d_x || !d_offset || !d_weight || !d_out || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform16_workspace(d, z, n_img, FRCNN_DEFORM_WS_FORWARD)) return FRCNN_EINVAL;
    OPS_ELEM_DISPATCH(elem_type, E, deform16_forward<E>(elem_type, d, z, c_out, groups, n_img, static_cast<const E*>(d_x),
                                                        static_cast<const E*>(d_offset), static_cast<const E*>(d_mask),
                                                        static_cast<const E*>(d_weight), static_cast<const E*>(d_bias), static_cast<E*>(d_out),
                                                        static_cast<char*>(d_ws), (hipStream_t)stream));
}

int frcnn_ops_deform_backward_columns_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_weight, const void* d_dout,
                                         float* d_dcol, void* d_ws, size_t ws_bytes, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform16_elem(elem_type) || !deform_geom(g, n_img, d, c_out, groups, 8)) return FRCNN_EINVAL;
    const Deform16Sizes z = deform16_sizes(d, c_out, groups, n_img);
    if (!d_weight || !d_dout || !d_dcol || !aligned16(d_dcol) || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform16_workspace(d, z, n_img, FRCNN_DEFORM_WS_BACKWARD_COLUMNS)) return FRCNN_EINVAL;
    OPS_ELEM_DISPATCH(elem_type, E, deform16_backward_columns<E>(elem_type, d, z, c_out, groups, n_img, static_cast<const E*>(d_weight),
                                                                 static_cast<const E*>(d_dout), d_dcol, static_cast<char*>(d_ws),
                                                                 (hipStream_t)stream));
}

int frcnn_ops_deform_backward_offset_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_x, const void* d_offset,
                                        const void* d_mask, const float* d_dcol, void* d_doffset, void* d_dmask, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, deform_backward_offset_impl<E>(g, n_img, 8, static_cast<const E*>(d_x), static_cast<const E*>(d_offset),
                                                                   static_cast<const E*>(d_mask), d_dcol, static_cast<E*>(d_doffset),
                                                                   static_cast<E*>(d_dmask), stream));
}

int frcnn_ops_deform_input_plan_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_offset, const void* d_mask,
                                   int64_t* d_keys, float* d_weights, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, deform_input_plan_impl<E>(g, n_img, 8, static_cast<const E*>(d_offset), static_cast<const E*>(d_mask),
                                                              d_keys, d_weights, stream));
}

int frcnn_ops_deform_backward_input_16(int elem_type, const frcnn_deform_geom* g, int n_img, const int64_t* d_sorted_keys,
                                       const int64_t* d_order, const float* d_weights, const float* d_dcol, void* d_dx, void* d_ws,
                                       size_t ws_bytes, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, deform_backward_input_impl<E>(g, n_img, 8, d_sorted_keys, d_order, d_weights, d_dcol,
                                                                  static_cast<E*>(d_dx), d_ws, ws_bytes, stream));
}

int frcnn_ops_deform_backward_weight_16(int elem_type, const frcnn_deform_geom* g, int n_img, const void* d_x, const void* d_offset,
                                        const void* d_mask, const void* d_dout, float* d_dweight, int accumulate, void* d_ws,
                                        size_t ws_bytes, void* stream)
{
    DeformGeom d; int c_out, groups;
    if (!deform16_elem(elem_type) || !deform_geom(g, n_img, d, c_out, groups, 8)) return FRCNN_EINVAL;
    const Deform16Sizes z = deform16_sizes(d, c_out, groups, n_img);
    if (!d_x || !d_offset || !d_dout || !d_dweight || !d_ws || !aligned16(d_ws)) return FRCNN_EINVAL;
    if (ws_bytes < deform16_workspace(d, z, n_img, FRCNN_DEFORM_WS_BACKWARD_WEIGHT)) return FRCNN_EINVAL;
    OPS_ELEM_DISPATCH(elem_type, E, deform16_backward_weight<E>(elem_type, d, z, c_out, groups, n_img, static_cast<const E*>(d_x),
                                                                static_cast<const E*>(d_offset), static_cast<const E*>(d_mask),
                                                                static_cast<const E*>(d_dout), d_dweight, accumulate,
                                                                static_cast<char*>(d_ws), (hipStream_t)stream));
}

}  // extern "C"
