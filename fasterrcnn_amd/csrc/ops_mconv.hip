// ops_mconv.hip -- masked_conv2d (mmcv.ops.MaskedConv2d, the sparse convolution of Guided Anchoring's heads; include/frcnn_hip.h
// states the contract): a stride-1 convolution evaluated at the ACTIVE output pixels only, +0.0 everywhere else, with the active count
// never leaving the device.
//
//   mconv_compact_kernel   one pass over the uint8 mask [n oh ow]: an active pixel appends its flat index b oh ow + p to the list in
//                          the workspace (a wave's ballot, one integer atomicAdd per wave on the count, so the list's order is not
//                          fixed: no output bit depends on it); an inactive pixel writes its C_out zeros through the output's strides.
//                          Every inactive output element is written exactly once, and no active one is touched.
//   mconv_kernel<E>        the implicit GEMM  out[co][pixel] = sum_r weight[co][r] tap[pixel][r],  r = (c kh + i) kw + j, over tiles of
//                          MC_T listed pixels x MC_CO output channels.  The grid holds the worst case ceil(n oh ow / MC_T) tiles; a
//                          block whose tile starts at or past the device-side count returns at once.
//
// A block of four waves owns a 64 x 64 tile, a wave one 32 x 32 accumulator.  Per chunk of MC_KC reduction indices the block stages
// weight[MC_CO][MC_KC] and tap[MC_T][MC_KC] in LDS, in the element type: weights by rows (32 consecutive r per half wave), taps
// gathered straight from the map through its element strides (b, c, y, x), a lane per pixel and a wave per 8 consecutive r, whose
// (c, i, j) is wave-uniform and stepped without a division.  The loads of chunk s + 1 are in flight behind the MFMAs of chunk s.
// A tap outside the map, a reduction index >= K, a channel >= C_out and a pixel past the count are zeros formed in registers: their
// addresses are never formed.  float32 multiplies on v_mfma_f32_32x32x2_f32 (an f32 fma chain in ascending r), float16 / bfloat16 on
// v_mfma_f32_32x32x16_{f16,bf16} with float32 accumulators; the bias is added in float32 and the store rounds once (ops_elem.h).
//
// The reduction of one output element walks r = 0, 1, ... in chunks of MC_KC inside one wave's accumulator: its order depends on
// (C_in, kh, kw) alone, and the other rows and columns of the tile (other pixels, other channels, zero padding) do not enter it.
#include "ops_elem.h"

namespace frcnn {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

static constexpr int MC_T = 64;          // listed pixels of a block's tile
static constexpr int MC_CO = 64;         // output channels of a block's tile
static constexpr int MC_KC = 32;         // reduction indices of one LDS stage
static constexpr int MC_WS_HEAD = 16;    // ints before the list: the count, padded to 64 bytes
static constexpr long long MC_MAX_INDEX = 2147483647LL - 1024;

// sizes and element strides of one call; is / os: the strides of (b, c, y, x) in the input and the output
struct McGeom {
    int n, c, h, w, co, kh, kw, ph, pw, oh, ow;
    int is[4], os[4];
};

// the matrix pipe of an element type: the LDS row (padded against bank conflicts, 16-byte rows for the 16-bit fragments) and the
// MFMAs of one staged chunk; a, b: the lane's rows of the weight and the tap image
template <typename E> struct McPipe;
template <> struct McPipe<float> {
    static constexpr int ROW = MC_KC + 1;
    static __device__ __forceinline__ f32x16 chunk(const float* a, const float* b, int lh, f32x16 acc)
    {
#pragma unroll
        for (int s = 0; s < MC_KC / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s + lh], b[2 * s + lh], acc, 0, 0, 0);
        return acc;
    }
};
template <> struct McPipe<f16> {
    static constexpr int ROW = MC_KC + 8;
    static __device__ __forceinline__ f32x16 chunk(const f16* a, const f16* b, int lh, f32x16 acc)
    {
#pragma unroll
        for (int s = 0; s < MC_KC / 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8_t*>(a + 16 * s + 8 * lh),
                                                         *reinterpret_cast<const f16x8_t*>(b + 16 * s + 8 * lh), acc, 0, 0, 0);
        return acc;
    }
};
template <> struct McPipe<bf16> {
    static constexpr int ROW = MC_KC + 8;
    static __device__ __forceinline__ f32x16 chunk(const bf16* a, const bf16* b, int lh, f32x16 acc)
    {
#pragma unroll
        for (int s = 0; s < MC_KC / 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(a + 16 * s + 8 * lh),
                                                          *reinterpret_cast<const bf16x8_t*>(b + 16 * s + 8 * lh), acc, 0, 0, 0);
        return acc;
    }
};

// Z: the unsigned integer of the element's size (a zero of every element type is all bits clear)
template <typename Z>
__global__ __launch_bounds__(256)
void mconv_compact_kernel(const uint8_t* __restrict__ mask, int npix, int* __restrict__ ws, Z* __restrict__ out, McGeom g)
{
    const int flat = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = flat < npix;
    const bool active = in && mask[flat] != 0;
    const unsigned long long bits = __ballot(active);
    int base = 0;
    if (lane == 0 && bits) base = atomicAdd(ws, __popcll(bits));
    base = __shfl(base, 0);
    if (active) ws[MC_WS_HEAD + base + __popcll(bits & ((1ull << lane) - 1ull))] = flat;
    if (!in || active) return;
    const int plane = g.oh * g.ow, b = flat / plane, p = flat - b * plane, y = p / g.ow, x = p - y * g.ow;
    Z* o = out + (b * g.os[0] + y * g.os[2] + x * g.os[3]);
    for (int co = 0; co < g.co; ++co) o[co * g.os[1]] = (Z)0;
}

template <typename E>
__global__ __launch_bounds__(256)
void mconv_kernel(const E* __restrict__ x, const E* __restrict__ wt, const E* __restrict__ bias, E* __restrict__ out,
                  const int* __restrict__ ws, McGeom g)
{
    constexpr int ROW = McPipe<E>::ROW;
    __shared__ __attribute__((aligned(16))) E s_w[MC_CO * ROW];
    __shared__ __attribute__((aligned(16))) E s_t[MC_T * ROW];
    const int count = ws[0], tile0 = blockIdx.x * MC_T;
    if (tile0 >= count) return;                                  // block-uniform: before any barrier
    const int* list = ws + MC_WS_HEAD;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), li = lane & 31, lh = lane >> 5;
    const int taps = g.kh * g.kw, K = g.c * taps, co0 = blockIdx.y * MC_CO, plane = g.oh * g.ow;

    // the lane's pixel of the gather: image offset and the map coordinates of its tap (0, 0)
    const bool live = tile0 + lane < count;
    int gb = 0, gy = 0, gx = 0;
    if (live) {
        const int flat = list[tile0 + lane], b = flat / plane, p = flat - b * plane, y = p / g.ow;
        gb = b * g.is[0]; gy = y - g.ph; gx = p - y * g.ow - g.pw;
    }
    const int wk = t & 31, wrow = t >> 5;                        // the thread's weights: column wk of rows wrow + 8 q

    E rw[8], rt[8];
    auto load = [&](int r0) {
        const int r = r0 + wk;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int co = co0 + wrow + 8 * q;
            rw[q] = E{};
            if (co < g.co && r < K) rw[q] = wt[co * K + r];
        }
        const int rq = r0 + 8 * wave;                            // wave-uniform: (c, i, j) of the wave's 8 reduction indices
        int c = rq / taps, i = (rq - c * taps) / g.kw, j = rq - c * taps - i * g.kw;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int yy = gy + i, xx = gx + j;
            rt[q] = E{};
            if (live && rq + q < K && yy >= 0 && yy < g.h && xx >= 0 && xx < g.w) rt[q] = x[gb + c * g.is[1] + yy * g.is[2] + xx * g.is[3]];
            if (++j == g.kw) { j = 0; if (++i == g.kh) { i = 0; ++c; } }
        }
    };

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const E* aw = s_w + (32 * (wave >> 1) + li) * ROW;
    const E* at = s_t + (32 * (wave & 1) + li) * ROW;
    const int chunks = (K + MC_KC - 1) / MC_KC;
    load(0);
    for (int s = 0; s < chunks; ++s) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            s_w[(wrow + 8 * q) * ROW + wk] = rw[q];
            s_t[lane * ROW + 8 * wave + q] = rt[q];
        }
        __syncthreads();
        if (s + 1 < chunks) load((s + 1) * MC_KC);
        acc = McPipe<E>::chunk(aw, at, lh, acc);
        __syncthreads();
    }

    // C/D map of the 32 x 32 MFMA: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int pix = tile0 + 32 * (wave & 1) + li;
    if (pix >= count) return;
    const int flat = list[pix], b = flat / plane, p = flat - b * plane, y = p / g.ow;
    E* o = out + (b * g.os[0] + y * g.os[2] + (p - y * g.ow) * g.os[3]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int co = co0 + 32 * (wave >> 1) + (i & 3) + 8 * (i >> 2) + 4 * lh;
        if (co >= g.co) continue;
        const float v = bias ? acc[i] + widen(bias[co]) : acc[i];
        round_to(v, o[co * g.os[1]]);
    }
}

template <typename E>
static int mconv_launch(const void* x, const void* wt, const void* bias, void* out, const int* ws, const McGeom& g, int npix, hipStream_t s)
{
    hipLaunchKernelGGL((mconv_kernel<E>), dim3(cdiv(npix, MC_T), cdiv(g.co, MC_CO)), dim3(256), 0, s, static_cast<const E*>(x),
                       static_cast<const E*>(wt), static_cast<const E*>(bias), static_cast<E*>(out), ws, g);
    return check_launch();
}

// 1 + the largest element offset of a [d0, d1, d2, d3] tensor with these strides; 0 when a stride is negative
static long long mconv_extent(const int64_t* stride, int d0, int d1, int d2, int d3)
{
    const int d[4] = {d0, d1, d2, d3};
    long long e = 1;
    for (int k = 0; k < 4; ++k) {
        if (stride[k] < 0 || stride[k] > MC_MAX_INDEX) return 0;
        e += (long long)(d[k] - 1) * stride[k];
        if (e > MC_MAX_INDEX) return MC_MAX_INDEX + 1;
    }
    return e;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_masked_conv2d_tile_pixels(void) { return MC_T; }
int frcnn_ops_masked_conv2d_tile_channels(void) { return MC_CO; }
int frcnn_ops_masked_conv2d_k_chunk(void) { return MC_KC; }
int frcnn_ops_masked_conv2d_max_index(void) { return (int)MC_MAX_INDEX; }

size_t frcnn_ops_masked_conv2d_workspace_bytes(int n_img, int oh, int ow)
{
    if (n_img < 1 || oh < 1 || ow < 1 || (long long)n_img * oh * ow > MC_MAX_INDEX) return 0;
    return ((size_t)MC_WS_HEAD + (size_t)n_img * oh * ow) * sizeof(int);
}

int frcnn_ops_masked_conv2d(int elem_type, const void* d_input, const int64_t* in_stride, int n_img, int c_in, int h, int w,
                            const void* d_weight, const void* d_bias, int c_out, int kh, int kw, int pad_h, int pad_w,
                            const uint8_t* d_mask, void* d_out, const int64_t* out_stride, void* d_ws, size_t ws_bytes, void* stream)
{
    if (elem_type != FRCNN_OPS_F32 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    if (n_img < 1 || c_in < 1 || h < 1 || w < 1 || c_out < 1 || kh < 1 || kw < 1 || pad_h < 0 || pad_w < 0) return FRCNN_EINVAL;
    if (!d_input || !in_stride || !d_weight || !d_mask || !d_out || !out_stride || !d_ws || (reinterpret_cast<uintptr_t>(d_ws) & 3))
        return FRCNN_EINVAL;
    const long long oh = (long long)h + 2LL * pad_h - kh + 1, ow = (long long)w + 2LL * pad_w - kw + 1;
    if (oh < 1 || ow < 1 || oh > MC_MAX_INDEX || ow > MC_MAX_INDEX) return FRCNN_EINVAL;
    const long long npix = (long long)n_img * oh * ow, K = (long long)c_in * kh * kw;
    if (npix > MC_MAX_INDEX || K > MC_MAX_INDEX || K * c_out > MC_MAX_INDEX || cdiv(c_out, MC_CO) > 65535) return FRCNN_EINVAL;
    if ((long long)h + pad_h + kh > MC_MAX_INDEX || (long long)w + pad_w + kw > MC_MAX_INDEX) return FRCNN_EINVAL;
    const long long in_extent = mconv_extent(in_stride, n_img, c_in, h, w), out_extent = mconv_extent(out_stride, n_img, c_out, (int)oh, (int)ow);
    if (in_extent < 1 || in_extent > MC_MAX_INDEX || out_extent < 1 || out_extent > MC_MAX_INDEX) return FRCNN_EINVAL;
    if (ws_bytes < frcnn_ops_masked_conv2d_workspace_bytes(n_img, (int)oh, (int)ow)) return FRCNN_EINVAL;

    McGeom g = {n_img, c_in, h, w, c_out, kh, kw, pad_h, pad_w, (int)oh, (int)ow, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int k = 0; k < 4; ++k) { g.is[k] = (int)in_stride[k]; g.os[k] = (int)out_stride[k]; }
    const hipStream_t s = (hipStream_t)stream;
    int* ws = static_cast<int*>(d_ws);
    FRCNN_HIP_TRY(hipMemsetAsync(ws, 0, sizeof(int), s));          // the count; the list needs no initial value
    if (elem_type == FRCNN_OPS_F32)
        hipLaunchKernelGGL((mconv_compact_kernel<uint32_t>), dim3(cdiv((int)npix, 256)), dim3(256), 0, s, d_mask, (int)npix, ws,
                           static_cast<uint32_t*>(d_out), g);
    else
        hipLaunchKernelGGL((mconv_compact_kernel<uint16_t>), dim3(cdiv((int)npix, 256)), dim3(256), 0, s, d_mask, (int)npix, ws,
                           static_cast<uint16_t*>(d_out), g);
    const int rc = check_launch();
    if (rc) return rc;
    if (elem_type == FRCNN_OPS_F32) return mconv_launch<float>(d_input, d_weight, d_bias, d_out, ws, g, (int)npix, s);
    OPS_ELEM_DISPATCH(elem_type, E, mconv_launch<E>(d_input, d_weight, d_bias, d_out, ws, g, (int)npix, s));
}

}  // extern "C"
