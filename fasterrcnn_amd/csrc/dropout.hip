// dropout.hip -- nn.Dropout(p) of the VGG-16 head in training mode (reference: models/vgg16.py:129-133, built with
// `--dropout p`, __main__.py:284), and its backward fused with the ReLU backward in front of it.
//
//   dropout_kernel               in place on the ReLU output: keep = uniform < 1 - p, y = keep ? x * scale : 0, scale = 1 / (1 - p).
//                                The uniform of element i is word (i & 3) of Philox4x32-10 (Salmon et al., SC'11; the Random123
//                                constants) with key = the 64-bit seed (lo, hi) and counter = (i >> 2 lo, i >> 2 hi, stream_id, rank):
//                                uniform = (word >> 8) * 2^-24, exact in float32.  One Philox call serves four consecutive elements.
//                                The seed is read from device memory, so drawing it never synchronises the host.
//   dropout_relu_backward_kernel dy = y > 0 ? dy * scale : 0 with y the saved output AFTER dropout: y > 0 exactly when the element was
//                                kept and relu(z) > 0 (scale >= 1 is finite), which is where autograd of dropout(relu(z)) passes
//                                dy * mask * scale = dy * scale.  No mask is stored.
#include "common.h"

namespace frcnn {

namespace {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += kPhiloxW0; k1 += kPhiloxW1; }
        const uint32_t lo0 = kPhiloxM0 * c[0], hi0 = __umulhi(kPhiloxM0, c[0]);
        const uint32_t lo1 = kPhiloxM1 * c[2], hi1 = __umulhi(kPhiloxM1, c[2]);
        c = u32x4{hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
    }
    return c;
}

// uniform in [0, 1) on the 2^-24 grid, compared in float32 against 1 - p
__device__ __forceinline__ bool keep_of(uint32_t word, float keep_below)
{
    return (float)(word >> 8) * 0x1p-24f < keep_below;
}

__global__ __launch_bounds__(256)
void dropout_kernel(float* __restrict__ x, size_t n4, size_t n, float keep_below, float scale, int write_x,
                    const uint64_t* __restrict__ seed_p, uint32_t stream_id, uint32_t rank, uint8_t* __restrict__ keep_out)
{
    const uint64_t seed = *seed_p;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    // groups of four elements: g < n4 are whole float4s, g == n4 is the n % 4 tail (if any)
    const size_t groups = (n + 3) / 4;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const u32x4 r = philox4x32_10(u32x4{(uint32_t)g, (uint32_t)(g >> 32), stream_id, rank}, k0, k1);
        if (g < n4) {
            f32x4 v = reinterpret_cast<const f32x4*>(x)[g];
            bool kp[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kp[j] = keep_of(r[j], keep_below);
                v[j] = kp[j] ? v[j] * scale : 0.f;
            }
            if (write_x) reinterpret_cast<f32x4*>(x)[g] = v;
            if (keep_out) {
#pragma unroll
                for (int j = 0; j < 4; ++j) keep_out[4 * g + j] = kp[j] ? 1 : 0;
            }
        } else {
            for (size_t i = 4 * g; i < n; ++i) {
                const bool kp = keep_of(r[i & 3], keep_below);
                if (write_x) x[i] = kp ? x[i] * scale : 0.f;
                if (keep_out) keep_out[i] = kp ? 1 : 0;
            }
        }
    }
}

__global__ __launch_bounds__(256)
void dropout_relu_backward_kernel(float* __restrict__ dy, const float* __restrict__ y, size_t n4, size_t n, float scale)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 g = reinterpret_cast<f32x4*>(dy)[i];
        const f32x4 v = reinterpret_cast<const f32x4*>(y)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? g[j] * scale : 0.f;
        reinterpret_cast<f32x4*>(dy)[i] = g;
    }
    if (blockIdx.x == 0)
        for (size_t i = 4 * n4 + threadIdx.x; i < n; i += 256) dy[i] = y[i] > 0.f ? dy[i] * scale : 0.f;
}

// memory-bound elementwise: 256 threads, at most 2048 blocks, grid-stride for the rest
int grid_2048(size_t items)
{
    size_t b = (items + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

}  // namespace

int launch_dropout(float* x, size_t n, float p, float scale, const uint64_t* seed, uint32_t stream_id, uint32_t rank,
                   uint8_t* keep_out, hipStream_t s)
{
    if (reinterpret_cast<uintptr_t>(x) & 15) return FRCNN_EINVAL;
    const int write_x = p > 0.f;
    if (n == 0 || (!write_x && !keep_out)) return FRCNN_OK;          // p == 0: x is left untouched
    hipLaunchKernelGGL(dropout_kernel, dim3(grid_2048((n + 3) / 4)), dim3(256), 0, s, x, n / 4, n, 1.0f - p, scale, write_x, seed,
                       stream_id, rank, keep_out);
    return check_launch();
}

int launch_dropout_relu_backward(float* dy, const float* y, size_t n, float scale, hipStream_t s)
{
    if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y)) & 15) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    hipLaunchKernelGGL(dropout_relu_backward_kernel, dim3(grid_2048(n / 4 + 1)), dim3(256), 0, s, dy, y, n / 4, n, scale);
    return check_launch();
}

}  // namespace frcnn
