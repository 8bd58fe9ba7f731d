// gemm_nt16.hip -- the dense product of the 16-bit deformable convolution (ops_deform.hip): both operands float16 or bfloat16 IN
// MEMORY, float32 accumulators, on v_mfma_f32_32x32x16_{f16,bf16}.
//
//   C[m][n] = sum_r A[m][r] B[n][r]         A: M rows of stride lda, B: N rows of stride ldb, both contiguous along the reduction r
//
// Requirements (checked by the launchers): A and B 16-byte aligned, lda and ldb multiples of 8 elements, R a multiple of 8, and the
// producer has written the elements r in [true length, R) of every row as zeros.  Rows are never padded: a lane whose row lies
// beyond M (N) reads the last row instead and its results are not stored.
//
// Fragments go from global memory straight to registers, without LDS: with both operands reduction-contiguous, the eight
// consecutive r that lane (row l & 31, half l >> 5) feeds one MFMA are ONE aligned 16-byte load, already in the instruction's
// operand order (A[row][8 half + j], B[8 half + j][col]), so there is nothing to transpose or convert on the way, and a kernel
// without LDS has no barrier.  A 128 x 128 block tile is four waves of 64 x 64 (2 x 2 MFMA tiles: each fragment feeds two MFMAs);
// the 2 x 2 waves of a block re-read each other's rows through the vector L1.  The products of deformable convolution are short
// and wide (C_out, K <= a few thousand against n_img oh ow columns) and bound by the column matrix's traffic, which this form reads
// exactly once from HBM and which is half of what the float32 operator moves.
//
// The reduction of one output element is sequential inside one wave.  Without a split (splits == 1) the result does not depend on
// anything but the operands; with one, split z sums r in [z rps, (z + 1) rps) into plane z of a float32 workspace and
// gemm_nt16_reduce_kernel adds the planes in ascending z: deterministic, no atomics.
#include "ops_elem.h"

namespace frcnn {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

static constexpr int NT_TILE = 128;          // block tile (M and N); tests/deform16_cases.py sizes its tile-edge shape by it
static constexpr int NT_MAX_SPLITS = 64;
static constexpr int NT_SPLIT_BLOCKS = 512;  // blocks a split product aims at (2 per CU)

template <typename E> struct NtFrag;
template <> struct NtFrag<f16> {
    typedef f16x8_t vec;
    static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct NtFrag<bf16> {
    typedef bf16x8_t vec;
    static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// where the accumulators go
struct NtStore {
    float* c;            // float32 form: plane z, element c[z plane + m ldc + n]
    int ldc;
    size_t plane;
    void* out;           // NCHW form: out[(n / P) c_total + c_base + m][n % P] = round(acc + bias[c_base + m]), elements of type E
    const void* bias;    //   [c_total] elements of type E, or NULL
    int P, c_total, c_base;
};

template <typename E, bool NCHW>
__global__ __launch_bounds__(256)
void gemm_nt16_kernel(const E* __restrict__ A, int lda, const E* __restrict__ B, int ldb, int M, int N, int R, int rps, NtStore st)
{
    typedef typename NtFrag<E>::vec vec;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int m0 = blockIdx.y * NT_TILE + (wave >> 1) * 64, n0 = blockIdx.x * NT_TILE + (wave & 1) * 64;
    if (m0 >= M || n0 >= N) return;                            // the wave's tile is empty (no barrier anywhere in this kernel)
    const int rb = blockIdx.z * rps, re = min(R, rb + rps);   // rps is a multiple of 16, R of 8
    const E* ap[2];
    const E* bp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        ap[t] = A + (size_t)min(m0 + t * 32 + li, M - 1) * lda + lh * 8;
        bp[t] = B + (size_t)min(n0 + t * 32 + li, N - 1) * ldb + lh * 8;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
    // whole steps of 16: two register stages, the loads of the next step in flight behind the four MFMAs of this one
    auto load = [&](vec (&af)[2], vec (&bf)[2], int k) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            af[t] = *reinterpret_cast<const vec*>(ap[t] + k);
            bf[t] = *reinterpret_cast<const vec*>(bp[t] + k);
        }
    };
    auto multiply = [&](const vec (&af)[2], const vec (&bf)[2]) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = NtFrag<E>::mfma(af[mt], bf[nt], acc[mt][nt]);
    };
    int k = rb, steps = (re - rb) / 16;
    vec a0[2], b0[2], a1[2], b1[2];
    if (steps > 0) load(a0, b0, k);
    for (; steps >= 2; steps -= 2, k += 32) {
        load(a1, b1, k + 16);
        multiply(a0, b0);
        if (steps > 2) load(a0, b0, k + 32);
        multiply(a1, b1);
    }
    if (steps == 1) { multiply(a0, b0); k += 16; }
    if (k < re) {                                              // eight elements are left: the upper half's fragment lies beyond the row
        vec af[2], bf[2];
        const u32x4_t zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const u32x4_t a = lh == 0 ? *reinterpret_cast<const u32x4_t*>(ap[t] + k) : zero;
            const u32x4_t b = lh == 0 ? *reinterpret_cast<const u32x4_t*>(bp[t] + k) : zero;
            af[t] = __builtin_bit_cast(vec, a);
            bf[t] = __builtin_bit_cast(vec, b);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = NtFrag<E>::mfma(af[mt], bf[nt], acc[mt][nt]);
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = n0 + nt * 32 + li;
        if (n >= N) continue;
        int b = 0, p = 0;
        if (NCHW) { b = n / st.P; p = n - b * st.P; }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = m0 + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
                if (m >= M) continue;
                if (NCHW) {
                    const int co = st.c_base + m;
                    const float v = st.bias ? acc[mt][nt][i] + Elem<E>::load(static_cast<const E*>(st.bias), co) : acc[mt][nt][i];
                    round_to(v, static_cast<E*>(st.out)[((size_t)b * st.c_total + co) * st.P + p]);
                } else {
                    st.c[(size_t)blockIdx.z * st.plane + (size_t)m * st.ldc + n] = acc[mt][nt][i];
                }
            }
    }
}

// dst[m][n] (row stride ldd) = (accumulate ? dst[m][n] : 0) + (plane 0 + plane 1 + ... in ascending order)[m][n] (dense, N wide)
__global__ __launch_bounds__(256)
void gemm_nt16_reduce_kernel(const float* __restrict__ part, int splits, size_t plane, int N, float* __restrict__ dst, int ldd,
                             int accumulate, size_t total)
{
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int n = (int)(idx % N);
        const size_t m = idx / N;
        float v = part[idx];
        for (int z = 1; z < splits; ++z) v += part[(size_t)z * plane + idx];
        float* d = dst + m * ldd + n;
        *d = accumulate ? *d + v : v;
    }
}

static bool nt16_operands_ok(const void* A, int lda, const void* B, int ldb, int M, int N, int R)
{
    return A && B && !(reinterpret_cast<uintptr_t>(A) & 15) && !(reinterpret_cast<uintptr_t>(B) & 15) && M >= 1 && N >= 1 && R >= 8 &&
           R % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && lda >= R && ldb >= R && cdiv(M, NT_TILE) <= 65535;
}

// the split of a product with a long reduction and a small result: a function of the sizes alone, so the sum order is too
int gemm_nt16_splits(int M, int N, int R)
{
    const long long tiles = (long long)cdiv(M, NT_TILE) * cdiv(N, NT_TILE);
    long long s = NT_SPLIT_BLOCKS / tiles;
    s = std::min<long long>(s, cdiv(R, 256));                  // at least 256 reduction elements per split
    s = std::max<long long>(1, std::min<long long>(s, NT_MAX_SPLITS));
    const int rps = cdiv(cdiv(R, (int)s), 16) * 16;
    return cdiv(R, rps);                                       // no empty split
}

size_t gemm_nt16_workspace_bytes(int M, int N, int R) { return (size_t)gemm_nt16_splits(M, N, R) * M * N * sizeof(float); }

template <typename E, bool NCHW>
static int nt16_launch(const void* A, int lda, const void* B, int ldb, int M, int N, int R, int splits, const NtStore& st, hipStream_t s)
{
    const int rps = cdiv(cdiv(R, splits), 16) * 16;
    hipLaunchKernelGGL((gemm_nt16_kernel<E, NCHW>), dim3(cdiv(N, NT_TILE), cdiv(M, NT_TILE), splits), dim3(256), 0, s,
                       static_cast<const E*>(A), lda, static_cast<const E*>(B), ldb, M, N, R, rps, st);
    return check_launch();
}

// C (float32, row stride ldc) = A B^T without a split
int launch_gemm_nt16(int elem_type, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int R, hipStream_t s)
{
    if (!nt16_operands_ok(A, lda, B, ldb, M, N, R) || !C || ldc < N) return FRCNN_EINVAL;
    NtStore st = {C, ldc, 0, nullptr, nullptr, 0, 0, 0};
    OPS_ELEM_DISPATCH(elem_type, E, nt16_launch<E, false>(A, lda, B, ldb, M, N, R, 1, st, s));
}

// C (float32, row stride ldc) = or += A B^T through the deterministic split of gemm_nt16_splits; ws: gemm_nt16_workspace_bytes
int launch_gemm_nt16_split(int elem_type, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int R,
                           int accumulate, void* ws, size_t ws_bytes, hipStream_t s)
{
    if (!nt16_operands_ok(A, lda, B, ldb, M, N, R) || !C || ldc < N || !ws || (reinterpret_cast<uintptr_t>(ws) & 15)) return FRCNN_EINVAL;
    if (ws_bytes < gemm_nt16_workspace_bytes(M, N, R)) return FRCNN_EINVAL;
    const int splits = gemm_nt16_splits(M, N, R);
    const size_t plane = (size_t)M * N;
    NtStore st = {static_cast<float*>(ws), N, plane, nullptr, nullptr, 0, 0, 0};
    const int rc = [&]() -> int { OPS_ELEM_DISPATCH(elem_type, E, nt16_launch<E, false>(A, lda, B, ldb, M, N, R, splits, st, s)); }();
    if (rc) return rc;
    const size_t blocks = (plane + 255) / 256;
    hipLaunchKernelGGL(gemm_nt16_reduce_kernel, dim3((unsigned)std::min<size_t>(blocks, 16384)), dim3(256), 0, s,
                       static_cast<const float*>(ws), splits, plane, N, C, ldc, accumulate, plane);
    return check_launch();
}

// out[(n / P) c_total + c_base + m][n % P] = round(A B^T + bias[c_base + m]) in the operands' element type, without a split
int launch_gemm_nt16_nchw(int elem_type, const void* A, int lda, const void* B, int ldb, int M, int N, int R, const void* bias, void* out,
                          int P, int c_total, int c_base, hipStream_t s)
{
    if (!nt16_operands_ok(A, lda, B, ldb, M, N, R) || !out || P < 1 || N % P != 0 || c_base < 0 || c_base + M > c_total) return FRCNN_EINVAL;
    NtStore st = {nullptr, 0, 0, out, bias, P, c_total, c_base};
    OPS_ELEM_DISPATCH(elem_type, E, nt16_launch<E, true>(A, lda, B, ldb, M, N, R, 1, st, s));
}

}  // namespace frcnn
