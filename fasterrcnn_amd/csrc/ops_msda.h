// ops_msda.h -- what the channels-last deformable samplers share (ops_msda.hip: multi-scale deformable attention; ops_dcn.h: DCNv3 and
// DCNv4): the 16-byte runs of the element types (ops_elem.h), the lanes-along-channels mapping, and the sorted-plan gather of the
// value / input gradient.
#pragma once
#include "ops_elem.h"

namespace frcnn {

static constexpr int MSDA_MAX_CHANNELS = 256;            // D, the channels of one head (of one group of DCNv3)
static constexpr int MSDA_BLOCK = 256;
static constexpr int MSDA_LDS_SAMPLES = 1024;            // samples of a block's items staged in LDS: 12 KB
static constexpr int MSDA_SCALAR_PASSES = MSDA_MAX_CHANNELS / 64;
static constexpr int MSDA_SEGMENT = 512;                 // entries of one piece of a long d_value segment
static constexpr long long MSDA_MAX_SIDE = 1 << 24;      // H_l, W_l: exact in float32
static constexpr long long MSDA_MAX_INDEX = (long long)INT32_MAX - 1024;   // plan entries and cells of one call
static constexpr int MSDA_MAX_BLOCKS = 16384;            // of the one-thread-per-element kernels: grid-stride beyond

template <int R> struct MsVec { float v[R]; };

template <typename E> struct MsElem { static constexpr int RUN = ELEM_WIDE_RUN<E>; };

// R consecutive channels from p (16-byte aligned when R > 1), widened exactly
template <typename E, int R> __device__ __forceinline__ MsVec<R> ms_load(const E* p)
{
    MsVec<R> r;
    if constexpr (sizeof(E) == 4) {
        if constexpr (R == 4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int j = 0; j < 4; ++j) r.v[j] = t[j];
        } else {
            r.v[0] = p[0];
        }
    } else {
        typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
        unsigned short u[R];
        if constexpr (R == 8) {
            const u16x8 t = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
            for (int j = 0; j < 8; ++j) u[j] = t[j];
        } else {
            u[0] = *reinterpret_cast<const unsigned short*>(p);
        }
#pragma unroll
        for (int j = 0; j < R; ++j) r.v[j] = widen(__builtin_bit_cast(E, u[j]));
    }
    return r;
}

// rounded once (ops_elem.h)
template <typename E, int R> __device__ __forceinline__ void ms_store(E* p, const MsVec<R>& a)
{
    if constexpr (sizeof(E) == 4) {
        if constexpr (R == 4) {
            *reinterpret_cast<f32x4*>(p) = f32x4{a.v[0], a.v[1], a.v[2], a.v[3]};
        } else {
            p[0] = a.v[0];
        }
    } else {
        typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
        unsigned short u[R];
#pragma unroll
        for (int j = 0; j < R; ++j) u[j] = __builtin_bit_cast(unsigned short, narrow<E>(a.v[j]));
        if constexpr (R == 8) {
            u16x8 t;
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = u[j];
            *reinterpret_cast<u16x8*>(p) = t;
        } else {
            *reinterpret_cast<unsigned short*>(p) = u[0];
        }
    }
}

// what the host and the kernels agree on for one (D, samples per item, element type): the lanes of a group, a lane's passes, the items
// of a block
struct MsMap { int R, T, nruns, passes, ipb, threads; };

static inline int pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

static inline MsMap ms_map(int d, int lp, int run, bool vector)
{
    MsMap m;
    m.R = vector ? run : 1;
    m.nruns = d / m.R;
    m.T = pow2_ceil(m.nruns) < 64 ? pow2_ceil(m.nruns) : 64;
    m.passes = (m.nruns + m.T - 1) / m.T;
    const int by_lds = MSDA_LDS_SAMPLES / (lp > 0 ? lp : 1);
    m.ipb = MSDA_BLOCK / m.T < by_lds ? MSDA_BLOCK / m.T : by_lds;
    m.threads = (m.ipb * m.T + 63) / 64 * 64;
    return m;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline unsigned msda_blocks(long long total)
{
    const long long b = (total + MSDA_BLOCK - 1) / MSDA_BLOCK;
    return (unsigned)(b < MSDA_MAX_BLOCKS ? (b ? b : 1) : MSDA_MAX_BLOCKS);
}

// The sorted-plan gather (ops_msda.hip).  The plan holds samples4 = 4 * (samples per item) entries for each of n_entries / samples4
// items, entry e belonging to item e / samples4; sorted_keys / order are its stably sorted keys (cell indices in [0, n_cells), the
// sentinel n_cells for a corner that counts 0) and the permutation.  dvalue[c][:] = the sum over cell c's entries in ascending e of
// wts[e] * dout[e / samples4][:], rows of d elements; every cell is written; a segment of more than MSDA_SEGMENT entries is summed in
// pieces.  elem_type 0: float32 rows, else FRCNN_OPS_F16 / FRCNN_OPS_BF16.  The caller has bounded n_cells and n_entries by
// MSDA_MAX_INDEX and d by MSDA_MAX_CHANNELS.
size_t msda_gather_workspace(int n_cells, int n_entries, int d);
int msda_gather(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout, int n_cells,
                int n_entries, int samples4, int d, void* dvalue, void* ws, size_t ws_bytes, hipStream_t stream);

}  // namespace frcnn
