// ops_run.h -- what the RoI and NMS kernels of fasterrcnn_amd.ops share across files (ops.hip, ops_rot.hip, ops_quadri.hip): the limits, the runs
// Run<E> of maps and gradients (ops_elem.h's), the ordered culling of the backward gathers, the entry points' argument checks and
// 16-bit dispatch, and the launcher of the greedy NMS pass.
#pragma once
#include "ops_geom.h"
#include "ops_elem.h"

namespace frcnn {

typedef unsigned long long u64;

static constexpr int OPS_TILE = 2;           // backward tile: 2 x 2 cells, one per wave, 64 channel runs per block
static_assert(OPS_TILE * OPS_TILE == 4, "the backward kernels give each of a block's four waves one cell of the tile");
static constexpr int OPS_LIST = 1024;        // RoIs culled per pass of a tile
static constexpr int OPS_MAX_OUT = 64;       // out_h, out_w <= 64
static constexpr int OPS_MAX_SAMPLING = 16;  // sampling_ratio <= 16
static constexpr int OPS_NMS_MAX_WORDS = 8192;   // removed-bits of one segment in 64 KB of LDS: n <= 524288
static constexpr int OPS_MS_MAX_LEVELS = 8;  // multi-scale RoIAlign: feature maps per call

// ---- storage types --------------------------------------------------------------------------------------------------------------
// A 16-bit element carries the width N of a lane's run in its type, so that one tensor can be walked in runs of 8 or of 4 channels
template <typename E, int N> struct run_t : E {};

// 16-bit channels per lane.  8 = 16 B per load and store, as a float quad: measured faster than 4 in every forward kernel and in the
// backward kernels once C / 8 fills a wave (C >= 512).  Below that a backward block, whose lanes are the channel runs of one cell,
// would idle half of each wave: there the gather walks the same tensors in runs of 4 (C = 256: 7 % faster forward + backward).
static constexpr int OPS_HALF_RUN = 8, OPS_HALF_RUN_NARROW = 4;

// Run<E>: V consecutive channels of one pixel, in memory as E, in registers as float32 (vec): ops_elem.h's run and its roundings
template <typename E> struct Run;
template <> struct Run<float> : ElemRun<float, 4> {};
template <typename E, int N> struct Run<run_t<E, N>> : ElemRun<E, N> {};

template <typename E> __device__ __forceinline__ void zero_row(E* orow, int n)
{
    const typename Run<E>::vec z = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) Run<E>::store(orow, i, z);
}

// Ordered culling shared by the two backward kernels: appends to s_list, in ascending order, the RoIs r >= r_begin for which
// touches(r) holds, until OPS_LIST are listed.  Returns the first RoI not examined (k when all were).  Block of 256 threads.
template <typename Touches>
__device__ int cull_rois(int r_begin, int k, Touches touches, int* s_list, int* s_cnt, int* s_n)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                     // the previous pass has finished reading s_list
    if (tid == 0) *s_n = 0;
    int r0 = r_begin;
    for (; r0 < k; r0 += 256) {
        const int r = r0 + tid;
        const bool hit = r < k && touches(r);
        const u64 m = __ballot(hit);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        const int base = *s_n;
        const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (base + total > OPS_LIST) break;              // uniform: the list is full; this group starts the next pass
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_cnt[w];
        if (hit) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        if (tid == 0) *s_n = base + total;
    }
    __syncthreads();
    return r0 < k ? r0 : k;
}

// v: the channels of a lane's run (Run<E>::V)
static inline bool roi_args_ok(int n_img, int fh, int fw, int c, int k, int out_h, int out_w, int v)
{
    return n_img >= 1 && fh >= 1 && fw >= 1 && c >= v && c % v == 0 && k >= 0 && out_h >= 1 && out_h <= OPS_MAX_OUT && out_w >= 1 &&
           out_w <= OPS_MAX_OUT && (size_t)fh * fw <= (size_t)INT32_MAX && (size_t)n_img * cdiv(c / v, 64) <= 65535;   // backward grid z
}

// the run of a backward gather over c channels: the wide one when its runs fill the 64 lanes that share a cell
static inline int backward_run(int c) { return c / OPS_HALF_RUN >= 64 ? OPS_HALF_RUN : OPS_HALF_RUN_NARROW; }

// ops.hip: ops_nms_reduce_kernel on a mask of 64 x 64 bit tiles (ops_nms_mask_kernel's layout; nw = ceil(n / 64) words per row)
int launch_ops_nms_reduce(const u64* mask, const int64_t* order, const int64_t* cats, int n, int nw, uint8_t* keep, hipStream_t s);

}  // namespace frcnn

// A 16-bit entry point's body by element-type code, in runs of `run` channels; c must hold whole runs of OPS_HALF_RUN either way.
#define OPS_DISPATCH_16(elem_type, c, run, impl, ...)                                                                         \
    do {                                                                                                                      \
        if ((c) % OPS_HALF_RUN != 0) return FRCNN_EINVAL;                                                                     \
        const bool wide = (run) == OPS_HALF_RUN;                                                                              \
        OPS_ELEM_DISPATCH(elem_type, E_, wide ? impl<run_t<E_, OPS_HALF_RUN>>(__VA_ARGS__)                                    \
                                              : impl<run_t<E_, OPS_HALF_RUN_NARROW>>(__VA_ARGS__));                           \
    } while (0)
