// ops_msda.hip -- multi-scale deformable attention, the sampling core of Deformable DETR (mmcv's ms_deform_attn), in both directions:
// the frcnn_ops_msda* entry points of include/frcnn_hip.h.  Restated from the published algorithm (third party, absent here: restated,
// unpinned, like the other operators of fasterrcnn_amd.ops; where the two differ include/frcnn_hip.h holds).
//
//   value [n][S][M][D], shapes int64 [L][2] rows (H_l, W_l), starts int64 [L], loc float32 [n][Q][M][L][P][2] (x, y), attn float32
//   [n][Q][M][L][P], out [n][Q][M D].  Sample (b, q, m, l, p): x = fmaf(loc_x, W_l, -0.5f), y = fmaf(loc_y, H_l, -0.5f); it counts iff
//   x > -1 && y > -1 && x < W_l && y < H_l (a NaN fails); corners (y0, x0), (y0, x1), (y1, x0), (y1, x1) of floor / floor + 1 with the
//   weights hy hx, hy lx, ly hx, ly lx; a corner outside the level, or whose cell start_l + yy W_l + xx lies outside [0, S), counts 0.
//   out[b][q][m D + d] = sum over (l, p) ascending of attn * ((w0 v0 + w1 v1) + w2 v2 + w3 v3), every product and sum in float32.
//
// The shape tensors stay on the GPU and are read by the kernels, so nothing here trusts them: a level with H or W outside
// [1, MSDA_MAX_SIDE] or a start outside [-MSDA_MAX_START, S) contributes nothing, and every cell index is checked against [0, S) in 64
// bits before it is used.
//
// Mapping (forward and d_loc / d_attn): an item is one (b, q, m); a group of T lanes (a power of two <= 64) serves it, lanes along D, so
// a corner read is one contiguous run of value[b][cell][m][:]: R = 4 floats or 8 16-bit values per lane (16 B) when D holds whole runs
// and the tensors are 16-byte aligned, else the scalar body (R = 1, a lane walks d = t, t + T, ...: at most MSDA_SCALAR_PASSES).  256 / T
// items share a block (several queries per wave when D is small), fewer when their L P samples would not fit MSDA_LDS_SAMPLES: the
// block's locations and weights are one contiguous piece of loc / attn, staged once in LDS by coalesced loads.
// d_loc / d_attn: per sample, a lane's partial sums over its channels, then an xor butterfly over the T lanes (a fixed order:
// deterministic), one store per (b, q, m, l, p) by the group's lane 0.
// d_value: deterministic and without atomics, as ops_deform.hip builds its input gradient.  The plan writes one entry per sample and
// corner, e = ((((b Q + q) M + m) L + l) P + p) 4 + corner, with the key (b S + cell) M + m, or the sentinel n S M for a rejected
// corner, and the weight corner weight * attn.  The caller sorts the keys stably; a binary search finds the segment starts; one group
// of T lanes per (b, cell, m) sums its entries in ascending e, weight * dout[b][q][m][:], and stores its run: every cell is written,
// zeros included.  A few cells own thousands of entries where the median owns tens (every query samples every coarse level), and a
// gather runs as long as its most loaded wave, so a segment longer than MSDA_SEGMENT entries is cut, from its own start, into pieces of
// MSDA_SEGMENT: groups of their own sum the pieces into the workspace, and the cell's group adds the pieces' sums in ascending order.
// A window of MSDA_SEGMENT sorted positions holds the start of at most two such pieces (of the segment that crosses the window's first
// position and of a long one that begins inside it), so the pieces need no count and no host sync: two slots per window.  The cuts
// depend on the segment alone and a cell's entries all belong to its own image, so no bit of the result depends on how the images
// are chunked.
//
// Element types: templates over the storage type E of value, dout, out and d_value (float, float16, bfloat16): widened exactly on load,
// the float32 body, one rounding to nearest even on store as Tensor.to() rounds.  loc, attn, d_loc and d_attn are float32.
#include "ops_msda.h"

namespace frcnn {

static constexpr int MSDA_MAX_LEVELS = 8;
static constexpr int MSDA_MAX_POINTS = 16;
static constexpr long long MSDA_MAX_START = 1LL << 50;

static_assert(MSDA_MAX_LEVELS * MSDA_MAX_POINTS <= MSDA_LDS_SAMPLES, "one item's samples fit the staging buffer");

// ---- geometry ----------------------------------------------------------------------------------------------------------------------
struct MsLevel { long long start; int h, w; bool ok; };

__device__ __forceinline__ MsLevel ms_level(const long long* __restrict__ shapes, const long long* __restrict__ starts, int l, long long S)
{
    const long long h = shapes[2 * l], w = shapes[2 * l + 1], st = starts[l];
    MsLevel v;
    v.ok = h >= 1 && h <= MSDA_MAX_SIDE && w >= 1 && w <= MSDA_MAX_SIDE && st >= -MSDA_MAX_START && st < S;
    v.h = v.ok ? (int)h : 1; v.w = v.ok ? (int)w : 1; v.start = v.ok ? st : 0;
    return v;
}

// valid: the sample counts.  cell[k] >= 0: corner k lies inside the level and inside [0, S); w[k]: its bilinear weight (set for all four)
struct MsSample { long long cell[4]; float w[4]; float hy, hx, ly, lx; bool valid; };

__device__ __forceinline__ MsSample ms_sample(const MsLevel& lv, float loc_x, float loc_y, long long S)
{
    MsSample s;
    const float x = fmaf(loc_x, (float)lv.w, -0.5f), y = fmaf(loc_y, (float)lv.h, -0.5f);
    s.valid = lv.ok && x > -1.0f && y > -1.0f && x < (float)lv.w && y < (float)lv.h;
#pragma unroll
    for (int k = 0; k < 4; ++k) { s.cell[k] = -1; s.w[k] = 0.f; }
    s.hy = s.hx = s.ly = s.lx = 0.f;
    if (!s.valid) return s;
    const float fy = floorf(y), fx = floorf(x);
    const int y0 = (int)fy, x0 = (int)fx;
    s.ly = y - fy; s.lx = x - fx; s.hy = 1.0f - s.ly; s.hx = 1.0f - s.lx;
    s.w[0] = s.hy * s.hx; s.w[1] = s.hy * s.lx; s.w[2] = s.ly * s.hx; s.w[3] = s.ly * s.lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
        if (yy < 0 || yy > lv.h - 1 || xx < 0 || xx > lv.w - 1) continue;
        const long long c = lv.start + (long long)yy * lv.w + xx;
        if (c >= 0 && c < S) s.cell[k] = c;
    }
    return s;
}

// the tensors of one call as the sampling kernels see them
struct MsDims { long long items, S; int QM, M, D, L, P, T, nruns, ipb; };

// ---- forward -------------------------------------------------------------------------------------------------------------------------
template <typename E, int R, int PASSES>
__global__ __launch_bounds__(MSDA_BLOCK)
void msda_forward_kernel(const E* __restrict__ value, const long long* __restrict__ shapes, const long long* __restrict__ starts,
                         const float* __restrict__ loc, const float* __restrict__ attn, MsDims g, E* __restrict__ out)
{
    __shared__ float s_loc[2 * MSDA_LDS_SAMPLES];
    __shared__ float s_w[MSDA_LDS_SAMPLES];
    const int LP = g.L * g.P;
    const long long item0 = (long long)blockIdx.x * g.ipb;
    const long long left = g.items - item0;
    const int n_here = left < g.ipb ? (int)left : g.ipb;
    for (int i = threadIdx.x; i < n_here * LP * 2; i += blockDim.x) s_loc[i] = loc[item0 * LP * 2 + i];
    for (int i = threadIdx.x; i < n_here * LP; i += blockDim.x) s_w[i] = attn[item0 * LP + i];
    __syncthreads();
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    if (grp >= n_here) return;
    const long long item = item0 + grp;
    const int m = (int)(item % g.M);
    const long long b = item / g.QM;
    const size_t cell_stride = (size_t)g.M * g.D;
    const E* const vb = value + ((size_t)b * g.S * g.M + m) * g.D;
    MsVec<R> acc[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[it].v[j] = 0.f;
    for (int l = 0; l < g.L; ++l) {
        const MsLevel lv = ms_level(shapes, starts, l, g.S);
        for (int p = 0; p < g.P; ++p) {
            const int si = grp * LP + l * g.P + p;
            const MsSample s = ms_sample(lv, s_loc[2 * si], s_loc[2 * si + 1], g.S);
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
                    const float val = s.w[0] * v[0].v[j] + s.w[1] * v[1].v[j] + s.w[2] * v[2].v[j] + s.w[3] * v[3].v[j];
                    acc[it].v[j] += aw * val;
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int run = t + it * g.T;
        if (run < g.nruns) ms_store<E, R>(out + (size_t)item * g.D + (size_t)run * R, acc[it]);
    }
}

// ---- d_loc, d_attn -----------------------------------------------------------------------------------------------------------------------
template <typename E, int R, int PASSES>
__global__ __launch_bounds__(MSDA_BLOCK)
void msda_backward_loc_kernel(const E* __restrict__ value, const long long* __restrict__ shapes, const long long* __restrict__ starts,
                              const float* __restrict__ loc, const float* __restrict__ attn, const E* __restrict__ dout, MsDims g,
                              float* __restrict__ dloc, float* __restrict__ dattn)
{
    __shared__ float s_loc[2 * MSDA_LDS_SAMPLES];
    __shared__ float s_w[MSDA_LDS_SAMPLES];
    const int LP = g.L * g.P;
    const long long item0 = (long long)blockIdx.x * g.ipb;
    const long long left = g.items - item0;
    const int n_here = left < g.ipb ? (int)left : g.ipb;
    for (int i = threadIdx.x; i < n_here * LP * 2; i += blockDim.x) s_loc[i] = loc[item0 * LP * 2 + i];
    for (int i = threadIdx.x; i < n_here * LP; i += blockDim.x) s_w[i] = attn[item0 * LP + i];
    __syncthreads();
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    const bool active = grp < n_here;                     // an idle group still takes part in the butterflies of its wave
    const long long item = active ? item0 + grp : item0;
    const int m = (int)(item % g.M);
    const long long b = item / g.QM;
    const size_t cell_stride = (size_t)g.M * g.D;
    const E* const vb = value + ((size_t)b * g.S * g.M + m) * g.D;
    MsVec<R> gr[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int run = t + it * g.T;
        if (active && run < g.nruns) {
            gr[it] = ms_load<E, R>(dout + (size_t)item * g.D + (size_t)run * R);
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) gr[it].v[j] = 0.f;
        }
    }
    for (int l = 0; l < g.L; ++l) {
        const MsLevel lv = ms_level(shapes, starts, l, g.S);
        for (int p = 0; p < g.P; ++p) {
            const int si = active ? grp * LP + l * g.P + p : 0;
            const MsSample s = ms_sample(lv, s_loc[2 * si], s_loc[2 * si + 1], g.S);
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
                        const float val = s.w[0] * v[0].v[j] + s.w[1] * v[1].v[j] + s.w[2] * v[2].v[j] + s.w[3] * v[3].v[j];
                        // the slopes of the published backward: the validly indexed corners, the right-hand slope at an integer
                        const float gy = ((0.f - s.hx * v[0].v[j]) - s.lx * v[1].v[j]) + s.hx * v[2].v[j] + s.lx * v[3].v[j];
                        const float gx = ((0.f - s.hy * v[0].v[j]) + s.hy * v[1].v[j]) - s.ly * v[2].v[j] + s.ly * v[3].v[j];
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
                const size_t o = (size_t)item * LP + l * g.P + p;
                if (dattn) dattn[o] = pw;
                if (dloc) { dloc[2 * o] = (float)lv.w * px; dloc[2 * o + 1] = (float)lv.h * py; }
            }
        }
    }
}

// ---- d_value: plan, segment starts, gather ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MSDA_BLOCK)
void msda_plan_kernel(const long long* __restrict__ shapes, const long long* __restrict__ starts, const float* __restrict__ loc,
                      const float* __restrict__ attn, long long total, long long S, int QM, int M, int L, int P, long long sentinel,
                      long long* __restrict__ keys, float* __restrict__ wts)
{
    const int LP = L * P;
    for (long long idx = (long long)blockIdx.x * MSDA_BLOCK + threadIdx.x; idx < total; idx += (long long)gridDim.x * MSDA_BLOCK) {
        const long long item = idx / LP;
        const int l = (int)(idx - item * LP) / P;
        const int m = (int)(item % M);
        const long long b = item / QM;
        const MsLevel lv = ms_level(shapes, starts, l, S);
        const MsSample s = ms_sample(lv, loc[2 * idx], loc[2 * idx + 1], S);
        const float aw = attn[idx];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            keys[4 * idx + k] = s.cell[k] >= 0 ? (b * S + s.cell[k]) * M + m : sentinel;
            wts[4 * idx + k] = s.cell[k] >= 0 ? s.w[k] * aw : 0.f;
        }
    }
}

// start[c] = the first position of the sorted keys that holds a key >= c, for c in [0, n_cells]
__global__ __launch_bounds__(MSDA_BLOCK)
void msda_segments_kernel(const long long* __restrict__ sorted_keys, int n_entries, int n_cells, int* __restrict__ start)
{
    for (long long c = (long long)blockIdx.x * MSDA_BLOCK + threadIdx.x; c <= n_cells; c += (long long)gridDim.x * MSDA_BLOCK) {
        int lo = 0, hi = n_entries;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (sorted_keys[mid] < c) lo = mid + 1; else hi = mid;
        }
        start[c] = lo;
    }
}

// what the two kernels of the value gradient share
struct MsGather { int n_cells, n_entries, D, LP4, T, nruns, n_windows; };

// acc += the sum over the sorted positions [i0, i1), ascending, of weight * dout[item][:] for the lane's runs
template <typename E, int R, int PASSES>
__device__ __forceinline__ void ms_sum_entries(const long long* __restrict__ order, const float* __restrict__ wts,
                                               const E* __restrict__ dout, const MsGather& g, int t, int i0, int i1, MsVec<R>* acc)
{
    for (int i = i0; i < i1; ++i) {
        const long long e = order[i];
        if (e < 0 || e >= g.n_entries) continue;                      // a permutation of [0, n_entries) by contract
        const float w = wts[e];
        const E* const gp = dout + (size_t)(e / g.LP4) * g.D;
#pragma unroll
        for (int it = 0; it < PASSES; ++it) {
            const int run = t + it * g.T;
            if (run >= g.nruns) continue;
            const MsVec<R> gv = ms_load<E, R>(gp + (size_t)run * R);
#pragma unroll
            for (int j = 0; j < R; ++j) acc[it].v[j] += w * gv.v[j];
        }
    }
}

// the segment of cell c in the sorted keys, clamped to the array (the starts come from the caller's sorted keys)
__device__ __forceinline__ void ms_segment(const int* __restrict__ start, int c, int n_entries, int& i0, int& i1)
{
    i0 = start[c]; i1 = start[c + 1];
    i0 = i0 < 0 ? 0 : i0; i1 = i1 > n_entries ? n_entries : i1;
}

// One group of T lanes per (window w of MSDA_SEGMENT sorted positions, slot): slot 0 serves the segment that holds the window's first
// position, slot 1 the segment that holds its last position when that is another one.  If the segment is long and one of its pieces
// (cut from the segment's own start) begins inside the window, the group sums that piece into partial[2 w + slot][:].
template <typename E, int R, int PASSES>
__global__ __launch_bounds__(MSDA_BLOCK)
void msda_value_pieces_kernel(const int* __restrict__ start, const long long* __restrict__ sorted_keys,
                              const long long* __restrict__ order, const float* __restrict__ wts, const E* __restrict__ dout, MsGather g,
                              float* __restrict__ partial)
{
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    const long long item = (long long)blockIdx.x * (MSDA_BLOCK / g.T) + grp;
    if (item >= 2LL * g.n_windows) return;
    const int w = (int)(item >> 1), slot = (int)(item & 1);
    const int lo = w * MSDA_SEGMENT, hi = g.n_entries - lo < MSDA_SEGMENT ? g.n_entries : lo + MSDA_SEGMENT;
    const long long c = sorted_keys[slot ? hi - 1 : lo];
    if (c < 0 || c >= g.n_cells) return;                              // the sentinel: corners that count 0
    if (slot == 1 && sorted_keys[lo] == c) return;                    // one segment spans the window: slot 0 serves it
    int i0, i1;
    ms_segment(start, (int)c, g.n_entries, i0, i1);
    if (i1 - i0 <= MSDA_SEGMENT) return;
    const int k = i0 >= lo ? 0 : (lo - i0 + MSDA_SEGMENT - 1) / MSDA_SEGMENT;
    const int ps = i0 + k * MSDA_SEGMENT;                             // the first piece that begins at or after lo
    if (ps >= hi || ps >= i1) return;
    const int pe = i1 - ps < MSDA_SEGMENT ? i1 : ps + MSDA_SEGMENT;
    MsVec<R> acc[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[it].v[j] = 0.f;
    ms_sum_entries<E, R, PASSES>(order, wts, dout, g, t, ps, pe, acc);
    float* const row = partial + (size_t)item * g.D;
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int run = t + it * g.T;
        if (run >= g.nruns) continue;
#pragma unroll
        for (int j = 0; j < R; ++j) row[run * R + j] = acc[it].v[j];
    }
}

// one group of T lanes per c = (b S + cell) M + m; d_value[c][:] = the sum over the cell's entries, ascending, of weight * dout[item][:]:
// directly for a segment of at most MSDA_SEGMENT entries, else the sums of its pieces in ascending order
template <typename E, int R, int PASSES>
__global__ __launch_bounds__(MSDA_BLOCK)
void msda_value_grad_kernel(const int* __restrict__ start, const long long* __restrict__ sorted_keys,
                            const long long* __restrict__ order, const float* __restrict__ wts, const E* __restrict__ dout, MsGather g,
                            const float* __restrict__ partial, E* __restrict__ dvalue)
{
    const int grp = threadIdx.x / g.T, t = threadIdx.x - grp * g.T;
    const long long c = (long long)blockIdx.x * (MSDA_BLOCK / g.T) + grp;
    if (c >= g.n_cells) return;
    int i0, i1;
    ms_segment(start, (int)c, g.n_entries, i0, i1);
    MsVec<R> acc[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[it].v[j] = 0.f;
    if (i1 - i0 <= MSDA_SEGMENT) {
        ms_sum_entries<E, R, PASSES>(order, wts, dout, g, t, i0, i1, acc);
    } else {
        for (int ps = i0; ps < i1; ps += MSDA_SEGMENT) {
            const int w = ps / MSDA_SEGMENT;
            const int slot = sorted_keys[(size_t)w * MSDA_SEGMENT] == c ? 0 : 1;
            const float* const row = partial + ((size_t)2 * w + slot) * g.D;
#pragma unroll
            for (int it = 0; it < PASSES; ++it) {
                const int run = t + it * g.T;
                if (run >= g.nruns) continue;
#pragma unroll
                for (int j = 0; j < R; ++j) acc[it].v[j] += row[run * R + j];
            }
        }
    }
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int run = t + it * g.T;
        if (run < g.nruns) ms_store<E, R>(dvalue + (size_t)c * g.D + (size_t)run * R, acc[it]);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static bool msda_args_ok(int n_img, int s, int m, int d, int q, int levels, int points)
{
    if (n_img < 1 || s < 1 || m < 1 || q < 1 || d < 1 || d > MSDA_MAX_CHANNELS) return false;
    if (levels < 1 || levels > MSDA_MAX_LEVELS || points < 1 || points > MSDA_MAX_POINTS) return false;
    if ((long long)n_img * s > MSDA_MAX_INDEX / m) return false;                              // cells: n S M
    const long long lp4 = 4LL * levels * points;
    if ((long long)n_img * q > MSDA_MAX_INDEX / m / lp4) return false;                         // plan entries: n Q M L P 4
    return true;
}

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int msda_windows(int n_entries) { return (n_entries + MSDA_SEGMENT - 1) / MSDA_SEGMENT; }

// the segment starts, then two rows of d float32 per window of MSDA_SEGMENT sorted entries (the sums of the long segments' pieces)
static inline size_t msda_starts_bytes(int n_cells) { return align256(((size_t)n_cells + 1) * sizeof(int)); }

size_t msda_gather_workspace(int n_cells, int n_entries, int d)
{
    return msda_starts_bytes(n_cells) + align256((size_t)msda_windows(n_entries) * 2 * d * sizeof(float));
}

template <typename E>
static int msda_forward_impl(const void* value, const int64_t* shapes, const int64_t* starts, const float* loc, const float* attn,
                             int n_img, int s, int m, int d, int q, int levels, int points, void* out, void* stream)
{
    if (!msda_args_ok(n_img, s, m, d, q, levels, points) || !value || !shapes || !starts || !loc || !attn || !out) return FRCNN_EINVAL;
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = d % RUN == 0 && aligned16(value) && aligned16(out);
    const MsMap mp = ms_map(d, levels * points, RUN, vector);
    const MsDims g = {(long long)n_img * q * m, (long long)s, q * m, m, d, levels, points, mp.T, mp.nruns, mp.ipb};
    const dim3 grid((unsigned)((g.items + mp.ipb - 1) / mp.ipb)), block(mp.threads);
    const long long* sh = reinterpret_cast<const long long*>(shapes);
    const long long* st = reinterpret_cast<const long long*>(starts);
    if (vector)
        hipLaunchKernelGGL((msda_forward_kernel<E, RUN, 1>), grid, block, 0, (hipStream_t)stream, static_cast<const E*>(value), sh, st, loc,
                           attn, g, static_cast<E*>(out));
    else
        hipLaunchKernelGGL((msda_forward_kernel<E, 1, MSDA_SCALAR_PASSES>), grid, block, 0, (hipStream_t)stream,
                           static_cast<const E*>(value), sh, st, loc, attn, g, static_cast<E*>(out));
    return check_launch();
}

template <typename E>
static int msda_backward_loc_impl(const void* value, const int64_t* shapes, const int64_t* starts, const float* loc, const float* attn,
                                  const void* dout, int n_img, int s, int m, int d, int q, int levels, int points, float* dloc,
                                  float* dattn, void* stream)
{
    if (!msda_args_ok(n_img, s, m, d, q, levels, points) || !value || !shapes || !starts || !loc || !attn || !dout) return FRCNN_EINVAL;
    if (!dloc && !dattn) return FRCNN_EINVAL;
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = d % RUN == 0 && aligned16(value) && aligned16(dout);
    const MsMap mp = ms_map(d, levels * points, RUN, vector);
    const MsDims g = {(long long)n_img * q * m, (long long)s, q * m, m, d, levels, points, mp.T, mp.nruns, mp.ipb};
    const dim3 grid((unsigned)((g.items + mp.ipb - 1) / mp.ipb)), block(mp.threads);
    const long long* sh = reinterpret_cast<const long long*>(shapes);
    const long long* st = reinterpret_cast<const long long*>(starts);
    if (vector)
        hipLaunchKernelGGL((msda_backward_loc_kernel<E, RUN, 1>), grid, block, 0, (hipStream_t)stream, static_cast<const E*>(value), sh, st,
                           loc, attn, static_cast<const E*>(dout), g, dloc, dattn);
    else
        hipLaunchKernelGGL((msda_backward_loc_kernel<E, 1, MSDA_SCALAR_PASSES>), grid, block, 0, (hipStream_t)stream,
                           static_cast<const E*>(value), sh, st, loc, attn, static_cast<const E*>(dout), g, dloc, dattn);
    return check_launch();
}

// the gather uses the samples of an item only as their number: multi-scale deformable attention has levels * points of them, DCNv3
// kh * kw
template <typename E>
static int msda_gather_impl(const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout, int n_cells,
                            int n_entries, int samples4, int d, void* dvalue, void* ws, size_t ws_bytes, hipStream_t st)
{
    if (!sorted_keys || !order || !wts || !dout || !dvalue) return FRCNN_EINVAL;
    if (!ws || !aligned16(ws) || ws_bytes < msda_gather_workspace(n_cells, n_entries, d)) return FRCNN_EINVAL;
    constexpr int RUN = MsElem<E>::RUN;
    const bool vector = d % RUN == 0 && aligned16(dvalue) && aligned16(dout);
    const MsMap mp = ms_map(d, samples4 / 4, RUN, vector);
    MsGather g;
    g.n_cells = n_cells; g.LP4 = samples4; g.n_entries = n_entries; g.D = d; g.T = mp.T; g.nruns = mp.nruns;
    g.n_windows = msda_windows(g.n_entries);
    int* start = static_cast<int*>(ws);
    float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + msda_starts_bytes(n_cells));
    const long long* keys = reinterpret_cast<const long long*>(sorted_keys);
    const long long* ord = reinterpret_cast<const long long*>(order);
    hipLaunchKernelGGL(msda_segments_kernel, dim3(msda_blocks((long long)g.n_cells + 1)), dim3(MSDA_BLOCK), 0, st, keys, g.n_entries,
                       g.n_cells, start);
    int rc = check_launch();
    if (rc != FRCNN_OK) return rc;
    const int per_block = MSDA_BLOCK / mp.T;
    const dim3 block(MSDA_BLOCK), pieces((unsigned)((2LL * g.n_windows + per_block - 1) / per_block));
    const dim3 cells((unsigned)((g.n_cells + per_block - 1) / per_block));
    const E* gout = static_cast<const E*>(dout);
    if (vector) {
        hipLaunchKernelGGL((msda_value_pieces_kernel<E, RUN, 1>), pieces, block, 0, st, start, keys, ord, wts, gout, g, partial);
        if ((rc = check_launch()) != FRCNN_OK) return rc;
        hipLaunchKernelGGL((msda_value_grad_kernel<E, RUN, 1>), cells, block, 0, st, start, keys, ord, wts, gout, g, partial,
                           static_cast<E*>(dvalue));
    } else {
        hipLaunchKernelGGL((msda_value_pieces_kernel<E, 1, MSDA_SCALAR_PASSES>), pieces, block, 0, st, start, keys, ord, wts, gout, g,
                           partial);
        if ((rc = check_launch()) != FRCNN_OK) return rc;
        hipLaunchKernelGGL((msda_value_grad_kernel<E, 1, MSDA_SCALAR_PASSES>), cells, block, 0, st, start, keys, ord, wts, gout, g, partial,
                           static_cast<E*>(dvalue));
    }
    return check_launch();
}

int msda_gather(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout, int n_cells,
                int n_entries, int samples4, int d, void* dvalue, void* ws, size_t ws_bytes, hipStream_t stream)
{
    if (n_cells < 1 || n_entries < 1 || samples4 < 4 || d < 1 || d > MSDA_MAX_CHANNELS) return FRCNN_EINVAL;
    if (elem_type == 0)
        return msda_gather_impl<float>(sorted_keys, order, wts, dout, n_cells, n_entries, samples4, d, dvalue, ws, ws_bytes, stream);
    OPS_ELEM_DISPATCH(elem_type, E,
                      msda_gather_impl<E>(sorted_keys, order, wts, dout, n_cells, n_entries, samples4, d, dvalue, ws, ws_bytes, stream));
}

static int msda_backward_value(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout,
                               int n_img, int s, int m, int d, int q, int levels, int points, void* dvalue, void* ws, size_t ws_bytes,
                               void* stream)
{
    if (!msda_args_ok(n_img, s, m, d, q, levels, points)) return FRCNN_EINVAL;
    const int lp4 = levels * points * 4;
    return msda_gather(elem_type, sorted_keys, order, wts, dout, n_img * s * m, n_img * q * m * lp4, lp4, d, dvalue, ws, ws_bytes,
                       (hipStream_t)stream);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_msda_max_levels(void) { return MSDA_MAX_LEVELS; }
int frcnn_ops_msda_max_points(void) { return MSDA_MAX_POINTS; }
int frcnn_ops_msda_max_channels(void) { return MSDA_MAX_CHANNELS; }

int frcnn_ops_msda_block_items(int d, int levels, int points, int elem_type)
{
    if (d < 1 || d > MSDA_MAX_CHANNELS || levels < 1 || levels > MSDA_MAX_LEVELS || points < 1 || points > MSDA_MAX_POINTS) return 0;
    if (elem_type != 0 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return 0;
    const int run = elem_type == 0 ? MsElem<float>::RUN : MsElem<f16>::RUN;
    return ms_map(d, levels * points, run, d % run == 0).ipb;
}

int frcnn_ops_msda_segment(void) { return MSDA_SEGMENT; }

size_t frcnn_ops_msda_workspace_bytes(int n_img, int s, int m, int d, int q, int levels, int points)
{
    if (!msda_args_ok(n_img, s, m, d, q, levels, points)) return 0;
    return msda_gather_workspace(n_img * s * m, n_img * q * m * levels * points * 4, d);
}

int frcnn_ops_msda_forward(const float* d_value, const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc, const float* d_attn,
                           int n_img, int s, int m, int d, int q, int levels, int points, float* d_out, void* stream)
{
    return msda_forward_impl<float>(d_value, d_shapes, d_starts, d_loc, d_attn, n_img, s, m, d, q, levels, points, d_out, stream);
}

int frcnn_ops_msda_backward_loc(const float* d_value, const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc,
                                const float* d_attn, const float* d_dout, int n_img, int s, int m, int d, int q, int levels, int points,
                                float* d_dloc, float* d_dattn, void* stream)
{
    return msda_backward_loc_impl<float>(d_value, d_shapes, d_starts, d_loc, d_attn, d_dout, n_img, s, m, d, q, levels, points, d_dloc,
                                         d_dattn, stream);
}

int frcnn_ops_msda_plan(const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc, const float* d_attn, int n_img, int s, int m,
                        int q, int levels, int points, int64_t* d_keys, float* d_weights, void* stream)
{
    if (!msda_args_ok(n_img, s, m, 1, q, levels, points) || !d_shapes || !d_starts || !d_loc || !d_attn || !d_keys || !d_weights)
        return FRCNN_EINVAL;
    const long long total = (long long)n_img * q * m * levels * points;
    hipLaunchKernelGGL(msda_plan_kernel, dim3(msda_blocks(total)), dim3(MSDA_BLOCK), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(d_shapes), reinterpret_cast<const long long*>(d_starts), d_loc, d_attn, total,
                       (long long)s, q * m, m, levels, points, (long long)n_img * s * m, reinterpret_cast<long long*>(d_keys), d_weights);
    return check_launch();
}

int frcnn_ops_msda_backward_value(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                  int n_img, int s, int m, int d, int q, int levels, int points, float* d_dvalue, void* d_ws,
                                  size_t ws_bytes, void* stream)
{
    return msda_backward_value(0, d_sorted_keys, d_order, d_weights, d_dout, n_img, s, m, d, q, levels, points, d_dvalue, d_ws, ws_bytes,
                               stream);
}

int frcnn_ops_msda_forward_16(int elem_type, const void* d_value, const int64_t* d_shapes, const int64_t* d_starts, const float* d_loc,
                              const float* d_attn, int n_img, int s, int m, int d, int q, int levels, int points, void* d_out,
                              void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, msda_forward_impl<E>(d_value, d_shapes, d_starts, d_loc, d_attn, n_img, s, m, d, q, levels, points,
                                                         d_out, stream));
}

int frcnn_ops_msda_backward_loc_16(int elem_type, const void* d_value, const int64_t* d_shapes, const int64_t* d_starts,
                                   const float* d_loc, const float* d_attn, const void* d_dout, int n_img, int s, int m, int d, int q,
                                   int levels, int points, float* d_dloc, float* d_dattn, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, msda_backward_loc_impl<E>(d_value, d_shapes, d_starts, d_loc, d_attn, d_dout, n_img, s, m, d, q,
                                                              levels, points, d_dloc, d_dattn, stream));
}

int frcnn_ops_msda_backward_value_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                     const void* d_dout, int n_img, int s, int m, int d, int q, int levels, int points, void* d_dvalue,
                                     void* d_ws, size_t ws_bytes, void* stream)
{
    if (elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    return msda_backward_value(elem_type, d_sorted_keys, d_order, d_weights, d_dout, n_img, s, m, d, q, levels, points, d_dvalue, d_ws,
                               ws_bytes, stream);
}

}  // extern "C"
