// ops_softnms.hip -- Soft-NMS (Bodla et al., 2017: naive, linear and gaussian rescoring), per label: the frcnn_ops_soft_nms* entry
// points of include/frcnn_hip.h, which states the contract (mmcv's CPU-only soft_nms restated, unpinned).
//
// The algorithm is a chain of dependent picks -- pick t + 1 needs the scores pick t left behind -- so the design is about the cost of
// one pick and about running the labels side by side:
//   * One workgroup owns one problem (one label's run of d_order) from its first pick to its last.  Workgroups never talk to each
//     other: no grid barrier, no ticket, no spin-wait.  Every loop is bounded by the problem's length (each pick takes one box out of
//     the live set, the pick loop runs at most len times), so the kernel terminates on any input, NaNs and arbitrary labels included.
//   * A pick costs ONE pass over the live boxes of the problem and ONE block-wide argmax, fused: while a thread rescales its boxes
//     with pick t it keeps, in registers, its best box for pick t + 1.  The argmax key packs (not-NaN, score, lower position) into 64
//     bits, monotonically; positions are distinct, so the key is a total order and its maximum does not depend on the shape of the
//     reduction tree: six xor-shuffles inside a wave, then each wave's winner -- key and box -- goes to one LDS slot, one barrier,
//     and every thread reads the SNMS_WAVES slots.  The slots are double-buffered by the pick's parity, which is what makes one
//     barrier a pick enough: the writers of pick t + 1 use the other buffer, and nobody writes this one before the barrier of t + 1.
//     (Reducing the 32-bit score half alone, with a second reduction of the position only when lanes tie, was measured: 1.66 ms
//     against 1.71 ms for 4000 boxes -- the pass, not the reduction, is the larger part of a pick -- and not kept.)
//   * Thread i owns the boxes at positions i, i + T, i + 2 T, ... of its problem and nobody else ever touches them, so the state
//     (corners, area, score, position) needs no synchronisation at all, and a thread compacts its own list in place, stably, in the
//     same pass that rescales it: a dropped or picked box is simply not written back.  The pass therefore walks live boxes only,
//     SNMS_CHUNK list entries at a time with their loads issued together (the stores of an entry only go to slots at or before it).
//   * The state lives in LDS for problems of up to SNMS_LDS_BOXES boxes (7 words a box: 112 KB of the CU's 160 KB), in the caller's
//     workspace above that (same code, same slots; the workspace slice of a problem is its run of positions, private to its block).
//   * A problem of at most 64 boxes is one box a lane: wave 0 runs it in registers with shuffles only, no LDS and no barrier -- what
//     many-label inputs consist of.
//   * Problems are found as ops_nms_reduce_kernel finds its segments, in parallel: block b owns the candidate positions b + i grid,
//     one lane each (n <= 65536 = 64 x 1024), a ballot gives the starts among them and a block without one exits at once.
// Within a problem d_order is ascending in the box index, so "ties to the smaller index" is "ties to the smaller position".
// All stores are ordinary vector stores from plain C++.
#include "common.h"
#include <math.h>

namespace frcnn {

typedef unsigned long long snms_key_t;

static constexpr int SNMS_THREADS = 512;
static constexpr int SNMS_WAVES = SNMS_THREADS / 64;
static constexpr int SNMS_LDS_BOXES = 4096;      // 7 words a box in LDS
static constexpr int SNMS_MAX_BOXES = 65536;
static constexpr int SNMS_GRID = 1024;           // blocks of a labelled launch: ceil(n / 1024) <= 64 candidate starts a block, one a lane
static constexpr int SNMS_WORDS = 7;             // x1, y1, x2, y2, area, score, position
static constexpr int SNMS_CHUNK = 4;             // boxes of a thread's list whose loads are issued together
static_assert(SNMS_MAX_BOXES <= 64 * SNMS_GRID, "a block's candidate starts fit one ballot");
static_assert(SNMS_LDS_BOXES % SNMS_THREADS == 0, "whole slots per thread");

struct SnmsParams {
    float thr, sigma, min_score, off;
    int method;                                  // 0 naive, 1 linear, 2 gaussian
};

struct SnmsBox { float x1, y1, x2, y2, area, s; };

struct SnmsState { float *x1, *y1, *x2, *y2, *area, *s; int* pos; };

// (not-NaN, score, lower position) as one integer, larger is better; 0 is "no box".  -0 and +0 are one score.
__device__ __forceinline__ snms_key_t snms_key(float s, int pos)
{
    unsigned u = __float_as_uint(s), k = 1u;                               // every NaN: below -inf (0x007FFFFF), above "no box"
    if (s == s) {
        if (s == 0.f) u = 0u;
        k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((snms_key_t)k << 32) | (unsigned)(0x7fffffff - pos);
}

__device__ __forceinline__ int snms_key_pos(snms_key_t k) { return 0x7fffffff - (int)(unsigned)(k & 0xffffffffull); }

__device__ __forceinline__ snms_key_t snms_wave_max(snms_key_t k)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const snms_key_t o = __shfl_xor(k, m);
        k = o > k ? o : k;
    }
    return k;
}

// the weight pick p puts on box b: every operation rounded on its own (-ffp-contract=off), the division IEEE
__device__ __forceinline__ float snms_weight(const SnmsParams& a, const SnmsBox& p, const SnmsBox& b)
{
    const float w = fmaxf(0.f, fminf(p.x2, b.x2) - fmaxf(p.x1, b.x1) + a.off);
    const float h = fmaxf(0.f, fminf(p.y2, b.y2) - fmaxf(p.y1, b.y1) + a.off);
    const float inter = w * h;
    float ovr = inter / ((p.area + b.area) - inter);
    if (ovr != ovr) ovr = 0.f;
    if (a.method == 2) return expf(-(ovr * ovr) / a.sigma);
    if (ovr >= a.thr) return a.method == 1 ? 1.f - ovr : 0.f;
    return 1.f;
}

__device__ __forceinline__ SnmsBox snms_load(const float* __restrict__ boxes, const float* __restrict__ scores, int64_t idx, float off)
{
    const float* v = boxes + (size_t)idx * 4;
    SnmsBox b;
    b.x1 = v[0]; b.y1 = v[1]; b.x2 = v[2]; b.y2 = v[3];
    b.area = (b.x2 - b.x1 + off) * (b.y2 - b.y1 + off);
    b.s = scores[idx];
    return b;
}

// A problem of len <= 64 boxes in the registers of one whole wave: lane j holds the box at position s0 + j.
__device__ __forceinline__ void snms_wave(const float* __restrict__ boxes, const float* __restrict__ scores,
                                          const int64_t* __restrict__ order, int s0, int len, const SnmsParams& a,
                                          float* __restrict__ scores_out, uint8_t* __restrict__ keep)
{
    const int lane = threadIdx.x & 63;
    bool live = lane < len;
    SnmsBox b = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) b = snms_load(boxes, scores, order[s0 + lane], a.off);
    for (int t = 0; t < len; ++t) {
        const snms_key_t best = snms_wave_max(live ? snms_key(b.s, lane) : 0ull);
        if (best == 0ull) break;                                             // wave-uniform
        const int pl = snms_key_pos(best);
        SnmsBox p;
        p.x1 = __shfl(b.x1, pl); p.y1 = __shfl(b.y1, pl); p.x2 = __shfl(b.x2, pl); p.y2 = __shfl(b.y2, pl); p.area = __shfl(b.area, pl);
        p.s = 0.f;
        if (!live) continue;
        bool out = lane == pl;
        if (!out) {
            b.s = b.s * snms_weight(a, p, b);
            out = b.s < a.min_score;
        }
        if (out) {
            live = false;
            keep[s0 + lane] = (uint8_t)(lane == pl);
            scores_out[s0 + lane] = b.s;
        }
    }
}

// A problem of any length on the whole block; st: the problem's state slots [0, len), slot k T + i owned by thread i.
__device__ __forceinline__ void snms_block(const SnmsState st, const float* __restrict__ boxes, const float* __restrict__ scores,
                                           const int64_t* __restrict__ order, int s0, int len, const SnmsParams& a,
                                           float* __restrict__ scores_out, uint8_t* __restrict__ keep,
                                           snms_key_t (*slot_key)[SNMS_WAVES], SnmsBox (*slot_box)[SNMS_WAVES])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0;
    snms_key_t bk = 0ull;                                                   // this thread's best live box, for the next pick
    SnmsBox bb = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = tid; j < len; j += SNMS_THREADS, ++cnt) {
        const SnmsBox b = snms_load(boxes, scores, order[s0 + j], a.off);
        st.x1[j] = b.x1; st.y1[j] = b.y1; st.x2[j] = b.x2; st.y2[j] = b.y2; st.area[j] = b.area; st.s[j] = b.s; st.pos[j] = j;
        const snms_key_t k = snms_key(b.s, j);
        if (k > bk) { bk = k; bb = b; }
    }
    for (int t = 0; t < len; ++t) {
        const int par = t & 1;
        const snms_key_t wk = snms_wave_max(bk);
        if (wk == 0ull) {
            if (lane == 0) slot_key[par][wave] = 0ull;
        } else if (bk == wk) {                                              // one lane: positions are distinct
            slot_key[par][wave] = wk;
            slot_box[par][wave] = bb;
        }
        __syncthreads();
        snms_key_t best = 0ull;
        int bw = 0;
#pragma unroll
        for (int w = 0; w < SNMS_WAVES; ++w) {
            const snms_key_t k = slot_key[par][w];
            if (k > best) { best = k; bw = w; }
        }
        if (best == 0ull) break;                                             // block-uniform: the live set is empty
        const int ppos = snms_key_pos(best);
        const SnmsBox p = slot_box[par][bw];
        bk = 0ull;
        int w = 0;
        for (int k0 = 0; k0 < cnt; k0 += SNMS_CHUNK) {
            // the chunk's loads first, all in flight together: the stores below go to slots <= the one being handled, never to a later one
            SnmsBox cb[SNMS_CHUNK];
            int cpos[SNMS_CHUNK];
#pragma unroll
            for (int u = 0; u < SNMS_CHUNK; ++u) {
                const int src = (k0 + u) * SNMS_THREADS + tid;
                if (k0 + u < cnt) {
                    cpos[u] = st.pos[src];
                    cb[u].x1 = st.x1[src]; cb[u].y1 = st.y1[src]; cb[u].x2 = st.x2[src]; cb[u].y2 = st.y2[src];
                    cb[u].area = st.area[src]; cb[u].s = st.s[src];
                }
            }
#pragma unroll
            for (int u = 0; u < SNMS_CHUNK; ++u) {
                if (k0 + u >= cnt) break;
                const int src = (k0 + u) * SNMS_THREADS + tid;
                const int pos = cpos[u];
                SnmsBox b = cb[u];
                bool out = pos == ppos;
                if (!out) {
                    b.s = b.s * snms_weight(a, p, b);
                    out = b.s < a.min_score;
                }
                if (out) {                                                   // picked (kept with its current score) or dropped
                    keep[s0 + pos] = (uint8_t)(pos == ppos);
                    scores_out[s0 + pos] = b.s;
                    continue;
                }
                const int dst = w * SNMS_THREADS + tid;                      // dst <= src: the thread's own, stable compaction
                if (dst != src) { st.x1[dst] = b.x1; st.y1[dst] = b.y1; st.x2[dst] = b.x2; st.y2[dst] = b.y2; st.area[dst] = b.area; st.pos[dst] = pos; }
                st.s[dst] = b.s;
                const snms_key_t key = snms_key(b.s, pos);
                if (key > bk) { bk = key; bb = b; }
                ++w;
            }
        }
        cnt = w;
    }
    __syncthreads();                                                         // the slots are free for the block's next problem
}

__global__ __launch_bounds__(SNMS_THREADS)
void ops_soft_nms_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const int64_t* __restrict__ order,
                         const int64_t* __restrict__ cats, int n, SnmsParams a, float* __restrict__ scores_out,
                         uint8_t* __restrict__ keep, float* __restrict__ ws)
{
    __shared__ float lds[SNMS_WORDS][SNMS_LDS_BOXES];
    __shared__ snms_key_t slot_key[2][SNMS_WAVES];
    __shared__ SnmsBox slot_box[2][SNMS_WAVES];
    const int lane = threadIdx.x & 63;
    // the starts among this block's candidate positions: the same ballot in every wave
    const int cand = (int)blockIdx.x + lane * (int)gridDim.x;
    snms_key_t starts = __ballot(cand < n && (!cats || cand == 0 || cats[order[cand]] != cats[order[cand - 1]]));
    if (!cats) starts &= blockIdx.x == 0 ? 1ull : 0ull;                      // no labels: one problem
    while (starts) {
        const int s0 = (int)blockIdx.x + (__ffsll((long long)starts) - 1) * (int)gridDim.x;
        starts &= starts - 1ull;
        int s1 = n;
        if (cats) {
            const int64_t cat = cats[order[s0]];
            for (int base = s0 + 1; base < n; base += 64) {
                const int j = base + lane;
                const snms_key_t m = __ballot(j < n && cats[order[j]] != cat);
                if (m) { s1 = base + __ffsll((long long)m) - 1; break; }
            }
        }
        const int len = s1 - s0;
        if (len <= 64) {
            if (threadIdx.x < 64) snms_wave(boxes, scores, order, s0, len, a, scores_out, keep);
        } else if (len <= SNMS_LDS_BOXES) {
            const SnmsState st = {lds[0], lds[1], lds[2], lds[3], lds[4], lds[5], reinterpret_cast<int*>(lds[6])};
            snms_block(st, boxes, scores, order, s0, len, a, scores_out, keep, slot_key, slot_box);
        } else {
            float* g = ws + s0;
            const size_t m = (size_t)n;
            const SnmsState st = {g, g + m, g + 2 * m, g + 3 * m, g + 4 * m, g + 5 * m, reinterpret_cast<int*>(g + 6 * m)};
            snms_block(st, boxes, scores, order, s0, len, a, scores_out, keep, slot_key, slot_box);
        }
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_soft_nms_block_threads(void) { return SNMS_THREADS; }
int frcnn_ops_soft_nms_lds_boxes(void) { return SNMS_LDS_BOXES; }
int frcnn_ops_soft_nms_max_boxes(void) { return SNMS_MAX_BOXES; }

size_t frcnn_ops_soft_nms_workspace_bytes(int n)
{
    if (n <= 0 || n > SNMS_MAX_BOXES) return 0;
    return (size_t)n * SNMS_WORDS * sizeof(float);
}

int frcnn_ops_soft_nms(const float* d_boxes, const float* d_scores, const int64_t* d_order, const int64_t* d_categories, int n,
                       float iou_threshold, float sigma, float min_score, int method, int offset, float* d_scores_out, uint8_t* d_keep,
                       void* d_ws, size_t ws_bytes, void* stream)
{
    if (n < 0 || n > SNMS_MAX_BOXES || method < 0 || method > 2 || (offset != 0 && offset != 1)) return FRCNN_EINVAL;
    if (!(sigma > 0.f) || isinf(sigma) || iou_threshold != iou_threshold || min_score != min_score) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_boxes || !d_scores || !d_order || !d_scores_out || !d_keep || !d_ws || ws_bytes < frcnn_ops_soft_nms_workspace_bytes(n))
        return FRCNN_EINVAL;
    const SnmsParams a = {iou_threshold, sigma, min_score, (float)offset, method};
    const int grid = d_categories ? (n < SNMS_GRID ? n : SNMS_GRID) : 1;
    hipLaunchKernelGGL(ops_soft_nms_kernel, dim3(grid), dim3(SNMS_THREADS), 0, (hipStream_t)stream, d_boxes, d_scores, d_order,
                       d_categories, n, a, d_scores_out, d_keep, static_cast<float*>(d_ws));
    return check_launch();
}

}  // extern "C"
