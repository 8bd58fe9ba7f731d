// ops_border.hip -- BorderAlign, the border pooling of BorderDet (mmcv's border_align), over N images with a deterministic backward
// pass: the frcnn_ops_border_align* entry points of include/frcnn_hip.h.  Restated from the published definition (mmcv is third party,
// absent here: restated, unpinned); where the two differ the header's text holds.
//
// For every box and each of its four edges the operator takes pool_size + 1 bilinear samples along the edge, from the edge's own group
// of channels, and keeps per channel the largest one and its index.  Sample i of edge e lies at (x0 + (float)i dx, y0 + (float)i dy),
// the product first, in the forward AND the backward, so the backward lands on the forward's sample exactly.  A sample counts iff
// -1 <= y <= H and -1 <= x <= W (a NaN fails: border_axis tests it before axis_weights of geometry.h, which lets NaN through);
// otherwise its value is exactly 0 and it receives nothing.  No coordinate becomes an int before that test.
//
// Layouts: the map is NHWC [n][h][w][4 c], group e (0 top, 1 left, 2 bottom, 3 right) in channels [e c, (e + 1) c); c is the host's
// padded group size, whole runs, so a lane's Run<E> never straddles two groups.  Boxes are float32 [n][k][4].  Output, argmax (int32)
// and the output gradient are [n][k][4][c]: a channels_last [n][c][k][4] tensor.
// Forward: one lane per (box, edge, channel run), one pass that writes output and argmax.  The four edges of a box are neighbouring
//   lanes' work and read the same 16 bytes of box.  Along an edge one coordinate is constant (y0 + (float)i 0 == y0), so its cells and
//   weights are computed once; of the moving coordinate's two columns the lane keeps the last pair loaded and reloads only a column
//   that changed (a stride of at most one cell reloads one column or none).
// Backward: the 2 x 2-cell tile gather of ops.hip, per edge group and without its lists: a block owns one tile and 64 channel runs, and
//   wave e of the block owns edge group e, alone -- no LDS, no barrier.  A wave tests 64 boxes at once, one per lane: a box is taken
//   for edge e when that edge's segment -- sample 0 to sample pool, which bound every sample because fl(x0 + fl(i dx)) is monotone in
//   i -- grown by one cell and rounded outwards meets the tile.  The ballot of the 64 tests is the cull list: the wave walks its set
//   bits from the lowest, so boxes come in ascending order over all groups of 64.  The argmax is per channel, so for a taken box each
//   lane loads its run of argmax and dout once, re-derives each channel's sample from that channel's argmax and adds dout wy wx to
//   those of the tile's four cells the sample touches; four accumulators in registers, one store each.  No atomics: two runs agree
//   bit for bit.  (ops.hip's form, a wave per CELL behind an LDS list of 1024 boxes, loads every listed run four times and re-derives
//   every sample four times: measured at BorderDet's shape, forward + backward 3.68 ms against this form's 2.17 ms -- INTEGRATION.md.)
//   Why not the sorted plan of the sampler backwards (_sorted_gather): the argmax makes its entries per channel, 4 corners x 4 edges =
//   16 n c k keys (249 M keys, 3 GB of keys and weights to sort, at BorderDet's n = 2, c = 256, k = 15200), where the gather reads 32 n c k
//   bytes once per tile the grown segment meets and sorts nothing.
// Every loop is bounded by pool_size, k or the channel count; the grids are flat and their sizes are checked on the host (FRCNN_EINVAL).
//
// Element types: templates over the storage type E (ops_run.h): widened exactly on load, geometry, weights, comparisons and sums in
// float32 in one shared body, rounded once on store, so that op(x_T) == op(x_T.float()).to(T) bit for bit for the output and d_x, and
// the argmax is that of the widened map.
#include "ops_run.h"
#include <climits>
#include <cstdint>

namespace frcnn {

static constexpr int BORDER_MAX_POOL = 64;                  // pool_size <= 64
static constexpr int BORDER_MAX_SIDE = 1 << 24;             // fh, fw: coordinates up to the map's size are exact in float32
static constexpr int BORDER_GROUP = 64;                     // boxes a wave of the backward tests at once, one per lane
static constexpr int BORDER_AHEAD = 4;                      // groups it tests before it walks the first one
static constexpr size_t BORDER_MAX_INDEX = (size_t)INT32_MAX - 1024;   // forward lanes and backward blocks: the flat grids' 32-bit indices

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
// edge e of the box (x1, y1, x2, y2): top and left start at (x1, y1) and step forwards, bottom and right start at (x2, y2) and step back
struct BorderEdge { float x0, y0, dx, dy; };

__device__ __forceinline__ BorderEdge border_edge(const float* box, int e, int pool)
{
    const float x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
    const bool back = e >= 2, along_x = (e & 1) == 0;
    const float s = (along_x ? x2 - x1 : y2 - y1) / (float)pool, step = back ? -s : s;
    BorderEdge g;
    g.x0 = back ? x2 : x1;
    g.y0 = back ? y2 : y1;
    g.dx = along_x ? step : 0.0f;
    g.dy = along_x ? 0.0f : step;
    return g;
}

__device__ __forceinline__ void border_sample(const BorderEdge& g, int i, float& x, float& y)
{
    x = g.x0 + (float)i * g.dx;
    y = g.y0 + (float)i * g.dy;
}

// axis_weights with the NaN test it lacks
__device__ __forceinline__ bool border_axis(float v, int n, int& lo, int& hi, float& wl, float& wh)
{
    return v == v && axis_weights(v, n, lo, hi, wl, wh);
}

__device__ __forceinline__ bool border_cell(float v, int n, int cell, float& w) { return v == v && cell_weight(v, n, cell, w); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// items = n k 4 (C / V): lane `item` owns channel run c4 of edge e of box (img, r), item = ((img k + r) 4 + e) (C / V) + c4, which is
// also the index of its run in out and argmax.
template <typename E>
__global__ __launch_bounds__(256)
void ops_border_forward_kernel(const E* __restrict__ x, int fh, int fw, int C, const float* __restrict__ boxes, int k, long long items,
                               int pool, E* __restrict__ out, int* __restrict__ argmax)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    typedef typename R::ivec ivec;
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= items) return;
    const int C4 = C / R::V, c4 = (int)(item % C4);
    const long long t = item / C4, box = t >> 2;
    const int e = (int)(t & 3), img = (int)(box / k);
    const BorderEdge g = border_edge(boxes + box * 4, e, pool);
    const E* const fm = x + (size_t)img * fh * fw * C * 4;
    const size_t run = (size_t)e * C4 + c4, cell_runs = (size_t)C4 * 4;
    // the fixed coordinate (f) and the moving one (m): top and bottom move along x
    const bool along_x = (e & 1) == 0;
    const int mn = along_x ? fw : fh;
    const size_t m_stride = along_x ? 1 : (size_t)fw, f_stride = along_x ? (size_t)fw : 1;
    int f_lo = 0, f_hi = 0;
    float wf_lo = 0.f, wf_hi = 0.f;
    const bool f_ok = border_axis(along_x ? g.y0 : g.x0, along_x ? fh : fw, f_lo, f_hi, wf_lo, wf_hi);
    auto cell = [&](int m, int f) { return R::load(fm, ((size_t)m * m_stride + (size_t)f * f_stride) * cell_runs + run); };

    vec best = 0.f;
    ivec arg = 0;
    int c_lo = -1, c_hi = -1;                                               // the columns held in p (lo: p00, p01; hi: p10, p11)
    vec p00 = 0.f, p01 = 0.f, p10 = 0.f, p11 = 0.f;                        // p[column][f_lo, f_hi]
    for (int i = 0; i <= pool; ++i) {
        float sx, sy;
        border_sample(g, i, sx, sy);
        int m_lo, m_hi;
        float wm_lo, wm_hi;
        vec val = 0.f;
        if (f_ok && border_axis(along_x ? sx : sy, mn, m_lo, m_hi, wm_lo, wm_hi)) {
            vec n00, n01, n10, n11;
            if (m_lo == c_lo) { n00 = p00; n01 = p01; }
            else if (m_lo == c_hi) { n00 = p10; n01 = p11; }
            else { n00 = cell(m_lo, f_lo); n01 = cell(m_lo, f_hi); }
            if (m_hi == m_lo) { n10 = n00; n11 = n01; }
            else if (m_hi == c_hi) { n10 = p10; n11 = p11; }
            else if (m_hi == c_lo) { n10 = p00; n11 = p01; }
            else { n10 = cell(m_hi, f_lo); n11 = cell(m_hi, f_hi); }
            p00 = n00; p01 = n01; p10 = n10; p11 = n11;
            c_lo = m_lo; c_hi = m_hi;
            // RoIAlign's form: (y low, x low), (y low, x high), (y high, x low), (y high, x high)
            const float wy_lo = along_x ? wf_lo : wm_lo, wy_hi = along_x ? wf_hi : wm_hi;
            const float wx_lo = along_x ? wm_lo : wf_lo, wx_hi = along_x ? wm_hi : wf_hi;
            const float w1 = wy_lo * wx_lo, w2 = wy_lo * wx_hi, w3 = wy_hi * wx_lo, w4 = wy_hi * wx_hi;
            const vec v2 = along_x ? p10 : p01, v3 = along_x ? p01 : p10;
            val = ((p00 * w1 + v2 * w2) + v3 * w3) + p11 * w4;
        }
        if (i == 0) best = val;
        else {
#pragma unroll
            for (int j = 0; j < R::V; ++j)
                if (val[j] > best[j]) { best[j] = val[j]; arg[j] = i; }    // a NaN never wins; a NaN at i == 0 stays
        }
    }
    R::store(out, (size_t)item, best);
    reinterpret_cast<ivec*>(argmax)[item] = arg;
}

// ---- d_x: the gather --------------------------------------------------------------------------------------------------------------------
// grid: (img n_chunks + chunk) tiles_y tiles_x + tile, flat; wave e of the block owns edge group e of the tile and never meets the others
template <typename E>
__global__ __launch_bounds__(256)
void ops_border_backward_kernel(const float* __restrict__ boxes, int k, int fh, int fw, int C, int pool, int tiles_y, int tiles_x,
                                const int* __restrict__ argmax, const E* __restrict__ dout, E* __restrict__ dx)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    typedef typename R::ivec ivec;
    const int C4 = C / R::V, n_chunks = (C4 + 63) >> 6;
    unsigned t = blockIdx.x;
    const int tx0 = (int)(t % tiles_x) * OPS_TILE;
    t /= tiles_x;
    const int ty0 = (int)(t % tiles_y) * OPS_TILE;
    t /= tiles_y;
    const int chunk = (int)(t % n_chunks), img = (int)(t / n_chunks);
    const int ty1 = min(ty0 + OPS_TILE, fh) - 1, tx1 = min(tx0 + OPS_TILE, fw) - 1;
    const int lane = threadIdx.x & 63, e = threadIdx.x >> 6;
    const int c4 = chunk * 64 + lane;
    const bool act = c4 < C4;
    const float* const img_boxes = boxes + (size_t)img * k * 4;

    // edge e's segment, sample 0 .. sample pool (they bound the others), grown by one cell and rounded outwards.  fminf / fmaxf drop a
    // NaN end: such a box may be taken, and its samples then fail the exact test below
    auto touches = [&](int r) {
        const BorderEdge g = border_edge(img_boxes + (size_t)r * 4, e, pool);
        float xa, ya, xb, yb;
        border_sample(g, 0, xa, ya);
        border_sample(g, pool, xb, yb);
        return floorf(fminf(xa, xb)) - 1.0f <= (float)tx1 && ceilf(fmaxf(xa, xb)) + 1.0f >= (float)tx0 &&
               floorf(fminf(ya, yb)) - 1.0f <= (float)ty1 && ceilf(fmaxf(ya, yb)) + 1.0f >= (float)ty0;
    };

    vec acc[OPS_TILE][OPS_TILE];                                            // the tile's cells [row][column]
#pragma unroll
    for (int a = 0; a < OPS_TILE; ++a)
#pragma unroll
        for (int b = 0; b < OPS_TILE; ++b) acc[a][b] = 0.f;
    // What box r sends to the tile's cells through this lane's channels.  The edge's fixed coordinate (y0 + (float)i 0 == y0) is the same
    // for every sample, so its weights on the tile's two rows (columns) are formed once a box, and only the moving one per channel.
    const bool along_x = (e & 1) == 0;
    const int fn = along_x ? fh : fw, mn = along_x ? fw : fh, f0 = along_x ? ty0 : tx0, m0 = along_x ? tx0 : ty0;
    auto take = [&](int r) {
        const BorderEdge g = border_edge(img_boxes + (size_t)r * 4, e, pool);
        float wf[OPS_TILE], wm[OPS_TILE];
        bool hf[OPS_TILE], hm[OPS_TILE];
#pragma unroll
        for (int a = 0; a < OPS_TILE; ++a) hf[a] = border_cell(along_x ? g.y0 : g.x0, fn, f0 + a, wf[a]);
        const float start = along_x ? g.x0 : g.y0, step = along_x ? g.dx : g.dy;
        const size_t o = (((size_t)img * k + r) * 4 + e) * C4 + c4;
        const ivec am = reinterpret_cast<const ivec*>(argmax)[o];
        const vec gr = R::load(dout, o);
#pragma unroll
        for (int j = 0; j < R::V; ++j) {
            const float m = start + (float)am[j] * step;                    // border_sample's moving coordinate
#pragma unroll
            for (int b = 0; b < OPS_TILE; ++b) hm[b] = border_cell(m, mn, m0 + b, wm[b]);
#pragma unroll
            for (int a = 0; a < OPS_TILE; ++a)
#pragma unroll
                for (int b = 0; b < OPS_TILE; ++b) {                         // cell (row a, column b)
                    const bool hy = along_x ? hf[a] : hm[a], hx = along_x ? hm[b] : hf[b];
                    const float wy = along_x ? wf[a] : wm[a], wx = along_x ? wm[b] : wf[b];
                    if (hy && hx) acc[a][b][j] = acc[a][b][j] + gr[j] * (wy * wx);
                }
        }
    };
    // BORDER_AHEAD groups are tested before the first is walked, so that a wave has that many box loads in flight, not one (the scan of
    // the k boxes is a chain of load latencies otherwise); wave-uniform trip counts: every lane meets every ballot
    for (int r0 = 0; r0 < k; r0 += BORDER_AHEAD * BORDER_GROUP) {
        u64 group[BORDER_AHEAD];
#pragma unroll
        for (int q = 0; q < BORDER_AHEAD; ++q) {
            const int rl = r0 + q * BORDER_GROUP + lane;
            group[q] = __ballot(rl < k && touches(rl));
        }
#pragma unroll
        for (int q = 0; q < BORDER_AHEAD; ++q)
            for (u64 hits = group[q]; hits; hits &= hits - 1)              // ascending box order
                if (act) take(r0 + q * BORDER_GROUP + __builtin_ctzll(hits));
    }
    if (act)
#pragma unroll
        for (int a = 0; a < OPS_TILE; ++a)
#pragma unroll
            for (int b = 0; b < OPS_TILE; ++b)
                if (ty0 + a <= ty1 && tx0 + b <= tx1)
                    R::store(dx + (size_t)img * fh * fw * C * 4, ((size_t)(ty0 + a) * fw + tx0 + b) * C4 * 4 + (size_t)e * C4 + c4, acc[a][b]);
}

// ---- the entry points' bodies, one per element type ---------------------------------------------------------------------------------
// c: the channels of one edge group; v: those of a lane's run
static bool border_args_ok(int n_img, int fh, int fw, int c, int k, int pool, int v)
{
    return n_img >= 1 && fh >= 1 && fh <= BORDER_MAX_SIDE && fw >= 1 && fw <= BORDER_MAX_SIDE && c >= v && c % v == 0 && k >= 0 &&
           pool >= 1 && pool <= BORDER_MAX_POOL && (size_t)fh * fw <= (size_t)INT32_MAX;
}

template <typename E>
static int border_forward_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_boxes, int k, int pool, void* d_out,
                               int* d_argmax, void* stream)
{
    if (!border_args_ok(n_img, fh, fw, c, k, pool, Run<E>::V)) return FRCNN_EINVAL;
    const size_t items = (size_t)n_img * k * 4 * (c / Run<E>::V);
    if (items > BORDER_MAX_INDEX) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_boxes || !d_out || !d_argmax) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_border_forward_kernel<E>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const E*>(d_x), fh, fw, c, d_boxes, k, (long long)items, pool, static_cast<E*>(d_out), d_argmax);
    return check_launch();
}

template <typename E>
static int border_backward_impl(const float* d_boxes, int k, int n_img, int fh, int fw, int c, int pool, const int* d_argmax,
                                const void* d_dout, void* d_dx, void* stream)
{
    if (!border_args_ok(n_img, fh, fw, c, k, pool, Run<E>::V)) return FRCNN_EINVAL;
    const int tiles_y = cdiv(fh, OPS_TILE), tiles_x = cdiv(fw, OPS_TILE);
    const size_t blocks = (size_t)n_img * cdiv(c / Run<E>::V, 64) * tiles_y * tiles_x;
    if (blocks > BORDER_MAX_INDEX || !d_dx) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (k == 0) {
        FRCNN_HIP_TRY(hipMemsetAsync(d_dx, 0, (size_t)n_img * fh * fw * c * 4 * sizeof(E), s));
        return FRCNN_OK;
    }
    if (!d_boxes || !d_argmax || !d_dout) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_border_backward_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, s, d_boxes, k, fh, fw, c, pool, tiles_y,
                       tiles_x, d_argmax, static_cast<const E*>(d_dout), static_cast<E*>(d_dx));
    return check_launch();
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_border_align_cull_list(void) { return BORDER_GROUP; }

int frcnn_ops_border_align(const float* d_x, int n_img, int fh, int fw, int c, const float* d_boxes, int k, int pool_size, float* d_out,
                           int* d_argmax, void* stream)
{
    return border_forward_impl<float>(d_x, n_img, fh, fw, c, d_boxes, k, pool_size, d_out, d_argmax, stream);
}

int frcnn_ops_border_align_backward(const float* d_boxes, int k, int n_img, int fh, int fw, int c, int pool_size, const int* d_argmax,
                                    const float* d_dout, float* d_dx, void* stream)
{
    return border_backward_impl<float>(d_boxes, k, n_img, fh, fw, c, pool_size, d_argmax, d_dout, d_dx, stream);
}

int frcnn_ops_border_align_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_boxes, int k,
                              int pool_size, void* d_out, int* d_argmax, void* stream)
{
    if (c % OPS_HALF_RUN != 0) return FRCNN_EINVAL;
    // the forward always walks runs of OPS_HALF_RUN: only those two kernels are built
    OPS_ELEM_DISPATCH(elem_type, E,
                      border_forward_impl<run_t<E, OPS_HALF_RUN>>(d_x, n_img, fh, fw, c, d_boxes, k, pool_size, d_out, d_argmax, stream));
}

int frcnn_ops_border_align_backward_16(int elem_type, const float* d_boxes, int k, int n_img, int fh, int fw, int c, int pool_size,
                                       const int* d_argmax, const void* d_dout, void* d_dx, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), border_backward_impl, d_boxes, k, n_img, fh, fw, c, pool_size, d_argmax, d_dout, d_dx,
                    stream);
}

}  // extern "C"
