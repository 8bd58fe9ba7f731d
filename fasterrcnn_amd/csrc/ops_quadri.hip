// ops_quadri.hip -- the quadrilateral operators of fasterrcnn_amd.ops (heads that predict four free corners, the point-set assigners):
// box_iou_quadri, nms_quadri and points_in_polygons: the frcnn_ops_box_iou_quadri / frcnn_ops_nms_quadri /
// frcnn_ops_points_in_polygons entry points of include/frcnn_hip.h, which states the contract.  Written from that contract; mmcv's
// kernels of the same names (third party, absent here) take the four vertices in the order given and are half-open on the boundary,
// and are not followed there.
//
// A quadrilateral is 4 vertices in any order (8 floats) and stands for Q, their convex hull: ops_convex.h's cvx_own_hull, the notion of
// polygon convex_iou has.  The IoU of two of them is cvx_inter's clip of hull 1 against hull 2's half-planes on coordinates relative to
// hull 2's smallest vertex (quad_iou, the one device function behind the matrix, the aligned pairs and the NMS mask), so a quadrilateral
// and a point set that repeats its first vertex five times give convex_iou's bits.
//
// Every list indexed at run time lives in LDS, one column per lane of a 64-lane block (element k of a lane at [k * 64 + lane]).  The
// clip's two lists hold CVX_ALL vertices each although a quadrilateral clipped by four half-planes has at most 8: cvx_clip caps its
// output at CVX_ALL, and the lists are sized to that cap, not to the geometry.
//
// box_iou_quadri: a workgroup owns QUAD_TILE_ROWS rows x 64 columns.  Lanes hull the tile's rows and its columns into LDS once; then
// lane j sweeps the rows for its column, reading a row's hull as an LDS broadcast; the bounding boxes are compared before any clip.
// Aligned pairs: one lane per pair.  nms_quadri: ops_rot_nms_mask_kernel's grid, skipping and bit layout with the column hulls formed
// once per tile, then ops.hip's greedy pass.  points_in_polygons: QUAD_POINT_ROWS points x 64 polygons per workgroup; a lane keeps its
// polygon's hull, padded to four edges by repeating the first vertex (an edge of length zero passes every point), in registers.
#include "ops_run.h"
#include "ops_convex.h"

namespace frcnn {

static constexpr int QUAD_TILE_ROWS = 32;         // rows of box_iou_quadri's tile (its columns: the block's 64 lanes)
static constexpr int QUAD_POINT_ROWS = 256;       // points of points_in_polygons' tile
static constexpr int QUAD_MAX_COLS = 65535 * 64;  // columns of a matrix: the tile columns of a launch grid
static constexpr int QUAD_LISTS = 2 * 2 * CVX_ALL * 64;   // floats of the clip's two vertex lists
static_assert(QUAD_TILE_ROWS <= 64, "one lane hulls one row of the tile");
static_assert(QUAD_LISTS >= 2 * 2 * CVX_QUAD * 64, "before the clip the lists hold a quadrilateral's raw and relative vertices");

// The hull of one quadrilateral: n its vertex count, -1 for a dead row; (ox, oy) its smallest point; area its hull's; the bounding box
struct QuadHull { int n; float ox, oy, area, x0, x1, y0, y1; };

// Forms the hull of the row g in the lane's columns: raw receives the four vertices, rel those relative to the smallest, idx the hull
__device__ __forceinline__ QuadHull quad_hull(const float* __restrict__ g, float* raw, float* rel, int* idx)
{
    QuadHull h;
    h.n = -1; h.ox = 0.f; h.oy = 0.f; h.area = 0.f;
    h.x0 = FLT_MAX; h.x1 = -FLT_MAX; h.y0 = FLT_MAX; h.y1 = -FLT_MAX;
    bool ok = true;
    for (int i = 0; i < CVX_QUAD; ++i) {
        const float x = g[2 * i], y = g[2 * i + 1];
        raw[(2 * i) * 64] = x; raw[(2 * i + 1) * 64] = y;
        ok = ok && cvx_finite(x) && cvx_finite(y);
        h.x0 = fminf(h.x0, x); h.x1 = fmaxf(h.x1, x); h.y0 = fminf(h.y0, y); h.y1 = fmaxf(h.y1, y);
    }
    if (ok) {
        const int m = cvx_own_hull(raw, CVX_QUAD, rel, idx, h.ox, h.oy);
        h.area = cvx_hull_area(rel, idx, m);
        if (h.area >= CVX_MIN_AREA) h.n = m;
    }
    return h;
}

// copies the hull's vertices, in hull order, from the points pts to the column dst
__device__ __forceinline__ void quad_stage(const float* pts, const int* idx, int n, float* dst)
{
    for (int v = 0; v < n; ++v) {
        const int i = idx[v * 64];
        dst[(2 * v) * 64] = pts[(2 * i) * 64];
        dst[(2 * v + 1) * 64] = pts[(2 * i + 1) * 64];
    }
}

// IoU (mode 0) or IoF (mode 1) of quadrilateral a with quadrilateral b.  p: a's hull in raw coordinates, q: b's hull relative to its
// smallest vertex; l0 / l1: the clip's lists in the lane's column.
__device__ __forceinline__ float quad_iou(const float* p, const QuadHull& a, const float* q, const QuadHull& b, int mode, float* l0, float* l1)
{
    if (a.n < 0 || b.n < 0) return 0.f;
    if (a.x1 < b.x0 || b.x1 < a.x0 || a.y1 < b.y0 || b.y1 < a.y0) return 0.f;
    const float inter = cvx_inter(p, a.n, b.ox, b.oy, q, b.n, l0, l1);
    const float den = mode ? a.area : (a.area + b.area) - inter;
    return den >= CVX_MIN_AREA ? inter / den : 0.f;
}

// ---- box_iou_quadri -------------------------------------------------------------------------------------------------------------------
// out[i][j] of quads1[i] and quads2[j]: grid (ceil(n / QUAD_TILE_ROWS), ceil(m / 64)), one wave per tile, a lane per column
__global__ __launch_bounds__(64)
void ops_quadri_iou_kernel(const float* __restrict__ quads1, int n, const float* __restrict__ quads2, int m, int mode,
                           float* __restrict__ out)
{
    __shared__ float s_list[QUAD_LISTS];                     // the clip's two vertex lists; before the sweep, the hulls' workspace
    __shared__ int s_idx[CVX_QUAD * 64];
    __shared__ float s_row[2 * CVX_QUAD * 64];               // row r's hull, raw coordinates, at [.. * 64 + r]
    __shared__ float s_col[2 * CVX_QUAD * 64];               // column t's hull relative to its smallest vertex
    __shared__ QuadHull s_rowh[QUAD_TILE_ROWS];
    const int t = threadIdx.x, i0 = blockIdx.x * QUAD_TILE_ROWS, j = blockIdx.y * 64 + t;
    float* raw = s_list + t;
    float* rel = s_list + 2 * CVX_QUAD * 64 + t;
    int* idx = s_idx + t;

    if (t < QUAD_TILE_ROWS && i0 + t < n) {
        const QuadHull h = quad_hull(quads1 + (size_t)(i0 + t) * (2 * CVX_QUAD), raw, rel, idx);
        quad_stage(raw, idx, h.n, s_row + t);
        s_rowh[t] = h;
    }
    __syncthreads();                                         // the rows are staged; the workspace is free again

    if (j >= m) return;                                      // no barrier follows
    const QuadHull c = quad_hull(quads2 + (size_t)j * (2 * CVX_QUAD), raw, rel, idx);
    quad_stage(rel, idx, c.n, s_col + t);
    const int imax = min(n - i0, QUAD_TILE_ROWS);
    for (int i = 0; i < imax; ++i)
        out[(size_t)(i0 + i) * m + j] = quad_iou(s_row + i, s_rowh[i], s_col + t, c, mode, s_list + t, s_list + 2 * CVX_ALL * 64 + t);
}

// out[i] of the aligned pair quads1[i], quads2[i]: one lane per pair, the matrix's diagonal bit for bit
__global__ __launch_bounds__(64)
void ops_quadri_iou_aligned_kernel(const float* __restrict__ quads1, const float* __restrict__ quads2, int n, int mode,
                                   float* __restrict__ out)
{
    __shared__ float s_list[QUAD_LISTS];
    __shared__ int s_idx[CVX_QUAD * 64];
    __shared__ float s_p[2 * CVX_QUAD * 64], s_q[2 * CVX_QUAD * 64];
    const int t = threadIdx.x, i = blockIdx.x * 64 + t;
    if (i >= n) return;                                      // no barrier in this kernel
    float* raw = s_list + t;
    float* rel = s_list + 2 * CVX_QUAD * 64 + t;
    int* idx = s_idx + t;
    const QuadHull a = quad_hull(quads1 + (size_t)i * (2 * CVX_QUAD), raw, rel, idx);
    quad_stage(raw, idx, a.n, s_p + t);
    const QuadHull b = quad_hull(quads2 + (size_t)i * (2 * CVX_QUAD), raw, rel, idx);
    quad_stage(rel, idx, b.n, s_q + t);
    out[i] = quad_iou(s_p + t, a, s_q + t, b, mode, s_list + t, s_list + 2 * CVX_ALL * 64 + t);
}

// ---- nms_quadri ---------------------------------------------------------------------------------------------------------------------------
// ops_rot_nms_mask_kernel (ops_rot.hip) on quadrilaterals: the same grid, tiles, skipping and bit layout; bit j of row i =
// quad_iou(sorted i, sorted j) > thr
__global__ __launch_bounds__(64)
void ops_quadri_nms_mask_kernel(const float* __restrict__ quads, const int64_t* __restrict__ order, const int64_t* __restrict__ cats, int n,
                                int nw, float thr, u64* __restrict__ mask)
{
    const int by = blockIdx.y, bx = blockIdx.x;
    if (bx < by) return;
    if (cats && cats[order[bx * 64]] > cats[order[min(by * 64 + 63, n - 1)]]) return;
    __shared__ float s_list[QUAD_LISTS];
    __shared__ int s_idx[CVX_QUAD * 64];
    __shared__ float s_col[2 * CVX_QUAD * 64];               // column j's hull relative to its smallest vertex, at [.. * 64 + j]
    __shared__ float s_own[2 * CVX_QUAD * 64];               // the lane's row: its hull in raw coordinates
    __shared__ QuadHull colh[64];
    __shared__ int64_t colc[64];
    const int t = threadIdx.x;
    float* raw = s_list + t;
    float* rel = s_list + 2 * CVX_QUAD * 64 + t;
    int* idx = s_idx + t;
    const int jn = bx * 64 + t;
    if (jn < n) {
        const QuadHull h = quad_hull(quads + (size_t)order[jn] * (2 * CVX_QUAD), raw, rel, idx);
        quad_stage(rel, idx, h.n, s_col + t);
        colh[t] = h;
        colc[t] = cats ? cats[order[jn]] : 0;
    }
    __syncthreads();
    const int i = by * 64 + t;
    if (i >= n) return;
    const QuadHull a = quad_hull(quads + (size_t)order[i] * (2 * CVX_QUAD), raw, rel, idx);
    quad_stage(raw, idx, a.n, s_own + t);
    const int64_t ca = cats ? cats[order[i]] : 0;
    u64 bits = 0ull;
    const int jmax = min(n - bx * 64, 64);
    for (int j = 0; j < jmax; ++j)
        if (bx * 64 + j > i && colc[j] == ca &&
            quad_iou(s_own + t, a, s_col + j, colh[j], 0, s_list + t, s_list + 2 * CVX_ALL * 64 + t) > thr)
            bits |= 1ull << j;
    mask[(size_t)i * nw + bx] = bits;
}

// ---- points_in_polygons ---------------------------------------------------------------------------------------------------------------
// out[i][j] = 1 when point i lies in the closed hull of polygon j: grid (ceil(n / QUAD_POINT_ROWS), ceil(m / 64)), one wave per tile,
// a lane per polygon.  For every edge a -> b, on coordinates relative to the hull's smallest vertex:
// (b_x - a_x) (p_y - a_y) >= (b_y - a_y) (p_x - a_x), the two rounded products compared.
__global__ __launch_bounds__(64)
void ops_points_in_polygons_kernel(const float* __restrict__ points, int n, const float* __restrict__ polys, int m, float* __restrict__ out)
{
    __shared__ float s_raw[2 * CVX_QUAD * 64], s_rel[2 * CVX_QUAD * 64], s_col[2 * CVX_QUAD * 64];
    __shared__ int s_idx[CVX_QUAD * 64];
    __shared__ float s_px[QUAD_POINT_ROWS], s_py[QUAD_POINT_ROWS];
    __shared__ int s_pok[QUAD_POINT_ROWS];
    const int t = threadIdx.x, i0 = blockIdx.x * QUAD_POINT_ROWS, j = blockIdx.y * 64 + t;
    const int imax = min(n - i0, QUAD_POINT_ROWS);
    for (int r = t; r < imax; r += 64) {
        const float x = points[(size_t)(i0 + r) * 2], y = points[(size_t)(i0 + r) * 2 + 1];
        s_px[r] = x; s_py[r] = y;
        s_pok[r] = cvx_finite(x) && cvx_finite(y);
    }
    __syncthreads();
    if (j >= m) return;                                      // no barrier follows
    float* col = s_col + t;
    const QuadHull c = quad_hull(polys + (size_t)j * (2 * CVX_QUAD), s_raw + t, s_rel + t, s_idx + t);
    quad_stage(s_rel + t, s_idx + t, c.n, col);
    if (c.n == 3) { col[(2 * 3) * 64] = col[0]; col[(2 * 3 + 1) * 64] = col[64]; }       // a fourth edge of length zero
    // a live hull has 3 or 4 vertices; a dead polygon's column is not read
    const bool live = c.n >= 3;
    float ax[CVX_QUAD], ay[CVX_QUAD], ex[CVX_QUAD], ey[CVX_QUAD];
#pragma unroll
    for (int e = 0; e < CVX_QUAD; ++e) { ax[e] = live ? col[(2 * e) * 64] : 0.f; ay[e] = live ? col[(2 * e + 1) * 64] : 0.f; }
#pragma unroll
    for (int e = 0; e < CVX_QUAD; ++e) {
        const int e1 = e + 1 == CVX_QUAD ? 0 : e + 1;
        ex[e] = ax[e1] - ax[e]; ey[e] = ay[e1] - ay[e];
    }
    for (int i = 0; i < imax; ++i) {
        const float px = s_px[i] - c.ox, py = s_py[i] - c.oy;
        bool in = live && s_pok[i];
#pragma unroll
        for (int e = 0; e < CVX_QUAD; ++e) in = in && ex[e] * (py - ay[e]) >= ey[e] * (px - ax[e]);
        out[(size_t)(i0 + i) * m + j] = in ? 1.f : 0.f;
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_box_iou_quadri_tile_rows(void) { return QUAD_TILE_ROWS; }
int frcnn_ops_points_in_polygons_tile_rows(void) { return QUAD_POINT_ROWS; }
int frcnn_ops_quadri_max_rows(void) { return CVX_MAX_ROWS; }
int frcnn_ops_quadri_max_columns(void) { return QUAD_MAX_COLS; }

int frcnn_ops_box_iou_quadri(const float* d_quads1, int n, const float* d_quads2, int m, int mode, int aligned, float* d_out, void* stream)
{
    if (n < 0 || n > CVX_MAX_ROWS || m < 0 || (mode != 0 && mode != 1) || (aligned ? n != m : m > QUAD_MAX_COLS)) return FRCNN_EINVAL;
    if (n == 0 || m == 0) return FRCNN_OK;
    if (!d_quads1 || !d_quads2 || !d_out) return FRCNN_EINVAL;
    if (aligned)
        hipLaunchKernelGGL(ops_quadri_iou_aligned_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_quads1, d_quads2, n, mode,
                           d_out);
    else
        hipLaunchKernelGGL(ops_quadri_iou_kernel, dim3(cdiv(n, QUAD_TILE_ROWS), cdiv(m, 64)), dim3(64), 0, (hipStream_t)stream, d_quads1, n,
                           d_quads2, m, mode, d_out);
    return check_launch();
}

int frcnn_ops_nms_quadri(const float* d_quads, const int64_t* d_order, const int64_t* d_categories, int n, float iou_threshold,
                         uint8_t* d_keep, void* d_ws, size_t ws_bytes, void* stream)
{
    if (n < 0 || n > 64 * OPS_NMS_MAX_WORDS) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_quads || !d_order || !d_keep || !d_ws || ws_bytes < frcnn_ops_nms_workspace_bytes(n)) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    const int nw = cdiv(n, 64);
    u64* mask = static_cast<u64*>(d_ws);
    hipLaunchKernelGGL(ops_quadri_nms_mask_kernel, dim3(nw, nw), dim3(64), 0, s, d_quads, d_order, d_categories, n, nw, iou_threshold, mask);
    const int rc = check_launch();
    if (rc) return rc;
    return launch_ops_nms_reduce(mask, d_order, d_categories, n, nw, d_keep, s);
}

int frcnn_ops_points_in_polygons(const float* d_points, int n, const float* d_polygons, int m, float* d_out, void* stream)
{
    if (n < 0 || n > CVX_MAX_ROWS || m < 0 || m > QUAD_MAX_COLS) return FRCNN_EINVAL;
    if (n == 0 || m == 0) return FRCNN_OK;
    if (!d_points || !d_polygons || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_points_in_polygons_kernel, dim3(cdiv(n, QUAD_POINT_ROWS), cdiv(m, 64)), dim3(64), 0, (hipStream_t)stream, d_points,
                       n, d_polygons, m, d_out);
    return check_launch();
}

}  // extern "C"
