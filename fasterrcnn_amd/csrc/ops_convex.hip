// ops_convex.hip -- the point-set operators of fasterrcnn_amd.ops (Oriented RepPoints, CFA, SASM): convex_iou, convex_giou and
// min_area_polygons: the frcnn_ops_convex_iou / frcnn_ops_convex_giou / frcnn_ops_min_area_polygons entry points of
// include/frcnn_hip.h, which states the contract.  Written from that contract; mmcv's kernels of the same names (third party, absent
// here) differ in their epsilons, their hull tie-breaks and the scaling of their gradient, and are not followed.
//
// A point set is 9 points (18 floats), a polygon 4 vertices in any order (8 floats).  P = hull(set), Q = hull(polygon), H = hull(all 13).
//
// The hull (cvx_hull, cvx_own_hull), the areas and the intersection (cvx_clip, cvx_inter) are ops_convex.h's, shared with the
// quadrilateral operators of ops_quadri.hip; that header states their rules and the LDS column layout of every runtime-indexed list.
//
// convex_iou: a workgroup owns CVX_TILE_ROWS rows x 64 columns.  Lanes hull the tile's rows and its columns into LDS once; then
// lane j sweeps the rows for its column, reading a row's hull as an LDS broadcast.  A pair whose bounding boxes are apart is 0 without
// a clip (the assigner's common case).  convex_giou: one launch, one lane per aligned pair, value and gradient; the closed form is in
// the header.  min_area_polygons: one launch, one lane per set, rotating calipers over the hull's edges in hull order.
#include "ops_convex.h"

namespace frcnn {

static constexpr int CVX_TILE_ROWS = 32;          // rows of convex_iou's tile (its columns: the block's 64 lanes)
static constexpr float CVX_RECT_TIE = 1.f - 0x1p-18f;   // min_area_polygons: a later edge wins only with an area below this times the best

// ---- convex_iou ---------------------------------------------------------------------------------------------------------------------
// out[i][j] = I / U of set i and polygon j: grid (ceil(n / CVX_TILE_ROWS), ceil(k / 64)), one wave per tile, a lane per column
__global__ __launch_bounds__(64)
void ops_convex_iou_kernel(const float* __restrict__ sets, int n, const float* __restrict__ polys, int k, float* __restrict__ out)
{
    __shared__ float s_list[2 * 2 * CVX_ALL * 64];           // the clip's two vertex lists; before the sweep, the hulls' workspace
    __shared__ int s_idx[CVX_SET * 64];
    __shared__ float s_row[2 * CVX_SET * 64];                // row r's hull, raw coordinates, at [.. * 64 + r]
    __shared__ float s_quad[2 * CVX_QUAD * 64];              // column t's hull relative to its smallest vertex
    __shared__ float s_row_area[CVX_TILE_ROWS], s_row_box[4][CVX_TILE_ROWS];
    __shared__ int s_row_n[CVX_TILE_ROWS];                   // vertices of the row's hull; -1: a dead row
    const int t = threadIdx.x, i0 = blockIdx.x * CVX_TILE_ROWS, j = blockIdx.y * 64 + t;
    float* raw = s_list + t;
    float* rel = s_list + 2 * CVX_SET * 64 + t;
    int* idx = s_idx + t;

    if (t < CVX_TILE_ROWS && i0 + t < n) {
        const float* g = sets + (size_t)(i0 + t) * (2 * CVX_SET);
        bool ok = true;
        float x0 = FLT_MAX, x1 = -FLT_MAX, y0 = FLT_MAX, y1 = -FLT_MAX;
        for (int i = 0; i < CVX_SET; ++i) {
            const float x = g[2 * i], y = g[2 * i + 1];
            raw[(2 * i) * 64] = x; raw[(2 * i + 1) * 64] = y;
            ok = ok && cvx_finite(x) && cvx_finite(y);
            x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
        }
        int m = -1;
        if (ok) {
            float ox, oy;
            m = cvx_own_hull(raw, CVX_SET, rel, idx, ox, oy);
            s_row_area[t] = cvx_hull_area(rel, idx, m);
            for (int v = 0; v < m; ++v) {
                const int i = idx[v * 64];
                s_row[(2 * v) * 64 + t] = raw[(2 * i) * 64];
                s_row[(2 * v + 1) * 64 + t] = raw[(2 * i + 1) * 64];
            }
            s_row_box[0][t] = x0; s_row_box[1][t] = x1; s_row_box[2][t] = y0; s_row_box[3][t] = y1;
        }
        s_row_n[t] = m;
    }
    __syncthreads();                                         // the rows are staged; the workspace is free again

    int nq = -1;
    float qox = 0.f, qoy = 0.f, qarea = 0.f, qx0 = FLT_MAX, qx1 = -FLT_MAX, qy0 = FLT_MAX, qy1 = -FLT_MAX;
    if (j < k) {
        const float* g = polys + (size_t)j * (2 * CVX_QUAD);
        bool ok = true;
        for (int i = 0; i < CVX_QUAD; ++i) {
            const float x = g[2 * i], y = g[2 * i + 1];
            raw[(2 * i) * 64] = x; raw[(2 * i + 1) * 64] = y;
            ok = ok && cvx_finite(x) && cvx_finite(y);
            qx0 = fminf(qx0, x); qx1 = fmaxf(qx1, x); qy0 = fminf(qy0, y); qy1 = fmaxf(qy1, y);
        }
        if (ok) {
            const int m = cvx_own_hull(raw, CVX_QUAD, rel, idx, qox, qoy);
            qarea = cvx_hull_area(rel, idx, m);
            if (qarea >= CVX_MIN_AREA) {
                nq = m;
                for (int v = 0; v < m; ++v) {
                    const int i = idx[v * 64];
                    s_quad[(2 * v) * 64 + t] = rel[(2 * i) * 64];
                    s_quad[(2 * v + 1) * 64 + t] = rel[(2 * i + 1) * 64];
                }
            }
        }
    }
    if (j >= k) return;                                      // no barrier follows
    const int imax = min(n - i0, CVX_TILE_ROWS);
    for (int i = 0; i < imax; ++i) {
        const int np = s_row_n[i];
        float iou = 0.f;
        if (np >= 0 && nq >= 0 && !(s_row_box[1][i] < qx0 || qx1 < s_row_box[0][i] || s_row_box[3][i] < qy0 || qy1 < s_row_box[2][i])) {
            const float inter = cvx_inter(s_row + i, np, qox, qoy, s_quad + t, nq, s_list + t, s_list + 2 * CVX_ALL * 64 + t);
            const float u = (s_row_area[i] + qarea) - inter;
            if (u >= CVX_MIN_AREA) iou = inter / u;
        }
        out[(size_t)(i0 + i) * k + j] = iou;
    }
}

// ---- convex_giou ----------------------------------------------------------------------------------------------------------------------
// giou[i] and grad[i][18] of the aligned pair i: one lane per pair.  The gradient (header): over P's edges a -> b with
// N = (b_y - a_y, a_x - b_x), dA_P adds N / 2 to both ends and dI adds N (s1 - s2) to a and N s2 to b, [t0, t1] the part of the edge
// inside Q (Cyrus-Beck); dC is dA_P's sum over H's edges for the ends that are points of the set;
// d giou = (1 / U - cU) dI + cU dA_P - U / C^2 dC with cU = 1 / C - I / U^2.  A vertex's terms are added in hull order.
__global__ __launch_bounds__(64)
void ops_convex_giou_kernel(const float* __restrict__ sets, const float* __restrict__ polys, int n, float* __restrict__ giou,
                            float* __restrict__ grad)
{
    __shared__ float s_list[2 * 2 * CVX_ALL * 64];           // the clip's two vertex lists; before the clip, the hulls' workspace
    __shared__ float s_set[2 * CVX_SET * 64];                // the raw points; at the end, the row of the gradient
    __shared__ float s_quad[2 * CVX_QUAD * 64];
    __shared__ float s_all[2 * CVX_ALL * 64];                // P's hull, then Q's, relative to Q's smallest vertex
    __shared__ float s_acc[2 * CVX_SET * 64];                // the gradient of P's vertex v
    __shared__ int s_hp[CVX_SET * 64], s_hq[CVX_QUAD * 64], s_hh[CVX_ALL * 64];
    const int t = threadIdx.x, i = blockIdx.x * 64 + t;
    if (i >= n) return;                                      // no barrier in this kernel
    float* set = s_set + t;
    float* quad = s_quad + t;
    float* all = s_all + t;
    float* acc = s_acc + t;
    float* rel = s_list + t;
    int* hp = s_hp + t;
    int* hq = s_hq + t;
    int* hh = s_hh + t;
    float* grow = grad + (size_t)i * (2 * CVX_SET);

    bool ok = true;
    for (int c = 0; c < 2 * CVX_SET; ++c) { const float v = sets[(size_t)i * (2 * CVX_SET) + c]; set[c * 64] = v; ok = ok && cvx_finite(v); }
    for (int c = 0; c < 2 * CVX_QUAD; ++c) { const float v = polys[(size_t)i * (2 * CVX_QUAD) + c]; quad[c * 64] = v; ok = ok && cvx_finite(v); }
    float value = 0.f, inter = 0.f, u = 0.f, cc = 0.f;
    int np = 0, nq = 0, nh = 0;
    if (ok) {
        float ox, oy, px, py;
        nq = cvx_own_hull(quad, CVX_QUAD, rel, hq, ox, oy);
        const float qarea = cvx_hull_area(rel, hq, nq);
        np = cvx_own_hull(set, CVX_SET, rel, hp, px, py);
        const float parea = cvx_hull_area(rel, hp, np);
        for (int v = 0; v < np; ++v) {
            const int p = hp[v * 64];
            all[(2 * v) * 64] = set[(2 * p) * 64] - ox;
            all[(2 * v + 1) * 64] = set[(2 * p + 1) * 64] - oy;
        }
        for (int v = 0; v < nq; ++v) {
            const int q = hq[v * 64];
            all[(2 * (np + v)) * 64] = quad[(2 * q) * 64] - ox;
            all[(2 * (np + v) + 1) * 64] = quad[(2 * q + 1) * 64] - oy;
        }
        ok = qarea >= CVX_MIN_AREA;
        if (ok) {
            inter = cvx_inter(all, np, 0.f, 0.f, all + 2 * np * 64, nq, s_list + t, s_list + 2 * CVX_ALL * 64 + t);
            nh = cvx_hull(all, np + nq, hh);
            cc = cvx_hull_area(all, hh, nh);
            u = (parea + qarea) - inter;
            ok = u >= CVX_MIN_AREA && cc >= CVX_MIN_AREA;
        }
    }
    for (int c = 0; c < 2 * CVX_SET; ++c) set[c * 64] = 0.f;     // from here on: the gradient's row
    if (ok) {
        value = (inter / u + u / cc) - 1.f;
        // I / U^2 and U / C^2 as two divisions each: the square of an area would overflow at coordinates of 2^32
        const float cu = 1.f / cc - (inter / u) / u, ci = 1.f / u - cu, ch = -((u / cc) / cc);
        const float* q = all + 2 * np * 64;
        for (int c = 0; c < 2 * np; ++c) acc[c * 64] = 0.f;
        for (int v = 0; v < np && np >= 2; ++v) {
            const int w = v + 1 == np ? 0 : v + 1;
            const float ax = all[(2 * v) * 64], ay = all[(2 * v + 1) * 64], bx = all[(2 * w) * 64], by = all[(2 * w + 1) * 64];
            const float nx = by - ay, ny = ax - bx;
            float t0 = 0.f, t1 = 1.f;
            for (int e = 0; e < nq; ++e) {
                const int e1 = e + 1 == nq ? 0 : e + 1;
                const float qx = q[(2 * e) * 64], qy = q[(2 * e + 1) * 64], ex = q[(2 * e1) * 64] - qx, ey = q[(2 * e1 + 1) * 64] - qy;
                const float da = ex * (ay - qy) - ey * (ax - qx), db = ex * (by - qy) - ey * (bx - qx);
                if (da >= 0.f && db >= 0.f) continue;
                if (da < 0.f && db < 0.f) { t1 = -1.f; break; }
                const float tc = da / (da - db);
                if (da < 0.f) t0 = fmaxf(t0, tc); else t1 = fminf(t1, tc);
            }
            float wa = 0.5f * cu, wb = 0.5f * cu;
            if (t1 > t0 && np >= 3) {
                const float s1 = t1 - t0, s2 = 0.5f * (t1 * t1 - t0 * t0);
                wa = wa + ci * (s1 - s2);
                wb = wb + ci * s2;
            }
            acc[(2 * v) * 64] = acc[(2 * v) * 64] + wa * nx;
            acc[(2 * v + 1) * 64] = acc[(2 * v + 1) * 64] + wa * ny;
            acc[(2 * w) * 64] = acc[(2 * w) * 64] + wb * nx;
            acc[(2 * w + 1) * 64] = acc[(2 * w + 1) * 64] + wb * ny;
        }
        for (int v = 0; v < nh && nh >= 2; ++v) {
            const int a = hh[v * 64], b = hh[(v + 1 == nh ? 0 : v + 1) * 64];
            const float wn = 0.5f * ch;
            const float nx = wn * (all[(2 * b + 1) * 64] - all[(2 * a + 1) * 64]), ny = wn * (all[(2 * a) * 64] - all[(2 * b) * 64]);
            if (a < np) { acc[(2 * a) * 64] = acc[(2 * a) * 64] + nx; acc[(2 * a + 1) * 64] = acc[(2 * a + 1) * 64] + ny; }
            if (b < np) { acc[(2 * b) * 64] = acc[(2 * b) * 64] + nx; acc[(2 * b + 1) * 64] = acc[(2 * b + 1) * 64] + ny; }
        }
        for (int v = 0; v < np; ++v) {
            const int p = hp[v * 64];
            set[(2 * p) * 64] = acc[(2 * v) * 64];
            set[(2 * p + 1) * 64] = acc[(2 * v + 1) * 64];
        }
    }
    giou[i] = value;
    for (int c = 0; c < 2 * CVX_SET; ++c) grow[c] = set[c * 64];
}

// ---- min_area_polygons ----------------------------------------------------------------------------------------------------------------
// out[i][8]: the rectangle of the smallest area on an edge of set i's hull, one lane per set.  For edge k = a -> b, u its unit direction
// and v = (-u_y, u_x): the extents [u_min, u_max] x [0, v_max] of the hull's vertices relative to a; the first k of the smallest
// (u_max - u_min) v_max wins; corners (u_min, 0), (u_max, 0), (u_max, v_max), (u_min, v_max).  Equal areas are no accident: the edges
// of an acute triangle all give twice its area, and so do the edges of any hull whose rectangle rests on three vertices.  Rounding
// would pick among them at random, so areas within a relative 2^-18 (ten times the rounding of an area) count as tied.
__global__ __launch_bounds__(64)
void ops_min_area_polygons_kernel(const float* __restrict__ sets, int n, float* __restrict__ out)
{
    __shared__ float s_raw[2 * CVX_SET * 64], s_rel[2 * CVX_SET * 64];
    __shared__ int s_idx[CVX_SET * 64];
    const int t = threadIdx.x, i = blockIdx.x * 64 + t;
    if (i >= n) return;
    float* raw = s_raw + t;
    float* rel = s_rel + t;
    int* idx = s_idx + t;
    bool ok = true;
    for (int c = 0; c < 2 * CVX_SET; ++c) { const float v = sets[(size_t)i * (2 * CVX_SET) + c]; raw[c * 64] = v; ok = ok && cvx_finite(v); }
    float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) {
        float ox, oy;
        const int m = cvx_own_hull(raw, CVX_SET, rel, idx, ox, oy);
        if (m <= 2) {
            const int a = idx[0], b = idx[(m - 1) * 64];
            c[0] = c[6] = raw[(2 * a) * 64]; c[1] = c[7] = raw[(2 * a + 1) * 64];
            c[2] = c[4] = raw[(2 * b) * 64]; c[3] = c[5] = raw[(2 * b + 1) * 64];
        } else {
            float best = FLT_MAX, bax = 0.f, bay = 0.f, bux = 1.f, buy = 0.f, bu0 = 0.f, bu1 = 0.f, bv1 = 0.f;
            for (int v = 0; v < m; ++v) {
                const int a = idx[v * 64], b = idx[(v + 1 == m ? 0 : v + 1) * 64];
                const float ax = rel[(2 * a) * 64], ay = rel[(2 * a + 1) * 64];
                const float ex = rel[(2 * b) * 64] - ax, ey = rel[(2 * b + 1) * 64] - ay;
                const float scale = fmaxf(fabsf(ex), fabsf(ey));        // > 0: hull vertices differ.  Scaled first, so that the
                const float sx = ex / scale, sy = ey / scale;           // squares neither underflow nor overflow: len in [1, sqrt 2]
                const float len = sqrtf(sx * sx + sy * sy);
                const float ux = sx / len, uy = sy / len;
                float u0 = 0.f, u1 = 0.f, v1 = 0.f;
                for (int w = 0; w < m; ++w) {
                    const int p = idx[w * 64];
                    const float dx = rel[(2 * p) * 64] - ax, dy = rel[(2 * p + 1) * 64] - ay;
                    const float pu = dx * ux + dy * uy, pv = dy * ux - dx * uy;
                    u0 = fminf(u0, pu); u1 = fmaxf(u1, pu); v1 = fmaxf(v1, pv);
                }
                const float area = (u1 - u0) * v1;
                if (area < best * CVX_RECT_TIE) { best = area; bax = ax; bay = ay; bux = ux; buy = uy; bu0 = u0; bu1 = u1; bv1 = v1; }
            }
            const float x0 = bax + bu0 * bux, y0 = bay + bu0 * buy, x1 = bax + bu1 * bux, y1 = bay + bu1 * buy;
            const float vx = -(bv1 * buy), vy = bv1 * bux;
            c[0] = ox + x0; c[1] = oy + y0;
            c[2] = ox + x1; c[3] = oy + y1;
            c[4] = ox + (x1 + vx); c[5] = oy + (y1 + vy);
            c[6] = ox + (x0 + vx); c[7] = oy + (y0 + vy);
        }
    }
    float4* o = reinterpret_cast<float4*>(out + (size_t)i * 8);
    o[0] = make_float4(c[0], c[1], c[2], c[3]);
    o[1] = make_float4(c[4], c[5], c[6], c[7]);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_convex_iou_tile_rows(void) { return CVX_TILE_ROWS; }

int frcnn_ops_convex_iou(const float* d_pointsets, int n, const float* d_polygons, int k, float* d_out, void* stream)
{
    if (n < 0 || n > CVX_MAX_ROWS || k < 0 || k > 65535 * 64) return FRCNN_EINVAL;
    if (n == 0 || k == 0) return FRCNN_OK;
    if (!d_pointsets || !d_polygons || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_convex_iou_kernel, dim3(cdiv(n, CVX_TILE_ROWS), cdiv(k, 64)), dim3(64), 0, (hipStream_t)stream, d_pointsets, n,
                       d_polygons, k, d_out);
    return check_launch();
}

int frcnn_ops_convex_giou(const float* d_pointsets, const float* d_polygons, int n, float* d_giou, float* d_grad, void* stream)
{
    if (n < 0 || n > CVX_MAX_ROWS) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_pointsets || !d_polygons || !d_giou || !d_grad) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_convex_giou_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_pointsets, d_polygons, n, d_giou,
                       d_grad);
    return check_launch();
}

int frcnn_ops_min_area_polygons(const float* d_pointsets, int n, float* d_out, void* stream)
{
    if (n < 0 || n > CVX_MAX_ROWS) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_pointsets || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_min_area_polygons_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_pointsets, n, d_out);
    return check_launch();
}

}  // extern "C"
