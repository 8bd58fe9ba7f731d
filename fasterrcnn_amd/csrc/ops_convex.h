// ops_convex.h -- the hull, area and clip device functions that the point-set operators (ops_convex.hip) and the quadrilateral
// operators (ops_quadri.hip) share: one notion of polygon for both families.  include/frcnn_hip.h states the contract.
//
// Hull (cvx_hull): a gift-wrapping walk from the point with the smallest (x, y), counter-clockwise; from the current vertex the next
// is the point no other point lies to the right of, the farthest of those on one ray, the smallest index of equal points.  The list is
// a function of the set, so permuting the points changes no result bit -- as long as the candidates' order is total: a strict turn is
// decided by comparing the two rounded products of the cross product, which is exact in sign, but where the products of points that
// are NOT collinear round to one value the distance decides, and three nearly collinear candidates can then win in scan order.
// A set's own hull is decided on coordinates relative to its own smallest point (cvx_own_hull); everything that involves a pair -- the
// clip, the hull of 13, every normal -- on coordinates relative to Q's smallest vertex, so that boxes near x = 4096 behave as boxes
// near 0.
//
// Intersection (cvx_inter): Sutherland-Hodgman of P's hull (at most 9 vertices) against Q's 3 or 4 half-planes, at most 13 vertices,
// then the fan of triangles from the first vertex, clamped at 0.  P = Q clips to itself exactly.
//
// Every list indexed at run time lives in LDS, one column per lane of a 64-lane block (element k of a lane at [k * 64 + lane]), as
// ops_rot.hip's ROT_POLY_FLOATS: a runtime-indexed register array would go to scratch memory.
#pragma once
#include "common.h"
#include <cfloat>
#include <cstdint>

namespace frcnn {

static constexpr int CVX_SET = 9;                 // points of a set
static constexpr int CVX_QUAD = 4;                // vertices of a polygon
static constexpr int CVX_ALL = CVX_SET + CVX_QUAD;
static constexpr float CVX_MIN_AREA = 1e-14f;     // ROT_MIN_AREA's value
static constexpr int CVX_MAX_ROWS = INT32_MAX - 1024;   // rows of any entry point: the grids' ceilings are formed in int

__device__ __forceinline__ bool cvx_finite(float v) { return fabsf(v) <= FLT_MAX; }

// Point i of a lane's column is (p[(2 i) * 64], p[(2 i + 1) * 64]).

// The hull of the n points pts: hull[m * 64] receives the index of vertex m; returns the vertex count (0 for n = 0).
__device__ __forceinline__ int cvx_hull(const float* pts, int n, int* hull)
{
    if (n <= 0) return 0;
    int s = 0;
    float sx = pts[0], sy = pts[64];
    for (int i = 1; i < n; ++i) {
        const float x = pts[(2 * i) * 64], y = pts[(2 * i + 1) * 64];
        if (x < sx || (x == sx && y < sy)) { s = i; sx = x; sy = y; }
    }
    int m = 0, cur = s;
    float cx = sx, cy = sy;
    while (m < n) {
        hull[m * 64] = cur;
        ++m;
        int best = -1;
        float bx = 0.f, by = 0.f;                                      // best - current
        for (int i = 0; i < n; ++i) {
            const float dx = pts[(2 * i) * 64] - cx, dy = pts[(2 * i + 1) * 64] - cy;
            if (dx == 0.f && dy == 0.f) continue;                      // the current vertex and its copies
            if (best < 0) { best = i; bx = dx; by = dy; continue; }
            const float l = bx * dy, r = by * dx;                      // l - r = cross(best - current, point - current)
            if (l < r || (l == r && dx * dx + dy * dy > bx * bx + by * by)) { best = i; bx = dx; by = dy; }
        }
        if (best < 0) break;                                           // every point equals the start
        cur = best;
        cx = pts[(2 * cur) * 64]; cy = pts[(2 * cur + 1) * 64];
        if (cx == sx && cy == sy) break;                               // back at the start
    }
    return m;
}

// The hull of a set on coordinates relative to its own smallest point: raw holds the n points, rel receives raw - origin, (ox, oy) the
// origin.  Returns the vertex count.
__device__ __forceinline__ int cvx_own_hull(const float* raw, int n, float* rel, int* hull, float& ox, float& oy)
{
    ox = raw[0]; oy = raw[64];
    for (int i = 1; i < n; ++i) {
        const float x = raw[(2 * i) * 64], y = raw[(2 * i + 1) * 64];
        if (x < ox || (x == ox && y < oy)) { ox = x; oy = y; }
    }
    for (int i = 0; i < n; ++i) {
        rel[(2 * i) * 64] = raw[(2 * i) * 64] - ox;
        rel[(2 * i + 1) * 64] = raw[(2 * i + 1) * 64] - oy;
    }
    return cvx_hull(rel, n, hull);
}

// The signed area (counter-clockwise positive) of the polygon whose vertex k is point idx[k * 64] of pts: the fan from vertex 0
__device__ __forceinline__ float cvx_hull_area(const float* pts, const int* idx, int m)
{
    float sum = 0.f;
    if (m >= 3) {
        const int i0 = idx[0], i1 = idx[64];
        const float x0 = pts[(2 * i0) * 64], y0 = pts[(2 * i0 + 1) * 64];
        float ex = pts[(2 * i1) * 64] - x0, ey = pts[(2 * i1 + 1) * 64] - y0;
        for (int k = 2; k < m; ++k) {
            const int i = idx[k * 64];
            const float fx = pts[(2 * i) * 64] - x0, fy = pts[(2 * i + 1) * 64] - y0;
            sum = sum + (ex * fy - fx * ey);
            ex = fx; ey = fy;
        }
    }
    return 0.5f * sum;
}

// the same for the vertex list pts itself
__device__ __forceinline__ float cvx_list_area(const float* pts, int m)
{
    float sum = 0.f;
    if (m >= 3) {
        const float x0 = pts[0], y0 = pts[64];
        float ex = pts[2 * 64] - x0, ey = pts[3 * 64] - y0;
        for (int k = 2; k < m; ++k) {
            const float fx = pts[(2 * k) * 64] - x0, fy = pts[(2 * k + 1) * 64] - y0;
            sum = sum + (ex * fy - fx * ey);
            ex = fx; ey = fy;
        }
    }
    return 0.5f * sum;
}

// One Sutherland-Hodgman pass: the part of the polygon `in` (n vertices) on the left of the line through (ax, ay) with direction
// (ex, ey); a vertex on the line is inside.  Returns the new count (at most CVX_ALL).
__device__ __forceinline__ int cvx_clip(const float* in, float* out, int n, float ax, float ay, float ex, float ey)
{
    if (n == 0) return 0;
    int m = 0;
    float px = in[(2 * (n - 1)) * 64], py = in[(2 * (n - 1) + 1) * 64];
    float pd = ex * (py - ay) - ey * (px - ax);
    for (int i = 0; i < n; ++i) {
        const float qx = in[(2 * i) * 64], qy = in[(2 * i + 1) * 64];
        const float qd = ex * (qy - ay) - ey * (qx - ax);
        if ((pd >= 0.f) != (qd >= 0.f) && m < CVX_ALL) {
            const float t = pd / (pd - qd);
            out[(2 * m) * 64] = px + t * (qx - px);
            out[(2 * m + 1) * 64] = py + t * (qy - py);
            ++m;
        }
        if (qd >= 0.f && m < CVX_ALL) {
            out[(2 * m) * 64] = qx;
            out[(2 * m + 1) * 64] = qy;
            ++m;
        }
        px = qx; py = qy; pd = qd;
    }
    return m;
}

// area(P n Q) >= 0.  p: the np vertices of P's hull, made relative by subtracting (ox, oy); q: the nq vertices of Q's hull, relative
// already.  l0 / l1: two lists of CVX_ALL vertices in the lane's column.
__device__ __forceinline__ float cvx_inter(const float* p, int np, float ox, float oy, const float* q, int nq, float* l0, float* l1)
{
    if (np < 3) return 0.f;                                            // a degenerate set has no area to share
    for (int k = 0; k < np; ++k) {
        l0[(2 * k) * 64] = p[(2 * k) * 64] - ox;
        l0[(2 * k + 1) * 64] = p[(2 * k + 1) * 64] - oy;
    }
    int n = np;
    float* in = l0;
    float* out = l1;
    for (int e = 0; e < nq && n > 0; ++e) {
        const int e1 = e + 1 == nq ? 0 : e + 1;
        const float ax = q[(2 * e) * 64], ay = q[(2 * e + 1) * 64];
        n = cvx_clip(in, out, n, ax, ay, q[(2 * e1) * 64] - ax, q[(2 * e1 + 1) * 64] - ay);
        float* tmp = in; in = out; out = tmp;
    }
    return fmaxf(cvx_list_area(in, n), 0.f);
}

}  // namespace frcnn
