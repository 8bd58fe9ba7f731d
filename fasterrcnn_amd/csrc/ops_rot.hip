// ops_rot.hip -- rotated-box operators of fasterrcnn_amd.ops (oriented detection): box_iou_rotated, nms_rotated and roi_align_rotated
// with its backward: the frcnn_ops_box_iou_rotated / frcnn_ops_nms_rotated / frcnn_ops_roi_align_rotated* entry points of
// include/frcnn_hip.h.  Restated from the published definitions of mmcv's box_iou_rotated, nms_rotated and roi_align_rotated (third
// party, absent here: restated, unpinned); where the two differ the header's text holds.
//
// Box (cx, cy, w, h, angle), float32, angle in radians: local point (u, v), |u| <= w / 2, |v| <= h / 2, lies at
// (cx + u cos a - v sin a, cy + u sin a + v cos a).  The kernels know this one convention; the caller negates angles for the other.
//
// IoU: one device function, rot_iou, for the pairwise kernels and the NMS mask kernel, on per-box records (centre, cos, sin, half
// extents, area, validity) computed once per box and tile and staged in LDS.  Box A's corners are expressed in box B's frame -- the
// centre difference first, so that large common coordinates cancel before any product -- and the quadrilateral is clipped against B's
// four half-planes (Sutherland-Hodgman, at most 8 vertices); the area is the fan of triangles from the first vertex.  Continuous in its
// inputs, unlike the candidate-points-plus-hull method.  The relative rotation is a product of two unit vectors, unit only to rounding:
// where one of its components is exactly zero (parallel or perpendicular boxes, a box against itself among them) the other is set to
// +-1, so that a box clips to itself exactly and IoU(b, b) == 1.  The vertex lists live in LDS, one column per lane (a runtime-indexed
// register array would go to scratch).  A pair is exactly 0 when either box has a non-finite component, a negative side or w h < 1e-14.
//
// Differentiable IoU of aligned pairs (frcnn_ops_diff_iou_rotated*; mmcv's diff_iou_rotated_2d restated): the forward is rot_iou handing
// back the intersection area too; the backward is one launch that clips again with a tag per vertex and sums the closed-form gradient
// over the edges of the final polygon (ops_rot_diff_iou_backward_kernel).
//
// NMS: ops_rot_nms_mask_kernel writes ops_nms_mask_kernel's 64 x 64 bit tiles (ops.hip) with the same diagonal and category skipping,
// bit j of row i = rot_iou(sorted i, sorted j) > thr; ops_nms_reduce_kernel then runs the greedy pass unchanged.
//
// roi_align_rotated: RoI rows (b, cx, cy, w, h, angle); layouts, element types (Run<E>), limits and the batch-index rule are ops.hip's.
// Forward: one block per (RoI, ph), lanes over (pw, channel run).  Backward: no atomics; ops.hip's gather -- one block per 2 x 2 cells
// of one image and 64 channel runs, RoIs culled in ascending order (cull_rois) against the rotated RoI's bounding box grown by two
// pixels, one wave per cell, the sum in registers over every pass, one store.  A rotation is an isometry: a sample can touch a cell
// only if its local coordinates lie within sqrt(2) of the cell's on both local axes, which bounds the candidate sample rows and columns
// analytically (rot_sample_range); every candidate is then tested exactly with the forward's own expressions.  Per RoI the bins are
// visited in (ph, pw) order and a bin sends dout (sum of its samples' weights, in (iy, ix) order) / count.
//
// riroi_align_rotated (frcnn_ops_riroi_align_rotated*; mmcv's riroi_align_rotated restated): roi_align_rotated's pooling of C n channels,
// then each group's n orientation channels rotated by the RoI's angle and blended between the two nearest.  The forward pools and blends
// in one launch through LDS (ops_riroi_align_kernel); the backward is the gather above with the blend where it loads a bin's gradient.
#include "ops_run.h"
#include <cfloat>

namespace frcnn {

static constexpr int ROT_MAX_VERTS = 8;                        // a quadrilateral clipped by four half-planes
static constexpr int ROT_POLY_FLOATS = 2 * ROT_MAX_VERTS * 2 * 64;   // two vertex lists of (x, y) per lane of a 64-thread block
static constexpr float ROT_MIN_AREA = 1e-14f;

// ---- rotated IoU ------------------------------------------------------------------------------------------------------------------
struct RotBox { float cx, cy, c, s, hw, hh, area; int ok; };

__device__ __forceinline__ bool rot_finite(float v) { return fabsf(v) <= FLT_MAX; }

__device__ __forceinline__ RotBox rot_box(const float* p)
{
    RotBox b;
    const float w = p[2], h = p[3], a = p[4];
    b.cx = p[0]; b.cy = p[1];
    b.c = cosf(a); b.s = sinf(a);
    b.hw = 0.5f * w; b.hh = 0.5f * h;
    b.area = w * h;
    b.ok = rot_finite(p[0]) && rot_finite(p[1]) && rot_finite(w) && rot_finite(h) && rot_finite(a) && w >= 0.f && h >= 0.f &&
           b.area >= ROT_MIN_AREA;
    return b;
}

// One Sutherland-Hodgman pass: keeps the part of the polygon `in` (n vertices) with SIGN * coordinate[AXIS] <= bound.  in / out point
// at the lane's column: vertex i is (in[(2 i) * 64], in[(2 i + 1) * 64]).  A vertex on the boundary is inside.
// TAGGED (the differentiable IoU's backward): vertex i carries in bits [3 i, 3 i + 3) of tin / tout the tag of the boundary piece that
// leaves it -- 0..3 an edge of box A, 4 + AXIS + (SIGN < 0 ? 2 : 0) this pass's line.  A kept vertex keeps its tag; a crossing where the
// polygon leaves the half-plane starts a piece of the clip line; one where it enters continues the edge that left p.
template <int AXIS, int SIGN, bool TAGGED = false>
__device__ __forceinline__ int rot_clip(const float* in, float* out, int n, float bound, unsigned tin = 0u, unsigned* tout = nullptr)
{
    constexpr unsigned LINE = 4 + AXIS + (SIGN < 0 ? 2 : 0);
    unsigned tags = 0u;
    if (TAGGED) *tout = 0u;
    if (n == 0) return 0;
    int m = 0;
    float px = in[(2 * (n - 1)) * 64], py = in[(2 * (n - 1) + 1) * 64];
    float pd = (float)SIGN * (AXIS ? py : px);
    bool pin = pd <= bound;
    unsigned ptag = TAGGED ? (tin >> (3 * (n - 1))) & 7u : 0u;
    for (int i = 0; i < n; ++i) {
        const float qx = in[(2 * i) * 64], qy = in[(2 * i + 1) * 64];
        const float qd = (float)SIGN * (AXIS ? qy : qx);
        const bool qin = qd <= bound;
        const unsigned qtag = TAGGED ? (tin >> (3 * i)) & 7u : 0u;
        if (pin != qin && m < ROT_MAX_VERTS) {
            const float t = (bound - pd) / (qd - pd);
            out[(2 * m) * 64] = AXIS ? px + t * (qx - px) : (float)SIGN * bound;
            out[(2 * m + 1) * 64] = AXIS ? (float)SIGN * bound : py + t * (qy - py);
            if (TAGGED) tags |= (pin ? LINE : ptag) << (3 * m);
            ++m;
        }
        if (qin && m < ROT_MAX_VERTS) {
            out[(2 * m) * 64] = qx;
            out[(2 * m + 1) * 64] = qy;
            if (TAGGED) tags |= qtag << (3 * m);
            ++m;
        }
        px = qx; py = qy; pd = qd; pin = qin; ptag = qtag;
    }
    if (TAGGED) *tout = tags;
    return m;
}

// Box a in box b's frame (both ok): its centre, the rotation from a's frame to b's, and its quadrilateral clipped against b's four
// half-planes, left in the first vertex list of the lane's column `poly` of the block's ROT_POLY_FLOATS; returns the vertex count.  The
// four start vertices carry a's edge numbers 0..3: edge 0 is the local +h/2 side, 1 is -w/2, 2 is -h/2, 3 is +w/2.
struct RotFrame { float ox, oy, cd, sd; };

template <bool TAGGED = false>
__device__ __forceinline__ int rot_polygon(const RotBox& a, const RotBox& b, float* poly, RotFrame& f, unsigned* tags = nullptr)
{
    const float dx = a.cx - b.cx, dy = a.cy - b.cy;
    const float ox = dx * b.c + dy * b.s, oy = dy * b.c - dx * b.s;       // a's centre in b's frame
    float cd = a.c * b.c + a.s * b.s, sd = a.s * b.c - a.c * b.s;        // the rotation from a's frame to b's
    if (sd == 0.f) cd = cd < 0.f ? -1.f : 1.f;
    if (cd == 0.f) sd = sd < 0.f ? -1.f : 1.f;
    const float ux = a.hw * cd, uy = a.hw * sd, vx = -a.hh * sd, vy = a.hh * cd;
    float* p0 = poly;
    float* p1 = poly + ROT_MAX_VERTS * 2 * 64;
    p0[0 * 64] = (ox + ux) + vx; p0[1 * 64] = (oy + uy) + vy;
    p0[2 * 64] = (ox - ux) + vx; p0[3 * 64] = (oy - uy) + vy;
    p0[4 * 64] = (ox - ux) - vx; p0[5 * 64] = (oy - uy) - vy;
    p0[6 * 64] = (ox + ux) - vx; p0[7 * 64] = (oy + uy) - vy;
    f.ox = ox; f.oy = oy; f.cd = cd; f.sd = sd;
    unsigned t = 0u | 1u << 3 | 2u << 6 | 3u << 9;
    int n = rot_clip<0, 1, TAGGED>(p0, p1, 4, b.hw, t, &t);
    n = rot_clip<1, 1, TAGGED>(p1, p0, n, b.hh, t, &t);
    n = rot_clip<0, -1, TAGGED>(p0, p1, n, b.hw, t, &t);
    n = rot_clip<1, -1, TAGGED>(p1, p0, n, b.hh, t, &t);
    if (TAGGED) *tags = t;
    return n;
}

// the area of the polygon rot_polygon left (n vertices): the fan of triangles from the first vertex
__device__ __forceinline__ float rot_area(const float* p0, int n)
{
    float sum = 0.f;
    if (n >= 3) {
        const float x0 = p0[0], y0 = p0[64];
        float ex = p0[2 * 64] - x0, ey = p0[3 * 64] - y0;
        for (int i = 2; i < n; ++i) {
            const float fx = p0[(2 * i) * 64] - x0, fy = p0[(2 * i + 1) * 64] - y0;
            sum = sum + (ex * fy - fx * ey);
            ex = fx; ey = fy;
        }
    }
    return 0.5f * fabsf(sum);
}

// iof == 0: inter / (area a + area b - inter); else inter / area a.  poly: the lane's column of the block's ROT_POLY_FLOATS.
// inter_out, when given, receives inter (0 under the zero rule).
__device__ __forceinline__ float rot_iou(const RotBox& a, const RotBox& b, int iof, float* poly, float* inter_out = nullptr)
{
    if (inter_out) *inter_out = 0.f;
    if (!a.ok || !b.ok) return 0.f;
    RotFrame f;
    const int n = rot_polygon(a, b, poly, f);
    const float inter = rot_area(poly, n);
    if (inter_out) *inter_out = inter;
    return iof ? inter / a.area : inter / ((a.area + b.area) - inter);
}

// out[i][j] = rot_iou(boxes1[i], boxes2[j]): grid (ceil(m / 64), ceil(n / 64)), one wave per 64 x 64 tile, a lane per column
__global__ __launch_bounds__(64)
void ops_rot_iou_kernel(const float* __restrict__ boxes1, int n, const float* __restrict__ boxes2, int m, int iof, float* __restrict__ out)
{
    __shared__ float s_poly[ROT_POLY_FLOATS];
    __shared__ RotBox rows[64];
    const int t = threadIdx.x, i0 = blockIdx.y * 64, j = blockIdx.x * 64 + t;
    if (i0 + t < n) rows[t] = rot_box(boxes1 + (size_t)(i0 + t) * 5);
    __syncthreads();
    if (j >= m) return;
    const RotBox b = rot_box(boxes2 + (size_t)j * 5);
    const int imax = min(n - i0, 64);
    for (int i = 0; i < imax; ++i) out[(size_t)(i0 + i) * m + j] = rot_iou(rows[i], b, iof, s_poly + t);
}

// out[i] = rot_iou(boxes1[i], boxes2[i])
__global__ __launch_bounds__(64)
void ops_rot_iou_aligned_kernel(const float* __restrict__ boxes1, const float* __restrict__ boxes2, int n, int iof, float* __restrict__ out)
{
    __shared__ float s_poly[ROT_POLY_FLOATS];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = rot_iou(rot_box(boxes1 + (size_t)i * 5), rot_box(boxes2 + (size_t)i * 5), iof, s_poly + threadIdx.x);
}

// ---- the differentiable IoU of aligned pairs (diff_iou_rotated) ---------------------------------------------------------------------
// iou[i] = rot_iou(boxes1[i], boxes2[i]), bit for bit ops_rot_iou_aligned_kernel's value, and inter[i] the intersection area it divides
__global__ __launch_bounds__(64)
void ops_rot_diff_iou_kernel(const float* __restrict__ boxes1, const float* __restrict__ boxes2, int n, float* __restrict__ iou,
                             float* __restrict__ inter)
{
    __shared__ float s_poly[ROT_POLY_FLOATS];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float area;
    iou[i] = rot_iou(rot_box(boxes1 + (size_t)i * 5), rot_box(boxes2 + (size_t)i * 5), 0, s_poly + threadIdx.x, &area);
    inter[i] = area;
}

__device__ __forceinline__ void rot_store_box(float* __restrict__ d, int i, float v0, float v1, float v2, float v3, float v4)
{
    if (!d) return;
    d += (size_t)i * 5;
    d[0] = v0; d[1] = v1; d[2] = v2; d[3] = v3; d[4] = v4;
}

// The gradients of sum_i (grad_iou[i] iou[i] + grad_inter[i] inter[i]) for the ten parameters of pair i: one lane per pair, no atomics,
// every element of a wanted gradient written once.  The lane clips again, with tags, and sums over the edges of the final polygon: moving
// a boundary line outward at unit speed adds the length L of the polygon's edges that lie on it.  In b's frame, with o a's centre, d the
// relative angle and n_k the outward normal of a's edge k ((-sd, cd), (-cd, -sd), (sd, -cd), (cd, sd)):
//   dI/d(b.hw) = sum of L on x = +-b.hw, dI/d(b.hh) likewise; dI/d(a.hw) = L on edges 1, 3; dI/d(a.hh) = L on edges 0, 2;
//   dI/do = sum over a's edges of L n_k; dI/dd = sum over a's edges of L (n_k . perp(mid - o)), perp(x, y) = (-y, x);
// chained by o = R(-angle_b)(centre_a - centre_b) (so do/d angle_b = (oy, -ox)), d = angle_a - angle_b, w = 2 hw.  With U = Sa + Sb - I the
// adjoint of I is grad_inter + grad_iou (U + I) / U^2 and that of each area S = w h is -grad_iou I / U^2.  A pair under the zero rule, or
// whose polygon has fewer than 3 vertices, gets exact zeros.  grad_iou / grad_inter may be null (zeros), d1 / d2 null (skipped).
__global__ __launch_bounds__(64)
void ops_rot_diff_iou_backward_kernel(const float* __restrict__ boxes1, const float* __restrict__ boxes2, const float* __restrict__ grad_iou,
                                      const float* __restrict__ grad_inter, int n, float* __restrict__ d1, float* __restrict__ d2)
{
    __shared__ float s_poly[ROT_POLY_FLOATS];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* pa = boxes1 + (size_t)i * 5;
    const float* pb = boxes2 + (size_t)i * 5;
    const RotBox a = rot_box(pa), b = rot_box(pb);
    const float* p0 = s_poly + threadIdx.x;
    RotFrame f;
    unsigned tags = 0u;
    const int nv = a.ok && b.ok ? rot_polygon<true>(a, b, s_poly + threadIdx.x, f, &tags) : 0;
    if (nv < 3) {
        rot_store_box(d1, i, 0.f, 0.f, 0.f, 0.f, 0.f);
        rot_store_box(d2, i, 0.f, 0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float inter = rot_area(p0, nv);
    float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f, lbw = 0.f, lbh = 0.f, gd = 0.f;     // lengths per tag; dI/dd
    float px = p0[(2 * (nv - 1)) * 64], py = p0[(2 * (nv - 1) + 1) * 64];
    unsigned tag = (tags >> (3 * (nv - 1))) & 7u;                                    // of the edge p -> q
    for (int v = 0; v < nv; ++v) {
        const float qx = p0[(2 * v) * 64], qy = p0[(2 * v + 1) * 64];
        const float ex = qx - px, ey = qy - py;
        const float len = sqrtf(ex * ex + ey * ey);
        if (tag < 4u) {
            const float nx = tag == 0u ? -f.sd : tag == 1u ? -f.cd : tag == 2u ? f.sd : f.cd;
            const float ny = tag == 0u ? f.cd : tag == 1u ? -f.sd : tag == 2u ? -f.cd : f.sd;
            const float mx = 0.5f * (px + qx) - f.ox, my = 0.5f * (py + qy) - f.oy;
            gd += len * (ny * mx - nx * my);
            l0 += tag == 0u ? len : 0.f; l1 += tag == 1u ? len : 0.f; l2 += tag == 2u ? len : 0.f; l3 += tag == 3u ? len : 0.f;
        } else {
            lbw += (tag & 1u) ? 0.f : len;
            lbh += (tag & 1u) ? len : 0.f;
        }
        px = qx; py = qy;
        tag = (tags >> (3 * v)) & 7u;
    }
    const float gox = f.sd * (l2 - l0) + f.cd * (l3 - l1), goy = f.cd * (l0 - l2) + f.sd * (l3 - l1);     // dI/do
    const float u = (a.area + b.area) - inter;
    const float gi = grad_iou ? grad_iou[i] : 0.f;
    const float g_inter = (grad_inter ? grad_inter[i] : 0.f) + gi * ((u + inter) / (u * u));
    const float g_area = -gi * (inter / (u * u));
    const float gx = g_inter * (gox * b.c - goy * b.s), gy = g_inter * (gox * b.s + goy * b.c);         // to a's centre; b's gets the negative
    rot_store_box(d1, i, gx, gy, g_inter * (0.5f * (l1 + l3)) + g_area * pa[3], g_inter * (0.5f * (l0 + l2)) + g_area * pa[2],
                  g_inter * gd);
    rot_store_box(d2, i, -gx, -gy, g_inter * (0.5f * lbw) + g_area * pb[3], g_inter * (0.5f * lbh) + g_area * pb[2],
                  g_inter * ((gox * f.oy - goy * f.ox) - gd));
}

// ops_nms_mask_kernel (ops.hip) on rotated boxes: the same grid, tiles, skipping and bit layout
__global__ __launch_bounds__(64)
void ops_rot_nms_mask_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ order, const int64_t* __restrict__ cats, int n,
                             int nw, float thr, u64* __restrict__ mask)
{
    const int by = blockIdx.y, bx = blockIdx.x;
    if (bx < by) return;
    if (cats && cats[order[bx * 64]] > cats[order[min(by * 64 + 63, n - 1)]]) return;
    __shared__ float s_poly[ROT_POLY_FLOATS];
    __shared__ RotBox colb[64];
    __shared__ int64_t colc[64];
    const int t = threadIdx.x;
    const int jn = bx * 64 + t;
    if (jn < n) {
        colb[t] = rot_box(boxes + (size_t)order[jn] * 5);
        colc[t] = cats ? cats[order[jn]] : 0;
    }
    __syncthreads();
    const int i = by * 64 + t;
    if (i >= n) return;
    const RotBox a = rot_box(boxes + (size_t)order[i] * 5);
    const int64_t ca = cats ? cats[order[i]] : 0;
    u64 bits = 0ull;
    const int jmax = min(n - bx * 64, 64);
    for (int j = 0; j < jmax; ++j)
        if (bx * 64 + j > i && colc[j] == ca && rot_iou(a, colb[j], 0, s_poly + t) > thr) bits |= 1ull << j;
    mask[(size_t)i * nw + bx] = bits;
}

// ---- roi_align_rotated ------------------------------------------------------------------------------------------------------------
// The sampling plan of one RoI row (b, cx, cy, w, h, angle): centre, the local start (-size / 2), bins, cos and sin of the signed angle.
struct RotGeom { float cx, cy, start_h, start_w, bin_h, bin_w, c, s; int grid_h, grid_w; float count; };

// the adaptive grid ceil(size / out); 0 (no samples) for a size that is not positive, NaN, or beyond 2^30 samples per bin
__device__ __forceinline__ int rot_grid(float size, int n_out, int sampling_ratio)
{
    if (sampling_ratio > 0) return sampling_ratio;
    const float v = ceilf(size / (float)n_out);
    return v > 0.f && v <= 1073741824.f ? (int)v : 0;
}

__device__ __forceinline__ RotGeom rot_geom(const float* roi, float scale, int out_h, int out_w, int sampling_ratio, int aligned,
                                            int clockwise)
{
    RotGeom g;
    const float offset = aligned ? 0.5f : 0.0f;
    g.cx = roi[1] * scale - offset;
    g.cy = roi[2] * scale - offset;
    float rw = roi[3] * scale, rh = roi[4] * scale;
    if (!aligned) { rw = rw < 1.0f ? 1.0f : rw; rh = rh < 1.0f ? 1.0f : rh; }       // a NaN size stays NaN
    const float t = clockwise ? -roi[5] : roi[5];
    g.c = cosf(t); g.s = sinf(t);
    g.bin_h = rh / (float)out_h;
    g.bin_w = rw / (float)out_w;
    g.grid_h = rot_grid(rh, out_h, sampling_ratio);
    g.grid_w = rot_grid(rw, out_w, sampling_ratio);
    g.start_h = -rh / 2.0f;
    g.start_w = -rw / 2.0f;
    g.count = fmaxf((float)g.grid_h * (float)g.grid_w, 1.0f);
    return g;
}

// the image position of the sample at local (yy, xx)
__device__ __forceinline__ void rot_sample(const RotGeom& g, float yy, float xx, float& y, float& x)
{
    x = (yy * g.s + xx * g.c) + g.cx;
    y = (yy * g.c - xx * g.s) + g.cy;
}

// axis_weights / cell_weight behind a range test that NaN fails: a NaN or infinite coordinate never reaches the conversion to an integer
__device__ __forceinline__ bool rot_axis(float v, int n, int& low, int& high, float& wl, float& wh)
{
    if (!(v >= -1.0f && v <= (float)n)) return false;
    return axis_weights(v, n, low, high, wl, wh);
}

__device__ __forceinline__ bool rot_cell_weight(float v, int n, int cell, float& w)
{
    if (!(v >= -1.0f && v <= (float)n)) return false;
    return cell_weight(v, n, cell, w);
}

template <typename E>
__global__ __launch_bounds__(256)
void ops_rot_roi_align_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, const float* __restrict__ rois, int out_h,
                              int out_w, float scale, int sampling_ratio, int aligned, int clockwise, E* __restrict__ out)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    const int r = blockIdx.x, ph = blockIdx.y, C4 = C / R::V;
    const float* roi = rois + (size_t)r * 6;
    E* orow = out + ((size_t)r * out_h + ph) * out_w * C;
    int b;
    if (!roi_image(roi[0], n_img, b)) {
        zero_row(orow, out_w * C4);
        return;
    }
    const RotGeom g = rot_geom(roi, scale, out_h, out_w, sampling_ratio, aligned, clockwise);
    const E* fm = x + (size_t)b * fh * fw * C;
    for (int i = threadIdx.x; i < out_w * C4; i += 256) {
        const int pw = i / C4, c4 = i - pw * C4;
        vec acc = 0.f;
        for (int iy = 0; iy < g.grid_h; ++iy) {
            const float yy = sample_coord(g.start_h, g.bin_h, g.grid_h, ph, iy);
            for (int ix = 0; ix < g.grid_w; ++ix) {
                const float xx = sample_coord(g.start_w, g.bin_w, g.grid_w, pw, ix);
                float y, xs;
                rot_sample(g, yy, xx, y, xs);
                int yl, yh, xl, xh; float hy, ly, hx, lx;
                if (!rot_axis(y, fh, yl, yh, hy, ly) || !rot_axis(xs, fw, xl, xh, hx, lx)) continue;
                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                const vec v1 = R::load(fm + ((size_t)yl * fw + xl) * C, c4);
                const vec v2 = R::load(fm + ((size_t)yl * fw + xh) * C, c4);
                const vec v3 = R::load(fm + ((size_t)yh * fw + xl) * C, c4);
                const vec v4 = R::load(fm + ((size_t)yh * fw + xh) * C, c4);
                acc = acc + (((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4);
            }
        }
        R::store(orow, i, acc / g.count);
    }
}

// ---- riroi_align_rotated (ReDet's rotation-invariant RoI pooling) --------------------------------------------------------------------
// Channel c n + o of the map is orientation o of group c (n = num_orientations).  The operator is roi_align_rotated's pooled S (aligned
// off, the opposite clockwise flag) with each group's orientations rotated by the RoI's angle: with f = angle n / (2 pi) formed in
// double and rounded once, ind = floor(f), l = f - ind, r = 1 - l, k = ind mod n >= 0,
//   out[c n + o] = r S[c n + (o - k) mod n] + l S[c n + (o - k + 1) mod n].
static constexpr int RIROI_MAX_ORIENTATIONS = 64;    // a group, wherever it starts in its run, lies inside the 64 runs of one wave

struct RiBlend { float l, r; int k; };

// false: the RoI pools to zeros and sends no gradient (a non-finite angle, |f| >= 2^24)
__device__ __forceinline__ bool riroi_blend(float angle, int n, RiBlend& b)
{
    if (!rot_finite(angle)) return false;
    const float f = (float)((double)angle * (double)n / 6.283185307179586);
    if (!(fabsf(f) < 16777216.f)) return false;
    const float ind = floorf(f);
    b.l = f - ind;
    b.r = 1.0f - b.l;
    const int k = (int)ind % n;
    b.k = k < 0 ? k + n : k;
    return true;
}

// Forward: roi_align_rotated's loop, one block per (RoI, ph), but a wave owns whole (pw, channel chunk) pieces: `cl` lanes hold the
// pooled runs of one piece, 64 / cl pieces share a wave when the channels are few.  chunk_runs is a multiple of lcm(n, V) / V, so a
// chunk starts on a group's first channel and no group leaves its piece: the pooled runs go to the wave's LDS row, each lane blends its
// run's channels from there and stores once.  Channels from c_real on belong to no group and are written as zeros.
template <typename E>
__global__ __launch_bounds__(256)
void ops_riroi_align_kernel(const E* __restrict__ x, int n_img, int fh, int fw, int C, int c_real, const float* __restrict__ rois,
                            int out_h, int out_w, float scale, int sampling_ratio, int clockwise, int n_orient, int chunk_runs,
                            E* __restrict__ out)
{
    typedef Run<E> R;
    typedef typename R::vec vec;
    constexpr int V = R::V;
    __shared__ float s_pool[4][64 * V];
    const int r = blockIdx.x, ph = blockIdx.y, C4 = C / V;
    const float* roi = rois + (size_t)r * 6;
    E* orow = out + ((size_t)r * out_h + ph) * out_w * C;
    int b;
    RiBlend bl;
    if (!roi_image(roi[0], n_img, b) || !riroi_blend(roi[5], n_orient, bl)) {
        zero_row(orow, out_w * C4);
        return;
    }
    const RotGeom g = rot_geom(roi, scale, out_h, out_w, sampling_ratio, 0, !clockwise);
    const E* fm = x + (size_t)b * fh * fw * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_chunks = (C4 + chunk_runs - 1) / chunk_runs;
    const int cl = n_chunks == 1 ? C4 : chunk_runs;                // <= 64
    const int ppw = 64 / cl;                                       // pieces (bins pw) of a wave
    const int sub = lane / cl, li = lane - sub * cl;
    const int total = ((out_w + ppw - 1) / ppw) * n_chunks;
    float* pool = s_pool[wave] + (sub < ppw ? sub * cl * V : 0);
    for (int it0 = 0; it0 < total; it0 += 4) {                     // uniform over the block: the barriers below
        const int item = it0 + wave;
        const int pwg = item / n_chunks, ck = item - pwg * n_chunks;
        const int pw = pwg * ppw + sub, r0 = ck * chunk_runs, c4 = r0 + li;
        const bool act = item < total && sub < ppw && pw < out_w && c4 < C4;
        if (act) {
            vec acc = 0.f;
            for (int iy = 0; iy < g.grid_h; ++iy) {
                const float yy = sample_coord(g.start_h, g.bin_h, g.grid_h, ph, iy);
                for (int ix = 0; ix < g.grid_w; ++ix) {
                    const float xx = sample_coord(g.start_w, g.bin_w, g.grid_w, pw, ix);
                    float y, xs;
                    rot_sample(g, yy, xx, y, xs);
                    int yl, yh, xl, xh; float hy, ly, hx, lx;
                    if (!rot_axis(y, fh, yl, yh, hy, ly) || !rot_axis(xs, fw, xl, xh, hx, lx)) continue;
                    const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                    const vec v1 = R::load(fm + ((size_t)yl * fw + xl) * C, c4);
                    const vec v2 = R::load(fm + ((size_t)yl * fw + xh) * C, c4);
                    const vec v3 = R::load(fm + ((size_t)yh * fw + xl) * C, c4);
                    const vec v4 = R::load(fm + ((size_t)yh * fw + xh) * C, c4);
                    acc = acc + (((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4);
                }
            }
            acc = acc / g.count;
#pragma unroll
            for (int j = 0; j < V; ++j) pool[li * V + j] = acc[j];
        }
        __syncthreads();
        if (act) {
            vec o;
            int base = c4 * V / n_orient * n_orient, ori = c4 * V - base;        // of the run's first channel; one division per run
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float v = 0.f;
                if (c4 * V + j < c_real) {
                    int s1 = ori - bl.k;
                    s1 = s1 < 0 ? s1 + n_orient : s1;
                    const int s2 = s1 + 1 == n_orient ? 0 : s1 + 1;
                    const float* grp = pool + (base - r0 * V);
                    v = bl.r * grp[s1] + bl.l * grp[s2];
                }
                o[j] = v;
                if (++ori == n_orient) { ori = 0; base += n_orient; }
            }
            R::store(orow, (size_t)pw * C4 + c4, o);
        }
        __syncthreads();                                           // the next piece overwrites the row
    }
}

// Backward: what a lane of the gather knows of its run's V channels -- per channel the first channel of its group (-1: no group) and its
// orientation -- and the pooled gradient blended from the gradient row of one bin (gp [C]):
//   dS[c n + j] = r dout[c n + (j + k) mod n] + l dout[c n + (j + k - 1) mod n].
template <int V> struct RiLane { int base[V], o[V]; };

template <int V>
__device__ __forceinline__ RiLane<V> riroi_lane(int c4, int n, int c_real)
{
    RiLane<V> rl;
    int base = c4 * V / n * n, o = c4 * V - base;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const bool real = c4 * V + j < c_real;
        rl.base[j] = real ? base : -1;
        rl.o[j] = real ? o : 0;
        if (++o == n) { o = 0; base += n; }
    }
    return rl;
}

template <typename E>
__device__ __forceinline__ typename Run<E>::vec riroi_grad(const E* __restrict__ gp, const RiLane<Run<E>::V>& rl, const RiBlend& bl, int n)
{
    typename Run<E>::vec v;
#pragma unroll
    for (int j = 0; j < Run<E>::V; ++j) {
        float d = 0.f;
        if (rl.base[j] >= 0) {
            int a = rl.o[j] + bl.k;
            a = a >= n ? a - n : a;
            const int p = a == 0 ? n - 1 : a - 1;
            d = bl.r * Run<E>::at(gp, rl.base[j] + a) + bl.l * Run<E>::at(gp, rl.base[j] + p);
        }
        v[j] = d;
    }
    return v;
}

// The sample positions s = p * grid + i (0 <= s < n_out * grid) whose local coordinate can lie within `radius` of loc: the linear model
// of the positions (start + (s + 0.5) bin / grid), widened by one sample and a relative margin for rounding; the caller evaluates every
// candidate exactly.  ops.hip's sample_range around a local coordinate.
__device__ __forceinline__ void rot_sample_range(float loc, float radius, float start, float bin, int grid, int n_out, int& s_lo, int& s_hi)
{
    const long long last = min((long long)n_out * grid, (long long)INT32_MAX) - 1;      // grid >= 1 here
    const float step = bin / (float)grid;
    if (!(step > 0.f)) { s_lo = 0; s_hi = (int)last; return; }
    const float pad = 1.0f + 1e-4f * (fabsf(start) + fabsf(bin) * (float)n_out + 2.0f) / step;
    const float a = ((loc - radius) - start) / step - 0.5f - pad;
    const float e = ((loc + radius) - start) / step - 0.5f + pad;
    // clamped in float first (the conversion of an out-of-range float is undefined), then exactly in integers
    s_lo = (int)fminf(fmaxf(floorf(a), 0.f), 2.0e9f);
    s_hi = (int)min((long long)fmaxf(fminf(ceilf(e), 2.0e9f), -1.0f), last);
}

// whether a RoI's samples can touch the tile of cells [ty0, ty1] x [tx0, tx1]: the bounding box of the rotated rectangle that holds
// every sample, grown by one pixel for the bilinear footprint and one more (and a relative margin) for rounding.  NaN fails every test.
__device__ __forceinline__ bool rot_touches_tile(const RotGeom& g, int ty0, int ty1, int tx0, int tx1)
{
    if (g.grid_h <= 0 || g.grid_w <= 0) return false;
    const float ex = fabsf(g.start_w * g.c) + fabsf(g.start_h * g.s), ey = fabsf(g.start_w * g.s) + fabsf(g.start_h * g.c);
    const float m = 2.0f + 1e-5f * (((fabsf(g.cx) + fabsf(g.cy)) + ex) + ey);
    return (g.cx + ex) + m >= (float)tx0 && (g.cx - ex) - m <= (float)tx1 && (g.cy + ey) + m >= (float)ty0 && (g.cy - ey) - m <= (float)ty1;
}

// Adds to acc the gradient that one RoI (plan g) sends to cell (cy, cx) for the lane's channel run: load(bin) is the RoI's output gradient
// of that run at bin ph * out_w + pw, as float32
template <typename E, typename Load>
__device__ __forceinline__ void rot_cell_grad(const RotGeom& g, Load load, int fh, int fw, int cy, int cx, int out_h, int out_w, bool act,
                                              typename Run<E>::vec& acc)
{
    // the cell in the RoI's local frame (the inverse of rot_sample); a touching sample is within sqrt(2) of it on both local axes
    const float dx = (float)cx - g.cx, dy = (float)cy - g.cy;
    const float lx = dx * g.c - dy * g.s, ly = dx * g.s + dy * g.c;
    const float radius = 1.5f + 1e-5f * (fabsf(dx) + fabsf(dy));
    int ys0, ys1, xs0, xs1;
    rot_sample_range(ly, radius, g.start_h, g.bin_h, g.grid_h, out_h, ys0, ys1);
    rot_sample_range(lx, radius, g.start_w, g.bin_w, g.grid_w, out_w, xs0, xs1);
    for (int sy = ys0; sy <= ys1; ) {
        const int ph = sy / g.grid_h;
        const int y_end = (int)min((long long)ys1, (long long)(ph + 1) * g.grid_h - 1);
        for (int sx = xs0; sx <= xs1; ) {
            const int pw = sx / g.grid_w;
            const int x_end = (int)min((long long)xs1, (long long)(pw + 1) * g.grid_w - 1);
            float w_sum = 0.f;
            bool hit = false;
            for (int s = sy; s <= y_end; ++s) {
                const float yy = sample_coord(g.start_h, g.bin_h, g.grid_h, ph, s - ph * g.grid_h);
                for (int q = sx; q <= x_end; ++q) {
                    const float xx = sample_coord(g.start_w, g.bin_w, g.grid_w, pw, q - pw * g.grid_w);
                    float y, xs, wy, wx;
                    rot_sample(g, yy, xx, y, xs);
                    if (rot_cell_weight(y, fh, cy, wy) && rot_cell_weight(xs, fw, cx, wx)) {
                        w_sum += wy * wx;
                        hit = true;
                    }
                }
            }
            if (hit && act) acc = acc + (load((size_t)ph * out_w + pw) * w_sum) / g.count;
            sx = x_end + 1;
        }
        sy = y_end + 1;
    }
}

// RIROI (riroi_align_rotated's backward, below): dout is the gradient of the blended output; the pooled gradient dS a bin sends is blended
// from it on the fly (riroi_grad), a RoI that riroi_blend refuses is never listed, and the channels from c_real on belong to no group.
template <typename E, bool RIROI>
__global__ __launch_bounds__(256)
void ops_rot_roi_align_backward_kernel(const float* __restrict__ rois, int k, int n_img, int fh, int fw, int C, int out_h, int out_w,
                                       float scale, int sampling_ratio, int aligned, int clockwise, int n_orient, int c_real,
                                       const E* __restrict__ dout, E* __restrict__ dx)
{
    __shared__ int s_list[OPS_LIST];
    __shared__ int s_cnt[4];
    __shared__ int s_n;
    const int C4 = C / Run<E>::V, n_chunks = (C4 + 63) >> 6;
    const int img = blockIdx.z / n_chunks, chunk = blockIdx.z - img * n_chunks;
    const int ty0 = blockIdx.y * OPS_TILE, tx0 = blockIdx.x * OPS_TILE;
    const int ty1 = min(ty0 + OPS_TILE, fh) - 1, tx1 = min(tx0 + OPS_TILE, fw) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = chunk * 64 + lane;
    const bool act = c4 < C4;
    const int cy = ty0 + wave / OPS_TILE, cx = tx0 + wave % OPS_TILE;       // this wave's cell, for every pass
    const bool cell_ok = cy <= ty1 && cx <= tx1;

    auto touches = [&](int r) {
        const float* roi = rois + (size_t)r * 6;
        int b;
        if (!roi_image(roi[0], n_img, b) || b != img) return false;
        RiBlend bl;
        if (RIROI && !riroi_blend(roi[5], n_orient, bl)) return false;
        return rot_touches_tile(rot_geom(roi, scale, out_h, out_w, sampling_ratio, aligned, clockwise), ty0, ty1, tx0, tx1);
    };

    RiLane<Run<E>::V> rl;
    if constexpr (RIROI) rl = riroi_lane<Run<E>::V>(c4, n_orient, c_real);
    typename Run<E>::vec acc = 0.f;
    int r_next = 0;
    do {
        r_next = cull_rois(r_next, k, touches, s_list, s_cnt, &s_n);
        const int n_list = s_n;
        if (cell_ok)
            for (int li = 0; li < n_list; ++li) {
                const int r = s_list[li];
                const float* roi = rois + (size_t)r * 6;
                const E* dr = dout + (size_t)r * out_h * out_w * C;
                const RotGeom g = rot_geom(roi, scale, out_h, out_w, sampling_ratio, aligned, clockwise);
                if constexpr (RIROI) {
                    RiBlend bl;
                    riroi_blend(roi[5], n_orient, bl);                 // a listed RoI passed it
                    rot_cell_grad<E>(g, [&](size_t bin) { return riroi_grad<E>(dr + bin * C, rl, bl, n_orient); }, fh, fw, cy, cx, out_h,
                                     out_w, act, acc);
                } else {
                    rot_cell_grad<E>(g, [&](size_t bin) { return Run<E>::load(dr, bin * C4 + c4); }, fh, fw, cy, cx, out_h, out_w, act, acc);
                }
            }
    } while (r_next < k);
    if (cell_ok && act) Run<E>::store(dx + (size_t)img * fh * fw * C, ((size_t)cy * fw + cx) * C4 + c4, acc);
}

// ---- the entry points' bodies -------------------------------------------------------------------------------------------------------
// roi_align's limits (roi_args_ok) and the backward grid's tile rows
static bool rot_args_ok(int n_img, int fh, int fw, int c, int k, int out_h, int out_w, int sampling_ratio, int v)
{
    return roi_args_ok(n_img, fh, fw, c, k, out_h, out_w, v) && sampling_ratio <= OPS_MAX_SAMPLING && fh <= 65535 * OPS_TILE;
}

template <typename E>
static int rot_roi_align_impl(const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                              float spatial_scale, int sampling_ratio, int aligned, int clockwise, void* d_out, void* stream)
{
    if (!rot_args_ok(n_img, fh, fw, c, k, out_h, out_w, sampling_ratio, Run<E>::V)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_rot_roi_align_kernel<E>, dim3(k, out_h), dim3(256), 0, (hipStream_t)stream, static_cast<const E*>(d_x), n_img,
                       fh, fw, c, d_rois, out_h, out_w, spatial_scale, sampling_ratio, aligned ? 1 : 0, clockwise ? 1 : 0,
                       static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int rot_roi_align_backward_impl(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                       float spatial_scale, int sampling_ratio, int aligned, int clockwise, const void* d_dout, void* d_dx,
                                       void* stream)
{
    if (!rot_args_ok(n_img, fh, fw, c, k, out_h, out_w, sampling_ratio, Run<E>::V)) return FRCNN_EINVAL;
    if (!d_dx || (k > 0 && (!d_rois || !d_dout))) return FRCNN_EINVAL;
    hipLaunchKernelGGL((ops_rot_roi_align_backward_kernel<E, false>),
                       dim3(cdiv(fw, OPS_TILE), cdiv(fh, OPS_TILE), n_img * cdiv(c / Run<E>::V, 64)), dim3(256), 0, (hipStream_t)stream, d_rois,
                       k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, aligned ? 1 : 0, clockwise ? 1 : 0, 1, c,
                       static_cast<const E*>(d_dout), static_cast<E*>(d_dx));
    return check_launch();
}

// c: the channels in memory (whole runs); c_real <= c of them form groups of n_orient
static bool riroi_args_ok(int n_img, int fh, int fw, int c, int c_real, int k, int out_h, int out_w, int num_samples, int n_orient, int v)
{
    return rot_args_ok(n_img, fh, fw, c, k, out_h, out_w, num_samples, v) && n_orient >= 1 && n_orient <= RIROI_MAX_ORIENTATIONS &&
           c_real >= n_orient && c_real <= c && c_real % n_orient == 0;
}

static int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

template <typename E>
static int riroi_align_impl(const void* d_x, int n_img, int fh, int fw, int c, int c_real, const float* d_rois, int k, int out_h, int out_w,
                            float spatial_scale, int num_samples, int n_orient, int clockwise, void* d_out, void* stream)
{
    constexpr int V = Run<E>::V;
    if (!riroi_args_ok(n_img, fh, fw, c, c_real, k, out_h, out_w, num_samples, n_orient, V)) return FRCNN_EINVAL;
    if (k == 0) return FRCNN_OK;
    if (!d_x || !d_rois || !d_out) return FRCNN_EINVAL;
    const int period = n_orient / gcd_int(n_orient, V);            // runs after which groups and runs line up again: <= 64
    hipLaunchKernelGGL(ops_riroi_align_kernel<E>, dim3(k, out_h), dim3(256), 0, (hipStream_t)stream, static_cast<const E*>(d_x), n_img, fh,
                       fw, c, c_real, d_rois, out_h, out_w, spatial_scale, num_samples, clockwise ? 1 : 0, n_orient, 64 / period * period,
                       static_cast<E*>(d_out));
    return check_launch();
}

template <typename E>
static int riroi_align_backward_impl(const float* d_rois, int k, int n_img, int fh, int fw, int c, int c_real, int out_h, int out_w,
                                     float spatial_scale, int num_samples, int n_orient, int clockwise, const void* d_dout, void* d_dx,
                                     void* stream)
{
    if (!riroi_args_ok(n_img, fh, fw, c, c_real, k, out_h, out_w, num_samples, n_orient, Run<E>::V)) return FRCNN_EINVAL;
    if (!d_dx || (k > 0 && (!d_rois || !d_dout))) return FRCNN_EINVAL;
    hipLaunchKernelGGL((ops_rot_roi_align_backward_kernel<E, true>),
                       dim3(cdiv(fw, OPS_TILE), cdiv(fh, OPS_TILE), n_img * cdiv(c / Run<E>::V, 64)), dim3(256), 0, (hipStream_t)stream, d_rois,
                       k, n_img, fh, fw, c, out_h, out_w, spatial_scale, num_samples, 0, clockwise ? 0 : 1, n_orient, c_real,
                       static_cast<const E*>(d_dout), static_cast<E*>(d_dx));
    return check_launch();
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_box_iou_rotated(const float* d_boxes1, int n, const float* d_boxes2, int m, int mode, int aligned, float* d_out, void* stream)
{
    if (n < 0 || m < 0 || (mode != 0 && mode != 1) || (aligned && n != m) || cdiv(n, 64) > 65535) return FRCNN_EINVAL;
    if (n == 0 || m == 0) return FRCNN_OK;
    if (!d_boxes1 || !d_boxes2 || !d_out) return FRCNN_EINVAL;
    if (aligned)
        hipLaunchKernelGGL(ops_rot_iou_aligned_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_boxes1, d_boxes2, n, mode,
                           d_out);
    else
        hipLaunchKernelGGL(ops_rot_iou_kernel, dim3(cdiv(m, 64), cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_boxes1, n, d_boxes2, m,
                           mode, d_out);
    return check_launch();
}

int frcnn_ops_diff_iou_rotated(const float* d_boxes1, const float* d_boxes2, int n, float* d_iou, float* d_inter, void* stream)
{
    if (n < 0 || cdiv(n, 64) > 65535) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_boxes1 || !d_boxes2 || !d_iou || !d_inter) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_rot_diff_iou_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_boxes1, d_boxes2, n, d_iou, d_inter);
    return check_launch();
}

int frcnn_ops_diff_iou_rotated_backward(const float* d_boxes1, const float* d_boxes2, const float* d_grad_iou, const float* d_grad_inter,
                                        int n, float* d_dboxes1, float* d_dboxes2, void* stream)
{
    if (n < 0 || cdiv(n, 64) > 65535) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_boxes1 || !d_boxes2 || !(d_grad_iou || d_grad_inter) || !(d_dboxes1 || d_dboxes2)) return FRCNN_EINVAL;
    hipLaunchKernelGGL(ops_rot_diff_iou_backward_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, d_boxes1, d_boxes2,
                       d_grad_iou, d_grad_inter, n, d_dboxes1, d_dboxes2);
    return check_launch();
}

int frcnn_ops_nms_rotated(const float* d_boxes, const int64_t* d_order, const int64_t* d_categories, int n, float iou_threshold,
                          uint8_t* d_keep, void* d_ws, size_t ws_bytes, void* stream)
{
    if (n < 0 || n > 64 * OPS_NMS_MAX_WORDS) return FRCNN_EINVAL;
    if (n == 0) return FRCNN_OK;
    if (!d_boxes || !d_order || !d_keep || !d_ws || ws_bytes < frcnn_ops_nms_workspace_bytes(n)) return FRCNN_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    const int nw = cdiv(n, 64);
    u64* mask = static_cast<u64*>(d_ws);
    hipLaunchKernelGGL(ops_rot_nms_mask_kernel, dim3(nw, nw), dim3(64), 0, s, d_boxes, d_order, d_categories, n, nw, iou_threshold, mask);
    const int rc = check_launch();
    if (rc) return rc;
    return launch_ops_nms_reduce(mask, d_order, d_categories, n, nw, d_keep, s);
}

int frcnn_ops_roi_align_rotated_cull_list(void) { return OPS_LIST; }

int frcnn_ops_roi_align_rotated(const float* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h, int out_w,
                                float spatial_scale, int sampling_ratio, int aligned, int clockwise, float* d_out, void* stream)
{
    return rot_roi_align_impl<float>(d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale, sampling_ratio, aligned, clockwise,
                                     d_out, stream);
}

int frcnn_ops_roi_align_rotated_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h, int out_w,
                                         float spatial_scale, int sampling_ratio, int aligned, int clockwise, const float* d_dout,
                                         float* d_dx, void* stream)
{
    return rot_roi_align_backward_impl<float>(d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale, sampling_ratio, aligned, clockwise,
                                              d_dout, d_dx, stream);
}

int frcnn_ops_roi_align_rotated_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, const float* d_rois, int k, int out_h,
                                   int out_w, float spatial_scale, int sampling_ratio, int aligned, int clockwise, void* d_out,
                                   void* stream)
{
    OPS_DISPATCH_16(elem_type, c, OPS_HALF_RUN, rot_roi_align_impl, d_x, n_img, fh, fw, c, d_rois, k, out_h, out_w, spatial_scale,
                    sampling_ratio, aligned, clockwise, d_out, stream);
}

int frcnn_ops_roi_align_rotated_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int out_h,
                                            int out_w, float spatial_scale, int sampling_ratio, int aligned, int clockwise,
                                            const void* d_dout, void* d_dx, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), rot_roi_align_backward_impl, d_rois, k, n_img, fh, fw, c, out_h, out_w, spatial_scale,
                    sampling_ratio, aligned, clockwise, d_dout, d_dx, stream);
}

int frcnn_ops_riroi_align_rotated_max_orientations(void) { return RIROI_MAX_ORIENTATIONS; }

int frcnn_ops_riroi_align_rotated(const float* d_x, int n_img, int fh, int fw, int c, int c_real, const float* d_rois, int k, int out_h,
                                  int out_w, float spatial_scale, int num_samples, int num_orientations, int clockwise, float* d_out,
                                  void* stream)
{
    return riroi_align_impl<float>(d_x, n_img, fh, fw, c, c_real, d_rois, k, out_h, out_w, spatial_scale, num_samples, num_orientations,
                                   clockwise, d_out, stream);
}

int frcnn_ops_riroi_align_rotated_backward(const float* d_rois, int k, int n_img, int fh, int fw, int c, int c_real, int out_h, int out_w,
                                           float spatial_scale, int num_samples, int num_orientations, int clockwise, const float* d_dout,
                                           float* d_dx, void* stream)
{
    return riroi_align_backward_impl<float>(d_rois, k, n_img, fh, fw, c, c_real, out_h, out_w, spatial_scale, num_samples,
                                            num_orientations, clockwise, d_dout, d_dx, stream);
}

int frcnn_ops_riroi_align_rotated_16(int elem_type, const void* d_x, int n_img, int fh, int fw, int c, int c_real, const float* d_rois,
                                     int k, int out_h, int out_w, float spatial_scale, int num_samples, int num_orientations,
                                     int clockwise, void* d_out, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, OPS_HALF_RUN, riroi_align_impl, d_x, n_img, fh, fw, c, c_real, d_rois, k, out_h, out_w, spatial_scale,
                    num_samples, num_orientations, clockwise, d_out, stream);
}

int frcnn_ops_riroi_align_rotated_backward_16(int elem_type, const float* d_rois, int k, int n_img, int fh, int fw, int c, int c_real,
                                              int out_h, int out_w, float spatial_scale, int num_samples, int num_orientations,
                                              int clockwise, const void* d_dout, void* d_dx, void* stream)
{
    OPS_DISPATCH_16(elem_type, c, backward_run(c), riroi_align_backward_impl, d_rois, k, n_img, fh, fw, c, c_real, out_h, out_w,
                    spatial_scale, num_samples, num_orientations, clockwise, d_dout, d_dx, stream);
}

}  // extern "C"
