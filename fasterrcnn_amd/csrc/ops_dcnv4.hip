// ops_dcnv4.hip -- DCNv4, the deformable convolution v4 of the FlashInternImage backbones, in both directions: the frcnn_ops_dcnv4* entry
// points of include/frcnn_hip.h.  Restated from the published operator (third party, absent here: restated, unpinned, like the other
// operators of fasterrcnn_amd.ops; where the two differ include/frcnn_hip.h holds).
//
//   offset_mask float32 [n][Ho][Wo][L], one record a pixel: the slice of group g at [3 P g, 3 P (g + 1)), inside it (dx, dy) of point p at
//   [2 p, 2 p + 1] and its mask value (not soft-maxed: unbounded, signed) at [2 P + p]; L = ceil(3 G P / 8) 8, the last L - 3 G P words
//   are padding: never read, their gradient written as zeros.  P = kh kw, or kh kw - 1 with remove_center (kh == kw, odd, >= 3): the
//   grid point (kw / 2, kh / 2) is left out and the later points move down by one.  This is the DcPacked layout of ops_dcn.h, which
//   holds the sampling rule, the mapping and the kernels (shared with ops_dcnv3.hip: with remove_center == 0 the two operators agree
//   bit for bit).  A block stages the slices of its items from the records directly: one coalesced pass of 16-byte loads over the span
//   from its first item's slice to its last one's, the words of the pad and of neighbouring blocks' items dropped, so the staging holds
//   for a block that begins or ends inside a record and across the gap between two records.
#include "ops_dcn.h"

namespace frcnn {

static inline int dcnv4_record(int g, int p) { return (3 * g * p + 7) / 8 * 8; }

// the arguments of one call, checked (false: FRCNN_EINVAL), and the record's length
static bool dcnv4_geom(int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                       float offset_scale, int remove_center, DcGeom& s, int& L)
{
    if (!dc_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, remove_center, s)) return false;
    L = dcnv4_record(g, s.K);                            // 4 G P <= 2^31 - 1025 (the plan's entries), so 3 G P + 7 fits an int
    return true;
}

template <typename E>
static int dcnv4_forward_impl(const void* input, const float* om, int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw,
                              int ph, int pw, int dh, int dw, float offset_scale, int remove_center, void* out, void* stream)
{
    DcGeom s;
    int L;
    if (!dcnv4_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, remove_center, s, L) || !input || !om || !out)
        return FRCNN_EINVAL;
    return dc_forward<E>(input, DcPacked{om, nullptr, L, aligned16(om)}, n_img, s, gc, out, stream);
}

template <typename E>
static int dcnv4_backward_offset_mask_impl(const void* input, const float* om, const void* dout, int n_img, int h, int w, int g, int gc,
                                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale,
                                           int remove_center, float* dom, void* stream)
{
    DcGeom s;
    int L;
    if (!dcnv4_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, remove_center, s, L) || !input || !om || !dout || !dom)
        return FRCNN_EINVAL;
    return dc_backward_offset<E>(input, dout, DcPacked{om, dom, L, aligned16(om)}, n_img, s, gc, stream);
}

static int dcnv4_backward_input(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout,
                                int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                int remove_center, void* dinput, void* ws, size_t ws_bytes, void* stream)
{
    DcGeom s;
    int L;
    if (!dcnv4_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, 1.0f, remove_center, s, L)) return FRCNN_EINVAL;
    return dc_backward_input(elem_type, sorted_keys, order, wts, dout, n_img, h, w, s, gc, dinput, ws, ws_bytes, stream);
}

// kernel and remove_center alone: the points an item samples, 0 for a bad combination
static int dcnv4_points(int kh, int kw, int remove_center)
{
    if (kh < 1 || kh > DCN_MAX_KERNEL || kw < 1 || kw > DCN_MAX_KERNEL) return 0;
    if (remove_center != 0 && (remove_center != 1 || kh != kw || kh % 2 == 0 || kh < 3)) return 0;
    return kh * kw - remove_center;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_dcnv4_record(int g, int kernel_h, int kernel_w, int remove_center)
{
    const int p = dcnv4_points(kernel_h, kernel_w, remove_center);
    if (p == 0 || g < 1 || g > MSDA_MAX_INDEX / (4LL * p)) return 0;
    return dcnv4_record(g, p);
}

int frcnn_ops_dcnv4_block_items(int gc, int kernel_h, int kernel_w, int remove_center, int elem_type)
{
    const int p = dcnv4_points(kernel_h, kernel_w, remove_center);
    if (p == 0 || gc < 1 || gc > MSDA_MAX_CHANNELS) return 0;
    if (elem_type != 0 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return 0;
    const int run = elem_type == 0 ? MsElem<float>::RUN : MsElem<f16>::RUN;
    return ms_map(gc, p, run, gc % run == 0).ipb;
}

size_t frcnn_ops_dcnv4_workspace_bytes(int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w, int remove_center)
{
    DcGeom s;
    int L;
    if (!dcnv4_geom(n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, 1.0f, remove_center, s, L))
        return 0;
    return msda_gather_workspace(n_img * h * w * g, (int)(dc_items(n_img, s) * s.K * 4), gc);
}

int frcnn_ops_dcnv4_forward(const float* d_input, const float* d_offset_mask, int n_img, int h, int w, int g, int gc, int kernel_h,
                            int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale,
                            int remove_center, float* d_out, void* stream)
{
    return dcnv4_forward_impl<float>(d_input, d_offset_mask, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h,
                                     dil_w, offset_scale, remove_center, d_out, stream);
}

int frcnn_ops_dcnv4_backward_offset_mask(const float* d_input, const float* d_offset_mask, const float* d_dout, int n_img, int h, int w,
                                         int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                         int dil_h, int dil_w, float offset_scale, int remove_center, float* d_doffset_mask, void* stream)
{
    return dcnv4_backward_offset_mask_impl<float>(d_input, d_offset_mask, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                                                  pad_h, pad_w, dil_h, dil_w, offset_scale, remove_center, d_doffset_mask, stream);
}

int frcnn_ops_dcnv4_plan(const float* d_offset_mask, int n_img, int h, int w, int g, int kernel_h, int kernel_w, int stride_h, int stride_w,
                         int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, int remove_center, int64_t* d_keys,
                         float* d_weights, void* stream)
{
    DcGeom s;
    int L;
    if (!dcnv4_geom(n_img, h, w, g, 1, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, remove_center, s,
                    L) || !d_offset_mask || !d_keys || !d_weights)
        return FRCNN_EINVAL;
    return dc_plan(DcPacked{d_offset_mask, nullptr, L, 0}, n_img, h, w, s, d_keys, d_weights, stream);
}

int frcnn_ops_dcnv4_backward_input(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                   int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dil_h, int dil_w, int remove_center, float* d_dinput, void* d_ws,
                                   size_t ws_bytes, void* stream)
{
    return dcnv4_backward_input(0, d_sorted_keys, d_order, d_weights, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                                pad_h, pad_w, dil_h, dil_w, remove_center, d_dinput, d_ws, ws_bytes, stream);
}

int frcnn_ops_dcnv4_forward_16(int elem_type, const void* d_input, const float* d_offset_mask, int n_img, int h, int w, int g, int gc,
                               int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                               float offset_scale, int remove_center, void* d_out, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, dcnv4_forward_impl<E>(d_input, d_offset_mask, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h,
                                                          stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, remove_center, d_out,
                                                          stream));
}

int frcnn_ops_dcnv4_backward_offset_mask_16(int elem_type, const void* d_input, const float* d_offset_mask, const void* d_dout, int n_img,
                                            int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                            int pad_w, int dil_h, int dil_w, float offset_scale, int remove_center, float* d_doffset_mask,
                                            void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, dcnv4_backward_offset_mask_impl<E>(d_input, d_offset_mask, d_dout, n_img, h, w, g, gc, kernel_h,
                                                                       kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w,
                                                                       offset_scale, remove_center, d_doffset_mask, stream));
}

int frcnn_ops_dcnv4_backward_input_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                      const void* d_dout, int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h,
                                      int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int remove_center, void* d_dinput,
                                      void* d_ws, size_t ws_bytes, void* stream)
{
    if (elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    return dcnv4_backward_input(elem_type, d_sorted_keys, d_order, d_weights, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h,
                                stride_w, pad_h, pad_w, dil_h, dil_w, remove_center, d_dinput, d_ws, ws_bytes, stream);
}

}  // extern "C"
