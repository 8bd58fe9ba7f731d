// ops_dcnv3.hip -- DCNv3, the deformable convolution v3 of the InternImage backbones, in both directions: the frcnn_ops_dcnv3* entry
// points of include/frcnn_hip.h.  Restated from the published operator (third party, absent here: restated, unpinned, like the other
// operators of fasterrcnn_amd.ops; where the two differ include/frcnn_hip.h holds).
//
//   offset float32 [n][Ho][Wo][G K 2] pairs (dx, dy), mask float32 [n][Ho][Wo][G K], K = kh kw: the DcPlanar layout of ops_dcn.h, which
//   holds the sampling rule, the mapping and the kernels (shared with ops_dcnv4.hip).  A block's offsets and masks are one contiguous piece
//   of each tensor, staged in LDS by coalesced loads (consecutive lanes write consecutive words: no bank conflict).
#include "ops_dcn.h"

namespace frcnn {

static bool dcnv3_geom(int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                       float offset_scale, DcGeom& s)
{
    return dc_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, 0, s);
}

template <typename E>
static int dcnv3_forward_impl(const void* input, const float* offset, const float* mask, int n_img, int h, int w, int g, int gc, int kh,
                              int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale, void* out, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, s) || !input || !offset || !mask || !out)
        return FRCNN_EINVAL;
    return dc_forward<E>(input, DcPlanar{offset, mask, nullptr, nullptr}, n_img, s, gc, out, stream);
}

template <typename E>
static int dcnv3_backward_offset_impl(const void* input, const float* offset, const float* mask, const void* dout, int n_img, int h, int w,
                                      int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale,
                                      float* doffset, float* dmask, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, s) || !input || !offset || !mask || !dout)
        return FRCNN_EINVAL;
    if (!doffset && !dmask) return FRCNN_EINVAL;
    return dc_backward_offset<E>(input, dout, DcPlanar{offset, mask, doffset, dmask}, n_img, s, gc, stream);
}

static int dcnv3_backward_input(int elem_type, const int64_t* sorted_keys, const int64_t* order, const float* wts, const void* dout,
                                int n_img, int h, int w, int g, int gc, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                void* dinput, void* ws, size_t ws_bytes, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kh, kw, sh, sw, ph, pw, dh, dw, 1.0f, s)) return FRCNN_EINVAL;
    return dc_backward_input(elem_type, sorted_keys, order, wts, dout, n_img, h, w, s, gc, dinput, ws, ws_bytes, stream);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_ops_dcnv3_max_kernel(void) { return DCN_MAX_KERNEL; }
int frcnn_ops_dcnv3_max_channels(void) { return MSDA_MAX_CHANNELS; }

int frcnn_ops_dcnv3_block_items(int gc, int kernel_h, int kernel_w, int elem_type)
{
    if (gc < 1 || gc > MSDA_MAX_CHANNELS || kernel_h < 1 || kernel_h > DCN_MAX_KERNEL || kernel_w < 1 || kernel_w > DCN_MAX_KERNEL)
        return 0;
    if (elem_type != 0 && elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return 0;
    const int run = elem_type == 0 ? MsElem<float>::RUN : MsElem<f16>::RUN;
    return ms_map(gc, kernel_h * kernel_w, run, gc % run == 0).ipb;
}

size_t frcnn_ops_dcnv3_workspace_bytes(int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, 1.0f, s)) return 0;
    return msda_gather_workspace(n_img * h * w * g, (int)(dc_items(n_img, s) * s.K * 4), gc);
}

int frcnn_ops_dcnv3_forward(const float* d_input, const float* d_offset, const float* d_mask, int n_img, int h, int w, int g, int gc,
                            int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                            float offset_scale, float* d_out, void* stream)
{
    return dcnv3_forward_impl<float>(d_input, d_offset, d_mask, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                     dil_h, dil_w, offset_scale, d_out, stream);
}

int frcnn_ops_dcnv3_backward_offset(const float* d_input, const float* d_offset, const float* d_mask, const float* d_dout, int n_img, int h,
                                    int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                    int dil_h, int dil_w, float offset_scale, float* d_doffset, float* d_dmask, void* stream)
{
    return dcnv3_backward_offset_impl<float>(d_input, d_offset, d_mask, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                                             pad_h, pad_w, dil_h, dil_w, offset_scale, d_doffset, d_dmask, stream);
}

int frcnn_ops_dcnv3_plan(const float* d_offset, const float* d_mask, int n_img, int h, int w, int g, int kernel_h, int kernel_w,
                         int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, int64_t* d_keys,
                         float* d_weights, void* stream)
{
    DcGeom s;
    if (!dcnv3_geom(n_img, h, w, g, 1, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, s) || !d_offset ||
        !d_mask || !d_keys || !d_weights)
        return FRCNN_EINVAL;
    return dc_plan(DcPlanar{d_offset, d_mask, nullptr, nullptr}, n_img, h, w, s, d_keys, d_weights, stream);
}

int frcnn_ops_dcnv3_backward_input(const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights, const float* d_dout,
                                   int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dil_h, int dil_w, float* d_dinput, void* d_ws, size_t ws_bytes, void* stream)
{
    return dcnv3_backward_input(0, d_sorted_keys, d_order, d_weights, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h, stride_w,
                                pad_h, pad_w, dil_h, dil_w, d_dinput, d_ws, ws_bytes, stream);
}

int frcnn_ops_dcnv3_forward_16(int elem_type, const void* d_input, const float* d_offset, const float* d_mask, int n_img, int h, int w,
                               int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                               int dil_w, float offset_scale, void* d_out, void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, dcnv3_forward_impl<E>(d_input, d_offset, d_mask, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h,
                                                          stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, d_out, stream));
}

int frcnn_ops_dcnv3_backward_offset_16(int elem_type, const void* d_input, const float* d_offset, const float* d_mask, const void* d_dout,
                                       int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, float* d_doffset, float* d_dmask,
                                       void* stream)
{
    OPS_ELEM_DISPATCH(elem_type, E, dcnv3_backward_offset_impl<E>(d_input, d_offset, d_mask, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w,
                                                                  stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, offset_scale, d_doffset,
                                                                  d_dmask, stream));
}

int frcnn_ops_dcnv3_backward_input_16(int elem_type, const int64_t* d_sorted_keys, const int64_t* d_order, const float* d_weights,
                                      const void* d_dout, int n_img, int h, int w, int g, int gc, int kernel_h, int kernel_w, int stride_h,
                                      int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, void* d_dinput, void* d_ws, size_t ws_bytes,
                                      void* stream)
{
    if (elem_type != FRCNN_OPS_F16 && elem_type != FRCNN_OPS_BF16) return FRCNN_EINVAL;
    return dcnv3_backward_input(elem_type, d_sorted_keys, d_order, d_weights, d_dout, n_img, h, w, g, gc, kernel_h, kernel_w, stride_h,
                                stride_w, pad_h, pad_w, dil_h, dil_w, d_dinput, d_ws, ws_bytes, stream);
}

}  // extern "C"
