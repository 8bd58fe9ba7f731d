"""
The kernels that write the A operands of the tile-record GEMMs, through the C ABI, held to tests/operand_record_cases.py
(tests/test_operand_records_cpu.py states which seam each case reaches and holds the references to independent truth):
  * frcnn_roi_pool_x3t (csrc/roipool.hip: roi_scale_x3t_kernel, roi_pool_x3t_rows_kernel, the lane-per-RoI roi_pool_x3t_kernel) against
    the float32 truth, and against frcnn_roi_pool + frcnn_split_rows_x3t under the same scales: "same maxima, same scale, same split";
  * frcnn_roi_pool (roi_pool_kernel) bit for bit;
  * frcnn_rows_scale_x3t + frcnn_split_rows_x3t against the scale and split contract, and against frcnn_pack_rows_x3t;
  * the im2col producers frcnn_split_patches3x3_x3t / _x6t and frcnn_split_pixels_x6t against explicit im2col matrices;
  * one strided 3x3 convolution through the producers and frcnn_gemm_x3t against float64.
Every output buffer holds garbage before the call (0x5B bytes, NaN floats): an unwritten byte shows.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import operand_record_cases as R
from fasterrcnn_amd import _native as nv
from fasterrcnn_amd.models import vgg16 as V

DEV = "cuda"


def S():
    return nv.stream_ptr()


def garbage(nbytes):
    return torch.full((int(nbytes),), 0x5B, dtype=torch.int8, device=DEV)


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)            # (a copy: the cached case arrays are read-only)


def is_power_of_two(v):
    m, _ = np.frexp(v.astype(np.float64))
    return bool((m == 0.5).all())


def split_rows_x3t(a, lda, a_batch, inv, rows, rows_padded, k, batches=1):
    """frcnn_split_rows_x3t under the given scales -> record bytes"""
    rec = garbage(batches * R.x3t_record_bytes(rows_padded, k))
    nv.check(nv.lib().frcnn_split_rows_x3t(nv.ptr(a), lda, a_batch, nv.ptr(inv), nv.ptr(rec), rows, rows_padded, k, batches, S()), "split_rows_x3t")
    return host(rec)


def pack_rows_x3t(a, rows_padded):
    """frcnn_pack_rows_x3t of a contiguous [batches][R][K] tensor -> blob bytes (host), the device blob"""
    nb, r, k = (int(v) for v in a.shape)
    blob = garbage(nb * (R.x3t_record_bytes(rows_padded, k) + 4 * rows_padded))
    assert blob.numel() == int(nv.lib().frcnn_x3t_blob_bytes(rows_padded, k, nb))
    nv.check(nv.lib().frcnn_pack_rows_x3t(nv.ptr(a), k, r * k, nv.ptr(blob), r, rows_padded, k, nb, S()), "pack_rows_x3t")
    return host(blob), blob


def split_rows_x6t(a, rows_padded):
    nb, r, k = (int(v) for v in a.shape)
    rec = garbage(nb * R.x6t_record_bytes(rows_padded, k))
    assert rec.numel() == nb * int(nv.lib().frcnn_x6t_record_bytes(rows_padded, k))
    nv.check(nv.lib().frcnn_split_rows_x6t(nv.ptr(a), k, r * k, nv.ptr(rec), r, rows_padded, k, nb, S()), "split_rows_x6t")
    return host(rec)


# ---- 1. RoI pooling into f32x3 records ------------------------------------------------------------------------------------------------------
def roi_pool_x3t(fm, rois, n, case):
    """-> record bytes, inv (host), inv (device)"""
    k = case.pooled * case.pooled * case.c
    rec = garbage(R.x3t_record_bytes(case.rec_rows, k))
    assert rec.numel() == int(nv.lib().frcnn_x3t_record_bytes(case.rec_rows, k))
    inv, cmax = nans(case.rec_rows), nans(case.fh * case.fw)
    nv.check(nv.lib().frcnn_roi_pool_x3t(nv.ptr(fm), case.fh, case.fw, case.c, nv.ptr(rois), nv.ptr(n), case.max_rois, case.pooled, R.SCALE,
                                         nv.ptr(cmax), nv.ptr(inv), nv.ptr(rec), case.rec_rows, S()), "roi_pool_x3t")
    return host(rec), host(inv), inv


def roi_pool_f32(fm, rois, n, fh, fw, c, max_rois, pooled):
    out = nans(max_rois, pooled, pooled, c)
    nv.check(nv.lib().frcnn_roi_pool(nv.ptr(fm), fh, fw, c, nv.ptr(rois), nv.ptr(n), max_rois, pooled, R.SCALE, nv.ptr(out), S()), "roi_pool")
    return out


def check_roi_records(case, fm, rois):
    """assertions (a) - (e) of one frcnn_roi_pool_x3t case; -> scaled reference [n][K], for the callers that ask more"""
    n_live = min(case.n, case.max_rois)
    k = case.pooled * case.pooled * case.c
    ref = R.roi_pool_ref(fm, rois[:n_live], case.pooled, R.SCALE).reshape(n_live, k).astype(np.float64)
    d_fm, d_rois = dev(fm), dev(rois)
    d_n = torch.tensor([case.n], dtype=torch.int32, device=DEV)                # the device counter, as the model passes it
    rec, inv, d_inv = roi_pool_x3t(d_fm, d_rois, d_n, case)
    hi, lo = (p[0] for p in R.decode_x3t(rec, case.rec_rows, k))
    # (a) exact powers of two; 1 for the rows that hold no RoI and for a RoI with every bin empty
    assert np.isfinite(inv).all() and is_power_of_two(inv), inv
    assert (inv[n_live:] == 1.0).all()
    dead = [r for r in range(n_live) if not any(h > 0 and w > 0 for _, _, h, w in
                                                R.window_list(R.roi_windows(rois[r], case.fh, case.fw, case.pooled, R.SCALE)))]
    assert (inv[dead] == 1.0).all() and not ref[dead].any()
    # (b) the split's contract against the truth
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    scaled = ref / inv[:n_live, None].astype(np.float64)
    err = np.abs(hi[:n_live] + lo[:n_live] - scaled)
    over = err > R.split_error_bound(scaled)
    assert not over.any(), "%s: %d values beyond the split's bound, first at (row, k) %s: records %r, truth %r" % (
        case.name, int(over.sum()), tuple(np.argwhere(over)[0]), (hi[:n_live] + lo[:n_live])[over][0], scaled[over][0])
    assert (np.abs(scaled) < 2.0 ** 15).all(), "a row scale that does not bound its row"
    # (c) the rows from n on are zero in both planes
    assert not hi[n_live:].any() and not lo[n_live:].any()
    # (d) the records of the float32 pooling split under the SAME scales
    out = roi_pool_f32(d_fm, d_rois, d_n, case.fh, case.fw, case.c, case.max_rois, case.pooled)
    out_h = host(out).reshape(case.max_rois, k)
    assert np.array_equal(out_h[:n_live].view(np.uint32), ref.astype(np.float32).view(np.uint32)) and not out_h[n_live:].any()
    hi2, lo2 = (p[0] for p in R.decode_x3t(split_rows_x3t(out, k, 0, d_inv, case.max_rois, case.rec_rows, k), case.rec_rows, k))
    assert np.array_equal(hi, hi2) and np.array_equal(lo, lo2), "%s: %d hi and %d lo values differ from split_rows_x3t(roi_pool) under the same scales" % (
        case.name, int((hi != hi2).sum()), int((lo != lo2).sum()))
    # (e) a second run: the same bytes
    rec_b, inv_b, _ = roi_pool_x3t(d_fm, d_rois, d_n, case)
    assert np.array_equal(rec, rec_b) and np.array_equal(inv.view(np.uint32), inv_b.view(np.uint32))
    return scaled


@pytest.mark.parametrize("case", R.ROI_X3T_CASES, ids=lambda c: c.name)
def test_roi_pool_x3t_records_are_the_float32_pooling_under_a_bounding_scale(case):
    fm, rois, n_live = R.roi_case_inputs(case)
    check_roi_records(case, fm, rois)


@pytest.mark.parametrize("name", R.TIGHT_ROIS)
def test_roi_scale_x3t_is_drawn_from_the_union_of_the_bins_and_no_further(name):
    """a non-negative map with cells of 1000 x its maximum immediately outside the union of one RoI's bins: that RoI's scale must put its
    largest pooled value into [2^14, 2^15) -- a scale drawn from a wider region (or from stale maxima) is 2^10 too small and still passes
    the split's bound.  On a non-negative map the row's maximum IS the largest channel maximum of the union's cells, so the range is exact.
    "edge57": the union is the bins' (one column past [rs, rs + roi) in float32) and its maximum sits in that column: a scale drawn from the
    shorter range does not bound the row."""
    fm, rois, row, planted = R.tightness_inputs(name)
    case = R.RoiCase("tight_" + name, fm.shape[0], fm.shape[1], 32, 7, 32, len(rois), len(rois), "tight")
    scaled = check_roi_records(case, fm, rois)
    top = np.abs(scaled[row]).max()
    print("%s: %d cells planted, max |ref / inv| = %.6g" % (name, planted, top))
    assert 2.0 ** 14 <= top < 2.0 ** 15
    # every live row of the call, the target or not: a planted cell INSIDE another RoI's union is simply that row's maximum
    rowmax = np.abs(scaled).max(axis=1)
    assert (rowmax > 0).all() and ((rowmax >= 2.0 ** 14) & (rowmax < 2.0 ** 15)).all(), rowmax


def test_roi_scale_x3t_every_live_row_of_a_non_negative_map_is_tight():
    """the ten RoIs on the ReLU'd map without planted cells: every RoI with a live bin has its scaled maximum in [2^14, 2^15)"""
    case = R.RoiCase("tight_all", 13, 21, 32, 7, 32, 10, 10, "13x21")
    fm = np.maximum(R.signed_map(13, 21, 32, 77), 0)
    scaled = check_roi_records(case, fm, R.ROIS_13x21)
    rowmax = np.abs(scaled).max(axis=1)
    live = rowmax > 0
    assert int(live.sum()) == 9 and ((rowmax[live] >= 2.0 ** 14) & (rowmax[live] < 2.0 ** 15)).all(), rowmax


# ---- 2. the float32 RoI pooling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.ROI_F32_CHANNELS)
def test_roi_pool_f32_is_the_reference_bit_for_bit(c):
    fm, rois = R.signed_map(13, 21, c, 2000 + c), R.ROIS_13x21
    n, max_rois = len(rois), len(rois) + 3
    ref = R.roi_pool_ref(fm, rois, 7, R.SCALE)
    d_rois = dev(np.concatenate([rois, rois[:3]]))                              # live boxes behind the counter
    out = host(roi_pool_f32(dev(fm), d_rois, torch.tensor([n], dtype=torch.int32, device=DEV), 13, 21, c, max_rois, 7))
    bad = out[:n].view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "C = %d: %d values differ, first at (roi, ph, pw, c) %s" % (c, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    assert not out[n:].view(np.uint32).any(), "the surplus rows are +0"


# ---- 3. row scale + split ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ROWS_CASES, ids=lambda c: "b%d_r%d_k%d_lda%d" % (c.batches, c.R, c.K, c.lda))
def test_rows_scale_and_split_x3t(case):
    lib = nv.lib()
    buf, a, special = R.rows_operand(case)
    nb, r, k, rp = case.batches, case.R, case.K, case.rows_padded
    d_buf = dev(buf)
    inv_d = nans(nb, rp)
    nv.check(lib.frcnn_rows_scale_x3t(nv.ptr(d_buf), case.lda, case.a_batch, nv.ptr(inv_d), r, rp, k, nb, S()), "rows_scale_x3t")
    inv = host(inv_d)
    want = np.ones((nb, rp), dtype=np.float32)
    want[:, :r] = R.row_scale_ref(np.abs(a).max(axis=2))
    assert np.array_equal(inv.view(np.uint32), want.view(np.uint32)), "inv is hx_row_scale of the row's maximum over K columns (not lda), to the bit"
    rec = split_rows_x3t(d_buf, case.lda, case.a_batch, inv_d, r, rp, k, nb)
    hi, lo = R.decode_x3t(rec, rp, k, nb)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    assert not hi[:, r:].any() and not lo[:, r:].any()
    scaled = a.astype(np.float64) / inv[:, :r, None].astype(np.float64)
    err = np.abs(hi[:, :r] + lo[:, :r] - scaled)
    assert (err <= R.split_error_bound(scaled)).all(), float((err / R.split_error_bound(scaled)).max())
    rowmax = np.abs(scaled).max(axis=2)
    ranged = np.ones((nb, r), dtype=bool)
    if special:
        ranged[:, [special["zero"], special["subnormal"]]] = False
        assert (inv[:, special["zero"]] == 1.0).all() and not hi[:, special["zero"]].any()
        assert (inv[:, special["subnormal"]] == np.float32(2.0 ** -100)).all()
        assert (np.abs(hi[:, special["below_pow2"]]).max(axis=1) == 32768.0).all(), "hi rounds up to 2^15 and stays finite"
        assert (hi[:, special["pow2"]].max(axis=1) == 16384.0).all()
        assert (hi[:, special["negmax"]].min(axis=1) == -np.abs(hi[:, special["negmax"]]).max(axis=1)).all()
    assert ((rowmax[ranged] >= 2.0 ** 14) & (rowmax[ranged] < 2.0 ** 15)).all()
    # pack = scale + split, on a contiguous copy: lda > K, the batch stride and the 1e30 around the matrix change nothing
    blob, _ = pack_rows_x3t(dev(a), rp)
    nrec = nb * R.x3t_record_bytes(rp, k)
    assert np.array_equal(blob[nrec:].view(np.uint8), inv.reshape(-1).view(np.uint8))
    assert np.array_equal(blob[:nrec].view(np.uint8), rec.view(np.uint8))


# ---- 4. 3x3 im2col producers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c,stride,rp", R.PATCH_CASES)
def test_split_patches3x3_x6t_is_the_im2col_matrix_exactly(n, h, w, c, stride, rp):
    x = R.scaled_pixels(n, h, w, c)
    a = R.im2col3x3_ref(x, stride)
    rows, k = a.shape
    rec = garbage(R.x6t_record_bytes(rp, k))
    nv.check(nv.lib().frcnn_split_patches3x3_x6t(nv.ptr(dev(x)), nv.ptr(rec), n, h, w, c, stride, rp, S()), "split_patches3x3_x6t")
    rec = host(rec)
    hi, mid, lo = (p[0] for p in R.decode_x6t(rec, rp, k))
    total = (hi + mid + lo).astype(np.float32)
    bad = total[:rows].view(np.uint32) != a.view(np.uint32)
    assert not bad.any(), "%d values differ, first at (row, k) %s" % (int(bad.sum()), tuple(np.argwhere(bad)[0]))
    assert not hi[rows:].any() and not mid[rows:].any() and not lo[rows:].any()
    assert np.array_equal(rec.view(np.uint8), split_rows_x6t(dev(a[None]), rp).view(np.uint8))


@pytest.mark.parametrize("n,h,w,c,stride,rp", R.PATCH_CASES)
def test_split_patches3x3_x3t_is_pack_rows_of_the_im2col_matrix(n, h, w, c, stride, rp):
    """the row maximum over the in-map patch pixels' channel maxima is the im2col row's own maximum, and a maximum is exact: the scales, and
    with them every record byte, are those of frcnn_pack_rows_x3t of the explicit matrix"""
    lib = nv.lib()
    x = R.scaled_pixels(n, h, w, c)
    a = R.im2col3x3_ref(x, stride)
    rows, k = a.shape
    d_x = dev(x)
    cmax = nans(n * h * w)
    nv.check(lib.frcnn_pixel_absmax(nv.ptr(d_x), nv.ptr(cmax), n * h * w, c, S()), "pixel_absmax")
    assert np.array_equal(host(cmax), np.abs(x).max(axis=3).reshape(-1))
    rec, inv = garbage(R.x3t_record_bytes(rp, k)), nans(rp)
    nv.check(lib.frcnn_split_patches3x3_x3t(nv.ptr(d_x), nv.ptr(cmax), nv.ptr(rec), nv.ptr(inv), n, h, w, c, stride, rp, S()), "split_patches3x3_x3t")
    rec, inv = host(rec), host(inv)
    blob, _ = pack_rows_x3t(dev(a[None]), rp)
    nrec = R.x3t_record_bytes(rp, k)
    assert np.array_equal(inv.view(np.uint32), R.row_scale_ref(np.concatenate([np.abs(a).max(axis=1), np.zeros(rp - rows, np.float32)])).view(np.uint32))
    assert (inv[rows:] == 1.0).all()
    assert np.array_equal(inv.view(np.uint8), blob[nrec:].view(np.uint8)), "the scales of pack_rows_x3t of the im2col matrix"
    if not np.array_equal(rec.view(np.uint8), blob[:nrec].view(np.uint8)):
        hi, lo = (p[0] for p in R.decode_x3t(rec, rp, k))
        hi2, lo2 = (p[0] for p in R.decode_x3t(blob[:nrec], rp, k))
        bad = (hi != hi2) | (lo != lo2)
        pytest.fail("%d record values differ from pack_rows_x3t of the im2col matrix, first at (row, k) %s (tap %d)" % (
            int(bad.sum()), tuple(np.argwhere(bad)[0]) if bad.any() else "(signs of zeros only)", int(np.argwhere(bad)[0][1]) // c if bad.any() else -1))


# ---- 5. 1x1 producer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c,stride", R.PIXEL_CASES)
def test_split_pixels_x6t_is_the_gathered_matrix_exactly(n, h, w, c, stride):
    x = R.scaled_pixels(n, h, w, c)
    a = R.pixels_ref(x, stride)
    rows = a.shape[0]
    rp = R.pad_to(rows, 32)
    rec = garbage(R.x6t_record_bytes(rp, c))
    nv.check(nv.lib().frcnn_split_pixels_x6t(nv.ptr(dev(x)), nv.ptr(rec), n, h, w, c, stride, rp, S()), "split_pixels_x6t")
    rec = host(rec)
    hi, mid, lo = (p[0] for p in R.decode_x6t(rec, rp, c))
    total = (hi + mid + lo).astype(np.float32)
    bad = total[:rows].view(np.uint32) != a.view(np.uint32)
    assert not bad.any(), "%d values differ, first at (row, k) %s" % (int(bad.sum()), tuple(np.argwhere(bad)[0]))
    assert not hi[rows:].any() and not mid[rows:].any() and not lo[rows:].any()
    assert np.array_equal(rec.view(np.uint8), split_rows_x6t(dev(a[None]), rp).view(np.uint8))


# ---- 6. a strided 3x3 convolution through the producers -------------------------------------------------------------------------------------
def test_strided_conv3x3_through_the_x3t_producers_against_float64():
    """frcnn_pixel_absmax + frcnn_split_patches3x3_x3t + frcnn_gemm_x3t with tap-major weights packed by frcnn_pack_rows_x3t against F.conv2d
    in float64, at the bar of tests/test_gemm_x3t_gpu.py test_gemm_x3t_against_float64_and_the_exact_f32_kernel: error (per output row,
    relative to the row's largest |y|) <= 1.5 x the exact-f32 kernel's on the same im2col matrix + 2e-7.  Both errors are measured against
    the float64 reference."""
    lib = nv.lib()
    n, h, w, cin, cout, stride = R.CONV_CASE
    gen = torch.Generator().manual_seed(6)
    x = torch.randn((n, h, w, cin), generator=gen) * torch.exp(torch.randn((1, 1, 1, cin), generator=gen))       # per-channel scales
    x = x * torch.exp2(torch.randint(-12, 13, (n, h, w, 1), generator=gen).float())                              # pixels of very different size
    wt = torch.randn((cout, cin, 3, 3), generator=gen) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), generator=gen) * 0.1
    ho, wo = R.out_hw(h, w, stride)
    m, k = n * ho * wo, 9 * cin
    ref = (F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), b.double(), padding=1, stride=stride).permute(0, 2, 3, 1).reshape(m, cout))
    d_x, d_b = x.cuda().contiguous(), b.cuda()
    wmat = dev(R.tap_major(wt.numpy()))                                                                          # [cout][9 cin]
    a_rows, b_rows = R.pad_to(m, nv.X6T_ROW_TILE), R.pad_to(cout, nv.X6T_COL_TILE)
    cmax = nans(n * h * w)
    nv.check(lib.frcnn_pixel_absmax(nv.ptr(d_x), nv.ptr(cmax), n * h * w, cin, S()), "pixel_absmax")
    a_rec, a_inv = garbage(R.x3t_record_bytes(a_rows, k)), nans(a_rows)
    nv.check(lib.frcnn_split_patches3x3_x3t(nv.ptr(d_x), nv.ptr(cmax), nv.ptr(a_rec), nv.ptr(a_inv), n, h, w, cin, stride, a_rows, S()), "split_patches3x3_x3t")
    _, w_blob = pack_rows_x3t(wmat[None], b_rows)
    w_rec = R.x3t_record_bytes(b_rows, k)
    y = nans(m, cout)
    wsb = int(lib.frcnn_gemm_x3t_workspace_bytes(m, cout, k, 1))
    ws = torch.empty((max(wsb, 4),), dtype=torch.uint8, device=DEV)
    nv.check(lib.frcnn_gemm_x3t(nv.ptr(a_rec), nv.ptr(a_inv), a_rows, 0, 0, nv.ptr(w_blob), w_blob.data_ptr() + w_rec, b_rows, 0, 0, nv.ptr(d_b), None,
                                nv.ptr(y), cout, 0, m, cout, k, 1, 0, nv.ptr(ws), wsb, S()), "gemm_x3t")
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    row_scale = ref.abs().amax(dim=1, keepdim=True).clamp(min=1e-30)
    e3 = float(((y.cpu().double() - ref).abs() / row_scale).max())
    a = dev(R.im2col3x3_ref(x.numpy(), stride))
    y32 = V.linear(a, wmat, d_b, cout, False)
    e32 = float(((y32.cpu().double() - ref).abs() / row_scale).max())
    print("conv3x3 / stride 2 through the x3t producers: max err / row max|y| = %.3g (exact-f32 kernel on the im2col matrix: %.3g)" % (e3, e32))
    assert e3 <= 1.5 * e32 + 2e-7
