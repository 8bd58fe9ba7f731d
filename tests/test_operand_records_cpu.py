"""
tests/operand_record_cases.py held to independent truth, without a GPU, so that tests/test_operand_records_gpu.py does not rest on unchecked
code:
  * the RoI pooling reference against oracle/frcnn_oracle.py's, bit for bit, and the im2col references against F.conv2d in float64;
  * the record codecs: decoder(encoder(planes)) is the identity, and the layout against a position-coded matrix;
  * the coverage the RoI sets and the case tables claim, computed from roi_windows -- never from a kernel -- so that no case silently stops
    being what it claims;
  * the argument checks of the entry points, which refuse bad arguments before touching the device.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from tests import operand_record_cases as R
from fasterrcnn_amd import _native as nv
from oracle import frcnn_oracle as O

EINVAL = -1


# ---- what the RoI sets reach ----------------------------------------------------------------------------------------------------------------
def live_windows(rois, fh, fw, pooled=7):
    """-> [(roi index, ph, pw, height, width, Windows)] of the non-empty bins"""
    out = []
    for i, roi in enumerate(rois):
        win = R.roi_windows(roi, fh, fw, pooled, R.SCALE)
        out += [(i, ph, pw, h, w, win) for ph, pw, h, w in R.window_list(win) if h > 0 and w > 0]
    return out


def cut_borders(live):
    """the borders that cut a window which survives the cut"""
    return {name for name, flag, axis in (("top", "clip_top", 1), ("bottom", "clip_bottom", 1), ("left", "clip_left", 2), ("right", "clip_right", 2))
            if any(getattr(l[5], flag)[l[axis]] for l in live)}


def test_the_ten_rois_cover_the_window_seams_of_a_13x21_map():
    live = live_windows(R.ROIS_13x21, 13, 21)
    cells = [h * w for _, _, _, h, w, _ in live]
    assert {n % 4 for n in cells} == {0, 1, 2, 3}, "the rows kernel's four-cell tail: every residue"
    assert 1 in cells
    assert any(w == 1 and h > 1 for _, _, _, h, w, _ in live), "a one-column window of several rows (the cell index with ww = 1)"
    per_roi = [sum(1 for l in live if l[0] == i) for i in range(len(R.ROIS_13x21))]
    assert any(0 < n < 49 for n in per_roi), "an empty bin inside an otherwise live RoI"
    assert per_roi[R.ROI_NAMES_13x21.index("outside")] == 0 and sorted(per_roi)[1] > 0, "exactly one RoI has every bin empty"
    # clipping at each border.  Top, bottom and right cut a window that survives.  The left border cuts bins of "topleft" only, whose bin is
    # exactly one column wide: the bins it cuts are emptied, none is cut and survives -- on this table the left border is met by a live RoI,
    # not by a live window.  A live window cut on the left is asserted where the GPU cases have one: in the jittered copies of this table
    # (below) and on the 38 x 63 map (next test).
    assert cut_borders(live) == {"top", "bottom", "right"}
    tl = R.roi_windows(R.ROIS_13x21[R.ROI_NAMES_13x21.index("topleft")], 13, 21, 7, R.SCALE)
    assert tl.clip_left[:3].all() and not tl.clip_left[3:].any() and (tl.we[:3] == 0).all() and per_roi[R.ROI_NAMES_13x21.index("topleft")] > 0
    assert cut_borders(live_windows(R.jittered_rois(70, 75), 13, 21)) == {"top", "bottom", "left", "right"}
    print("13 x 21: %d live windows, cell counts %s, live bins per RoI %s" % (len(live), sorted(set(cells)), per_roi))


def test_the_three_rois_cover_the_wide_windows_of_a_38x63_map():
    live = live_windows(R.ROIS_38x63, 38, 63)
    widths = {w for _, _, _, _, w, _ in live}
    assert {6, 7, 9, 11} <= widths, "widths that are no power of two: the reciprocal-multiply cell index (%s)" % sorted(widths)
    assert max(h * w for _, _, _, h, w, _ in live) >= 90
    assert cut_borders(live) == {"top", "bottom", "left", "right"}
    print("38 x 63: widths %s, largest window %d cells" % (sorted(widths), max(h * w for _, _, _, h, w, _ in live)))


def test_the_union_of_the_bins_is_not_the_rounded_roi():
    """ceil(7 * (roi / 7.0f)) is roi + 1 in float32 for roi = 57: roi_windows' union is the bins', one row past [rs, re]"""
    win = R.roi_windows(np.array([0, 0, 56 * 16, 16], dtype=np.float32), 60, 60, 7, R.SCALE)
    assert win.union[:2] == (0, 58) and int(win.he[6]) == 58
    for rois, fh, fw in ((R.ROIS_13x21, 13, 21), (R.ROIS_38x63, 38, 63), (R.ROIS_5x6, 5, 6), (R.jittered_rois(75, 75), 13, 21)):
        for roi in rois:
            for pooled in (1, 2, 7):
                win = R.roi_windows(roi, fh, fw, pooled, R.SCALE)
                assert win.union == (int(win.hs[0]), int(win.he[-1]), int(win.ws[0]), int(win.we[-1])), "first bin's start, last bin's end"
                assert (win.hs[1:] <= win.he[:-1]).all() and (win.ws[1:] <= win.we[:-1]).all(), "the bins leave no cell of the union out"


def test_the_case_tables_hold_what_they_claim():
    by = R.ROI_X3T_BY_NAME
    # kernel choice: a MIRROR of launch_roi_pool_x3t's rule, there so that a change of the rule moves the case
    assert 32 * (1264 + 4) * 4 <= 160 * 1024 < 32 * (1280 + 4) * 4
    assert R.rows_kernel_takes(by["c1264_rows"].c) and not R.rows_kernel_takes(by["c1280_lanes"].c) and by["c1280_lanes"].c - by["c1264_rows"].c == 16
    assert all(R.rows_kernel_takes(c.c) for c in R.ROI_X3T_CASES if c.name != "c1280_lanes")
    assert by["c1024"].c > 512 and by["c1264_rows"].c > 1024, "a second and a third pass of the rows kernel's channel loop"
    assert {c.n for c in R.ROI_X3T_CASES if c.rois == "cycled"} == {0, 1, 32, 33, 64, 65, 70, 75}
    assert all(c.rec_rows == 96 and c.max_rois == 70 for c in R.ROI_X3T_CASES if c.rois == "cycled")
    assert {c.pooled for c in R.ROI_X3T_CASES} == {1, 2, 7} and by["pooled1"].pooled ** 2 * by["pooled1"].c == 16
    for c in R.ROI_X3T_CASES:
        fm, rois, n = R.roi_case_inputs(c)
        assert fm.shape == (c.fh, c.fw, c.c) and float(fm.min()) < 0 < float(fm.max()) and rois.shape == (max(c.n, c.max_rois), 4)
        assert n == min(c.n, c.max_rois) and c.rec_rows % 32 == 0 and c.rec_rows >= c.max_rois and c.c % 16 == 0
    # the 13 x 21 set clips differently on the 38 x 63 map: "botright" is cut there by no border
    _, rois, n = R.roi_case_inputs(by["c1024"])
    assert n == 13 and len(live_windows(rois[3:], 38, 63)) > len(live_windows(rois[3:], 13, 21))
    # the jitter moves window edges: the cycled copies of a RoI are not all the same windows
    j = R.jittered_rois(70, 75)
    assert np.abs(j - R.ROIS_13x21[np.arange(70) % 10]).max() < 8.0
    edges = {tuple(np.concatenate(R.roi_windows(r, 13, 21, 7, R.SCALE)[:4]).tolist()) for r in j[7::10]}
    assert len(edges) > 1
    # roi_pool_kernel: 128 threads x two channel quads per pass of 256 quads
    quads = [c // 4 for c in R.ROI_F32_CHANNELS]
    assert quads == [1, 5, 129, 257, 384]
    assert quads[0] < 128 and quads[1] < 128                      # a partial first pass: has_a false for some threads, has_b for all
    assert 128 < quads[2] < 256                                   # has_b true for one thread only
    assert quads[3] == 256 + 1 and quads[4] == 256 + 128          # a second pass with one quad, and with a full half
    # the tightness maps: cells are planted all round "mid", "ragged" and "edge57"; "whole" has no cell outside its bins
    for name in R.TIGHT_ROIS:
        fm, rois, row, planted = R.tightness_inputs(name)
        assert float(fm.min()) == 0.0 and (planted > 0) == (name != "whole")
        u = R.roi_windows(rois[row], fm.shape[0], fm.shape[1], 7, R.SCALE).union
        inside = fm[u[0]:u[1], u[2]:u[3]]
        assert float(inside.max()) * 100.0 < float(fm.max()) or planted == 0, "nothing planted inside the union"
        if name != "whole":
            ring = fm[max(u[0] - 1, 0):u[1] + 1, max(u[2] - 1, 0):u[3] + 1].copy()
            ring[u[0] - max(u[0] - 1, 0):, u[2] - max(u[2] - 1, 0):][:u[1] - u[0], :u[3] - u[2]] = fm.max()
            assert (ring.max(axis=2) == fm.max()).all(), "every in-map cell that touches the union holds the planted value"
    # "edge57": the bins reach one column past [rs, rs + roi), and the union's maximum is in that column
    fm, rois, row, _ = R.tightness_inputs("edge57")
    win = R.roi_windows(rois[row], 9, 63, 7, R.SCALE)
    assert (win.union[2], win.union[3]) == (3, 61) and int(win.we[6]) == 61 and int(win.ws[0]) == 3
    inside = fm[win.union[0]:win.union[1]]
    assert float(inside[:, 60].max()) == float(inside[:, 3:61].max()) >= 4.0 * float(inside[:, 3:60].max())


# ---- independent truth --------------------------------------------------------------------------------------------------------------------
def test_roi_pool_ref_is_the_oracles_bit_for_bit():
    for rois, fh, fw in ((R.ROIS_13x21, 13, 21), (R.ROIS_38x63, 38, 63), (np.concatenate([R.ROIS_38x63, R.ROIS_13x21]), 38, 63),
                         (R.ROIS_5x6, 5, 6), (R.jittered_rois(75, 75), 13, 21)):
        fm = R.signed_map(fh, fw, 8, 5)
        for pooled in (1, 2, 7):
            got = R.roi_pool_ref(fm, rois, pooled, R.SCALE)
            boxes = np.concatenate([np.zeros((len(rois), 1), np.float32), rois[:, [1, 0, 3, 2]]], axis=1)      # (batch, x1, y1, x2, y2)
            want = O.roi_pool(fm.transpose(2, 0, 1)[None], boxes, pooled, R.SCALE)                            # (n, C, out, out)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.transpose(0, 2, 3, 1).view(np.uint32))
            assert (fh, pooled) != (13, 7) or float(got.min()) < 0, "a signed map: the maximum of a one-cell window can be negative"


def test_row_scale_ref_against_exact_arithmetic():
    mx = np.array([0.0, 1.0, 1.5, 2.0, np.nextafter(np.float32(2.0), np.float32(0)), 2.0 ** 14, 2.0 ** 15, 3e-30, 65504.0, 1e38, 2.0 ** -126,
                   1e-40, 2.0 ** -149, 2.0 ** -100, 2.0 ** 120], dtype=np.float32)
    inv = R.row_scale_ref(mx)
    assert inv.dtype == np.float32 and inv[0] == 1.0
    for m, i in zip(mx[1:].astype(np.float64), inv[1:].astype(np.float64)):
        e = -np.log2(i)
        assert e == round(e) and -100 <= e <= 100
        assert 2.0 ** 14 <= m / i < 2.0 ** 15 or abs(e) == 100
    assert inv[1] == 2.0 ** -14 and inv[4] == 2.0 ** -14 and inv[3] == 2.0 ** -13 and inv[5] == 1.0 and inv[6] == 2.0
    assert inv[11] == inv[12] == 2.0 ** -100 and inv[14] == 2.0 ** 100


def test_im2col_times_weights_is_conv2d_exactly():
    rng = np.random.default_rng(3)
    for stride in (1, 2):
        for n, h, w in ((2, 5, 7), (1, 6, 4), (1, 6, 5), (2, 1, 1), (1, 2, 3), (1, 7, 8)):                 # odd and even H and W
            c, cout = 3, 4
            x = rng.integers(-8, 9, (n, h, w, c)).astype(np.float64)
            wt = rng.integers(-8, 9, (cout, c, 3, 3)).astype(np.float64)
            a = R.im2col3x3_ref(x, stride)
            ho, wo = R.out_hw(h, w, stride)
            want = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), padding=1, stride=stride).permute(0, 2, 3, 1).numpy()
            assert want.shape == (n, ho, wo, cout) and a.shape == (n * ho * wo, 9 * c)
            assert np.array_equal((a @ R.tap_major(wt).T).reshape(want.shape), want)
            p = R.pixels_ref(x, stride)
            want1 = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt[:, :, :1, :1].copy()), stride=stride).permute(0, 2, 3, 1).numpy()
            assert np.array_equal((p @ wt[:, :, 0, 0].T).reshape(want1.shape), want1)


def test_the_producer_inputs_are_what_they_claim():
    for n, h, w, c, stride, rp in R.PATCH_CASES:
        x = R.scaled_pixels(n, h, w, c)
        ho, wo = R.out_hw(h, w, stride)
        assert rp % 32 == 0 and rp >= n * ho * wo
        zero_pixels = int((np.abs(x).max(axis=3) == 0).sum())
        assert zero_pixels == (1 if n * h * w > 1 else 0) and int((x == 0).sum()) == zero_pixels * c and float(x.min()) < 0
        if n * h * w > 4:
            m = np.abs(x).max(axis=3)
            assert m[m > 0].max() / m[m > 0].min() >= 2.0 ** 10
    assert {(c[1] % 2, c[2] % 2) for c in R.PATCH_CASES if c[4] == 2} >= {(0, 1), (1, 1)}
    assert any(n * R.out_hw(h, w, s)[0] * R.out_hw(h, w, s)[1] % 32 != 0 and n > 1 for n, h, w, c, s, rp in R.PATCH_CASES)
    for case in R.ROWS_CASES:
        buf, a, special = R.rows_operand(case)
        assert buf.size == case.batches * case.a_batch and a.shape == (case.batches, case.R, case.K)
        assert int((buf == R.FILL).sum()) == buf.size - a.size
        assert bool(special) == (case.R >= 33)
        if special:
            mx = np.abs(a).max(axis=2)
            assert (mx[:, special["zero"]] == 0).all() and (mx[:, special["pow2"]] == 128.0).all()
            assert (mx[:, special["below_pow2"]] == np.nextafter(np.float32(2.0 ** -7), np.float32(0))).all()
            assert (a[:, special["negmax"]].min(axis=1) == -mx[:, special["negmax"]]).all() and (a[:, special["negmax"]].max(axis=1) < mx[:, special["negmax"]]).all()
            assert (mx[:, special["subnormal"]] < 2.0 ** -126).all() and (np.abs(a[:, special["subnormal"]]).min() > 0)
            live = np.delete(mx, list(special.values()), axis=1)
            assert live.max() / live.min() >= 2.0 ** 30


# ---- the codecs ---------------------------------------------------------------------------------------------------------------------------
def test_the_record_codecs_round_trip():
    rng = np.random.default_rng(11)
    for b, rp, k in ((1, 32, 16), (2, 96, 48), (1, 64, 272)):
        hi = rng.standard_normal((b, rp, k)).astype(np.float16).astype(np.float64) * 1024
        lo = rng.standard_normal((b, rp, k)).astype(np.float16).astype(np.float64)
        inv = np.exp2(rng.integers(-20, 20, (b, rp))).astype(np.float32)
        rec = R.encode_x3t(hi, lo)
        assert rec.dtype == np.uint8 and rec.size == b * R.x3t_record_bytes(rp, k)
        h2, l2 = R.decode_x3t(rec, rp, k, b)
        assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
        h3, l3, i3 = R.decode_x3t_blob(R.encode_x3t_blob(hi, lo, inv), rp, k, b)
        assert np.array_equal(h3, hi) and np.array_equal(l3, lo) and np.array_equal(i3, inv)
        assert np.array_equal(R.encode_x3t(*R.decode_x3t(rec, rp, k, b)), rec)
        bf = lambda v: (v.astype(np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)      # noqa: E731
        t = [bf(rng.standard_normal((b, rp, k)) * s) for s in (100.0, 0.5, 0.002)]
        rec6 = R.encode_x6t(*t)
        assert rec6.size == b * R.x6t_record_bytes(rp, k)
        for got, want in zip(R.decode_x6t(rec6, rp, k, b), t):
            assert np.array_equal(got, want)
        assert np.array_equal(R.encode_x6t(*R.decode_x6t(rec6, rp, k, b)), rec6)


def test_the_record_layout_is_the_documented_one():
    """a matrix whose element (row, k) is (7 row + k) mod 256 (integers up to 256 are exact in fp16 and bfloat16): the 8 values of row r, chunk ch, k-half kh sit
    at byte ((ch rbt + rb) T + term) 1024 + kh 512 + (r % 32) 16 of a T-term array (x3t.h; csrc/gemm_x3t.hip and gemm_x6t.hip's headers)"""
    rp, k = 64, 32
    m = ((7 * np.arange(rp)[:, None] + np.arange(k)[None, :]) % 256).astype(np.float64)[None]
    z = np.zeros_like(m)
    for terms, rec, elem in ((2, R.encode_x3t(m, z), np.float16), (3, R.encode_x6t(m, z, z), None)):
        for row, ch, kh in ((0, 0, 0), (33, 1, 1), (63, 0, 1), (31, 1, 0)):
            off = ((ch * (rp // 32) + row // 32) * terms + 0) * 1024 + kh * 512 + (row % 32) * 16
            raw = rec[off:off + 16]
            vals = raw.view(np.float16).astype(np.float64) if elem else (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
            assert np.array_equal(vals, m[0, row, ch * 16 + kh * 8:ch * 16 + kh * 8 + 8]), (terms, row, ch, kh)
            assert not rec[off + 1024:off + 1040].any(), "the next term's piece holds the zero plane"


# ---- arguments refused before the device is touched -----------------------------------------------------------------------------------------
def test_the_producers_refuse_bad_arguments_without_a_gpu():
    lib = nv.lib()
    raw = (C.c_float * 96)()
    x = (C.addressof(raw) + 63) & ~63              # a 64-byte aligned host address; none of these calls may read or write it

    def roi(c=32, rec_rows=32, max_rois=10, cmax=x, inv=x):
        return lib.frcnn_roi_pool_x3t(x, 13, 21, c, x, x, max_rois, 7, 0.0625, cmax, inv, x, rec_rows, None)
    assert roi(c=24) == EINVAL and roi(c=8) == EINVAL              # c % 16 != 0
    assert roi(rec_rows=48) == EINVAL                              # rec_rows % 32 != 0
    assert roi(rec_rows=32, max_rois=33) == EINVAL                 # rec_rows < max_rois
    assert roi(cmax=None) == EINVAL and roi(inv=None) == EINVAL

    def splits(n=1, h=5, w=7, c=32, stride=1, rp=64):
        return {"patches_x3t": lib.frcnn_split_patches3x3_x3t(x, x, x, x, n, h, w, c, stride, rp, None),
                "patches_x6t": lib.frcnn_split_patches3x3_x6t(x, x, n, h, w, c, stride, rp, None),
                "pixels_x6t": lib.frcnn_split_pixels_x6t(x, x, n, h, w, c, stride, rp, None)}

    def all_einval(**kw):
        got = splits(**kw)
        assert set(got.values()) == {EINVAL}, (kw, got)
    all_einval(c=24)                               # C % 16 != 0
    all_einval(c=8)
    all_einval(stride=0)
    all_einval(stride=3)
    all_einval(rp=48)                              # rows_padded % 32 != 0
    all_einval(rp=32)                              # 35 rows
    all_einval(n=2, stride=2, rp=0)                # 24 rows
    assert lib.frcnn_split_patches3x3_x3t(x, None, x, x, 1, 5, 7, 32, 1, 64, None) == EINVAL          # a null d_cmax
    assert lib.frcnn_split_patches3x3_x3t(x, x, x, None, 1, 5, 7, 32, 1, 64, None) == EINVAL          # ... d_inv_scale

    def rows(r=35, rp=64, k=48, lda=48):
        return {lib.frcnn_rows_scale_x3t(x, lda, 0, x, r, rp, k, 1, None), lib.frcnn_split_rows_x3t(x, lda, 0, x, x, r, rp, k, 1, None),
                lib.frcnn_split_rows_x6t(x, lda, 0, x, r, rp, k, 1, None), lib.frcnn_pack_rows_x3t(x, lda, 0, x, r, rp, k, 1, None)}
    assert rows(k=40, lda=40) == {EINVAL}          # K % 16 != 0
    assert rows(rp=48) == {EINVAL} and rows(rp=32) == {EINVAL} and rows(lda=32) == {EINVAL} and rows(r=0) == {EINVAL}
    assert lib.frcnn_split_rows_x3t(x, 48, 0, None, x, 35, 64, 48, 1, None) == EINVAL
