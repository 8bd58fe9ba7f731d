"""
Case tables, numpy references and record decoders for the kernels that WRITE the A operands of the tile-record GEMMs (csrc/gemm_x3t.hip,
csrc/gemm_x6t.hip): RoI pooling into f32x3 records (csrc/roipool.hip roi_scale_x3t_kernel, roi_pool_x3t_rows_kernel, roi_pool_x3t_kernel),
the float32 RoI pooling beside it (roi_pool_kernel), the row scale and split (rows_scale_x3t_kernel, split_rows_x3t_kernel) and the im2col
producers (split_patches3x3_x3t_kernel, split_patches3x3_x6t_kernel, split_pixels_x6t_kernel).  No GPU, nothing imported from the kernels
or from the other test files: tests/test_operand_records_cpu.py holds this file to independent truth, tests/test_operand_records_gpu.py
holds the kernels to this file.

Record layouts (x3t.h, gemm_x3t.hip, gemm_x6t.hip), row-major matrix X[rows][K], K % 16 == 0, rows padded to a multiple of 32:
    x3t: [K/16 chunks][rows/32 row blocks][2 terms hi, lo][2 k-halves][32 rows][8 fp16]   values scaled by 1 / inv[row], inv = 2^-e
    x6t: [K/16 chunks][rows/32 row blocks][3 terms hi, mid, lo][2 k-halves][32 rows][8 bf16]
A batched array is [batches] of these.
"""
import functools
import math
from collections import namedtuple

import numpy as np

SCALE = 1.0 / 16.0            # spatial scale of every RoI case (exact in float32)


def pad_to(n, t):
    return -(-n // t) * t


# ---- record codecs ----------------------------------------------------------------------------------------------------------------
def _planes_of(elems, rows_padded, k, batches, terms):
    """elems: the record array's 16-bit elements as float64, flat -> [batches][terms][rows_padded][k]"""
    a = elems.reshape(batches, k // 16, rows_padded // 32, terms, 2, 32, 8)          # [b][chunk][row block][term][k-half][row][8]
    return a.transpose(0, 3, 2, 5, 1, 4, 6).reshape(batches, terms, rows_padded, k)   # [b][term][row block, row][chunk, k-half, 8]


def _elems_of(planes, rows_padded, k, batches, terms):
    """the inverse of _planes_of: [batches][terms][rows_padded][k] -> flat, in record order"""
    a = planes.reshape(batches, terms, rows_padded // 32, 32, k // 16, 2, 8)          # [b][term][row block][row][chunk][k-half][8]
    return np.ascontiguousarray(a.transpose(0, 4, 2, 1, 5, 3, 6)).reshape(-1)


def _bytes(raw):
    return np.ascontiguousarray(np.asarray(raw)).view(np.uint8).reshape(-1)


def x3t_record_bytes(rows_padded, k):
    return (k // 16) * (rows_padded // 32) * 2 * 1024


def x6t_record_bytes(rows_padded, k):
    return (k // 16) * (rows_padded // 32) * 3 * 1024


def decode_x3t(rec, rows_padded, k, batches=1):
    """x3t record bytes -> hi, lo float64 [batches][rows_padded][k]"""
    raw = _bytes(rec)
    assert raw.size == batches * x3t_record_bytes(rows_padded, k)
    p = _planes_of(raw.view(np.float16).astype(np.float64), rows_padded, k, batches, 2)
    return p[:, 0], p[:, 1]


def decode_x3t_blob(blob, rows_padded, k, batches=1):
    """a packed x3t operand (the record arrays of every batch, then [batches][rows_padded] float32 scales) -> hi, lo, inv"""
    raw = _bytes(blob)
    nrec = batches * x3t_record_bytes(rows_padded, k)
    assert raw.size == nrec + 4 * batches * rows_padded
    hi, lo = decode_x3t(raw[:nrec], rows_padded, k, batches)
    return hi, lo, raw[nrec:].view(np.float32).reshape(batches, rows_padded).copy()


def encode_x3t(hi, lo):
    """hi, lo [batches][rows_padded][k] holding fp16 values -> the record bytes"""
    b, rp, k = hi.shape
    planes = np.stack([hi, lo], axis=1).astype(np.float16)
    return _elems_of(planes, rp, k, b, 2).view(np.uint8)


def encode_x3t_blob(hi, lo, inv):
    return np.concatenate([encode_x3t(hi, lo), np.ascontiguousarray(inv, dtype=np.float32).reshape(-1).view(np.uint8)])


def decode_x6t(rec, rows_padded, k, batches=1):
    """x6t record bytes -> hi, mid, lo float64 [batches][rows_padded][k]"""
    raw = _bytes(rec)
    assert raw.size == batches * x6t_record_bytes(rows_padded, k)
    f32 = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)              # a bfloat16 is the upper half of a float32
    p = _planes_of(f32.astype(np.float64), rows_padded, k, batches, 3)
    return p[:, 0], p[:, 1], p[:, 2]


def encode_x6t(hi, mid, lo):
    """hi, mid, lo [batches][rows_padded][k] holding bfloat16 values -> the record bytes"""
    b, rp, k = hi.shape
    f32 = np.stack([hi, mid, lo], axis=1).astype(np.float32)
    bits = f32.view(np.uint32)
    assert not (bits & 0xFFFF).any(), "not bfloat16 values"
    return _elems_of((bits >> 16).astype(np.uint16), rp, k, b, 3).view(np.uint8)


def split_error_bound(scaled):
    """the split's contract (gemm_x3t.hip; the bound tests/test_gemm_x3t_gpu.py test_x3t_split_scales_and_layout states): 2^-22 relative
    where the low term is a normal fp16 number, 2^-25 absolute (half an ulp of the smallest fp16 subnormal) below"""
    return np.maximum(2.0 ** -22 * np.abs(scaled), 2.0 ** -25)


# ---- RoI pooling --------------------------------------------------------------------------------------------------------------------
ROI_NAMES_13x21 = ("whole", "onecell", "outside", "topleft", "thincol", "thinrow", "botright", "mid", "wide", "ragged")
ROIS_13x21 = np.array([            # y1, x1, y2, x2 in pixels; map 13 x 21 at scale 1/16, 7 x 7 bins
    [0, 0, 208, 336],              # whole
    [40, 40, 40, 40],              # onecell
    [400, 500, 450, 600],          # outside
    [-40, -40, 30, 50],            # topleft
    [0, 100, 200, 100],            # thincol
    [100, 0, 100, 330],            # thinrow
    [150, 250, 400, 500],          # botright
    [30, 50, 120, 200],            # mid
    [16, 0, 60, 335],              # wide
    [20, 30, 150, 170],            # ragged
], dtype=np.float32)
ROIS_38x63 = np.array([[0, 0, 608, 1008], [100, 37, 500, 900], [-64, -64, 672, 1072]], dtype=np.float32)
ROIS_5x6 = np.array([[0, 0, 79, 95],           # the whole map
                     [40, 40, 40, 40],         # one cell
                     [400, 500, 450, 600],     # outside
                     [-40, -40, 30, 50]],      # straddling the top-left corner
                    dtype=np.float32)

# clipped bin edges per axis (hs, he, ws, we: `pooled` ints each; a bin (ph, pw) is rows [hs[ph], he[ph]) x columns [ws[pw], we[pw])), whether the
# map's border cut the bin's un-clipped range (per axis: top / bottom per ph, left / right per pw), and the clipped union of the bins
# (uh0, uh1, uw0, uw1): rows [uh0, uh1) x columns [uw0, uw1)
Windows = namedtuple("Windows", "hs he ws we clip_top clip_bottom clip_left clip_right union")


def _round_half_away(v32):
    """C roundf of a float32, computed in float64 (|v| + 0.5 is exact there)"""
    v = float(v32)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def _axis(c1, c2, size, pooled, scale):
    s32 = np.float32(scale)
    rs, re = _round_half_away(np.float32(c1) * s32), _round_half_away(np.float32(c2) * s32)
    roi = max(re - rs + 1, 1)
    b = np.float32(roi) / np.float32(pooled)                                    # float32 throughout
    lo = [int(np.floor(np.float32(p) * b)) + rs for p in range(pooled)]
    hi = [int(np.ceil(np.float32(p + 1) * b)) + rs for p in range(pooled)]
    clip = lambda v: min(max(v, 0), size)                                     # noqa: E731
    union = (clip(rs), clip(int(np.ceil(np.float32(pooled) * b)) + rs))        # NOT [rs, re]: ceil(pooled * (roi / pooled)) can be roi + 1
    return (np.array([clip(v) for v in lo]), np.array([clip(v) for v in hi]), np.array([v < 0 for v in lo]),
            np.array([v > size for v in hi]), union)


def roi_windows(roi, fh, fw, pooled, scale):
    """the float32 edge arithmetic of torchvision's RoIPool for one RoI (y1, x1, y2, x2): rs = roundf(coord * scale) half away from zero,
    size = max(re - rs + 1, 1), bin = size / pooled in float32, bin p = [floor(p bin) + rs, ceil((p + 1) bin) + rs) clipped to the map"""
    hs, he, top, bottom, uh = _axis(roi[0], roi[2], fh, pooled, scale)
    ws, we, left, right, uw = _axis(roi[1], roi[3], fw, pooled, scale)
    return Windows(hs, he, ws, we, top, bottom, left, right, uh + uw)


def window_list(win):
    """-> [(ph, pw, height, width)] of every bin (height or width 0: an empty bin)"""
    return [(ph, pw, max(int(win.he[ph] - win.hs[ph]), 0), max(int(win.we[pw] - win.ws[pw]), 0))
            for ph in range(len(win.hs)) for pw in range(len(win.ws))]


def roi_pool_ref(fm, rois, pooled, scale):
    """fm [fh][fw][C] float32, rois [n][4] -> [n][pooled][pooled][C] float32: the maximum over each bin's window (a maximum is exact: this
    is the truth), +0 for an empty window"""
    fm = np.asarray(fm, dtype=np.float32)
    fh, fw, c = fm.shape
    out = np.zeros((len(rois), pooled, pooled, c), dtype=np.float32)
    for r, roi in enumerate(rois):
        win = roi_windows(roi, fh, fw, pooled, scale)
        for ph, pw, h, w in window_list(win):
            if h > 0 and w > 0:
                out[r, ph, pw] = fm[win.hs[ph]:win.he[ph], win.ws[pw]:win.we[pw]].max(axis=(0, 1))
    return out


def rows_kernel_takes(c):
    """A MIRROR of launch_roi_pool_x3t's own rule (csrc/roipool.hip): the block-per-(bin, 32 RoIs) kernel keeps [32][c + 4] floats in LDS and
    is taken while they fit in 160 KB; wider maps take the lane-per-RoI kernel.  It is here so that a change of the rule moves the case
    (tests/test_operand_records_cpu.py pins both sides of the threshold)."""
    return c % 8 == 0 and 32 * (c + 4) * 4 <= 160 * 1024


@functools.lru_cache(maxsize=None)
def signed_map(fh, fw, c, seed):
    fm = np.random.default_rng(seed).standard_normal((fh, fw, c), dtype=np.float32)
    fm.setflags(write=False)
    return fm


def jittered_rois(n, seed):
    """the ten RoIs of ROIS_13x21, cycled, each moved as a whole by a seeded offset of less than half a cell (8 px) in y and in x"""
    rng = np.random.default_rng(seed)
    base = ROIS_13x21[np.arange(n) % len(ROIS_13x21)]
    d = rng.uniform(-7.9, 7.9, (n, 2)).astype(np.float32)
    return (base + np.concatenate([d, d], axis=1)).astype(np.float32)


# name, map, channels, bins, record rows, max_rois, n (as the device counter holds it), RoI set
RoiCase = namedtuple("RoiCase", "name fh fw c pooled rec_rows max_rois n rois")
ROI_X3T_CASES = [RoiCase("ten", 13, 21, 32, 7, 32, 10, 10, "13x21")]
# more than one 32-RoI row block; n at a block edge, one past it, at max_rois and above it (n = 75 must behave as 70)
ROI_X3T_CASES += [RoiCase("blocks_n%d" % n, 13, 21, 32, 7, 96, 70, n, "cycled") for n in (0, 1, 32, 33, 64, 65, 70, 75)]
ROI_X3T_CASES += [
    RoiCase("c1024", 38, 63, 1024, 7, 32, 13, 13, "38x63+13x21"),    # the rows kernel's second 512-channel pass, wide windows
    RoiCase("c1264_rows", 5, 6, 1264, 7, 32, 4, 4, "5x6"),           # the last width that takes the rows kernel (a third, short pass)
    RoiCase("c1280_lanes", 5, 6, 1280, 7, 32, 4, 4, "5x6"),          # the lane-per-RoI fallback
    RoiCase("pooled1", 13, 21, 16, 1, 32, 10, 10, "13x21"),          # K = 16: one chunk
    RoiCase("pooled2", 13, 21, 16, 2, 32, 10, 10, "13x21"),
    RoiCase("pooled7_c16", 13, 21, 16, 7, 32, 10, 10, "13x21"),
]
ROI_X3T_BY_NAME = {c.name: c for c in ROI_X3T_CASES}


def roi_case_inputs(case):
    """-> fm [fh][fw][c] (signed), rois [max(n, max_rois)][4], the number of RoIs the kernels must pool (min(n, max_rois)).  The rows of
    `rois` from n on hold live boxes: a kernel that reads them writes something a zero check sees."""
    fm = signed_map(case.fh, case.fw, case.c, 1000 + case.c)
    rows = max(case.n, case.max_rois)
    if case.rois == "13x21":
        rois = ROIS_13x21
    elif case.rois == "cycled":
        rois = jittered_rois(rows, 75)
    elif case.rois == "38x63+13x21":
        rois = np.concatenate([ROIS_38x63, ROIS_13x21])
    else:
        rois = ROIS_5x6
    assert len(rois) >= rows
    return fm, np.ascontiguousarray(rois[:rows], dtype=np.float32), min(case.n, case.max_rois)


ROI_F32_CHANNELS = (4, 20, 516, 1028, 1536)        # roi_pool_kernel: C / 4 = 1, 5, 129, 257, 384 channel quads (see the CPU test)

TIGHT_ROIS = ("mid", "ragged", "whole", "edge57")
# "edge57": 57 columns from column 3 of a 9 x 63 map.  ceil(7 * (57 / 7.0f)) is 58 in float32, so the last bin reaches column 60, one past
# [rs, rs + roi): the map's largest in-union value sits THERE (a scale drawn from [rs, rs + roi) does not bound it), and the planted cells
# start at column 61 (a scale drawn from anything wider than the bins is 2^10 too small).
EDGE57_ROI = np.array([16, 48, 100, 944], dtype=np.float32)


def tightness_inputs(name):
    """-> fm (a ReLU'd 32-channel map with cells of 1000 x its maximum immediately outside the union of the target RoI's bins, where the map
    has such cells), the RoIs of the call, the target's row among them, the number of cells planted"""
    if name == "edge57":
        fh, fw, rois, row = 9, 63, np.stack([EDGE57_ROI, np.array([0, 0, 143, 300], dtype=np.float32)]), 0
    else:
        fh, fw, rois, row = 13, 21, ROIS_13x21[[ROI_NAMES_13x21.index(r) for r in TIGHT_ROIS[:3]]], TIGHT_ROIS.index(name)
    fm = np.maximum(signed_map(fh, fw, 32, 77), 0).copy()
    top = fm.max()
    uh0, uh1, uw0, uw1 = roi_windows(rois[row], fh, fw, 7, SCALE).union
    if name == "edge57":
        fm[uh0 + 2, uw1 - 1, 5] = np.float32(8.0) * top            # the last column of the last bin holds the union's maximum
    big = np.float32(1000.0) * top
    planted = 0
    for y in (uh0 - 1, uh1):
        for x in range(max(uw0 - 1, 0), min(uw1 + 1, fw)):         # the rows above and below, corners included
            if 0 <= y < fh:
                fm[y, x] = big
                planted += 1
    for x in (uw0 - 1, uw1):
        for y in range(uh0, uh1):                                  # the columns left and right
            if 0 <= x < fw:
                fm[y, x] = big
                planted += 1
    return fm, np.ascontiguousarray(rois), row, planted


# ---- row scale and split ------------------------------------------------------------------------------------------------------------
def row_scale_ref(mx):
    """x3t.h hx_row_scale: inv = 2^-(14 - floor(log2 mx)), the exponent clamped to +-100, 1 for mx == 0.  frexp, no logarithm: mx = m 2^x with
    m in [0.5, 1), so floor(log2 mx) = x - 1 (a float32 subnormal has floor(log2) <= -127: clamped either way)."""
    mx = np.asarray(mx, dtype=np.float32)
    _, x = np.frexp(mx)
    e = np.clip(14 - (x.astype(np.int64) - 1), -100, 100)
    return np.where(mx > 0, np.ldexp(np.float32(1.0), -e), np.float32(1.0)).astype(np.float32)


# batches, rows, K, lda, rows_padded, floats between two batches
RowsCase = namedtuple("RowsCase", "batches R K lda rows_padded a_batch")
ROWS_CASES = [
    RowsCase(2, 70, 48, 64, 96, 70 * 64 + 32),       # lda > K and a batch stride that is not R lda
    RowsCase(1, 1, 16, 16, 32, 16),                  # one row, one chunk
    RowsCase(1, 33, 272, 272, 64, 33 * 272),         # K beyond one 256-float sweep of the scale kernel's wave; one row past a block
    RowsCase(1, 300, 4096, 4096, 320, 300 * 4096),   # fc2's operand
]
SPECIAL_ROWS = {"zero": 1, "pow2": 2, "below_pow2": 3, "negmax": 4, "subnormal": 5}    # row indices, in every batch of a case with R >= 33
FILL = np.float32(1e30)                              # what the columns K .. lda - 1 and the gap between two batches hold


def rows_operand(case):
    """-> flat float32 buffer [batches][a_batch] holding [R][lda] matrices (everything outside [R][K] is 1e30), the contiguous
    [batches][R][K] copy, and the row indices of the specials ({} when the case is too small to hold them)"""
    rng = np.random.default_rng(case.R * 1000 + case.K)
    a = rng.standard_normal((case.batches, case.R, case.K), dtype=np.float32)
    a *= np.exp2(rng.integers(-30, 31, (case.batches, case.R, 1))).astype(np.float32)          # rows 2^+-30 apart
    special = SPECIAL_ROWS if case.R >= 33 else {}
    if special:
        k, j = 7, case.K - 3
        u = rng.uniform(-1, 1, (case.batches, 3, case.K)).astype(np.float32)
        a[:, special["zero"]] = 0.0
        a[:, special["pow2"]] = u[:, 0] * np.float32(0.9 * 2.0 ** k)
        a[:, special["pow2"], j] = np.float32(2.0 ** k)                                        # the maximum is exactly 2^k
        a[:, special["below_pow2"]] = u[:, 1] * np.float32(0.9 * 2.0 ** -k)
        a[:, special["below_pow2"], j] = np.nextafter(np.float32(2.0 ** -k), np.float32(0))    # hi rounds up to 32768
        a[:, special["negmax"]] = u[:, 2] * np.float32(0.5 * 2.0 ** k)
        a[:, special["negmax"], 0] = np.float32(-0.9 * 2.0 ** k)                               # the largest magnitude is negative
        sub = rng.integers(1, 1 << 22, (case.batches, case.K)).astype(np.uint32) | (rng.integers(0, 2, (case.batches, case.K)).astype(np.uint32) << 31)
        a[:, special["subnormal"]] = sub.view(np.float32)                                      # float32 subnormals only
    buf = np.full((case.batches * case.a_batch,), FILL, dtype=np.float32)
    for b in range(case.batches):
        view = buf[b * case.a_batch:b * case.a_batch + case.R * case.lda].reshape(case.R, case.lda)
        view[:, :case.K] = a[b]
    return buf, a, dict(special)


# ---- im2col -----------------------------------------------------------------------------------------------------------------------------
def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def im2col3x3_ref(x, stride):
    """x [N][H][W][C] -> [N Ho Wo][9 C] of the 3x3 / padding 1 convolution: row (n, oy, ox), column k = (3 r + s) C + c reading
    x[n, oy stride - 1 + r, ox stride - 1 + s, c], +0 outside the map"""
    n, h, w, c = x.shape
    ho, wo = out_hw(h, w, stride)
    xp = np.zeros((n, h + 2, w + 2, c), dtype=x.dtype)
    xp[:, 1:h + 1, 1:w + 1] = x
    out = np.zeros((n, ho, wo, 9, c), dtype=x.dtype)
    for r in range(3):
        for s in range(3):
            out[:, :, :, 3 * r + s] = xp[:, r:r + (ho - 1) * stride + 1:stride, s:s + (wo - 1) * stride + 1:stride]
    return out.reshape(n * ho * wo, 9 * c)


def pixels_ref(x, stride):
    """x [N][H][W][C] -> [N Ho Wo][C]: the pixels a 1x1 convolution of that stride reads"""
    return np.ascontiguousarray(x[:, ::stride, ::stride]).reshape(-1, x.shape[3])


# N, H, W, C, stride, rows_padded
PATCH_CASES = [
    (1, 1, 1, 16, 1, 32),         # eight of the nine taps are padding
    (1, 2, 3, 16, 2, 32),
    (2, 5, 7, 32, 1, 96),         # 70 rows: a ragged last row block, two maps
    (3, 6, 5, 48, 2, 32),         # three chunks per tap; H even and W odd under stride 2
    (1, 7, 7, 272, 2, 320),       # rows_padded far above the 16 rows
]
# N, H, W, C, stride (rows_padded: the rows padded to 32)
PIXEL_CASES = [(3, 7, 7, 1024, 1), (5, 7, 7, 1024, 2), (1, 9, 13, 16, 1), (1, 5, 6, 272, 2), (2, 1, 1, 16, 2)]


@functools.lru_cache(maxsize=None)
def scaled_pixels(n, h, w, c, seed=0):
    """signed values, per-pixel magnitudes 2^+-20 apart, one all-zero pixel (the last; a map of one pixel keeps it: nothing else would be
    left to check), no other exact zero"""
    rng = np.random.default_rng(seed + 7 * n + 100 * h + 1000 * w + c)
    x = rng.standard_normal((n, h, w, c), dtype=np.float32)
    x[x == 0] = 1.0
    x *= np.exp2(rng.integers(-20, 21, (n, h, w, 1))).astype(np.float32)
    if n * h * w > 1:
        x[n - 1, h - 1, w - 1] = 0.0
    x.setflags(write=False)
    return x


CONV_CASE = (2, 9, 11, 64, 128, 2)             # N, H, W, cin, cout, stride of the end-to-end convolution


def tap_major(wt):
    """[cout][cin][3][3] -> [cout][9 cin], column (3 r + s) cin + c: the B operand that im2col3x3_ref's columns meet"""
    return np.ascontiguousarray(wt.transpose(0, 2, 3, 1)).reshape(wt.shape[0], -1)
