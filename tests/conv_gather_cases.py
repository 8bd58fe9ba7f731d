"""
Case tables, float64 references and a plan mirror for the gather convolutions of csrc/conv_gather.hip (conv_gather_mfma_kernel,
conv_gather_bf16_kernel, conv_gather_x3_kernel, forward and data-gradient form) and the weight gradient beside them
(csrc/gemm_tn.hip launch_conv_wgrad).  No GPU, nothing imported from the kernels: tests/test_conv_gather_cpu.py holds this file to
independent truth and to the library's own workspace sizes, tests/test_conv_gather_gpu.py holds the kernels to this file.

Exact-integer operands.  Activations, weights, bias, residual and upstream gradient are dense random integers with |v| <= 8, and every
reduction is short enough that the sum of the MAGNITUDES of its addends stays below 2^24.  Then
  * float32 products and sums are exact in any order and under any split of the reduction;
  * rounding an operand to bfloat16 is the identity (4 significant bits);
  * the f32x3 split under one power-of-two scale per tensor is exact: x3t.h hx_row_scale returns 2^e with max|t| 2^e in [2^14, 2^15),
    so an integer |v| <= 8 becomes v 2^e with e >= 11: at most 4 significant bits, magnitude in [2^11, 2^15) -- a normal fp16 number,
    hi = fp16(v 2^e) holds it and lo = fp16(v 2^e - hi) = 0 (conv_gather.hip gx_split4); the accumulators hold integers times 2^(ex + ew)
    and the un-scaling multiplies by an exact power of two.
So there is exactly ONE right answer in all three arithmetics: the float64 reference cast to float32, to the bit.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

VMAX = 8                      # |operand| <= VMAX
EXACT_LIMIT = 1 << 24         # every partial sum stays below this in magnitude

Case = namedtuple("Case", "name N H W cin cout k stride pad")


def cdiv(a, b):
    return -(-a // b)


def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def rows_forward(c):
    ho, wo = out_hw(c)
    return c.N * ho * wo


def forward_ok(c):
    """frcnn_conv_nhwc(_math) takes the case"""
    return c.cin % 16 == 0 and c.cout % 4 == 0


def dgrad_ok(c):
    """frcnn_conv_dgrad(_math) takes the case"""
    return c.cout % 16 == 0 and c.cin % 4 == 0


def wgrad_ok(c):
    """frcnn_conv_wgrad(_math) takes the case"""
    return c.cin % 4 == 0 and c.cout % 4 == 0 and c.k <= 7


# ---- the case table -------------------------------------------------------------------------------------------------------------
# name, N, H, W, cin, cout, k, stride, pad.  The smallest shapes that reach the code; tests/test_conv_gather_cpu.py states, through the
# plan mirror below, which tile / split / pipeline seam each of them reaches, and fails if the table stops reaching one.
X3_GEOMETRY = [
    # 3x3 at pad 0 / 1 / 2 (pad_e of the pipelined kernel: 0 / 1 / 2 forward, 2 / 1 / 0 in the data gradient), stride 1 and 2; odd and
    # even maps under stride 2 so that (H + 2 pad - 3) % 2 takes both values; N > 1 with Ho Wo neither a multiple of a tile nor a power of two
    Case("k3p0s1", 2, 9, 11, 32, 64, 3, 1, 0),
    Case("k3p1s1", 2, 9, 11, 64, 64, 3, 1, 1),
    Case("k3p2s1", 2, 9, 11, 32, 128, 3, 1, 2),
    Case("k3p0s2_odd", 2, 9, 11, 32, 64, 3, 2, 0),
    Case("k3p0s2_even", 2, 10, 12, 32, 64, 3, 2, 0),
    Case("k3p1s2_odd", 2, 9, 11, 64, 32, 3, 2, 1),
    Case("k3p1s2_even", 2, 10, 12, 64, 32, 3, 2, 1),
    Case("k3p2s2_odd", 2, 9, 11, 32, 64, 3, 2, 2),
    Case("k3p2s2_even", 2, 10, 12, 32, 64, 3, 2, 2),
    Case("k1s1", 2, 9, 11, 64, 64, 1, 1, 0),
    Case("k1s2", 2, 9, 11, 64, 64, 1, 2, 0),
    Case("k1s2_even", 2, 10, 12, 64, 64, 1, 2, 0),
    Case("k1s3", 2, 9, 11, 64, 64, 1, 3, 0),
    # gather_x3_takes puts no bound on the forward stride: 3x3 at stride 3 (with a remainder) and 4 run the pipelined kernel too
    Case("k3s3_x3", 2, 9, 11, 32, 32, 3, 3, 0),
    Case("k3s4_x3", 2, 9, 11, 32, 32, 3, 4, 1),
    # maps smaller than the filter (cout 32: the data gradient in math 1 runs the pipelined kernel too, at pad_e 1 and 0)
    Case("tiny1x1_p1", 3, 1, 1, 32, 32, 3, 1, 1),
    Case("tiny1x1_p2", 3, 1, 1, 32, 32, 3, 1, 2),
    Case("tiny1x2_p1", 3, 1, 2, 32, 32, 3, 1, 1),
    Case("tiny1x2_p2", 3, 1, 2, 32, 32, 3, 1, 2),
    Case("tiny2x2_p1", 3, 2, 2, 32, 32, 3, 1, 1),
    Case("tiny2x2_p2", 3, 2, 2, 32, 32, 3, 1, 2),
    Case("tiny2x5_p1", 3, 2, 5, 32, 32, 3, 1, 1),
    Case("tiny2x5_p2", 3, 2, 5, 32, 32, 3, 1, 2),
    # a tile straddles an image boundary: 3 x 49 rows, seams at 64 and 128
    Case("straddle", 3, 7, 7, 32, 64, 3, 1, 1),
    # many tiny maps: the pipelined kernel's float-reciprocal row decode (m -> image, row, column) at m up to 198 000.  It is stated exact
    # for m < 2^24; reaching that needs a 2 GB activation tensor and is not part of this suite.  (25 MB of activations.)
    Case("many_tiny_maps", 22000, 3, 3, 32, 4, 3, 1, 1),
]

GENERIC_GEOMETRY = [
    # conv_gather_mfma_kernel / conv_gather_bf16_kernel only: frcnn_conv_nhwc_x3g answers FRCNN_EUNSUPPORTED, math 1 falls back to the
    # older bf16 kernel.  cin 16 and 48: cin % 32 != 0
    Case("k2", 2, 6, 7, 16, 64, 2, 1, 0),
    Case("k2_p1s2", 2, 6, 7, 48, 32, 2, 2, 1),
    Case("k5", 2, 6, 7, 16, 32, 5, 1, 2),
    Case("k5_cin64_last_split_short", 1, 6, 7, 64, 16, 5, 1, 2),
    Case("k7_stem_like", 1, 9, 10, 16, 16, 7, 2, 3),
    Case("k3s3", 2, 8, 10, 48, 32, 3, 3, 1),
    Case("k3s4", 2, 9, 11, 48, 32, 3, 4, 1),            # stride larger than the filter: whole rows and columns of dx receive no tap
    Case("k1_p1", 2, 5, 6, 32, 32, 1, 1, 1),            # pad > R - 1: a ring of bias-only outputs
    Case("k1_p1s2", 2, 5, 6, 16, 32, 1, 2, 1),
    Case("k3_p3", 2, 5, 6, 32, 32, 3, 1, 3),
    Case("k3_p3s2", 2, 5, 6, 48, 16, 3, 2, 3),
]

CHANNEL_TAILS = (
    [Case("cout%d" % co, 1, 6, 7, 32, co, 3, 1, 1) for co in (4, 60, 64, 68, 128, 132)] +
    # the data gradient's output channels are the forward cin: cin % 16 != 0 is not a forward shape, those cases run the data and weight
    # gradients only (cout 32: math 1 reaches the pipelined kernel)
    [Case("cin%d" % ci, 1, 6, 7, ci, 32, 3, 1, 1) for ci in (4, 60, 64, 68, 128, 132)]
)

PLAN_SEAMS = [
    # rows at BM - 1, BM, BM + 1 (64: the pipelined kernel's cfg 3; 128: the float32 cfg 0; 256: the float32 cfg 1)
    Case("m63", 1, 7, 9, 32, 64, 1, 1, 0),
    Case("m64", 1, 8, 8, 64, 64, 1, 1, 0),
    Case("m65", 1, 5, 13, 96, 64, 1, 1, 0),
    Case("m127", 1, 1, 127, 128, 128, 1, 1, 0),
    Case("m128", 2, 8, 8, 32, 128, 3, 1, 1),
    Case("m129", 3, 1, 43, 32, 128, 3, 1, 1),
    Case("m255", 1, 15, 17, 32, 64, 3, 1, 1),
    Case("m256", 1, 16, 16, 32, 32, 1, 1, 0),
    Case("m257", 1, 1, 257, 32, 64, 1, 1, 0),
    # the pipelined kernel's block -> tile map: 7, 8, 9 row blocks of 64 (surplus blocks of a group of 8 leave; the next group starts)
    Case("mb7", 7, 8, 8, 32, 64, 3, 1, 1),
    Case("mb8", 8, 8, 8, 32, 128, 1, 1, 0),
    Case("mb9", 1, 19, 27, 32, 132, 3, 1, 1),
    # more than one row block AND column block of the 128 x 128 tile in the float32 and the older bf16 kernel, forward and data gradient
    Case("old_bf16_cfg0", 1, 6, 7, 16, 128, 3, 1, 1),
    Case("grid2x2_fwd", 1, 12, 13, 48, 132, 3, 1, 1),
    Case("grid2x2_dgrad", 1, 12, 13, 132, 48, 3, 1, 1),
    # deep reductions on small maps: splits, a last split shorter than the others, a last split shorter than the pipeline
    Case("split_k3_c64", 1, 7, 7, 64, 64, 3, 1, 1),
    Case("split_k3_c96", 1, 7, 7, 96, 128, 3, 1, 1),
    Case("split_k1_c544", 1, 5, 7, 544, 32, 1, 1, 0),
    Case("split_k3_c160", 2, 4, 4, 160, 160, 3, 1, 1),
    # the 128-row tiles of the pipelined kernel are the cost model's choice on large maps only: 128 x 64 (cfg 2) and 128 x 128 (cfg 0),
    # un-split (one row in the last tile), split (127 rows / one row in the last tile), and split with a last part of ONE stage, which is
    # shorter than their pipeline (D = 2)
    Case("x3cfg2", 1, 129, 129, 64, 16, 1, 1, 0),
    Case("x3cfg2_split", 1, 23, 89, 128, 16, 3, 1, 1),
    Case("x3cfg2_short", 1, 55, 55, 128, 16, 3, 1, 1),
    Case("x3cfg0", 1, 61, 149, 96, 132, 1, 1, 0),
    Case("x3cfg0_split", 1, 23, 89, 128, 128, 3, 1, 1),
    Case("x3cfg0_short", 1, 57, 58, 128, 128, 3, 1, 1),
]

CASES = X3_GEOMETRY + GENERIC_GEOMETRY + CHANNEL_TAILS + PLAN_SEAMS
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Gaussian data on the geometries only the generic kernels take (one per geometry)
RANDOM_CASES = [BY_NAME[n] for n in ("k2", "k5", "k7_stem_like", "k3s3", "k3s4", "k1_p1", "k3_p3")]

# impulses: one 1 in the activations (forward) or in the upstream gradient (data gradient), weights that name the tap
IMPULSE_CASES = [Case("impulse_k3p1", 3, 7, 7, 32, 32, 3, 1, 1), Case("impulse_k3p0", 3, 7, 7, 32, 32, 3, 1, 0),
                 Case("impulse_k3p2", 3, 7, 7, 32, 32, 3, 1, 2), Case("impulse_k3p1s2", 3, 7, 7, 32, 32, 3, 2, 1)]


def impulse_positions(n, h, w):
    """pixels (image, y, x) of an [n][h][w] map: the four corners, the last pixel of an image and the first of the next, and the rows on
    both sides of the 64- and 128-row tile seams where the map has them"""
    pos = [(0, 0, 0), (0, 0, w - 1), (0, h - 1, 0), (0, h - 1, w - 1), (n - 1, h - 1, w - 1)]
    if n > 1:
        pos.append((1, 0, 0))
    for m in (63, 64, 127, 128):
        if m < n * h * w:
            pos.append((m // (h * w), (m % (h * w)) // w, m % w))
    return sorted(set(pos))


def impulse_weights(c):
    """OIHW float32: w[co][ci][r][s] = 1 + tap on a few (co, ci) pairs, zero elsewhere"""
    w = torch.zeros(c.cout, c.cin, c.k, c.k)
    taps = 1.0 + torch.arange(c.k * c.k, dtype=torch.float32).reshape(c.k, c.k)
    for co, ci in ((0, 0), (1, 5), (c.cout - 1, c.cin - 1), (c.cout // 2, 17)):
        w[co, ci] = taps
    return w


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _gen(c, what):
    return torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (c.name, what)).encode()))


def _ints(shape, g):
    return torch.randint(-VMAX, VMAX + 1, shape, generator=g).to(torch.float32)


@functools.lru_cache(maxsize=None)
def operands(c):
    """dict of float32 CPU tensors: x [N][H][W][cin], w [cout][cin][k][k], b [cout], res_y / dz [N][Ho][Wo][cout], res_x [N][H][W][cin]"""
    ho, wo = out_hw(c)
    return {
        "x": _ints((c.N, c.H, c.W, c.cin), _gen(c, "x")),
        "w": _ints((c.cout, c.cin, c.k, c.k), _gen(c, "w")),
        "b": _ints((c.cout,), _gen(c, "b")),
        "res_y": _ints((c.N, ho, wo, c.cout), _gen(c, "res_y")),
        "dz": _ints((c.N, ho, wo, c.cout), _gen(c, "dz")),
        "res_x": _ints((c.N, c.H, c.W, c.cin), _gen(c, "res_x")),
    }


@functools.lru_cache(maxsize=None)
def gaussian_operands(c):
    g = _gen(c, "gauss")
    ho, wo = out_hw(c)
    return {
        "x": torch.randn((c.N, c.H, c.W, c.cin), generator=g),
        "w": torch.randn((c.cout, c.cin, c.k, c.k), generator=g) * (2.0 / (c.cin * c.k * c.k)) ** 0.5,
        "b": torch.randn((c.cout,), generator=g) * 0.1,
        "res_y": torch.randn((c.N, ho, wo, c.cout), generator=g),
        "dz": torch.randn((c.N, ho, wo, c.cout), generator=g),
        "res_x": torch.randn((c.N, c.H, c.W, c.cin), generator=g),
    }


def pack(w):
    """[cout][cin][k][k] -> the gather kernels' [k*k][cout][cin] pack"""
    cout, cin, k, _ = w.shape
    return w.permute(2, 3, 0, 1).reshape(k * k, cout, cin).contiguous()


def unpack(wp, k):
    """[k*k][cout][cin] -> [cout][cin][k][k]"""
    _, cout, cin = wp.shape
    return wp.reshape(k, k, cout, cin).permute(2, 3, 0, 1).contiguous()


def pack_dgrad(w):
    """[cout][cin][k][k] -> frcnn_pack_conv_dgrad's [k*k][cin][cout]"""
    return pack(w).permute(0, 2, 1).contiguous()


# ---- float64 references ---------------------------------------------------------------------------------------------------------
def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def ref_forward(c, x, w, b, res=None, relu=False, dtype=torch.float64):
    """F.conv2d plus bias, residual and ReLU; NHWC in, NHWC out"""
    y = nhwc(F.conv2d(nchw(x.to(dtype)), w.to(dtype), b.to(dtype), stride=c.stride, padding=c.pad))
    if res is not None:
        y = y + res.to(dtype)
    return torch.relu(y) if relu else y


def ref_dgrad(c, dz, w, res=None, dtype=torch.float64):
    """torch.nn.grad.conv2d_input (+ residual); NHWC in, NHWC out"""
    dx = nhwc(torch.nn.grad.conv2d_input((c.N, c.cin, c.H, c.W), w.to(dtype), nchw(dz.to(dtype)).contiguous(), stride=c.stride, padding=c.pad))
    return dx + res.to(dtype) if res is not None else dx


def ref_wgrad(c, x, dz, dtype=torch.float64):
    """torch.nn.grad.conv2d_weight, as the [k*k][cout][cin] pack"""
    dw = torch.nn.grad.conv2d_weight(nchw(x.to(dtype)).contiguous(), (c.cout, c.cin, c.k, c.k), nchw(dz.to(dtype)).contiguous(), stride=c.stride,
                                     padding=c.pad)
    return pack(dw)


@functools.lru_cache(maxsize=None)
def exact_references(c):
    """float64 references of the integer operands: 'y' / 'y_plain' (bias + residual + ReLU / bias only), 'dx' / 'dx_res', 'dw'; only the
    operations that take the case.  Computed once and shared: callers must not write to them."""
    o = operands(c)
    out = {}
    if forward_ok(c):
        out["y_plain"] = ref_forward(c, o["x"], o["w"], o["b"])
        out["y"] = ref_forward(c, o["x"], o["w"], o["b"], o["res_y"], relu=True)
    if dgrad_ok(c):
        out["dx"] = ref_dgrad(c, o["dz"], o["w"])
        out["dx_res"] = out["dx"] + o["res_x"].double()
    if wgrad_ok(c):
        out["dw"] = ref_wgrad(c, o["x"], o["dz"])
    return out


def untouched_dx_pixels(c):
    """bool [H][W]: input pixels no tap of any output pixel reads (stride past the filter, or trailing rows and columns where the stride does
    not divide H + 2 pad - k): their data gradient is the residual alone"""
    ho, wo = out_hw(c)

    def axis(n, no):
        hit = np.zeros(n, dtype=bool)
        for o in range(no):
            for r in range(c.k):
                i = o * c.stride - c.pad + r
                if 0 <= i < n:
                    hit[i] = True
        return hit
    return ~np.outer(axis(c.H, ho), axis(c.W, wo))


# ---- plan mirror (csrc/conv_gather.hip plan_gather, plan_gather_x3, gather_x3_takes and the launchers; default knobs) -------------
Plan = namedtuple("Plan", "kernel cfg bm bn depth mblocks nblocks splits sps stages M")
KNOBS = ("FRCNN_GATHER_BLOCKS", "FRCNN_GATHER_X3_CHIP", "FRCNN_GATHER_X3_SPLIT_US")
X3G_TILE_COUNTERS = 16384


def last_part(p):
    """stages of the last split"""
    return p.stages - p.sps * (p.splits - 1)


def plan_gather(M, cout, stages, bf16=False):
    cfg = 1 if cout <= 64 else 0
    bm, bn = (256, 64) if cfg == 1 else (128, 128)
    mblocks, nblocks = cdiv(M, bm), cdiv(cout, bn)
    blocks = mblocks * nblocks
    want = (256 if bf16 else 1280) // max(blocks, 1)
    cap = max(stages // 8, 1)
    want = max(min(want, cap), 1)
    if M * cout * 4 > (40 << 20):
        want = 1
    if blocks >= 512 and M >= 32768:
        want = 1
    sps = cdiv(stages, want)
    return Plan("bf16" if bf16 else "f32", cfg, bm, bn, 2, mblocks, nblocks, cdiv(stages, sps), sps, stages, M)


def plan_gather_x3(M, cout, stages):
    chip_bytes_per_us, split_us = 6.0e6, 3.5
    big = (2, 128, 64, 0.70, 2) if cout <= 64 else (0, 128, 128, 1.05, 2)
    best, best_t = None, 1e30
    for cfg, bm, bn, stage_us, depth in (big, (3, 64, 64, 0.42, 3)):
        mb, nb = cdiv(M, bm), cdiv(cout, bn)
        tiles = float(mb) * nb
        t_chip = tiles * stages * (bm + bn) * 128.0 / chip_bytes_per_us
        max_splits = min(max(stages // 4, 1), 16)
        for want in range(1, max_splits + 1):
            sps = cdiv(stages, want)
            splits = cdiv(stages, sps)
            if splits != want:
                continue
            rounds = float(cdiv(int(tiles * splits), 512))
            t = rounds * sps * stage_us
            if t < t_chip:
                t = t_chip
            t += 3.5
            if splits > 1:
                if splits * M * cout * 4 > (40 << 20):
                    continue
                t += split_us + float(splits + 1) * M * cout * 4.0 / 4.0e6
            if t < best_t:
                best_t, best = t, Plan("x3", cfg, bm, bn, depth, mb, nb, splits, sps, stages, M)
    return best


def x3_takes(N, H, W, cin, cout, k, pad, transposed, stride):
    """H, W, cin: the source tensor's (the upstream gradient's in the transposed form)"""
    return (k in (1, 3) and cin % 32 == 0 and pad <= k - 1 and not (transposed and stride != 1) and
            (N * H * W + k * W + k) * cin * 4 < (1 << 31) and k * k * cout * cin * 4 < (1 << 31))


def forward_takes_x3(c):
    return forward_ok(c) and x3_takes(c.N, c.H, c.W, c.cin, c.cout, c.k, c.pad, False, c.stride)


def dgrad_takes_x3(c):
    ho, wo = out_hw(c)
    return dgrad_ok(c) and x3_takes(c.N, ho, wo, c.cout, c.cin, c.k, c.pad, True, c.stride)


def forward_plans(c):
    """arithmetic -> Plan of the launch with the full workspace: 'f32' (frcnn_conv_nhwc, math 0), 'bf16' (math 1), 'x3g' where taken"""
    if not forward_ok(c):
        return {}
    M, taps = rows_forward(c), c.k * c.k
    plans = {"f32": plan_gather(M, c.cout, (c.cin // 16) * taps)}
    if forward_takes_x3(c):
        plans["x3g"] = plan_gather_x3(M, c.cout, (c.cin // 32) * taps)
        plans["bf16"] = plans["x3g"]
    else:
        plans["bf16"] = plan_gather(M, c.cout, (c.cin // 16) * taps, bf16=True)
    return plans


def dgrad_plans(c):
    """arithmetic -> Plan: rows are the input pixels, output channels the forward cin, the reduction runs over cout"""
    if not dgrad_ok(c):
        return {}
    M, taps = c.N * c.H * c.W, c.k * c.k
    plans = {"f32": plan_gather(M, c.cin, (c.cout // 16) * taps)}
    if dgrad_takes_x3(c):
        plans["bf16"] = plan_gather_x3(M, c.cin, (c.cout // 32) * taps)
    else:
        plans["bf16"] = plan_gather(M, c.cin, (c.cout // 16) * taps, bf16=True)
    return plans


def dgrad_pad_e(c):
    """the padding the pipelined kernel works with in the data-gradient form"""
    return c.k - 1 - c.pad


def conv_workspace_bytes(N, H, W, cin, cout, k, stride, pad):
    """mirror of frcnn_conv_workspace_bytes"""
    if cin % 16 != 0 or cout % 4 != 0:
        return 0
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if ho < 1 or wo < 1:
        return 0
    M = N * ho * wo
    p = plan_gather(M, cout, (cin // 16) * k * k)
    q = plan_gather_x3(M, cout, max(cin // 32, 1) * k * k)
    splits = max(p.splits, q.splits)
    return splits * M * cout * 4 if splits > 1 else 0


def dgrad_workspace_bytes(N, H, W, cin, cout, k, stride, pad):
    """mirror of frcnn_conv_dgrad_workspace_bytes"""
    if N < 1 or H < 1 or W < 1 or cout % 16 != 0 or k < 1 or stride < 1:
        return 0
    M = N * H * W
    p = plan_gather(M, cin, (cout // 16) * k * k)
    q = plan_gather_x3(M, cin, max(cout // 32, 1) * k * k)
    splits = max(p.splits, q.splits)
    return splits * M * cin * 4 if splits > 1 else 0


def ticket_finish(p):
    """the in-kernel finish of frcnn_conv_nhwc_x3g_tickets is taken (else the call behaves as frcnn_conv_nhwc_x3g)"""
    return p.splits > 1 and 8 * p.nblocks * cdiv(p.mblocks, 8) <= X3G_TILE_COUNTERS
