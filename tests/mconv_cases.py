"""Cases of fasterrcnn_amd.ops.masked_conv2d, their float64 truth and a float32 restatement; torch on the CPU only.

The truth of a case is F.conv2d in float64 on the CPU times the mask.  `restated` is the same sum evaluated in float32 on the CPU; for a
16-bit case it is that sum on the 16-bit-valued inputs, rounded once to the dtype.  rel_err(a, truth) = max|a - truth| / max|truth| over
the case.  The shapes are the smallest at which the kernels can still go wrong: they are built from the tile of listed pixels T, the tile
of output channels CO and the K chunk KC that fasterrcnn_amd.ops mirrors from the library's getters."""
import functools

import torch
import torch.nn.functional as F

from fasterrcnn_amd import ops

T, CO, KC = ops.MASKED_CONV_TILE_PIXELS, ops.MASKED_CONV_TILE_CHANNELS, ops.MASKED_CONV_K_CHUNK
F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
HALF = DTYPES[1:]
ROUNDING = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # half an ulp, relative: one rounding to nearest

COUNT_W = -(-(2 * T + 1) // 5)                                          # the smallest 5-row map that holds 2 T + 1 pixels
COUNTS = (0, 1, T - 1, T, T + 1, 2 * T + 1, 5 * COUNT_W)


def _case(n, c, h, w, co, k, pad, mask, seed):
    return dict(n=n, c=c, h=h, w=w, co=co, k=k, pad=pad, mask=mask, seed=seed)


CASES = {}
# active counts around the pixel tile: 3 x 3, pad 1, so the output grid is the 5-row map itself
for _i, _cnt in enumerate(COUNTS):
    CASES["count_%d" % _cnt] = _case(1, 3, 5, COUNT_W, 5, (3, 3), (1, 1), ("count", _cnt), 100 + _i)
# K = C_in kh kw: the odd tail of the 2-deep float32 MFMA, the non-multiples of 8 and 16 of the 16-bit one, one chunk + 1
K_SHAPES = {1: (1, 1, 1), 2: (2, 1, 1), 3: (1, 1, 3), 9: (1, 3, 3), 27: (3, 3, 3), 45: (5, 3, 3), 50: (2, 5, 5), KC + 1: ((KC + 1) // 3, 1, 3)}
assert all(c * kh * kw == k for k, (c, kh, kw) in K_SHAPES.items())
for _i, (_k, (_c, _kh, _kw)) in enumerate(K_SHAPES.items()):
    CASES["K_%d" % _k] = _case(2, _c, 7, 9, 5, (_kh, _kw), (_kh // 2, _kw // 2), ("random", 0.5), 200 + _i)
# C_out around the channel tile
C_OUTS = (1, 4, 31, 32, 33, 80, CO + 1)
for _i, _co in enumerate(C_OUTS):
    CASES["Cout_%d" % _co] = _case(1, 4, 6, 7, _co, (3, 3), (1, 1), ("random", 0.5), 300 + _i)
# kernels and paddings: the output grid equal to, smaller than and larger than the map
KERNELS = {"1x1_p0": ((1, 1), (0, 0)), "3x3_p1": ((3, 3), (1, 1)), "3x3_p0": ((3, 3), (0, 0)), "3x3_p2": ((3, 3), (2, 2)),
           "1x3_p01": ((1, 3), (0, 1)), "5x5_p2": ((5, 5), (2, 2))}
for _i, (_name, (_k, _pad)) in enumerate(KERNELS.items()):
    CASES["kernel_" + _name] = _case(2, 3, 7, 8, 6, _k, _pad, ("random", 0.5), 400 + _i)
# three images: an empty mask, a full one, a random one
CASES["n3"] = _case(3, 3, 6, 9, 5, (3, 3), (1, 1), ("n3",), 500)

VALUE_CASES = tuple(n for n in CASES if n != "count_0")                 # count_0 has no scale: its output is checked to be all +0.0
COUNT_CASES = tuple("count_%d" % c for c in COUNTS)


def out_grid(spec):
    return spec["h"] + 2 * spec["pad"][0] - spec["k"][0] + 1, spec["w"] + 2 * spec["pad"][1] - spec["k"][1] + 1


@functools.lru_cache(maxsize=None)
def case(name, dtype=F32):
    """(features, mask, weight, bias) on the CPU: features, weight and bias of `dtype`, a float32 mask with negatives and zeros where it
    is inactive.  A 16-bit case holds the float32 case's values rounded to the dtype."""
    s = CASES[name]
    g = torch.Generator().manual_seed(s["seed"])
    n, c, co, (kh, kw) = s["n"], s["c"], s["co"], s["k"]
    oh, ow = out_grid(s)
    x = torch.randn((n, c, s["h"], s["w"]), generator=g)
    wt = torch.randn((co, c, kh, kw), generator=g) / (c * kh * kw) ** 0.5          # outputs of order 1: far from float16's subnormals
    b = torch.randn((co,), generator=g)
    kind = s["mask"][0]
    if kind == "count":
        active = torch.zeros(n * oh * ow, dtype=torch.bool)
        active[torch.randperm(n * oh * ow, generator=g)[:s["mask"][1]]] = True
        active = active.view(n, oh, ow)
    elif kind == "random":
        active = torch.rand((n, oh, ow), generator=g) < s["mask"][1]
    else:
        active = torch.rand((n, oh, ow), generator=g) < 0.5
        active[0], active[1] = False, True
    values = torch.rand((n, oh, ow), generator=g) + 0.25
    mask = torch.where(active, values, torch.where(values > 0.75, -values, torch.zeros_like(values)))
    return x.to(dtype), mask, wt.to(dtype), b.to(dtype)


def dense(x, mask, wt, b, pad, dtype):
    """conv2d evaluated in `dtype` on the CPU, times the mask."""
    y = F.conv2d(x.to(dtype), wt.to(dtype), None if b is None else b.to(dtype), padding=pad)
    return y * (mask > 0)[:, None].to(dtype)


@functools.lru_cache(maxsize=None)
def truth(name, dtype=F32):
    """float64, from the case's (possibly 16-bit-valued) inputs."""
    x, mask, wt, b = case(name, dtype)
    return dense(x, mask, wt, b, CASES[name]["pad"], F64)


@functools.lru_cache(maxsize=None)
def restated(name, dtype=F32):
    """The same sum in float32 on the CPU, rounded once to a 16-bit dtype."""
    x, mask, wt, b = case(name, dtype)
    return dense(x, mask, wt, b, CASES[name]["pad"], F32).to(dtype)


def rel_err(a, want):
    return float((a.to(F64) - want).abs().max() / want.abs().max())
