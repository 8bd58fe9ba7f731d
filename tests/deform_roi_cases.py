"""Cases and a torch restatement of deformable RoI pooling (fasterrcnn_amd.ops.deform_roi_pool), shared by tests/test_ops_droi_cpu.py
and tests/test_ops_droi_gpu.py.  The definition is the one include/frcnn_hip.h states (mmcv's deform_roi_pool restated, unpinned).

The restatement runs on the CPU in float64 (the truth) or float32 (whose error against the truth measures the bound of the GPU tests):
the forward is vectorised over (RoI, ph, pw, iy, ix, channel), d_x and d_offset are written out by the published formulas, not autograd.
The forward follows the device of the case's tensors (tools/ops_bench.py times it on the GPU as the composition from torch operations).

Seams.  Every quantity jumps where a sample coordinate crosses -1 or size, and d_offset jumps at every integer (its formula uses the
corner indices), so a float32 and a float64 evaluation may decide a sample that lies within rounding of an integer differently.
near_seam(case) marks, in float64, every (RoI, bin) one of whose grid_h + grid_w sample coordinates lies within DELTA = 2**-10 of an
integer in [-1, size]; marked bins get a zero grad_output and are left out of the output and d_offset comparisons.  Two conditions make
that sufficient and are asserted per case (check_conditions): at most 5 % of a case's bins are marked, and the float32 coordinates
differ from the float64 ones by less than DELTA / 4 -- so an unmarked coordinate is on the same side of every integer in both.  The
second is taken over the samples whose float64 coordinate is finite and below 2**20 in magnitude; the others (the +inf, -inf, NaN and
1e30 offsets of the `nonfinite` case) must be non-finite or beyond 2**20 in float32 as well: both evaluations reject them.
"""
import functools

import torch

F32, F64 = torch.float32, torch.float64
DELTA = 2.0 ** -10
FAR = 2.0 ** 20
CULL_LIST = 256                                    # ops.DEFORM_ROI_CULL_LIST (asserted by the CPU test)


def f32(v):
    """A Python float rounded to float32, as the kernels receive spatial_scale and gamma."""
    return float(torch.tensor(v, dtype=F32))


# name: (N, C, H, W), output_size, sampling_ratio, gamma, spatial_scale, K, RoI kind, offset kind, seed
# RoI kinds: "mixed" (ordinary RoIs of both images interleaved, with a zero-width, a negative-height and a larger-than-the-map RoI and
# the batch indices -1, N and NaN at fixed rows when K >= 16), "cover" (every RoI covers the whole map: they all reach every tile).
# Offset kinds: None, "zeros", "normal" (N(0, 0.5)), "border" (a tenth of the bins pushed wholly off the map, a tenth straddling its
# border, the rest N(0, 0.5)), "nonfinite" (N(0, 0.5) with +inf, -inf, NaN and 1e30 in four bins).
CASES = {
    "1x1-k1": ((1, 4, 1, 1), (1, 1), 2, 0.1, 1.0, 1, "mixed", "normal", 11),
    "1x1-adaptive": ((1, 4, 1, 1), (3, 5), 0, 1.0, 1.0, 37, "mixed", "normal", 12),
    "5x4-c6-adaptive": ((2, 6, 5, 4), (3, 5), 0, 0.1, 1 / 16, 37, "mixed", "normal", 13),
    "13x17-border": ((2, 6, 13, 17), (7, 7), 2, 1.0, 1 / 16, 37, "mixed", "border", 14),
    "13x17-none": ((2, 4, 13, 17), (7, 7), 0, 0.1, 1.0, 37, "mixed", None, 15),
    "13x17-zeros": ((2, 6, 13, 17), (3, 5), 2, 0.1, 1 / 16, 37, "mixed", "zeros", 16),
    "c260-cull": ((1, 260, 5, 4), (1, 1), 2, 0.1, 1.0, CULL_LIST + 1, "cover", "normal", 17),
    "c260-two-images": ((2, 260, 5, 4), (3, 5), 2, 1.0, 1.0, 37, "mixed", "normal", 18),
    "nonfinite": ((2, 6, 13, 17), (3, 5), 2, 0.1, 1 / 16, 37, "mixed", "nonfinite", 19),
    "k0": ((1, 4, 5, 4), (3, 5), 2, 0.1, 1.0, 0, "mixed", "normal", 20),
}
NONFINITE = (float("inf"), float("-inf"), float("nan"), 1e30)
NONFINITE_BINS = ((0, 0, 1, 2), (2, 1, 0, 4), (4, 0, 2, 0), (6, 1, 1, 1))      # (RoI, offset channel, ph, pw) of the four values


def _rois(gen, n, h, w, k, kind, scale):
    u = lambda lo, hi: torch.rand((k,), generator=gen, dtype=F64) * (hi - lo) + lo     # noqa: E731
    if kind == "cover":
        x1, y1, x2, y2 = u(-1.0, 0.0), u(-1.0, 0.0), u(w - 1.0, w), u(h - 1.0, h)
    else:
        x1, y1 = u(-1.0, 0.6 * w), u(-1.0, 0.6 * h)
        x2, y2 = x1 + u(0.5, 0.7 * w + 0.5), y1 + u(0.5, 0.7 * h + 0.5)
    b = (torch.arange(k) % n).to(F64)
    if kind == "mixed" and k >= 16:
        x2[3] = x1[3]                                                      # zero width
        y2[5] = y1[5] - 2.0                                                # negative height
        x1[7], y1[7], x2[7], y2[7] = -float(w), -float(h), 2.0 * w, 2.0 * h   # larger than the map
        b[9], b[11], b[13] = -1.0, float(n), float("nan")
    # map coordinates + 0.5 (the aligned half pixel), in image coordinates
    box = (torch.stack([x1, y1, x2, y2], 1) + 0.5) / scale
    return torch.cat([b[:, None], box], 1).to(F32)


def _offsets(gen, case, kind):
    k = case["rois"].shape[0]
    oh, ow = case["output_size"]
    if kind is None:
        return None
    if kind == "zeros":
        return torch.zeros((k, 2, oh, ow), dtype=F32)
    off = (torch.randn((k, 2, oh, ow), generator=gen, dtype=F64) * 0.5)
    if kind == "border":
        g = geometry(dict(case, offset=None), F64)
        _, _, h, w = case["input"].shape
        pick = torch.rand((k, oh, ow), generator=gen, dtype=F64)
        side = torch.rand((k, oh, ow), generator=gen, dtype=F64) < 0.5
        usable = (g["valid"] & (g["roi_w"] > 0.5) & (g["roi_h"] > 0.5))[:, None, None]
        for ch, size, roi, start, binsz, grid, p in ((0, w, g["roi_w"], g["start_w"], g["bin_w"], g["grid_w"], torch.arange(ow)[None, None, :]),
                                                     (1, h, g["roi_h"], g["start_h"], g["bin_h"], g["grid_h"], torch.arange(oh)[None, :, None])):
            roi, start, binsz, grid = (t[:, None, None] for t in (roi, start, binsz, grid.clamp(min=1).to(F64)))
            shift = case["gamma"] * roi
            axis = (torch.arange(k)[:, None, None] + ch) % 2 == 0           # which axis of this bin is moved
            gone = torch.where(side, -2.0 - roi, torch.full_like(roi, size + 1.0))
            edge = torch.where(side, torch.full_like(roi, -1.0), torch.full_like(roi, float(size))) - (p + 0.5) * binsz + 0.13 * binsz / grid
            off[:, ch] = torch.where(usable & axis & (pick < 0.1), (gone - start) / shift, off[:, ch])
            off[:, ch] = torch.where(usable & axis & (pick >= 0.1) & (pick < 0.2), (edge - start) / shift, off[:, ch])
    off = off.to(F32)
    if kind == "nonfinite":
        for (r, ch, ph, pw), v in zip(NONFINITE_BINS, NONFINITE):
            off[r, ch, ph, pw] = v
    return off


@functools.lru_cache(maxsize=None)
def make_case(name):
    (n, c, h, w), out, sr, gamma, scale, k, roi_kind, off_kind, seed = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    case = {"name": name, "input": torch.randn((n, c, h, w), generator=gen, dtype=F32), "output_size": out, "sampling_ratio": sr,
            "gamma": f32(gamma), "spatial_scale": f32(scale), "offset_kind": off_kind}
    case["rois"] = _rois(gen, n, h, w, k, roi_kind, case["spatial_scale"])
    case["offset"] = _offsets(gen, case, off_kind)
    grad = torch.randn((k, c) + out, generator=gen, dtype=F32)
    case["seam"] = near_seam(case)
    case["grad"] = torch.where(case["seam"][:, None], torch.zeros(()), grad)              # marked bins send nothing
    return case


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def geometry(case, dtype, offset=None):
    """The sampling plan in `dtype`: per RoI start, size, bin, grid, count, validity and image; per (RoI, ph, pw) the shifted starts;
    per sample the coordinates y [K, oh, ow, Gh], x [K, oh, ow, Gw] and which samples exist (iy < grid_h, ix < grid_w).
    offset: a tensor to use in place of the case's (the CPU test passes one that requires grad)."""
    r = case["rois"].to(dtype)
    n = case["input"].shape[0]
    oh, ow = case["output_size"]
    k, dev = r.shape[0], r.device
    scale, gamma, sr = case["spatial_scale"], case["gamma"], case["sampling_ratio"]
    valid = (r[:, 0] > -1) & (r[:, 0] < n)                                                # NaN fails
    g = {"valid": valid, "image": torch.where(valid, r[:, 0], torch.zeros_like(r[:, 0])).to(torch.int64)}
    g["start_w"], g["start_h"] = r[:, 1] * scale - 0.5, r[:, 2] * scale - 0.5
    g["roi_w"], g["roi_h"] = (r[:, 3] * scale - 0.5) - g["start_w"], (r[:, 4] * scale - 0.5) - g["start_h"]
    g["bin_w"], g["bin_h"] = g["roi_w"] / ow, g["roi_h"] / oh
    if sr > 0:
        g["grid_w"] = g["grid_h"] = torch.full((k,), sr, dtype=torch.int64, device=dev)
    else:
        g["grid_w"], g["grid_h"] = torch.ceil(g["roi_w"] / ow).to(torch.int64), torch.ceil(g["roi_h"] / oh).to(torch.int64)
    g["count"] = (g["grid_h"] * g["grid_w"]).clamp(min=1).to(dtype)
    sw, sh = g["start_w"][:, None, None].expand(k, oh, ow), g["start_h"][:, None, None].expand(k, oh, ow)
    off = case["offset"] if offset is None else offset
    if off is not None:
        off = off.to(dtype)
        sw = sw + (gamma * g["roi_w"])[:, None, None] * off[:, 0]
        sh = sh + (gamma * g["roi_h"])[:, None, None] * off[:, 1]
    g["sw"], g["sh"] = sw, sh
    for axis, start, binsz, grid, p in (("y", sh, g["bin_h"], g["grid_h"], torch.arange(oh, device=dev)[None, :, None, None]),
                                        ("x", sw, g["bin_w"], g["grid_w"], torch.arange(ow, device=dev)[None, None, :, None])):
        top = max(int(grid.max()), 1) if k else 1
        i = torch.arange(top, device=dev)[None, None, None, :]
        binsz, grid = binsz[:, None, None, None], grid[:, None, None, None]
        g[axis] = (start[..., None] + p.to(dtype) * binsz) + ((i.to(dtype) + 0.5) * binsz) / grid.clamp(min=1).to(dtype)
        g["exists_" + axis] = i < grid
    return g


def _axis(v, exists, size, dtype):
    """axis_weights over a tensor of coordinates: (accepted, low, high, weight of low, weight of high); a NaN or infinite coordinate
    fails the range test and is replaced before the conversion to an integer."""
    ok = exists & (v >= -1) & (v <= size)
    c = torch.where(ok, v, torch.zeros_like(v)).clamp(min=0)
    low = c.detach().floor().to(torch.int64)
    top = low >= size - 1
    low = torch.where(top, torch.full_like(low, size - 1), low)
    high = torch.where(top, low, low + 1)
    c = torch.where(top, low.to(dtype), c)
    wh = c - low.to(dtype)
    return ok, low, high, 1 - wh, wh


def _samples(case, dtype, offset=None, input=None):
    g = geometry(case, dtype, offset)
    x = (case["input"] if input is None else input).to(dtype).permute(0, 2, 3, 1)          # [N, H, W, C]
    h, w = x.shape[1:3]
    yok, yl, yh, hy, ly = (t[..., :, None] for t in _axis(g["y"], g["exists_y"], h, dtype))
    xok, xl, xh, hx, lx = (t[..., None, :] for t in _axis(g["x"], g["exists_x"], w, dtype))
    b = g["image"][:, None, None, None, None]
    s = {"g": g, "x": x, "mask": (yok & xok & g["valid"][:, None, None, None, None])[..., None], "b": b, "yl": yl, "yh": yh, "xl": xl, "xh": xh}
    s["w"] = [(hy * hx)[..., None], (hy * lx)[..., None], (ly * hx)[..., None], (ly * lx)[..., None]]
    s["v"] = [x[b, yl, xl], x[b, yl, xh], x[b, yh, xl], x[b, yh, xh]]                       # [K, oh, ow, Gh, Gw, C]
    return s


def forward_ref(case, dtype, offset=None, input=None):
    """[K, C, oh, ow] in dtype; differentiable in `input` and `offset` when they are given and require grad."""
    s = _samples(case, dtype, offset, input)
    (v1, v2, v3, v4), (w1, w2, w3, w4) = s["v"], s["w"]
    val = ((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4
    out = torch.where(s["mask"], val, torch.zeros_like(val)).sum((3, 4)) / s["g"]["count"][:, None, None, None]
    return out.permute(0, 3, 1, 2)


def grads_ref(case, dtype, grad=None):
    """(d_x [N, C, H, W], d_offset [K, 2, oh, ow] or None) by the published formulas."""
    s = _samples(case, dtype)
    g = s["g"]
    grad = (case["grad"] if grad is None else grad).to(dtype).permute(0, 2, 3, 1)
    gm = (grad / g["count"][:, None, None, None])[:, :, :, None, None, :]
    gm = torch.where(s["mask"], gm, torch.zeros_like(gm))                                 # [K, oh, ow, Gh, Gw, C]
    dx = torch.zeros_like(s["x"])
    for (iy, ix), wt in zip(((s["yl"], s["xl"]), (s["yl"], s["xh"]), (s["yh"], s["xl"]), (s["yh"], s["xh"])), s["w"]):
        idx = torch.broadcast_tensors(s["b"], iy, ix)
        dx.index_put_(tuple(idx), gm * wt, accumulate=True)
    doff = None
    if case["offset"] is not None:
        v1, v2, v3, v4 = s["v"]
        ok = s["mask"][..., 0]
        y = torch.where(ok, g["y"][..., :, None], torch.zeros((), dtype=dtype))[..., None]      # as computed, before the clamp
        x = torch.where(ok, g["x"][..., None, :], torch.zeros((), dtype=dtype))[..., None]
        yl, yh, xl, xh = (s[n][..., None].to(dtype) for n in ("yl", "yh", "xl", "xh"))
        tx = ((v4 * (y - yl) + v2 * (yh - y)) + v3 * (yl - y)) + v1 * (y - yh)
        ty = ((v4 * (x - xl) + v3 * (xh - x)) + v2 * (xl - x)) + v1 * (x - xh)
        gamma = case["gamma"]
        doff = torch.stack([(gamma * g["roi_w"])[:, None, None] * (gm * tx).sum((3, 4, 5)),
                            (gamma * g["roi_h"])[:, None, None] * (gm * ty).sum((3, 4, 5))], 1)
        doff = torch.where(g["valid"][:, None, None, None], doff, torch.zeros_like(doff))
    return dx.permute(0, 3, 1, 2), doff


def roi_align_ref(case, dtype):
    """Aligned RoIAlign restated on its own, without the offset path: per RoI one product grid of out_h grid_h sample rows and
    out_w grid_w sample columns, whose axis weights are computed once per row and column; [K, C, oh, ow]."""
    r = case["rois"].to(dtype)
    x = case["input"].to(dtype)
    n, c, h, w = x.shape
    oh, ow = case["output_size"]
    scale, sr = case["spatial_scale"], case["sampling_ratio"]
    out = torch.zeros((r.shape[0], c, oh, ow), dtype=dtype)
    for k in range(r.shape[0]):
        b = float(r[k, 0])
        if not (b > -1 and b < n):
            continue
        plane = x[int(b)]
        grid, lo, hi, wl, wh, ok = ({} for _ in range(6))
        for axis, c1, c2, n_out, limit in (("y", 2, 4, oh, h), ("x", 1, 3, ow, w)):
            start = r[k, c1] * scale - 0.5
            size = (r[k, c2] * scale - 0.5) - start
            binsz = size / n_out
            grid[axis] = sr if sr > 0 else int(torch.ceil(size / n_out))
            if grid[axis] <= 0:
                break
            p = torch.arange(n_out).repeat_interleave(grid[axis]).to(dtype)
            i = torch.arange(grid[axis]).repeat(n_out).to(dtype)
            v = (start + p * binsz) + ((i + 0.5) * binsz) / grid[axis]
            ok[axis] = (v >= -1) & (v <= limit)
            v = torch.where(ok[axis], v, torch.zeros_like(v)).clamp(min=0)
            low = v.floor().to(torch.int64)
            top = low >= limit - 1
            lo[axis] = torch.where(top, torch.full_like(low, limit - 1), low)
            hi[axis] = torch.where(top, lo[axis], low + 1)
            v = torch.where(top, lo[axis].to(dtype), v)
            wh[axis] = torch.where(ok[axis], v - lo[axis].to(dtype), torch.zeros_like(v))
            wl[axis] = torch.where(ok[axis], 1 - (v - lo[axis].to(dtype)), torch.zeros_like(v))
        if grid.get("y", 0) <= 0 or grid.get("x", 0) <= 0:
            continue
        ly, hy, lx, hx = lo["y"][:, None], hi["y"][:, None], lo["x"][None, :], hi["x"][None, :]
        val = ((plane[:, ly, lx] * (wl["y"][:, None] * wl["x"][None, :]) + plane[:, ly, hx] * (wl["y"][:, None] * wh["x"][None, :]))
               + plane[:, hy, lx] * (wh["y"][:, None] * wl["x"][None, :])) + plane[:, hy, hx] * (wh["y"][:, None] * wh["x"][None, :])
        count = max(grid["y"] * grid["x"], 1)
        out[k] = val.reshape(c, oh, grid["y"], ow, grid["x"]).sum((2, 4)) / count
    return out


# ---- seams ------------------------------------------------------------------------------------------------------------------------------
def near_seam(case):
    """bool [K, oh, ow]: the bins one of whose sample coordinates (float64) lies within DELTA of an integer in [-1, size]."""
    g = geometry(case, F64)
    h, w = case["input"].shape[2:]
    marks = []
    for axis, size in (("y", h), ("x", w)):
        v = g[axis]
        nearest = torch.round(v)
        near = g["exists_" + axis] & ((v - nearest).abs() < DELTA) & (nearest >= -1) & (nearest <= size)
        marks.append(near.any(-1))
    return (marks[0] | marks[1]) & g["valid"][:, None, None]


def interior(case):
    """bool [K, oh, ow]: the bins whose samples (float64) all lie strictly inside (0, size - 1) on both axes, where the published
    d_offset is the exact derivative of the forward."""
    g = geometry(case, F64)
    h, w = case["input"].shape[2:]
    inside = []
    for axis, size in (("y", h), ("x", w)):
        v = g[axis]
        inside.append((~g["exists_" + axis] | ((v > 0) & (v < size - 1))).all(-1) & g["exists_" + axis].any(-1))
    return inside[0] & inside[1] & g["valid"][:, None, None]


def check_conditions(case):
    """The two conditions of the module docstring, and equal sampling grids in float32 and float64; returns the marked fraction."""
    seam = case["seam"]
    fraction = float(seam.double().mean()) if seam.numel() else 0.0
    assert fraction <= 0.05, (case["name"], fraction)
    g32, g64 = geometry(case, F32), geometry(case, F64)
    assert torch.equal(g32["grid_h"], g64["grid_h"]) and torch.equal(g32["grid_w"], g64["grid_w"]), case["name"]
    for axis in ("y", "x"):
        a, b = g32[axis].double(), g64[axis]
        exists = g64["exists_" + axis] & g64["valid"][:, None, None, None]
        near = exists & torch.isfinite(b) & (b.abs() < FAR)
        far = exists & ~near
        if near.any():
            assert float((a - b)[near].abs().max()) < DELTA / 4, (case["name"], axis)
        assert bool((~torch.isfinite(a[far]) | (a[far].abs() >= FAR)).all()), (case["name"], axis)
    return fraction


def rel_err(a, truth):
    return float((a.double() - truth.double()).abs().max() / truth.double().abs().max())


def masked(t, case):
    """t [K, C or 2, oh, ow] with the near-seam bins zeroed: what the comparisons look at."""
    return torch.where(case["seam"][:, None].to(t.device), torch.zeros((), dtype=t.dtype, device=t.device), t)
