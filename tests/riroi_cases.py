"""Cases and the restatement of RiRoIAlignRotated (fasterrcnn_amd.ops.riroi_align_rotated), shared by tests/test_ops_riroi_cpu.py and
tests/test_ops_riroi_gpu.py.  The definition is the one include/frcnn_hip.h states (mmcv's riroi_align_rotated restated, unpinned):
pool every source channel as roi_align_rotated does (aligned off, the opposite clockwise flag), then blend each group's orientations.

reference(case, dtype) is the contract as a loop over (RoI, bin, sample) on numpy scalars of `dtype`, vectorised over the channels only:
in float64 it is the truth, with its analytic d_input; in float32 it is the mirror, written in the kernels' order (the backward sums per
cell over RoIs, then bins, each bin sending dS * (the sum of its samples' weights) / count), whose error against the truth measures the
bound of the tolerance tests:
    err(a) = max|a - truth| / max|truth|,   err_gpu <= 4 * max(err_ref, 2**-24),   max|truth| > 0.1,   no element masked.
The blend factors are part of the contract (f is rounded to float32 once), so the truth takes the same f and forms l, r = 1 - l exactly.

Nothing is masked, so the generic cases must stay away from the two places where the contract jumps: conditions_hold asserts that no
blend factor l lies within 1e-3 of 0 or 1 (there ind, and with it the source channels, would flip under a rounding of the angle) and that
no sample coordinate lies within 1e-3 of -1 or of the map's size (there a sample appears or vanishes).  make_case takes the first seed of
base, base + 1000, ... that meets them; the CPU test asserts them for every case."""
import functools
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
GAP = 1e-3
NAN, INF = float("nan"), float("inf")
CULL_LIST = 1024                                   # ops.ROI_ALIGN_ROTATED_CULL_LIST (asserted by the CPU test)
MAX_ORIENTATIONS = 64                              # ops.MAX_RIROI_ORIENTATIONS (asserted by the CPU test)

# name: (N, C, n, H, W), output_size, num_samples, clockwise, spatial_scale, K, seed
CASES = {
    "n8-c2": ((2, 2, 8, 12, 10), (3, 2), 2, False, 0.5, 6, 1),
    "n8-c2-clockwise": ((2, 2, 8, 12, 10), (3, 2), 2, True, 0.5, 6, 2),
    "n8-c2-adaptive": ((2, 2, 8, 12, 10), (3, 2), 0, False, 0.5, 6, 3),
    "n8-c2-adaptive-clockwise": ((2, 2, 8, 12, 10), (3, 2), 0, True, 0.5, 6, 4),
    "n1-c5": ((2, 5, 1, 12, 10), (3, 2), 2, False, 0.5, 6, 5),           # both sources are the channel itself; one pad run
    "n3-c3": ((2, 3, 3, 12, 10), (3, 2), 2, False, 0.5, 6, 6),           # 9 channels: groups straddle runs, one pad run
    "n4-c4": ((2, 4, 4, 12, 10), (3, 2), 2, True, 0.5, 6, 7),            # float16: two groups per run
    "n3-c86": ((2, 86, 3, 12, 10), (3, 2), 2, False, 0.5, 6, 8),         # 258 channels: a group across the 64-run boundary, pad
    "n64-c1": ((2, 1, 64, 12, 10), (3, 2), 0, False, 0.5, 6, 9),         # the largest group
    "n6-c11": ((2, 11, 6, 12, 10), (3, 2), 2, True, 0.5, 6, 10),         # 66 channels in 17 runs: three bins share a wave
}
TOLERANCE_CASES = list(CASES)


def f32(v):
    return float(np.float32(v))


def blend(angle, n):
    """The contract's blend factors of one angle: None for a RoI that pools to zeros, else (l, r = 1 - l in float32, k)."""
    a = float(np.float32(angle))
    if not math.isfinite(a):
        return None
    f = np.float32(np.float64(a) * n / (2 * np.pi))
    if not abs(f) < 2.0 ** 24:
        return None
    ind = np.floor(f)
    left = np.float32(f - ind)
    return left, np.float32(1) - left, int(ind) % n


def _build(name, seed):
    (n_img, c, n, h, w), out, ns, clockwise, scale, k, _ = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: torch.rand((k,), generator=gen, dtype=F64) * (hi - lo) + lo     # noqa: E731
    x = torch.randn((n_img, c * n, h, w), generator=gen, dtype=F32)
    cx, cy, rw, rh, ang = u(0.1 * w, 0.9 * w), u(0.1 * h, 0.9 * h), u(1.5, 0.7 * w), u(1.5, 0.7 * h), u(-math.pi, math.pi)
    b = (torch.arange(k) % n_img).to(F64)
    rois = torch.stack([b, cx / scale, cy / scale, rw / scale, rh / scale, ang], 1).to(F32)
    grad = torch.randn((k, c * n) + out, generator=gen, dtype=F32)
    return {"name": name, "input": x, "rois": rois, "output_size": out, "num_samples": ns, "clockwise": clockwise,
            "spatial_scale": f32(scale), "num_orientations": n, "grad": grad, "seed": seed}


def _axis(v, size, ft):
    """roi_align's rule for one coordinate known to lie in [-1, size]: (low, high, weight of low, weight of high)."""
    if v <= 0:
        v = ft(0)
    low = int(v)
    if low >= size - 1:
        low = high = size - 1
        v = ft(low)
    else:
        high = low + 1
    wh = v - ft(low)
    return low, high, ft(1) - wh, wh


def plan_of(case, dtype):
    """Per RoI None (a batch index outside (-1, N)) or (image, count, bins): bins[(ph, pw)] is the list, in (iy, ix) order, of the
    accepted samples (yl, yh, xl, xh, wyl, wyh, wxl, wxh); also the smallest distance of a sample coordinate to -1 or the map's size."""
    ft = np.float64 if dtype == F64 else np.float32
    rois = case["rois"].numpy().astype(ft)
    n_img, _, h, w = case["input"].shape
    oh, ow = case["output_size"]
    scale, ns = ft(case["spatial_scale"]), case["num_samples"]
    plans, seam = [], INF
    with np.errstate(invalid="ignore", over="ignore"):
        for roi in rois:
            if not (roi[0] > -1 and roi[0] < n_img):
                plans.append(None)
                continue
            cx, cy = roi[1] * scale, roi[2] * scale
            rw, rh = max(roi[3] * scale, ft(1)), max(roi[4] * scale, ft(1))
            t = roi[5] if case["clockwise"] else -roi[5]              # roi_align_rotated under the opposite flag
            cos, sin = np.cos(t), np.sin(t)
            bin_h, bin_w = rh / ft(oh), rw / ft(ow)
            gh = ns if ns > 0 else int(np.ceil(rh / ft(oh)))
            gw = ns if ns > 0 else int(np.ceil(rw / ft(ow)))
            count = ft(max(gh * gw, 1))
            bins = {}
            for ph in range(oh):
                for pw in range(ow):
                    hits = []
                    for iy in range(gh):
                        yy = (-rh / ft(2) + ft(ph) * bin_h) + ((ft(iy) + ft(0.5)) * bin_h) / ft(gh)
                        for ix in range(gw):
                            xx = (-rw / ft(2) + ft(pw) * bin_w) + ((ft(ix) + ft(0.5)) * bin_w) / ft(gw)
                            x = (yy * sin + xx * cos) + cx
                            y = (yy * cos - xx * sin) + cy
                            if math.isfinite(float(x)) and math.isfinite(float(y)):
                                seam = min(seam, abs(float(y) + 1), abs(float(y) - h), abs(float(x) + 1), abs(float(x) - w))
                            if not (-1 <= y <= h and -1 <= x <= w):       # a NaN fails
                                continue
                            hits.append(_axis(y, h, ft) + _axis(x, w, ft))
                    bins[(ph, pw)] = [(a[0], a[1], a[4], a[5], a[2], a[3], a[6], a[7]) for a in hits]
            plans.append((int(roi[0]), count, bins))
    return plans, seam


def reference(case, dtype):
    """(output [K, C n, oh, ow], d_input [N, C n, H, W], pooled S [K, C n, oh, ow]) of the contract in `dtype`, as torch tensors."""
    ft = np.float64 if dtype == F64 else np.float32
    x = case["input"].numpy().astype(ft)
    grad = case["grad"].numpy().astype(ft)
    n = case["num_orientations"]
    k_rois, channels = grad.shape[:2]
    oh, ow = case["output_size"]
    plans, _ = plan_of(case, dtype)
    pooled, out, dx = np.zeros(grad.shape, dtype=ft), np.zeros(grad.shape, dtype=ft), np.zeros(x.shape, dtype=ft)
    ch = np.arange(channels)
    base, o = ch // n * n, ch % n
    for r, plan in enumerate(plans):
        bl = blend(case["rois"][r, 5], n)
        if plan is None or bl is None:
            continue
        left, right, k = ft(bl[0]), (ft(1) - ft(bl[0]) if dtype == F64 else ft(bl[1])), bl[2]
        image, count, bins = plan
        fm = x[image]
        d_pooled = right * grad[r, base + (o + k) % n] + left * grad[r, base + (o + k - 1) % n]
        for (ph, pw), hits in bins.items():
            acc = np.zeros((channels,), dtype=ft)
            w_sum = {}
            for yl, yh, xl, xh, wyl, wyh, wxl, wxh in hits:
                acc = acc + (((fm[:, yl, xl] * (wyl * wxl) + fm[:, yl, xh] * (wyl * wxh)) + fm[:, yh, xl] * (wyh * wxl))
                             + fm[:, yh, xh] * (wyh * wxh))
                rows = {yl: wyl + wyh} if yl == yh else {yl: wyl, yh: wyh}
                cols = {xl: wxl + wxh} if xl == xh else {xl: wxl, xh: wxh}
                for cy, wy in rows.items():
                    for cx, wx in cols.items():
                        w_sum[(cy, cx)] = w_sum.get((cy, cx), ft(0)) + wy * wx
            pooled[r, :, ph, pw] = acc / count
            for (cy, cx), ws in w_sum.items():
                dx[image, :, cy, cx] += (d_pooled[:, ph, pw] * ws) / count
        out[r] = right * pooled[r, base + (o - k) % n] + left * pooled[r, base + (o - k + 1) % n]
    return torch.from_numpy(out), torch.from_numpy(dx), torch.from_numpy(pooled)


def blended_grad(case):
    """dS of the contract in float32 numpy, [K, C n, oh, ow]: what roi_align_rotated's backward must be given to reproduce d_input."""
    grad = case["grad"].numpy()
    n = case["num_orientations"]
    ch = np.arange(grad.shape[1])
    base, o = ch // n * n, ch % n
    ds = np.zeros_like(grad)
    n_img = case["input"].shape[0]
    for r in range(grad.shape[0]):
        bl = blend(case["rois"][r, 5], n)
        b = float(case["rois"][r, 0])
        if bl is None or not (b > -1 and b < n_img):
            continue
        left, right, k = bl
        ds[r] = right * grad[r, base + (o + k) % n] + left * grad[r, base + (o + k - 1) % n]
    return torch.from_numpy(ds)


def conditions_hold(case, truth):
    """The conditions of the module's docstring; returns a message, or None when they hold."""
    if not (float(truth[0].abs().max()) > 0.1 and float(truth[1].abs().max()) > 0.1):
        return "max|truth| <= 0.1"
    for angle in case["rois"][:, 5].tolist():
        bl = blend(angle, case["num_orientations"])
        if bl is None or not GAP < float(bl[0]) < 1 - GAP:
            return "a blend factor within 1e-3 of 0 or 1"
    if plan_of(case, F64)[1] < GAP:
        return "a sample within 1e-3 of -1 or of the map's size"
    return None


def check_conditions(case, truth):
    message = conditions_hold(case, truth)
    assert message is None, (case["name"], message)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(case, truth, mirror), computed once; the first seed of base, base + 1000, ... that meets the conditions."""
    base = CASES[name][6]
    for attempt in range(64):
        case = _build(name, base + 1000 * attempt)
        truth = reference(case, F64)
        if conditions_hold(case, truth) is None:
            return case, truth, reference(case, F32)
    raise AssertionError("no seed of %s meets the conditions" % name)


def rel_err(a, truth):
    return float((a.double() - truth.double()).abs().max()) / float(truth.double().abs().max())


def with_angles(case, angles):
    """The case with its first RoIs' angles replaced."""
    case = dict(case, rois=case["rois"].clone())
    for i, a in enumerate(angles):
        case["rois"][i, 5] = a
    return case


# ind = -1 with l near 1; more than a turn either way; the float32 nearest to pi / 4 from either side (n = 8: f next to 1)
QUARTER = np.float32(math.pi / 4)
WRAP_ANGLES = (-1e-3, 2 * math.pi + 0.3, -7.0, float(np.nextafter(QUARTER, np.float32(0))), float(QUARTER),
               float(np.nextafter(QUARTER, np.float32(1))))


def skipped_case():
    """A normal RoI (row 0) beside RoIs that pool to zeros: batch indices -1 and N, a NaN and an infinite angle, |f| >= 2 ** 24."""
    case = dict(_build("n8-c2", 1))
    n_img = case["input"].shape[0]
    rois = case["rois"].clone()
    rois[1, 0], rois[2, 0], rois[3, 5], rois[4, 5], rois[5, 5] = -1.0, float(n_img), NAN, INF, 2.0 ** 24
    rois[3:, 0] = 0.0
    case["rois"] = rois
    return case
