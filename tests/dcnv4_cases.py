"""DCNv4 (fasterrcnn_amd.ops.dcnv4) restated twice in float64, and the named, seeded cases the CPU and GPU tests share.

  dcnv4_composition  unpack the record, drop the centre location when asked, then the composition users know: pad, reference points and
                     the dilated grid in normalised coordinates of the padded map, one F.grid_sample(align_corners=False, zero padding),
                     the sum over the P points weighted by the raw masks (no softmax).
  dcnv4_explicit     the rule of include/frcnn_hip.h written out: the record read in place (slice of group g at 3 P g, pairs (dx, dy) at
                     2 p, masks at 2 P + p, the pad never touched), a loop over the P points and the four corners; the integer part of the
                     coordinate plus ((i dil - b) + offset) * offset_scale in pixels of the unpadded map, the "x > -1 and x < W" test, the
                     corners floor / floor + 1 with their weights, a corner outside the map counting 0.  floor carries no gradient, so
                     autograd gives the right-hand slope at an integer coordinate and nothing for a sample that does not count.  It runs
                     in any dtype: in float64 it is the truth, in float32 on the CPU it measures the error a float32 evaluation makes
                     (err_ref of the GPU tests).

Gradients come from torch.autograd through both: d_input and ONE d_offset_mask laid out as offset_mask.  Every case is checked when it is
first built: the two restatements agree (forward 1e-13, gradients 1e-12 relative to the largest entry), the fractional part of every
coordinate lies in [1/16, 15/16] as float32 and as float64 evaluate it (d_offset is discontinuous at integer coordinates and the sample
test flips at -1 and at the size), and the explicit restatement's gradient on the pad lanes is exactly 0.  The pad lanes of every case
hold a non-zero constant; masks are randn (signed, not normalised) except in "one-cell", which keeps dcnv3's softmax masks to measure
the same gather at the same depth.
"""
import functools

import torch

from fasterrcnn_amd import _native as nv

from tests import dcnv3_cases as K3

F32, F64 = torch.float32, torch.float64
CORNERS = K3.CORNERS
LABELS = ("out", "d_input", "d_offset", "d_mask")
PAD_VALUE = 7.0
out_size = K3.out_size


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def points(kh, kw, remove_center):
    """The grid points (i along x, j along y) an item samples, in order: x is the outer index; the centre is dropped when asked."""
    pts = [(i, j) for i in range(kw) for j in range(kh)]
    if remove_center:
        pts.remove((kw // 2, kh // 2))
    return pts


def record(group, p):
    return (group * p * 3 + 7) // 8 * 8


def unpack(offset_mask, group, p):
    """(offset [N, Ho, Wo, G P 2], mask [N, Ho, Wo, G P], pad [N, Ho, Wo, L - 3 G P]) of a packed tensor (views where possible)."""
    n, ho, wo, length = offset_mask.shape
    assert length == record(group, p)
    rec = offset_mask[..., :group * p * 3].reshape(n, ho, wo, group, p * 3)
    return rec[..., :2 * p].reshape(n, ho, wo, group * p * 2), rec[..., 2 * p:].reshape(n, ho, wo, group * p), offset_mask[..., group * p * 3:]


def pack(offset, mask, group, p, fill=0.0):
    """offset [N, Ho, Wo, G P 2] and mask [N, Ho, Wo, G P] as one [N, Ho, Wo, L] tensor, the pad lanes holding fill."""
    n, ho, wo, _ = offset.shape
    rec = torch.cat([offset.reshape(n, ho, wo, group, 2 * p), mask.reshape(n, ho, wo, group, p)], -1).reshape(n, ho, wo, group * p * 3)
    return torch.nn.functional.pad(rec, [0, record(group, p) - group * p * 3], value=fill)


def geometry(kernel, stride=(1, 1), pad=(0, 0), dil=(1, 1), group=1, gc=1, scale=1.0, remove_center=False):
    """The trailing arguments of dcnv4_core_pytorch, in upstream's order, from pairs (h, w)."""
    return (kernel[0], kernel[1], stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], group, gc, scale, remove_center)


def apply_args(geom, im2col_step=256):
    """geom with im2col_step where DCNv4Function.apply takes it: before remove_center."""
    return geom[:-1] + (im2col_step, geom[-1])


# ---- the two restatements -------------------------------------------------------------------------------------------------------------
def coordinates(offset_mask, h, w, kh, kw, sh, sw, ph, pw, dh, dw, group, scale, remove_center):
    """(x, y) [N, Ho, Wo, G, P] of every sample in offset_mask's dtype: the integer part exactly, then ((i dil - b) + offset) * scale."""
    n, ho, wo = offset_mask.shape[:3]
    pts = points(kh, kw, remove_center)
    p = len(pts)
    dtype = offset_mask.dtype
    rec = offset_mask[..., :group * p * 3].reshape(n, ho, wo, group, p * 3)
    bx, by = (dw * (kw - 1)) // 2, (dh * (kh - 1)) // 2
    base_x = (torch.arange(wo) * sw - pw + bx).to(dtype).view(1, 1, wo, 1, 1)
    base_y = (torch.arange(ho) * sh - ph + by).to(dtype).view(1, ho, 1, 1, 1)
    tap_x = torch.tensor([i * dw - bx for i, j in pts]).to(dtype).view(1, 1, 1, 1, p)
    tap_y = torch.tensor([j * dh - by for i, j in pts]).to(dtype).view(1, 1, 1, 1, p)
    return base_x + (tap_x + rec[..., 0:2 * p:2]) * scale, base_y + (tap_y + rec[..., 1:2 * p:2]) * scale


def dcnv4_explicit(input, offset_mask, kh, kw, sh, sw, ph, pw, dh, dw, group, gc, scale, remove_center):
    """[N, Ho, Wo, G Gc] in input's dtype; differentiable in input and offset_mask."""
    dtype = input.dtype
    n, h, w, _ = input.shape
    ho, wo = offset_mask.shape[1], offset_mask.shape[2]
    p_n = len(points(kh, kw, remove_center))
    om = offset_mask.to(dtype)
    rec = om[..., :group * p_n * 3].reshape(n, ho, wo, group, p_n * 3)
    cells = input.reshape(n, h * w, group, gc)
    xs, ys = coordinates(om, h, w, kh, kw, sh, sw, ph, pw, dh, dw, group, scale, remove_center)
    bi = torch.arange(n).view(n, 1, 1, 1).expand(n, ho, wo, group)
    gi = torch.arange(group).view(1, 1, 1, group).expand(n, ho, wo, group)
    out = input.new_zeros((n, ho, wo, group, gc))
    for p in range(p_n):
        x, y = xs[..., p], ys[..., p]
        ok = (x > -1) & (y > -1) & (x < w) & (y < h)                      # a NaN fails
        x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
        lx, ly = x - x0, y - y0
        hx, hy = 1 - lx, 1 - ly
        zero = torch.zeros_like(x)
        wts = [torch.where(ok, t, zero) for t in (hy * hx, hy * lx, ly * hx, ly * lx)]
        vals = []
        for dy, dx in CORNERS:
            yy, xx = y0 + dy, x0 + dx
            inn = ok & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
            cell = torch.where(inn, yy * w + xx, zero).long()
            v = cells[bi, cell, gi]
            vals.append(torch.where(inn[..., None], v, torch.zeros_like(v)))
        sample = ((wts[0][..., None] * vals[0] + wts[1][..., None] * vals[1]) + wts[2][..., None] * vals[2]) + wts[3][..., None] * vals[3]
        out = out + rec[..., 2 * p_n + p, None] * sample
    return out.view(n, ho, wo, group * gc)


def dcnv4_composition(input, offset_mask, kh, kw, sh, sw, ph, pw, dh, dw, group, gc, scale, remove_center):
    pts = points(kh, kw, remove_center)
    p = len(pts)
    off, msk, _ = unpack(offset_mask, group, p)
    x = torch.nn.functional.pad(input, [0, 0, pw, pw, ph, ph])
    n, hp, wp, _ = x.shape
    ho, wo = offset_mask.shape[1], offset_mask.shape[2]
    bx, by = (dw * (kw - 1)) // 2, (dh * (kh - 1)) // 2
    ar = lambda count: torch.arange(count, dtype=x.dtype)                  # noqa: E731
    ref_x = ((ar(wo) * sw + bx + 0.5) / wp).view(1, 1, wo, 1, 1)
    ref_y = ((ar(ho) * sh + by + 0.5) / hp).view(1, ho, 1, 1, 1)
    grid_x = torch.tensor([(i * dw - bx) / wp for i, j in pts], dtype=x.dtype).view(1, 1, 1, 1, p) * scale
    grid_y = torch.tensor([(j * dh - by) / hp for i, j in pts], dtype=x.dtype).view(1, 1, 1, 1, p) * scale
    o = off.reshape(n, ho, wo, group, p, 2)
    loc = torch.stack([ref_x + grid_x + o[..., 0] * scale / wp, ref_y + grid_y + o[..., 1] * scale / hp], -1)
    maps = x.reshape(n, hp * wp, group, gc).permute(0, 2, 3, 1).reshape(n * group, gc, hp, wp)
    grids = (2 * loc - 1).view(n, ho * wo, group, p, 2).transpose(1, 2).flatten(0, 1)
    sampled = torch.nn.functional.grid_sample(maps, grids, mode="bilinear", padding_mode="zeros", align_corners=False)
    weights = msk.reshape(n, ho * wo, group, p).transpose(1, 2).reshape(n * group, 1, ho * wo, p)
    out = (sampled * weights).sum(-1).view(n, group * gc, ho * wo)
    return out.transpose(1, 2).reshape(n, ho, wo, group * gc)


def with_gradients(fn, input, offset_mask, geom, grad):
    """(out, d_input, d_offset_mask) of a restatement, all in input's dtype."""
    x, om = (t.detach().clone().requires_grad_(True) for t in (input, offset_mask.to(input.dtype)))
    out = fn(x, om, *geom)
    out.backward(grad.to(input.dtype))
    return out.detach(), x.grad, om.grad


def parts(result, group, p):
    """(out, d_input, d_offset_mask) as (out, d_input, d_offset, d_mask) and the pad part of d_offset_mask."""
    out, dx, dom = result
    doff, dmask, dpad = unpack(dom, group, p)
    return (out, dx, doff, dmask), dpad


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def segment():
    """Entries of one piece of a long gather segment (frcnn_ops_msda_segment): the input gradient runs on that gather."""
    return nv.lib().frcnn_ops_msda_segment()


def block_items(gc, kh, kw, remove_center=False, elem=0):
    n = nv.lib().frcnn_ops_dcnv4_block_items(gc, kh, kw, int(remove_center), elem)
    assert n >= 1
    return n


# name: (N, H, W, G, Gc, kernel, stride, pad, dilation, offset_scale, remove_center, mode), pairs (h, w).  mode "spread": displacements of
# about 2 px, so that a share of the samples leaves the map; "one-cell": every sample inside cell (1, 1).
SPLIT_G, SPLIT_GC = 3, 8
CASES = {
    "base":      (2, 7, 9, 2, 8, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, False, "spread"),    # 3 G P = 54, L = 56: two pad lanes
    "rc3":       (2, 7, 9, 3, 8, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, True, "spread"),     # P = 8, 3 G P = L = 72: no pad lane
    "rc5":       (1, 6, 6, 1, 4, (5, 5), (1, 1), (2, 2), (1, 1), 0.5, True, "spread"),
    "pad7":      (1, 5, 6, 3, 4, (3, 3), (2, 1), (1, 1), (1, 2), 1.5, False, "spread"),    # 81 -> 88: seven pad lanes
    "even":      (1, 6, 8, 2, 8, (2, 4), (1, 2), (0, 2), (1, 1), 1.5, False, "spread"),
    "g5rc":      (1, 4, 5, 5, 2, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, True, "spread"),     # a G that does not divide a block's items
    "k1":        (1, 4, 5, 3, 4, (1, 1), (1, 1), (0, 0), (1, 1), 1.0, False, "spread"),    # 9 -> 16: the pad is longer than a group's data
    "gc3":       (1, 5, 6, 2, 3, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, True, "spread"),     # the scalar body, below a run; without the centre
    "gc70":      (1, 2, 3, 1, 70, (1, 3), (1, 1), (0, 1), (1, 1), 1.0, False, "spread"),   # the scalar body's second pass
    "gc72":      (1, 3, 3, 1, 72, (3, 1), (1, 1), (1, 0), (1, 1), 1.0, False, "spread"),   # 18 float32 runs (9 16-bit ones): idle lanes
    "gc256":     (1, 2, 3, 1, 256, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, False, "spread"),  # the most channels a group holds: 64 lanes
    "k7rc":      (1, 9, 9, 1, 4, (7, 7), (1, 1), (3, 3), (1, 1), 1.0, True, "spread"),     # P = 48: the LDS bound sets the items of a block
    "one-cell":  (2, 12, 12, 1, 4, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, False, "one-cell"),  # 1296 entries on each of four cells an image
    # sized from frcnn_ops_dcnv4_block_items when it is built (shape_of): two rows of just over a block's items / G pixels, G = 3
    "split":     (1, 2, None, SPLIT_G, SPLIT_GC, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, False, "spread"),
}


def shape_of(name):
    """CASES[name], the width of "split" filled in: a block's last item and the next block's first one share a pixel."""
    c = CASES[name]
    if name != "split":
        return c
    ipb = block_items(SPLIT_GC, 3, 3)
    assert ipb % SPLIT_G != 0
    return c[:2] + (ipb // SPLIT_G + 1,) + c[3:]


def points_of(name):
    c = CASES[name]
    return len(points(c[5][0], c[5][1], c[10]))


def geom_of(name):
    n, h, w, g, gc, kernel, stride, pad, dil, scale, rc, mode = CASES[name]
    return geometry(kernel, stride, pad, dil, g, gc, scale, rc)


@functools.lru_cache(maxsize=None)
def case(name):
    """(input, offset_mask, grad): input and grad float64 holding float32 values, offset_mask float32 with PAD_VALUE in its pad lanes.
    Checked: see the module docstring."""
    n, h, w, g, gc, kernel, stride, pad, dil, scale, rc, mode = shape_of(name)
    geom = geom_of(name)
    gen = torch.Generator().manual_seed(sum(ord(c) for c in name) * 7919)
    ho, wo = out_size(h, kernel[0], stride[0], pad[0], dil[0]), out_size(w, kernel[1], stride[1], pad[1], dil[1])
    p = points_of(name)
    input = torch.randn((n, h, w, g * gc), generator=gen, dtype=F32).to(F64)
    # where the undisplaced samples lie, then the wanted coordinates, then the offsets that give them
    gx, gy = coordinates(torch.zeros((n, ho, wo, record(g, p)), dtype=F64), h, w, *geom[:8], g, scale, rc)
    if mode == "one-cell":
        want = [torch.ones_like(gx), torch.ones_like(gy)]
    else:
        want = [torch.floor(c + 2.0 * torch.randn(c.shape, generator=gen, dtype=F64)) for c in (gx, gy)]
    want = [c + 0.08 + 0.84 * torch.rand(c.shape, generator=gen, dtype=F64) for c in want]
    off = torch.stack([(want[0] - gx) / scale, (want[1] - gy) / scale], -1).reshape(n, ho, wo, g * p * 2).to(F32)
    mask = torch.randn((n, ho, wo, g, p), generator=gen, dtype=F32)
    if mode == "one-cell":
        mask = torch.softmax(mask, -1)
    om = pack(off, mask.reshape(n, ho, wo, g * p), g, p, fill=PAD_VALUE)
    grad = torch.randn((n, ho, wo, g * gc), generator=gen, dtype=F32).to(F64)
    check_positions(om, name)
    return input, om, grad


def check_positions(offset_mask, name):
    """Every coordinate, as float64 and as float32 evaluate it, has its fractional part in [1/16, 15/16]."""
    n, h, w, g, gc, kernel, stride, pad, dil, scale, rc, mode = shape_of(name)
    for dtype in (F64, F32):
        for c in coordinates(offset_mask.to(dtype), h, w, *geom_of(name)[:8], g, scale, rc):
            frac = (c - torch.floor(c)).to(F64)
            assert bool(((frac >= 1 / 16) & (frac <= 15 / 16)).all()), name


def rel_err(a, truth):
    return float((a.to(F64) - truth).abs().max() / truth.abs().max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """((out, d_input, d_offset_mask) in float64, the same from the explicit restatement run in float32 on the CPU).  Computed once and
    shared: do not modify.  Asserts that the two float64 restatements agree on this case, part by part, and that the explicit one's
    gradient on the pad lanes is exactly 0."""
    input, om, grad = case(name)
    geom, g, p = geom_of(name), CASES[name][3], points_of(name)
    truth = with_gradients(dcnv4_explicit, input, om.to(F64), geom, grad)
    other = with_gradients(dcnv4_composition, input, om.to(F64), geom, grad)
    (tp, tpad), (op, opad) = parts(truth, g, p), parts(other, g, p)
    for i, (a, c) in enumerate(zip(tp, op)):
        assert a.shape == c.shape and a.dtype == F64
        assert rel_err(c, a) <= (1e-13 if i == 0 else 1e-12), (name, i, rel_err(c, a))
    assert not bool(tpad.any()) and not bool(opad.any()), name
    single = with_gradients(dcnv4_explicit, input.to(F32), om, geom, grad.to(F32))
    assert not bool(parts(single, g, p)[1].any()), name
    return truth, single
