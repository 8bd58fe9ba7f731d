"""Multi-scale deformable attention (fasterrcnn_amd.ops.multi_scale_deformable_attn) restated twice in float64, and the named, seeded
cases the CPU and GPU tests share.

  msda_grid_sample   the composition users know: one F.grid_sample(align_corners=False, zero padding) per level, the weighted sum over
                     (l, p), torch.autograd for the three gradients.
  msda_explicit      the formula of include/frcnn_hip.h written out: a loop over levels, points and corners; x = loc_x W - 0.5, the
                     "x > -1 and x < W" test, the four corners with their weights, cells start + yy W + xx checked against [0, S), and the
                     published gradients (no autograd).  It runs in any dtype: in float64 it is the truth, in float32 on the CPU it
                     measures the error a float32 evaluation makes (err_ref of the GPU tests).

Every case is checked here, when it is first built: the two restatements agree (forward 1e-13, gradients 1e-12 relative to the largest
entry), and the position of every sample is controlled.  Cases are built from PIXEL coordinates, loc = float32((x + 0.5) / W): the
coordinate the kernels recover, fmaf(loc, W, -0.5), then has its fractional part in [1/16, 15/16] and lies no nearer than 1/16 to -1 or
to the size, because d_loc is discontinuous at integer coordinates and the sample test flips at -1 and at the size.
"""
import functools

import torch

from fasterrcnn_amd import _native as nv

F32, F64 = torch.float32, torch.float64
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))


def levels_of(shapes):
    """(int64 [L, 2], int64 [L]) for a list of (H, W): the levels packed one after another."""
    starts, s = [], 0
    for h, w in shapes:
        starts.append(s)
        s += h * w
    return torch.tensor(shapes, dtype=torch.int64).view(-1, 2), torch.tensor(starts, dtype=torch.int64)


# ---- the two restatements -------------------------------------------------------------------------------------------------------------
def msda_grid_sample(value, shapes, loc, attn):
    """[B, Q, M * D]; value [B, S, M, D] with S the sum of H W; shapes a list of (H, W)."""
    b, _, m, d = value.shape
    q, levels, points = loc.shape[1], loc.shape[3], loc.shape[4]
    out = value.new_zeros((b, m, d, q))
    start = 0
    for l, (h, w) in enumerate(shapes):
        v = value[:, start:start + h * w].permute(0, 2, 3, 1).reshape(b * m, d, h, w)
        grid = (2 * loc[:, :, :, l] - 1).permute(0, 2, 1, 3, 4).reshape(b * m, q, points, 2)
        sampled = torch.nn.functional.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [B M, D, Q, P]
        a = attn[:, :, :, l].permute(0, 2, 1, 3).reshape(b * m, 1, q, points)
        out = out + (sampled * a).sum(-1).view(b, m, d, q)
        start += h * w
    return out.permute(0, 3, 1, 2).reshape(b, q, m * d)


def grid_sample_gradients(value, shapes, loc, attn, grad):
    v, lo, a = (t.detach().clone().requires_grad_(True) for t in (value, loc, attn))
    msda_grid_sample(v, shapes, lo, a).backward(grad)
    return v.grad, lo.grad, a.grad


def msda_explicit(value, shapes, starts, loc, attn, grad=None):
    """(out, d_value, d_loc, d_attn) in value's dtype (the gradients None without grad); shapes and starts lists of ints.  S is
    whatever value holds: a corner whose cell falls outside [0, S) counts 0 and receives nothing."""
    dtype = value.dtype
    b, s, m, d = value.shape
    q, levels, points = loc.shape[1], loc.shape[3], loc.shape[4]
    loc, attn = loc.to(dtype), attn.to(dtype)
    out = value.new_zeros((b, q, m, d))
    g = None if grad is None else grad.to(dtype).view(b, q, m, d)
    dv, dloc, dattn = (None, None, None) if g is None else (torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(attn))
    bi = torch.arange(b).view(b, 1, 1).expand(b, q, m)
    mi = torch.arange(m).view(1, 1, m).expand(b, q, m)
    for l, ((h, w), start) in enumerate(zip(shapes, starts)):
        for p in range(points):
            x = loc[:, :, :, l, p, 0] * w - 0.5
            y = loc[:, :, :, l, p, 1] * h - 0.5
            ok = (x > -1) & (y > -1) & (x < w) & (y < h)                  # a NaN fails
            x0, y0 = torch.floor(x), torch.floor(y)
            lx, ly = x - x0, y - y0
            hx, hy = 1 - lx, 1 - ly
            wts = (hy * hx, hy * lx, ly * hx, ly * lx)
            aw = attn[:, :, :, l, p]
            vals, cells, inside = [], [], []
            for dy, dx in CORNERS:
                yy, xx = y0 + dy, x0 + dx
                inn = ok & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
                cell = torch.where(inn, start + yy * w + xx, torch.zeros_like(x)).long()
                inn = inn & (cell >= 0) & (cell < s)
                cell = torch.where(inn, cell, torch.zeros_like(cell))
                v = value[bi, cell, mi] if s > 0 else value.new_zeros((b, q, m, d))
                vals.append(torch.where(inn[..., None], v, torch.zeros_like(v)))
                cells.append(cell)
                inside.append(inn)
            zero = torch.zeros_like(x)
            wts = tuple(torch.where(ok, t, zero) for t in wts)
            sample = wts[0][..., None] * vals[0] + wts[1][..., None] * vals[1] + wts[2][..., None] * vals[2] + wts[3][..., None] * vals[3]
            out = out + aw[..., None] * sample
            if g is None:
                continue
            dattn[:, :, :, l, p] = (g * sample).sum(-1)
            hx_, lx_, hy_, ly_ = (torch.where(ok, t, zero)[..., None] for t in (hx, lx, hy, ly))
            slope_x = (hy_ * vals[1] - hy_ * vals[0]) + (ly_ * vals[3] - ly_ * vals[2])
            slope_y = (hx_ * vals[2] - hx_ * vals[0]) + (lx_ * vals[3] - lx_ * vals[1])
            ga = g * aw[..., None]
            dloc[:, :, :, l, p, 0] = w * (ga * slope_x).sum(-1)
            dloc[:, :, :, l, p, 1] = h * (ga * slope_y).sum(-1)
            for k in range(4):
                contrib = torch.where(inside[k][..., None], (wts[k] * aw)[..., None] * g, torch.zeros_like(g))
                dv.index_put_((bi, cells[k], mi), contrib, accumulate=True)
    return out.view(b, q, m * d), dv, dloc, dattn


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def block_items(d, levels, points, elem=0):
    """(b, q, m) items one block of the forward kernel serves (frcnn_ops_msda_block_items)."""
    n = nv.lib().frcnn_ops_msda_block_items(d, levels, points, elem)
    assert n >= 1
    return n


# name: (B, Q, M, D, [(H, W)...], P, mode).  Q None: one more item than a block serves (M = 1, B = 1).  mode "spread": integer parts
# from -3 to size + 1, so that a share of the samples lies outside on each side; "one-cell": every sample inside cell (1, 1) of level 0.
CASES = {
    "base":        (2, 9, 3, 5, [(4, 5), (3, 3), (2, 7)], 4, "spread"),            # the case of the self-check: odd W, D below the run
    "d1-block":    (1, None, 1, 1, [(3, 5)], 1, "spread"),                         # D = P = L = M = 1; one item more than a block's
    "d32-levels":  (2, 7, 3, 32, [(3, 5), (2, 3), (1, 2), (1, 1)], 2, "spread"),   # L = 4 with a 1 x 2 and a 1 x 1 level; M = 3
    "d72":         (1, 5, 2, 72, [(3, 4), (2, 3)], 3, "spread"),                   # one run above a wave's 64 float32 channels of 16-bit runs
    "d70-scalar":  (1, 3, 1, 70, [(2, 3)], 2, "spread"),                           # no whole runs and D > 64: a lane's second pass
    "chunks":      (3, 4, 2, 8, [(2, 3), (1, 3)], 2, "spread"),                    # B above the tests' im2col_step of 2 (and not a multiple)
    "one-cell":    (2, 321, 1, 4, [(3, 3)], 4, "one-cell"),                        # 1284 entries on each of four cells an image: long segments
}


def segment():
    """Entries of one piece of a long d_value segment (frcnn_ops_msda_segment): "one-cell" holds segments of more than two pieces, and
    a number of entries per image that is no multiple of it, so an image's pieces sit elsewhere in the sorted plan when the images
    are chunked otherwise."""
    return nv.lib().frcnn_ops_msda_segment()


def _pixel_coordinates(gen, shape, size, mode):
    if mode == "one-cell":
        k = torch.ones(shape, dtype=F64)
    else:
        k = torch.randint(-3, size + 2, shape, generator=gen).to(F64)
        inside = torch.rand(shape, generator=gen, dtype=F64) < 0.7             # most samples inside, the rest anywhere in [-3, size + 2)
        k = torch.where(inside, torch.randint(-1, size, shape, generator=gen).to(F64), k)
    frac = 0.08 + 0.84 * torch.rand(shape, generator=gen, dtype=F64)
    return k + frac


@functools.lru_cache(maxsize=None)
def case(name):
    """(value, shapes, starts, loc, attn, grad): value, attn and grad float64 holding float32 values, loc float32, shapes / starts
    lists of ints.  Checked: see the module docstring."""
    b, q, m, d, shapes, points, mode = CASES[name]
    if q is None:
        q = block_items(d, len(shapes), points) + 1
    gen = torch.Generator().manual_seed(sum(ord(c) for c in name) * 7919)
    s = sum(h * w for h, w in shapes)
    starts = [sum(h * w for h, w in shapes[:l]) for l in range(len(shapes))]
    value = torch.randn((b, s, m, d), generator=gen, dtype=F32).to(F64)
    loc = torch.empty((b, q, m, len(shapes), points, 2), dtype=F32)
    for l, (h, w) in enumerate(shapes):
        loc[:, :, :, l, :, 0] = ((_pixel_coordinates(gen, (b, q, m, points), w, mode) + 0.5) / w).to(F32)
        loc[:, :, :, l, :, 1] = ((_pixel_coordinates(gen, (b, q, m, points), h, mode) + 0.5) / h).to(F32)
    attn = torch.softmax(torch.randn((b, q, m, len(shapes) * points), generator=gen, dtype=F32), -1).view(b, q, m, len(shapes), points)
    grad = torch.randn((b, q, m * d), generator=gen, dtype=F32).to(F64)
    check_positions(loc, shapes)
    return value, shapes, starts, loc, attn.to(F64), grad


def check_positions(loc, shapes):
    """Every coordinate the kernels recover has its fractional part in [1/16, 15/16] and keeps 1/16 from -1 and from the size."""
    for l, (h, w) in enumerate(shapes):
        for axis, size in ((0, w), (1, h)):
            for c in (loc[:, :, :, l, :, axis].to(F64) * size - 0.5,                                # the truth's coordinate
                      (loc[:, :, :, l, :, axis] * float(size) - 0.5).to(F64)):                  # the same in float32
                frac = c - torch.floor(c)
                assert bool(((frac >= 1 / 16) & (frac <= 15 / 16)).all()), (l, axis)
                assert bool(((c + 1).abs() >= 1 / 16).all()) and bool(((c - size).abs() >= 1 / 16).all()), (l, axis)


def rel_err(a, truth):
    return float((a.to(F64) - truth).abs().max() / truth.abs().max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """((out, d_value, d_loc, d_attn) in float64, the same from the explicit restatement run in float32 on the CPU).  Computed once and
    shared; asserts that the two float64 restatements agree on this case."""
    value, shapes, starts, loc, attn, grad = case(name)
    truth = msda_explicit(value, shapes, starts, loc.to(F64), attn, grad)
    other = (msda_grid_sample(value, shapes, loc.to(F64), attn),) + grid_sample_gradients(value, shapes, loc.to(F64), attn, grad)
    for i, (a, c) in enumerate(zip(truth, other)):
        assert a.shape == c.shape and a.dtype == F64
        assert rel_err(c, a) <= (1e-13 if i == 0 else 1e-12), (name, i, rel_err(c, a))
    single = msda_explicit(value.to(F32), shapes, starts, loc, attn.to(F32), grad.to(F32))
    return truth, single


def hand_example():
    """One 2 x 2 level holding 1, 2, 3, 4; one query with two points: the map's centre (x = y = 0.5: the mean 2.5) with weight 0.5 and
    the centre of cell (0, 1) (x = 1, y = 0: the value 2) with weight 2.  out = 0.5 * 2.5 + 2 * 2 = 5.25."""
    value = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=F64).view(1, 4, 1, 1)
    loc = torch.tensor([[0.5, 0.5], [0.75, 0.25]], dtype=F64).view(1, 1, 1, 1, 2, 2)
    attn = torch.tensor([0.5, 2.0], dtype=F64).view(1, 1, 1, 1, 2)
    return value, [(2, 2)], [0], loc, attn, torch.tensor([[[5.25]]], dtype=F64)
