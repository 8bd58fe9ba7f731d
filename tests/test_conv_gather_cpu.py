"""
tests/conv_gather_cases.py held to independent truth, without a GPU, so that tests/test_conv_gather_gpu.py does not rest on unchecked code:
  * the float64 references (F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight) against plain numpy tap loops;
  * the "exact" claim of the integer cases, on the data: references integral and below 2^24 with every partial sum bounded, operands
    unchanged by a round trip through bfloat16, float16 and the f32x3 split under the tensor's power-of-two scale;
  * the plan mirror against the library: frcnn_conv_workspace_bytes / frcnn_conv_dgrad_workspace_bytes over the table and a sweep;
  * the coverage the table claims (which tile, split and pipeline seam each kernel reaches), naming the cases;
  * the argument table of the entry points, which refuse bad arguments before touching the device.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from tests import conv_gather_cases as G
from fasterrcnn_amd import _native as nv

EINVAL, EUNSUPPORTED = -1, -4

needs_default_knobs = pytest.mark.skipif(any(os.environ.get(k) for k in G.KNOBS),
                                         reason="the plan mirror states the default plan: %s must be unset" % ", ".join(G.KNOBS))


# ---- references against plain tap loops -----------------------------------------------------------------------------------------------
def np_patch(c, xp, r, s):
    ho, wo = G.out_hw(c)
    return xp[:, r:r + (ho - 1) * c.stride + 1:c.stride, s:s + (wo - 1) * c.stride + 1:c.stride, :]


def np_forward(c, x, w, b):
    xp = np.zeros((c.N, c.H + 2 * c.pad, c.W + 2 * c.pad, c.cin))
    xp[:, c.pad:c.pad + c.H, c.pad:c.pad + c.W] = x
    ho, wo = G.out_hw(c)
    y = np.zeros((c.N, ho, wo, c.cout)) + b
    for r in range(c.k):
        for s in range(c.k):
            y += np_patch(c, xp, r, s) @ w[:, :, r, s].T
    return y


def np_dgrad(c, dz, w):
    dxp = np.zeros((c.N, c.H + 2 * c.pad, c.W + 2 * c.pad, c.cin))
    for r in range(c.k):
        for s in range(c.k):
            np_patch(c, dxp, r, s)[...] += dz @ w[:, :, r, s]
    return dxp[:, c.pad:c.pad + c.H, c.pad:c.pad + c.W]


def np_wgrad(c, x, dz):
    xp = np.zeros((c.N, c.H + 2 * c.pad, c.W + 2 * c.pad, c.cin))
    xp[:, c.pad:c.pad + c.H, c.pad:c.pad + c.W] = x
    return np.stack([np.einsum("nhwo,nhwi->oi", dz, np_patch(c, xp, t // c.k, t % c.k)) for t in range(c.k * c.k)])


SMALL = [c for c in G.CASES if c.N * c.H * c.W * c.cin <= 200000]


def test_the_small_cases_cover_every_geometry_family():
    names = {c.name for c in SMALL}
    assert {"k3p0s1", "k3p2s2_odd", "k1s3", "tiny1x1_p2", "k2", "k5", "k7_stem_like", "k3s4", "k1_p1", "k3_p3", "cin60", "cout132"} <= names


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_references_match_plain_tap_loops(c):
    o = {k: v.double().numpy() for k, v in G.operands(c).items()}
    ref = G.exact_references(c)
    if G.forward_ok(c):
        want = np_forward(c, o["x"], o["w"], o["b"])
        assert np.array_equal(ref["y_plain"].numpy(), want)
        assert np.array_equal(ref["y"].numpy(), np.maximum(want + o["res_y"], 0.0))
    if G.dgrad_ok(c):
        want = np_dgrad(c, o["dz"], o["w"])
        assert np.array_equal(ref["dx"].numpy(), want)
        assert np.array_equal(ref["dx_res"].numpy(), want + o["res_x"])
        untouched = G.untouched_dx_pixels(c)
        assert not want[:, untouched].any(), "a pixel no tap reads has a zero data gradient"
    if G.wgrad_ok(c):
        assert np.array_equal(ref["dw"].numpy(), np_wgrad(c, o["x"], o["dz"]))


def test_pack_layouts():
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3, 3)
    wp = G.pack(w)
    for t in range(9):
        assert torch.equal(wp[t], w[:, :, t // 3, t % 3])
        assert torch.equal(G.pack_dgrad(w)[t], w[:, :, t // 3, t % 3].T)
    assert torch.equal(G.unpack(wp, 3), w)


def test_gaussian_references_in_float32_are_float32_close():
    """the yardstick of the random-valued GPU cases is torch's own float32 convolution: it must be a float32-class distance from the truth"""
    for c in G.RANDOM_CASES:
        o = G.gaussian_operands(c)
        t = G.ref_forward(c, o["x"], o["w"], o["b"])
        e = float((G.ref_forward(c, o["x"], o["w"], o["b"], dtype=torch.float32).double() - t).abs().max() / t.abs().max())
        assert e <= 1e-5, (c.name, e)


# ---- "exact" rests on the data ------------------------------------------------------------------------------------------------------------
def x3_split_is_exact(t):
    """x3t.h hx_row_scale + conv_gather.hip gx_split4 on tensor t: hi = fp16(v 2^e) holds the value, lo = 0"""
    mx = float(t.abs().max())
    if mx == 0.0:
        return True
    e = 14 - int(np.floor(np.log2(mx)))
    assert 2.0 ** 14 <= mx * 2.0 ** e < 2.0 ** 15
    scaled = t * 2.0 ** e
    return torch.equal(scaled.to(torch.float16).to(torch.float32), scaled) and float(scaled.abs().max()) <= 65504.0


@pytest.mark.parametrize("c", G.CASES + G.IMPULSE_CASES, ids=lambda c: c.name)
def test_exact_cases_have_one_right_answer(c):
    o = G.operands(c)
    for name, t in o.items():
        assert t.dtype == torch.float32 and float(t.abs().max()) <= G.VMAX, name
        assert torch.equal(t, t.round()), name
        assert torch.equal(t.to(torch.bfloat16).to(torch.float32), t), name
        assert torch.equal(t.to(torch.float16).to(torch.float32), t), name
        assert x3_split_is_exact(t), name
    # every partial sum, in any order: the sum of the addends' magnitudes is below 2^24
    K, Kd, M = c.cin * c.k * c.k, c.cout * c.k * c.k, G.rows_forward(c)
    assert G.VMAX * G.VMAX * K + 2 * G.VMAX < G.EXACT_LIMIT and G.VMAX * G.VMAX * Kd + G.VMAX < G.EXACT_LIMIT
    if G.wgrad_ok(c):
        assert G.VMAX * G.VMAX * M < G.EXACT_LIMIT
    if c in G.IMPULSE_CASES:
        return
    refs = G.exact_references(c)
    assert set(refs) == ({"y", "y_plain"} if G.forward_ok(c) else set()) | ({"dx", "dx_res"} if G.dgrad_ok(c) else set()) | \
        ({"dw"} if G.wgrad_ok(c) else set())
    for name, t in refs.items():
        assert t.dtype == torch.float64
        assert torch.equal(t, t.round()) and float(t.abs().max()) < G.EXACT_LIMIT, name
        assert torch.equal(t.to(torch.float32).double(), t), name
    if G.forward_ok(c):
        assert float(refs["y"].max()) > 0 and float(refs["y_plain"].min()) < 0, "the ReLU has something to cut"


def test_impulse_positions_and_weights():
    for c in G.IMPULSE_CASES:
        ho, wo = G.out_hw(c)
        for n, h, w in ((c.N, c.H, c.W), (c.N, ho, wo)):
            pos = G.impulse_positions(n, h, w)
            assert (0, 0, 0) in pos and (n - 1, h - 1, w - 1) in pos and (0, h - 1, w - 1) in pos and (1, 0, 0) in pos
            flat = {(i * h + y) * w + x for i, y, x in pos}
            assert {m for m in (63, 64, 127, 128) if m < n * h * w} <= flat
            assert all(0 <= i < n and 0 <= y < h and 0 <= x < w for i, y, x in pos)
        wt = G.impulse_weights(c)
        assert sorted(set(wt[0, 0].flatten().tolist())) == [float(t + 1) for t in range(c.k * c.k)]
        assert int((wt != 0).sum()) == 4 * c.k * c.k


# ---- the mirror is the library's plan -----------------------------------------------------------------------------------------------------
def sweep_shapes():
    rnd = random.Random(20240611)
    shapes = []
    for _ in range(400):
        k = rnd.choice((1, 1, 2, 3, 3, 3, 5, 7))
        shapes.append((rnd.choice((1, 1, 2, 3, 8, 64, 300)), rnd.randint(1, 80), rnd.randint(1, 130), 16 * rnd.randint(1, 64),
                       rnd.choice((4, 16, 32, 60, 64, 68, 128, 256, 512, 1024)), k, rnd.choice((1, 1, 2, 3)), rnd.randint(0, k)))
    # the sizes the backbones run (models/resnet.py: 600 x 1000 images, per-RoI maps of the head)
    shapes += [(1, 150, 250, 64, 256, 1, 1, 0), (1, 150, 250, 256, 64, 1, 1, 0), (1, 75, 125, 512, 128, 1, 1, 0), (1, 75, 125, 128, 128, 3, 2, 1),
               (1, 38, 63, 1024, 256, 1, 1, 0), (1, 38, 63, 256, 256, 3, 1, 1), (8, 75, 125, 512, 128, 1, 1, 0), (300, 7, 7, 512, 512, 3, 1, 1),
               (300, 14, 14, 1024, 512, 1, 2, 0), (128, 4, 4, 64, 256, 1, 1, 0), (2, 600, 1000, 64, 64, 1, 1, 0)]
    return shapes


@needs_default_knobs
def test_workspace_sizes_are_the_mirrors():
    lib = nv.lib()
    shapes = [tuple(c[1:]) for c in G.CASES] + sweep_shapes()
    assert len(shapes) >= 400
    split_f, split_d = 0, 0
    for s in shapes:
        want_f, want_d = G.conv_workspace_bytes(*s), G.dgrad_workspace_bytes(*s)
        assert int(lib.frcnn_conv_workspace_bytes(*s)) == want_f, s
        assert int(lib.frcnn_conv_dgrad_workspace_bytes(*s)) == want_d, s
        split_f += want_f > 0
        split_d += want_d > 0
    assert split_f >= 100 and split_d >= 100 and split_f <= len(shapes) - 50, "the sweep sees split and un-split plans"


@needs_default_knobs
def test_workspace_of_a_case_is_the_larger_plan():
    for c in G.CASES:
        fp, dp = G.forward_plans(c), G.dgrad_plans(c)
        if fp:
            M = G.rows_forward(c)
            assert max(p.splits for p in fp.values()) * M * c.cout * 4 <= max(G.conv_workspace_bytes(*c[1:]), M * c.cout * 4), c.name
        if dp:
            M = c.N * c.H * c.W
            assert max(p.splits for p in dp.values()) * M * c.cin * 4 <= max(G.dgrad_workspace_bytes(*c[1:]), M * c.cin * 4), c.name


# ---- what the table reaches -----------------------------------------------------------------------------------------------------------------
def launches():
    """(case name, 'fwd' / 'dgrad', arithmetic, Plan) of every launch of the exact cases with the full workspace"""
    out = []
    for c in G.CASES:
        out += [(c.name, "fwd", a, p) for a, p in G.forward_plans(c).items()]
        out += [(c.name, "dgrad", a, p) for a, p in G.dgrad_plans(c).items()]
    return out


def reached(what, pred):
    names = sorted({"%s/%s/%s" % (n, d, a) for n, d, a, p in launches() if pred(n, d, a, p)})
    print("%-64s %s" % (what, ", ".join(names[:4]) + (" ... (%d)" % len(names) if len(names) > 4 else "")))
    assert names, what
    return names


@needs_default_knobs
def test_the_table_reaches_the_float32_plan_seams():
    for kernel in ("f32", "bf16"):           # conv_gather_mfma_kernel, conv_gather_bf16_kernel
        for d in ("fwd", "dgrad"):
            for cfg in (0, 1):
                reached("%s %s cfg %d un-split" % (kernel, d, cfg), lambda n, dd, a, p: p.kernel == kernel and dd == d and p.cfg == cfg and p.splits == 1)
                reached("%s %s cfg %d split" % (kernel, d, cfg), lambda n, dd, a, p: p.kernel == kernel and dd == d and p.cfg == cfg and p.splits > 1)
            reached("%s %s last split shorter" % (kernel, d),
                    lambda n, dd, a, p: p.kernel == kernel and dd == d and p.splits > 1 and G.last_part(p) < p.sps)
            reached("%s %s more than one row block and column block" % (kernel, d),
                    lambda n, dd, a, p: p.kernel == kernel and dd == d and p.mblocks > 1 and p.nblocks > 1)
    for bm, cfg in ((128, 0), (256, 1)):
        for M in (bm - 1, bm, bm + 1):
            reached("f32 cfg %d rows %d" % (cfg, M), lambda n, dd, a, p: p.kernel == "f32" and p.cfg == cfg and p.M == M)
    reached("f32 single-stage reduction", lambda n, dd, a, p: p.kernel == "f32" and p.stages == 1)


@needs_default_knobs
def test_the_table_reaches_the_pipelined_plan_seams():
    x3 = lambda p: p.kernel == "x3"                                                                       # noqa: E731
    for a in ("x3g", "bf16"):
        for cfg in (0, 2, 3):
            reached("x3 %s cfg %d un-split" % (a, cfg), lambda n, d, aa, p: x3(p) and aa == a and d == "fwd" and p.cfg == cfg and p.splits == 1)
            reached("x3 %s cfg %d split" % (a, cfg), lambda n, d, aa, p: x3(p) and aa == a and d == "fwd" and p.cfg == cfg and p.splits > 1)
            # a split whose last part is shorter than the pipeline is deep (D = 3 at cfg 3, 2 at the 128-row tiles)
            reached("x3 %s cfg %d last part shorter than D" % (a, cfg),
                    lambda n, d, aa, p: x3(p) and aa == a and p.cfg == cfg and p.splits > 1 and G.last_part(p) < p.depth)
    for mb in (1, 7, 8, 9):
        reached("x3 fwd %d row blocks of 64" % mb, lambda n, d, a, p: x3(p) and d == "fwd" and p.cfg == 3 and p.mblocks == mb)
    reached("x3 more than 8 row blocks of 128", lambda n, d, a, p: x3(p) and p.cfg in (0, 2) and p.mblocks > 8 and p.mblocks % 8 != 0)
    reached("x3 column blocks > 1", lambda n, d, a, p: x3(p) and p.nblocks > 1)
    reached("x3 row blocks > 8 and column blocks > 1", lambda n, d, a, p: x3(p) and p.nblocks > 1 and p.mblocks > 8)
    for st in (1, 2, 3, 4):
        reached("x3 cfg 3 (D = 3) total stages %d" % st, lambda n, d, a, p: x3(p) and p.cfg == 3 and p.stages == st and p.splits == 1)
    for st in (1, 2, 3):
        reached("x3 128-row tile (D = 2) stages in a part %d" % st,
                lambda n, d, a, p: x3(p) and p.cfg in (0, 2) and (p.sps == st or G.last_part(p) == st))
    for M in (63, 64, 65):
        reached("x3 cfg 3 rows %d" % M, lambda n, d, a, p: x3(p) and p.cfg == 3 and p.M == M)
    for cfg in (0, 2):
        for rem in (1, 127):
            reached("x3 cfg %d last tile of %d rows" % (cfg, rem), lambda n, d, a, p: x3(p) and p.cfg == cfg and p.M % 128 == rem)
    # the data-gradient form of the pipelined kernel at each effective padding, split and un-split
    for pad_e in (0, 1, 2):
        reached("x3 dgrad pad_e %d" % pad_e, lambda n, d, a, p: x3(p) and d == "dgrad" and G.BY_NAME[n].k == 3 and G.dgrad_pad_e(G.BY_NAME[n]) == pad_e)
        reached("x3 fwd 3x3 pad %d stride 1" % pad_e, lambda n, d, a, p: x3(p) and d == "fwd" and G.BY_NAME[n][6:] == (3, 1, pad_e))
        reached("x3 fwd 3x3 pad %d stride 2" % pad_e, lambda n, d, a, p: x3(p) and d == "fwd" and G.BY_NAME[n][6:] == (3, 2, pad_e))
    reached("x3 dgrad split", lambda n, d, a, p: x3(p) and d == "dgrad" and p.splits > 1)
    reached("x3 dgrad 1x1", lambda n, d, a, p: x3(p) and d == "dgrad" and G.BY_NAME[n].k == 1)
    reached("x3 row decode beyond 2^17", lambda n, d, a, p: x3(p) and p.M > (1 << 17))
    # the in-kernel finish is taken on a split plan, and refused by a plan that does not split
    reached("x3g ticket finish", lambda n, d, a, p: a == "x3g" and G.ticket_finish(p))
    reached("x3g tickets without a split", lambda n, d, a, p: a == "x3g" and not G.ticket_finish(p))


def test_the_table_reaches_the_geometry_the_issue_lists():
    cs = G.CASES
    fwd_x3 = [c for c in cs if G.forward_takes_x3(c)]
    generic = [c for c in cs if G.forward_ok(c) and not G.forward_takes_x3(c)]
    assert {(c.k, c.stride, c.pad) for c in fwd_x3} >= {(3, s, p) for s in (1, 2) for p in (0, 1, 2)} | {(1, 1, 0), (1, 2, 0), (1, 3, 0)}
    assert {(c.H, c.W, c.pad) for c in fwd_x3 if c.k == 3} >= {(h, w, p) for h, w in ((1, 1), (1, 2), (2, 2), (2, 5)) for p in (1, 2)}
    assert {(c.H + 2 * c.pad - c.k) % 2 for c in fwd_x3 if c.stride == 2 and c.k == 3} == {0, 1}
    assert {c.k for c in generic} >= {2, 5, 7} and {c.stride for c in generic} >= {3} and {c.cin for c in generic} >= {16, 48}
    assert any(c.k == 3 and c.stride == 4 for c in cs) and any(c.k == 1 and c.pad == 1 for c in generic) and any(c.k == 3 and c.pad == 3 for c in generic)
    assert all(c in generic for c in G.GENERIC_GEOMETRY) and all(c in generic for c in G.RANDOM_CASES)
    assert {(c.k, c.stride) for c in fwd_x3} >= {(3, 3), (3, 4)}, "the pipelined kernel takes any forward stride"
    assert {c.cout for c in cs if G.forward_ok(c)} >= {4, 60, 64, 68, 128, 132} and {c.cin for c in cs if G.dgrad_ok(c)} >= {4, 60, 64, 68, 128, 132}
    # the data gradient of every forward case that has one, with pixels no tap reads among them
    assert all(G.dgrad_plans(c) for c in cs if G.forward_ok(c) and c.cout % 16 == 0)
    holes = [c.name for c in cs if G.dgrad_ok(c) and G.untouched_dx_pixels(c).any()]
    assert {"k3s4", "k1s2", "k1s3", "k3p0s2_even"} <= set(holes), holes
    assert any(G.dgrad_ok(c) and (c.H + 2 * c.pad - c.k) % c.stride != 0 and c.stride == 3 for c in cs)
    many = G.BY_NAME["many_tiny_maps"]
    assert 20e6 <= many.N * many.H * many.W * many.cin * 4 <= 30e6 and (many.H, many.W, many.cin, many.cout) == (3, 3, 32, 4)
    big = [c.name for c in cs if c.N * c.H * c.W * c.cin * 4 > 8e6]
    assert big == ["many_tiny_maps"], big


# ---- arguments refused before the device is touched -----------------------------------------------------------------------------------------
def test_conv_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = nv.lib()
    raw = (C.c_float * 96)()
    x = (C.addressof(raw) + 63) & ~63              # a 64-byte aligned host address; none of these calls may read or write it
    big = C.c_size_t(1 << 30)

    def fwd(N=1, H=8, W=8, cin=32, cout=32, k=3, stride=1, pad=1):
        """every forward entry point's answer to the shape (x3g: with both maxima)"""
        a = (N, H, W, cin, cout, k, stride, pad, 0)
        return {"nhwc": lib.frcnn_conv_nhwc(x, x, x, None, x, *a, x, big, None),
                "math0": lib.frcnn_conv_nhwc_math(x, x, x, None, x, *a, 0, x, big, None),
                "math1": lib.frcnn_conv_nhwc_math(x, x, x, None, x, *a, 1, x, big, None),
                "x3g": lib.frcnn_conv_nhwc_x3g(x, x, x, None, x, *a, x, x, x, x, big, None),
                "tickets": lib.frcnn_conv_nhwc_x3g_tickets(x, x, x, None, x, *a, x, x, x, x, big, x, None)}

    def all_einval(**kw):
        got = fwd(**kw)
        assert set(got.values()) == {EINVAL}, (kw, got)
    all_einval(cin=24)                       # cin % 16 != 0
    all_einval(cin=0 + 8)
    all_einval(cout=30)                      # cout % 4 != 0
    all_einval(k=0)
    all_einval(stride=0)
    all_einval(N=0)
    all_einval(pad=-1)
    all_einval(H=2, pad=0)                   # H + 2 pad < R
    all_einval(W=1, k=5, pad=1)
    all_einval(H=4, W=4, k=7, pad=1, cin=16)
    a = (1, 8, 8, 32, 32, 3, 1, 1, 0)
    assert lib.frcnn_conv_nhwc_math(x, x, x, None, x, *a, 7, x, big, None) == EINVAL                     # math 7
    assert lib.frcnn_conv_nhwc_math(x, x, x, None, x, *a, -1, x, big, None) == EINVAL
    assert lib.frcnn_conv_nhwc_math(x, x, x, None, x, *a, 2, x, big, None) == EINVAL                     # (the x3g arithmetic has its own entry point)
    assert lib.frcnn_conv_nhwc_x3g(x, x, x, None, x, *a, None, x, x, x, big, None) == EINVAL             # a missing maximum
    assert lib.frcnn_conv_nhwc_x3g(x, x, x, None, x, *a, x, None, x, x, big, None) == EINVAL
    assert lib.frcnn_conv_nhwc_x3g_tickets(x, x, x, None, x, *a, x, None, x, x, big, x, None) == EINVAL
    assert lib.frcnn_conv_nhwc_x3g_tickets(x, x, x, None, x, *a, x, x, x, x, big, None, None) == EINVAL  # a missing ticket array
    assert lib.frcnn_conv_nhwc(None, x, x, None, x, *a, x, big, None) == EINVAL
    assert lib.frcnn_conv_nhwc(x, x, None, None, x, *a, x, big, None) == EINVAL

    def x3g_unsupported(**kw):
        got = fwd(**kw)
        assert got["x3g"] == EUNSUPPORTED and got["tickets"] == EUNSUPPORTED, (kw, got)
    x3g_unsupported(k=5, pad=2)
    x3g_unsupported(cin=48)
    x3g_unsupported(k=3, pad=3)              # pad = R
    x3g_unsupported(k=1, pad=1)
    x3g_unsupported(k=2, pad=0)
    x3g_unsupported(k=7, pad=3, cin=64)
    for c in G.GENERIC_GEOMETRY:
        if G.forward_ok(c) and not G.forward_takes_x3(c):
            x3g_unsupported(N=c.N, H=c.H, W=c.W, cin=c.cin, cout=c.cout, k=c.k, stride=c.stride, pad=c.pad)

    def dgrad(N=1, H=8, W=8, cin=32, cout=32, k=3, stride=1, pad=1):
        a = (N, H, W, cin, cout, k, stride, pad)
        return {lib.frcnn_conv_dgrad(x, x, None, x, *a, x, big, None), lib.frcnn_conv_dgrad_math(x, x, None, x, *a, 0, x, big, None),
                lib.frcnn_conv_dgrad_math(x, x, None, x, *a, 1, x, big, None)}
    assert dgrad(cout=24) == {EINVAL}        # cout % 16 != 0
    assert dgrad(cout=8) == {EINVAL}
    assert dgrad(cin=30) == {EINVAL}         # cin % 4 != 0
    assert dgrad(H=2, pad=0) == {EINVAL}     # H + 2 pad < R
    assert dgrad(W=1, k=5, pad=1) == {EINVAL}
    assert dgrad(k=0) == {EINVAL} and dgrad(stride=0) == {EINVAL} and dgrad(N=0) == {EINVAL} and dgrad(pad=-1) == {EINVAL}
    a = (1, 8, 8, 32, 32, 3, 1, 1)
    assert lib.frcnn_conv_dgrad_math(x, x, None, x, *a, 7, x, big, None) == EINVAL
    assert lib.frcnn_conv_dgrad_math(x, x, None, x, *a, 2, x, big, None) == EINVAL
    assert lib.frcnn_conv_dgrad(None, x, None, x, *a, x, big, None) == EINVAL

    def wgrad(N=1, H=8, W=8, cin=32, cout=32, k=3, stride=1, pad=1):
        a = (N, H, W, cin, cout, k, stride, pad)
        return {lib.frcnn_conv_wgrad(x, x, x, *a, x, big, None), lib.frcnn_conv_wgrad_math(x, x, x, *a, 0, x, big, None),
                lib.frcnn_conv_wgrad_math(x, x, x, *a, 1, x, big, None)}
    assert wgrad(cin=30) == {EINVAL} and wgrad(cout=30) == {EINVAL} and wgrad(k=0) == {EINVAL} and wgrad(k=8, pad=4) == {EINVAL}
    assert wgrad(H=2, pad=0) == {EINVAL} and wgrad(stride=0) == {EINVAL} and wgrad(N=0) == {EINVAL} and wgrad(pad=-1) == {EINVAL}
    assert lib.frcnn_conv_wgrad(x + 4, x, x, *a, x, big, None) == EINVAL                                # operands 16-byte aligned

    # an output of size zero needs no workspace
    assert lib.frcnn_conv_workspace_bytes(1, 2, 8, 512, 64, 3, 1, 0) == 0
    assert lib.frcnn_conv_workspace_bytes(1, 8, 1, 512, 64, 5, 1, 1) == 0
    assert lib.frcnn_conv_workspace_bytes(1, 8, 8, 24, 64, 3, 1, 1) == 0 and lib.frcnn_conv_workspace_bytes(1, 8, 8, 512, 30, 3, 1, 1) == 0
    assert lib.frcnn_conv_wgrad_workspace_bytes(1, 2, 8, 512, 64, 3, 1, 0) == 0
    assert lib.frcnn_conv_dgrad_workspace_bytes(0, 8, 8, 64, 512, 3, 1, 1) == 0
    assert lib.frcnn_conv_dgrad_workspace_bytes(1, 0, 8, 64, 512, 3, 1, 1) == 0
    assert lib.frcnn_conv_dgrad_workspace_bytes(1, 8, 8, 64, 24, 3, 1, 1) == 0
    assert lib.frcnn_conv_workspace_bytes(1, 7, 7, 512, 64, 3, 1, 1) > 0 and lib.frcnn_conv_dgrad_workspace_bytes(1, 7, 7, 64, 512, 3, 1, 1) > 0
