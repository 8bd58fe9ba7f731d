"""
The gather convolutions (csrc/conv_gather.hip: conv_gather_mfma_kernel, conv_gather_bf16_kernel, conv_gather_x3_kernel in the forward and
the data-gradient form) and the weight gradient beside them (csrc/gemm_tn.hip launch_conv_wgrad), through the C ABI, at the padding, tap
and plan seams of tests/conv_gather_cases.py (tests/test_conv_gather_cpu.py states which seam each case reaches and holds the references
to independent truth).

Exact cases: integer operands with one right answer in float32, bfloat16 and f32x3 arithmetic alike -- every entry point must return the
float64 reference to the bit, with the workspace the library asks for and with none (the un-split path of the same shape).
Guard bands: every input sits in the middle of a larger allocation filled with NaN (a masked tap that fetched memory in front of or
behind the tensor poisons the output; all of it is allocated, nothing can fault), every output and workspace sits between sentinels and
is NaN before the call.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_gather_cases as G
from fasterrcnn_amd import _native as nv

DEV = "cuda"
F32, BF16 = 0, 1
EUNSUPPORTED = -4
SENTINEL = -24680.0
NAN = float("nan")


def S():
    return nv.stream_ptr()


def margin_of(w, ch):
    """floats of guard band on each side: at least (2 W + 2) C (what a 3x3 tap at padding 2 could reach), a multiple of 64"""
    return ((2 * w + 2) * ch + 1024 + 63) // 64 * 64


class Guarded:
    """a tensor in the middle of a larger allocation: `t` is the view the kernel gets"""

    def __init__(self, shape, margin, band, inside):
        n = int(np.prod(shape))
        self.margin, self.n, self.band = margin, n, band
        self.buf = torch.full((2 * margin + n,), band, device=DEV)
        self.t = self.buf[margin:margin + n].view(shape)
        if isinstance(inside, torch.Tensor):
            self.t.copy_(inside)
        else:
            self.t.fill_(inside)

    def check(self, what):
        """an output after the call: written everywhere, nothing written around it"""
        assert not bool(torch.isnan(self.t).any()), "%s: an element was not written (or a NaN was fetched)" % what
        lo, hi = self.buf[:self.margin], self.buf[self.margin + self.n:]
        assert bool((lo == self.band).all()) and bool((hi == self.band).all()), "%s: a write outside the tensor" % what


def guard_in(t, w, ch):
    return Guarded(tuple(t.shape), margin_of(w, ch), NAN, t)


def guard_out(shape, w, ch):
    return Guarded(tuple(shape), margin_of(w, ch), SENTINEL, NAN)


class Workspace:
    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        assert self.nbytes % 4 == 0
        self.g = Guarded((self.nbytes // 4,), 1024, SENTINEL, NAN)           # the sentinel starts at the first byte past the request

    def args(self, use):
        return (nv.ptr(self.g.t), self.nbytes) if use and self.nbytes else (None, 0)

    def check(self, what):
        lo, hi = self.g.buf[:1024], self.g.buf[1024 + self.nbytes // 4:]
        assert len(hi) == 1024 and bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), "%s: a write outside the workspace" % what


@pytest.fixture(scope="module")
def tickets():
    return torch.zeros(nv.X3G_TILE_COUNTERS, dtype=torch.int32, device=DEV)


def absmax(t):
    out = torch.zeros(1, device=DEV)
    nv.check(nv.lib().frcnn_tensor_absmax(nv.ptr(t), t.numel(), nv.ptr(out), S()), "tensor_absmax")
    assert float(out) == float(t.abs().max())
    return out


class Forward:
    """the operands of one case on the device and every forward entry point over them"""

    def __init__(self, c, o, tickets):
        self.c, self.tickets = c, tickets
        self.shape = (c.N, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.pad)
        self.ho, self.wo = G.out_hw(c)
        self.x = guard_in(o["x"], c.W, c.cin)
        self.wp = guard_in(G.pack(o["w"]), 0, 0)
        self.b = o["b"].to(DEV)
        self.res = o["res_y"].to(DEV)
        self.ws = Workspace(nv.lib().frcnn_conv_workspace_bytes(*self.shape))
        self.x3 = G.forward_takes_x3(c)
        if self.x3:
            self.xmax, self.wmax = absmax(self.x.t), absmax(self.wp.t)
            self.wsplit = torch.empty_like(self.wp.t)
            nv.check(nv.lib().frcnn_pack_conv_x3g_weights(nv.ptr(self.wp.t), nv.ptr(self.wmax), nv.ptr(self.wsplit), c.k * c.k, c.cout, c.cin, S()),
                     "pack_conv_x3g_weights")

    def entries(self):
        return ["nhwc", "math0", "math1"] + (["x3g", "x3g_tickets", "x3g_wsplit", "x3g_wsplit_tickets"] if self.x3 else [])

    def run(self, entry, relu, with_res, use_ws):
        """-> (y, ymax or None); the guard bands of y and of the workspace are checked"""
        lib, c = nv.lib(), self.c
        y = guard_out((c.N, self.ho, self.wo, c.cout), self.wo, c.cout)
        self.ws.g.t.fill_(NAN)
        head = (nv.ptr(self.x.t), nv.ptr(self.wp.t), nv.ptr(self.b), nv.ptr(self.res) if with_res else None, nv.ptr(y.t)) + self.shape
        flags = nv.RELU if relu else 0
        ws = self.ws.args(use_ws)
        ymax = None
        if entry == "nhwc":
            rc = lib.frcnn_conv_nhwc(*head, flags, *ws, S())
        elif entry in ("math0", "math1"):
            rc = lib.frcnn_conv_nhwc_math(*head, flags, F32 if entry == "math0" else BF16, *ws, S())
        else:
            ymax = torch.zeros(1, device=DEV)
            if "wsplit" in entry:
                head = (head[0], nv.ptr(self.wsplit)) + head[2:]
                flags |= nv.X3G_WSPLIT
            scales = (nv.ptr(self.xmax), nv.ptr(self.wmax), nv.ptr(ymax))
            if entry.endswith("tickets"):
                rc = lib.frcnn_conv_nhwc_x3g_tickets(*head, flags, *scales, *ws, nv.ptr(self.tickets), S())
            else:
                rc = lib.frcnn_conv_nhwc_x3g(*head, flags, *scales, *ws, S())
        what = "%s %s relu=%d res=%d ws=%d" % (c.name, entry, relu, with_res, use_ws)
        nv.check(rc, what)
        torch.cuda.synchronize()
        y.check(what)
        self.ws.check(what)
        if entry.endswith("tickets"):
            assert int(self.tickets.abs().max()) == 0, "%s: the ticket array is zero again" % what
        return y.t, ymax


def first_difference(got, want):
    d = (got != want).nonzero()
    return "%d of %d elements differ, first at %s: got %s, want %s" % (
        len(d), got.numel(), tuple(d[0].tolist()), float(got[tuple(d[0])]), float(want[tuple(d[0])])) if len(d) else "equal"


def assert_bits(got, want, what):
    assert torch.equal(got, want), "%s: %s" % (what, first_difference(got, want))


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in G.CASES if G.forward_ok(c)], ids=lambda c: c.name)
def test_forward_is_the_float64_convolution_to_the_bit(c, tickets):
    refs = G.exact_references(c)
    want = {(True, True): refs["y"].to(torch.float32).to(DEV), (False, False): refs["y_plain"].to(torch.float32).to(DEV)}
    tickets.zero_()
    sat = nv.x3_saturation_count()
    f = Forward(c, G.operands(c), tickets)
    if not f.x3:
        y = torch.zeros((c.N, f.ho, f.wo, c.cout), device=DEV)
        one = torch.ones(1, device=DEV)
        head = (nv.ptr(f.x.t), nv.ptr(f.wp.t), nv.ptr(f.b), None, nv.ptr(y)) + f.shape
        assert nv.lib().frcnn_conv_nhwc_x3g(*head, 0, nv.ptr(one), nv.ptr(one), None, *f.ws.args(True), S()) == EUNSUPPORTED
        assert nv.lib().frcnn_conv_nhwc_x3g_tickets(*head, 0, nv.ptr(one), nv.ptr(one), None, *f.ws.args(True), nv.ptr(tickets), S()) == EUNSUPPORTED
    for (relu, with_res), ref in want.items():
        for use_ws in (True, False):
            for entry in f.entries():
                for rep in range(3 if entry.endswith("tickets") and use_ws else 1):
                    y, ymax = f.run(entry, relu, with_res, use_ws)
                    what = "%s %s relu=%d res=%d ws=%d call %d" % (c.name, entry, relu, with_res, use_ws, rep)
                    assert_bits(y, ref, what)
                    if ymax is not None:
                        assert float(ymax) == float(ref.abs().max()), "%s: the emitted maximum is the tensor's" % what
    assert nv.x3_saturation_count() == sat, "a true maximum never saturates"


class Backward:
    def __init__(self, c, o):
        self.c = c
        self.shape = (c.N, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.pad)
        self.ho, self.wo = G.out_hw(c)
        self.dz = guard_in(o["dz"], self.wo, c.cout)
        self.x = guard_in(o["x"], c.W, c.cin)
        self.res = o["res_x"].to(DEV)
        self.w = o["w"]

    def dgrad(self, math, with_res, use_ws, plain_entry=False):
        lib, c = nv.lib(), self.c
        if not hasattr(self, "wd"):
            wp = G.pack(self.w).to(DEV)
            self.wd = guard_in(torch.zeros(c.k * c.k, c.cin, c.cout), 0, 0)
            nv.check(lib.frcnn_pack_conv_dgrad(nv.ptr(wp), nv.ptr(self.wd.t), c.k * c.k, c.cout, c.cin, S()), "pack_conv_dgrad")
            assert torch.equal(self.wd.t.cpu(), G.pack_dgrad(self.w))
            self.ws_d = Workspace(lib.frcnn_conv_dgrad_workspace_bytes(*self.shape))
        dx = guard_out((c.N, c.H, c.W, c.cin), c.W, c.cin)
        self.ws_d.g.t.fill_(NAN)
        head = (nv.ptr(self.dz.t), nv.ptr(self.wd.t), nv.ptr(self.res) if with_res else None, nv.ptr(dx.t)) + self.shape
        if plain_entry:
            rc = lib.frcnn_conv_dgrad(*head, *self.ws_d.args(use_ws), S())
        else:
            rc = lib.frcnn_conv_dgrad_math(*head, math, *self.ws_d.args(use_ws), S())
        what = "%s dgrad math=%s res=%d ws=%d" % (c.name, "-" if plain_entry else math, with_res, use_ws)
        nv.check(rc, what)
        torch.cuda.synchronize()
        dx.check(what)
        self.ws_d.check(what)
        return dx.t, what

    def wgrad(self, math, use_ws, plain_entry=False):
        lib, c = nv.lib(), self.c
        if not hasattr(self, "ws_w"):
            self.ws_w = Workspace(lib.frcnn_conv_wgrad_workspace_bytes(*self.shape))
        dwp = guard_out((c.k * c.k, c.cout, c.cin), 0, 0)
        self.ws_w.g.t.fill_(NAN)
        head = (nv.ptr(self.x.t), nv.ptr(self.dz.t), nv.ptr(dwp.t)) + self.shape
        if plain_entry:
            rc = lib.frcnn_conv_wgrad(*head, *self.ws_w.args(use_ws), S())
        else:
            rc = lib.frcnn_conv_wgrad_math(*head, math, *self.ws_w.args(use_ws), S())
        what = "%s wgrad math=%s ws=%d" % (c.name, "-" if plain_entry else math, use_ws)
        nv.check(rc, what)
        torch.cuda.synchronize()
        dwp.check(what)
        self.ws_w.check(what)
        return dwp.t, what


@pytest.mark.parametrize("c", [c for c in G.CASES if G.dgrad_ok(c)], ids=lambda c: c.name)
def test_data_gradient_is_the_float64_gradient_to_the_bit(c):
    refs = G.exact_references(c)
    want = {False: refs["dx"].to(torch.float32).to(DEV), True: refs["dx_res"].to(torch.float32).to(DEV)}
    untouched = torch.from_numpy(G.untouched_dx_pixels(c)).to(DEV)
    bw = Backward(c, G.operands(c))
    for with_res in (False, True):
        for use_ws in (True, False):
            runs = [bw.dgrad(F32, with_res, use_ws), bw.dgrad(BF16, with_res, use_ws)]
            if use_ws:
                runs.append(bw.dgrad(F32, with_res, use_ws, plain_entry=True))
            for dx, what in runs:
                assert_bits(dx, want[with_res], what)
                if bool(untouched.any()):       # pixels no tap reads: exactly the residual, or zero without one
                    assert torch.equal(dx[:, untouched], bw.res[:, untouched] if with_res else torch.zeros_like(dx[:, untouched])), what


@pytest.mark.parametrize("c", [c for c in G.CASES if G.wgrad_ok(c)], ids=lambda c: c.name)
def test_weight_gradient_is_the_float64_gradient_to_the_bit(c):
    want = G.exact_references(c)["dw"].to(torch.float32).to(DEV)
    bw = Backward(c, G.operands(c))
    for use_ws in (True, False):
        for dwp, what in [bw.wgrad(F32, use_ws), bw.wgrad(BF16, use_ws)] + ([bw.wgrad(F32, use_ws, plain_entry=True)] if use_ws else []):
            assert_bits(dwp, want, what)


# ---- impulses ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.IMPULSE_CASES, ids=lambda c: c.name)
def test_an_impulse_meets_every_tap_once(c, tickets):
    """one 1 in the activations (forward) or in the upstream gradient (data gradient) and weights w[tap] = 1 + tap on four (co, ci) pairs:
    the output names the tap that was used for every pixel around the impulse -- at the corners, across an image boundary and on both sides
    of the 64- and 128-row tile seams"""
    wt = G.impulse_weights(c)
    ho, wo = G.out_hw(c)
    zeros = dict(G.operands(c))
    zeros.update(w=wt, b=torch.zeros(c.cout))
    channels_in, channels_out = (0, 5, 17, c.cin - 1), (0, 1, c.cout // 2, c.cout - 1)
    tickets.zero_()
    for i, (n, yy, xx) in enumerate(G.impulse_positions(c.N, c.H, c.W)):
        x = torch.zeros(c.N, c.H, c.W, c.cin)
        x[n, yy, xx, channels_in[i % 4]] = 1.0
        want = G.ref_forward(c, x, wt, zeros["b"]).to(torch.float32)
        assert int((want != 0).sum()) >= 1
        f = Forward(c, dict(zeros, x=x), tickets)
        for entry in ("nhwc", "math1", "x3g", "x3g_tickets"):
            for use_ws in (True, False):
                y, _ = f.run(entry, False, False, use_ws)
                assert_bits(y, want.to(DEV), "%s forward %s ws=%d impulse at %s" % (c.name, entry, use_ws, (n, yy, xx)))
    for i, (n, yy, xx) in enumerate(G.impulse_positions(c.N, ho, wo)):
        dz = torch.zeros(c.N, ho, wo, c.cout)
        dz[n, yy, xx, channels_out[i % 4]] = 1.0
        want = G.ref_dgrad(c, dz, wt).to(torch.float32).to(DEV)
        bw = Backward(c, dict(zeros, dz=dz))
        for math in (F32, BF16):
            for use_ws in (True, False):
                dx, what = bw.dgrad(math, False, use_ws)
                assert_bits(dx, want, "%s impulse at %s" % (what, (n, yy, xx)))


# ---- the two finishes of a split reduction, on data whose sum depends on the order --------------------------------------------------------------
@pytest.mark.parametrize("name", ["k3p1s1", "split_k3_c64", "split_k3_c96", "split_k1_c544", "split_k3_c160", "x3cfg2_split", "x3cfg2_short",
                                  "x3cfg0_split", "x3cfg0_short", "k3p2s1", "x3cfg0"])
def test_split_finishes_agree_to_the_bit_on_gaussian_data(name, tickets):
    """frcnn_conv_nhwc_x3g (separate finishing pass) and frcnn_conv_nhwc_x3g_tickets (the last block of a tile finishes) sum the partial planes
    in the same order: the same bits, output and emitted maximum, with float32 and with pre-split weights; three calls in a row leave the
    ticket array zero.  The last two cases do not split: tickets passed to a plan that has no use for them."""
    c = G.BY_NAME[name]
    plan = G.forward_plans(c)["x3g"]
    assert (plan.splits > 1) == (name not in ("k3p2s1", "x3cfg0"))
    tickets.zero_()
    o = G.gaussian_operands(c)
    f = Forward(c, o, tickets)
    truth = G.ref_forward(c, o["x"], o["w"], o["b"], o["res_y"], relu=True)
    y0, m0 = f.run("x3g", True, True, True)
    e = float((y0.cpu().double() - truth).abs().max() / truth.abs().max())
    assert e <= 1e-6, "f32x3 under a tensor scale (the bound of tests/test_conv_x3g_gpu.py): %g" % e
    assert float(m0) == float(y0.abs().max())
    for entry in ("x3g_tickets", "x3g_wsplit", "x3g_wsplit_tickets"):
        for rep in range(3):
            y1, m1 = f.run(entry, True, True, True)
            assert_bits(y1, y0, "%s %s call %d" % (name, entry, rep))
            assert float(m1) == float(m0)
    # without a workspace the launch does not split, tickets or none: one sum per output, the same in both entry points
    y2, m2 = f.run("x3g", True, True, False)
    y3, m3 = f.run("x3g_tickets", True, True, False)
    assert_bits(y3, y2, "%s un-split" % name)
    assert float(m2) == float(m3) == float(y2.abs().max())


# ---- Gaussian data on the geometries only the generic kernels take ----------------------------------------------------------------------------
def r16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def rel_err(got, truth64):
    return float((got.double().cpu() - truth64).abs().max()) / max(float(truth64.abs().max()), 1e-30)


@pytest.mark.parametrize("math", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", G.RANDOM_CASES, ids=lambda c: c.name)
def test_generic_geometries_on_gaussian_data(c, math, tickets):
    """the criterion of tests/test_train_bf16_gpu.py: the error against the float64 result, relative to the truth's largest magnitude, within
    the larger of 4 x torch's float32 CPU convolution's own error on the same operands and 1.2e-7 sqrt(K); bf16: both sides round the operands"""
    o = G.gaussian_operands(c)
    rnd = r16 if math == BF16 else (lambda t: t)
    x, w, dz = rnd(o["x"]), rnd(o["w"]), rnd(o["dz"])
    f = Forward(c, o, tickets)
    assert not f.x3
    bw = Backward(c, o)
    entry = "math1" if math == BF16 else "nhwc"
    truth = G.ref_forward(c, x, w, o["b"], o["res_y"], relu=True)
    yard = rel_err(G.ref_forward(c, x, w, o["b"], o["res_y"], relu=True, dtype=torch.float32), truth)
    tol = max(4 * yard, 1.2e-7 * (c.cin * c.k * c.k) ** 0.5)
    for use_ws in (True, False):
        y, _ = f.run(entry, True, True, use_ws)
        e = rel_err(y, truth)
        print("%s forward math %d ws %d: %.3g (torch float32 %.3g, bound %.3g)" % (c.name, math, use_ws, e, yard, tol))
        assert e <= tol, (e, yard, tol)
    if G.dgrad_ok(c):
        truth = G.ref_dgrad(c, dz, w, o["res_x"])
        yard = rel_err(G.ref_dgrad(c, dz, w, o["res_x"], dtype=torch.float32), truth)
        tol = max(4 * yard, 1.2e-7 * (c.cout * c.k * c.k) ** 0.5)
        for use_ws in (True, False):
            dx, _ = bw.dgrad(math, True, use_ws)
            e = rel_err(dx, truth)
            print("%s dgrad math %d ws %d: %.3g (torch float32 %.3g, bound %.3g)" % (c.name, math, use_ws, e, yard, tol))
            assert e <= tol, (e, yard, tol)
    if G.wgrad_ok(c):
        truth = G.ref_wgrad(c, x, dz)
        yard = rel_err(G.ref_wgrad(c, x, dz, dtype=torch.float32), truth)
        tol = max(4 * yard, 1.2e-7 * G.rows_forward(c) ** 0.5)
        for use_ws in (True, False):
            dwp, _ = bw.wgrad(math, use_ws)
            e = rel_err(dwp, truth)
            print("%s wgrad math %d ws %d: %.3g (torch float32 %.3g, bound %.3g)" % (c.name, math, use_ws, e, yard, tol))
            assert e <= tol, (e, yard, tol)
