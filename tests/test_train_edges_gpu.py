"""
The train step's small kernels (csrc/train.hip, softmax_rows of csrc/linear.hip) on the GPU, through the C ABI, at their stride, chunk
and tail seams, against the references of tests/train_edge_cases.py (checked without a GPU by tests/test_train_edges_cpu.py):
  * the one-block loss kernels beyond one pass of their 256 threads, with no samples, without a gradient buffer, at every row stride;
  * the RoI-pool scatter across its 64-RoI chunks, with its 64 x 49 hit list exactly full, beyond 256 channels;
  * the grid-stride kernels beyond their grid caps, where the second stride pass runs, and at their tails: to the bit.
Every output buffer starts as NaN (or a sentinel) and is one row longer than the kernel may write.
"""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from tests import train_edge_cases as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = E.U


def S():
    return nv.stream_ptr()


def gpu(x):
    return torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x).to(DEV).contiguous()


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def same_bits(got, want):
    """torch.equal on the values (no NaN anywhere) and on their bit patterns (-0.0 is not +0.0)."""
    want = torch.as_tensor(want)
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    return torch.equal(got, want) and torch.equal(got.view(torch.int32), want.view(torch.int32))


def rel(got, want):
    return abs(float(got) - want) / abs(want) if want != 0 else (0.0 if float(got) == 0.0 else float("inf"))


# ---- frcnn_rpn_loss -----------------------------------------------------------------------------------------------------------------
def run_rpn_loss(head, ld, sample, rpn_map, with_grad=True):
    P = head.shape[0]
    d_head, d_sample, d_map = gpu(head), gpu(sample), gpu(rpn_map)
    losses = nans(3)
    dh = nans(P + 1, ld) if with_grad else None
    nv.check(nv.lib().frcnn_rpn_loss(nv.ptr(d_head), ld, P, nv.ptr(d_sample) if len(sample) else None, len(sample), nv.ptr(d_map),
                                     nv.ptr(losses), nv.ptr(dh), S()), "rpn_loss")
    return losses.cpu(), (dh.cpu() if with_grad else None)


@pytest.mark.parametrize("mix", E.RPN_MIXES)
@pytest.mark.parametrize("ld", E.RPN_LD)
@pytest.mark.parametrize("n_sample", E.RPN_N_SAMPLE)
def test_rpn_loss_at_the_block_stride(n_sample, ld, mix):
    head, sample, rpn_map = E.rpn_case(n_sample, ld, mix)
    t_c, t_r, t_d = E.rpn_loss_truth(head, sample, rpn_map)
    losses, dh = run_rpn_loss(head, ld, sample, rpn_map)
    print("rpn_loss n=%d ld=%d %s: class %.9g (truth %.9g) regression %.9g (truth %.9g)" % (n_sample, ld, mix, float(losses[0]), t_c,
                                                                                          float(losses[1]), t_r))
    assert torch.isnan(losses[2]) and torch.isnan(dh[E.RPN_P]).all()                 # nothing past the two losses / the map's rows
    dh = dh[:E.RPN_P].numpy()
    assert not np.isnan(dh).any()
    assert rel(losses[0], t_c) <= 1e-5 and rel(losses[1], t_r) <= 1e-5
    gmax = np.abs(t_d).max()
    print("  gradient error %.3g of max %.3g" % (np.abs(dh - t_d).max(), gmax))
    assert np.abs(dh - t_d).max() <= 1e-5 * gmax
    # exactly zero outside the sampled anchors' columns, pad columns included
    touched = np.zeros(head.shape, dtype=bool)
    for a in sample:
        touched[a // 9, a % 9] = True
        touched[a // 9, 9 + 4 * (a % 9):13 + 4 * (a % 9)] = True
    assert not dh[~touched].any() and not dh[:, 45:].any()
    if n_sample == 0:
        assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0 and not dh.any()
    if mix == "background":
        assert float(losses[1]) == 0.0 and not dh[:, 9:].any()
    # without a gradient buffer: the same two losses, to the bit
    l2, _ = run_rpn_loss(head, ld, sample, rpn_map, with_grad=False)
    assert torch.equal(l2[:2].view(torch.int32), losses[:2].view(torch.int32)) and torch.isnan(l2[2])


# ---- frcnn_detector_loss ------------------------------------------------------------------------------------------------------------
def run_detector_loss(classes, deltas, onehot, gtd, ncls, ld, with_grad=True):
    n = classes.shape[0]
    bufs = [gpu(v) for v in (classes, deltas, onehot, gtd)]
    losses = nans(3)
    dl = nans(n + 1, ld) if with_grad else None
    nv.check(nv.lib().frcnn_detector_loss(*[nv.ptr(b) if n else None for b in bufs], n, ncls, nv.ptr(losses), nv.ptr(dl), ld, S()),
             "detector_loss")
    return losses.cpu(), (dl.cpu() if with_grad else None)


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("ncls", E.DET_NCLS)
@pytest.mark.parametrize("n", E.DET_S)
def test_detector_loss_at_the_block_stride(n, ncls, pad):
    nd = 4 * (ncls - 1)
    ld = 128 if pad else ncls + nd
    assert ld >= ncls + nd
    classes, deltas, onehot, gtd, cls, kind = E.detector_case(n, ncls)
    t1, t2, tg = E.detector_loss_truth(classes, deltas, onehot, gtd)
    losses, dl = run_detector_loss(classes, deltas, onehot, gtd, ncls, ld)
    print("detector_loss S=%d ncls=%d ld=%d: class %.9g (truth %.9g) regression %.9g (truth %.9g)" % (n, ncls, ld, float(losses[0]), t1,
                                                                                                    float(losses[1]), t2))
    assert torch.isnan(losses[2]) and torch.isnan(dl[n]).all()                       # the guard row is untouched
    if n == 0:
        assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0
    else:
        dl = dl[:n].numpy()
        assert not np.isnan(dl).any()
        assert rel(losses[0], t1) <= 1e-5 and rel(losses[1], t2) <= 1e-5
        e_c, e_d = np.abs(dl[:, :ncls] - tg[:, :ncls]).max(), np.abs(dl[:, ncls:ncls + nd] - tg[:, ncls:]).max()
        print("  class gradient error %.3g of max %.3g, delta gradient error %.3g of max %.3g" % (e_c, np.abs(tg[:, :ncls]).max(), e_d,
                                                                                                np.abs(tg[:, ncls:]).max()))
        assert e_c <= 2e-5 * np.abs(tg[:, :ncls]).max()
        assert e_d <= 1e-6 * np.abs(tg[:, ncls:]).max() or not tg[:, ncls:].any() and e_d == 0.0
        assert not dl[:, ncls:ncls + nd][gtd[:, 0, :] == 0].any()                    # mask-zero delta gradients
        assert not dl[:, ncls + nd:].any()                                           # pad columns
    l2, _ = run_detector_loss(classes, deltas, onehot, gtd, ncls, ld, with_grad=False)
    assert torch.equal(l2[:2].view(torch.int32), losses[:2].view(torch.int32)) and torch.isnan(l2[2])


# ---- frcnn_roi_pool_backward -----------------------------------------------------------------------------------------------------------
def run_roi_pool_backward(fm, rois, pooled, dout, base=None):
    fh, fw, c = fm.shape
    n = rois.shape[0]
    lib = nv.lib()
    d_fm, d_rois, d_dout = gpu(fm), gpu(rois), gpu(dout)
    wsb = int(lib.frcnn_roi_pool_backward_workspace_bytes(n, pooled, c))
    assert wsb == n * pooled * pooled * c * 4
    ws = torch.empty((wsb // 4 + 1,), dtype=torch.int32, device=DEV)
    dfm = nans(fh + 1, fw, c)
    if base is not None:
        dfm[:fh] = gpu(base)
    nv.check(lib.frcnn_roi_pool_backward(nv.ptr(d_fm), fh, fw, c, nv.ptr(d_rois) if n else None, n, pooled, E.ROI_SCALE,
                                         nv.ptr(d_dout) if n else None, nv.ptr(dfm), 0 if base is None else 1,
                                         nv.ptr(ws) if n else None, wsb, S()), "roi_pool_backward")
    out = dfm.cpu()
    assert torch.isnan(out[fh]).all()
    return out[:fh]


def check_roi_pool_backward(fm, rois, pooled):
    fh, fw, c = fm.shape
    n = rois.shape[0]
    r = E.rng_of(fh, fw, c, pooled, n)
    dout = r.randn(n, pooled, pooled, c).astype(np.float32)
    truth, count, sum_abs = E.roi_pool_backward_truth(fm, rois, pooled, E.ROI_SCALE, dout)
    got_t = run_roi_pool_backward(fm, rois, pooled, dout)
    got = got_t.numpy()
    assert not np.isnan(got).any()
    # the addends are the same float32 numbers; only the order of their float32 sum may differ
    err, bound = np.abs(got.astype(np.float64) - truth), count * U * sum_abs
    print("roi_pool_backward %dx%dx%d pooled %d, %d RoIs: max error %.3g, max addends %d, cells with addends %d of %d" % (
        fh, fw, c, pooled, n, err.max(), count.max() if n else 0, int((count > 0).sum()), count.size))
    assert (err <= bound).all(), float((err - bound).max())
    assert not got[count == 0].any()
    base = r.randn(fh, fw, c).astype(np.float32)
    acc = run_roi_pool_backward(fm, rois, pooled, dout, base=base)
    assert same_bits(acc, torch.from_numpy(base) + got_t)                            # one rounding per cell
    return got, count


@pytest.mark.parametrize("fh,fw,c,pooled,n", E.ROI_SHAPES)
def test_roi_pool_backward_across_chunks_and_channel_passes(fh, fw, c, pooled, n):
    fm = E.roi_map(fh, fw, c)
    got, count = check_roi_pool_backward(fm, E.roi_boxes(fh, fw, n), pooled)
    if n == 0:
        assert not got.any()                                                         # accumulate = 0: all zeros; = 1: the base (above)
    else:
        assert count.any()
    if c > 256:
        assert count[:, :, 256:].any()                                               # the channels of the later passes receive gradient


def test_roi_pool_backward_with_a_full_hit_list():
    fm = E.roi_map(8, 9, 8)
    rois = E.full_hit_list_boxes()
    got, count = check_roi_pool_backward(fm, rois, 7)
    assert (count[3, 4] >= 65 * 49).all()
    for m in (64, 65):                                                               # the list exactly full with and without a next chunk
        check_roi_pool_backward(fm, rois[:m], 7)


# ---- the bit-exact group ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.RELU_N)
def test_relu_backward_bit_exact(n):
    dy, y = E.relu_case(n)
    want = E.relu_backward_ref(dy, y)
    assert not np.isnan(want).any()
    d = nans(n + 4)
    d[:n] = gpu(dy)
    d_y = gpu(y)
    nv.check(nv.lib().frcnn_relu_backward(nv.ptr(d), nv.ptr(d_y), n, S()), "relu_backward")
    got = d.cpu()
    assert torch.isnan(got[n:]).all()
    assert same_bits(got[:n], want)


@pytest.mark.parametrize("n", E.ADD_N)
def test_add_inplace_bit_exact(n):
    r = E.rng_of(n, 3)
    a, b = r.randn(n).astype(np.float32), r.randn(n).astype(np.float32)
    d = nans(n + 1)
    d[:n] = gpu(a)
    d_b = gpu(b)
    nv.check(nv.lib().frcnn_add_inplace(nv.ptr(d), nv.ptr(d_b), n, S()), "add_inplace")
    got = d.cpu()
    assert torch.isnan(got[n]) and same_bits(got[:n], E.add_ref(a, b))


@pytest.mark.parametrize("H,W,c", E.MAXPOOL_SHAPES)
def test_maxpool2x2_backward_bit_exact(H, W, c):
    # (no NaN in x: torch sends the gradient to a NaN, this kernel's '>' does not -- out of scope here)
    x, dy = E.maxpool_case(H, W, c)
    want = E.maxpool2x2_backward_ref(x, dy)
    d_x, d_dy = gpu(x), gpu(dy)
    dx = nans(H + 1, W, c)
    nv.check(nv.lib().frcnn_maxpool2x2_backward(nv.ptr(d_x), nv.ptr(d_dy), nv.ptr(dx), H, W, c, S()), "maxpool2x2_backward")
    got = dx.cpu()
    del dx, d_x
    assert torch.isnan(got[H]).all()
    assert same_bits(got[:H], want)
    if H % 2:
        assert not got[H - 1].any()
    if W % 2:
        assert not got[:H, W - 1].any()


@pytest.mark.parametrize("rows,cols", E.TRANSPOSE_SHAPES)
def test_transpose_bit_exact_with_padded_strides(rows, cols):
    ldi, ldo = cols + 3, rows + 5
    x = E.rng_of(rows, cols).randn(rows, ldi).astype(np.float32)
    d_x = gpu(x)
    y = nans(cols + 1, ldo)
    nv.check(nv.lib().frcnn_transpose(nv.ptr(d_x), ldi, nv.ptr(y), ldo, rows, cols, S()), "transpose")
    got = y.cpu()
    assert torch.isnan(got[cols]).all()                                              # the guard row
    assert same_bits(got[:cols], E.transpose_ref(x, rows, cols, ldo))
    assert not got[:cols, rows:].any()


@pytest.mark.parametrize("row_floats", E.GATHER_ROW_FLOATS)
def test_gather_rows_bit_exact(row_floats):
    r = E.rng_of(row_floats, 4)
    src = r.randn(9, row_floats).astype(np.float32)
    idx = np.array([8, 0, 3, 3, 8, 0, 5], dtype=np.int32)                            # duplicates, the first row, the last row
    d_src, d_idx = gpu(src), gpu(idx)
    dst = nans(len(idx) + 1, row_floats)
    nv.check(nv.lib().frcnn_gather_rows(nv.ptr(d_src), nv.ptr(d_idx), len(idx), row_floats, nv.ptr(dst), S()), "gather_rows")
    got = dst.cpu()
    assert torch.isnan(got[len(idx)]).all() and same_bits(got[:len(idx)], E.gather_ref(src, idx))
    dst = nans(2, row_floats)
    nv.check(nv.lib().frcnn_gather_rows(nv.ptr(d_src), nv.ptr(d_idx), 0, row_floats, nv.ptr(dst), S()), "gather_rows")
    assert torch.isnan(dst.cpu()).all()                                              # n = 0: untouched


@pytest.mark.parametrize("taps,cout,cin", E.PACK_SHAPES)
def test_weight_packs_and_scale_rows_bit_exact(taps, cout, cin):
    r = E.rng_of(taps, cout, cin)
    wp = r.randn(taps, cout, cin).astype(np.float32)
    scale = (r.rand(cout) + 0.5).astype(np.float32)
    lib = nv.lib()
    d_wp, d_scale = gpu(wp), gpu(scale)
    n = taps * cout * cin
    out = nans(n + 1)
    nv.check(lib.frcnn_pack_conv_dgrad(nv.ptr(d_wp), nv.ptr(out), taps, cout, cin, S()), "pack_conv_dgrad")
    got = out.cpu()
    assert torch.isnan(got[n]) and same_bits(got[:n].reshape(taps, cin, cout), E.pack_conv_dgrad_ref(wp))
    if taps == 9:
        out = nans(n + 1)
        nv.check(lib.frcnn_pack_conv3x3_dgrad(nv.ptr(d_wp), nv.ptr(out), cout, cin, S()), "pack_conv3x3_dgrad")
        got = out.cpu()
        assert torch.isnan(got[n]) and same_bits(got[:n].reshape(9, cin, cout), E.pack_conv3x3_dgrad_ref(wp))
    out = nans(n + 1)
    nv.check(lib.frcnn_scale_rows(nv.ptr(d_wp), nv.ptr(d_scale), nv.ptr(out), taps, cout, cin, S()), "scale_rows")
    got = out.cpu()
    assert torch.isnan(got[n]) and same_bits(got[:n].reshape(taps, cout, cin), E.scale_rows_ref(wp, scale))


@pytest.mark.parametrize("N,H,W,c", E.MEAN_SHAPES)
def test_spatial_mean_backward_bit_exact(N, H, W, c):
    dy = E.rng_of(N, H, W, c).randn(N, c).astype(np.float32)
    want = E.spatial_mean_backward_ref(dy, H, W)
    if H * W > 1 and (H * W) & (H * W - 1):
        # on these inputs the two-division reference differs from the one-division form, so the test can tell them apart
        assert not np.array_equal(want[:, 0, 0, :], (dy / np.float32(H * W)).astype(np.float32))
    d_dy = gpu(dy)
    n = N * H * W * c
    dx = nans(n + 1)
    nv.check(nv.lib().frcnn_spatial_mean_backward(nv.ptr(d_dy), nv.ptr(dx), N, H, W, c, S()), "spatial_mean_backward")
    got = dx.cpu()
    assert torch.isnan(got[n]) and same_bits(got[:n].reshape(N, H, W, c), want)


def run_sgd_steps(shape, momentum, wd, fold):
    """Three steps of frcnn_sgd_step / frcnn_sgd_step_fold against E.sgd_ref: w, buf and folded to the bit after every step."""
    n = int(np.prod(shape))
    r = E.rng_of(n, int(momentum * 10), int(wd * 1e4), int(fold))
    w = r.randn(*shape).astype(np.float32)
    scale = (r.rand(shape[1]) + 0.5).astype(np.float32) if fold else None
    lib = nv.lib()
    d_w = nans(n + 1)
    d_w[:n] = gpu(w.reshape(-1))
    d_buf = nans(n + 1) if momentum else None
    d_folded = nans(n + 1) if fold else None
    d_scale = gpu(scale) if fold else None
    buf = None
    for step in range(3):
        g = r.randn(*shape).astype(np.float32)
        d_g = gpu(g.reshape(-1))
        first = 1 if step == 0 else 0
        if fold:
            nv.check(lib.frcnn_sgd_step_fold(nv.ptr(d_w), nv.ptr(d_g), nv.ptr(d_buf), n, E.SGD_LR, momentum, wd, first, nv.ptr(d_scale),
                                             nv.ptr(d_folded), shape[1], shape[2], S()), "sgd_step_fold")
        else:
            nv.check(lib.frcnn_sgd_step(nv.ptr(d_w), nv.ptr(d_g), nv.ptr(d_buf), n, E.SGD_LR, momentum, wd, first, S()), "sgd_step")
        w, buf, folded = E.sgd_ref(w, g, buf, E.SGD_LR, momentum, wd, first, scale)
        got = d_w.cpu()
        assert torch.isnan(got[n]) and same_bits(got[:n], w.reshape(-1)), ("w", step)
        if momentum:
            got = d_buf.cpu()
            assert torch.isnan(got[n]) and same_bits(got[:n], buf.reshape(-1)), ("buf", step)
        if fold:
            got = d_folded.cpu()
            assert torch.isnan(got[n]) and same_bits(got[:n], folded.reshape(-1)), ("folded", step)


@pytest.mark.parametrize("momentum,wd", E.SGD_CONFIGS)
@pytest.mark.parametrize("n", E.SGD_N)
def test_sgd_step_bit_exact(n, momentum, wd):
    run_sgd_steps((n,), momentum, wd, fold=False)


@pytest.mark.parametrize("momentum,wd", E.SGD_CONFIGS)
@pytest.mark.parametrize("taps,cout,cin", E.SGD_FOLD_SHAPES)
def test_sgd_step_fold_bit_exact(taps, cout, cin, momentum, wd):
    run_sgd_steps((taps, cout, cin), momentum, wd, fold=True)


# ---- frcnn_bn_scale_shift ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.BN_C)
def test_bn_scale_shift_against_float64(c):
    gamma, beta, mean, var = E.bn_case(c)
    t_scale, t_shift, _ = E.bn_affine_truth(gamma, beta, mean, var, E.BN_EPS)
    bufs = [gpu(v) for v in (gamma, beta, mean, var)]
    scale, shift = nans(c + 1), nans(c + 1)
    nv.check(nv.lib().frcnn_bn_scale_shift(*[nv.ptr(b) for b in bufs], E.BN_EPS, c, nv.ptr(scale), nv.ptr(shift), S()), "bn_scale_shift")
    sc, sh = scale.cpu().numpy().astype(np.float64), shift.cpu().numpy().astype(np.float64)
    assert np.isnan(sc[c]) and np.isnan(sh[c])
    e_sc = np.abs(sc[:c] - t_scale) / np.abs(t_scale)
    e_sh = np.abs(sh[:c] - t_shift) / (np.abs(beta) + np.abs(mean * t_scale))
    print("bn_scale_shift c=%d: scale error %.3g, shift error %.3g (units of 2^-24)" % (c, e_sc.max() / U, e_sh.max() / U))
    assert (e_sc <= 4 * U).all()                                                     # three float32 roundings
    assert (e_sh <= 4 * U).all()


# ---- frcnn_softmax_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", E.SOFTMAX_NCLS)
@pytest.mark.parametrize("M", E.SOFTMAX_M)
def test_softmax_rows_two_classes_per_lane(M, ncls):
    """2e-7 absolute against the float64 softmax.  With the float32 butterfly sum the kernel had before, this measured 2.11e-7 at
    (M, ncls) = (5, 64) and 2.05e-7 at (301, 81) (1.77e-7 at (301, 21)); the kernel now sums and divides in float64."""
    for ldx in (ncls, ncls + 7):
        x, kind = E.softmax_case(M, ncls, ldx)
        truth = E.softmax_truth(x[:, :ncls])
        d_x = gpu(x)
        y = nans(M * ncls + ncls)
        nv.check(nv.lib().frcnn_softmax_rows(nv.ptr(d_x), ldx, nv.ptr(y), M, ncls, S()), "softmax_rows")
        got = y.cpu().numpy()
        assert np.isnan(got[M * ncls:]).all()                                        # nothing past M * ncls
        got = got[:M * ncls].reshape(M, ncls).astype(np.float64)
        assert np.isfinite(got).all()
        print("softmax_rows M=%d ncls=%d ldx=%d: max error %.3g, row sums off by %.3g" % (M, ncls, ldx, np.abs(got - truth).max(),
                                                                                       np.abs(got.sum(axis=1) - 1).max()))
        assert np.abs(got - truth).max() <= 2e-7
        assert np.abs(got.sum(axis=1) - 1).max() <= 128 * U
        assert not got[np.isneginf(x[:, :ncls])].any()                               # -inf entries: exactly 0
        if (kind == 0).any():
            assert np.abs(got[kind == 0] - 1.0 / ncls).max() <= 2e-7
