"""
The references of tests/train_edge_cases.py against torch autograd and oracle/train_oracle.py (no GPU), so that
tests/test_train_edges_gpu.py does not rest on unchecked code; and the FRCNN_EINVAL cases of the training entry points, which refuse
bad arguments before touching the device.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_edge_cases as E
from fasterrcnn_amd import _native as nv
from oracle import train_oracle as TO

EINVAL = -1


def test_c_round_is_half_away_from_zero():
    for v, want in ((0.5, 1), (1.5, 2), (2.5, 3), (4.5, 5), (-0.5, -1), (-2.5, -3), (0.49999997, 0), (-0.49999997, 0), (2.4999998, 2),
                    (0.0, 0), (7.0, 7), (-7.0, -7), (8388609.0, 8388609)):
        assert E.c_round(np.float32(v)) == want, v
    assert int(np.round(np.float32(2.5))) == 2          # what the reference must not do


# ---- losses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", E.RPN_MIXES)
@pytest.mark.parametrize("n_sample,ld", [(0, 45), (1, 48), (255, 128), (256, 45), (257, 48), (315, 128)])
def test_rpn_loss_truth_matches_the_oracle_under_float64_autograd(n_sample, ld, mix):
    head, sample, rpn_map = E.rpn_case(n_sample, ld, mix)
    assert len(set(sample.tolist())) == n_sample
    if n_sample >= 2:
        assert 0 in sample and 9 * E.RPN_P - 1 in sample
    hr = torch.from_numpy(head).double().requires_grad_(True)
    y_true = torch.from_numpy(rpn_map).double().reshape(1, E.RPN_FH, E.RPN_FW, 9, 6)
    scores = torch.sigmoid(hr[:, 0:9]).reshape(1, E.RPN_FH, E.RPN_FW, 9)
    deltas = hr[:, 9:45].reshape(1, E.RPN_FH, E.RPN_FW, 36)
    lc, lr = TO.rpn_class_loss(scores, y_true), TO.rpn_regression_loss(deltas, y_true)
    (lc + lr).backward()
    lc, lr = lc.detach(), lr.detach()
    t_c, t_r, t_d = E.rpn_loss_truth(head, sample, rpn_map)
    assert abs(t_c - float(lc)) <= 1e-12 * max(abs(float(lc)), 1e-30) and abs(t_r - float(lr)) <= 1e-12 * max(abs(float(lr)), 1e-30)
    want = hr.grad.numpy()
    assert np.abs(t_d - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-30)
    assert np.array_equal(t_d == 0, want == 0) or n_sample == 0
    if mix == "background" or n_sample == 0:
        assert t_r == 0.0 and not t_d[:, 9:].any()
    if n_sample == 0:
        assert t_c == 0.0 and not t_d.any()
    if mix != "background" and n_sample >= 255:
        # the case has what it claims: residuals on both sides of 1/9 in both signs, an exact zero, saturated logits
        obj = [int(a) for a in sample if rpn_map[a, 1] != 0]
        res = np.concatenate([rpn_map[a, 2:6] - head[a // 9, 9 + 4 * (a % 9):13 + 4 * (a % 9)] for a in obj])
        assert (res == 0).any() and (res > 1 / 9).any() and (res < -1 / 9).any()
        assert ((res > 0) & (res < 1 / 9)).any() and ((res < 0) & (res > -1 / 9)).any()
        logits = np.array([head[a // 9, a % 9] for a in sample])
        assert (logits == 120).any() and (logits == -120).any()


@pytest.mark.parametrize("ncls", E.DET_NCLS)
@pytest.mark.parametrize("S", E.DET_S)
def test_detector_loss_truth_matches_the_oracle_under_float64_autograd(S, ncls):
    classes, deltas, onehot, gtd, cls, kind = E.detector_case(S, ncls)
    if S >= 255:
        rows = np.arange(S)
        assert (classes[rows, cls][kind == 1] == 0.0).all() and (kind == 1).any()          # p == 0.0 exactly on the true class
        assert (classes[rows, cls][kind == 3] == 1.0).all() and (kind == 3).any()          # p == 1.0 exactly
        assert (cls[kind == 5] == 0).all() and not gtd[kind == 5, 0, :].any()              # background rows: empty mask
    # (a) on the float32 softmax outputs as a leaf: the loss, and its gradient through the softmax backward
    p = torch.from_numpy(classes).double().requires_grad_(True)
    d = torch.from_numpy(deltas).double().requires_grad_(True)
    l1 = TO.detector_class_loss(p, torch.from_numpy(onehot).double())
    l2 = TO.detector_regression_loss(d, torch.from_numpy(gtd).double())
    (l1 + l2).backward()
    l1, l2 = l1.detach(), l2.detach()
    t1, t2, tg = E.detector_loss_truth(classes, deltas, onehot, gtd, eps_in_float32=False)
    assert abs(t1 - float(l1)) <= 1e-12 * max(abs(float(l1)), 1e-30) and abs(t2 - float(l2)) <= 1e-12 * max(abs(float(l2)), 1e-30)
    nd = 4 * (ncls - 1)
    if S:
        assert np.abs(tg[:, ncls:] - d.grad.numpy()).max() <= 1e-12 * max(np.abs(d.grad.numpy()).max(), 1e-30)
        assert not tg[:, ncls:][gtd[:, 0, :] == 0].any()
    # (b) through torch's own softmax: logits -> softmax -> loss in float64, the truth fed those float64 probabilities
    r = E.rng_of(S, ncls, 3)
    lg = torch.from_numpy(r.randn(S, ncls) * 3).requires_grad_(True)
    pr = F.softmax(lg, dim=1)
    TO.detector_class_loss(pr, torch.from_numpy(onehot).double()).backward()
    _, _, tg2 = E.detector_loss_truth(pr.detach().numpy(), deltas, onehot, gtd, eps_in_float32=False)
    if S:
        assert np.abs(tg2[:, :ncls] - lg.grad.numpy()).max() <= 1e-11 * np.abs(lg.grad.numpy()).max()
    # (c) adding the 1e-7 in float32 moves p + eps by at most one float32 rounding: |d log| <= 2^-24 per row, 1 / (p + eps) by 2^-24 relative
    f1, f2, fg = E.detector_loss_truth(classes, deltas, onehot, gtd, eps_in_float32=True)
    assert f2 == t2 and abs(f1 - t1) <= 1.01 * E.U
    assert np.abs(fg - tg).max() <= 2.02 * E.U * max(np.abs(tg).max(), 1e-30) if S else fg.size == 0
    assert fg.shape == (S, ncls + nd)


# ---- RoI pool backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fh,fw,c,n", [(5, 6, 4, 1), (9, 11, 20, 65), (8, 9, 8, 64), (8, 9, 8, 66)])
def test_roi_pool_backward_truth_matches_the_oracle_autograd(fh, fw, c, n):
    fm = E.roi_map(fh, fw, c)
    rois = E.full_hit_list_boxes() if n == 66 else E.roi_boxes(fh, fw, n)
    dout = E.rng_of(fh, fw, n).randn(n, 7, 7, c).astype(np.float32)
    # the oracle's RoIPool pools into float32 whatever the map's type, so its backward sums the float32 addends in float32: it is held
    # to the float64 sum by the bound of a float32 sum of that many terms, and to the bit where a cell has one addend
    fmr = torch.from_numpy(fm).double().permute(2, 0, 1).unsqueeze(0).requires_grad_(True)
    pooled = TO.roi_pool_autograd(fmr, torch.from_numpy(rois))
    pooled.backward(torch.from_numpy(dout).permute(0, 3, 1, 2))
    want = fmr.grad[0].permute(1, 2, 0).numpy().astype(np.float64)
    grad, count, sum_abs = E.roi_pool_backward_truth(fm, rois, 7, E.ROI_SCALE, dout)
    assert (np.abs(grad - want) <= count * E.U * sum_abs).all()
    assert np.array_equal(grad[count == 1], want[count == 1]) and (count == 1).any() and (count > 1).any()
    assert np.array_equal(want == 0, grad == 0)
    assert np.array_equal(count == 0, sum_abs == 0) and not grad[count == 0].any()
    assert (np.abs(grad) <= sum_abs * (1 + 1e-12)).all()
    assert int(count.sum()) <= n * 49 * c
    if n == 66:
        # the single-cell RoIs: all 49 bins of each of the 65 send their gradient to cell (3, 4)
        assert (count[3, 4, :] >= 65 * 49).all()


def test_roi_boxes_hold_the_cases_they_claim():
    fh, fw = 9, 11
    b = E.roi_boxes(fh, fw, 65)
    s = b * np.float32(E.ROI_SCALE)
    half = np.abs(s - np.trunc(s)) == 0.5
    assert half[:, :].any() and (s[half] < 0).any() and (s[half] > 0).any()
    # a corner where round-half-to-even would differ from roundf
    assert any(E.c_round(v) != int(np.round(v)) for v in s[half])
    assert (b[:, 0] > 16 * fh).any() and (b[:, 2] < 0).any()                      # wholly off the map
    assert ((b[:, 2] < b[:, 0]) & (b[:, 3] < b[:, 1])).any()                      # inverted
    assert ((b[:, 0] < 0) & (b[:, 1] < 0) & (b[:, 2] > 16 * fh) & (b[:, 3] > 16 * fw)).any()       # larger than the map
    # empty bins exist: some RoI contributes nothing
    fm = E.roi_map(fh, fw, 4)
    dout = np.ones((1, 7, 7, 4), dtype=np.float32)
    assert not E.roi_pool_backward_truth(fm, b[4:5], 7, E.ROI_SCALE, dout)[1].any()
    fm = E.roi_map(fh, fw, 64)
    assert (fm == 0).mean() > 0.3 and (fm[1:3, 2:4] == 0.75).all()


# ---- softmax, BatchNorm affine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,ncls", [(5, 1), (5, 2), (301, 21), (4, 65), (5, 128)])
def test_softmax_truth_matches_torch(M, ncls):
    x, kind = E.softmax_case(M, ncls, ncls + 7)
    assert (x[:, ncls:] == np.float32(E.SOFTMAX_PAD)).all()
    xs = x[:, :ncls]
    dy = E.rng_of(M, ncls).randn(M, ncls)
    xt = torch.from_numpy(xs).double().requires_grad_(True)
    p = F.softmax(xt, dim=1)
    p.backward(torch.from_numpy(dy))
    tp, tdx = E.softmax_truth(xs, dy)
    assert np.abs(tp - p.detach().numpy()).max() <= 1e-14
    assert np.abs(tdx - xt.grad.numpy()).max() <= 1e-13 * max(np.abs(dy).max(), 1.0)
    assert (tp[np.isneginf(xs)] == 0).all()
    assert np.abs(tp[kind == 0] - 1.0 / ncls).max() <= 1e-15 if (kind == 0).any() else True
    assert np.isfinite(tp).all() and np.abs(tp.sum(axis=1) - 1).max() <= 1e-13
    if M >= 4:
        assert (np.abs(xs[kind == 1]) > 9e3).all() and np.isneginf(xs[kind == 2]).any() == (ncls >= 2)


@pytest.mark.parametrize("c", E.BN_C)
def test_bn_affine_truth_matches_torch(c):
    gamma, beta, mean, var = E.bn_case(c)
    assert var.min() <= 1e-8 * 1.001
    eps = float(np.float32(E.BN_EPS))
    tg, tb, tm = (torch.from_numpy(v).double().requires_grad_(True) for v in (gamma, beta, mean))
    tv = torch.from_numpy(var).double()
    # eval-mode BatchNorm, y = (x - mean) / sqrt(var + eps) * gamma + beta, on x = 0 and x = 1 gives shift and scale + shift;
    # the values also from F.batch_norm itself
    y0 = (0.0 - tm) / torch.sqrt(tv + eps) * tg + tb
    y1 = (1.0 - tm) / torch.sqrt(tv + eps) * tg + tb
    with torch.no_grad():
        f0 = F.batch_norm(torch.zeros((1, c), dtype=torch.float64), tm, tv, tg, tb, False, 0.0, eps)[0]
    assert float((f0 - y0.detach()).abs().max()) <= 1e-12 * float(y0.detach().abs().max())
    scale, shift, grads = E.bn_affine_truth(gamma, beta, mean, var, E.BN_EPS)
    assert np.abs(shift - y0.detach().numpy()).max() <= 1e-12 * np.abs(shift).max()
    assert np.abs(scale - (y1 - y0).detach().numpy()).max() <= 1e-11 * np.abs(scale).max()
    g_gamma, g_beta, g_mean = torch.autograd.grad(y0.sum(), (tg, tb, tm), retain_graph=True)
    assert np.abs(grads["dshift_dgamma"] - g_gamma.numpy()).max() <= 1e-12 * max(np.abs(g_gamma.numpy()).max(), 1e-30)
    assert np.abs(grads["dshift_dbeta"] - g_beta.numpy()).max() <= 1e-12
    assert np.abs(grads["dshift_dmean"] - g_mean.numpy()).max() <= 1e-12 * np.abs(g_mean.numpy()).max()
    (g_scale,) = torch.autograd.grad((y1 - y0).sum(), (tg,))
    assert np.abs(grads["dscale_dgamma"] - g_scale.numpy()).max() <= 1e-10 * np.abs(g_scale.numpy()).max()


# ---- the float32 references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,c", E.MAXPOOL_SHAPES[:5])
def test_maxpool_backward_ref_matches_torch_autograd(H, W, c):
    x, dy = E.maxpool_case(H, W, c)
    assert not np.isnan(x).any()
    xr = torch.from_numpy(x).permute(2, 0, 1).unsqueeze(0).clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(torch.from_numpy(dy).permute(2, 0, 1).unsqueeze(0))
    got = E.maxpool2x2_backward_ref(x, dy)
    assert got.dtype == np.float32 and np.array_equal(got, xr.grad[0].permute(1, 2, 0).numpy())
    if H % 2:
        assert not got[H - 1].any()
    if W % 2:
        assert not got[:, W - 1].any()
    if (H, W, c) == (2, 7, 8):
        # every tie kind is on the map, and goes to the first maximum
        assert got[0, 0, 0] == dy[0, 0, 0] and got[0, 1, 1] == dy[0, 0, 1] and got[1, 0, 2] == dy[0, 0, 2]
        assert got[0, 0, 3] == dy[0, 0, 3] and got[0, 0, 4] == dy[0, 0, 4]


@pytest.mark.parametrize("N,H,W,c", E.MEAN_SHAPES[:3])
def test_spatial_mean_backward_ref_matches_torch_autograd(N, H, W, c):
    dy = E.rng_of(N, H, W, c).randn(N, c).astype(np.float32)
    x = torch.zeros((N, c, H, W), requires_grad=True)
    x.mean(-1).mean(-1).backward(torch.from_numpy(dy))
    got = E.spatial_mean_backward_ref(dy, H, W)
    assert got.dtype == np.float32 and np.array_equal(got, x.grad.permute(0, 2, 3, 1).numpy())
    x64 = torch.zeros((N, c, H, W), dtype=torch.float64, requires_grad=True)
    x64.mean(-1).mean(-1).backward(torch.from_numpy(dy).double())
    want = x64.grad.permute(0, 2, 3, 1).numpy()
    assert (np.abs(got - want) <= 2 * E.U * np.abs(want)).all()


def test_relu_add_transpose_gather_pack_refs_match_torch():
    dy, y = E.relu_case(1025)
    yt = torch.from_numpy(y)
    assert (y[:4].view(np.int32) == np.array([0, -2 ** 31, 1, 0x7f800000], dtype=np.int64).astype(np.int32)).all()
    # torch's threshold backward: the subnormal counts as positive, -0.0 and +0.0 do not
    want = torch.where(yt > 0, torch.from_numpy(dy), torch.zeros(()))
    got = E.relu_backward_ref(dy, y)
    assert np.array_equal(got, want.numpy()) and not np.isnan(got).any() and got[2] == dy[2] and got[0] == 0 and got[1] == 0
    a, b = E.rng_of(1).randn(257).astype(np.float32), E.rng_of(2).randn(257).astype(np.float32)
    assert np.array_equal(E.add_ref(a, b), (torch.from_numpy(a) + torch.from_numpy(b)).numpy())
    x = E.rng_of(3).randn(33, 34).astype(np.float32)
    t = E.transpose_ref(x, 33, 31, 38)
    assert np.array_equal(t[:, :33], x[:, :31].T) and not t[:, 33:].any() and t.shape == (31, 38)
    src = E.rng_of(4).randn(6, 5).astype(np.float32)
    assert np.array_equal(E.gather_ref(src, np.array([5, 5, 0], dtype=np.int32)), src[[5, 5, 0]])
    # the data gradient of a convolution is the convolution of dz with the rotated, channel-transposed filter
    w = E.rng_of(5).randn(5, 3, 3, 3).astype(np.float32)                                  # [cout][cin][3][3]
    wp = np.ascontiguousarray(w.transpose(2, 3, 0, 1).reshape(9, 5, 3))                   # the forward pack [tap][co][ci]
    wrot = np.flip(w, axis=(2, 3)).transpose(1, 0, 2, 3)                                   # [cin][cout][3][3]
    assert np.array_equal(E.pack_conv3x3_dgrad_ref(wp), wrot.transpose(2, 3, 0, 1).reshape(9, 3, 5))
    assert np.array_equal(E.pack_conv_dgrad_ref(wp), w.transpose(2, 3, 1, 0).reshape(9, 3, 5))
    sc = (E.rng_of(6).rand(5) + 0.5).astype(np.float32)
    want = (torch.from_numpy(wp) * torch.from_numpy(sc).reshape(1, 5, 1)).numpy()
    assert np.array_equal(E.scale_rows_ref(wp, sc), want)
    flat = E.scale_rows_ref(wp, sc).reshape(-1)
    assert all(flat[i] == wp.reshape(-1)[i] * sc[(i // 3) % 5] for i in range(flat.size))


@pytest.mark.parametrize("momentum,wd", E.SGD_CONFIGS)
def test_sgd_ref_matches_torch_optim_in_float64(momentum, wd):
    taps, cout, cin = 9, 5, 3
    r = E.rng_of(taps, cout, cin, int(momentum * 10), int(wd * 1e4))
    w = r.randn(taps, cout, cin).astype(np.float32)
    scale = (r.rand(cout) + 0.5).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(w).double())
    opt = torch.optim.SGD([p], lr=E.SGD_LR, momentum=momentum, weight_decay=wd)
    buf = None
    for step in range(3):
        g = r.randn(taps, cout, cin).astype(np.float32)
        p.grad = torch.from_numpy(g).double()
        opt.step()
        w, buf, folded = E.sgd_ref(w, g, buf, E.SGD_LR, momentum, wd, step == 0, scale)
        assert w.dtype == np.float32 and folded.dtype == np.float32
        want = p.detach().numpy()
        # each step rounds w once (2^-24 |w|); the update's own rounding is lr times smaller
        assert np.abs(w - want).max() <= (step + 1) * 2 * E.U * np.abs(want).max(), step
        if momentum:
            wb = opt.state[p]["momentum_buffer"].numpy()
            # g + wd w, momentum buf, + g: three roundings a step, the earlier ones carried on with factor momentum
            assert np.abs(buf - wb).max() <= (step + 1) * 4 * E.U * np.abs(wb).max(), step
        else:
            assert buf is None
        wf = want * scale.astype(np.float64).reshape(1, cout, 1)
        assert np.abs(folded - wf).max() <= ((step + 1) * 2 + 1) * E.U * np.abs(wf).max()
        flat = folded.reshape(-1)
        assert all(flat[i] == w.reshape(-1)[i] * scale[(i // cin) % cout] for i in range(flat.size))


def test_mean_backward_case_tells_the_two_divisions_apart():
    N, H, W, c = E.MEAN_SHAPES[1]
    dy = E.rng_of(N, H, W, c).randn(N, c).astype(np.float32)
    one = (dy / np.float32(H * W)).astype(np.float32)
    assert not np.array_equal(E.spatial_mean_backward_ref(dy, H, W)[:, 0, 0, :], one)


# ---- FRCNN_EINVAL before the device is touched ------------------------------------------------------------------------------------------------
def test_training_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = nv.lib()
    raw = (C.c_float * 96)()
    x = (C.addressof(raw) + 63) & ~63              # a 64-byte aligned host address; none of these calls may read or write it
    big = C.c_size_t(1 << 30)
    # frcnn_rpn_loss(head, ld, cells, sample, n_sample, rpn_map, losses, d_head, stream)
    assert lib.frcnn_rpn_loss(x, 44, 35, x, 4, x, x, x, None) == EINVAL                     # ld < 45
    assert lib.frcnn_rpn_loss(x, 45, 0, x, 4, x, x, x, None) == EINVAL                      # cells < 1
    assert lib.frcnn_rpn_loss(x, 45, 35, x, -1, x, x, x, None) == EINVAL                    # n_sample < 0
    # frcnn_detector_loss(classes, deltas, onehot, gt_deltas, S, ncls, losses, d_logits, ld, stream)
    assert lib.frcnn_detector_loss(x, x, x, x, -1, 21, x, x, 128, None) == EINVAL           # S < 0
    assert lib.frcnn_detector_loss(x, x, x, x, 4, 1, x, x, 128, None) == EINVAL             # ncls < 2
    assert lib.frcnn_detector_loss(x, x, x, x, 4, 21, x, x, 100, None) == EINVAL            # ld < ncls + nd with a gradient buffer
    assert lib.frcnn_detector_loss(x, x, x, x, 4, 26, x, x, 125, None) == EINVAL
    # frcnn_roi_pool_backward(fm, fh, fw, c, rois, n, pooled, scale, dout, dfm, accumulate, ws, ws_bytes, stream)
    assert lib.frcnn_roi_pool_backward(x, 4, 4, 1025, x, 2, 7, 0.0625, x, x, 0, x, big, None) == EINVAL     # C > 1024
    assert lib.frcnn_roi_pool_backward(x, 4, 4, 8, x, 2, 0, 0.0625, x, x, 0, x, big, None) == EINVAL        # pooled 0
    assert lib.frcnn_roi_pool_backward(x, 4, 4, 8, x, 2, 8, 0.0625, x, x, 0, x, big, None) == EINVAL        # pooled 8
    need = int(lib.frcnn_roi_pool_backward_workspace_bytes(2, 7, 8))
    assert need == 2 * 49 * 8 * 4
    assert lib.frcnn_roi_pool_backward(x, 4, 4, 8, x, 2, 7, 0.0625, x, x, 0, x, need - 1, None) == EINVAL   # workspace too small
    assert lib.frcnn_roi_pool_backward(x, 4, 4, 8, x, 2, 7, 0.0625, x, x, 0, None, 0, None) == EINVAL
    # frcnn_maxpool2x2_backward(x, dy, dx, H, W, c, stream)
    assert lib.frcnn_maxpool2x2_backward(x, x, x, 1, 4, 4, None) == EINVAL                  # H < 2
    assert lib.frcnn_maxpool2x2_backward(x, x, x, 4, 1, 4, None) == EINVAL                  # W < 2
    assert lib.frcnn_maxpool2x2_backward(x, x, x, 4, 4, 6, None) == EINVAL                  # C % 4 != 0
    assert lib.frcnn_maxpool2x2_backward(x, x, x, 4, 4, 3, None) == EINVAL
    # frcnn_relu_backward(dy, y, n, stream): both pointers 16-byte aligned
    assert lib.frcnn_relu_backward(x + 4, x, 8, None) == EINVAL
    assert lib.frcnn_relu_backward(x, x + 8, 8, None) == EINVAL
    # frcnn_transpose(x, ldi, y, ldo, rows, cols, stream)
    assert lib.frcnn_transpose(x, 4, x, 8, 8, 5, None) == EINVAL                            # ldi < cols
    assert lib.frcnn_transpose(x, 8, x, 7, 8, 5, None) == EINVAL                            # ldo < rows
    # frcnn_softmax_rows(x, ldx, y, M, ncls, stream)
    assert lib.frcnn_softmax_rows(x, 128, x, 4, 0, None) == EINVAL
    assert lib.frcnn_softmax_rows(x, 256, x, 4, 129, None) == EINVAL
    assert lib.frcnn_softmax_rows(x, 20, x, 4, 21, None) == EINVAL                          # ldx < ncls
    # frcnn_sgd_step_fold(w, g, buf, n, lr, momentum, wd, first, scale, folded, cout, cin, stream)
    assert lib.frcnn_sgd_step_fold(x, x, x, 9 * 5 * 3 + 1, 1e-3, 0.9, 0.0, 1, x, x, 5, 3, None) == EINVAL   # n % (cout cin) != 0
    assert lib.frcnn_sgd_step_fold(x, x, None, 9 * 5 * 3, 1e-3, 0.9, 0.0, 1, x, x, 5, 3, None) == EINVAL    # momentum without a buffer
    # frcnn_sgd_step(w, g, buf, n, lr, momentum, wd, first, stream)
    assert lib.frcnn_sgd_step(x, x, None, 16, 1e-3, 0.9, 0.0, 1, None) == EINVAL
    # the no-ops: nothing to do, so nothing is launched
    assert lib.frcnn_relu_backward(None, None, 0, None) == 0
    assert lib.frcnn_add_inplace(None, None, 0, None) == 0
    assert lib.frcnn_gather_rows(None, None, 0, 8, None, None) == 0
    assert lib.frcnn_sgd_step(None, None, None, 0, 1e-3, 0.0, 0.0, 1, None) == 0
