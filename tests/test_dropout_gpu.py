"""
Training-mode dropout of the VGG-16 head (reference: `--dropout p`, __main__.py:284 -> models/vgg16.py:129-133) on a real MI355X:
  * frcnn_dropout against the numpy Philox4x32-10 mirror (tests/dropout_mirror.py): masks exactly, outputs bit for bit;
  * the masks' statistics, and their independence across seeds, stream ids and ranks;
  * frcnn_dropout_relu_backward against torch CPU autograd of dropout(relu(z)) under the same mask;
  * train_step with dropout: the head's gradients against a float64 recomputation from the step's own tensors and masks, the same
    anchor / proposal samples as without dropout, determinism under torch.manual_seed, and inference left untouched.
No bitwise parity with torch's own CUDA dropout masks is claimed (a different generator): only the arithmetic x * mask * scale is torch's.
"""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import synthetic
from fasterrcnn_amd import training as T
from fasterrcnn_amd.datasets.training_sample import Box
from fasterrcnn_amd.models import vgg16 as V
from oracle import frcnn_oracle as O
from tests import dropout_mirror as DM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run_dropout(x_np, p, seed, sid, rank):
    """frcnn_dropout on a device copy of x_np -> (y, keep) as numpy arrays."""
    x = torch.from_numpy(np.ascontiguousarray(x_np, dtype=np.float32)).to(DEV)
    keep = torch.full((x.numel(),), 7, dtype=torch.uint8, device=DEV)
    s = torch.tensor([seed], dtype=torch.int64, device=DEV)
    V.dropout_(x, p, s, sid, rank, keep)
    return x.cpu().numpy(), keep.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 4, 63, 64, 65, 4097, 128 * 4096, 300 * 4096])
def test_dropout_kernel_matches_mirror(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32) * np.float32(3.0)
    x[rng.random(n) < 0.05] = np.float32(0.0)
    for seed, sid, rank in ((0, 1, 0), (-0x5DEECE66D1234567, 2, 0), (2 ** 62 + 12345, 1, 3)):
        words = DM.random_words(n, seed, sid, rank)
        u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        for p in (0.0, 0.1, 0.5, 0.9, 1.0):
            want_keep = (u < np.float32(1.0) - np.float32(p)).astype(np.uint8)
            y, keep = run_dropout(x, p, seed, sid, rank)
            assert np.array_equal(keep, want_keep), (n, seed, sid, rank, p)
            if p == 0:
                assert keep.all() and np.array_equal(y.view(np.uint32), x.view(np.uint32))
                continue
            with np.errstate(invalid="ignore"):                   # p == 1: 0 * inf on the (dropped) zeros
                want_y = np.where(want_keep.astype(bool), x * DM.scale_of(p), np.float32(0.0)).astype(np.float32)
            assert np.array_equal(y.view(np.uint32), want_y.view(np.uint32)), (n, seed, sid, rank, p)


def test_dropout_zero_length_and_p0_without_mask_are_no_ops():
    x = torch.arange(16, dtype=torch.float32, device=DEV)
    s = torch.tensor([1], dtype=torch.int64, device=DEV)
    lib = nv.lib()
    assert lib.frcnn_dropout(nv.ptr(x), 0, 0.5, 2.0, nv.ptr(s), 1, 0, None, nv.stream_ptr()) == 0
    assert lib.frcnn_dropout(nv.ptr(x), 16, 0.0, 1.0, nv.ptr(s), 1, 0, None, nv.stream_ptr()) == 0
    assert lib.frcnn_dropout_relu_backward(nv.ptr(x), nv.ptr(x), 0, 2.0, nv.stream_ptr()) == 0
    assert torch.equal(x.cpu(), torch.arange(16, dtype=torch.float32))
    assert lib.frcnn_dropout(x.data_ptr() + 4, 8, 0.5, 2.0, nv.ptr(s), 1, 0, None, nv.stream_ptr()) == -1      # not 16-byte aligned


def test_dropout_statistics_and_independence():
    n = 1 << 22
    x = np.ones(n, dtype=np.float32)
    for p in (0.1, 0.5, 0.9):
        _, k = run_dropout(x, p, 12345, 1, 0)
        frac = k.mean(dtype=np.float64)
        sigma = np.sqrt(p * (1 - p) / n)
        assert abs(frac - (1 - p)) <= 5 * sigma, (p, frac)
        q = (1 - p) ** 2 + p ** 2                           # agreement of two independent masks
        sq = np.sqrt(q * (1 - q) / n)
        for other in ((12346, 1, 0), (-12345, 1, 0), (12345, 2, 0), (12345, 1, 1)):
            _, k2 = run_dropout(x, p, *other)
            agree = (k == k2).mean(dtype=np.float64)
            assert abs(agree - q) <= 5 * sq, (p, other, agree, q)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_relu_backward_matches_torch_autograd(p):
    n = 4096 * 3 + 3
    rng = np.random.default_rng(7)
    z = rng.standard_normal(n).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e38, -3e38, 1e30, 2.5e-38, -2.5e-38], dtype=np.float32)
    z[:len(special)] = special
    z[-len(special):] = special
    z[rng.random(n) < 0.02] = np.float32(1e-42)                       # denormals
    scale = DM.scale_of(p)
    seed = 987654321
    y, keep = run_dropout(np.maximum(z, np.float32(0.0)), p, seed, 2, 0)
    assert np.array_equal(keep, DM.keep_mask(n, p, seed, 2, 0))
    dy = (rng.standard_normal(n) * 10).astype(np.float32)
    dy[:4] = np.array([0.0, -0.0, 1e-41, -7.0], dtype=np.float32)
    # torch CPU: out = dropout(relu(z)) written as torch's dropout arithmetic input * mask * scale, under the kernel's mask
    zt = torch.from_numpy(z.copy()).requires_grad_(True)
    mask = torch.from_numpy(keep.astype(np.float32))
    out = F.relu(zt) * mask * float(scale)
    assert np.array_equal(out.detach().numpy(), y)                    # the forward, value for value (signed zeros compare equal)
    out.backward(torch.from_numpy(dy))
    g = torch.from_numpy(dy.copy()).to(DEV)
    V.dropout_relu_backward_(g, torch.from_numpy(y).to(DEV), p)
    got, want = g.cpu().numpy(), zt.grad.numpy()
    assert np.isfinite(want).all() and np.array_equal(got, want)     # value for value: a dropped element is +0 here, +-0 in autograd
    kept = (y > 0)
    assert np.array_equal(got.view(np.uint32)[kept], want.view(np.uint32)[kept])


# ---- the train step ------------------------------------------------------------------------------------------
def _sample(h=600, w=1000, seed=2):
    img = synthetic.image(seed, h, w).unsqueeze(0).cuda()
    gts = synthetic.ground_truth(seed, h, w)
    boxes = [Box(class_index=c, class_name="x", corners=k) for c, k in gts]
    am, vm = O.generate_anchor_maps((3, h, w), (512, h // 16, w // 16), 16)
    rmap, obj, bg = O.generate_rpn_map(am, vm, np.stack([k for _, k in gts]))
    return img, am, vm, torch.from_numpy(rmap).unsqueeze(0).cuda(), obj, bg, boxes


def _model(sd_cpu, p, grad_math="f32"):
    from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
    model = FasterRCNNModel(num_classes=21, backbone=V.VGG16Backbone(dropout_probability=p))
    model.load_state_dict(sd_cpu, strict=True)
    model = model.cuda()
    model.grad_math = grad_math
    return model


def _step(model, opt, sample, detail=None):
    img, am, vm, rmap, obj, bg, boxes = sample
    return T.train_step(model, opt, img, am, vm, rmap, [obj], [bg], [boxes], detail=detail)


@pytest.fixture(scope="module")
def sample600():
    return _sample()


def test_train_step_head_gradients_with_dropout(sd_cpu, sample600):
    """p = 0.5: the step's masks are the mirror's for its seed (stream ids 1 / 2, rank 0), and fc1 / fc2 weight gradients, the RoI
    feature gradient and the forward h2 agree with a float64 recomputation from the step's own roi_out, masks, weights and dh2."""
    p = 0.5
    model = _model(sd_cpu, p)
    opt = T.create_optimizer(model, learning_rate=1e-6)
    random.seed(5); torch.manual_seed(5)
    detail = {}
    _step(model, opt, sample600, detail)
    seed = detail["dropout_seed"]
    keep1, keep2 = (k.cpu().numpy() for k in detail["dropout_keep"])
    roi = detail["roi_out"].cpu().double()
    S = roi.shape[0]
    assert S > 0 and keep1.shape == (S, 4096) and keep2.shape == (S, 4096)
    assert np.array_equal(keep1.reshape(-1), DM.keep_mask(S * 4096, p, seed, 1, 0))
    assert np.array_equal(keep2.reshape(-1), DM.keep_mask(S * 4096, p, seed, 2, 0))
    assert 0.45 < keep1.mean() < 0.55 and not np.array_equal(keep1, keep2)
    h1g, h2g = detail["h1"].cpu(), detail["h2"].cpu()
    assert torch.all(h1g[torch.from_numpy(keep1 == 0)] == 0) and torch.all(h2g[torch.from_numpy(keep2 == 0)] == 0)
    pv = "_stage3_detector_network._pool_to_feature_vector."
    w1 = sd_cpu[pv + "_fc1.weight"].double().reshape(4096, 512, 49).permute(0, 2, 1).reshape(4096, 49 * 512)   # (7, 7, C) order
    b1, w2, b2 = sd_cpu[pv + "_fc1.bias"].double(), sd_cpu[pv + "_fc2.weight"].double(), sd_cpu[pv + "_fc2.bias"].double()
    scale = float(DM.scale_of(p))
    # the forward with the kernel's dropout masks and float64 arithmetic
    m1, m2 = torch.from_numpy(keep1).double(), torch.from_numpy(keep2).double()
    a1 = roi @ w1.T + b1
    h2_64 = torch.relu(torch.relu(a1) * m1 * scale @ w2.T + b2) * m2 * scale
    e = float((h2g.double() - h2_64).abs().max() / h2_64.abs().max())
    assert e <= 1e-5, e
    # autograd of the head under the step's own ReLU x dropout decisions (h > 0; ReLU ties of float32 against float64 left out)
    d1, d2 = (h1g > 0).double(), (h2g > 0).double()
    assert torch.equal(d1 * m1, d1) and torch.equal(d2 * m2, d2)
    r = roi.clone().requires_grad_(True)
    W1, W2 = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    h1 = (r @ W1.T + b1) * d1 * scale
    h2 = (h1 @ W2.T + b2) * d2 * scale
    (h2 * detail["dh2"].cpu().double()).sum().backward()
    for name, got, want in (("fc1", detail["grads"]["fc1"], W1.grad), ("fc2", detail["grads"]["fc2"], W2.grad),
                            ("droi", detail["droi"], r.grad)):
        e = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print("dropout head %s: error / max|g| = %.2e" % (name, e))
        assert e <= 1e-5, (name, e)


def test_dropout_does_not_move_the_samples(sd_cpu, sample600):
    """The masks come from the device generator: the anchor (python random) and proposal (CPU torch generator) samples of a
    p = 0.5 step are those of a p = 0 step from the same seeds."""
    out = []
    for p in (0.5, 0.0):
        model = _model(sd_cpu, p)
        opt = T.create_optimizer(model, learning_rate=1e-6)
        random.seed(11); torch.manual_seed(11)
        detail = {}
        _step(model, opt, sample600, detail)
        out.append((detail["rpn_sample"].cpu().numpy(), detail["sample_idx"].numpy(), "dropout_seed" in detail))
        del model
    (r5, s5, has5), (r0, s0, has0) = out
    assert np.array_equal(r5, r0) and np.array_equal(s5, s0)
    assert has5 and not has0


@pytest.mark.parametrize("grad_math", ["f32", "bf16"])
def test_train_step_with_dropout_is_deterministic_and_learns(sd_cpu, sample600, grad_math):
    """Three p = 0.5 steps, twice from the same seeds: bit-identical losses and weights; another device seed (same samples) gives other
    fc gradients; with the masks held fixed (the device generator restored before each step) the loss falls."""
    def run(cuda_seed=None, fixed_masks=False):
        model = _model(sd_cpu, 0.5, grad_math)
        opt = T.create_optimizer(model, learning_rate=1e-6)
        random.seed(5); torch.manual_seed(5)
        if cuda_seed is not None:
            torch.cuda.manual_seed(cuda_seed)
        state = torch.cuda.get_rng_state()
        losses, first = [], {}
        for i in range(3):
            if fixed_masks:
                torch.cuda.set_rng_state(state)
            losses.append(_step(model, opt, sample600, first if i == 0 else None))
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        return losses, sd, first
    l0, s0, f0 = run()
    l1, s1, f1 = run()
    assert [x.total for x in l0] == [x.total for x in l1]
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert all(np.isfinite([x.rpn_class, x.rpn_regression, x.detector_class, x.detector_regression, x.total]).all() for x in l0)
    _, _, f2 = run(cuda_seed=99)
    assert np.array_equal(f2["sample_idx"].numpy(), f0["sample_idx"].numpy()) and f2["dropout_seed"] != f0["dropout_seed"]
    for name in ("fc1", "fc2"):
        assert not torch.equal(f2["grads"][name], f0["grads"][name]), name
    lf, _, _ = run(fixed_masks=True)
    assert lf[-1].total < lf[0].total, [x.total for x in lf]


def test_inference_is_unaffected_and_training_forward_applies_the_masks(sd_cpu):
    m0, m5 = _model(sd_cpu, 0.0).eval(), _model(sd_cpu, 0.5).eval()
    img = synthetic.image(3, 224, 320).unsqueeze(0).cuda()
    d0, d5 = m0.predict(img, 0.05), m5.predict(img, 0.05)
    assert sorted(d0) == sorted(d5) and all(np.array_equal(d0[c], d5[c]) for c in d0)
    f0, f5 = m0.forward(img), m5.forward(img)
    assert all(torch.equal(a, b) for a, b in zip(f0, f5))
    # training mode: PoolToFeatureVector.forward draws one seed from the device generator and drops after each ReLU, in every fc arithmetic
    pv = m5._stage3_detector_network._pool_to_feature_vector
    rois = torch.randn(13, 512, 7, 7, generator=torch.Generator().manual_seed(3)).cuda()
    n, scale = 13 * 4096, DM.scale_of(0.5)
    x = rois.permute(0, 2, 3, 1).contiguous().reshape(13, 49 * 512)
    for mode, fc in (("f32", V.linear), ("f32x3", V.linear_x3t)):
        m0.fc_math_mode = m5.fc_math_mode = mode
        assert torch.equal(pv(rois), m0._stage3_detector_network._pool_to_feature_vector(rois))      # eval: the identity
        pv.train()
        state = torch.cuda.get_rng_state()
        seed = int(V.draw_dropout_seed(DEV).item())
        torch.cuda.set_rng_state(state)
        y = pv(rois)
        pv.eval()
        w1p, b1, w2, b2 = pv.packed(mode)
        h1 = fc(x, w1p, b1, 4096, relu=True).cpu().numpy().reshape(-1)
        k1 = DM.keep_mask(n, 0.5, seed, 1, 0).astype(bool)
        h1 = np.where(k1, h1 * scale, np.float32(0.0)).astype(np.float32).reshape(13, 4096)
        h2 = fc(torch.from_numpy(h1).cuda(), w2, b2, 4096, relu=True).cpu().numpy().reshape(-1)
        k2 = DM.keep_mask(n, 0.5, seed, 2, 0).astype(bool)
        want = np.where(k2, h2 * scale, np.float32(0.0)).astype(np.float32).reshape(13, 4096)
        got = y.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), mode
        assert 0.4 < (got > 0).mean() / max((h2 > 0).mean(), 1e-9) < 0.6
