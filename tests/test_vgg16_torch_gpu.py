"""
The torchvision-layout VGG-16 backbone (models/vgg16_torch.py, the reference's `--backbone vgg16-torch`) on an MI355X:
  * bit identity with models/vgg16.py holding the same tensors under the remapped keys: forward, predict, predict_async slots, train_step
    with and without dropout -- the two backbones reach the same kernels through one set of packing and training code;
  * forward / predict / one train_step against the imported reference's vgg16-torch model (tests/golden/vgg16_torch_224x320_s3.npz,
    tests/golden/train_vgg16_torch_352x480_s6.npz: tools/make_vgg16_torch_golden.py), under the criteria of tests/test_model_gpu.py and
    tests/test_train_gpu.py;
  * the host path: HostFeeder's RGB / ImageNet preprocessing on the device == PIL + the reference's float32 arithmetic on the host.
"""
import os
import random

import numpy as np
import pytest
import torch

from fasterrcnn_amd import evaluate as E
from fasterrcnn_amd import synthetic
from fasterrcnn_amd import training as T
from fasterrcnn_amd.datasets.training_sample import Box
from fasterrcnn_amd.models import vgg16, vgg16_torch
from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
from oracle import frcnn_oracle as O

from test_model_gpu import GATE_PX, ROW_BOUND_PX, ROW_FRACTION_FLOOR
from test_train_gpu import canonical_grads, sample_positions

pytestmark = pytest.mark.gpu


def make_model(kind, sd_t, p=0.0):
    """kind "torch": vgg16_torch with sd_t; "vgg16": models/vgg16.py with the same tensors under its own keys."""
    if kind == "torch":
        m = FasterRCNNModel(num_classes=21, backbone=vgg16_torch.VGG16Backbone(dropout_probability=p))
        m.load_state_dict(sd_t, strict=True)
    else:
        m = FasterRCNNModel(num_classes=21, backbone=vgg16.VGG16Backbone(dropout_probability=p))
        m.load_state_dict(vgg16_torch.to_vgg16_state_dict(sd_t), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def sd_t():
    return synthetic.vgg16_torch_state_dict(1234)


@pytest.fixture(scope="module")
def models(sd_t):
    return make_model("torch", sd_t).eval(), make_model("vgg16", sd_t).eval()


def assert_same_detections(a, b):
    assert sorted(a) == sorted(b) == list(range(1, 21))
    for c in a:
        assert a[c].dtype == b[c].dtype and np.array_equal(a[c], b[c]), c


# ---- bit identity with models/vgg16.py ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,h,w", [(3, 224, 320), (0, 600, 1000)])
def test_inference_is_bit_identical_to_vgg16(models, seed, h, w):
    mt, mv = models
    img = synthetic.image_rgb(seed, h, w).unsqueeze(0).cuda()
    out_t, out_v = mt(image_data=img), mv(image_data=img)
    for a, b in zip(out_t, out_v):
        assert a.shape == b.shape and torch.equal(a, b)
    assert out_t[0].shape[0] > 0
    assert_same_detections(mt.predict(image_data=img, score_threshold=0.05), mv.predict(image_data=img, score_threshold=0.05))
    # the in-flight slots (their own streams and layer tables)
    hs = [(mt.predict_async(img, 0.05, slot=s), mv.predict_async(img, 0.05, slot=s)) for s in (1, 2)]
    for ht, hv in hs:
        assert_same_detections(ht.result(), hv.result())
    # the weight-pack caches follow the vgg16-torch parameters: a changed conv weight changes the output, restoring it restores the bits
    conv = mt._stage1_feature_extractor._layers[28]
    saved = conv.weight.detach().clone()
    with torch.no_grad():
        conv.weight.mul_(0.5)
    assert not torch.equal(mt(image_data=img)[1], out_t[1])
    with torch.no_grad():
        conv.weight.copy_(saved)
    assert torch.equal(mt(image_data=img)[1], out_t[1])


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_train_step_is_bit_identical_to_vgg16(sd_t, p):
    h, w, seed = 352, 480, 4
    img = synthetic.image_rgb(seed, h, w).unsqueeze(0).cuda()
    gts = synthetic.ground_truth(seed, h, w)
    boxes = [Box(class_index=c, class_name="x", corners=k) for c, k in gts]
    am, vm = O.generate_anchor_maps((3, h, w), (512, h // 16, w // 16), 16)
    rmap, obj, bg = O.generate_rpn_map(am, vm, np.stack([k for _, k in gts]))
    rmap = torch.from_numpy(rmap).unsqueeze(0).cuda()
    out = {}
    for kind in ("torch", "vgg16"):
        model = make_model(kind, sd_t, p)
        opt = T.create_optimizer(model, learning_rate=1e-3, momentum=0.9, weight_decay=5e-4)
        random.seed(7); torch.manual_seed(7)
        losses = [T.train_step(model, opt, img, am, vm, rmap, [obj], [bg], [boxes]) for _ in range(2)]
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        out[kind] = ([(x.rpn_class, x.rpn_regression, x.detector_class, x.detector_regression, x.total) for x in losses],
                     sd if kind == "vgg16" else vgg16_torch.to_vgg16_state_dict(sd))
        del model, opt
        torch.cuda.empty_cache()
    (lt, st), (lv, sv) = out["torch"], out["vgg16"]
    assert lt == lv and all(np.isfinite(x).all() for x in lt)
    for k in sv:
        assert torch.equal(st[k], sv[k]), k
    # the step trained the backbone (blocks 3-5 and fc1 / fc2 moved; blocks 1-2 frozen)
    assert not torch.equal(sv["_stage1_feature_extractor._block5_conv3.weight"], vgg16_torch.to_vgg16_state_dict(sd_t)[
        "_stage1_feature_extractor._block5_conv3.weight"])
    assert torch.equal(st["_stage1_feature_extractor._block2_conv2.weight"], vgg16_torch.to_vgg16_state_dict(sd_t)[
        "_stage1_feature_extractor._block2_conv2.weight"])


# ---- the imported reference's vgg16-torch model ------------------------------------------------------------------------------------
def load_case(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "vgg16_torch_%s.npz" % tag))
    img = synthetic.image_rgb(int(g["seed"]), int(g["height"]), int(g["width"])).unsqueeze(0)
    return g, img


def test_forward_matches_reference_golden(models, golden_dir):
    g, img = load_case(golden_dir, "224x320_s3")
    mt, _ = models
    props, classes, deltas = mt(image_data=img.cuda())
    assert props.shape[0] == classes.shape[0] == deltas.shape[0] == g["proposals"].shape[0]
    # row by row, in the reference's order (tests/test_model_gpu.py)
    err = np.abs(props.cpu().numpy().astype(np.float64) - g["proposals"].astype(np.float64)).max(axis=1)
    ok = err <= GATE_PX
    print("vgg16-torch forward: %d/%d proposals at their row within 1e-3 px (worst %.3g px)" % (int(ok.sum()), len(ok), err.max()))
    assert err.max() <= ROW_BOUND_PX
    assert ok.mean() >= ROW_FRACTION_FLOOR
    c_err = np.abs(classes.cpu().numpy()[ok] - g["classes"][ok]).max()
    d_err = np.abs(deltas.cpu().numpy()[ok] - g["box_deltas"][ok]).max()
    assert c_err <= 1e-4 and d_err <= 1e-3, (c_err, d_err)


def test_predict_matches_reference_golden(models, golden_dir):
    g, img = load_case(golden_dir, "224x320_s3")
    mt, _ = models
    det = mt.predict(image_data=img.cuda(), score_threshold=float(g["score_threshold"]))
    ref = g["detections"]
    n_ref, n_ok, worst = 0, 0, 0.0
    for c in range(1, 21):
        r = ref[ref[:, 0] == c][:, 1:]
        n_ref += len(r)
        if len(r) == 0:
            continue
        m = min(len(r), len(det[c]))
        err = np.full(len(r), np.inf)
        err[:m] = np.abs(det[c][:m, :4] - r[:m, :4]).max(axis=1)
        serr = np.full(len(r), np.inf)
        serr[:m] = np.abs(det[c][:m, 4] - r[:m, 4])
        n_ok += int(((err <= GATE_PX) & (serr <= 1e-4)).sum())
        worst = max(worst, float(err[:m].max()) if m else 0.0)
    n_ours = sum(len(v) for v in det.values())
    print("vgg16-torch predict: %d/%d detections at their row (ours %d, worst %.3g px)" % (n_ok, n_ref, n_ours, worst))
    assert n_ref > 0 and n_ours == n_ref and worst <= ROW_BOUND_PX
    assert n_ok >= ROW_FRACTION_FLOOR * n_ref


@pytest.mark.parametrize("math_mode", ["f32_winograd", "f32"])
def test_train_step_matches_reference_golden(sd_t, golden_dir, math_mode):
    gold = np.load(os.path.join(golden_dir, "train_vgg16_torch_352x480_s6.npz"))
    seed, h, w = int(gold["seed"]), int(gold["height"]), int(gold["width"])
    model = make_model("torch", sd_t)
    assert model.math_mode == "f32_winograd"          # the default; in it the wide forward / data-gradient convolutions are Winograd layers
    model.math_mode = math_mode
    img = synthetic.image_rgb(seed, h, w).unsqueeze(0).cuda()
    gts = synthetic.ground_truth(seed, h, w)
    boxes = [Box(class_index=c, class_name="x", corners=k) for c, k in gts]
    am, vm = O.generate_anchor_maps((3, h, w), (512, h // 16, w // 16), 16)
    rmap, obj, bg = O.generate_rpn_map(am, vm, np.stack([k for _, k in gts]))
    lr, mom, wd = float(gold["lr"]), float(gold["momentum"]), float(gold["weight_decay"])
    opt = T.create_optimizer(model, learning_rate=lr, momentum=mom, weight_decay=wd)
    keys = [str(k) for k in gold["train_keys"]]
    n_samp = int(gold["sample_count"])
    before = {k: v.clone() for k, v in model.state_dict().items()}
    random.seed(int(gold["rng_seed"])); torch.manual_seed(int(gold["rng_seed"]))
    detail = {}
    loss = T.train_step(model, opt, img, am, vm, torch.from_numpy(rmap).unsqueeze(0), [obj], [bg], [boxes], detail=detail)
    # selections: identical to the reference's (step 0 runs on identical weights)
    assert np.array_equal(detail["rpn_sample"].cpu().numpy(), gold["s0_rpn_sample_flat"])
    assert int(detail["counts"][2].item()) == int(gold["s0_n_rpn_proposals"])
    assert detail["labelled"][0].shape[0] == int(gold["s0_n_labelled"])
    assert np.array_equal(detail["sample_idx"].numpy().astype(np.int32), gold["s0_proposal_sample_indices"])
    assert np.array_equal(detail["sampled_onehot"].cpu().numpy().argmax(axis=1).astype(np.int32), gold["s0_sampled_class_idx"])
    assert np.abs(detail["sampled_props"].cpu().numpy() - gold["s0_sampled_props"]).max() <= 1e-3
    got = np.array([loss.rpn_class, loss.rpn_regression, loss.detector_class, loss.detector_regression, loss.total])
    want = gold["s0_losses"]
    assert np.all(np.abs(got - want) <= 2e-5 * np.abs(want) + 1e-7), (got, want)
    # gradients and updates under tests/test_train_gpu.py's criteria (median / L2 / norm of sampled entries), in the reference's layouts
    grads = vgg16_torch.from_vgg16_state_dict(canonical_grads(detail["grads"]))
    gscale = max(float(gold["s0_gnorm/" + k]) for k in keys)
    med_tol, l2_tol, norm_tol = 1e-4, 1e-2, 5e-3
    for k in keys:
        gk = grads[k].reshape(-1)
        pos = torch.from_numpy(sample_positions(gk.shape[0], n_samp)).to(gk.device)
        got_s = gk[pos].cpu().numpy().astype(np.float64)
        want_s = gold["s0_gsample/" + k].astype(np.float64)
        wn = float(gold["s0_gnorm/" + k])
        assert abs(float(gk.double().norm()) - wn) <= norm_tol * wn + 1e-7 * gscale, (k, "norm")
        ref_max = max(float(np.abs(want_s).max()), 1e-7 * gscale)
        d = np.abs(got_s - want_s)
        assert np.median(d) <= med_tol * ref_max, (k, "median")
        assert np.linalg.norm(got_s - want_s) <= l2_tol * max(np.linalg.norm(want_s), 1e-7 * gscale), (k, "L2")
    after = model.state_dict()
    for k in keys:
        dw = (after[k].double() - before[k].double()).reshape(-1)
        pos = torch.from_numpy(sample_positions(dw.shape[0], n_samp)).to(dw.device)
        got_s = dw[pos].cpu().numpy()
        want_s = gold["s0_dwsample/" + k].astype(np.float64)
        wn = float(gold["s0_dwnorm/" + k])
        floor = 6e-8 * float(after[k].abs().max())
        d = np.abs(got_s - want_s)
        assert np.median(d) <= med_tol * float(np.abs(want_s).max()) + 2 * floor, (k, "dw median")
        assert np.linalg.norm(got_s - want_s) <= l2_tol * np.linalg.norm(want_s) + 2 * floor * len(d) ** 0.5, (k, "dw L2")
        assert abs(float(dw.norm()) - wn) <= norm_tol * wn + floor * dw.shape[0] ** 0.5, (k, "dw norm")
    for k in before:
        if k not in keys:
            assert torch.equal(after[k], before[k]), "frozen parameter / bias changed: %s" % k
    del model, opt
    torch.cuda.empty_cache()


# ---- host path -------------------------------------------------------------------------------------------------------------------
def test_host_feeder_rgb_path_equals_pil_preprocessing(models):
    """HostFeeder.submit(rgb_u8) -> frcnn_preprocess with the backbone's RGB / 1/255 / ImageNet parameters (bgr = 0) -> predict_async ==
    predict on the image preprocessed on the host as the reference's load_image does (PIL BILINEAR resize, then datasets/image.py's
    float32 arithmetic)."""
    from PIL import Image
    mt, _ = models
    params = mt.backbone.image_preprocessing_params
    frame = synthetic.image_u8(71)                                    # 375 x 625 -> 600 x 1000
    pil = Image.fromarray(frame.numpy(), mode="RGB")
    pil = pil.resize((1000, 600), resample=Image.BILINEAR)
    data = np.array(pil).astype(np.float32)                           # RGB: no channel swap
    for c in range(3):
        data[:, :, c] *= params.scaling
    for c in range(3):
        data[:, :, c] = (data[:, :, c] - params.means[c]) / params.stds[c]
    host = torch.from_numpy(data.transpose([2, 0, 1]).copy())
    # the device preprocessing of the same frame is the host's, value for value
    from fasterrcnn_amd.datasets import image as I
    dev_img, scale, _ = I.preprocess_image(frame.numpy(), params, 600, False)
    assert abs(scale - 1.6) < 1e-12 and torch.equal(dev_img.cpu(), host)
    base = mt.predict(image_data=host.unsqueeze(0).cuda(), score_threshold=0.05)
    assert sum(len(v) for v in base.values()) > 0
    saved = mt.inflight_conv_blocks_target, mt.inflight_winograd_tile_rows, mt.inflight_x6_gemm_tiles, mt.inflight_winograd_x3f_layers
    mt.inflight_conv_blocks_target, mt.inflight_winograd_tile_rows, mt.inflight_x6_gemm_tiles = 0, 0, 0
    mt.inflight_winograd_x3f_layers = mt.alone_winograd_x3f_layers      # slot 0's table in the in-flight slot: the same bits as predict
    try:
        feeder = E.HostFeeder(mt)
        got = feeder.submit(frame.pin_memory(), 0.05, slot=1).result()
    finally:
        (mt.inflight_conv_blocks_target, mt.inflight_winograd_tile_rows, mt.inflight_x6_gemm_tiles,
         mt.inflight_winograd_x3f_layers) = saved
    assert_same_detections(got, base)
