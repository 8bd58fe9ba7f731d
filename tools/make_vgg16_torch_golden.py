"""
tools/make_vgg16_torch_golden.py -- fixtures of the torchvision-layout VGG-16 backbone (models/vgg16_torch.py); CPU only, needs the
reference tree that oracle/reference_shims.py imports (so it runs where oracle/make_golden.py runs, never on the GPU machines).

  python tools/make_vgg16_torch_golden.py --calibrate   prints synthetic.VGG16_TORCH_INPUT_GAIN
  python tools/make_vgg16_torch_golden.py               writes
      tests/golden/vgg16_torch_keys.json           the reference vgg16-torch model's state_dict keys and shapes, in order
      tests/golden/vgg16_torch_224x320_s3.npz      forward + predict of the reference model on image_rgb(3, 224, 320)
      tests/golden/train_vgg16_torch_352x480_s6.npz  one reference train_step (the layout of train_vgg16_352x480_s4.npz)

The reference's vgg16_torch.py builds its layers from torchvision.models.vgg16(weights=IMAGENET1K_V1, dropout=p).  torchvision is not
installed and nothing is downloaded: after reference_shims.install() the stub's `vgg16` is replaced by a builder of torchvision's VGG-16
architecture written below (VGG16_Weights.IMAGENET1K_V1 is a placeholder; the weights are then loaded from
synthetic.vgg16_torch_state_dict).  Each output is cross-checked bit for bit against oracle/frcnn_oracle.py / oracle/train_oracle.py run
on the same tensors under models/vgg16.py's keys, i.e. the reference's vgg16-torch network is the reference's vgg16 network.
"""
import argparse
import json
import os
import random
import sys
import time
import types

import numpy as np
import torch as t
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import frcnn_oracle as O                                          # noqa: E402
from oracle import reference_shims                                            # noqa: E402
from oracle.make_golden import assert_equal, flatten_detections, sample_positions   # noqa: E402
from fasterrcnn_amd import synthetic                                          # noqa: E402
from fasterrcnn_amd.models import vgg16_torch as ours                         # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
_CFG_D = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


class TorchvisionVGG16(nn.Module):
    """torchvision.models.VGG with configuration "D" (features: 31 modules, avgpool, classifier: 7 modules)."""
    def __init__(self, num_classes=1000, dropout=0.5):
        super().__init__()
        layers, cin = [], 3
        for v in _CFG_D:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(p=dropout),
                                        nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(p=dropout), nn.Linear(4096, num_classes))

    def forward(self, x):
        return self.classifier(t.flatten(self.avgpool(self.features(x)), 1))


def install():
    ref = reference_shims.install(O)
    tvm = sys.modules["torchvision.models"]
    tvm.vgg16 = lambda weights=None, progress=True, **kw: TorchvisionVGG16(**kw)
    tvm.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)        # placeholder: no download, weights come from load_state_dict
    from pytorch.FasterRCNN.models import vgg16_torch                    # noqa: E402
    ref.vgg16_torch = vgg16_torch
    return ref


def build(ref, sd, dropout=0.0):
    backbone = ref.vgg16_torch.VGG16Backbone(dropout_probability=dropout)
    model = ref.faster_rcnn.FasterRCNNModel(num_classes=21, backbone=backbone, allow_edge_proposals=True)
    model.load_state_dict(sd, strict=True)
    return model


def calibrate():
    sd = synthetic.vgg16_state_dict(1234)
    with t.no_grad():
        stds = [float(O.vgg16_features(sd, img(0).unsqueeze(0)).std()) for img in (synthetic.image, synthetic.image_rgb)]
    print("VGG16_TORCH_INPUT_GAIN = %.9g" % (stds[0] / stds[1]))


def keys(ref):
    model = build(ref, synthetic.vgg16_torch_state_dict(1234))
    out = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(GOLDEN, "vgg16_torch_keys.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote tests/golden/vgg16_torch_keys.json (%d keys)" % len(out))


def forward_case(ref, tag, seed, height, width, score_threshold=0.05):
    sd = synthetic.vgg16_torch_state_dict(1234)
    img = synthetic.image_rgb(seed, height, width).unsqueeze(0)
    model = build(ref, sd).eval()
    with t.no_grad():
        props, classes, deltas = model(image_data=img)
    det = model.predict(image_data=img, score_threshold=score_threshold)
    detail = {}
    o_props, o_classes, o_deltas = O.forward(ours.to_vgg16_state_dict(sd), img, detail=detail)
    assert_equal("proposals", o_props.numpy(), props.numpy())
    assert_equal("classes", o_classes.numpy(), classes.numpy())
    assert_equal("box_deltas", o_deltas.numpy(), deltas.numpy())
    o_det = O.detections(o_props.numpy(), o_classes.numpy(), o_deltas.numpy(), height, width, score_threshold)
    assert_equal("detections", flatten_detections(o_det), flatten_detections(det))
    with t.no_grad():
        fm = model._stage1_feature_extractor(image_data=img).numpy()[0]
    print("  %d proposals, %d detections, feature map std %.3g" % (props.shape[0], sum(v.shape[0] for v in det.values()), float(fm.std())))
    out = {"seed": np.int64(seed), "height": np.int64(height), "width": np.int64(width), "allow_edge": np.int64(1),
           "score_threshold": np.float64(score_threshold), "weights_seed": np.int64(1234),
           "proposals": props.numpy(), "classes": classes.numpy(), "box_deltas": deltas.numpy(), "detections": flatten_detections(det),
           "feature_map_sample": fm[::16].copy()}
    np.savez_compressed(os.path.join(GOLDEN, "vgg16_torch_%s.npz" % tag), **out)
    print("wrote tests/golden/vgg16_torch_%s.npz" % tag)


def train_case(ref, tag, seed, height, width, lr=1e-6, momentum=0.9, weight_decay=5e-4, sample_count=2048):
    """One reference train_step (torch.optim.SGD built as __main__.py:98-105 does), checked against oracle/train_oracle.py."""
    from oracle import train_oracle as TO
    sd0 = synthetic.vgg16_torch_state_dict(1234)
    sd0_v = ours.to_vgg16_state_dict(sd0)
    img = synthetic.image_rgb(seed, height, width).unsqueeze(0)
    gts = synthetic.ground_truth(seed, height, width)
    Box = ref.training_sample.Box
    boxes = [Box(c, "x", k) for c, k in gts]
    model = build(ref, sd0)
    ishape = tuple(img.shape[1:])
    am, vm = ref.anchors.generate_anchor_maps(ishape, model.backbone.compute_feature_map_shape(ishape), 16)
    rmap, obj, bg = ref.anchors.generate_rpn_map(am, vm, boxes)
    params = [{"params": [v], "weight_decay": weight_decay} for k, v in model.named_parameters() if v.requires_grad and "weight" in k]
    optimizer = t.optim.SGD(params, lr=lr, momentum=momentum)
    keys_v = TO.trainable_weight_keys(sd0_v)
    keys = [ours.KEY_MAP.get(k, k) for k in keys_v]
    assert sorted(keys) == sorted(k for k, v in model.named_parameters() if v.requires_grad and "weight" in k)
    rng_seed = 100 + seed
    random.seed(rng_seed); t.manual_seed(rng_seed)
    rng_py, rng_t = random.getstate(), t.get_rng_state()
    t0 = time.time()
    loss = model.train_step(optimizer=optimizer, image_data=img, anchor_map=am, anchor_valid_map=vm,
                            gt_rpn_map=t.from_numpy(rmap).unsqueeze(dim=0), gt_rpn_object_indices=[obj],
                            gt_rpn_background_indices=[bg], gt_boxes=[boxes])
    print("  reference step %.1f s: %s" % (time.time() - t0, loss))
    ref_grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if k in keys}
    ref_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    random.setstate(rng_py); t.set_rng_state(rng_t)
    detail = {}
    losses, grads, new_sd, _ = TO.train_step(sd0_v, img, am, vm, t.from_numpy(rmap).unsqueeze(dim=0), obj, bg,
                                             np.stack([k for _, k in gts]).astype(np.float32), np.array([c for c, _ in gts]),
                                             21, lr, momentum, weight_decay, None, detail=detail)
    for name in ("rpn_class", "rpn_regression", "detector_class", "detector_regression", "total"):
        assert_equal("loss.%s" % name, np.float64(losses[name]), np.float64(getattr(loss, name)))
    for kv, k in zip(keys_v, keys):
        assert_equal("grad %s" % k[-36:], grads[kv].numpy(), ref_grads[k].numpy())
        assert_equal("new  %s" % k[-36:], new_sd[kv].numpy(), ref_sd[k].numpy())
    out = {"seed": np.int64(seed), "height": np.int64(height), "width": np.int64(width), "weights_seed": np.int64(1234),
           "steps": np.int64(1), "lr": np.float64(lr), "momentum": np.float64(momentum), "weight_decay": np.float64(weight_decay),
           "rng_seed": np.int64(rng_seed), "sample_count": np.int64(sample_count), "train_keys": np.array(keys),
           "s0_losses": np.array([losses[n] for n in ("rpn_class", "rpn_regression", "detector_class", "detector_regression", "total")],
                                 dtype=np.float64),
           "s0_rpn_sample_flat": detail["rpn_sample_flat"],
           "s0_proposal_sample_indices": detail["proposal_sample_indices"].astype(np.int32),
           "s0_n_rpn_proposals": np.int64(detail["rpn_proposals"].shape[0]),
           "s0_n_labelled": np.int64(detail["labelled"][0].shape[0]),
           "s0_sampled_props": detail["sampled"][0].numpy(),
           "s0_sampled_class_idx": detail["sampled"][1].numpy().argmax(axis=1).astype(np.int32)}
    for k in keys:
        g = ref_grads[k].numpy().reshape(-1).astype(np.float64)
        pos = sample_positions(g.shape[0], sample_count)
        out["s0_gnorm/" + k] = np.float64(np.sqrt((g * g).sum()))
        out["s0_gsample/" + k] = g[pos].astype(np.float32)
        dw = ref_sd[k].numpy().reshape(-1).astype(np.float64) - sd0[k].numpy().reshape(-1).astype(np.float64)
        out["s0_dwnorm/" + k] = np.float64(np.sqrt((dw * dw).sum()))
        out["s0_dwsample/" + k] = dw[pos].astype(np.float32)
    np.savez_compressed(os.path.join(GOLDEN, "train_vgg16_torch_%s.npz" % tag), **out)
    print("wrote tests/golden/train_vgg16_torch_%s.npz" % tag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calibrate", action="store_true")
    args = ap.parse_args()
    t.manual_seed(0)
    if args.calibrate:
        calibrate()
        return
    ref = install()
    keys(ref)
    forward_case(ref, "224x320_s3", 3, 224, 320)
    # (seed 4 at this size holds an RPN near-tie: one proposal more or less after NMS in a float32 run other than the reference's)
    train_case(ref, "352x480_s6", 6, 352, 480)


if __name__ == "__main__":
    main()
