"""
Torchvision-layout VGG-16 backbone, mirroring pytorch/FasterRCNN/models/vgg16_torch.py: same class names, same module layout (->
identical state_dict keys: `_stage1_feature_extractor._layers.{0,2,5,...,28}.{weight,bias}` -- torchvision's `features[0:-1]` --
and `_stage3_detector_network._pool_to_feature_vector._layers.{0,3}.{weight,bias}` -- `classifier[0:-1]`), same Backbone properties
(RGB input scaled by 1/255 and normalised with the ImageNet mean / std).

The network is the one of models/vgg16.py -- the same 13 convolutions, four 2x2 pools, fc1 / fc2 with ReLU and dropout, blocks 1-2
frozen -- so the stage modules here are subclasses of vgg16.FeatureExtractor / vgg16.PoolToFeatureVector that only hold their
parameters in torchvision's layout: packing, the HIP forward, dropout and the train step are vgg16.py's, reached through convs() and
the _fc1 / _fc2 / _dropout1 / _dropout2 accessors.  FasterRCNNModel treats this backbone as VGG-16 everywhere.

The reference downloads torchvision's IMAGENET1K_V1 weights in the constructor.  Nothing is downloaded here: `weights=` takes a path
or a state_dict in torchvision's own VGG-16 layout (`features.N.*`, `classifier.{0,3}.*`; the 1000-way `classifier.6` is ignored),
and without it the layers are initialised as torchvision's VGG initialises them.
"""
import os

import torch as t
from torch import nn

from ..datasets import image
from . import vgg16

# torchvision's vgg16().features indices of the 13 convolutions (vgg16._LAYERS order) and classifier indices of fc1 / fc2
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
FC_INDICES = (0, 3)
_POOL_INDICES = (4, 9, 16, 23)       # (and 30, the final pool the reference drops)


def _features():
    """torchvision's VGG-16 `features[0:-1]`: Conv2d(3x3, padding 1) + ReLU per layer, MaxPool2d(2, 2) after blocks 1-4 (30 modules)."""
    layers = []
    for _, cin, cout, pool in vgg16._LAYERS:
        layers += [nn.Conv2d(cin, cout, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
        if pool:
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    seq = nn.Sequential(*layers)
    assert len(seq) == 30 and all(isinstance(seq[i], nn.Conv2d) for i in CONV_INDICES)
    assert all(isinstance(seq[i], nn.MaxPool2d) for i in _POOL_INDICES)
    return seq


class FeatureExtractor(vgg16.FeatureExtractor):
    """vgg16.FeatureExtractor over torchvision's module layout: the 13 convolutions live in `_layers` (the first four frozen)."""
    def _make_layers(self):
        self._layers = _features()

    def convs(self):
        return [self._layers[i] for i in CONV_INDICES]


class PoolToFeatureVector(vgg16.PoolToFeatureVector):
    """vgg16.PoolToFeatureVector over torchvision's `classifier[0:-1]`: Linear(25088, 4096), ReLU, Dropout(p), Linear(4096, 4096), ReLU,
    Dropout(p).  RoIs are flattened in (C, 7, 7) order, as vgg16_torch.py does."""
    def _make_layers(self, dropout_probability):
        self._layers = nn.Sequential(nn.Linear(512 * 7 * 7, 4096), nn.ReLU(inplace=True), nn.Dropout(p=dropout_probability),
                                     nn.Linear(4096, 4096), nn.ReLU(inplace=True), nn.Dropout(p=dropout_probability))

    # the names vgg16.PoolToFeatureVector, vgg16.dropout_probabilities and the train step read
    _fc1 = property(lambda self: self._layers[0])
    _fc2 = property(lambda self: self._layers[3])
    _dropout1 = property(lambda self: self._layers[2])
    _dropout2 = property(lambda self: self._layers[5])


class VGG16Backbone(vgg16.VGG16Backbone):
    _feature_extractor_class = FeatureExtractor
    _pool_to_feature_vector_class = PoolToFeatureVector

    def __init__(self, dropout_probability, weights=None):
        """weights: None (torchvision's initialisation), or a path / state_dict of torchvision's VGG-16 (`features.N.*`, `classifier.N.*`)."""
        super().__init__(dropout_probability)
        # Image pre-processing parameters of torchvision's VGG16_Weights.IMAGENET1K_V1 (vgg16_torch.py)
        self.image_preprocessing_params = image.PreprocessingParams(
            channel_order=image.ChannelOrder.RGB, scaling=1.0 / 255.0, means=[0.485, 0.456, 0.406], stds=[0.229, 0.224, 0.225])
        if weights is None:
            init_like_torchvision(self)
            print("No IMAGENET1K_V1 weights loaded for Torchvision VGG-16 backbone (weights=None): layers initialised as torchvision's VGG")
        else:
            load_torchvision_weights(self, weights)
            print("Loaded Torchvision VGG-16 backbone weights%s" % (" from '%s'" % weights if isinstance(weights, (str, os.PathLike)) else ""))


def init_like_torchvision(backbone):
    """torchvision.models.VGG's initialisation: convolutions Kaiming-normal (fan_out, ReLU) with zero bias, linear layers N(0, 0.01) with
    zero bias."""
    with t.no_grad():
        for conv in backbone.feature_extractor.convs():
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            nn.init.zeros_(conv.bias)
        pv = backbone.pool_to_feature_vector
        for fc in (pv._fc1, pv._fc2):
            nn.init.normal_(fc.weight, 0.0, 0.01)
            nn.init.zeros_(fc.bias)


def load_torchvision_weights(backbone, weights):
    """Copies a torchvision VGG-16 state_dict (or a file holding one) into the backbone: `features.N.*` into the feature extractor's
    `_layers`, `classifier.0.*` / `classifier.3.*` into fc1 / fc2; `classifier.6.*` (the ImageNet classifier) is ignored.  Every other key,
    a missing key or a shape mismatch raises."""
    sd = t.load(weights, map_location="cpu", weights_only=True) if isinstance(weights, (str, os.PathLike)) else weights
    features, classifier, other = {}, {}, []
    for k, v in sd.items():
        if k.startswith("features."):
            features[k[len("features."):]] = v
        elif k.startswith("classifier.6."):
            continue
        elif k.startswith("classifier."):
            classifier[k[len("classifier."):]] = v
        else:
            other.append(k)
    if other:
        raise KeyError("not a torchvision VGG-16 state_dict: unexpected keys %s" % other[:4])
    with t.no_grad():
        backbone.feature_extractor._layers.load_state_dict(features, strict=True)
        backbone.pool_to_feature_vector._layers.load_state_dict(classifier, strict=True)


def _key_map():
    """{models/vgg16.py model key: vgg16-torch model key} of the 30 backbone tensors (the RPN and detector heads share their keys)."""
    out = {}
    for (name, _, _, _), i in zip(vgg16._LAYERS, CONV_INDICES):
        for p in ("weight", "bias"):
            out["_stage1_feature_extractor.%s.%s" % (name, p)] = "_stage1_feature_extractor._layers.%d.%s" % (i, p)
    for name, i in zip(("_fc1", "_fc2"), FC_INDICES):
        for p in ("weight", "bias"):
            out["_stage3_detector_network._pool_to_feature_vector.%s.%s" % (name, p)] = \
                "_stage3_detector_network._pool_to_feature_vector._layers.%d.%s" % (i, p)
    return out


KEY_MAP = _key_map()
_INVERSE_KEY_MAP = {v: k for k, v in KEY_MAP.items()}


def from_vgg16_state_dict(sd):
    """A models/vgg16.py FasterRCNNModel state_dict -> the same tensors under this backbone's keys (other keys unchanged)."""
    return {KEY_MAP.get(k, k): v for k, v in sd.items()}


def to_vgg16_state_dict(sd):
    """Inverse of from_vgg16_state_dict."""
    return {_INVERSE_KEY_MAP.get(k, k): v for k, v in sd.items()}
