"""
The torchvision-layout VGG-16 backbone (models/vgg16_torch.py, the reference's `--backbone vgg16-torch`) without a GPU: state_dict keys and
shapes against the reference model's (tests/golden/vgg16_torch_keys.json, tools/make_vgg16_torch_golden.py), preprocessing parameters,
`weights=` in torchvision's layout, torchvision's initialisation, the frozen blocks, the key remap to models/vgg16.py, checkpoint loading
and the model-level wiring that does not launch a kernel.
"""
import json
import os

import pytest
import torch

from fasterrcnn_amd import state
from fasterrcnn_amd import synthetic
from fasterrcnn_amd.datasets import image
from fasterrcnn_amd.models import vgg16, vgg16_torch
from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel


@pytest.fixture(scope="module")
def model_t():
    m = FasterRCNNModel(num_classes=21, backbone=vgg16_torch.VGG16Backbone(dropout_probability=0.0))
    m.load_state_dict(synthetic.vgg16_torch_state_dict(1234), strict=True)
    return m


@pytest.fixture(scope="module")
def model_v():
    return FasterRCNNModel(num_classes=21, backbone=vgg16.VGG16Backbone(dropout_probability=0.0))


def torchvision_state_dict(seed=5):
    """A torchvision VGG-16 state_dict (features.N / classifier.N, ImageNet head included) with distinct random tensors."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for (_, cin, cout, _), i in zip(vgg16._LAYERS, vgg16_torch.CONV_INDICES):
        sd["features.%d.weight" % i] = torch.randn((cout, cin, 3, 3), generator=g)
        sd["features.%d.bias" % i] = torch.randn((cout,), generator=g)
    for i, (n_in, n_out) in zip((0, 3, 6), ((25088, 4096), (4096, 4096), (4096, 1000))):
        sd["classifier.%d.weight" % i] = torch.randn((n_out, n_in), generator=g) * 0.01
        sd["classifier.%d.bias" % i] = torch.randn((n_out,), generator=g)
    return sd


def test_state_dict_keys_and_shapes_equal_the_reference(model_t, golden_dir):
    with open(os.path.join(golden_dir, "vgg16_torch_keys.json")) as f:
        want = [(k, list(s)) for k, s in json.load(f)]
    got = [(k, list(v.shape)) for k, v in model_t.state_dict().items()]
    assert got == want


def test_backbone_properties_and_preprocessing():
    b = vgg16_torch.VGG16Backbone(dropout_probability=0.3)
    assert (b.feature_map_channels, b.feature_pixels, b.feature_vector_size) == (512, 16, 4096)
    assert b.compute_feature_map_shape((3, 333, 517)) == (512, 20, 32)
    p = b.image_preprocessing_params
    assert p.channel_order == image.ChannelOrder.RGB
    assert p.scaling == 1.0 / 255.0
    assert p.means == [0.485, 0.456, 0.406] and p.stds == [0.229, 0.224, 0.225]
    assert vgg16.dropout_probabilities(b.pool_to_feature_vector) == (0.3, 0.3)
    layers = b.pool_to_feature_vector._layers
    assert [type(m) for m in layers] == [torch.nn.Linear, torch.nn.ReLU, torch.nn.Dropout] * 2
    assert b.pool_to_feature_vector._fc1 is layers[0] and b.pool_to_feature_vector._fc2 is layers[3]
    assert b.pool_to_feature_vector._dropout1 is layers[2] and b.pool_to_feature_vector._dropout2 is layers[5]
    feats = b.feature_extractor._layers
    assert len(feats) == 30 and not isinstance(feats[29], torch.nn.MaxPool2d)
    assert [i for i, m in enumerate(feats) if isinstance(m, torch.nn.Conv2d)] == list(vgg16_torch.CONV_INDICES)
    assert b.feature_extractor.convs() == [feats[i] for i in vgg16_torch.CONV_INDICES]


def test_first_four_convolutions_are_frozen():
    b = vgg16_torch.VGG16Backbone(dropout_probability=0.0)
    convs = b.feature_extractor.convs()
    for i, c in enumerate(convs):
        assert c.weight.requires_grad == (i >= 4) and c.bias.requires_grad == (i >= 4), i
    pv = b.pool_to_feature_vector
    assert all(p.requires_grad for p in pv.parameters())


def test_weights_none_initialises_like_torchvision(capsys):
    torch.manual_seed(0)
    b = vgg16_torch.VGG16Backbone(dropout_probability=0.0)
    assert "No IMAGENET1K_V1 weights loaded" in capsys.readouterr().out
    for c in b.feature_extractor.convs():
        cout = c.weight.shape[0]
        want = (2.0 / (cout * 9)) ** 0.5                      # Kaiming normal, fan_out, ReLU gain
        assert abs(float(c.weight.detach().std()) / want - 1) < 0.05
        assert not c.bias.any()
    for fc in (b.pool_to_feature_vector._fc1, b.pool_to_feature_vector._fc2):
        assert abs(float(fc.weight.detach().std()) / 0.01 - 1) < 0.01 and abs(float(fc.weight.detach().mean())) < 1e-4
        assert not fc.bias.any()


@pytest.mark.parametrize("as_path", [False, True])
def test_weights_in_torchvision_layout_land_in_the_right_tensors(tmp_path, as_path, capsys):
    sd = torchvision_state_dict()
    arg = sd
    if as_path:
        arg = str(tmp_path / "vgg16.pth")
        torch.save(sd, arg)
    b = vgg16_torch.VGG16Backbone(dropout_probability=0.0, weights=arg)
    assert "Loaded Torchvision VGG-16 backbone weights" in capsys.readouterr().out
    for c, i in zip(b.feature_extractor.convs(), vgg16_torch.CONV_INDICES):
        assert torch.equal(c.weight, sd["features.%d.weight" % i]) and torch.equal(c.bias, sd["features.%d.bias" % i])
    pv = b.pool_to_feature_vector
    for fc, i in ((pv._fc1, 0), (pv._fc2, 3)):
        assert torch.equal(fc.weight, sd["classifier.%d.weight" % i]) and torch.equal(fc.bias, sd["classifier.%d.bias" % i])
    # classifier.6 (the 1000-way ImageNet head) is ignored: it has no home here and nothing else took its values
    assert all(p.shape[0] != 1000 for p in list(b.feature_extractor.parameters()) + list(pv.parameters()))
    # the frozen layers stay frozen after the load
    assert not b.feature_extractor.convs()[0].weight.requires_grad and b.feature_extractor.convs()[4].weight.requires_grad


def test_weights_in_another_layout_are_refused():
    sd = torchvision_state_dict()
    with pytest.raises(KeyError):
        vgg16_torch.VGG16Backbone(dropout_probability=0.0, weights=dict(sd, **{"fc.weight": torch.zeros(1)}))
    sd.pop("features.28.bias")
    with pytest.raises(RuntimeError):
        vgg16_torch.VGG16Backbone(dropout_probability=0.0, weights=sd)


def test_key_remap_is_a_bijection_onto_vgg16_keys(model_t, model_v):
    sd_v = model_v.state_dict()
    sd_t = model_t.state_dict()
    mapped = vgg16_torch.from_vgg16_state_dict(sd_v)
    assert len(mapped) == len(sd_v) == len(sd_t)
    assert set(mapped) == set(sd_t)
    assert all(tuple(mapped[k].shape) == tuple(sd_t[k].shape) for k in sd_t)
    assert set(vgg16_torch.to_vgg16_state_dict(sd_t)) == set(sd_v)
    assert len(set(vgg16_torch.KEY_MAP.values())) == len(vgg16_torch.KEY_MAP) == 30
    back = vgg16_torch.to_vgg16_state_dict(vgg16_torch.from_vgg16_state_dict(sd_v))
    assert list(back) == list(sd_v) and all(back[k] is sd_v[k] for k in sd_v)
    # the synthetic recipe: vgg16_state_dict's tensors, the last convolution scaled for ImageNet-normalised RGB input
    sv, st = synthetic.vgg16_state_dict(1234), synthetic.vgg16_torch_state_dict(1234)
    for k, v in sv.items():
        w = st[vgg16_torch.KEY_MAP.get(k, k)]
        if k == "_stage1_feature_extractor._block5_conv3.weight":
            assert torch.equal(w, v * synthetic.VGG16_TORCH_INPUT_GAIN)
        else:
            assert torch.equal(w, v)


def test_model_treats_the_backbone_as_vgg16(model_t, model_v):
    assert not model_t._is_resnet
    assert model_t.fc_math_mode == model_v.fc_math_mode == "f32x3"
    assert model_t.math_mode == model_v.math_mode == "f32_winograd"
    for slot in (0, 1):
        assert model_t.layer_tables(slot) == model_v.layer_tables(slot)
        assert model_t.layer_forms(slot) == model_v.layer_forms(slot)
    fe_t, fe_v = model_t._stage1_feature_extractor, model_v._stage1_feature_extractor
    assert (fe_t.x6_layers, fe_t.x3_layers, fe_t.x3f_layers) == (fe_v.x6_layers, fe_v.x3_layers, fe_v.x3f_layers)
    assert [fe_t.layer_math(i) for i in range(13)] == [fe_v.layer_math(i) for i in range(13)]
    assert model_t._stage3_detector_network._pool_to_feature_vector.fc_math_mode == "f32x3"
    # (the tables only: the fixtures' state_dicts, all the other tests read, do not depend on them)
    forms = {"conv4_1": "f32x6", "conv5_3": "f32x3_one_launch"}
    model_t.set_layer_forms(forms)
    model_v.set_layer_forms(forms)
    assert model_t.layer_forms(0) == model_v.layer_forms(0) and model_t.layer_forms(1) == model_v.layer_forms(1)
    assert [fe_t.layer_math(i) for i in range(13)] == [fe_v.layer_math(i) for i in range(13)]


def test_reference_checkpoint_loads_strictly(tmp_path, model_t):
    sd = synthetic.vgg16_torch_state_dict(1234)
    sd = {k: v.clone() + 1.0 for k, v in sd.items()}
    path = str(tmp_path / "ckpt.pth")
    torch.save({"epoch": 3, "model_state_dict": sd}, path)
    m = FasterRCNNModel(num_classes=21, backbone=vgg16_torch.VGG16Backbone(dropout_probability=0.0))
    assert state.load(m, path) == []
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_caffe_layout_file_loads_into_the_torchvision_layout(tmp_path):
    sd = torchvision_state_dict(seed=9)
    path = str(tmp_path / "vgg16_caffe.pth")
    torch.save(sd, path)
    m = FasterRCNNModel(num_classes=21, backbone=vgg16_torch.VGG16Backbone(dropout_probability=0.0))
    not_loaded = state.load(m, path)
    assert all(not k.startswith(("_stage1", "_stage3_detector_network._pool_to_feature_vector")) for k in not_loaded)
    fe = m._stage1_feature_extractor
    assert torch.equal(fe._layers[28].weight, sd["features.28.weight"])
    assert torch.equal(m._stage3_detector_network._pool_to_feature_vector._layers[3].weight, sd["classifier.3.weight"])
