"""
frcnn_predict_submit (one image enqueued natively) against the Python sequence it replaces (model.native_submit = False): the same bits on
every output, the dependency on the producer stream kept when the producer is busy and skipped when it is idle, the packed output block,
and the hipGraph path.
"""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import runtime as rt
from fasterrcnn_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r50():
    from fasterrcnn_amd.models import resnet
    from fasterrcnn_amd.models.faster_rcnn import FasterRCNNModel
    m = FasterRCNNModel(num_classes=21, backbone=resnet.ResNetBackbone(resnet.Architecture.ResNet50))
    m.load_state_dict(synthetic.resnet_state_dict(1234, "ResNet50"), strict=True)
    return m.cuda().eval()


def _slot_of(model, index):
    return model._slots[(str(model._device()), index)]


def _run(model, img, slot_index, score_threshold, native):
    """One image through slot `slot_index`; returns (result, props, classes, deltas, counts, host counts) -- clones of the slot's buffers."""
    model.native_submit = native
    try:
        if score_threshold is None:
            with torch.no_grad():
                res = model._enqueue(img, None, None, None, slot_index).result()
        else:
            res = model.predict_async(img, score_threshold, slot_index).result()
    finally:
        model.native_submit = True
    torch.cuda.synchronize()
    s = _slot_of(model, slot_index)
    return res, s.props.clone(), s.classes.clone(), s.deltas.clone(), s.counts.clone(), s.h_counts.clone()


def _same_detections(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for c in a:
        assert a[c].dtype == b[c].dtype == np.float64 and a[c].shape == b[c].shape, c
        assert np.array_equal(a[c], b[c]), c


@pytest.mark.parametrize("score_threshold", [0.05, None])
@pytest.mark.parametrize("slot_index", [0, 1, 4])
@pytest.mark.parametrize("H,W", [(600, 1000), (224, 320)])
@pytest.mark.parametrize("backbone", ["vgg16", "resnet50"])
def test_native_submit_gives_the_bits_of_the_python_sequence(gpu_model, r50, backbone, H, W, slot_index, score_threshold):
    model = gpu_model if backbone == "vgg16" else r50
    make = synthetic.image if backbone == "vgg16" else synthetic.image_rgb
    img = make(5, H, W).unsqueeze(0).cuda()
    torch.cuda.synchronize()
    py = _run(model, img, slot_index, score_threshold, native=False)
    na = _run(model, img, slot_index, score_threshold, native=True)
    for name, x, y in zip(("props", "classes", "deltas", "counts", "h_counts"), py[1:], na[1:]):
        assert torch.equal(x, y), name
    assert torch.equal(na[4].cpu(), na[5])                       # the host mirror is the device's counts
    assert int(na[4][2]) > 0
    if score_threshold is None:
        for x, y in zip(py[0], na[0]):
            assert torch.equal(x, y)
    else:
        _same_detections(py[0], na[0])
        assert sum(len(v) for v in na[0].values()) > 0


def _busy(n=6):
    """Ordinary work that keeps the current stream occupied for several milliseconds."""
    x = torch.randn(4096, 4096, device="cuda")
    for _ in range(n):
        x = (x @ x).clamp_(-1.0, 1.0)
    return x


@pytest.mark.parametrize("producer", ["default", "side"])
def test_dependency_is_taken_when_the_producer_is_busy(gpu_model, producer):
    model = gpu_model
    images = [synthetic.image(10 + i, 224, 320).unsqueeze(0).cuda() for i in range(4)]
    model.predict_async(images[0], 0.05, 1).result()                     # packs the weights, makes the slot
    torch.cuda.synchronize()
    want = [model.predict_async(im, 0.05, 1).result() for im in images]  # every image complete in memory before its submission
    torch.cuda.synchronize()
    ctx = model.context(1)
    stream = torch.cuda.Stream() if producer == "side" else torch.cuda.current_stream()
    staging = torch.zeros_like(images[0])
    for im, ref in zip(images, want):
        staging.zero_()
        torch.cuda.synchronize()
        taken0, skipped0 = ctx.submit_stats()
        with torch.cuda.stream(stream):
            keep = _busy()
            staging.copy_(im)                                            # the image is produced BEHIND the busy work, on the producer stream
            pending = model.predict_async(staging, 0.05, 1)
        got = pending.result()
        taken1, skipped1 = ctx.submit_stats()
        assert (taken1 - taken0, skipped1 - skipped0) == (1, 0)
        _same_detections(ref, got)
        del keep
    torch.cuda.synchronize()


def test_dependency_is_skipped_when_the_producer_is_idle(gpu_model):
    model = gpu_model
    img = synthetic.image(3, 224, 320).unsqueeze(0).cuda()
    ref = model.predict_async(img, 0.05, 2).result()
    ctx = model.context(2)
    for _ in range(3):
        torch.cuda.synchronize()
        taken0, skipped0 = ctx.submit_stats()
        got = model.predict_async(img, 0.05, 2).result()
        taken1, skipped1 = ctx.submit_stats()
        assert (taken1 - taken0, skipped1 - skipped0) == (0, 1)
        _same_detections(ref, got)
    # slot 0 runs on the caller's stream: there is no second stream to order, nothing is counted
    model.predict_async(img, 0.05, 0).result()
    t0 = model.context(0).submit_stats()
    _same_detections(ref, model.predict_async(img, 0.05, 0).result())
    assert model.context(0).submit_stats() == t0


def test_packed_block_views_on_the_device(gpu_model):
    model = gpu_model
    img = synthetic.image(3, 224, 320).unsqueeze(0).cuda()
    res = model.predict_async(img, 0.05, 3).result()
    torch.cuda.synchronize()
    s = _slot_of(model, 3)
    nfg, R = s.num_classes - 1, s.max_rois
    o_counts, o_cnt, o_det, total = nv.output_block_layout(R, s.num_classes)
    assert s.block.numel() == s.h_block.numel() == total and s.h_block.is_pinned()
    for dev_t, host_t, shape, dtype, off in ((s.counts, s.h_counts, (4,), torch.int32, o_counts), (s.det_cnt, s.h_det_cnt, (nfg,), torch.int32, o_cnt),
                                            (s.det, s.h_det, (nfg, R, 5), torch.float64, o_det)):
        assert tuple(dev_t.shape) == tuple(host_t.shape) == shape and dev_t.dtype == host_t.dtype == dtype
        assert dev_t.data_ptr() == s.block.data_ptr() + off and host_t.data_ptr() == s.h_block.data_ptr() + off
        assert dev_t.data_ptr() % 16 == 0 and host_t.data_ptr() % 16 == 0
        assert torch.equal(dev_t.cpu(), host_t)                          # one copy brought all three regions
    assert torch.equal(s.block.cpu(), s.h_block)
    for c in range(nfg):
        assert np.array_equal(res[c + 1], s.h_det.numpy()[c, : int(s.h_det_cnt[c])])


def test_slot_streams_do_not_share_a_queue_with_each_other_when_avoidable(gpu_model):
    """runtime.slot_stream passes over streams that landed on another slot's hardware queue.  With as many queues as slots (the default
    stream included in neither count) every pair of slot streams must be apart; the default stream may share with one of them."""
    import os
    dev = gpu_model._device()
    streams = [rt.slot_stream(dev, i) for i in range(1, 5)]
    q = int(os.environ.get("GPU_MAX_HW_QUEUES") or 4)
    n = min(len(streams), q)
    for i in range(n):
        for j in range(i + 1, n):
            assert not rt.streams_share_queue(streams[i], streams[j]), (i + 1, j + 1)
    torch.cuda.synchronize()


def test_hip_graph_path_equals_eager_on_the_golden_image(gpu_model):
    model = gpu_model
    img = synthetic.image(3, 224, 320).unsqueeze(0).cuda()
    torch.cuda.synchronize()
    eager = model.predict_async(img, 0.05, 1).result()
    assert sum(len(v) for v in eager.values()) > 0
    model.use_hip_graphs = True
    try:
        # first call eager (remembers the key), second captures and replays, third replays
        for _ in range(3):
            _same_detections(eager, model.predict_async(img, 0.05, 1).result())
        assert _slot_of(model, 1).graph is not None
    finally:
        model.use_hip_graphs = False
        torch.cuda.synchronize()
    _same_detections(eager, model.predict_async(img, 0.05, 1).result())


@pytest.mark.parametrize("native", [True, False])
def test_hip_graph_replay_behind_a_busy_producer(gpu_model, native):
    model = gpu_model
    img = synthetic.image(3, 224, 320).unsqueeze(0).cuda()
    torch.cuda.synchronize()
    eager = model.predict_async(img, 0.05, 1).result()
    model.use_hip_graphs, model.native_submit = True, native
    try:
        for _ in range(3):
            _same_detections(eager, model.predict_async(img, 0.05, 1).result())
        assert _slot_of(model, 1).graph is not None
        staging = torch.zeros_like(img)
        torch.cuda.synchronize()
        t0 = model.context(1).submit_stats()
        keep = _busy()
        staging.copy_(img)
        got = model.predict_async(staging, 0.05, 1).result()
        print("native", native, "stats", t0, model.context(1).submit_stats(), "rows", sum(len(v) for v in got.values()))
        _same_detections(eager, got)
        del keep
    finally:
        model.use_hip_graphs, model.native_submit = False, True
        torch.cuda.synchronize()
