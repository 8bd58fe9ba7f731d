"""
The box-decision kernels at their IoU thresholds and on degenerate inputs, against the oracle, exactly (keep lists, labels, index lists):
frcnn_nms (csrc/proposals.hip: nms_keys_kernel, iou_gt), the per-class detection NMS (csrc/detect.hip), anchor labelling
(csrc/targets.hip) and proposal labelling (csrc/train.hip: label_proposals_kernel).  The inputs come from tests/box_decisions_cases.py,
whose families tests/test_box_decisions_cpu.py checks without a GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import runtime as rt
from oracle import frcnn_oracle as O
from oracle import train_oracle as TO
from tests import box_decisions_cases as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -1


def S():
    return nv.stream_ptr()


def gpu(x):
    return torch.as_tensor(x).to(DEV).contiguous()


@pytest.fixture(scope="module")
def ctx():
    return rt.Context(DEV, 608, 1008, 300)


@pytest.fixture(scope="module")
def pctx():
    return rt.Context(DEV, 608, 1008, 0, proposals_only=True)


def nms_rc(c, boxes, scores, thr, max_keep=2048):
    n = boxes.shape[0]
    keep = torch.full((2048,), -1, dtype=torch.int32, device=DEV)
    nk = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    bb = gpu(boxes) if n else torch.zeros((1, 4), device=DEV)
    ss = gpu(scores) if n else torch.zeros((1,), device=DEV)
    rc = nv.lib().frcnn_nms(c.handle, nv.ptr(bb), nv.ptr(ss), n, thr, max_keep, nv.ptr(keep), nv.ptr(nk), S())
    torch.cuda.synchronize()
    return rc, keep.cpu().numpy()[: max(int(nk.item()), 0)]


def check_nms(c, boxes, scores, thr, max_keep=2048, what=""):
    rc, got = nms_rc(c, boxes, scores, thr, max_keep)
    nv.check(rc, "nms")
    ref = O.nms(boxes, scores, thr)[:max_keep].astype(np.int32)
    assert got.shape == ref.shape and np.array_equal(got, ref), (what, got[:20], ref[:20])


# ---- 1. at the threshold ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", B.NMS_SCALES)
@pytest.mark.parametrize("thr", B.NMS_THRESHOLDS)
def test_nms_at_the_threshold(ctx, scale, thr):
    for k, (boxes, scores, _) in enumerate(B.threshold_calls(scale, thr)):
        check_nms(ctx, boxes, scores, thr, what="%s %g isolated call %d" % (scale, thr, k))
    boxes, scores = B.dense_call(scale, thr)
    check_nms(ctx, boxes, scores, thr, what="%s %g dense" % (scale, thr))


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 8191, 8193, 8300, 12000, 16384])
def test_nms_threshold_pairs_across_tiles(ctx, n):
    """Pairs at the threshold straddle 64-box tiles (off-diagonal mask words) and sit past 8192 (the upper half of removed[])."""
    fam = B.threshold_pairs("pixel", 0.7)
    a = np.concatenate([fam[k][0][:8] for k in B.KINDS]); b = np.concatenate([fam[k][1][:8] for k in B.KINDS])
    pos = [p for p in (0, 30, 63, 127, 191, 4095, 8191, 8192 + 63, 8192 + 1000, n - 2) if p + 1 < n]
    pos = sorted(set(pos))[: a.shape[0]]
    boxes, scores = B.tiled_call(n, (a, b), pos)
    check_nms(ctx, boxes, scores, 0.7, what="n %d" % n)


# ---- 2. degenerate boxes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.degenerate_families()))
@pytest.mark.parametrize("thr", [0.7, 0.3, 0.0])
def test_nms_degenerate_boxes(ctx, name, thr):
    boxes, scores = B.degenerate_families()[name]
    check_nms(ctx, boxes, scores, thr, what=name)


def test_nms_inverted_box_is_kept_as_torchvision_keeps_it(ctx):
    """(0, 10, 10, 0) 0.9 and (2, 2, 8, 8) 0.8 at 0.7: union -64, IoU 0 / -64 = -0.0, not > 0.7: both are kept."""
    boxes, scores = B.degenerate_families()["issue_directed"]
    rc, got = nms_rc(ctx, boxes, scores, 0.7)
    nv.check(rc, "nms")
    assert got.tolist() == [0, 1]


@pytest.mark.parametrize("thr", [0.7, 0.5, 0.3])
def test_nms_degenerate_boxes_mixed(ctx, thr):
    boxes, scores = B.degenerate_mixed()
    check_nms(ctx, boxes, scores, thr, what="mixed")


# ---- 3. score order -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.score_families()))
def test_nms_score_order(ctx, name):
    boxes, scores = B.score_families()[name]
    check_nms(ctx, boxes, scores, 0.5, what=name)                        # overlapping: the first in order suppresses the rest
    boxes, scores = B.isolated_score_call(scores)
    check_nms(ctx, boxes, scores, 0.5, what=name + " isolated")          # disjoint: the keep list is the whole order


def test_nms_score_order_many(ctx):
    """Every odd score in one 4000-box call over the clustered boxes."""
    rng = np.random.RandomState(5)
    boxes = B.cluster_boxes(4000, 5)
    pool = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-44, -1e-44, 0.5, 0.25], np.float32)
    scores = pool[rng.randint(0, pool.shape[0], 4000)]
    check_nms(ctx, boxes, scores, 0.5)
    boxes, scores = B.isolated_score_call(scores[:2048])
    check_nms(ctx, boxes, scores, 0.5)


# ---- 4. contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["full", "proposals"])
def test_nms_contract(ctx, pctx, which):
    c = ctx if which == "full" else pctx
    boxes = B.cluster_boxes(16385, 9)
    scores = np.random.RandomState(9).rand(16385).astype(np.float32)
    check_nms(c, boxes[:16384], scores[:16384], 0.7)
    assert nms_rc(c, boxes, scores, 0.7)[0] == EINVAL
    check_nms(c, boxes[:5000], scores[:5000], 0.7, max_keep=1)
    assert nms_rc(c, boxes[:100], scores[:100], 0.7, max_keep=0)[0] == EINVAL
    assert nms_rc(c, boxes[:100], scores[:100], 0.7, max_keep=2049)[0] == EINVAL


# ---- 5. detection NMS ---------------------------------------------------------------------------------------------------------------
def test_detections_at_the_threshold():
    props, classes, n, _ = B.detection_case()
    maxr, ncls = props.shape[0], classes.shape[1]
    deltas = np.zeros((maxr, 80), np.float32)
    out = torch.zeros((20, maxr, 5), dtype=torch.float64, device=DEV)
    cnt = torch.full((20,), -1, dtype=torch.int32, device=DEV)
    nr = torch.tensor([n], dtype=torch.int32, device=DEV)
    dp, dc, dd = gpu(props), gpu(classes), gpu(deltas)
    nv.check(nv.lib().frcnn_detections(nv.ptr(dp), nv.ptr(dc), nv.ptr(dd), nv.ptr(nr), maxr, ncls,
                                       600, 1000, 0.05, B.DET_THR, nv.ptr(out), nv.ptr(cnt), S()), "detections")
    ref = O.detections(props[:n], classes[:n], deltas[:n], 600, 1000, 0.05)
    got_cnt = cnt.cpu().numpy()
    got = out.cpu().numpy()
    for c in range(1, 21):
        k = ref[c].shape[0]
        assert got_cnt[c - 1] == k, (c, got_cnt[c - 1], k)
        if k:
            assert np.array_equal(got[c - 1, :k, 4], ref[c][:, 4])
            assert np.abs(got[c - 1, :k, :4] - ref[c][:, :4]).max() <= 1e-9
    assert got_cnt[18] == 1 and got_cnt[19] == 0


# ---- 6. anchor labelling ------------------------------------------------------------------------------------------------------------
MAPS = {"600x1000": ((3, 600, 1000), (512, 37, 62)), "ragged": ((3, 333, 517), (512, 20, 32))}
RPN_CASES = ["thresholds", "two_gt_tie", "anchors_tied", "zero_area_gt", "gt_outside", "gt_invalid_only"]


@pytest.fixture(scope="module")
def rpn_inputs():
    out = {}
    for k, (shp, fm) in MAPS.items():
        am, vm = B.anchor_maps(shp, fm)
        out[k] = (am, vm, B.rpn_cases(am, vm))
    return out


@pytest.mark.parametrize("case", RPN_CASES)
@pytest.mark.parametrize("mp", sorted(MAPS))
def test_rpn_targets_edges(rpn_inputs, mp, case):
    from fasterrcnn_amd.datasets.training_sample import Box
    from fasterrcnn_amd.models import anchors as A
    am, vm, cases = rpn_inputs[mp]
    gt = cases[case]
    rmap, obj, bg = A.generate_rpn_map(am, vm, [Box(1, "x", c) for c in gt])
    omap, oobj, obg = O.generate_rpn_map(am, vm, gt)
    assert np.array_equal(rmap[..., 0:2], omap[..., 0:2])
    assert np.array_equal(obj, oobj) and np.array_equal(bg, obg)
    assert np.array_equal(rmap[..., 2:4], omap[..., 2:4])
    lr, lo = rmap[..., 4:6], omap[..., 4:6]                             # log(0) = -inf for a zero-area GT: at the same places
    fin = np.isfinite(lo)
    assert np.array_equal(np.isfinite(lr), fin) and np.array_equal(lr[~fin], lo[~fin])
    assert np.abs(lr[fin] - lo[fin]).max() <= 1e-6


# ---- 7. proposal labelling ----------------------------------------------------------------------------------------------------------
def label_on_gpu(props, n_valid, max_props, gt, gt_cls, ncls, bg_thr, obj_thr):
    cap = max_props + gt.shape[0]
    nd = 4 * (ncls - 1)
    out_p = torch.empty((cap, 4), device=DEV)
    out_c = torch.empty((cap,), dtype=torch.int32, device=DEV)
    out_o = torch.empty((cap, ncls), device=DEV)
    out_d = torch.empty((cap, 2, nd), device=DEV)
    cnt = torch.zeros((1,), dtype=torch.int32, device=DEV)
    means = (C.c_float * 4)(0, 0, 0, 0)
    stds = (C.c_float * 4)(0.1, 0.1, 0.2, 0.2)
    dp, dn, dg, dgc = gpu(props), gpu(torch.tensor([n_valid], dtype=torch.int32)), gpu(gt), gpu(gt_cls.astype(np.int32))
    nv.check(nv.lib().frcnn_label_proposals(nv.ptr(dp), nv.ptr(dn), max_props, nv.ptr(dg), nv.ptr(dgc), gt.shape[0], ncls, bg_thr,
                                            obj_thr, means, stds, nv.ptr(out_p), nv.ptr(out_c), nv.ptr(out_o), nv.ptr(out_d),
                                            nv.ptr(cnt), S()), "label")
    k = int(cnt.item())
    return out_p[:k].cpu(), out_c[:k].cpu(), out_o[:k].cpu(), out_d[:k].cpu()


@pytest.mark.parametrize("bg_thr", [0.0, 0.1])
@pytest.mark.parametrize("clamp", [False, True])
def test_label_proposals_edges(bg_thr, clamp):
    p, gt, gt_cls = B.label_case()
    n = p.shape[0]
    max_props = n - 3 if clamp else n                                   # clamp: the device count says n, only max_props rows are read
    buf = np.vstack([p, np.full((5, 4), 7.0, np.float32)])
    got = label_on_gpu(buf[:max_props], n, max_props, gt, gt_cls, 21, bg_thr, 0.5)
    rp, ro, rd = TO.label_proposals(torch.from_numpy(p[:max_props]), torch.from_numpy(gt), torch.from_numpy(gt_cls), 21, bg_thr, 0.5)
    gp, gc, go, gd = got
    assert torch.equal(gp, rp) and torch.equal(go, ro) and torch.equal(gc.long(), ro.argmax(dim=1))
    assert torch.equal(gd[:, 0, :], rd[:, 0, :])
    for col in (0, 1):
        assert np.array_equal(gd[:, 1, col::4].numpy(), rd[:, 1, col::4].numpy(), equal_nan=True)
    fin = torch.isfinite(rd[:, 1, :])
    assert torch.equal(torch.isfinite(gd[:, 1, :]), fin)
    assert np.array_equal(gd[:, 1, :][~fin].numpy(), rd[:, 1, :][~fin].numpy(), equal_nan=True)
    if fin.any():
        assert float((gd[:, 1, :][fin] - rd[:, 1, :][fin]).abs().max()) <= 2e-6 * max(1.0, float(rd[:, 1, :][fin].abs().max()))
