"""
The case families of tests/box_decisions_cases.py are what they claim to be, checked with the oracle's own expressions on a machine
without a GPU: a later change to a generator cannot quietly empty a family that tests/test_box_decisions_gpu.py relies on.
"""
import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as O
from oracle import train_oracle as TO
from tests import box_decisions_cases as B

F32 = np.float32


@pytest.mark.parametrize("scale", B.NMS_SCALES)
@pytest.mark.parametrize("thr", B.NMS_THRESHOLDS)
def test_threshold_families(scale, thr):
    calls = B.threshold_calls(scale, thr)
    kinds = np.concatenate([c[2] for c in calls])
    want = {"eq": 15, "up": 15, "down": 0 if thr == 0.0 else 15, "band": 0 if thr == 0.0 else 15}
    if (scale, thr) == ("subnormal", 0.5):
        want["down"] = 0          # 0.5 - ulp (2^-25 below) is not a quotient of two subnormal areas this generator reaches
    for k, n in want.items():
        assert (kinds == k).sum() >= n, (scale, thr, k, int((kinds == k).sum()))
    thr_f = F32(thr)
    for boxes, scores, pk in calls:
        a, b = boxes[0::2], boxes[1::2]
        iou, inter, uni = B.iou_f32(a, b)
        assert np.all(iou[pk == "eq"] == thr_f)
        if thr > 0:
            assert np.all(iou[pk == "up"] == np.nextafter(thr_f, F32(1)))
            assert np.all(iou[pk == "down"] == np.nextafter(thr_f, F32(0)))
        else:
            assert np.all((iou[pk == "up"] > 0) & (iou[pk == "up"] < 1e-4))
        assert np.all(B.iou_gt_takes_division(a[pk == "band"], b[pk == "band"], thr))
        assert np.all(np.diff(scores) < 0)                                 # box 2p is processed before box 2p + 1
        # isolated: no box of one pair overlaps a box of another pair, so the oracle keeps b exactly when IoU <= thr
        keep = set(O.nms(boxes, scores, thr).tolist())
        assert all((2 * p + 1 in keep) == (not iou[p] > thr_f) for p in range(a.shape[0]))
        if scale == "subnormal":
            sa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
            assert np.all((sa > 0) & (sa < np.finfo(F32).tiny))          # areas in the float32 subnormal range


def test_threshold_dense_calls_cross_the_threshold():
    for scale in B.NMS_SCALES:
        boxes, scores = B.dense_call(scale, 0.7)
        assert boxes.shape[0] >= 900
        iou, _, _ = B.iou_f32(boxes[0::2], boxes[1::2])
        assert (iou == F32(0.7)).sum() >= 100 and (iou > F32(0.7)).sum() >= 100 and (iou < F32(0.7)).sum() >= 100


def test_inverted_boxes_are_where_iou_gt_used_to_disagree():
    """A float32 emulation of the pre-fix iou_gt (shortcuts for every union) disagrees with the oracle's division on the directed case
    and on the inverted rows of the mixed call; the fixed rule (shortcuts only for union > 0) agrees everywhere."""
    def old_rule(a, b, thr):
        _, inter, uni = B.iou_f32(a, b)
        t = F32(thr) * uni
        with np.errstate(all="ignore"):
            return np.where(inter > t * F32(1.000001), True, np.where(inter < t * F32(0.999999), False, inter / uni > F32(thr)))

    def new_rule(a, b, thr):
        _, inter, uni = B.iou_f32(a, b)
        t = F32(thr) * uni
        with np.errstate(all="ignore"):
            div = inter / uni > F32(thr)
            return np.where(uni > 0, np.where(inter > t * F32(1.000001), True, np.where(inter < t * F32(0.999999), False, div)), div)

    boxes, scores = B.degenerate_families()["issue_directed"]
    assert O.nms(boxes, scores, 0.7).tolist() == [0, 1]
    assert bool(old_rule(boxes[0], boxes[1], 0.7)) and not bool(new_rule(boxes[0], boxes[1], 0.7))
    boxes, _ = B.degenerate_mixed()
    i, j = np.triu_indices(600, 1)
    a, b = boxes[i], boxes[j]
    iou, _, _ = B.iou_f32(a, b)
    with np.errstate(invalid="ignore"):
        truth = iou > F32(0.7)
    assert (old_rule(a, b, 0.7) != truth).sum() >= 20
    assert np.array_equal(new_rule(a, b, 0.7), truth)


def test_degenerate_and_score_families():
    fam = {k: v[0] for k, v in B.degenerate_families().items()}
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert (area(fam["zero_width"]) == 0).sum() >= 2 and (area(fam["point"]) == 0).sum() >= 3
    assert (area(fam["inverted_one_axis"]) < 0).sum() >= 2 and (area(fam["inverted_both_axes"]) > 0).all()
    assert (fam["inverted_both_axes"][:, 2] < fam["inverted_both_axes"][:, 0]).sum() >= 2
    boxes, _ = B.degenerate_mixed()
    assert boxes.shape[0] == 6000
    w, h = boxes[:, 3] - boxes[:, 1], boxes[:, 2] - boxes[:, 0]
    assert ((w == 0) & (h > 0)).sum() > 300 and ((h == 0) & (w > 0)).sum() > 300 and ((w == 0) & (h == 0)).sum() > 300
    assert ((w < 0) & (h > 0)).sum() > 300 and ((w < 0) & (h < 0)).sum() > 300
    assert len({tuple(r) for r in boxes.tolist()}) < 5700                   # identical rows
    sf = B.score_families()
    s = sf["signed_zero"][1]
    assert np.signbit(s).any() and (s == 0).all()
    assert np.isnan(sf["nan"][1]).sum() == 3 and np.signbit(sf["nan"][1][np.isnan(sf["nan"][1])]).any()
    assert (np.abs(sf["subnormal"][1][sf["subnormal"][1] != 0]) < np.finfo(F32).tiny).all()
    assert O.nms(*sf["signed_zero"], 0.5).tolist() == [0]                  # the oracle: +0.0 and -0.0 tie, input order
    boxes, scores = B.isolated_score_call(sf["nan"][1])
    assert O.nms(boxes, scores, 0.5).tolist() == [1, 4, 2, 0, 3, 5]        # NaNs last, in input order


def test_detection_families():
    props, classes, n, cls_of = B.detection_case()
    kinds = B.detection_pair_classes(props, cls_of, n)
    assert kinds.count("band") >= 20 and kinds.count("margin") >= 10 and kinds.count("zero") >= 18
    assert ((classes[:n, 1:] > 0.05).sum(axis=0) == 1).any()                # a class with exactly one row
    c1 = classes[:n, 1]
    assert (np.unique(c1[c1 > 0.05], return_counts=True)[1] > 1).any()     # equal class scores


def test_rpn_families():
    for shp, fm in (((3, 600, 1000), (512, 37, 62)), ((3, 333, 517), (512, 20, 32))):
        am, vm = B.anchor_maps(shp, fm)
        cases = B.rpn_cases(am, vm)
        corners = B.anchor_corners_f64(am)
        valid = vm.reshape(-1) > 0
        for g, (a, thr, side) in zip(cases["thresholds"], B.rpn_cases.targets):
            v = B.iou_rpn(corners, g)[a]
            assert (v < thr) if side == "below" else (v >= thr)
            assert abs(v - thr) <= 1e-7 * thr, (thr, side, v)
        if shp[1] == 600:
            rmap, _, _ = O.generate_rpn_map(am, vm, cases["thresholds"])
            flags = rmap.reshape(-1, 6)[:, 0:2]
            (a_lo, _, _), (a_hi, _, _) = B.rpn_cases.targets[:2]
            assert flags[a_lo, 1] == 0 and flags[a_hi, 1] == 1                   # decided by >= 0.7, not by "best anchor of its GT"
        i0, i1 = B.iou_rpn(corners, cases["two_gt_tie"][0]), B.iou_rpn(corners, cases["two_gt_tie"][1])
        assert ((i0 == i1) & (i0 > 0.7) & valid).any()
        it = B.iou_rpn(corners, cases["anchors_tied"][0]); it[~valid] = -1
        assert (it == it.max()).sum() >= 2
        for name in ("zero_area_gt", "gt_outside", "gt_invalid_only"):
            iz = B.iou_rpn(corners, cases[name][0])
            assert iz[valid].max() == 0.0, name
        assert B.iou_rpn(corners, cases["gt_invalid_only"][0])[~valid].max() > 0


def test_label_families():
    p, gt, gt_cls = B.label_case()
    iou = B.iou_label(p, gt)
    best = iou.max(axis=1)
    assert (best == F32(0.5)).sum() >= 2 and (best == np.nextafter(F32(0.5), F32(0))).sum() == 1
    assert (best == F32(0.1)).sum() == 1 and (best == 0).sum() >= 2
    assert (iou[1] == 1).sum() == 2 and gt_cls[1] != gt_cls[2]            # identical to two duplicate GT boxes of different classes
    assert ((p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) == 0).any()
    rp, ro, rd = TO.label_proposals(torch.from_numpy(p), torch.from_numpy(gt), torch.from_numpy(gt_cls), 21, 0.0, 0.5)
    assert not torch.isfinite(rd[:, 1]).all()                              # the zero-area row's targets are inf / NaN
    assert int(ro[1].argmax()) == 9
