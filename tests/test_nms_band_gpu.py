"""
The banded NMS of csrc/proposals.hip (NMS_BAND = 32 chunks of 64 boxes: phase A reduces the leading 2048 x 2048 of the mask, phase B
the whole list where `done` reads 0) through frcnn_nms and frcnn_rpn_proposals, index for index against a greedy NMS in numpy: below
the band, at its edge (2048 and 2049 boxes), the last kept box in phase A's last row and in phase B's first, forced fallbacks (also
with more than 8192 boxes), fewer survivors than max_keep, and fallback / no fallback / fallback back to back on one context.

Boxes are 20 x 20 px squares on a 32 px grid of cells, shifted by 0 / 2 / 4 / 10 px inside their cell: IoU 1, 0.818, 0.667, 0.333 or 0,
never within 1e-3 of the 0.7 threshold (asserted over every pair of distinct boxes of a case), so no case needs leaving out.
frcnn_nms bands only lists of >= 4096 boxes with max_keep <= 512 (launch_nms); frcnn_rpn_proposals every list of more than 2048.
"""
import functools

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import runtime as rt

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
THR = 0.7
BAND = 32 * 64          # boxes phase A covers
GUARD = 64


def S():
    return nv.stream_ptr()


def gpu(x):
    return torch.as_tensor(x).to(DEV).contiguous()


@pytest.fixture(scope="module")
def pctx():
    return rt.Context(DEV, 352, 5296, 0, proposals_only=True)


# ---- cases: boxes (y1, x1, y2, x2) in score order, max_keep ----------------------------------------------------------------------------
SHIFTS = (0, 2, 4, 10)


def cell_box(cell, shift=0):
    y, x = 32 * (cell // 100), 32 * (cell % 100) + shift
    return (y, x, y + 20, x + 20)


def mixture(n, cells, seed):
    """n boxes over `cells` cells, random shifts: chains of suppressed / surviving neighbours, the greedy order decides."""
    rng = np.random.RandomState(seed)
    return [cell_box(int(c), SHIFTS[int(s)]) for c, s in zip(rng.randint(0, cells, n), rng.randint(0, len(SHIFTS), n))]


def copies_then_disjoint(n_copies, n_disjoint):
    return [cell_box(0)] * n_copies + [cell_box(1 + i) for i in range(n_disjoint)]


def last_kept_at(index, max_keep, n):
    """Box 0 and its copies, then max_keep - 1 disjoint boxes that end at `index`, then disjoint boxes up to n: the max_keep-th kept box
    is box `index`."""
    lead = index + 1 - (max_keep - 1)
    return [cell_box(0)] * lead + [cell_box(1 + i) for i in range(n - lead)]


CASES = {
    # name: (boxes, max_keep)
    "below_band_n1000": (mixture(1000, 60, 1), 300),                                  # n < 64 B0, not a multiple of 64
    "below_band_n1000_keep_all": (mixture(1000, 60, 1), 2048),                        # max_keep above the survivors
    "below_band_n1999": (mixture(1999, 1500, 8), 300),                                # ... and max_keep reached below the band
    "edge_n2048": (mixture(2047, 40, 2) + [cell_box(4000)], 300),                     # exactly the band; the last box survives
    "edge_n2049": (mixture(2048, 40, 3) + [cell_box(4000)], 300),                     # one box behind the band, and it survives
    "last_row_of_phase_a": (last_kept_at(BAND - 1, 40, 4100), 40),                    # room reaches 0 at chunk B0 - 1: no fallback
    "first_row_of_phase_b": (last_kept_at(BAND, 40, 4100), 40),                       # ... one box later: fallback
    "fallback_n4100": (copies_then_disjoint(BAND, 2052), 300),
    "fallback_wide_n8300": (copies_then_disjoint(BAND, 6252), 300),                   # more than 8192 boxes: words 128 .. 255 of removed[]
    "no_fallback_n4100": (mixture(4100, 3000, 4), 300),
    "no_fallback_late_n4100": (mixture(4100, 150, 9), 300),                           # the 300th box is kept deep inside the band
    "no_fallback_wide_n8300": (mixture(8300, 3000, 5), 300),
    "survivors_short_n4100": (mixture(4100, 30, 6), 300),                             # banded, fewer survivors than max_keep
    "survivors_short_wide_n8300": (mixture(8300, 30, 7), 300),
}


def iou_matrix_row(b, rest):
    ih = np.clip(np.minimum(b[2], rest[:, 2]) - np.maximum(b[0], rest[:, 0]), 0, None)
    iw = np.clip(np.minimum(b[3], rest[:, 3]) - np.maximum(b[1], rest[:, 1]), 0, None)
    inter = ih * iw
    area = lambda q: (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    return inter / (area(b) + area(rest) - inter)


@functools.lru_cache(maxsize=None)
def case(name):
    """boxes (float64, score order), max_keep and the greedy reference's kept indices (positions in score order), computed once."""
    boxes, max_keep = CASES[name]
    b = np.asarray(boxes, np.float64)
    u = np.unique(b, axis=0)                                 # IoU depends on the two boxes alone: every pair of distinct boxes
    gap = min(float(np.abs(iou_matrix_row(q, u) - THR).min()) for q in u)
    assert gap >= 1e-3, "a pair's IoU lies within 1e-3 of the threshold: %g" % gap
    alive = np.ones(len(b), bool)
    kept = []
    for i in range(len(b)):
        if not alive[i]:
            continue
        kept.append(i)
        if len(kept) == max_keep:
            break
        alive[i + 1:] &= ~(iou_matrix_row(b[i], b[i + 1:]) > THR)
    b.setflags(write=False)
    return b, max_keep, np.asarray(kept, np.int64)


def run_nms(pctx, name):
    b, max_keep, ref = case(name)
    n = len(b)
    perm = np.random.RandomState(n).permutation(n)            # score order -> input index
    boxes = np.empty((n, 4), np.float32)
    scores = np.empty(n, np.float32)
    boxes[perm] = b
    scores[perm] = np.linspace(1.0, 0.0, n, dtype=np.float32)          # distinct: 1 / 8300 apart at the least
    keep = torch.full((max_keep + GUARD,), -1, dtype=torch.int32, device=DEV)
    nk = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    bb, ss = gpu(boxes), gpu(scores)
    nv.check(nv.lib().frcnn_nms(pctx.handle, nv.ptr(bb), nv.ptr(ss), n, THR, max_keep, nv.ptr(keep), nv.ptr(nk), S()), "nms")
    torch.cuda.synchronize()
    got, k = keep.cpu().numpy(), int(nk.item())
    assert k == len(ref)
    assert np.array_equal(got[:k], perm[ref])
    assert (got[k:] == -1).all()


def run_rpn(pctx, name):
    b, max_keep, ref = case(name)
    n = len(b)
    fw = -(-n // 9)
    A = fw * 9
    anchors = np.zeros((A, 4), np.float32)
    anchors[:, 2:] = 20.0
    anchors[:n, 0], anchors[:n, 1] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2          # cy, cx (half-integers), h = w = 20
    valid = np.zeros(A, np.float32)
    valid[:n] = 1.0
    head = np.zeros((fw, 45), np.float32)                     # zero deltas: the proposal is the anchor
    logits = np.linspace(4.0, -4.0, A, dtype=np.float32)      # anchor i is the i-th best: sigmoid keeps 8300 of them distinct
    head[:, :9] = logits.reshape(fw, 9)
    scores = torch.full((A,), -7.0, device=DEV)
    sidx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    props = torch.full((max_keep + GUARD, 4), -1.0, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    dh, da, dv = gpu(head), gpu(anchors), gpu(valid)
    nv.check(nv.lib().frcnn_rpn_proposals(pctx.handle, nv.ptr(dh), 45, nv.ptr(da), nv.ptr(dv), 1, fw, 4096, 4096, n, max_keep, THR, 16.0,
                                          nv.ptr(scores), nv.ptr(sidx), nv.ptr(props), nv.ptr(counts), S()), "rpn_proposals")
    torch.cuda.synchronize()
    s = scores.cpu().numpy()[:n]
    assert (s[1:] < s[:-1]).all(), "the test's scores must be strictly descending"
    c, p = counts.cpu().numpy(), props.cpu().numpy()
    assert c[0] == n and c[1] == n and np.array_equal(sidx.cpu().numpy(), np.arange(n))
    assert c[2] == len(ref)
    assert np.array_equal(p[:len(ref)], b[ref].astype(np.float32))
    assert not p[len(ref):max_keep].any() and (p[max_keep:] == -1.0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_nms_band(pctx, name):
    run_nms(pctx, name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rpn_proposals_band(pctx, name):
    run_rpn(pctx, name)


@pytest.mark.parametrize("run", [run_nms, run_rpn], ids=["nms", "rpn_proposals"])
def test_band_back_to_back(pctx, run):
    """One context, no call in between: a fallback leaves `done` = 1 and a whole mask behind, the list after it needs phase A alone and
    leaves phase B's tiles stale, the third must not take the stale `done` for its own nor read a stale tile."""
    for name in ("fallback_n4100", "no_fallback_n4100", "first_row_of_phase_b", "last_row_of_phase_a", "fallback_wide_n8300",
                 "no_fallback_wide_n8300", "survivors_short_n4100"):
        run(pctx, name)
