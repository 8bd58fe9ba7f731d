"""
frcnn_detections (csrc/detect.hip: detections_kernel) against the oracle on the families of tests/detection_cases.py: the cross-word
paths of the IoU bit matrix and the greedy pass, the rank sort, the count contract, the class stride, the float64 decode at its
overflow / clip edges and the float32 pre-filter at the edge of its domain.  These are decisions: counts, scores and row order are
compared exactly; the only tolerance is 1e-12 of the image's longer side on the box coordinates (exp's last bits).

The inputs a call may read are max_rois rows; the test puts them inside larger device buffers whose other rows hold bait (valid boxes,
scores above every threshold), so a read outside them changes the result instead of depending on what the allocator left there, and
gives the outputs a sentinel-filled tail, so a write past a class's rows or past the last class shows.
"""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from tests import detection_cases as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -4
GUARD = 512                                                      # rows of bait / sentinel past the buffers' ends (the kernel's DET_MAX)


def launch(case):
    props, classes, deltas, n, max_rois, ncls, H, W, sthr, nthr = case
    def baited(x, fill, cols=None):
        buf = torch.full((GUARD + max_rois + GUARD, cols or x.shape[1]), fill, dtype=torch.float32, device=DEV)
        view = buf.reshape(-1)[GUARD * buf.shape[1]:]                                        # the call's pointer: bait on both sides of its rows
        view[:x.size] = torch.from_numpy(x.reshape(-1)).to(DEV)
        return view
    dp = baited(props, 100.0)
    dp.reshape(-1, 4)[max_rois:] = torch.tensor([10.0, 10.0, 200.0, 300.0], device=DEV)
    dc = baited(classes, 0.999)
    dd = baited(deltas, 0.0, cols=max(deltas.shape[1], 84))                                 # (a zero tail for any class stride)
    out = torch.full(((ncls - 1) * max_rois + GUARD, 5), D.SENTINEL, dtype=torch.float64, device=DEV)
    cnt = torch.full((ncls - 1 + 8,), -1, dtype=torch.int32, device=DEV)
    nr = torch.tensor([n, 12345], dtype=torch.int32, device=DEV)
    rc = nv.lib().frcnn_detections(nv.ptr(dp), nv.ptr(dc), nv.ptr(dd), nv.ptr(nr), max_rois, ncls, H, W, sthr, nthr, nv.ptr(out),
                                   nv.ptr(cnt), nv.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), cnt.cpu().numpy()


def check_case(name, case):
    props, classes, deltas, n, max_rois, ncls, H, W, sthr, nthr = case
    rc, out, cnt = launch(case)
    nv.check(rc, "frcnn_detections")
    ref = D.reference(case)
    assert (cnt[ncls - 1:] == -1).all(), name                                               # nothing past the last class's count
    assert (out[(ncls - 1) * max_rois:] == D.SENTINEL).all(), name                         # ... or past its rows
    got = out[:(ncls - 1) * max_rois].reshape(ncls - 1, max_rois, 5)
    bar = 1e-12 * max(H, W)
    for c in range(1, ncls):
        k = ref[c].shape[0]
        assert cnt[c - 1] == k, (name, c, int(cnt[c - 1]), k)                              # every class's count is written, zeros included
        assert np.array_equal(got[c - 1, :k, 4], ref[c][:, 4]), (name, c)                  # scores, in the oracle's order
        if k:
            err = np.abs(got[c - 1, :k, :4] - ref[c][:, :4]).max()
            assert err <= bar, (name, c, err)                                               # (row order: a swapped row is far outside the bar)
        assert (got[c - 1, k:] == D.SENTINEL).all(), (name, c)                             # rows past the count are untouched
    rc2, out2, cnt2 = launch(case)
    assert rc2 == 0 and np.array_equal(out.view(np.int64), out2.view(np.int64)) and np.array_equal(cnt, cnt2), name   # bit-identical rerun


@pytest.mark.parametrize("fam,i", D.case_ids(), ids=lambda v: str(v))
def test_detections_case(fam, i):
    name, case, _ = D.family(fam)[i]
    check_case(name, case)


def test_refusals():
    """Bad shapes are FRCNN_EINVAL; an image one pixel past the limit is FRCNN_EUNSUPPORTED and writes nothing, the limit itself runs
    (the margin family's second image of every threshold is the limit)."""
    name, case, _ = D.family("classes")[2]
    for max_rois, ncls in D.REFUSALS:
        buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
        p = nv.ptr(buf)
        assert nv.lib().frcnn_detections(p, p, p, p, max_rois, ncls, 600, 1000, 0.05, 0.3, p, p, nv.stream_ptr()) == EINVAL
    for thr in (0.3, 0.7):
        lim = D.image_limit(thr)
        inside = case[:6] + (lim, lim, 0.05, thr)
        check_case("inside %g" % thr, inside)
        for H, W in ((lim + 1, 600), (600, lim + 1)):
            rc, out, cnt = launch(case[:6] + (H, W, 0.05, thr))
            assert rc == EUNSUPPORTED, (thr, H, W, rc)
            assert (out == D.SENTINEL).all() and (cnt == -1).all()
