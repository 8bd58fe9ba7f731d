"""
frcnn_rpn_proposals (csrc/proposals.hip) at the seams of its top-k -- keys in registers or streamed, five or six radix digits, every sort
size and emit branch, present against wanted, the filter's and the clip's thresholds -- exactly: the order, the three counts and the
proposals equal the numpy reference of tests/proposal_cases.py, which is built from the scores the kernel itself returned.  Then the
argument checks of the launcher, and frcnn_nms at the sort sizes between 1024 and 4096.  tests/test_proposals_cpu.py checks the cases and
the reference without a GPU.
"""
import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import runtime as rt
from oracle import frcnn_oracle as O
from tests import proposal_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -1
GUARD = 64              # elements behind each output that must keep their sentinel


def S():
    return nv.stream_ptr()


def gpu(x):
    return torch.as_tensor(x).to(DEV).contiguous()


@pytest.fixture(scope="module")
def pctx():
    return rt.Context(DEV, 352, 5296, 0, proposals_only=True)       # 22 x 331 cells: a_cap = 65538, room for every case


def call(pctx, c, head=None, **over):
    """One frcnn_rpn_proposals call on sentinel-filled outputs.  Returns rc, scores, sorted_idx, props, counts (numpy, guards included)."""
    i = c.inputs()
    a = dict(fh=c.fh, fw=c.fw, ld=c.ld, pre=c.pre, post=c.post)
    a.update(over)
    dh, dam = gpu(c.head() if head is None else head), gpu(i["anchors"])
    dvm = None if i["valid"] is None else gpu(i["valid"])
    scores = torch.full((c.a + GUARD,), -7.0, device=DEV)
    sidx = torch.full((c.pre + GUARD,), -1, dtype=torch.int32, device=DEV)
    props = torch.full((c.post + GUARD, 4), -1.0, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    rc = nv.lib().frcnn_rpn_proposals(pctx.handle, nv.ptr(dh), a["ld"], nv.ptr(dam), nv.ptr(dvm), a["fh"], a["fw"], c.image_h, c.image_w,
                                      a["pre"], a["post"], c.nms_thr, c.min_side, nv.ptr(scores), nv.ptr(sidx), nv.ptr(props),
                                      nv.ptr(counts), S())
    torch.cuda.synchronize()
    return rc, scores.cpu().numpy(), sidx.cpu().numpy(), props.cpu().numpy(), counts.cpu().numpy()


def check_scores(c, scores):
    """Within the 2e-7 of test_rpn_proposals_vs_oracle of the float64 sigmoid; equal logits give bit-equal scores."""
    logits = c.inputs()["logits"]
    assert (scores[c.a:] == -7.0).all()
    s = scores[:c.a]
    truth = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    assert np.abs(s.astype(np.float64) - truth).max() <= 2e-7
    o = np.argsort(logits, kind="stable")
    same = logits[o][1:] == logits[o][:-1]
    assert (s[o][1:][same] == s[o][:-1][same]).all()
    return s


def check_layout(c, r, sidx, props, counts):
    """What holds exactly in every case: order and counts against the reference, sentinels and zero rows behind them."""
    n_sel = int(counts[0])
    assert n_sel == r["n_selected"]
    assert np.array_equal(sidx[:n_sel], r["sorted_idx"])
    assert (sidx[n_sel:] == -1).all(), "sorted_idx was written past counts[0]"
    assert int(counts[1]) == r["n_after_filter"]
    n = int(counts[2])
    assert n == r["proposals"].shape[0]
    assert int(counts[3]) == 0
    assert not props[n:c.post].any(), "rows past the count must be zero"
    assert (props[c.post:] == -1.0).all(), "props was written past post_nms"
    return n


@pytest.mark.parametrize("c", P.EXACT, ids=repr)
def test_proposals_exact(pctx, c):
    rc, scores, sidx, props, counts = call(pctx, c)
    nv.check(rc, "rpn_proposals")
    s = check_scores(c, scores)
    r = c.reference(s)
    n = check_layout(c, r, sidx, props, counts)
    assert np.array_equal(props[:n], r["proposals"])
    e = c.expect
    if e.get("all_equal"):
        assert np.array_equal(sidx[:c.pre], np.arange(c.a - 1, c.a - 1 - c.pre, -1))
    if c.present == 0 or e.get("all_filtered"):
        assert counts[2] == 0 and counts[1] == 0 and not props[:c.post].any()
    if c.present == 0:
        assert counts[0] == 0


@pytest.mark.parametrize("c", P.TOLERANCE, ids=repr)
def test_proposals_with_size_deltas(pctx, c):
    """Non-zero dh / dw: expf differs from numpy's by an ulp, so the boxes get the 1e-3 px of test_rpn_proposals_vs_oracle; order and counts
    stay exact (tests/test_proposals_cpu.py: no side within 1e-2 px of min_side, no IoU near the threshold)."""
    rc, scores, sidx, props, counts = call(pctx, c)
    nv.check(rc, "rpn_proposals")
    s = check_scores(c, scores)
    r = c.reference(s)
    n = check_layout(c, r, sidx, props, counts)
    err = float(np.abs(props[:n] - r["proposals"]).max())
    print("proposals: %d, max |d| %.3g px" % (n, err))
    assert err <= 1e-3


@pytest.mark.parametrize("what,over", [
    ("A > a_cap", dict(fh=23, fw=331)), ("fh == 0", dict(fh=0)), ("fw == 0", dict(fw=0)), ("pre_nms 0", dict(pre=0)),
    ("pre_nms 16385", dict(pre=16385)), ("post_nms 0", dict(post=0)), ("post_nms 2049", dict(post=2049)), ("ld_head 44", dict(ld=44))])
def test_proposals_einval(pctx, what, over):
    """Refused by the launcher before anything is launched: no output is touched (counts are cleared by the entry point itself)."""
    c = P.BY_NAME["small_a1026_ld45"]
    head = np.zeros((23 * 331, 128), np.float32) if "fh" in over and over["fh"] else None      # (never read; sized for the call all the same)
    rc, scores, sidx, props, counts = call(pctx, c, head=head, **over)
    assert rc == EINVAL, what
    assert (scores == -7.0).all() and (sidx == -1).all() and (props == -1.0).all()
    assert (counts == 0).all()


@pytest.mark.parametrize("n", P.NMS_SORT_SIZES)
def test_nms_sort_sizes(pctx, n):
    """frcnn_nms with 1024 < n <= 4097: the LDS bitonic sort at sort_n 2048 / 4096 and the generic emit loop with per 2 / 4 (and 8192
    again just above), exact against O.nms on quantised scores -- many ties, the stable order decides."""
    boxes, scores = P.nms_sort_case(n)
    keep = torch.full((2048 + GUARD,), -1, dtype=torch.int32, device=DEV)
    nk = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    bb, ss = gpu(boxes), gpu(scores)
    nv.check(nv.lib().frcnn_nms(pctx.handle, nv.ptr(bb), nv.ptr(ss), n, 0.7, 2048, nv.ptr(keep), nv.ptr(nk), S()), "nms")
    torch.cuda.synchronize()
    ref = O.nms(boxes, scores, 0.7)[:2048].astype(np.int32)
    k = int(nk.item())
    got = keep.cpu().numpy()
    assert k == ref.shape[0] and np.array_equal(got[:k], ref)
    assert (got[k:] == -1).all()
