"""fasterrcnn_amd.ops.soft_nms on the GPU against the numpy loop of tests/soft_nms_cases.py (the contract of include/frcnn_hip.h).

naive and linear are compared bit for bit (inds and scores) with the float32 loop: at the seams of the kernel -- one wave (<= 64 boxes),
the block's thread count, the largest problem kept in LDS -- with offset 0 and 1 and thr 0.3 and 0.5, on the longest chain
(min_score = 0: every box is picked), with min_score above every score, with labels (300 of them, values negative, huge and
non-contiguous, int32 and int64; against per-label calls and against the labelled reference), and on the special cases, which the
reference mirrors: identical boxes, exact ties, NaN scores, zero-area boxes, inverted boxes, a non-contiguous view, a non-default stream,
N == 0.

gaussian runs on the cases that pass the margin rule of the cases module (float64 pick gap and min_score margin >= 1e-5): inds must equal
the float64 truth's, and err_gpu <= 4 * max(err_ref, 2**-24) must hold for the scores, both errors against the float64 truth relative to
its largest score, err_ref that of the float32 numpy loop: the convention of tests/test_ops_rot_gpu.py.  Both errors are printed.

Largest err_gpu / max(err_ref, 2**-24) measured on an MI355X over the gaussian cases below: 1.43 (n = 64, the one-wave path; 1.00 or less on
every case of more than 64 boxes), inside the margin of 4."""
import functools

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import soft_nms_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 4.0
FLOOR = 2.0 ** -24
OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor")
BLOCK = nv.lib().frcnn_ops_soft_nms_block_threads()
LDS = nv.lib().frcnn_ops_soft_nms_lds_boxes()
SEAMS = (1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3000) + ((LDS, LDS + 1) if LDS else ())


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(boxes, scores, method, offset=0, thr=S.THR, min_score=S.MIN_SCORE, labels=None):
    """(inds, final scores) of ops.soft_nms as numpy arrays; checks the shape of the result."""
    b = boxes if isinstance(boxes, torch.Tensor) else g(boxes)
    dets, inds = ops.soft_nms(b, g(scores), thr, S.SIGMA, min_score, method, offset, None if labels is None else
                              (labels if isinstance(labels, torch.Tensor) else g(labels)))
    assert dets.dtype == torch.float32 and inds.dtype == torch.int64 and dets.shape == (inds.shape[0], 5) and dets.is_cuda
    assert torch.equal(dets[:, :4], b[inds]) and not dets.requires_grad
    return inds.cpu().numpy(), dets[:, 4].cpu().numpy()


def same(got, ref):
    return np.array_equal(got[0], ref["inds"]) and np.array_equal(got[1], ref["scores"], equal_nan=True)


# ---- 1. naive and linear, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["naive", "linear"])
@pytest.mark.parametrize("n", SEAMS)
def test_naive_and_linear_bit_for_bit_at_the_seams(n, method):
    for offset in (0, 1):
        for thr in (0.3, 0.5):
            boxes, scores, ref = S.single(n, method, offset, thr)
            assert same(run(boxes, scores, method, offset, thr), ref), (n, method, offset, thr)


@pytest.mark.parametrize("method", ["naive", "linear"])
def test_min_score_zero_picks_every_box(method):
    """The longest chain: 1025 dependent picks (gaussian: in section 2, on a case that passes the margin rule)."""
    boxes, scores = S.clustered(1025, 3)
    ref = S.reference(boxes, scores, min_score=0.0, method=method)
    inds, final = run(boxes, scores, method, min_score=0.0)
    assert inds.size == 1025 and np.array_equal(np.sort(inds), np.arange(1025)) and same((inds, final), ref)


@pytest.mark.parametrize("method", ["naive", "linear", "gaussian"])
def test_min_score_above_every_score_keeps_the_first_pick_of_each_problem(method):
    boxes, scores, labels = S.labelled()
    inds, final = run(boxes[:700], scores[:700], method, min_score=2.0)
    assert inds.tolist() == [int(np.argmax(scores[:700]))] and final[0] == scores[:700].max()
    ref = S.reference(boxes, scores, min_score=2.0, method=method, labels=labels)
    got = run(boxes, scores, method, min_score=2.0, labels=labels)
    assert got[0].size == 300 and same(got, ref) and np.array_equal(got[1], scores[got[0]])


# ---- 2. gaussian against the float64 truth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,min_score", [(n, S.MIN_SCORE) for n in SEAMS] + [(1025, 0.0)])
def test_gaussian_on_the_qualifying_cases(n, min_score):
    boxes, scores, truth, seed = S.qualifying(n, "gaussian", min_score=min_score)
    ref = S.reference(boxes, scores, min_score=min_score, method="gaussian")
    inds, final = run(boxes, scores, "gaussian", min_score=min_score)
    assert np.array_equal(inds, truth["inds"]), (n, seed)
    assert min_score > 0 or inds.size == n                                  # min_score = 0: every box is picked
    scale = float(np.abs(truth["scores"]).max())
    err_gpu = float(np.abs(final.astype(np.float64) - truth["scores"]).max()) / scale
    err_ref = float(np.abs(ref["scores"].astype(np.float64) - truth["scores"]).max()) / scale
    print("gaussian n %d seed %d err_gpu %.3e err_ref %.3e ratio %.3f" % (n, seed, err_gpu, err_ref, err_gpu / max(err_ref, FLOOR)))
    assert err_gpu <= MARGIN * max(err_ref, FLOOR), (n, err_gpu, err_ref)


# ---- 3. labels ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def labelled_reference(method, small):
    boxes, scores, labels = S.labelled(small)
    return S.reference(boxes, scores, method=method, labels=labels)


@pytest.mark.parametrize("method", ["naive", "linear"])
@pytest.mark.parametrize("small", [False, True])
def test_labels_against_the_labelled_reference(small, method):
    boxes, scores, labels = S.labelled(small)
    got = run(boxes, scores, method, labels=g(labels.astype(np.int32)) if small else labels)
    assert same(got, labelled_reference(method, small))


def test_labels_equal_per_label_calls_merged():
    boxes, scores, labels = S.labelled()
    b, s = g(boxes), g(scores)
    parts = []
    for v in np.unique(labels):
        rows = np.flatnonzero(labels == v)
        dets, inds = ops.soft_nms(b[g(rows)], s[g(rows)], S.THR, S.SIGMA, S.MIN_SCORE, "linear")
        parts.append((rows[inds.cpu().numpy()], dets[:, 4].cpu().numpy()))
    inds, final = S.merged(parts)
    got = run(boxes, scores, "linear", labels=labels)
    assert np.array_equal(got[0], inds) and np.array_equal(got[1], final)


@pytest.mark.parametrize("n", [40, 700, 3000] + ([LDS + 1] if LDS else []))
def test_one_label_holding_everything_equals_no_labels(n):
    boxes, scores = S.clustered(n, 4)
    for value, dtype in ((-7, torch.int64), (2 ** 31 - 1, torch.int32), (3, torch.uint8)):
        labels = torch.full((n,), value, dtype=dtype, device=DEV)
        for method in ("linear", "gaussian"):
            a, b = run(boxes, scores, method), run(boxes, scores, method, labels=labels)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_two_long_problems_and_many_short_ones_side_by_side():
    """A label beyond the LDS bound beside one inside it and a crowd of single boxes: every path of the kernel in one launch."""
    big = (LDS or BLOCK) + 200
    boxes, scores = S.clustered(big + 1500 + 300, 5)
    labels = np.concatenate([np.full(big, 9), np.full(1500, -4), 100 + np.arange(300)]).astype(np.int64)
    perm = np.random.RandomState(0).permutation(labels.size)
    boxes, scores, labels = boxes[perm], scores[perm], labels[perm]
    for method in ("naive", "linear"):
        assert same(run(boxes, scores, method, labels=labels), S.reference(boxes, scores, method=method, labels=labels))


# ---- 4. the special cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["naive", "linear"])
@pytest.mark.parametrize("name", S.SPECIALS)
def test_special_cases_bit_for_bit(name, method):
    for n in S.SPECIAL_SIZES:
        boxes, scores, offset = S.special(name, n)
        ref = S.reference(boxes, scores, method=method, offset=offset)
        got = run(boxes, scores, method, offset)
        assert same(got, ref), (name, n)
        if name == "nan_scores":
            k = int(np.isnan(scores).sum())
            assert k > 0 and np.isnan(got[1][-k:]).all() and np.array_equal(got[0][-k:], np.flatnonzero(np.isnan(scores)))
        if name == "ties":
            order = got[0][np.argsort(-got[1], kind="stable")]
            assert np.array_equal(order, got[0])
            for v in np.unique(got[1]):
                assert np.all(np.diff(got[0][got[1] == v]) > 0)             # ascending index wins


def test_non_contiguous_boxes_non_default_stream_and_empty_input():
    boxes, scores, ref = S.single(257, "linear")
    wide = torch.zeros((257, 9), device=DEV)
    wide[:, 2:6] = g(boxes)
    view = wide[:, 2:6]
    assert not view.is_contiguous() and same(run(view, scores, "linear"), ref)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = run(boxes, scores, "linear")
    stream.synchronize()
    assert same(got, ref)
    for labels in (None, torch.empty((0,), dtype=torch.int64, device=DEV)):
        dets, inds = ops.soft_nms(torch.empty((0, 4), device=DEV), torch.empty((0,), device=DEV), labels=labels)
        assert dets.shape == (0, 5) and inds.shape == (0,) and inds.dtype == torch.int64 and dets.dtype == torch.float32


# ---- 5. consistency with nms, determinism, opcheck ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,thr", [(300, 0.3), (1000, 0.5)])
def test_naive_with_a_low_min_score_is_the_library_nms(n, thr):
    boxes, scores = S.nms_case(n, thr)
    b, s = g(boxes), g(scores)
    dets, inds = ops.soft_nms(b, s, thr, S.SIGMA, 0.01, "naive", 0)
    assert torch.equal(inds, ops.nms(b, s, thr)) and torch.equal(dets[:, 4], s[inds])
    labels = g(np.random.RandomState(1).randint(-3, 3, n).astype(np.int64))
    assert torch.equal(ops.soft_nms(b, s, thr, S.SIGMA, 0.01, "naive", 0, labels)[1], ops.batched_nms(b, s, labels, thr))


def test_two_runs_give_identical_bits():
    boxes, scores, labels = S.labelled()
    for method in ("linear", "gaussian"):
        for lab in (None, labels):
            a, b = run(boxes, scores, method, labels=lab), run(boxes, scores, method, labels=lab)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_opcheck_with_and_without_labels():
    boxes, scores = S.clustered(200, 6)
    b, s = g(boxes), g(scores)
    labels = g(np.random.RandomState(2).randint(0, 5, 200).astype(np.int64))
    torch.library.opcheck(torch.ops.frcnn.soft_nms.default, (b, s, None, 0.3, 0.5, 0.05, 1, 0), test_utils=OPCHECK)
    torch.library.opcheck(torch.ops.frcnn.soft_nms.default, (b, s, labels, 0.3, 0.5, 0.05, 2, 1), test_utils=OPCHECK)
