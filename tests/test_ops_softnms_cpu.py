"""fasterrcnn_amd.ops.soft_nms / soft_nms_pytorch without a GPU: names and documents, the header / SYMBOLS / library agreement and the
ABI number, the validation of the C entry point, every TypeError and ValueError of the wrappers on meta and CPU tensors, the known
answer, soft_nms_pytorch against the numpy loop of tests/soft_nms_cases.py, and the conditions on the inputs that the GPU tests rely on
(the kept fraction of the clustered cases, the margin rule of the cases compared against float64).

soft_nms_pytorch runs the contract's operations one by one in the same order as the numpy loop, so naive and linear agree with it bit for
bit in float32 and in float64; for gaussian the two exponentials (torch's and numpy's) may differ by an ulp, so the scores are held to
4 * max(err_ref, eps) against the float64 truth, err_ref the float32 numpy loop's error -- the bound of the GPU test."""
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import soft_nms_cases as S

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("soft_nms", "soft_nms_pytorch")
ENTRY_POINTS = {"frcnn_ops_soft_nms", "frcnn_ops_soft_nms_workspace_bytes", "frcnn_ops_soft_nms_block_threads",
                "frcnn_ops_soft_nms_lds_boxes", "frcnn_ops_soft_nms_max_boxes"}
BLOCK = nv.lib().frcnn_ops_soft_nms_block_threads()
LDS = nv.lib().frcnn_ops_soft_nms_lds_boxes()
SEAMS = (1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1025, 3000) + ((LDS, LDS + 1) if LDS else ())


def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, truth):
    return float(np.abs(np.asarray(got, dtype=np.float64) - truth).max() / np.abs(truth).max())


# ---- 1. names, documents, ABI -----------------------------------------------------------------------------------------------------------
def test_names_are_exported_and_documented():
    for name in NAMES:
        assert name in ops.__all__ and callable(getattr(ops, name)) and name in ops.__doc__ and getattr(ops, name).__doc__
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "soft_nms" in open(os.path.join(ROOT, doc)).read(), doc
    assert "MAX_SOFT_NMS_BOXES" in ops.__doc__ and ops.MAX_SOFT_NMS_BOXES == 65536 == nv.lib().frcnn_ops_soft_nms_max_boxes()
    assert "from mmcv.ops import soft_nms" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_abi_number_and_the_entry_points():
    text = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert re.search(r"#define FRCNN_ABI_VERSION (\d+)", text).group(1) == "21"
    assert nv.ABI_VERSION == 21 == nv.lib().frcnn_abi_version()
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert ENTRY_POINTS <= declared and declared == set(nv.SYMBOLS)
    assert {s for s in nv.SYMBOLS if "soft_nms" in s} == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(nv.lib(), name), name
    assert BLOCK % 64 == 0 and 64 < BLOCK <= 1024 and (LDS == 0 or (LDS > BLOCK and LDS < ops.MAX_SOFT_NMS_BOXES))
    assert "ops_softnms.hip" in open(os.path.join(ROOT, "fasterrcnn_amd", "csrc", "Makefile")).read()


# ---- 2. FRCNN_EINVAL of the entry point, with null pointers and no device ---------------------------------------------------------------
def test_entry_point_validates_before_touching_the_gpu():
    lib, p = nv.lib(), 0x1000                                              # never dereferenced: every call below fails validation first
    fn, size = lib.frcnn_ops_soft_nms, lib.frcnn_ops_soft_nms_workspace_bytes
    assert size(0) == 0 and size(-1) == 0 and size(ops.MAX_SOFT_NMS_BOXES + 1) == 0
    assert size(1) > 0 and size(ops.MAX_SOFT_NMS_BOXES) >= size(1000) > 0
    big = size(8)

    def call(boxes=p, scores=p, order=p, cats=p, n=8, thr=0.3, sigma=0.5, low=0.05, method=1, offset=0, out=p, keep=p, ws=p, ws_bytes=big):
        return fn(boxes, scores, order, cats, n, thr, sigma, low, method, offset, out, keep, ws, ws_bytes, None)

    assert call(n=-1) == -1 and call(n=ops.MAX_SOFT_NMS_BOXES + 1, ws_bytes=1 << 40) == -1
    for method in (-1, 3):
        assert call(method=method) == -1
    for offset in (-1, 2):
        assert call(offset=offset) == -1
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        assert call(sigma=sigma) == -1
    assert call(thr=float("nan")) == -1 and call(low=float("nan")) == -1
    for null in ("boxes", "scores", "order", "out", "keep", "ws"):
        assert call(**{null: None}) == -1, null
    assert call(ws_bytes=big - 1) == -1
    assert fn(None, None, None, None, 0, 0.3, 0.5, 0.05, 1, 0, None, None, None, 0, None) == 0      # no boxes: nothing to do
    assert fn(None, None, None, None, 0, 0.3, 0.5, 0.05, 3, 0, None, None, None, 0, None) == -1     # but the arguments are still checked


# ---- 3. the wrappers' errors, on meta and CPU tensors -------------------------------------------------------------------------------------
def test_wrapper_rejects_bad_arguments():
    b, s = meta(5, 4), meta(5)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.soft_nms([[0.0, 0.0, 1.0, 1.0]], s)
    with pytest.raises(TypeError, match="float64"):
        ops.soft_nms(b.double(), s)
    with pytest.raises(TypeError, match="soft_nms_pytorch"):
        ops.soft_nms(b, s.double())
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            ops.soft_nms(meta(5, 4, dtype=dtype), s)
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            ops.soft_nms(b, meta(5, dtype=dtype))
    with pytest.raises(TypeError, match="integer"):
        ops.soft_nms(b, s, labels=meta(5))
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.soft_nms(b, s, labels=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match=r"\(5, 5\)"):
        ops.soft_nms(meta(5, 5), s)
    with pytest.raises(ValueError, match=r"\(4,\)"):
        ops.soft_nms(meta(4), meta(4))
    with pytest.raises(ValueError, match=r"\(6,\)"):
        ops.soft_nms(b, meta(6))
    with pytest.raises(ValueError, match=r"\(5, 1\)"):
        ops.soft_nms(b, meta(5, 1))
    with pytest.raises(ValueError, match=r"\(4,\)"):
        ops.soft_nms(b, s, labels=meta(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="'cosine'"):
        ops.soft_nms(b, s, method="cosine")
    with pytest.raises(ValueError, match="method"):
        ops.soft_nms(b, s, method=1)
    for offset in (2, -1, 0.5, True):
        with pytest.raises(ValueError, match="offset"):
            ops.soft_nms(b, s, offset=offset)
    for sigma in (0.0, -0.5, float("inf"), float("nan"), 1e-60):            # 1e-60 rounds to 0 in float32
        with pytest.raises(ValueError, match="sigma"):
            ops.soft_nms(b, s, sigma=sigma)
    with pytest.raises(ValueError, match="iou_threshold"):
        ops.soft_nms(b, s, iou_threshold=float("nan"))
    with pytest.raises(ValueError, match="min_score"):
        ops.soft_nms(b, s, min_score=float("nan"))
    n = ops.MAX_SOFT_NMS_BOXES + 1
    with pytest.raises(ValueError, match=str(n)):
        ops.soft_nms(meta(n, 4), meta(n))
    with pytest.raises(ValueError, match="no CPU implementation"):
        ops.soft_nms(torch.zeros(3, 4), torch.zeros(3))
    with pytest.raises(ValueError, match="soft_nms_pytorch"):
        ops.soft_nms(torch.zeros(3, 4), torch.zeros(3))
    with pytest.raises(ValueError, match="cpu"):
        ops.soft_nms(b, torch.zeros(5))                                     # one on meta, one on the CPU
    with pytest.raises(ValueError, match="same device"):
        ops.soft_nms(b, s, labels=torch.zeros(5, dtype=torch.int64))
    with FakeTensorMode():
        with pytest.raises(ValueError, match="same device"):
            ops.soft_nms(torch.empty((3, 4), device="cuda:0"), torch.empty((3,), device="cuda:1"))


def test_fake_tensors_get_one_dynamic_size_and_no_gradient():
    with FakeTensorMode(shape_env=torch.fx.experimental.symbolic_shapes.ShapeEnv()):
        b = torch.empty((9, 4), device="cuda").requires_grad_(True)
        dets, inds = ops.soft_nms(b, torch.empty((9,), device="cuda"), labels=torch.empty((9,), dtype=torch.int32, device="cuda"))
        assert dets.dim() == 2 and dets.shape[1] == 5 and dets.dtype == F32 and inds.dtype == torch.int64 and inds.dim() == 1
        assert dets.shape[0] == inds.shape[0] and dets.device.type == "cuda" and not dets.requires_grad


def test_pytorch_fallback_rejects_bad_arguments():
    b, s = torch.zeros(3, 4), torch.zeros(3)
    with pytest.raises(TypeError, match="float16"):
        ops.soft_nms_pytorch(b.half(), s.half())
    with pytest.raises(TypeError, match="one dtype"):
        ops.soft_nms_pytorch(b.double(), s)
    with pytest.raises(ValueError, match="method"):
        ops.soft_nms_pytorch(b, s, method="soft")
    with pytest.raises(ValueError, match="sigma"):
        ops.soft_nms_pytorch(b, s, sigma=0)
    with pytest.raises(TypeError, match="integer"):
        ops.soft_nms_pytorch(b, s, labels=torch.zeros(3))
    dets, inds = ops.soft_nms_pytorch(b[:0], s[:0])
    assert dets.shape == (0, 5) and inds.shape == (0,) and inds.dtype == torch.int64


# ---- 4. the known answer ----------------------------------------------------------------------------------------------------------------
KNOWN_BOXES = np.float32([[0, 0, 10, 10], [0, 0, 10, 5], [20, 20, 30, 30]])  # A; B, IoU 0.5 with A; C, apart
KNOWN_SCORES = np.float32([0.9, 0.8, 0.7])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_known_answer(dtype):
    a, b, c = (float(v) if dtype is np.float64 else v for v in KNOWN_SCORES)
    linear = dtype(b) * dtype(0.5)
    for run in (lambda m: (lambda r: (r["inds"], r["scores"]))(S.reference(KNOWN_BOXES, KNOWN_SCORES, 0.3, 0.5, 1e-3, m, dtype=dtype)),
                lambda m: (lambda d, i: (i.numpy(), d[:, 4].numpy()))(*ops.soft_nms_pytorch(
                    t(KNOWN_BOXES.astype(dtype)), t(KNOWN_SCORES.astype(dtype)), 0.3, 0.5, 1e-3, m))):
        inds, scores = run("linear")
        assert inds.tolist() == [0, 2, 1] and scores.dtype == dtype and scores.tolist() == [dtype(a), dtype(c), linear]
        inds, scores = run("naive")
        assert inds.tolist() == [0, 2] and scores.tolist() == [dtype(a), dtype(c)]
        inds, scores = run("gaussian")
        assert inds.tolist() == [0, 2, 1] and scores[:2].tolist() == [dtype(a), dtype(c)]
        assert abs(float(scores[2]) - float(dtype(b)) * np.exp(-0.5)) <= 4 * np.finfo(dtype).eps
    dets, _ = ops.soft_nms_pytorch(t(KNOWN_BOXES), t(KNOWN_SCORES), 0.3, 0.5, 1e-3, "linear")
    assert dets.dtype == F32 and dets[:, :4].numpy().tolist() == KNOWN_BOXES[[0, 2, 1]].tolist()


# ---- 5. the conditions on the inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["naive", "linear", "gaussian"])
def test_clustered_cases_keep_between_3_and_60_percent(method):
    """Of the clustered cases with at least 63 boxes (a case of one or two boxes keeps one of them at least)."""
    for n in SEAMS:
        if n < 63:
            continue
        for thr in (0.3, 0.5):
            ref = S.single(n, method, 0, thr)[2]
            assert 0.03 <= ref["kept"] <= 0.60, (n, method, thr, ref["kept"])


@pytest.mark.parametrize("n", SEAMS)
def test_margin_rule_holds_for_every_case_compared_against_float64(n):
    """qualifying() asserts that a case is found within MAX_TRIES seeds; float32 and float64 agree on the order of each."""
    boxes, scores, truth, seed = S.qualifying(n, "gaussian")
    assert truth["gap"] >= S.MARGIN and truth["margin"] >= S.MARGIN and 0 <= seed < S.MAX_TRIES
    ref = S.reference(boxes, scores, method="gaussian")
    assert np.array_equal(ref["inds"], truth["inds"])
    err = rel_err(ref["scores"], truth["scores"])
    print("n %d seed %d gap %.2e margin %.2e float32 error %.2e" % (n, seed, truth["gap"], truth["margin"], err))
    assert err <= S.MARGIN / 10
    if n <= 65:
        assert truth["gap"] >= 1e-4 and truth["margin"] >= 1e-4 and seed == 0


def test_nms_cases_keep_their_ious_away_from_the_threshold():
    for n, thr in ((300, 0.3), (1000, 0.5)):
        boxes, scores = S.nms_case(n, thr)
        assert S.pair_iou_margin(boxes, thr) >= S.MARGIN and float(scores.min()) >= 0.02


def test_labelled_case_is_what_it_says():
    for small in (False, True):
        boxes, scores, labels = S.labelled(small)
        values, counts = np.unique(labels, return_counts=True)
        assert values.size == 300 and counts.min() >= 1 and counts.max() <= 40 and labels.dtype == np.int64
        assert values.min() < 0 and np.diff(values.astype(np.float64)).min() > 1
        assert (np.abs(values.astype(np.float64)).max() > 2.0 ** 62) != small
        kept = S.reference(boxes, scores, labels=labels)["kept"]
        assert 0.3 < kept < 0.9


# ---- 6. soft_nms_pytorch against the numpy loop ---------------------------------------------------------------------------------------------
def run_pytorch(boxes, scores, method, offset=0, thr=S.THR, labels=None, dtype=F32, min_score=S.MIN_SCORE):
    dets, inds = ops.soft_nms_pytorch(t(boxes).to(dtype), t(scores).to(dtype), thr, S.SIGMA, min_score, method, offset,
                                      None if labels is None else t(labels))
    assert dets.dtype == dtype and torch.equal(dets[:, :4], t(boxes).to(dtype)[inds])
    return inds.numpy(), dets[:, 4].numpy()


@pytest.mark.parametrize("method", ["naive", "linear"])
@pytest.mark.parametrize("n", [1, 2, 65, 257, 1025])
def test_pytorch_naive_and_linear_bit_for_bit(n, method):
    for offset, thr in ((0, 0.3), (1, 0.5)):
        boxes, scores, ref = S.single(n, method, offset, thr)
        inds, final = run_pytorch(boxes, scores, method, offset, thr)
        assert np.array_equal(inds, ref["inds"]) and np.array_equal(final, ref["scores"])
    boxes, scores, _ = S.single(n, method)
    truth = S.reference(boxes, scores, method=method, dtype=np.float64)
    inds, final = run_pytorch(boxes, scores, method, dtype=F64)
    assert final.dtype == np.float64 and np.array_equal(inds, truth["inds"]) and np.array_equal(final, truth["scores"])


@pytest.mark.parametrize("n", [65, 257, 1025])
def test_pytorch_gaussian_on_qualifying_cases(n):
    boxes, scores, truth, _ = S.qualifying(n, "gaussian")
    ref = S.reference(boxes, scores, method="gaussian")
    inds, final = run_pytorch(boxes, scores, "gaussian")
    assert np.array_equal(inds, truth["inds"])
    err, err_ref = rel_err(final, truth["scores"]), rel_err(ref["scores"], truth["scores"])
    print("n %d err %.3e err_ref %.3e" % (n, err, err_ref))
    assert err <= 4 * max(err_ref, 2.0 ** -24)
    inds, final = run_pytorch(boxes, scores, "gaussian", dtype=F64)
    assert np.array_equal(inds, truth["inds"]) and rel_err(final, truth["scores"]) <= 4 * 2.0 ** -53 * 64      # 64 picks' worth of ulps


@pytest.mark.parametrize("method", ["naive", "linear"])
@pytest.mark.parametrize("name", S.SPECIALS)
def test_pytorch_on_the_special_cases(name, method):
    for n in S.SPECIAL_SIZES:
        boxes, scores, offset = S.special(name, n)
        ref = S.reference(boxes, scores, method=method, offset=offset)
        inds, final = run_pytorch(boxes, scores, method, offset)
        assert np.array_equal(inds, ref["inds"]) and np.array_equal(final, ref["scores"], equal_nan=True), (name, n)
    if name == "nan_scores":
        k = int(np.isnan(scores).sum())
        assert k > 0 and np.isnan(final[-k:]).all() and not np.isnan(final[:-k]).any()       # picked last, kept, score NaN
        assert np.array_equal(inds[-k:], np.flatnonzero(np.isnan(scores)))


def test_pytorch_with_labels_offset_one_and_extreme_min_scores():
    boxes, scores, labels = S.labelled()
    for method, offset in (("linear", 0), ("naive", 1)):
        ref = S.reference(boxes, scores, method=method, offset=offset, labels=labels)
        inds, final = run_pytorch(boxes, scores, method, offset, labels=labels)
        assert np.array_equal(inds, ref["inds"]) and np.array_equal(final, ref["scores"])
    b, s, l = boxes[:700], scores[:700], labels[:700]
    inds, final = run_pytorch(b, s, "linear", labels=l, min_score=2.0)      # above every score: the first pick of each label only
    ref = S.reference(b, s, min_score=2.0, labels=l)
    assert np.array_equal(inds, ref["inds"]) and inds.size == np.unique(l).size and np.array_equal(final, s[inds])
    inds, final = run_pytorch(b, s, "linear", min_score=0.0)               # nothing is ever dropped
    assert np.array_equal(np.sort(inds), np.arange(700)) and np.array_equal(inds, S.reference(b, s, min_score=0.0)["inds"])
