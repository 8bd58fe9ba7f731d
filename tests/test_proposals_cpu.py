"""
tests/proposal_cases.py without a GPU: its reference agrees with oracle/frcnn_oracle.py: proposals_from_maps on every exact case the
oracle can express (it hard-codes the 16-pixel filter and the 0.7 threshold), and every case is what its name says -- on the intended
side of a seam of csrc/proposals.hip, with its ties, thresholds and dropped ranks where they are meant to be.  These conditions keep a
case from silently testing nothing; they hold for the reference alone, so that tests/test_proposals_gpu.py does not rest on unchecked code.
"""
import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as O
from tests import proposal_cases as P

F32 = np.float32


@pytest.fixture(scope="module")
def refs():
    """The reference of every case on numpy's float32 sigmoid of its logits, computed once."""
    return {c.name: c.reference(P.sigmoid_f32(c.inputs()["logits"])) for c in P.CASES}


def full_order(c):
    i = c.inputs()
    scores = P.sigmoid_f32(i["logits"])
    idx = np.arange(c.a) if i["valid"] is None else np.flatnonzero(i["valid"] > 0)
    return scores, idx[np.lexsort((idx, scores[idx]))[::-1]]


def test_the_table_covers_every_seam():
    assert 25 <= len(P.CASES) <= 40
    assert {c.a for c in P.CASES} >= {9, 1017, 1026, 24570, 24579, 37800, 65529, 65538}
    assert {c.pre for c in P.CASES if c.a == 24570} >= {1, 31, 32, 33, 1024, 1025, 2048, 3000, 4096, 4097, 8192, 8193, 12000, 16384}
    assert {c.sort_n for c in P.CASES} == {1024, 2048, 4096, 8192, 16384}
    assert {c.per for c in P.CASES if c.expect.get("wave")} == {2, 4, 8, 16}
    assert {c.ld for c in P.CASES} == {45, 48, 128}
    assert {c.levels for c in P.CASES} == {1, 3, 17, 1000}
    assert {c.present for c in P.CASES if c.present is not None} >= {0, 1, 499, 500, 501}
    assert {c.min_side for c in P.CASES if c.thresholds} == {16.0, 100.0}
    assert all(c.post <= 300 for c in P.CASES)
    assert {c.expect.get("residency") for c in P.TOLERANCE} == {"regs", "streamed"}
    # the rank kernel with a ragged last block of keys and a segment length that its unrolled-by-4 loop does not divide
    ragged = [c for c in P.CASES if c.present is None and c.a > c.pre and c.pre % 32 and (((c.pre + 31) & ~31) >> 5) % 4]
    assert len(ragged) >= 3


@pytest.mark.parametrize("c", P.CASES, ids=repr)
def test_case_sits_where_its_name_says(c, refs):
    r, e, i = refs[c.name], c.expect, c.inputs()
    present = c.a if i["valid"] is None else int((i["valid"] > 0).sum())
    assert r["n_selected"] == min(present, c.pre)
    assert r["sorted_idx"].shape == (r["n_selected"],) and len(set(r["sorted_idx"].tolist())) == r["n_selected"]
    assert c.sort_n == P.pow2_at_least(c.pre) and c.sort_n >= c.pre and (c.sort_n == 1024 or c.sort_n < 2 * c.pre)
    if c.present is not None:
        assert present == c.present
    if e.get("residency") == "regs":
        assert c.a <= P.REG_KEYS < c.a + 9
    if e.get("residency") == "streamed":
        assert c.a > P.REG_KEYS and present > 0
    if e.get("digits") == 5:
        assert c.a < P.SHORT_IDX_BELOW <= c.a + 9 and present > c.pre
    if e.get("digits") == 6:
        assert c.a >= P.SHORT_IDX_BELOW > c.a - 9 and present > c.pre          # (the select only runs with more present than wanted)
    if e.get("tie"):
        scores, order = full_order(c)
        assert present > c.pre
        assert scores[order[c.pre - 1]] == scores[order[c.pre]], "the pre_nms boundary is not inside a run of equal scores"
        assert order[c.pre - 1] > order[c.pre]
    if e.get("all_equal"):
        assert np.array_equal(r["sorted_idx"], np.arange(c.a - 1, c.a - 1 - c.pre, -1))
        if e["digits"] == 6:
            assert (r["sorted_idx"][:3] + 1 >= 65536).all() and (r["sorted_idx"][3:] + 1 < 65536).all()
    if e.get("straddle"):
        big = np.flatnonzero(r["sorted_idx"] + 1 >= 65536)
        assert big.min() == 0 and c.pre // 4 < big.max() < 3 * c.pre // 4       # bit 16 of the key's low word at the top and in mid-list
        assert (r["sorted_idx"] < 60000).sum() > 100
    if e.get("wave"):
        n = 64 * c.per
        assert not r["keep"][:n].any(), "the first wave's ranks must all fail the filter"
        assert set(r["sorted_idx"][:n].tolist()) <= set(i["special"].tolist())
        rest = r["keep"][n + 37:]
        flips = int((rest[1:] != rest[:-1]).sum())
        assert flips > 0.8 * (rest.shape[0] - 1), "keep / drop must alternate behind it"
    if e.get("all_filtered"):
        assert r["n_selected"] == c.pre and r["n_after_filter"] == 0 and r["proposals"].shape == (0, 4)
    if c.present == 0:
        assert r["n_selected"] == 0 and r["n_after_filter"] == 0 and r["proposals"].shape == (0, 4)
    if c.kinds == "mixed" and r["n_selected"] >= 31:
        assert 0 < r["n_after_filter"] < r["n_selected"]                        # the compaction has something to do
        assert 0 < r["proposals"].shape[0] <= c.post
    if c.exact:
        assert not i["deltas"][:, 2:4].any()


@pytest.mark.parametrize("c", [c for c in P.CASES if c.thresholds], ids=repr)
def test_threshold_rows_are_one_ulp_apart(c, refs):
    r, i = refs[c.name], c.inputs()
    m = F32(c.min_side)
    rank_of = {int(a): k for k, a in enumerate(r["sorted_idx"])}
    seen = set()
    for a, (tag, axis) in zip(i["special"], i["tags"]):
        k = rank_of[int(a)]                                                   # (selected: they carry the highest level)
        side = (r["side_h"], r["side_w"])[axis][k]
        other = (r["side_w"], r["side_h"])[axis][k]
        raw = r["boxes"][k, 2 + axis] - r["boxes"][k, axis]
        assert other >= F32(2) * m
        if tag == "eq":
            assert side == m and r["keep"][k]
        elif tag == "below":
            assert side == np.nextafter(m, F32(0)) and side < m and not r["keep"][k]
        elif tag == "edge":
            assert raw >= m and side == F32(0.5) * m and not r["keep"][k]
        elif tag == "outside":
            assert raw >= m and side < 0 and not r["keep"][k]
        seen.add((tag, axis))
    assert seen == {(t, ax) for t in ("eq", "below", "edge", "outside") for ax in (0, 1)}
    tags = [t for t, _ in i["tags"]]
    assert tags.count("edge") == 4 and tags.count("outside") == 4             # once per image edge


@pytest.mark.parametrize("c", [c for c in P.EXACT if c.min_side == 16.0 and c.nms_thr == 0.7], ids=repr)
def test_reference_matches_the_oracle(c, refs):
    r, i = refs[c.name], c.inputs()
    scores = torch.from_numpy(P.sigmoid_f32(i["logits"])).reshape(1, c.fh, c.fw, 9)
    deltas = torch.from_numpy(i["deltas"]).reshape(1, c.fh, c.fw, 36)
    valid = i["valid"] if i["valid"] is not None else np.ones(c.a, F32)
    detail = {}
    out = O.proposals_from_maps(scores, deltas, (3, c.image_h, c.image_w), i["anchors"], valid, c.pre, c.post, i["valid"] is None, detail)
    assert np.array_equal(detail["sorted_idx"], r["sorted_idx"])
    assert detail["n_after_filter"] == r["n_after_filter"]
    assert np.array_equal(out.numpy(), r["proposals"])


@pytest.mark.parametrize("c", P.TOLERANCE, ids=repr)
def test_tolerance_cases_have_no_decision_within_reach_of_expf(c, refs):
    """An ulp of expf moves a side by ~1e-5 px.  No side may be within 1e-2 px of min_side (float64), and no NMS decision may be close:
    the candidates of a site overlap its first one by more than 0.75 and the sites are disjoint."""
    r, i = refs[c.name], c.inputs()
    assert i["deltas"][:, 2:4].any()
    top = r["sorted_idx"]
    a, d = i["anchors"][top].astype(np.float64), i["deltas"][top].astype(np.float64)
    ctr = a[:, 2:4] * d[:, 0:2] + a[:, 0:2]
    size = a[:, 2:4] * np.exp(d[:, 2:4])
    lo = np.maximum(ctr - 0.5 * size, 0.0)
    hi = np.minimum(ctr + 0.5 * size, np.array([c.image_h, c.image_w], np.float64))
    side = hi - lo
    assert np.abs(side - c.min_side).min() >= 1e-2
    keep = (side >= c.min_side).all(axis=1)
    assert np.array_equal(keep, r["keep"]) and 0 < keep.sum() < keep.shape[0]
    lo, hi, site = lo[keep], hi[keep], i["site"][top][keep]
    first = {}
    for k, s in enumerate(site.tolist()):
        first.setdefault(s, k)
    f = np.array([first[s] for s in site.tolist()])
    inter = np.prod(np.maximum(np.minimum(hi, hi[f]) - np.maximum(lo, lo[f]), 0.0), axis=1)
    union = np.prod(hi - lo, axis=1) + np.prod(hi[f] - lo[f], axis=1) - inter
    assert (inter / union).min() > 0.75
    assert (hi - lo).max() + 2 * 0.01 * 41.0 < 48.0                              # sides plus the centres' jitter stay inside the sites' spacing
    assert r["proposals"].shape[0] == min(len(first), c.post)


def test_nms_sort_size_cases_have_ties():
    for n in P.NMS_SORT_SIZES:
        boxes, scores = P.nms_sort_case(n)
        assert boxes.shape == (n, 4) and scores.shape == (n,) and np.unique(scores).shape[0] <= 51
        assert P.pow2_at_least(n) == (2048 if n <= 2048 else 4096 if n <= 4096 else 8192)
        ref = O.nms(boxes, scores, 0.7)
        assert 40 <= ref.shape[0] < n
