"""
The case families of tests/detection_cases.py are what they claim to be, checked with the oracle on a machine without a GPU (a later
edit that empties a family or breaks its structure fails here), and the float32 pre-filter of csrc/detect.hip agrees with the float64
decision on its numpy mirror inside the image limit that launch_detections enforces.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from oracle import frcnn_oracle as O
from tests import box_decisions_cases as B
from tests import detection_cases as D

F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -4


def all_cases():
    return [(name, case, facts) for f in D.FAMILIES for name, case, facts in D.family(f)]


def test_every_family_is_there_and_small():
    for f in D.FAMILIES:
        assert len(D.family(f)) >= 1, f
    assert len(D.family("rank")) == len(D.RANK_N) and len(D.family("count")) == 4 * len(D.COUNT_MAX_ROIS)
    assert len(D.family("classes")) == len(D.CLASSES_NCLS) and len(D.family("margin")) == 2 * len(D.MARGIN_THRESHOLDS)
    for name, case, _ in all_cases():
        props, classes, deltas, n, max_rois, ncls, H, W, sthr, nthr = case
        assert props.shape[0] == max_rois <= 512 and 2 <= ncls <= 128, name
        assert max(H, W) <= D.image_limit(nthr), name
        assert np.isfinite(props).all() and not np.isnan(deltas).any(), name
        assert not (np.signbit(classes) & (classes == 0)).any(), name                       # no -0.0 scores (out of scope)


def test_generic_reference_is_the_oracles_at_its_threshold():
    """reference() at thresholds other than 0.3 repeats O.detections' steps with O.nms: at 0.3 the two must be the same rows."""
    for fam in ("words", "decode", "classes"):
        name, case, _ = D.family(fam)[0]
        ref = D.reference(case)
        other = D.reference(case[:9] + (float(np.nextafter(F32(0.3), F32(1))),))         # takes the generic path
        again = D.reference(case[:9] + (0.3,))
        for c in ref:
            assert np.array_equal(ref[c], again[c], equal_nan=True)
            boxes, scores, _ = D.decode_class(case, c)
            keep = O.nms(boxes, scores, 0.3)
            assert np.array_equal(ref[c][:, :4], boxes[keep]) and np.array_equal(ref[c][:, 4], scores[keep].astype(np.float64)), (name, c)
            assert other[c].shape[1] == 5


def test_words_family():
    fam = {name: (case, facts) for name, case, facts in D.family("words")}
    assert sorted(fam) == ["words_all_kept", "words_edges_mirrored", "words_patterns"]
    for name, (case, facts) in fam.items():
        assert facts["candidates"] == 512 >= 449 and facts["rank_is_index"], name
        ref = D.reference(case)[1]
        assert ref.shape[0] == facts["kept"] == sum(facts["kept_per_word"]), name          # the oracle keeps what the structure says
    p = fam["words_patterns"][1]
    assert all(p["a"]) and p["b"] == {1: True, 3: True, 6: True} and p["c"] and p["e"] == [4]
    assert p["kept_per_word"][0] == 64 and p["kept_per_word"][4] == 0 and p["kept"] > 64
    assert all(0 < k < 64 for w, k in enumerate(p["kept_per_word"]) if w not in (0, 4))    # every other word: some kept, some suppressed
    q = fam["words_edges_mirrored"][1]
    for r in D.WORD_EDGE_ROWS:                                                              # (d): each edge row in both roles over the two cases
        if r != 511:
            assert r in p["suppressors"] or r in q["suppressors"], r
        assert r in p["suppressed"] or r in q["suppressed"], r
    assert 511 not in q["suppressed"] and 448 in q["suppressed"]                           # the chain through the last word: 511 is kept
    assert fam["words_all_kept"][1]["kept_per_word"] == [64] * 8


def test_rank_family():
    assert [c[1][3] for c in D.family("rank")] == list(D.RANK_N)
    sites = D.site_boxes(512).astype(np.float64)
    seen = collections.Counter()
    for name, case, facts in D.family("rank"):
        props, classes, deltas, n, max_rois, ncls = case[:6]
        assert max_rois == 512 and (classes[n:, 1:] > 0.9).all()                           # bait past n
        ref = D.reference(case)
        for k, v in enumerate(D.RANK_VARIANTS):
            order = facts["order"][k + 1]
            assert np.array_equal(ref[k + 1][:, :4], sites[order]), (name, v)               # isolated boxes: the output order is the sort
            assert np.array_equal(ref[k + 1][:, 4], classes[order, k + 1].astype(np.float64))
            seen[v] += order.shape[0]
            if v == "permuted" and n > 8:
                assert not np.array_equal(order, np.arange(n))                             # rank != index
            if v == "all_equal":
                assert np.array_equal(order, np.arange(n))
            if v == "none":
                assert order.shape[0] == 0
            if v == "last_only":
                assert order.tolist() == [n - 1]
            if v == "one_nan":
                assert order.shape[0] == n - 1 and n // 2 not in order
            if v == "every_third":
                assert order.shape[0] == (n + 2) // 3
            if v == "tie_runs" and n >= 15:
                s = classes[:n, k + 1]
                half = (n + 1) >> 1; h8 = (half + 7) & ~7
                for edge in (half, h8, 256):                                               # a run of equal scores straddles each edge
                    assert edge >= n or s[edge - 1] == s[edge], (name, edge)
    assert all(seen[v] > 0 for v in D.RANK_VARIANTS if v != "none")


def test_count_family():
    for name, case, facts in D.family("count"):
        props, classes, deltas, n, max_rois, ncls = case[:6]
        assert props.shape[0] == max_rois and n in (0, max_rois, max_rois + 7, 10 * max_rois)
        c1, c2, c3 = facts["counts"]
        assert c3 == 0
        if n == 0:
            assert c1 == c2 == 0
        else:
            assert 1 <= c1 <= max_rois and 1 <= c2 <= (max_rois + 1) // 2
            if max_rois >= 63:
                assert c1 < max_rois                                                       # some rows are suppressed: sentinel rows remain


def test_classes_family():
    assert [c[1][5] for c in D.family("classes")] == list(D.CLASSES_NCLS)
    for name, case, facts in D.family("classes"):
        ncls = case[5]
        assert len(facts["candidates"]) == ncls - 1 and min(facts["candidates"]) >= 2, name
        assert facts["distinct_boxes_of_a_row"] == ncls - 1, name                          # a wrong stride changes every box
        assert facts["suppressed"] >= 5, name
    assert len(D.REFUSALS) == 4


def test_decode_family():
    (name, case, facts), = D.family("decode")
    assert all(f["finite"] and f["rows"] == 64 for f in facts.values())                    # no NaN: every proposal has a positive size
    assert facts["moderate"]["kept"] < 64
    assert facts["overflow"]["whole_height"] >= 16 and facts["overflow"]["whole_width"] >= 16
    assert facts["underflow"]["zero_area"] >= 36
    assert facts["pushed_out"]["zero_at_bottom"] >= 8 and facts["pushed_out"]["zero_at_left"] >= 8
    assert facts["outside_props"]["zero_area"] >= 3 and facts["outside_props"]["clipped"] >= 8
    assert facts["outside_props"]["whole_height"] >= 1 and facts["outside_props"]["whole_width"] >= 1


def test_margin_family():
    fam = D.family("margin")
    seen = set()
    for name, case, facts in fam:
        props, classes, deltas, n, max_rois, ncls, H, W, sthr, thr = case
        seen.add((H, W, thr))
        t = D.thr64(thr)
        kinds = collections.Counter(facts["kinds"])
        # IoU >= 0: nothing is "below" threshold 0 but 0 itself, and float32 cannot turn an overlap of a pixel into none
        empty_by_construction = {"fast_down", "margin_down", "f32_sign_differs"} if thr == 0.0 else set()
        for kd in D.MARGIN_KINDS:
            assert (kinds[kd] >= 6) != (kd in empty_by_construction), (name, kd, kinds[kd])
        assert facts["max_side_fraction"] >= 0.99, name                                    # sides up to the whole image
        Da, Db = facts["pairs"]
        ref = D.reference(case)
        for p, kd in enumerate(facts["kinds"]):
            path = B.det_pair_class(Da[p], Db[p], t)                                        # the scalar classifier agrees with the mirror
            want = {"band": "band", "fast_up": "fast", "fast_down": "fast", "margin_up": "margin", "margin_down": "margin", "f32_sign_differs": "margin",
                    "never_fired": "fast"}.get(kd)
            assert want is None or path == want, (name, p, kd, path)
            assert path == {"never": "fast"}.get(facts["path"][p], facts["path"][p]), (name, p)
            assert ref[p + 1].shape[0] == (1 if facts["suppressed"][p] else 2), (name, p, kd)   # isolated: b is kept iff IoU <= thr
            if kd in ("fast_up", "margin_up"):
                assert facts["suppressed"][p]
            if kd in ("fast_down", "margin_down", "never_fired", "gap_not_fired"):
                assert not facts["suppressed"][p]
    assert seen == {(H, W, thr) for thr in D.MARGIN_THRESHOLDS for (H, W) in ((600, 1000), (D.image_limit(thr),) * 2)}


# ---- the pre-filter's domain ----------------------------------------------------------------------------------------------------------
def mirror_stats(H, W, thr, k=1000000, seed=0):
    A, Bx = D.near_threshold_pairs(H, W, thr, k, seed)
    extra = [f for n, c, f in (D.margin_case(H, W, thr, seed=1, per_kind=400),)]
    A = np.concatenate([A, extra[0]["pairs"][0]]); Bx = np.concatenate([Bx, extra[0]["pairs"][1]])
    m = D.pair_mirror(A, Bx, thr)
    live = ~m["zero"] & ~m["never"]
    err = np.abs(m["lhs"] - m["E"])[live]
    near = (np.abs(m["E"]) <= 3.5 * m["margin"])[live]
    return {"pairs": int(live.sum()), "near": int(near.sum()), "wrong": int((m["dec"] != m["dec64"]).sum()),
            "never_wrong": int((m["never"] & m["dec64"]).sum()),
            "err_over_margin": float((err / m["margin"][live]).max()),
            "err_over_bound": float((err / D.derived_bound(m["s"][live], max(H, W) - 1.0, thr)).max())}


@pytest.mark.parametrize("thr", D.MARGIN_THRESHOLDS)
def test_prefilter_mirror(thr):
    """At 600 x 1000 and at the limit: no pair that float32 decides disagrees with float64, the measured error stays inside the derived
    bound and inside half the margin.  At 2 x and 4 x the limit's sides the bound must still hold; whether float32 decides a pair
    wrongly there is printed (a finding, recorded in tests/detection_cases.py), not asserted."""
    lim = D.image_limit(thr)
    for scale, (H, W) in ((0, (600, 1000)), (1, (lim, lim)), (2, (2 * lim, 2 * lim)), (4, (4 * lim, 4 * lim))):
        st = mirror_stats(H, W, thr, seed=scale)
        print("prefilter thr %g image %d x %d: %s" % (thr, H, W, st))
        assert st["near"] >= 900000 and st["never_wrong"] == 0
        assert st["err_over_bound"] <= 1.0
        if scale <= 1:
            assert st["wrong"] == 0 and st["err_over_margin"] <= 0.5


def test_limit_formula():
    assert [D.image_limit(t) for t in (0.0, 0.3, 0.5, 0.7, 1.0)] == [6711, 2970, 2165, 1704, 1291]
    assert D.DET_LIMIT_K == 1e-3 / (2 * D.U)


def test_refusals_without_a_gpu():
    """Argument checks come before the launch: bad shapes are FRCNN_EINVAL, an image past the limit is FRCNN_EUNSUPPORTED."""
    from fasterrcnn_amd import _native as nv
    lib = nv.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for max_rois, ncls in D.REFUSALS:
        assert lib.frcnn_detections(p, p, p, p, max_rois, ncls, 600, 1000, 0.05, 0.3, p, p, None) == EINVAL, (max_rois, ncls)
    for thr in (0.0, 0.3, 0.5, 0.7, 1.0):
        lim = D.image_limit(thr)
        assert lib.frcnn_detections(p, p, p, p, 300, 21, lim + 1, 600, 0.05, thr, p, p, None) == EUNSUPPORTED, thr
        assert lib.frcnn_detections(p, p, p, p, 300, 21, 600, lim + 1, 0.05, thr, p, p, None) == EUNSUPPORTED, thr
    assert lib.frcnn_detections(p, p, p, p, 300, 21, 9600, 16000, 0.05, 0.3, p, p, None) == EUNSUPPORTED
    assert lib.frcnn_detections(p, p, p, p, 0, 21, 9600, 16000, 0.05, 0.3, p, p, None) == EINVAL          # a bad shape comes first
