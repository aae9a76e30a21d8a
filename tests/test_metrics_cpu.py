"""Host tests of the device-metrics feature: the synthetic cases of ``tests/metrics_cases.py`` reach every branch of the kernels
(asserted on the host restatement's own output), the two C-ABI entries are declared and exported, and ``RecallMeter`` refuses what it
cannot run."""
import os
import re

import numpy as np
import pytest

from tests import metrics_cases as MC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scans():
    """Per state: the scans of the plain and the Top-3 mode at K = 128 and the precision flags."""
    out = {}
    for name, st in MC.states():
        out[name] = dict(plain=MC.recall_counters(st, MC.rank_host(st, 128)), top3=MC.recall_counters(st, MC.rank_host(st, 128, True), top3=True),
                         precision=MC.precision_counters(st, MC.rank_host(st, 128)), st=st)
    return out


def test_cases_reach_every_branch_of_the_recall_scan(scans):
    seen = scans["high_ranks"]["plain"][1]
    assert any(h is not None and h >= 64 for _, h, _, _, _ in seen)                           # the second ballot round
    assert any(w for _, _, w, _, _ in seen)                                                    # a label-and-box match with another predicate ahead
    assert any(h is None for _, h, _, _, _ in seen)
    st = scans["ties_and_inf"]["st"]
    rk = MC.rank_host(st, 100)
    b = int(np.argmin(rk["count"]))
    scores = st["conf"][rk["pair"][b, :rk["count"][b]], rk["slot"][b, :rk["count"][b]]]
    assert rk["count"][b] < 100 and np.isinf(scores).any()                                     # -inf candidates inside the window, count < K
    assert len(np.unique(scores[np.isfinite(scores)])) < np.isfinite(scores).sum() / 2         # ties
    c20, c100 = MC.recall_counters(st, MC.rank_host(st, 20))[0], MC.recall_counters(st, rk)[0]
    assert 0 < c20["hits"][0] == c100["hits"][0] < c100["hits"][1] < c100["hits"][2] < c100["targets"][0]
    st = scans["ragged_8_images"]["st"]
    assert 5 not in st["image"] and st["n_img"] == 8 and (st["directed"][st["image"] == 2] == -1).all()      # no rows; no connected target
    assert st["included"] is not None and 0 < st["included"].mean() < 1
    rk = MC.rank_host(st, 100)
    assert rk["count"][5] == 0 and rk["count"][1] == 3 and (rk["count"] == 100).any()


def test_cases_reach_both_sides_of_the_top3_rule(scans):
    seen = scans["top3_rule"]["top3"][1]
    per_image = {b: n for b, _, _, n, _ in seen}
    assert per_image[0] > 50 and 0 < per_image[1] < 20
    assert any(b == 0 and h is not None and 20 <= h < n for b, h, _, n, _ in seen)             # counts for k = 20 although rank >= 20
    assert any(b == 0 and h is not None and h >= max(50, n) for b, h, _, n, _ in seen)         # does not count for k = 50
    assert any(b == 1 and h is not None and h < 20 for b, h, _, n, _ in seen)
    c = scans["top3_rule"]["top3"][0]
    assert c["hits"][0] == c["hits"][1] < c["hits"][2] < c["targets"][0]


def test_cases_reach_zero_shot_and_empty_boxes(scans):
    for name in ("high_ranks", "ragged_8_images"):
        c, seen = scans[name]["plain"]
        assert 0 < c["zs_targets"][0] < c["targets"][0] and 0 < c["zs_hits"][-1] < c["hits"][-1], name
        assert {z for *_, z in seen} == {True, False}
    st = scans["zero_area_and_clones"]["st"]
    empty = [o for o in range(len(st["cats"])) if not MC._mask(st, o).any()]
    assert len(empty) == 4 and MC.iou(st, empty[0], empty[0]) == 0 and MC.iou_union(st, empty[0], empty[1], empty[0], empty[1]) == 0
    t = np.nonzero(st["directed"] != -1)[0]
    assert any(st["sub_idx"][p] in empty for p in t)                                           # a target that cannot be hit: union == 0
    assert any(w for _, _, w, _, _ in scans["zero_area_and_clones"]["top3"][1])                # a clone's pair ahead of the true hit


def test_cases_reach_the_four_precision_outcomes(scans):
    flags = set(scans["union_cases"]["precision"][1])
    assert flags == {(True, True), (True, False), (False, True), (False, False)}
    c = scans["union_cases"]["precision"][0]
    assert c["num_ap"].sum() == 38 and (c["ap"] != c["ap_union"]).any() and ((0 < c["ap"]) & (c["ap"] < c["num_ap"])).any()


def test_zero_shot_words_follow_the_bitmap_layout():
    st = dict(MC.states())["union_cases"]
    words = MC.zero_shot_words(st)
    bit = (1 * MC.R + 4) * MC.C + 2
    assert int(words.astype(np.uint64).sum()) == 1 << (bit & 31) and words[bit >> 5] == 1 << (bit & 31)


def test_metric_entry_points_are_declared_and_exported():
    from scene_graph_commonsense_amd import _lib
    hdr = open(os.path.join(REPO, "include", "sgc_relhead.h")).read()
    declared = set(re.findall(r"\bint\s+(sgc_\w+)\s*\(", hdr))
    assert {"sgc_recall_accumulate", "sgc_precision_accumulate"} <= declared
    assert "evaluator.py:306-367" in hdr and "evaluator.py:522-557" in hdr
    lib = _lib.load()
    assert hasattr(lib, "sgc_recall_accumulate") and hasattr(lib, "sgc_precision_accumulate")


def test_meter_is_gpu_only_and_bounds_top_k():
    from scene_graph_commonsense_amd.metrics import RecallMeter
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    args = HeadConfig().args()
    with pytest.raises(ValueError, match="top_k"):
        RecallMeter(args, 50, top_k=(20, 50, 129))
    with pytest.raises(RuntimeError, match="GPU"):
        RecallMeter(args, 50, device="cpu")
