"""SGDET / SGCLS training targets, the parts that need no GPU: the fixtures hold every case they are meant to hold, the target
table with every relation, the identity "detections = ground-truth objects gives the PredCLS targets" on the restatement, and
the C ABI's declaration."""
import os
import re

import numpy as np

from tests import sgdet_train_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(res, s, o):
    pidx = res["pidx"]
    (p,) = np.nonzero((pidx.sub == s) & (pidx.obj == o))[0]
    return int(p)


def test_crafted_fixture_properties():
    c = C.crafted()
    eq = C.equiv_table()
    on = C.assign_reference(c["num_objects"], c["cats"], c["boxes"], c["table"], eq, c["R"])
    off = C.assign_reference(c["num_objects"], c["cats"], c["boxes"], c["table"], None, c["R"])
    t_image, t_rel = c["table"][0], c["table"][1]
    assert c["num_objects"] == [5, 1, 7] and len(t_rel) == 9 and on["pidx"].n_pairs == 5 * 4 + 7 * 6
    # |M| >= 2 with different relations: the IoU product decides, also against the row order
    p = _pair(on, C.D_A2, C.D_B)
    assert on["cands"][p] == [C.ROW_A_B, C.ROW_A2_B] and t_rel[C.ROW_A_B] != t_rel[C.ROW_A2_B]
    assert on["matched"][p] == C.ROW_A2_B and on["directed"][p] == t_rel[C.ROW_A2_B]
    p = _pair(on, C.D_A, C.D_B)
    assert on["cands"][p] == [C.ROW_A_B, C.ROW_A2_B] and on["matched"][p] == C.ROW_A_B
    # an exact tie between two rows (different boxes, equal integer products): the smaller row wins
    p = _pair(on, C.D_B, C.D_A)
    assert on["cands"][p] == [C.ROW_TIE_LO, C.ROW_TIE_HI] and on["matched"][p] == C.ROW_TIE_LO
    b_a = C.grid_box(c["boxes"][C.D_A], 32)
    q = [C.inter_union(b_a, C.grid_box(c["table"][5][t], 32)) for t in (C.ROW_TIE_LO, C.ROW_TIE_HI)]
    assert q[0][0] * q[1][1] == q[1][0] * q[0][1] and tuple(c["table"][5][C.ROW_TIE_LO]) != tuple(c["table"][5][C.ROW_TIE_HI])
    assert on["matched"][_pair(on, C.D_B, C.D_A2)] == C.ROW_TIE_HI                 # ... and no tie for the second detection of A
    # a row no detection matches
    assert 0 <= t_rel[C.ROW_UNMATCHED] < c["R"] and on["target_hit"][C.ROW_UNMATCHED] == 0
    # two detections of one ground-truth object both receive its relations
    for d in (C.D_A, C.D_A2):
        p = _pair(on, d, C.D_B)
        assert C.ROW_A_B in on["cands"][p] and on["directed"][p] >= 0
    # the asymmetric equivalence, read as equiv[target][detection], in both directions; equality only without the table
    assert c["cats"][C.D_VEHICLE] == 123 and c["table"][2][C.ROW_CAR] == 14 and eq[14][123]
    assert c["cats"][C.D_CAR] == 14 and c["table"][2][C.ROW_VEHICLE] == 123 and eq[123][14]
    assert not eq[14][63] and eq[123][63]                                           # not transitive: the order of the indices matters
    for d, row in ((C.D_VEHICLE, C.ROW_CAR), (C.D_CAR, C.ROW_VEHICLE)):
        p = _pair(on, d, C.D_B)
        assert on["matched"][p] == row and off["matched"][p] == -1
        assert on["target_hit"][row] == 1 and off["target_hit"][row] == 0
    # slice clipping: a negative coordinate and one beyond the grid
    bx = c["boxes"][C.D_CLIP]
    assert bx.min() < 0 and bx.max() > 32 and C.grid_box(bx, 32) == (28, 32, 24, 31)
    assert on["matched"][_pair(on, C.D_B, C.D_CLIP)] == C.ROW_CLIP
    # an empty box matches nothing
    assert C.grid_box(c["boxes"][C.D_EMPTY], 32)[0] == C.grid_box(c["boxes"][C.D_EMPTY], 32)[1]
    pidx = on["pidx"]
    touched = (pidx.sub == C.D_EMPTY) | (pidx.obj == C.D_EMPTY)
    assert touched.sum() == 12 and (on["matched"][touched] == -1).all()
    # a row with rel >= R is no candidate - and would be one with more relations
    assert t_rel[C.ROW_BAD_REL] >= c["R"] and on["target_hit"][C.ROW_BAD_REL] == 0
    more = C.assign_reference(c["num_objects"], c["cats"], c["boxes"], c["table"], eq, 100)
    assert more["matched"][_pair(more, C.D_CLIP, C.D_B)] == C.ROW_BAD_REL
    # an image with one detection (no pairs), an image with pairs and no rows whose detections would match another image's rows
    assert not (pidx.image == 1).any() and not (t_image == 1).any()
    assert (pidx.image == 0).sum() == 20 and not (t_image == 0).any() and (on["matched"][pidx.image == 0] == -1).all()
    assert tuple(c["boxes"][0]) == tuple(c["boxes"][C.D_A]) and c["cats"][0] == c["cats"][C.D_A]
    # raw: the reversed pair's relation where the pair itself has none
    p, r = _pair(on, C.D_B, C.D_CLIP), _pair(on, C.D_CLIP, C.D_B)
    assert on["directed"][r] == -1 and on["raw"][r] == on["directed"][p] == on["raw"][p] == 5
    assert set(np.nonzero(on["target_hit"])[0]) == {0, 1, 2, 3, 4, 5, 7}


def test_drawn_fixture_properties():
    d = C.drawn()
    res = C.assign_reference(d["num_objects"], d["cats"], d["boxes"], d["table"], C.equiv_table(), d["R"])
    assert len(d["num_objects"]) == 4 and all(8 <= n <= 12 for n in d["num_objects"])
    T = len(d["table"][1])
    assigned, hit = int((res["matched"] >= 0).sum()), int(res["target_hit"].sum())
    assert T >= 20 and 0 < hit < T and assigned > hit                      # some rows lost (missed classes), duplicates share rows
    off = C.assign_reference(d["num_objects"], d["cats"], d["boxes"], d["table"], None, d["R"])
    print("rows", T, "hit", hit, "assigned", assigned, "without the equivalence classes", int(off["target_hit"].sum()), int((off["matched"] >= 0).sum()))
    assert int((off["matched"] >= 0).sum()) < assigned                     # some pairs match through the equivalence classes only


def _as_sets(table):
    return sorted((int(i), int(r), int(s), int(o), tuple(sb.tolist()), tuple(ob.tolist())) for i, r, s, o, sb, ob in zip(*table))


def test_target_table_with_every_relation():
    from scene_graph_commonsense_amd.pairs import enumerate_pairs, pair_targets_fast, sg_target_ptr, sg_target_table
    from tests import sgdet_case
    from tests.golden_cases import load_case
    _, _, batch, _, _ = sgdet_case.make_case()
    batches = [batch, load_case("vg_full")[2], C.drawn()["gt"]]
    grew = 0
    for bt in batches:
        args = (bt.relationships, bt.subj_or_obj, bt.categories, bt.bbox)
        default, again, full = sg_target_table(*args), sg_target_table(*args, drop_last_graph_object=True), sg_target_table(*args, drop_last_graph_object=False)
        for a, b in zip(default, again):
            np.testing.assert_array_equal(a, b)
        # the default is today's table, row for row: match_target_sgd's lists concatenated
        from scene_graph_commonsense_amd.pairs import match_target_sgd
        cs, co, bs, bo, rt = match_target_sgd(*args)
        keep = [i for i, r in enumerate(rt) if r is not None]
        if keep:
            np.testing.assert_array_equal(default[0], np.concatenate([np.full(len(rt[i]), i) for i in keep]))
            np.testing.assert_array_equal(default[1], np.concatenate([rt[i].numpy() for i in keep]))
            np.testing.assert_array_equal(default[2], np.concatenate([cs[i].numpy() for i in keep]))
            np.testing.assert_array_equal(default[3], np.concatenate([co[i].numpy() for i in keep]))
            np.testing.assert_array_equal(default[4], np.concatenate([bs[i].numpy() for i in keep]).astype(np.float32))
            np.testing.assert_array_equal(default[5], np.concatenate([bo[i].numpy() for i in keep]).astype(np.float32))
        else:
            assert default[0].size == 0
        have, want = _as_sets(full), _as_sets(default)
        assert all(r in have for r in want) and len(have) >= len(want)
        grew += len(have) - len(want)
        assert (np.diff(full[0]) >= 0).all()
        # exactly the relations of pair_targets_fast: one row per connected ordered pair
        n = [int(b.shape[0]) for b in bt.bbox]
        pidx = enumerate_pairs(n)
        directed = pair_targets_fast(bt.relationships, bt.subj_or_obj, pidx)
        cats = np.concatenate([np.asarray(c) for c in bt.categories])
        box = np.concatenate([np.asarray(b) for b in bt.bbox]).astype(np.float32)
        conn = np.nonzero(directed != -1)[0]
        expect = sorted((int(pidx.image[p]), int(directed[p]), int(cats[pidx.sub[p]]), int(cats[pidx.obj[p]]), tuple(box[pidx.sub[p]].tolist()),
                         tuple(box[pidx.obj[p]].tolist())) for p in conn)
        assert have == expect
        ptr = sg_target_ptr(full[0], len(n))
        assert ptr[0] == 0 and ptr[-1] == full[0].size and all((full[0][ptr[b]:ptr[b + 1]] == b).all() for b in range(len(n)))
    assert grew > 0                                                          # the loop-bound quirk drops something somewhere


def _identity_inputs():
    """PredCLS batches on which the identity must hold: every box non-empty, and no two objects of an image with equivalent labels
    and grid IoU >= 0.5 (either would make a detection match another object's relations too)."""
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch
    return [C.identity_case()[2], C.drawn()["gt"], make_scene_batch(HeadConfig(), (9, 2, 1, 6), seed=23, connect_frac=0.5)]


def check_identity_condition(batch, eq):
    for cats, box in zip(batch.categories, batch.bbox):
        gb = [C.grid_box(r, 32) for r in box.numpy()]
        for i in range(len(gb)):
            for j in range(len(gb)):
                if i != j and (C.label_ok(int(cats[i]), int(cats[j]), eq) or C.label_ok(int(cats[j]), int(cats[i]), eq)):
                    assert not C.iou_ok(gb[i], gb[j], 0.5), "two objects with equivalent labels and overlapping boxes"


def connected_objects_have_area(batch):
    """An object with an empty box has grid IoU 0 with itself (union 0): its relations cannot be assigned to it."""
    from scene_graph_commonsense_amd.pairs import enumerate_pairs, pair_targets_fast
    n = [int(b.shape[0]) for b in batch.bbox]
    pidx = enumerate_pairs(n)
    directed = pair_targets_fast(batch.relationships, batch.subj_or_obj, pidx)
    box = np.concatenate([np.asarray(b) for b in batch.bbox])
    area = np.array([(lambda g: max(g[1] - g[0], 0) * max(g[3] - g[2], 0))(C.grid_box(r, 32)) for r in box])
    conn = directed != -1
    return bool((area[pidx.sub[conn]] > 0).all() and (area[pidx.obj[conn]] > 0).all())


def test_identity_detections_equal_ground_truth_gives_predcls_targets():
    from scene_graph_commonsense_amd.pairs import enumerate_pairs, pair_targets, pair_targets_fast, sg_target_table
    eq = C.equiv_table()
    for batch in _identity_inputs():
        check_identity_condition(batch, eq)
        assert connected_objects_have_area(batch)
        n = [int(b.shape[0]) for b in batch.bbox]
        cats = np.concatenate([np.asarray(c) for c in batch.categories])
        box = np.concatenate([np.asarray(b) for b in batch.bbox]).astype(np.float32)
        table = sg_target_table(batch.relationships, batch.subj_or_obj, batch.categories, batch.bbox, drop_last_graph_object=False)
        res = C.assign_reference(n, cats, box, table, eq, 50)
        pidx = enumerate_pairs(n)
        directed = pair_targets_fast(batch.relationships, batch.subj_or_obj, pidx)
        assert (directed != -1).sum() > 0
        np.testing.assert_array_equal(res["directed"], directed)
        np.testing.assert_array_equal(res["raw"], pair_targets(batch.relationships, batch.subj_or_obj, pidx)[1])
        assert res["target_hit"].all() and (res["matched"] >= 0).sum() == len(table[1])


def test_identity_on_vg_full_as_stored_drops_what_evaluation_cannot_credit():
    """vg_full as stored has a zero-area object: its relations (grid IoU 0 with itself) are exactly the ones that are not assigned."""
    from scene_graph_commonsense_amd.pairs import enumerate_pairs, pair_targets_fast, sg_target_table
    batch = C.identity_case(give_area=False)[2]
    assert not connected_objects_have_area(batch)
    creditable, dropped = C.without_uncreditable(batch)
    assert dropped == 5 and connected_objects_have_area(creditable)
    n = [int(b.shape[0]) for b in batch.bbox]
    cats = np.concatenate([np.asarray(c) for c in batch.categories])
    box = np.concatenate([np.asarray(b) for b in batch.bbox]).astype(np.float32)
    table = sg_target_table(batch.relationships, batch.subj_or_obj, batch.categories, batch.bbox, drop_last_graph_object=False)
    res = C.assign_reference(n, cats, box, table, C.equiv_table(), 50)
    np.testing.assert_array_equal(res["directed"], pair_targets_fast(creditable.relationships, creditable.subj_or_obj, enumerate_pairs(n)))
    assert int(res["target_hit"].sum()) == len(table[1]) - dropped


def test_header_declares_the_assignment_entry():
    hdr = open(os.path.join(REPO, "include", "sgc_relhead.h")).read()
    m = re.search(r"\bint\s+sgc_assign_pair_targets\s*\(([^;]*)\)\s*;", hdr)
    assert m is not None, "include/sgc_relhead.h does not declare sgc_assign_pair_targets"
    args = " ".join(m.group(1).split())
    for name in ("t_ptr", "equiv", "feature_size", "iou_thresh", "directed", "raw", "matched", "target_hit", "stream"):
        assert re.search(r"\b%s\b" % name, args), name
    assert "evaluator.py:306-356" in hdr and "train_utils.py:169-187" in hdr
