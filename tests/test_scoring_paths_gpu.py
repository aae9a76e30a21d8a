"""Characterisation of ``pair_loop``'s six evaluation entry points (``evaluate_minibatch``, ``score_minibatch``, ``predict_scene_graphs``,
``mine_commonsense_candidates``, ``evaluate_sgdet_minibatch``, ``score_sgdet_minibatch``): they run ONE forward - the same ``PairOutputs``
bit for bit on the same scene, in one pass and in image groups - each touches exactly its own ``model.last_*`` attributes, and their
``ValueError`` texts are what callers have seen so far.  What the calls do with the outputs is pinned by the routes' own test files."""
import os
import types

import numpy as np
import pytest
import torch

from tests import sgdet_case
from tests.golden_cases import GOLDEN
from tests.test_metrics_gpu import retarget

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FX = os.path.join(GOLDEN, "ref_fixtures") + os.sep
TOP_K = [20, 50, 100]
FIELDS = ("relation", "super_relation", "connectivity", "hidden", "cand_conf", "cand_pred")
FLAGS = [(False, False), (False, True), (True, False), (True, True)]          # (overlap_filtering, skip_filtered)
LAST = ("last_image_groups", "last_outputs", "last_connectivity_stats")


def _model(cfg, sd):
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    args = cfg.args(fixtures=FX)
    model = BayesianRelationClassifier(args).cuda()
    model.load_state_dict(sd)
    return args, model.eval()


@pytest.fixture(scope="module")
def vg():
    """Default head, seed-0 weights, one minibatch with a 2-object image (fewer candidates than any K) and targets from the model's
    own predictions."""
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    args, model = _model(cfg, make_state_dict(cfg, seed=0))
    batch = retarget(model, cfg, make_scene_batch(cfg, (12, 2, 9, 5, 7), seed=33, connect_frac=0.0), seed=5)
    return types.SimpleNamespace(cfg=cfg, args=args, model=model, batch=batch)


@pytest.fixture(scope="module")
def sg():
    """The seeded SGDET case of tests/test_sg_metrics_gpu.py: the front end's object lists and the stored ground truth."""
    from scene_graph_commonsense_amd.object_frontend import DetrFrontEnd
    from scene_graph_commonsense_amd.synthetic import default_sub2super
    cfg, sd, batch, logits, boxes = sgdet_case.make_case()
    sgdet_case.apply_stored_targets(batch, np.load(os.path.join(GOLDEN, "sgdet_vg.npz")))
    args, model = _model(cfg, sd)
    cats, confs, bxs, kept = DetrFrontEnd(sgdet_case.alp2fre_table().tolist()).sgdet(logits.cuda(), boxes.cuda())
    assert kept == [0, 1, 2]
    return types.SimpleNamespace(cfg=cfg, args=args, model=model, feat=batch.image_feature.cuda(), depth=batch.image_depth.cuda(),
                                 lists=(cats, confs, bxs), targets=(batch.relationships, batch.subj_or_obj, batch.categories, batch.bbox),
                                 sub2super=default_sub2super(cfg.num_classes, cfg.num_super_classes))


def _budget_and_groups(cfg, bbox, n_groups):
    """(workspace budget, the image groups ``plan_image_groups`` makes of it): one group, or a budget found by asking the planner
    (host arithmetic only, as tests/test_sgdet_train_gpu.py derives its own) under which the minibatch is cut into two or more."""
    from scene_graph_commonsense_amd.pair_loop import image_workspace_bytes, plan_image_groups
    holder = types.SimpleNamespace(bbox=bbox)
    if n_groups == 1:
        return 1e15, [(0, len(bbox))]
    cost = [1.15 * image_workspace_bytes(cfg, b, False) for b in bbox]
    for k in range(1, len(cost)):
        budget = 1.001 * max(sum(cost[:k]), sum(cost[k:]))
        groups = plan_image_groups(cfg, holder, False, budget)
        if len(groups) >= 2:
            return budget, groups
    raise AssertionError("no budget gives two groups")


def _call(model, fn):
    """Run ``fn`` with a fresh sentinel on every ``model.last_*`` attribute; returns (result, {attribute: value or "untouched"})."""
    marks = {name: object() for name in LAST}
    for name, mark in marks.items():
        setattr(model, name, mark)
    res = fn()
    return res, {name: "untouched" if getattr(model, name) is marks[name] else getattr(model, name) for name in LAST}


def _assert_outputs_equal(a, b, what):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (what, f)
        assert x is None or (x.dtype == y.dtype and torch.equal(x, y)), (what, f)


def _assert_stats(seen, expect_none, what):
    stats = seen["last_connectivity_stats"]
    if expect_none:
        assert stats is None, what
    else:
        assert torch.is_tensor(stats) and stats.dtype == torch.int64 and tuple(stats.shape) == (5,), what
    return stats


@pytest.mark.parametrize("n_groups", [1, 2])
@pytest.mark.parametrize("overlap,skip", FLAGS)
def test_predcls_entry_points_share_one_forward(vg, overlap, skip, n_groups):
    from scene_graph_commonsense_amd.evaluator import Evaluator, Evaluator_Top3
    from scene_graph_commonsense_amd.metrics import RecallMeter
    from scene_graph_commonsense_amd.pair_loop import (evaluate_minibatch, mine_commonsense_candidates, predict_scene_graphs,
                                                       score_minibatch)
    from scene_graph_commonsense_amd.pairs import flatten_scene
    cfg, model, batch, R = vg.cfg, vg.model, vg.batch, vg.cfg.num_relations
    budget, groups = _budget_and_groups(cfg, batch.bbox, n_groups)
    assert len(groups) >= n_groups
    scene = flatten_scene(cfg, batch, DEV)
    assert scene.raw_target is not None
    selects = skip and overlap                       # the only combination in which a call hands a pair selection to the forward
    ev, t3 = Evaluator(vg.args, R, 0.5, TOP_K), Evaluator_Top3(vg.args, R, 0.5, TOP_K)
    meter = RecallMeter(vg.args, R, iou_thresh=0.5, top_k=TOP_K, device=DEV)

    got, seen = _call(model, lambda: evaluate_minibatch(model, batch, ev, t3, overlap_filtering=overlap, scene=scene,
                                                        skip_filtered=skip, workspace_budget=budget))
    assert got[0] is scene and len(got) == 4
    out_e = got[1]
    assert seen["last_image_groups"] == groups and seen["last_outputs"] == "untouched"
    stats_e = _assert_stats(seen, selects, "evaluate_minibatch")

    got, seen = _call(model, lambda: score_minibatch(model, batch, meter, overlap_filtering=overlap, scene=scene, skip_filtered=skip,
                                                     workspace_budget=budget))
    assert got[0] is scene and len(got) == 2
    out_s = got[1]
    assert seen["last_image_groups"] == groups and seen["last_outputs"] is out_s
    stats_s = _assert_stats(seen, selects, "score_minibatch")
    assert selects or torch.equal(stats_e, stats_s)

    _, seen = _call(model, lambda: predict_scene_graphs(model, batch, overlap_filtering=overlap, scene=scene, workspace_budget=budget))
    out_p = seen["last_outputs"]
    assert seen["last_image_groups"] == groups and seen["last_connectivity_stats"] == "untouched"

    _, seen = _call(model, lambda: mine_commonsense_candidates(model, batch, overlap_filtering=overlap, scene=scene,
                                                               workspace_budget=budget))
    out_m = seen["last_outputs"]
    assert seen["last_image_groups"] == groups and seen["last_connectivity_stats"] == "untouched"

    assert int(out_e.cand_conf.shape[0]) == scene.n_pairs == sum(n * (n - 1) for n in (12, 2, 9, 5, 7))
    _assert_outputs_equal(out_e, out_s, "evaluate / score")
    _assert_outputs_equal(out_p, out_m, "predict / mine")
    if not selects:                                  # no selection anywhere: all four ran the same forward
        _assert_outputs_equal(out_e, out_p, "evaluate / predict")


@pytest.mark.parametrize("n_groups", [1, 2])
@pytest.mark.parametrize("overlap,skip", FLAGS)
def test_sgdet_entry_points_share_one_forward(sg, overlap, skip, n_groups):
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.metrics import RecallMeter
    from scene_graph_commonsense_amd.pair_loop import evaluate_sgdet_minibatch, score_sgdet_minibatch
    model, R = sg.model, sg.cfg.num_relations
    budget, groups = _budget_and_groups(sg.cfg, [b.detach().float().cpu() for b in sg.lists[2]], n_groups)
    assert len(groups) >= n_groups
    ev = Evaluator(sg.args, R, 0.5, TOP_K)
    meter = RecallMeter(sg.args, R, iou_thresh=0.5, top_k=TOP_K, device=DEV)
    kw = dict(sub2super=sg.sub2super, targets=sg.targets, overlap_filtering=overlap, skip_filtered=skip, workspace_budget=budget)

    got, seen = _call(model, lambda: evaluate_sgdet_minibatch(model, sg.feat, sg.depth, *sg.lists, ev, **kw))
    assert len(got) == 3 and isinstance(got[2], np.ndarray) and got[2].dtype == np.bool_
    out_e = got[1]
    assert seen == dict(last_image_groups=groups, last_outputs="untouched", last_connectivity_stats="untouched")

    got, seen = _call(model, lambda: score_sgdet_minibatch(model, sg.feat, sg.depth, *sg.lists, meter, **kw))
    assert len(got) == 2
    out_s = got[1]
    assert seen["last_image_groups"] == groups and seen["last_outputs"] is out_s and seen["last_connectivity_stats"] == "untouched"
    assert int(out_e.cand_conf.shape[0]) == got[0].n_pairs > 0
    _assert_outputs_equal(out_e, out_s, "evaluate_sgdet / score_sgdet")


def _raises(text, fn):
    with pytest.raises(ValueError) as err:
        fn()
    assert str(err.value) == text


def test_error_messages_word_for_word(vg, sg):
    from scene_graph_commonsense_amd import pair_loop as PL
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.metrics import RecallMeter
    from scene_graph_commonsense_amd.pairs import flatten_scene
    from scene_graph_commonsense_amd.synthetic import SceneBatch
    cfg, model, b = vg.cfg, vg.model, vg.batch
    bare = SceneBatch(b.image_feature, b.image_depth, b.bbox, b.categories, b.super_categories, None, None)
    scene = flatten_scene(cfg, bare, DEV)
    assert scene.directed is None
    ev = Evaluator(vg.args, cfg.num_relations, 0.5, TOP_K)
    meter = RecallMeter(vg.args, cfg.num_relations, iou_thresh=0.5, top_k=TOP_K, device=DEV)
    out = model.forward_pairs(scene)
    _raises("the evaluator feed needs relation targets: flatten the scene from a batch with relationships / subj_or_obj",
            lambda: PL.feed_evaluators(model, scene, out, ev))
    _raises("the metrics need relation targets: a batch with relationships / subj_or_obj",
            lambda: PL.score_minibatch(model, bare, meter, scene=scene))
    _raises("the candidate mining needs relation targets: a batch with relationships / subj_or_obj",
            lambda: PL.mine_commonsense_candidates(model, bare, scene=scene))
    _raises("training_step needs relation targets: build the scene from a batch with relationships / subj_or_obj, "
            "or pass them (or a directed array) here", lambda: model.training_step(scene, None, None))
    short = [torch.zeros(int(x.shape[0]) - 1) for x in b.bbox]
    _raises("cat_confidence must hold one value per object", lambda: PL.predict_scene_graphs(model, bare, cat_confidence=short, scene=scene))
    cats, confs, bxs = sg.lists
    _raises("cat_pred_confidence must hold one value per predicted object",
            lambda: PL.score_sgdet_minibatch(sg.model, sg.feat, sg.depth, cats, [c[:-1] for c in confs], bxs, meter,
                                             sub2super=sg.sub2super, targets=sg.targets))
    _raises("one predicted-object list per image is required (the reference drops the whole minibatch otherwise)",
            lambda: PL._sgdet_scene(sg.model, sg.feat, sg.depth, cats[:-1], bxs[:-1], sg.sub2super))
    _raises("sub2super_cat_dict is required for Visual Genome label vectors",
            lambda: PL._sgdet_scene(sg.model, sg.feat, sg.depth, cats, bxs, None))
