"""GPU tests of the commonsense candidate mining (run_mode prepare_cs): the evaluator route against the real reference's outputs, the
kernel ``sgc_related_topk`` against the pinned host loop on synthetic states, the fused route against the evaluator route, and the
``eval_pc`` driver's two steps."""
import os

import numpy as np
import pytest
import torch

from tests import mining_cases as MC
from tests.golden_cases import GOLDEN

pytestmark = pytest.mark.gpu
FX = os.path.join(GOLDEN, "ref_fixtures") + os.sep


@pytest.fixture(scope="module")
def fx():
    return MC.load_fixture()


def _names(fx):
    return fx["object_names"].tolist(), fx["relation_names"].tolist()


def _evaluator(args=None, hierarchical=True):
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    cfg = HeadConfig(hierarchical=hierarchical)
    args = args or cfg.args(run_mode="prepare_cs", fixtures=FX)
    return Evaluator(args, cfg.num_relations, 0.5, [20, 50, 100]), args


def _state_of(ev):
    """The evaluator's flat state as host arrays, through its reference-named attributes."""
    h = lambda t: t.detach().cpu().numpy()
    return dict(which=h(ev.which_in_batch), conf=h(ev.confidence), pred=h(ev.relation_pred), scat=h(ev.subject_cat_pred),
                ocat=h(ev.object_cat_pred), sbox=h(ev.subject_bbox_pred), obox=h(ev.object_bbox_pred), which_t=h(ev.which_in_batch_target),
                rel_t=h(ev.relation_target), scat_t=h(ev.subject_cat_target), ocat_t=h(ev.object_cat_target),
                sbox_t=h(ev.subject_bbox_target), obox_t=h(ev.object_bbox_target))


# ------------------------------------------------------------------------------------------------ (a) reference state
@pytest.mark.parametrize("top_k", [10, 30])
def test_evaluator_route_matches_the_reference(fx, top_k, tmp_path):
    """The reference's evaluator state rebuilt through ``accumulate`` from the fixture's per-step inputs; strings, relation ids, boxes,
    ranks, confidences (the same f32: a maximum over stored inputs) and the saved lists and paths equal the reference's own."""
    ev, args = _evaluator()
    args["dataset"]["annot_dir"] = str(tmp_path)
    for step in MC.fixture_steps(fx):
        ev.accumulate(*[x.cuda() if torch.is_tensor(x) else x for x in step])
    st = _state_of(ev)
    for k in MC.STATE_KEYS:
        np.testing.assert_array_equal(st[k], fx["ref_" + k], err_msg=k)
    ev.load_annotation_paths(["image_%d_annotations.pkl" % b for b in range(len(fx["num_objects"]))])
    calls = []

    def judge(predictions, context):
        calls.append((context["image"], context["annot_name"], context["top_k"]))
        return MC.crc_judge(predictions)
    preds, graphs, pct = ev.get_related_top_k_predictions_parallel(top_k, judge=judge, names=_names(fx))
    ref_preds, ref_graphs, ref_saved = MC.fixture_lists(fx, top_k)
    assert preds == ref_preds and pct == 0
    assert len(graphs) == len(ref_graphs) and all(MC.edges_equal(a, b) for a, b in zip(graphs, ref_graphs))
    assert calls == [(b, "image_%d_annotations.pkl" % b, top_k) for b in range(len(preds)) if preds[b]]
    written = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert written == sorted(ref_saved)
    for rel in written:
        assert MC.edges_equal(torch.load(os.path.join(str(tmp_path), rel)), ref_saved[rel]), rel
    np.testing.assert_array_equal(ev.confidence.cpu().numpy(), fx["ref_conf"])            # the state is left as it was: no `+= connectivity`


def test_evaluator_route_errors(fx, monkeypatch):
    ev, args = _evaluator()
    for step in MC.fixture_steps(fx):
        ev.accumulate(*[x.cuda() if torch.is_tensor(x) else x for x in step])
    ev.load_annotation_paths(["image_%d_annotations.pkl" % b for b in range(3)])
    import sys
    monkeypatch.setitem(sys.modules, "query_llm", None)               # no host repository on the path
    monkeypatch.setitem(sys.modules, "dataset_utils", None)
    with pytest.raises(RuntimeError, match="names"):
        ev.get_related_top_k_predictions_parallel(10, judge=MC.crc_judge)
    with pytest.raises(RuntimeError, match="judge"):
        ev.get_related_top_k_predictions_parallel(10, names=_names(fx))
    args["models"]["llm_model"] = "gpt4v"
    with pytest.raises(RuntimeError, match="gpt4v"):
        ev.get_related_top_k_predictions_parallel(10, names=_names(fx))
    with pytest.raises(ValueError):
        ev.get_related_top_k_predictions_parallel(129, judge=MC.crc_judge, names=_names(fx))
    ev.accumulate_target([None], [None], [None], [None], [None])
    with pytest.raises(ValueError, match="PredCLS"):
        ev.get_related_top_k_predictions_parallel(10, judge=MC.crc_judge, names=_names(fx))


# ------------------------------------------------------------------------------------------------ (b) property test
@pytest.fixture(scope="module")
def property_cases():
    """Every synthetic state fed once to a flat-head evaluator through ``accumulate`` (it takes max / argmax over the predicate axis,
    so a row holding the confidence at its predicate and -inf elsewhere reproduces the state)."""
    out = {}
    for name, st in MC.property_states():
        ev, _ = _evaluator(hierarchical=False)
        n = len(st["which"])
        rel = np.full((n, 50), -np.inf, dtype=np.float32)
        rel[np.arange(n), st["pred"]] = st["conf"]
        st = dict(st, pred=np.where(np.isinf(st["conf"]), 0, st["pred"]))          # argmax of an all -inf row is 0
        c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        ev.accumulate(c(st["which"]), c(rel), c(st["rel_t"]), None, torch.zeros(n, device="cuda"), c(st["scat"]), c(st["ocat"]),
                      c(st["scat_t"]), c(st["ocat_t"]), c(st["sbox"]), c(st["obox"]), c(st["sbox_t"]), c(st["obox_t"]),
                      torch.ones(n, dtype=torch.bool, device="cuda"))
        got = _state_of(ev)
        for k in MC.STATE_KEYS:
            np.testing.assert_array_equal(got[k], st[k], err_msg=name + " " + k)
        out[name] = (ev, st)
    return out


@pytest.mark.parametrize("top_k", MC.TOP_KS)
@pytest.mark.parametrize("name", [n for n, _ in MC.property_states()])
def test_kernel_matches_the_host_loop(property_cases, name, top_k):
    ev, st = property_cases[name]
    want = MC.related_top_k_host(st, top_k)
    images, pos, rank, count, conf = ev.related_top_k_device(top_k)
    assert images.tolist() == np.unique(st["which"]).tolist()
    pos, rank, count, conf = pos.cpu().numpy(), rank.cpu().numpy(), count.cpu().numpy(), conf.cpu().numpy()
    assert count.tolist() == [len(g) for g in want]
    for r, g in enumerate(want):
        assert list(zip(pos[r, :len(g)].tolist(), rank[r, :len(g)].tolist())) == g, (name, top_k, r)
        assert (pos[r, len(g):] == -1).all() and (rank[r, len(g):] == -1).all() and np.isnan(conf[r, len(g):]).all()
        np.testing.assert_array_equal(conf[r, :len(g)], st["conf"][[p for p, _ in g]])
    if name == "eleven_edges":
        assert count.tolist() == [{1: 1, 10: 10}.get(top_k, 11)]
        if top_k > 10:
            assert rank[0, 10] == 0 and rank[0, :10].tolist() == list(range(1, 11))     # rank 0 accepted last, after the count reached 10


def test_property_cases_reach_every_branch(property_cases):
    """The cases are worth their name: caps reached, -inf accepted, ties inside the window, images that yield nothing."""
    counts = {(n, k): [len(g) for g in MC.related_top_k_host(st, k)] for n, (_, st) in property_cases.items() for k in (10, 128)}
    assert any(max(c) == 11 for c in counts.values()) and any(10 in c for c in counts.values())
    assert any(0 in c for c in counts.values()) and max(max(c) for c in counts.values()) == 11
    assert sum(counts[("all_minus_inf", 10)]) > 0
    st = property_cases["many_ties"][1]
    top = np.sort(st["conf"][st["which"] == 0])[::-1][:64]
    assert len(np.unique(top)) < len(top) / 2
    st = property_cases["high_ranks"][1]
    assert max(j for g in MC.related_top_k_host(st, 128) for _, j in g) >= 65                # the second register set is read
    assert [len(g) for g in MC.related_top_k_host(st, 63)] != [len(g) for g in MC.related_top_k_host(st, 64)]   # rank 63 is accepted
    st = property_cases["ragged_8_images"][1]
    assert sorted(np.bincount(st["which"])[np.unique(st["which"])].tolist())[:3] == [1, 5, 31] and 5 not in st["which"]


# ------------------------------------------------------------------------------------------------ (c) fused route
@pytest.fixture(scope="module")
def model_and_batch():
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    args = cfg.args(run_mode="prepare_cs", fixtures=FX)
    model = BayesianRelationClassifier(args).cuda()
    model.load_state_dict(make_state_dict(cfg, seed=8, head_gain=6.0))
    model.eval()
    return model, make_scene_batch(cfg, (7, 3, 5, 4, 6), seed=33, connect_frac=0.5), args


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("top_k", [10, 40])
def test_fused_route_equals_the_evaluator_route(fx, model_and_batch, overlap, top_k, tmp_path):
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.pair_loop import evaluate_minibatch, mine_commonsense_candidates
    model, batch, args = model_and_batch
    args = dict(args, dataset=dict(args["dataset"], annot_dir=str(tmp_path)))
    ev = Evaluator(args, 50, 0.5, [20, 50, 100])
    evaluate_minibatch(model, batch, ev, None, overlap_filtering=overlap)
    ev.load_annotation_paths(["image_%d_annotations.pkl" % b for b in range(len(batch.bbox))])
    preds, graphs, _ = ev.get_related_top_k_predictions_parallel(top_k, judge=MC.crc_judge, names=_names(fx))
    mined = mine_commonsense_candidates(model, batch, top_k=top_k, overlap_filtering=overlap)
    got_preds, got_graphs = mined.to_lists(_names(fx))
    assert got_preds == preds and sum(len(p) for p in preds) >= len(preds)
    assert len(got_graphs) == len(graphs) and all(MC.edges_equal(a, b) for a, b in zip(got_graphs, graphs))
    assert [g == [[list(e[0]), e[1], list(e[2]), e[3], e[4]] for e in h] for g, h in zip(got_graphs, graphs)] == [True] * len(graphs)
    assert tuple(mined.pair.shape) == (len(batch.bbox), 16) and mined.count.tolist() == [len(p) for p in preds]
    # the fields index the forward's outputs: the score is the candidate's own confidence
    out = model.last_outputs
    for b in range(len(batch.bbox)):
        for e in range(int(mined.count[b])):
            assert float(mined.score[b, e]) == float(out.cand_conf[int(mined.pair[b, e]), int(mined.slot[b, e])])
            assert int(mined.predicate[b, e]) == int(out.cand_pred[int(mined.pair[b, e]), int(mined.slot[b, e])])


# ------------------------------------------------------------------------------------------------ (d) driver
class TinyVG(torch.utils.data.Dataset):
    """The reference loader's 9-tuples with the image slot holding the [256,32,32] encoder features (as tests/test_drivers_gpu.py),
    plus the two hooks of ``prepare_cs``: ``train_cs_step`` and a recording ``save_all_triplets``."""

    def __init__(self, cfg, n_items, seed):
        from scene_graph_commonsense_amd.synthetic import make_scene_batch
        sizes = [3 + (i * 5) % 4 for i in range(n_items)]
        self.b = make_scene_batch(cfg, sizes, seed=seed, connect_frac=0.5)
        self.train_cs_step, self.fetched, self.saved = None, [], 0

    def __len__(self):
        return len(self.b.bbox)

    def __getitem__(self, i):
        b = self.b
        self.fetched.append((self.train_cs_step, i))
        return (b.image_feature[i], b.image_feature[i] * 0.9 + 0.05, b.image_depth[i], b.categories[i], b.super_categories[i], b.bbox[i],
                b.relationships[i], b.subj_or_obj[i], "img_%d_annotations.pkl" % i)

    def save_all_triplets(self):
        self.saved += 1


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


@pytest.fixture(scope="module")
def driver(fx, tmp_path_factory):
    """Model, its checkpoint in the reference's naming, the dataset and the args of the three driver tests (built once)."""
    from scene_graph_commonsense_amd import train_test
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_state_dict
    root = tmp_path_factory.mktemp("prepare_cs")
    cfg = HeadConfig()
    args = cfg.args(run_mode="prepare_cs", fixtures=FX)
    args["models"]["feature_encoder"] = "precomputed"
    args["training"].update(batch_size=2, print_freq_test=1, eval_freq_test=1, test_epoch=0, save_vis_results=False,
                            result_path=str(root) + os.sep, checkpoint_path=str(root) + os.sep)
    model = train_test.build_classifier(args, 0)
    model.load_state_dict(make_state_dict(cfg, seed=9, head_gain=5.0))
    model.eval()
    train_test.save_checkpoint(model, train_test.checkpoint_name(args, 0, False)[1])
    return model, args, TinyVG(cfg, 4, seed=42), root


def _driver_args(driver, monkeypatch, fx, annot_dir, judge):
    from scene_graph_commonsense_amd.evaluator import Evaluator
    model, args, data, root = driver
    args = dict(args, models=dict(args["models"]), dataset=dict(args["dataset"], annot_dir=str(annot_dir)))
    if judge is not None:
        args["models"]["cs_judge"] = judge
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("MASTER_PORT", _free_port())
    monkeypatch.setattr(Evaluator, "names", _names(fx))
    return model, args, data, root


def test_eval_pc_prepare_cs_step_1(fx, driver, tmp_path, monkeypatch):
    """One aligned and one violated file per image that has edges, equal to a direct mining call on the driver's minibatches."""
    import json
    from scene_graph_commonsense_amd import evaluate, pair_loop
    from scene_graph_commonsense_amd.synthetic import SceneBatch
    annot_dir = tmp_path / "annot"
    model, args, data, root = _driver_args(driver, monkeypatch, fx, annot_dir, MC.crc_judge)
    evaluate.eval_pc(0, args, data, data, 1)
    assert data.train_cs_step == 1 and not torch.distributed.is_initialized()
    assert json.load(open(os.path.join(str(root), "test_results_0.json"))) == []          # step 1 writes no result record
    n_files = 0
    order = list(torch.utils.data.distributed.DistributedSampler(data, num_replicas=1, rank=0))       # the driver's own sampler
    for first in (0, 2):                                               # its two minibatches
        idx, b = order[first:first + 2], data.b
        mb = SceneBatch(torch.stack([b.image_feature[i] for i in idx]).cuda(), torch.stack([b.image_depth[i] for i in idx]).cuda(),
                        [b.bbox[i] for i in idx], [b.categories[i] for i in idx], [b.super_categories[i] for i in idx],
                        [b.relationships[i] for i in idx], [b.subj_or_obj[i] for i in idx])
        preds, graphs = pair_loop.mine_commonsense_candidates(model, mb, top_k=10).to_lists(_names(fx))
        for k, (p, g) in enumerate(zip(preds, graphs)):
            stem = "img_%d_pseudo_annotations.pkl" % idx[k]
            pa, pv = annot_dir / "cs_aligned_top10_gpt3p5_temp" / stem, annot_dir / "cs_violated_top10_gpt3p5_temp" / stem
            if not g:
                assert not pa.exists() and not pv.exists()
                continue
            resp = MC.crc_judge(p)
            assert MC.edges_equal(torch.load(str(pa)), [e for e, r in zip(g, resp) if r == 1])
            assert MC.edges_equal(torch.load(str(pv)), [e for e, r in zip(g, resp) if r != 1])
            n_files += 2
    assert n_files >= 2 and n_files == sum(len(fs) for _, _, fs in os.walk(str(annot_dir)))


def test_eval_pc_prepare_cs_step_1_needs_a_judge(fx, driver, tmp_path, monkeypatch):
    """Without ``args['models']['cs_judge']`` and without a host ``query_llm``: the documented error, and nothing written."""
    import sys
    from scene_graph_commonsense_amd import evaluate
    model, args, data, root = _driver_args(driver, monkeypatch, fx, tmp_path / "annot", None)
    monkeypatch.setitem(sys.modules, "query_llm", None)
    try:
        with pytest.raises(RuntimeError, match="judge"):
            evaluate.eval_pc(0, args, data, data, 1)
    finally:
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
    assert not (tmp_path / "annot").exists()


def test_eval_pc_prepare_cs_step_2(fx, driver, tmp_path, monkeypatch):
    """No forward: every item is fetched once under ``train_cs_step == 2`` and ``save_all_triplets`` is called once."""
    from scene_graph_commonsense_amd import evaluate
    model, args, data, root = _driver_args(driver, monkeypatch, fx, tmp_path / "annot", MC.crc_judge)

    def no_forward(*a, **k):
        raise AssertionError("step 2 must not build or run the model")
    monkeypatch.setattr(evaluate, "evaluate_minibatch", no_forward)
    monkeypatch.setattr(evaluate, "build_classifier", no_forward)
    data.fetched.clear()
    saved = data.saved
    evaluate.eval_pc(0, args, data, data, 2)
    assert data.train_cs_step == 2 and data.saved == saved + 1
    assert sorted(data.fetched) == [(2, i) for i in range(4)]
    assert not torch.distributed.is_initialized()


def test_eval_pc_rejects_a_step_without_the_run_mode(driver):
    from scene_graph_commonsense_amd import evaluate
    model, args, data, root = driver
    with pytest.raises(ValueError, match="prepare_cs_step"):
        evaluate.eval_pc(0, args, data, data, -1)
    eval_args = dict(args, training=dict(args["training"], run_mode="eval"))
    with pytest.raises(ValueError, match="prepare_cs_step"):
        evaluate.eval_pc(0, eval_args, data, data, 1)
