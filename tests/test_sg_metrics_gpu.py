"""GPU tests of the device-resident SGDET / SGCLS metrics (``sgc_recall_accumulate_targets``, ``metrics.RecallMeter.update(sg_targets=,
cat_conf=)``, ``pair_loop.score_sgdet_minibatch``, the ``device_metrics`` switch of ``evaluate.eval_sgd`` / ``eval_sgc``): the kernel
against the host restatement of ``Evaluator.compute(predcls=False)`` on synthetic states and against the PredCLS kernel, the fused route
against the evaluator route counter for counter, the reference's own numbers, and the drivers."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import metrics_cases as MC
from tests import sg_metrics_cases as SG
from tests import sgdet_case
from tests.golden_cases import GOLDEN
from tests.test_metrics_gpu import _DeviceState, _assert_counters, _dev, _plain, _same, retarget

pytestmark = pytest.mark.gpu
FX = os.path.join(GOLDEN, "ref_fixtures") + os.sep
GOLD = np.load(os.path.join(GOLDEN, "sgdet_vg.npz"))
TOP_K = [20, 50, 100]
NAMES = ("hits", "hits_pc", "targets", "targets_pc", "zs_hits", "zs_hits_pc", "zs_targets", "zs_targets_pc")


# ------------------------------------------------------------------------------------------------ the kernel through the C ABI
def _zero_counters(n_k, R):
    sizes = dict(hits=n_k, hits_pc=n_k * R, targets=1, targets_pc=R)
    return {k: torch.zeros(sizes[k[3:] if k.startswith("zs_") else k], dtype=torch.int64, device="cuda") for k in NAMES}


def _unaligned(a):
    """The [T,4] f32 array on the device at an address that is no multiple of 16 (the target table promises no alignment)."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).cuda()
    view = buf[1:]
    assert a.size == 0 or view.data_ptr() % 16 != 0
    return view


def accumulate_targets(st, rk, tg, equiv, counters=None, top_k=MC.TOP_K, K=None, zero_shot=True, check=True):
    """``sgc_recall_accumulate_targets`` on numpy tables; returns the counters (or the status with ``check=False``)."""
    from scene_graph_commonsense_amd import _lib as L
    lib = L.load()
    n_k, R = len(top_k), st["R"]
    d = {k: _dev(rk[k]) for k in ("predicate", "subject", "object", "count")}
    cats, boxes = _dev(st["cats"]), _dev(st["boxes"])
    t = {k: _dev(tg[k]) for k in ("image", "rel", "scat", "ocat")}
    sbox, obox = _unaligned(tg["sbox"]), _dev(tg["obox"])
    eq = None if equiv is None else _dev(equiv.astype(np.uint8))
    zs = _dev(MC.zero_shot_words(st).view(np.int32)) if zero_shot else None
    c = counters if counters is not None else _zero_counters(min(n_k, 8), R)
    z = (lambda k: L.ptr(c[k])) if zero_shot else (lambda k: L.ptr(None))
    status = lib.sgc_recall_accumulate_targets(
        L.ptr(d["predicate"]), L.ptr(d["subject"]), L.ptr(d["object"]), L.ptr(d["count"]), st["n_img"],
        int(rk["subject"].shape[1]) if K is None else K, L.ptr(cats), L.ptr(boxes), int(st["cats"].shape[0]), L.ptr(t["image"]),
        L.ptr(t["rel"]), L.ptr(t["scat"]), L.ptr(t["ocat"]), L.ptr(sbox), L.ptr(obox), int(tg["rel"].shape[0]), L.ptr(eq),
        0 if equiv is None else int(equiv.shape[0]), (ctypes.c_int * n_k)(*top_k), n_k, L.ptr(zs), st["C"], R, st["F"],
        ctypes.c_double(MC.IOU), L.ptr(c["hits"]), L.ptr(c["hits_pc"]), L.ptr(c["targets"]), L.ptr(c["targets_pc"]), z("zs_hits"),
        z("zs_hits_pc"), z("zs_targets"), z("zs_targets_pc"), L.stream_ptr())
    torch.cuda.synchronize()
    if not check:
        return status
    L.check(status, "sgc_recall_accumulate_targets")
    return c


# ------------------------------------------------------------------------------------------------ 1. kernel against the host restatement
@pytest.mark.parametrize("use_equiv", [True, False])
@pytest.mark.parametrize("K", SG.KS)
@pytest.mark.parametrize("name", [n for n, _ in SG.states()])
def test_kernel_matches_the_host_restatement(name, K, use_equiv):
    from scene_graph_commonsense_amd.evaluator import _equiv_matrix
    st = dict(SG.states())[name]
    rk = SG.ranked_lists(st, K)
    want, seen = SG.sg_counters(st, rk, use_equiv)
    assert want["targets"][0] > 0 and 0 < want["hits"][0] and (K < 100 or want["hits"][0] < want["hits"][2] < want["targets"][0])
    equiv = _equiv_matrix() if use_equiv else None
    got = accumulate_targets(st, rk, st["targets"], equiv)
    _assert_counters(got, want, 1, (name, K, use_equiv))
    _assert_counters(accumulate_targets(st, rk, st["targets"], equiv, counters=got), want, 2, (name, K, use_equiv, "twice"))


# ------------------------------------------------------------------------------------------------ 2. cross-check with the PredCLS kernel
@pytest.mark.parametrize("K", MC.KS)
@pytest.mark.parametrize("name", [n for n, _ in MC.states()])
def test_connected_rows_as_a_table_give_the_predcls_counters(name, K):
    """The scene's connected rows of the kept steps, written as a target table (classes and boxes of the rows' objects, no
    equivalence table), count exactly as ``sgc_recall_accumulate`` counts the rows themselves."""
    st = dict(MC.states())[name]
    rk = MC.rank_host(st, K)
    want = _DeviceState(st).recall(rk, top3=False)
    rows = np.nonzero((st["directed"] != -1) & (st["included"] != 0 if st["included"] is not None else True))[0]
    s, o = st["sub_idx"][rows], st["obj_idx"][rows]
    tg = dict(image=st["image"][rows].astype(np.int32), rel=st["directed"][rows].astype(np.int64), scat=st["cats"][s], ocat=st["cats"][o],
              sbox=st["boxes"][s], obox=st["boxes"][o])
    got = accumulate_targets(st, rk, tg, None)
    assert int(want["targets"][0]) == len(rows) > 0
    for k in NAMES:
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), err_msg="%s %s %s" % (name, K, k))


# ------------------------------------------------------------------------------------------------ the SGDET case, both routes
@pytest.fixture(scope="module")
def sg(tmp_path_factory):
    """The seeded SGDET case with the stored targets: model, the front end's object lists (SGDET) and the matched lists (SGCLS), and
    args whose zero-shot file also holds every other ground-truth triple of the case (so that zero-shot targets exist)."""
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    from scene_graph_commonsense_amd.object_frontend import DetrFrontEnd
    from scene_graph_commonsense_amd.pairs import sg_target_table
    from scene_graph_commonsense_amd.synthetic import default_sub2super
    cfg, sd, batch, logits, boxes = sgdet_case.make_case()
    sgdet_case.apply_stored_targets(batch, GOLD)
    args = cfg.args(fixtures=FX)
    model = BayesianRelationClassifier(args).cuda()
    model.load_state_dict(sd)
    model.eval()
    fe = DetrFrontEnd(sgdet_case.alp2fre_table().tolist())
    cats, confs, bxs, kept = fe.sgdet(logits.cuda(), boxes.cuda())
    assert kept == [0, 1, 2]
    matched = fe.match_object_categories(cats, confs, bxs, [b.float().cuda() for b in batch.bbox])
    assert sum(len(x) for x in matched[0]) > sum(sgdet_case.NOBJ)        # repeated-box ties duplicate some ground-truth boxes
    targets = (batch.relationships, batch.subj_or_obj, batch.categories, batch.bbox)
    _, rel, scat, ocat, _, _ = sg_target_table(*targets)
    own = ["%d_%d_%d" % (scat[t], rel[t], ocat[t]) for t in range(0, len(rel), 2)]
    path = str(tmp_path_factory.mktemp("zs") / "zero_shot_triplets.pt")
    torch.save(list(torch.load(FX + "zero_shot_triplets.pt")) + own, path)
    args["dataset"]["zero_shot_triplets"] = path
    return types.SimpleNamespace(cfg=cfg, args=args, model=model, batch=batch, targets=targets, sgdet=(cats, confs, bxs), sgcls=matched[:3],
                                 sub2super=default_sub2super(cfg.num_classes, cfg.num_super_classes))


def _routes(sg, lists, ev, meter, **kw):
    """One minibatch through both routes; returns the evaluator's 6-tuple (computed, then cleared)."""
    from scene_graph_commonsense_amd.pair_loop import evaluate_sgdet_minibatch, score_sgdet_minibatch
    feat, depth = sg.batch.image_feature.cuda(), sg.batch.image_depth.cuda()
    evaluate_sgdet_minibatch(sg.model, feat, depth, *lists, ev, sub2super=sg.sub2super, targets=sg.targets, **kw)
    want = ev.compute(per_class=True, predcls=False)
    ev.clear_data()
    scene, out = score_sgdet_minibatch(sg.model, feat, depth, *lists, meter, sub2super=sg.sub2super, targets=sg.targets, **kw)
    assert out is sg.model.last_outputs and scene.n_pairs == int(out.cand_conf.shape[0])
    return want


def _new(sg):
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.metrics import RecallMeter
    return Evaluator(sg.args, sg.cfg.num_relations, 0.5, TOP_K), RecallMeter(sg.args, sg.cfg.num_relations, iou_thresh=0.5, top_k=TOP_K,
                                                                             device="cuda:0")


def _assert_counters_equal(meter, ev):
    i64 = lambda x: np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x).astype(np.int64)
    view = lambda n: meter.view(n).cpu().numpy()
    for name, sfx in (("recall", ""), ("zero_shot", "_zs")):
        np.testing.assert_array_equal(view(name + ".hits"), i64([getattr(ev, "result_dict" + sfx)[k] for k in TOP_K]), err_msg=name)
        np.testing.assert_array_equal(view(name + ".hits_pc"), np.stack([i64(getattr(ev, "result_per_class" + sfx)[k]) for k in TOP_K]), err_msg=name)
        assert int(view(name + ".targets")[0]) == int(getattr(ev, "num_connected_target" + sfx)), name
        np.testing.assert_array_equal(view(name + ".targets_pc"), i64(getattr(ev, "num_conn_target_per_class" + sfx)), err_msg=name)
    for part in ("top3.hits", "top3.hits_pc", "top3.targets", "top3.targets_pc", "precision.ap", "precision.ap_union", "precision.num_ap"):
        assert int(meter.view(part).abs().sum()) == 0, part            # eval_sgd / eval_sgc record neither Top-3 nor wmAP


# ------------------------------------------------------------------------------------------------ 3. fused route = evaluator route
@pytest.mark.parametrize("overlap,skip", [(True, False), (False, False), (True, True)])
def test_fused_sgdet_route_equals_the_evaluator_route(sg, overlap, skip):
    ev, meter = _new(sg)
    want = _routes(sg, sg.sgdet, ev, meter, overlap_filtering=overlap, skip_filtered=skip)
    print("evaluator: hits %s targets %d zero-shot hits %s targets %d" % ([ev.result_dict[k] for k in TOP_K], ev.num_connected_target,
                                                                          [ev.result_dict_zs[k] for k in TOP_K], ev.num_connected_target_zs))
    assert 0 < ev.result_dict[100] and 0 < ev.num_connected_target_zs < ev.num_connected_target       # the condition, on the Evaluator's numbers
    _assert_counters_equal(meter, ev)
    assert _same(meter.compute(per_class=True), want)


# ------------------------------------------------------------------------------------------------ 4. the reference's own numbers
def test_sgdet_meter_matches_the_reference_golden(sg):
    ev, meter = _new(sg)
    _routes(sg, sg.sgdet, ev, meter)
    assert meter.view("recall.hits").tolist() == [int(h) for h in GOLD["hits"].tolist()]
    assert int(meter.view("recall.targets")[0]) == int(GOLD["num_connected_target"])
    np.testing.assert_allclose(np.array([float(r) for r in meter.compute(per_class=True)[0]]), GOLD["recall"], atol=0.1)


# ------------------------------------------------------------------------------------------------ 5. SGCLS
def test_fused_sgcls_route_equals_the_evaluator_route(sg):
    ev, meter = _new(sg)
    want = _routes(sg, sg.sgcls, ev, meter)
    assert ev.num_connected_target > 0
    _assert_counters_equal(meter, ev)
    assert _same(meter.compute(per_class=True), want)


# ------------------------------------------------------------------------------------------------ 6. running counters
def test_sg_counters_run_on_across_minibatches(sg):
    ev, meter = _new(sg)
    seen = []
    for lists in (sg.sgdet, sg.sgcls):
        want = _routes(sg, lists, ev, meter)
        _assert_counters_equal(meter, ev)
        assert _same(meter.compute(per_class=True), want)
        seen.append(ev.num_connected_target)
    assert seen[1] > seen[0] > 0
    meter.reset()
    assert int(meter.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ 7. drivers
@pytest.mark.parametrize("mode", ["sgd", "sgc"])
def test_sg_drivers_with_device_metrics_write_the_same_records(tmp_path, monkeypatch, mode):
    from scene_graph_commonsense_amd import evaluate, train_test
    from scene_graph_commonsense_amd.metrics import RecallMeter
    from scene_graph_commonsense_amd.synthetic import make_state_dict
    from tests.test_drivers_gpu import FakeDetr, TinySGDet, _args, _free_port
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("WORLD_SIZE", "1")
    cfg, args = _args(tmp_path, "eval")
    args["models"].update(feature_encoder=FakeDetr(), topk_cat=2, nms=0.5)
    args["dataset"]["object_class_alp2fre"] = sgdet_case.alp2fre_table().tolist()
    args["training"]["eval_mode"] = mode
    model = train_test.build_classifier(args, 0)
    model.load_state_dict(make_state_dict(cfg, seed=9, head_gain=5.0))
    train_test.save_checkpoint(model, train_test.checkpoint_name(args, 0, False)[1])
    data = TinySGDet(cfg, 4, seed=77)
    data.b = retarget(model.eval(), cfg, data.b, seed=3, frac=1.0)       # ground truth from the model's own predictions: hits exist
    del model
    fed, reads, update, compute = [], [], RecallMeter.update, RecallMeter.compute
    monkeypatch.setattr(RecallMeter, "update", lambda self, *a, **k: (fed.append(k.get("sg_targets") is not None), update(self, *a, **k))[1])
    monkeypatch.setattr(RecallMeter, "compute", lambda self, *a, **k: (reads.append(1), compute(self, *a, **k))[1])
    records, returned = [], []
    for device_metrics in (False, True):
        monkeypatch.setenv("MASTER_PORT", _free_port())
        run = dict(args, training=dict(args["training"], device_metrics=device_metrics))
        returned.append((evaluate.eval_sgd if mode == "sgd" else evaluate.eval_sgc)(0, run, data))
        records.append(json.load(open(os.path.join(str(tmp_path), "test_results_0.json"))))
        assert not torch.distributed.is_initialized()
    assert fed == [True, True]                                   # the meter was fed on the device-metrics run only, once per minibatch
    assert len(records[0]) == 2 and len(records[0][-1]["recall_relationship"]) == 3 and len(reads) == len(records[1])
    assert 0.0 < records[0][-1]["recall_relationship"][2] <= 1.0     # the condition, on the evaluator route's record
    assert _same(_plain(records[1]), _plain(records[0]))
    assert _same(returned[1], returned[0])


# ------------------------------------------------------------------------------------------------ 8. errors
def test_sg_meter_errors(sg):
    from scene_graph_commonsense_amd.metrics import upload_sg_targets
    from scene_graph_commonsense_amd.pair_loop import score_sgdet_minibatch
    from scene_graph_commonsense_amd.pairs import sg_target_table
    _, meter = _new(sg)
    feat, depth = sg.batch.image_feature.cuda(), sg.batch.image_depth.cuda()
    with pytest.raises(ValueError, match="targets"):
        score_sgdet_minibatch(sg.model, feat, depth, *sg.sgdet, meter, sub2super=sg.sub2super, targets=None)
    scene, out = score_sgdet_minibatch(sg.model, feat, depth, *sg.sgdet, meter, sub2super=sg.sub2super, targets=sg.targets)
    meter.reset()
    table = sg_target_table(*sg.targets)
    dev_table = upload_sg_targets(table, "cuda:0")
    with pytest.raises(RuntimeError, match="GPU"):
        meter.update(scene, out, sg_targets=tuple(torch.from_numpy(a) for a in table))
    with pytest.raises(RuntimeError, match="GPU"):
        meter.update(scene, out, sg_targets=dev_table, cat_conf=torch.zeros(scene.n_pairs))
    with pytest.raises(ValueError, match="length"):
        meter.update(scene, out, sg_targets=dev_table[:4] + (dev_table[4][:-1], dev_table[5]))
    with pytest.raises(ValueError, match="length"):
        meter.update(scene, out, sg_targets=(dev_table[0][:-1],) + dev_table[1:])
    with pytest.raises(ValueError, match="directed"):
        meter.update(scene, out, sg_targets=dev_table, directed=torch.zeros(scene.n_pairs, dtype=torch.int32, device="cuda"))
    assert int(meter.counters.abs().sum()) == 0


@pytest.mark.parametrize("K,n_k", [(0, 3), (129, 3), (100, 9)])
def test_argument_checks_return_sgc_err_arg(K, n_k):
    st = dict(SG.states())["crafted"]
    rk = SG.ranked_lists(st, 100)
    top_k = tuple(range(10, 10 + n_k))
    counters = _zero_counters(9, st["R"])
    assert accumulate_targets(st, rk, st["targets"], None, counters=counters, top_k=top_k, K=K, check=False) == 1      # SGC_ERR_ARG
    assert accumulate_targets(st, rk, st["targets"], None, counters=counters, zero_shot=False, check=False) == 0
    assert sum(int(v.abs().sum()) for k, v in counters.items() if k.startswith("zs_")) == 0 and int(counters["targets"][0]) > 0
    empty = {k: v[:0] for k, v in st["targets"].items()}
    assert accumulate_targets(st, rk, empty, None, check=False) == 0                                                  # n_targets == 0 is SGC_OK
