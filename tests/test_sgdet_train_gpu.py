"""SGDET / SGCLS training on the device: ``sgc_assign_pair_targets`` against the plain-loop restatement of tests/sgdet_train_cases.py,
the identity with the PredCLS targets, ``train_sgdet_minibatch`` against ``train_minibatch`` bit for bit, the image-group path of an
assigned scene, and the C ABI's argument checks."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import sgdet_train_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _detected_scene(cfg, num_objects, cats, boxes, feature=None, depth=None):
    """The DeviceScene of detections given flat (classes, boxes) and per-image counts - what ``pair_loop._sgdet_scene`` builds."""
    from scene_graph_commonsense_amd.pairs import flatten_scene
    from scene_graph_commonsense_amd.synthetic import SceneBatch, default_sub2super
    B, F = len(num_objects), cfg.feature_size
    off = np.concatenate([[0], np.cumsum(num_objects)])
    table = default_sub2super(cfg.num_classes, cfg.num_super_classes)
    cl = [torch.from_numpy(np.asarray(cats[off[b]:off[b + 1]], dtype=np.int64)) for b in range(B)]
    bl = [torch.from_numpy(np.asarray(boxes[off[b]:off[b + 1]], dtype=np.float32).reshape(-1, 4)) for b in range(B)]
    sp = [[torch.as_tensor(table[int(c)]) for c in cs.tolist()] for cs in cl]
    feature = torch.zeros(B, 2 * cfg.hidden_dim, F, F) if feature is None else feature
    depth = torch.zeros(B, 1, F, F) if depth is None else depth
    return flatten_scene(cfg, SceneBatch(feature, depth, bl, cl, sp, None, None), DEV)


def _check(assignment, ref, scene):
    for name in ("directed", "raw", "matched", "target_hit"):
        got = getattr(assignment, name)
        assert got.dtype == torch.int32 and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), ref[name], err_msg=name)
    assert scene.directed is assignment.directed and scene.raw_target is assignment.raw
    counts = assignment.counts()
    assert counts.dtype == torch.int64 and counts.is_cuda
    assert counts.tolist() == [len(ref["target_hit"]), int(ref["target_hit"].sum()), int((ref["matched"] >= 0).sum())]


@pytest.fixture(scope="module")
def cases():
    return dict(crafted=C.crafted(), drawn=C.drawn())


@pytest.mark.parametrize("equiv", [True, False])
@pytest.mark.parametrize("name", ["crafted", "drawn"])
def test_assignment_equals_the_restatement(cases, name, equiv):
    from scene_graph_commonsense_amd.pair_loop import assign_sgdet_targets, upload_sgdet_targets
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    c = cases[name]
    ref = C.assign_reference(c["num_objects"], c["cats"], c["boxes"], c["table"], C.equiv_table() if equiv else None, c["R"])
    scene = _detected_scene(HeadConfig(), c["num_objects"], c["cats"], c["boxes"])
    table = upload_sgdet_targets(c["table"], len(c["num_objects"]), DEV)
    got = assign_sgdet_targets(scene, table, equiv=equiv, num_relations=c["R"])
    print(name, "equiv", equiv, "pairs", scene.n_pairs, "rows", len(ref["target_hit"]), "counts", got.counts().tolist())
    _check(got, ref, scene)
    # the six-array table (metrics.upload_sg_targets): the row pointer derived on the device
    scene6 = _detected_scene(HeadConfig(), c["num_objects"], c["cats"], c["boxes"])
    _check(assign_sgdet_targets(scene6, table[:6], equiv=equiv, num_relations=c["R"]), ref, scene6)
    if equiv:                                   # an explicit table is read like the built-in one
        eq = torch.from_numpy(C.equiv_table()).to(DEV)
        third = assign_sgdet_targets(_detected_scene(HeadConfig(), c["num_objects"], c["cats"], c["boxes"]), table, equiv=eq,
                                     num_relations=c["R"])
        assert torch.equal(third.matched, got.matched)


def test_assignment_without_targets_and_without_pairs(cases):
    from scene_graph_commonsense_amd.pair_loop import assign_sgdet_targets, upload_sgdet_targets
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    c = cases["crafted"]
    empty = tuple(a[:0] for a in c["table"])
    scene = _detected_scene(HeadConfig(), c["num_objects"], c["cats"], c["boxes"])
    got = assign_sgdet_targets(scene, upload_sgdet_targets(empty, 3, DEV), num_relations=c["R"])
    P = scene.n_pairs
    assert P == 62 and got.target_hit.numel() == 0
    for t in (got.directed, got.raw, got.matched):
        assert t.numel() == P and bool((t == -1).all())
    assert got.counts().tolist() == [0, 0, 0]
    # one detection per image: no pairs, no launch - target_hit is cleared all the same
    lone = _detected_scene(HeadConfig(), [1, 1, 1], c["cats"][[0, 5, 6]], c["boxes"][[0, 5, 6]])
    got = assign_sgdet_targets(lone, upload_sgdet_targets(c["table"], 3, DEV), num_relations=c["R"])
    assert lone.n_pairs == 0 and got.directed.numel() == 0 and got.matched.numel() == 0
    assert got.target_hit.numel() == 9 and got.counts().tolist() == [9, 0, 0]


@pytest.mark.parametrize("which", ["vg_full", "drawn_gt"])
def test_identity_with_the_predcls_targets_on_the_device(cases, which):
    """The PredCLS batches of tests/test_sgdet_train_cpu.py's identity test: detections = ground-truth objects."""
    from scene_graph_commonsense_amd.pair_loop import assign_sgdet_targets, upload_sgdet_targets
    from scene_graph_commonsense_amd.pairs import flatten_scene, sg_target_table
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    cfg = HeadConfig()
    batch = C.identity_case()[2] if which == "vg_full" else cases["drawn"]["gt"]
    pred = flatten_scene(cfg, batch, DEV)
    n = [int(b.shape[0]) for b in batch.bbox]
    det = _detected_scene(cfg, n, torch.cat(batch.categories).numpy(), torch.cat(batch.bbox).float().numpy())
    table = sg_target_table(batch.relationships, batch.subj_or_obj, batch.categories, batch.bbox, drop_last_graph_object=False)
    got = assign_sgdet_targets(det, upload_sgdet_targets(table, len(n), DEV), num_relations=cfg.num_relations)
    assert int((pred.directed >= 0).sum()) == len(table[1]) > 0
    assert torch.equal(got.directed, pred.directed) and torch.equal(got.raw, pred.raw_target)
    assert got.counts().tolist() == [len(table[1])] * 3


# ------------------------------------------------------------------------------------------------------------ training steps
@pytest.fixture(scope="module")
def vg_full_model():
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    cfg, sd, _ = C.identity_case()
    model = BayesianRelationClassifier(cfg.args()).to(DEV)
    model.load_state_dict(sd)
    model.eval()                                # dropout off
    return cfg, model


def _commonsense():
    from tests.golden_cases import GOLDEN
    fx = os.path.join(GOLDEN, "ref_fixtures") + os.sep
    return (list(torch.load(fx + "commonsense_aligned_triplets.pt").keys()), list(torch.load(fx + "commonsense_violated_triplets.pt").keys()))


def _step(model, fn):
    model.zero_grad(set_to_none=True)
    loss = fn()
    torch.cuda.synchronize()
    return dict(loss=loss.detach().clone(), grads={n: p.grad.clone() for n, p in model.named_parameters()},
                stats=model.last_connectivity_stats.tolist(), rel=model.last_outputs.relation.clone(), groups=list(model.last_image_groups))


@pytest.mark.parametrize("case", ["area", "area+commonsense", "as_stored"])
def test_twin_step_equals_the_predcls_step_bit_for_bit(vg_full_model, case):
    """``train_sgdet_minibatch`` with detections equal to the ground truth against ``train_minibatch`` on the PredCLS batch: the same
    loss and the same gradient of every parameter, bit for bit (eval mode, ``optimizer=None``).  The batch is vg_full - weights,
    features, 5 / 4 / 3 objects.  'area': its zero-area object (7,7,2,9) widened to (7,8,2,9) in ground truth and detections alike, see
    ``sgdet_train_cases.identity_case`` - as stored, 5 of the 12 relations touch an object evaluation can never credit (grid IoU 0
    with itself), and those the assignment must NOT hand out.  'as_stored': vg_full untouched; the PredCLS twin is then the batch
    without exactly those 5 relations."""
    from scene_graph_commonsense_amd.pair_loop import train_minibatch, train_sgdet_minibatch
    from scene_graph_commonsense_amd.synthetic import default_sub2super
    cfg, model = vg_full_model
    batch = C.identity_case(give_area=case != "as_stored")[2]
    twin = batch
    if case == "as_stored":
        twin, dropped = C.without_uncreditable(batch)
        assert dropped == 5
    kw = dict(lambda_connectivity=0.15)
    if case.endswith("commonsense"):
        kw.update(commonsense=_commonsense(), lambda_commonsense=0.5)
    cats, boxes, targets = C.detections_of(batch)
    one = _step(model, lambda: train_minibatch(model, twin, None, **kw))
    two = _step(model, lambda: train_sgdet_minibatch(model, batch.image_feature, batch.image_depth, cats, boxes, targets,
                                                     sub2super=default_sub2super(cfg.num_classes, cfg.num_super_classes), **kw))
    print(case, "loss", float(one["loss"]), float(two["loss"]), "stats", one["stats"], two["stats"],
          "assignment counts", model.last_assignment.counts().tolist())
    assert float(one["loss"]) != 0.0 and torch.isfinite(one["loss"])
    assert torch.equal(one["loss"], two["loss"])
    for n in one["grads"]:
        assert torch.equal(one["grads"][n], two["grads"][n]), n
    assert one["stats"] == two["stats"] and torch.equal(one["rel"], two["rel"])
    assert model.last_assignment.counts().tolist() == [12, 12 if case != "as_stored" else 7, 12 if case != "as_stored" else 7]


def _two_group_budget(cfg, bbox_pred, share=1.0):
    """A workspace budget under which ``plan_image_groups`` cuts the minibatch into exactly two image groups (host arithmetic only);
    ``share``: the part of the budget ``train_minibatch`` plans with (0.85 with an augmented view)."""
    from scene_graph_commonsense_amd.pair_loop import image_workspace_bytes, plan_image_groups
    cost = [1.15 * image_workspace_bytes(cfg, b, True) for b in bbox_pred]
    holder = types.SimpleNamespace(bbox=bbox_pred)
    for k in range(1, len(cost)):
        budget = 1.001 * max(sum(cost[:k]), sum(cost[k:]))
        if len(plan_image_groups(cfg, holder, True, budget)) == 2:
            return budget / share
    raise AssertionError("no budget gives two groups")


@pytest.mark.parametrize("terms", ["plain", "coupled"])
def test_image_groups_of_an_assigned_scene_equal_the_one_pass_step(vg_full_model, cases, terms):
    """'coupled': with the contrastive and the commonsense term, which read the assigned targets of EVERY group's pairs before any
    group's backward runs (``pair_loop._coupled_terms``)."""
    from scene_graph_commonsense_amd.pair_loop import train_sgdet_minibatch
    from scene_graph_commonsense_amd.synthetic import default_sub2super, hash_normal
    cfg, model = vg_full_model
    d = cases["drawn"]
    gt = d["gt"]
    s2s = default_sub2super(cfg.num_classes, cfg.num_super_classes)
    kw = dict(lambda_connectivity=0.15)
    if terms == "coupled":
        f = gt.image_feature
        kw.update(image_feature_aug=(0.9 * f + 0.3 * torch.from_numpy(hash_normal(4242, f.numel()).reshape(f.shape))).to(DEV),
                  lambda_contrast=0.7, commonsense=_commonsense(), lambda_commonsense=0.5)
    res = []
    for budget in (1e15, _two_group_budget(cfg, d["bbox_pred"], 0.85 if terms == "coupled" else 1.0)):
        model.last_contrast_loss = None
        res.append(_step(model, lambda: train_sgdet_minibatch(model, gt.image_feature, gt.image_depth, d["cats_pred"], d["bbox_pred"], d["targets"],
                                                              sub2super=s2s, workspace_budget=budget, **kw)))
        res[-1]["contrast"] = None if model.last_contrast_loss is None else float(model.last_contrast_loss)
    one, many = res
    if terms == "coupled":
        # the tolerances of tests/test_chunking_gpu.py::test_chunked_step_with_minibatch_coupled_terms_equals_the_one_pass_step
        print("contrastive", one["contrast"], many["contrast"])
        assert one["contrast"] is not None and abs(one["contrast"] - many["contrast"]) <= 1e-6 * abs(one["contrast"])
        assert abs(float(one["loss"]) - float(many["loss"])) <= 1e-5 * abs(float(one["loss"]))
        assert len(one["groups"]) == 1 and len(many["groups"]) == 2 and torch.equal(one["rel"], many["rel"])
        for n in one["grads"]:
            e = float((one["grads"][n].double() - many["grads"][n].double()).norm() / one["grads"][n].double().norm().clamp(min=1e-30))
            print(n, "%.1e" % e)
            assert e <= (1e-4 if n.startswith(("conv1", "conv2")) else 1e-5), (n, e)
        return
    ref = C.assign_reference(d["num_objects"], d["cats"], d["boxes"], d["table"], C.equiv_table(), d["R"])
    np.testing.assert_array_equal(model.last_assignment.directed.cpu().numpy(), ref["directed"])
    print("groups", many["groups"], "loss", float(one["loss"]), float(many["loss"]), "stats", one["stats"], many["stats"])
    assert len(one["groups"]) == 1 and len(many["groups"]) == 2
    assert one["stats"][1] == int((ref["directed"] >= 0).sum()) > 0
    # the tolerances of tests/test_chunking_gpu.py::test_chunked_training_step_equals_the_one_pass_step (the PredCLS path's comparison)
    assert abs(float(one["loss"]) - float(many["loss"])) <= 1e-5 * abs(float(one["loss"]))
    assert torch.equal(one["rel"], many["rel"]) and one["stats"] == many["stats"]
    worst = {n: float((one["grads"][n].double() - many["grads"][n].double()).norm() / one["grads"][n].double().norm().clamp(min=1e-30))
             for n in one["grads"]}
    print({k: "%.1e" % v for k, v in worst.items()})
    for n, e in worst.items():
        assert e <= 2e-4, (n, e)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_return_err_arg(cases):
    from scene_graph_commonsense_amd import _lib
    from scene_graph_commonsense_amd.metrics import scene_boxes
    from scene_graph_commonsense_amd.pair_loop import assign_sgdet_targets, upload_sgdet_targets
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    c = cases["crafted"]
    scene = _detected_scene(HeadConfig(), c["num_objects"], c["cats"], c["boxes"])
    table = upload_sgdet_targets(c["table"], 3, DEV)
    with pytest.raises(RuntimeError, match="status 1"):
        assign_sgdet_targets(scene, table, num_relations=c["R"], feature_size=129)
    assert scene.directed is None                                           # nothing was set
    with pytest.raises(RuntimeError, match="cuda"):
        assign_sgdet_targets(scene, tuple(t.cpu() for t in table), num_relations=c["R"])
    P, T = scene.n_pairs, 9
    out = torch.full((3 * P + T,), 7, dtype=torch.int32, device=DEV)
    outs = [out[:P], out[P:2 * P], out[2 * P:3 * P], out[3 * P:]]
    lib = _lib.load()

    def call(F=32, null=None, pairs=P, R=c["R"]):
        o = [None if i == null else t for i, t in enumerate(outs)]
        return lib.sgc_assign_pair_targets(
            _lib.ptr(scene.sub_idx), _lib.ptr(scene.obj_idx), _lib.ptr(scene.image), pairs, _lib.ptr(scene.pid), int(scene.pid.shape[1]),
            _lib.ptr(scene.img_ptr), _lib.ptr(scene.cats), _lib.ptr(scene_boxes(scene, DEV)), int(scene.cats.numel()), _lib.ptr(table[6]), 3,
            _lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(table[3]), _lib.ptr(table[4]), _lib.ptr(table[5]), T, _lib.ptr(None), 0, R, F,
            ctypes.c_double(0.5), _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]), _lib.ptr(o[3]), _lib.stream_ptr())

    assert call(F=129) == 1 and call(F=0) == 1 and call(pairs=-1) == 1 and call(R=0) == 1
    for k in range(4):
        assert call(null=k) == 1, k
    torch.cuda.synchronize()
    assert bool((out[:3 * P] == 7).all())                                   # a refused call writes no pair output
    assert call() == 0
    torch.cuda.synchronize()
    ref = C.assign_reference(c["num_objects"], c["cats"], c["boxes"], c["table"], None, c["R"])
    np.testing.assert_array_equal(outs[2].cpu().numpy(), ref["matched"])
    np.testing.assert_array_equal(outs[3].cpu().numpy(), ref["target_hit"])
