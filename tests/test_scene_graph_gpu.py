"""GPU tests of scene-graph inference (``sgc_scene_graph_topk``, ``scene_graph.rank_scene_graphs``, ``pair_loop.predict_scene_graphs``):

* the kernel against a numpy restatement (a stable argsort over the tie key) on inputs full of ties and -inf, bit for bit;
* ``predict_scene_graphs`` against the evaluator route (``evaluate_minibatch`` into an ``Evaluator``, ``compute()``, ``last_topk``
  mapped through the evaluator's stored arrays): identical predicates, categories, boxes, bit-identical scores;
* against the reference's own ranked lists stored in the goldens, with the gap rule of
  ``test_evaluator_gpu.test_fused_eval_matches_reference_golden`` restated here;
* chunked = one pass, determinism, and the plug-and-play path against the evaluator route with ``call_sizes=[M]``.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests.golden_cases import GOLDEN, load_case

pytestmark = pytest.mark.gpu
FX = os.path.join(GOLDEN, "ref_fixtures") + os.sep
NEG = -float("inf")


@functools.lru_cache(maxsize=None)
def _triplets():
    return torch.load(FX + "commonsense_aligned_triplets.pt"), torch.load(FX + "commonsense_violated_triplets.pt")


@functools.lru_cache(maxsize=None)
def _bitmaps():
    from scene_graph_commonsense_amd.commonsense import TripletBitmaps
    aligned, violated = _triplets()
    return TripletBitmaps(aligned.keys(), violated.keys(), 150, 50, "cuda:0")


@functools.lru_cache(maxsize=None)
def _frequent():
    """(object classes, predicates) that occur most in the aligned triplets: random triples over them pass the filter often enough."""
    import collections
    aligned, _ = _triplets()
    c = collections.Counter()
    for s, _, o in aligned:
        c[s] += 1
        c[o] += 1
    objs = [k for k, _ in c.most_common(6)]
    r = collections.Counter(rel for s, rel, o in aligned if s in objs and o in objs)
    return objs, [k for k, _ in r.most_common(8)]


# ------------------------------------------------------------------------------------------------ kernel vs numpy restatement
def _random_inputs(rows_per_image, rep, seed, objects_per_image=None):
    """Host arrays of a ragged minibatch.  With ``objects_per_image`` the rows are all ordered pairs of every image, scattered over
    the row space (so the per-image list is needed); confidences on 8 levels, connectivity on 4, category confidence on 3 - all
    exact in f32, so sums tie everywhere - and about 30 % -inf (15 % in cand_conf itself, the rest through the mask)."""
    rng = np.random.default_rng(seed)
    objs, rels = _frequent()
    if objects_per_image is not None:
        rows_per_image = [n * (n - 1) for n in objects_per_image]
        off = np.concatenate([[0], np.cumsum(objects_per_image)])
        sub = np.concatenate([[off[b] + i for i in range(n) for j in range(n) if i != j] for b, n in enumerate(objects_per_image)] + [[]]).astype(np.int32)
        obj = np.concatenate([[off[b] + j for i in range(n) for j in range(n) if i != j] for b, n in enumerate(objects_per_image)] + [[]]).astype(np.int32)
        n_obj = int(off[-1])
    else:
        n_obj = 40
    P = int(sum(rows_per_image))
    image = np.repeat(np.arange(len(rows_per_image)), rows_per_image)
    if objects_per_image is None:
        sub, obj = rng.integers(0, n_obj, P).astype(np.int32), rng.integers(0, n_obj, P).astype(np.int32)
    perm = rng.permutation(P)                                          # row of the k-th pair
    row_image = np.empty(P, dtype=np.int64); row_image[perm] = image
    row_sub = np.empty(P, dtype=np.int32); row_sub[perm] = sub
    row_obj = np.empty(P, dtype=np.int32); row_obj[perm] = obj
    ptr = np.concatenate([[0], np.cumsum(rows_per_image)]).astype(np.int32)
    lst = np.concatenate([np.sort(np.nonzero(row_image == b)[0]) for b in range(len(rows_per_image))] + [[]]).astype(np.int32)
    conf = (rng.integers(0, 8, (P, rep)) * 0.25 - 1.0).astype(np.float32)
    conf[rng.random((P, rep)) < 0.15] = NEG
    return dict(rep=rep, ptr=ptr, list=lst, cand_conf=conf, cand_pred=rng.choice(rels, (P, rep)).astype(np.int32),
                conn=(-0.5 * rng.integers(0, 4, P)).astype(np.float32), cat_conf=(0.125 * rng.integers(0, 3, P)).astype(np.float32),
                mask=(rng.random(P) >= 0.18).astype(np.uint8), included=(rng.random(P) >= 0.25).astype(np.uint8),
                sub_idx=row_sub, obj_idx=row_obj, cats=rng.choice(objs, max(n_obj, 1)).astype(np.int64))


def _restatement(x, K, slot_major, use):
    """Stable argsort over the tie key, per image: candidates are laid out in append order, scored in f32 in the kernel's order
    of operations, and ``np.argsort(kind="stable")`` of the negated scores ranks them."""
    aligned, violated = _triplets()
    B, rep = len(x["ptr"]) - 1, x["rep"]
    out = dict(pair=np.full((B, K), -1, np.int32), slot=np.full((B, K), -1, np.int32), predicate=np.full((B, K), -1, np.int32),
               subject=np.full((B, K), -1, np.int32), object=np.full((B, K), -1, np.int32), score=np.full((B, K), NEG, np.float32),
               count=np.zeros(B, np.int32), n_finite=np.zeros(B, np.int32))
    for b in range(B):
        rows = x["list"][x["ptr"][b]:x["ptr"][b + 1]]
        order = [(p, s) for s in range(rep) for p in rows] if slot_major else [(p, s) for p in rows for s in range(rep)]
        cand, score = [], []
        for p, s in order:
            if "included" in use and not x["included"][p]:
                continue
            c = np.float32(x["cand_conf"][p, s])
            if "cat_conf" in use:
                c = np.float32(c + x["cat_conf"][p])
            if "mask" in use and not x["mask"][p]:
                c = np.float32(NEG)
            if "bitmaps" in use:
                t = (int(x["cats"][x["sub_idx"][p]]), int(x["cand_pred"][p, s]), int(x["cats"][x["obj_idx"][p]]))
                if not (t in aligned and t not in violated):
                    c = np.float32(NEG)
            cand.append((p, s))
            score.append(np.float32(c + x["conn"][p]))
        score = np.asarray(score, dtype=np.float32)
        top = np.argsort(-score, kind="stable")[:K]
        out["count"][b] = len(top)
        out["n_finite"][b] = int(np.isfinite(score[top]).sum())
        for r, c in enumerate(top):
            p, s = cand[c]
            out["pair"][b, r], out["slot"][b, r], out["predicate"][b, r] = p, s, x["cand_pred"][p, s]
            out["subject"][b, r], out["object"][b, r], out["score"][b, r] = x["sub_idx"][p], x["obj_idx"][p], score[c]
    return out


def _run_kernel(x, K, slot_major, use):
    from scene_graph_commonsense_amd.scene_graph import rank_scene_graphs
    d = lambda k: torch.from_numpy(x[k]).cuda()
    g = rank_scene_graphs(d("cand_conf"), d("cand_pred"), d("conn"), d("ptr"), top_k=K, pair_list=d("list"), slot_major=slot_major,
                          cat_conf=d("cat_conf") if "cat_conf" in use else None, mask=d("mask") if "mask" in use else None,
                          included=d("included") if "included" in use else None, sub_idx=d("sub_idx"), obj_idx=d("obj_idx"),
                          cats=d("cats"), bitmaps=_bitmaps() if "bitmaps" in use else None)
    return {k: getattr(g, k).cpu().numpy() for k in ("pair", "slot", "predicate", "subject", "object", "score", "count", "n_finite")}


def _assert_same(got, ref, what):
    for k in ("count", "n_finite", "pair", "slot", "predicate", "subject", "object"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
    np.testing.assert_array_equal(got["score"].view(np.int32), ref["score"].view(np.int32), err_msg="%s score bits" % (what,))


OBJECTS = [0, 1, 2, 3, 5, 12, 20]          # 0, 0, 6, 18, 60, 396, 1140 candidates at rep 3: none, < K, around K, > 256 and no multiple of 64
VARIANTS = {"plain": (), "mask": ("mask",), "included": ("included",), "cat_conf": ("cat_conf",), "bitmaps": ("bitmaps",),
            "all": ("mask", "included", "cat_conf", "bitmaps")}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("slot_major", [False, True], ids=["pair_major", "slot_major"])
@pytest.mark.parametrize("rep", [1, 3])
def test_kernel_matches_numpy_restatement(rep, slot_major, variant):
    use = VARIANTS[variant]
    x = _random_inputs(None, rep, seed=10 * rep + len(variant), objects_per_image=OBJECTS)
    assert [int(n) * rep for n in np.diff(x["ptr"])] == [n * (n - 1) * rep for n in OBJECTS]
    for K in (1, 20, 100, 128):
        got, ref = _run_kernel(x, K, slot_major, use), _restatement(x, K, slot_major, use)
        _assert_same(got, ref, "K=%d" % K)
        if "included" not in use:
            assert ref["count"].tolist() == [min(K, n * (n - 1) * rep) for n in OBJECTS]
    # the inputs exercise what they are meant to: ties across the K-th place, -inf inside the ranked window, filters that bite
    s = ref["score"][-1]
    assert len(np.unique(s[np.isfinite(s)])) < 32          # at most 29 distinct sums over hundreds of candidates: ties at every K
    assert (ref["n_finite"] < ref["count"]).any()
    if "bitmaps" in use:
        plain = _restatement(x, 128, slot_major, tuple(u for u in use if u != "bitmaps"))
        assert 0 < ref["n_finite"].sum() < plain["n_finite"].sum()


@pytest.mark.parametrize("slot_major", [False, True], ids=["pair_major", "slot_major"])
@pytest.mark.parametrize("rep,K", [(1, 20), (1, 128), (3, 21), (3, 20), (3, 126)])
def test_exactly_k_and_k_plus_one_candidates(rep, K, slot_major):
    rows = {(1, 20): [20, 21], (1, 128): [128, 129], (3, 21): [7], (3, 20): [7], (3, 126): [42]}[(rep, K)]
    x = _random_inputs(rows, rep, seed=K + rep)
    cands = [r * rep for r in rows]
    assert any(c in (K, K + 1) for c in cands)
    for use in ((), ("mask", "cat_conf")):
        got, ref = _run_kernel(x, K, slot_major, use), _restatement(x, K, slot_major, use)
        _assert_same(got, ref, "rows %s" % rows)
        assert ref["count"].tolist() == [min(K, c) for c in cands]


@pytest.mark.parametrize("slot_major", [False, True], ids=["pair_major", "slot_major"])
def test_image_larger_than_the_cached_keys(slot_major):
    """65 objects = 4160 pairs = 12480 candidates at rep 3: past the 12288 keys the kernel keeps in LDS, the rest are formed again
    in every pass."""
    x = _random_inputs(None, 3, seed=65, objects_per_image=[65, 3])
    use = VARIANTS["all"]
    got, ref = _run_kernel(x, 100, slot_major, use), _restatement(x, 100, slot_major, use)
    _assert_same(got, ref, "65 objects")
    # the last cached slots and the first uncached ones can all be ranked: only they are finite
    y = dict(x)
    y["cand_conf"] = np.full_like(x["cand_conf"], NEG)
    rows = x["list"][x["ptr"][0]:x["ptr"][1]]
    edge = rows[4090:4102] if not slot_major else rows[-70:]          # slots around 12288 in either order
    y["cand_conf"][edge] = x["cand_conf"][edge]
    got, ref = _run_kernel(y, 100, slot_major, ()), _restatement(y, 100, slot_major, ())
    _assert_same(got, ref, "around the cache boundary")
    assert ref["n_finite"][0] > 12


# ------------------------------------------------------------------------------------------------ end to end
_MODEL = {}
_case = functools.lru_cache(maxsize=None)(load_case)


def _model(name):
    """One full-size module for the whole file; the state dict of case ``name`` is loaded when it changes."""
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    cfg, sd, batch, gold = _case(name)
    if "m" not in _MODEL:
        _MODEL["m"] = BayesianRelationClassifier(cfg.args(fixtures=FX)).cuda()
        _MODEL["m"].eval()
    if _MODEL.get("name") != name:
        _MODEL["m"].load_state_dict(sd)
        _MODEL["name"] = name
    return _MODEL["m"], cfg, batch, gold


def _scene(name):
    from scene_graph_commonsense_amd.synthetic import make_scene_batch
    if name == "synthetic_3x20":
        model, cfg, _, _ = _model("vg_full")
        return model, cfg, make_scene_batch(cfg, (20, 20, 20), seed=23, connect_frac=0.1), None
    return _model(name)


def _evaluator_args(cfg, run_mode):
    args = cfg.args(run_mode=run_mode, fixtures=FX)
    args["dataset"]["commonsense_aligned_triplets"] = FX + "commonsense_aligned_triplets.pt"
    args["dataset"]["commonsense_violated_triplets"] = FX + "commonsense_violated_triplets.pt"
    return args


def _evaluator_route(model, cfg, batch, K, run_mode):
    """The parent's way to the ranked lists: per image (predicates, subject / object categories, boxes, confidences) at every rank."""
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.pair_loop import evaluate_minibatch
    ev = Evaluator(_evaluator_args(cfg, run_mode), cfg.num_relations, 0.5, [K])
    evaluate_minibatch(model, batch, ev)
    ev.compute()
    which = ev.which_in_batch.cpu().numpy()
    h = {k: ev._cat(k).cpu().numpy() for k in ("conf", "pred", "scat", "ocat", "sbox", "obox")}
    out = {}
    for image, top in ev.last_topk.items():
        idx = np.nonzero(which == image)[0][np.asarray(top)]
        out[image] = {k: v[idx] for k, v in h.items()}
    return out


@pytest.mark.parametrize("run_mode", ["eval", "eval_cs"])
@pytest.mark.parametrize("name", ["vg_full", "vg_full_hit", "synthetic_3x20"])
def test_predict_equals_the_evaluator_route(name, run_mode):
    from scene_graph_commonsense_amd.pair_loop import predict_scene_graphs
    model, cfg, batch, _ = _scene(name)
    cs = _triplets() if run_mode == "eval_cs" else None
    for K in (20, 100):
        ref = _evaluator_route(model, cfg, batch, K, run_mode)
        g = predict_scene_graphs(model, batch, top_k=K, overlap_filtering=True, commonsense=cs)
        count = g.count.cpu().numpy()
        assert g.score.shape == (len(batch.bbox), K) and g.image.tolist() == list(range(len(batch.bbox)))
        n_ranked = 0
        for b in range(len(batch.bbox)):
            r = ref.get(b)
            n = 0 if r is None else len(r["pred"])
            assert count[b] == n, (b, count[b], n)
            if n == 0:
                continue
            np.testing.assert_array_equal(g.predicate[b, :n].cpu().numpy(), r["pred"])
            np.testing.assert_array_equal(g.subject_cat[b, :n].cpu().numpy(), r["scat"])
            np.testing.assert_array_equal(g.object_cat[b, :n].cpu().numpy(), r["ocat"])
            np.testing.assert_array_equal(g.subject_box[b, :n].cpu().numpy(), r["sbox"])
            np.testing.assert_array_equal(g.object_box[b, :n].cpu().numpy(), r["obox"])
            np.testing.assert_array_equal(g.score[b, :n].cpu().numpy().view(np.int32), r["conf"].astype(np.float32).view(np.int32))
            assert int(g.n_finite[b]) == int(np.isfinite(r["conf"]).sum())
            assert bool((g.pair[b, n:] == -1).all()) and bool(torch.isinf(g.score[b, n:]).all())
            n_ranked += n
        assert n_ranked > 0
        # the ranked rows point at the forward's outputs of this call
        out = model.last_outputs
        sel = g.pair[g.pair >= 0].long()
        assert torch.equal(out.cand_pred[sel, g.slot[g.pair >= 0].long()], g.predicate[g.pair >= 0])


def test_predict_needs_no_relation_targets_and_takes_category_confidences():
    """A batch without relationships / subj_or_obj (the deployed case), with per-object category confidences: equal to the SGDET
    evaluator route (``evaluate_sgdet_minibatch``), which adds subject + object confidence to every candidate of a pair."""
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.pair_loop import evaluate_sgdet_minibatch, predict_scene_graphs
    from scene_graph_commonsense_amd.synthetic import SceneBatch
    model, cfg, batch, _ = _scene("vg_full")
    rng = np.random.default_rng(3)
    cat_conf = [torch.from_numpy(-rng.integers(0, 4, int(b.shape[0])).astype(np.float32) * 0.25) for b in batch.bbox]
    sub2super = {int(c): s for cats, sp in zip(batch.categories, batch.super_categories) for c, s in zip(cats.tolist(), sp)}
    bare = SceneBatch(batch.image_feature, batch.image_depth, [b.float() for b in batch.bbox], [c.long() for c in batch.categories],
                      [[torch.as_tensor(sub2super[int(c)]) for c in cats.tolist()] for cats in batch.categories], None, None)
    g = predict_scene_graphs(model, bare, top_k=100, cat_confidence=cat_conf)
    ev = Evaluator(cfg.args(fixtures=FX), cfg.num_relations, 0.5, [100])
    evaluate_sgdet_minibatch(model, batch.image_feature, batch.image_depth, batch.categories, cat_conf, batch.bbox, ev, sub2super=sub2super)
    ev._targets_by_image = ([None] * len(batch.bbox),) * 5
    ev.compute(predcls=False)
    which, conf, pred = ev.which_in_batch.cpu().numpy(), ev.confidence.cpu().numpy(), ev.relation_pred.cpu().numpy()
    assert len(ev.last_topk) > 0
    for image, top in ev.last_topk.items():
        idx = np.nonzero(which == image)[0][np.asarray(top)]
        n = len(idx)
        assert int(g.count[image]) == n
        np.testing.assert_array_equal(g.predicate[image, :n].cpu().numpy(), pred[idx])
        np.testing.assert_array_equal(g.score[image, :n].cpu().numpy().view(np.int32), conf[idx].astype(np.float32).view(np.int32))


def _golden_triples(cfg, batch, gold):
    """(subject_id, relation_id, object_id) of every candidate of the reference's Evaluator state, in its append order: per kept
    direction-step the pairs of the step three times (geometric, possessive, semantic block; ``evaluator.py:231-246``)."""
    from scene_graph_commonsense_amd.pairs import enumerate_pairs
    pidx = enumerate_pairs([int(b.shape[0]) for b in batch.bbox])
    cats = torch.cat([c.reshape(-1) for c in batch.categories]).numpy()
    kept = set(map(tuple, gold["eval_steps"].tolist()))
    rows = np.asarray([k for k in range(pidx.n_pairs) if (int(pidx.g[k]), int(pidx.e[k])) in kept])
    pair_of, r0 = [], 0
    for b in gold["eval_call_sizes"].tolist():
        pair_of += [rows[r0:r0 + b]] * 3
        r0 += b
    pair_of = np.concatenate(pair_of)
    assert r0 == len(rows) and len(pair_of) == len(gold["ev_relation_pred"])
    np.testing.assert_array_equal(pidx.image[pair_of], gold["ev_which_in_batch"])
    return np.stack([cats[pidx.sub[pair_of]], gold["ev_relation_pred"], cats[pidx.obj[pair_of]]], axis=1)


@pytest.mark.parametrize("name", ["vg_full", "vg_full_hit"])
def test_predict_matches_reference_golden(name):
    """The ranked triples against the reference's own ranking (``ev_top100_stable``: the stable sort of ITS confidences) and ITS
    predicates.  Equal at every rank that ``test_fused_eval_matches_reference_golden`` calls resolvable - the reference's
    confidence there is separated from both neighbours by more than twice the forward tolerance (2e-3 of the largest finite
    confidence) and is finite - and at 80 % of all ranks at least, as that test requires of the ranked indices."""
    from scene_graph_commonsense_amd.pair_loop import predict_scene_graphs
    model, cfg, batch, gold = _scene(name)
    triples = _golden_triples(cfg, batch, gold)
    g = predict_scene_graphs(model, batch, top_k=100)
    mine_all = torch.stack([g.subject_cat, g.predicate.long(), g.object_cat], dim=2).cpu().numpy()
    count = g.count.cpu().numpy()
    which = gold["ev_which_in_batch"]
    refc = gold["ev_confidence"] + gold["ev_connectivity"]
    gap = 2e-3 * np.abs(refc[np.isfinite(refc)]).max()
    n_res = n_all = n_same = n_res_same = 0
    for row, image in enumerate(np.unique(which)):
        ref = gold["ev_top100_stable"][row]
        ref = ref[ref >= 0]
        c = refc[which == image]
        cs = c[np.argsort(-c, kind="stable")]
        with np.errstate(invalid="ignore"):
            d = cs[:-1] - cs[1:]
            ok = (np.concatenate([[np.inf], d]) > gap) & (np.concatenate([d, [np.inf]]) > gap) & np.isfinite(cs)
        ok = ok[:len(ref)]
        assert count[image] == len(ref)
        want, mine = triples[which == image][ref], mine_all[image, :len(ref)]
        same = (want == mine).all(axis=1)
        n_res, n_all, n_same, n_res_same = n_res + int(ok.sum()), n_all + len(ref), n_same + int(same.sum()), n_res_same + int(same[ok].sum())
    print(name, "ranked triples: %d of %d ranks resolvable, %d of them equal, %d equal overall" % (n_res, n_all, n_res_same, n_same))
    assert n_res > 0 and n_res_same == n_res
    assert n_same >= 0.8 * n_all


def test_chunked_prediction_equals_one_pass_and_is_deterministic():
    from scene_graph_commonsense_amd.pair_loop import predict_scene_graphs
    from scene_graph_commonsense_amd.synthetic import make_scene_batch
    model, cfg, _, _ = _scene("vg_full")
    batch = make_scene_batch(cfg, [12] * 6, seed=77, connect_frac=0.1)
    fields = ("pair", "slot", "predicate", "subject", "object", "count", "n_finite", "subject_cat", "object_cat", "subject_box", "object_box")
    runs = []
    for budget in (1e15, 1e15, 300e6):
        g = predict_scene_graphs(model, batch, top_k=100, workspace_budget=budget)
        runs.append((g, list(model.last_image_groups)))
    (one, g1), (again, _), (many, gn) = runs
    assert len(g1) == 1 and len(gn) >= 2
    for other in (again, many):
        for k in fields:
            assert torch.equal(getattr(one, k), getattr(other, k)), k
        assert torch.equal(one.score.view(torch.int32), other.score.view(torch.int32))
    assert int(one.count.min()) == 100 and int(one.n_finite.sum()) > 0


def test_plug_and_play_ranking_equals_the_evaluator_route():
    """``rank_scene_graphs`` on ``BayesianHead.candidates`` (M = 300 rows of width 64 in 4 images of 0 / 1 / 99 / 200 rows), slot-major,
    against ONE blocked append to an ``Evaluator`` (``call_sizes=[M]``) + ``compute()``."""
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.model import BayesianHead
    from scene_graph_commonsense_amd.scene_graph import rank_scene_graphs
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    cfg = HeadConfig()
    torch.manual_seed(5)
    head = BayesianHead(input_dim=64, num_geometric=cfg.num_geometric, num_possessive=cfg.num_possessive, num_semantic=cfg.num_semantic).cuda()
    gen = torch.Generator(device="cuda").manual_seed(6)
    rows, M, K = [0, 1, 99, 200], 300, 100
    h = 3 * torch.randn(M, 64, device="cuda", generator=gen)
    conf, pred, _ = head.candidates(h)
    which = torch.repeat_interleave(torch.arange(4, device="cuda"), torch.tensor(rows, device="cuda"))
    conn = -0.5 * torch.randint(0, 4, (M,), device="cuda", generator=gen).float()
    mask = torch.rand(M, device="cuda", generator=gen) >= 0.8              # most candidates tie at -inf inside image 2's window
    cat = torch.randint(0, 150, (M, 2), device="cuda", generator=gen)
    box = torch.randint(0, 32, (M, 2, 4), device="cuda", generator=gen).float()
    ev = Evaluator(cfg.args(fixtures=FX), cfg.num_relations, 0.5, [K])
    ev.accumulate_candidates(which, conf, pred, torch.full((M,), -1, device="cuda"), conn, cat[:, 0], cat[:, 1], box[:, 0], box[:, 1],
                             iou_mask=mask, call_sizes=[M])
    ev.compute()
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32, device="cuda")
    g = rank_scene_graphs(conf, pred, conn, ptr, top_k=K, mask=mask)
    assert g.subject_cat is None and bool((g.subject == -1).all())
    which_c, conf_c, pred_c = ev.which_in_batch.cpu().numpy(), ev.confidence.cpu().numpy(), ev.relation_pred.cpu().numpy()
    assert g.count.tolist() == [0, 3, 100, 100] and sorted(ev.last_topk) == [1, 2, 3]
    for image, top in ev.last_topk.items():
        idx = np.nonzero(which_c == image)[0][np.asarray(top)]             # append position s * M + row
        n = len(idx)
        assert int(g.count[image]) == n
        np.testing.assert_array_equal(g.pair[image, :n].cpu().numpy(), idx % M)
        np.testing.assert_array_equal(g.slot[image, :n].cpu().numpy(), idx // M)
        np.testing.assert_array_equal(g.predicate[image, :n].cpu().numpy(), pred_c[idx])
        np.testing.assert_array_equal(g.score[image, :n].cpu().numpy().view(np.int32), conf_c[idx].astype(np.float32).view(np.int32))
    assert int(g.n_finite[2]) < 100                                        # -inf ties were ranked, in slot-major order
