"""Fused replacements for the reference's pair loops (the bodies of ``testing()`` / ``eval_pc`` and ``training()``).

``evaluate_minibatch`` is what ``train_test.py:373-437`` + ``train_utils.py:160-196`` do for one minibatch: score
every ordered pair, apply the overlap filter (a step in which no image's two boxes overlap is skipped entirely -
no candidates and no targets), and feed the Recall@K evaluators in the reference's candidate order.
``train_minibatch`` is ``train_test.py:174-277`` (pass ``image_feature_aug`` for the contrastive term, ``commonsense`` for train_cs).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .pairs import DeviceScene, flatten_scene, match_target_sgd, pair_targets_fast


# ------------------------------------------------------------------------------------------------ image-group chunking
# A minibatch is scored in ONE fused pass whose workspace grows with its ordered pairs (~2.3 MB per pair in training at
# 11 % pair-specific windows).  The reference's per-step loop handles any object count (``evaluate.py:375-444``: up to 2 x 100
# predicted objects per image, 16 images), so a minibatch that does not fit is cut into consecutive IMAGE GROUPS that run back to
# back: images are independent in the forward, the evaluator is fed in the reference's candidate order across groups from the
# scattered outputs, and in training the per-pair loss coefficients are computed for the WHOLE minibatch first (its per-step means
# and running-sum weights couple the images) so that the groups' gradients simply add (tests/test_configs_gpu.py: additivity).
# Bytes per pair / per pair-specific window / per object, measured with tools/mem_report.py (+15 % margin in ``plan_image_groups``):
_COST = {
    # (per pair, per X window, per pair on the per-pair kernels, per object)
    True: (0.95e6, 0.09e6, 2.7e6, 8.0e6),           # training: z f16 + routing codes + dz (no bf16 copy of the pairs' z: -0.33e6), patch forms of
                                                    # the backward (16 + 20 rows of 1 KB per convolved window; the column forms of rounds 1-2: 0.125e6)
    False: (0.40e6, 0.03e6, 0.60e6, 3.0e6),         # evaluation: z f16, window-major rows, f32 fc1 products
}


def freeze_setup_objects() -> int:
    """Call once after the model, datasets and evaluators are built, before the minibatch loop: collects garbage and moves everything
    alive (``torch``'s and ``numpy``'s module objects, the annotations: 2-3 x 10^5 tracked containers) to the permanent generation.
    Without it CPython's full (generation-2) collection walks all of them every few dozen minibatches - 77 ms measured on the MI355X
    box, a step and a half of the benchmark's 43-46 ms, landing in the middle of an asynchronous launch sequence
    (profiles/r05_host_gc.txt).  The per-minibatch garbage (pair tables, ragged lists) stays collectable.  Returns the number frozen."""
    import gc
    gc.collect()
    gc.freeze()
    return gc.get_freeze_count()


def slice_batch(batch, a: int, b: int):
    """Images [a, b) of a ``SceneBatch`` (views; the per-image lists are shared)."""
    from .synthetic import SceneBatch
    pick = lambda x: None if x is None else list(x[a:b])
    return SceneBatch(batch.image_feature[a:b], batch.image_depth[a:b], pick(batch.bbox), pick(batch.categories),
                      pick(batch.super_categories), pick(getattr(batch, "relationships", None)), pick(getattr(batch, "subj_or_obj", None)),
                      [int(x.shape[0]) for x in batch.bbox[a:b]])


def default_workspace_budget(model) -> int:
    """70 % of what this process could allocate right now: free HBM + the allocator's cached blocks + the engine's own workspace
    (it is reused)."""
    dev = next(model.parameters()).device
    free, _ = torch.cuda.mem_get_info(dev)
    cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    eng = getattr(model, "_engine", None)
    own = eng.ws.nbytes() if eng is not None else 0
    return int(0.7 * (free + cached + own))


def image_workspace_bytes(cfg, bbox, train: bool) -> float:
    """Estimated workspace of one image's pairs in a fused pass (``bbox``: its [n,4] boxes as given)."""
    from .engine import shared_conv3_enabled
    from .pairs import count_shared_windows, normalise_boxes
    n = int(bbox.shape[0])
    pairs = n * (n - 1)
    per_pair, per_win, per_pair_full, per_obj = _COST[bool(train)]
    if pairs == 0:
        return per_obj * n
    xw = None
    if cfg.feature_size == 32:
        bb = normalise_boxes(torch.as_tensor(bbox).detach().cpu(), cfg.feature_size)
        xw = count_shared_windows(bb, [0, n])
    if xw is not None and shared_conv3_enabled(xw, pairs):
        return per_pair * pairs + per_win * xw + per_obj * n
    return per_pair_full * pairs + per_obj * n


def plan_image_groups(cfg, batch, train: bool, budget_bytes: float):
    """Consecutive image ranges [(a, b), ...] whose estimated workspace (+15 %) stays within ``budget_bytes``; an image that
    exceeds the budget on its own is a group of one (its pairs cannot be split: loss and ranking are per image)."""
    n = [int(b.shape[0]) for b in batch.bbox]
    if 1.15 * sum(_COST[bool(train)][2] * k * (k - 1) + _COST[bool(train)][3] * k for k in n) <= budget_bytes:
        return [(0, len(n))]                        # fits even on the per-pair kernels: no need to count windows (the usual case)
    cost = [1.15 * image_workspace_bytes(cfg, b, train) for b in batch.bbox]
    groups, a, acc = [], 0, 0.0
    for k, c in enumerate(cost):
        if k > a and acc + c > budget_bytes:
            groups.append((a, k))
            a, acc = k, 0.0
        acc += c
    groups.append((a, len(cost)))
    return groups


def split_balanced(num_objects, k: int):
    """At most ``k`` consecutive image ranges with about equal numbers of ordered pairs (lanes of the two-stream step)."""
    pairs = np.asarray([n * (n - 1) for n in num_objects], dtype=np.float64)
    total, B = float(pairs.sum()), len(pairs)
    if k <= 1 or B < 2 or total == 0:
        return [(0, B)]
    cum = np.cumsum(pairs)
    cuts = [0]
    for j in range(1, k):
        c = int(np.searchsorted(cum, total * j / k, side="left")) + 1
        c = min(max(c, cuts[-1] + 1), B - (k - j))
        cuts.append(c)
    cuts.append(B)
    return [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]


def _budget(model, workspace_budget):
    if workspace_budget is not None:
        return float(workspace_budget)
    b = getattr(model, "workspace_budget_bytes", None)
    if b is not None:
        return float(b)
    # measured when first needed and again every 64 calls (the planner runs every step; what ELSE lives in HBM - the feature
    # extractor, an evaluator's state, another model - changes over an epoch)
    n = getattr(model, "_auto_budget_calls", 0)
    if getattr(model, "_auto_budget", None) is None or n >= 64:
        model._auto_budget = float(default_workspace_budget(model))
        n = 0
    model._auto_budget_calls = n + 1
    return model._auto_budget


def _group_rows(scene: DeviceScene, a: int, b: int) -> torch.Tensor:
    """Pairs of the images [a, b) in the whole minibatch's pair order = the pair order of the group's own scene (restricting
    ``keep_in_batch`` to a subset of images keeps their relative order)."""
    img = scene.image
    return torch.nonzero((img >= a) & (img < b)).flatten()


def forward_pairs_chunked(model, cfg, batch, scene: DeviceScene, groups, iou: Optional[torch.Tensor], select: Optional[torch.Tensor]):
    """``model.forward_pairs`` over image groups; the groups' rows are scattered into full-size outputs in the minibatch's pair order."""
    from .engine import PairOutputs
    dev = scene.bbox.device
    P = scene.n_pairs
    nc = 3 if cfg.hierarchical else 1
    full = PairOutputs(torch.zeros(P, cfg.num_relations, device=dev), torch.zeros(P, 3, device=dev) if cfg.hierarchical else None,
                       torch.zeros(P, device=dev), torch.zeros(P, 512, device=dev), torch.full((P, nc), -float("inf"), device=dev),
                       torch.zeros(P, nc, dtype=torch.int32, device=dev))
    for a, b in groups:
        rows = _group_rows(scene, a, b)
        if rows.numel() == 0:
            continue
        sub = flatten_scene(cfg, slice_batch(batch, a, b), dev)
        assert sub.n_pairs == int(rows.numel())
        out = model.forward_pairs(sub, iou_mask=None if iou is None else iou[rows].contiguous(),
                                  select=None if select is None else select[rows].contiguous())
        full.relation[rows] = out.relation
        if full.super_relation is not None:
            full.super_relation[rows] = out.super_relation
        full.connectivity[rows] = out.connectivity
        full.hidden[rows] = out.hidden
        full.cand_conf[rows] = out.cand_conf
        full.cand_pred[rows] = out.cand_pred
    return full


def overlap_mask(scene: DeviceScene) -> torch.Tensor:
    """[P] uint8: the pair's two boxes share a grid cell (``train_test.py:403-408``)."""
    lib = _lib.load()
    P = scene.n_pairs
    out = torch.empty(P, dtype=torch.uint8, device=scene.bbox.device)
    _lib.check(lib.sgc_overlap_filter(_lib.ptr(scene.bbox), _lib.ptr(scene.sub_idx), _lib.ptr(scene.obj_idx), _lib.ptr(out), P,
                                      _lib.stream_ptr()), "sgc_overlap_filter")
    return out


def _step_filter(scene: DeviceScene, iou: Optional[torch.Tensor]):
    """(included [P] bool, any_overlap [T] bool) on the device: a direction-step is kept when at least one image's two boxes
    overlap (``train_test.py:403-410``; the filter is symmetric and tested once per (g, e), so both directions share the decision)."""
    dev = scene.bbox.device
    if iou is None:
        return torch.ones(scene.n_pairs, dtype=torch.bool, device=dev), torch.ones(scene.n_steps, dtype=torch.bool, device=dev)
    step = scene.step.long()
    per_step = torch.zeros(scene.n_steps, dtype=torch.int32, device=dev).index_add_(0, step, iou.int())
    any_overlap = per_step > 0
    return any_overlap[step], any_overlap


def _unfiltered_selection(scene: DeviceScene, iou: torch.Tensor, evaluators) -> torch.Tensor:
    """[P] bool (device): the pairs whose trunk must be computed when the overlap filter is on.  A filtered candidate can only
    matter when its image has fewer unfiltered pairs than the evaluator ranks (then -inf entries enter the top K and may still
    match a ground-truth triple): such images are computed completely."""
    k_max = max([100] + [int(e.top_k[-1]) for e in evaluators if e is not None])
    image = scene.image.long()
    per_image = torch.zeros(int(scene.image_feature.shape[0]), dtype=torch.int32, device=iou.device).index_add_(0, image, iou.int())
    return iou.bool() | (per_image < k_max)[image]


def raw_boxes(scene: DeviceScene) -> torch.Tensor:
    """[n_obj,4] device copy of ``scene.bbox_raw`` in its own dtype (the boxes as given: what the evaluators and the ranked graphs carry;
    the kernels' f32 copy is ``metrics.scene_boxes``), made once and kept on the scene."""
    if scene._bbox_raw_d is None:
        scene._bbox_raw_d = torch.from_numpy(scene.bbox_raw).to(scene.bbox.device)
    return scene._bbox_raw_d


def directed_targets(scene: DeviceScene, relationships, subj_or_obj, needs: str, fresh: bool = False) -> torch.Tensor:
    """[P] int32 device: the directed target of every pair - what ``flatten_scene`` (or ``assign_sgdet_targets``) left on the scene, else
    (or with ``fresh``: the lists are not the ones the scene was flattened from) derived from the lists and uploaded.  ``needs``: the
    caller's ``ValueError`` text when there are neither."""
    if scene.directed is not None and not fresh:
        return scene.directed
    if relationships is None:
        raise ValueError(needs)
    return torch.from_numpy(pair_targets_fast(relationships, subj_or_obj, scene.pidx).astype(np.int32)).to(scene.bbox.device)


def pair_cat_confidence(scene: DeviceScene, per_image, needs: str) -> torch.Tensor:
    """[P] f32 device: subject + object category confidence of every pair from per-image lists of per-object confidences
    (``evaluator.py:129-130``); ``needs``: the caller's ``ValueError`` text when they do not hold one value per object."""
    conf_obj = torch.cat([torch.as_tensor(c).reshape(-1).to(scene.bbox.device, torch.float32) for c in per_image])
    if int(conf_obj.numel()) != int(scene.cats.numel()):
        raise ValueError(needs)
    return conf_obj[scene.sub_idx.long()] + conf_obj[scene.obj_idx.long()]


_FEED_NEEDS_TARGETS = "the evaluator feed needs relation targets: flatten the scene from a batch with relationships / subj_or_obj"
_SGDET_NEEDS_CONFIDENCES = "cat_pred_confidence must hold one value per predicted object"


def feed_evaluators(model, scene: DeviceScene, out, evaluator=None, evaluator_top3=None, overlap=None, directed=None, *,
                    cat_confidence=None, targets: bool = True):
    """Append one minibatch to the Recall@K evaluators in the reference's candidate order (``evaluator.py:231-246``).
    ``overlap`` = [P] uint8 device mask of the overlap filter (``train_test.py:403-410``): direction-steps in which no image's
    boxes overlap are skipped entirely (no candidates, no targets); ``None`` = no filter (``training()``, ``:209``).
    SGDET / SGCLS: ``cat_confidence`` [P] (``pair_cat_confidence``) is added to every candidate of the pair and ``targets=False``
    appends no relation targets (they come from ``Evaluator.accumulate_target``).
    Everything stays on the device (the pair tables of the scene are device tensors); the only host synchronisation is the size
    of the kept set.  Returns ``included`` [P] bool device tensor (pairs of the kept steps)."""
    cfg = model.head_config()
    dev = scene.bbox.device
    included, any_overlap = _step_filter(scene, overlap)
    if evaluator is None and evaluator_top3 is None:
        return included
    if targets and directed is None:
        directed = directed_targets(scene, None, None, _FEED_NEEDS_TARGETS)
    iou = overlap if overlap is not None else torch.ones(scene.n_pairs, dtype=torch.uint8, device=dev)
    sel = torch.nonzero(included).flatten()
    sizes = (scene.step_ptr[1:] - scene.step_ptr[:-1])[any_overlap]            # pairs per kept direction-step, in order
    which = scene.image.long()[sel]
    tgt = torch.as_tensor(directed).to(dev)[sel].long() if targets else None
    sub, obj = scene.sub_idx.long()[sel], scene.obj_idx.long()[sel]
    scat, ocat = scene.cats[sub], scene.cats[obj]
    raw = raw_boxes(scene)
    sbox, obox = raw[sub], raw[obj]
    logsig = torch.log(torch.sigmoid(out.connectivity[sel]))
    iou_sel = iou[sel].bool()
    if evaluator is not None:
        evaluator.accumulate_candidates(which, out.cand_conf[sel], out.cand_pred[sel], tgt, logsig, scat, ocat, sbox, obox,
                                        iou_mask=iou_sel, call_sizes=sizes,
                                        cat_confidence=None if cat_confidence is None else cat_confidence[sel])
    if evaluator_top3 is not None and cfg.hierarchical:
        conf3 = out.cand_conf[sel].max(dim=1)[0]
        evaluator_top3.accumulate_candidates(which, conf3, out.cand_pred[sel], tgt, logsig, scat, ocat, sbox, obox, iou_mask=iou_sel)
    return included


class MinibatchLookahead:
    """Iterate the minibatches of a loader ONE AHEAD: ``prepare(data)`` (the drivers' ``_to_batch`` + ``flatten_scene``: loader,
    feature extractor launches, ragged lists -> pinned staging -> device) of minibatch k+1 runs when the consumer calls
    ``fetch_next()`` - which ``evaluate_minibatch(while_running=...)`` does right after it has enqueued the forward of minibatch k,
    i.e. while the device is busy, instead of after the feed's host synchronisation with the device idle (4-5 ms of a 20 ms evaluated
    minibatch at 8 x 64).  ``prepare(index, data)`` returns None for a minibatch to skip and ``MinibatchLookahead.STOP`` to end the
    iteration.  Yields (index, prepared)."""
    STOP = object()

    def __init__(self, loader, prepare):
        self._it, self._prepare, self._next, self._fetched = enumerate(loader), prepare, None, False
        self.fetch_next()

    def fetch_next(self):
        if self._fetched:
            return
        self._fetched, self._next = True, None
        for i, data in self._it:
            item = self._prepare(i, data)
            if item is MinibatchLookahead.STOP:
                self._it = iter(())
                return
            if item is not None:
                self._next = (i, item)
                return

    def __iter__(self):
        return self

    def __next__(self):
        self.fetch_next()                        # the consumer did not look ahead (an exception path, a caller without the hook)
        if self._next is None:
            raise StopIteration
        cur, self._fetched = self._next, False
        return cur


# ------------------------------------------------------------------------------------------------ the six evaluation entry points
# share one prologue (``_scene_of``, ``_filters``, the table helpers above) and one forward (``_scoring_forward``).  In all but
# ``evaluate_minibatch`` every upload and per-scene table is made BEFORE the forward is enqueued and nothing after it synchronises
# with the host.  Which ``model.last_*`` attributes a call touches is part of its contract (train_test.py reads ``last_outputs is None``
# as a signal, bench.py reads ``last_outputs`` and ``last_image_groups``):
#
#   call                          last_image_groups   last_outputs   last_connectivity_stats
#   evaluate_minibatch            set                 untouched      set: None, or the stats when select is None and the scene has raw targets
#   evaluate_sgdet_minibatch      set                 untouched      untouched
#   predict_scene_graphs          set                 set            untouched
#   score_minibatch               set                 set            as evaluate_minibatch
#   score_sgdet_minibatch         set                 set            untouched
#   mine_commonsense_candidates   set                 set            untouched
def _scoring_forward(model, cfg, batch, scene, iou, select, workspace_budget):
    """The fused forward over the scene's pairs, in image groups when the minibatch exceeds the workspace budget (16 images x 100+
    detections).  The only place of the evaluation path that plans image groups, runs the forward or sets ``model.last_image_groups``."""
    groups = plan_image_groups(cfg, batch, False, _budget(model, workspace_budget))
    if len(groups) > 1:
        out = forward_pairs_chunked(model, cfg, batch, scene, groups, iou, select)
    else:
        out = model.forward_pairs(scene, iou_mask=iou, select=select)
    model.last_image_groups = groups
    return out


def _scene_of(model, batch, scene: Optional[DeviceScene] = None):
    """(cfg, device, scene): the caller's scene, else the batch flattened on the model's device."""
    cfg = model.head_config()
    dev = next(model.parameters()).device
    return cfg, dev, scene if scene is not None else flatten_scene(cfg, batch, dev)


def _filters(scene: DeviceScene, overlap_filtering: bool, skip_filtered: bool, rankers, *, steps: bool = True):
    """(iou, included, select): the overlap mask [P] u8 or None (filter off); the pairs of the kept steps [P] bool or None (filter off,
    or ``steps=False``: the evaluator feed decides them itself, after the forward); the pairs to compute [P] bool when both flags
    are set (``rankers``: the evaluators or the meter whose ``top_k`` bounds what a filtered pair can reach), else None."""
    iou = overlap_mask(scene) if overlap_filtering else None
    included = _step_filter(scene, iou)[0] if (overlap_filtering and steps) else None
    select = _unfiltered_selection(scene, iou, rankers) if (skip_filtered and overlap_filtering) else None
    return iou, included, select


def _bitmaps_of(model, commonsense, dev):
    """``commonsense`` as a ``commonsense.TripletBitmaps``: one passes through, (aligned, violated) collections are converted."""
    from .commonsense import TripletBitmaps
    if commonsense is None or isinstance(commonsense, TripletBitmaps):
        return commonsense
    return model._commonsense_bitmaps(commonsense, dev)


def _connectivity_stats(model, scene: DeviceScene, out, directed, included, select):
    """Sets ``model.last_connectivity_stats``: the counters of ``evaluate_one_direction`` over the kept steps, None when pairs were
    skipped or the scene has no raw targets."""
    model.last_connectivity_stats = None
    if select is None and scene.raw_target is not None:
        model.last_connectivity_stats = model.engine().connectivity_stats(
            out.connectivity, directed, scene.raw_target, None if included is None else included.to(torch.uint8))


def evaluate_minibatch(model, batch, evaluator=None, evaluator_top3=None, overlap_filtering: bool = True,
                       scene: Optional[DeviceScene] = None, skip_filtered: bool = False, workspace_budget: Optional[float] = None,
                       while_running=None):
    """Returns (scene, outputs, included[P] bool numpy, directed targets numpy).
    ``skip_filtered=True`` runs the per-pair trunk only for the pairs that pass the overlap filter (about 40 % of the ordered pairs
    on the synthetic boxes) in every image that has at least top-K such pairs: Recall@K is unchanged (a filtered pair's
    confidence is -inf either way, ``evaluator.py:131-134``, and cannot reach the top K there); ``outputs`` of the skipped pairs
    are zeros.  The reference cannot skip them: its batched per-step call always scores the whole batch.
    ``model.last_connectivity_stats`` holds the counters of ``evaluate_one_direction`` (``train_utils.py:176-184``) summed over the
    kept steps ([5] int64 device tensor; None with ``skip_filtered``).
    ``workspace_budget`` (bytes; default ``model.workspace_budget_bytes`` or 70 % of the free HBM): a minibatch whose fused pass
    would need more is scored in consecutive image groups (``plan_image_groups``) - same outputs, same evaluator feed.
    ``while_running``: called once, with no arguments, after the forward has been enqueued and before the evaluator feed's first
    host synchronisation - the place for host work that does not depend on this minibatch (``MinibatchLookahead.fetch_next``)."""
    cfg, _, scene = _scene_of(model, batch, scene)
    iou, _, select = _filters(scene, overlap_filtering, skip_filtered, (evaluator, evaluator_top3), steps=False)
    out = _scoring_forward(model, cfg, batch, scene, iou, select, workspace_budget)
    if while_running is not None:
        while_running()
    # the one caller that derives its targets AFTER the forward is enqueued: ``while_running`` must run with the device busy and before
    # anything here waits for it (MinibatchLookahead)
    directed_d = directed_targets(scene, batch.relationships, batch.subj_or_obj, _FEED_NEEDS_TARGETS)
    included = feed_evaluators(model, scene, out, evaluator, evaluator_top3, overlap=iou, directed=directed_d)
    _connectivity_stats(model, scene, out, directed_d, included, select)
    return scene, out, included.cpu().numpy(), directed_d.cpu().numpy().astype(np.int64)


def _sgdet_scene(model, image_feature, image_depth, categories_pred, bbox_pred, sub2super):
    """(cfg, device, batch, scene): the ``SceneBatch`` and ``DeviceScene`` of the PREDICTED objects of one SGDET / SGCLS minibatch
    (``evaluate.py:375-444``) - the batch construction ``evaluate_sgdet_minibatch`` and ``score_sgdet_minibatch`` share."""
    from .synthetic import SceneBatch
    cfg = model.head_config()
    if len(categories_pred) != int(image_feature.shape[0]):
        raise ValueError("one predicted-object list per image is required (the reference drops the whole minibatch otherwise)")
    sp = None
    if cfg.dataset == "vg":
        if sub2super is None:
            raise ValueError("sub2super_cat_dict is required for Visual Genome label vectors")
        sp = [[torch.as_tensor(sub2super[int(c)]) for c in cats.tolist()] for cats in categories_pred]
    batch = SceneBatch(image_feature, image_depth, [b.detach().float().cpu() for b in bbox_pred],
                       [c.detach().cpu().long() for c in categories_pred], sp, None, None)
    _, dev, scene = _scene_of(model, batch)
    return cfg, dev, batch, scene


def evaluate_sgdet_minibatch(model, image_feature, image_depth, categories_pred, cat_pred_confidence, bbox_pred, evaluator,
                             sub2super=None, targets=None, overlap_filtering: bool = True, skip_filtered: bool = False,
                             workspace_budget: Optional[float] = None):
    """SGDET evaluation of one minibatch (``evaluate.py:375-444``): every ordered pair of the PREDICTED objects of each image
    (per-image lists as returned by ``object_frontend.DetrFrontEnd.sgdet``: categories, category confidences, boxes
    (x0,x1,y0,y1) on the grid, one entry per image of ``image_feature``), overlap filter, evaluator fed in the reference's
    candidate order with ``predcls=False`` semantics (category confidences added).  ``targets`` =
    (relationships, subj_or_obj, categories_target, bbox_target) sets the ground truth through ``match_target_sgd`` +
    ``Evaluator.accumulate_target``; call ``evaluator.compute(per_class, predcls=False)`` afterwards.
    ``sub2super``: the ``sub2super_cat_dict`` (VG hierarchical label vectors)."""
    cfg, _, batch, scene = _sgdet_scene(model, image_feature, image_depth, categories_pred, bbox_pred, sub2super)
    iou, _, select = _filters(scene, overlap_filtering, skip_filtered, (evaluator,), steps=False)
    out = _scoring_forward(model, cfg, batch, scene, iou, select, workspace_budget)
    cat_conf = pair_cat_confidence(scene, cat_pred_confidence, _SGDET_NEEDS_CONFIDENCES)
    included = feed_evaluators(model, scene, out, evaluator, overlap=iou, cat_confidence=cat_conf, targets=False)
    if targets is not None:
        cs, co, bs, bo, rt = match_target_sgd(*targets)
        evaluator.accumulate_target(rt, cs, co, bs, bo)
    return scene, out, included.cpu().numpy()


def score_sgdet_minibatch(model, image_feature, image_depth, categories_pred, cat_pred_confidence, bbox_pred, meter, sub2super=None,
                          targets=None, overlap_filtering: bool = True, skip_filtered: bool = False,
                          workspace_budget: Optional[float] = None):
    """``evaluate_sgdet_minibatch`` for a ``metrics.RecallMeter``: SGDET / SGCLS Recall@K and zero-shot recall as device counters,
    without the appended int64 copies of every candidate, without ``match_target_sgd``'s per-element lists and without a read-back.
    The arguments are ``evaluate_sgdet_minibatch``'s; ``targets`` = (relationships, subj_or_obj, categories_target, bbox_target) is
    required (a meter without targets measures nothing).  The ground truth becomes one table (``pairs.sg_target_table``); it, the
    per-pair category confidences, the image lists and the boxes are put on the device BEFORE the forward is enqueued, and after
    it only ``meter.update(sg_targets=..., cat_conf=...)`` runs - nothing synchronises with the host; the numbers are the caller's
    ``meter.compute(per_class)``, the 6-tuple of ``Evaluator.compute(per_class, predcls=False)``.  Sets ``model.last_outputs``.
    Returns (scene, outputs)."""
    from .metrics import scene_boxes, upload_sg_targets
    from .pairs import sg_target_table
    if targets is None:
        raise ValueError("the metrics need the ground truth: targets=(relationships, subj_or_obj, categories_target, bbox_target)")
    cfg, dev, batch, scene = _sgdet_scene(model, image_feature, image_depth, categories_pred, bbox_pred, sub2super)
    table = upload_sg_targets(sg_target_table(*targets), dev)
    cat_conf = pair_cat_confidence(scene, cat_pred_confidence, _SGDET_NEEDS_CONFIDENCES)
    image_pair_lists(scene)                         # the per-scene tables of the update, made (and uploaded) once, before the forward
    scene_boxes(scene, dev)
    iou, included, select = _filters(scene, overlap_filtering, skip_filtered, (meter,))
    model.last_outputs = out = _scoring_forward(model, cfg, batch, scene, iou, select, workspace_budget)
    meter.update(scene, out, overlap=iou, included=included, sg_targets=table, cat_conf=cat_conf)
    return scene, out


def image_pair_lists(scene: DeviceScene):
    """(ptr [B+1] int32, list [P] int32) on the device: the pair rows of every image in ascending order - the per-image view of
    the step-major pair order that ``sgc_scene_graph_topk`` walks.  Derived once per scene (one stable device sort) and kept on it."""
    if scene._image_pairs is None:
        n = np.asarray(scene.num_objects, dtype=np.int64)
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(n * (n - 1))]).astype(np.int32)).to(scene.bbox.device)
        scene._image_pairs = (ptr, torch.sort(scene.image, stable=True)[1].to(torch.int32))
    return scene._image_pairs


def predict_scene_graphs(model, batch, top_k: int = 20, overlap_filtering: bool = True, commonsense=None, cat_confidence=None,
                         scene: Optional[DeviceScene] = None, workspace_budget: Optional[float] = None):
    """Image + objects in, the ranked top-``top_k`` (subject, predicate, object) triples of every image out (``scene_graph.SceneGraphs``,
    device tensors; ``.to_list(heights, widths, names)`` gives the reference's ``predicted_graph``, ``evaluator.py:465-503``).
    Needs no relation targets and no ``Evaluator``: the forward's outputs are ranked in place by one kernel
    (``sgc_scene_graph_topk``), with the confidences, filters and tie order of ``evaluate_minibatch`` + ``Evaluator.compute()``
    (``overlap_filtering``: a direction-step in which no image's boxes overlap contributes no candidates, a filtered pair's
    candidates rank at -inf).  ``commonsense`` = (aligned, violated) triplet collections or a ``commonsense.TripletBitmaps``: the
    ``eval_cs`` filter.  ``cat_confidence``: per-image lists of per-object category confidences, as ``evaluate_sgdet_minibatch``
    takes them (subject + object confidence is added to every candidate of the pair).  A minibatch over ``workspace_budget`` is
    scored in image groups like ``evaluate_minibatch``.  Everything the ranking needs besides the forward's outputs is put on the
    device BEFORE the forward is enqueued; nothing after it synchronises with the host."""
    from .scene_graph import attach_objects, rank_scene_graphs
    cfg, dev, scene = _scene_of(model, batch, scene)
    ptr, lst = image_pair_lists(scene)
    raw = raw_boxes(scene)
    bitmaps = _bitmaps_of(model, commonsense, dev)
    cat_conf = None if cat_confidence is None else pair_cat_confidence(scene, cat_confidence, "cat_confidence must hold one value per object")
    iou, included, _ = _filters(scene, overlap_filtering, False, ())
    model.last_outputs = out = _scoring_forward(model, cfg, batch, scene, iou, None, workspace_budget)
    # torch's own log(sigmoid(x)), as the evaluator feed forms it: the ranked scores are bit for bit the evaluator's confidences
    logsig = torch.log(torch.sigmoid(out.connectivity))
    graphs = rank_scene_graphs(out.cand_conf, out.cand_pred, logsig, ptr, top_k=top_k, pair_list=lst, slot_major=False, cat_conf=cat_conf,
                               mask=iou, included=included, sub_idx=scene.sub_idx, obj_idx=scene.obj_idx, cats=scene.cats, bitmaps=bitmaps)
    graphs.image = torch.arange(int(ptr.numel()) - 1, dtype=torch.int32, device=dev)
    return attach_objects(graphs, scene.cats, raw, cfg.feature_size)


def score_minibatch(model, batch, meter, overlap_filtering: bool = True, scene: Optional[DeviceScene] = None, skip_filtered: bool = False,
                    workspace_budget: Optional[float] = None, commonsense=None):
    """``evaluate_minibatch`` for a ``metrics.RecallMeter`` instead of the two evaluators: the fused forward, then the meter's counters
    (Recall@K, zero-shot recall, Top-3 for a hierarchical Visual Genome head, the OpenImages precision counters) updated on the device
    from the forward's outputs and the scene's tables - the candidates, filters and tie order of ``evaluate_minibatch`` +
    ``Evaluator.compute()`` + ``Evaluator_Top3.compute()`` / ``compute_precision()``, without the appended int64 copies and without a
    read-back.  ``batch`` needs relation targets.  ``skip_filtered`` / ``workspace_budget`` as ``evaluate_minibatch``; ``commonsense``
    as ``predict_scene_graphs`` (default: the meter's own sets in run mode eval_cs).  Sets ``model.last_outputs`` and, when the scene has
    raw targets and nothing was skipped, ``model.last_connectivity_stats``.  Everything the update needs besides the forward's outputs
    is put on the device BEFORE the forward is enqueued; nothing after it synchronises with the host - the numbers are the caller's
    ``meter.compute*()``.  PredCLS; the SGDET / SGCLS counterpart is ``score_sgdet_minibatch``.
    Returns (scene, outputs)."""
    from .metrics import scene_boxes
    cfg, dev, scene = _scene_of(model, batch, scene)
    directed = directed_targets(scene, getattr(batch, "relationships", None), getattr(batch, "subj_or_obj", None),
                                "the metrics need relation targets: a batch with relationships / subj_or_obj")
    image_pair_lists(scene)                         # the two per-scene tables of the update, made (and uploaded) once, before the forward
    scene_boxes(scene, dev)
    bitmaps = _bitmaps_of(model, commonsense, dev)
    iou, included, select = _filters(scene, overlap_filtering, skip_filtered, (meter,))
    model.last_outputs = out = _scoring_forward(model, cfg, batch, scene, iou, select, workspace_budget)
    meter.update(scene, out, overlap=iou, included=included, commonsense=bitmaps, top3=cfg.dataset == "vg", directed=directed)
    _connectivity_stats(model, scene, out, directed, included, select)
    return scene, out


def mine_commonsense_candidates(model, batch, top_k: int = 10, overlap_filtering: bool = True, scene: Optional[DeviceScene] = None,
                                workspace_budget: Optional[float] = None):
    """The candidate mining of ``run_mode prepare_cs`` for one minibatch without an ``Evaluator`` (``scene_graph.MinedCandidates``,
    device tensors; ``.to_lists(names)`` gives the lists of ``Evaluator.get_related_top_k_predictions_parallel``, and equals them
    exactly: both rank the same forward outputs).  The forward's candidates are ranked in place by ``sgc_scene_graph_topk`` - no
    connectivity term (``evaluate.py:200`` mines instead of ``compute()``), the overlap mask and the kept steps of
    ``predict_scene_graphs`` - and the ranked fields go straight to ``sgc_related_topk`` with the connected targets of the kept steps,
    per image in pair order (what ``feed_evaluators`` appends).  ``batch`` needs relation targets.  No appended int64 copies, and
    nothing after the forward synchronises with the host."""
    from .evaluator import related_topk
    from .scene_graph import MinedCandidates, rank_scene_graphs
    cfg, dev, scene = _scene_of(model, batch, scene)
    directed = directed_targets(scene, getattr(batch, "relationships", None), getattr(batch, "subj_or_obj", None),
                                "the candidate mining needs relation targets: a batch with relationships / subj_or_obj")
    ptr, lst = image_pair_lists(scene)
    raw = raw_boxes(scene)
    iou, included, _ = _filters(scene, overlap_filtering, False, ())
    model.last_outputs = out = _scoring_forward(model, cfg, batch, scene, iou, None, workspace_budget)
    P, B, K = scene.n_pairs, int(ptr.numel()) - 1, int(top_k)
    g = rank_scene_graphs(out.cand_conf, out.cand_pred, torch.zeros(P, device=dev), ptr, top_k=K, pair_list=lst, slot_major=False,
                          mask=iou, included=included, sub_idx=scene.sub_idx, obj_idx=scene.obj_idx, cats=scene.cats)   # x + 0 is exact
    # the ranked [B,K] fields ARE the flat candidate arrays of the scan: candidate b*K + j is rank j of image b
    ranked = g.subject >= 0
    sub, obj = g.subject.clamp(min=0).long().reshape(-1), g.object.clamp(min=0).long().reshape(-1)
    if int(scene.cats.numel()) == 0:
        return MinedCandidates(*[torch.full((B, 16), -1, dtype=torch.int32, device=dev) for _ in range(6)],
                               torch.full((B, 16), float("nan"), device=dev), torch.zeros(B, dtype=torch.int32, device=dev), g.count,
                               scene.cats, raw)
    cand = dict(scat=scene.cats[sub], ocat=scene.cats[obj], pred=g.predicate.reshape(-1), sbox=raw[sub], obox=raw[obj], conf=g.score.reshape(-1))
    keep_pos = torch.where(ranked, torch.arange(B * K, dtype=torch.int32, device=dev).view(B, K), torch.full_like(g.subject, -1))
    # connected targets of the kept steps, per image in pair order, compacted without a host synchronisation
    rows = lst.long()
    flag = directed.to(dev)[rows] != -1
    if included is not None:
        flag &= included[rows].bool()
    incl = torch.cumsum(flag.int(), 0)
    t_ptr = torch.cat((torch.zeros(1, dtype=incl.dtype, device=dev), incl))[ptr.long()].int()
    dest = torch.where(flag, incl.long() - 1, torch.full_like(rows, P))                 # row P: the slot the others are dropped into
    t_sub, t_obj = scene.sub_idx.long()[rows], scene.obj_idx.long()[rows]
    compact = lambda v: torch.zeros((P + 1,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev).index_put_((dest,), v)[:P]
    tg = dict(scat=compact(scene.cats[t_sub]), ocat=compact(scene.cats[t_obj]), sbox=compact(raw[t_sub].float()), obox=compact(raw[t_obj].float()))
    pos, rank, count, score = related_topk(cand, keep_pos.contiguous(), g.count, K, tg, t_ptr)
    at = rank.clamp(min=0).long()
    pick = lambda t: torch.where(rank >= 0, t.gather(1, at), torch.full_like(rank, -1))
    return MinedCandidates(pick(g.pair), pick(g.slot), pick(g.predicate), pick(g.subject), pick(g.object), rank, score, count, g.count,
                           scene.cats, raw)


def train_minibatch(model, batch, optimizer=None, reducer=None, scene: Optional[DeviceScene] = None,
                    workspace_budget: Optional[float] = None, streams: Optional[int] = None, input_grads: bool = False, **loss_kw):
    """One optimisation step over all ordered pairs of the minibatch; returns the loss tensor.
    ``input_grads=True``: ``model.last_input_grads`` holds d loss / d ``image_feature`` / ``image_depth`` / ``image_feature_aug`` of the
    whole minibatch (``model.training_step``; image groups write their own image slices, images without pairs get zeros; local to
    this rank with a ``reducer``), and a batch tensor that requires grad is driven backwards with it (``torch.autograd.backward``)
    after the head's backward and before ``optimizer.step()``: whatever produced the features - an adapter, the encoder - then has
    its ``.grad`` as after ``loss.backward()`` and can share the optimizer.
    A minibatch whose fused pass would exceed ``workspace_budget`` (bytes; default ``model.workspace_budget_bytes`` or 70 % of
    the free HBM) is run in consecutive image groups: whole-minibatch loss coefficients first, then forward + backward per group
    with its rows of them, the gradients summed and reduced across ranks once.  Equal to the one-pass step up to f32 summation
    order (dropout masks differ: the keep bit is indexed by a pair's position within its pass).
    ``streams`` (default ``model.pipeline_streams`` or 1): image groups run on that many concurrent HIP streams, each with its own
    engine workspace - the HBM-bound kernels of one group (expansion, contraction, im2col / col2im, fc1 assembly, ...) then share
    the chip with the MFMA-bound GEMMs of the other instead of leaving the matrix cores idle; a minibatch that fits in one pass
    is cut into ``streams`` balanced groups for that purpose.  Same arithmetic as the sequential groups.
    After a step taken HERE (``optimizer`` given) with ``TUNING.fused_sgd`` (default) ``model.fc1.weight.grad`` is None - its gradient
    lived in the engine's scratch in GEMM order and the fused update consumed it - while every other parameter keeps its ``.grad``
    like the reference's optimizer leaves it; callers that want to look at fc1.weight's gradient (norm logging, clipping) pass
    ``optimizer=None`` and step themselves, or run under ``engine.tuning(fused_sgd=False)``."""
    cfg = model.head_config()
    dev = next(model.parameters()).device
    if optimizer is not None:
        optimizer.zero_grad(set_to_none=True)
    lanes = int(streams if streams is not None else getattr(model, "pipeline_streams", 1) or 1)
    chunk_free = loss_kw.get("image_feature_aug") is None and loss_kw.get("commonsense") is None
    budget = _budget(model, workspace_budget)
    if loss_kw.get("image_feature_aug") is not None:
        budget *= 0.85          # the augmented view's trunk for the connected pairs lives in a second engine's workspace
    groups = plan_image_groups(cfg, batch, True, budget)
    if len(groups) == 1 and lanes > 1 and chunk_free:
        groups = split_balanced([int(b.shape[0]) for b in batch.bbox], lanes)
    model.last_image_groups = groups
    if scene is None:
        scene = flatten_scene(cfg, batch, dev)
    # fc1.weight's gradient in GEMM order for an optimizer that consumes it (optim.FusedSGD / distributed.ShardedSGD: ``fuse_fc1``):
    # the backward skips the transposition to the reference's column order, the optimizer's fused update un-permutes on the fly.  Not
    # with an all-reduce reducer over several ranks (a rank without pairs would apply its peers' mean gradient untagged); a ShardedSGD
    # that has taken one such gradient takes every later one that way (its accumulators and its peers' must agree).
    fuse_eng = None
    from .engine import TUNING
    # the object that ends up holding the step's gradients: a reducer that owns them (ShardedSGD - also when the caller steps it later,
    # ``optimizer=None``: gradient accumulation), else the optimizer
    owner = reducer if (reducer is not None and getattr(reducer, "owns_grads", False)) else optimizer
    sharded = owner is reducer and reducer is not None
    if sharded and optimizer is not None and optimizer is not reducer:
        raise ValueError("a reducer that owns the gradients (ShardedSGD) is its own optimizer: pass it as both, or optimizer=None")
    allreduce = reducer is not None and not sharded and getattr(reducer, "active", False)
    # decided by configuration only, never by this rank's data: every rank of a step must hand over the same column order (a rank
    # without pairs contributes zeros - order-free - but its optimizer must read its peers' mean gradient the way they wrote it)
    # (a ShardedSGD switches in ``attach`` only, where the ranks agree on it; a local FusedSGD whenever the tuning flag is on)
    if owner is not None and not allreduce and (getattr(owner, "fc1_gemm_order", False) or (not sharded and TUNING.fused_sgd)):
        fuse = getattr(owner, "fuse_fc1", None)
        fuse_eng = fuse(model) if fuse is not None else None
        if fuse_eng is None and getattr(owner, "fc1_gemm_order", False):
            raise RuntimeError("the gradient owner expects fc1.weight's gradient in GEMM order but this module cannot produce it")
    try:
        if fuse_eng is not None:
            fuse_eng.fc1_grad_gemm_order = True
        if len(groups) == 1:
            loss = model.training_step(scene, batch.relationships, batch.subj_or_obj, reducer=reducer, input_grads=bool(input_grads), **loss_kw)
        else:
            loss = _train_image_groups(model, cfg, batch, scene, groups, reducer, loss_kw, lanes=lanes, input_grads=bool(input_grads))
    except BaseException:
        # a GEMM-order gradient that may already hang on fc1.weight is a view of the engine's scratch in an order nobody else reads
        fc1 = getattr(model, "fc1", None)
        if fuse_eng is not None and fc1 is not None and getattr(fc1.weight, "_sgc_grad_gemm_order", False):
            fc1.weight.grad = None
            fc1.weight._sgc_grad_gemm_order = False
        raise
    finally:
        if fuse_eng is not None:
            fuse_eng.fc1_grad_gemm_order = False
    model.last_scene = scene
    if input_grads:
        _drive_input_autograd(batch, loss_kw.get("image_feature_aug"), model.last_input_grads)
    if optimizer is not None:
        try:
            optimizer.step()
        except BaseException:
            fc1 = getattr(model, "fc1", None)
            if fc1 is not None and getattr(fc1.weight, "_sgc_grad_gemm_order", False):
                fc1.weight.grad = None
                fc1.weight._sgc_grad_gemm_order = False
            raise
    return loss


class SgdetAssignment:
    """What ``assign_sgdet_targets`` wrote, all int32 on the device: ``directed`` [P] (the pair's predicate or -1), ``raw`` [P]
    (``directed``, or the reversed pair's where the pair itself is not connected), ``matched`` [P] (row of the target table or -1),
    ``target_hit`` [T] (1: the row was a candidate of some pair)."""

    def __init__(self, directed, raw, matched, target_hit):
        self.directed, self.raw, self.matched, self.target_hit = directed, raw, matched, target_hit

    def counts(self) -> torch.Tensor:
        """[3] int64 on the device: (targets, targets hit, pairs assigned).  Torch reductions; nothing is read back."""
        dev = self.matched.device
        return torch.stack((torch.full((), int(self.target_hit.numel()), dtype=torch.int64, device=dev),
                            self.target_hit.sum(dtype=torch.int64), (self.matched >= 0).sum(dtype=torch.int64)))


_EQUIV_DEVICE = {}


def _equiv_table(dev) -> torch.Tensor:
    """[160,160] u8 device copy of ``evaluator._equiv_matrix()``, uploaded once per device (as ``RecallMeter._equiv`` is)."""
    key = torch.device(dev)
    if key not in _EQUIV_DEVICE:
        from .evaluator import _equiv_matrix
        _EQUIV_DEVICE[key] = torch.from_numpy(_equiv_matrix().astype(np.uint8)).to(key)
    return _EQUIV_DEVICE[key]


def upload_sgdet_targets(table, n_img: int, dev):
    """``pairs.sg_target_table``'s numpy arrays plus their per-image row pointer as the device tensors ``assign_sgdet_targets`` takes:
    (image, relation, subject class, object class, subject box, object box, t_ptr [n_img+1] int32)."""
    from .pairs import _PinnedRing, _RINGS, sg_target_ptr
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise RuntimeError("upload_sgdet_targets stages the table for sgc_assign_pair_targets: it needs a GPU device (no CPU fallback)")
    ptr = sg_target_ptr(table[0], n_img)                # host: also checks that the rows are sorted by image
    # like flatten_scene: one pinned staging buffer, ONE asynchronous copy (seven pageable copies would each wait for the device to
    # finish the previous step's work); every array starts on a 16-byte boundary
    kinds = ((np.int32, torch.int32), (np.int64, torch.int64), (np.int64, torch.int64), (np.int64, torch.int64), (np.float32, torch.float32),
             (np.float32, torch.float32), (np.int32, torch.int32))
    parts = [np.ascontiguousarray(a, dtype=k[0]) for a, k in zip(tuple(table[:6]) + (ptr,), kinds)]
    offs, total = [], 0
    for a in parts:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    ring = _RINGS.setdefault(dev, _PinnedRing())
    with torch.cuda.device(dev):
        slot, host = ring.take(total)
        hv = host.numpy()
        for o, a in zip(offs, parts):
            hv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        stage = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        stage[:total].copy_(host[:total], non_blocking=True)
        ring.sent(slot)
    out = [stage[o:o + a.nbytes].view(k[1]) if a.nbytes else torch.empty(0, dtype=k[1], device=dev) for o, a, k in zip(offs, parts, kinds)]
    out[4], out[5] = out[4].view(-1, 4), out[5].view(-1, 4)
    return tuple(out)


def assign_sgdet_targets(scene: DeviceScene, table, *, equiv=True, iou_thresh: float = 0.5, num_relations: int,
                         feature_size: Optional[int] = None) -> SgdetAssignment:
    """Per-pair training targets of a scene of DETECTED objects from the ground truth as one table (``sgc_assign_pair_targets``;
    INTEGRATION.md section J has the semantics in full).  ``table``: the device tensors of ``upload_sgdet_targets`` - or the six of
    ``metrics.upload_sg_targets``, sorted by image; the row pointer is then derived on the device.  A row is a candidate of a pair
    when evaluation would credit the pair for it apart from the predicate: 0 <= relation < ``num_relations``, labels equal or -
    ``equiv=True``: the reference's equivalence classes, ``evaluator._equiv_matrix()``; a [n,n] u8 device tensor: that table;
    ``False`` / ``None``: equality only (OpenImages) - equivalent as ``equiv[target class][detection class]``, both grid IoUs >=
    ``iou_thresh``.  The pair gets the candidate with the largest product of the two grid IoUs (exact integers; smallest row on a
    tie).  Sets ``scene.directed`` and ``scene.raw_target``, so that the loss coefficients, the coupled terms and the connectivity
    statistics see an assigned scene like a PredCLS one.  Nothing synchronises with the host; there is no CPU path."""
    from .metrics import scene_boxes
    dev = scene.cats.device
    if dev.type != "cuda":
        raise RuntimeError("assign_sgdet_targets runs on the GPU (sgc_assign_pair_targets, no CPU fallback): the scene must be on a cuda device")
    if len(table) not in (6, 7):
        raise ValueError("table is (image, relation, subject class, object class, subject box, object box[, t_ptr])")
    for t in table:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("assign_sgdet_targets runs on the GPU (no CPU fallback): the target table must be cuda tensors")
    T = int(table[0].numel())
    if any(int(t.numel()) != n * T for t, n in zip(table, (1, 1, 1, 1, 4, 4))):
        raise ValueError("the arrays of the target table disagree in length: [T] image, relation and classes, [T,4] boxes")
    B, P, n_obj = int(scene.image_feature.shape[0]), int(scene.n_pairs), int(scene.cats.numel())
    t_image = table[0].to(torch.int32).contiguous()
    t_rel, t_scat, t_ocat = (t.to(torch.int64).contiguous() for t in table[1:4])
    t_sbox, t_obox = (t.to(torch.float32).contiguous() for t in table[4:6])
    if len(table) == 7:
        t_ptr = table[6].to(torch.int32).contiguous()
        if int(t_ptr.numel()) != B + 1:
            raise ValueError("t_ptr must hold one entry per image of the scene plus one")
    else:
        t_ptr = torch.searchsorted(t_image, torch.arange(B + 1, dtype=torch.int32, device=dev)).to(torch.int32)
    eq = None
    if equiv is True:
        eq = _equiv_table(dev)
    elif torch.is_tensor(equiv):
        if not equiv.is_cuda or equiv.dim() != 2 or equiv.shape[0] != equiv.shape[1]:
            raise ValueError("equiv must be a square [n,n] cuda tensor")
        eq = equiv.to(torch.uint8).contiguous()
    elif equiv not in (False, None):
        raise ValueError("equiv is True (the reference's classes), False / None (equality only) or a [n,n] u8 cuda tensor")
    F = int(scene.image_feature.shape[-1]) if feature_size is None else int(feature_size)
    out = torch.empty(3 * P + T, dtype=torch.int32, device=dev)
    directed, raw, matched, hit = out[:P], out[P:2 * P], out[2 * P:3 * P], out[3 * P:]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sgc_assign_pair_targets(
            _lib.ptr(scene.sub_idx), _lib.ptr(scene.obj_idx), _lib.ptr(scene.image), P, _lib.ptr(scene.pid), int(scene.pid.shape[1]),
            _lib.ptr(scene.img_ptr), _lib.ptr(scene.cats), _lib.ptr(scene_boxes(scene, dev)), n_obj, _lib.ptr(t_ptr), B, _lib.ptr(t_rel),
            _lib.ptr(t_scat), _lib.ptr(t_ocat), _lib.ptr(t_sbox), _lib.ptr(t_obox), T, _lib.ptr(eq), 0 if eq is None else int(eq.shape[0]),
            int(num_relations), F, ctypes.c_double(float(iou_thresh)), _lib.ptr(directed), _lib.ptr(raw), _lib.ptr(matched), _lib.ptr(hit),
            _lib.stream_ptr()), "sgc_assign_pair_targets")
    scene.directed, scene.raw_target = directed, raw
    return SgdetAssignment(directed, raw, matched, hit)


def train_sgdet_minibatch(model, image_feature, image_depth, categories_pred, bbox_pred, targets, optimizer=None, reducer=None,
                          sub2super=None, equiv=True, iou_thresh: float = 0.5, workspace_budget: Optional[float] = None,
                          streams: Optional[int] = None, input_grads: bool = False, **loss_kw):
    """One optimisation step on the DETECTED objects of an SGDET minibatch (``BASELINE.json`` configs[3]): ``train_minibatch`` over every
    ordered pair of the predicted objects (per-image lists ``categories_pred`` / ``bbox_pred`` as ``evaluate_sgdet_minibatch`` takes
    them), with the ground truth ``targets`` = (relationships, subj_or_obj, categories_target, bbox_target) assigned to those pairs on
    the device (``assign_sgdet_targets``): a pair is trained towards a relation exactly when evaluation would credit it for that
    relation.  SGCLS training is the same call with the lists ``match_object_categories`` returns (ground-truth boxes, predicted
    labels).  Every relation is collected (``sg_target_table(drop_last_graph_object=False)``).  The table is built and uploaded
    before anything is enqueued behind it; nothing synchronises between the assignment and the step.  ``equiv`` / ``iou_thresh`` as
    ``assign_sgdet_targets``; everything else - ``image_feature_aug=`` and ``commonsense=`` included - as ``train_minibatch``.
    Returns the loss; ``model.last_assignment`` holds the ``SgdetAssignment``."""
    from .pairs import sg_target_table
    table = upload_sgdet_targets(sg_target_table(*targets, drop_last_graph_object=False), len(categories_pred),
                                 next(model.parameters()).device)
    cfg, dev, batch, scene = _sgdet_scene(model, image_feature, image_depth, categories_pred, bbox_pred, sub2super)
    model.last_assignment = assign_sgdet_targets(scene, table, equiv=equiv, iou_thresh=iou_thresh, num_relations=cfg.num_relations,
                                                 feature_size=cfg.feature_size)
    return train_minibatch(model, batch, optimizer, reducer, scene=scene, workspace_budget=workspace_budget, streams=streams,
                           input_grads=input_grads, **loss_kw)


def _drive_input_autograd(batch, aug, grads):
    """Hand the head's input gradients to the autograd graph that produced the minibatch's tensors (those that require grad)."""
    roots, gs = [], []
    for t, g in ((batch.image_feature, grads["image_feature"]), (batch.image_depth, grads["image_depth"]), (aug, grads["image_feature_aug"])):
        if torch.is_tensor(t) and t.requires_grad and g is not None:
            roots.append(t)
            gs.append(g.to(device=t.device, dtype=t.dtype).view_as(t))
    if roots:
        torch.autograd.backward(roots, gs)


_LANE_STREAMS = {}


def _lane_stream(dev, k):
    key = (torch.device(dev), k)
    if key not in _LANE_STREAMS:
        _LANE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _LANE_STREAMS[key]


def _coupled_terms(model, cfg, batch, scene: DeviceScene, groups, subs, aug, commonsense, lam):
    """The minibatch-level pieces of the contrastive (``train_test.py:260-273``, ``sup_contrast/losses.py:85-181``) and commonsense
    (``train_utils.py:36-62``) terms for a minibatch that runs in image groups.  Both couple all pairs through the FORWARD: the
    SupCon loss reads the hidden rows of every connected pair of the minibatch (two views), the commonsense penalty's per-step
    means count the flagged candidates of every image in the step.  So every group's training-mode forward runs first
    (``model.coupled_forward``; nothing but [M, 512] rows and [P, n_cand] predicates is kept), the loss and its feature gradient /
    the per-candidate coefficients are computed ONCE for the minibatch, and the groups' second pass (same dropout seeds: the same
    forward bit for bit) gets its rows of them.  Costs one extra forward per group - the price of not holding every group's
    workspace at once.  Returns (per-group ``coupled`` dicts, contrastive loss tensor or None)."""
    dev = scene.bbox.device
    eng = model.refresh_weights(backward=True)
    P = scene.n_pairs
    nc = 3 if cfg.hierarchical else 1
    cand_full = torch.zeros(P, nc, dtype=torch.int32, device=dev) if commonsense is not None else None
    conn_full = torch.nonzero(scene.directed >= 0).flatten() if aug is not None else None
    M = int(conn_full.numel()) if conn_full is not None else 0
    feats = torch.zeros(2 * M, 512, dtype=torch.float32, device=dev) if M > 0 else None
    per_group = []
    for (a, b), (rows, sub) in zip(groups, subs):
        if sub is None:
            per_group.append(None)
            continue
        st = model.coupled_forward(sub, None if aug is None else aug[a:b], want_candidates=commonsense is not None)
        pos = None
        if cand_full is not None:
            cand_full[rows] = st["cand_pred"]
        if aug is not None and st["conn_idx"] is not None and int(st["conn_idx"].numel()) > 0:
            pos = torch.searchsorted(conn_full, rows[st["conn_idx"]])       # this group's connected pairs in the minibatch's list
            feats[pos] = st["hidden"]
            feats[M + pos] = st["hidden_aug"]
        per_group.append(dict(seeds=st["seeds"], pos=pos))
    cs_full = None
    if commonsense is not None:
        cs_full = eng.commonsense_coefficients(cand_full, model._commonsense_bitmaps(commonsense, dev), scene.step.long(), scene.n_steps,
                                               scene.cats[scene.sub_idx.long()], scene.cats[scene.obj_idx.long()],
                                               lam["lambda_commonsense"], lam["lambda_cs_weak"], lam["lambda_cs_strong"])
    loss_c, dF = None, None
    if M > 0:
        lam2 = float(lam["lambda_contrast"]) ** 2
        loss_c, dF = eng.supcon_loss(feats, scene.directed[conn_full].to(torch.int32).contiguous(), grad_scale=lam2)
    out = []
    for (rows, sub), g in zip(subs, per_group):
        if g is None:
            out.append(None)
            continue
        out.append(dict(seeds=g["seeds"], cs_coef=None if cs_full is None else cs_full[rows],
                        contrast=None if (dF is None or g["pos"] is None) else (dF[g["pos"]], dF[M + g["pos"]])))
    return out, loss_c


def _train_image_groups(model, cfg, batch, scene: DeviceScene, groups, reducer, loss_kw, lanes: int = 1, input_grads: bool = False):
    from .engine import PairOutputs
    dev = scene.bbox.device
    kw = dict(loss_kw)
    aug, commonsense = kw.pop("image_feature_aug", None), kw.pop("commonsense", None)
    ig = None
    if input_grads:                                 # minibatch-sized; every group writes its own image slice (zeros where it has no pairs)
        ig = {"image_feature": torch.zeros_like(scene.image_feature), "image_depth": torch.zeros_like(scene.image_depth),
              "image_feature_aug": torch.zeros_like(scene.image_feature) if aug is not None else None}
        w = model.refresh_weights(backward=True).w
        if lanes > 1 and "wd1" in w.deferred:       # deferred copy: made on the caller's stream, before the lanes' streams read it
            w["wd1"]
    lam = dict(lambda_contrast=kw.pop("lambda_contrast", 1.0), lambda_commonsense=kw.pop("lambda_commonsense", 1.0),
               lambda_cs_weak=kw.pop("lambda_cs_weak", 0.1), lambda_cs_strong=kw.pop("lambda_cs_strong", 10.0))
    coupled_terms = aug is not None or commonsense is not None
    if coupled_terms:
        lanes = 1                                   # two passes per group on the module's own engine
        if scene.directed is None:
            raise ValueError("the contrastive / commonsense terms need relation targets in the scene")
    coefs = model.minibatch_loss_coefficients(scene, kw.pop("class_weight", None), kw.pop("lambda_connectivity", 0.1),
                                              kw.pop("lambda_not_connected", 1.0))
    # a scene whose targets were ASSIGNED (assign_sgdet_targets: the batch of detected objects has no relationship lists): every group
    # gets its rows of them - the group's pair order is the minibatch's restricted to its images - instead of list slices
    assigned = getattr(batch, "relationships", None) is None and scene.directed is not None
    subs = []
    for a, b in groups:
        rows = _group_rows(scene, a, b)
        if rows.numel() == 0:
            subs.append((rows, None))
            continue
        sub_b = slice_batch(batch, a, b)
        sub = flatten_scene(cfg, sub_b, dev)
        assert sub.n_pairs == int(rows.numel())
        if assigned:
            sub.directed = scene.directed[rows].contiguous()
            sub.raw_target = None if scene.raw_target is None else scene.raw_target[rows].contiguous()
        sub._batch = sub_b
        subs.append((rows, sub))
    coupled, loss_c = (None, None)
    if coupled_terms:
        coupled, loss_c = _coupled_terms(model, cfg, batch, scene, groups, subs, aug, commonsense, lam)
    P = scene.n_pairs
    nc = 3 if cfg.hierarchical else 1
    full = PairOutputs(torch.zeros(P, cfg.num_relations, device=dev), torch.zeros(P, 3, device=dev) if cfg.hierarchical else None,
                       torch.zeros(P, device=dev), torch.zeros(P, 512, device=dev), torch.zeros(P, nc, device=dev),
                       torch.zeros(P, nc, dtype=torch.int32, device=dev))
    lanes = max(1, min(int(lanes), len(groups)))
    main = torch.cuda.current_stream(dev)
    lane = [dict(stream=main if lanes == 1 else _lane_stream(dev, k), engine=model.lane_engine(k), acc={},
                 stats=torch.zeros(5, dtype=torch.int64, device=dev), loss=torch.zeros((), device=dev)) for k in range(lanes)]
    if lanes > 1:
        for ln in lane:
            ln["stream"].wait_stream(main)          # coefficients, weights and the full-size outputs are ready; last step's reads are done
    for gi, (a, b) in enumerate(groups):
        ln = lane[gi % lanes]
        with torch.cuda.stream(ln["stream"]):
            rows, sub = subs[gi]
            if sub is None:
                continue
            sub_b = sub._batch
            extra = {}
            if coupled is not None:
                extra = dict(coupled=coupled[gi], image_feature_aug=None if aug is None else aug[a:b])
            if ig is not None:
                extra["input_grads"] = {k: (None if t is None else t[a:b]) for k, t in ig.items()}
            ln["loss"] = ln["loss"] + model.training_step(sub, sub_b.relationships, sub_b.subj_or_obj,
                                                          loss_coefs=tuple(c[rows] for c in coefs), grads_out=ln["acc"],
                                                          engine=ln["engine"] if coupled is None else None, **extra, **kw)
            out = model.last_outputs
            full.relation[rows] = out.relation
            if full.super_relation is not None:
                full.super_relation[rows] = out.super_relation
            full.connectivity[rows] = out.connectivity
            full.hidden[rows] = out.hidden
            full.cand_conf[rows] = out.cand_conf
            full.cand_pred[rows] = out.cand_pred
            if model.last_connectivity_stats is not None:
                ln["stats"] += model.last_connectivity_stats
    if lanes > 1:
        for ln in lane:
            main.wait_stream(ln["stream"])
    acc, stats, loss = lane[0]["acc"], lane[0]["stats"], lane[0]["loss"]
    for ln in lane[1:]:                               # lane sums -> the minibatch's sums (fixed order: deterministic)
        for name, g in ln["acc"].items():
            if name in acc:
                acc[name].add_(g)
            else:
                acc[name] = g
        stats, loss = stats + ln["stats"], loss + ln["loss"]
    if loss_c is not None:
        if not bool(torch.isnan(loss_c)):
            loss = loss + float(lam["lambda_contrast"]) ** 2 * loss_c          # lambda applied twice (train_test.py:270-273)
        model.last_contrast_loss = loss_c
    for name, p in model.named_parameters():          # no group had a pair: a zero gradient, not a missing one
        if name not in acc:
            acc[name] = torch.zeros_like(p)
    # the minibatch's gradient = the sum over its image groups: mean-reduce it across ranks once, then accumulate like autograd
    if reducer is not None:
        if getattr(reducer, "owns_grads", False) and bool(getattr(reducer, "fc1_gemm_order", False)) != bool(lane[0]["engine"].fc1_grad_gemm_order):
            raise RuntimeError("fc1.weight's gradient order differs from what the sharded optimizer accumulates")
        if "fc1.weight" in acc:
            reducer.hook("fc1.weight", acc["fc1.weight"])
        reducer.finish_grads(acc)
    if not getattr(reducer, "owns_grads", False):
        model.accumulate_grads(acc, lane[0]["engine"])
    model.last_outputs, model.last_connectivity_stats = full, stats
    model.last_input_grads = ig
    return loss
