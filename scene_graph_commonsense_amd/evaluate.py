"""Drop-in for the reference's ``evaluate.py``: ``eval_pc`` (``evaluate.py:29-227``), ``eval_sgd`` (``:230-461``) and ``eval_sgc``
(``:464-702``) with the reference's signatures, so ``main.py``'s ``from evaluate import eval_pc, eval_sgc, eval_sgd`` +
``mp.spawn(eval_*, ...)`` (``main.py:15,112-123``) run on the MI355X path.

One process per GPU over RCCL; the pair loops are one fused call per minibatch (``pair_loop.evaluate_minibatch`` /
``evaluate_sgdet_minibatch``); the DETR decoder outputs go through the HIP object front-end (``object_frontend.DetrFrontEnd``:
soft-max / top-k / class re-indexing / boxes / per-class NMS, and the SGCLS label matching).  Evaluation needs no collective;
every rank writes its own ``test_results_<rank>.json`` as in the reference.

``run_mode prepare_cs`` (``evaluate.py:41-42,99-101,193-221``) runs here too: step 1 is the PredCLS pass with
``Evaluator.get_related_top_k_predictions_parallel(top_k=10)`` in the place of ``compute()`` - ranking and the candidate scan on the
device, the judged edge lists written per image - and step 2 walks the loader without a forward (the host dataset accumulates the
triplets in ``__getitem__``) and ends with ``curr_dataset.save_all_triplets()``.  The LLM itself stays outside: the judge is
``args['models']['cs_judge']`` or the host repository's ``query_llm``; this package opens no connection.  Out of scope as in
DESIGN.md: ``save_vis_results`` (it raises).
"""
from __future__ import annotations

import json
import os

import torch
import torch.distributed as dist

from .evaluator import Evaluator, Evaluator_Top3
from .object_frontend import DetrFrontEnd
from .metrics import RecallMeter
from .pair_loop import (MinibatchLookahead, evaluate_minibatch, evaluate_sgdet_minibatch, freeze_setup_objects, score_minibatch,
                        score_sgdet_minibatch)
from .pairs import flatten_scene
from .train_test import (_collate, _host, _record_test, _to_batch, build_classifier, build_feature_encoder, load_checkpoint, setup)
from .train_utils import process_image_features


def _loader(args, test_subset, rank, world_size):
    sampler = torch.utils.data.distributed.DistributedSampler(test_subset, num_replicas=world_size, rank=rank)
    return torch.utils.data.DataLoader(test_subset, batch_size=args["training"]["batch_size"], shuffle=False,
                                       collate_fn=_host("collate_fn", _collate), num_workers=0, drop_last=True, sampler=sampler)


def _start(gpu, args, test_subset, with_model=True):
    rank = gpu
    world_size = int(os.environ.get("WORLD_SIZE", 0)) or max(torch.cuda.device_count(), 1)
    setup(rank, world_size)
    print("rank", rank, "torch.distributed.is_initialized", dist.is_initialized())
    loader = _loader(args, test_subset, rank, world_size)
    print("Finished loading the datasets...")
    with open(args["training"]["result_path"] + "test_results_" + str(rank) + ".json", "w") as f:
        json.dump([], f)
    if not with_model:
        return rank, loader, None, None
    model = build_classifier(args, rank)
    detr = build_feature_encoder(args, rank)
    model.eval()
    load_checkpoint(model, args, args["training"]["test_epoch"], args["training"]["run_mode"] == "eval_cs", rank)
    return rank, loader, model, detr


def _finish(name):
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    print("FINISHED TESTING %s\n" % name)


def _meter_results(meter, vg, hier):
    """The record's numbers from a ``RecallMeter`` - its only host reads: (recall, mean_recall, recall_top3, mean_recall_top3, recall_zs,
    mean_recall_zs, wmap_rel, wmap_phrase), None where the evaluator route leaves None."""
    recall, _, mean_recall, recall_zs, _, mean_recall_zs = meter.compute(per_class=True)
    recall_top3 = mean_recall_top3 = wmap_rel = wmap_phrase = None
    if vg and hier:
        recall_top3, _, mean_recall_top3 = meter.compute_top3(per_class=True)
    if not vg:
        wmap_rel, wmap_phrase = meter.compute_precision()
    return recall, mean_recall, recall_top3, mean_recall_top3, recall_zs, mean_recall_zs, wmap_rel, wmap_phrase


def eval_pc(gpu, args, test_subset, curr_dataset=None, prepare_cs_step=-1):
    """Predicate classification (``evaluate.py:29-227``).  With ``args['training']['device_metrics']`` (not in ``prepare_cs``) the two
    evaluators are replaced by one ``metrics.RecallMeter``: ``pair_loop.score_minibatch`` updates its device counters per minibatch
    and the host reads them only where a record is written; the records are the same."""
    T = args["training"]
    prepare_cs = T["run_mode"] == "prepare_cs"
    if prepare_cs != (prepare_cs_step != -1) or (prepare_cs and prepare_cs_step not in (1, 2)):
        raise ValueError("prepare_cs_step is 1 or 2 with run_mode prepare_cs and -1 otherwise (main.py:112-114)")
    if T.get("save_vis_results"):
        raise NotImplementedError("save_vis_results is outside this package's scope (DESIGN.md)")
    if prepare_cs:
        if curr_dataset is None:
            raise ValueError("run_mode prepare_cs needs curr_dataset (the dataset behind test_subset: its train_cs_step selects the step)")
        if args["dataset"]["dataset"] != "vg":
            raise ValueError("run_mode prepare_cs is defined for Visual Genome only (evaluate.py:192-200)")
        curr_dataset.train_cs_step = prepare_cs_step
    if prepare_cs_step == 2:
        # nothing to score: the host dataset's __getitem__ accumulates every image's triplets from the files of step 1
        rank, loader, _, _ = _start(gpu, args, test_subset, with_model=False)
        print("Start Testing PC...")
        for _ in loader:
            pass
        curr_dataset.save_all_triplets()
        _finish("PC")
        return None, None
    rank, loader, model, detr = _start(gpu, args, test_subset)
    hier, vg = args["models"]["hierarchical_pred"], args["dataset"]["dataset"] == "vg"
    record_test = _host("record_test_results", _record_test)
    test_record = []
    stats = torch.zeros(5, dtype=torch.int64, device=rank)
    recall = recall_top3 = mean_recall_top3 = mean_recall = recall_zs = mean_recall_zs = wmap_rel = wmap_phrase = None
    skip = bool(T.get("skip_filtered_pairs", False))
    print("Start Testing PC...")
    freeze_setup_objects()
    cfg, dev = model.head_config(), next(model.parameters()).device

    def prepare(batch_count, data):
        """minibatch k+1 is loaded, encoded and flattened while the device scores minibatch k (pair_loop.MinibatchLookahead)"""
        try:
            batch, _, annot_path = _to_batch(args, data, detr, rank, with_aug=False)
        except (ValueError, IndexError):
            return None
        return batch, annot_path, flatten_scene(cfg, batch, dev)
    if T.get("device_metrics") and not prepare_cs:
        meter = RecallMeter(args, args["models"]["num_relations"], iou_thresh=0.5, top_k=[20, 50, 100], device=dev)
        with torch.no_grad():
            ahead = MinibatchLookahead(loader, prepare)
            for batch_count, (batch, annot_path, scene) in ahead:
                last = batch_count + 1 == len(loader)
                feed = batch_count % T["eval_freq_test"] == 0 or last
                if feed:
                    score_minibatch(model, batch, meter, skip_filtered=skip, scene=scene)
                else:
                    evaluate_minibatch(model, batch, None, None, skip_filtered=skip, scene=scene)
                if model.last_connectivity_stats is not None:
                    stats += model.last_connectivity_stats
                if feed and (batch_count % T["print_freq_test"] == 0 or last):
                    recall, mean_recall, recall_top3, mean_recall_top3, recall_zs, mean_recall_zs, wmap_rel, wmap_phrase = \
                        _meter_results(meter, vg, hier)
                    s = stats.tolist()
                    record_test(args, test_record, rank, T["test_epoch"], recall_top3, recall, mean_recall_top3, mean_recall, recall_zs,
                                mean_recall_zs, torch.tensor(float(s[4])), s[1], s[0], torch.tensor(float(s[3])), s[2], wmap_rel, wmap_phrase)
        _finish("PC")
        return recall, mean_recall
    Recall = Evaluator(args=args, num_classes=args["models"]["num_relations"], iou_thresh=0.5, top_k=[20, 50, 100])
    Recall_top3 = Evaluator_Top3(args=args, num_classes=args["models"]["num_relations"], iou_thresh=0.5, top_k=[20, 50, 100]) if vg else None
    if prepare_cs:
        Recall_top3 = None                  # the mining reads Recall only; the reference's Top-3 result of this mode is never recorded
    with torch.no_grad():
        ahead = MinibatchLookahead(loader, prepare)
        for batch_count, (batch, annot_path, scene) in ahead:
            Recall.load_annotation_paths(annot_path)
            last = batch_count + 1 == len(loader)
            feed = batch_count % T["eval_freq_test"] == 0 or last
            evaluate_minibatch(model, batch, Recall if feed else None, Recall_top3 if (feed and hier) else None, skip_filtered=skip,
                               scene=scene, while_running=ahead.fetch_next)
            if model.last_connectivity_stats is not None:
                stats += model.last_connectivity_stats
            if feed:
                if prepare_cs:
                    # candidates mined from the state as accumulated: no connectivity term, no recall (evaluate.py:193-202)
                    _, _, cache_hit_percentage = Recall.get_related_top_k_predictions_parallel(top_k=10)
                    if last:
                        print("cache hit percentage", cache_hit_percentage)
                elif vg:
                    recall, _, mean_recall, recall_zs, _, mean_recall_zs = Recall.compute(per_class=True)
                    if hier:
                        recall_top3, _, mean_recall_top3 = Recall_top3.compute(per_class=True)
                        Recall_top3.clear_data()
                else:
                    recall, _, mean_recall, _, _, _ = Recall.compute(per_class=True)
                    wmap_rel, wmap_phrase = Recall.compute_precision()
                if not prepare_cs and (batch_count % T["print_freq_test"] == 0 or last):
                    s = stats.tolist()
                    record_test(args, test_record, rank, T["test_epoch"], recall_top3, recall, mean_recall_top3, mean_recall, recall_zs,
                                mean_recall_zs, torch.tensor(float(s[4])), s[1], s[0], torch.tensor(float(s[3])), s[2], wmap_rel, wmap_phrase)
                Recall.clear_data()
    _finish("PC")
    return recall, mean_recall


def _detr_outputs(detr, image2, rank):
    """``detr(nested_tensor_from_tensor_list(image2))`` -> (pred_logits [B,100,C+1], pred_boxes [B,100,4]) (``evaluate.py:309``);
    a feature encoder that is not the DETR module must offer ``detect(images)`` returning the same dict."""
    images = [im.to(rank) for im in image2]
    if hasattr(detr, "detect"):
        out = detr.detect(images)
    else:
        try:
            from utils import nested_tensor_from_tensor_list        # host repository helper
        except Exception:
            from .detr import nested_tensor_from_tensor_list
        out = detr(nested_tensor_from_tensor_list(images))
    return out["pred_logits"], out["pred_boxes"]


def _sg_common(gpu, args, test_subset, sgcls: bool):
    """``eval_sgd`` / ``eval_sgc``.  With ``args['training']['device_metrics']`` the ``Evaluator`` is replaced by one
    ``metrics.RecallMeter``: ``pair_loop.score_sgdet_minibatch`` updates its device counters per minibatch from the ground truth as one
    target table, and the host reads them only where a record is written; records and return values are the same."""
    T = args["training"]
    rank, loader, model, detr = _start(gpu, args, test_subset)
    meter = Recall = None
    if T.get("device_metrics"):
        meter = RecallMeter(args, args["models"]["num_relations"], iou_thresh=0.5, top_k=[20, 50, 100],
                            device=next(model.parameters()).device)
    else:
        Recall = Evaluator(args=args, num_classes=args["models"]["num_relations"], iou_thresh=0.5, top_k=[20, 50, 100])
    sub2super = torch.load(args["dataset"]["sub2super_cat_dict"])
    try:
        from dataset_utils import object_class_alp2fre                # the host repository's own class-index table
        alp2fre = object_class_alp2fre()
    except Exception:
        alp2fre = args["dataset"].get("object_class_alp2fre")
        if alp2fre is None:
            raise RuntimeError("the DETR (alphabetical) -> dataset (frequency) class table is needed: make the host repository's "
                               "dataset_utils importable or pass args['dataset']['object_class_alp2fre']")
    fe = DetrFrontEnd(alp2fre, num_classes=args["models"]["num_classes"], topk_cat=args["models"]["topk_cat"],
                      feature_size=args["models"]["feature_size"], nms=args["models"]["nms"])
    record_test = _host("record_test_results", _record_test)
    test_record = []
    recall = mean_recall = recall_zs = mean_recall_zs = None
    unread = False
    name = "SGC" if sgcls else "SGD"
    print("Start Testing %s..." % name)
    freeze_setup_objects()
    with torch.no_grad():
        for batch_count, data in enumerate(loader):
            try:
                images, image2, image_depth, categories_target, _, bbox_target, relationships, subj_or_obj = data[:8]
            except ValueError:
                continue
            image_feature = process_image_features(args, images, detr, rank)
            depth = torch.stack([d.to(rank) for d in image_depth])
            logits, boxes = _detr_outputs(detr, image2, rank)
            categories_pred, cat_conf, bbox_pred, kept = fe.sgdet(logits, boxes)
            if len(kept) != int(image_feature.shape[0]):
                continue              # an image without any detected object: the reference's index bookkeeping breaks there too
            cats_t = [c.to(rank) for c in categories_target]
            box_t = [b.to(rank) for b in bbox_target]
            if sgcls:                 # ground-truth boxes, labels matched from the predictions (utils.py:376-425)
                matched = fe.match_object_categories(categories_pred, cat_conf, bbox_pred, box_t)
                if matched[0] is None or matched[1] is None:
                    continue
                categories_pred, cat_conf, bbox_pred = matched[0], matched[1], matched[2]
            last = batch_count + 1 == len(loader)
            if batch_count % T["eval_freq_test"] == 0 or last:
                write = batch_count % T["print_freq_test"] == 0 or last
                if meter is not None:
                    # the target table is built on the host: the loader's own (host) class and box lists, not their device copies
                    score_sgdet_minibatch(model, image_feature, depth, categories_pred, cat_conf, bbox_pred, meter, sub2super=sub2super,
                                          targets=(relationships, subj_or_obj, categories_target, bbox_target),
                                          skip_filtered=bool(T.get("skip_filtered_pairs", False)))
                    unread = not write
                    if write:               # the meter's host read: only where a record is written
                        recall, _, mean_recall, recall_zs, _, mean_recall_zs = meter.compute(per_class=True)
                else:
                    evaluate_sgdet_minibatch(model, image_feature, depth, categories_pred, cat_conf, bbox_pred, Recall,
                                             sub2super=sub2super, targets=(relationships, subj_or_obj, cats_t, box_t),
                                             skip_filtered=bool(T.get("skip_filtered_pairs", False)))
                    recall, _, mean_recall, recall_zs, _, mean_recall_zs = Recall.compute(per_class=True, predcls=False)
                    Recall.clear_data()
                if write:
                    record_test(args, test_record, rank, T["test_epoch"], None, recall, None, mean_recall, recall_zs, mean_recall_zs,
                                torch.tensor(0.0), 0.0, 0.0, torch.tensor(0.0), 0.0, None, None)
    if unread:                              # minibatches scored after the last record: the return value counts them, as the evaluator's does
        recall, _, mean_recall, _, _, _ = meter.compute(per_class=True)
    _finish(name)
    return recall, mean_recall


def eval_sgd(gpu, args, test_subset):
    """Scene graph detection (``evaluate.py:230-461``): predicted boxes and labels."""
    return _sg_common(gpu, args, test_subset, sgcls=False)


def eval_sgc(gpu, args, test_subset):
    """Scene graph classification (``evaluate.py:464-702``): ground-truth boxes, predicted labels."""
    return _sg_common(gpu, args, test_subset, sgcls=True)
