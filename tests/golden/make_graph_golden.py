#!/usr/bin/env python3
"""Generate tests/golden/predicted_graph.npz by running the REAL reference's ``Evaluator.save_visualization_results``
(``evaluator.py:465-519``) on the Evaluator state of the ``vg_full_hit`` case.

Runs only in the build container (needs /root/reference), with the stubs and helpers of ``make_golden.py``.  The eval loop of
``train_test.py`` is restated around the reference's own ``evaluate_one_direction`` / ``Evaluator`` exactly as ``make_golden.py``
does; ``save_visualization_results`` is then called the way ``evaluate.py:190`` calls it (before ``compute()``, top_k=15) inside a
temporary working directory.  It writes every image's result to the same file, so the dicts are taken from its ``torch.save``
calls; its per-image ``torch.argsort`` results are recorded too, to store the raw grid boxes of the ranked candidates (the
formatter's input) next to the pixel boxes it printed (the formatter's expected output).

Only data is stored: ids, boxes, edge strings, the two name lists, heights and widths - no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_graph_golden.py
"""
import os
import sys
import tempfile

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as MG

NAME, TOP_K = "vg_full_hit", 15
HEIGHTS, WIDTHS = [480, 375, 600], [640, 500, 431]          # non-square on purpose: the reference scales x by height, y by width


def main():
    ref_model, ref_train, ref_eval = MG.import_reference()
    import dataset_utils as ref_names                        # the two name tables (data)
    kw, nobj, seed, gain, cfrac, edge = MG.CASES[NAME]
    cfg = MG.HeadConfig(**kw)
    args = MG.ref_args(cfg)
    sd = MG.make_state_dict(cfg, seed=seed, head_gain=gain)
    batch = MG.make_scene_batch(cfg, nobj, seed=seed, connect_frac=cfrac, edge_boxes=edge)
    gold = dict(np.load(os.path.join(HERE, NAME + ".npz")))
    for b, n in enumerate(nobj):
        for g in range(1, n):
            batch.relationships[b][g - 1] = torch.from_numpy(gold["tgt_rel_%d_%d" % (b, g)])
            batch.subj_or_obj[b][g - 1] = torch.from_numpy(gold["tgt_dir_%d_%d" % (b, g)])
    model = MG.build_ref_model(ref_model, cfg, args, sd)
    masks = MG.ref_masks(batch.bbox, cfg.feature_size)
    relations_target, direction_target = MG.targets(batch, masks)
    Recall = ref_eval.Evaluator(args=args, num_classes=cfg.num_relations, iou_thresh=0.5, top_k=[20, 50, 100])
    Top3 = ref_eval.Evaluator_Top3(args=args, num_classes=cfg.num_relations, iou_thresh=0.5, top_k=[20, 50, 100])
    num_graph_iter = torch.as_tensor([len(m) for m in masks])
    with torch.no_grad():
        for g in range(max(num_graph_iter)):
            keep = torch.nonzero(num_graph_iter > g).view(-1)
            gm = torch.stack([torch.unsqueeze(masks[i][g], dim=0) for i in keep])
            h_graph = torch.cat((batch.image_feature[keep] * gm, batch.image_depth[keep] * gm), dim=1)
            cat_graph = torch.tensor([torch.unsqueeze(batch.categories[i][g], dim=0) for i in keep])
            sp_graph = [batch.super_categories[i][g] for i in keep]
            bb_graph = torch.stack([batch.bbox[i][g] for i in keep])
            for e in range(g):
                em = torch.stack([torch.unsqueeze(masks[i][e], dim=0) for i in keep])
                h_edge = torch.cat((batch.image_feature[keep] * em, batch.image_depth[keep] * em), dim=1)
                cat_edge = torch.tensor([torch.unsqueeze(batch.categories[i][e], dim=0) for i in keep])
                sp_edge = [batch.super_categories[i][e] for i in keep]
                bb_edge = torch.stack([batch.bbox[i][e] for i in keep])
                j_or, j_and = torch.logical_or(gm, em), torch.logical_and(gm, em)
                ratio = (torch.sum(torch.sum(j_or, dim=-1), dim=-1) / torch.sum(torch.sum(j_and, dim=-1), dim=-1)).flatten()
                ratio[torch.isinf(ratio)] = 0
                iou_mask = ratio > 0
                if torch.sum(iou_mask) == 0:
                    continue
                ref_train.evaluate_one_direction(model, args, h_graph, h_edge, cat_graph, cat_edge, sp_graph, sp_edge, bb_graph,
                                                 bb_edge, iou_mask, "cpu", g, e, keep, Recall, Top3, relations_target,
                                                 direction_target, 0, 1, first_direction=True)
                ref_train.evaluate_one_direction(model, args, h_edge, h_graph, cat_edge, cat_graph, sp_edge, sp_graph, bb_edge,
                                                 bb_graph, iou_mask, "cpu", g, e, keep, Recall, Top3, relations_target,
                                                 direction_target, 0, 1, first_direction=False)
    assert np.array_equal(Recall.which_in_batch.numpy(), gold["ev_which_in_batch"])

    saved, ranked = [], []
    real_save, real_argsort = torch.save, torch.argsort

    def spy_save(obj, path, *a, **k):
        saved.append(obj)
        return real_save(obj, path, *a, **k)

    def spy_argsort(*a, **k):
        r = real_argsort(*a, **k)
        ranked.append(r.clone())
        return r

    B = len(nobj)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "results", "visualization_results", "cs"))
        os.chdir(tmp)
        torch.save, torch.argsort = spy_save, spy_argsort
        try:
            Recall.save_visualization_results(["image_%d_annotations.pkl" % b for b in range(B)], [None] * B, HEIGHTS, WIDTHS,
                                              [None] * B, [None] * B, batch.bbox, batch.categories, 0, top_k=TOP_K)
        finally:
            torch.save, torch.argsort = real_save, real_argsort
            os.chdir(cwd)
    images = torch.unique(Recall.which_in_batch).tolist()
    assert len(saved) == len(ranked) == len(images) == B

    out = {"heights": np.asarray(HEIGHTS, dtype=np.int64), "widths": np.asarray(WIDTHS, dtype=np.int64),
           "feature_size": np.asarray([cfg.feature_size], dtype=np.int64), "top_k": np.asarray([TOP_K], dtype=np.int64),
           "image": np.asarray(images, dtype=np.int64)}
    onames, rnames = ref_names.object_class_int2str(), ref_names.relation_by_super_class_int2str()
    out["object_names"] = np.asarray([onames[i] for i in range(len(onames))])
    out["relation_names"] = np.asarray([rnames[i] for i in range(len(rnames))])
    count = np.zeros(B, dtype=np.int64)
    ids = np.full((B, TOP_K, 3), -1, dtype=np.int64)
    raw = np.full((B, TOP_K, 2, 4), -1, dtype=np.float32)
    pix = np.full((B, TOP_K, 2, 4), -1, dtype=np.int64)
    edges = np.full((B, TOP_K), "", dtype="U64")
    for row, (image, vis, order) in enumerate(zip(images, saved, ranked)):
        cur = Recall.which_in_batch == image
        graph = vis["predicted_graph"]
        keep = order[:len(graph)]
        count[row] = len(graph)
        assert vis["height"] == HEIGHTS[image] and vis["width"] == WIDTHS[image]
        sb, ob = Recall.subject_bbox_pred[cur][keep], Recall.object_bbox_pred[cur][keep]
        for r, edge in enumerate(graph):
            ids[row, r] = [edge["subject_id"], edge["relation_id"], edge["object_id"]]
            assert int(Recall.relation_pred[cur][keep[r]]) == edge["relation_id"]
            raw[row, r, 0], raw[row, r, 1] = sb[r].float().numpy(), ob[r].float().numpy()
            pix[row, r, 0], pix[row, r, 1] = edge["bbox_sub"], edge["bbox_obj"]
            edges[row, r] = edge["edge"]
    out.update(count=count, ids=ids, raw_boxes=raw, pixel_boxes=pix, edges=edges)
    np.savez_compressed(os.path.join(HERE, "predicted_graph.npz"), **out)
    print("predicted_graph: images", images, "ranked edges", count.tolist(), "first", edges[0, 0], pix[0, 0].tolist())


if __name__ == "__main__":
    main()
