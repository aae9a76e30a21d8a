#!/usr/bin/env python3
"""Generate tests/golden/mined_candidates.npz by running the REAL reference's commonsense candidate mining
(``Evaluator.get_related_top_k_predictions_parallel``, ``evaluator.py:375-462``) and its triplet bookkeeping
(``VisualGenomeDataset.accumulate_triplets`` / ``save_all_triplets``, ``dataloader.py:168-244``).

Runs only in the build container (needs /root/reference), with the stubs and helpers of ``make_golden.py``.  The eval loop of
``evaluate.py`` is restated around the reference's own ``evaluate_one_direction`` / ``Evaluator`` as ``make_graph_golden.py`` does,
on three images of a full-size model with the overlap filter on.  ``query_llm.batch_query_openai_gpt`` is replaced by a
deterministic judge (aligned when the CRC-32 of the string is even) and ``torch.save`` is recorded.  The mining method is called
BEFORE ``compute()`` (as ``evaluate.py:200`` does), once with top_k=10 and once with top_k=30.  The dataloader's two methods are
called unbound on a plain namespace, with stub modules for the dataloader's unused imports.

Only data is stored: the per-step evaluator inputs (they rebuild the state through ``Evaluator.accumulate``), the flat state, the
strings, edges, saved lists and paths, the three triplet dictionaries and the two name tables - no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mining_golden.py
"""
import os
import sys
import tempfile
import types
import zlib

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as MG

NOBJ, SEED, GAIN, CONNECT = (8, 7, 6), 27, 6.0, 0.45
TOP_KS = (10, 30)
MAX_EDGES = 16


def crc_judge(predicted_edges, edge_cache, batch_size=4, cache_hits=0, **kw):
    return [1 if zlib.crc32(s.encode()) % 2 == 0 else 0 for s in predicted_edges], cache_hits


def main():
    for name in ("requests", "PIL", "PIL.Image", "tqdm"):
        try:
            __import__(name)
        except Exception:
            MG._stub(name)
    if not hasattr(sys.modules["PIL"], "Image"):
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    ref_model, ref_train, ref_eval = MG.import_reference()
    import dataset_utils as ref_names
    cfg = MG.HeadConfig()
    args = MG.ref_args(cfg)
    args["training"]["run_mode"] = "prepare_cs"
    args["training"]["eval_mode"] = "pc"
    args["models"]["llm_model"] = "gpt3.5"
    sd = MG.make_state_dict(cfg, seed=SEED, head_gain=GAIN)
    batch = MG.make_scene_batch(cfg, NOBJ, seed=SEED, connect_frac=CONNECT)
    model = MG.build_ref_model(ref_model, cfg, args, sd)
    masks = MG.ref_masks(batch.bbox, cfg.feature_size)
    relations_target, direction_target = MG.targets(batch, masks)
    Recall = ref_eval.Evaluator(args=args, num_classes=cfg.num_relations, iou_thresh=0.5, top_k=[20, 50, 100])

    steps = []

    class NoTop3:
        def accumulate(self, *a, **k):
            pass

    class Feed:                                           # records what evaluate_one_direction hands to Evaluator.accumulate
        def accumulate(self, *a, **k):
            steps.append([x.detach().clone() if torch.is_tensor(x) else x for x in a])
            Recall.accumulate(*a, **k)

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
                                                 bb_edge, iou_mask, "cpu", g, e, keep, Feed(), NoTop3(), relations_target,
                                                 direction_target, 0, 1, first_direction=True)
                ref_train.evaluate_one_direction(model, args, h_edge, h_graph, cat_edge, cat_graph, sp_edge, sp_graph, bb_edge,
                                                 bb_graph, iou_mask, "cpu", g, e, keep, Feed(), NoTop3(), relations_target,
                                                 direction_target, 0, 1, first_direction=False)

    B = len(NOBJ)
    images = torch.unique(Recall.which_in_batch).tolist()
    assert images == list(range(B))
    onames, rnames = ref_names.object_class_int2str(), ref_names.relation_by_super_class_int2str()
    out = {"object_names": np.asarray([onames[i] for i in range(len(onames))]),
           "relation_names": np.asarray([rnames[i] for i in range(len(rnames))]),
           "num_objects": np.asarray(NOBJ, dtype=np.int64), "top_ks": np.asarray(TOP_KS, dtype=np.int64)}
    cat = lambda k: torch.cat([s[k] for s in steps]).numpy()
    out.update(step_sizes=np.asarray([len(s[0]) for s in steps], dtype=np.int64), step_which=cat(0).astype(np.int64),
               step_relation=cat(1).astype(np.float32), step_target=cat(2).astype(np.int64), step_conn=cat(4).astype(np.float32),
               step_scat=cat(5).astype(np.int64), step_ocat=cat(6).astype(np.int64), step_sbox=cat(9).astype(np.float32),
               step_obox=cat(10).astype(np.float32), step_iou=cat(13).astype(np.bool_))
    for s in steps:                                       # targets are the step's own objects (train_utils.py:190-191)
        assert torch.equal(s[5], s[7]) and torch.equal(s[6], s[8]) and torch.equal(s[9], s[11]) and torch.equal(s[10], s[12])
    assert np.array_equal(cat(9), cat(9).astype(np.float32)) and Recall.confidence.dtype == torch.float32
    ref_state = dict(which=Recall.which_in_batch, conf=Recall.confidence, pred=Recall.relation_pred, scat=Recall.subject_cat_pred,
                     ocat=Recall.object_cat_pred, sbox=Recall.subject_bbox_pred, obox=Recall.object_bbox_pred,
                     which_t=Recall.which_in_batch_target, rel_t=Recall.relation_target, scat_t=Recall.subject_cat_target,
                     ocat_t=Recall.object_cat_target, sbox_t=Recall.subject_bbox_target, obox_t=Recall.object_bbox_target)
    for k, v in ref_state.items():
        v = v.clone().numpy()
        out["ref_" + k] = v.astype(np.float32) if k in ("conf", "sbox", "obox", "sbox_t", "obox_t") else v.astype(np.int64)
    # no two confidences inside any image's top-30 window are equal: the reference's unstable argsort cannot matter
    for image in images:
        c = np.sort(out["ref_conf"][out["ref_which"] == image])[::-1][:max(TOP_KS) + 1]
        assert len(c) > max(TOP_KS) and np.isfinite(c).all() and (np.diff(c) < 0).all(), (image, c)

    annot = ["image_%d_annotations.pkl" % b for b in range(B)]
    Recall.load_annotation_paths(annot)
    ref_eval.batch_query_openai_gpt = crc_judge           # `from query_llm import *` bound the name in the evaluator module
    real_save = torch.save
    runs, dup_skips = {}, 0
    with tempfile.TemporaryDirectory() as tmp:
        args["dataset"]["annot_dir"] = tmp
        for top_k in TOP_KS:
            saved = {}
            torch.save = lambda obj, path, *a, **k: saved.__setitem__(os.path.relpath(path, tmp), obj)
            try:
                preds, graphs, pct = Recall.get_related_top_k_predictions_parallel(top_k=top_k)
            finally:
                torch.save = real_save
            assert pct == 0 and len(preds) == len(graphs) == B
            runs[top_k] = (preds, graphs, saved)
    counts = {k: [len(g) for g in runs[k][1]] for k in TOP_KS}
    assert max(max(c) for c in counts.values()) >= 10 and min(min(c) for c in counts.values()) < 10, counts
    assert max(max(c) for c in counts.values()) < MAX_EDGES

    for top_k, (preds, graphs, saved) in runs.items():
        tag = "k%d_" % top_k
        cnt = np.asarray([len(g) for g in graphs], dtype=np.int64)
        strings = np.full((B, MAX_EDGES), "", dtype="U64")
        sbox, obox = np.full((B, MAX_EDGES, 4), -1, dtype=np.float32), np.full((B, MAX_EDGES, 4), -1, dtype=np.float32)
        rel, rank = np.full((B, MAX_EDGES), -1, dtype=np.int64), np.full((B, MAX_EDGES), -1, dtype=np.int64)
        conf = np.full((B, MAX_EDGES), np.nan, dtype=np.float32)
        for r, (p, g) in enumerate(zip(preds, graphs)):
            assert len(p) == len(g) and len(set(p)) == len(p)
            for e, (s, edge) in enumerate(zip(p, g)):
                strings[r, e], sbox[r, e], rel[r, e], obox[r, e], rank[r, e] = s, edge[0], edge[1], edge[2], edge[4]
                conf[r, e] = edge[3]
                assert float(conf[r, e]) == edge[3]        # the confidence is an f32 value
        paths = sorted(saved)
        assert len(paths) == 2 * int((cnt > 0).sum())
        saved_row, saved_edges = [], np.full((len(paths), MAX_EDGES), -1, dtype=np.int64)
        for i, path in enumerate(paths):
            row = int(os.path.basename(path).split("_")[1])
            saved_row.append(row)
            for e, edge in enumerate(saved[path]):
                saved_edges[i, e] = graphs[row].index(edge)
        out.update({tag + "count": cnt, tag + "strings": strings, tag + "sbox": sbox, tag + "obox": obox, tag + "rel": rel,
                    tag + "rank": rank, tag + "conf": conf, tag + "saved_paths": np.asarray(paths),
                    tag + "saved_row": np.asarray(saved_row, dtype=np.int64), tag + "saved_edges": saved_edges})

    # a duplicate triple was skipped: the literal loop, counting the candidates that matched but were already in the list
    sys.path.insert(0, os.path.dirname(HERE))
    import mining_cases as MC
    st = {k: out["ref_" + k] for k in MC.STATE_KEYS}
    names = (out["object_names"].tolist(), out["relation_names"].tolist())
    for top_k in TOP_KS:
        stats = {}
        picks = MC.related_top_k_host(st, top_k, names, stats)
        dup_skips += stats.get("duplicates", 0)
        got = MC.lists_from_picks(st, picks, names)
        assert got[0] == runs[top_k][0], "the host loop of tests/mining_cases.py differs from the reference"
    assert dup_skips > 0

    # ---------------------------------------------------------------- step 2: dataloader.py:168-244 on the top-10 files
    import dataloader as ref_loader
    ns = types.SimpleNamespace(args=args, triplets_train_gt={}, triplets_train_pseudo={}, commonsense_aligned_triplets={},
                               commonsense_violated_triplets={})
    saved10 = runs[10][2]
    for b in range(B):
        stem = "image_%d_pseudo_annotations.pkl" % b
        yes = saved10.get(os.path.join("cs_aligned_top10_gpt3p5_temp", stem))
        no = saved10.get(os.path.join("cs_violated_top10_gpt3p5_temp", stem))
        if yes is None or no is None:
            continue
        ref_loader.VisualGenomeDataset.accumulate_triplets(ns, batch.categories[b], batch.relationships[b], batch.subj_or_obj[b],
                                                           batch.bbox[b], yes, no)
    written = {}
    torch.save = lambda obj, path, *a, **k: written.__setitem__(path, dict(obj))
    try:
        ref_loader.VisualGenomeDataset.save_all_triplets(ns)
    finally:
        torch.save = real_save
    assert sorted(written) == ["triplets/commonsense_aligned_triplets_gpt3p5_temp.pt", "triplets/commonsense_violated_triplets_gpt3p5_temp.pt"]
    table = lambda d: np.asarray([[k[0], k[1], k[2], v] for k, v in d.items()], dtype=np.int64).reshape(-1, 4)
    out.update(trip_gt=table(ns.triplets_train_gt), trip_aligned=table(written["triplets/commonsense_aligned_triplets_gpt3p5_temp.pt"]),
               trip_violated=table(written["triplets/commonsense_violated_triplets_gpt3p5_temp.pt"]))
    assert len(out["trip_gt"]) > 0 and len(out["trip_aligned"]) > len(out["trip_gt"]) and len(out["trip_violated"]) > 0
    for b in range(B):
        out["cats_%d" % b] = batch.categories[b].numpy().astype(np.int64)
        out["bbox_%d" % b] = batch.bbox[b].numpy().astype(np.float32)
        out["tri_rel_%d" % b] = torch.cat([r.reshape(-1) for r in batch.relationships[b]]).numpy().astype(np.int64)
        out["tri_dir_%d" % b] = torch.cat([r.reshape(-1) for r in batch.subj_or_obj[b]]).numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "mined_candidates.npz"), **out)
    print("mined_candidates: edges per image", counts, "duplicate skips", dup_skips, "triplets gt/aligned/violated",
          len(out["trip_gt"]), len(out["trip_aligned"]), len(out["trip_violated"]))


if __name__ == "__main__":
    main()
