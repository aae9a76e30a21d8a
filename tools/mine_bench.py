#!/usr/bin/env python3
"""Time three ways to the mined commonsense candidates (run_mode prepare_cs, top_k = 10) of one evaluation minibatch (GPU box), on
8 images x 64 objects and on 12 images x 20 objects:

* ``fused``     - ``pair_loop.mine_commonsense_candidates``: fused forward, ``sgc_scene_graph_topk``, ``sgc_related_topk``;
* ``evaluator`` - ``evaluate_minibatch`` into an ``Evaluator``, then its ``related_top_k_device`` (``sgc_topk_per_image`` +
  ``sgc_related_topk``), the device part of ``get_related_top_k_predictions_parallel``;
* ``host loop`` - the same evaluator state copied to the host and scanned by the literal loop of ``tests/mining_cases.py``, which is
  what the reference does (on numpy arrays here; the reference compares device scalars one by one, which is slower still);
* ``forward``   - what all share (flatten, overlap filter, fused forward), to show the part of each behind the forward.

Every route ends with its picks (candidate, rank j per image) on the host; they are compared first.  The routes are run alternately
inside one process (order rotated every round), each timed with a host clock around a device synchronise; medians are reported.

    python tools/mine_bench.py [--rounds 30] [--warmup 5] [--top-k 10]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd.evaluator import Evaluator                                # noqa: E402
from scene_graph_commonsense_amd.model import BayesianRelationClassifier                   # noqa: E402
from scene_graph_commonsense_amd.pair_loop import evaluate_minibatch, mine_commonsense_candidates, overlap_mask  # noqa: E402
from scene_graph_commonsense_amd.pairs import flatten_scene                                # noqa: E402
from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict  # noqa: E402
from tests import mining_cases as MC                                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--top-k", type=int, default=10)
opt = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mine_bench.py measures on the GPU; there is none here")

FX = os.path.join(REPO, "tests", "golden", "ref_fixtures") + os.sep
cfg = HeadConfig()
args = cfg.args(run_mode="prepare_cs", fixtures=FX)
K = opt.top_k
model = BayesianRelationClassifier(args).cuda()
model.load_state_dict(make_state_dict(cfg, seed=0))
model.eval()
print("Commonsense candidate mining on %s (tools/mine_bench.py), top_k = %d; ms per minibatch, host clock around a device synchronise,"
      % (torch.cuda.get_device_name(0), K))
print("routes alternated in one process, median of %d rounds (p10 / p90)" % opt.rounds)


def state_of(ev):
    h = lambda t: t.cpu().numpy()
    return dict(which=h(ev.which_in_batch), conf=h(ev.confidence), pred=h(ev.relation_pred), scat=h(ev.subject_cat_pred),
                ocat=h(ev.object_cat_pred), sbox=h(ev.subject_bbox_pred), obox=h(ev.object_bbox_pred), which_t=h(ev.which_in_batch_target),
                rel_t=h(ev.relation_target), scat_t=h(ev.subject_cat_target), ocat_t=h(ev.object_cat_target),
                sbox_t=h(ev.subject_bbox_target), obox_t=h(ev.object_bbox_target))


for images, objects in ((8, 64), (12, 20)):
    batch = make_scene_batch(cfg, [objects] * images, seed=3, connect_frac=0.02)
    batch.image_feature, batch.image_depth = batch.image_feature.cuda(), batch.image_depth.cuda()

    def fed():
        ev = Evaluator(args, cfg.num_relations, 0.5, [20, 50, 100])
        evaluate_minibatch(model, batch, ev)
        return ev

    def fused():
        m = mine_commonsense_candidates(model, batch, top_k=K)
        return m.count.cpu(), m.pair.cpu(), m.slot.cpu(), m.rank.cpu()

    def evaluator():
        ev = fed()
        _, pos, rank, count, _ = ev.related_top_k_device(K)
        return ev, count.cpu(), pos.cpu(), rank.cpu()

    def host_loop():
        return MC.related_top_k_host(state_of(fed()), K)

    def forward():
        scene = flatten_scene(cfg, batch, "cuda:0")
        return model.forward_pairs(scene, iou_mask=overlap_mask(scene))

    # the three routes pick the same candidates at the same ranks
    ev, count, pos, rank = evaluator()
    want = host_loop()
    f_count, f_pair, f_slot, f_rank = fused()
    conf = ev.confidence.cpu()
    out = model.last_outputs.cand_conf.cpu()
    assert count.tolist() == f_count.tolist() == [len(g) for g in want]
    for r, g in enumerate(want):
        assert list(zip(pos[r, :len(g)].tolist(), rank[r, :len(g)].tolist())) == g and f_rank[r, :len(g)].tolist() == [j for _, j in g]
        assert [float(conf[p]) for p, _ in g] == [float(out[f_pair[r, e], f_slot[r, e]]) for e in range(len(g))]
    routes = [("fused", fused), ("evaluator", evaluator), ("host loop", host_loop), ("forward", forward)]
    times = {name: [] for name, _ in routes}
    for it in range(opt.warmup + opt.rounds):
        for k in range(len(routes)):
            name, fn = routes[(k + it) % len(routes)]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if it >= opt.warmup:
                times[name].append((t1 - t0) * 1e3)
    med = {name: float(np.median(times[name])) for name, _ in routes}
    print("%d images x %d objects (%d ordered pairs, %d candidates, %d connected targets, %d mined edges; equal picks on all routes)"
          % (images, objects, images * objects * (objects - 1), int(conf.numel()), int((ev.relation_target != -1).sum()), int(count.sum())))
    for name, _ in routes:
        t = np.asarray(times[name])
        behind = "" if name == "forward" else "   behind the forward %7.2f" % (med[name] - med["forward"])
        print("    %-10s %8.2f  (%.2f / %.2f)%s" % (name, med[name], np.percentile(t, 10), np.percentile(t, 90), behind))
