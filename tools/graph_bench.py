#!/usr/bin/env python3
"""Time two ways to the ranked top-K triples of one minibatch (GPU box), 8 images x 64 objects, K = 100:

* ``predict``   - ``pair_loop.predict_scene_graphs``: fused forward, then ONE ranking kernel on its outputs (``sgc_scene_graph_topk``);
* ``evaluator`` - the way before that kernel: ``evaluate_minibatch`` into an ``Evaluator`` (appended, permuted, filtered int64 copies)
  plus ``rank_topk_device`` on confidence + connectivity, as ``Evaluator.compute()`` ranks;
* ``forward``   - what both share (flatten, overlap filter, fused forward), to show the post-forward part of each.

The three are run alternately inside one process (order rotated every round), each timed with a host clock around a device
synchronise; the medians are reported with the 10th / 90th percentiles.  The ranked predicates of both routes are compared first.

    python tools/graph_bench.py [--rounds 40] [--warmup 5] [--images 8] [--objects 64] [--top-k 100]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd.evaluator import Evaluator, rank_topk_device          # noqa: E402
from scene_graph_commonsense_amd.model import BayesianRelationClassifier               # noqa: E402
from scene_graph_commonsense_amd.pair_loop import evaluate_minibatch, overlap_mask, predict_scene_graphs  # noqa: E402
from scene_graph_commonsense_amd.pairs import flatten_scene                            # noqa: E402
from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--images", type=int, default=8)
ap.add_argument("--objects", type=int, default=64)
ap.add_argument("--top-k", type=int, default=100)
opt = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("graph_bench.py measures on the GPU; there is none here")

FX = os.path.join(REPO, "tests", "golden", "ref_fixtures") + os.sep
cfg = HeadConfig()
args = cfg.args(fixtures=FX)
K = opt.top_k
model = BayesianRelationClassifier(args).cuda()
model.load_state_dict(make_state_dict(cfg, seed=0))
model.eval()
batch = make_scene_batch(cfg, [opt.objects] * opt.images, seed=3, connect_frac=0.02)
batch.image_feature, batch.image_depth = batch.image_feature.cuda(), batch.image_depth.cuda()


def predict():
    return predict_scene_graphs(model, batch, top_k=K)


def evaluator():
    ev = Evaluator(args, cfg.num_relations, 0.5, [K])
    evaluate_minibatch(model, batch, ev)
    conf, which = ev.confidence + ev.connectivity, ev.which_in_batch
    return ev, which, rank_topk_device(conf, which, K)


def forward():
    scene = flatten_scene(cfg, batch, "cuda:0")
    return model.forward_pairs(scene, iou_mask=overlap_mask(scene))


# same ranked lists (section "when results must not change"): predicates at every rank of every image
g = predict()
ev, which, (images, keep_pos, cnt, _, _, _) = evaluator()
pred = ev.relation_pred
for r, image in enumerate(images.tolist()):
    n = int(cnt[r])
    assert int(g.count[image]) == n
    assert torch.equal(g.predicate[image, :n].long(), pred[keep_pos[r, :n].long()]), image
print("ranked predicates of both routes are equal (%d images, K = %d, %d ordered pairs)" % (len(images), K, opt.images * opt.objects * (opt.objects - 1)))

routes = [("predict", predict), ("evaluator", evaluator), ("forward", forward)]
times = {name: [] for name, _ in routes}
for it in range(opt.warmup + opt.rounds):
    for k in range(len(routes)):
        name, fn = routes[(k + it) % len(routes)]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if it >= opt.warmup:
            times[name].append((t1 - t0) * 1e3)
med = {}
for name, _ in routes:
    t = np.asarray(times[name])
    med[name] = float(np.median(t))
    print("%-9s %7.2f ms per minibatch (median of %d; p10 %.2f, p90 %.2f)" % (name, med[name], len(t), np.percentile(t, 10), np.percentile(t, 90)))
post_p, post_e = med["predict"] - med["forward"], med["evaluator"] - med["forward"]
print("post-forward part: predict %.2f ms, evaluator route %.2f ms (%.1f x)" % (post_p, post_e, post_e / max(post_p, 1e-9)))
