#!/usr/bin/env python3
"""Time the two ways to the SGDET / SGCLS evaluation metrics of one minibatch (GPU box) at 16 images x 36 predicted objects
(BASELINE ``configs[2]``: SGCLS end to end, batch 16):

* ``forward``   - what both share: the batch of the predicted objects, flatten, overlap filter, fused forward;
* ``meter``     - ``pair_loop.score_sgdet_minibatch`` into a ``metrics.RecallMeter`` and nothing else: the ground truth as one target
  table, the counters stay on the device (``sgc_scene_graph_topk``, ``sgc_recall_accumulate_targets``); no ``compute()`` in the timed part;
* ``evaluator`` - ``evaluate_sgdet_minibatch`` into an ``Evaluator``, then ``compute(per_class=True, predcls=False)``, then
  ``clear_data()``: what ``eval_sgd`` / ``eval_sgc`` do per minibatch with ``eval_freq_test: 1``.

The three routes run alternately inside one process after ``--warmup`` untimed rounds, in a freshly shuffled order every round
(seeded).  Each call is timed with a host clock from a device synchronise before it to a device synchronise after it; the evaluator
route also synchronises inside (its read-backs), the meter route only at that final synchronise.  Medians with the 10th / 90th
percentiles; the forward's own p10-p90 spread is printed next to the two distances from it.
The predicted objects are a synthetic minibatch's objects with seeded category confidences; the ground truth is the same objects, and
its relations are drawn from the model's own ranking (per image 12 / 6 / 6 candidates from the ranks below 20 / 50 / 100 and 10 from
anywhere, each with that candidate's predicate), so that hits exist at every K, misses too, and the hit branches of both routes run.
Before timing, the counters of both routes after one minibatch are compared (integers, equal).

    python tools/sgdet_metrics_bench.py [--rounds 40] [--warmup 5] [--out profiles/sgdet_metrics_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd.evaluator import Evaluator                            # noqa: E402
from scene_graph_commonsense_amd.metrics import RecallMeter                            # noqa: E402
from scene_graph_commonsense_amd.model import BayesianRelationClassifier               # noqa: E402
from scene_graph_commonsense_amd.pair_loop import (_scoring_forward, _sgdet_scene, evaluate_sgdet_minibatch, overlap_mask,  # noqa: E402
                                                   pair_cat_confidence, score_sgdet_minibatch)
from scene_graph_commonsense_amd.synthetic import HeadConfig, default_sub2super, make_scene_batch, make_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sgdet_metrics_bench.txt"))
opt = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sgdet_metrics_bench.py measures on the GPU; there is none here")

FX = os.path.join(REPO, "tests", "golden", "ref_fixtures") + os.sep
TOP_K = [20, 50, 100]
SIZES = [36] * 16
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


cfg = HeadConfig()
args = cfg.args(fixtures=FX)
model = BayesianRelationClassifier(args).cuda()
model.load_state_dict(make_state_dict(cfg, seed=0, head_gain=6.0))
model.eval()
batch = make_scene_batch(cfg, SIZES, seed=3, connect_frac=0.0)
feat, depth = batch.image_feature.cuda(), batch.image_depth.cuda()
sub2super = default_sub2super(cfg.num_classes, cfg.num_super_classes)
g = np.random.default_rng(7)
cats = [c.cuda() for c in batch.categories]
confs = [torch.from_numpy(np.log(g.uniform(0.3, 1.0, int(c.numel()))).astype(np.float32)).cuda() for c in batch.categories]
boxes = [b.cuda() for b in batch.bbox]
lists = (cats, confs, boxes)


def draw_targets():
    """One forward over the predicted objects; each image's candidates (pair, slot) ordered by the evaluator's SGDET score (confidence
    + category confidences + log sigmoid connectivity, -inf where the overlap filter drops the pair); the ground-truth relations are 12
    / 6 / 6 candidates from the ranks [0,20) / [20,50) / [50,100) of that order and 10 from anywhere, at most one per unordered pair
    (the first drawn stays), the predicate that of the candidate."""
    _, dev, b, scene = _sgdet_scene(model, feat, depth, cats, boxes, sub2super)
    with torch.no_grad():
        mask = overlap_mask(scene)
        out = model.forward_pairs(scene, iou_mask=mask)
        cc = pair_cat_confidence(scene, confs, "one category confidence per predicted object")
        score = (out.cand_conf.float() + cc.reshape(-1, 1)) + torch.nn.functional.logsigmoid(out.connectivity.float().reshape(-1, 1))
        score = torch.where(mask.reshape(-1, 1) != 0, score, torch.full_like(score, -float("inf"))).cpu().numpy()
    pred, pidx, S = out.cand_pred.cpu().numpy(), scene.pidx, score.shape[1]
    rels, dirs = [], []
    for im, n in enumerate(scene.num_objects):
        rows = np.nonzero(pidx.image == im)[0]
        cand = np.argsort(-score[rows].reshape(-1), kind="stable")
        pick = np.concatenate([g.choice(cand[lo:hi], size=m, replace=False) for lo, hi, m in ((0, 20, 12), (20, 50, 6), (50, 100, 6))]
                              + [g.choice(cand, size=10, replace=False)])
        rel_b = [torch.full((gi,), -1, dtype=torch.int64) for gi in range(1, n)]
        dir_b = [torch.full((gi,), -1.0) for gi in range(1, n)]
        for c in pick:
            k, slot = rows[c // S], c % S
            gi, e = int(pidx.g[k]), int(pidx.e[k])
            if int(rel_b[gi - 1][e]) == -1:
                rel_b[gi - 1][e], dir_b[gi - 1][e] = int(pred[k, slot]), 1.0 if pidx.first[k] else 0.0
        rels.append(rel_b); dirs.append(dir_b)
    return rels, dirs, batch.categories, batch.bbox


targets = draw_targets()
meter = RecallMeter(args, cfg.num_relations, 0.5, TOP_K, device="cuda:0")
ev = Evaluator(args, cfg.num_relations, 0.5, TOP_K)


def forward():
    c, _, b, scene = _sgdet_scene(model, feat, depth, cats, boxes, sub2super)
    return _scoring_forward(model, c, b, scene, overlap_mask(scene), None, None)


def meter_route():
    score_sgdet_minibatch(model, feat, depth, *lists, meter, sub2super=sub2super, targets=targets)


def evaluator_route():
    evaluate_sgdet_minibatch(model, feat, depth, *lists, ev, sub2super=sub2super, targets=targets)
    ev.compute(per_class=True, predcls=False)
    ev.clear_data()


with torch.no_grad():
    meter_route()
    evaluator_route()
    i64 = lambda x: np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x).astype(np.int64)
    view = lambda n: meter.view(n).cpu().numpy()
    for name, sfx in (("recall", ""), ("zero_shot", "_zs")):
        assert (view(name + ".hits") == i64([getattr(ev, "result_dict" + sfx)[k] for k in TOP_K])).all(), name
        assert (view(name + ".hits_pc") == np.stack([i64(getattr(ev, "result_per_class" + sfx)[k]) for k in TOP_K])).all(), name
        assert int(view(name + ".targets")[0]) == int(getattr(ev, "num_connected_target" + sfx)), name
    say("sgcls_16x36: counters of both routes are equal (%d ordered pairs, %d connected targets, hits@20/50/100 %s)"
        % (sum(n * (n - 1) for n in SIZES), int(view("recall.targets")[0]), view("recall.hits").tolist()))
    routes = [("forward", forward), ("meter", meter_route), ("evaluator", evaluator_route)]
    times = {r: [] for r, _ in routes}
    order = np.random.default_rng(0)
    for it in range(opt.warmup + opt.rounds):
        for k in order.permutation(len(routes)):
            route, fn = routes[k]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if it >= opt.warmup:
                times[route].append((t1 - t0) * 1e3)
say("%d timed rounds after %d warm-up rounds, three routes in shuffled order in one process; ms per minibatch, host clock between device synchronises"
    % (opt.rounds, opt.warmup))
med, pct = {}, {}
for route, _ in routes:
    t = np.asarray(times[route])
    med[route], pct[route] = float(np.median(t)), (float(np.percentile(t, 10)), float(np.percentile(t, 90)))
    say("sgcls_16x36 %-9s %7.2f ms (median of %d; p10 %.2f, p90 %.2f)" % (route, med[route], len(t), pct[route][0], pct[route][1]))
pm, pe = med["meter"] - med["forward"], med["evaluator"] - med["forward"]
say("sgcls_16x36 past the forward: meter %+.2f ms, evaluator route %+.2f ms (the forward's own p10-p90 spread: %.2f ms); "
    "meter / forward %.3f, evaluator / forward %.3f"
    % (pm, pe, pct["forward"][1] - pct["forward"][0], med["meter"] / med["forward"], med["evaluator"] / med["forward"]))
say("the meter route is %s to the forward than the evaluator route" % ("closer" if pm < pe else "NOT closer"))
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    f.write("\n".join(lines) + "\n")
