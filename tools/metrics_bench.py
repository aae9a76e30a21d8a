#!/usr/bin/env python3
"""Time the two ways to the evaluation metrics of one minibatch (GPU box), at 8 images x 64 objects (Visual Genome head) and
4 images x 100 objects (OpenImages head):

* ``forward``   - what both share: flatten, overlap filter, fused forward;
* ``meter``     - ``pair_loop.score_minibatch`` into a ``metrics.RecallMeter`` and nothing else: the counters stay on the device
  (``sgc_scene_graph_topk``, ``sgc_recall_accumulate``, ``sgc_precision_accumulate``); no ``compute*()`` in the timed part;
* ``evaluator`` - ``evaluate_minibatch`` into ``Evaluator`` / ``Evaluator_Top3``, then ``compute(per_class=True)`` and
  ``Evaluator_Top3.compute`` (Visual Genome) or ``compute_precision`` (OpenImages), then ``clear_data()``: what the drivers do per
  minibatch with ``eval_freq_test: 1``.

All six (three routes, two sizes) run alternately inside one process after ``--warmup`` untimed rounds, in a freshly shuffled order
every round (seeded): a route that always ran behind the evaluator route's host loops would start on an idle device every time.
Each call is timed with a host clock from a device synchronise before it to a device synchronise after it; the evaluator route also
synchronises inside (its read-backs), the meter route only at that final synchronise.  Medians with the 10th / 90th percentiles.
The targets are drawn from the model's own ranking (``targets_from_ranking``: per image 12 / 6 / 6 candidates from the ranks below
20 / 50 / 100 and 10 from anywhere, each with that candidate's predicate), so that hits exist at every K, misses too, and the hit
branches of both routes run.
Before timing, the counters of both routes after one minibatch are compared (integers, equal).

    python tools/metrics_bench.py [--rounds 40] [--warmup 5] [--out profiles/metrics_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd.evaluator import Evaluator, Evaluator_Top3           # noqa: E402
from scene_graph_commonsense_amd.metrics import RecallMeter                           # noqa: E402
from scene_graph_commonsense_amd.model import BayesianRelationClassifier              # noqa: E402
from scene_graph_commonsense_amd.pair_loop import evaluate_minibatch, overlap_mask, score_minibatch  # noqa: E402
from scene_graph_commonsense_amd.pairs import flatten_scene                           # noqa: E402
from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics_bench.txt"))
opt = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("metrics_bench.py measures on the GPU; there is none here")

FX = os.path.join(REPO, "tests", "golden", "ref_fixtures") + os.sep
TOP_K = [20, 50, 100]
OIV6 = dict(dataset="oiv6", num_classes=601, num_super_classes=0, num_geometric=4, num_possessive=2, num_semantic=24)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def targets_from_ranking(model, cfg, batch, seed):
    """Replace the batch's relation targets: one forward, each image's candidates (pair, slot) ordered by the evaluator's score
    (confidence + log sigmoid connectivity, -inf where the overlap filter drops the pair); targets are 12 / 6 / 6 candidates from
    the ranks [0,20) / [20,50) / [50,100) of that order and 10 from anywhere, at most one per unordered pair (the first drawn
    stays), the predicate that of the candidate."""
    scene = flatten_scene(cfg, batch, "cuda:0")
    with torch.no_grad():
        mask = overlap_mask(scene)
        out = model.forward_pairs(scene, iou_mask=mask)
        score = out.cand_conf.float() + torch.nn.functional.logsigmoid(out.connectivity.float().reshape(-1, 1))
        score = torch.where(mask.reshape(-1, 1) != 0, score, torch.full_like(score, -float("inf"))).cpu().numpy()
    pred, pidx, g, S = out.cand_pred.cpu().numpy(), scene.pidx, np.random.default_rng(seed), score.shape[1]
    rels, dirs = [], []
    for b, n in enumerate(scene.num_objects):
        rows = np.nonzero(pidx.image == b)[0]
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
    batch.relationships, batch.subj_or_obj = rels, dirs


class Case:
    def __init__(self, name, cfg, sizes, seed):
        self.name, self.cfg, self.vg = name, cfg, cfg.dataset == "vg"
        self.args = cfg.args(fixtures=FX)
        self.model = BayesianRelationClassifier(self.args, num_classes=cfg.num_classes, num_super_classes=cfg.num_super_classes,
                                                num_geometric=cfg.num_geometric, num_possessive=cfg.num_possessive,
                                                num_semantic=cfg.num_semantic).cuda()
        self.model.load_state_dict(make_state_dict(cfg, seed=seed, head_gain=6.0))
        self.model.eval()
        self.batch = make_scene_batch(cfg, sizes, seed=3, connect_frac=0.02)
        self.batch.image_feature, self.batch.image_depth = self.batch.image_feature.cuda(), self.batch.image_depth.cuda()
        targets_from_ranking(self.model, cfg, self.batch, seed + 7)
        self.pairs = sum(n * (n - 1) for n in sizes)
        self.meter = RecallMeter(self.args, cfg.num_relations, 0.5, TOP_K, device="cuda:0")
        self.ev = Evaluator(self.args, cfg.num_relations, 0.5, TOP_K)
        self.t3 = Evaluator_Top3(self.args, cfg.num_relations, 0.5, TOP_K) if self.vg else None

    def forward(self):
        scene = flatten_scene(self.cfg, self.batch, "cuda:0")
        return self.model.forward_pairs(scene, iou_mask=overlap_mask(scene))

    def meter_route(self):
        score_minibatch(self.model, self.batch, self.meter)

    def evaluator_route(self):
        evaluate_minibatch(self.model, self.batch, self.ev, self.t3)
        self.ev.compute(per_class=True)
        if self.vg:
            self.t3.compute(per_class=True)
            self.t3.clear_data()
        else:
            self.ev.compute_precision()
        self.ev.clear_data()

    def check(self):
        """One minibatch through both routes from zero: every counter equal as integers."""
        self.meter_route()
        self.evaluator_route()
        i64 = lambda x: np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x).astype(np.int64)
        view = lambda n: self.meter.view(n).cpu().numpy()
        pairs = [("recall", self.ev, "")] + ([("zero_shot", self.ev, "_zs"), ("top3", self.t3, "")] if self.vg else [])
        for name, e, sfx in pairs:
            assert (view(name + ".hits") == i64([getattr(e, "result_dict" + sfx)[k] for k in TOP_K])).all(), name
            assert (view(name + ".hits_pc") == np.stack([i64(getattr(e, "result_per_class" + sfx)[k]) for k in TOP_K])).all(), name
            assert int(view(name + ".targets")[0]) == int(getattr(e, "num_connected_target" + sfx)), name
        if not self.vg:
            for part, attr in (("ap", "result_per_class_ap"), ("ap_union", "result_per_class_ap_union"), ("num_ap", "num_conn_target_per_class_ap")):
                assert (view("precision." + part) == i64(getattr(self.ev, attr))).all(), part
        say("%s: counters of both routes are equal (%d ordered pairs, %d connected targets, hits@20/50/100 %s%s)"
            % (self.name, self.pairs, int(view("recall.targets")[0]), view("recall.hits").tolist(),
               "" if self.vg else "; precision ap / ap_union / num_ap sums %d / %d / %d"
               % tuple(int(view("precision." + p).sum()) for p in ("ap", "ap_union", "num_ap"))))


cases = [Case("vg_8x64", HeadConfig(), [64] * 8, 0), Case("oiv6_4x100", HeadConfig(**OIV6), [100] * 4, 1)]
for c in cases:
    c.check()
routes = [(c.name, r, getattr(c, fn)) for c in cases for r, fn in (("forward", "forward"), ("meter", "meter_route"), ("evaluator", "evaluator_route"))]
times = {(n, r): [] for n, r, _ in routes}
order = np.random.default_rng(0)
for it in range(opt.warmup + opt.rounds):
    for k in order.permutation(len(routes)):
        name, route, fn = routes[k]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if it >= opt.warmup:
            times[(name, route)].append((t1 - t0) * 1e3)
say("%d timed rounds after %d warm-up rounds, six routes in shuffled order in one process; ms per minibatch, host clock between device synchronises"
    % (opt.rounds, opt.warmup))
for c in cases:
    med = {}
    for route in ("forward", "meter", "evaluator"):
        t = np.asarray(times[(c.name, route)])
        med[route] = float(np.median(t))
        say("%-11s %-9s %7.2f ms (median of %d; p10 %.2f, p90 %.2f)" % (c.name, route, med[route], len(t), np.percentile(t, 10), np.percentile(t, 90)))
    pm, pe = med["meter"] - med["forward"], med["evaluator"] - med["forward"]
    say("%-11s past the forward: meter %+.2f ms, evaluator route %+.2f ms; meter / forward %.3f, evaluator / forward %.3f"
        % (c.name, pm, pe, med["meter"] / med["forward"], med["evaluator"] / med["forward"]))
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    f.write("\n".join(lines) + "\n")
