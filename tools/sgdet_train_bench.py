#!/usr/bin/env python3
"""Time what training on detected objects adds to a training step (GPU box) at 16 images x 36 detections, the shape of
``tools/sgdet_metrics_bench.py`` (20 160 ordered pairs), with the ground truth drawn as that tool draws it (34 candidates per image
from the model's own ranking, at most one relation per unordered pair):

* ``assign``      - (a) ``pair_loop.assign_sgdet_targets`` alone on a scene and a target table that are already on the device
  (``sgc_assign_pair_targets``: one memset and two launches);
* ``host_assign`` - (b) what a user would write without it: the same assignment in vectorised numpy on the host (per image, one pass
  of array operations per target row over all pairs of the image, exact integer cross-multiplication; the host pair index and the
  normalised boxes are precomputed outside the timed part, in the host route's favour) plus the upload of directed / raw;
* ``step_free``   - (c) ``train_minibatch`` on the detected scene with ``directed`` / ``raw_target`` precomputed on the device: the
  step with "targets for free" (the scene of the detections is built inside the timed part, as in the next route);
* ``step_sgdet``  - (c) ``train_sgdet_minibatch``: target table built on the host and uploaded, assignment, the same step;
* ``loop_free`` / ``loop_sgdet`` - the same two steps as a training loop runs them: ``LOOP`` steps back to back with no synchronise
  between them (host work of step k+1 - the target table among it - overlaps the device's work on step k), time per step.

The routes run alternately inside one process after ``--warmup`` untimed rounds, in a freshly shuffled order every round (seeded).
Each call is timed with a host clock from a device synchronise before it to a device synchronise after it.  Medians with the 10th /
90th percentiles.  Before timing, the host route's result and the device's are compared (integers, equal), and the two steps' losses.

    python tools/sgdet_train_bench.py [--rounds 40] [--warmup 5] [--out profiles/sgdet_train_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd.evaluator import _equiv_matrix                        # noqa: E402
from scene_graph_commonsense_amd.model import BayesianRelationClassifier               # noqa: E402
from scene_graph_commonsense_amd.optim import FusedSGD                                 # noqa: E402
from scene_graph_commonsense_amd.pair_loop import (_sgdet_scene, assign_sgdet_targets, overlap_mask, pair_cat_confidence,  # noqa: E402
                                                   train_minibatch, train_sgdet_minibatch, upload_sgdet_targets)
from scene_graph_commonsense_amd.pairs import normalise_boxes, sg_target_ptr, sg_target_table       # noqa: E402
from scene_graph_commonsense_amd.synthetic import HeadConfig, default_sub2super, make_scene_batch, make_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sgdet_train_bench.txt"))
opt = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sgdet_train_bench.py measures on the GPU; there is none here")

FX = os.path.join(REPO, "tests", "golden", "ref_fixtures") + os.sep
SIZES = [36] * 16
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


cfg = HeadConfig()
args = cfg.args(fixtures=FX)
model = BayesianRelationClassifier(args).cuda()
model.load_state_dict(make_state_dict(cfg, seed=0, head_gain=6.0))
batch = make_scene_batch(cfg, SIZES, seed=3, connect_frac=0.0)
feat, depth = batch.image_feature.cuda(), batch.image_depth.cuda()
sub2super = default_sub2super(cfg.num_classes, cfg.num_super_classes)
g = np.random.default_rng(7)
cats = [c.cuda() for c in batch.categories]
confs = [torch.from_numpy(np.log(g.uniform(0.3, 1.0, int(c.numel()))).astype(np.float32)).cuda() for c in batch.categories]
boxes = [b.cuda() for b in batch.bbox]


def draw_targets():
    """``tools/sgdet_metrics_bench.py``'s ground truth: one forward over the detections; per image 12 / 6 / 6 candidates from the ranks
    [0,20) / [20,50) / [50,100) of the evaluator's SGDET score and 10 from anywhere, at most one per unordered pair, the predicate that
    of the candidate."""
    model.eval()
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
model.train()
opt_sgd = FusedSGD(model.parameters(), lr=1e-12, momentum=0.9, weight_decay=1e-4)     # the timed steps update, and stay finite
R, F, B = cfg.num_relations, cfg.feature_size, len(SIZES)
dev = feat.device

# what both assignment routes start from: the detected scene on the device, the table on the host
_, _, det_batch, scene0 = _sgdet_scene(model, feat, depth, cats, boxes, sub2super)
table_np = sg_target_table(*targets, drop_last_graph_object=False)
table_d = upload_sgdet_targets(table_np, B, dev)
pidx0 = scene0.pidx
n_obj = int(sum(SIZES))
det_cats = torch.cat([c.cpu() for c in batch.categories]).numpy()
det_box = normalise_boxes(torch.cat([b.cpu().float() for b in batch.bbox]), F).astype(np.int64)
EQ = _equiv_matrix()


def _inter_union(a, b):
    """a [n,4], b [m,4] normalised (x0,x1,y0,y1) -> (intersection, union) [m,n] int64 cell counts."""
    area = lambda x: np.maximum(x[:, 1] - x[:, 0], 0) * np.maximum(x[:, 3] - x[:, 2], 0)
    iw = np.maximum(np.minimum(a[None, :, 1], b[:, None, 1]) - np.maximum(a[None, :, 0], b[:, None, 0]), 0)
    ih = np.maximum(np.minimum(a[None, :, 3], b[:, None, 3]) - np.maximum(a[None, :, 2], b[:, None, 2]), 0)
    inter = np.where((area(a)[None, :] > 0) & (area(b)[:, None] > 0), iw * ih, 0)
    return inter, area(a)[None, :] + area(b)[:, None] - inter


def host_assign(thr=0.5):
    """The assignment in vectorised numpy + the upload of its result (directed, raw)."""
    t_image, t_rel, t_scat, t_ocat, t_sbox, t_obox = table_np
    t_ptr = sg_target_ptr(t_image, B)
    tsb, tob = normalise_boxes(torch.from_numpy(t_sbox), F).astype(np.int64), normalise_boxes(torch.from_numpy(t_obox), F).astype(np.int64)
    P = pidx0.n_pairs
    directed, matched = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    hit = np.zeros(len(t_rel), np.int32)
    for b in range(B):
        r0, r1 = int(t_ptr[b]), int(t_ptr[b + 1])
        pr = np.nonzero(pidx0.image == b)[0]
        if r1 == r0 or pr.size == 0:
            continue
        s, o = pidx0.sub[pr], pidx0.obj[pr]
        rows = slice(r0, r1)
        lab = (((t_scat[rows, None] == det_cats[None, s]) | EQ[t_scat[rows]][:, det_cats[s]])
               & ((t_ocat[rows, None] == det_cats[None, o]) | EQ[t_ocat[rows]][:, det_cats[o]]))
        i_s, u_s = _inter_union(det_box[s], tsb[rows])
        i_o, u_o = _inter_union(det_box[o], tob[rows])
        ok = lab & ((t_rel[rows] >= 0) & (t_rel[rows] < R))[:, None]
        ok &= (np.where(u_s > 0, i_s / np.maximum(u_s, 1), 0.0) >= thr) & (np.where(u_o > 0, i_o / np.maximum(u_o, 1), 0.0) >= thr)
        hit[rows] = ok.any(axis=1)
        num, den = i_s * i_o, u_s * u_o
        best, bn, bd = np.full(pr.size, -1, np.int64), np.zeros(pr.size, np.int64), np.zeros(pr.size, np.int64)
        for t in range(r1 - r0):                                             # ascending rows, strictly better only: smallest row on a tie
            better = ok[t] & ((best < 0) | (num[t] * bd > bn * den[t]))
            best, bn, bd = np.where(better, r0 + t, best), np.where(better, num[t], bn), np.where(better, den[t], bd)
        matched[pr] = best
        directed[pr] = np.where(best >= 0, t_rel[np.maximum(best, 0)], -1)
    where = np.full(n_obj * n_obj, -1, np.int64)
    where[pidx0.sub.astype(np.int64) * n_obj + pidx0.obj] = np.arange(P)
    rev = where[pidx0.obj.astype(np.int64) * n_obj + pidx0.sub]
    raw = np.where(directed >= 0, directed, directed[rev]).astype(np.int32)
    return torch.from_numpy(directed).to(dev), torch.from_numpy(raw).to(dev), matched, hit


def device_assign():
    return assign_sgdet_targets(scene0, table_d, num_relations=R, feature_size=F)


ref = device_assign()
hd, hr, hm, hh = host_assign()
assert torch.equal(hd, ref.directed) and torch.equal(hr, ref.raw), "host and device assignment differ"
assert (hm == ref.matched.cpu().numpy()).all() and (hh == ref.target_hit.cpu().numpy()).all(), "host and device assignment differ"
counts = ref.counts().tolist()
say("sgdet_train_16x36: host (numpy) and device assignment are equal: %d ordered pairs, %d target rows, %d rows hit, %d pairs assigned"
    % (scene0.n_pairs, counts[0], counts[1], counts[2]))
directed0, raw0 = ref.directed.clone(), ref.raw.clone()


def step_free(optimizer=opt_sgd):
    _, _, b, scene = _sgdet_scene(model, feat, depth, cats, boxes, sub2super)
    scene.directed, scene.raw_target = directed0, raw0
    return train_minibatch(model, b, optimizer, scene=scene)


def step_sgdet(optimizer=opt_sgd):
    return train_sgdet_minibatch(model, feat, depth, cats, boxes, targets, optimizer=optimizer, sub2super=sub2super)


model.eval()                                    # dropout off and no update: the two steps see the same weights and must agree exactly
la, lb = float(step_free(None)), float(step_sgdet(None))
model.zero_grad(set_to_none=True)
model.train()
say("sgdet_train_16x36: loss of the step with precomputed targets %.6f, of train_sgdet_minibatch %.6f (eval mode, no update between them)" % (la, lb))
assert la == lb, (la, lb)

LOOP = 6


def loop_of(fn):
    def run():
        for _ in range(LOOP):
            fn()
    return run


routes = [("assign", device_assign), ("host_assign", host_assign), ("step_free", step_free), ("step_sgdet", step_sgdet),
          ("loop_free", loop_of(step_free)), ("loop_sgdet", loop_of(step_sgdet))]
times = {r: [] for r, _ in routes}
order = np.random.default_rng(0)
for it in range(opt.warmup + opt.rounds):
    for k in order.permutation(len(routes)):
        route, fn = routes[k]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if it >= opt.warmup:
            times[route].append((t1 - t0) * 1e3 / (LOOP if route.startswith("loop_") else 1))
say("%d timed rounds after %d warm-up rounds, six routes in shuffled order in one process; ms per call (per step for the loops of %d), host clock between device synchronises"
    % (opt.rounds, opt.warmup, LOOP))
med, pct = {}, {}
for route, _ in routes:
    t = np.asarray(times[route])
    med[route], pct[route] = float(np.median(t)), (float(np.percentile(t, 10)), float(np.percentile(t, 90)))
    say("sgdet_train_16x36 %-11s %9.3f ms (median of %d; p10 %.3f, p90 %.3f)" % (route, med[route], len(t), pct[route][0], pct[route][1]))
spread = pct["step_free"][1] - pct["step_free"][0]
say("sgdet_train_16x36 (a) assignment alone %.3f ms; (b) numpy assignment + upload %.3f ms (%.0f x the device call); (c) train_sgdet_minibatch "
    "%+.3f ms past the step with precomputed targets (that step's own p10-p90 spread: %.3f ms), ratio %.4f"
    % (med["assign"], med["host_assign"], med["host_assign"] / med["assign"], med["step_sgdet"] - med["step_free"], spread,
       med["step_sgdet"] / med["step_free"]))
lspread = pct["loop_free"][1] - pct["loop_free"][0]
say("sgdet_train_16x36 back to back: train_sgdet_minibatch %+.3f ms per step past the step with precomputed targets (%.3f against %.3f ms; "
    "that loop's own p10-p90 spread: %.3f ms), ratio %.4f"
    % (med["loop_sgdet"] - med["loop_free"], med["loop_sgdet"], med["loop_free"], lspread, med["loop_sgdet"] / med["loop_free"]))
say("the assignment launch %s inside the step's spread; the whole entry (host table + upload + assignment) %s for a single synchronised step "
    "and %s back to back"
    % ("disappears" if med["assign"] <= spread else "does NOT disappear",
       "does too" if med["step_sgdet"] - med["step_free"] <= spread else "does not",
       "does" if med["loop_sgdet"] - med["loop_free"] <= lspread else "does not"))
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    f.write("\n".join(lines) + "\n")
