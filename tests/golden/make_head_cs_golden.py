#!/usr/bin/env python3
"""Commonsense goldens of the plug-and-play ``BayesianHead`` from the REAL reference (build container only; needs the reference): for
the cases of tests/head_cs_cases.py the reference's ``BayesianHead`` (model.py:9-34) sits behind a stub classifier that the
reference's own ``train_one_direction`` calls in run_mode ``train_cs`` (train_utils.py:36-60); stored are its ``loss_commonsense``, the
gradients of that penalty (dh and the weights as L2 norm plus a fixed sample of entries, the biases whole), the numbers of weak and
strong candidates, and ``confidence`` / ``relation_pred`` of the reference's ``Evaluator.accumulate`` in run_mode ``eval_cs``
(evaluator.py:160-194) on the same outputs.  The triplet sets are the seeded ones of the cases, given to the reference as the dicts
it looks tuples up in.  Only data is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_head_cs_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                      # noqa: E402  (stubs + reference import helpers of the main generator)

import numpy as np                           # noqa: E402
import torch                                 # noqa: E402

sys.path.insert(0, G.REPO)
from scene_graph_commonsense_amd.synthetic import HeadConfig                              # noqa: E402
from tests.head_cs_cases import GAP_TOL, cs_case, flags, top2_gaps                         # noqa: E402
from tests.head_train_cases import CASES, SPLIT, TEMPS, sample                            # noqa: E402


class Stub(torch.nn.Module):
    """The reference classifier's call form (model.py:185) around the plug-and-play head: features in, the head's four outputs,
    a constant connectivity and hidden state."""

    def __init__(self, head):
        super().__init__()
        self.head = head

    def forward(self, h_sub, h_obj, cat_sub, cat_obj, spcat_sub, spcat_obj, rank, h_sub_aug=None, h_obj_aug=None):
        r1, r2, r3, sup = self.head(h_sub)
        zero = torch.zeros(h_sub.shape[0], 1)
        return r1, r2, r3, sup, zero, zero, zero


def _store(out, key, t, whole):
    t = t.detach()
    if whole:
        out[key] = t.numpy().copy()
    else:
        out[key + "__l2"] = np.array([float(t.double().norm())])
        out[key + "__sample"] = sample(t).numpy().copy()


def _dict(mask):
    return {tuple(k): 1 for k in torch.nonzero(mask).tolist()}


def main():
    ref_model, ref_train, ref_eval = G.import_reference()
    cfg = HeadConfig()
    assert (cfg.num_geometric, cfg.num_possessive, cfg.num_semantic) == SPLIT
    out = {}
    for name, (D, M, _) in CASES.items():
        h, sd, tgt, cw, sc, oc, aligned, violated = cs_case(name)
        head = ref_model.BayesianHead(input_dim=D, num_geometric=SPLIT[0], num_possessive=SPLIT[1], num_semantic=SPLIT[2],
                                      T1=TEMPS[0], T2=TEMPS[1], T3=TEMPS[2])
        head.load_state_dict(sd)
        al, vi = _dict(aligned), _dict(violated)

        # the properties the tests rely on, from float64
        pred64, gap, big = top2_gaps(h, list(head.parameters()))
        assert float(gap.min()) > GAP_TOL * big, (name, float(gap.min()), big)
        weak, strong = flags(pred64, sc, oc, aligned, violated)
        assert int(weak.sum()) >= 5 and int(strong.sum()) >= 5 and int((weak & strong).sum()) >= 1
        assert int(((sc < 0) | (sc >= aligned.shape[0]) | (oc < 0) | (oc >= aligned.shape[0])).sum()) >= 1

        targs = G.ref_args(cfg)
        targs["training"]["run_mode"] = "train_cs"
        targs["training"]["eval_freq"] = 10 ** 9
        crit = [torch.nn.NLLLoss(weight=cw[:SPLIT[0]]), torch.nn.NLLLoss(weight=cw[SPLIT[0]:SPLIT[0] + SPLIT[1]]),
                torch.nn.NLLLoss(weight=cw[SPLIT[0] + SPLIT[1]:]), torch.nn.NLLLoss()]
        keep = torch.zeros(M, dtype=torch.long)
        bbox = torch.zeros(M, 4)
        iou_mask = torch.ones(M, dtype=torch.bool)
        sp = [[0]] * M
        x = h.clone().requires_grad_(True)
        head.zero_grad()
        # one direction-step (graph_iter 1, edge_iter 0) whose rows are all connected; the call form of make_golden.py:366
        r = ref_train.train_one_direction(Stub(head), targs, x, x, sc, oc, sp, sp, bbox, bbox, x, x, iou_mask, "cpu", 1, 0, keep,
                                          None, None, crit, torch.nn.BCEWithLogitsLoss(), [[tgt]], [[torch.ones(M)]], 1, [[]], [[]],
                                          al, vi, 10 ** 6, first_direction=True)
        pen = r[2]
        pen.backward()
        out[name + "__penalty"] = np.array([float(pen.detach())])
        out[name + "__counts"] = np.array([int(weak.sum()), int(strong.sum())], dtype=np.int64)
        _store(out, name + "__dh", x.grad, False)
        for pn, p in head.named_parameters():
            _store(out, "%s__d_%s" % (name, pn.replace(".", "_")), p.grad, pn.endswith("bias"))

        eargs = G.ref_args(cfg)
        eargs["training"]["run_mode"] = "eval_cs"
        ev = ref_eval.Evaluator(args=eargs, num_classes=cfg.num_relations, iou_thresh=0.5, top_k=[20, 50, 100])
        ev.commonsense_aligned_triplets, ev.commonsense_violated_triplets = al, vi
        with torch.no_grad():
            r1, r2, r3, sup = head(h)
            ev.accumulate(keep, torch.cat((r1, r2, r3), dim=1), tgt, sup, torch.zeros(M), sc, oc, sc, oc, bbox, bbox, bbox, bbox,
                          iou_mask)
        out[name + "__ev_confidence"] = ev.confidence.numpy().copy()            # [3M]: the three blocks one after the other
        out[name + "__ev_relation_pred"] = ev.relation_pred.numpy().copy()
        # the reference's own counts agree with the float64 flags (its arg-max is the float64 one at these gaps)
        assert np.array_equal(out[name + "__ev_relation_pred"], pred64.T.reshape(-1).numpy())
        assert int(np.isneginf(out[name + "__ev_confidence"]).sum()) == int((weak | strong).sum())
        print(name, "penalty", float(pen), "N_w", int(weak.sum()), "N_s", int(strong.sum()), "both", int((weak & strong).sum()),
              "min gap", float(gap.min()), "bar", GAP_TOL * big)
    path = os.path.join(HERE, "head_cs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
