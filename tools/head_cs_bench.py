#!/usr/bin/env python3
"""Time one training step of the plug-and-play BayesianHead in run_mode train_cs (GPU box): the class-weighted hierarchical NLL plus
the commonsense penalty of train_utils.py:36-60, at M in {4096, 65536} rows and D in {512, 4096} input features, about 30 % of the rows
without a relation, random triplet sets of 60 % aligned / 10 % violated density over 150 x 50 x 150.  Three routes, three repeats in
one process with the routes alternated (a, b, c, a, b, c, ...), each repeat the mean of --iters warm steps between HIP events:

    (a) head.hierarchical_nll(x, tgt, cw).backward()                                   today's step without commonsense: the floor
    (b) head.hierarchical_nll(x, tgt, cw, commonsense=..., ...).backward()              the fused kernels
    (c) head(x), the criterion and the penalty in torch, backward()                    the unfused device route: softmax, max and
        arg-max per block, lookups in an unpacked bool [C, R, C] tensor

Acceptance: (b) is below (c) at every shape by more than the spread (max - min over the repeats) of both.  (b) - (a) is printed next to
the extra bytes the fused design moves (the penalty direction written and read once, the flags, the categories, the bitmaps).

    python tools/head_cs_bench.py [--out FILE] [--iters N]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from head_bench import SPLIT, TEMPS, timed, torch_criterion                          # noqa: E402
from scene_graph_commonsense_amd.commonsense import TripletBitmaps                   # noqa: E402
from scene_graph_commonsense_amd.model import BayesianHead                           # noqa: E402

C, R = 150, sum(SPLIT)
OFF = (0, SPLIT[0], SPLIT[0] + SPLIT[1])
LAM, LAM_WEAK, LAM_STRONG = 1.0, 0.1, 10.0
REPEATS = 3


def torch_penalty(outs, sc, oc, aligned, violated):
    """train_utils.py:36-60 on the device: the reference's host lookups become gathers in two bool [C, R, C] tensors."""
    probs, preds = [], []
    for k, r in enumerate(outs[:3]):
        p, a = torch.max(F.softmax(r, dim=1), dim=1)
        probs.append(p)
        preds.append(a + OFF[k])
    probs, preds = torch.hstack(probs), torch.hstack(preds)
    s, o = sc.repeat(3), oc.repeat(3)
    weak, strong = ~aligned[s, preds, o], violated[s, preds, o]
    loss = 0.0
    if probs[weak].numel() > 0:
        loss = loss + LAM_WEAK * probs[weak].mean()
    if probs[strong].numel() > 0:
        loss = loss + LAM_STRONG * probs[strong].mean()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "head_cs_bench needs an MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    aligned = torch.rand(C, R, C, device="cuda", generator=g) < 0.6
    violated = torch.rand(C, R, C, device="cuda", generator=g) < 0.1
    bm = TripletBitmaps.from_masks(aligned, violated, "cuda")
    lines = ["BayesianHead training step in run_mode train_cs on %s, f32, 30 %% of the rows without a relation, sets of 60 %% / 10 %% "
             "density; ms per step, %d repeats (routes alternated) of the mean of %d warm steps (HIP events).  (a) hierarchical_nll "
             "without commonsense, (b) the fused call with commonsense, (c) head(x) + the criterion + the penalty in torch.  spread = "
             "max - min over the repeats; margin = mean (c) - mean (b) - both spreads (> 0 required); extra = bytes (b) moves beyond "
             "(a): dir [M,64] f32 written and read, flags [M,3], two int64 category tables, two bitmaps."
             % (torch.cuda.get_device_name(), REPEATS, args.iters),
             "%6s %5s | %-26s | %-26s | %-26s | %7s %7s %7s | %8s %9s %8s" % (
                 "M", "D", "(a) ms x3", "(b) ms x3", "(c) ms x3", "c / b", "b / a", "margin", "b - a ms", "extra MB", "GB/s")]
    ok = True
    for D in (512, 4096):
        torch.manual_seed(1)
        head = BayesianHead(D, *SPLIT, T1=TEMPS[0], T2=TEMPS[1], T3=TEMPS[2]).cuda()
        for M in (4096, 65536):
            h = torch.randn(M, D, device="cuda", generator=g)
            x = h.clone().requires_grad_(True)
            tgt = torch.randint(0, R, (M,), device="cuda", generator=g)
            tgt = torch.where(torch.rand(M, device="cuda", generator=g) < 0.3, torch.full_like(tgt, -1), tgt)
            cw = torch.rand(R, device="cuda", generator=g) + 0.5
            sc = torch.randint(0, C, (M,), device="cuda", generator=g)
            oc = torch.randint(0, C, (M,), device="cuda", generator=g)

            def step(loss_fn):
                def run():
                    head.zero_grad(set_to_none=True)
                    x.grad = None
                    loss_fn().backward()
                return run

            def unfused():
                outs = head(x)
                return torch_criterion(outs, tgt, cw) + LAM * torch_penalty(outs, sc, oc, aligned, violated)

            routes = (step(lambda: head.hierarchical_nll(x, tgt, cw)),
                      step(lambda: head.hierarchical_nll(x, tgt, cw, commonsense=bm, subject_cat=sc, object_cat=oc,
                                                         lambda_commonsense=LAM, lambda_cs_weak=LAM_WEAK, lambda_cs_strong=LAM_STRONG)),
                      step(unfused))
            t = [[], [], []]
            for _ in range(REPEATS):
                for r, fn in enumerate(routes):
                    t[r].append(timed(fn, args.iters))
            mean = [sum(v) / len(v) for v in t]
            spread = [max(v) - min(v) for v in t]
            margin = mean[2] - mean[1] - spread[1] - spread[2]
            ok = ok and margin > 0
            extra = 2 * 4.0 * M * 64 + 2 * 3.0 * M + 2 * 8.0 * M + 2 * 4.0 * ((C * R * C + 31) // 32)
            d = mean[1] - mean[0]
            lines.append("%6d %5d | %-26s | %-26s | %-26s | %7.2f %7.2f %7.4f | %8.4f %9.2f %8s" % (
                M, D, " ".join("%.4f" % v for v in t[0]), " ".join("%.4f" % v for v in t[1]), " ".join("%.4f" % v for v in t[2]),
                mean[2] / mean[1], mean[1] / mean[0], margin, d, extra / 1e6, "%.0f" % (extra / (d * 1e-3) / 1e9) if d > 0 else "-"))
            del h, x
    lines.append("acceptance ((b) below (c) by more than both spreads at every shape): %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
