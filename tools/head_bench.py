#!/usr/bin/env python3
"""Time the plug-and-play BayesianHead (GPU box): warm HIP-event times of forward and forward + backward on the HIP head kernels
(csrc/kernels_head.hip) against a plain f32 torch restatement of the reference module (model.py:24-34: four nn.Linear, log_softmax)
on the same GPU, at M in {4096, 65536} rows and D in {512, 4096} input features.  Prints executed-FLOP fractions of the f32 matrix
peak (157.3 TFLOP/s) and algorithmic-byte fractions of 6.3 TB/s.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`
as a separate command.

With --loss-out it also times one training step with the REAL criterion (the class-weighted hierarchical NLL, train_utils.py:116-157;
30 % of the rows carry no relation) at the same four shapes, in the same process: (a) head(x), the criterion in torch on the connected
rows, backward(); (b) head.hierarchical_nll(x, tgt, cw).backward(), the fused kernels; (c) the torch restatement of the module with
the same criterion - and candidates(h) against forward() + three torch.max.

    python tools/head_bench.py [--out FILE] [--loss-out FILE] [--iters N]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd.model import HEAD_ANY_ROWS, BayesianHead   # noqa: E402

PEAK_F32 = 157.3e12
HBM = 6.3e12
SPLIT, TEMPS = (15, 11, 24), (1.0, 2.0, 0.5)


def torch_head(head, h):
    """The reference module's forward in plain torch f32 (model.py:25-33)."""
    sup = F.log_softmax(F.linear(h, head.fc5.weight, head.fc5.bias), dim=1)
    out = []
    for k, fc in enumerate((head.fc3_1, head.fc3_2, head.fc3_3)):
        out.append(F.log_softmax(F.linear(h, fc.weight, fc.bias) / TEMPS[k], dim=1) + sup[:, k].view(-1, 1))
    return out + [sup]


def torch_criterion(outs, tgt, cw):
    """The reference's criterion in torch (train_utils.py:116-157): the connected rows, NLL of the super category, class-weighted NLL
    of each block that has rows."""
    off = (0, SPLIT[0], SPLIT[0] + SPLIT[1], sum(SPLIT))
    idx = torch.nonzero(tgt >= 0).flatten()
    r1, r2, r3, sup = [o[idx] for o in outs]
    t = tgt[idx]
    st = (t >= off[1]).long() + (t >= off[2]).long()
    loss = F.nll_loss(sup, st)
    for k, r in enumerate((r1, r2, r3)):
        rows = torch.nonzero(st == k).flatten()
        if rows.numel():
            loss = loss + F.nll_loss(r[rows], t[rows] - off[k], weight=cw[off[k]:off[k + 1]])
    return loss


def loss_rows(head, h, x, g, iters):
    """ms of one training step with the real criterion, three ways, and of the candidates, two ways."""
    M = h.shape[0]
    tgt = torch.randint(0, sum(SPLIT), (M,), device="cuda", generator=g)
    tgt = torch.where(torch.rand(M, device="cuda", generator=g) < 0.3, torch.full_like(tgt, -1), tgt)
    cw = torch.rand(sum(SPLIT), device="cuda", generator=g) + 0.5

    def step(loss_fn):
        def run():
            head.zero_grad(set_to_none=True)
            x.grad = None
            loss_fn().backward()
        return run

    def cand_torch():
        with torch.no_grad():
            r1, r2, r3, _ = head(h)
            return [torch.max(r, dim=1) for r in (r1, r2, r3)]

    t_a = timed(step(lambda: torch_criterion(head(x), tgt, cw)), iters)
    t_b = timed(step(lambda: head.hierarchical_nll(x, tgt, cw)), iters)
    t_c = timed(step(lambda: torch_criterion(torch_head(head, x), tgt, cw)), iters)
    t_cf = timed(lambda: head.candidates(h), iters)
    t_ct = timed(cand_torch, iters)
    return "%6d %6d | %9.4f %9.4f %9.4f %7.2f %7.2f | %9.4f %9.4f %7.2f" % (M, h.shape[1], t_a, t_b, t_c, t_a / t_b, t_c / t_b,
                                                                        t_ct, t_cf, t_ct / t_cf)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--loss-out", default=None, help="also time the step with the real criterion and the candidates; table to this file")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "head_bench needs an MI355X"
    lines = ["BayesianHead on %s, f32; ms per call = mean of %d warm calls (HIP events); fractions: executed MFMA FLOP (64 packed "
             "output rows) / 157.3 TFLOP/s, algorithmic bytes / 6.3 TB/s" % (torch.cuda.get_device_name(), args.iters),
             "%6s %6s | %9s %9s %6s %6s | %9s %9s %6s %6s | %7s %7s" % ("M", "D", "fwd ms", "torch ms", "flop", "bytes",
                                                                   "f+b ms", "torch ms", "flop", "bytes", "fwd x", "f+b x")]
    loss_lines = ["BayesianHead training step with the class-weighted hierarchical NLL on %s, f32, 30 %% of the rows without a relation; "
                  "ms per step = mean of %d warm steps (HIP events).  (a) head(x) + the criterion in torch + backward, (b) "
                  "head.hierarchical_nll(x, tgt, cw).backward(), (c) the module and the criterion in torch.  Candidates: forward() + "
                  "three torch.max against candidates(h)." % (torch.cuda.get_device_name(), args.iters),
                  "%6s %6s | %9s %9s %9s %7s %7s | %9s %9s %7s" % ("M", "D", "(a) ms", "(b) ms", "(c) ms", "a / b", "c / b",
                                                               "fwd+max", "cand ms", "x")]
    g = torch.Generator(device="cuda").manual_seed(0)
    for D in (512, 4096):
        torch.manual_seed(1)
        head = BayesianHead(D, *SPLIT, T1=TEMPS[0], T2=TEMPS[1], T3=TEMPS[2]).cuda()
        for M in (4096, 65536):
            h = torch.randn(M, D, device="cuda", generator=g)
            up = [torch.randn(M, c, device="cuda", generator=g) for c in SPLIT + (3,)]
            x = h.clone().requires_grad_(True)

            def fwd_hip():
                with torch.no_grad():
                    head(h)

            def fwd_torch():
                with torch.no_grad():
                    torch_head(head, h)

            def step(fn):
                def run():
                    head.zero_grad(set_to_none=True)
                    x.grad = None
                    sum((o * u).sum() for o, u in zip(fn(head, x), up)).backward()
                return run

            t_f, t_ft = timed(fwd_hip, args.iters), timed(fwd_torch, args.iters)
            t_b = timed(step(lambda m, v: m(v)), args.iters)
            t_bt = timed(step(torch_head), args.iters)
            R = sum(SPLIT) + 3
            flop_f = 2.0 * M * 64 * D
            bytes_f = 4.0 * (M * D + 64 * D + M * R)
            n_part = (M + HEAD_ANY_ROWS - 1) // HEAD_ANY_ROWS
            bytes_b = bytes_f + 4.0 * (2 * M * D + 2 * M * R + 2 * n_part * 64 * (D + 1))
            lines.append("%6d %6d | %9.4f %9.4f %6.3f %6.3f | %9.4f %9.4f %6.3f %6.3f | %7.2f %7.2f" % (
                M, D, t_f, t_ft, flop_f / (t_f * 1e-3) / PEAK_F32, bytes_f / (t_f * 1e-3) / HBM,
                t_b, t_bt, 3 * flop_f / (t_b * 1e-3) / PEAK_F32, bytes_b / (t_b * 1e-3) / HBM, t_ft / t_f, t_bt / t_b))
            if args.loss_out:
                loss_lines.append(loss_rows(head, h, x, g, args.iters))
            del h, x, up
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.loss_out:
        text = "\n".join(loss_lines)
        print(text, flush=True)
        with open(args.loss_out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
