#!/usr/bin/env python3
"""Time the plug-and-play BayesianHead (GPU box): warm HIP-event times of forward and forward + backward on the HIP head kernels
(csrc/kernels_head.hip) against a plain f32 torch restatement of the reference module (model.py:24-34: four nn.Linear, log_softmax)
on the same GPU, at M in {4096, 65536} rows and D in {512, 4096} input features.  Prints executed-FLOP fractions of the f32 matrix
peak (157.3 TFLOP/s) and algorithmic-byte fractions of 6.3 TB/s.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`
as a separate command.

    python tools/head_bench.py [--out FILE] [--iters N]
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
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "head_bench needs an MI355X"
    lines = ["BayesianHead on %s, f32; ms per call = mean of %d warm calls (HIP events); fractions: executed MFMA FLOP (64 packed "
             "output rows) / 157.3 TFLOP/s, algorithmic bytes / 6.3 TB/s" % (torch.cuda.get_device_name(), args.iters),
             "%6s %6s | %9s %9s %6s %6s | %9s %9s %6s %6s | %7s %7s" % ("M", "D", "fwd ms", "torch ms", "flop", "bytes",
                                                                   "f+b ms", "torch ms", "flop", "bytes", "fwd x", "f+b x")]
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
            del h, x, up
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
