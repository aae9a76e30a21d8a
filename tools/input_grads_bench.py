#!/usr/bin/env python3
"""Time the input gradient of the relation head (GPU box).

(a) ``sgc_conv1_dgrad`` at n_img = 8 (8192 x 257 x 256, both roles, feature + depth outputs) against a torch restatement on the same
    bf16 operands: ``torch.matmul`` of the concatenated roles (bf16 result) + ONE copy kernel that permutes and casts to NCHW f32 (the
    concatenation of the roles is prepared outside the timed window).  HIP events around windows of back-to-back calls after warm-up
    (20000 calls: 0.3 - 0.5 s per window), the two alternated, median window.  The calls of a window reuse the same 12.8 MB, so this is
    a WARM figure - operands and outputs stay in the caches, as ``dpre1`` does in the step, where the kernel that wrote it has just run;
    the bytes-over-time figure is therefore no HBM rate.
(b) one training step (``pair_loop.train_minibatch`` with ``optim.FusedSGD``, training mode) at 8 images x 64 objects with the switch
    off and on, alternated step by step in one process; host clock around a device synchronise; median of ``--steps`` steps each.

    python tools/input_grads_bench.py [--out profiles/input_grads_bench.txt] [--steps 24] [--no-step]
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scene_graph_commonsense_amd import _lib   # noqa: E402

N_IMG, HW, CP = 8, 1024, 288


def window_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def kernel_rows(calls=20000, windows=5):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    n_pix = N_IMG * HW
    dp = [torch.randn(n_pix, 128, device="cuda", generator=g).to(torch.bfloat16) for _ in (0, 1)]
    wt = torch.zeros(2, CP, 128, device="cuda", dtype=torch.bfloat16)
    wt[:, :257] = (torch.randn(2, 257, 128, device="cuda", generator=g) / 16).to(torch.bfloat16)
    feat = torch.empty(N_IMG, 256, HW, device="cuda")
    depth = torch.empty(N_IMG, 1, HW, device="cuda")
    dcat = torch.cat(dp, dim=1).contiguous()                                   # [n_pix, 256]
    wcat = torch.cat([wt[0, :257].t(), wt[1, :257].t()], dim=0).contiguous()   # [256, 257]
    out_t = torch.empty(N_IMG, 257, HW, device="cuda")
    st = _lib.stream_ptr()

    def hip():
        _lib.check(lib.sgc_conv1_dgrad(_lib.ptr(dp[0]), _lib.ptr(wt[0]), _lib.ptr(dp[1]), _lib.ptr(wt[1]), _lib.ptr(feat), 256, _lib.ptr(depth), 1,
                                       N_IMG, HW, 0, st), "sgc_conv1_dgrad")

    def restated():
        out_t.copy_(torch.matmul(dcat, wcat).view(N_IMG, HW, 257).permute(0, 2, 1))

    for fn in (hip, restated):
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    t_hip, t_torch = [], []
    for _ in range(windows):                                                   # alternated windows of back-to-back calls
        t_hip.append(window_us(hip, calls))
        t_torch.append(window_us(restated, calls))
    diff = float((torch.cat([feat, depth], dim=1) - out_t).abs().max() / out_t.abs().max())
    moved = 2 * n_pix * 128 * 2 + 2 * CP * 128 * 2 + n_pix * 257 * 4
    m_hip, m_torch = statistics.median(t_hip), statistics.median(t_torch)
    return ["(a) sgc_conv1_dgrad, n_img = 8 (8192 x 257 x 256, %.1f MB moved), WARM (every call on the same buffers: cache-resident): median of %d "
            "alternated windows of %d back-to-back calls, HIP events"
            % (moved / 1e6, windows, calls),
            "    HIP kernel          %8.2f us per call  (windows %s)" % (m_hip, " ".join("%.2f" % t for t in t_hip)),
            "    torch restatement   %8.2f us per call  (windows %s)" % (m_torch, " ".join("%.2f" % t for t in t_torch)),
            "    torch / HIP = %.2f; algorithmic bytes / time = %.2f TB/s (warm caches: not an HBM rate); max |difference| / max |value| = %.1e (the restatement rounds the product to bf16)"
            % (m_torch / m_hip, moved / (m_hip * 1e-6) / 1e12, diff)], m_hip <= m_torch


def step_rows(steps):
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    from scene_graph_commonsense_amd.optim import FusedSGD
    from scene_graph_commonsense_amd.pair_loop import freeze_setup_objects, train_minibatch
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    model = BayesianRelationClassifier(cfg.args()).cuda()
    model.load_state_dict(make_state_dict(cfg, seed=0))
    model.train()
    opt = FusedSGD(model.parameters(), lr=1e-9, momentum=0.9, weight_decay=1e-4)      # small: the weights stay where the gradients mean something
    batch = make_scene_batch(cfg, [64] * 8, seed=1000, connect_frac=0.02)
    freeze_setup_objects()

    loss = [None]

    def step(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss[0] = train_minibatch(model, batch, opt, input_grads=on)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(4):
        step(False)
        step(True)
    t = {False: [], True: []}
    for _ in range(steps):                                                     # alternated step by step
        for on in (False, True):
            t[on].append(step(on))
    g = model.last_input_grads["image_feature"]
    off, on = statistics.median(t[False]), statistics.median(t[True])
    spread = lambda v: "min %.2f, quartiles %.2f / %.2f, max %.2f" % (min(v), statistics.quantiles(v, n=4)[0], statistics.quantiles(v, n=4)[2], max(v))
    return ["(b) training step, 8 images x 64 objects (32256 ordered pairs), training mode, FusedSGD; alternated, median of %d steps each; host clock "
            "around a device synchronise" % steps,
            "    input_grads off     %8.2f ms  (%s)" % (off, spread(t[False])),
            "    input_grads on      %8.2f ms  (%s)" % (on, spread(t[True])),
            "    difference %+.3f ms (%+.2f %%); last step: loss %.4e, |d loss / d image_feature| max = %.3e"
            % (on - off, 100 * (on - off) / off, float(loss[0]), float(g.abs().max()))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "input_grads_bench.txt"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--no-step", action="store_true", help="only the kernel comparison")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "input_grads_bench needs an MI355X"
    assert args.steps >= 20
    lines = ["Input gradient of the relation head on %s (tools/input_grads_bench.py)" % torch.cuda.get_device_name()]
    rows, ok = kernel_rows()
    lines += rows
    if not args.no_step:
        lines += step_rows(args.steps)
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if not ok:
        sys.exit("condition missed: the HIP kernel is slower than the torch restatement")


if __name__ == "__main__":
    main()
