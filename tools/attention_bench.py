#!/usr/bin/env python3
"""Fused head-dim-32 attention (``sgc_mha_fwd``, scene_graph_commonsense_amd/attention.py) against torch's routes, one process, the
routes alternating, median of ``--runs`` synchronised runs after warm-up:

  (a) the attention between the projections on the same projected tensors, f32 and bf16, at the encoder shape (Lq = Lk = 1024, B = 8,
      H = 8) and the decoder cross shape (Lq = 100, Lk = 1024): the kernel; the math of ``F.multi_head_attention_forward`` as detr.py
      reaches it today (need_weights: scores, softmax, head-averaged weights, P V, head-split transposes); and
      ``F.scaled_dot_product_attention``.  Then the whole block (projections included): ``nn.MultiheadAttention`` as detr.py calls it
      against ``attention.mha_forward``.
  (b) ``DETR.encode`` on 8 x 1024^2 with the fused route off / on, f32 and bf16 autocast.
  (c) the full ``DETR.forward`` likewise.

    python tools/attention_bench.py [--runs 20] > profiles/attention_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def alternate(routes, runs, warmup=3):
    """{name: median ms} of the callables in ``routes``, run in turn (a, b, c, a, b, c, ...), each run between two synchronisations."""
    times = {n: [] for n in routes}
    for it in range(warmup + runs):
        for n, fn in routes.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[n].append((time.perf_counter() - t) * 1e3)
    return {n: statistics.median(v) for n, v in times.items()}


def device_ms(fn, n=50):
    """Device time per call of ``n`` back-to-back calls between two events (no host synchronisation inside): what the work costs
    when the launches are hidden behind one another, as inside the extractor."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def mha_math(q, k, v, H, mask):
    """What F.multi_head_attention_forward does between its projections when need_weights keeps its default."""
    Lq, B, E = q.shape
    Lk = k.shape[0]
    hd = E // H
    qh = q.reshape(Lq, B * H, hd).transpose(0, 1)
    kh = k.reshape(Lk, B * H, hd).transpose(0, 1)
    vh = v.reshape(Lk, B * H, hd).transpose(0, 1)
    am = torch.zeros(B, 1, 1, Lk, dtype=q.dtype, device=q.device).masked_fill(mask.view(B, 1, 1, Lk), float("-inf"))
    am = am.expand(B, H, 1, Lk).reshape(B * H, 1, Lk)
    w = torch.softmax(torch.baddbmm(am, qh * hd ** -0.5, kh.transpose(1, 2)), dim=-1)
    out = torch.bmm(w, vh).transpose(0, 1).contiguous().view(Lq, B, E)
    return out, w.view(B, H, Lq, Lk).mean(dim=1)


def sdpa(q, k, v, H, mask):
    Lq, B, E = q.shape
    Lk = k.shape[0]
    sp = lambda t, L: t.reshape(L, B, H, E // H).permute(1, 2, 0, 3)
    o = F.scaled_dot_product_attention(sp(q, Lq), sp(k, Lk), sp(v, Lk), attn_mask=~mask.view(B, 1, 1, Lk))
    return o.permute(2, 0, 1, 3).reshape(Lq, B, E)


def part_a(runs):
    from scene_graph_commonsense_amd.attention import fused_mha, mha_forward
    B, H, E = 8, 8, 256
    block = {}
    print("(a) attention alone on projected tensors, B = 8, H = 8, head dim 32, all-false key padding mask; median ms of %d" % runs)
    for dtype, dn in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        for shape, Lq, Lk in (("encoder", 1024, 1024), ("decoder cross", 100, 1024)):
            torch.manual_seed(0)
            q = torch.randn(Lq, B, E, device="cuda").to(dtype)
            k, v = torch.randn(Lk, B, E, device="cuda").to(dtype), torch.randn(Lk, B, E, device="cuda").to(dtype)
            mask = torch.zeros(B, Lk, dtype=torch.bool, device="cuda")
            routes = {"kernel": lambda: fused_mha(q, k, v, H, mask), "mha math": lambda: mha_math(q, k, v, H, mask)}
            try:
                sdpa(q, k, v, H, mask)
                routes["sdpa"] = lambda: sdpa(q, k, v, H, mask)
            except Exception as e:                                         # a backend torch does not have for this input
                print("    sdpa unavailable: %s" % str(e).splitlines()[0])
            with torch.no_grad():
                r = alternate(routes, runs)
            print("  %-4s %-13s Lq %4d Lk %4d: kernel %7.3f   mha math %7.3f (x%.2f)   sdpa %s" % (
                dn, shape, Lq, Lk, r["kernel"], r["mha math"], r["mha math"] / r["kernel"],
                "%7.3f (x%.2f)" % (r["sdpa"], r["sdpa"] / r["kernel"]) if "sdpa" in r else "   n/a"))
            with torch.no_grad():
                d = {n: device_ms(fn) for n, fn in routes.items()}
            flop = 4.0 * B * H * Lq * Lk * 32
            print("       back to back, device events, ms per call: kernel %7.4f (%.0f TFLOP/s)   mha math %7.4f   sdpa %s" % (
                d["kernel"], flop / d["kernel"] * 1e-9, d["mha math"], "%7.4f" % d["sdpa"] if "sdpa" in d else "   n/a"))
    print("    whole block, projections included: nn.MultiheadAttention as detr.py calls it / attention.mha_forward")
    torch.manual_seed(1)
    mha = nn.MultiheadAttention(E, H).cuda().eval()
    for dn, ac in (("f32", None), ("bf16", torch.bfloat16)):
        for shape, Lq, Lk in (("encoder", 1024, 1024), ("decoder cross", 100, 1024)):
            x, pos = torch.randn(Lk, B, E, device="cuda"), torch.randn(Lk, B, E, device="cuda")
            mask = torch.zeros(B, Lk, dtype=torch.bool, device="cuda")
            kk = x + pos
            qq = kk if Lq == Lk else torch.randn(Lq, B, E, device="cuda")
            with torch.no_grad(), torch.autocast("cuda", dtype=ac, enabled=ac is not None):
                r = alternate({"module": lambda: mha(qq, kk, value=x, key_padding_mask=mask)[0],
                               "fused": lambda: mha_forward(mha, qq, kk, x, mask)}, runs)
            block[(dn, shape)] = r
            print("  %-4s %-13s Lq %4d Lk %4d: module %7.3f   mha_forward %7.3f (x%.2f)" % (dn, shape, Lq, Lk, r["module"], r["fused"],
                                                                                         r["module"] / r["fused"]))
    return block


def part_bc(runs, block):
    from scene_graph_commonsense_amd.detr import DETR
    torch.manual_seed(0)
    m = DETR(151).cuda().eval()
    x = torch.randn(8, 3, 1024, 1024, device="cuda")
    print("(b) DETR.encode and (c) DETR.forward, 8 x 1024^2, random weights; median ms of %d" % runs)
    for dn, ac, fmt in (("f32", None, torch.contiguous_format), ("bf16", torch.bfloat16, torch.channels_last)):
        mm = m.to(memory_format=fmt)
        xx = x.contiguous(memory_format=fmt)
        r = alternate({"off": lambda: mm.encode(xx, autocast=ac, fused_attention=False),
                       "on": lambda: mm.encode(xx, autocast=ac, fused_attention=True)}, runs)
        share = 6 * block[(dn, "encoder")]["module"] / r["off"]
        print("  %-4s encode : unfused %7.2f   fused %7.2f (x%.3f)   6 unfused attention blocks = %.2f ms = %.1f %% of the unfused encode" % (
            dn, r["off"], r["on"], r["off"] / r["on"], 6 * block[(dn, "encoder")]["module"], 100 * share))

        def fwd(flag):
            mm.set_fused_attention(flag)
            with torch.no_grad(), torch.autocast("cuda", dtype=ac, enabled=ac is not None):
                mm(xx)
        r = alternate({"off": lambda: fwd(False), "on": lambda: fwd(True)}, runs)
        mm.set_fused_attention(False)
        print("  %-4s forward: unfused %7.2f   fused %7.2f (x%.3f)" % (dn, r["off"], r["on"], r["off"] / r["on"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    runs = max(20, a.runs)
    print("tools/attention_bench.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    block = part_a(runs)
    part_bc(runs, block)


if __name__ == "__main__":
    main()
