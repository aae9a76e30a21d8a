#!/usr/bin/env python3
"""Benchmark of the pairwise relation head on MI355X: ordered object-pairs/sec, forward + backward.

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one minibatch of synthetic input already resident in HBM, from the RAW
minibatch (the reference's data contract: features, depth, ragged boxes / categories / relation targets): pair
enumeration and targets (row a2), per-image conv1, per-object conv2 halves, pair expansion, conv3, fc1, fc2, Bayesian
head, hierarchical loss, full backward, (N>1: RCCL gradient all-reduce), SGD-momentum update of the f32 master weights
and re-derivation of the 16-bit compute copies.  8 images x 64 objects per GPU -> 32 256 ordered pairs per GPU and
step.  Weak scaling: every rank owns 8 images.  Rank 0 prints ONE JSON line.

A plain run does only what that line's headline needs: set-up, W warm-up steps, K timed steps, the line (``metric``, ``value``,
``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step`` = wall time of the K timed steps / K).  ``--full`` adds everything else
the benchmark measures: per-kernel HIP-event timers in the timed steps, the roofline / HBM records, one single-stream pass for the
backward's kernel times, the box-size sensitivity sweep, the pass with every sharing identity off and the CPU-oracle baseline.
``--dump-outputs DIR`` writes what the timed path handed its caller in the last timed step (``write_outputs``).

Multi-GPU: one process per GPU.  Under ``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`` the ranks
come from the environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*; the reference spawns them with ``mp.spawn``,
``main.py:103,112-123``).  Called directly with ``--gpus N`` (N > 1) this file is its own launcher: the parent starts N
child ranks BEFORE it touches the GPU, waits for them and exits with the worst of their codes.  ``--gpus`` must equal
the world size, otherwise the run is refused (no silent single-rank numbers).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

MFMA_PEAK_TFLOPS = 2500.0      # dense bf16/f16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
CPU_BASELINE_THREADS = 32      # fastest single-process setting on the GPU box's 256 host threads (profiles/r04_oracle_threads.txt: 8 / 32 / 128 threads = 20 / 30 / 11 pairs/s)
# conv3 forward over the pair-specific windows: f16 implicit 3x3 GEMM whose rows are gathered from the window list, ReLU + max-pool
# epilogue (gemm_nt_pp_kernel<ELEM, EPI_POOL, ABL, ACG = 1>: the ping-pong block with gathered conv rows).  With conv3 AND fc1
# computed over shared windows (csrc/kernels_shared.hip) the three GEMMs over those windows are the longest launches of the step
# (forward / data gradient / weight gradient, 7.4 / 7.9 / 8.3 ms); the forward one is reported here, the others are in kernels_ms.
# The three GEMMs over the convolved windows are the longest launches of the step.  key of engine.timers -> (rocprofv3 kernel names,
# newest first, what the launch is).  ``roofline`` reports the LONGEST of them (backward durations from a single-stream pass of the
# same step: on two streams HIP-event intervals of overlapping launches are not kernel times), ``roofline_kernels`` all three.
WINDOW_GEMMS = {
    "conv3_fwd_windows": (("gemm_nt_pp_kernel<0, 3, 0, 1, 0>", "gemm_nt_pp_kernel<0, 3, 0, 1>"),
                          "gemm_nt_pp_kernel<f16,relu+pool,conv-gather> (sgc_conv3_relu_pool_windows_wm: conv3 forward over the listed windows)"),
    "conv3_dgrad_windows": (("gemm_nt_sp_kernel", "gemm_nt_pp_kernel<1, 0, 0, 0, 1>"),
                            "gemm_nt_sp_kernel (sgc_windows_dgrad_patches_sparse: conv3 data gradient of the real pairs' listed windows in patch "
                            "form on the sparse matrix cores; executed = issued multiply-adds, 20 of the dense form's 36 per window)"),
    "conv3_wgrad_windows": (("gemm_tn_sp_kernel<2>", "gemm_tn_sp_kernel<1>"),
                            "gemm_tn_sp_kernel<gather> (sgc_windows_wgrad_gather_sparse: conv3 weight gradient of the real pairs' listed windows, "
                            "2:4-sparse un-pooled gradient x 4x4 input patches gathered from the forward's f16 maps, K ranges per XCD; "
                            "executed = non-zero multiply-adds only)"),
}
PMC_TAGS = ("r06_final", "r05_final7", "r05_final6", "r05_final5", "r05_final3", "r05_final2", "r05_final", "r05_mid", "r04_final5", "r04_final4", "r04_final3", "r04_final2", "r04_final", "r03_final6")   # newest committed profile sets first


BENCH_LR_SCALE = 1e-3
# the fields of a plain run's line (without --full)
PLAIN_FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "loss", "loss_first_step", "host", "backward_streams", "image_group_lanes", "peak_memory_gb", "ranks_seen",
                "rank_ms_per_step", "dp_mode", "exposed_comm_ms")
DUMP_SAMPLE = 1 << 21          # --dump-outputs: larger tensors are written as this many elements at fixed seeded positions


def usable_cpus():
    """Host threads this process may really use: ``os.cpu_count()`` counts the whole machine, a job is often given fewer
    (affinity mask, cgroup CPU quota, OMP_NUM_THREADS set by whoever started it)."""
    n = os.cpu_count() or 8
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    try:
        n = min(n, int(os.environ.get("OMP_NUM_THREADS", "") or n))
    except ValueError:
        pass
    return max(1, n)


def write_outputs(out_dir, loss, outputs, model):
    """``--dump-outputs``: what a caller of the timed path holds after its last timed step, one ``<name>.npy`` per array - ``loss``
    (float64 [1]), the step's pair outputs ``out_<field>`` (``PairOutputs``: relation log-probs, super-relation, connectivity, fc2
    hidden, candidate scores / predicates) and, unless ``--forward-only``, every parameter after the update (``param_<name>``), all
    float32, in their own shapes.  A tensor of more than DUMP_SAMPLE elements is written as DUMP_SAMPLE elements of its flattened form
    at sorted positions drawn from a generator seeded by its name, the same in every run: two builds compare output for output
    (about 45 MB in all at the default workload)."""
    import zlib
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrays = []
    if loss is not None:
        arrays.append(("loss", torch.tensor([float(loss)], dtype=torch.float64)))
    if outputs is not None:
        for f in ("relation", "super_relation", "connectivity", "hidden", "cand_conf", "cand_pred"):
            t = getattr(outputs, f, None)
            if t is not None:
                arrays.append(("out_" + f, t))
    if model is not None:
        arrays += [("param_" + n, p) for n, p in model.named_parameters()]
    total = 0
    for name, t in arrays:
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            t = t.flatten()
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(t.numel(), DUMP_SAMPLE, replace=False))
            t = t[torch.from_numpy(idx).to(t.device)]
        a = (t.double() if t.dtype == torch.float64 else t.float()).cpu().numpy()
        total += a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)
    assert total <= 64 << 20, "dumped outputs exceed 64 MB: %d bytes" % total


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--objects", type=int, default=64)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--cached-scene", action="store_true",
                    help="flatten the minibatch and build the targets once, outside the timed loop (round-1 behaviour; A/B only)")
    ap.add_argument("--torch-sgd", action="store_true", help="torch.optim.SGD instead of the one-pass optim.FusedSGD (same update)")
    ap.add_argument("--dataset", default="vg", choices=["vg", "oiv6"], help="oiv6 = 601 classes, (4,2,24) head, no super-classes")
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
    ap.add_argument("--dp-mode", default="sharded", choices=["sharded", "allreduce"],
                    help="N > 1: reduce-scatter + sharded SGD + all-gather (distributed.ShardedSGD, default) or all-reduce + full SGD on every rank")
    ap.add_argument("--streams", type=int, default=None,
                    help="image-group lanes on concurrent HIP streams inside one step (pair_loop.train_minibatch; default: the model's setting)")
    ap.add_argument("--no-sensitivity", action="store_true", help="skip the three short box-size sensitivity runs (N=1 only)")
    ap.add_argument("--box-scale", type=float, default=1.0,
                    help="scale every box about its centre (clipped to the image); >= 100 = every box is the full image")
    ap.add_argument("--box-dist", default="survey", choices=["survey", "vg03", "vg06", "vg12"],
                    help="survey: SURVEY 8d's boxes (the benchmark); vgNN: raw boxes with ASSUMED VG-like marginals (median area NN %% of the "
                         "image) through the reference's own box pipeline (synthetic.vg_like_boxes, tools/vg_box_statistic.py)")
    ap.add_argument("--full", action="store_true",
                    help="also the per-kernel timers, roofline / HBM records, single-stream pass, box-size sensitivity, identity-off pass "
                         "and CPU baseline (a plain run: set-up, warm-up, timed steps, the headline line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps: the last timed step's loss, pair outputs and updated parameters as DIR/<name>.npy "
                         "(float32 / float64; tensors above 2^21 elements as a fixed seeded sample)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / reduction plumbing only, no GPU work (the CPU test of the N-rank launch uses it with gloo)")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------ launcher
def launch_ranks(args, argv):
    """Start ``args.gpus`` child ranks of this script (one per GPU) and wait.  Runs before anything in this process has
    initialised the GPU; children are fresh interpreters, never an exec of this one."""
    if not args.dry_run and os.environ.get("SGC_BENCH_SHARE_GPU") != "1":
        import torch
        have = torch.cuda.device_count()                     # counting devices does not initialise the runtime
        if have < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible" % (args.gpus, have))
    with socket.socket() as sk:                              # a rendezvous port the OS knows to be free right now
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    code = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                rc = p.poll()
                if rc is None:
                    continue
                pending.remove(p)
                if rc != 0:                                  # one rank died: the others would wait in a collective forever
                    code = code or rc
                    for q in pending:
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return code


# ------------------------------------------------------------------------------------------------ measurement helpers
def state_plan_total(eng):
    """Length of the window list of the last step (X windows of the real pairs + the windows the pseudo-pairs compute themselves)."""
    t = getattr(eng, "_xw_total", None)
    return None if t is None else int(t[0])


def pmc_traffic(names):
    """(bytes per launch, rocprof average ms per launch, profile tag) of the kernel called one of ``names`` from the NEWEST committed
    profile set under profiles/ that has it: HBM-side bytes from the separate rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE runs,
    profiles/<tag>_pmc_{f,w}.csv; FETCH_SIZE is doubled: gfx950 counts 128-B requests of wide coalesced reads as 64 B,
    MI355X_MICROARCH.md HBM section; both counters are KiB) and the warm-only kernel-trace average of the same set
    (profiles/<tag>_kernel_stats.csv).  These describe the COMMITTED profile run of ``tag``, not this process: the JSON line names the
    tag next to them and keeps its own live HIP-event duration apart (``ms_per_launch`` / ``frac`` vs ``frac_rocprof``)."""
    for tag in PMC_TAGS:
        for name in names:                   # names in priority order: the first one the set knows is the launch (older sets: older kernels)
            vals = {}
            for suffix, ctr in (("f", "FETCH_SIZE"), ("w", "WRITE_SIZE")):
                path = os.path.join(REPO, "profiles", "%s_pmc_%s.csv" % (tag, suffix))
                if not os.path.exists(path):
                    break
                for line in open(path):
                    if name in line and "," + ctr + "," in line:
                        vals[ctr] = float(line.rsplit(",", 1)[1])
                        break
            if len(vals) == 2:
                avg = None
                ks = os.path.join(REPO, "profiles", "%s_kernel_stats.csv" % tag)
                if os.path.exists(ks):
                    for line in open(ks):
                        if name in line:
                            avg = float(line.split(",")[2])          # calls,total_ms,avg_ms,...
                            break
                return int((2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024), avg, tag
    return None, None, None


def expansion_bytes(pixrect, sub, obj, n_obj, bf16_copy):
    """Algorithmic HBM bytes of one launch of the pair expansion over pixel rectangles (``pair_expand_dense_kernel``, SURVEY 8d's
    "write every z_ij once, read every U_i / V_j once" restricted to the pixels conv3 over shared windows reads): per live
    (pair, 16-grid pixel) one 1 KiB channel row of z (f16) + 256 B of routing codes (two 4-bit codes per byte) [+ 1 KiB bf16 copy],
    and per DISTINCT (object, role, pixel) that some pair needs the four 1 KiB source rows of its 2x2 pooling window (read once;
    re-reads are served by LDS / L2 and are not algorithmic).  ``pixrect`` packs y0 | y1 << 5 | x0 << 10 | x1 << 15."""
    import numpy as np
    r = pixrect.astype(np.int64)
    y0, y1, x0, x1 = r & 31, (r >> 5) & 31, (r >> 10) & 31, (r >> 15) & 31
    live = int(((y1 - y0).clip(0) * (x1 - x0).clip(0)).sum())
    reads = 0
    ok = (y1 > y0) & (x1 > x0)
    for idx in (sub, obj):
        d = np.zeros((n_obj, 18, 18), dtype=np.int32)
        o = idx[ok].astype(np.int64)
        np.add.at(d, (o, y0[ok], x0[ok]), 1)
        np.add.at(d, (o, y1[ok], x0[ok]), -1)
        np.add.at(d, (o, y0[ok], x1[ok]), -1)
        np.add.at(d, (o, y1[ok], x1[ok]), 1)
        cover = d.cumsum(1).cumsum(2)[:, :16, :16] > 0
        reads += int(cover.sum()) * 4 * 1024
    return live * (1024 + 256 + (1024 if bf16_copy else 0)) + reads, live


def window_gemm_bytes(key, n_list, e_obj, live_rows, n_ps):
    """ALGORITHMIC HBM bytes of one launch of a GEMM over the listed windows (what ``roofline.traffic`` is to be compared with; the
    units are stated in DESIGN.md 7): every operand byte read once, every result byte written once.
      conv3_fwd_windows:   the distinct z rows under the listed windows' 4 x 4 patches (1 KiB f16 each; ``live_rows`` of the real pairs
                           from the expansion's pixel rectangles, at most 16 per per-object window / 256 per pseudo-pair map) + the 9.4 MB
                           of weights; per listed window 2 KiB pooled y (f16) + 2 KiB bf16 copy + 1 KiB routing bytes written.
      conv3_dgrad_windows: per listed window of the sparse launch 4 masked pooled rows of 2 KiB + 4 x 256 B index words read, 16 patch
                           rows of 1 KiB written; 42 MB of weights.
      conv3_wgrad_windows: the distinct z rows under the windows' 4 x 4 patches (1 KiB each, gathered from the forward's maps; at most 16 per
                           window) + per listed window 4 KiB packed gradient + 512 B index words read; the 18.9 MB f32 result written
                           once (its split-K slabs are not algorithmic)."""
    e_real = max(n_list - e_obj, 0)
    if key == "conv3_fwd_windows":
        rows = (live_rows if live_rows is not None else e_real * 16) + min(e_obj * 16, n_ps * 256)
        return int(rows * 1024 + 1024 * 4608 * 2 + n_list * 5120)
    if key == "conv3_dgrad_windows":
        e = (e_real // 256) * 256
        return int(e * (4 * 2048 + 4 * 256 + 16 * 1024) + 20 * 512 * 2048 * 2)
    if key == "conv3_wgrad_windows":
        e = (e_real // 16) * 16
        # second operand: the distinct f16 z rows under the windows' patches (gathered from the maps: neighbouring windows share rows),
        # at most 16 per window
        rows = min(live_rows, e * 16) if live_rows is not None else e * 16
        return int(rows * 1024 + e * (4096 + 512) + 1024 * 4608 * 4)
    return None


def scale_boxes(batch, factor):
    """Boxes of a synthetic minibatch scaled about their centres and clipped to the 32x32 grid (>= 100: the whole image).  The
    reference's cost does not depend on the boxes (``model.py:138-150`` runs every pixel of every pair); this implementation's does
    - the pair-specific share of conv3 / fc1 grows with the overlap of the per-object window rectangles - hence the sweep."""
    import torch
    out = []
    for bb in batch.bbox:
        b = bb.double()
        if factor >= 100:
            nb = torch.tensor([0, 32, 0, 32], dtype=torch.float64).repeat(b.shape[0], 1)
        else:
            cx, cy = (b[:, 0] + b[:, 1]) / 2, (b[:, 2] + b[:, 3]) / 2
            hw, hh = (b[:, 1] - b[:, 0]) * factor / 2, (b[:, 3] - b[:, 2]) * factor / 2
            nb = torch.stack([torch.floor(cx - hw), torch.ceil(cx + hw), torch.floor(cy - hh), torch.ceil(cy + hh)], 1).clamp(0, 32)
        out.append(nb.to(bb.dtype))
    batch.bbox = out
    return batch


def executed_flops(P, n_img, n_obj, n_x, n_list, shared, forward_only=False, linear=None):
    """Matrix flops one step really executes (2 x multiply-adds of every GEMM launch, padding rows not counted): what
    ``roofline.step_frac`` divides by the step time.  ``shared``: conv3 / fc1 over shared windows (csrc/kernels_shared.hip) - the
    per-pair GEMMs run over the ``n_list`` listed windows (``n_x`` of them pair-specific) and whole conv3 maps remain only for the
    background maps; otherwise every pair is a whole map.  Passes: forward, data gradient, weight gradient (conv1: no data gradient)."""
    passes = 1 if forward_only else 3
    n_objx = n_obj + (n_img if shared else 0)
    f = {"conv1": 2 * (2.0 * n_img * 1024 * 257 * 128) * (1 if forward_only else 2),
         "conv2": 2 * (2.0 * n_objx * 1024 * 1152 * 512) * passes,
         "fc2": 2.0 * P * 4096 * 512 * passes}
    if shared:
        f["conv3"] = (2.0 * n_list * 4 * 1024 * 4608 + 2.0 * n_img * 256 * 1024 * 4608) * passes
        if linear:          # linear pairs: one forward launch for the raw pre-activations of the per-object entries + the background windows
            f["conv3"] += 2.0 * (linear[1] + 64 * n_img) * 4 * 1024 * 4608
        if linear and not forward_only:
            from scene_graph_commonsense_amd.engine import TUNING
            if TUNING.sparse_wgrad and TUNING.patch_wgrad:
                # the weight gradient of the real pairs' windows runs on the SPARSE matrix cores: half of its multiply-adds (the
                # structural zeros of the un-pooled gradient) are not executed - they are not counted as work either
                e_sp = ((n_list - linear[1]) // 16) * 16
                f["conv3"] -= 0.5 * 2.0 * e_sp * 4 * 1024 * 4608
            if TUNING.sparse_dgrad and TUNING.patch_dgrad and TUNING.weight_kernels and (n_list - linear[1]) >= 4096:
                # the data gradient of the real pairs' windows likewise: 20 sparse instructions' worth of issued multiply-adds per
                # (window, 1024 x 512 block) instead of 36 dense ones
                f["conv3"] -= 2.0 * (((n_list - linear[1]) // 256) * 256) * 16 * 1024 * 512
        f["fc1"] = 2.0 * (n_x + 64 * 2 * n_obj) * 1024 * 4096 * passes
    else:
        f["conv3"] = 2.0 * P * 256 * 1024 * 4608 * passes
        f["fc1"] = 2.0 * P * 65536 * 4096 * passes
    return f


def cpu_baseline(cfg, sd, reps=5, steps_per_rep=16, threads=None):
    """The CPU oracle (literal reference restatement) timed on this host, SURVEY 8d's protocol: f32, fwd + loss + bwd of the
    reference's per-step calls (b = 8 images per call; the per-call cost does not depend on (g, e)); 2 warm-up calls, then ``reps``
    timings of ``2 * steps_per_rep`` calls each (>= 64 calls in all), value = pairs per timing / MEDIAN seconds, spread reported.
    ``threads``: torch intra-op threads (default: the count tools/oracle_threads.py found fastest on this class of host - one
    b = 8 call does not scale past a few dozen threads - capped by the cores present)."""
    import numpy as np
    import torch
    from oracle import relhead_oracle as O
    from scene_graph_commonsense_amd.synthetic import make_scene_batch, predicate_counts
    if threads is None:
        threads = min(usable_cpus(), CPU_BASELINE_THREADS)
    prev = torch.get_num_threads()
    torch.set_num_threads(int(threads))
    try:
        batch = make_scene_batch(cfg, [7] * 8, seed=123, connect_frac=0.3)      # 21 (g, e) steps: room for 16 per timing
        w = O.class_weights(predicate_counts(cfg))
        sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}

        def run(steps):
            for p in sdr.values():
                p.grad = None
            t0 = time.time()
            out = O.run_pair_loop(sdr, batch, cfg, mode="train", weights=w, max_steps=steps)
            out["losses"].backward()
            return time.time() - t0, sum(len(r["keep"]) for r in out["records"]), len(out["records"])

        run(1)                                             # warm-up: one (g, e) step = 2 calls
        times, pairs, calls = [], 0, 0
        for _ in range(reps):
            dt, pairs, calls = run(steps_per_rep)
            times.append(dt)
        med = float(np.median(times))
        return {"value": round(pairs / med, 2), "unit": "pairs/s", "cores": int(threads), "kind": "port",
                "n_calls": calls * reps, "calls_per_timing": calls, "timings": reps, "median_s": round(med, 3),
                "min_s": round(min(times), 3), "max_s": round(max(times), 3),
                "sample": "2 warm-up calls, then %d timings of %d reference calls of b=8 pairs each (%d calls; fwd+loss+bwd, f32, "
                          "%d torch threads of %d host threads); value = %d pairs / median %.2f s (min %.2f, max %.2f)"
                          % (reps, calls, calls * reps, threads, usable_cpus(), pairs, med, min(times), max(times))}
    finally:
        torch.set_num_threads(prev)


def dry_run(args):
    """Everything of a rank except the GPU work: rendezvous, barrier, MAX-reduced time, one JSON line from rank 0."""
    import torch
    import torch.distributed as dist
    from scene_graph_commonsense_amd import distributed as sgd_dist
    rank, world, _ = sgd_dist.init_from_env(backend=args.backend or "gloo")
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d: refusing to report a number for the wrong rank count" % (args.gpus, world))
    if world > 1:
        dist.barrier()
    t0 = time.time()
    for _ in range(args.steps):
        time.sleep(0.001 * (rank + 1))
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.time() - t0], dtype=torch.float64)
    ranks = torch.tensor([1.0])
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(ranks, op=dist.ReduceOp.SUM)
    if rank == 0:
        print(json.dumps({"metric": "dry run (launcher plumbing only)", "value": 0.0, "unit": "pairs/s", "n_gpus": world,
                          "ranks_seen": int(ranks.item()), "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(float(t.item()) / max(args.steps, 1) * 1e3, 3), "dry_run": True}), flush=True)
    if world > 1:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ one rank
def run_rank(args):
    import numpy as np
    import torch
    from scene_graph_commonsense_amd import distributed as sgd_dist
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    if os.environ.get("SGC_BENCH_SHARE_GPU") == "1":
        # TEST HOOK: every rank on the devices that exist (rank % device_count) - exercises the whole multi-rank path (launcher,
        # rendezvous, early + flat gradient reduction, MAX-reduced time) on a one-GPU box over gloo; RCCL refuses to share a device
        os.environ["LOCAL_RANK"] = str(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    rank, world, local = sgd_dist.init_from_env(backend=args.backend)
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d: refusing to report a number for the wrong rank count" % (args.gpus, world))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    from scene_graph_commonsense_amd.pairs import flatten_scene
    cfg = HeadConfig() if args.dataset == "vg" else HeadConfig(dataset="oiv6", num_classes=601, num_super_classes=0,
                                                               num_geometric=4, num_possessive=2, num_semantic=24)
    sd = make_state_dict(cfg, seed=0)
    model = BayesianRelationClassifier(cfg.args(run_mode="train"), num_classes=cfg.num_classes,
                                       num_super_classes=cfg.num_super_classes, num_geometric=cfg.num_geometric,
                                       num_possessive=cfg.num_possessive, num_semantic=cfg.num_semantic).to(dev)
    model.load_state_dict(sd)
    model.train()
    batch = make_scene_batch(cfg, [args.objects] * args.images, seed=1000 + rank, connect_frac=0.02)
    if args.box_scale != 1.0:
        scale_boxes(batch, args.box_scale)
    if args.box_dist != "survey":
        from scene_graph_commonsense_amd.synthetic import with_vg_like_boxes
        with_vg_like_boxes(batch, 1000 + rank, median_area=int(args.box_dist[2:]) / 100.0)
    # inputs resident in HBM when the timed region starts (the DETR features are produced on the GPU upstream); the ragged
    # annotation lists stay host-side Python objects exactly as the reference's dataloader hands them over
    batch.image_feature = batch.image_feature.to(dev)
    batch.image_depth = batch.image_depth.to(dev)
    if args.torch_sgd:
        opt = torch.optim.SGD(model.parameters(), lr=1e-5, momentum=0.9, weight_decay=1e-4)
    else:                                    # same update in one pass over (grad, weight, momentum buffer): optim.FusedSGD
        from scene_graph_commonsense_amd.optim import FusedSGD
        opt = FusedSGD(model.parameters(), lr=1e-5, momentum=0.9, weight_decay=1e-4)
    reducer = sgd_dist.GradReducer(world)
    if world > 1 and args.dp_mode == "sharded" and not args.torch_sgd:
        # one object is both: reduce-scatter of the gradients, SGD on this rank's shard, all-gather of the updated parameters
        opt = reducer = sgd_dist.ShardedSGD(model.named_parameters(), world, rank, lr=1e-5, momentum=0.9, weight_decay=1e-4,
                                            defer_gather=True).attach(model)
    eng = model.engine()
    # what train_test.training does before its epoch loop: a full CPython collection walks ~2.7 x 10^5 set-up objects (77 ms measured) and
    # fell into the timed region about once per 25 steps (+2.5 ms per step in the driver's --steps 20 --warmup 5 run of round 4)
    from scene_graph_commonsense_amd.pair_loop import freeze_setup_objects
    freeze_setup_objects()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def measure(batch, steps, warmup):
        """W untimed + K timed steps on ``batch`` (barrier + device synchronisation on both sides); this rank's wall time and
        what the engine did."""
        scene0 = flatten_scene(cfg, batch, dev)
        # SGD as in the reference (momentum 0.9, wd 1e-4, lr 1e-5 at its largest case N=20, i.e. T=380 direction-steps).
        # The running-sum loss quirk scales the gradient with T^2, so the learning rate is scaled by (380/T)^2 to keep
        # the update as stable as the reference's at N=64 (T=4032): otherwise the weights diverge within three steps and
        # the timed kernels would run on inf/NaN data (data-dependent clocks, meaningless ReLU masks).
        # Round 5: and a further 1e-3 (BENCH_LR_SCALE).  At the stable rate the synthetic problem still collapsed within tens of steps -
        # zero fraction of z 0.46 -> 0.999 and of h1 0.75 -> 0.965 after 70 steps - and a collapsed network draws less power: the SAME
        # launches ran 45.9 -> 43.2 ms (profiles/r05_host_gc.txt), so "--warmup 40" read 8 % faster than "--warmup 5".  The update
        # kernel does the same work at any rate; with the small one every timed step sees the activation statistics of the
        # initialisation, whatever --warmup / --steps are.
        opt.param_groups[0]["lr"] = BENCH_LR_SCALE * 1e-5 * min(1.0, (380.0 / max(scene0.n_steps, 1)) ** 2)

        last = {}

        def step():
            if args.forward_only:
                last["out"] = model.forward_pairs(scene0 if args.cached_scene else flatten_scene(cfg, batch, dev))
                return None
            return train_minibatch(model, batch, opt, reducer=reducer, scene=scene0 if args.cached_scene else None, streams=args.streams)

        # per-kernel HIP events (engine.timers) only for --full: a plain run times the step without them
        eng.timers = {} if args.full else None
        eng._xw = None
        first_loss = None
        for _ in range(warmup):
            l0 = step()
            if first_loss is None and l0 is not None:
                first_loss = float(l0)
        eng.timers = {} if args.full else None
        torch.cuda.reset_peak_memory_stats(dev)
        barrier()
        reducer.pop_exposed_ms()
        t0 = time.time()
        loss = None
        for _ in range(steps):
            loss = step()
        barrier()
        dt = time.time() - t0
        kern = {name: float(np.mean([a.elapsed_time(b) for a, b in evs])) for name, evs in (eng.timers or {}).items()}
        outputs = last.get("out") if args.forward_only else model.last_outputs
        xw = getattr(eng, "_xw", None)
        n_x = int(xw[1][-1]) if xw is not None else 0
        exp_bytes = None
        Pn = scene0.n_pairs
        one_group = eng.ws.bufs["xw_pixrect"].numel() >= Pn if "xw_pixrect" in eng.ws.bufs else False    # image groups / lanes: per-group tables
        if args.full and xw is not None and "expand_dense" in kern and one_group and not args.forward_only and (args.streams or 1) == 1:
            exp_bytes = expansion_bytes(eng.ws.bufs["xw_pixrect"][:Pn].cpu().numpy(), scene0.sub_idx.cpu().numpy(), scene0.obj_idx.cpu().numpy(),
                                        int(scene0.obj_img.shape[0]), bf16_copy="z_pad_bf" in eng.ws.bufs and
                                        eng.ws.bufs["z_pad_bf"].numel() >= (Pn + 1) * 18 * 18 * 512)
        n_list = (int(state_plan_total(eng)) if state_plan_total(eng) else n_x) if xw is not None else 0
        return dict(dt=dt, loss=None if loss is None else float(loss), first_loss=first_loss, kern=kern, P=scene0.n_pairs,
                    shared=xw is not None, n_x=n_x, n_list=n_list, n_obj=int(scene0.obj_img.shape[0]),
                    linear=getattr(eng, "_xw_linear", None) if xw is not None else None,
                    exposed_ms=reducer.pop_exposed_ms() / max(steps, 1), exp_bytes=exp_bytes,
                    peak_gb=torch.cuda.max_memory_allocated(dev) / 1e9, outputs=outputs)

    m = measure(batch, args.steps, args.warmup)
    P, loss, first_loss, kern = m["P"], m["loss"], m["first_loss"], m["kern"]
    if args.dump_outputs:
        if hasattr(opt, "wait_gathers"):
            opt.wait_gathers()                               # a deferred all-gather may still be writing fc1.weight
        if rank == 0:
            write_outputs(args.dump_outputs, loss, m["outputs"], None if args.forward_only else model)
    m["outputs"] = None
    t = torch.tensor([m["dt"]], device=dev, dtype=torch.float64)
    rank_ms = torch.zeros(world, device=dev, dtype=torch.float64)
    rank_ms[rank] = m["dt"] / args.steps * 1e3
    ranks = torch.ones(1, device=dev)
    if world > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(ranks, op=torch.distributed.ReduceOp.SUM)
        torch.distributed.all_reduce(rank_ms, op=torch.distributed.ReduceOp.SUM)
    dt = float(t.item())
    assert int(ranks.item()) == args.gpus, "ranks that took part in the timed region != --gpus"

    # ---- per-kernel durations of the BACKWARD launches: the timed step runs its backward on two streams (weight-gradient chain beside
    # the data-gradient chain), where HIP-event intervals of overlapping launches are not kernel times.  One more short pass of the
    # same step on ONE stream (after the timed region; 1 warm-up + 2 steps) gives them; rank 0, N = 1 only.
    kern_1s = None
    from scene_graph_commonsense_amd import engine as _engine_mod
    if args.full and world == 1 and not args.forward_only and _engine_mod.TUNING.bwd_streams:
        with _engine_mod.tuning(bwd_streams=False):
            kern_1s = measure(batch, 2, 1)["kern"]
    elif args.full and not args.forward_only:
        kern_1s = kern

    # ---- box-size sensitivity (N=1): the same step on scaled boxes - the pair-specific share of conv3 / fc1, hence the step time
    # and the workspace, depend on how much the objects' window rectangles overlap; the reference's cost does not
    sensitivity = None
    if args.full and world == 1 and not args.no_sensitivity and not args.forward_only and args.box_scale == 1.0 and args.box_dist == "survey":
        sensitivity = []
        from scene_graph_commonsense_amd.synthetic import with_vg_like_boxes
        vg = "raw boxes with assumed VG-like marginals (median area %d %% of the image) through the reference's box pipeline"
        for label, factor in ((vg % 3, -0.03), (vg % 6, -0.06), (vg % 12, -0.12), ("boxes x1.5", 1.5), ("boxes x2.5", 2.5), ("every box = full image", 100.0)):
            eng.ws.bufs.clear()                       # the workspace only grows: start every point from an empty one
            model._weights_version = None
            torch.cuda.empty_cache()
            b2 = make_scene_batch(cfg, [args.objects] * args.images, seed=1000 + rank, connect_frac=0.02)
            b2 = with_vg_like_boxes(b2, 1000 + rank, median_area=-factor) if factor < 0 else scale_boxes(b2, factor)
            b2.image_feature, b2.image_depth = batch.image_feature, batch.image_depth
            r = measure(b2, 2, 1)
            fl = executed_flops(r["P"], args.images, r["n_obj"], r["n_x"], r["n_list"], r["shared"], linear=r["linear"])
            sensitivity.append({"boxes": label, "pair_specific_fraction": round(r["n_x"] / max(64 * r["P"], 1), 4) if r["shared"] else 1.0,
                                "path": "shared windows" if r["shared"] else "per-pair kernels (more than SGC_SHARED_MAX_FRACTION of the windows pair-specific)",
                                "ms_per_step": round(r["dt"] / 2 * 1e3, 2), "pairs_per_s": round(r["P"] * 2 / r["dt"], 1),
                                "peak_memory_gb": round(r["peak_gb"], 1),
                                "step_frac": round(sum(fl.values()) / (r["dt"] / 2) / 1e12 / MFMA_PEAK_TFLOPS, 4)})

    # ---- the same step with every sharing identity off (SGC_SHARED_LEVEL=0: conv3 / fc1 per pair over whole maps): the ONLY form whose
    # multiply-adds are SURVEY 8d's 8.99 GFLOP per ordered pair, so its rate is what "fraction of the MFMA peak on the survey's flop
    # count" honestly means (``survey_equivalent_tflops`` of the headline exceeds the peak because most of that work is not executed)
    survey_pass = None
    if args.full and world == 1 and not args.no_sensitivity and not args.forward_only and args.box_scale == 1.0 \
            and args.box_dist == "survey" and (args.streams or 1) == 1 and args.images * args.objects <= 1024:
        eng.ws.bufs.clear()
        model._weights_version = None
        torch.cuda.empty_cache()
        with _engine_mod.tuning(shared_conv3=False, shared_fc1=False, shared_objects=False, shared_linear=False, shared_conv2=False):
            r0 = measure(batch, 2, 1)
        survey_pass = {"ms_per_step": round(r0["dt"] / 2 * 1e3, 2), "pairs_per_s": round(r0["P"] * 2 / r0["dt"], 1),
                       "survey_flops_step_frac": round(r0["P"] * 8.99e9 / (r0["dt"] / 2) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                       "peak_memory_gb": round(r0["peak_gb"], 1),
                       "note": "two steps (after one warm-up) of the same minibatch on the per-pair kernels, every restructuring identity off; "
                               "8.99 GFLOP per ordered pair (SURVEY 8d) / step time / 2.5 PFLOP/s"}
        eng.ws.bufs.clear()
        model._weights_version = None
        torch.cuda.empty_cache()

    if rank == 0:
        ms = dt / args.steps * 1e3
        value = P * world * args.steps / dt
        flops = {"conv3_fwd": 2.0 * P * 256 * 1024 * 4608, "conv3_dgrad": 2.0 * P * 256 * 512 * 9216,
                 "conv3_wgrad": 2.0 * P * 256 * 1024 * 4608, "fc1_fwd": 2.0 * P * 65536 * 4096,
                 "fc1_dgrad": 2.0 * P * 65536 * 4096, "fc1_wgrad": 2.0 * P * 65536 * 4096}
        from scene_graph_commonsense_amd.engine import TUNING
        two_streams = TUNING.bwd_streams and not args.forward_only
        fwd_only = ("conv2_fwd", "expand_dense", "expand", "expand_train", "conv3_fwd", "conv3_fwd_objects", "conv3_fwd_windows", "conv3_fwd_raw", "conv3_fwd_linear",
                    "conv3_fwd_assemble", "fc1_fwd", "fc1_fwd_windows", "fc1_fwd_integral", "fc1_fwd_assemble", "fc2_fwd")
        xw = True if m["shared"] else None
        n_x, n_list = m["n_x"], m["n_list"]          # X windows; X windows + the pseudo-pairs' own windows
        if xw is not None:                         # conv3 / fc1 over shared windows: flops of what is actually computed
            n_ps = 2 * args.objects * args.images
            flops["conv3_fwd_windows"] = 2.0 * n_list * 4 * 1024 * 4608
            # whole maps that still go through the ordinary conv3 kernel: the images' background maps (second level of sharing:
            # TUNING.shared_objects) or every pseudo-pair (first level)
            flops["conv3_fwd_objects"] = 2.0 * (args.images if (TUNING.shared_objects and TUNING.shared_fc1) else n_ps) * 256 * 1024 * 4608
            flops["conv3_dgrad_windows"] = flops["conv3_wgrad_windows"] = flops["conv3_fwd_windows"]
            if m["linear"] and TUNING.sparse_wgrad and TUNING.patch_wgrad:
                # the timer "conv3_wgrad_windows" is the SPARSE launch over the real pairs' windows (the dense tail has its own timer):
                # executed = the non-zero half of its dense-equivalent multiply-adds
                e_sp = ((n_list - m["linear"][1]) // 16) * 16
                flops["conv3_wgrad_windows"] = 0.5 * 2.0 * e_sp * 4 * 1024 * 4608
            if m["linear"] and TUNING.sparse_dgrad and TUNING.patch_dgrad and TUNING.weight_kernels and (n_list - m["linear"][1]) >= 4096:
                # likewise the timer "conv3_dgrad_windows" = the SPARSE launch (csrc/kernels_dgrad_sp.hip): 20 slots x 1024 compressed k x 512
                # issued multiply-adds per window (the dense form: 36 x 1024 x 512)
                flops["conv3_dgrad_windows"] = 2.0 * (((n_list - m["linear"][1]) // 256) * 256) * 20 * 1024 * 512
            flops["fc1_fwd_windows"] = 2.0 * (n_x + 64 * n_ps) * 1024 * 4096          # padding rows not counted
            flops["fc1_dgrad"] = flops["fc1_wgrad"] = flops["fc1_fwd_windows"]
        else:
            flops["conv3_fwd_windows"] = flops["conv3_fwd"]

        def gemm_record(key, ms, source):
            names, what = WINDOW_GEMMS[key]
            ach = flops[key] / (ms * 1e-3) / 1e12
            traffic, rocprof_ms, tag = pmc_traffic(names) if (P == 32256 and args.box_scale == 1.0 and args.dataset == "vg") else (None, None, None)
            alg = window_gemm_bytes(key, n_list, m["linear"][1] if m["linear"] else 0, m["exp_bytes"][1] if m.get("exp_bytes") else None,
                                    2 * args.objects * args.images)
            return {"bound": "mfma", "kernel": "%s: %d listed windows x 4 pixels x 1024 x 4608 (the pair-specific windows of the %d per-pair windows + "
                                               "the per-object windows; the rest is shared)" % (what, n_list, P * 64),
                    "timer": key, "achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
                    "traffic": traffic, "algorithmic_bytes": alg,
                    "traffic_over_algorithmic": None if not (traffic and alg) else round(traffic / alg, 2),
                    "traffic_note": "bytes/launch = (2*FETCH_SIZE + WRITE_SIZE)*1024 from profiles/%s_pmc_{f,w}.csv (separate rocprofv3 --pmc passes "
                                    "at this workload)" % tag,
                    "ms_per_launch": round(ms, 3), "ms_source": source, "executed_tflop": round(flops[key] / 1e12, 3),
                    # the two timings, kept apart: ``frac`` = this process's HIP events on this box; ``frac_rocprof`` = the warm-only
                    # rocprofv3 --kernel-trace average of the committed profile set ``profile_tag`` (the set ``traffic`` comes from; same
                    # workload and window list, possibly another box / an older commit)
                    "profile_tag": tag, "ms_per_launch_rocprof": rocprof_ms,
                    "frac_rocprof": None if not rocprof_ms else round(flops[key] / (rocprof_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}

        roof, roof_all = None, []
        for key in WINDOW_GEMMS:
            if key == "conv3_fwd_windows":
                ms_k, src = kern.get(key, 0.0), "HIP events on the launch stream, timed steps"
            else:
                ms_k, src = (kern_1s or {}).get(key, 0.0), "HIP events, single-stream pass of the same step after the timed region"
            if xw is not None and ms_k > 0:
                roof_all.append(gemm_record(key, ms_k, src))
        if not roof_all and kern.get("conv3_fwd", 0) > 0:           # per-pair kernels (no shared windows): conv3 forward over whole maps
            ach = flops["conv3_fwd"] / (kern["conv3_fwd"] * 1e-3) / 1e12
            roof_all.append({"bound": "mfma", "kernel": "conv16_halo_pp_kernel<f16,relu+pool> (sgc_conv3_relu_pool: every pair a whole map)", "timer": "conv3_fwd",
                             "achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4), "traffic": None,
                             "ms_per_launch": round(kern["conv3_fwd"], 3)})
        if roof_all:
            roof = dict(max(roof_all, key=lambda r: r["ms_per_launch"]))       # the step's longest launch
        hbm = None
        if m.get("exp_bytes") and kern.get("expand_dense", 0) > 0:
            # north_star names the pair expansion's HBM rate: the longest HBM-bound launch of the forward
            eb, live = m["exp_bytes"]
            gbs = eb / (kern["expand_dense"] * 1e-3) / 1e9
            hbm = {"bound": "hbm", "kernel": "pair_expand_dense_list_kernel (sgc_pair_expand_dense_windows: z_ij = maxpool2(relu(U_i + V_j)) on the "
                                             "%d live (pair, pixel) items next to the pair-specific windows, of %d)" % (live, P * 256),
                   "bytes": int(eb), "ms_per_launch": round(kern["expand_dense"], 3), "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                   "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                   "note": "algorithmic bytes: 1 KiB z row + 256 B routing codes per live item, 4 KiB per distinct (object, role, pixel) read "
                           "once; the launch is bound by its vector instructions (~156 per lane and item after round 6's v_fma_mix_f32 / "
                           "v_max3_f32 form, ~200 before: profiles/r06_expand_ab.txt), not by these bytes"}
        ex = executed_flops(P, args.images, m["n_obj"], n_x, n_list, m["shared"], args.forward_only, linear=m["linear"])
        if roof is not None:
            # whole-step efficiency on EXECUTED matrix flops (the per-pair form SURVEY 8d prices is mostly not executed any more)
            roof["step_frac"] = round(sum(ex.values()) / (dt / args.steps) / 1e12 / MFMA_PEAK_TFLOPS, 4)
            roof["step_executed_tflop"] = {k: round(v / 1e12, 2) for k, v in ex.items()}
        out = {
            "metric": "ordered object-pairs/sec (relation head fwd+bwd), batch=%d, N=%d" % (args.images, args.objects)
                      if not args.forward_only else "ordered object-pairs/sec (relation head forward only)",
            "value": round(value, 1), "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f16 fwd / bf16 bwd (f32 accumulate, f32 master weights)", "data": "synthetic",
            "config": {"workload": "%s PredCLS synthetic, %d images x %d objects per GPU = %d ordered pairs per GPU per step%s"
                                   % (args.dataset.upper(), args.images, args.objects, P,
                                      " (scene flattened once outside the loop)" if args.cached_scene else ", from the raw minibatch"),
                       "parallelism": "dp%d" % world},
            "loss": None if loss is None else float(loss), "loss_first_step": first_loss,
            "host": {"gc": "set-up objects frozen before the loop (pair_loop.freeze_setup_objects, as train_test.training does)",
                     "lr_scale": BENCH_LR_SCALE,
                     "lr_note": "SGD runs in full at a rate small enough that every timed step sees the initialisation's activation "
                                "statistics (at the round-4 rate the synthetic problem collapsed to all-zero activations within ~70 "
                                "steps and the same launches ran 6 % faster on the idle data)"},
            "roofline": roof,
            "roofline_kernels": roof_all,           # the three GEMMs over the listed windows, each against the dense MFMA peak
            "hbm": hbm,
            # SURVEY 8d priced the path at 2.996 (fwd) / 8.99 (fwd+bwd) GFLOP per ordered pair, taking conv3 / fc1 per pair as
            # irreducible; with the shared windows most of that is no longer executed, so this is an equivalence, not a rate
            "survey_equivalent_tflops": round(value / max(world, 1) * (2.996e9 if args.forward_only else 8.99e9) / 1e12, 1),
            "survey_flops_pass": survey_pass,
            "survey_flops_step_frac": None if survey_pass is None else survey_pass["survey_flops_step_frac"],
            "shared_windows": None if xw is None else {"pair_specific": n_x, "of": P * 64, "fraction": round(n_x / max(P * 64, 1), 4),
                                                       "combined_not_convolved": m["linear"][0] if m["linear"] else 0,
                                                       "note": "conv3 and fc1 run per pair only on these pooling windows; the rest is computed "
                                                               "once per object (csrc/kernels_shared.hip)"},
            "kernels_ms": {k: round(v, 3) for k, v in sorted(kern.items()) if k in fwd_only or not two_streams},
            "kernels_tflops": {k: round(flops[k] / (kern[k] * 1e-3) / 1e12, 1) for k in kern
                               if k in flops and kern[k] > 0 and (k in fwd_only or not two_streams)},
            # every launch of the step on ONE stream (the pass after the timed region): per-kernel times of the backward
            "kernels_ms_single_stream": None if (kern_1s is None or kern_1s is kern) else {k: round(v, 3) for k, v in sorted(kern_1s.items())},
            "backward_streams": 2 if two_streams else 1,
            "image_group_lanes": len(getattr(model, "last_image_groups", None) or [1]) if not args.forward_only else 1,
            "peak_memory_gb": round(m["peak_gb"], 1),
            "ranks_seen": int(ranks.item()), "rank_ms_per_step": [round(float(x), 2) for x in rank_ms.tolist()],
            "sensitivity": sensitivity,
        }
        if world > 1:
            out["dp_mode"] = args.dp_mode if not args.torch_sgd else "allreduce"
            out["exposed_comm_ms"] = round(m["exposed_ms"], 3)      # rank 0: time its compute stream waited for collectives, per step
        if not args.full:
            # a plain run: the headline, its configuration and this run's own bookkeeping; the analysis fields are --full's
            out = {k: v for k, v in out.items() if k in PLAIN_FIELDS}
        elif two_streams:
            out["kernels_note"] = ("backward launches run on two streams and overlap: their HIP-event durations are not kernel times and "
                                   "are omitted (SGC_BWD_STREAMS=0 for single-stream per-kernel numbers, as in profiles/)")
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg, sd)
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args, argv))
    if args.dry_run:
        return dry_run(args)
    run_rank(args)


if __name__ == "__main__":
    main()
