"""bench.py's contract: one JSON line, n_gpus equal to --gpus, roofline object present with --full, headline only without it,
outputs written by --dump-outputs, refusals.  The multi-rank test runs it as the
driver does - a subprocess that launches its ranks; the single-rank line and the two refusals call ``bench.main(argv)`` in this
process (same entry point and argument parsing; a fresh interpreter + ``import torch`` costs 10 s on a quiet box and has been seen to
take over a minute on a busy one, four times per suite)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _main_in_process(capsys, monkeypatch, *flags, env=None):
    """``bench.main(flags)`` here; returns (exit code or None, stdout + stderr text)."""
    sys.path.insert(0, REPO)
    import bench
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    code = None
    try:
        bench.main(list(flags))
    except SystemExit as e:
        code = e.code
    cap = capsys.readouterr()
    return code, cap.out + cap.err + (code if isinstance(code, str) else "")


def test_bench_single_rank_line(capsys, monkeypatch):
    import gc
    import torch
    code, text = _main_in_process(capsys, monkeypatch, "--gpus", "1", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--full")
    gc.collect()
    torch.cuda.empty_cache()                             # the sensitivity points grew a 100+ GB workspace in this process
    assert code in (None, 0), text[-3000:]
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert len(lines) == 1, text
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 1 and out["unit"] == "pairs/s" and out["scaling"] == "weak"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert "from the raw minibatch" in out["config"]["workload"] and "32256" in out["config"]["workload"]
    roof = out["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and roof["ms_per_launch"] < out["ms_per_step"]
    assert out["loss"] == out["loss"]          # finite, not NaN
    # no printed rate may exceed the chip's dense peak (a mis-labelled flop count once printed 14x the peak), the
    # roofline record is the step's LONGEST launch among the three window GEMMs, backward durations from the single-stream pass
    import bench
    rk = out["roofline_kernels"]
    assert {r["timer"] for r in rk} == {"conv3_fwd_windows", "conv3_dgrad_windows", "conv3_wgrad_windows"}
    assert all(0 < r["frac"] < 1 and 0 < r["achieved"] < bench.MFMA_PEAK_TFLOPS for r in rk)
    assert roof["ms_per_launch"] == max(r["ms_per_launch"] for r in rk)
    assert all(0 < v < bench.MFMA_PEAK_TFLOPS for v in out["kernels_tflops"].values()), out["kernels_tflops"]
    assert out["hbm"] is None or 0 < out["hbm"]["frac"] < 1
    assert out["kernels_ms_single_stream"] and "conv3_dgrad_windows" in out["kernels_ms_single_stream"]
    # whole-step efficiency on executed flops, and the box-size sensitivity sweep of the default invocation
    assert 0 < roof["step_frac"] < roof["frac"] + 0.2 and roof["step_frac"] < 1
    assert out["ranks_seen"] == 1 and len(out["rank_ms_per_step"]) == 1 and out["peak_memory_gb"] > 1
    sens = out["sensitivity"]
    assert [s["boxes"] for s in sens[3:]] == ["boxes x1.5", "boxes x2.5", "every box = full image"]
    assert all("VG-like marginals" in s["boxes"] for s in sens[:3])
    vgf = [s["pair_specific_fraction"] for s in sens[:3]]
    assert vgf == sorted(vgf) and 0.03 < vgf[0] < vgf[2] < 0.35       # median area 3 / 6 / 12 %: tools/vg_box_statistic.py gives 0.07 / 0.12 / 0.22
    fr = [out["shared_windows"]["fraction"]] + [s["pair_specific_fraction"] for s in sens[3:]]
    assert fr == sorted(fr) and fr[-1] == 1.0 and sens[-1]["path"].startswith("per-pair")
    assert all(s["ms_per_step"] > 0 and s["peak_memory_gb"] > 1 for s in sens)
    # self-auditing fields: algorithmic bytes beside the counter traffic for all three window GEMMs, and the step
    # with every identity off priced on SURVEY 8d's own flop count - the honest counterpart of ``survey_equivalent_tflops``
    for r in rk:
        assert r["algorithmic_bytes"] > 1e9
        if r["traffic"]:
            assert r["traffic_over_algorithmic"] == round(r["traffic"] / r["algorithmic_bytes"], 2) and r["traffic_over_algorithmic"] >= 0.9
    assert roof["algorithmic_bytes"] > 1e9
    sp = out["survey_flops_pass"]
    assert 0.2 < out["survey_flops_step_frac"] < 1 and out["survey_flops_step_frac"] == sp["survey_flops_step_frac"]
    assert sp["ms_per_step"] > out["ms_per_step"]                      # the per-pair form is slower than the shipped step (5x when both are warm)
    assert out["survey_equivalent_tflops"] > 0


def test_bench_plain_line_and_dumped_outputs(capsys, monkeypatch, tmp_path):
    """Without --full the line holds the headline and its configuration only (no per-kernel timers, no extra passes); --dump-outputs
    writes the last timed step's loss, pair outputs and updated parameters as float32 / float64 .npy files, at most 64 MB."""
    import gc
    import numpy as np
    import torch
    code, text = _main_in_process(capsys, monkeypatch, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    gc.collect()
    torch.cuda.empty_cache()
    assert code in (None, 0), text[-3000:]
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert len(lines) == 1, text
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["unit"] == "pairs/s" and out["higher_is_better"] is True
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["dtype"] and out["metric"].startswith("ordered object-pairs/sec")
    import bench
    assert set(out) <= set(bench.PLAIN_FIELDS)
    files = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert {"loss", "out_relation", "out_connectivity", "out_hidden", "param_fc1.weight", "param_conv3_1.weight"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert float(files["loss"][0]) == out["loss"] and np.isfinite(files["out_relation"]).all()
    assert files["out_relation"].shape == (32256, 50) and files["param_fc1.weight"].shape == (bench.DUMP_SAMPLE,)


def test_bench_refuses_a_world_size_that_is_not_gpus(capsys, monkeypatch):
    code, text = _main_in_process(capsys, monkeypatch, "--gpus", "2", "--steps", "1", "--warmup", "0",
                                  env=dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert code not in (None, 0) and "refusing" in text


def test_bench_launcher_refuses_more_ranks_than_gpus(capsys, monkeypatch):
    """``--gpus N`` with fewer than N devices: the launcher says so instead of starting ranks that would share a GPU."""
    import torch
    n = torch.cuda.device_count()
    code, text = _main_in_process(capsys, monkeypatch, "--gpus", str(n + 1), "--steps", "1", "--warmup", "0")
    assert code not in (None, 0) and "GPU(s) visible" in text


def test_bench_two_ranks_end_to_end_on_one_gpu_over_gloo():
    """The whole multi-rank bench path on hardware - launcher, rendezvous, per-rank synthetic shards, early fc1 reduction from the
    side stream + flat bucket, barrier, MAX-reduced time, one JSON line with n_gpus = 2 - with both ranks sharing the one GPU of
    the test box over gloo (test hook SGC_BENCH_SHARE_GPU; RCCL itself needs one GPU per rank and is the driver's to run)."""
    env = dict(os.environ, SGC_BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--objects", "20",
                        "--images", "4", "--backend", "gloo", "--no-cpu-baseline"], capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["value"] > 0
    assert out["loss"] == out["loss"] and out["scaling"] == "weak"


def test_bench_eight_ranks_end_to_end_on_one_gpu_over_gloo():
    """The node size the path is built for (8 ranks, ``/root/reference/train_test.py:72-80``) through ONE real step without eight
    GPUs: all ranks share the test box's device over gloo (SGC_BENCH_SHARE_GPU), smallest scene.  Exercises what world = 2 never
    does: ShardedSGD's 8 row blocks x 8 shards of the real fc1.weight (2^28 elements), the padded flat bucket at W = 8, the early
    reduce-scatters from the side stream, deferred gathers, eight per-rank synthetic shards, MAX-reduced time."""
    env = dict(os.environ, SGC_BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "1", "--objects", "6",
                        "--images", "2", "--backend", "gloo", "--no-cpu-baseline"], capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["ranks_seen"] == 8 and out["config"]["parallelism"] == "dp8" and out["value"] > 0
    assert out["dp_mode"] == "sharded" and len(out["rank_ms_per_step"]) == 8 and all(t > 0 for t in out["rank_ms_per_step"])
    assert out["loss"] == out["loss"] and out["scaling"] == "weak"
