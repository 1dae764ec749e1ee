"""bench.py as the driver runs it: a subprocess, ONE parseable JSON line on stdout.

  * `python bench.py --gpus 2 --full ...` on a one-GPU box (HPV_BENCH_ONE_GPU=1: both ranks on cuda:0, gloo group, mailbox
    exchange): the self-launch under torch.distributed.run -> N ranks -> sharded model -> timed windows -> per-rank gather -> one
    line path that the 8-GPU SCALE run depends on (the throughput of two processes sharing a GPU is meaningless and not asserted);
  * the driver-style single-GPU call `--steps 20 --warmup 5 --full`: short windows must be timed 25 times after a wall-clock
    warm-up and the line must carry `roofline` and `cpu_baseline`;
  * the plain call `--steps K --warmup W --dump-outputs DIR`: ONE timed window of exactly K steps, the headline fields only, and
    the dumped parameters / optimizer state are those of K iterations from the seeded initial state.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(args, extra_env=None, timeout=900):
    env = dict(os.environ)
    env.update(extra_env or {})
    if "RANK" not in (extra_env or {}):
        env.pop("RANK", None)
        env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_self_launch_on_one_gpu():
    out = _run_bench(["--gpus", "2", "--steps", "16", "--warmup", "8", "--l2-iters", "600", "--full"], {"HPV_BENCH_ONE_GPU": "1"})
    assert out["n_gpus"] == 2 and out["steps"] == 16 and out["warmup"] == 8
    assert out["metric"].startswith("variational-loss iterations/sec") and out["unit"] == "it/s" and out["value"] > 0
    assert out["scaling"] == "strong" and out["dtype"] == "f64" and out["higher_is_better"] is True
    cfg = out["config"]
    assert cfg["parallelism"] == "element-sharded dp2" and len(cfg["per_rank"]) == 2
    assert sorted(r["rank"] for r in cfg["per_rank"]) == [0, 1]
    assert all(r["pass_structure"] in ("separate", "fused-reverse", "whole-iteration", "whole-iteration-split") for r in cfg["per_rank"])
    assert out["timing"]["windows"] in (5, 25) and len(out["timing"]["window_it_per_s"]) == out["timing"]["windows"]
    assert out["roofline"]["bound"] == "mfma" and out["roofline"]["frac"] > 0
    assert "weak_scaling_probe" in out and "scaled_strong_64x64" in out and "extras_error" not in out, out.get("extras_error")
    assert out["rel_l2_error"]["value"] < 1.5          # (600 iterations: far from converged, but finite and sane)


def test_bench_eight_ranks_self_launch_on_one_gpu():
    """The SCALE run's N = 8 call walked end to end on this one-GPU box (verdict round 5, item 1b): `python bench.py --gpus 8`
    launches itself under torch.distributed.run, eight ranks own 32-element shards of config 4 (gloo group + mailbox exchange: RCCL
    refuses eight ranks on one device), the line gathers eight per-rank records and both scaled probes at N = 8."""
    out = _run_bench(["--gpus", "8", "--steps", "16", "--warmup", "8", "--l2-iters", "400", "--full"], {"HPV_BENCH_ONE_GPU": "1"}, timeout=1500)
    assert out["n_gpus"] == 8 and out["steps"] == 16 and out["value"] > 0 and out["scaling"] == "strong"
    cfg = out["config"]
    assert cfg["parallelism"] == "element-sharded dp8" and len(cfg["per_rank"]) == 8
    assert sorted(r["rank"] for r in cfg["per_rank"]) == list(range(8))
    assert sorted(tuple(r["elements"]) for r in cfg["per_rank"]) == [(32 * k, 32 * k + 32) for k in range(8)]
    assert all(r["exchange"] == cfg["per_rank"][0]["exchange"] for r in cfg["per_rank"])
    assert "extras_error" not in out, out.get("extras_error")
    assert out["scaled_strong_64x64"]["elements"] == 4096 and out["scaled_strong_64x64"]["elements_per_gpu"] == 512
    assert out["weak_scaling_probe"]["elements"] == 2048 and out["weak_scaling_probe"]["elements_per_gpu"] == 256
    assert out["scaled_strong_64x64"]["it_per_s"] > 0 and out["weak_scaling_probe"]["it_per_s"] > 0
    assert out["rel_l2_error"]["value"] < 1.5


def test_bench_driver_style_single_gpu_line():
    out = _run_bench(["--steps", "20", "--warmup", "5", "--l2-iters", "2000", "--residual-elems", "16384", "--cpu-iters", "1",
                      "--full"])
    assert out["n_gpus"] == 1 and out["steps"] == 20 and out["config"]["pass_structure"] == "whole-iteration"
    bi = out["config"]["build"]
    assert bi["test_hooks"] == "0" and bi["k_iter_fused"] in ("ok", "no-quarter-tile")
    assert out["config"]["kernel_variant"] == "k_iter_fused<L=3,SPLIT=false,QT=%s>" % ("true" if bi["k_iter_fused"] == "ok" else "false")
    t = out["timing"]
    assert t["windows"] == 25 and t["untimed_warmup_iterations"] * out["ms_per_step"] * 1e-3 >= 0.2
    assert t["min_it_per_s"] <= out["value"] <= t["max_it_per_s"]
    assert t["max_it_per_s"] / t["min_it_per_s"] < 1.25, t         # clocks have ramped: the windows agree
    r = out["roofline"]
    assert r["bound"] == "mfma" and 0.2 < r["frac"] < 1.0 and r["traffic_source"]
    # the dominant kernel's duration: back-to-back launches between one event pair (event overhead amortised), next to the per-launch pairs
    assert "hpv_time_iteration_kernel" in r["timer"], r["timer"]
    per_launch = out["kernel_ms_per_launch_events"]["mlp_bwd"]
    assert 0.85 * per_launch < r["avg_ms"] < per_launch, (r["avg_ms"], per_launch)
    assert r["avg_ms"] < out["ms_per_step"]
    import shutil
    if shutil.which("rocprofv3") and r["traffic_source"] == "measured in this run":
        # measured in the run (two --pmc passes of a short child run), not read from the committed table
        assert 1.5e6 < r["traffic"] < 8e6 and r["traffic_detail"]["launches_profiled"] >= 64, r     # 1.9 MB algorithmic; 5.0 MB in round 4
    else:      # (no profiler on this box, or a pass failed: the line must say so and carry the committed table's value -- never nothing)
        assert "not measured in this run (" in r["traffic_source"] and r["traffic"] > 0, r
        print("roofline.traffic NOT measured in this run:", r["traffic_source"])
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and len(cb["windows"]) == 3
    assert out["cpu_baseline_vectorized"]["omp"]["OMP_PROC_BIND"] == "close"
    assert out["roofline_residual"]["bound"] == "hbm"
    # the N = 1 line is the base of the driver's 1 -> 8 ratio on the scaled batch: both probes are there at N = 1 too
    assert "extras_error" not in out, out.get("extras_error")
    sc, wk = out["scaled_strong_64x64"], out["weak_scaling_probe"]
    assert sc["elements"] == 4096 and sc["elements_per_gpu"] == 4096 and sc["it_per_s"] > 0 and sc["exchange"] == "none"
    assert wk["elements"] == 256 and wk["elements_per_gpu"] == 256 and wk["it_per_s"] > 0
    assert 0.5 < wk["it_per_s"] / out["value"] < 1.5, (wk, out["value"])    # at N = 1 the weak probe IS config 4 again


def test_bench_default_rccl_exchange_with_a_one_rank_group():
    """What N ranks run by DEFAULT -- the library's own ncclAllReduce inside its iteration graphs (HPV_EXCHANGE unset = rccl) --
    driven through bench.py on one rank (HPV_FORCE_DIST=1: a 1-rank nccl group; the 2-rank test above runs gloo + mailboxes)."""
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    out = _run_bench(["--steps", "16", "--warmup", "8", "--l2-iters", "600", "--no-cpu-baseline", "--no-residual-roofline", "--no-pmc",
                      "--full"],
                     {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "HPV_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1",
                      "MASTER_PORT": str(port)})
    cfg = out["config"]
    assert out["n_gpus"] == 1 and cfg["per_rank"][0]["exchange"] == "rccl" and cfg["exchange"].startswith("in-library ncclAllReduce")
    assert cfg["per_rank"][0]["graphs"] is True, cfg          # the collective was captured into the iteration graphs
    assert cfg["pass_structure"] == "whole-iteration" and out["value"] > 0
    assert out["rel_l2_error"]["value"] < 1.5
    # evidence fields of the collective (verdict round 5, item 1c): the communicator's own rank count, the all-reduce alone
    assert cfg["rccl_world"] == 1 and cfg["per_rank"][0]["rccl_world"] == 1
    assert isinstance(cfg["collective_us"], float) and 0.0 < cfg["collective_us"] < 200.0, cfg["collective_us"]     # (one rank: RCCL has nothing to move, ~0.05 us)


def test_bench_plain_run_times_exactly_the_steps_and_dumps_their_outputs(tmp_path):
    """The plain call does what the headline needs and nothing else: one timed window of exactly `--steps` iterations, and
    `--dump-outputs` writes what those iterations computed -- K Adam iterations from the seeded initial state, whatever the
    wall-clock warm-up ran before them."""
    import numpy as np
    d = tmp_path / "out"
    out = _run_bench(["--steps", "24", "--warmup", "6", "--dump-outputs", str(d)])
    assert out["n_gpus"] == 1 and out["steps"] == 24 and out["warmup"] == 6 and out["value"] > 0
    assert out["metric"].startswith("variational-loss iterations/sec") and out["unit"] == "it/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and abs(out["ms_per_step"] * 1e-3 * out["value"] - 1.0) < 1e-9
    assert out["timing"]["windows"] == 1
    for k in ("roofline", "kernel_ms", "rel_l2_error", "cpu_baseline", "roofline_residual", "scaled_strong_64x64", "weak_scaling_probe"):
        assert k not in out, k
    params, state = np.load(d / "params.npy"), np.load(d / "optimizer_state.npy")
    assert params.dtype == np.float64 and state.dtype == np.float64 and params.shape == (921,) and state.shape == (3 * 921 + 2,)
    import bench
    from hp_vpinns_amd.drivers import poisson2d
    from hp_vpinns_amd.init import xavier_init
    theta = xavier_init(bench.LAYERS, 1234)
    m = poisson2d.build_model(poisson2d.setup(**bench.CFG4, with_test_grid=False), bench.LAYERS, var_form=1, init_params=theta)
    m._step(24, False)
    ref = m.get_params()
    assert np.max(np.abs(params - ref)) <= 1e-10 * np.max(np.abs(ref)), np.max(np.abs(params - ref))
    assert np.max(np.abs(params - theta)) > 1e-6                # (the steps did move the parameters)
    assert np.array_equal(state[:921], params)
