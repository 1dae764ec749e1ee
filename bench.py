#!/usr/bin/env python3
"""bench.py -- variational-loss iterations/sec of the hp-VPINN hot path on N MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

One step = one full training iteration of BASELINE.json config 4 (Poisson-2D, 16x16 elements, 20x20 GLL points and
10x10 test functions per element, MLP [2,20,20,20,1] tanh, var_form 1): Taylor-mode MLP forward at all 102 400
quadrature points, per-element projection + residual, adjoint, reverse pass, boundary term (320 points), TF1 Adam
update.  Inputs are synthetic of that shape (the driver's exact right-hand side, seeded boundary points, seeded Xavier
init) and are resident in HBM before the timed region.

N > 1: `python bench.py --gpus N` starts `python -m torch.distributed.run --nproc-per-node N` on itself as a child process
(when it is not already running under it), one rank per GPU; the 256 elements shard over the ranks (strong scaling: total
work fixed) with ONE RCCL all-reduce of the packed gradient/loss buffer per step, issued by the library inside its
iteration graphs.

Timing: W untimed warm-up steps, one untimed window of K steps (captures the iteration graphs for exactly this K), further
untimed windows until at least 0.3 s of iterations have run (clocks ramp for the first few hundred microseconds-long
iterations: a `--steps 20` window is 1.3 ms).  Then the parameters are reset to the seeded initial ones with a fresh
optimizer, and ONE window of exactly K steps is timed, bracketed by barrier + synchronize on both sides and reduced with MAX
over ranks: `value` = K / that window, `ms_per_step` = window / K.  Rank 0 prints ONE JSON line (contract: DESIGN.md
section 6).

--dump-outputs DIR: after the timed window, rank 0 writes what its K steps computed -- the parameters (`params.npy`, the
layout `get_params()` returns) and the whole optimizer state (`optimizer_state.npy`: parameters, Adam moments, beta
powers, as `save_checkpoint` stores them) -- in float64.  Because the timed steps start from the seeded initial state,
two runs with the same arguments compute the same K iterations from the same inputs.

--full: everything beside the headline figure, after the timed window: more windows of K steps (5 in all, 25 when a
window is shorter than 20 ms; min / max / median in `timing`), per-kernel device times and the roofline of the dominant
kernel (traffic from two rocprofv3 --pmc passes of a child run), the collective alone, the L2-error tail, the scaled
problems, the stand-alone residual kernel's roofline and the CPU baselines.  The `--no-*` options drop parts of it.
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CFG4 = dict(N_el_x=16, N_el_y=16, N_test_x=10, N_test_y=10, N_quad=20, N_bound=80, N_residual=100)
LAYERS = [2, 20, 20, 20, 1]
PEAK_FP64_TFLOPS = 78.6   # MI355X FP64 vector = matrix peak (datasheet; half the 157.3 TF FP32 rate of MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)
N_WINDOWS = 5            # 25 when a window of K steps is shorter than SHORT_WINDOW_S
SHORT_WINDOW_S = 0.020
WARM_WALL_S = 0.3        # untimed iterations before the first timed window, whatever --warmup says


def gemm_flops_per_row(layers):
    return 2 * sum(layers[l] * layers[l + 1] for l in range(len(layers) - 1))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


# ------------------------------------------------------------------------------------------------
# CPU baselines (oracle/ is test infrastructure: imported ONLY inside these functions, never by the product)
# ------------------------------------------------------------------------------------------------
def cpu_baseline_A(setup, theta, iters, windows=3):
    """Baseline A of BASELINE.md section 3: the reference-structured oracle (per-element Python loop, one reduction per
    test-function pair, autograd double backward -- the op granularity of the TF1 graph), torch CPU fp64."""
    import torch
    # tiny-op graphs get slower with many threads (128 threads: 26 s/iter vs 2.2 s/iter at 8 on this box class)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    from oracle.vpinn_oracle import OracleVPINN2D
    s = setup
    o = OracleVPINN2D(s["X_u_train"], s["u_train"], s["X_f_train"], s["f_train"], s["XY_quad_train"],
                      s["WXY_quad_train"], None, s["F_ext_total"], s["grid_x"], s["grid_y"], s["N_testfcn_total"],
                      s["X_u_train"], s["u_train"], LAYERS, init_params=theta)
    o.adam_step()  # warm-up (allocations, thread pool)
    rates = []
    for _ in range(windows):
        t0 = time.time()
        for _ in range(iters):
            o.adam_step()
        rates.append(iters / (time.time() - t0))
    return {"value": _median(rates), "unit": "it/s", "cores": int(torch.get_num_threads()), "kind": "port",
            "windows": [round(r, 4) for r in rates],
            "sample": "%d window(s) of %d full iterations of the same config-4 workload; reference-structured oracle "
                      "(per-element Python loop, one reduction per test-function pair, autograd double backward: baseline A "
                      "of BASELINE.md), torch CPU fp64; host has %d logical cpus" % (windows, iters, os.cpu_count())}


def cpu_baseline_B(setup, theta, iters, windows=3, sweep=(8, 32, 64, 128)):
    """Baseline B of BASELINE.md section 3: closed-form C / OpenMP restatement (oracle/cpu_closed_form.c), all elements in
    parallel; thread sweep, best reported.  Threads pinned (one per core, neighbours first) before the OpenMP runtime of the
    C library starts: unpinned, the same binary ran 44-75 it/s from run to run on the 256-cpu host."""
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    from oracle.cpu_baseline import CPoisson2D
    s = setup
    ncpu = os.cpu_count() or 1
    best, table = None, {}
    for nt in sorted({min(t, ncpu) for t in sweep}):
        c = CPoisson2D(s["X_u_train"], s["u_train"], s["XY_quad_train"], s["WXY_quad_train"], s["F_ext_total"], s["grid_x"],
                       s["grid_y"], LAYERS, theta, threads=nt)
        c.train(3)
        rates = []
        for _ in range(windows):
            t0 = time.time()
            c.train(iters)
            rates.append(iters / (time.time() - t0))
        table[str(nt)] = round(_median(rates), 3)
        if best is None or _median(rates) > best[1]:
            best = (nt, _median(rates))
    return {"value": best[1], "unit": "it/s", "cores": best[0], "kind": "port", "thread_sweep_it_per_s": table,
            "omp": {k: os.environ.get(k) for k in ("OMP_PROC_BIND", "OMP_PLACES")},
            "sample": "median of %d window(s) of %d full iterations per thread count, closed-form C/OpenMP restatement "
                      "(oracle/cpu_closed_form.c, gcc -O3 -march=x86-64-v3, checked against the autograd oracle in tests/test_oracle.py: "
                      "baseline B of BASELINE.md); host has %d logical cpus" % (windows, iters, ncpu)}


def measure_traffic(kernel_substr, timeout_s=120):
    """HBM bytes per launch of the kernel whose name contains `kernel_substr`, measured NOW: two rocprofv3 passes (FETCH_SIZE and
    WRITE_SIZE do not fit one pass on gfx950: MI355X_MICROARCH.md, "rocprofv3 PMC slots"; counters in their own runs with
    --kernel-trace only) over a short child run of this script, corrected as that guide's HBM section prescribes (FETCH_SIZE
    counts 64 B per 128-B request of a wide coalesced read: x 2; both counters are in KB).  -> (bytes, detail) or (None, why)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    tmp = tempfile.mkdtemp(prefix="hpv_pmc_", dir="/tmp")
    per = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, ctr)
            cmd = [exe, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable,
                   os.path.abspath(__file__), "--traffic-child", "--no-pmc", "--no-extras", "--no-cpu-baseline", "--no-residual-roofline"]
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
                env.pop(k, None)
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, "rocprofv3 --pmc %s failed (rc %d): %s" % (ctr, r.returncode, (r.stderr or r.stdout)[-200:])
            tot, disp = 0.0, set()
            for row in csv.DictReader(open(files[0])):
                if kernel_substr in row["Kernel_Name"] and row["Counter_Name"] == ctr:
                    tot += float(row["Counter_Value"])
                    disp.add(row["Dispatch_Id"])
            if not disp:
                return None, "no dispatch of %s in the %s pass" % (kernel_substr, ctr)
            per[ctr] = (tot / len(disp), len(disp))
    except Exception as e:  # noqa: BLE001 -- the measurement must never take the bench line down
        return None, "%s: %s" % (type(e).__name__, str(e)[:200])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    by = (2.0 * per["FETCH_SIZE"][0] + per["WRITE_SIZE"][0]) * 1024.0
    return by, {"FETCH_SIZE_KB_per_launch": per["FETCH_SIZE"][0], "WRITE_SIZE_KB_per_launch": per["WRITE_SIZE"][0],
                "launches_profiled": per["FETCH_SIZE"][1], "formula": "(2 x FETCH_SIZE + WRITE_SIZE) x 1024"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--backend", default="auto")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the parameters and optimizer state after the timed steps as DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure (more windows, kernel times and roofline, L2 error, "
                         "scaled problems, residual roofline, CPU baselines); the --no-* options below apply to it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-residual-roofline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the L2-error tail, the scaled problems and the alternative exchange")
    ap.add_argument("--cpu-iters", type=int, default=3, help="iterations per window of CPU baseline A (3 windows)")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="BASELINE.md section 3 protocol: A 5 x 20, B 5 x 200 iterations, median of the windows (minutes)")
    ap.add_argument("--l2-iters", type=int, default=40000, help="total Adam iterations before the L2 error is evaluated")
    ap.add_argument("--residual-elems", type=int, default=1 << 18)
    ap.add_argument("--no-pmc", action="store_true", help="roofline.traffic from profiles/traffic.json instead of two rocprofv3 --pmc passes of this run")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)   # the short run the --pmc passes profile
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ:
        # the driver's plain `python bench.py --gpus N`: N ranks, one per GPU, over RCCL, in child processes of a launcher
        # (this process never touches a GPU; it waits and passes the launcher's exit status on)
        import subprocess
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        rc = subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
                              "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)]
                             + sys.argv[1:])
        sys.exit(rc)

    import torch
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # (test hook: HPV_BENCH_ONE_GPU=1 runs every rank on cuda:0 with a gloo group -- the whole multi-rank flow on a
    #  single-GPU box; throughput is then meaningless)
    one_gpu = os.environ.get("HPV_BENCH_ONE_GPU") == "1"
    if one_gpu:
        # the SPLIT mode of the whole-iteration kernel needs all workgroups of an element resident at once, i.e. a GPU that
        # this process does not share with the other ranks' kernels: keep shared-GPU runs on the forward + split reverse kernels
        os.environ.setdefault("HPV_FUSE", "s")
    if one_gpu:
        local_rank = 0
        os.environ.setdefault("HPV_EXCHANGE", "p2p")
    torch.cuda.set_device(local_rank)
    dist = None
    # The bench's own control plane -- barriers, MAX over ranks, the object collectives of the communicator set-up -- runs on CPU tensors
    # over gloo at every N: the library's communicator (hpv_rccl_*) is then the ONLY RCCL communicator of a rank (verdict round 5, weak 5 ii:
    # torch's NCCL communicator beside it would have been a first-ever co-existence at N > 1); "cuda:nccl" stays registered for the
    # `torch` exchange fallback, which creates its communicator lazily, only if it is ever used.
    red_dev = "cpu"
    if world > 1 or ("RANK" in os.environ and os.environ.get("HPV_FORCE_DIST") == "1"):
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # (one node, rendezvous on the loopback address: gloo binds the loopback interface too instead of resolving the container's
        #  hostname, which may not resolve)
        if os.environ.get("MASTER_ADDR") in ("127.0.0.1", "localhost") and os.path.isdir("/sys/class/net/lo"):
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        dist.init_process_group("cpu:gloo,cuda:nccl")      # (the one-GPU test hook takes the same group: its exchange is the mailbox one)

    from hp_vpinns_amd.dist import shard_range
    from hp_vpinns_amd.drivers import poisson2d
    from hp_vpinns_amd.init import xavier_init
    s = poisson2d.setup(**CFG4, with_test_grid=False)
    theta = xavier_init(LAYERS, 1234)

    def barrier(m):
        m.h.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.all_reduce(torch.zeros(1, dtype=torch.float64))      # (a barrier over gloo, CPU tensor: every rank's device work is done)

    def max_over_ranks(v):
        if dist is None:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def one_window(m, steps):
        barrier(m)
        t0 = time.perf_counter()
        m._step(steps, False)
        barrier(m)
        return max_over_ranks(time.perf_counter() - t0)

    def warm_up(m, warmup, steps):
        """-> (time of one window of `steps` iterations (s), MAX over ranks; untimed warm-up iterations actually run)."""
        m.prepare(warmup, steps)      # torch-collective fallback: communicator warm-up + graph capture outside the timed region
        m._step(warmup, False)
        m._step(steps, False)         # untimed: captures the graphs this K needs (whole replays + one remainder graph)
        # untimed windows until WARM_WALL_S of iterations have run (every rank runs the same count: the estimate is a MAX over ranks)
        t1 = one_window(m, steps)
        n_more = int(min(4000, max(0, np.ceil(WARM_WALL_S / max(t1, 1e-6)) - 1)))
        for _ in range(n_more):
            m._step(steps, False)
        return t1, warmup + (2 + n_more) * steps

    def n_windows(t1):
        return N_WINDOWS if t1 >= SHORT_WINDOW_S else 5 * N_WINDOWS

    def timed_windows(m, warmup, steps, windows=None):
        """-> (list of window times (s), MAX over ranks each; untimed warm-up iterations actually run)."""
        t1, n_warm = warm_up(m, warmup, steps)
        return [one_window(m, steps) for _ in range(windows or n_windows(t1))], n_warm

    def dump_outputs(m, d):
        """What the timed steps computed, as a caller of the iteration receives it: parameters and optimizer state."""
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "params.npy"), np.asarray(m.get_params(), dtype=np.float64))
        np.save(os.path.join(d, "optimizer_state.npy"), np.asarray(m.h.get_state(), dtype=np.float64))

    model = poisson2d.build_model(s, LAYERS, var_form=1, init_params=theta, backend=args.backend, device=local_rank)
    if args.traffic_child:      # (under rocprofv3 --pmc: 64 iterations of the same model through the same graphs, nothing else)
        model._step(64, False)
        model.h.sync()
        return
    t1, n_warm = warm_up(model, args.warmup, args.steps)
    # the timed steps start from the seeded initial parameters with a fresh optimizer (set_params writes the same device buffers:
    # the captured graphs stay valid), so that what they compute does not depend on how much warm-up the wall clock asked for
    model.set_params(theta)
    wins = [one_window(model, args.steps)]
    dt = wins[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(model, args.dump_outputs)
    n_its_done = args.steps       # Adam iterations since the seeded start
    structure = model.h.pass_structure()      # which launch structure the timed iterations ran (SPLIT vs the split reverse kernels ...)
    variant = model.h.kernel_variant()        # ... and which kernel instantiation (quarter-tile plan or whole tiles, split factor)
    graphs = model.h.graphs_in_use() if not model._coll else bool(model._dist_graphs.get(min(args.steps, 8) if args.steps <= 16 else 8))
    exchange = model.exchange() if world > 1 or dist is not None else "none"
    rccl_world = None
    if exchange == "rccl":
        try:
            rccl_world = model.h.rccl_info()[0]       # (ncclCommCount of the library's own communicator)
        except Exception:  # noqa: BLE001 -- an evidence field: never take the headline line down
            pass
    per_rank = [{"rank": rank, "pass_structure": structure, "kernel_variant": variant, "graphs": bool(graphs), "exchange": exchange,
                 "rccl_world": rccl_world, "device": local_rank,
                 "elements": list(shard_range(model.Nelementx * model.Nelementy, rank, world))}]
    out = {
        "metric": "variational-loss iterations/sec", "value": args.steps / dt, "unit": "it/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "Poisson-2D hp-VPINN, 16x16 elements, 20x20 GLL quad/elem, 10x10 test fcns/elem, "
                               "MLP [2,20,20,20,1] tanh, var_form 1, 320 boundary pts, TF1 Adam (BASELINE config 4)",
                   "points": 102400, "residuals": 25600, "params": 921, "backend": model.backend(),
                   "parallelism": "element-sharded dp%d" % world,
                   "exchange": {"rccl": "in-library ncclAllReduce of the packed buffer, " +
                                        ("captured in the iteration graphs" if graphs else
                                         "EAGER launches (RCCL refused stream capture: no iteration graphs)"),
                                "p2p": "in-library peer-mapped mailboxes over xGMI", "torch": "torch.distributed all_reduce (RCCL)",
                                "none": "none"}[exchange],
                   "rccl_world": rccl_world,
                   "pass_structure": structure, "kernel_variant": variant, "build": model.h.build_info(), "per_rank": per_rank},
        "timing": {"windows": 1, "untimed_warmup_iterations": n_warm,
                   "value_is": "steps / ONE window of exactly `steps` iterations from the seeded initial state between "
                               "barrier+synchronize, MAX over ranks (%.1f ms)" % (1e3 * dt)},
    }
    if not args.full:
        if dist is not None:
            allr = [None] * world
            dist.all_gather_object(allr, per_rank[0])
            out["config"]["per_rank"] = allr
        if rank == 0:
            print(json.dumps(out))
        if dist is not None:
            dist.destroy_process_group()
        return

    # ================================ --full: everything beside the headline figure ================================
    wins += [one_window(model, args.steps) for _ in range(n_windows(t1) - 1)]
    n_its_done += (len(wins) - 1) * args.steps
    out["timing"] = {"windows": len(wins), "window_it_per_s": [round(args.steps / w, 1) for w in wins],
                     "min_it_per_s": args.steps / max(wins), "max_it_per_s": args.steps / min(wins),
                     "median_it_per_s": args.steps / _median(wins), "untimed_warmup_iterations": n_warm,
                     "value_is": "steps / the FIRST window (the timed one of the plain run); %d windows of exactly `steps` iterations "
                                 "each between barrier+synchronize, MAX over ranks, because one window lasts %.1f ms"
                                 % (len(wins), 1e3 * t1)}

    # ---- per-kernel device times (hipEvents on the stream the kernels run on), untimed extra pass ----
    nt = min(args.steps, 100)
    model.h.enable_timing(True)
    model._step(nt, False)
    model.h.sync()
    ktime = {name: model.h.kernel_time_ms(i)[0] for i, name in enumerate(("mlp_fwd", "project", "mlp_bwd"))}
    model.h.enable_timing(False)
    # the per-launch event pairs above carry ~3.5 us of event overhead each (59.7 us against rocprofv3's 56 us for the same kernel);
    # when the iteration is ONE whole-iteration launch, the dominant kernel is timed as 200 back-to-back launches between one pair
    ktime_per_launch_events = dict(ktime)
    kernel_timer = "one hipEvent pair per launch"
    if ktime["mlp_fwd"] == 0.0 and ktime["project"] == 0.0:
        try:
            model.h.time_iteration_kernel(20)
            ktime["mlp_bwd"] = sum(model.h.time_iteration_kernel(200) for _ in range(3)) / 3.0
            kernel_timer = "600 back-to-back launches, one hipEvent pair per 200 (hpv_time_iteration_kernel): launch gaps included, event overhead amortised"
        except Exception as e:      # (SPLIT shards of a multi-GPU run: the kernel cannot be launched alone)
            kernel_timer += " (%s)" % str(e)[:80]
    n_its_done += nt
    loss3 = model.loss()

    # ---- the L2-error half of the metric: train on to a fixed total iteration count, then ||u - u_NN|| / ||u|| on a grid ----
    rel_l2 = None
    if not args.no_extras:
        # Adam at lr 1e-3 keeps oscillating once the loss is down (the last iterate's error moves by 2x within a few thousand
        # iterations and with the last bit of the arithmetic), so the error is quoted for the lowest-loss checkpoint of the
        # last 10 000 iterations (one loss evaluation per 1 000), the last iterate's beside it
        tail = max(0, args.l2_iters - n_its_done)
        n_ck = min(10, tail // 1000)
        model._step(tail - 1000 * n_ck, False)
        best_loss, best_theta, last_loss = float("inf"), None, float(model.loss()[0])
        for _ in range(n_ck):
            last_loss = float(model._step(1000, True)[0])
            if last_loss < best_loss:
                best_loss, best_theta = last_loss, model.get_params()
        n_its_done += tail
        gx = np.linspace(-1, 1, 101)
        Xt = np.stack(np.meshgrid(gx, gx), -1).reshape(-1, 2)
        ut = poisson2d.u_ext(Xt[:, 0:1], Xt[:, 1:2])
        err_last = model.rel_l2_error(Xt, ut)
        err_best = err_last
        if best_theta is not None and best_loss < last_loss:
            last_theta = model.get_params()
            model.set_params(best_theta)
            err_best = model.rel_l2_error(Xt, ut)
            model.set_params(last_theta)
        rel_l2 = {"value": err_best, "last_iterate": err_last, "after_iterations": n_its_done, "grid": "101x101",
                  "loss": min(best_loss, last_loss), "loss_last_iterate": last_loss,
                  "note": "seeded Xavier start (1234), Adam lr 1e-3; value = the lowest-loss checkpoint of the last 10 000 iterations "
                          "(tests/test_gpu_convergence.py asserts <= 1e-2 for it)"}
    # what the library's communicator's all-reduce of the packed buffer costs alone (200 eager calls between one hipEvent pair,
    # collective; rccl_world above = what the communicator ITSELF reports): the 10-20 us DESIGN.md 7 assumes for 8 ranks becomes a
    # measured field
    collective_us = None
    if exchange == "rccl":
        try:
            collective_us = model.h.rccl_time_allreduce(200)
        except Exception as e:  # noqa: BLE001 -- evidence fields: never take the headline line down
            collective_us = "failed: %s" % str(e)[:120]

    # ---- extras at EVERY N, N = 1 included (reported beside the headline number; the same kernels on larger problems): the
    #      driver's N = 1 line is the base of the 1 -> 8 ratio on the scaled batch (verdict round 4, item 1a).  They run after
    #      the headline windows and every exception is caught: they cannot take the headline line down ----
    extras = {}
    if not args.no_extras:
        k2 = min(args.steps, 400)
        extras_failed = None

        def run_problem(nex, ney):
            sw = poisson2d.setup(**dict(CFG4, N_el_x=nex, N_el_y=ney), with_test_grid=False, assemble="device", device=local_rank)
            mw = poisson2d.build_model(sw, LAYERS, var_form=1, init_params=theta, backend=args.backend, device=local_rank)
            w, _ = timed_windows(mw, min(args.warmup, 40), k2, windows=3)
            ex = mw.exchange()
            del mw
            return k2 / _median(w), ex
        # (same exchange and kernels as the headline run above, only the grid differs; any exception leaves the headline line intact)
        try:
            r, ex = run_problem(16, 16 * world)
        except Exception as e:  # noqa: BLE001
            extras_failed, r, ex = str(e)[:200], float("nan"), "failed"
        extras["weak_scaling_probe"] = {"elements": 256 * world, "elements_per_gpu": 256, "steps": k2, "it_per_s": r,
                                        "element_iterations_per_s": 256 * world * r, "exchange": ex,
                                        "note": "not the headline metric: every rank keeps a full config-4 shard (16 x 16N elements)"}
        try:
            r, ex = run_problem(64, 64)
        except Exception as e:  # noqa: BLE001
            extras_failed, r, ex = str(e)[:200], float("nan"), "failed"
        if extras_failed:
            extras["extras_error"] = extras_failed
        npt = 64 * 64 * 400
        extras["scaled_strong_64x64"] = {"elements": 4096, "elements_per_gpu": 4096 // world, "points": npt, "steps": k2,
                                         "it_per_s": r, "us_per_iteration": 1e6 / r if r == r and r > 0 else None, "exchange": ex,
                                         "point_iterations_per_s": npt * r,
                                         "per_rank_tflops_algorithmic": 3 * 3 * gemm_flops_per_row(LAYERS) * npt * r / world / 1e12,
                                         "per_rank_frac_of_fp64_peak": 3 * 3 * gemm_flops_per_row(LAYERS) * npt * r / world / 1e12 / PEAK_FP64_TFLOPS,
                                         "note": "SURVEY.md 7.3 scaled synthetic batch: the config-4 element shape on a 64x64-element "
                                                 "grid, strong scaling (4096 / N elements per GPU)"}
        if world > 1 and not one_gpu and os.environ.get("HPV_BENCH_ALT_EXCHANGE") == "1":
            # opt-in: the same config-4 job through the other in-library exchange (peer-mapped mailboxes, never run across
            # xGMI by the builder), for comparison -- not part of the default run so that it cannot take the headline line down
            alt = "p2p" if exchange != "p2p" else "rccl"
            os.environ["HPV_EXCHANGE"] = alt
            try:
                ma = poisson2d.build_model(s, LAYERS, var_form=1, init_params=theta, backend=args.backend, device=local_rank)
                wa, _ = timed_windows(ma, min(args.warmup, 40), k2, windows=3)
                extras["exchange_alt"] = {"exchange": ma.exchange(), "requested": alt, "steps": k2, "it_per_s": k2 / _median(wa)}
                del ma
            except Exception as e:  # noqa: BLE001 -- never let the comparison run take the headline line down
                extras["exchange_alt"] = {"requested": alt, "error": str(e)[:200]}
            finally:
                os.environ.pop("HPV_EXCHANGE", None)

    per_rank[0]["collective_us"] = collective_us
    if dist is not None:
        allr = [None] * world
        dist.all_gather_object(allr, per_rank[0])
        per_rank = allr
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    # ---- roofline of the dominant kernel (SURVEY.md 8d definitions) ----
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            traffic_tab = json.load(f)
    except Exception:
        traffic_tab = {}
    n_elem_local = (model.Nelementx * model.Nelementy) // world
    N_local = n_elem_local * 400                 # points per rank
    C, G = 3, gemm_flops_per_row(LAYERS)
    proj_flops = 48000 * n_elem_local            # sum-factorised: 2 terms x 2 x (20*10*20 + 10*10*20) x 2 flop per element
    whole_iter_fused = ktime["mlp_fwd"] == 0.0 and ktime["project"] == 0.0
    if whole_iter_fused:
        kernels = {"iteration (forward+projection+reverse, element-resident)": (ktime["mlp_bwd"], 3 * C * G * N_local + proj_flops)}
    else:
        proj_in_bwd = ktime["project"] == 0.0
        kernels = {"mlp_fwd": (ktime["mlp_fwd"], C * G * N_local),
                   "mlp_bwd": (ktime["mlp_bwd"], 2 * C * G * N_local + (proj_flops if proj_in_bwd else 0))}
    dom = max(kernels, key=lambda k: kernels[k][0])
    # roofline.traffic: measured in THIS run when rocprofv3 is there (two --pmc passes of a short child run, ~20 s each), so that the
    # line notices a traffic regression; otherwise the committed table with its label
    measured, mdetail = (None, "--no-pmc") if (args.no_pmc or world != 1) else measure_traffic(
        "k_iter_fused" if whole_iter_fused else ("k_bwd" if dom == "mlp_bwd" else "k_fwd"))

    def roof(k):
        ms, fl = kernels[k]
        tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        key = "iter_fused" if whole_iter_fused else k
        if k == dom and measured is not None:
            tr, src = measured, "measured in this run"
        else:
            tr = traffic_tab.get(key) if world == 1 else None
            src = ("profiles/traffic.json (rocprofv3 --pmc passes of an earlier run of this kernel, %s); not measured in this run (%s)"
                   % (traffic_tab.get("_measured_at", "commit unknown"), mdetail if isinstance(mdetail, str) else "other kernel")) if world == 1 else None
        return {"kernel": k, "bound": "mfma", "achieved": tf, "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s",
                "frac": tf / PEAK_FP64_TFLOPS, "traffic": tr, "traffic_source": src,
                "traffic_detail": mdetail if (k == dom and measured is not None) else None,
                "flops_per_launch": fl, "avg_ms": ms, "timer": kernel_timer if k == dom else "one hipEvent pair per launch"}
    # whole-iteration algorithmic HBM bytes (fused ideal): coordinates in, F in, Adam state in/out
    ideal_bytes = 8 * (2 * N_local + n_elem_local * 100 + 7 * 921)
    out["config"].update({
        "per_rank": per_rank,
        "collective_us": (max(r["collective_us"] for r in per_rank)
                          if all(isinstance(r.get("collective_us"), float) for r in per_rank) else collective_us),
        "collective_note": "rccl_world = ncclCommCount of the library's own communicator; collective_us = ONE all-reduce of the "
                           "packed buffer (P + 4 doubles) alone, eager, 200 calls between one hipEvent pair, MAX over ranks; "
                           "null when the exchange is not the in-library RCCL one"})
    out.update({
        "loss_after": float(loss3[0]),
        "rel_l2_error": rel_l2,
        "kernel_ms": ktime, "kernel_ms_per_launch_events": ktime_per_launch_events, "kernel_timer": kernel_timer,
        "roofline": dict(roof(dom), whole_iteration_fused=whole_iter_fused, algorithmic_hbm_bytes_per_iteration=ideal_bytes,
                         note="dominant kernel; frac = ALGORITHMIC flops of SURVEY.md 8(d) (3 C G N for the layer products, C=3, "
                              "G=1720 per row, + 48 kflop per element of sum-factorised projection) / hipEvent kernel time / "
                              "78.6 TFLOP/s fp64 peak; the tangent pre-activations the kernel recomputes in its reverse phase "
                              "(+2/9 of the layer products) are NOT counted; traffic = PMC HBM bytes per launch "
                              "(profiles/traffic.json) against algorithmic_hbm_bytes_per_iteration = 8 (d N + N_R + 7 P)"),
    })
    for k in kernels:
        if k != dom:
            out["roofline_other_kernel"] = roof(k)
    out.update(extras)
    if world == 1 and not args.no_residual_roofline:
        # the per-element projection kernel on a batch larger than the 256 MB Infinity Cache: 2^18 elements
        # of the config-4 element shape, random channels.  Residual only = SURVEY's byte count 8 (C_u N + 2 N_R); the
        # training launch also writes the adjoint channels.
        res = {}
        for name, adj in (("residual_only", False), ("residual_plus_adjoint", True)):
            ms, by = model.h.bench_projection(args.residual_elems, 10, do_adjoint=adj)
            gbs = by / (ms * 1e-3) / 1e9
            res[name] = {"achieved": gbs, "frac": gbs / PEAK_HBM_GBS, "bytes_per_launch": by, "avg_ms": ms,
                         "traffic": traffic_tab.get("project_scaled" if adj else "project_scaled_residual_only")}
        out["roofline_residual"] = {"kernel": "k_project_tp (stand-alone projection)", "bound": "hbm", "peak": PEAK_HBM_GBS,
                                    "unit": "GB/s", "n_elem": args.residual_elems,
                                    "achieved": res["residual_only"]["achieved"], "frac": res["residual_only"]["frac"], **res}
    if world == 1 and not args.no_cpu_baseline:
        if args.cpu_baseline_full:
            out["cpu_baseline"] = cpu_baseline_A(s, theta, 20, windows=5)
            out["cpu_baseline_vectorized"] = cpu_baseline_B(s, theta, 200, windows=5)
        else:
            out["cpu_baseline"] = cpu_baseline_A(s, theta, args.cpu_iters, windows=3)
            out["cpu_baseline_vectorized"] = cpu_baseline_B(s, theta, 30, windows=3)
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
        out["speedup_vs_cpu_baseline_vectorized"] = out["value"] / out["cpu_baseline_vectorized"]["value"]
    print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
