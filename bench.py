#!/usr/bin/env python3
"""bench.py — driver-contract benchmark: gradient updates/sec (whole node).

``python bench.py --gpus N --steps K --warmup W [--model M] [--full]
[--dump-outputs DIR]``

A *step* is one applied gradient update at the parameter server (the
reference's iteration ``k``, SparkASGDThread.scala:199). W warmup updates run
untimed, then EXACTLY K updates are timed (wall stamps taken by the
single-writer server), bracketed by barrier + torch.cuda.synchronize on both
sides; rank 0 prints ONE JSON line; value = whole-node updates/sec.

Default model = BASELINE config 2: ASGD on synthetic mnist8m-shape
(8.1M x 784 dense bf16, b=0.01, tau=20M, random-init weights). The dataset
stays FIXED as N grows (sharded over ranks) => strong scaling, matching the
reference's fixed-dataset/more-partitions semantics. The other BASELINE
configs (1,3,4,5) are selectable via --model (single-node; N>1 supports the
flagship ASGD/ASAGA models, dense and CSR).

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print the result line. ``--full`` additionally measures the
BASELINE metric's second clause (wall-clock-to-target-loss: an objective
sweep of the optVars snapshots over the whole dataset after the run);
without it ``config.wall_clock_to_target_loss`` is null. ``--dump-outputs
DIR`` writes what the timed path returned to its caller (final weights
``w.npy`` and, where the path records them, the optVars weight snapshots
``opt_vars.npy``) as float32 .npy files after the timed steps; inputs are
seeded, so two builds can be compared output for output (the engines are
asynchronous, so outputs agree to optimisation noise, not bitwise).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from asyncframework_amd import run as runner
from asyncframework_amd.data.shard import row_shards
from asyncframework_amd.data.synthetic import synthetic_csr, synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.local import AsyncEngine, SyncEngine
from asyncframework_amd.engine.server import Server
from asyncframework_amd.engine.worker import Shard, Worker

BASE = dict(taw=20_000_000, gamma=1.5625e-3, bucket_ratio=0.7, seed=42)

MODELS = {
    # BASELINE.json configs. config 1 is the CPU plumbing check.
    "sync-tiny-cpu": dict(rows=1_000, cols=784, rate=0.3, algo="asgd",
                          sync=True, dtype="fp32", sparse=False,
                          engine="threads", device="cpu", workers=2,
                          objective="logistic"),  # BASELINE config 1 names
                                                  # logistic regression
    # flagship: 32 async workers (the reference's fixed partitions=32,
    # README.md) on the native C++ engine: wave dispatch + event-free
    # pinned-host completion + batched fused updates — 188-191k updates/s
    # fresh-box validated (profiles/r02_wave_dispatch.md). --engine
    # resident runs the same config inside ONE persistent HIP kernel
    # (77.2k: zero host API calls, but the reference's avail>=gate quorum
    # turns its static-partition round latency into idle —
    # profiles/r02_resident_profile.md); --engine graph = 1-worker hipGraph
    "asgd-mnist8m": dict(rows=8_100_000, cols=784, rate=0.01, algo="asgd",
                         sync=False, dtype="bf16", sparse=False,
                         engine="native", workers=32),
    "asaga-rcv1": dict(rows=697_641, cols=47_236, rate=0.02, algo="asaga",
                       sync=False, dtype="fp32", sparse=True,
                       engine="native", workers=32),
    "asgd-epsilon-delay": dict(rows=400_000, cols=2_000, rate=0.01,
                               algo="asgd", sync=False, dtype="fp32",
                               sparse=False, engine="native",
                               delay_coeff=1.0, workers=8),
    "asaga-mnist8m-hostspill": dict(rows=8_100_000, cols=784, rate=0.01,
                                    algo="asaga", sync=False, dtype="bf16",
                                    sparse=False, engine="native",
                                    history="host", workers=32),
}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="asgd-mnist8m", choices=list(MODELS))
    p.add_argument("--gpus", type=int, default=1)
    # defaults sized so the timed region is >=0.15 s at the flagship's
    # measured ~190k updates/s (a 2000-step region was ~10 ms — too noisy)
    p.add_argument("--steps", type=int, default=30000)
    p.add_argument("--warmup", type=int, default=3000)
    p.add_argument("--rows", type=int, default=0)
    p.add_argument("--cols", type=int, default=0)
    p.add_argument("--rate", type=float, default=0.0)
    p.add_argument("--dtype", default="", choices=["", "bf16", "fp32"])
    p.add_argument("--objective", default="",
                   choices=["", "lsq", "logistic"])
    p.add_argument("--algo", default="", choices=["", "asgd", "asaga"])
    p.add_argument("--device", default=None, help="override (cpu for debug)")
    p.add_argument("--engine", default="",
                   choices=["", "graph", "threads", "native", "resident"])
    p.add_argument("--workers", type=int, default=0,
                   help="logical workers (threads/native engines)")
    p.add_argument("--dist-engine", default="",
                   choices=["", "python", "native"],
                   help="N>1 control plane: python (default) or the C++ "
                        "server (also via ASYNCAMD_DIST_ENGINE=native)")
    p.add_argument("--full", action="store_true",
                   help="also measure everything beyond the headline "
                        "figure (wall-clock-to-target-loss objective "
                        "sweep); off by default")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="write the timed path's outputs (final weights, "
                        "optVars snapshots) as DIR/<name>.npy")
    args = p.parse_args()
    # marks record at exact post-increment update counts, so k=0 is
    # unreachable: clamp to >=1 warmup step (negligible) rather than fail
    # if a caller passes --warmup 0; likewise a 1-step timed region is
    # meaningless — keep at least 2
    args.warmup = max(1, args.warmup)
    args.steps = max(2, args.steps)
    preset = MODELS[args.model]
    args.rows = args.rows or preset["rows"]
    args.cols = args.cols or preset["cols"]
    args.rate = args.rate or preset["rate"]
    args.dtype = args.dtype or preset["dtype"]
    args.algo = args.algo or preset["algo"]
    args.objective = args.objective or preset.get("objective", "lsq")
    args.engine = args.engine or preset["engine"]
    if args.device is None and "device" in preset:
        args.device = preset["device"]
    args.sparse = preset.get("sparse", False)
    args.sync = preset.get("sync", False)
    args.delay_coeff = preset.get("delay_coeff", 0.0)
    args.history = preset.get("history", "device")
    args.preset_workers = args.workers or preset.get("workers", 0)
    return args


def make_cfg(args, num_workers, device):
    return EngineConfig(
        d=args.cols, N=args.rows, num_workers=num_workers,
        num_iterations=args.warmup + args.steps + 1,
        gamma=BASE["gamma"], taw=BASE["taw"], batch_rate=args.rate,
        bucket_ratio=BASE["bucket_ratio"], printer_freq=1 << 30,
        delay_coeff=args.delay_coeff, seed=BASE["seed"], algo=args.algo,
        sync=args.sync, objective=args.objective, dtype=args.dtype,
        device=str(device), history_placement=args.history,
        calib_factor=10 if args.delay_coeff else 100,
        snapshot_weights=False)


def snap_cadence(args) -> int:
    """optVars snapshot cadence for the to-target clause: <=40 snapshots
    over the whole run (3 KB D2D copy each — negligible in the timed
    region), floor 100 so short debug runs stay cheap."""
    return max(100, (args.warmup + args.steps) // 40)


def to_target_summary(args, data, opt_vars, target_frac: float = 0.5):
    """BASELINE metric second clause, measured in-run: wall-clock (ms from
    run start) until the objective first reaches target_frac x initial
    objective, from the optVars snapshot ring (the reference's loss-curve
    mechanism, SparkASGDThread.scala:389-404: snapshot during the run,
    objective swept once at the end)."""
    if not opt_vars or len(opt_vars) < 2:
        return None
    from asyncframework_amd.ops.torch_ref import (objective_sweep,
                                                  objective_sweep_csr)
    W = torch.stack([w.float() for _, w in opt_vars])
    if args.sparse:
        indptr, indices, values, y = data
        W = W.to(indptr.device)
        obj = objective_sweep_csr(indptr, indices, values, y, W,
                                  args.objective)
    else:
        X, y = data
        W = W.to(X.device)
        obj = objective_sweep(X, y, W, args.objective)
    obj = [float(o) for o in obj.cpu()]
    o0 = obj[0]
    target = o0 * target_frac
    ms = next((t for (t, _), o in zip(opt_vars, obj) if o <= target), None)
    # always-defined convergence-speed clause: wall ms until the run first
    # covered 95% of the objective progress it achieved (short benches at
    # the reference's production gamma never reach 0.5*obj0)
    best = min(obj)
    t95 = o0 - 0.95 * (o0 - best)
    ms95 = next((t for (t, _), o in zip(opt_vars, obj) if o <= t95), None)
    return {"target_frac": target_frac, "obj_initial": round(o0, 6),
            "obj_final": round(obj[-1], 6),
            "target_loss": round(target, 6), "ms_to_target": ms,
            "ms_to_95pct_of_achieved_progress": ms95,
            "n_snapshots": len(obj)}


DUMP_BUDGET_BYTES = 64 << 20  # cap on everything --dump-outputs writes


def _sample_to_budget(a: np.ndarray, budget: int) -> np.ndarray:
    """Whole array if it fits the byte budget, else a fixed seeded sample
    of its elements (same indices every run, so dumps stay comparable)."""
    if a.nbytes <= budget:
        return a
    n = max(1, budget // a.itemsize)
    idx = np.sort(np.random.default_rng(0).choice(a.size, n, replace=False))
    return a.reshape(-1)[idx]


def dump_outputs(args, w, opt_vars=None) -> None:
    """--dump-outputs: what the timed path handed back after its last step
    — the final weight vector and, where recorded, the optVars weight
    snapshots — as float32 .npy files (snapshot wall stamps are timing,
    not output, and are left out)."""
    if not args.dump_outputs:
        return
    os.makedirs(args.dump_outputs, exist_ok=True)
    arrays = {"w": w.detach().float().cpu().numpy()}
    if opt_vars:
        arrays["opt_vars"] = torch.stack(
            [v.detach().float().cpu() for _, v in opt_vars]).numpy()
    budget = DUMP_BUDGET_BYTES // len(arrays)
    for name, a in arrays.items():
        np.save(os.path.join(args.dump_outputs, name + ".npy"),
                _sample_to_budget(np.ascontiguousarray(a, np.float32),
                                  budget))


def emit(args, cfg, elapsed: float, n_gpus: int, to_target=None):
    ups = args.steps / elapsed
    out = {
        "metric": "gradient updates/sec (whole node)",
        "value": round(ups, 2),
        "unit": "updates/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed * 1000.0 / args.steps, 6),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic",
        "config": {
            "model": args.model,
            "algo": args.algo, "objective": args.objective,
            "rows": args.rows, "cols": args.cols,
            "batch_rate": args.rate, "taw": cfg.taw,
            "gamma": cfg.gamma, "bucket_ratio": cfg.bucket_ratio,
            "global_batch": int(args.rate * args.rows),
            "seq_len": args.cols,
            "parallelism": ("sync" if args.sync else "async-ps") +
                           f"-dp{n_gpus}-w{cfg.num_workers}",
            # BASELINE.json's metric second clause, measured IN THIS RUN
            # from the optVars snapshot ring under --full (None in a plain
            # run and where a path has no snapshot support, e.g. N>1
            # rank-sharded data):
            "wall_clock_to_target_loss": to_target,
        },
    }
    print(json.dumps(out))


def run_single(args, device):
    """One process (N=1): graph engine (device-resident loop) or the
    threaded mailbox engine (delay injection / host-spill / sync / CPU)."""
    n_workers = args.preset_workers or 1
    if args.engine == "graph":
        n_workers = 1
    cfg = make_cfg(args, n_workers, device)
    dt = cfg.torch_dtype()
    if args.sparse:
        data = synthetic_csr(args.rows, args.cols, seed=BASE["seed"],
                             device=device, dtype=dt)
    else:
        data = synthetic_dense(args.rows, args.cols, seed=BASE["seed"],
                               dtype=dt, device=device,
                               objective=args.objective)

    if args.engine in ("native", "resident") and device.type == "cuda":
        # native: C++ event-loop engine (multi-worker async, zero Python
        # per round). resident: the whole loop in ONE persistent kernel
        # (zero host API calls per round; dense only).
        shards = []
        for s, t in row_shards(args.rows, n_workers):
            if args.sparse:
                indptr, indices, values, y = data
                base = int(indptr[s])
                shards.append(Shard(
                    row_start=s, n_rows=t - s,
                    indptr=(indptr[s:t + 1] - base).contiguous(),
                    indices=indices[base:int(indptr[t])],
                    values=values[base:int(indptr[t])], y=y[s:t]))
            else:
                X, y = data
                shards.append(Shard(row_start=s, n_rows=t - s, X=X[s:t],
                                    y=y[s:t]))
        if args.engine == "resident":
            from asyncframework_amd.engine.resident import ResidentEngine
            try:
                neng = ResidentEngine(cfg, shards, device)
                elapsed, res = neng.bench(args.warmup, args.steps,
                                          snapshot_every=snap_cadence(args))
            except (RuntimeError, AssertionError) as e:
                # co-residency refusal / wedge abort: fall back to the
                # host-driven C++ engine rather than fail the bench run
                print(f"[bench] resident engine unavailable ({e}); "
                      f"falling back to native", file=sys.stderr)
                from asyncframework_amd.engine.native import \
                    NativeLocalEngine
                neng = NativeLocalEngine(cfg, shards, device)
                elapsed, res = neng.bench(args.warmup, args.steps,
                                          snapshot_every=snap_cadence(args))
        else:
            from asyncframework_amd.engine.native import NativeLocalEngine
            neng = NativeLocalEngine(cfg, shards, device)
            elapsed, res = neng.bench(args.warmup, args.steps,
                                      snapshot_every=snap_cadence(args))
        dump_outputs(args, neng.w, res.get("opt_vars"))
        tt = (to_target_summary(args, data, res.get("opt_vars"))
              if args.full else None)
        emit(args, cfg, elapsed, n_gpus=1, to_target=tt)
        return

    if args.engine == "graph" and device.type == "cuda":
        from asyncframework_amd.engine.graph import GraphEngine
        if args.sparse:
            sh = Shard(row_start=0, n_rows=args.rows, indptr=data[0],
                       indices=data[1], values=data[2], y=data[3])
        else:
            sh = Shard(row_start=0, n_rows=args.rows, X=data[0], y=data[1])
        eng = GraphEngine(cfg, sh, device)
        torch.cuda.synchronize()
        t0, t1 = eng.bench(args.warmup, args.steps)
        dump_outputs(args, eng.w)
        emit(args, cfg, t1 - t0, n_gpus=1)
        return

    if args.sparse:
        workers = runner.build_csr_workers(cfg, *data)
    else:
        workers = runner.build_dense_workers(cfg, *data)
    # threads engine: optVars snapshots via the server's printer_freq hook
    cfg.snapshot_weights = True
    cfg.printer_freq = snap_cadence(args)
    server = Server(cfg, device=device)
    eng_cls = SyncEngine if cfg.sync else AsyncEngine
    eng = eng_cls(cfg, workers=workers, server=server)
    eng.verbose = False
    eng.mark_at = {args.warmup, args.warmup + args.steps}
    if device.type == "cuda":
        torch.cuda.synchronize()
    eng.run(max_wall_s=1800)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = eng.marks.get(args.warmup)
    t1 = eng.marks.get(args.warmup + args.steps)
    if t0 is None or t1 is None or t1 <= t0:
        print(json.dumps({"error": "marks missing"}))
        sys.exit(1)
    dump_outputs(args, server.w, server.opt_vars)
    tt = (to_target_summary(args, data, server.opt_vars)
          if args.full else None)
    emit(args, cfg, t1 - t0, n_gpus=1, to_target=tt)


def run_dist(args, device, rank, world):
    """N>1: one process per GPU over RCCL. Logical workers stay at the
    preset's count (the reference's FIXED partitions=32 model): each rank
    hosts M = preset_workers/world workers on independent HIP streams and
    per-worker pair communicators, so the whole-node worker pool (and the
    quorum-gate semantics) is identical at every N — only the hardware
    underneath it scales."""
    import torch.distributed as dist
    from asyncframework_amd.engine.dist import DistEngine
    M = max(1, (args.preset_workers or world) // world)
    P = M * world
    cfg = make_cfg(args, P, device)
    dt = cfg.torch_dtype()
    shards = row_shards(args.rows, P)
    workers = []
    for j in range(M):
        wid = rank * M + j
        s, t = shards[wid]
        if args.sparse:
            indptr, indices, values, yv = synthetic_csr(
                t - s, args.cols, seed=BASE["seed"] + wid, device=device,
                dtype=dt)
            sh = Shard(row_start=s, n_rows=t - s, indptr=indptr,
                       indices=indices, values=values, y=yv)
        else:
            X, y = synthetic_dense(t - s, args.cols, seed=BASE["seed"] + wid,
                                   dtype=dt, device=device,
                                   objective=args.objective)
            sh = Shard(row_start=s, n_rows=t - s, X=X, y=y)
        workers.append(Worker(wid, sh, cfg, device=device))
    dist.init_process_group("nccl" if device.type == "cuda" else "gloo",
                            rank=rank, world_size=world)
    dist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    dist_engine = (args.dist_engine
                   or os.environ.get("ASYNCAMD_DIST_ENGINE", "")
                   or "native")
    if dist_engine == "native":
        # DEFAULT N>1 control plane: C++ rank-0 server
        # (csrc/server_dist.cpp). Wire-compatible with the Python path and
        # 3-5x faster in every control-plane A/B
        # (profiles/r01_dist_control_plane.md: python flat at ~650
        # updates/s from 2->8 ranks; C++ 1.3k->3.7k). RCCL refuses
        # same-device ranks (profiles/r02_validation.md), so 1-GPU leases
        # cap pre-driver validation at world=1 GPU + world 2-8 gloo.
        from asyncframework_amd.engine.dist_native import NativeDistEngine
        neng = NativeDistEngine(
            cfg, workers, device,
            mark_at=[args.warmup, args.warmup + args.steps])
        res = neng.run(verbose=False, max_wall_s=1800)
        if device.type == "cuda":
            torch.cuda.synchronize()
        if rank == 0:
            t0 = neng.marks.get(args.warmup)
            t1 = neng.marks.get(args.warmup + args.steps)
            if t0 is None or t1 is None or t1 <= t0:
                print(json.dumps({"error": "marks missing"}))
            else:
                dump_outputs(args, res.w)
                emit(args, cfg, t1 - t0, n_gpus=world)
        dist.destroy_process_group()
        return
    deng = DistEngine(cfg, workers, device)
    if rank == 0:
        eng, server, channels = deng.build_engine()
        eng.verbose = False
        eng.mark_at = {args.warmup, args.warmup + args.steps}
        eng.run(max_wall_s=1800)
        dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()
        t0 = eng.marks.get(args.warmup)
        t1 = eng.marks.get(args.warmup + args.steps)
        if t0 is None or t1 is None or t1 <= t0:
            print(json.dumps({"error": "marks missing"}))
        else:
            dump_outputs(args, server.w)
            emit(args, cfg, t1 - t0, n_gpus=world)
    else:
        deng.worker_loop()
        dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()
    dist.destroy_process_group()


def _start_heartbeat(period_s: float = 30.0):
    """stderr heartbeat so a driver watching the process can tell a slow
    bench from a wedged one (round-1: a deadlocked engine was silent for
    30 min). The native engine additionally hard-aborts via its C++ stall
    watchdog (csrc/engine_native.cpp) if no update lands for 60 s."""
    import threading
    t0 = time.perf_counter()

    def beat():
        while True:
            time.sleep(period_s)
            print(f"[bench heartbeat] alive t={time.perf_counter() - t0:.0f}s",
                  file=sys.stderr, flush=True)

    th = threading.Thread(target=beat, daemon=True)
    th.start()


def main():
    args = parse_args()
    _start_heartbeat()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    if args.device:
        device = torch.device(args.device)
        if device.type == "cuda":
            torch.cuda.set_device(device)
    elif torch.cuda.is_available():
        device = torch.device(f"cuda:{local_rank}")
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    if device.type == "cuda":
        import asyncframework_amd.ops as ops
        assert ops.hip_available(), "HIP extension missing on a GPU box"

    if world > 1:
        run_dist(args, device, rank, world)
    else:
        run_single(args, device)


if __name__ == "__main__":
    main()
