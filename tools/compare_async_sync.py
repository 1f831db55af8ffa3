#!/usr/bin/env python3
"""Async (ASGD) vs synchronous baseline under straggler injection — the
reference's headline experiment ("ASYNC is ~4x faster than
Spark" time-to-equal-error under the cloud long-tail delay model).

Round-2 fidelity upgrade: ``--preset fig7-mnist8m`` /
``--preset fig7-epsilon`` reproduce the reference's Figure-7
parameterization exactly (README.md "For Figures 7 and 8": 32 workers,
beta=0.7, delay intensity -1, batch rate 0.1, per-arm tuned step sizes and
iteration counts — mnist8m ASYNC 420k iters @ gamma 3.3333e-3 vs Sync 14k
@ 0.1; epsilon ASYNC 40k @ 3.33e-1 vs Sync 13k @ 10). Each arm runs with
its own gamma/iters, the shared cloud delay model, and the same synthetic
dataset; we report wall-clock-to-common-target and the speedup as one JSON
line.

The async arm runs on the native C++ event-loop engine (the framework's
production async path); the sync arm on the SyncEngine full-barrier path
(the framework's Spark-sync analog) — matching the reference's comparison
of its async system against the synchronous system, both under the same
delay model on the same hardware. ``--async-engine threads`` selects the
Python engine for an apples-to-apples control, and ``--sync-engine native``
runs the sync arm through the native engine's synchronous mode, so both
arms share one control plane (the reference compares both arms on one
substrate, SparkASGDSync.scala:239-277). The multiplier to publish is the
same-substrate one; the default (threads sync vs native async) is
cross-substrate.

Usage: python tools/compare_async_sync.py --preset fig7-mnist8m
   or: python tools/compare_async_sync.py [--rows N] [--cols D] [...]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asyncframework_amd import run as runner  # noqa: E402
from asyncframework_amd.data.shard import row_shards  # noqa: E402
from asyncframework_amd.data.synthetic import synthetic_dense  # noqa: E402
from asyncframework_amd.engine.config import EngineConfig  # noqa: E402
from asyncframework_amd.engine.worker import Shard  # noqa: E402
from asyncframework_amd.ops import torch_ref  # noqa: E402

# Reference README.md "For Figures 7 and 8" (exact): 32 workers, beta=0.7,
# delay intensity -1, batch rate 0.1; per-dataset-and-arm iters/step size.
PRESETS = {
    "fig7-mnist8m": dict(rows=8_100_000, cols=784, workers=32, rate=0.1,
                         bucket_ratio=0.7, coeff=-1.0, dtype="bf16",
                         iters_async=420_000, gamma_async=3.3333e-3,
                         iters_sync=14_000, gamma_sync=0.1),
    "fig7-epsilon": dict(rows=400_000, cols=2_000, workers=32, rate=0.1,
                         bucket_ratio=0.7, coeff=-1.0, dtype="fp32",
                         iters_async=40_000, gamma_async=3.33e-1,
                         iters_sync=13_000, gamma_sync=10.0),
}


def sync_loss_curve(cfg, X, y, max_wall_s):
    workers = runner.build_dense_workers(cfg, X, y)
    res, srv = runner.run_engine(cfg, workers, max_wall_s=max_wall_s,
                                 verbose=False)
    W = torch.stack([w for (_, w) in res.opt_vars]).to(X.device)
    obj = torch_ref.objective_sweep(X, y, W, cfg.objective)
    return ([(t, float(o)) for (t, _), o in zip(res.opt_vars, obj)],
            res.k, res.elapsed_ms)


def async_loss_curve_native(cfg, X, y, max_wall_s, snap_every):
    from asyncframework_amd.engine.native import NativeLocalEngine
    shards = [Shard(row_start=s, n_rows=t - s, X=X[s:t], y=y[s:t])
              for s, t in row_shards(X.shape[0], cfg.num_workers)]
    eng = NativeLocalEngine(cfg, shards, X.device)
    res = eng.run(max_wall_s=max_wall_s, snapshot_every=snap_every)
    ov = res["opt_vars"]
    W = torch.stack([w for (_, w) in ov]).to(X.device)
    obj = torch_ref.objective_sweep(X, y, W, cfg.objective)
    return ([(t, float(o)) for (t, _), o in zip(ov, obj)],
            res["k"], res["elapsed_ms"])


def time_to_target(curve, target):
    for t_ms, o in curve:
        if o <= target:
            return t_ms
    return None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--preset", default="", choices=[""] + list(PRESETS))
    p.add_argument("--device", default="cuda:0" if torch.cuda.is_available()
                   else "cpu")
    p.add_argument("--rows", type=int, default=400_000)   # epsilon shape
    p.add_argument("--cols", type=int, default=2_000)
    p.add_argument("--workers", type=int, default=32)
    p.add_argument("--iters-async", type=int, default=2000)
    p.add_argument("--iters-sync", type=int, default=0,
                   help="sync rounds (default iters_async // workers)")
    p.add_argument("--gamma-async", type=float, default=1.0)
    p.add_argument("--gamma-sync", type=float, default=0.0,
                   help="default = gamma_async")
    p.add_argument("--rate", type=float, default=0.1)
    p.add_argument("--bucket-ratio", type=float, default=0.7)
    p.add_argument("--taw", type=int, default=20_000_000)
    p.add_argument("--coeff", type=float, default=-1.0)
    p.add_argument("--calib-factor", type=int, default=10)
    p.add_argument("--target-rel", type=float, default=0.35,
                   help="target = rel * initial objective (floored at the "
                        "worse arm's best achieved + 2%%)")
    p.add_argument("--dtype", default="fp32")
    p.add_argument("--max-wall-s", type=float, default=300.0)
    p.add_argument("--async-engine", default="",
                   choices=["", "native", "threads"])
    p.add_argument("--sync-engine", default="threads",
                   choices=["threads", "native"],
                   help="sync arm substrate: the Python-threads SyncEngine "
                        "(default) or the native engine's synchronous mode "
                        "(same substrate as the native async arm)")
    args = p.parse_args()
    if args.preset:
        for key, v in PRESETS[args.preset].items():
            setattr(args, key, v)
    if not args.gamma_sync:
        args.gamma_sync = args.gamma_async
    if not args.iters_sync:
        args.iters_sync = max(1, args.iters_async // args.workers)
    on_gpu = args.device.startswith("cuda")
    async_engine = args.async_engine or ("native" if on_gpu else "threads")

    def mk_cfg(sync):
        iters = args.iters_sync if sync else args.iters_async
        return EngineConfig(
            d=args.cols, N=args.rows, num_workers=args.workers,
            num_iterations=iters,
            gamma=args.gamma_sync if sync else args.gamma_async,
            taw=args.taw, batch_rate=args.rate,
            bucket_ratio=args.bucket_ratio,
            printer_freq=max(1, iters // 60), delay_coeff=args.coeff,
            seed=42, algo="asgd", sync=sync, objective="lsq",
            dtype=args.dtype, device=args.device,
            calib_factor=args.calib_factor, snapshot_weights=True)

    acfg = mk_cfg(False)
    X, y = synthetic_dense(args.rows, args.cols, seed=42,
                           dtype=acfg.torch_dtype(), device=args.device)

    if async_engine == "native" and on_gpu:
        async_curve, ak, ams = async_loss_curve_native(
            acfg, X, y, args.max_wall_s, max(1, args.iters_async // 60))
    else:
        async_curve, ak, ams = sync_loss_curve(acfg, X, y, args.max_wall_s)
    scfg = mk_cfg(True)
    if args.sync_engine == "native":
        # same substrate as the async arm: NativeLocalEngine dispatches a
        # sync cfg to the engine's stream-ordered barrier rounds
        assert on_gpu, "--sync-engine native needs a GPU device"
        sync_curve, sk, sms = async_loss_curve_native(
            scfg, X, y, args.max_wall_s, scfg.printer_freq)
    else:
        sync_curve, sk, sms = sync_loss_curve(scfg, X, y, args.max_wall_s)

    obj0 = async_curve[0][1]
    floor = max(min(o for _, o in async_curve),
                min(o for _, o in sync_curve))
    target = max(args.target_rel * obj0, floor * 1.02)
    ta = time_to_target(async_curve, target)
    ts = time_to_target(sync_curve, target)
    out = {
        "experiment": "async_vs_sync_time_to_target_loss",
        "preset": args.preset or None,
        "delay_model": ("cloud-long-tail" if args.coeff == -1.0
                        else f"coeff={args.coeff}"),
        "config": {"rows": args.rows, "cols": args.cols,
                   "workers": args.workers, "rate": args.rate,
                   "bucket_ratio": args.bucket_ratio,
                   "gamma_async": args.gamma_async,
                   "gamma_sync": args.gamma_sync,
                   "iters_async": args.iters_async,
                   "iters_sync": args.iters_sync,
                   "dtype": args.dtype, "device": args.device,
                   "async_engine": async_engine,
                   "sync_engine": args.sync_engine},
        "initial_objective": obj0,
        "target_objective": target,
        "async": {"iters": ak, "elapsed_ms": ams,
                  "time_to_target_ms": ta,
                  "final_obj": async_curve[-1][1]},
        "sync": {"rounds": sk, "elapsed_ms": sms,
                 "time_to_target_ms": ts,
                 "final_obj": sync_curve[-1][1]},
        "speedup_to_target": (round(ts / ta, 3)
                              if (ta is not None and ts is not None and ta > 0)
                              else None),
        # sync truncated by the wall cap without reaching the target =>
        # the true speedup is at least elapsed_sync / ta
        "speedup_lower_bound": (round(sms / ta, 3)
                                if (ts is None and ta not in (None, 0))
                                else None),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
