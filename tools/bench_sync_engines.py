#!/usr/bin/env python3
"""Synchronous rounds/s: the native engine's synchronous mode vs the
Python-threads SyncEngine on one config (default: mnist8m shape, dense 784
columns bf16, 32 workers, batch rate 0.1, no injected delays). Prints one
JSON line. The numbers in profiles/r03_native_sync.md come from here.

Usage: python tools/bench_sync_engines.py [--rows N] [--cols D] [...]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asyncframework_amd import run as runner  # noqa: E402
from asyncframework_amd.data.synthetic import synthetic_dense  # noqa: E402
from asyncframework_amd.engine.config import EngineConfig  # noqa: E402
from asyncframework_amd.engine.native import NativeLocalEngine  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--rows", type=int, default=8_100_000)
    p.add_argument("--cols", type=int, default=784)
    p.add_argument("--workers", type=int, default=32)
    p.add_argument("--rate", type=float, default=0.1)
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--algo", default="asgd",
                   choices=["asgd", "asaga", "mllib"])
    p.add_argument("--native-rounds", type=int, default=500)
    p.add_argument("--native-warmup", type=int, default=50)
    p.add_argument("--threads-rounds", type=int, default=150)
    p.add_argument("--max-wall-s", type=float, default=120.0)
    a = p.parse_args()

    def cfg(iters):
        return EngineConfig(
            d=a.cols, N=a.rows, num_workers=a.workers, num_iterations=iters,
            gamma=0.01, batch_rate=a.rate, printer_freq=1 << 30,
            delay_coeff=0.0, seed=42, algo=a.algo, sync=True,
            objective="lsq", dtype=a.dtype, device=a.device,
            snapshot_weights=False)

    c = cfg(a.threads_rounds)
    X, y = synthetic_dense(a.rows, a.cols, seed=42, dtype=c.torch_dtype(),
                           device=a.device)
    workers = runner.build_dense_workers(c, X, y)

    neng = NativeLocalEngine(cfg(10 ** 9), [w.shard for w in workers],
                             torch.device(a.device))
    n_s, nres = neng.bench(warmup=a.native_warmup, steps=a.native_rounds,
                           max_wall_s=a.max_wall_s)
    del neng

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res, _ = runner.run_engine(c, workers, max_wall_s=a.max_wall_s,
                               verbose=False, engine="threads")
    torch.cuda.synchronize()
    t_s = time.perf_counter() - t0

    print(json.dumps({
        "experiment": "sync_rounds_per_s_native_vs_threads",
        "config": {"rows": a.rows, "cols": a.cols, "workers": a.workers,
                   "rate": a.rate, "dtype": a.dtype, "algo": a.algo,
                   "delay_coeff": 0.0, "device": a.device},
        "native": {"rounds": a.native_rounds, "seconds": n_s,
                   "rounds_per_s": a.native_rounds / n_s,
                   "ms_per_round": 1e3 * n_s / a.native_rounds},
        "threads": {"rounds": res.k, "seconds": t_s,
                    "rounds_per_s": res.k / t_s,
                    "ms_per_round": 1e3 * t_s / max(res.k, 1)},
        "native_over_threads": (a.native_rounds / n_s) / (res.k / t_s),
    }))


if __name__ == "__main__":
    main()
