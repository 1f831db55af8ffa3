"""Time ops.evaluate[_csr] (the fused evaluation kernels) against
ops.objective_sweep[_csr] (the GEMM-backed sweep) on the same data in the
same process, and print ONE JSON line.

Cases: a dense bf16 matrix of mnist8m's row length (default 1M x 784) and an
rcv1-shape CSR matrix (default 697,641 x 47,236, ~73 nnz/row), each with
T in {1, 8, 64} stacked iterates. Per (case, T) the two ops are warmed up,
then timed alternately (evaluate, sweep, evaluate, ...) `--reps` times, each
timing a host clock around the call and a device synchronise; the medians
and the spread (min, max) are reported.

``bytes`` is what each op needs BY THE SHAPES, not a counter: the fused
kernel reads the data once per tile of `tile` iterates (+ y and the W
tile); the sweep reads the data once (CSR: the fp32 copy of the values it
makes first is counted as a write and a read) and writes and re-reads the
[rows, T] fp32 score matrix for its elementwise passes. ``gbps`` is those
bytes over the median time — a whole-call rate, launches and allocations
included, not a kernel's share of peak.

``--curve K [K ...]`` times the threshold sweep instead: per (T, K) one
ops.evaluate_curve call with K thresholds, one ops.evaluate call (the
floor) and K ops.evaluate calls (a K-point curve without the sweep),
alternated rep by rep on the dense case, with both ratios and the blocks
per CU of every sweep kernel next to its K9 twin's.

Needs a GPU: there is no CPU fallback."""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(f_eval, f_sweep, warmup: int, reps: int):
    for _ in range(warmup):
        f_eval()
        f_sweep()
    te, ts = [], []
    for _ in range(reps):
        te.append(_time(f_eval))
        ts.append(_time(f_sweep))
    return te, ts


def _stats(times, nbytes):
    med = statistics.median(times)
    return {"median_ms": med * 1e3, "min_ms": min(times) * 1e3,
            "max_ms": max(times) * 1e3, "bytes": int(nbytes),
            "gbps": nbytes / med / 1e9}


def _curve_mode(a) -> dict:
    """--curve: one threshold sweep of K thresholds against one evaluate
    call (the floor: the same pass with one threshold) and against K
    evaluate calls (the only way to K points without the sweep), on the
    dense bf16 case, alternated rep by rep."""
    from asyncframework_amd import ops
    from asyncframework_amd.data.synthetic import synthetic_dense
    import asyncframework_amd._hip_core as core
    dev = "cuda:0"
    n, d = a.dense_rows, a.dense_cols
    out = {"device": torch.cuda.get_device_name(0), "tile": core.eval_tile(),
           "curve_tile": core.eval_curve_tile(), "objective": a.objective,
           "warmup": a.warmup, "reps": a.reps, "cases": []}
    gen = torch.Generator(device=dev).manual_seed(1)
    X, y = synthetic_dense(n, d, seed=42, dtype=torch.bfloat16, device=dev,
                           objective=a.objective)
    for T in a.T:
        W = torch.randn(T, d, generator=gen, device=dev) * 0.1
        for K in a.curve:
            z = ops.curve_thresholds(X, W, K)
            # the K calls take the thresholds in the user's units
            users = (torch.sigmoid(z[0]).clamp(1e-9, 1 - 1e-9)
                     if a.objective == "logistic" else z[0]).tolist()

            def f_curve():
                return ops.evaluate_curve(X, y, W, a.objective,
                                          z_thresholds=z)

            def f_one():
                return ops.evaluate(X, y, W, a.objective)

            def f_calls():
                for thr in users:
                    ops.evaluate(X, y, W, a.objective, threshold=thr)

            for _ in range(a.warmup):
                f_curve()
                f_one()
            f_calls()
            tc, t1, tk = [], [], []
            for _ in range(a.reps):
                tc.append(_time(f_curve))
                t1.append(_time(f_one))
                tk.append(_time(f_calls))
            tiles = math.ceil(T / out["tile"])
            passes = math.ceil(K / out["curve_tile"])
            per_pass = n * d * 2 + n * 4 + out["tile"] * d * 4
            mc, m1, mk = (statistics.median(t) for t in (tc, t1, tk))
            out["cases"].append({
                "case": "dense_bf16", "rows": n, "d": d, "T": T, "K": K,
                "passes": tiles * passes,
                "evaluate_curve": _stats(tc, tiles * passes * per_pass),
                "evaluate_once": _stats(t1, tiles * per_pass),
                "evaluate_K_calls": _stats(tk, K * tiles * per_pass),
                "curve_over_once": mc / m1, "K_calls_over_curve": mk / mc})
    # blocks per CU of every sweep kernel next to its K9 twin's
    k9 = core.eval_kernel_info()
    out["occupancy"] = {}
    for name, e in core.eval_curve_kernel_info().items():
        twin = k9[name.replace("eval_curve_", "eval_")]
        out["occupancy"][name] = {
            "blocks_per_cu": e["max_active_blocks_per_cu"],
            "lds_bytes": e["lds_bytes"], "num_regs": e["num_regs"],
            "k9_blocks_per_cu": twin["max_active_blocks_per_cu"],
            "k9_lds_bytes": twin["lds_bytes"],
            "k9_num_regs": twin["num_regs"]}
    return out


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--curve", type=int, nargs="+", default=None,
                   metavar="K",
                   help="time ops.evaluate_curve with K thresholds against "
                        "one and against K ops.evaluate calls (dense case) "
                        "instead of the evaluate / sweep comparison")
    p.add_argument("--dense-rows", type=int, default=1_000_000)
    p.add_argument("--dense-cols", type=int, default=784)
    p.add_argument("--csr-rows", type=int, default=697_641)
    p.add_argument("--csr-cols", type=int, default=47_236)
    p.add_argument("--T", type=int, nargs="+", default=[1, 8, 64])
    p.add_argument("--objective", default="logistic",
                   choices=["lsq", "logistic", "hinge"])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--skip-csr", action="store_true")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_evaluate needs a GPU", file=sys.stderr)
        return 2
    if a.curve:
        print(json.dumps(_curve_mode(a)))
        return 0

    from asyncframework_amd import ops
    from asyncframework_amd.data.synthetic import (synthetic_csr,
                                                   synthetic_dense)
    import asyncframework_amd._hip_core as core
    tile = core.eval_tile()
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "tile": tile,
           "objective": a.objective, "warmup": a.warmup, "reps": a.reps,
           "cases": []}
    gen = torch.Generator(device=dev).manual_seed(1)

    n, d = a.dense_rows, a.dense_cols
    X, y = synthetic_dense(n, d, seed=42, dtype=torch.bfloat16, device=dev,
                           objective=a.objective)
    for T in a.T:
        W = torch.randn(T, d, generator=gen, device=dev) * 0.1
        te, ts = _alternate(
            lambda: ops.evaluate(X, y, W, a.objective),
            lambda: ops.objective_sweep(X, y, W, a.objective),
            a.warmup, a.reps)
        tiles = math.ceil(T / tile)
        b_eval = tiles * (n * d * 2 + n * 4 + tile * d * 4)
        b_sweep = n * d * 2 + n * 4 + T * d * 2 + 2 * n * T * 4
        out["cases"].append({
            "case": "dense_bf16", "rows": n, "d": d, "T": T,
            "evaluate": _stats(te, b_eval),
            "objective_sweep": _stats(ts, b_sweep)})
    del X, y

    if not a.skip_csr:
        n, d = a.csr_rows, a.csr_cols
        indptr, indices, values, y = synthetic_csr(
            n, d, seed=42, device=dev, objective=a.objective)
        nnz = int(values.numel())
        for T in a.T:
            W = torch.randn(T, d, generator=gen, device=dev) * 0.1
            te, ts = _alternate(
                lambda: ops.evaluate_csr(indptr, indices, values, y, W,
                                         a.objective),
                lambda: ops.objective_sweep_csr(indptr, indices, values, y,
                                                W, a.objective),
                a.warmup, a.reps)
            tiles = math.ceil(T / tile)
            # per non-zero: value + column id + the tile's weights of that
            # column (served by the cache when columns repeat: an upper
            # bound on HBM traffic)
            b_eval = tiles * (nnz * (4 + 4 + tile * 4) + (n + 1) * 4 + n * 4)
            b_sweep = (nnz * (4 + 4) + 2 * nnz * 4 + nnz * T * 4
                       + (n + 1) * 4 + n * 4 + 2 * n * T * 4)
            out["cases"].append({
                "case": "csr_fp32", "rows": n, "d": d, "nnz": nnz, "T": T,
                "evaluate": _stats(te, b_eval),
                "objective_sweep": _stats(ts, b_sweep)})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
