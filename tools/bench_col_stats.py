"""Time ops.col_stats[_csr] and the in-place scale kernels against torch's
own ops on the same tensors in the same process, and print ONE JSON line.

Dense case: a bf16 slice of the flagship shape (default 1M x 784, which fits
beside the fp32 copy torch makes of it). Timed alternately, rep by rep:

* ``col_stats``      ops.col_stats(X): one pass, eight statistics;
* ``torch_var_mean`` X.float().var(0) and X.float().mean(0): torch's way to
                     two of them, through an fp32 expansion of X;
* ``scale``          the in-place scale kernel (std only, as --standardize);
* ``torch_mul_``     X.mul_(f), torch's in-place broadcast multiply;
* ``evaluate``       ops.evaluate with one iterate: this project's tuned
                     one-pass streaming read of the same X, as a ceiling.

CSR case: an rcv1-shape matrix (default 697,641 x 47,236, ~73 nnz/row):
ops.col_stats_csr against the index_add_ reference run on the GPU tensors,
ops.scale_csr_ against values.mul_(f[indices]), and ops.evaluate_csr.

``bytes`` is what each op needs BY THE SHAPES, not a counter: the
statistics read X once (their partials and outputs are counted too), the
scale reads and writes X once, torch's var + mean write and twice re-read an
fp32 copy. ``gbps`` is those bytes over the median time — a whole-call rate,
launches and allocations included, not a kernel's share of peak.

Needs a GPU: there is no CPU fallback."""

from __future__ import annotations

import argparse
import json
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


def _alternate(fns: dict, warmup: int, reps: int) -> dict:
    for _ in range(warmup):
        for f in fns.values():
            f()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(_time(f))
    return times


def _stats(times, nbytes):
    med = statistics.median(times)
    return {"median_ms": med * 1e3, "min_ms": min(times) * 1e3,
            "max_ms": max(times) * 1e3, "bytes": int(nbytes),
            "gbps": nbytes / med / 1e9}


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--dense-rows", type=int, default=1_000_000)
    p.add_argument("--dense-cols", type=int, default=784)
    p.add_argument("--csr-rows", type=int, default=697_641)
    p.add_argument("--csr-cols", type=int, default=47_236)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--skip-csr", action="store_true")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_col_stats needs a GPU", file=sys.stderr)
        return 2

    from asyncframework_amd import ops
    from asyncframework_amd.data.scale import StandardScaler
    from asyncframework_amd.data.synthetic import (synthetic_csr,
                                                   synthetic_dense)
    from asyncframework_amd.ops import torch_ref
    import asyncframework_amd._hip_core as core
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "reps": a.reps, "cases": [],
           "kernel_info": {k: dict(v) for k, v in
                           core.col_stats_kernel_info().items()}}

    n, d = a.dense_rows, a.dense_cols
    X, y = synthetic_dense(n, d, seed=42, dtype=torch.bfloat16, device=dev)
    geom = dict(core.col_stats_geom(X.data_ptr(), n, d, 1))
    # a factor of exactly one: repeated in-place passes leave X as it is
    one = torch.ones(d, device=dev)
    zero = torch.zeros(d, device=dev)
    one_bf = one.to(torch.bfloat16)
    W = torch.randn(1, d, device=dev) * 0.1
    t = _alternate({
        "col_stats": lambda: ops.col_stats(X),
        "torch_var_mean": lambda: (X.float().var(0), X.float().mean(0)),
        "scale": lambda: ops.scale_(X, zero, one),
        "torch_mul_": lambda: X.mul_(one_bf),
        "evaluate": lambda: ops.evaluate(X, y, W, "lsq"),
    }, a.warmup, a.reps)
    xb = n * d * 2
    part = geom["grid_y"] * d * (5 * 8 + 2 * 4 + 4)
    tile = core.eval_tile()
    case = {
        "case": "dense_bf16", "rows": n, "d": d, "geometry": geom,
        "col_stats": _stats(t["col_stats"], xb + 2 * part + d * 7 * 8),
        # two expansions (read bf16, write fp32), var and mean each re-read
        "torch_var_mean": _stats(t["torch_var_mean"],
                                 2 * (xb + 2 * xb) + 2 * (2 * xb)),
        "scale": _stats(t["scale"], 2 * xb + 2 * d * 4),
        "torch_mul_": _stats(t["torch_mul_"], 2 * xb + d * 2),
        "evaluate": _stats(t["evaluate"], xb + n * 4 + tile * d * 4)}
    m = {k: statistics.median(v) for k, v in t.items()}
    case["torch_var_mean_over_col_stats"] = m["torch_var_mean"] / m["col_stats"]
    case["torch_mul_over_scale"] = m["torch_mul_"] / m["scale"]
    case["col_stats_over_evaluate"] = m["col_stats"] / m["evaluate"]
    out["cases"].append(case)
    # the real thing once: fit + transform, and what it leaves
    model = StandardScaler().fit(ops.col_stats(X))
    model.transform_(X)
    sd = X.float().std(0)
    out["standardized_std_min_max"] = [float(sd.min()), float(sd.max())]
    del X, y

    if not a.skip_csr:
        n, d = a.csr_rows, a.csr_cols
        indptr, indices, values, y = synthetic_csr(n, d, seed=42, device=dev)
        nnz = int(values.numel())
        one = torch.ones(d, device=dev)
        W = torch.randn(1, d, device=dev) * 0.1
        idx64 = indices.long()
        t = _alternate({
            "col_stats_csr": lambda: ops.col_stats_csr(indptr, indices,
                                                       values, d),
            "torch_index_add": lambda: torch_ref.col_stats_csr(
                indptr, indices, values, d),
            "scale_csr": lambda: ops.scale_csr_(indices, values, one),
            "torch_mul_": lambda: values.mul_(one[idx64]),
            "evaluate_csr": lambda: ops.evaluate_csr(indptr, indices, values,
                                                     y, W, "lsq"),
        }, a.warmup, a.reps)
        case = {
            "case": "csr_fp32", "rows": n, "d": d, "nnz": nnz,
            # per entry: value + column id, and six atomics of 8/8/8/4/4/4 B
            "col_stats_csr": _stats(t["col_stats_csr"],
                                    nnz * (8 + 36) + d * (6 * 8 + 13 * 8)),
            "torch_index_add": _stats(t["torch_index_add"], nnz * (8 + 36)),
            "scale_csr": _stats(t["scale_csr"], nnz * (4 + 4 + 4 + 4)),
            "torch_mul_": _stats(t["torch_mul_"],
                                 nnz * (8 + 4 + 4 + 4 + 4 + 4)),
            "evaluate_csr": _stats(t["evaluate_csr"],
                                   nnz * (4 + 4 + tile * 4) + (2 * n + 1) * 4)}
        m = {k: statistics.median(v) for k, v in t.items()}
        case["torch_index_add_over_col_stats_csr"] = (
            m["torch_index_add"] / m["col_stats_csr"])
        case["torch_mul_over_scale_csr"] = m["torch_mul_"] / m["scale_csr"]
        out["cases"].append(case)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
