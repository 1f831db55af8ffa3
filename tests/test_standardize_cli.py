"""--standardize through the drivers (CPU, threads engine): the flag's run
prints what the same run prints when it is assembled through the API on data
standardised by hand with numpy, and without the flag nothing changes.

Stdouts are compared line for line. The only fields that differ between two
runs of anything here are wall-clock readings — the elapsed-time line and the
millisecond stamp in front of each logged iterate — so those digits, and only
those, are masked before the comparison."""

import argparse
import io
import re
from contextlib import redirect_stdout

import numpy as np
import torch

from asyncframework_amd import run as runner
from asyncframework_amd.cli import drivers
from asyncframework_amd.utils import logfmt

ARGS13 = ["synthetic", "synthetic", "16", "200", "2", "30", "0.5", "1000000",
          "0.3", "0.5", "10", "0", "42"]
ARGS8 = ["synthetic", "synthetic", "16", "200", "2", "30", "0.5", "0.3"]


def _capture(fn, *args):
    buf = io.StringIO()
    with redirect_stdout(buf):
        fn(*args)
    return buf.getvalue()


def _mask_clock(out):
    lines = []
    for l in out.splitlines():
        l = re.sub(r"^Elapsed time\(ms\): \d+$", "Elapsed time(ms): T", l)
        l = re.sub(r"^\d+,", "T,", l)
        lines.append(l)
    return lines


def _hand_factor(cols_fp64, n):
    """fp32(1 / unbiased std) per column, 0 for a constant column, in numpy
    fp64 from the dense fp64 columns [n, d]."""
    mean = cols_fp64.sum(0) / n
    var = ((cols_fp64 - mean) ** 2).sum(0) / (n - 1)
    const = (cols_fp64.min(0) == cols_fp64.max(0)) | (var == 0)
    return np.where(const, 0.0, 1.0 / np.sqrt(np.where(const, 1.0, var))
                    ).astype(np.float32)


def _scale_dense_by_hand(X, factor):
    X.copy_(torch.from_numpy(X.float().numpy() * factor).to(X.dtype))


def _api_run_13(args, app, algo, sync, standardise):
    """What drivers._run does for one process, spelled out, with
    `standardise(data, test_data)` between the load and the engine."""
    a = drivers._parse13(args, "test")
    cfg = drivers._cfg13(a, algo, sync=sync)
    logfmt.print_header(app, drivers.ARG_NAMES_13, drivers._vals13(a))
    data, test_data = drivers._load(cfg, a, a.sparse, a.device)
    standardise(data, test_data)
    workers = runner.build_dense_workers(cfg, *data)
    res, _ = runner.run_engine(cfg, workers, engine="threads")
    runner.final_report(cfg, res, data, a.sparse, device=a.device)
    drivers._evaluate(cfg, a, res, test_data, a.sparse, a.device)


def test_asgd_sync_standardize_equals_the_hand_path():
    extra = ["--test-rows", "64"]

    def by_hand(data, test_data):
        X, Xt = data[0], test_data[0]
        f = _hand_factor(X.double().numpy(), X.shape[0])
        _scale_dense_by_hand(X, f)
        _scale_dense_by_hand(Xt, f)  # the TRAINING scaler

    got = _capture(drivers.asgd_sync, ARGS13 + extra + ["--standardize"])
    want = _capture(_api_run_13, ARGS13 + extra, "ASGDSync", "asgd", True,
                    by_hand)
    assert "Held-out rows: 64" in got
    assert _mask_clock(got) == _mask_clock(want)
    # and the flag did something: the plain run prints other objectives
    plain = _capture(drivers.asgd_sync, ARGS13 + extra)
    assert _mask_clock(plain) != _mask_clock(got)


def test_without_the_flag_nothing_changes():
    """A namespace from before the flag existed (no `standardize` attribute)
    runs, and prints what today's parser prints without the flag."""
    got = _capture(drivers.asgd_sync, ARGS13 + ["--test-rows", "64"])
    a = drivers._parse13(ARGS13 + ["--test-rows", "64"], "asgd-sync")
    assert a.standardize is False
    old = argparse.Namespace(**{k: v for k, v in vars(a).items()
                                if k != "standardize"})
    cfg = drivers._cfg13(old, "asgd", sync=True)
    want = _capture(drivers._run, cfg, old, "ASGDSync", drivers.ARG_NAMES_13,
                    drivers._vals13(old))
    assert _mask_clock(got) == _mask_clock(want)
    # no line of the output speaks of the scaler, with or without the flag
    flagged = _capture(drivers.asgd_sync, ARGS13 + ["--standardize"])
    assert len(flagged.splitlines()) == len(
        _capture(drivers.asgd_sync, ARGS13).splitlines())


def _hand_factor_csr(indices, values, n, d):
    """The summarizer's formulas over the stored entries, in numpy fp64:
    every stored entry is one observation of its column (the synthetic CSR
    generator may repeat a column within a row), and the n - nnz implicit
    zeros contribute mean^2 each to M2."""
    j, v = indices.numpy().astype(np.int64), values.double().numpy()
    nnz = np.bincount(j, minlength=d).astype(np.float64)
    mean = np.bincount(j, weights=v, minlength=d) / n
    m2 = np.bincount(j, weights=(v - mean[j]) ** 2, minlength=d) \
        + (n - nnz) * mean * mean
    var = m2 / (n - 1)
    lo, hi = np.full(d, np.inf), np.full(d, -np.inf)
    np.minimum.at(lo, j, v)
    np.maximum.at(hi, j, v)
    lo = np.where(nnz < n, np.minimum(lo, 0.0), lo)
    hi = np.where(nnz < n, np.maximum(hi, 0.0), hi)
    const = (lo == hi) | (var == 0)
    return np.where(const, 0.0, 1.0 / np.sqrt(np.where(const, 1.0, var))
                    ).astype(np.float32)


def test_sgd_mllib_sparse_standardize_matches_the_hand_path():
    args = ARGS8 + ["--sparse"]
    got = _capture(drivers.sgd_mllib, args + ["--standardize"])

    def hand():
        a = drivers._parse8(args, "test")
        cfg = drivers.EngineConfig(
            d=int(a.d), N=int(a.N), num_workers=int(a.numPart),
            num_iterations=int(a.numIter), gamma=float(a.gamma),
            batch_rate=float(a.b), algo="mllib", sync=True, printer_freq=100,
            objective=a.objective, dtype=a.dtype, device=a.device, seed=42,
            delay_coeff=0.0, l2=a.l2, l1=a.l1)
        logfmt.print_header("MLlib SGD", drivers.ARG_NAMES_8,
                            [a.pathname, a.fname, a.d, a.N, a.numPart,
                             a.numIter, a.gamma, a.b])
        data, _ = drivers._load(cfg, a, True, a.device)
        indptr, indices, values, y = data
        f = _hand_factor_csr(indices, values, indptr.shape[0] - 1, cfg.d)
        values.copy_(torch.from_numpy(
            values.numpy() * f[indices.numpy()]))
        workers = runner.build_csr_workers(cfg, *data)
        res, _ = runner.run_engine(cfg, workers, engine="threads")
        runner.final_report(cfg, res, data, True, device=a.device)

    want = _capture(hand)
    sep = lambda ls: max(i for i, l in enumerate(ls)
                         if l.startswith("*********"))
    gl, wl = _mask_clock(got), _mask_clock(want)
    obj_got, obj_want = gl[sep(gl) + 1:], wl[sep(wl) + 1:]
    assert obj_got[-1] == "finished" and len(obj_got) >= 2
    assert obj_got == obj_want
    assert gl == wl
