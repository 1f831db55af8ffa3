"""High-level run API shared by the five CLI drivers and the bench.

Builds shards/workers/engine from an EngineConfig + dataset, runs it, and
emits the reference's stdout contract (SURVEY §2.1 "API surface to keep
compatible")."""

from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from .data.shard import row_shards
from .data.synthetic import synthetic_csr, synthetic_dense
from .data.libsvm import load_libsvm
from .engine.config import EngineConfig
from .engine.delay import DelayInjector
from .engine.local import AsyncEngine, RunResult, SyncEngine
from .engine.server import Server
from .engine.worker import Shard, Worker
from .utils import logfmt


def is_synthetic(pathname: str, fname: str) -> bool:
    return fname.startswith("synthetic") or pathname.startswith("synthetic")


def load_dataset(cfg: EngineConfig, pathname: str, fname: str,
                 sparse: bool = False, device: str = "cpu",
                 return_w_true: bool = False):
    """'synthetic' fname -> generated data of (cfg.N, cfg.d); otherwise a
    LibSVM file at pathname+fname (reference MLUtils.loadLibSVMFile).
    ``return_w_true`` (synthetic only) returns (data, w_true): the planted
    model, for load_test_dataset."""
    dt = cfg.torch_dtype()
    if is_synthetic(pathname, fname):
        gen = synthetic_csr if sparse else synthetic_dense
        out = gen(cfg.N, cfg.d, seed=cfg.seed, device=device,
                  objective=cfg.objective, dtype=dt,
                  return_w_true=return_w_true)
        return (out[:-1], out[-1]) if return_w_true else out
    assert not return_w_true, "a file input has no planted model"
    path = pathname + fname
    if sparse:
        return load_libsvm(path, n_features=cfg.d, dense=False, dtype=dt,
                           device=device)
    return load_libsvm(path, n_features=cfg.d, dense=True, dtype=dt,
                       device=device)


def check_test_flags(pathname: str, fname: str, test_file: str,
                     test_rows: int) -> None:
    """--test-file belongs to a file input, --test-rows to a synthetic one,
    and only one of them may be given."""
    if test_file and test_rows:
        raise ValueError("give --test-file or --test-rows, not both")
    if test_rows < 0:
        raise ValueError(f"--test-rows must be positive, got {test_rows}")
    synth = is_synthetic(pathname, fname)
    if test_file and synth:
        raise ValueError("--test-file needs a file input; a synthetic input "
                         "takes --test-rows")
    if test_rows and not synth:
        raise ValueError("--test-rows needs a synthetic input; a file input "
                         "takes --test-file")


def load_test_dataset(cfg: EngineConfig, pathname: str, *,
                      test_file: str = "", test_rows: int = 0, w_true=None,
                      sparse: bool = False, device: str = "cpu"):
    """Held-out rows: a LibSVM file at pathname+test_file with cfg.d
    features, or test_rows synthetic rows of the training set's planted
    model ``w_true`` drawn with seed cfg.seed + 1."""
    dt = cfg.torch_dtype()
    if test_rows:
        gen = synthetic_csr if sparse else synthetic_dense
        return gen(test_rows, cfg.d, seed=cfg.seed + 1, device=device,
                   objective=cfg.objective, dtype=dt, w_true=w_true)
    return load_libsvm(pathname + test_file, n_features=cfg.d,
                       dense=not sparse, dtype=dt, device=device)


def standardize_(data, test_data=None, sparse: bool = False,
                 d: Optional[int] = None):
    """Fit a unit-variance scaler (no centring: MLlib's useFeatureScaling)
    on the training rows and rescale the training rows and, with the SAME
    scaler, the held-out rows, in place. ``data`` / ``test_data`` are the
    tuples of load_dataset / load_test_dataset; ``d`` is the number of
    columns of CSR data (default: the largest column id present, plus one).
    Returns the ScalerModel; its unscale_weights maps trained weights back
    to the raw features."""
    from .data.scale import StandardScaler
    if sparse:
        indptr, indices, values, _ = data
        if d is None:
            ids = [p[1] for p in (data, test_data)
                   if p is not None and p[1].numel()]
            d = max((int(i.max()) + 1 for i in ids), default=0)
        stats = ops.col_stats_csr(indptr, indices, values, d)
    else:
        stats = ops.col_stats(data[0])
    model = StandardScaler(with_mean=False, with_std=True).fit(stats)
    for part in (data, test_data):
        if part is None:
            continue
        if sparse:
            model.transform_csr_(part[1], part[2])
        else:
            model.transform_(part[0])
    return model


def build_dense_workers(cfg: EngineConfig, X: torch.Tensor, y: torch.Tensor,
                        devices: Optional[List[torch.device]] = None
                        ) -> List[Worker]:
    """Shard rows over numPart workers (replaces the reference's
    repartition shuffle, SparkASGDThread.scala:76). ``devices`` maps worker
    -> device for multi-GPU single-process setups; default: data's device."""
    shards = row_shards(X.shape[0], cfg.num_workers)
    workers = []
    for wid, (s, t) in enumerate(shards):
        dev = devices[wid] if devices else X.device
        Xs = X[s:t].to(dev) if X.device != dev else X[s:t]
        ys = y[s:t].to(dev) if y.device != dev else y[s:t]
        workers.append(Worker(wid, Shard(row_start=s, n_rows=t - s, X=Xs,
                                         y=ys), cfg, device=dev))
    return workers


def build_csr_workers(cfg: EngineConfig, indptr, indices, values, y,
                      devices=None) -> List[Worker]:
    n_rows = indptr.shape[0] - 1
    shards = row_shards(n_rows, cfg.num_workers)
    workers = []
    for wid, (s, t) in enumerate(shards):
        dev = devices[wid] if devices else values.device
        base = int(indptr[s])
        ip = (indptr[s:t + 1] - base).to(dev)
        lo, hi = base, int(indptr[t])
        workers.append(Worker(wid, Shard(
            row_start=s, n_rows=t - s,
            indptr=ip, indices=indices[lo:hi].to(dev),
            values=values[lo:hi].to(dev), y=y[s:t].to(dev)),
            cfg, device=torch.device(dev)))
    return workers


def run_engine(cfg: EngineConfig, workers: List[Worker],
               max_wall_s: Optional[float] = None,
               verbose: bool = True, engine: str = "threads",
               resume_from: str = ""):
    """engine='threads' (the Python mailbox engine — CPU + semantics
    oracle) or 'native' (the C++ engine, GPU only: the async event loop, or
    for ``cfg.sync`` its stream-ordered synchronous rounds).
    ``resume_from`` restores a checkpoint first; both engines read and
    write the one engine/checkpoint.py schema (``cfg.checkpoint_path`` +
    ``cfg.checkpoint_every``), so a file from either resumes on the other."""
    if engine == "native":
        if cfg.sync:
            # first, before the extension is imported or anything allocated
            assert workers[0].device.type == "cuda", \
                "native sync engine is GPU-only"
        from .engine.native import NativeLocalEngine
        neng = NativeLocalEngine(cfg, [w.shard for w in workers],
                                 workers[0].device)
        if resume_from:
            from .engine.checkpoint import load_checkpoint
            neng.restore_state(load_checkpoint(resume_from))
        nres = neng.run(max_wall_s=max_wall_s or 1800.0,
                        snapshot_every=(cfg.printer_freq
                                        if cfg.snapshot_weights else 0))
        if verbose:
            # sync: k counts rounds — one line every printer_freq rounds,
            # as SyncEngine prints them; a resumed run prints only the
            # iterations of this process
            pf = cfg.printer_freq
            first = -(-nres["k0"] // pf) * pf
            for i in range(first, nres["k"], pf):
                print(f"Iteration {i} is finished")
        if cfg.sync:  # SyncEngine leaves waiting_time empty
            waiting = {}
        else:
            waiting = {i: int(ms)
                       for i, ms in enumerate(nres["waiting_ms"])}
        res = RunResult(k=int(nres["k"]), elapsed_ms=int(nres["elapsed_ms"]),
                        opt_vars=nres.get("opt_vars", []),
                        waiting_time=waiting, w=neng.w,
                        applied=int(nres["applied"]),
                        rejected=int(nres["rejected"]))
        return res, neng
    server = Server(cfg, device=workers[0].device)
    if resume_from:
        from .engine.checkpoint import load_checkpoint, restore
        restore(server, workers, load_checkpoint(resume_from))
    delay = DelayInjector(cfg.num_workers, cfg.delay_coeff, cfg.seed,
                          calib_window=cfg.calib_factor * cfg.num_workers)
    eng_cls = SyncEngine if cfg.sync else AsyncEngine
    eng = eng_cls(cfg, workers, server=server, delay=delay)
    eng.verbose = verbose
    res = eng.run(max_wall_s=max_wall_s)
    return res, server


def final_report(cfg: EngineConfig, res: RunResult, data, sparse: bool,
                 device: str = "cpu") -> None:
    """The shutdown epilogue: elapsed, waiting times, and the per-iterate
    objective sweep in one pass (reference SparkASGDThread.scala:346-410)."""
    logfmt.elapsed(res.elapsed_ms)
    logfmt.waiting_times(res.waiting_time, max(res.k, 1))
    if res.opt_vars:
        W = torch.stack([w for (_, w) in res.opt_vars]).to(device)
        if sparse:
            indptr, indices, values, y = data
            obj = ops.objective_sweep_csr(indptr, indices, values, y, W,
                                          cfg.objective, N_total=cfg.N,
                                          l2=cfg.l2, l1=cfg.l1)
        else:
            X, y = data
            obj = ops.objective_sweep(X, y, W, cfg.objective, l2=cfg.l2,
                                      l1=cfg.l1)
        logfmt.objective_lines(
            (t_ms, float(o)) for (t_ms, _), o in zip(res.opt_vars, obj))
    else:
        logfmt.objective_lines([])


def evaluation_report(cfg: EngineConfig, res: RunResult, test_data,
                      sparse: bool, device: str = "cpu",
                      threshold: Optional[float] = None,
                      curve_bins: int = 0) -> None:
    """Held-out block after the epilogue: loss and accuracy of every logged
    iterate on rows the run never trained on (ops.evaluate[_csr]: the fused
    kernels on a GPU, the fp64 reference on the CPU). curve_bins > 0 adds a
    second block: areas under the ROC and PR curves and the best F1 of every
    iterate from a curve_bins-point threshold sweep
    (ops.evaluate_curve[_csr])."""
    y = test_data[-1]
    n = int(y.shape[0])
    if not res.opt_vars:
        logfmt.evaluation_lines(n, [])
        if curve_bins > 0:
            logfmt.curve_lines(curve_bins, [])
        return
    W = torch.stack([w for (_, w) in res.opt_vars]).to(device)
    if sparse:
        indptr, indices, values, y = test_data
        ev = ops.evaluate_csr(indptr, indices, values, y, W, cfg.objective,
                              threshold=threshold)
    else:
        X, y = test_data
        ev = ops.evaluate(X, y, W, cfg.objective, threshold=threshold)
    logfmt.evaluation_lines(
        n, ((t_ms, float(l), float(a)) for (t_ms, _), l, a
            in zip(res.opt_vars, ev.loss, ev.accuracy)))
    if curve_bins <= 0:
        return
    if sparse:
        cv = ops.evaluate_curve_csr(indptr, indices, values, y, W,
                                    cfg.objective, num_bins=curve_bins)
    else:
        cv = ops.evaluate_curve(X, y, W, cfg.objective, num_bins=curve_bins)
    f1, best = cv.f_measure(1.0).max(dim=1)
    z_best = cv.z_thr.gather(1, best[:, None])[:, 0]
    # the threshold in the user's units: a probability for logistic
    thr = torch.sigmoid(z_best) if cfg.objective == "logistic" else z_best
    logfmt.curve_lines(
        curve_bins, ((t_ms, float(a), float(p), float(f), float(t))
                     for (t_ms, _), a, p, f, t
                     in zip(res.opt_vars, cv.auc_roc(), cv.auc_pr(), f1,
                            thr)))
