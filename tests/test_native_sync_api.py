"""Native engine synchronous mode: the CPU-side contract.

The sync drivers may select ``--engine native`` on a GPU; on CPU workers
that request must fail with an AssertionError before the extension is
imported or anything is allocated, and unsupported configurations
(host-spill history) must be rejected the same way."""

import sys

import pytest
import torch

from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.worker import Shard
from asyncframework_amd.run import (build_dense_workers, load_dataset,
                                    run_engine)


def _sync_cfg(**kw):
    base = dict(d=4, N=16, num_workers=2, num_iterations=4, sync=True)
    base.update(kw)
    return EngineConfig(**base)


@pytest.mark.parametrize("algo", ["asgd", "asaga", "mllib"])
def test_native_sync_on_cpu_workers_is_gpu_only(algo, monkeypatch):
    cfg = _sync_cfg(algo=algo)
    X, y = load_dataset(cfg, "synthetic", "synthetic")
    workers = build_dense_workers(cfg, X, y)
    # raised FIRST: the native adapter module must not even be imported
    monkeypatch.delitem(sys.modules, "asyncframework_amd.engine.native",
                        raising=False)
    with pytest.raises(AssertionError, match="GPU-only"):
        run_engine(cfg, workers, engine="native", verbose=False)
    assert "asyncframework_amd.engine.native" not in sys.modules


def test_sgd_mllib_passes_engine_through(capsys):
    """sgd-mllib used to parse --engine and then run the threads engine."""
    from asyncframework_amd.cli import drivers
    with pytest.raises(AssertionError, match="GPU-only"):
        drivers.sgd_mllib(["synthetic", "synthetic", "4", "64", "2", "3",
                           "0.1", "0.5", "--device", "cpu",
                           "--engine", "native"])
    assert "finished" not in capsys.readouterr().out.splitlines()


def test_asgd_sync_cli_native_on_cpu_asserts():
    from asyncframework_amd.cli import drivers
    with pytest.raises(AssertionError, match="GPU-only"):
        drivers.asgd_sync(["synthetic", "synthetic", "4", "64", "2", "3",
                           "0.1", "1000", "0.5", "0.5", "1", "0", "42",
                           "--device", "cpu", "--engine", "native"])


def test_native_sync_rejects_host_spill_before_gpu_work():
    """history_placement='host' is out of scope for sync mode: the adapter
    refuses it before importing the extension or touching the device (the
    shards here are CPU tensors and no GPU is needed to get the error)."""
    from asyncframework_amd.engine.native import NativeLocalEngine
    cfg = _sync_cfg(algo="asaga", history_placement="host")
    X, y = load_dataset(cfg, "synthetic", "synthetic")
    shards = [Shard(row_start=0, n_rows=8, X=X[:8], y=y[:8]),
              Shard(row_start=8, n_rows=8, X=X[8:], y=y[8:])]
    with pytest.raises(AssertionError, match="history_placement"):
        NativeLocalEngine(cfg, shards, torch.device("cuda:0"))


def test_native_sync_host_spill_via_run_engine_asserts():
    cfg = _sync_cfg(algo="asaga", history_placement="host")
    X, y = load_dataset(cfg, "synthetic", "synthetic")
    workers = build_dense_workers(cfg, X, y)
    with pytest.raises(AssertionError):
        run_engine(cfg, workers, engine="native", verbose=False)
