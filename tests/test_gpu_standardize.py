"""run.standardize_ on MI355X, end to end: a native synchronous asgd run on
data standardised by the kernels against the same engine on data
standardised by the CPU reference.

The two standardised matrices are compared bit for bit. The engine itself
sums its minibatch gradient with float atomics, so two runs of it on
identical data agree to rounding, not bitwise; its own two-run comparisons
(tests/test_gpu_native_sync.py, BOUND) hold the iterates to a relative
1e-4 at this round count, and so does this test."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops
from asyncframework_amd import run as runner
from asyncframework_amd.data.scale import StandardScaler
from asyncframework_amd.data.shard import row_shards
from asyncframework_amd.data.synthetic import synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.native import NativeLocalEngine
from asyncframework_amd.engine.worker import Shard

DEV = "cuda:0"
BOUND = 1e-4  # tests/test_gpu_native_sync.py


def _train(cfg, X, y):
    shards = [Shard(row_start=s, n_rows=t - s, X=X[s:t], y=y[s:t])
              for s, t in row_shards(cfg.N, cfg.num_workers)]
    eng = NativeLocalEngine(cfg, shards, torch.device(DEV))
    res = eng.run(max_wall_s=120)
    assert res["k"] == cfg.num_iterations and res["rejected"] == 0
    return eng.w.clone()


def test_standardize_then_native_sync_asgd():
    n, d = 2048, 784
    cfg = EngineConfig(d=d, N=n, num_workers=4, num_iterations=40, gamma=0.3,
                       taw=1 << 30, batch_rate=0.05, bucket_ratio=0.5,
                       printer_freq=1 << 30, delay_coeff=0.0, seed=42,
                       device=DEV, dtype="bf16", snapshot_weights=False,
                       sync=True)
    X, y = synthetic_dense(n, d, seed=3, dtype=torch.float32, device="cpu")
    X = (X * (10.0 ** (torch.arange(d) % 4 - 1))).to(torch.bfloat16)
    Xt = X[:100].clone()

    # the CPU reference path
    X_ref, Xt_ref = X.clone(), Xt.clone()
    ref_model = StandardScaler().fit(ops.col_stats(X_ref))
    ref_model.transform_(X_ref)
    ref_model.transform_(Xt_ref)

    # the kernels
    X_gpu, Xt_gpu, y_gpu = X.to(DEV), Xt.to(DEV), y.to(DEV)
    model = runner.standardize_((X_gpu, y_gpu), (Xt_gpu, y_gpu[:100]), False)
    assert torch.equal(model.factor.cpu(), ref_model.factor)
    assert torch.equal(X_gpu.cpu(), X_ref)
    assert torch.equal(Xt_gpu.cpu(), Xt_ref)  # the TRAINING scaler
    sd = X_gpu.float().std(0)
    assert float((sd - 1.0).abs().max()) < 0.02  # bf16 rounding of the rows

    w_gpu = _train(cfg, X_gpu, y_gpu)
    w_ref = _train(cfg, X_ref.to(DEV), y_gpu)
    rel = float((w_gpu - w_ref).norm() / (w_ref.norm() + 1e-12))
    print("w rel", rel, "bitwise", torch.equal(w_gpu, w_ref))
    assert float(w_ref.norm()) > 0
    assert rel < BOUND, rel
