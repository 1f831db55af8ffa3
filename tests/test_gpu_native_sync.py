"""Native engine synchronous mode (csrc/engine_native.cpp run_sync +
sync_round_update_kernel) on MI355X: asgd-sync / asaga-sync / sgd-mllib
rounds against closed-form torch loops over the WHOLE dataset.

Shard boundaries are 4-aligned (row_shards), so the union of the workers'
Philox masks is the whole-set mask and the sum of shard gradients is the
whole-set gradient — the references below never look at P. The bound
rel < 1e-4 is the one test_native_p1_matches_sequential_ref already holds
these gradient kernels to at this shape and round count."""

import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd.data.shard import row_shards
from asyncframework_amd.data.synthetic import synthetic_csr, synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.native import NativeLocalEngine
from asyncframework_amd.engine.worker import Shard
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.utils.philox import bernoulli_mask

DEV = "cuda:0"
BOUND = 1e-4


def _cfg(**kw):
    base = dict(d=64, N=40_000, num_workers=4, num_iterations=40, gamma=0.3,
                taw=1 << 30, batch_rate=0.05, bucket_ratio=0.5,
                printer_freq=1 << 30, delay_coeff=0.0, seed=42,
                device=DEV, snapshot_weights=False, sync=True)
    base.update(kw)
    return EngineConfig(**base)


def _shards(cfg, X, y):
    return [Shard(row_start=s, n_rows=t - s, X=X[s:t], y=y[s:t])
            for s, t in row_shards(cfg.N, cfg.num_workers)]


def _csr_shards(cfg, indptr, indices, values, y):
    out = []
    for s, t in row_shards(cfg.N, cfg.num_workers):
        base = int(indptr[s])
        out.append(Shard(row_start=s, n_rows=t - s,
                         indptr=(indptr[s:t + 1] - base).contiguous(),
                         indices=indices[base:int(indptr[t])],
                         values=values[base:int(indptr[t])], y=y[s:t]))
    return out


def _engine(cfg, X, y):
    return NativeLocalEngine(cfg, _shards(cfg, X, y), torch.device(DEV))


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def _mask(cfg, k, device):
    return torch.from_numpy(
        bernoulli_mask(cfg.seed, k + 1, 0, cfg.N, cfg.batch_rate)).to(device)


def _ref_sgd(cfg, X, y, rounds, mllib=False):
    """Iterates after each round of sync SGD over the whole dataset: step
    gamma/sqrt(k+1), divisor rate*N (asgd) or the actual count (mllib)."""
    w = torch.zeros(cfg.d, device=X.device)
    out = []
    for k in range(rounds):
        mask = _mask(cfg, k, X.device)
        g, n = torch_ref.grad_dense(X.float(), y, w, mask, cfg.objective)
        div = max(int(mask.sum()), 1) if mllib else cfg.batch_rate * cfg.N
        w = w - (cfg.gamma / math.sqrt(k + 1)) * g / div
        out.append(w.clone())
    return out


@pytest.fixture(scope="module")
def asgd_case():
    """Shared fp32 dataset + closed-form asgd iterates (tests 1, 2, 8)."""
    cfg = _cfg()
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1, device=DEV)
    return X, y, _ref_sgd(cfg, X, y, 40)


def test_sync_asgd_matches_closed_form(asgd_case):
    X, y, ref = asgd_case
    cfg = _cfg()
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120)
    assert res["k"] == 40
    assert res["rejected"] == 0
    assert list(res["waiting_ms"]) == [0.0] * cfg.num_workers
    rel = _rel(eng.w, ref[-1])
    print("asgd P=4 rel", rel)
    assert rel < BOUND, rel


def test_sync_asgd_is_independent_of_P(asgd_case):
    X, y, ref = asgd_case
    ws = {}
    for P in (1, 4, 8):
        cfg = _cfg(num_workers=P)
        eng = _engine(cfg, X, y)
        assert eng.run(max_wall_s=120)["k"] == 40
        ws[P] = eng.w.clone()
    for a, b in ((1, 4), (1, 8), (4, 8)):
        rel = _rel(ws[a], ws[b])
        print(f"P={a} vs P={b} rel", rel)
        assert rel < BOUND, (a, b, rel)


def test_sync_asaga_matches_closed_form():
    cfg = _cfg(algo="asaga", gamma=0.05, num_workers=2)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=4, device=DEV)
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120)
    assert res["k"] == 40 and res["rejected"] == 0
    # one global history table, committed every round; ONE update per round
    w = torch.zeros(cfg.d, device=DEV)
    alpha = torch.zeros(cfg.N, device=DEV)
    alpha_bar = torch.zeros(cfg.d, device=DEV)
    inv_batch = 1.0 / (cfg.batch_rate * cfg.N)
    for k in range(40):
        mask = _mask(cfg, k, DEV)
        g, idx, e, _ = torch_ref.saga_grad_dense(X, y, w, alpha, mask,
                                                 cfg.objective)
        w = w - cfg.gamma * (g * inv_batch + alpha_bar)  # OLD alpha_bar
        alpha_bar = alpha_bar + g / cfg.N
        alpha[idx] = e
    rel_w = _rel(eng.w, w)
    rel_ab = _rel(eng.alpha_bar, alpha_bar)
    print("asaga rel w", rel_w, "alpha_bar", rel_ab)
    assert rel_w < BOUND, rel_w
    assert rel_ab < BOUND, rel_ab
    assert any(int((a != 0).sum()) > 0 for a in eng.alpha_tables)


def test_sync_mllib_divides_by_actual_count_and_resets_counters():
    cfg = _cfg(algo="mllib", batch_rate=0.01, num_iterations=30)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=7, device=DEV)
    ref = _ref_sgd(cfg, X, y, 30, mllib=True)[-1]
    counts = [int(bernoulli_mask(cfg.seed, k + 1, 0, cfg.N,
                                 cfg.batch_rate).sum()) for k in range(30)]
    assert any(c != round(cfg.batch_rate * cfg.N) for c in counts)
    eng = _engine(cfg, X, y)
    assert eng.run(max_wall_s=120)["k"] == 30
    w1 = eng.w.clone()
    rel = _rel(w1, ref)
    print("mllib rel", rel)
    assert rel < BOUND, rel
    # same engine, same buffers, from w=0 again: a counter that survived a
    # round (or the run) would inflate n and shrink every step
    eng.w.zero_()
    assert eng.run(max_wall_s=120)["k"] == 30
    rel2 = _rel(eng.w, ref)
    print("mllib second run rel", rel2, "vs first", _rel(eng.w, w1))
    assert rel2 < BOUND, rel2
    assert _rel(eng.w, w1) < BOUND


def test_sync_csr_asgd_matches_closed_form():
    cfg = _cfg(N=8_000, d=256, batch_rate=0.02, num_iterations=20)
    indptr, indices, values, y = synthetic_csr(cfg.N, cfg.d, seed=11,
                                               device=DEV)
    eng = NativeLocalEngine(cfg, _csr_shards(cfg, indptr, indices, values, y),
                            torch.device(DEV))
    assert eng.run(max_wall_s=120)["k"] == 20
    # the row-loop reference runs on the host (one sync per row otherwise)
    ip, ix, vv, yy = (t.cpu() for t in (indptr, indices, values, y))
    w = torch.zeros(cfg.d)
    for k in range(20):
        mask = _mask(cfg, k, "cpu")
        g, _ = torch_ref.grad_csr(ip, ix, vv, yy, w, mask, cfg.objective)
        w = w - (cfg.gamma / math.sqrt(k + 1)) * g / (cfg.batch_rate * cfg.N)
    rel = _rel(eng.w.cpu(), w)
    print("csr rel", rel)
    assert rel < BOUND, rel


def test_sync_generic_fallback_d_not_multiple_of_4():
    cfg = _cfg(d=66, num_workers=2, num_iterations=20)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=8, device=DEV)
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120)
    assert res["k"] == 20 and res["rejected"] == 0
    rel = _rel(eng.w, _ref_sgd(cfg, X, y, 20)[-1])
    print("d=66 rel", rel)
    assert rel < BOUND, rel


def test_sync_asgd_bf16():
    cfg = _cfg(dtype="bf16")
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1, device=DEV,
                           dtype=torch.bfloat16)
    eng = _engine(cfg, X, y)
    assert eng.run(max_wall_s=120)["k"] == 40
    rel = _rel(eng.w, _ref_sgd(cfg, X, y, 40)[-1])  # ref reads X.float()
    print("bf16 rel", rel)
    assert rel < BOUND, rel


def test_sync_snapshots(asgd_case):
    X, y, ref = asgd_case
    eng = _engine(_cfg(), X, y)
    res = eng.run(max_wall_s=120, snapshot_every=10)
    ov = res["opt_vars"]
    assert len(ov) == 1 + 4
    assert ov[0][0] == 0 and float(ov[0][1].abs().sum()) == 0.0
    times = [t for t, _ in ov]
    assert times == sorted(times)
    for j in range(1, 5):
        rel = _rel(ov[j][1].to(DEV), ref[10 * (j - 1)])
        print("snapshot", j, "rel", rel)
        assert rel < BOUND, (j, rel)


def test_sync_delay_model():
    cfg = _cfg(num_workers=8, num_iterations=300, delay_coeff=-1.0,
               calib_factor=3, N=80_000)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=5, device=DEV)
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120)
    assert res["k"] == 300
    assert res["avg_delay_ms"] > 0  # calibration activated


def test_sync_bench_marks():
    cfg = _cfg(num_iterations=10 ** 9)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=6, device=DEV)
    eng = _engine(cfg, X, y)
    elapsed, res = eng.bench(warmup=10, steps=40, max_wall_s=120)
    assert elapsed > 0
    assert res["k"] >= 50


def _check_stdout_contract(out):
    lines = out.splitlines()
    assert lines[-1] == "finished"
    assert any(l.startswith("Iteration ") for l in lines)
    assert "Individual waiting times:" in lines
    sep = max(i for i, l in enumerate(lines) if l.startswith("*********"))
    csv = [l for l in lines[sep + 1:] if re.match(r"^\d+,[0-9.eE+-]+$", l)]
    assert len(csv) >= 2
    objs = [float(l.split(",")[1]) for l in csv]
    assert objs[-1] < objs[0]


def test_sync_cli_asgd_sync_native(capsys):
    from asyncframework_amd.cli import drivers
    drivers.asgd_sync(["synthetic", "synthetic", "64", "20000", "4", "60",
                       "0.3", "1000000", "0.05", "0.5", "20", "0", "42",
                       "--device", DEV, "--engine", "native"])
    _check_stdout_contract(capsys.readouterr().out)


def test_sync_cli_sgd_mllib_native(capsys):
    from asyncframework_amd.cli import drivers
    drivers.sgd_mllib(["synthetic", "synthetic", "64", "20000", "4", "250",
                       "0.3", "0.05", "--device", DEV, "--engine", "native"])
    _check_stdout_contract(capsys.readouterr().out)
