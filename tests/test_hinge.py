"""objective="hinge" on the CPU tier: the torch reference against MLlib's
HingeGradient.compute written out below, one closed-form SyncEngine round
per algorithm, the sweep at w = 0 and the LBFGS refusal."""

import math

import numpy as np
import pytest
import torch

from asyncframework_amd import ops
from asyncframework_amd.algos.lbfgs import LBFGS
from asyncframework_amd.data.synthetic import synthetic_csr, synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.local import SyncEngine
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.run import build_csr_workers, build_dense_workers
from asyncframework_amd.utils.philox import bernoulli_mask


def _scala_hinge(z: float, label: float):
    """HingeGradient.compute: (gradient coefficient on x, loss)."""
    label_scaled = 2 * label - 1.0
    if 1.0 > label_scaled * z:
        return -label_scaled, 1.0 - label_scaled * z
    return 0.0, 0.0


# s*z == 1 exactly in rows 2 and 3: the strict inequality gives 0 there
_Z = [0.0, 0.5, 1.0, -1.0, 1.5, -1.5, 0.999, -0.999, -3.0, 3.0, 1.0, -1.0]
_Y = [1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0]


def test_hinge_coefficient_and_loss_match_scala_definition():
    z = torch.tensor(_Z)
    y = torch.tensor(_Y)
    want = [_scala_hinge(a, b) for a, b in zip(_Z, _Y)]
    e = torch_ref._link(z, y, "hinge")
    assert e.tolist() == [c for c, _ in want]
    assert e[2] == 0.0 and e[3] == 0.0  # on the margin
    loss = torch_ref._row_loss(z.double()[:, None], y, "hinge")[:, 0]
    assert torch.allclose(loss, torch.tensor([l for _, l in want],
                                             dtype=torch.float64),
                          rtol=0, atol=1e-7)  # 0.999 is not exact in fp32
    # through X @ w: d = 1, x = z, w = 1
    e2 = torch_ref._residual(z[:, None], y, torch.ones(1), "hinge")
    assert torch.equal(e, e2)


def test_hinge_grad_dense_and_csr_against_row_loop():
    n, d = 64, 12
    g = torch.Generator().manual_seed(3)
    X = torch.randn(n, d, generator=g)
    y = (torch.rand(n, generator=g) > 0.5).float()
    w = torch.randn(d, generator=g) * 0.7
    mask = torch.from_numpy(bernoulli_mask(5, 2, 0, n, 0.6))
    want = torch.zeros(d, dtype=torch.float64)
    kinds = set()
    for i in mask.nonzero()[:, 0].tolist():
        c, _ = _scala_hinge(float(X[i].double() @ w.double()), float(y[i]))
        kinds.add(c != 0.0)
        want += c * X[i].double()
    assert kinds == {True, False}
    got, cnt = torch_ref.grad_dense(X, y, w, mask, "hinge")
    assert cnt == int(mask.sum())
    assert torch.allclose(got.double(), want, atol=1e-5)
    # the same rows as CSR
    indptr = torch.arange(0, n * d + 1, d, dtype=torch.int32)
    indices = torch.arange(d, dtype=torch.int32).repeat(n)
    got_csr, _ = torch_ref.grad_csr(indptr, indices, X.reshape(-1), y, w,
                                    mask, "hinge")
    assert torch.allclose(got_csr.double(), want, atol=1e-5)
    alpha = torch.randn(n, generator=g)
    gs, idx, e, _ = torch_ref.saga_grad_csr(indptr, indices, X.reshape(-1),
                                            y, w, alpha, mask, "hinge")
    gd, idx_d, e_d, _ = torch_ref.saga_grad_dense(X, y, w, alpha, mask,
                                                  "hinge")
    assert torch.equal(idx, idx_d) and torch.allclose(e, e_d)
    assert torch.allclose(gs, gd, atol=1e-5)
    assert set(e.tolist()) <= {-1.0, 0.0, 1.0}


def _cfg(algo, l2, **kw):
    base = dict(d=16, N=400, num_workers=2, num_iterations=1, gamma=0.25,
                batch_rate=0.3, bucket_ratio=1.0, printer_freq=1000,
                delay_coeff=0.0, seed=7, device="cpu", sync=True, algo=algo,
                objective="hinge", snapshot_weights=False, l2=l2)
    base.update(kw)
    return EngineConfig(**base)


@pytest.mark.parametrize("l2", [0.0, 0.1])
@pytest.mark.parametrize("algo", ["asgd", "asaga", "mllib"])
def test_sync_round_from_zero_is_the_exact_masked_sum(algo, l2):
    """At w = 0 every score is 0, so every row is inside the margin and its
    coefficient is -s: the round's gradient is the exact sum of -s_i x_i
    over the Philox mask. w = 0 also makes the l2 decay of this first step
    vanish (v = w - eta*(ghat + l2*w)), so both l2 cases share the value."""
    cfg = _cfg(algo, l2)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=3, objective="hinge")
    assert set(y.tolist()) == {0.0, 1.0}
    eng = SyncEngine(cfg, build_dense_workers(cfg, X, y))
    eng.verbose = False
    res = eng.run(max_wall_s=60)
    assert res.k == 1
    mask = torch.from_numpy(
        bernoulli_mask(cfg.seed, 1, 0, cfg.N, cfg.batch_rate))
    s = 2.0 * y.double() - 1.0
    g = -(X.double()[mask] * s[mask][:, None]).sum(dim=0)
    n = int(mask.sum())
    assert 0 < n < cfg.N
    if algo == "asgd":
        want = -cfg.gamma * g / (cfg.batch_rate * cfg.N)
    elif algo == "mllib":
        want = -cfg.gamma * g / n
    else:
        want = -cfg.gamma * g / (cfg.batch_rate * cfg.N)
        ab = eng.server.alpha_bar.double()
        assert torch.allclose(ab, g / cfg.N, rtol=1e-5, atol=1e-7)
    assert torch.allclose(res.w.double(), want, rtol=1e-5, atol=1e-7)
    assert float(res.w.abs().max()) > 0


def test_sync_csr_round_from_zero():
    cfg = _cfg("asgd", 0.0, d=50)
    data = synthetic_csr(cfg.N, cfg.d, nnz_per_row=6, seed=4,
                         objective="hinge")
    indptr, indices, values, y = data
    assert set(y.tolist()) == {0.0, 1.0}
    eng = SyncEngine(cfg, build_csr_workers(cfg, *data))
    eng.verbose = False
    res = eng.run(max_wall_s=60)
    mask = bernoulli_mask(cfg.seed, 1, 0, cfg.N, cfg.batch_rate)
    g = np.zeros(cfg.d)
    for i in np.nonzero(mask)[0]:
        a, b = int(indptr[i]), int(indptr[i + 1])
        np.add.at(g, indices[a:b].numpy(),
                  -(2.0 * float(y[i]) - 1.0) * values[a:b].double().numpy())
    want = torch.from_numpy(-cfg.gamma * g / (cfg.batch_rate * cfg.N))
    assert torch.allclose(res.w.double(), want, rtol=1e-5, atol=1e-7)


def test_objective_sweep_hinge_at_zero_is_exactly_one():
    X, y = synthetic_dense(300, 20, seed=5, objective="hinge")
    W = torch.zeros(3, 20)
    assert ops.objective_sweep(X, y, W, "hinge").tolist() == [1.0] * 3
    data = synthetic_csr(300, 40, nnz_per_row=5, seed=6, objective="hinge")
    W = torch.zeros(2, 40)
    assert ops.objective_sweep_csr(*data, W, "hinge").tolist() == [1.0] * 2
    # the penalty constant of hinge is 1, as for logistic
    W1 = torch.ones(1, 20)
    assert float(torch_ref.penalty(W1, "hinge", 0.5, 0.25)[0]) == \
        0.5 * 0.5 * 20 + 0.25 * 20


def test_hinge_training_lowers_the_hinge_objective():
    cfg = _cfg("asgd", 0.01, num_iterations=60, gamma=1.0)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=8, objective="hinge")
    eng = SyncEngine(cfg, build_dense_workers(cfg, X, y))
    eng.verbose = False
    res = eng.run(max_wall_s=60)
    obj = ops.objective_sweep(X, y, res.w[None], "hinge")
    assert float(obj[0]) < 1.0


def test_lbfgs_refuses_hinge():
    with pytest.raises(ValueError, match="non-smooth"):
        LBFGS(objective="hinge")
    LBFGS(objective="logistic")


def test_unknown_objective_is_an_error():
    with pytest.raises(ValueError):
        torch_ref._link(torch.zeros(1), torch.zeros(1), "huber")
    assert ops._OBJ_CODE["hinge"] == 2
    from asyncframework_amd.engine.native import _OBJ
    assert _OBJ == ops._OBJ_CODE
    assert math.isclose(ops.score_threshold("hinge"), 0.0)
