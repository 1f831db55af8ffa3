"""Elastic-net (l2 / l1) regularisation on the CPU tier: the torch update
ops against the contract written out in fp64, the Python engines against
hand loops over the same Philox masks, the exact-zero property of the
soft-threshold, MLlib's SquaredL2Updater / L1Updater written out from their
definitions, the penalised objective sweep, ridge via L-BFGS, the engines
that refuse a penalty, the CLI flags and the checkpoint warning.

Contract (one applied step, step size eta, normalised data direction ghat):
    v = w - eta*(ghat + l2*w)
    w = v > t ? v - t : (v < -t ? v + t : +0),  t = eta*l1
asgd: eta = gamma_k; mllib: eta = gamma/sqrt(k+1), ghat = s/max(n,1);
asaga: eta = gamma, ghat = inv_batch*g + alpha_bar_old, and afterwards
alpha_bar += g/N with no penalty in it."""

import io
import math
import re
import warnings
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from asyncframework_amd import ops
from asyncframework_amd import run as runner
from asyncframework_amd.algos import LBFGS
from asyncframework_amd.data.synthetic import synthetic_csr, synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.server import Server
from asyncframework_amd.engine.worker import Shard
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.utils.philox import bernoulli_mask

L2, L1 = 0.1, 0.01


def _soft64(v, t):
    return np.where(v > t, v - t, np.where(v < -t, v + t, 0.0))


def _csv_objs(lines):
    """The time_ms,objective lines of the epilogue (after the separator)."""
    sep = max(i for i, l in enumerate(lines) if l.startswith("*********"))
    return [float(l.split(",")[1]) for l in lines[sep + 1:]
            if re.match(r"^\d+,[0-9.eE+-]+$", l)]


def _step64(w, ghat, eta, l2, l1):
    return _soft64(w - eta * (ghat + l2 * w), eta * l1)


# ------------------------------------------------------------------ ops layer

def _vecs(d=37, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(d, generator=gen), torch.randn(d, generator=gen),
            torch.randn(d, generator=gen))


@pytest.mark.parametrize("l2,l1", [(0.25, 0.0), (0.0, 0.8), (0.25, 0.8)])
def test_torch_ref_sgd_update_matches_fp64_contract(l2, l1):
    w, g, _ = _vecs()
    gamma_k, inv_batch = 0.3, 0.5
    ref = _step64(w.double().numpy(), inv_batch * g.double().numpy(), gamma_k,
                  l2, l1)
    torch_ref.sgd_update(w, g, gamma_k, inv_batch, l2=l2, l1=l1)
    assert np.abs(w.double().numpy() - ref).max() < 1e-6
    if l1:
        clipped = ref == 0.0
        assert clipped.any() and (~clipped).any()
        assert bool((w[torch.from_numpy(clipped)] == 0).all())


@pytest.mark.parametrize("l2,l1", [(0.25, 0.0), (0.0, 0.8), (0.25, 0.8)])
def test_torch_ref_saga_update_matches_fp64_contract(l2, l1):
    w, g, ab = _vecs(seed=1)
    gamma, inv_batch, inv_N = 0.3, 0.5, 0.125
    w64, g64, ab64 = (t.double().numpy() for t in (w, g, ab))
    ref = _step64(w64, inv_batch * g64 + ab64, gamma, l2, l1)
    ab_ref = ab64 + inv_N * g64  # no penalty in alpha_bar
    torch_ref.saga_update(w, g, ab, gamma, inv_batch, inv_N, l2=l2, l1=l1)
    assert np.abs(w.double().numpy() - ref).max() < 1e-6
    assert np.abs(ab.double().numpy() - ab_ref).max() < 1e-6
    if l1:
        assert (ref == 0.0).any() and (ref != 0.0).any()


def test_explicit_zero_penalties_are_bit_identical():
    w, g, ab = _vecs(seed=2)
    for fn in (torch_ref, ops):
        a, b = w.clone(), w.clone()
        fn.sgd_update(a, g, 0.3, 0.5)
        fn.sgd_update(b, g, 0.3, 0.5, l2=0.0, l1=0.0)
        assert torch.equal(a, b)
        a, b, aba, abb = w.clone(), w.clone(), ab.clone(), ab.clone()
        fn.saga_update(a, g, aba, 0.3, 0.5, 0.125)
        fn.saga_update(b, g, abb, 0.3, 0.5, 0.125, l2=0.0, l1=0.0)
        assert torch.equal(a, b) and torch.equal(aba, abb)


def test_ops_update_routes_penalties_on_cpu():
    w, g, _ = _vecs(seed=3)
    a, b = w.clone(), w.clone()
    ops.sgd_update(a, g, 0.3, 0.5, l2=0.25, l1=0.8)
    torch_ref.sgd_update(b, g, 0.3, 0.5, l2=0.25, l1=0.8)
    assert torch.equal(a, b)
    with pytest.raises(TypeError):
        ops.sgd_update(a, g, 0.3, 0.5, 0.25, 0.8)  # keyword-only


# ---------------------------------------------------- engines vs a hand loop

def _cfg(**kw):
    base = dict(d=32, N=512, num_workers=4, num_iterations=30, gamma=0.3,
                taw=2 ** 30, batch_rate=0.25, bucket_ratio=0.5,
                printer_freq=1 << 30, delay_coeff=0.0, seed=42, device="cpu",
                snapshot_weights=False, l2=L2, l1=L1)
    base.update(kw)
    return EngineConfig(**base)


def _mask(cfg, k):
    return torch.from_numpy(
        bernoulli_mask(cfg.seed, k + 1, 0, cfg.N, cfg.batch_rate))


def _soft(v, t):
    return torch.where(v > t, v - t,
                       torch.where(v < -t, v + t, torch.zeros_like(v)))


def _hand_loop(cfg, X, y, rounds, mode, inv_batch):
    """Whole-dataset loop, contract formulas inline (no update op).
    mode: 'asgd' (divisor 1/inv_batch), 'mllib' (actual count), 'asaga'.
    Returns (w, alpha_bar)."""
    w = torch.zeros(cfg.d)
    ab = torch.zeros(cfg.d)
    alpha = torch.zeros(cfg.N)
    for k in range(rounds):
        mask = _mask(cfg, k)
        if mode == "asaga":
            g, idx, e, _ = torch_ref.saga_grad_dense(X, y, w, alpha, mask,
                                                     cfg.objective)
            eta = cfg.gamma
            ghat = inv_batch * g + ab
            ab = ab + g / cfg.N
            alpha[idx] = e
        else:
            g, n = torch_ref.grad_dense(X, y, w, mask, cfg.objective)
            eta = cfg.gamma / math.sqrt(k + 1)
            ghat = g / max(n, 1) if mode == "mllib" else inv_batch * g
        w = _soft(w - eta * (ghat + cfg.l2 * w), eta * cfg.l1)
    return w, ab


@pytest.mark.parametrize("algo", ["asgd", "asaga", "mllib"])
def test_sync_engine_matches_hand_loop(algo):
    cfg = _cfg(sync=True, algo=algo, gamma=0.1 if algo == "asaga" else 0.3)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1)
    res, srv = runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                                 verbose=False)
    assert res.k == cfg.num_iterations
    w, ab = _hand_loop(cfg, X, y, cfg.num_iterations, algo,
                       1.0 / (cfg.batch_rate * cfg.N))
    assert torch.allclose(res.w, w, atol=1e-5), float((res.w - w).abs().max())
    if algo == "asaga":
        assert torch.allclose(srv.alpha_bar, ab, atol=1e-5)
    # the penalty is really in the run: the same engine without it differs
    cfg0 = _cfg(sync=True, algo=algo, gamma=cfg.gamma, l2=0.0, l1=0.0)
    res0, _ = runner.run_engine(cfg0, runner.build_dense_workers(cfg0, X, y),
                                verbose=False)
    assert float((res0.w - w).norm() / w.norm()) > 0.05


@pytest.mark.parametrize("algo", ["asgd", "asaga"])
def test_async_engine_one_worker_matches_hand_loop(algo):
    cfg = _cfg(sync=False, algo=algo, num_workers=1,
               gamma=0.1 if algo == "asaga" else 0.3)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=2)
    res, srv = runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                                 verbose=False)
    k = res.k
    assert k >= cfg.num_iterations and res.applied == k
    # one worker: round j is computed at the iterate after j updates, with
    # step gamma/sqrt(j // 1 + 1) and divisor par_recs = b*N/1
    w, ab = _hand_loop(cfg, X, y, k, algo, 1.0 / cfg.par_recs)
    assert torch.allclose(res.w, w, atol=1e-5), float((res.w - w).abs().max())
    if algo == "asaga":
        assert torch.allclose(srv.alpha_bar, ab, atol=1e-5)


# --------------------------------------------------------- exact-zero property

@pytest.mark.parametrize("algo,sync", [("asgd", True), ("asaga", True),
                                       ("mllib", True), ("asgd", False),
                                       ("asaga", False)])
def test_w_stays_exactly_zero_above_the_l1_threshold(algo, sync):
    """batch_rate = 1: the minibatch is the whole set, so at w = 0 every
    round's ghat is -X^T y / N. With l1 = 1.5 * its inf-norm the prox clips
    every coordinate, every round: w never leaves exactly 0."""
    N, d = 256, 16
    X, y = synthetic_dense(N, d, seed=3)
    l1 = 1.5 * float((X.double().t() @ y.double() / N).abs().max())
    cfg = _cfg(d=d, N=N, num_workers=2 if sync else 1, num_iterations=12,
               batch_rate=1.0, sync=sync, algo=algo, l1=l1, l2=0.05,
               snapshot_weights=True, printer_freq=1)
    res, srv = runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                                 verbose=False)
    applied = res.k if sync else res.applied
    assert applied > 0
    assert len(res.opt_vars) >= applied  # every round's iterate was recorded
    for _, wk in res.opt_vars:
        assert torch.equal(wk, torch.zeros(d))
    assert torch.equal(res.w, torch.zeros(d))
    assert not bool(torch.signbit(res.w).any())  # clipped value is +0.0
    if algo == "asaga":
        assert float(srv.alpha_bar.abs().max()) > 0


# ---------------------------------------------------- MLlib updaters, by hand

def _squared_l2_updater(w, grad, step, it, reg):
    """Updater.scala SquaredL2Updater.compute:
    thisIterStepSize = stepSize / sqrt(iter);
    w := w * (1 - thisIterStepSize*regParam) - thisIterStepSize * gradient"""
    s = step / math.sqrt(it)
    return w * (1.0 - s * reg) - s * grad


def _l1_updater(w, grad, step, it, reg):
    """Updater.scala L1Updater.compute: take the gradient step, then
    w_i := signum(w_i) * max(0, |w_i| - regParam*thisIterStepSize)."""
    s = step / math.sqrt(it)
    w = w - s * grad
    shrink = reg * s
    return np.sign(w) * np.maximum(0.0, np.abs(w) - shrink)


@pytest.mark.parametrize("which", ["l2", "l1"])
def test_mllib_mode_reproduces_mllib_updaters(which):
    reg = 0.2 if which == "l2" else 0.05
    cfg = _cfg(sync=True, algo="mllib", l2=reg if which == "l2" else 0.0,
               l1=reg if which == "l1" else 0.0)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=4)
    res, _ = runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                               verbose=False)
    upd = _squared_l2_updater if which == "l2" else _l1_updater
    X64, y64 = X.double().numpy(), y.double().numpy()
    w = np.zeros(cfg.d)
    for k in range(cfg.num_iterations):
        m = _mask(cfg, k).numpy()
        grad = X64[m].T @ (X64[m] @ w - y64[m]) / max(int(m.sum()), 1)
        w = upd(w, grad, cfg.gamma, k + 1, reg)  # MLlib iterations from 1
    err = np.abs(res.w.double().numpy() - w).max()
    assert err < 1e-5, err


# ------------------------------------------------------------ objective sweep

@pytest.mark.parametrize("objective,c", [("lsq", 2.0), ("logistic", 1.0)])
def test_objective_sweep_adds_closed_form_penalty(objective, c):
    X, y = synthetic_dense(200, 12, seed=5, objective=objective)
    W = torch.randn(4, 12, generator=torch.Generator().manual_seed(6))
    W[0] = 0
    pen = c * (0.5 * L2 * (W.double() ** 2).sum(1) + L1 * W.double().abs().sum(1))
    for fn in (ops, torch_ref):
        base = fn.objective_sweep(X, y, W, objective)
        reg = fn.objective_sweep(X, y, W, objective, l2=L2, l1=L1)
        assert reg.dtype == torch.float64
        assert torch.allclose(reg, base + pen, rtol=0, atol=1e-12)
        assert torch.equal(fn.objective_sweep(X, y, W, objective, l2=0.0,
                                              l1=0.0), base)
    assert float(pen[1]) > 0 and float(pen[0]) == 0


@pytest.mark.parametrize("objective,c", [("lsq", 2.0), ("logistic", 1.0)])
def test_objective_sweep_csr_adds_closed_form_penalty(objective, c):
    indptr, indices, values, y = synthetic_csr(120, 24, nnz_per_row=5, seed=7,
                                               objective=objective)
    W = torch.randn(3, 24, generator=torch.Generator().manual_seed(8))
    pen = c * (0.5 * L2 * (W.double() ** 2).sum(1) + L1 * W.double().abs().sum(1))
    for fn in (ops, torch_ref):
        base = fn.objective_sweep_csr(indptr, indices, values, y, W, objective)
        reg = fn.objective_sweep_csr(indptr, indices, values, y, W, objective,
                                     l2=L2, l1=L1)
        assert torch.allclose(reg, base + pen, rtol=0, atol=1e-12)


def test_final_report_prints_the_penalised_objective():
    cfg = EngineConfig(d=8, N=64, num_workers=2, objective="lsq", l2=0.5,
                       l1=0.25)
    data = runner.load_dataset(cfg, "synthetic", "synthetic")
    from asyncframework_amd.engine.local import RunResult
    wv = torch.full((8,), 0.5)
    res = RunResult(k=2, elapsed_ms=1, opt_vars=[(0, torch.zeros(8)), (5, wv)],
                    waiting_time={0: 1}, w=wv)

    def objs(c):
        buf = io.StringIO()
        with redirect_stdout(buf):
            runner.final_report(c, res, data, sparse=False)
        return _csv_objs(buf.getvalue().splitlines())
    plain = objs(EngineConfig(d=8, N=64, num_workers=2, objective="lsq"))
    reg = objs(cfg)
    assert len(plain) == len(reg) == 2
    assert reg[0] == plain[0]  # w = 0 carries no penalty
    expect = 2.0 * (0.5 * 0.5 * 8 * 0.25 + 0.25 * 8 * 0.5)
    assert abs(reg[1] - plain[1] - expect) < 1e-4 * max(1.0, plain[1])


# ---------------------------------------------------------------------- LBFGS

def test_lbfgs_l2_reaches_the_ridge_solution():
    X, y = synthetic_dense(2000, 30, seed=0, dtype=torch.float32,
                           device=torch.device("cpu"), objective="lsq")
    lam = 0.5
    w = LBFGS(max_iter=200, printer_freq=10, l2=lam).optimize(X, y)
    Xd, yd = X.double(), y.double()
    N = X.shape[0]
    w_star = torch.linalg.solve(Xd.t() @ Xd / N + lam * torch.eye(30).double(),
                                Xd.t() @ yd / N)

    def F(v):  # mean r^2 + 2*(lam/2)|v|^2: twice the ridge objective
        return float(((Xd @ v - yd) ** 2).mean() + lam * v.dot(v))
    # tolerance of tests/test_lbfgs.py against scipy
    assert F(w.double()) <= F(w_star) * 1.02 + 1e-6
    w_plain = LBFGS(max_iter=200, printer_freq=10).optimize(X, y)
    assert F(w_plain.double()) > F(w_star) * 1.02 + 1e-6  # l2 did the work
    with pytest.raises(TypeError):
        LBFGS(l1=0.1)  # non-smooth: not offered
    with pytest.raises(ValueError):
        LBFGS(l2=-1.0)


# ------------------------------------------------- validation and refusals

@pytest.mark.parametrize("kw", [dict(l2=-1e-3), dict(l1=-1.0),
                                dict(l2=float("nan")), dict(l1=float("inf"))])
def test_bad_penalties_raise_value_error(kw):
    cfg = _cfg(**{**dict(l2=0.0, l1=0.0), **kw})
    with pytest.raises(ValueError, match="l[12]"):
        Server(cfg)
    from asyncframework_amd.engine.native import NativeLocalEngine
    with pytest.raises(ValueError, match="l[12]"):
        # ahead of the GPU-only assert and of the extension import
        NativeLocalEngine(cfg, [], torch.device("cpu"))


def _tiny_shard(cfg):
    X, y = synthetic_dense(cfg.N, cfg.d, seed=9)
    return Shard(row_start=0, n_rows=cfg.N, X=X, y=y)


@pytest.mark.parametrize("kw", [dict(l2=0.1, l1=0.0), dict(l2=0.0, l1=0.1)])
def test_uncovered_engines_refuse_penalties_by_name(kw):
    cfg = _cfg(num_workers=1, **kw)
    cpu = torch.device("cpu")
    from asyncframework_amd.engine.dist_native import NativeDistEngine
    from asyncframework_amd.engine.graph import GraphEngine
    from asyncframework_amd.engine.resident import ResidentEngine
    with pytest.raises(AssertionError, match="GraphEngine.*l1/l2"):
        GraphEngine(cfg, _tiny_shard(cfg), cpu)
    with pytest.raises(AssertionError, match="ResidentEngine.*l1/l2"):
        ResidentEngine(cfg, [_tiny_shard(cfg)], cpu)
    with pytest.raises(AssertionError, match="NativeDistEngine.*l1/l2"):
        NativeDistEngine(cfg, [], cpu)
    # the message names what to use instead
    with pytest.raises(AssertionError, match="native engine"):
        GraphEngine(cfg, _tiny_shard(cfg), cpu)


# ------------------------------------------------------------------------ CLI

_ARGS13 = ["synthetic", "synthetic", "16", "256", "2", "40", "0.3", "1000000",
           "0.25", "0.5", "10", "0", "42"]


def test_cli_flags_parse_into_the_config(monkeypatch):
    from asyncframework_amd.cli import drivers
    seen = {}
    monkeypatch.setattr(drivers, "_run",
                        lambda cfg, a, *r: seen.setdefault("cfg", cfg))
    for drv in (drivers.asgd_thread, drivers.asgd_sync, drivers.asaga_thread,
                drivers.asaga_sync):
        seen.clear()
        drv(_ARGS13 + ["--l2", "1e-3", "--l1", "2e-4"])
        assert (seen["cfg"].l2, seen["cfg"].l1) == (1e-3, 2e-4)
        seen.clear()
        drv(_ARGS13)
        assert (seen["cfg"].l2, seen["cfg"].l1) == (0.0, 0.0)


def _cli_objs(drv, argv, capsys):
    drv(argv)
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1] == "finished"
    return lines, _csv_objs(lines)


def test_cli_threads_run_changes_the_objective_lines(capsys):
    from asyncframework_amd.cli import drivers
    l0, plain = _cli_objs(drivers.asgd_sync, _ARGS13, capsys)
    l1, reg = _cli_objs(drivers.asgd_sync, _ARGS13 + ["--l2", "0.5", "--l1",
                                                      "0.05"], capsys)
    assert len(l0) == len(l1)  # stdout contract: no new lines
    assert len(plain) == len(reg) >= 2
    assert plain[0] == reg[0]  # w = 0
    assert all(abs(a - b) > 1e-6 for a, b in zip(plain[1:], reg[1:]))
    _, mreg = _cli_objs(drivers.sgd_mllib,
                        ["synthetic", "synthetic", "16", "256", "2", "150",
                         "0.3", "0.25", "--l2", "0.5"], capsys)
    _, mplain = _cli_objs(drivers.sgd_mllib,
                          ["synthetic", "synthetic", "16", "256", "2", "150",
                           "0.3", "0.25"], capsys)
    assert len(mreg) == len(mplain) >= 2 and mreg[-1] != mplain[-1]


def test_cli_negative_penalty_raises(capsys):
    from asyncframework_amd.cli import drivers
    with pytest.raises(ValueError, match="l2"):
        drivers.asgd_thread(_ARGS13 + ["--l2", "-0.1"])
    with pytest.raises(ValueError, match="l1"):
        drivers.sgd_mllib(["synthetic", "synthetic", "16", "256", "2", "10",
                           "0.3", "0.25", "--l1", "-1"])
    assert capsys.readouterr().out == ""  # refused before the header


# ----------------------------------------------------------------- checkpoint

def test_checkpoint_carries_penalties_and_warns_on_mismatch():
    from asyncframework_amd.engine.checkpoint import capture_state, restore
    cfg = _cfg()
    state = capture_state(Server(cfg))
    assert state["cfg"]["l2"] == L2 and state["cfg"]["l1"] == L1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        restore(Server(_cfg()), None, state)  # same penalties: silent
    with pytest.warns(RuntimeWarning, match="l2"):
        restore(Server(_cfg(l2=0.0)), None, state)
    with pytest.warns(RuntimeWarning, match="l1"):
        restore(Server(_cfg(l1=0.5)), None, state)
    old = dict(state, cfg={k: v for k, v in state["cfg"].items()
                           if k not in ("l1", "l2")})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        restore(Server(_cfg(l1=0.0, l2=0.0)), None, old)  # pre-feature file
