"""Checkpoint and resume of the native engine (csrc/engine_native.cpp) on
MI355X, async and sync, against the closed forms of
tests/test_gpu_native_sync.py and tests/test_gpu_native.py at their shapes
(d=64, N=40,000 — 20,000 at P=1 async —, rate 0.05, fp32, lsq).

BOUND = 1e-4 is the bound those files already hold these kernels to against
the same closed forms. It is also what separates a consistent SAGA state
from an inconsistent one: one uncommitted round of one worker shows as
~1e-3 in rel(alpha_bar, X^T alpha / N) around k = 80, a consistent state as
~1e-7 (docs/TESTING.md). Every measured rel is printed."""

import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import run as runner
from asyncframework_amd.data.shard import row_shards
from asyncframework_amd.data.synthetic import synthetic_csr, synthetic_dense
from asyncframework_amd.engine.checkpoint import load_checkpoint
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


def _acfg(**kw):
    """Async base of tests/test_gpu_native.py (P=1, N=20,000)."""
    base = dict(N=20_000, num_workers=1, num_iterations=60, sync=False)
    base.update(kw)
    return _cfg(**base)


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


def _dense_engine(cfg, data):
    return NativeLocalEngine(cfg, _shards(cfg, *data), torch.device(DEV))


def _csr_engine(cfg, data):
    return NativeLocalEngine(cfg, _csr_shards(cfg, *data), torch.device(DEV))


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _mask(cfg, k, device):
    return torch.from_numpy(
        bernoulli_mask(cfg.seed, k + 1, 0, cfg.N, cfg.batch_rate)).to(device)


def _ref_sgd(cfg, X, y, rounds, mllib=False):
    """Iterates after each round of sync SGD over the whole dataset: step
    gamma/sqrt(k+1), divisor rate*N (asgd) or the actual count (mllib).
    At P=1 this is also the async engine's sequential algorithm."""
    w = torch.zeros(cfg.d, device=X.device)
    out = []
    for k in range(rounds):
        mask = _mask(cfg, k, X.device)
        g, _ = torch_ref.grad_dense(X.float(), y, w, mask, cfg.objective)
        div = max(int(mask.sum()), 1) if mllib else cfg.batch_rate * cfg.N
        w = w - (cfg.gamma / math.sqrt(k + 1)) * g / div
        out.append(w.clone())
    return out


def _ref_saga(cfg, X, y, rounds):
    """(w, alpha_bar, alpha) after each round of SAGA with one global
    history table committed every round — the sync closed form, and at P=1
    the async engine's sequential algorithm."""
    w = torch.zeros(cfg.d, device=X.device)
    alpha = torch.zeros(cfg.N, device=X.device)
    alpha_bar = torch.zeros(cfg.d, device=X.device)
    inv_batch = 1.0 / (cfg.batch_rate * cfg.N)
    out = []
    for k in range(rounds):
        mask = _mask(cfg, k, X.device)
        g, idx, e, _ = torch_ref.saga_grad_dense(X, y, w, alpha, mask,
                                                 cfg.objective)
        w = w - cfg.gamma * (g * inv_batch + alpha_bar)  # OLD alpha_bar
        alpha_bar = alpha_bar + g / cfg.N
        alpha[idx] = e
        out.append((w.clone(), alpha_bar.clone(), alpha.clone()))
    return out


def _alpha(eng_or_state):
    """History concatenated by worker id (engine tables or file contents)."""
    if isinstance(eng_or_state, dict):
        tabs = eng_or_state["alpha"]
        return torch.cat([tabs[i].cpu() for i in sorted(tabs)])
    return torch.cat([t.cpu() for t in eng_or_state.alpha_tables])


def _identity_dense(X, alpha_bar, alpha):
    """rel(alpha_bar, X^T alpha / N) in fp64 — an identity of SAGA at any
    quiescent point (lsq: row i's stored gradient is alpha_i * x_i)."""
    Xd = X.detach().cpu().double()
    ref = Xd.t() @ alpha.detach().cpu().double() / X.shape[0]
    return _rel(alpha_bar, ref)


def _identity_csr(data, d, alpha_bar, alpha):
    indptr, indices, values, _ = (t.detach().cpu() for t in data)
    n = indptr.shape[0] - 1
    rows = torch.repeat_interleave(torch.arange(n),
                                   (indptr[1:] - indptr[:-1]).long())
    ref = torch.zeros(d, dtype=torch.float64)
    ref.index_add_(0, indices.long(),
                   values.double() * alpha.detach().cpu().double()[rows])
    return _rel(alpha_bar, ref / n)


def _objective(X, y, w):
    return float(((X.float() @ w.to(X.device).float() - y) ** 2).mean())


def _run_to_checkpoint(make_engine, data, path, upto, every, **kw):
    """Fresh engine, run to ``upto`` with checkpointing every ``every``."""
    cfg = _cfg(num_iterations=upto, checkpoint_path=path,
               checkpoint_every=every, **kw)
    eng = make_engine(cfg, data)
    res = eng.run(max_wall_s=120)
    return eng, res


def _resume(make_engine, data, path, upto, **kw):
    """Fresh engine restored from the file, run to ``upto`` in total."""
    cfg = _cfg(num_iterations=upto, **kw)
    eng = make_engine(cfg, data)
    eng.restore_state(load_checkpoint(path))
    res = eng.run(max_wall_s=120)
    return eng, res


@pytest.fixture(scope="module")
def asgd_case():
    """Shared fp32 dataset + closed-form sync asgd iterates (tests 1, 8)."""
    cfg = _cfg()
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1, device=DEV)
    return X, y, _ref_sgd(cfg, X, y, 40)


@pytest.fixture(scope="module")
def saga_case():
    """Shared dataset + closed-form sync asaga states (tests 1, 2)."""
    cfg = _cfg(algo="asaga", gamma=0.05, num_workers=2)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=4, device=DEV)
    return X, y, _ref_saga(cfg, X, y, 40)


# -- 1. sync resume equals straight, against the closed form ----------------

def _check_sync_resume(make_engine, data, ref, path, **kw):
    engA, resA = _run_to_checkpoint(make_engine, data, path, 20, 20, **kw)
    assert resA["k"] == 20 and resA["checkpoints"] == 1
    state = load_checkpoint(path)
    assert state["k"] == 20
    rel_ck = _rel(state["w"], ref[19])
    print("checkpoint k=20 rel", rel_ck)
    assert rel_ck < BOUND, rel_ck
    engB, resB = _resume(make_engine, data, path, 40, **kw)
    assert resB["k"] == 40 and resB["applied"] == 20
    rel = _rel(engB.w, ref[39])
    print("resumed k=40 rel", rel)
    assert rel < BOUND, rel
    return state, engB


def test_sync_asgd_resume_matches_closed_form(asgd_case, tmp_path):
    X, y, ref = asgd_case
    _check_sync_resume(_dense_engine, (X, y), ref, str(tmp_path / "c.ckpt"))


def test_sync_asaga_resume_matches_closed_form(saga_case, tmp_path):
    X, y, ref = saga_case
    state, eng = _check_sync_resume(
        _dense_engine, (X, y), [r[0] for r in ref], str(tmp_path / "c.ckpt"),
        algo="asaga", gamma=0.05, num_workers=2)
    for name, got, want in (
            ("file alpha_bar", state["alpha_bar"], ref[19][1]),
            ("file alpha", _alpha(state), ref[19][2]),
            ("resumed alpha_bar", eng.alpha_bar, ref[39][1]),
            ("resumed alpha", _alpha(eng), ref[39][2])):
        rel = _rel(got, want)
        print(name, "rel", rel)
        assert rel < BOUND, (name, rel)


def test_sync_mllib_resume_matches_closed_form(tmp_path):
    kw = dict(algo="mllib", batch_rate=0.01)
    cfg = _cfg(**kw)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=7, device=DEV)
    ref = _ref_sgd(cfg, X, y, 40, mllib=True)
    _check_sync_resume(_dense_engine, (X, y), ref, str(tmp_path / "c.ckpt"),
                       **kw)


@pytest.mark.parametrize("d", [64, 66])
def test_sync_asaga_midrun_checkpoints_leave_the_run_unchanged(saga_case,
                                                               tmp_path, d):
    """Checkpoints at rounds 10, 20, 30 and 40 of one run commit the staged
    history early; the round after each must neither re-apply that staging
    nor lose it — the run still is the closed form, and so is the file.
    d=64 commits through the wave kernel, d=66 through the per-worker one."""
    X, y, ref = saga_case
    kw = dict(algo="asaga", gamma=0.05, num_workers=2, d=d)
    if d != 64:
        cfg = _cfg(**kw)
        X, y = synthetic_dense(cfg.N, cfg.d, seed=4, device=DEV)
        ref = _ref_saga(cfg, X, y, 40)
    path = str(tmp_path / "c.ckpt")
    eng, res = _run_to_checkpoint(_dense_engine, (X, y), path, 40, 10, **kw)
    assert res["k"] == 40 and res["checkpoints"] == 4
    state = load_checkpoint(path)
    assert state["k"] == 40
    for name, got, want in (
            ("w", eng.w, ref[39][0]),
            ("alpha_bar", eng.alpha_bar, ref[39][1]),
            ("alpha", _alpha(eng), ref[39][2]),
            ("file w", state["w"], ref[39][0]),
            ("file alpha", _alpha(state), ref[39][2])):
        rel = _rel(got, want)
        print("4 checkpoints in 40 rounds:", name, "rel", rel)
        assert rel < BOUND, (name, rel)


# -- 2. sync asaga history is complete at the end of a run -------------------

def test_sync_asaga_history_complete_at_end(saga_case):
    X, y, ref = saga_case
    cfg = _cfg(algo="asaga", gamma=0.05, num_workers=2)
    eng = _dense_engine(cfg, (X, y))
    assert eng.run(max_wall_s=120)["k"] == 40
    union = torch.zeros(cfg.N, dtype=torch.bool)
    for k in range(40):
        union |= _mask(cfg, k, "cpu").bool()
    alpha = _alpha(eng)
    # the last round's rows are in the pattern only if it was committed
    assert torch.equal(alpha != 0, union)
    rel = _rel(alpha, ref[39][2])
    print("alpha after 40 rounds rel", rel)
    assert rel < BOUND, rel


# -- 3. d % 4 != 0 and CSR ----------------------------------------------------

def test_sync_asgd_resume_d63(tmp_path):
    cfg = _cfg(d=63)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=8, device=DEV)
    _check_sync_resume(_dense_engine, (X, y), _ref_sgd(cfg, X, y, 40),
                       str(tmp_path / "c.ckpt"), d=63)


def test_sync_csr_asgd_resume(tmp_path):
    kw = dict(N=8_000, d=256, batch_rate=0.02)
    cfg = _cfg(**kw)
    data = synthetic_csr(cfg.N, cfg.d, seed=11, device=DEV)
    # the row-loop reference runs on the host (one sync per row otherwise)
    ip, ix, vv, yy = (t.cpu() for t in data)
    w = torch.zeros(cfg.d)
    ref = []
    for k in range(40):
        mask = _mask(cfg, k, "cpu")
        g, _ = torch_ref.grad_csr(ip, ix, vv, yy, w, mask, cfg.objective)
        w = w - (cfg.gamma / math.sqrt(k + 1)) * g / (cfg.batch_rate * cfg.N)
        ref.append(w.clone())
    _check_sync_resume(_csr_engine, data, ref, str(tmp_path / "c.ckpt"), **kw)


# -- 4. async P=1 is still the sequential algorithm across checkpoints -------

def test_async_p1_asgd_sequential_across_checkpoints(tmp_path):
    path = str(tmp_path / "c.ckpt")
    kw = dict(N=20_000, num_workers=1, sync=False)
    cfg = _cfg(**kw)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1, device=DEV)
    ref = _ref_sgd(cfg, X, y, 90)  # P=1: gamma/sqrt(k//P+1), divisor rate*N
    engA, resA = _run_to_checkpoint(_dense_engine, (X, y), path, 60, 20, **kw)
    assert resA["k"] == 60 and resA["checkpoints"] == 3
    rel = _rel(engA.w, ref[59])
    print("P=1 asgd, 3 checkpoints, k=60 rel", rel)
    assert rel < BOUND, rel
    state = load_checkpoint(path)
    assert state["k"] == 60
    assert _rel(state["w"], ref[59]) < BOUND
    engB, resB = _resume(_dense_engine, (X, y), path, 90, **kw)
    assert resB["k"] == 90 and resB["applied"] == 30
    rel = _rel(engB.w, ref[89])
    print("P=1 asgd resumed k=90 rel", rel)
    assert rel < BOUND, rel


@pytest.mark.parametrize("placement", ["device", "host"])
def test_async_p1_asaga_sequential_across_checkpoints(tmp_path, placement):
    path = str(tmp_path / "c.ckpt")
    kw = dict(N=20_000, num_workers=1, sync=False, algo="asaga", gamma=0.05,
              history_placement=placement)
    cfg = _cfg(**kw)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=3, device=DEV)
    ref = _ref_saga(cfg, X, y, 90)
    engA, resA = _run_to_checkpoint(_dense_engine, (X, y), path, 60, 20, **kw)
    assert resA["k"] == 60 and resA["checkpoints"] == 3
    state = load_checkpoint(path)
    assert state["k"] == 60
    engB, resB = _resume(_dense_engine, (X, y), path, 90, **kw)
    assert resB["k"] == 90
    if placement == "host":
        assert engB.alpha_tables[0].is_pinned()
    for name, got, want in (
            ("k=60 w", engA.w, ref[59][0]),
            ("k=60 alpha_bar", engA.alpha_bar, ref[59][1]),
            ("k=60 alpha", _alpha(engA), ref[59][2]),
            ("file w", state["w"], ref[59][0]),
            ("file alpha_bar", state["alpha_bar"], ref[59][1]),
            ("file alpha", _alpha(state), ref[59][2]),
            ("k=90 w", engB.w, ref[89][0]),
            ("k=90 alpha_bar", engB.alpha_bar, ref[89][1]),
            ("k=90 alpha", _alpha(engB), ref[89][2])):
        rel = _rel(got, want)
        print(placement, name, "rel", rel)
        assert rel < BOUND, (placement, name, rel)


# -- 5. async P>1 checkpoints are consistent SAGA states ---------------------

@pytest.mark.parametrize("tau_kw", [{}, dict(taw=0, bucket_ratio=0.3)],
                         ids=["accept-all", "taw0"])
def test_async_p4_asaga_checkpoint_is_consistent(tmp_path, tau_kw):
    path = str(tmp_path / "c.ckpt")
    kw = dict(sync=False, algo="asaga", gamma=0.05, **tau_kw)
    cfg = _cfg(**kw)
    P = cfg.num_workers
    X, y = synthetic_dense(cfg.N, cfg.d, seed=4, device=DEV)
    engA, resA = _run_to_checkpoint(_dense_engine, (X, y), path, 100, 40,
                                    **kw)
    print("rejected", resA["rejected"], "checkpoints", resA["checkpoints"],
          "checkpoint_ms", resA["checkpoint_ms"])
    assert resA["k"] >= 100 and resA["checkpoints"] >= 2
    state = load_checkpoint(path)
    assert 80 <= state["k"] < 80 + P, state["k"]
    rel_file = _identity_dense(X, state["alpha_bar"], _alpha(state))
    rel_end = _identity_dense(X, engA.alpha_bar, _alpha(engA))
    print("identity: file k=%d" % state["k"], rel_file, "end of run", rel_end)
    assert rel_file < BOUND, rel_file
    assert rel_end < BOUND, rel_end
    # resume this checkpoint to 200 updates
    engB, resB = _resume(_dense_engine, (X, y), path, 200, **kw)
    print("resumed: rejected", resB["rejected"])
    assert resB["k"] >= 200
    rel_res = _identity_dense(X, engB.alpha_bar, _alpha(engB))
    obj_ck, obj_res = _objective(X, y, state["w"]), _objective(X, y, engB.w)
    print("identity after resume", rel_res, "objective", obj_ck, "->", obj_res)
    assert rel_res < BOUND, rel_res
    assert obj_res < obj_ck


def test_async_csr_asaga_checkpoint_is_consistent(tmp_path):
    path = str(tmp_path / "c.ckpt")
    kw = dict(sync=False, algo="asaga", gamma=0.05, num_workers=2, N=80_000,
              d=256, batch_rate=0.02, delay_coeff=-1.0, calib_factor=3)
    cfg = _cfg(**kw)
    data = synthetic_csr(cfg.N, cfg.d, seed=17, device=DEV)
    engA, resA = _run_to_checkpoint(_csr_engine, data, path, 100, 40, **kw)
    assert resA["k"] >= 100 and resA["checkpoints"] >= 2
    state = load_checkpoint(path)
    assert 80 <= state["k"] < 80 + cfg.num_workers, state["k"]
    rel_file = _identity_csr(data, cfg.d, state["alpha_bar"], _alpha(state))
    rel_end = _identity_csr(data, cfg.d, engA.alpha_bar, _alpha(engA))
    print("csr identity: file k=%d" % state["k"], rel_file, "end", rel_end)
    assert rel_file < BOUND, rel_file
    assert rel_end < BOUND, rel_end


def test_async_end_state_commits_idle_workers():
    """bucket_ratio=1 makes the gate P: a finished worker idles, its
    accepted round uncommitted, until all four have finished. 98 = 24*4 + 2
    updates end the run inside a wave — two workers idle with uncommitted
    history, two rounds in flight and dropped — whatever the timing. The
    quiescent end must still leave a consistent SAGA state, and a second
    run on the same buffers must start from clean gradient sums."""
    cfg = _cfg(sync=False, algo="asaga", gamma=0.05, bucket_ratio=1.0,
               num_iterations=98)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=4, device=DEV)
    eng = _dense_engine(cfg, (X, y))
    res = eng.run(max_wall_s=120)
    assert res["k"] == 98
    rel = _identity_dense(X, eng.alpha_bar, _alpha(eng))
    print("identity with idle uncommitted workers at exit", rel)
    assert rel < BOUND, rel
    # continue on the same engine: dropped rounds must not leak into g
    eng.restore_state(eng.capture_state(res["k"], res["clock"], res))
    res2 = eng.run(num_iterations=150, max_wall_s=120)
    assert res2["k"] == 150 and res2["k0"] == 98
    rel2 = _identity_dense(X, eng.alpha_bar, _alpha(eng))
    print("identity after continuing to 150", rel2)
    assert rel2 < BOUND, rel2


# -- 6. delay state survives --------------------------------------------------

def test_async_delay_state_survives_resume(tmp_path):
    path = str(tmp_path / "c.ckpt")
    kw = dict(sync=False, num_workers=8, N=80_000, delay_coeff=-1.0,
              calib_factor=3)
    cfg = _cfg(**kw)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=5, device=DEV)
    # calibration ends at k = calib_factor * P = 24
    _, resA = _run_to_checkpoint(_dense_engine, (X, y), path, 150, 100, **kw)
    assert resA["k"] >= 150 and resA["checkpoints"] == 1
    state = load_checkpoint(path)
    nd = state["native_delay"]
    print("stored delay state", nd)
    assert nd["delay_flag"] is True and nd["avg_delay_ms"] > 0
    assert nd["avg_delay_ms"] == resA["avg_delay_ms"]
    _, resB = _resume(_dense_engine, (X, y), path, 200, **kw)
    assert resB["k"] >= 200
    assert resB["avg_delay_ms"] == nd["avg_delay_ms"] > 0
    assert resB["delay_flag"] is True
    assert resB["cul_count"] == nd["cul_count"]


# -- 7. checkpoint off is inert ----------------------------------------------

@pytest.mark.parametrize("sync", [False, True])
def test_checkpoint_off_is_inert(asgd_case, sync):
    X, y, _ = asgd_case
    eng = _dense_engine(_cfg(sync=sync), (X, y))
    res = eng.run(max_wall_s=120)
    assert res["k"] >= 40
    assert res["checkpoints"] == 0
    assert res["checkpoint_ms"] == 0
    assert res["k0"] == 0


def test_callback_error_propagates_and_engine_stays_usable(asgd_case,
                                                           tmp_path):
    """A checkpoint that cannot be written raises out of run() (the loop is
    quiescent there); the engine's buffers stay valid for another run."""
    X, y, _ = asgd_case
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    cfg = _cfg(sync=False, checkpoint_every=20,
               checkpoint_path=str(blocker / "sub" / "c.ckpt"))
    eng = _dense_engine(cfg, (X, y))
    with pytest.raises(OSError):
        eng.run(max_wall_s=120)
    eng.cfg.checkpoint_path = ""
    eng.w.zero_()
    res = eng.run(max_wall_s=120)
    assert res["k"] >= 40 and res["checkpoints"] == 0
    assert _objective(X, y, eng.w) < _objective(X, y, torch.zeros(cfg.d))


# -- 8. schema interchange (sync asgd) ----------------------------------------

def test_native_checkpoint_resumes_on_threads_engine(asgd_case, tmp_path):
    X, y, ref = asgd_case
    path = str(tmp_path / "n.ckpt")
    _run_to_checkpoint(_dense_engine, (X, y), path, 20, 20)
    assert load_checkpoint(path)["k"] == 20
    cfg = _cfg(num_iterations=40)
    res, _ = runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                               max_wall_s=120, verbose=False,
                               engine="threads", resume_from=path)
    assert res.k == 40
    rel = _rel(res.w, ref[39])
    print("native -> threads rel", rel)
    assert rel < BOUND, rel


def test_threads_checkpoint_resumes_on_native_engine(asgd_case, tmp_path):
    X, y, ref = asgd_case
    path = str(tmp_path / "t.ckpt")
    cfg = _cfg(num_iterations=20, checkpoint_path=path, checkpoint_every=20)
    runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                      max_wall_s=120, verbose=False, engine="threads")
    assert load_checkpoint(path)["k"] == 20
    cfg = _cfg(num_iterations=40)
    res, neng = runner.run_engine(cfg, runner.build_dense_workers(cfg, X, y),
                                  max_wall_s=120, verbose=False,
                                  engine="native", resume_from=path)
    assert res.k == 40 and res.applied == 20
    rel = _rel(neng.w, ref[39])
    print("threads -> native rel", rel)
    assert rel < BOUND, rel


# -- 9. CLI ---------------------------------------------------------------------

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
    return lines


def test_cli_asaga_thread_native_checkpoint_and_resume(capsys, tmp_path):
    from asyncframework_amd.cli import drivers
    path = str(tmp_path / "cli.ckpt")
    P = 4
    # 190 updates, checkpoints as k crosses 50, 100, 150 (the file is
    # overwritten each time); the resumed run covers 150.. to 190
    argv = ["synthetic", "synthetic", "64", "20000", str(P), "190", "0.05",
            "1000000", "0.05", "0.5", "10", "0", "42", "--device", DEV,
            "--engine", "native"]
    drivers.asaga_thread(argv + ["--checkpoint-path", path,
                                 "--checkpoint-every", "50"])
    _check_stdout_contract(capsys.readouterr().out)
    assert os.path.exists(path)
    k_file = load_checkpoint(path)["k"]
    assert 150 <= k_file < 150 + P, k_file
    drivers.asaga_thread(argv + ["--resume-from", path])
    lines = _check_stdout_contract(capsys.readouterr().out)
    its = [int(l.split()[1]) for l in lines if l.startswith("Iteration ")]
    print("resumed from k =", k_file, "iteration lines", its)
    assert its and min(its) >= k_file  # only this process's iterations
