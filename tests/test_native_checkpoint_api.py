"""Checkpoint/resume of the native engine, the parts that need no GPU: the
run_engine(engine="native") argument contract, and check_compatible — the
one compatibility check restore(), the native dist server and the native
local engine share."""

import warnings

import pytest
import torch

from asyncframework_amd import run as runner
from asyncframework_amd.data.synthetic import synthetic_dense
from asyncframework_amd.engine import checkpoint as ckpt
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.server import Server


def _cfg(**kw):
    base = dict(d=16, N=256, num_workers=2, num_iterations=40, gamma=0.3,
                taw=1 << 30, batch_rate=0.3, bucket_ratio=0.5,
                printer_freq=1000, delay_coeff=0.0, seed=42, device="cpu",
                snapshot_weights=False)
    base.update(kw)
    return EngineConfig(**base)


def _state(cfg, with_alpha=True):
    """A capture_state dict of a server with non-trivial contents."""
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1)
    workers = runner.build_dense_workers(cfg, X, y)
    server = Server(cfg, device=torch.device("cpu"))
    server.k = 17
    server.AC.setCurrentTime(23)
    server.w.normal_()
    if server.alpha_bar is not None:
        server.alpha_bar.normal_()
    for wk in workers:
        if wk.alpha is not None:
            wk.alpha.normal_()
    return (ckpt.capture_state(server, workers if with_alpha else None),
            server, workers, (X, y))


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("resume", [False, True])
def test_native_checkpoint_settings_reach_the_gpu_only_check(tmp_path, sync,
                                                             resume):
    """Checkpoint settings (and resume_from) are accepted by the native
    engine: on CPU workers the only complaint left is the GPU-only one."""
    p = str(tmp_path / "n.ckpt")
    cfg = _cfg(sync=sync, checkpoint_path=p, checkpoint_every=10)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1)
    workers = runner.build_dense_workers(cfg, X, y)
    resume_from = ""
    if resume:
        resume_from = str(tmp_path / "from.ckpt")
        ckpt.save_checkpoint(resume_from,
                             Server(cfg, device=torch.device("cpu")), workers)
    with pytest.raises(AssertionError, match="GPU-only"):
        runner.run_engine(cfg, workers, verbose=False, engine="native",
                          resume_from=resume_from)


def test_check_compatible_rejects_other_pool_and_dimension():
    state, _, _, _ = _state(_cfg(num_workers=4, algo="asaga"))
    with pytest.raises(ValueError, match="num_workers"):
        ckpt.check_compatible(state, _cfg(num_workers=2, algo="asaga"))
    with pytest.raises(ValueError, match="dimensionality"):
        ckpt.check_compatible(state, _cfg(num_workers=4, d=32, algo="asaga"))
    # the matching config passes quietly and reports nothing missing
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert ckpt.check_compatible(
            state, _cfg(num_workers=4, algo="asaga"),
            alpha_ids=range(4)) == []


def test_check_compatible_warns_on_penalty_mismatch():
    state, _, _, _ = _state(_cfg(l2=0.0))
    with pytest.warns(RuntimeWarning, match="l2=0.0, resuming with l2=0.5"):
        ckpt.check_compatible(state, _cfg(l2=0.5))
    # a checkpoint from before the penalties existed counts as 0.0
    del state["cfg"]["l2"], state["cfg"]["l1"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.check_compatible(state, _cfg())
    with pytest.warns(RuntimeWarning, match="l1=0.0, resuming with l1=0.25"):
        ckpt.check_compatible(state, _cfg(l1=0.25))


def test_check_compatible_warns_on_missing_table():
    cfg = _cfg(algo="asaga")
    state, _, _, _ = _state(cfg)
    del state["alpha"][1]
    with pytest.warns(RuntimeWarning, match=r"no SAGA history table.*\[1\]"):
        missing = ckpt.check_compatible(state, cfg, alpha_ids=range(2))
    assert missing == [1]


def test_restore_is_unchanged_by_the_refactor():
    """The states of tests/test_checkpoint.py: exact round trip, the two
    ValueErrors, and a missing table that warns and leaves alpha alone."""
    cfg = _cfg(algo="asaga")
    state, server, workers, (X, y) = _state(cfg)
    server2 = Server(cfg, device=torch.device("cpu"))
    workers2 = runner.build_dense_workers(cfg, X, y)
    ckpt.restore(server2, workers2, state)
    assert server2.k == 17
    assert server2.AC.getCurrentTime() == 23
    assert torch.equal(server2.w, server.w)
    assert torch.equal(server2.alpha_bar, server.alpha_bar)
    for a, b in zip(workers2, workers):
        assert torch.equal(a.alpha, b.alpha)

    with pytest.raises(ValueError, match="num_workers"):
        ckpt.restore(Server(_cfg(algo="asaga", num_workers=4),
                            device=torch.device("cpu")), [], state)
    with pytest.raises(ValueError):
        ckpt.restore(Server(_cfg(algo="asaga", d=8),
                            device=torch.device("cpu")), [], state)

    del state["alpha"][0]
    server3 = Server(cfg, device=torch.device("cpu"))
    workers3 = runner.build_dense_workers(cfg, X, y)
    with pytest.warns(RuntimeWarning, match="no SAGA history table"):
        ckpt.restore(server3, workers3, state)
    assert float(workers3[0].alpha.abs().sum()) == 0.0
    assert torch.equal(workers3[1].alpha, workers[1].alpha)
    assert torch.equal(server3.w, server.w)
