"""Elastic-net (l2 / l1) regularisation on MI355X: the REG forms of
multi_update_kernel, sgd_update_kernel and saga_update_kernel against an
fp64 sequential loop, bit identity of the zero-penalty dispatch, the native
engine's synchronous rounds and its one-worker async loop against
whole-dataset torch loops, and the exact-zero property through the real
eight-worker event loop.

Contract (one applied step, step eta, normalised data direction ghat):
    v = w - eta*(ghat + l2*w)
    w = v > t ? v - t : (v < -t ? v + t : +0),  t = eta*l1

Datasets are generated on the host (same seeds and shapes as
tests/test_gpu_native_sync.py / test_gpu_native.py) and copied to the
device, so the zero / non-zero counts noted below are those of the data
the tests run on."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops
from asyncframework_amd.data.shard import row_shards
from asyncframework_amd.data.synthetic import synthetic_csr, synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.native import NativeLocalEngine
from asyncframework_amd.engine.worker import Shard
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.utils.philox import bernoulli_mask

DEV = "cuda:0"
BOUND = 1e-4   # tests/test_gpu_native_sync.py's own relative bound
L2, L1 = 0.1, 0.01


def _core():
    from asyncframework_amd import _hip_core
    return _hip_core


def _f32(v):
    return float(np.float32(v))


def _soft64(v, t):
    return np.where(v > t, v - t, np.where(v < -t, v + t, 0.0))


# ------------------------------------------------------------- kernel level

_MU_P = 32
_GAMMA = 2.0 ** -7
_INV_BATCH = 0.5
_INV_N = 2.0 ** -10
_KL2 = 2.0 ** -3
_T_TOTAL = 1.5  # summed threshold of a batch: the middle of |w0| in [.5,2.5)


def _mu_inputs(d, seed, device="cuda"):
    """The table layout of test_multi_update_matches_fp64_sequential:
    16-byte-aligned per-worker rows, |w0| and |alpha_bar0| in [0.5, 2.5),
    padding columns and untouched rows recognisable. Drawn from a host
    generator, so a seed gives the same values wherever it is checked."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    sgn = lambda t: torch.where(t >= 0, 1.0, -1.0)
    w0 = r(d)
    w0 = sgn(w0) * (0.5 + 2 * torch.rand(d, generator=gen))
    ab0 = r(d)
    ab0 = sgn(ab0) * (0.5 + 2 * torch.rand(d, generator=gen))
    dpad = (d + 3) // 4 * 4
    G = torch.zeros(_MU_P, dpad)
    G[:, :d] = r(_MU_P, d)
    WB = torch.full((_MU_P, dpad), 7.0)
    return tuple(t.to(device) for t in (w0, ab0, G, WB))


def _ref_steps(w64, ab64, gs, algo, scale, eta, l2, l1, gam, ib, iN):
    """fp64 sequential loop over the gradients ``gs`` with the fp32-rounded
    scalars. Returns (w, ab, wmax, abmax, safely_clipped): wmax is the
    largest magnitude the running value or v takes (w0 included);
    safely_clipped marks elements the LAST step clips with |v| further
    below t than any admissible rounding error."""
    wmax, abmax = np.abs(w64), np.abs(ab64)
    v = w64
    t = 0.0
    for j, gi in enumerate(gs):
        if algo == 0:
            e = eta[j]
            v = w64 - scale[j] * gi - e * l2 * w64
        else:
            e = gam
            v = w64 - gam * (ib * gi + ab64 + l2 * w64)
            ab64 = ab64 + iN * gi
        t = e * l1
        w64 = _soft64(v, t)
        wmax = np.maximum(wmax, np.maximum(np.abs(v), np.abs(w64)))
        abmax = np.maximum(abmax, np.abs(ab64))
    return w64, ab64, wmax, abmax, (v, t)


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("d", [5, 784])
@pytest.mark.parametrize("m", [0, 3])
@pytest.mark.parametrize("n", [1, 9, 32])
def test_multi_update_reg_matches_fp64_sequential(n, m, d, algo):
    """multi_update_kernel<VEC4, REG=true> vs the fp64 sequential loop in
    the same j order, l2 = 2^-3 and an l1 that makes the batch's summed
    threshold 1.5, the middle of |w0|'s range [0.5, 2.5) (for n = 1 that is
    eta*l1 itself), so the reference ends with clipped and unclipped
    elements — asserted.

    Bound per element: R * n * 2^-24 * (largest magnitude the running value
    or v takes). R counts the fp32 roundings of one step as written in
    csrc/kernels.hip (reg_dec / reg_thr / reg_step / reg_prox, every
    operation an explicit single-rounding intrinsic):
      dec  = fma(-eta, l2, 1)      1  (relative to dec*w <= |w|)
      dec*w                        1
      v    = fma(-step, g, dec*w)  1
      t    = eta*l1                1  (matters only where |v| >= t or
                                       within rounding of it: <= 2^-24 |v|)
      |v| - t (sign put back)      1
    R = 5 for asgd. asaga forms ghat = fma(inv_batch, g, alpha_bar) first:
    one more, R = 6. The soft-threshold is 1-Lipschitz, so a step does not
    amplify the error it inherits. alpha_bar is one fma per step: n * 2^-24
    * its running magnitude, as in the unregularised test."""
    core = _core()
    w, ab, G, WB = _mu_inputs(d, seed=2100 + 10 * n + m + d + algo)
    perm = np.random.RandomState(n * 7 + m).permutation(_MU_P)
    gw = [int(v) for v in perm[:n]]
    sw = [int(v) for v in perm[::-1][:m]]
    scale = [_f32(0.01 / np.sqrt(j + 1.0)) for j in range(n)]
    eta = [_f32(2.0 ** -4 / np.sqrt(j + 1.0)) for j in range(n)]
    gam, ib, iN, l2 = (_f32(v) for v in (_GAMMA, _INV_BATCH, _INV_N, _KL2))
    l1 = _f32(_T_TOTAL / (sum(eta) if algo == 0 else n * gam))
    G0, WB0 = G.clone(), WB.clone()

    g64 = G0[:, :d].double().cpu().numpy()
    w64, ab64, wmax, abmax, (v_last, t_last) = _ref_steps(
        w.double().cpu().numpy(), ab.double().cpu().numpy(),
        [g64[p] for p in gw], algo, scale, eta, l2, l1, gam, ib, iN)
    assert (w64 == 0).any() and (w64 != 0).any(), "reference not mixed"

    vec4 = core.multi_update(
        w.data_ptr(), [G[p].data_ptr() for p in range(_MU_P)],
        [WB[p].data_ptr() for p in range(_MU_P)],
        ab.data_ptr() if algo == 1 else 0, _GAMMA, _INV_BATCH, _INV_N, d,
        algo, gw, sw, scale if algo == 0 else [],
        torch.cuda.current_stream().cuda_stream,
        eta=eta if algo == 0 else [], l2=l2, l1=l1)
    torch.cuda.synchronize()
    assert vec4 == (d % 4 == 0)  # d=784 runs the float4 form, d=5 the scalar

    R = 5 if algo == 0 else 6
    w_gpu = w.double().cpu().numpy()
    w_err = np.abs(w_gpu - w64)
    w_bound = R * n * 2.0 ** -24 * wmax
    print(f"n={n} m={m} d={d} algo={algo} R={R} clipped={(w64 == 0).sum()} "
          f"max w err/bound={float((w_err / w_bound).max()):.3f}")
    assert (w_err <= w_bound).all()
    safe = np.abs(v_last) < t_last - w_bound
    assert safe.any()
    assert (w_gpu[safe] == 0).all(), "clipped element not exactly 0.0"
    assert not bool(torch.signbit(w).cpu().numpy()[safe].any()), "-0.0"
    if algo == 1:
        ab_err = np.abs(ab.double().cpu().numpy() - ab64)
        ab_bound = n * 2.0 ** -24 * abmax
        print(f"  max ab err/bound={float((ab_err / ab_bound).max()):.3f}")
        assert (ab_err <= ab_bound).all()
    used = torch.zeros(_MU_P, dtype=torch.bool)
    used[gw] = True
    assert bool((G[used][:, :d] == 0).all()), "consumed g not zeroed"
    assert torch.equal(G[~used], G0[~used]), "unconsumed g modified"
    snap = torch.zeros(_MU_P, dtype=torch.bool)
    snap[sw] = True
    for p in sw:
        assert torch.equal(WB[p, :d], w), f"snapshot {p} != w bit for bit"
    assert torch.equal(WB[~snap], WB0[~snap]), "non-target snapshot modified"
    assert torch.equal(G[:, d:], G0[:, d:]) and torch.equal(WB[:, d:],
                                                            WB0[:, d:])


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("d", [5, 784])
def test_ops_update_reg_matches_fp64(d, algo):
    """ops.sgd_update / ops.saga_update (sgd_update_kernel<true>,
    saga_update_kernel<true>): one step, same reference and bound with
    n = 1. sgd_update forms step = gamma_k*inv_batch in the kernel (one
    rounding more than multi_update, which gets it from the host): R = 6;
    saga_update as above: R = 6."""
    w, ab, G, _ = _mu_inputs(d, seed=3000 + d + algo)
    g = G[0, :d].contiguous()
    g0 = g.clone()
    gam, ib, iN, l2 = (_f32(v) for v in (_GAMMA, _INV_BATCH, _INV_N, _KL2))
    eta = _f32(2.0 ** -4)
    l1 = _f32(_T_TOTAL / (eta if algo == 0 else gam))
    w64, ab64, wmax, abmax, (v_last, t_last) = _ref_steps(
        w.double().cpu().numpy(), ab.double().cpu().numpy(),
        [g.double().cpu().numpy()], algo, [eta * ib], [eta], l2, l1, gam, ib,
        iN)
    assert (w64 == 0).any() and (w64 != 0).any(), "reference not mixed"
    if algo == 0:
        ops.sgd_update(w, g, eta, ib, l2=l2, l1=l1)
    else:
        ops.saga_update(w, g, ab, gam, ib, iN, l2=l2, l1=l1)
    torch.cuda.synchronize()
    w_gpu = w.double().cpu().numpy()
    w_err = np.abs(w_gpu - w64)
    w_bound = 6 * 2.0 ** -24 * wmax
    print(f"d={d} algo={algo} clipped={(w64 == 0).sum()} "
          f"max w err/bound={float((w_err / w_bound).max()):.3f}")
    assert (w_err <= w_bound).all()
    safe = np.abs(v_last) < t_last - w_bound
    assert safe.any() and (w_gpu[safe] == 0).all()
    if algo == 1:
        ab_err = np.abs(ab.double().cpu().numpy() - ab64)
        assert (ab_err <= 2.0 ** -24 * abmax).all()
    assert torch.equal(g, g0)  # these two kernels do not consume g


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("d", [5, 784])
def test_zero_penalty_dispatch_is_bit_identical(d, algo):
    """Explicit l1 = l2 = 0 (eta given) runs the REG=false instantiation:
    torch.equal to the legacy 13-argument call on w, alpha_bar, snapshots
    and the gradient tables; same for the two ops kernels."""
    core = _core()
    n, m = 9, 3
    perm = np.random.RandomState(5).permutation(_MU_P)
    gw, sw = [int(v) for v in perm[:n]], [int(v) for v in perm[::-1][:m]]
    scale = [_f32(0.01 / np.sqrt(j + 1.0)) for j in range(n)]
    eta = [_f32(2.0 ** -4 / np.sqrt(j + 1.0)) for j in range(n)]
    outs = []
    for explicit in (False, True):
        w, ab, G, WB = _mu_inputs(d, seed=4000 + d + algo)
        args = (w.data_ptr(), [G[p].data_ptr() for p in range(_MU_P)],
                [WB[p].data_ptr() for p in range(_MU_P)],
                ab.data_ptr() if algo == 1 else 0, _GAMMA, _INV_BATCH, _INV_N,
                d, algo, gw, sw, scale if algo == 0 else [],
                torch.cuda.current_stream().cuda_stream)
        if explicit:
            core.multi_update(*args, eta=eta if algo == 0 else [], l2=0.0,
                              l1=0.0)
        else:
            core.multi_update(*args)
        torch.cuda.synchronize()
        outs.append((w, ab, G, WB))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    w, ab, G, _ = _mu_inputs(d, seed=4100 + d + algo)
    g = G[0, :d].contiguous()
    wa, wb, aba, abb = w.clone(), w.clone(), ab.clone(), ab.clone()
    if algo == 0:
        ops.sgd_update(wa, g, 0.3, 0.5)
        ops.sgd_update(wb, g, 0.3, 0.5, l2=0.0, l1=0.0)
    else:
        ops.saga_update(wa, g, aba, 0.3, 0.5, _INV_N)
        ops.saga_update(wb, g, abb, 0.3, 0.5, _INV_N, l2=0.0, l1=0.0)
    assert torch.equal(wa, wb) and torch.equal(aba, abb)
    assert not torch.equal(wa, w)  # the update did run


def test_reg_instantiations_add_no_scratch_and_no_lds():
    info = _core().update_kernel_info()
    assert len(info) == 8
    for kern in ("multi_update_kernel", "sync_round_update_kernel"):
        for vec4 in ("true", "false"):
            reg = info[f"{kern}<{vec4},true>"]
            plain = info[f"{kern}<{vec4},false>"]
            print(kern, vec4, "REG", dict(reg), "plain", dict(plain))
            assert reg["local_size_bytes"] == 0
            assert reg["shared_size_bytes"] == plain["shared_size_bytes"]


# ------------------------------------------------- native sync, closed form

def _cfg(**kw):
    base = dict(d=64, N=40_000, num_workers=4, num_iterations=40, gamma=0.3,
                taw=1 << 30, batch_rate=0.05, bucket_ratio=0.5,
                printer_freq=1 << 30, delay_coeff=0.0, seed=42,
                device=DEV, snapshot_weights=False, sync=True, l2=L2, l1=L1)
    base.update(kw)
    return EngineConfig(**base)


def _shards(cfg, X, y):
    return [Shard(row_start=s, n_rows=t - s, X=X[s:t], y=y[s:t])
            for s, t in row_shards(cfg.N, cfg.num_workers)]


def _engine(cfg, X, y):
    return NativeLocalEngine(cfg, _shards(cfg, X, y), torch.device(DEV))


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def _mask(cfg, k, device):
    return torch.from_numpy(
        bernoulli_mask(cfg.seed, k + 1, 0, cfg.N, cfg.batch_rate)).to(device)


def _soft(v, t):
    return torch.where(v > t, v - t,
                       torch.where(v < -t, v + t, torch.zeros_like(v)))


def _ref_loop(cfg, X, y, rounds, mode, inv_batch, grad=None):
    """Whole-dataset torch loop with the contract written out. mode 'asgd'
    (ghat = inv_batch*g), 'mllib' (ghat = g/max(n,1)) or 'asaga'. asgd's
    step is gamma/sqrt(k // num_workers_async + 1): callers pass sync
    configs (k+1) or one async worker (k // 1 + 1), the same number.
    Returns (iterates, alpha_bar)."""
    dev = y.device
    w = torch.zeros(cfg.d, device=dev)
    ab = torch.zeros(cfg.d, device=dev)
    alpha = torch.zeros(cfg.N, device=dev)
    out = []
    for k in range(rounds):
        mask = _mask(cfg, k, dev)
        if mode == "asaga":
            g, idx, e, _ = torch_ref.saga_grad_dense(X, y, w, alpha, mask,
                                                     cfg.objective)
            eta = cfg.gamma
            ghat = inv_batch * g + ab  # OLD alpha_bar
            ab = ab + g / cfg.N        # the penalty stays out of alpha_bar
            alpha[idx] = e
        else:
            g, n = (grad(w, mask) if grad is not None else
                    torch_ref.grad_dense(X.float(), y, w, mask,
                                         cfg.objective))
            eta = cfg.gamma / math.sqrt(k + 1)
            ghat = g / max(n, 1) if mode == "mllib" else inv_batch * g
        w = _soft(w - eta * (ghat + cfg.l2 * w), eta * cfg.l1)
        out.append(w.clone())
    return out, ab


@pytest.fixture(scope="module")
def sync_data():
    X, y = synthetic_dense(40_000, 64, seed=1, device="cpu")
    return X.to(DEV), y.to(DEV)


@pytest.mark.parametrize("algo,gamma", [("asgd", 0.3), ("mllib", 0.3),
                                        ("asaga", 0.05)])
def test_native_sync_reg_matches_closed_form(sync_data, algo, gamma):
    """The case of tests/test_gpu_native_sync.py (d=64, N=40,000, P=4, 40
    rounds, gamma 0.3, rate 0.05, seed 42, data seed 1) with l1 = 0.01,
    l2 = 0.1, all three modes, plus the snapshot ring mid-run. On this data
    the fp32 host loop ends with 37 of 64 non-zero coordinates for asgd and
    mllib (fp32 vs fp64: 1.6e-7) and, at that file's own asaga step
    gamma = 0.05, 35 of 64; the unregularised iterate is > 0.9 relative
    away in every mode, so a dropped penalty misses BOUND by four orders."""
    X, y = sync_data
    cfg = _cfg(algo=algo, gamma=gamma)
    ref, ab_ref = _ref_loop(cfg, X, y, 40, algo,
                            1.0 / (cfg.batch_rate * cfg.N))
    nz = int((ref[-1] != 0).sum())
    print(algo, "reference non-zero", nz, "of", cfg.d)
    assert 0 < nz < cfg.d
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120, snapshot_every=10)
    assert res["k"] == 40 and res["rejected"] == 0
    rel = _rel(eng.w, ref[-1])
    print(algo, "rel", rel)
    assert rel < BOUND, rel
    assert int((eng.w == 0).sum()) > 0  # exact zeros, not small numbers
    if algo == "asaga":
        rel_ab = _rel(eng.alpha_bar, ab_ref)
        print("alpha_bar rel", rel_ab)
        assert rel_ab < BOUND, rel_ab
    # snapshots (fused snap_dst store) are the post-threshold iterates
    ov = res["opt_vars"]
    assert len(ov) == 1 + 4
    for j in range(1, 5):
        snap = ov[j][1].to(DEV)
        rs = _rel(snap, ref[10 * (j - 1)])
        print("snapshot", j, "rel", rs)
        assert rs < BOUND, (j, rs)
    assert int((ov[4][1] == 0).sum()) > 0


def test_native_sync_reg_csr():
    """CSR shards (that file's CSR case: N=8,000, d=256, rate 0.02, 20
    rounds): the host loop ends with 36 of 256 non-zero coordinates."""
    cfg = _cfg(N=8_000, d=256, batch_rate=0.02, num_iterations=20)
    indptr, indices, values, y = synthetic_csr(cfg.N, cfg.d, seed=11,
                                               device=DEV)
    shards = []
    for s, t in row_shards(cfg.N, cfg.num_workers):
        base = int(indptr[s])
        shards.append(Shard(row_start=s, n_rows=t - s,
                            indptr=(indptr[s:t + 1] - base).contiguous(),
                            indices=indices[base:int(indptr[t])],
                            values=values[base:int(indptr[t])], y=y[s:t]))
    eng = NativeLocalEngine(cfg, shards, torch.device(DEV))
    assert eng.run(max_wall_s=120)["k"] == 20
    ip, ix, vv, yy = (t.cpu() for t in (indptr, indices, values, y))
    ref, _ = _ref_loop(
        cfg, None, yy, 20, "asgd", 1.0 / (cfg.batch_rate * cfg.N),
        grad=lambda w, m: torch_ref.grad_csr(ip, ix, vv, yy, w, m,
                                             cfg.objective))
    nz = int((ref[-1] != 0).sum())
    assert 0 < nz < cfg.d
    rel = _rel(eng.w.cpu(), ref[-1])
    print("csr rel", rel, "non-zero", nz)
    assert rel < BOUND, rel


def test_native_sync_reg_scalar_form_d66():
    """d = 66 is no multiple of 4: sync_round_update_kernel<false, true>.
    Host loop: 39 of 66 non-zero."""
    cfg = _cfg(d=66, num_workers=2, num_iterations=20)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=8, device="cpu")
    X, y = X.to(DEV), y.to(DEV)
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120)
    assert res["k"] == 20 and res["rejected"] == 0
    ref, _ = _ref_loop(cfg, X, y, 20, "asgd", 1.0 / (cfg.batch_rate * cfg.N))
    nz = int((ref[-1] != 0).sum())
    assert 0 < nz < cfg.d
    rel = _rel(eng.w, ref[-1])
    print("d=66 rel", rel, "non-zero", nz)
    assert rel < BOUND, rel


# ------------------------------------------------------ native async, P = 1

@pytest.mark.parametrize("algo,gamma", [("asgd", 0.3), ("asaga", 0.05)])
def test_native_async_p1_reg_matches_sequential_ref(algo, gamma):
    """One worker is deterministic (test_native_p1_matches_sequential_ref:
    N=20,000, 60 updates, rel < 1e-4). Host loop: 42 (asgd) / 33 (asaga) of
    64 non-zero, > 1.0 relative away from the unregularised iterate."""
    cfg = _cfg(N=20_000, num_workers=1, num_iterations=60, sync=False,
               algo=algo, gamma=gamma)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=1, device="cpu")
    X, y = X.to(DEV), y.to(DEV)
    eng = _engine(cfg, X, y)
    res = eng.run(max_wall_s=120)
    assert res["k"] == cfg.num_iterations
    ref, ab_ref = _ref_loop(cfg, X, y, cfg.num_iterations, algo,
                            1.0 / cfg.par_recs)
    nz = int((ref[-1] != 0).sum())
    assert 0 < nz < cfg.d
    rel = _rel(eng.w, ref[-1])
    print(algo, "p1 rel", rel, "non-zero", nz)
    assert rel < 1e-4, rel
    assert int((eng.w == 0).sum()) > 0
    if algo == "asaga":
        assert _rel(eng.alpha_bar, ab_ref) < 1e-4


# ------------------------------------- native async, P = 8, exact-zero

@pytest.mark.parametrize("algo", ["asgd", "asaga"])
def test_native_async_p8_stays_exactly_zero(algo):
    """l1 is chosen first, on the host, as twice the largest |ghat|_inf any
    worker's round can produce at w = 0, over every worker and every round
    key the run can use (Philox masks). w then never leaves 0, so those
    gradients are the ones the run sees whatever the asynchronous schedule:
    batches of varying size go through the real event loop, every step is
    clipped, and w must end exactly +0.0.
    asgd: ghat = inv_batch * sum_S (-y_i x_i), taken exactly. asaga: a
    round's g sums (e_i - alpha_i) x_i with e_i = -y_i and alpha_i either 0
    or -y_i depending on which rounds were committed before it, and
    alpha_bar is -(1/N) sum over the committed rows of y_i x_i; both are
    bounded, for any history, by the sums of |y_i x_i|, which is what is
    taken."""
    P, iters = 8, 150
    cfg = _cfg(num_workers=P, num_iterations=iters, sync=False, algo=algo,
               gamma=0.05 if algo == "asaga" else 0.3, l2=L2, l1=0.0)
    X, y = synthetic_dense(cfg.N, cfg.d, seed=2, device="cpu")
    inv_batch = P / (cfg.batch_rate * cfg.N)
    yx = (X * y[:, None]).double()
    worst = 0.0
    for s, t in row_shards(cfg.N, P):
        blk = yx[s:t].abs() if algo == "asaga" else yx[s:t]
        for key in range(1, iters + 64):  # k_submit + 1 for every k_submit
            m = torch.from_numpy(bernoulli_mask(cfg.seed, key, s, t - s,
                                                cfg.batch_rate))
            worst = max(worst, float(blk[m].sum(0).abs().max()) * inv_batch)
    if algo == "asaga":
        worst += float(yx.abs().sum(0).max()) / cfg.N
    cfg.l1 = 2.0 * worst
    eng = _engine(cfg, X.to(DEV), y.to(DEV))
    res = eng.run(max_wall_s=120)
    print(algo, "l1", cfg.l1, "applied", res["applied"], "k", res["k"])
    assert res["applied"] > 0 and res["k"] >= iters
    assert torch.equal(eng.w, torch.zeros(cfg.d, device=DEV))
    assert not bool(torch.signbit(eng.w).any())
    if algo == "asaga":
        assert float(eng.alpha_bar.abs().max()) > 0
