"""objective="hinge" through the HIP gradient kernels and the GPU engines,
on MI355X, against ops.torch_ref.

The kink rule: the hinge coefficient is a step function of z (it switches at
s*z = 1, i.e. z = +1 or -1), so a row whose fp64 score lies within rounding
of a step may fall either side in fp32. Each case computes z_ref in fp64 on
the CPU from the exact (bf16-rounded) data and the rigorous dot-product
bound band_i = (d + 2) * 2^-23 * sum_j |x_ij||w_j|, removes — before any
kernel sees the data — every row with |z_ref -+ 1| <= band, asserts that at
most 10 % went, and trims to a multiple of 4 rows (one Philox eval decides
four). On what is left the kernels and the reference take the same side of
every step, and the tolerances are the ones tests/test_gpu_kernels.py holds
the same ops to."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops
from asyncframework_amd.data.shard import row_shards
from asyncframework_amd.data.synthetic import synthetic_dense
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.graph import GraphEngine
from asyncframework_amd.engine.native import NativeLocalEngine
from asyncframework_amd.engine.resident import ResidentEngine
from asyncframework_amd.engine.worker import Shard
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.utils.philox import bernoulli_mask

DEV = "cuda:0"
SCALES = [0.0, 1.5]  # w = 0: every row active; 1.5: |z| ~ 1.5, both kinds


def _require_hip():
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"


def _kink_filter(Xd, w, d):
    """Row indices to keep (fp64 X [n, d], fp32 w), a multiple of 4."""
    n = Xd.shape[0]
    wd = w.double()
    z = Xd @ wd
    band = (d + 2) * 2.0 ** -23 * (Xd.abs() @ wd.abs())
    keep = ((z - 1.0).abs() > band) & ((z + 1.0).abs() > band)
    if not bool(w.any()):
        assert bool(keep.all())  # z = 0 exactly: nothing near a step
    removed = n - int(keep.sum())
    print(f"kink rule: removed {removed}/{n}")
    assert removed <= 0.10 * n, f"kink rule removed {removed}/{n}"
    idx = keep.nonzero()[:, 0]
    return idx[:idx.numel() // 4 * 4]


def _dense_case(n, d, dtype, scale, seed):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(n, d, generator=g) / math.sqrt(d)).to(dtype)
    y = (torch.rand(n, generator=g) > 0.5).float()
    w = torch.randn(d, generator=g) * scale
    idx = _kink_filter(X.double(), w, d)
    return X[idx].contiguous().cuda(), y[idx].cuda(), w.cuda()


def _both_kinds(e, scale):
    """w = 0: every sampled row is inside the margin; otherwise the
    reference must hold active and inactive rows."""
    active = int((e != 0).sum())
    if scale == 0.0:
        assert active == e.numel() > 0
    else:
        assert 0 < active < e.numel(), (active, e.numel())


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,d", [(4096, 784), (2048, 787)])
def test_grad_dense_hinge_matches_ref(n, d, dtype, scale):
    """d = 784 runs the pipelined kernel, d = 787 the generic fallback."""
    _require_hip()
    X, y, w = _dense_case(n, d, dtype, scale, seed=d)
    n = X.shape[0]
    g, cnt = ops.grad_dense(X, y, w, seed=42, round_k=7, row_start=1000,
                            rate=0.3, objective="hinge")
    mask = torch.from_numpy(bernoulli_mask(42, 7, 1000, n, 0.3)).cuda()
    g_ref, cnt_ref = torch_ref.grad_dense(X.float(), y, w, mask, "hinge")
    _both_kinds(torch_ref._residual(X.float()[mask], y[mask], w, "hinge"),
                scale)
    assert cnt == cnt_ref
    rel = _rel(g, g_ref)
    print(f"d={d} {dtype} scale={scale} rel={rel:.3e}")
    assert rel < (2e-2 if dtype == torch.bfloat16 else 2e-4), rel


def _csr_case(n, d, nnz, scale, seed):
    """CSR rows as a dense fp64 matrix for the kink rule, then rebuilt."""
    g = torch.Generator().manual_seed(seed)
    cols = torch.stack([torch.randperm(d, generator=g)[:nnz].sort().values
                        for _ in range(n)])
    vals = torch.randn(n, nnz, generator=g) / math.sqrt(nnz)
    y = (torch.rand(n, generator=g) > 0.5).float()
    w = torch.randn(d, generator=g) * scale
    Xd = torch.zeros(n, d, dtype=torch.float64)
    Xd.scatter_(1, cols, vals.double())
    idx = _kink_filter(Xd, w, d)
    m = idx.numel()
    indptr = torch.arange(0, m * nnz + 1, nnz, dtype=torch.int32)
    return (indptr.cuda(), cols[idx].reshape(-1).int().cuda(),
            vals[idx].reshape(-1).contiguous().cuda(), y[idx].cuda(),
            w.cuda())


@pytest.mark.parametrize("scale", SCALES)
def test_grad_csr_hinge_matches_ref(scale):
    _require_hip()
    indptr, indices, values, y, w = _csr_case(3000, 500, 40, scale, seed=5)
    n = y.numel()
    g, cnt = ops.grad_csr(indptr, indices, values, y, w, seed=11, round_k=3,
                          row_start=500, rate=0.4, objective="hinge")
    mask = torch.from_numpy(bernoulli_mask(11, 3, 500, n, 0.4)).cuda()
    g_ref, cnt_ref = torch_ref.grad_csr(indptr, indices, values, y, w, mask,
                                        "hinge")
    z = (values.view(n, 40) * w[indices.view(n, 40).long()]).sum(dim=1)
    _both_kinds(torch_ref._link(z[mask], y[mask], "hinge"), scale)
    assert cnt == cnt_ref
    assert _rel(g, g_ref) < 1e-3


@pytest.mark.parametrize("scale", SCALES)
def test_saga_dense_hinge_matches_ref(scale):
    _require_hip()
    X, y, w = _dense_case(4096, 256, torch.float32, scale, seed=7)
    n = X.shape[0]
    alpha = torch.randn(n, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(8))
    g, idx, e, cnt = ops.saga_grad_dense(X, y, w, alpha, seed=21, round_k=5,
                                         row_start=0, rate=0.2,
                                         objective="hinge")
    mask = torch.from_numpy(bernoulli_mask(21, 5, 0, n, 0.2)).cuda()
    g_ref, idx_ref, e_ref, cnt_ref = torch_ref.saga_grad_dense(
        X, y, w, alpha, mask, "hinge")
    _both_kinds(e_ref, scale)
    assert cnt == cnt_ref
    order = torch.argsort(idx)
    assert torch.equal(idx[order], idx_ref)
    assert torch.allclose(e[order], e_ref, atol=1e-3, rtol=1e-3)
    assert torch.equal(e[order], e_ref)  # -1, 0 or +1: nothing to round
    assert _rel(g, g_ref) < 1e-3


@pytest.mark.parametrize("scale", SCALES)
def test_saga_csr_hinge_matches_ref(scale):
    _require_hip()
    indptr, indices, values, y, w = _csr_case(2000, 300, 20, scale, seed=9)
    n = y.numel()
    alpha = torch.randn(n, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(8))
    g, idx, e, cnt = ops.saga_grad_csr(indptr, indices, values, y, w, alpha,
                                       seed=31, round_k=2, row_start=100,
                                       rate=0.3, objective="hinge")
    mask = torch.from_numpy(bernoulli_mask(31, 2, 100, n, 0.3)).cuda()
    g_ref, idx_ref, e_ref, cnt_ref = torch_ref.saga_grad_csr(
        indptr, indices, values, y, w, alpha, mask, "hinge")
    _both_kinds(e_ref, scale)
    assert cnt == cnt_ref
    order = torch.argsort(idx)
    assert torch.equal(idx[order], idx_ref)
    assert torch.allclose(e[order], e_ref, atol=1e-3, rtol=1e-3)
    assert _rel(g, g_ref) < 1e-3


# ------------------------------------------------------------------ engines

def _cfg(**kw):
    base = dict(d=64, N=40_000, num_workers=2, num_iterations=40, gamma=0.3,
                taw=1 << 30, batch_rate=0.05, bucket_ratio=0.5,
                printer_freq=1 << 30, delay_coeff=0.0, seed=42, device=DEV,
                snapshot_weights=False, objective="hinge")
    base.update(kw)
    return EngineConfig(**base)


def _shards(cfg, X, y):
    return [Shard(row_start=s, n_rows=t - s, X=X[s:t], y=y[s:t])
            for s, t in row_shards(cfg.N, cfg.num_workers)]


@pytest.fixture(scope="module")
def data():
    cfg = _cfg()
    return synthetic_dense(cfg.N, cfg.d, seed=1, device=DEV,
                           objective="hinge")


def _hinge_obj(X, y, w):
    return float(ops.objective_sweep(X, y, w[None], "hinge")[0])


def test_native_sync_round_from_zero_is_closed_form(data):
    """At w = 0 every row is inside the margin: the round is the exact
    masked sum of -s_i x_i, to the bound of tests/test_gpu_native_sync.py."""
    X, y = data
    cfg = _cfg(sync=True, num_iterations=1)
    eng = NativeLocalEngine(cfg, _shards(cfg, X, y), torch.device(DEV))
    res = eng.run(max_wall_s=120)
    assert res["k"] == 1
    mask = torch.from_numpy(
        bernoulli_mask(cfg.seed, 1, 0, cfg.N, cfg.batch_rate)).to(DEV)
    s = 2.0 * y.double() - 1.0
    g = -(X.double()[mask] * s[mask][:, None]).sum(dim=0)
    want = -cfg.gamma * g / (cfg.batch_rate * cfg.N)
    rel = _rel(eng.w.double(), want)
    print("hinge sync round rel", rel)
    assert rel < 1e-4, rel


@pytest.mark.parametrize("sync", [False, True])
def test_native_forty_rounds_lower_the_hinge_objective(data, sync):
    X, y = data
    assert _hinge_obj(X, y, torch.zeros(64, device=DEV)) == 1.0
    cfg = _cfg(sync=sync)
    eng = NativeLocalEngine(cfg, _shards(cfg, X, y), torch.device(DEV))
    res = eng.run(max_wall_s=120)
    assert res["k"] >= 40
    assert bool(torch.isfinite(eng.w).all())
    obj = _hinge_obj(X, y, eng.w)
    print("sync" if sync else "async", "hinge objective", obj)
    assert obj < 1.0


def test_resident_engine_runs_hinge(data):
    X, y = data
    cfg = _cfg(num_iterations=60)
    eng = ResidentEngine(cfg, _shards(cfg, X, y), torch.device(DEV),
                         blocks_per_worker=4)
    res = eng.run(max_wall_s=120)
    assert res["k"] >= cfg.num_iterations
    assert bool(torch.isfinite(eng.w).all())
    assert _hinge_obj(X, y, eng.w) < 1.0


@pytest.mark.parametrize("algo", ["asgd", "asaga"])
def test_graph_engine_runs_hinge(data, algo):
    X, y = data
    cfg = _cfg(num_workers=1, num_iterations=40, algo=algo,
               gamma=0.3 if algo == "asgd" else 0.05)
    eng = GraphEngine(cfg, Shard(row_start=0, n_rows=cfg.N, X=X, y=y),
                      torch.device(DEV), unroll=10)
    eng.run(cfg.num_iterations)
    torch.cuda.synchronize()
    assert eng.k == cfg.num_iterations
    assert bool(torch.isfinite(eng.w).all())
    assert _hinge_obj(X, y, eng.w) < 1.0
