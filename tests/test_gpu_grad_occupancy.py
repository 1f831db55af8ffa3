"""Dense gradient kernel occupancy / row-bounds / batched-queue work and the
restructured multi_update kernel, on MI355X.

Dense references are ops.torch_ref on the bernoulli_mask mask with the
tolerances of test_gpu_kernels.test_grad_dense_matches_ref (relative L2 2e-4
fp32, 2e-2 bf16; counts exactly equal)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.utils.philox import bernoulli_mask


def _core():
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    import asyncframework_amd._hip_core as core
    return core


def _dense(n, d, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(n, d, generator=g, device="cuda", dtype=torch.float32)
    y = torch.randn(n, generator=g, device="cuda")
    w = torch.randn(d, generator=g, device="cuda")
    return X.to(dtype), y, w


def _tol(dtype):
    return 2e-2 if dtype == torch.bfloat16 else 2e-4


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


# ------------------------------------------------------------ resource guard

@pytest.mark.parametrize("d,bf16,saga,wave", [
    (784, 1, 0, 1),    # flagship wave kernel
    (784, 1, 1, 1),    # SAGA wave kernel
    (2000, 0, 0, 1),   # fp32 epsilon shape, ITERS=8
    (784, 1, 0, 0),    # solo pipe kernel
])
def test_dense_kernel_resources(d, bf16, saga, wave):
    """No scratch, and at least two 256-thread blocks per CU: two is what
    makes the 512-block wave grid co-resident on 256 CUs. (Before the body
    was inlined under a waves-per-SIMD hint the flagship read 1 block and
    12 B of scratch.)"""
    info = _core().dense_kernel_info(d, bf16, saga, wave)
    print(d, bf16, saga, wave, dict(info))
    assert info["iters"] == (d + 255) // 256
    assert info["local_size_bytes"] == 0, info
    assert info["max_active_blocks_per_cu"] >= 2, info


# ---------------------------------------------------------------- row bounds

_RB_SEED, _RB_ROUND, _RB_N, _RB_RATE = 5, 4, 64, 0.5


def test_row_bounds_mask_covers_last_row():
    """CPU-checkable premise of the row-bounds cases: the last row of X is
    sampled (its padded lanes would run past the end of X), and sampled
    rows are followed by unsampled (NaN) ones."""
    m = bernoulli_mask(_RB_SEED, _RB_ROUND, 0, _RB_N, _RB_RATE)
    assert m[-1]
    assert any(m[i] and not m[i + 1] for i in range(_RB_N - 1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [4, 256, 260, 784, 2048])
def test_row_bounds_ignore_neighbour_rows(d, dtype):
    """Every unsampled row is NaN. The loaders issue ITERS*64 lanes per row;
    lanes past d must be zero-filled by the descriptor's bounds check, not
    read from the next row (0 * NaN = NaN). d covers one active lane, an
    exact iteration, one lane in the tail iteration, the flagship tail and
    full ITERS=8."""
    _core()
    n = _RB_N
    X, y, w = _dense(n, d, seed=100 + d, dtype=dtype)
    m = bernoulli_mask(_RB_SEED, _RB_ROUND, 0, n, _RB_RATE)
    assert m[-1] and not m.all()
    mask = torch.from_numpy(m).cuda()
    X_ref = X.clone()
    X_ref[~mask] = 0
    X[~mask] = float("nan")
    g, cnt = ops.grad_dense(X, y, w, seed=_RB_SEED, round_k=_RB_ROUND,
                            row_start=0, rate=_RB_RATE)
    g_ref, cnt_ref = torch_ref.grad_dense(X_ref.float(), y, w, mask, "lsq")
    assert cnt == cnt_ref == int(m.sum())
    assert bool(torch.isfinite(g).all()), "neighbour-row NaN leaked into g"
    rel = _rel(g, g_ref)
    print(f"d={d} {dtype} rel={rel:.3e}")
    assert rel < _tol(dtype), f"rel err {rel}"


# ------------------------------------- queue chunking with batched y / alpha

@pytest.mark.parametrize("rate", [1.0, 0.5])
def test_single_block_queue_chunks_asgd(rate, monkeypatch):
    """One block (ASYNCAMD_GRAD_GRID=1) cycles scan / fetch / process several
    times over n=5000 rows, past the 1,024-entry scan break."""
    _core()
    monkeypatch.setenv("ASYNCAMD_GRAD_GRID", "1")
    n, d = 5000, 64
    X, y, w = _dense(n, d, seed=31)
    g, cnt = ops.grad_dense(X, y, w, seed=17, round_k=3, row_start=0,
                            rate=rate)
    m = bernoulli_mask(17, 3, 0, n, rate)
    assert int(m.sum()) > 1024
    g_ref, cnt_ref = torch_ref.grad_dense(
        X, y, w, torch.from_numpy(m).cuda(), "lsq")
    assert cnt == cnt_ref
    rel = _rel(g, g_ref)
    print(f"rate={rate} rel={rel:.3e}")
    assert rel < 2e-4, f"rel err {rel}"


@pytest.mark.parametrize("rate", [1.0, 0.5])
def test_single_block_queue_chunks_saga(rate, monkeypatch):
    _core()
    monkeypatch.setenv("ASYNCAMD_GRAD_GRID", "1")
    n, d = 5000, 64
    X, y, w = _dense(n, d, seed=32)
    alpha = torch.randn(n, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(33))
    g, idx, e, cnt = ops.saga_grad_dense(X, y, w, alpha, seed=17, round_k=3,
                                         row_start=0, rate=rate)
    m = bernoulli_mask(17, 3, 0, n, rate)
    assert int(m.sum()) > 1024
    g_ref, idx_ref, e_ref, cnt_ref = torch_ref.saga_grad_dense(
        X, y, w, alpha, torch.from_numpy(m).cuda(), "lsq")
    assert cnt == cnt_ref
    order = torch.argsort(idx)
    assert torch.equal(idx[order], idx_ref)
    assert torch.allclose(e[order], e_ref, atol=1e-3, rtol=1e-3)
    rel = _rel(g, g_ref)
    print(f"rate={rate} rel={rel:.3e}")
    assert rel < 2e-4, f"rel err {rel}"


# ------------------------------------- list form (scan_rows + grad_dense_list)

def _list_grad(X, y, w, seed, round_k, rate):
    """The graph engine's split form, launched directly: scan_rows fills the
    compacted row list, grad_dense_list writes per-block partials,
    reduce_partials sums them. Returns (g, listed row count)."""
    core = _core()
    n, d = X.shape
    st = torch.cuda.current_stream().cuda_stream
    G = int(core.grad_grid(n))
    rowlist = torch.zeros(n, dtype=torch.int32, device="cuda")
    ylist = torch.zeros(n, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    g_part = torch.zeros(d * G, device="cuda")
    g = torch.zeros(d, device="cuda")
    core.scan_rows(y.data_ptr(), rowlist.data_ptr(), ylist.data_ptr(),
                   count.data_ptr(), 0, n, seed, round_k, 0, rate, st)
    core.grad_dense_list(X.data_ptr(), w.data_ptr(), g_part.data_ptr(),
                         rowlist.data_ptr(), ylist.data_ptr(),
                         count.data_ptr(), n, d, 0,
                         1 if X.dtype == torch.bfloat16 else 0, st)
    core.reduce_partials(g_part.data_ptr(), g.data_ptr(), d, G, 1, st)
    torch.cuda.synchronize()
    return g, int(count.item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [4, 260, 2048])
def test_list_form_matches_ref(d, dtype):
    """The row-bounds shapes through the list kernel: one active lane, one
    lane in the tail iteration, full ITERS=8. The listed-row count is no
    multiple of DEPTH * waves, so the pipeline ends on clamped tail slots."""
    n = _RB_N
    X, y, w = _dense(n, d, seed=100 + d, dtype=dtype)
    m = bernoulli_mask(_RB_SEED, _RB_ROUND, 0, n, _RB_RATE)
    assert int(m.sum()) % 16 != 0
    g, cnt = _list_grad(X, y, w, _RB_SEED, _RB_ROUND, _RB_RATE)
    g_ref, cnt_ref = torch_ref.grad_dense(
        X.float(), y, w, torch.from_numpy(m).cuda(), "lsq")
    assert cnt == cnt_ref == int(m.sum())
    rel = _rel(g, g_ref)
    print(f"d={d} {dtype} rel={rel:.3e}")
    assert rel < _tol(dtype), f"rel err {rel}"


def test_list_form_depth_override(monkeypatch):
    """ASYNCAMD_PIPE_DEPTH reaches the list kernel like the other pipelined
    kernels: depth 1 (one row in flight per wave, every refill clamped or
    one row ahead) computes the same gradient."""
    monkeypatch.setenv("ASYNCAMD_PIPE_DEPTH", "1")
    n, d = _RB_N, 260
    X, y, w = _dense(n, d, seed=100 + d)
    m = bernoulli_mask(_RB_SEED, _RB_ROUND, 0, n, _RB_RATE)
    g, cnt = _list_grad(X, y, w, _RB_SEED, _RB_ROUND, _RB_RATE)
    g_ref, cnt_ref = torch_ref.grad_dense(
        X, y, w, torch.from_numpy(m).cuda(), "lsq")
    assert cnt == cnt_ref == int(m.sum())
    rel = _rel(g, g_ref)
    print(f"rel={rel:.3e}")
    assert rel < 2e-4, f"rel err {rel}"


def test_list_form_single_block_chunks(monkeypatch):
    """One block (ASYNCAMD_GRAD_GRID=1) owns the whole 5,000-row list and
    walks it in three queue-capacity chunks, the last one partial."""
    monkeypatch.setenv("ASYNCAMD_GRAD_GRID", "1")
    n, d = 5000, 64
    X, y, w = _dense(n, d, seed=34)
    g, cnt = _list_grad(X, y, w, 17, 3, 1.0)
    m = bernoulli_mask(17, 3, 0, n, 1.0)
    assert int(m.sum()) == n > 2 * 2048
    g_ref, cnt_ref = torch_ref.grad_dense(
        X, y, w, torch.from_numpy(m).cuda(), "lsq")
    assert cnt == cnt_ref == n
    rel = _rel(g, g_ref)
    print(f"rel={rel:.3e}")
    assert rel < 2e-4, f"rel err {rel}"


def test_list_form_ignores_neighbour_rows():
    """test_row_bounds_ignore_neighbour_rows through the list kernel: every
    unlisted row is NaN and none of it may reach g."""
    n, d = _RB_N, 260
    X, y, w = _dense(n, d, seed=100 + d)
    m = bernoulli_mask(_RB_SEED, _RB_ROUND, 0, n, _RB_RATE)
    assert m[-1] and not m.all()
    mask = torch.from_numpy(m).cuda()
    X_ref = X.clone()
    X_ref[~mask] = 0
    X[~mask] = float("nan")
    g, cnt = _list_grad(X, y, w, _RB_SEED, _RB_ROUND, _RB_RATE)
    g_ref, cnt_ref = torch_ref.grad_dense(X_ref, y, w, mask, "lsq")
    assert cnt == cnt_ref == int(m.sum())
    assert bool(torch.isfinite(g).all()), "neighbour-row NaN leaked into g"
    rel = _rel(g, g_ref)
    print(f"rel={rel:.3e}")
    assert rel < 2e-4, f"rel err {rel}"


# -------------------------------------------------------------- multi_update

_MU_P = 32           # worker buffers in the tables
_GAMMA = 2.0 ** -7   # engine-like step sizes: the correction is small
_INV_BATCH = 0.5     # next to the running value it is applied to
_INV_N = 2.0 ** -10


def _mu_inputs(d, seed):
    """Device-side tables of 16-byte-aligned per-worker buffers."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    # |w| and |alpha_bar| in [0.5, 2.5): the bound below is relative to the
    # running value, so keep that value away from zero
    sgn = lambda t: torch.where(t >= 0, 1.0, -1.0)
    w0 = r(d)
    w0 = sgn(w0) * (0.5 + 2 * torch.rand(d, device="cuda", generator=gen))
    ab0 = r(d)
    ab0 = sgn(ab0) * (0.5 + 2 * torch.rand(d, device="cuda", generator=gen))
    dpad = (d + 3) // 4 * 4  # rows of a [P, dpad] tensor stay 16-B aligned
    G = torch.zeros(_MU_P, dpad, device="cuda")
    G[:, :d] = r(_MU_P, d)
    WB = torch.full((_MU_P, dpad), 7.0, device="cuda")
    return w0, ab0, G, WB


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("d", [5, 784])
@pytest.mark.parametrize("m", [0, 3])
@pytest.mark.parametrize("n", [1, 9, 32])
def test_multi_update_matches_fp64_sequential(n, m, d, algo):
    """multi_update_kernel vs an fp64 sequential loop in the same j order.
    Each step rounds the running value once, so per element the error is at
    most n * 2^-24 * (largest magnitude the running value takes in the fp64
    loop); alpha_bar gets the same bound. Consumed g must be exactly zero,
    untouched g unchanged, snapshot targets bit-identical to w."""
    core = _core()
    w, ab, G, WB = _mu_inputs(d, seed=1000 + 10 * n + m + d + algo)
    perm = np.random.RandomState(n * 7 + m).permutation(_MU_P)
    gw = [int(v) for v in perm[:n]]            # distinct worker ids
    sw = [int(v) for v in perm[::-1][:m]]
    scale = [float(np.float32(0.01 / np.sqrt(j + 1.0))) for j in range(n)]
    G0 = G.clone()
    WB0 = WB.clone()

    # fp64 sequential reference + running-magnitude bounds
    w64 = w.double().cpu().numpy()
    ab64 = ab.double().cpu().numpy()
    g64 = G0[:, :d].double().cpu().numpy()
    gam, ib, iN = (float(np.float32(v)) for v in (_GAMMA, _INV_BATCH, _INV_N))
    wmax, abmax = np.abs(w64), np.abs(ab64)
    for j in range(n):
        gi = g64[gw[j]]
        if algo == 0:
            w64 = w64 - scale[j] * gi
        else:
            w64 = w64 - gam * (ib * gi + ab64)
            ab64 = ab64 + iN * gi
        wmax = np.maximum(wmax, np.abs(w64))
        abmax = np.maximum(abmax, np.abs(ab64))

    vec4 = core.multi_update(
        w.data_ptr(), [G[p].data_ptr() for p in range(_MU_P)],
        [WB[p].data_ptr() for p in range(_MU_P)],
        ab.data_ptr() if algo == 1 else 0, _GAMMA, _INV_BATCH, _INV_N, d,
        algo, gw, sw, scale if algo == 0 else [],
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert vec4 == (d % 4 == 0)  # d=784 runs the float4 form, d=5 the scalar

    w_err = np.abs(w.double().cpu().numpy() - w64)
    w_bound = n * 2.0 ** -24 * wmax
    print(f"n={n} m={m} d={d} algo={algo} "
          f"max w err/bound={float((w_err / w_bound).max()):.3f}")
    assert (w_err <= w_bound).all()
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
