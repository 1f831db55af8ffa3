"""Fused evaluation kernels (csrc/eval.h) on MI355X against an fp64 CPU
reference on the exact (bf16-rounded) data.

The kink rule: a predicted class is a step function of z, so a row whose
fp64 score lies within rounding of the threshold may fall either side in
fp32. Each case computes z_ref in fp64 and the rigorous dot-product bound
band_i = (d + 2) * 2^-23 * sum_j |x_ij| |w_j|, removes — before the kernel
sees the data — every row with |z_ref - z_thr| <= band for any iterate,
asserts that at most 10 % of the rows went, and then requires the counts to
match exactly. Tests that compare no decision against the reference
(tiling, repeatability, bounds) run on the unfiltered data."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops

OBJECTIVES = ["lsq", "logistic", "hinge"]
_ALT_THR = {"lsq": 0.3, "logistic": 0.3, "hinge": -0.25}
LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-6  # the fp32 objective sweep's bound

# (rows, d): one row; fewer rows than waves; flagship row length on a ragged
# grid; one lane into the second load round; largest pipelined d; the
# fallback on d > 2048; the fallback on d % 4 != 0
DENSE_SHAPES = [(1, 4), (3, 784), (1000, 784), (512, 260), (600, 2048),
                (300, 2052), (500, 787)]


def _core():
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    import asyncframework_amd._hip_core as core
    return core


def _ref(Z, y, objective, z_thr):
    """fp64 (loss_sum, tp, fp, tn, fn) per iterate from fp64 scores."""
    y = y.double()[:, None]
    s = 2.0 * y - 1.0
    if objective == "lsq":
        loss = (Z - y) ** 2
    elif objective == "logistic":
        loss = torch.clamp(-s * Z, min=0) + torch.log1p(
            torch.exp(-(s * Z).abs()))
    else:
        loss = torch.clamp(1.0 - s * Z, min=0)
    pos, pred = y > 0.5, Z > z_thr
    return (loss.sum(0), (pos & pred).sum(0), (~pos & pred).sum(0),
            (~pos & ~pred).sum(0), (pos & ~pred).sum(0))


def _kink_keep(Z, absZ, d, z_thr):
    """Rows to keep for decisions at z_thr: farther than the band from it
    for every iterate. Z, absZ: fp64 [n, T] scores and sum_j |x_ij||w_tj|.
    The removed share is capped at 10 %."""
    n = Z.shape[0]
    band = (d + 2) * 2.0 ** -23 * absZ
    keep = ((Z - z_thr).abs() > band).all(dim=1)
    removed = n - int(keep.sum())
    print(f"kink rule at z_thr={z_thr:.4g}: removed {removed}/{n}")
    assert removed <= 0.10 * n, f"kink rule removed {removed}/{n}"
    return keep


_DENSE_BASE, _DENSE_CASE = {}, {}


def _dense_base(n, d, dtype):
    """X ~ N(0, 1/sqrt(d)) rounded to dtype, W ~ N(0,1) with T = TT + 1
    iterates, {0,1} labels, and the fp64 scores — computed once per
    (shape, dtype) and shared by every test."""
    key = (n, d, dtype)
    if key not in _DENSE_BASE:
        tt = _core().eval_tile()
        g = torch.Generator().manual_seed(1000 * d + n)
        X = (torch.randn(n, d, generator=g) / math.sqrt(d)).to(dtype)
        W = torch.randn(tt + 1, d, generator=g)
        y = (torch.rand(n, generator=g) > 0.5).float()
        Xd, Wd = X.double(), W.double()
        _DENSE_BASE[key] = dict(X=X, y=y, W=W, Z=Xd @ Wd.t(),
                                absZ=Xd.abs() @ Wd.abs().t(), tt=tt)
    return _DENSE_BASE[key]


def _dense_case(n, d, dtype, z_thr=None):
    """The base case on the GPU; with z_thr, after the kink rule for
    decisions at that threshold."""
    key = (n, d, dtype, z_thr)
    if key not in _DENSE_CASE:
        b = _dense_base(n, d, dtype)
        keep = (torch.ones(n, dtype=torch.bool) if z_thr is None
                else _kink_keep(b["Z"], b["absZ"], d, z_thr))
        _DENSE_CASE[key] = dict(
            X=b["X"][keep].contiguous().cuda(), y=b["y"][keep].cuda(),
            W=b["W"].cuda(), y_cpu=b["y"][keep], Z=b["Z"][keep], tt=b["tt"])
    return _DENSE_CASE[key]


def _check(ev, ref, n, T):
    loss_sum, tp, fp, tn, fn = ref
    for name, got, want in (("tp", ev.tp, tp), ("fp", ev.fp, fp),
                            ("tn", ev.tn, tn), ("fn", ev.fn, fn)):
        assert got.dtype == torch.int64
        assert got.cpu().tolist() == want.tolist(), name
    assert (ev.tp + ev.fp + ev.tn + ev.fn).cpu().tolist() == [n] * T
    assert ev.loss.dtype == torch.float64
    got, want = ev.loss.cpu(), loss_sum / n
    err = float(((got - want).abs() / (LOSS_ATOL + LOSS_RTOL * want.abs()))
                .max())
    print(f"loss err/bound = {err:.3e}")
    assert torch.allclose(got, want, rtol=LOSS_RTOL, atol=LOSS_ATOL), (
        got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_counts_and_loss(shape, dtype):
    """Counts exact and loss within the sweep's fp32 bound of fp64 on the
    same (rounded) data — w is never rounded, so bf16 X gets no wider
    bound — for all three objectives at their default and one non-default
    threshold, with T = TT and T = TT + 1."""
    for objective in OBJECTIVES:
        for thr in (None, _ALT_THR[objective]):
            z_thr = ops.score_threshold(objective, thr)
            c = _dense_case(*shape, dtype, z_thr)
            n = c["X"].shape[0]
            for T in (c["tt"], c["tt"] + 1):
                ev = ops.evaluate(c["X"], c["y"], c["W"][:T], objective,
                                  threshold=thr)
                print(shape, dtype, objective, thr, T)
                _check(ev, _ref(c["Z"][:, :T], c["y_cpu"], objective, z_thr),
                       n, T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1000, 784), (300, 2052), (500, 787)])
def test_dense_tiling_and_repeatability(shape, dtype):
    """evaluate(W)[t] is bitwise evaluate(W[t:t+1])[0] (tile indexing), and
    two identical calls are bitwise equal."""
    c = _dense_case(*shape, dtype)
    T = c["tt"] + 1
    for objective in ("logistic", "hinge"):
        ev = ops.evaluate(c["X"], c["y"], c["W"], objective)
        ev2 = ops.evaluate(c["X"], c["y"], c["W"], objective)
        for a, b in zip(ev, ev2):
            assert torch.equal(a, b)
        for t in range(T):
            one = ops.evaluate(c["X"], c["y"], c["W"][t:t + 1], objective)
            for a, b in zip(ev, one):
                assert torch.equal(a[t:t + 1], b), (objective, t)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dense_cross_check_with_objective_sweep(objective):
    c = _dense_case(1000, 784, torch.float32)
    ev = ops.evaluate(c["X"], c["y"], c["W"], objective)
    sw = ops.objective_sweep(c["X"], c["y"], c["W"], objective)
    assert torch.allclose(ev.loss, sw, rtol=1e-4), (ev.loss, sw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 784), (512, 260), (600, 2048),
                                   (500, 787)])
def test_dense_bounds(shape, dtype):
    """X is the head of a larger buffer whose tail is NaN: nothing past the
    last row may be fetched into a result (0 * NaN = NaN), also by the
    clamped prefetch and the lanes past d."""
    c = _dense_case(*shape, dtype)
    n, d = c["X"].shape
    big = torch.full((n + 7, d), float("nan"), dtype=dtype, device="cuda")
    big[:n] = c["X"]
    ybig = torch.full((n + 7,), float("nan"), device="cuda")
    ybig[:n] = c["y"]
    want = ops.evaluate(c["X"], c["y"], c["W"], "logistic")
    got = ops.evaluate(big[:n], ybig[:n], c["W"], "logistic")
    assert bool(torch.isfinite(got.loss).all())
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# --------------------------------------------------------------------- CSR

_CSR_BASE, _CSR_CASE = {}, {}


def _csr_base(dtype):
    """513 rows, d = 1000: row 0 empty (z = 0), row 1 one entry, row 2 two
    hundred entries (> LPR), the rest ~20 entries."""
    if dtype not in _CSR_BASE:
        tt = _core().eval_tile()
        n, d = 513, 1000
        rng = np.random.default_rng(7)
        counts = rng.poisson(20, size=n).clip(1, 60)
        counts[0], counts[1], counts[2] = 0, 1, 200
        g = torch.Generator().manual_seed(8)
        W = torch.randn(tt + 1, d, generator=g)
        y = (torch.rand(n, generator=g) > 0.5).float()
        cols, vals = [], []
        X = torch.zeros(n, d, dtype=torch.float64)
        for i, c in enumerate(counts):
            cc = np.sort(rng.choice(d, size=c, replace=False))
            v = torch.from_numpy(
                rng.standard_normal(c) / math.sqrt(20)).float().to(dtype)
            cols.append(cc.astype(np.int32))
            vals.append(v)
            X[i, torch.from_numpy(cc)] = v.double()
        Wd = W.double()
        _CSR_BASE[dtype] = dict(counts=counts, cols=cols, vals=vals, y=y,
                                W=W, Z=X @ Wd.t(),
                                absZ=X.abs() @ Wd.abs().t(), tt=tt, n=n, d=d)
    return _CSR_BASE[dtype]


def _csr_case(dtype, z_thr=None):
    key = (dtype, z_thr)
    if key not in _CSR_CASE:
        b = _csr_base(dtype)
        keep = torch.ones(b["n"], dtype=torch.bool)
        if z_thr is not None:
            # the empty row's score is exactly 0 with band 0: it is exact in
            # every precision (also ON the threshold 0, where z > z_thr is
            # false), so it stays in
            keep[1:] = _kink_keep(b["Z"][1:], b["absZ"][1:], b["d"], z_thr)
            assert bool(keep[:3].all()), "a special row sits on a threshold"
        rows = keep.nonzero()[:, 0].tolist()
        indptr = np.zeros(len(rows) + 1, dtype=np.int32)
        indptr[1:] = np.cumsum([b["counts"][i] for i in rows])
        _CSR_CASE[key] = dict(
            indptr=torch.from_numpy(indptr).cuda(),
            indices=torch.from_numpy(
                np.concatenate([b["cols"][i] for i in rows])).cuda(),
            values=torch.cat([b["vals"][i] for i in rows]).cuda(),
            y=b["y"][keep].cuda(), y_cpu=b["y"][keep], W=b["W"].cuda(),
            Z=b["Z"][keep], tt=b["tt"], n=len(rows))
    return _CSR_CASE[key]


def _csr_eval(c, W, objective, **kw):
    return ops.evaluate_csr(c["indptr"], c["indices"], c["values"], c["y"],
                            W, objective, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_counts_and_loss(dtype):
    for objective in OBJECTIVES:
        for thr in (None, _ALT_THR[objective]):
            z_thr = ops.score_threshold(objective, thr)
            c = _csr_case(dtype, z_thr)
            for T in (c["tt"], c["tt"] + 1):
                ev = _csr_eval(c, c["W"][:T], objective, threshold=thr)
                print(dtype, objective, thr, T)
                _check(ev, _ref(c["Z"][:, :T], c["y_cpu"], objective, z_thr),
                       c["n"], T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_tiling_repeatability_and_bounds(dtype):
    c = _csr_case(dtype)
    T = c["tt"] + 1
    ev = _csr_eval(c, c["W"], "logistic")
    ev2 = _csr_eval(c, c["W"], "logistic")
    for a, b in zip(ev, ev2):
        assert torch.equal(a, b)
    for t in range(T):
        one = _csr_eval(c, c["W"][t:t + 1], "logistic")
        for a, b in zip(ev, one):
            assert torch.equal(a[t:t + 1], b), t
    # trailing NaN values (and wild column ids) beyond indptr[-1]
    nnz = c["values"].numel()
    vbig = torch.full((nnz + 300,), float("nan"), dtype=dtype, device="cuda")
    vbig[:nnz] = c["values"]
    ibig = torch.zeros(nnz + 300, dtype=torch.int32, device="cuda")
    ibig[:nnz] = c["indices"]
    got = ops.evaluate_csr(c["indptr"], ibig[:nnz], vbig[:nnz], c["y"],
                           c["W"], "logistic")
    assert bool(torch.isfinite(got.loss).all())
    for a, b in zip(got, ev):
        assert torch.equal(a, b)


def test_csr_cross_check_with_objective_sweep():
    c = _csr_case(torch.float32)
    for objective in OBJECTIVES:
        ev = _csr_eval(c, c["W"], objective)
        sw = ops.objective_sweep_csr(c["indptr"], c["indices"], c["values"],
                                     c["y"], c["W"], objective)
        assert torch.allclose(ev.loss, sw, rtol=1e-4), (ev.loss, sw)


# --------------------------------------------------------------- the rest

def test_zero_rows_launch_nothing():
    W = torch.randn(3, 8, device="cuda")
    ev = ops.evaluate(torch.zeros(0, 8, device="cuda"),
                      torch.zeros(0, device="cuda"), W, "hinge")
    assert ev.loss.is_cuda and ev.loss.tolist() == [0.0] * 3
    assert ev.tp.tolist() == [0] * 3


def test_eval_kernel_resources():
    """No instantiation spills, and every one of them is reported."""
    info = _core().eval_kernel_info()
    names = list(info)
    assert sum(n.startswith("eval_dense_kernel<") for n in names) == 16
    assert sum(n.startswith("eval_dense_generic_kernel<") for n in names) == 2
    assert sum(n.startswith("eval_csr_kernel<") for n in names) == 2
    for name, e in info.items():
        print(name, dict(e))
        assert e["local_size_bytes"] == 0, (name, dict(e))
        assert e["max_active_blocks_per_cu"] >= 1, (name, dict(e))
        assert e["num_regs"] > 0
