"""Threshold-sweep kernels (csrc/eval_curve.h) on MI355X against fp64 counts
computed here on the CPU from the exact (bf16-rounded) data.

The data recipes and the kink rule are those of tests/test_gpu_evaluate.py,
re-created here: a predicted class is a step function of z, so a row whose
fp64 score lies within the rigorous dot-product bound
band_i = (d + 2) * 2^-23 * sum_j |x_ij| |w_j| of a threshold may fall either
side in fp32. The exact real-valued tests remove such rows — for ANY of the
thresholds and iterates, at most 10 % of the rows — before the kernel sees
the data; the bracket test removes nothing and bounds every count between
the fp64 counts of z - band and z + band; the integer test needs neither,
because every partial sum is an integer below 2^24 and the fp32 score is
exact."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops

OBJECTIVES = ["lsq", "logistic", "hinge"]
COUNTS = ("tp", "fp", "tn", "fn")
# (rows, d): one row; fewer rows than waves; flagship row length on a ragged
# grid; one lane into the second load round; largest pipelined d; the
# fallback on d > 2048; the fallback on d % 4 != 0
DENSE_SHAPES = [(1, 4), (3, 784), (1000, 784), (512, 260), (600, 2048),
                (300, 2052), (500, 787)]
# the two thresholds of the exact real-valued tests, in the user's units
USER_THR = {"lsq": [-0.75, 0.75], "hinge": [-0.75, 0.75],
            "logistic": [0.32, 0.68]}  # z = -+0.7538


def _core():
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    import asyncframework_amd._hip_core as core
    return core


def _ref_counts(Z, y, thr):
    """fp64 counts: Z [n, T] scores, thr [T, K]. Returns the four [T, K]
    int64 tensors and (n_pos, n_neg)."""
    pos = (y > 0.5)[:, None, None]
    pred = Z[:, :, None] > thr[None]
    tp, fp = (pos & pred).sum(0), (~pos & pred).sum(0)
    n_pos = int((y > 0.5).sum())
    n_neg = Z.shape[0] - n_pos
    return dict(tp=tp, fp=fp, tn=n_neg - fp, fn=n_pos - tp), n_pos, n_neg


def _assert_counts(cv, Z, y, thr=None):
    thr = cv.z_thr.cpu() if thr is None else thr
    want, n_pos, n_neg = _ref_counts(Z, y, thr)
    T = Z.shape[1]
    for c in COUNTS:
        got = getattr(cv, c)
        assert got.dtype == torch.int64 and got.is_cuda
        assert torch.equal(got.cpu(), want[c]), c
    assert cv.n_pos.cpu().tolist() == [n_pos] * T
    assert cv.n_neg.cpu().tolist() == [n_neg] * T


def _mann_whitney(z, y):
    """Tie-aware P(z+ > z-) + P(z+ == z-) / 2 over all pairs, fp64."""
    pos, neg = z[y > 0.5], z[y <= 0.5]
    gt = (pos[:, None] > neg[None, :]).sum()
    eq = (pos[:, None] == neg[None, :]).sum()
    return (float(gt) + 0.5 * float(eq)) / (pos.numel() * neg.numel())


def _to_csr(X):
    """CSR of a dense CPU matrix, values in X's dtype, on the GPU."""
    sp = X.float().to_sparse_csr()
    return (sp.crow_indices().to(torch.int32).cuda(),
            sp.col_indices().to(torch.int32).cuda(),
            sp.values().to(X.dtype).cuda())


def _kink_keep(Z, absZ, d, z_thrs):
    """Rows farther than the band from every threshold for every iterate.
    The removed share is capped at 10 %."""
    n = Z.shape[0]
    band = (d + 2) * 2.0 ** -23 * absZ
    keep = torch.ones(n, dtype=torch.bool)
    for z_thr in z_thrs:
        keep &= ((Z - z_thr).abs() > band).all(dim=1)
    removed = n - int(keep.sum())
    print(f"kink rule at z_thr={z_thrs}: removed {removed}/{n}")
    assert removed <= 0.10 * n, f"kink rule removed {removed}/{n}"
    return keep


# ------------------------------------------------- exact, many thresholds

_INT = {}


def _int_case(d):
    """X in {-2..2} [700, 784], W in {-3..3} [TT + 1, 784], seed 5; d = 783
    cuts a column, d = 787 appends three more drawn from the same generator
    (both take the d % 4 != 0 fallback). |z| <= 300 is asserted."""
    if not _INT:
        tt = _core().eval_tile()
        g = torch.Generator().manual_seed(5)
        X = torch.randint(-2, 3, (700, 784), generator=g)
        W = torch.randint(-3, 4, (tt + 1, 784), generator=g)
        X = torch.cat([X, torch.randint(-2, 3, (700, 3), generator=g)], 1)
        W = torch.cat([W, torch.randint(-3, 4, (tt + 1, 3), generator=g)], 1)
        y = (torch.rand(700, generator=g) > 0.5).float()
        _INT.update(X=X.float(), W=W.float(), y=y)
    X, W, y = _INT["X"][:, :d], _INT["W"][:, :d], _INT["y"]
    Z = X.double() @ W.double().t()
    assert float(Z.abs().max()) <= 300
    return X.contiguous(), W.contiguous(), y, Z


INT_THR = [m + 0.5 for m in range(-301, 301)]  # 602: several passes


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", ["dense784", "dense783", "dense787", "csr"])
def test_integer_data_many_thresholds(form, dtype):
    """602 thresholds m + 1/2 between the integer scores: no kink is
    possible, the counts equal the fp64 ones and auc_roc is the tie-aware
    Mann-Whitney statistic of the fp64 scores."""
    X, W, y, Z = _int_case(int(form[5:]) if form != "csr" else 784)
    assert len(INT_THR) > 4 * _core().eval_curve_tile()
    Xd = X.to(dtype)
    if form == "csr":
        cv = ops.evaluate_curve_csr(*_to_csr(Xd), y.cuda(), W.cuda(),
                                    "hinge", z_thresholds=INT_THR)
    else:
        cv = ops.evaluate_curve(Xd.cuda(), y.cuda(), W.cuda(), "hinge",
                                z_thresholds=INT_THR)
    thr = torch.tensor(INT_THR, dtype=torch.float64).expand(W.shape[0], -1)
    _assert_counts(cv, Z, y, thr)
    auc = cv.auc_roc().cpu()
    for t in range(W.shape[0]):
        want = _mann_whitney(Z[:, t], y)
        print(form, dtype, t, float(auc[t]), want)
        assert float(auc[t]) == pytest.approx(want, abs=1e-12)


# ------------------------------------------------------ real-valued data

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


def _dense_case(n, d, dtype, z_thrs=None):
    """The base case on the GPU; with z_thrs, after the kink rule for
    decisions at all of those thresholds."""
    key = (n, d, dtype, z_thrs)
    if key not in _DENSE_CASE:
        b = _dense_base(n, d, dtype)
        keep = (torch.ones(n, dtype=torch.bool) if z_thrs is None
                else _kink_keep(b["Z"], b["absZ"], d, z_thrs))
        _DENSE_CASE[key] = dict(
            X=b["X"][keep].contiguous().cuda(), y=b["y"][keep].cuda(),
            W=b["W"].cuda(), y_cpu=b["y"][keep], Z=b["Z"][keep],
            absZ=b["absZ"][keep], tt=b["tt"], d=d)
    return _DENSE_CASE[key]


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


def _csr_case(dtype, z_thrs=None):
    key = (dtype, z_thrs)
    if key not in _CSR_CASE:
        b = _csr_base(dtype)
        keep = torch.ones(b["n"], dtype=torch.bool)
        if z_thrs is not None:
            # the empty row's score is exactly 0 with band 0: exact in every
            # precision, so it stays in
            keep[1:] = _kink_keep(b["Z"][1:], b["absZ"][1:], b["d"], z_thrs)
            removed = b["n"] - int(keep.sum())
            assert removed <= 0.01 * b["n"], removed
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
            Z=b["Z"][keep], absZ=b["absZ"][keep], tt=b["tt"], n=len(rows),
            d=b["d"])
    return _CSR_CASE[key]


def _csr_curve(c, W, objective, **kw):
    return ops.evaluate_curve_csr(c["indptr"], c["indices"], c["values"],
                                  c["y"], W, objective, **kw)


def _z_thrs(objective):
    return tuple(sorted(ops.score_threshold(objective, t)
                        for t in USER_THR[objective]))


def _check_two_thresholds(cv, ev_at, c, objective, T):
    """Counts exact against fp64, and column k equal to ops.evaluate at
    that threshold on the same filtered data."""
    z_thrs = _z_thrs(objective)
    assert cv.z_thr.cpu().tolist() == [list(z_thrs)] * T
    _assert_counts(cv, c["Z"][:, :T], c["y_cpu"])
    for k, thr in enumerate(sorted(USER_THR[objective])):
        ev = ev_at(thr)
        for name in COUNTS:
            assert torch.equal(getattr(cv, name)[:, k], getattr(ev, name)), (
                name, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_two_thresholds_exact(shape, dtype):
    for objective in OBJECTIVES:
        c = _dense_case(*shape, dtype, _z_thrs(objective))
        for T in (c["tt"], c["tt"] + 1):
            W = c["W"][:T]
            cv = ops.evaluate_curve(c["X"], c["y"], W, objective,
                                    thresholds=USER_THR[objective])
            print(shape, dtype, objective, T)
            _check_two_thresholds(
                cv, lambda thr: ops.evaluate(c["X"], c["y"], W, objective,
                                             threshold=thr),
                c, objective, T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_two_thresholds_exact(dtype):
    for objective in OBJECTIVES:
        c = _csr_case(dtype, _z_thrs(objective))
        for T in (c["tt"], c["tt"] + 1):
            W = c["W"][:T]
            cv = _csr_curve(c, W, objective, thresholds=USER_THR[objective])
            _check_two_thresholds(
                cv, lambda thr: ops.evaluate_csr(
                    c["indptr"], c["indices"], c["values"], c["y"], W,
                    objective, threshold=thr),
                c, objective, T)


def _check_bracket(cv, c):
    """Every count lies between the fp64 counts of z - band and z + band;
    the totals are exact."""
    thr = cv.z_thr.cpu()
    assert thr.shape[1] == 33 and bool((thr[:, 1:] >= thr[:, :-1]).all())
    band = (c["d"] + 2) * 2.0 ** -23 * c["absZ"]
    lo, n_pos, n_neg = _ref_counts(c["Z"] - band, c["y_cpu"], thr)
    hi, _, _ = _ref_counts(c["Z"] + band, c["y_cpu"], thr)
    for name in ("tp", "fp"):
        got = getattr(cv, name).cpu()
        width = int((hi[name] - lo[name]).max())
        print(f"{name}: widest bracket {width}")
        assert bool((lo[name] <= got).all() and (got <= hi[name]).all()), name
    T = thr.shape[0]
    assert cv.n_pos.cpu().tolist() == [n_pos] * T
    assert cv.n_neg.cpu().tolist() == [n_neg] * T
    assert torch.equal(cv.tp + cv.fn, cv.n_pos[:, None].expand(-1, 33))
    assert torch.equal(cv.fp + cv.tn, cv.n_neg[:, None].expand(-1, 33))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_bracket_nothing_removed(shape, dtype):
    c = _dense_case(*shape, dtype)
    _check_bracket(ops.evaluate_curve(c["X"], c["y"], c["W"], "logistic",
                                      num_bins=33), c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_bracket_nothing_removed(dtype):
    c = _csr_case(dtype)
    _check_bracket(_csr_curve(c, c["W"], "logistic", num_bins=33), c)


# ----------------------------------------------- tiling and repeatability

def _check_tiling(curve, W):
    """curve(W, z) -> CurveResult. Two calls are bitwise equal; iterate t
    alone gives row t; KT + 1 thresholds equal their two halves."""
    kt = _core().eval_curve_tile()
    K = kt + 1
    z = curve(W, num_bins=K).z_thr
    assert z.shape == (W.shape[0], K)
    cv, cv2 = curve(W, z_thresholds=z), curve(W, z_thresholds=z)
    for a, b in zip(cv, cv2):
        assert torch.equal(a, b)
    for t in range(W.shape[0]):
        one = curve(W[t:t + 1], z_thresholds=z[t:t + 1])
        for a, b in zip(cv, one):
            assert torch.equal(a[t:t + 1], b), t
    for cut in (kt, K // 2):
        left = curve(W, z_thresholds=z[:, :cut])
        right = curve(W, z_thresholds=z[:, cut:])
        for name in COUNTS + ("z_thr",):
            both = torch.cat([getattr(left, name), getattr(right, name)], 1)
            assert torch.equal(getattr(cv, name), both), (name, cut)
        assert torch.equal(cv.n_pos, left.n_pos)
        assert torch.equal(cv.n_neg, right.n_neg)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1000, 784), (300, 2052), (500, 787)])
def test_dense_tiling_and_repeatability(shape, dtype):
    c = _dense_case(*shape, dtype)
    _check_tiling(lambda W, **kw: ops.evaluate_curve(c["X"], c["y"], W,
                                                     "hinge", **kw), c["W"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_tiling_and_repeatability(dtype):
    c = _csr_case(dtype)
    _check_tiling(lambda W, **kw: _csr_curve(c, W, "hinge", **kw), c["W"])


# ----------------------------------------------------------------- bounds

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 784), (512, 260), (600, 2048),
                                   (500, 787)])
def test_dense_bounds(shape, dtype):
    """X is the head of a larger buffer whose tail is NaN: a NaN score lands
    below every threshold, so a fetch past the last row (or past d, or by
    the clamped prefetch) would move a count."""
    c = _dense_case(*shape, dtype)
    n, d = c["X"].shape
    big = torch.full((n + 7, d), float("nan"), dtype=dtype, device="cuda")
    big[:n] = c["X"]
    ybig = torch.full((n + 7,), float("nan"), device="cuda")
    ybig[:n] = c["y"]
    z = ops.curve_thresholds(c["X"], c["W"], 5)
    want = ops.evaluate_curve(c["X"], c["y"], c["W"], "logistic",
                              z_thresholds=z)
    got = ops.evaluate_curve(big[:n], ybig[:n], c["W"], "logistic",
                             z_thresholds=z)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert bool((got.tp + got.fp + got.tn + got.fn == n).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_bounds(dtype):
    """Trailing NaN values (and wild column ids) beyond indptr[-1]."""
    c = _csr_case(dtype)
    want = _csr_curve(c, c["W"], "logistic", num_bins=5)
    nnz = c["values"].numel()
    vbig = torch.full((nnz + 300,), float("nan"), dtype=dtype, device="cuda")
    vbig[:nnz] = c["values"]
    ibig = torch.zeros(nnz + 300, dtype=torch.int32, device="cuda")
    ibig[:nnz] = c["indices"]
    got = ops.evaluate_curve_csr(c["indptr"], ibig[:nnz], vbig[:nnz], c["y"],
                                 c["W"], "logistic",
                                 z_thresholds=want.z_thr)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# --------------------------------------------------------------- the rest

def test_nan_score_is_below_every_threshold():
    X = torch.tensor([[1.0, 0, 0, 0], [float("nan"), 0, 0, 0],
                      [-1.0, 0, 0, 0]], device="cuda")
    y = torch.tensor([1.0, 1.0, 0.0], device="cuda")
    W = torch.tensor([[1.0, 0, 0, 0]], device="cuda")
    cv = ops.evaluate_curve(X, y, W, "hinge", z_thresholds=[-5.0, 0.0])
    assert cv.tp.tolist() == [[1, 1]] and cv.fn.tolist() == [[1, 1]]
    assert cv.fp.tolist() == [[1, 0]] and cv.tn.tolist() == [[0, 1]]


def test_empty_inputs_launch_nothing():
    W = torch.randn(3, 8, device="cuda")
    X, y = torch.zeros(0, 8, device="cuda"), torch.zeros(0, device="cuda")
    cv = ops.evaluate_curve(X, y, W, "hinge", thresholds=[0.0, 1.0])
    assert cv.tp.is_cuda and cv.tp.tolist() == [[0, 0]] * 3
    assert cv.n_pos.tolist() == [0] * 3
    X, y = torch.randn(5, 8, device="cuda"), torch.ones(5, device="cuda")
    assert ops.evaluate_curve(X, y, W, "hinge",
                              z_thresholds=[]).tp.shape == (3, 0)
    assert ops.evaluate_curve(X, y, W[:0], "hinge",
                              num_bins=4).tp.shape == (0, 4)


def test_curve_kernel_resources():
    """Every instantiation is reported and none spills; the tile is what
    the LDS budget allows."""
    core = _core()
    assert core.eval_curve_tile() * core.eval_tile() * 16 <= 16 * 1024
    info = core.eval_curve_kernel_info()
    names = list(info)
    assert sum(n.startswith("eval_curve_dense_kernel<") for n in names) == 16
    assert sum(n.startswith("eval_curve_dense_generic_kernel<")
               for n in names) == 2
    assert sum(n.startswith("eval_curve_csr_kernel<") for n in names) == 2
    for name, e in info.items():
        print(name, dict(e))
        assert e["local_size_bytes"] == 0, (name, dict(e))
        assert e["max_active_blocks_per_cu"] >= 1, (name, dict(e))
        assert e["num_regs"] > 0
