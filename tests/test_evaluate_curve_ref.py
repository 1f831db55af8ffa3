"""ops.evaluate_curve / ops.evaluate_curve_csr on the CPU tier (the fp64
torch reference) against a brute-force count loop, the metrics of a
CurveResult against MLlib's definitions written out here, the threshold
picker, and the drivers' curve block.

MLlib conventions (BinaryClassificationMetrics, AreaUnderCurve), for the
confusion at one threshold with tp, fp and the totals P, N:
  precision = tp / (tp + fp), 1 when tp + fp == 0   (Precision)
  recall    = tp / P,         0 when P == 0          (Recall)
  fpr       = fp / N,         0 when N == 0          (FalsePositiveRate)
  F_beta    = (1 + b^2) p r / (b^2 p + r), 0 when p + r == 0   (FMeasure)
  roc()  = (0, 0), the (fpr, recall) points by DESCENDING threshold, (1, 1)
  pr()   = (0, p_first), the (recall, precision) points by descending
           threshold, p_first the precision of the first (highest) one
  area   = sum over consecutive points of (x1 - x0) * (y0 + y1) / 2"""

import io
import math
import re
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from asyncframework_amd import ops, run
from asyncframework_amd.cli import drivers
from asyncframework_amd.engine.config import EngineConfig
from asyncframework_amd.engine.local import RunResult
from asyncframework_amd.utils import logfmt

COUNTS = ("tp", "fp", "tn", "fn")


def _brute(Z, y, thr):
    """Count loop: Z [n, T] scores, thr [T, K]; a row is predicted positive
    iff z > thr. Returns dict of [T, K] lists and (n_pos, n_neg)."""
    n, T = Z.shape
    K = thr.shape[1]
    out = {c: [[0] * K for _ in range(T)] for c in COUNTS}
    for t in range(T):
        for k in range(K):
            for i in range(n):
                pos, pred = y[i] > 0.5, Z[i, t] > thr[t, k]
                name = ("tp" if pos and pred else "fp" if pred
                        else "fn" if pos else "tn")
                out[name][t][k] += 1
    n_pos = int(sum(1 for i in range(n) if y[i] > 0.5))
    return out, n_pos, n - n_pos


def _check(cv, Z, y, thr):
    want, n_pos, n_neg = _brute(Z, y, thr)
    T = Z.shape[1]
    assert cv.z_thr.dtype == torch.float64
    assert cv.z_thr.tolist() == thr.tolist()
    for c in COUNTS:
        got = getattr(cv, c)
        assert got.dtype == torch.int64
        assert got.tolist() == want[c], c
    assert cv.n_pos.tolist() == [n_pos] * T
    assert cv.n_neg.tolist() == [n_neg] * T


@pytest.fixture(scope="module")
def int_case():
    """Integer data: the scores are small integers, so thresholds can sit
    exactly on scores (z > thr is false there)."""
    g = torch.Generator().manual_seed(3)
    n, d, T = 80, 6, 3
    X = torch.randint(-2, 3, (n, d), generator=g).float()
    W = torch.randint(-2, 3, (T, d), generator=g).float()
    y = (torch.rand(n, generator=g) > 0.4).float()
    Z = (X.double() @ W.double().t()).numpy()
    return X, y, W, Z


def _to_csr(X):
    sp = X.to_sparse_csr()
    return (sp.crow_indices().to(torch.int32),
            sp.col_indices().to(torch.int32), sp.values())


def _both(X, y, W, **kw):
    yield ops.evaluate_curve(X, y, W, "hinge", **kw)
    yield ops.evaluate_curve_csr(*_to_csr(X), y, W, "hinge", **kw)


def test_counts_with_ties_and_duplicates(int_case):
    X, y, W, Z = int_case
    # integers are hit exactly by many rows; 1.0 and -2.5 are duplicated
    z = [-6.0, -2.5, -2.5, -1.0, 0.0, 0.5, 1.0, 1.0, 1.0, 3.0, 40.0]
    assert any(float(v) in z for v in Z.ravel())
    thr = np.tile(np.array(z), (W.shape[0], 1))
    for cv in _both(X, y, W, z_thresholds=z):
        _check(cv, Z, y.numpy(), thr)
        # duplicate thresholds give identical columns
        assert torch.equal(cv.tp[:, 6], cv.tp[:, 8])


def test_per_iterate_thresholds(int_case):
    X, y, W, Z = int_case
    thr = np.array([[-3.0, 0.0, 2.0, 2.0], [-1.5, -1.0, 4.0, 9.0],
                    [0.0, 0.0, 0.0, 1.0]])
    for cv in _both(X, y, W, z_thresholds=torch.from_numpy(thr)):
        _check(cv, Z, y.numpy(), thr)


def test_user_thresholds_are_mapped_and_sorted(int_case):
    X, y, W, Z = int_case
    cv = ops.evaluate_curve(X, y, W, "logistic", thresholds=[0.68, 0.32, 0.5])
    z = sorted(math.log(p / (1 - p)) if p != 0.5 else 0.0
               for p in (0.68, 0.32, 0.5))
    assert cv.z_thr[0].tolist() == z
    _check(cv, Z, y.numpy(), np.tile(np.array(z), (3, 1)))
    cv = ops.evaluate_curve(X, y, W, "lsq", thresholds=[0.75, -0.75])
    assert cv.z_thr[1].tolist() == [-0.75, 0.75]


def test_column_equals_evaluate(int_case):
    X, y, W, _ = int_case
    cv = ops.evaluate_curve(X, y, W, "hinge", thresholds=[-1.0, 0.25])
    for k, thr in enumerate((-1.0, 0.25)):
        ev = ops.evaluate(X, y, W, "hinge", threshold=thr)
        for c in COUNTS:
            assert torch.equal(getattr(cv, c)[:, k], getattr(ev, c))


def test_nan_score_is_below_every_threshold():
    X = torch.tensor([[1.0], [float("nan")], [-1.0]])
    y = torch.tensor([1.0, 1.0, 0.0])
    W = torch.tensor([[1.0]])
    cv = ops.evaluate_curve(X, y, W, "hinge", z_thresholds=[-5.0, 0.0])
    assert cv.tp.tolist() == [[1, 1]] and cv.fn.tolist() == [[1, 1]]
    assert cv.fp.tolist() == [[1, 0]] and cv.tn.tolist() == [[0, 1]]


def test_validation_errors(int_case):
    X, y, W, _ = int_case
    bad = [
        {},                                                     # none
        dict(thresholds=[0.0], num_bins=3),                     # two
        dict(thresholds=[0.0], z_thresholds=[0.0]),
        dict(z_thresholds=[0.0], num_bins=3),
        dict(z_thresholds=[0.0, float("inf")]),                 # not finite
        dict(z_thresholds=[float("nan")]),
        dict(z_thresholds=[1.0, 0.5]),                          # decreasing
        dict(z_thresholds=[[0.0, 1.0], [1.0, 0.0], [0.0, 0.0]]),
        dict(z_thresholds=torch.zeros(4, 2)),                   # T mismatch
        dict(z_thresholds=torch.zeros(1, 3, 2)),                # 3-D
        dict(thresholds=[[0.0]]),                               # not [K]
        dict(thresholds=[float("nan")]),
        dict(num_bins=0),
        dict(num_bins=2.5),
    ]
    csr = _to_csr(X)
    for kw in bad:
        with pytest.raises(ValueError):
            ops.evaluate_curve(X, y, W, "hinge", **kw)
        with pytest.raises(ValueError):
            ops.evaluate_curve_csr(*csr, y, W, "hinge", **kw)
    with pytest.raises(ValueError):  # a probability outside (0, 1)
        ops.evaluate_curve(X, y, W, "logistic", thresholds=[0.5, 1.0])
    with pytest.raises(ValueError):
        ops.evaluate_curve(X, y, W, "huber", thresholds=[0.5])
    with pytest.raises(ValueError):
        ops.evaluate_curve(X, y, W[:, :-1], "hinge", thresholds=[0.5])


def test_empty_inputs(int_case):
    X, y, W, _ = int_case
    cv = ops.evaluate_curve(X, y, W, "hinge", z_thresholds=[])
    assert cv.tp.shape == (3, 0) and cv.n_pos.tolist() == [0, 0, 0]
    assert cv.auc_roc().tolist() == [0.5] * 3
    cv = ops.evaluate_curve(X[:0], y[:0], W, "hinge", thresholds=[0.0, 1.0])
    assert cv.tp.tolist() == [[0, 0]] * 3 and cv.z_thr.shape == (3, 2)
    cv = ops.evaluate_curve(X, y, W[:0], "hinge", num_bins=4)
    assert cv.tp.shape == (0, 4) and cv.n_neg.shape == (0,)
    cv = ops.evaluate_curve_csr(torch.zeros(1, dtype=torch.int32),
                                torch.zeros(0, dtype=torch.int32),
                                torch.zeros(0), torch.zeros(0), W, "hinge",
                                num_bins=2)
    assert cv.fp.tolist() == [[0, 0]] * 3


# ---------------------------------------------------------------- metrics

def _mllib(tp, fp, P, N, beta):
    """The definitions of the module docstring for ONE iterate, in plain
    Python; tp, fp by ASCENDING threshold as a CurveResult stores them."""
    prec = [1.0 if a + b == 0 else a / (a + b) for a, b in zip(tp, fp)]
    rec = [0.0 if P == 0 else a / P for a in tp]
    fpr = [0.0 if N == 0 else b / N for b in fp]
    b2 = beta * beta
    f = [0.0 if p + r == 0 else (1 + b2) * p * r / (b2 * p + r)
         for p, r in zip(prec, rec)]
    roc = [(0.0, 0.0)] + list(zip(fpr[::-1], rec[::-1])) + [(1.0, 1.0)]
    pr = [(0.0, prec[-1])] + list(zip(rec[::-1], prec[::-1]))
    area = lambda pts: sum((b[0] - a[0]) * (a[1] + b[1]) / 2.0
                           for a, b in zip(pts, pts[1:]))
    return prec, rec, fpr, f, roc, pr, area(roc), area(pr)


def _result(tp, fp, P, N):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    tp, fp, P, N = i64(tp), i64(fp), i64(P), i64(N)
    return ops.CurveResult(torch.zeros(tp.shape, dtype=torch.float64), tp,
                           fp, N[:, None] - fp, P[:, None] - tp, P, N)


@pytest.mark.parametrize("beta", [1.0, 0.5, 2.0])
def test_metrics_follow_mllib(beta):
    cases = [
        ([9, 7, 4, 0], [12, 5, 1, 0], 10, 15),   # ordinary; last: nothing
        ([0, 0, 0, 0], [6, 3, 3, 0], 0, 6),      # predicted; no positives
        ([5, 2, 2, 1], [0, 0, 0, 0], 5, 0),      # no negatives
        ([0, 0, 0, 0], [0, 0, 0, 0], 4, 4),      # nothing predicted at all
        ([0, 0, 0, 0], [3, 1, 0, 0], 2, 3),      # p + r == 0 with p == 0
    ]
    cv = _result([c[0] for c in cases], [c[1] for c in cases],
                 [c[2] for c in cases], [c[3] for c in cases])
    got = (cv.precision(), cv.recall(), cv.fpr(), cv.f_measure(beta))
    roc, pr = cv.roc(), cv.pr()
    for t, (tp, fp, P, N) in enumerate(cases):
        prec, rec, fpr, f, wroc, wpr, aroc, apr = _mllib(tp, fp, P, N, beta)
        for g, w in zip(got, (prec, rec, fpr, f)):
            assert g.dtype == torch.float64
            assert g[t].tolist() == pytest.approx(w, abs=1e-15)
        for got_pts, want_pts in ((roc, wroc), (pr, wpr)):
            for axis in (0, 1):
                assert got_pts[axis][t].tolist() == pytest.approx(
                    [p[axis] for p in want_pts], abs=1e-15)
        assert float(cv.auc_roc()[t]) == pytest.approx(aroc, abs=1e-15)
        assert float(cv.auc_pr()[t]) == pytest.approx(apr, abs=1e-15)
    assert cv.f_measure().tolist() == cv.f_measure(1.0).tolist()


def _mann_whitney(z, y):
    """Tie-aware P(z+ > z-) + P(z+ == z-) / 2 over all pairs."""
    pos, neg = z[y > 0.5], z[y <= 0.5]
    gt = (pos[:, None] > neg[None, :]).sum()
    eq = (pos[:, None] == neg[None, :]).sum()
    return (gt + 0.5 * eq) / (len(pos) * len(neg))


def test_auc_roc_is_mann_whitney_at_every_distinct_score(int_case):
    X, y, W, Z = int_case
    T = W.shape[0]
    distinct = [np.unique(Z[:, t]) for t in range(T)]
    assert any(len(u) < Z.shape[0] for u in distinct)  # there are ties
    K = max(len(u) for u in distinct)
    # pad a row by repeating its largest score: a repeated point
    thr = np.stack([np.concatenate([u, np.full(K - len(u), u[-1])])
                    for u in distinct])
    for cv in _both(X, y, W, z_thresholds=torch.from_numpy(thr)):
        for t in range(T):
            assert float(cv.auc_roc()[t]) == pytest.approx(
                _mann_whitney(Z[:, t], y.numpy()), abs=1e-12)


# ------------------------------------------------------- curve_thresholds

def test_curve_thresholds_picks_strided_order_statistics():
    """Row i scores exactly i (and -i for the second iterate), so the
    thresholds name the rows they came from: floor(i * n / S) for the 8192
    strided rows, at the levels (k + 1/2) / B."""
    n, B, S = 20000, 7, 8192
    X = torch.arange(n, dtype=torch.float32)[:, None]
    W = torch.tensor([[1.0], [-1.0]])
    thr = ops.curve_thresholds(X, W, B)
    assert thr.dtype == torch.float64 and thr.shape == (2, B)
    rows = [(i * n) // S for i in range(S)]
    pick = [min(int(math.floor((k + 0.5) * S / B)), S - 1) for k in range(B)]
    assert thr[0].tolist() == [float(rows[p]) for p in pick]
    assert thr[1].tolist() == [-float(rows[S - 1 - p]) for p in pick]
    assert torch.equal(thr, ops.curve_thresholds(X, W, B))
    csr = ops.curve_thresholds_csr(*_to_csr(X)[:3], W, B)
    assert torch.equal(csr, thr)
    # fewer rows than the sample: every row is in it
    few = ops.curve_thresholds(X[:5], W, 5)
    assert few[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


def test_curve_thresholds_real_data_and_num_bins(int_case):
    X, y, W, Z = int_case
    for thr in (ops.curve_thresholds(X, W, 9),
                ops.curve_thresholds_csr(*_to_csr(X), W, 9)):
        assert bool((thr[:, 1:] >= thr[:, :-1]).all())
        for t in range(W.shape[0]):  # integer scores: exact in fp32
            assert set(thr[t].tolist()) <= set(Z[:, t].tolist())
    for cv in _both(X, y, W, num_bins=9):
        assert torch.equal(cv.z_thr, ops.curve_thresholds(X, W, 9))
        _check(cv, Z, y.numpy(), cv.z_thr.numpy())
    with pytest.raises(ValueError):
        ops.curve_thresholds(X, W, 0)


# ---------------------------------------------------- run layer and CLI

_FLOAT = r"(?:-?[0-9.]+(?:e[+-]?\d+)?|inf|nan)"


def _capture(fn, *args, **kw):
    buf = io.StringIO()
    with redirect_stdout(buf):
        fn(*args, **kw)
    return buf.getvalue()


def _check_curve_block(block, bins, times):
    assert block[0] == f"Held-out curve bins: {bins}"
    assert block[-1] == "curve finished"
    rows = block[1:-1]
    assert [r.split(",")[0] for r in rows] == [str(t) for t in times]
    out = []
    for r in rows:
        assert re.fullmatch(rf"\d+(,{_FLOAT}){{4}}", r), r
        vals = r.split(",")[1:]
        assert all(repr(float(v)) == v for v in vals)
        out.append(tuple(map(float, vals)))
    return out


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("objective", ["hinge", "logistic"])
def test_evaluation_report_curve_block(int_case, objective, sparse):
    X, y, W, _ = int_case
    cfg = EngineConfig(d=X.shape[1], N=X.shape[0], num_workers=1,
                       num_iterations=1, gamma=0.1, objective=objective)
    res = RunResult(k=3, elapsed_ms=5, opt_vars=[(10 * t, W[t])
                                                 for t in range(3)],
                    waiting_time={}, w=W[-1])
    data = (*_to_csr(X), y) if sparse else (X, y)
    plain = _capture(run.evaluation_report, cfg, res, data, sparse)
    assert plain == _capture(run.evaluation_report, cfg, res, data, sparse,
                             curve_bins=0)
    assert plain.endswith("evaluation finished\n") and "curve" not in plain
    full = _capture(run.evaluation_report, cfg, res, data, sparse,
                    curve_bins=6)
    assert full.startswith(plain)  # the first block is byte-for-byte the same
    rows = _check_curve_block(full[len(plain):].splitlines(), 6, [0, 10, 20])
    ev = ops.evaluate_curve_csr if sparse else ops.evaluate_curve
    cv = ev(*data, W, objective, num_bins=6)
    f1 = cv.f_measure()
    for t, (auc_roc, auc_pr, best, thr) in enumerate(rows):
        assert auc_roc == float(cv.auc_roc()[t])
        assert auc_pr == float(cv.auc_pr()[t])
        assert best == float(f1[t].max())
        z = float(cv.z_thr[t, int(f1[t].argmax())])
        want = 1.0 / (1.0 + math.exp(-z)) if objective == "logistic" else z
        assert thr == pytest.approx(want, rel=1e-12)
    # no logged iterate: header and footer only
    res.opt_vars = []
    out = _capture(run.evaluation_report, cfg, res, data, sparse,
                   curve_bins=6).splitlines()
    assert out[-3:] == ["evaluation finished", "Held-out curve bins: 6",
                        "curve finished"]


def test_curve_lines_format():
    out = _capture(logfmt.curve_lines, 4, [(7, 0.5, 0.25, 1.0, -0.125)])
    assert out == ("Held-out curve bins: 4\n7,0.5,0.25,1.0,-0.125\n"
                   "curve finished\n")


ARGS13 = ["synthetic", "synthetic", "16", "200", "2", "30", "0.5", "1000000",
          "0.3", "0.5", "10", "0", "42"]


def test_cli_curve_bins_block():
    lines = _capture(drivers.asgd_sync, ARGS13 + [
        "--objective", "logistic", "--test-rows", "80", "--curve-bins",
        "8"]).splitlines()
    at = lines.index("evaluation finished")
    first = lines.index("Held-out rows: 80")
    times = [int(l.split(",")[0]) for l in lines[first + 1:at]]
    rows = _check_curve_block(lines[at + 1:], 8, times)
    # the planted model is shared: the last iterate ranks well, and its
    # best-F1 threshold is a probability
    assert rows[-1][0] > 0.8 and 0.0 < rows[-1][3] < 1.0


def test_cli_without_curve_bins_prints_no_curve_block():
    lines = _capture(drivers.asgd_sync, ARGS13 + [
        "--objective", "hinge", "--test-rows", "80"]).splitlines()
    assert lines[-1] == "evaluation finished"
    assert not any("curve" in l for l in lines)


@pytest.mark.parametrize("drv", [drivers.asgd_thread, drivers.asaga_thread,
                                 drivers.asaga_sync])
def test_every_13_arg_driver_takes_the_flag(drv):
    lines = _capture(drv, ARGS13 + ["--objective", "hinge", "--test-rows",
                                    "40", "--curve-bins", "3"]).splitlines()
    assert lines[-1] == "curve finished"


def test_sgd_mllib_takes_the_flag():
    lines = _capture(drivers.sgd_mllib, [
        "synthetic", "synthetic", "16", "200", "2", "30", "0.5", "0.3",
        "--objective", "hinge", "--sparse", "--test-rows", "40",
        "--curve-bins", "3"]).splitlines()
    assert lines[-1] == "curve finished"
