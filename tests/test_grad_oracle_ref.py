"""CPU tests of the fp64 gradient oracle (tests/grad_oracle.py) over the
case lists of tests/test_gpu_grad_csr.py:

(a) the project's fp32 reference (ops.torch_ref) stays inside the oracle's
    bound on every case - the bound is not too tight;
(b) mutations of that reference - the kernel bugs the GPU tests exist for -
    leave the bound on at least one element - it is not too loose either;
(c) the hinge kink rule removes at most 10 % of the rows it is shown.

Also here, because it needs no device: the checks the HIP wrappers make
before a launch."""

import numpy as np
import pytest
import torch

import grad_oracle as go
from test_gpu_grad_csr import (BF16, CSR_COMBOS, CSR_SHAPES, DENSE_BIG_SHAPES,
                               DENSE_RATE, DENSE_ROW_START, DENSE_SHAPES, F32,
                               DenseShape, _combo_id, _dt, csr_case,
                               dense_case)
from asyncframework_amd.ops import torch_ref
from asyncframework_amd.utils.philox import bernoulli_mask

_t = torch.from_numpy


def _ref_csr(case, saga, mask=None, alpha=None):
    """(g, idx, e) of the fp32 reference; idx/e None for the plain form."""
    mask = _t(case.mask if mask is None else mask)
    args = (_t(case.indptr), _t(case.indices), case.values_t, _t(case.y),
            _t(case.w))
    if not saga:
        g, n = torch_ref.grad_csr(*args, mask, case.objective)
        return g.numpy(), None, None, n
    alpha = _t(case.alpha if alpha is None else alpha)
    g, idx, e, n = torch_ref.saga_grad_csr(*args, alpha, mask, case.objective)
    return g.numpy(), idx.numpy(), e.numpy(), n


def _ref_dense(case, saga, mask=None, alpha=None):
    mask = _t(case.mask if mask is None else mask)
    if not saga:
        g, n = torch_ref.grad_dense(case.X_t, _t(case.y), _t(case.w), mask,
                                    case.objective)
        return g.numpy(), None, None, n
    alpha = _t(case.alpha if alpha is None else alpha)
    g, idx, e, n = torch_ref.saga_grad_dense(case.X_t, _t(case.y), _t(case.w),
                                             alpha, mask, case.objective)
    return g.numpy(), idx.numpy(), e.numpy(), n


def _check_ref(case, saga, ref, label, logistic_tol):
    o = case.oracle(saga)
    g, idx, e, n = ref
    assert n == o.cnt
    if saga:
        assert np.array_equal(idx, o.idx)
    if case.objective == "logistic":
        rel = go.rel_l2(g, o.g)
        print(f"{label} rel={rel:.3e}")
        assert rel < logistic_tol
        return
    if saga:
        assert go.check_e(o, o.idx, e, label) <= 1.0
    assert go.check_g(o, g, label) <= 1.0


# ---------------------------------------------------------------- (a) + (c)

def test_case_lists_are_what_the_gpu_tests_claim():
    assert [s.n for s in CSR_SHAPES] == [1, 3, 255, 257, 1027, 2500, 2500,
                                         300, 600]
    assert {(s.n, s.rate, s.grid) for s in CSR_SHAPES if s.grid} == {
        (2500, 0.5, 1), (2500, 1.0, 1)}
    assert all(s.d == 97 for s in CSR_SHAPES if s.name != "wide")
    assert all(s.row_start % 4 == 0 for s in CSR_SHAPES)
    assert len(CSR_COMBOS) == 28
    full = {(c[2], c[3]) for c in CSR_COMBOS if c[0] and c[1] == "lsq"}
    assert full == {(l, t) for l in (8, 16, 32, 64) for t in (F32, BF16)}


@pytest.mark.parametrize("shape", CSR_SHAPES, ids=lambda s: s.name)
@pytest.mark.parametrize("combo", CSR_COMBOS, ids=_combo_id)
def test_fp32_reference_csr_is_inside_the_bound(combo, shape):
    saga, objective, lpr, dtype = combo
    case = csr_case(shape, lpr, dtype, objective)
    # what the generator promises, checked here on the CPU
    nnz = np.diff(case.indptr)
    assert case.mask.shape == (shape.n,) and case.mask.any()
    assert (case.mask & case.dup_rows).any()
    assert set(np.unique(nnz)) <= {0, 1, lpr - 1, lpr, lpr + 1, 200}
    if shape.n >= 255:
        assert (case.mask & (nnz == 0)).any()
        assert {0, 1, lpr - 1, lpr, lpr + 1, 200} == set(nnz[case.mask])
    assert np.array_equal(
        case.mask, bernoulli_mask(case.seed, case.round_k, shape.row_start,
                                  shape.n, shape.rate))
    assert (case.alpha != 0).all()
    if objective == "hinge":  # (c)
        assert case.removed <= 0.10 * case.drawn
        e = case.oracle(saga).e[case.mask]
        if shape.n >= 255:  # rows on both sides of the step
            assert 0 < int((e != 0).sum()) < e.shape[0]
    _check_ref(case, saga, _ref_csr(case, saga),
               f"ref csr {_combo_id(combo)} {shape.name}",
               go.LOGISTIC_CSR_TOL)


@pytest.mark.parametrize("saga", [False, True], ids=["plain", "saga"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("shape", DENSE_SHAPES + DENSE_BIG_SHAPES
                         + [DenseShape("d260", 1027, 260, 64, False)],
                         ids=lambda s: s.name)
def test_fp32_reference_dense_is_inside_the_bound(shape, dtype, saga):
    case = dense_case(shape, dtype, "lsq")
    assert np.array_equal(
        case.mask, bernoulli_mask(case.seed, case.round_k, DENSE_ROW_START,
                                  shape.n, DENSE_RATE))
    _check_ref(case, saga, _ref_dense(case, saga),
               f"ref dense {shape.name} {_dt(dtype)}", None)


@pytest.mark.parametrize("objective", ["hinge", "logistic"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_fp32_reference_dense_other_links(dtype, objective):
    case = dense_case(DenseShape("d123-lpr16", 1027, 123, 16, False), dtype,
                      objective)
    if objective == "hinge":  # (c)
        assert case.removed <= 0.10 * case.drawn
        e = case.oracle(True).e[case.mask]
        assert 0 < int((e != 0).sum()) < e.shape[0]
    _check_ref(case, True, _ref_dense(case, True),
               f"ref dense d123 {_dt(dtype)} {objective}",
               go.logistic_dense_tol(dtype == BF16))


# ------------------------------------------- wrapper guards (no GPU needed)

def test_wrapper_guards_and_launch_queries_on_the_host(monkeypatch):
    """The checks ops/hip.py makes before a launch, and the host-only queries
    behind them, need no device: the fallback's LDS need and limit, the
    override fall-backs, the 4-aligned row start."""
    pytest.importorskip("asyncframework_amd._hip_core")
    from asyncframework_amd.ops import hip
    core = hip._hip_core
    for v in ("ASYNCAMD_LPR", "ASYNCAMD_CSR_LPR", "ASYNCAMD_NO_PIPE"):
        monkeypatch.delenv(v, raising=False)
    assert core.dense_launch_form(784) == (True, 64, 0)
    assert core.dense_launch_form(787) == (False, 64, 20 * 787)
    assert core.dense_launch_form(4100) == (False, 64, 82000)
    assert core.csr_kernel_info()["lpr"] == 32
    hip._chk_dense_lds(8192)  # 163,840 bytes: the last d that fits
    with pytest.raises(ValueError, match=r"d=8196.*163840"):
        hip._chk_dense_lds(8196)
    monkeypatch.setenv("ASYNCAMD_LPR", "16")
    assert core.dense_launch_form(787) == (False, 16, 68 * 787)
    hip._chk_dense_lds(2409)  # 68 * 2409 = 163,812
    with pytest.raises(ValueError, match=r"d=2410.*16 lanes"):
        hip._chk_dense_lds(2410)
    monkeypatch.setenv("ASYNCAMD_LPR", "8")  # unknown: the default
    assert core.dense_launch_form(787)[1] == 64
    monkeypatch.setenv("ASYNCAMD_NO_PIPE", "1")
    assert core.dense_launch_form(784) == (False, 64, 20 * 784)
    for lpr, want in (("8", 8), ("16", 16), ("64", 64), ("12", 32)):
        monkeypatch.setenv("ASYNCAMD_CSR_LPR", lpr)
        assert core.csr_kernel_info()["lpr"] == want
    hip._chk_row_start(2 ** 34)
    with pytest.raises(AssertionError, match="4-aligned"):
        hip._chk_row_start(502)


# ---------------------------------------------------------------------- (b)

def _entry_scores(o, cols, vals):
    """Per stored entry: its contribution |c v| over the bound of the column
    it lands in (inf where nothing else lands there)."""
    contrib = np.abs(o.c[o.rows] * vals)
    b = o.g_bound[cols]
    return np.where(b > 0, contrib / np.where(b > 0, b, 1.0), np.inf)


def _row_contrib32(case, o, i):
    """Row i's fp32 contribution to g, as the reference would add it."""
    s, t = int(case.indptr[i]), int(case.indptr[i + 1])
    c32 = np.float32(o.c[i])
    out = np.zeros(case.w.shape[0], dtype=np.float32)
    np.add.at(out, case.indices[s:t],
              c32 * case.values[s:t].astype(np.float32))
    return out


def _outside(o, g):
    return go.ratio(g, o.g, o.g_bound) > 1.0


MUT_COMBOS = [("lsq", 32, F32), ("lsq", 8, BF16), ("hinge", 32, F32),
              ("hinge", 8, BF16)]
assert all((True, o, l, t) in CSR_COMBOS for o, l, t in MUT_COMBOS)


@pytest.mark.parametrize("shape", CSR_SHAPES, ids=lambda s: s.name)
@pytest.mark.parametrize("objective,lpr,dtype", MUT_COMBOS,
                         ids=lambda v: _dt(v) if isinstance(v, torch.dtype)
                         else str(v))
def test_mutations_of_the_csr_reference_leave_the_bound(objective, lpr,
                                                        dtype, shape):
    """Each mutated row is the one whose largest entry stands highest above
    its column's bound: with few rows every non-empty row is visible, in the
    2,500-row cases at d = 97 (about a thousand contributions per column)
    only the longer ones are - the printed share."""
    case = csr_case(shape, lpr, dtype, objective)
    o = case.oracle(True)
    n = shape.n
    g_ref, idx, e, cnt = _ref_csr(case, True)
    assert not _outside(o, g_ref)
    score = _entry_scores(o, case.indices, case.values)
    row_score = np.zeros(n)
    np.maximum.at(row_score, o.rows, score)
    nonempty = np.diff(case.indptr) > 0
    seen = o.mask & nonempty
    print(f"{shape.name}: a dropped row is visible for "
          f"{int((row_score[seen] > 1).sum())}/{int(seen.sum())} rows")

    # drop one sampled row / count it twice
    i = int(np.argmax(np.where(o.mask, row_score, -1.0)))
    assert o.mask[i] and row_score[i] > 1
    assert _outside(o, g_ref - _row_contrib32(case, o, i)), "dropped row"
    assert _outside(o, g_ref + _row_contrib32(case, o, i)), "row twice"

    # ignore alpha / take the next row's (the last row: a value of its own)
    assert _outside(o, _ref_csr(case, True, alpha=np.zeros_like(case.alpha))[0])
    shifted = np.concatenate([case.alpha[1:], [np.float32(0.625)]])
    assert (shifted[o.mask] != case.alpha[o.mask]).all()
    assert _outside(o, _ref_csr(case, True, alpha=shifted)[0])

    # flip one mask bit at a 4-row block edge
    pos4 = (shape.row_start + np.arange(n)) % 4
    edge = ((pos4 == 0) | (pos4 == 3)) & nonempty
    j = int(np.argmax(np.where(edge, row_score, -1.0)))
    assert edge[j] and row_score[j] > 1
    flipped = case.mask.copy()
    flipped[j] = not flipped[j]
    g_flip, _, _, cnt_flip = _ref_csr(case, True, mask=flipped)
    assert cnt_flip != cnt
    assert _outside(o, g_flip), "flipped mask bit"

    # a column stored twice in a sampled row, added once
    order = np.argsort(o.rows * shape.d + case.indices, kind="stable")
    key = (o.rows * shape.d + case.indices)[order]
    second = np.zeros(key.shape[0], dtype=bool)
    second[order[1:][key[1:] == key[:-1]]] = True  # a repeat of a column
    second &= o.mask[o.rows]
    assert second.any()
    p = int(np.argmax(np.where(second, score, -1.0)))
    assert score[p] > 1
    g_once = g_ref.copy()
    g_once[case.indices[p]] -= (np.float32(o.c[o.rows[p]])
                                * np.float32(case.values[p]))
    assert _outside(o, g_once), "duplicate column once"


@pytest.mark.parametrize("shape", [DENSE_SHAPES[1], DENSE_BIG_SHAPES[1]],
                         ids=lambda s: s.name)
def test_mutations_of_the_dense_reference_leave_the_bound(shape):
    case = dense_case(shape, F32, "lsq")
    o = case.oracle(True)
    n = shape.n
    g_ref = _ref_dense(case, True)[0]
    assert not _outside(o, g_ref)
    score = (np.abs(o.c[:, None] * case.X) / o.g_bound[None, :]).max(axis=1)
    c32 = o.c.astype(np.float32)[:, None] * case.X.astype(np.float32)
    i = int(np.argmax(np.where(o.mask, score, -1.0)))
    print(f"{shape.name}: a dropped row is visible for "
          f"{int((score[o.mask] > 1).sum())}/{o.cnt} rows")
    assert score[i] > 1
    assert _outside(o, g_ref - c32[i]), "dropped row"
    assert _outside(o, g_ref + c32[i]), "row twice"
    assert _outside(o, _ref_dense(case, True,
                                  alpha=np.zeros_like(case.alpha))[0])
    shifted = np.concatenate([case.alpha[1:], [np.float32(0.625)]])
    assert _outside(o, _ref_dense(case, True, alpha=shifted)[0])
    pos4 = (DENSE_ROW_START + np.arange(n)) % 4
    edge = (pos4 == 0) | (pos4 == 3)
    j = int(np.argmax(np.where(edge, score, -1.0)))
    assert score[j] > 1
    flipped = case.mask.copy()
    flipped[j] = not flipped[j]
    assert _outside(o, _ref_dense(case, True, mask=flipped)[0])
