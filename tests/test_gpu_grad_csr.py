"""The CSR gradient kernels (K2/K3, grad_csr_body) and the generic dense
fallback (grad_dense_kernel) against the fp64 oracle of tests/grad_oracle.py,
on MI355X: every element of g and every history scalar inside the derived
bound (lsq, hinge after the kink rule; logistic by the project's relative-L2
tolerances), counts and sampled ids exact.

The case generator and the case lists at the top are plain CPU code; the
CPU tier (tests/test_grad_oracle_ref.py) runs the fp32 reference and its
mutations over the same lists."""

import functools
from typing import NamedTuple, Optional

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_oracle as go
from asyncframework_amd import ops
from asyncframework_amd.utils.philox import bernoulli_mask

F32, BF16 = torch.float32, torch.bfloat16
_OBJ = {"lsq": 0, "logistic": 1, "hinge": 2}


# ------------------------------------------------------------------- cases

class Shape(NamedTuple):
    name: str
    n: int
    d: int
    rate: float
    row_start: int
    grid: Optional[int]  # ASYNCAMD_GRAD_GRID, None = the launcher's own


# n below one Philox block / one wave of rows / one block iteration and just
# past them; one block walking three grid-stride iterations with a partial
# last group (waves 2 and 3 start past n_rows); a non-zero high counter
# word; w too large for LDS (47,236 columns: it lives in L2).
CSR_SHAPES = [
    Shape("n1", 1, 97, 0.5, 0, None),
    Shape("n3", 3, 97, 0.5, 0, None),
    Shape("n255", 255, 97, 0.5, 0, None),
    Shape("n257", 257, 97, 0.5, 1000, None),
    Shape("n1027", 1027, 97, 0.5, 4096, None),
    Shape("grid1-half", 2500, 97, 0.5, 0, 1),
    Shape("grid1-all", 2500, 97, 1.0, 0, 1),
    Shape("c1", 300, 97, 0.5, 2 ** 34, None),
    Shape("wide", 600, 47236, 0.5, 0, None),
]

# (saga, objective, LPR, values dtype): the full LPR x dtype cross for lsq
# SAGA, LPR 8 and 32 for the rest
CSR_COMBOS = (
    [(True, "lsq", lpr, dt) for lpr in (8, 16, 32, 64) for dt in (F32, BF16)]
    + [(sg, obj, lpr, dt)
       for sg, obj in ((False, "lsq"), (False, "hinge"), (True, "hinge"),
                       (False, "logistic"), (True, "logistic"))
       for lpr in (8, 32) for dt in (F32, BF16)])


def _dt(dt):
    return "bf16" if dt == BF16 else "f32"


def _combo_id(c):
    return f"{'saga' if c[0] else 'plain'}-{c[1]}-lpr{c[2]}-{_dt(c[3])}"


def _round_to(a, dtype):
    """fp32 array rounded to the kernel's storage type: (torch tensor in
    that type, its exact values as fp64 numpy)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)
    return t, t.double().numpy()


def _labels(rng, m, objective):
    if objective == "lsq":
        return rng.standard_normal(m).astype(np.float32)
    return (rng.random(m) > 0.5).astype(np.float32)  # {0, 1}


def _rows_with_duplicates(indptr, indices, d):
    """Ids of the rows that store some column more than once."""
    nnz = np.diff(indptr)
    rows = np.repeat(np.arange(nnz.shape[0], dtype=np.int64), nnz)
    key = np.sort(rows * d + indices.astype(np.int64))
    return np.unique(key[1:][key[1:] == key[:-1]] // d)


def _draw_csr(shape, lpr, dtype, objective, trial):
    """One draw of the generator: row lengths per row from {0, 1, LPR-1, LPR,
    LPR+1, 200}, columns WITH replacement and unsorted (duplicates inside
    rows; at d = 97 rows collide heavily), values, w and alpha ~ N(0, 1).
    hinge draws spare rows, drops the ones the kink rule rejects (fp64
    scores straight from the CSR arrays) and keeps the first n."""
    rng = np.random.default_rng([shape.n, shape.d, lpr, trial])
    n, d = shape.n, shape.d
    m = n + max(8, n // 8) if objective == "hinge" else n
    lens = np.array([0, 1, lpr - 1, lpr, lpr + 1, 200])[
        rng.integers(0, 6, size=m)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, d, size=int(indptr[-1])).astype(np.int32)
    values_t, values = _round_to(rng.standard_normal(indices.shape[0]), dtype)
    y = _labels(rng, m, objective)
    w = rng.standard_normal(d).astype(np.float32)
    removed = 0
    if objective == "hinge":
        z, absdot, nnz, rows = go.csr_scores(indptr, indices, values, w)
        keep = go.kink_keep(z, absdot, nnz)
        removed = m - int(keep.sum())
        keep &= np.cumsum(keep) <= n  # the first n kept rows
        assert int(keep.sum()) == n
        sel = keep[rows]
        lens, y = lens[keep], y[keep]
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        indices, values = indices[sel], values[sel]
        values_t = values_t[torch.from_numpy(sel)]
    alpha = rng.standard_normal(n).astype(np.float32)
    seed, round_k = 1000 + trial, 1 + trial
    mask = bernoulli_mask(seed, round_k, shape.row_start, n, shape.rate)
    return dict(shape=shape, lpr=lpr, dtype=dtype, objective=objective,
                indptr=indptr.astype(np.int32), indices=indices,
                values=values, values_t=values_t.contiguous(), y=y, w=w,
                alpha=alpha, mask=mask, seed=seed, round_k=round_k,
                drawn=m, removed=removed)


@functools.lru_cache(maxsize=None)
def csr_case(shape, lpr, dtype, objective):
    """The first draw whose mask samples what the case is for: a row that
    stores a column twice (two lanes of one atomic instruction on one
    address) and, from n = 255 up, an empty row as well. n = 1 may sample
    nothing at a given key, so the key is part of the draw."""
    for trial in range(512):
        c = _draw_csr(shape, lpr, dtype, objective, trial)
        nnz = np.diff(c["indptr"])
        dup = np.zeros(shape.n, dtype=bool)
        dup[_rows_with_duplicates(c["indptr"], c["indices"], shape.d)] = True
        if not (c["mask"] & dup).any():
            continue
        if shape.n >= 255 and not (c["mask"] & (nnz == 0)).any():
            continue
        assert c["mask"].any()
        c["dup_rows"] = dup
        return SimpleCase(**c)
    raise AssertionError(f"no usable draw for {shape.name}")


class SimpleCase:
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._oracles = {}

    def oracle(self, saga):
        """Cached fp64 oracle (shared by the tests; never modified)."""
        if saga not in self._oracles:
            self._oracles[saga] = go.csr_oracle(
                self.indptr, self.indices, self.values, self.y, self.w,
                self.mask, self.objective, self.alpha if saga else None)
        return self._oracles[saga]


class DenseShape(NamedTuple):
    name: str
    n: int
    d: int
    lpr: int           # ASYNCAMD_LPR
    no_pipe: bool      # ASYNCAMD_NO_PIPE=1


# the generic kernel's sub-wave widths at a d with a scalar tail (123: one
# vector pass at most, 787: several), the aligned vector rows the pipe
# normally takes (784), and d just past the pipe's limit / past 64 KiB of
# dynamic LDS (20 d bytes at LPR 64)
DENSE_SHAPES = (
    [DenseShape(f"d{d}-lpr{lpr}", 1027, d, lpr, False)
     for lpr in (16, 32, 64) for d in (123, 787)]
    + [DenseShape("d784-nopipe", 1027, 784, 64, True)])
DENSE_BIG_SHAPES = [DenseShape("d2052", 64, 2052, 64, False),
                    DenseShape("d4100", 64, 4100, 64, False)]
DENSE_RATE, DENSE_ROW_START = 0.5, 2000


@functools.lru_cache(maxsize=None)
def dense_case(shape, dtype, objective):
    rng = np.random.default_rng([shape.n, shape.d, 7])
    n, d = shape.n, shape.d
    m = n + max(8, n // 8) if objective == "hinge" else n
    X_t, X = _round_to(rng.standard_normal((m, d)) / np.sqrt(d), dtype)
    y = _labels(rng, m, objective)
    w = rng.standard_normal(d).astype(np.float32)
    removed = 0
    if objective == "hinge":
        wd = w.astype(np.float64)
        keep = go.kink_keep(X @ wd, np.abs(X) @ np.abs(wd), d)
        removed = m - int(keep.sum())
        keep &= np.cumsum(keep) <= n
        X, y, X_t = X[keep], y[keep], X_t[torch.from_numpy(keep)]
    alpha = rng.standard_normal(n).astype(np.float32)
    seed, round_k = 77, 3
    mask = bernoulli_mask(seed, round_k, DENSE_ROW_START, n, DENSE_RATE)
    assert mask.any() and not mask.all()
    return SimpleDense(shape=shape, dtype=dtype, objective=objective, X=X,
                       X_t=X_t.contiguous(), y=y, w=w, alpha=alpha,
                       mask=mask, seed=seed, round_k=round_k, drawn=m,
                       removed=removed)


class SimpleDense(SimpleCase):
    def oracle(self, saga):
        if saga not in self._oracles:
            self._oracles[saga] = go.dense_oracle(
                self.X, self.y, self.w, self.mask, self.objective,
                self.alpha if saga else None)
        return self._oracles[saga]


# --------------------------------------------------------------- GPU side

def _core():
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    import asyncframework_amd._hip_core as core
    return core


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SENT_IDX = -7        # staging sentinels: a slot the kernel never wrote
_SENT_E = 12345.0


class _Run(NamedTuple):
    g: np.ndarray
    n_ctr: int
    pos: int
    idx: np.ndarray    # whole staging buffer
    e: np.ndarray
    alpha: np.ndarray  # after the launch


def _launch(case, saga, commit_now=0):
    """Direct launch through the raw bindings (both counters, the staging
    buffers and alpha are visible). Buffers hold n entries: a launch stages
    at most one entry per row."""
    core = _core()
    n = case.mask.shape[0]
    d = case.w.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    y, w = _cuda(case.y), _cuda(case.w)
    alpha = _cuda(case.alpha)
    g = torch.zeros(d, device="cuda")
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")  # [n, pos]
    idx = torch.full((n,), _SENT_IDX, dtype=torch.int32, device="cuda")
    e = torch.full((n,), _SENT_E, device="cuda")
    bf16 = 1 if case.dtype == BF16 else 0
    obj = _OBJ[case.objective]
    rs = case.shape.row_start if isinstance(case.shape, Shape) \
        else DENSE_ROW_START
    rate = case.shape.rate if isinstance(case.shape, Shape) else DENSE_RATE
    if isinstance(case.shape, Shape):
        ip, ix, vv = _cuda(case.indptr), _cuda(case.indices), \
            case.values_t.cuda()
        if saga:
            core.saga_grad_csr(ip.data_ptr(), ix.data_ptr(), vv.data_ptr(),
                               y.data_ptr(), w.data_ptr(), alpha.data_ptr(),
                               g.data_ptr(), ctr.data_ptr(), idx.data_ptr(),
                               e.data_ptr(), ctr.data_ptr() + 4, 0,
                               commit_now, n, case.seed, case.round_k, rs,
                               rate, obj, bf16, st)
        else:
            core.grad_csr(ip.data_ptr(), ix.data_ptr(), vv.data_ptr(),
                          y.data_ptr(), w.data_ptr(), g.data_ptr(),
                          ctr.data_ptr(), 0, n, case.seed, case.round_k, rs,
                          rate, obj, bf16, st)
    else:
        X = case.X_t.cuda()
        if saga:
            core.saga_grad_dense(X.data_ptr(), y.data_ptr(), w.data_ptr(),
                                 alpha.data_ptr(), g.data_ptr(), 0,
                                 ctr.data_ptr(), idx.data_ptr(),
                                 e.data_ptr(), ctr.data_ptr() + 4, 0,
                                 commit_now, n, d, case.seed, case.round_k,
                                 rs, rate, obj, bf16, st)
        else:
            core.grad_dense(X.data_ptr(), y.data_ptr(), w.data_ptr(),
                            g.data_ptr(), 0, ctr.data_ptr(), 0, n, d,
                            case.seed, case.round_k, rs, rate, obj, bf16, st)
    torch.cuda.synchronize()
    c = ctr.cpu().numpy()
    return _Run(g.cpu().numpy(), int(c[0]), int(c[1]), idx.cpu().numpy(),
                e.cpu().numpy(), alpha.cpu().numpy())


def _check_against_oracle(case, saga, run, label, logistic_tol):
    """Counts and ids exact; g (and the staged e) inside the bound, or for
    logistic inside the project's tolerance on the fp64 reference."""
    o = case.oracle(saga)
    assert run.n_ctr == o.cnt
    bounded = case.objective != "logistic"
    if saga:
        assert run.pos == o.cnt
        order = np.argsort(run.idx[:run.pos], kind="stable")
        assert np.array_equal(run.idx[:run.pos][order], o.idx)  # no dups
        assert (run.idx[run.pos:] == _SENT_IDX).all()
        assert (run.e[run.pos:] == np.float32(_SENT_E)).all()
        e = run.e[:run.pos][order]
        assert np.isfinite(e).all()
        if bounded:
            assert go.check_e(o, o.idx, e, label) <= 1.0
        else:
            assert np.allclose(e, o.e[o.idx], atol=1e-3, rtol=1e-3)
        assert np.array_equal(run.alpha, case.alpha)  # staged: not committed
    else:
        assert run.pos == 0
    if bounded:
        assert go.check_g(o, run.g, label) <= 1.0
    else:
        rel = go.rel_l2(run.g, o.g)
        print(f"{label} rel={rel:.3e}")
        assert rel < logistic_tol, rel


@pytest.mark.parametrize("shape", CSR_SHAPES, ids=lambda s: s.name)
@pytest.mark.parametrize("combo", CSR_COMBOS, ids=_combo_id)
def test_csr_matches_fp64_oracle(combo, shape, monkeypatch):
    saga, objective, lpr, dtype = combo
    core = _core()
    monkeypatch.setenv("ASYNCAMD_CSR_LPR", str(lpr))
    if shape.grid is not None:
        monkeypatch.setenv("ASYNCAMD_GRAD_GRID", str(shape.grid))
        assert core.grad_grid(shape.n) == shape.grid
    assert core.csr_kernel_info()["lpr"] == lpr
    case = csr_case(shape, lpr, dtype, objective)
    run = _launch(case, saga)
    _check_against_oracle(case, saga, run,
                          f"csr {_combo_id(combo)} {shape.name}",
                          go.LOGISTIC_CSR_TOL)


@pytest.mark.parametrize("lpr", [8, 16, 32, 64])
@pytest.mark.parametrize("objective", ["lsq", "hinge"])
def test_csr_commit_now_writes_alpha_in_place(objective, lpr, monkeypatch):
    """commit_now = 1 (the graph engine's form): alpha[sampled] = e inside
    the e bound, every other alpha bit-unchanged, staging and pos untouched,
    g as staged."""
    core = _core()
    monkeypatch.setenv("ASYNCAMD_CSR_LPR", str(lpr))
    assert core.csr_kernel_info()["lpr"] == lpr
    case = csr_case(CSR_SHAPES[4], lpr, F32, objective)
    o = case.oracle(True)
    run = _launch(case, True, commit_now=1)
    label = f"csr commit {objective} lpr{lpr}"
    assert run.n_ctr == o.cnt
    assert run.pos == 0
    assert (run.idx == _SENT_IDX).all() and (run.e == np.float32(_SENT_E)).all()
    assert np.array_equal(run.alpha[~o.mask].view(np.int32),
                          case.alpha[~o.mask].view(np.int32))
    assert go.check_e(o, o.idx, run.alpha[o.mask], label) <= 1.0
    assert go.check_g(o, run.g, label) <= 1.0


@pytest.mark.parametrize("d,kernel", [(260, "grad_dense_pipe_kernel"),
                                      (123, "grad_dense_kernel")])
def test_dense_commit_now_writes_alpha_in_place(d, kernel):
    core = _core()
    assert core.dense_kernel_info(d, 0, 1, 0)["kernel"] == kernel
    case = dense_case(DenseShape(f"d{d}", 1027, d, 64, False), F32, "lsq")
    o = case.oracle(True)
    run = _launch(case, True, commit_now=1)
    label = f"dense commit d={d}"
    assert run.n_ctr == o.cnt
    assert run.pos == 0
    assert (run.idx == _SENT_IDX).all() and (run.e == np.float32(_SENT_E)).all()
    assert np.array_equal(run.alpha[~o.mask].view(np.int32),
                          case.alpha[~o.mask].view(np.int32))
    assert go.check_e(o, o.idx, run.alpha[o.mask], label) <= 1.0
    assert go.check_g(o, run.g, label) <= 1.0


@pytest.mark.parametrize("scale", [1e2, 1e4])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_csr_logistic_saturates_cleanly(dtype, scale, monkeypatch):
    """Scores beyond +-100 and +-1e4 (w scaled up): sigmoid is 0 or 1 to
    fp32, so the staged e is finite and equals -y or 1 - y within 2^-23."""
    core = _core()
    monkeypatch.setenv("ASYNCAMD_CSR_LPR", "32")
    assert core.csr_kernel_info()["lpr"] == 32
    base = csr_case(CSR_SHAPES[4], 32, dtype, "logistic")
    case = SimpleCase(**{k: v for k, v in base.__dict__.items()
                         if k != "_oracles"})
    case.w = (base.w * np.float32(scale)).astype(np.float32)
    o = case.oracle(True)
    hi = o.mask & (o.z > scale)
    lo = o.mask & (o.z < -scale)
    assert hi.sum() >= 8 and lo.sum() >= 8, (hi.sum(), lo.sum())
    run = _launch(case, True)
    assert run.n_ctr == run.pos == o.cnt
    assert np.isfinite(run.e[:run.pos]).all()
    assert np.isfinite(run.g).all()
    got = np.full(o.mask.shape[0], np.nan)
    got[run.idx[:run.pos]] = run.e[:run.pos]
    yv = case.y.astype(np.float64)
    err_hi = np.abs(got[hi] - (1.0 - yv[hi])).max()
    err_lo = np.abs(got[lo] - (-yv[lo])).max()
    print(f"saturation scale={scale:g} {_dt(dtype)} rows hi/lo="
          f"{int(hi.sum())}/{int(lo.sum())} max err hi={err_hi:.3g} "
          f"lo={err_lo:.3g}")
    assert err_hi <= 2.0 ** -23 and err_lo <= 2.0 ** -23


# ------------------------------------------------- generic dense fallback

def _dense_env(shape, saga, dtype, monkeypatch):
    core = _core()
    monkeypatch.setenv("ASYNCAMD_LPR", str(shape.lpr))
    if shape.no_pipe:
        monkeypatch.setenv("ASYNCAMD_NO_PIPE", "1")
    info = core.dense_kernel_info(shape.d, 1 if dtype == BF16 else 0,
                                  1 if saga else 0, 0)
    assert info["kernel"] == "grad_dense_kernel", info
    assert info["lpr"] == shape.lpr, info
    assert info["dynamic_lds_bytes"] == \
        (1 + 4 * 64 // shape.lpr) * shape.d * 4, info
    return info


@pytest.mark.parametrize("saga", [False, True], ids=["plain", "saga"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: s.name)
def test_dense_fallback_matches_fp64_oracle(shape, dtype, saga, monkeypatch):
    _dense_env(shape, saga, dtype, monkeypatch)
    case = dense_case(shape, dtype, "lsq")
    run = _launch(case, saga)
    _check_against_oracle(
        case, saga, run,
        f"fallback {shape.name} {_dt(dtype)} {'saga' if saga else 'plain'}",
        None)


@pytest.mark.parametrize("objective", ["hinge", "logistic"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("lpr", [16, 32])
def test_dense_fallback_subwaves_other_links(lpr, dtype, objective,
                                             monkeypatch):
    """The sub-wave widths that tests/test_gpu_hinge.py (LPR 64 only) does
    not reach, SAGA with non-zero alpha."""
    shape = DenseShape(f"d123-lpr{lpr}", 1027, 123, lpr, False)
    _dense_env(shape, True, dtype, monkeypatch)
    case = dense_case(shape, dtype, objective)
    run = _launch(case, True)
    _check_against_oracle(case, True, run,
                          f"fallback {shape.name} {_dt(dtype)} {objective}",
                          go.logistic_dense_tol(dtype == BF16))


@pytest.mark.parametrize("saga", [False, True], ids=["plain", "saga"])
@pytest.mark.parametrize("shape", DENSE_BIG_SHAPES, ids=lambda s: s.name)
def test_dense_fallback_past_the_pipe_limit(shape, saga, monkeypatch):
    """d = 2052: the first d the pipelined kernel does not take. d = 4100:
    82,000 bytes of dynamic LDS, past 64 KiB."""
    info = _dense_env(shape, saga, F32, monkeypatch)
    assert (info["dynamic_lds_bytes"] > 65536) == (shape.d == 4100)
    case = dense_case(shape, F32, "lsq")
    run = _launch(case, saga)
    _check_against_oracle(
        case, saga, run,
        f"fallback {shape.name} {'saga' if saga else 'plain'}", None)


# ------------------------------------------------------- wrapper guards

def test_csr_wrappers_reject_unaligned_row_start():
    """The kernels take a row's Philox block as (row_start + i) / 4, so an
    unaligned start would silently sample other rows than
    utils.philox.bernoulli_mask. Rejected before any launch, as the dense
    wrappers do."""
    _core()
    case = csr_case(CSR_SHAPES[2], 32, F32, "lsq")
    ip, ix, vv = _cuda(case.indptr), _cuda(case.indices), case.values_t.cuda()
    y, w, alpha = _cuda(case.y), _cuda(case.w), _cuda(case.alpha)
    kw = dict(seed=1, round_k=1, row_start=502, rate=0.5)
    with pytest.raises(AssertionError, match="4-aligned"):
        ops.grad_csr(ip, ix, vv, y, w, **kw)
    with pytest.raises(AssertionError, match="4-aligned"):
        ops.saga_grad_csr(ip, ix, vv, y, w, alpha, **kw)
    n = case.mask.shape[0]
    rows = torch.full((n,), _SENT_IDX, dtype=torch.int32, device="cuda")
    ylist = torch.zeros(n, device="cuda")
    cnt = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError, match="4-aligned"):
        ops.spill_refresh(alpha, torch.zeros(n).pin_memory(), y, rows, ylist,
                          cnt, n, **kw)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 5 and bool((rows == _SENT_IDX).all())


@pytest.mark.parametrize("saga", [False, True], ids=["plain", "saga"])
def test_dense_wrappers_reject_lds_past_one_cu(saga):
    """d = 8196 at LPR 64 needs 20 d = 163,920 bytes of LDS, 80 past one
    CU's 163,840: the wrapper raises before any launch."""
    core = _core()
    d = 8196
    info = core.dense_kernel_info(d, 0, int(saga), 0)
    assert info["kernel"] == "grad_dense_kernel" and info["lpr"] == 64
    assert info["dynamic_lds_bytes"] == 20 * d > 163840
    X = torch.zeros(4, d, device="cuda")
    y = torch.zeros(4, device="cuda")
    w = torch.zeros(d, device="cuda")
    kw = dict(seed=1, round_k=1, row_start=0, rate=1.0)
    with pytest.raises(ValueError, match=r"d=8196.*163840"):
        if saga:
            ops.saga_grad_dense(X, y, w, torch.ones(4, device="cuda"), **kw)
        else:
            ops.grad_dense(X, y, w, **kw)


def test_unrecognised_override_runs_the_default(monkeypatch):
    """What the per-test asserts guard against: a value the launchers do
    not know selects the default instantiation without a word."""
    core = _core()
    monkeypatch.setenv("ASYNCAMD_CSR_LPR", "12")
    assert core.csr_kernel_info()["lpr"] == 32
    monkeypatch.setenv("ASYNCAMD_LPR", "8")
    assert core.dense_kernel_info(123, 0, 0, 0)["lpr"] == 64
