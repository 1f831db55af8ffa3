"""fp64 oracle of the gradient kernels (K1-K3) with a derived per-element
error bound. Plain vectorised numpy on the CPU: no loop over rows.

For a sampled row i with nnz_i stored entries v_ik in columns j_ik (dense
rows: nnz_i = d), labels y, weights w and SAGA history alpha (zeros for the
plain gradient), everything taken in fp64 from the exact (bf16-rounded)
data:

    z_i = sum_k v_ik w_jik            A_i = sum_k |v_ik||w_jik| + |y_i| + |alpha_i|
    e_i = link(z_i, y_i)              c_i = e_i - alpha_i
    g_j = sum_i c_i v_ij              S_j = sum_i |c_i||v_ij|
    m_j = number of contributions     D_j = sum_i |v_ij| (nnz_i + 3) A_i

(a column stored twice in a row contributes twice to g_j, S_j, m_j, D_j).

Bound, u = 2^-24 (fp32 unit roundoff), for lsq and for hinge after the kink
rule:

    |e_kernel[i] - e_i| <= 2u (nnz_i + 3) A_i
    |g_kernel[j] - g_j| <= 2u (D_j + (m_j + 1) S_j)

Derivation. An fp32 dot product of nnz terms, in any order, through any
shuffle tree, fused or not, errs by at most nnz u sum|v||w| to first order
(nnz product roundings and nnz - 1 additions, each relative to a partial sum
that sum|v||w| bounds). z - y and e - alpha add one rounding each, of a
value A_i bounds: |delta c_i| <= (nnz_i + 2) u A_i, inside (nnz_i + 3) u A_i.
That error reaches g_j scaled by |v_ij|: the D_j term. Each product c v
rounds once (u S_j in all), and m_j fp32 additions in any order - LDS slabs,
slab sums, atomics: a summation tree with m_j leaves whatever its shape -
add at most m_j u S_j. The factor 2 covers the second-order terms; it is
not a tuning knob. hinge's e is -1, 0 or +1, exact once the row is on the
same side of the step as in fp64, which the kink rule guarantees.

logistic has one more term, the error of the device's fast exp, that is not
derived here: logistic results are held to the project's relative-L2
tolerances against this fp64 reference instead (LOGISTIC_CSR_TOL,
logistic_dense_tol)."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
LOGISTIC_CSR_TOL = 1e-3


def logistic_dense_tol(bf16: bool) -> float:
    return 2e-2 if bf16 else 2e-4


def link64(z, y, objective):
    """asyncframework_amd.ops.torch_ref._link in fp64."""
    if objective == "lsq":
        return z - y
    if objective == "logistic":
        # stable at any |z|: never exponentiates a positive number
        ez = np.exp(-np.abs(z))
        return np.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez)) - y
    if objective == "hinge":
        s = 2.0 * y - 1.0
        return np.where(1.0 > s * z, -s, 0.0)
    raise ValueError(objective)


def kink_keep(z, absdot, nterms):
    """The project's hinge kink rule (tests/test_gpu_hinge.py::_kink_filter)
    on fp64 scores: keep a row iff its score is further from both steps
    (z = +1, z = -1) than the rigorous fp32 dot-product band
    (nterms + 2) 2^-23 sum|x||w|. Asserts the 10 % removal cap."""
    band = (np.asarray(nterms, dtype=np.float64) + 2.0) * 2.0 ** -23 * absdot
    keep = (np.abs(z - 1.0) > band) & (np.abs(z + 1.0) > band)
    n = keep.shape[0]
    removed = n - int(keep.sum())
    print(f"kink rule: removed {removed}/{n}")
    assert removed <= 0.10 * n, f"kink rule removed {removed}/{n}"
    return keep


def csr_scores(indptr, indices, values, w):
    """(z, sum|v||w|, nnz, row id of every stored entry), fp64."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.shape[0] - 1
    nnz = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), nnz)
    v = np.asarray(values, dtype=np.float64)
    wj = np.asarray(w, dtype=np.float64)[np.asarray(indices, dtype=np.int64)]
    z = np.bincount(rows, weights=v * wj, minlength=n)
    absdot = np.bincount(rows, weights=np.abs(v * wj), minlength=n)
    return z, absdot, nnz, rows


def _finish(o, mask):
    o.mask = np.asarray(mask, dtype=bool)
    o.idx = np.nonzero(o.mask)[0]
    o.cnt = int(o.mask.sum())
    o.e_bound = 2.0 * U * (o.nnz + 3.0) * o.A
    o.g_bound = 2.0 * U * (o.D + (o.m + 1.0) * o.S)
    return o


def csr_oracle(indptr, indices, values, y, w, mask, objective, alpha=None):
    """Oracle of grad_csr / saga_grad_csr. Arrays are numpy (values already
    rounded to the kernel's storage type). Per-row fields (z, A, e, c, nnz,
    e_bound) cover EVERY row, sampled or not; per-column fields (g, S, m, D,
    g_bound) sum the sampled rows only."""
    d = np.asarray(w).shape[0]
    indices = np.asarray(indices, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    z, absdot, nnz, rows = csr_scores(indptr, indices, v, w)
    a = np.zeros_like(y) if alpha is None else np.asarray(alpha, np.float64)
    o = SimpleNamespace(z=z, nnz=nnz.astype(np.float64), rows=rows)
    o.A = absdot + np.abs(y) + np.abs(a)
    o.e = link64(z, y, objective)
    o.c = o.e - a
    sel = np.asarray(mask, dtype=bool)[rows]
    cols, vs, rs = indices[sel], v[sel], rows[sel]
    o.g, o.S, o.m, o.D = (np.zeros(d) for _ in range(4))
    np.add.at(o.g, cols, o.c[rs] * vs)  # a duplicate column counts twice
    np.add.at(o.S, cols, np.abs(o.c[rs] * vs))
    np.add.at(o.m, cols, 1.0)
    np.add.at(o.D, cols, np.abs(vs) * ((o.nnz + 3.0) * o.A)[rs])
    return _finish(o, mask)


def dense_oracle(X, y, w, mask, objective, alpha=None):
    """Oracle of grad_dense / saga_grad_dense: every row holds d entries."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, d = X.shape
    mask = np.asarray(mask, dtype=bool)
    a = np.zeros_like(y) if alpha is None else np.asarray(alpha, np.float64)
    o = SimpleNamespace(z=X @ w, nnz=np.full(n, float(d)))
    o.A = np.abs(X) @ np.abs(w) + np.abs(y) + np.abs(a)
    o.e = link64(o.z, y, objective)
    o.c = o.e - a
    Xs, cs = X[mask], o.c[mask]
    o.g = Xs.T @ cs
    o.S = np.abs(Xs).T @ np.abs(cs)
    o.m = np.full(d, float(mask.sum()))
    o.D = np.abs(Xs).T @ ((d + 3.0) * o.A[mask])
    return _finish(o, mask)


def ratio(got, want, bound):
    """max |got - want| / bound. Where the bound is zero (no contribution,
    or nothing to round) the values must agree exactly: inf otherwise."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0),
                 np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def rel_l2(got, want):
    got = np.asarray(got, dtype=np.float64)
    return float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-12))


def check_g(o, g, label):
    """Prints max err/bound of a gradient against the oracle; returns it."""
    r = ratio(g, o.g, o.g_bound)
    print(f"{label} max g err/bound={r:.5f}")
    return r


def check_e(o, rows, e, label):
    """As check_g for the history scalars e of the given rows."""
    r = ratio(e, o.e[rows], o.e_bound[rows])
    print(f"{label} max e err/bound={r:.5f}")
    return r
