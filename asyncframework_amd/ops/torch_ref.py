"""Plain-PyTorch reference implementations of the compute hot path.

These are the numerics oracle for the HIP kernels (every HIP kernel's test
compares against these in fp32), the CPU execution path for the no-GPU test
tier, and the fallback is *never* silently used on a GPU box (see ops.__init__).

Semantics mirror the reference's JVM hot loops:

* per-sample least-squares gradient g_i = (x_i.w - y_i) x_i
  (reference examples/.../SparkASGDThread.scala:423-438 ``gradfun``),
* the logistic link variant g_i = (sigmoid(x_i.w) - y_i) x_i (the BASELINE
  north-star's hot path),
* SAGA history correction g_i - alpha_i x_i with scalar history alpha
  (reference SparkASAGAThread.scala:380-385),
* objective sweep sum((x.w - y)^2)/N (reference SparkASGDThread.scala:389-404).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch


OBJECTIVES = ("lsq", "logistic", "hinge")


def _link(z: torch.Tensor, y: torch.Tensor, objective: str) -> torch.Tensor:
    """Scalar gradient coefficient e from the score z = x.w and the label y
    (csrc/link.h): z - y for 'lsq', sigmoid(z) - y for 'logistic'; 'hinge'
    is MLlib's HingeGradient, labels in {0,1}, s = 2y - 1: e = -s when
    1 > s*z (strict), else 0."""
    y = y.float()
    if objective == "lsq":
        return z - y
    elif objective == "logistic":
        return torch.sigmoid(z) - y
    elif objective == "hinge":
        s = 2.0 * y - 1.0
        return torch.where(1.0 > s * z, -s, torch.zeros_like(s))
    raise ValueError(f"unknown objective {objective!r}")


def _row_loss(Z: torch.Tensor, y: torch.Tensor, objective: str
              ) -> torch.Tensor:
    """Loss of every (row, iterate) score Z[i, t], in Z's dtype: (z - y)^2,
    softplus(-s z) or max(0, 1 - s z), with s = 2y - 1."""
    y = y.to(Z.dtype)[:, None]
    if objective == "lsq":
        return (Z - y) ** 2
    zy = Z * (2.0 * y - 1.0)
    if objective == "logistic":
        return torch.nn.functional.softplus(-zy)
    elif objective == "hinge":
        return torch.clamp(1.0 - zy, min=0.0)
    raise ValueError(f"unknown objective {objective!r}")


def _residual(X: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
              objective: str) -> torch.Tensor:
    """Per-row scalar gradient coefficient e_i = _link(x_i.w, y_i)."""
    z = (X.to(w.dtype) @ w).float()
    return _link(z, y, objective)


def grad_dense(X: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
               mask: torch.Tensor, objective: str = "lsq") -> Tuple[torch.Tensor, int]:
    """Summed minibatch gradient over the masked rows: g = X_S^T e_S.

    Returns (g fp32 [d], n_sampled). Mirrors gradfun + the per-partition axpy
    fold (reference RDD.scala:1103-1123 reducePartition, comOp = axpy)."""
    idx = mask.nonzero(as_tuple=True)[0]
    n = int(idx.numel())
    if n == 0:
        return torch.zeros(X.shape[1], dtype=torch.float32, device=X.device), 0
    Xs = X[idx]
    e = _residual(Xs, y[idx], w, objective)
    g = (Xs.float().t() @ e)
    return g, n


def grad_csr(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
             y: torch.Tensor, w: torch.Tensor, mask: torch.Tensor,
             objective: str = "lsq") -> Tuple[torch.Tensor, int]:
    """CSR variant of grad_dense (reference sparse dot/axpy,
    mllib/.../linalg/BLAS.scala:74-90,134-160). g accumulated dense fp32."""
    d = w.shape[0]
    g = torch.zeros(d, dtype=torch.float32, device=w.device)
    idx = mask.nonzero(as_tuple=True)[0]
    n = int(idx.numel())
    wf = w.float()
    for i in idx.tolist():
        s, t = int(indptr[i]), int(indptr[i + 1])
        cols = indices[s:t].long()
        vals = values[s:t].float()
        z = torch.dot(vals, wf[cols])
        e = _link(z, y[i], objective)
        g.index_add_(0, cols, e * vals)
    return g, n


def saga_grad_dense(X: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
                    alpha: torch.Tensor, mask: torch.Tensor,
                    objective: str = "lsq"
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """SAGA corrected gradient over masked rows.

    Per sampled row i: e_i = link(x_i.w) - y_i; contribution (e_i - a_i) x_i
    (reference SparkASAGAThread.scala:380-385: ``g_i - alpha_i*x_i`` with the
    rank-1 reconstruction alpha_i*x_i of the historical gradient).

    Returns (g fp32 [d], sampled_idx int64 [n] — *shard-local* row indices,
    e fp32 [n] — the new history scalars, n). The caller commits
    ``alpha[sampled_idx] = e`` only when the server accepts the round
    (reference merges ScalarMap only inside the tau test,
    SparkASAGAThread.scala:191,206-208)."""
    idx = mask.nonzero(as_tuple=True)[0]
    n = int(idx.numel())
    d = X.shape[1]
    if n == 0:
        z = torch.zeros(d, dtype=torch.float32, device=X.device)
        return z, idx, torch.zeros(0, dtype=torch.float32, device=X.device), 0
    Xs = X[idx]
    e = _residual(Xs, y[idx], w, objective)
    corr = e - alpha[idx].float()
    g = Xs.float().t() @ corr
    return g, idx, e, n


def saga_grad_csr(indptr: torch.Tensor, indices: torch.Tensor,
                  values: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
                  alpha: torch.Tensor, mask: torch.Tensor,
                  objective: str = "lsq"
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """CSR SAGA gradient; see saga_grad_dense."""
    d = w.shape[0]
    g = torch.zeros(d, dtype=torch.float32, device=w.device)
    idx = mask.nonzero(as_tuple=True)[0]
    n = int(idx.numel())
    e_out = torch.zeros(n, dtype=torch.float32, device=w.device)
    wf = w.float()
    for j, i in enumerate(idx.tolist()):
        s, t = int(indptr[i]), int(indptr[i + 1])
        cols = indices[s:t].long()
        vals = values[s:t].float()
        z = torch.dot(vals, wf[cols])
        e = _link(z, y[i], objective)
        e_out[j] = e
        g.index_add_(0, cols, (e - alpha[i].float()) * vals)
    return g, idx, e_out, n


def objective_sweep(X: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
                    objective: str = "lsq", batch_rows: int = 262144,
                    l2: float = 0.0, l1: float = 0.0) -> torch.Tensor:
    """Objective of each of T logged iterates in one dataset pass.

    W is [T, d] (stacked iterates — the reference computes all logged
    objectives in a single job, SparkASGDThread.scala:389-398). Returns [T]
    fp64. lsq: sum((X w_t - y)^2)/N; logistic: mean log-loss; hinge: mean
    max(0, 1 - s z). Non-zero
    l2/l1 add ``penalty(W, objective, l2, l1)``."""
    T = W.shape[0]
    N = X.shape[0]
    out = torch.zeros(T, dtype=torch.float64, device=X.device)
    # bf16 X: cast the SMALL operand (W, [T,d]) once and run a bf16 MFMA
    # GEMM instead of converting every X chunk up to fp32 (the conversion
    # kernel costs as much as the GEMM itself — profiles/r02 MFMA capture)
    Wt = W.to(X.device, X.dtype if X.dtype == torch.bfloat16 else W.dtype)
    for s in range(0, N, batch_rows):
        Xb = X[s:s + batch_rows]
        yb = y[s:s + batch_rows].float()
        Z = (Xb @ Wt.t()).float()  # [B, T] — library GEMM (MFMA on gfx950)
        out += _row_loss(Z, yb, objective).double().sum(dim=0)
    out = out / N
    if l2 != 0.0 or l1 != 0.0:
        out = out + penalty(W, objective, l2, l1).to(out.device)
    return out


def objective_sweep_csr(indptr: torch.Tensor, indices: torch.Tensor,
                        values: torch.Tensor, y: torch.Tensor,
                        W: torch.Tensor, objective: str = "lsq",
                        N_total: Optional[int] = None, l2: float = 0.0,
                        l1: float = 0.0) -> torch.Tensor:
    """CSR objective sweep via torch.sparse mm."""
    n_rows = indptr.shape[0] - 1
    N = N_total if N_total is not None else n_rows
    sp = torch.sparse_csr_tensor(indptr, indices, values.float(),
                                 size=(n_rows, W.shape[1]))
    Z = torch.sparse.mm(sp, W.float().t())
    yb = y.float()
    out = _row_loss(Z, yb, objective).double().sum(dim=0)
    out = out / N
    if l2 != 0.0 or l1 != 0.0:
        out = out + penalty(W, objective, l2, l1).to(out.device)
    return out


def _confusion(Z: torch.Tensor, y: torch.Tensor, z_thr: float):
    """tp, fp, tn, fn per column of Z: actual positive iff y > 0.5,
    predicted positive iff z > z_thr."""
    pos = (y > 0.5)[:, None]
    pred = Z > z_thr
    return ((pos & pred).sum(dim=0), (~pos & pred).sum(dim=0),
            (~pos & ~pred).sum(dim=0), (pos & ~pred).sum(dim=0))


def evaluate(X: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
             objective: str, z_thr: float, batch_rows: int = 65536):
    """Reference of the fused evaluation kernels, in fp64 throughout:
    (loss_sum fp64 [T], tp, fp, tn, fn int64 [T]) of the stacked iterates
    W [T, d] over the rows of X. The row loss is _row_loss; the decision
    is _confusion at the score threshold z_thr."""
    T = W.shape[0]
    loss = torch.zeros(T, dtype=torch.float64, device=X.device)
    cnt = [torch.zeros(T, dtype=torch.int64, device=X.device)
           for _ in range(4)]
    Wd = W.to(X.device).double()
    for s in range(0, X.shape[0], batch_rows):
        yb = y[s:s + batch_rows].double()
        Z = X[s:s + batch_rows].double() @ Wd.t()
        loss += _row_loss(Z, yb, objective).sum(dim=0)
        for c, part in zip(cnt, _confusion(Z, yb, z_thr)):
            c += part
    return (loss, *cnt)


def evaluate_csr(indptr: torch.Tensor, indices: torch.Tensor,
                 values: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
                 objective: str, z_thr: float):
    """CSR form of evaluate (fp64 sparse product)."""
    n_rows = indptr.shape[0] - 1
    sp = torch.sparse_csr_tensor(indptr, indices, values.double(),
                                 size=(n_rows, W.shape[1]))
    Z = torch.sparse.mm(sp, W.to(values.device).double().t())
    yb = y.double()
    loss = _row_loss(Z, yb, objective).sum(dim=0)
    return (loss, *_confusion(Z, yb, z_thr))


def _curve_counts(Z: torch.Tensor, y: torch.Tensor, z_thr: torch.Tensor):
    """Confusion counts of the fp64 scores Z [n, T] at the thresholds
    z_thr [T, K] (rows non-decreasing): (tp, fp, tn, fn) int64 [T, K] and
    (n_pos, n_neg) int64 [T]. Predicted positive iff z > thr, so a score
    exactly on a threshold is below it; a NaN score is below every one."""
    T, K = z_thr.shape
    pos = y > 0.5
    # b = #{k : z > thr[k]} = #{k : thr[k] < z}
    b = torch.searchsorted(z_thr, Z.t().contiguous(), right=False)  # [T, n]
    b = torch.where(torch.isnan(Z.t()), torch.zeros_like(b), b)
    out = []
    for mask in (pos, ~pos):
        hist = torch.zeros(T, K + 1, dtype=torch.int64, device=Z.device)
        hist.scatter_add_(1, b[:, mask],
                          torch.ones_like(b[:, mask], dtype=torch.int64))
        # rows with b >= k + 1 are above threshold k
        above = hist.flip(1).cumsum(1).flip(1)[:, 1:]
        out.append((above, int(mask.sum()) - above))
    (tp, fn), (fp, tn) = out
    full = lambda v: torch.full((T,), int(v), dtype=torch.int64,
                                device=Z.device)
    return tp, fp, tn, fn, full(pos.sum()), full((~pos).sum())


def evaluate_curve(X: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
                   z_thr: torch.Tensor, batch_rows: int = 65536):
    """Reference of the threshold-sweep kernels, fp64 throughout: the
    counts of _curve_counts for the stacked iterates W [T, d] over the rows
    of X at the score thresholds z_thr [T, K]."""
    Wd = W.to(X.device).double()
    thr = z_thr.to(X.device).double().contiguous()
    total = None
    for s in range(0, X.shape[0], batch_rows):
        part = _curve_counts(X[s:s + batch_rows].double() @ Wd.t(),
                             y[s:s + batch_rows].double(), thr)
        total = part if total is None else tuple(
            a + b for a, b in zip(total, part))
    return total


def evaluate_curve_csr(indptr: torch.Tensor, indices: torch.Tensor,
                       values: torch.Tensor, y: torch.Tensor,
                       W: torch.Tensor, z_thr: torch.Tensor):
    """CSR form of evaluate_curve (fp64 sparse product)."""
    n_rows = indptr.shape[0] - 1
    sp = torch.sparse_csr_tensor(indptr, indices, values.double(),
                                 size=(n_rows, W.shape[1]))
    Z = torch.sparse.mm(sp, W.to(values.device).double().t())
    return _curve_counts(Z, y.double(),
                         z_thr.to(values.device).double().contiguous())


def _const_m2(m2: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor
              ) -> torch.Tensor:
    """M2 with exact zeros where the column holds one value: a two-pass mean
    is sum / n, which need not reproduce that value to the last bit."""
    return torch.where(mn == mx, torch.zeros_like(m2), m2)


def col_stats(X: torch.Tensor):
    """fp64 two-pass column statistics of X [n, d], n > 0 (MLlib
    Statistics.colStats): (mean, m2 = sum (x - mean)^2, num_nonzeros int64,
    min, max, norm_l1 = sum |x|, sumsq = sum x^2), each [d]."""
    Xd = X.double()
    mean = Xd.sum(0) / X.shape[0]
    mn, mx = Xd.min(0).values, Xd.max(0).values
    m2 = _const_m2(((Xd - mean) ** 2).sum(0), mn, mx)
    return (mean, m2, (Xd != 0).sum(0), mn, mx, Xd.abs().sum(0),
            (Xd * Xd).sum(0))


def col_stats_csr(indptr: torch.Tensor, indices: torch.Tensor,
                  values: torch.Tensor, d: int):
    """CSR form of col_stats with MultivariateOnlineSummarizer semantics:
    stored zeros are skipped and the implicit zeros count towards n, mean,
    m2, min and max. Two passes of index_add_ over the non-zeros; nothing is
    densified."""
    n = indptr.shape[0] - 1
    lo, hi = int(indptr[0]), int(indptr[n])
    v = values[lo:hi].double()
    j = indices[lo:hi].long()
    keep = v != 0
    v, j = v[keep], j[keep]
    z = lambda: torch.zeros(d, dtype=torch.float64, device=values.device)
    nnz = torch.zeros(d, dtype=torch.int64, device=values.device)
    nnz.index_add_(0, j, torch.ones_like(j))
    mean = z().index_add_(0, j, v) / n
    within = z().index_add_(0, j, (v - mean[j]) ** 2)
    m2 = within + (n - nnz).double() * mean * mean
    inf = torch.full((d,), float("inf"), dtype=torch.float64,
                     device=values.device)
    mn = inf.clone().scatter_reduce_(0, j, v, "amin")
    mx = (-inf).scatter_reduce_(0, j, v, "amax")
    zeros = nnz < n  # an implicit zero takes part in min and max
    mn = torch.where(zeros, mn.clamp(max=0.0), mn)
    mx = torch.where(zeros, mx.clamp(min=0.0), mx)
    return (mean, _const_m2(m2, mn, mx), nnz, mn, mx,
            z().index_add_(0, j, v.abs()), z().index_add_(0, j, v * v))


def scale_(X: torch.Tensor, mean: torch.Tensor, factor: torch.Tensor,
           with_mean: bool) -> None:
    """X <- (X - mean) * factor in fp32 (a subtraction and a multiplication,
    each rounded), then rounded to X's type, in place; without ``with_mean``
    X * factor."""
    Xf = X.float()
    if with_mean:
        Xf = Xf - mean.float()
    X.copy_((Xf * factor.float()).to(X.dtype))


def scale_csr_(indices: torch.Tensor, values: torch.Tensor,
               factor: torch.Tensor) -> None:
    """values <- values * factor[indices] in fp32, rounded to the values'
    type, in place."""
    values.copy_((values.float() * factor.float()[indices.long()])
                 .to(values.dtype))


def penalty(W: torch.Tensor, objective: str, l2: float,
            l1: float) -> torch.Tensor:
    """Elastic-net term of the REPORTED objective, per stacked iterate, fp64:
    c*((l2/2)*||w_t||^2 + l1*||w_t||_1). c = 2 for lsq (the sweep's lsq value
    is sum((x.w-y)^2)/N, twice the (1/2)(.)^2 loss whose gradient the kernels
    use), 1 for logistic and hinge — so the reported number is a constant
    multiple of the minimised F."""
    c = 2.0 if objective == "lsq" else 1.0
    Wd = W.double()
    return c * (0.5 * float(l2) * (Wd * Wd).sum(dim=1)
                + float(l1) * Wd.abs().sum(dim=1))


def _reg_step(w: torch.Tensor, ghat: torch.Tensor, eta: float, l2: float,
              l1: float) -> None:
    """One regularised step, in place:
    v = w - eta*(ghat + l2*w); w = soft_threshold(v, eta*l1), clipped
    elements exactly +0.0."""
    v = w - eta * (ghat + l2 * w)
    t = eta * l1
    w.copy_(torch.where(v > t, v - t,
                        torch.where(v < -t, v + t, torch.zeros_like(v))))


def sgd_update(w: torch.Tensor, g: torch.Tensor, gamma_k: float,
               inv_batch: float, *, l2: float = 0.0, l1: float = 0.0) -> None:
    """Fused scale+axpy weight update, in place:
    w -= gamma_k * (g * inv_batch). Reference updater thread
    SparkASGDThread.scala:188-192 (scalOp + axpyOp). With l2/l1 non-zero the
    step is the decay + soft-threshold of _reg_step (eta = gamma_k,
    ghat = inv_batch*g)."""
    if l2 != 0.0 or l1 != 0.0:
        _reg_step(w, inv_batch * g.to(w.dtype), gamma_k, l2, l1)
        return
    w.add_(g.to(w.dtype), alpha=-(gamma_k * inv_batch))


def saga_update(w: torch.Tensor, g: torch.Tensor, alpha_bar: torch.Tensor,
                gamma: float, inv_batch: float, inv_N: float, *,
                l2: float = 0.0, l1: float = 0.0) -> None:
    """Fused SAGA triple-axpy, in place (reference
    SparkASAGAThread.scala:217-220):
    w -= gamma * (g*inv_batch); w -= gamma*alpha_bar; alpha_bar += g*inv_N.
    With l2/l1 non-zero this is prox-SAGA: eta = gamma,
    ghat = inv_batch*g + alpha_bar_old; the penalty stays out of alpha_bar."""
    gf = g.float()
    if l2 != 0.0 or l1 != 0.0:
        _reg_step(w, inv_batch * gf.to(w.dtype) + alpha_bar.to(w.dtype),
                  gamma, l2, l1)
        alpha_bar.add_(gf, alpha=inv_N)
        return
    w.add_(gf.to(w.dtype), alpha=-(gamma * inv_batch))
    w.add_(alpha_bar.to(w.dtype), alpha=-gamma)
    alpha_bar.add_(gf, alpha=inv_N)
