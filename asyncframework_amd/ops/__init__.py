"""Op dispatch: hand-written HIP/CDNA4 kernels on GPU, plain torch on CPU.

On a GPU box the HIP extension (``asyncframework_amd._hip``, built in-tree by
``setup.py build_ext --inplace`` for gfx950) is REQUIRED: ops on CUDA tensors
raise if it is missing, so a silent eager fallback can never masquerade as
the native path. The torch reference path (ops.torch_ref) serves CPU tensors
and the numerics tests. Set ASYNCAMD_ALLOW_FALLBACK=1 to explicitly permit
torch fallback on GPU (debug only)."""

from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import torch_ref
from ..utils.philox import bernoulli_mask

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from . import hip as mod  # adapter over the in-tree _hip_core .so
        _hip = mod
    except ImportError as e:  # pragma: no cover - exercised on GPU box only
        _hip_err = str(e)
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _require_hip(op: str):
    mod = _load_hip()
    if mod is None:
        if os.environ.get("ASYNCAMD_ALLOW_FALLBACK") == "1":
            return None
        raise RuntimeError(
            f"{op}: HIP extension asyncframework_amd._hip_core is not built "
            f"(import error: {_hip_err}). On a GPU box the native kernels are "
            f"mandatory — run `python setup.py build_ext --inplace` "
            f"(PYTORCH_ROCM_ARCH=gfx950). Set ASYNCAMD_ALLOW_FALLBACK=1 only "
            f"for debugging.")
    return mod


_OBJ_CODE = {"lsq": 0, "logistic": 1, "hinge": 2}  # csrc/link.h


def make_mask(device: torch.device, seed: int, round_k: int, row_start: int,
              n_rows: int, rate: float) -> torch.Tensor:
    """Philox Bernoulli mask as a bool tensor (CPU path; GPU kernels compute
    the identical mask in-kernel from the same counters — csrc/philox.h)."""
    m = bernoulli_mask(seed, round_k, row_start, n_rows, rate)
    return torch.from_numpy(m).to(device)


def grad_dense(X: torch.Tensor, y: torch.Tensor, w: torch.Tensor, *,
               seed: int, round_k: int, row_start: int, rate: float,
               objective: str = "lsq",
               out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, int]:
    """Fused sample-mask + minibatch gradient (kernel K1 of SURVEY §2.5)."""
    if X.is_cuda:
        mod = _require_hip("grad_dense")
        if mod is not None:
            if out is None:
                out = torch.zeros(X.shape[1], dtype=torch.float32, device=X.device)
            else:
                out.zero_()
            n = mod.grad_dense(X, y, w, out, int(seed), int(round_k),
                               int(row_start), float(rate),
                               _OBJ_CODE[objective])
            return out, n
    mask = make_mask(X.device, seed, round_k, row_start, X.shape[0], rate)
    g, n = torch_ref.grad_dense(X, y, w, mask, objective)
    if out is not None:
        out.copy_(g)
        return out, n
    return g, n


def grad_csr(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
             y: torch.Tensor, w: torch.Tensor, *, seed: int, round_k: int,
             row_start: int, rate: float, objective: str = "lsq",
             out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, int]:
    """Fused sample-mask + CSR minibatch gradient (kernel K2)."""
    if w.is_cuda:
        mod = _require_hip("grad_csr")
        if mod is not None:
            if out is None:
                out = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
            else:
                out.zero_()
            n = mod.grad_csr(indptr, indices, values, y, w, out, int(seed),
                             int(round_k), int(row_start), float(rate),
                             _OBJ_CODE[objective])
            return out, n
    n_rows = indptr.shape[0] - 1
    mask = make_mask(w.device, seed, round_k, row_start, n_rows, rate)
    g, n = torch_ref.grad_csr(indptr, indices, values, y, w, mask, objective)
    if out is not None:
        out.copy_(g)
        return out, n
    return g, n


def saga_grad_dense(X: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
                    alpha: torch.Tensor, *, seed: int, round_k: int,
                    row_start: int, rate: float, objective: str = "lsq"
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """Fused mask + SAGA history gather + corrected gradient (kernel K3).
    Returns (g, sampled_idx, e_new, n); history commit is separate
    (saga_commit) so rejected rounds can be discarded."""
    if X.is_cuda:
        mod = _require_hip("saga_grad_dense")
        if mod is not None:
            g = torch.zeros(X.shape[1], dtype=torch.float32, device=X.device)
            idx, e = mod.saga_grad_dense(X, y, w, alpha, g, int(seed),
                                         int(round_k), int(row_start),
                                         float(rate), _OBJ_CODE[objective])
            return g, idx, e, int(idx.numel())
    mask = make_mask(X.device, seed, round_k, row_start, X.shape[0], rate)
    return torch_ref.saga_grad_dense(X, y, w, alpha, mask, objective)


def saga_grad_csr(indptr: torch.Tensor, indices: torch.Tensor,
                  values: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
                  alpha: torch.Tensor, *, seed: int, round_k: int,
                  row_start: int, rate: float, objective: str = "lsq"
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    if w.is_cuda:
        mod = _require_hip("saga_grad_csr")
        if mod is not None:
            g = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
            idx, e = mod.saga_grad_csr(indptr, indices, values, y, w, alpha,
                                       g, int(seed), int(round_k),
                                       int(row_start), float(rate),
                                       _OBJ_CODE[objective])
            return g, idx, e, int(idx.numel())
    n_rows = indptr.shape[0] - 1
    mask = make_mask(w.device, seed, round_k, row_start, n_rows, rate)
    return torch_ref.saga_grad_csr(indptr, indices, values, y, w, alpha, mask,
                                   objective)


def saga_commit(alpha: torch.Tensor, idx: torch.Tensor, e: torch.Tensor) -> None:
    """Commit new history scalars alpha[idx] = e (the accepted-round analog of
    the reference's ScalarMap merge, SparkASAGAThread.scala:206-208)."""
    if alpha.is_cuda:
        mod = _require_hip("saga_commit")
        if mod is not None:
            mod.saga_commit(alpha, idx, e)
            return
    alpha[idx] = e.to(alpha.dtype)


def saga_commit_pinned(alpha_pinned: torch.Tensor, idx: torch.Tensor,
                       e: torch.Tensor) -> None:
    """Spill-path commit: kernel scatter into the pinned-host master table
    (GPU-only; the CPU engines keep their tables device/host-resident)."""
    mod = _require_hip("saga_commit_pinned")
    if mod is not None:
        mod.saga_commit_pinned(alpha_pinned, idx, e)
        return
    alpha_pinned[idx.cpu().long()] = e.cpu().to(alpha_pinned.dtype)


def spill_refresh(alpha_dev, alpha_pinned, y, rowlist, ylist, cnt, cap, *,
                  seed, round_k, row_start, rate) -> None:
    """Spill-path staging refresh (scan mask + gather sampled entries)."""
    mod = _require_hip("spill_refresh")
    if mod is not None:
        mod.spill_refresh(alpha_dev, alpha_pinned, y, rowlist, ylist, cnt,
                          cap, seed=seed, round_k=round_k,
                          row_start=row_start, rate=rate)
        return
    alpha_dev.copy_(alpha_pinned, non_blocking=True)  # debug fallback


def sgd_update(w: torch.Tensor, g: torch.Tensor, gamma_k: float,
               inv_batch: float, *, l2: float = 0.0, l1: float = 0.0) -> None:
    """Fused weight update (kernel K5). Non-zero l2/l1: weight decay and
    soft-threshold in the same kernel (docs/KERNELS.md, Updates)."""
    if w.is_cuda:
        mod = _require_hip("sgd_update")
        if mod is not None:
            mod.sgd_update(w, g, float(gamma_k), float(inv_batch),
                           float(l2), float(l1))
            return
    torch_ref.sgd_update(w, g, gamma_k, inv_batch, l2=l2, l1=l1)


def saga_update(w: torch.Tensor, g: torch.Tensor, alpha_bar: torch.Tensor,
                gamma: float, inv_batch: float, inv_N: float, *,
                l2: float = 0.0, l1: float = 0.0) -> None:
    """Fused SAGA triple-axpy update (kernel K6). Non-zero l2/l1: prox-SAGA
    step in the same kernel; the penalty never enters alpha_bar."""
    if w.is_cuda:
        mod = _require_hip("saga_update")
        if mod is not None:
            mod.saga_update(w, g, alpha_bar, float(gamma), float(inv_batch),
                            float(inv_N), float(l2), float(l1))
            return
    torch_ref.saga_update(w, g, alpha_bar, gamma, inv_batch, inv_N, l2=l2,
                          l1=l1)


def objective_sweep(X: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
                    objective: str = "lsq", *, l2: float = 0.0,
                    l1: float = 0.0) -> torch.Tensor:
    """Objective of stacked iterates (K7). GEMM-shaped: goes through the
    library GEMM (hipBLASLt via torch.matmul) on GPU — a plain GEMM is
    library territory, only the fused hot ops are hand-written."""
    return torch_ref.objective_sweep(X, y, W, objective, l2=l2, l1=l1)


def objective_sweep_csr(indptr, indices, values, y, W, objective="lsq",
                        N_total=None, *, l2: float = 0.0,
                        l1: float = 0.0) -> torch.Tensor:
    return torch_ref.objective_sweep_csr(indptr, indices, values, y, W,
                                         objective, N_total, l2=l2, l1=l1)


class EvalResult(NamedTuple):
    """Held-out score of T stacked iterates: ``loss`` fp64 [T] (loss_sum / N,
    the normalisation of objective_sweep, no penalty term) and the confusion
    counts int64 [T] at the decision threshold."""
    loss: torch.Tensor
    tp: torch.Tensor
    fp: torch.Tensor
    tn: torch.Tensor
    fn: torch.Tensor

    @property
    def accuracy(self) -> torch.Tensor:
        """(tp + tn) / rows, fp64 [T] (0 when there are no rows)."""
        n = self.tp + self.fp + self.tn + self.fn
        return (self.tp + self.tn).double() / n.clamp(min=1).double()


def score_threshold(objective: str, threshold: Optional[float] = None
                    ) -> float:
    """The user's decision threshold as a threshold z_thr on the score
    z = x.w, in fp64; a row is predicted positive iff z > z_thr.
    hinge: z_thr = threshold, default 0 (MLlib SVMModel); lsq:
    z_thr = threshold, default 0.5; logistic: threshold is a probability in
    (0, 1), default 0.5, and z_thr = log(thr / (1 - thr)) — no sigmoid is
    evaluated for the decision (LogisticRegressionModel)."""
    if objective not in _OBJ_CODE:
        raise ValueError(f"unknown objective {objective!r}")
    if objective == "logistic":
        thr = 0.5 if threshold is None else float(threshold)
        if not 0.0 < thr < 1.0:
            raise ValueError(
                f"logistic threshold must lie in (0, 1), got {thr!r}")
        return 0.0 if thr == 0.5 else math.log(thr / (1.0 - thr))
    if threshold is None:
        return 0.5 if objective == "lsq" else 0.0
    thr = float(threshold)
    if not math.isfinite(thr):
        raise ValueError(f"threshold must be finite, got {thr!r}")
    return thr


def _eval_result(sums, n_rows: int, N_total: Optional[int]) -> EvalResult:
    loss_sum, tp, fp, tn, fn = sums
    N = N_total if N_total is not None else n_rows
    return EvalResult(loss_sum / max(int(N), 1), tp, fp, tn, fn)


def _eval_zeros(T: int, device) -> EvalResult:
    z = lambda dt: torch.zeros(T, dtype=dt, device=device)
    return EvalResult(z(torch.float64), *(z(torch.int64) for _ in range(4)))


def evaluate(X: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
             objective: str = "lsq", *, threshold: Optional[float] = None,
             N_total: Optional[int] = None) -> EvalResult:
    """Score the stacked iterates W [T, d] on the rows (X, y) — typically
    rows the model was not trained on — with the fused evaluation kernels
    (K9): one pass over X per tile of iterates, nothing of size rows x T
    written. w stays fp32 whatever X's dtype. CPU tensors take the fp64
    reference."""
    z_thr = score_threshold(objective, threshold)
    if W.dim() != 2 or W.shape[1] != X.shape[1]:
        raise ValueError(f"W must be [T, {X.shape[1]}], got {tuple(W.shape)}")
    n_rows, T = X.shape[0], W.shape[0]
    if n_rows == 0 or T == 0:
        return _eval_zeros(T, X.device)
    if X.is_cuda:
        mod = _require_hip("evaluate")
        if mod is not None:
            return _eval_result(
                mod.evaluate(X, y, W, _OBJ_CODE[objective], z_thr), n_rows,
                N_total)
    return _eval_result(torch_ref.evaluate(X, y, W, objective, z_thr),
                        n_rows, N_total)


class CurveResult(NamedTuple):
    """Confusion counts of T stacked iterates at K score thresholds each:
    ``z_thr`` fp64 [T, K], non-decreasing along K; ``tp``/``fp``/``tn``/
    ``fn`` int64 [T, K] at ``z > z_thr[t, k]``; ``n_pos``/``n_neg`` int64
    [T]. Every point lies exactly on the iterate's true curve; the
    thresholds only choose which points.

    The metrics follow MLlib's BinaryClassificationMetrics, in fp64. The
    by-threshold ones (precision, recall, fpr, f_measure) are [T, K],
    column k belonging to ``z_thr[:, k]``; roc() and pr() return the curve
    points in MLlib's order, descending threshold."""
    z_thr: torch.Tensor
    tp: torch.Tensor
    fp: torch.Tensor
    tn: torch.Tensor
    fn: torch.Tensor
    n_pos: torch.Tensor
    n_neg: torch.Tensor

    @staticmethod
    def _ratio(num: torch.Tensor, den: torch.Tensor, empty: float
               ) -> torch.Tensor:
        """num / den in fp64, `empty` where den == 0."""
        num, den = torch.broadcast_tensors(num.double(), den.double())
        safe = torch.where(den == 0, torch.ones_like(den), den)
        return torch.where(den == 0, torch.full_like(num, empty), num / safe)

    def precision(self) -> torch.Tensor:
        """tp / (tp + fp); 1 where nothing is predicted positive."""
        return self._ratio(self.tp, self.tp + self.fp, 1.0)

    def recall(self) -> torch.Tensor:
        """tp / n_pos (the true-positive rate); 0 without positives."""
        return self._ratio(self.tp, self.n_pos[:, None], 0.0)

    def fpr(self) -> torch.Tensor:
        """fp / n_neg; 0 without negatives."""
        return self._ratio(self.fp, self.n_neg[:, None], 0.0)

    def f_measure(self, beta: float = 1.0) -> torch.Tensor:
        """(1 + beta^2) p r / (beta^2 p + r); 0 where p + r == 0."""
        p, r, b2 = self.precision(), self.recall(), float(beta) ** 2
        return self._ratio((1.0 + b2) * p * r, b2 * p + r, 0.0)

    def roc(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(fpr, recall), each [T, K + 2]: the points by descending
        threshold, with (0, 0) prepended and (1, 1) appended."""
        T, dev = self.tp.shape[0], self.tp.device
        zero = torch.zeros(T, 1, dtype=torch.float64, device=dev)
        one = torch.ones(T, 1, dtype=torch.float64, device=dev)
        return (torch.cat([zero, self.fpr().flip(1), one], dim=1),
                torch.cat([zero, self.recall().flip(1), one], dim=1))

    def pr(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(recall, precision), each [T, K + 1]: the points by descending
        threshold, with (0, first precision) prepended (precision 1 when
        there is no point)."""
        T, dev = self.tp.shape[0], self.tp.device
        p = self.precision().flip(1)
        first = p[:, :1] if p.shape[1] else torch.ones(
            T, 1, dtype=torch.float64, device=dev)
        zero = torch.zeros(T, 1, dtype=torch.float64, device=dev)
        return (torch.cat([zero, self.recall().flip(1)], dim=1),
                torch.cat([first, p], dim=1))

    @staticmethod
    def _trapezoid(x: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """AreaUnderCurve: sum of (x1 - x0) (v0 + v1) / 2 over consecutive
        points."""
        return ((x[:, 1:] - x[:, :-1]) * (v[:, 1:] + v[:, :-1]) / 2.0).sum(1)

    def auc_roc(self) -> torch.Tensor:
        """areaUnderROC, fp64 [T]."""
        return self._trapezoid(*self.roc())

    def auc_pr(self) -> torch.Tensor:
        """areaUnderPR, fp64 [T]."""
        return self._trapezoid(*self.pr())


_CURVE_SAMPLE_ROWS = 8192


def _order_statistics(Z: torch.Tensor, num_bins: int) -> torch.Tensor:
    """fp64 [T, B]: per column of the sampled scores Z [S, T], the order
    statistics at the levels (k + 1/2) / B. Non-finite picks are clamped to
    the fp32 range so that every threshold is finite."""
    S = Z.shape[0]
    srt = Z.float().sort(dim=0).values
    pick = ((torch.arange(num_bins, dtype=torch.float64) + 0.5)
            * (S / num_bins)).floor().long().clamp(max=S - 1)
    big = torch.finfo(torch.float32).max
    thr = srt[pick.to(Z.device)].t().double()
    return torch.nan_to_num(thr, nan=big, posinf=big, neginf=-big).contiguous()


def _sample_rows(n_rows: int, device) -> torch.Tensor:
    """At most 8192 row ids, floor(i * n / S): strided, no RNG."""
    S = min(n_rows, _CURVE_SAMPLE_ROWS)
    return (torch.arange(S, dtype=torch.int64, device=device) * n_rows) // S


def _check_bins(num_bins) -> int:
    if int(num_bins) != num_bins or int(num_bins) < 1:
        raise ValueError(f"num_bins must be a positive integer, got "
                         f"{num_bins!r}")
    return int(num_bins)


def curve_thresholds(X: torch.Tensor, W: torch.Tensor, num_bins: int
                     ) -> torch.Tensor:
    """Score thresholds for a curve of num_bins points per iterate, fp64
    [T, num_bins], non-decreasing, without sorting the data: score at most
    8192 strided rows against all iterates (a small matmul on X's device),
    sort that sample, and take its order statistics at (k + 1/2) / B.
    Duplicates are possible; they repeat a point of the curve."""
    B = _check_bins(num_bins)
    if X.shape[0] == 0:
        return torch.zeros(W.shape[0], B, dtype=torch.float64,
                           device=X.device)
    rows = _sample_rows(X.shape[0], X.device)
    Z = X[rows].float() @ W.to(X.device).float().t()
    return _order_statistics(Z, B)


def curve_thresholds_csr(indptr: torch.Tensor, indices: torch.Tensor,
                         values: torch.Tensor, W: torch.Tensor,
                         num_bins: int) -> torch.Tensor:
    """CSR form of curve_thresholds: an index_add_ over the non-zeros of
    the sampled rows; nothing is densified."""
    B = _check_bins(num_bins)
    dev = values.device
    n_rows = indptr.shape[0] - 1
    if n_rows <= 0:
        return torch.zeros(W.shape[0], B, dtype=torch.float64, device=dev)
    rows = _sample_rows(n_rows, dev)
    start = indptr[rows].long()
    count = indptr[rows + 1].long() - start
    slot = torch.repeat_interleave(
        torch.arange(rows.numel(), device=dev), count)
    first = count.cumsum(0) - count  # of each sampled row, in `slot` order
    p = start[slot] + torch.arange(slot.numel(), device=dev) - first[slot]
    Wt = W.to(dev).float().t()  # [d, T]
    Z = torch.zeros(rows.numel(), W.shape[0], dtype=torch.float32, device=dev)
    Z.index_add_(0, slot, values[p].float()[:, None] * Wt[indices[p].long()])
    return _order_statistics(Z, B)


def _curve_z_thresholds(objective: str, T: int, device, thresholds,
                        z_thresholds, num_bins, from_bins) -> torch.Tensor:
    """The fp64 [T, K] score thresholds of an evaluate_curve call."""
    if objective not in _OBJ_CODE:
        raise ValueError(f"unknown objective {objective!r}")
    given = [a is not None for a in (thresholds, z_thresholds, num_bins)]
    if sum(given) != 1:
        raise ValueError("give exactly one of thresholds, z_thresholds and "
                         "num_bins")
    if num_bins is not None:
        return from_bins(_check_bins(num_bins))
    if thresholds is not None:
        thr = torch.as_tensor(thresholds, dtype=torch.float64).cpu()
        if thr.dim() != 1:
            raise ValueError(f"thresholds must be [K], got "
                             f"{tuple(thr.shape)}")
        z = torch.tensor([score_threshold(objective, v)
                          for v in thr.tolist()], dtype=torch.float64)
        z = z.sort().values
    else:
        z = torch.as_tensor(z_thresholds, dtype=torch.float64)
        if z.dim() not in (1, 2) or (z.dim() == 2 and z.shape[0] != T):
            raise ValueError(f"z_thresholds must be [K] or [{T}, K], got "
                             f"{tuple(z.shape)}")
        if not bool(torch.isfinite(z).all()):
            raise ValueError("z_thresholds must be finite")
        if bool((z[..., 1:] < z[..., :-1]).any()):
            raise ValueError("z_thresholds must be non-decreasing")
    if z.dim() == 1:
        z = z[None, :].expand(T, -1)
    return z.to(device).contiguous()


def _curve_zeros(z_thr: torch.Tensor) -> CurveResult:
    T = z_thr.shape[0]
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=z_thr.device)
    return CurveResult(z_thr, *(z(*z_thr.shape) for _ in range(4)), z(T),
                       z(T))


def evaluate_curve(X: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
                   objective: str = "lsq", *, thresholds=None,
                   z_thresholds=None, num_bins: Optional[int] = None
                   ) -> CurveResult:
    """Confusion counts of the stacked iterates W [T, d] on the rows (X, y)
    at K thresholds per iterate, from one pass over X per tile of iterates
    and eval_curve_tile() thresholds (the threshold-sweep kernels, K10) —
    the points of the ROC and PR curves, without a sort. Exactly one of:
    ``thresholds`` [K] in the user's units (each through score_threshold,
    then sorted), ``z_thresholds`` [K] or [T, K] finite non-decreasing score
    thresholds, ``num_bins`` (curve_thresholds picks the thresholds). CPU
    tensors take the fp64 reference."""
    if W.dim() != 2 or W.shape[1] != X.shape[1]:
        raise ValueError(f"W must be [T, {X.shape[1]}], got {tuple(W.shape)}")
    n_rows, T = X.shape[0], W.shape[0]
    z_thr = _curve_z_thresholds(
        objective, T, X.device, thresholds, z_thresholds, num_bins,
        lambda B: curve_thresholds(X, W, B))
    if n_rows == 0 or T == 0 or z_thr.shape[1] == 0:
        return _curve_zeros(z_thr)
    if X.is_cuda:
        mod = _require_hip("evaluate_curve")
        if mod is not None:
            return CurveResult(z_thr, *mod.evaluate_curve(X, y, W, z_thr))
    return CurveResult(z_thr, *torch_ref.evaluate_curve(X, y, W, z_thr))


def evaluate_curve_csr(indptr: torch.Tensor, indices: torch.Tensor,
                       values: torch.Tensor, y: torch.Tensor,
                       W: torch.Tensor, objective: str = "lsq", *,
                       thresholds=None, z_thresholds=None,
                       num_bins: Optional[int] = None) -> CurveResult:
    """CSR form of evaluate_curve."""
    if W.dim() != 2:
        raise ValueError(f"W must be [T, d], got {tuple(W.shape)}")
    n_rows, T = indptr.shape[0] - 1, W.shape[0]
    z_thr = _curve_z_thresholds(
        objective, T, values.device, thresholds, z_thresholds, num_bins,
        lambda B: curve_thresholds_csr(indptr, indices, values, W, B))
    if n_rows <= 0 or T == 0 or z_thr.shape[1] == 0:
        return _curve_zeros(z_thr)
    if values.is_cuda:
        mod = _require_hip("evaluate_curve_csr")
        if mod is not None:
            return CurveResult(
                z_thr, *mod.evaluate_curve_csr(indptr, indices, values, y, W,
                                               z_thr))
    return CurveResult(
        z_thr, *torch_ref.evaluate_curve_csr(indptr, indices, values, y, W,
                                             z_thr))


def evaluate_csr(indptr: torch.Tensor, indices: torch.Tensor,
                 values: torch.Tensor, y: torch.Tensor, W: torch.Tensor,
                 objective: str = "lsq", *, threshold: Optional[float] = None,
                 N_total: Optional[int] = None) -> EvalResult:
    """CSR form of evaluate: one column gather per non-zero serves the
    whole tile of iterates, and bf16 values are never expanded."""
    z_thr = score_threshold(objective, threshold)
    if W.dim() != 2:
        raise ValueError(f"W must be [T, d], got {tuple(W.shape)}")
    n_rows, T = indptr.shape[0] - 1, W.shape[0]
    if n_rows <= 0 or T == 0:
        return _eval_zeros(T, values.device)
    if values.is_cuda:
        mod = _require_hip("evaluate_csr")
        if mod is not None:
            return _eval_result(
                mod.evaluate_csr(indptr, indices, values, y, W,
                                 _OBJ_CODE[objective], z_thr), n_rows,
                N_total)
    return _eval_result(
        torch_ref.evaluate_csr(indptr, indices, values, y, W, objective,
                               z_thr), n_rows, N_total)


class ColStats(NamedTuple):
    """Per-column summary of a data matrix (MLlib Statistics.colStats /
    MultivariateOnlineSummarizer): ``count`` rows; ``mean``, ``m2`` =
    sum (x - mean)^2, ``min``, ``max``, ``norm_l1`` = sum |x| and ``sumsq`` =
    sum x^2 in fp64 [d]; ``num_nonzeros`` int64 [d]. For CSR data the
    implicit zeros count towards count, mean, m2, min and max."""
    count: int
    mean: torch.Tensor
    m2: torch.Tensor
    num_nonzeros: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    norm_l1: torch.Tensor
    sumsq: torch.Tensor

    @property
    def variance(self) -> torch.Tensor:
        """m2 / (count - 1), MLlib's unbiased form; 0 for count <= 1."""
        if self.count <= 1:
            return torch.zeros_like(self.m2)
        return self.m2 / (self.count - 1)

    @property
    def std(self) -> torch.Tensor:
        return self.variance.sqrt()

    @property
    def norm_l2(self) -> torch.Tensor:
        return self.sumsq.sqrt()

    def merge(self, other: "ColStats") -> "ColStats":
        """The summary of both row sets together (shards, a file read in
        chunks): the pairwise update of Chan et al. on (count, mean, m2),
        as the kernels merge their partials, on the host. A column that
        holds one value overall gets m2 == 0 exactly."""
        na, nb = self.count, other.count
        if nb == 0:
            return self
        if na == 0:
            return other
        o = ColStats(nb, *(t.to(self.mean.device) for t in other[1:]))
        n = na + nb
        delta = o.mean - self.mean
        mean = self.mean + delta * (nb / n)
        m2 = self.m2 + o.m2 + delta * delta * (na * nb / n)
        mn = torch.minimum(self.min, o.min)
        mx = torch.maximum(self.max, o.max)
        m2 = torch.where(mn == mx, torch.zeros_like(m2), m2)
        return ColStats(n, mean, m2, self.num_nonzeros + o.num_nonzeros, mn,
                        mx, self.norm_l1 + o.norm_l1, self.sumsq + o.sumsq)


def _col_stats_zeros(d: int, device) -> ColStats:
    z = lambda: torch.zeros(d, dtype=torch.float64, device=device)
    return ColStats(0, z(), z(), torch.zeros(d, dtype=torch.int64,
                                             device=device),
                    z(), z(), z(), z())


def col_stats(X: torch.Tensor) -> ColStats:
    """Column statistics of X [n, d] from one pass over it (K11,
    csrc/col_stats.h): fp64 accumulation about a per-column pivot, partials
    merged in a fixed order, so two calls are bit-identical and a constant
    column has m2 == 0 exactly. bf16 data is never expanded in memory. CPU
    tensors take the fp64 two-pass reference. Zero rows: zeros, with
    min = max = 0, without a launch."""
    if X.dim() != 2:
        raise ValueError(f"X must be [n, d], got {tuple(X.shape)}")
    n, d = X.shape
    if n == 0 or d == 0:
        return _col_stats_zeros(d, X.device)
    if X.is_cuda:
        mod = _require_hip("col_stats")
        if mod is not None:
            return ColStats(n, *mod.col_stats(X))
    return ColStats(n, *torch_ref.col_stats(X))


def col_stats_csr(indptr: torch.Tensor, indices: torch.Tensor,
                  values: torch.Tensor, d: int) -> ColStats:
    """CSR form of col_stats. On a GPU the sums over the non-zeros are fp64
    atomic adds: mean, m2, norm_l1 and sumsq are reproducible to the fp64
    summation bound (nnz_j * 2^-52 * sum |term|), not bitwise;
    num_nonzeros, min and max are exact, and a column that holds one value
    (implicit zeros included) has m2 == 0 exactly."""
    n = indptr.shape[0] - 1
    if n <= 0 or d == 0:
        return _col_stats_zeros(d, values.device)
    if values.is_cuda:
        mod = _require_hip("col_stats_csr")
        if mod is not None:
            return ColStats(n, *mod.col_stats_csr(indptr, indices, values,
                                                  int(d)))
    return ColStats(n, *torch_ref.col_stats_csr(indptr, indices, values,
                                                int(d)))


def scale_(X: torch.Tensor, mean: torch.Tensor, factor: torch.Tensor, *,
           with_mean: bool = False) -> None:
    """X <- (X - mean) * factor per column, in place: fp32 arithmetic,
    rounded once to X's type. ``mean`` and ``factor`` are fp32 [d]; without
    ``with_mean`` the mean is not read."""
    if X.is_cuda:
        mod = _require_hip("scale_")
        if mod is not None:
            mod.scale_(X, mean, factor, with_mean)
            return
    torch_ref.scale_(X, mean, factor, with_mean)


def scale_csr_(indices: torch.Tensor, values: torch.Tensor,
               factor: torch.Tensor) -> None:
    """values <- values * factor[indices], in place (fp32, rounded once)."""
    if values.is_cuda:
        mod = _require_hip("scale_csr_")
        if mod is not None:
            mod.scale_csr_(indices, values, factor)
            return
    torch_ref.scale_csr_(indices, values, factor)
