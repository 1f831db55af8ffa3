"""Tensor-level adapter over the raw CDNA4 kernel module
(``asyncframework_amd._hip_core``, built in-tree by setup.py with
``hipcc --offload-arch=gfx950``). Validates shapes/dtypes, extracts device
pointers and the current HIP stream, and returns torch-native results.

Importing this module raises ImportError when the extension .so is missing —
ops.__init__ turns that into a loud error on GPU boxes."""

from __future__ import annotations

from typing import Tuple

import torch

from .. import _hip_core  # in-tree .so — ImportError here is intentional


def _assert_provenance() -> None:
    """Backstop for the __init__ guard: the loaded binary's embedded source
    hash must match the csrc/ sources next to it (catches a manually swapped
    .so; the round-1 stale-binary hole)."""
    import sys
    bh = sys.modules.get("build_hip")
    if bh is None:  # not running from a source checkout
        return
    expect = bh.src_hash()
    got = getattr(_hip_core, "__src_hash__", "unstamped")
    if got != expect:
        raise ImportError(
            f"_hip_core.so provenance mismatch: binary built from {got}, "
            f"sources hash to {expect}; run `python build_hip.py --force`")


_assert_provenance()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, name: str, dtype=None, contiguous=True):
    assert t.is_cuda, f"{name} must be a CUDA tensor"
    if dtype is not None:
        assert t.dtype == dtype, f"{name} must be {dtype}, got {t.dtype}"
    if contiguous:
        assert t.is_contiguous(), f"{name} must be contiguous"


def _xcode(X: torch.Tensor) -> int:
    if X.dtype == torch.bfloat16:
        return 1
    if X.dtype == torch.float32:
        return 0
    raise TypeError(f"X dtype must be fp32 or bf16, got {X.dtype}")


CU_LDS_BYTES = 163840  # one CU's LDS (csrc/kernels.hip)


def _chk_row_start(row_start) -> None:
    # the kernels take the Philox block of a row as (row_start + i) / 4
    assert row_start % 4 == 0, "shard starts must be 4-aligned (philox block)"


def _chk_dense_lds(d: int) -> None:
    """The generic dense kernel (d > 2048, d % 4 != 0 or ASYNCAMD_NO_PIPE=1)
    keeps w and one gradient slab per sub-wave in LDS; past one CU's LDS it
    cannot launch."""
    pipe, lpr, lds = _hip_core.dense_launch_form(int(d))
    if not pipe and lds > CU_LDS_BYTES:
        raise ValueError(
            f"dense gradient at d={d}: the generic kernel needs {lds} bytes "
            f"of LDS at {lpr} lanes per row, over the limit of "
            f"{CU_LDS_BYTES} bytes per workgroup")


def grad_dense(X, y, w, out, seed, round_k, row_start, rate, obj) -> int:
    _chk(X, "X")
    _chk_row_start(row_start)
    _chk(y, "y", torch.float32)
    _chk(out, "out", torch.float32)
    w = w.float().contiguous()
    n_rows, d = X.shape
    _chk_dense_lds(d)
    n_ctr = torch.zeros(1, dtype=torch.int32, device=X.device)
    _hip_core.grad_dense(X.data_ptr(), y.data_ptr(), w.data_ptr(),
                         out.data_ptr(), 0, n_ctr.data_ptr(), 0, n_rows, d,
                         seed,
                         round_k & 0xFFFFFFFF, row_start, rate, obj,
                         _xcode(X), _stream())
    return int(n_ctr.item())


def grad_csr(indptr, indices, values, y, w, out, seed, round_k, row_start,
             rate, obj) -> int:
    _chk_row_start(row_start)
    _chk(indptr, "indptr", torch.int32)
    _chk(indices, "indices", torch.int32)
    _chk(values, "values")
    _chk(y, "y", torch.float32)
    _chk(out, "out", torch.float32)
    w = w.float().contiguous()
    n_rows = indptr.shape[0] - 1
    n_ctr = torch.zeros(1, dtype=torch.int32, device=w.device)
    _hip_core.grad_csr(indptr.data_ptr(), indices.data_ptr(),
                       values.data_ptr(), y.data_ptr(), w.data_ptr(),
                       out.data_ptr(), n_ctr.data_ptr(), 0, n_rows, seed,
                       round_k & 0xFFFFFFFF, row_start, rate, obj,
                       _xcode(values), _stream())
    return int(n_ctr.item())


def saga_grad_dense(X, y, w, alpha, g, seed, round_k, row_start, rate, obj
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    _chk(X, "X")
    _chk_row_start(row_start)
    _chk(alpha, "alpha", torch.float32)
    _chk(g, "g", torch.float32)
    w = w.float().contiguous()
    n_rows, d = X.shape
    _chk_dense_lds(d)
    cap = n_rows if rate >= 1.0 else min(n_rows,
                                         int(rate * n_rows * 2) + 4096)
    idx = torch.empty(cap, dtype=torch.int32, device=X.device)
    e = torch.empty(cap, dtype=torch.float32, device=X.device)
    ctr = torch.zeros(2, dtype=torch.int32, device=X.device)  # [n, pos]
    _hip_core.saga_grad_dense(X.data_ptr(), y.data_ptr(), w.data_ptr(),
                              alpha.data_ptr(), g.data_ptr(), 0,
                              ctr.data_ptr(), idx.data_ptr(), e.data_ptr(),
                              ctr.data_ptr() + 4, 0, 0, n_rows, d, seed,
                              round_k & 0xFFFFFFFF, row_start, rate, obj,
                              _xcode(X), _stream())
    n = int(ctr[1].item())
    return idx[:n].long(), e[:n]


def saga_grad_csr(indptr, indices, values, y, w, alpha, g, seed, round_k,
                  row_start, rate, obj) -> Tuple[torch.Tensor, torch.Tensor]:
    _chk_row_start(row_start)
    _chk(indptr, "indptr", torch.int32)
    _chk(alpha, "alpha", torch.float32)
    _chk(g, "g", torch.float32)
    w = w.float().contiguous()
    n_rows = indptr.shape[0] - 1
    cap = n_rows if rate >= 1.0 else min(n_rows,
                                         int(rate * n_rows * 2) + 4096)
    idx = torch.empty(cap, dtype=torch.int32, device=w.device)
    e = torch.empty(cap, dtype=torch.float32, device=w.device)
    ctr = torch.zeros(2, dtype=torch.int32, device=w.device)
    _hip_core.saga_grad_csr(indptr.data_ptr(), indices.data_ptr(),
                            values.data_ptr(), y.data_ptr(), w.data_ptr(),
                            alpha.data_ptr(), g.data_ptr(), ctr.data_ptr(),
                            idx.data_ptr(), e.data_ptr(), ctr.data_ptr() + 4,
                            0, 0, n_rows, seed, round_k & 0xFFFFFFFF, row_start,
                            rate, obj, _xcode(values), _stream())
    n = int(ctr[1].item())
    return idx[:n].long(), e[:n]


def saga_commit(alpha, idx, e) -> None:
    _chk(alpha, "alpha", torch.float32)
    idx32 = idx.to(torch.int32) if idx.dtype != torch.int32 else idx
    _hip_core.saga_commit(alpha.data_ptr(), idx32.data_ptr(), e.data_ptr(),
                          int(idx32.numel()), _stream())


def saga_commit_pinned(alpha_pinned, idx, e) -> None:
    """Commit staged history scalars into the pinned-host master table by
    kernel scatter (ROCm pinned memory is device-writable): replaces the
    round-1 spill path's two synchronous D2H copies + host scatter."""
    assert alpha_pinned.is_pinned() and alpha_pinned.dtype == torch.float32
    idx32 = idx.to(torch.int32) if idx.dtype != torch.int32 else idx
    _hip_core.saga_commit(alpha_pinned.data_ptr(), idx32.data_ptr(),
                          e.data_ptr(), int(idx32.numel()), _stream())


def spill_refresh(alpha_dev, alpha_pinned, y, rowlist, ylist, cnt, cap, *,
                  seed, round_k, row_start, rate) -> None:
    """Host-spill α staging refresh (BASELINE config 5): scan
    the round's Philox mask (same key the gradient kernel will use) into a
    device row list, then gather ONLY those entries from the pinned master
    into the device staging table — ~1% of the table instead of all of it,
    fully async on the current stream."""
    _chk_row_start(row_start)
    _chk(alpha_dev, "alpha_dev", torch.float32)
    assert alpha_pinned.is_pinned() and alpha_pinned.dtype == torch.float32
    cnt.zero_()
    _hip_core.scan_rows(y.data_ptr(), rowlist.data_ptr(), ylist.data_ptr(),
                        cnt.data_ptr(), 0, int(y.numel()), int(seed),
                        int(round_k) & 0xFFFFFFFF, int(row_start),
                        float(rate), _stream())
    _hip_core.alpha_gather(alpha_dev.data_ptr(), alpha_pinned.data_ptr(),
                           rowlist.data_ptr(), cnt.data_ptr(), int(cap),
                           _stream())


def sgd_update(w, g, gamma_k, inv_batch, l2=0.0, l1=0.0) -> None:
    _chk(w, "w", torch.float32)
    _chk(g, "g", torch.float32)
    _hip_core.sgd_update(w.data_ptr(), g.data_ptr(), gamma_k, inv_batch,
                         int(w.numel()), _stream(), l2, l1)


def saga_update(w, g, alpha_bar, gamma, inv_batch, inv_N, l2=0.0,
                l1=0.0) -> None:
    _chk(w, "w", torch.float32)
    _chk(alpha_bar, "alpha_bar", torch.float32)
    _hip_core.saga_update(w.data_ptr(), g.data_ptr(), alpha_bar.data_ptr(),
                          gamma, inv_batch, inv_N, int(w.numel()), _stream(),
                          l2, l1)


def _eval_buffers(W, d, device, grid, transposed):
    """Zero-padded fp32 tiles of the iterates + the kernels' scratch and
    output buffers. Returns (Wtiles, n_tiles, part_loss, part_cnt, out_loss,
    out_cnt)."""
    tt = _hip_core.eval_tile()
    T = W.shape[0]
    n_tiles = (T + tt - 1) // tt
    Wp = torch.zeros(n_tiles * tt, d, dtype=torch.float32, device=device)
    Wp[:T] = W.to(device=device, dtype=torch.float32)
    if transposed:  # [n_tiles][d][tt]
        Wp = Wp.view(n_tiles, tt, d).transpose(1, 2).contiguous()
    part_loss = torch.empty(grid * tt, dtype=torch.float64, device=device)
    part_cnt = torch.empty(grid * 4 * tt, dtype=torch.int64, device=device)
    out_loss = torch.empty(n_tiles * tt, dtype=torch.float64, device=device)
    out_cnt = torch.empty(4, n_tiles * tt, dtype=torch.int64, device=device)
    return Wp, n_tiles, part_loss, part_cnt, out_loss, out_cnt


def _curve_buffers(W, z_thr, d, device, grid, transposed):
    """The sweep's buffers: iterate tiles as _eval_buffers, the thresholds
    z_thr [T, K] padded with +inf to whole tiles and passes, scratch and
    outputs. Returns (Wtiles, thr, n_tiles, n_pass, part_tot, part_hist,
    out_cnt, out_tot)."""
    tt, kt = _hip_core.eval_tile(), _hip_core.eval_curve_tile()
    T, K = z_thr.shape
    Wp, n_tiles = _eval_buffers(W, d, device, 0, transposed)[:2]
    n_pass = (K + kt - 1) // kt
    thr = torch.full((n_tiles * tt, n_pass * kt), float("inf"),
                     dtype=torch.float64, device=device)
    thr[:T, :K] = z_thr.to(device=device, dtype=torch.float64)
    part_tot = torch.empty(grid * 2 * tt, dtype=torch.int64, device=device)
    # uint32 counts: a block sees fewer than 2^31 rows
    part_hist = torch.empty(grid * tt * kt * 2, dtype=torch.int32,
                            device=device)
    out_cnt = torch.empty(4, n_tiles * tt, K, dtype=torch.int64,
                          device=device)
    out_tot = torch.empty(2, n_tiles * tt, dtype=torch.int64, device=device)
    return Wp, thr, n_tiles, n_pass, part_tot, part_hist, out_cnt, out_tot


def _curve_result(out_cnt, out_tot, T):
    return (out_cnt[0, :T], out_cnt[1, :T], out_cnt[2, :T], out_cnt[3, :T],
            out_tot[0, :T], out_tot[1, :T])


def evaluate_curve(X, y, W, z_thr):
    """(tp, fp, tn, fn [T, K], n_pos, n_neg [T]) of the iterates W [T, d]
    over (X, y) at the score thresholds z_thr [T, K] (rows non-decreasing)."""
    _chk(X, "X")
    _chk(y, "y", torch.float32)
    n_rows, d = X.shape
    assert y.numel() == n_rows and W.shape[1] == d
    assert n_rows < 2 ** 31, "row ids are 32-bit"
    T, K = z_thr.shape
    assert T == W.shape[0] and K > 0
    grid = _hip_core.eval_grid(n_rows, d, 0)
    Wp, thr, n_tiles, n_pass, pt, ph, oc, ot = _curve_buffers(
        W, z_thr, d, X.device, grid, False)
    _hip_core.eval_curve_dense(X.data_ptr(), y.data_ptr(), Wp.data_ptr(),
                               thr.data_ptr(), n_tiles, n_pass, K, n_rows, d,
                               _xcode(X), pt.data_ptr(), ph.data_ptr(),
                               oc.data_ptr(), ot.data_ptr(), _stream())
    return _curve_result(oc, ot, T)


def evaluate_curve_csr(indptr, indices, values, y, W, z_thr):
    _chk(indptr, "indptr", torch.int32)
    _chk(indices, "indices", torch.int32)
    _chk(values, "values")
    _chk(y, "y", torch.float32)
    n_rows = indptr.shape[0] - 1
    assert y.numel() == n_rows
    T, d = W.shape
    K = z_thr.shape[1]
    assert z_thr.shape[0] == T and K > 0
    grid = _hip_core.eval_grid(n_rows, d, 1)
    Wp, thr, n_tiles, n_pass, pt, ph, oc, ot = _curve_buffers(
        W, z_thr, d, values.device, grid, True)
    _hip_core.eval_curve_csr(indptr.data_ptr(), indices.data_ptr(),
                             values.data_ptr(), y.data_ptr(), Wp.data_ptr(),
                             thr.data_ptr(), n_tiles, n_pass, K, n_rows, d,
                             _xcode(values), pt.data_ptr(), ph.data_ptr(),
                             oc.data_ptr(), ot.data_ptr(), _stream())
    return _curve_result(oc, ot, T)


def evaluate(X, y, W, obj, z_thr):
    """(loss_sum, tp, fp, tn, fn) of the iterates W [T, d] over (X, y)."""
    _chk(X, "X")
    _chk(y, "y", torch.float32)
    n_rows, d = X.shape
    assert y.numel() == n_rows and W.shape[1] == d
    assert n_rows < 2 ** 31, "row ids are 32-bit"
    T = W.shape[0]
    grid = _hip_core.eval_grid(n_rows, d, 0)
    Wp, n_tiles, pl, pc, ol, oc = _eval_buffers(W, d, X.device, grid, False)
    _hip_core.eval_dense(X.data_ptr(), y.data_ptr(), Wp.data_ptr(), n_tiles,
                         n_rows, d, obj, float(z_thr), _xcode(X),
                         pl.data_ptr(), pc.data_ptr(), ol.data_ptr(),
                         oc.data_ptr(), _stream())
    return (ol[:T], oc[0, :T], oc[1, :T], oc[2, :T], oc[3, :T])


def evaluate_csr(indptr, indices, values, y, W, obj, z_thr):
    _chk(indptr, "indptr", torch.int32)
    _chk(indices, "indices", torch.int32)
    _chk(values, "values")
    _chk(y, "y", torch.float32)
    n_rows = indptr.shape[0] - 1
    assert y.numel() == n_rows
    T, d = W.shape
    grid = _hip_core.eval_grid(n_rows, d, 1)
    Wp, n_tiles, pl, pc, ol, oc = _eval_buffers(W, d, values.device, grid,
                                                True)
    _hip_core.eval_csr(indptr.data_ptr(), indices.data_ptr(),
                       values.data_ptr(), y.data_ptr(), Wp.data_ptr(),
                       n_tiles, n_rows, d, obj, float(z_thr), _xcode(values),
                       pl.data_ptr(), pc.data_ptr(), ol.data_ptr(),
                       oc.data_ptr(), _stream())
    return (ol[:T], oc[0, :T], oc[1, :T], oc[2, :T], oc[3, :T])


def _col_stats_out(d, device):
    out_f64 = torch.empty(6, d, dtype=torch.float64, device=device)
    out_nnz = torch.empty(d, dtype=torch.int64, device=device)
    return out_f64, out_nnz


def _col_stats_result(out_f64, out_nnz):
    """(mean, m2, num_nonzeros, min, max, norm_l1, sumsq)."""
    return (out_f64[0], out_f64[1], out_nnz, out_f64[2], out_f64[3],
            out_f64[4], out_f64[5])


def col_stats(X):
    """Per-column statistics of X [n, d], n > 0 and d > 0, from one pass
    (csrc/col_stats.h)."""
    _chk(X, "X")
    n_rows, d = X.shape
    assert n_rows > 0 and d > 0
    assert n_rows < 2 ** 31, "per-block non-zero counts are 32-bit"
    bf = _xcode(X)
    gy = int(_hip_core.col_stats_geom(X.data_ptr(), n_rows, d, bf)["grid_y"])
    dev = X.device
    part_f64 = torch.empty(gy * 5 * d, dtype=torch.float64, device=dev)
    part_mm = torch.empty(gy * 2 * d, dtype=torch.float32, device=dev)
    part_nnz = torch.empty(gy * d, dtype=torch.int32, device=dev)
    out_f64, out_nnz = _col_stats_out(d, dev)
    _hip_core.col_stats_dense(X.data_ptr(), n_rows, d, bf,
                              part_f64.data_ptr(), part_mm.data_ptr(),
                              part_nnz.data_ptr(), out_f64.data_ptr(),
                              out_nnz.data_ptr(), _stream())
    return _col_stats_result(out_f64, out_nnz)


def col_stats_csr(indptr, indices, values, d):
    _chk(indptr, "indptr", torch.int32)
    _chk(indices, "indices", torch.int32)
    _chk(values, "values")
    n_rows = indptr.shape[0] - 1
    assert n_rows > 0 and d > 0 and n_rows < 2 ** 31
    assert indices.numel() == values.numel()
    dev = values.device
    sums = torch.empty(3 * d, dtype=torch.float64, device=dev)
    ints = torch.empty(3 * d, dtype=torch.int32, device=dev)
    out_f64, out_nnz = _col_stats_out(d, dev)
    _hip_core.col_stats_csr(indptr.data_ptr(), indices.data_ptr(),
                            values.data_ptr(), n_rows, d,
                            int(values.numel()), _xcode(values),
                            sums.data_ptr(), ints.data_ptr(),
                            out_f64.data_ptr(), out_nnz.data_ptr(), _stream())
    return _col_stats_result(out_f64, out_nnz)


def _chk_scale_vec(t, name, d, device):
    _chk(t, name, torch.float32)
    assert t.numel() == d and t.device == device, \
        f"{name} must be fp32 [{d}] on {device}"


def scale_(X, mean, factor, with_mean) -> None:
    """X <- ((X - mean) * factor) in fp32, rounded to X's type, in place."""
    _chk(X, "X")
    n_rows, d = X.shape
    if n_rows == 0 or d == 0:
        return
    _chk_scale_vec(mean, "mean", d, X.device)
    _chk_scale_vec(factor, "factor", d, X.device)
    _hip_core.scale_dense(X.data_ptr(), mean.data_ptr(), factor.data_ptr(),
                          n_rows, d, _xcode(X), int(bool(with_mean)),
                          _stream())


def scale_csr_(indices, values, factor) -> None:
    """values <- values * factor[indices] in fp32, rounded, in place."""
    _chk(indices, "indices", torch.int32)
    _chk(values, "values")
    if values.numel() == 0:
        return
    assert indices.numel() == values.numel()
    d = int(factor.numel())
    _chk_scale_vec(factor, "factor", d, values.device)
    _hip_core.scale_csr(indices.data_ptr(), values.data_ptr(),
                        factor.data_ptr(), int(values.numel()), d,
                        _xcode(values), _stream())
