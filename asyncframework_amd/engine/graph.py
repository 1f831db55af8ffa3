"""GPU-resident round loop: the whole ASGD/ASAGA iteration captured in a
hipGraph.

On one GPU with one worker, the async engine's round degenerates to the
strict sequence [sample+gradient, update] with staleness 0 — exactly the
reference's semantics at P=1 (every result accepted, clock advances once per
round). This engine keeps ALL round state on the device:

* ``k_dev``  — the round counter (the reference's iteration ``k``); the
  gradient kernel derives the Philox round key (= k+1, the analog of
  ``sample(false, b, seed+k+1)``) and the update kernel derives the step
  size gamma/sqrt(k/P+1) from it and increments it,
* ``w``/``g``/``alpha``/``alpha_bar`` — weights, gradient accumulator,
  SAGA history, SAGA average — so an unrolled sequence of kernel nodes is a
  complete hipGraph with zero host logic (measured: 780 updates/s with the
  threaded engine -> 17.2k with this engine on the mnist8m shape).

ASGD-dense additionally runs in OVERLAP mode: round r+1's Philox scan
(w-independent) executes on a side stream inside the captured graph,
concurrent with round r's gradient; rows land in a double-buffered global
(row, y) list consumed by a list-fed gradient kernel, and the update is
fused with the partial-slab reduction (last-finishing block advances k).
A dedicated scan-round counter, bumped stream-order on the side stream,
decouples the scan from the concurrently-incremented k.

This is the launch-bound-inner-loop -> hipGraph design the MI355X build
targets (no analog in the reference — Spark's per-iteration overhead is the
4x the paper beats; here we remove ours)."""

from __future__ import annotations

import time
from typing import List, Optional, Tuple

import torch

from .config import EngineConfig, refuse_penalties
from .worker import Shard


class GraphEngine:
    """Sequential device-resident ASGD/ASAGA on one GPU (num_workers == 1)."""

    UNROLL = 20

    def __init__(self, cfg: EngineConfig, shard: Shard,
                 device: torch.device, unroll: Optional[int] = None):
        # config-compat asserts first (testable without a GPU)
        refuse_penalties(cfg, "GraphEngine")
        assert not (cfg.algo == "asaga"
                    and cfg.history_placement == "host"), \
            "host-spill history needs the threads engine"
        assert cfg.delay_coeff == 0.0, \
            ("the graph engine is a single-worker device loop — straggler "
             "injection needs the threads/native/dist engines")
        from .. import _hip_core  # mandatory native path
        self._core = _hip_core
        assert device.type == "cuda"
        self.cfg = cfg
        self.shard = shard
        self.device = device
        self.unroll = unroll or self.UNROLL
        d = cfg.d
        self.w = torch.zeros(d, dtype=torch.float32, device=device)
        self.g = torch.zeros(d, dtype=torch.float32, device=device)
        self.k_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.n_dummy = torch.zeros(1, dtype=torch.int32, device=device)
        self.alpha = None
        self.alpha_bar = None
        if cfg.algo == "asaga":
            self.alpha = torch.zeros(shard.n_rows, dtype=torch.float32,
                                     device=device)
            self.alpha_bar = torch.zeros(d, dtype=torch.float32,
                                         device=device)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._obj_code = {"lsq": 0, "logistic": 1,
                          "hinge": 2}[cfg.objective]  # csrc/link.h
        # dense path: per-block partial slabs + parallel reduce (no global
        # atomics — measured 9%-of-HBM cap with the atomic finalize)
        self.g_part = None
        self._G = 0
        self._splits = 1
        if not shard.is_sparse:
            self._G = int(self._core.grad_grid(shard.n_rows))
            # reduce kernel parallelism: njc*splits blocks; G//8 keeps >=8
            # partials per thread (measured: splits=4 -> 16 blocks -> 7 us
            # latency-bound reduce; more blocks cut it to ~2-3 us)
            self._splits = max(1, min(64, self._G // 8))
            self.g_part = torch.zeros(d * self._G, dtype=torch.float32,
                                      device=device)
        # scan/compute overlap (ASGD dense): round r+1's Philox scan is
        # w-independent, so it runs on a side stream concurrent with round
        # r's gradient+update. Rows land in a double-buffered global list
        # with prefetched y values; a dedicated scan_round counter (bumped
        # stream-order on the side stream) avoids racing the k++ update.
        self._overlap = (cfg.algo == "asgd" and not shard.is_sparse
                         and d % 4 == 0 and d <= 2048)
        if self._overlap:
            n = shard.n_rows
            self._rowlist = [torch.zeros(n, dtype=torch.int32, device=device)
                             for _ in range(2)]
            self._ylist = [torch.zeros(n, dtype=torch.float32, device=device)
                           for _ in range(2)]
            self._count = [torch.zeros(1, dtype=torch.int32, device=device)
                           for _ in range(2)]
            self._scan_round = torch.zeros(1, dtype=torch.int32,
                                           device=device)
            self._ticket = torch.zeros(1, dtype=torch.int32, device=device)
            self._sideB = torch.cuda.Stream(device)
            self._ev_scan = [torch.cuda.Event(), torch.cuda.Event()]
            self._ev_grad = [torch.cuda.Event(), torch.cuda.Event()]
            self._cur = 0
            if self.unroll % 2:
                self.unroll += 1  # buffer parity must round-trip

    # -- one round = [grad(k_dev), fused_update(k_dev++)] --------------------
    def _launch_round(self) -> None:
        cfg, sh = self.cfg, self.shard
        stream = torch.cuda.current_stream().cuda_stream
        seed = cfg.seed
        if cfg.algo == "asaga":
            if sh.is_sparse:
                self._core.saga_grad_csr(
                    sh.indptr.data_ptr(), sh.indices.data_ptr(),
                    sh.values.data_ptr(), sh.y.data_ptr(), self.w.data_ptr(),
                    self.alpha.data_ptr(), self.g.data_ptr(),
                    self.n_dummy.data_ptr(), 0, 0, 0, self.k_dev.data_ptr(),
                    1, sh.n_rows, seed, 0, sh.row_start, cfg.batch_rate,
                    self._obj_code, 1 if sh.values.dtype == torch.bfloat16
                    else 0, stream)
            else:
                self._core.saga_grad_dense(
                    sh.X.data_ptr(), sh.y.data_ptr(), self.w.data_ptr(),
                    self.alpha.data_ptr(), self.g.data_ptr(),
                    self.g_part.data_ptr(), self.n_dummy.data_ptr(), 0, 0, 0,
                    self.k_dev.data_ptr(), 1, sh.n_rows, cfg.d, seed, 0,
                    sh.row_start, cfg.batch_rate, self._obj_code,
                    1 if sh.X.dtype == torch.bfloat16 else 0, stream)
                self._core.reduce_partials(self.g_part.data_ptr(),
                                           self.g.data_ptr(), cfg.d, self._G,
                                           self._splits, stream)
            self._core.saga_update_fused(
                self.w.data_ptr(), self.g.data_ptr(),
                self.alpha_bar.data_ptr(), self.k_dev.data_ptr(), cfg.gamma,
                1.0 / cfg.par_recs, 1.0 / cfg.N, cfg.d, stream)
        else:
            if sh.is_sparse:
                self._core.grad_csr(
                    sh.indptr.data_ptr(), sh.indices.data_ptr(),
                    sh.values.data_ptr(), sh.y.data_ptr(), self.w.data_ptr(),
                    self.g.data_ptr(), self.n_dummy.data_ptr(),
                    self.k_dev.data_ptr(), sh.n_rows, seed, 0, sh.row_start,
                    cfg.batch_rate, self._obj_code,
                    1 if sh.values.dtype == torch.bfloat16 else 0, stream)
            else:
                self._core.grad_dense(
                    sh.X.data_ptr(), sh.y.data_ptr(), self.w.data_ptr(),
                    self.g.data_ptr(), self.g_part.data_ptr(),
                    self.n_dummy.data_ptr(), self.k_dev.data_ptr(),
                    sh.n_rows, cfg.d, seed, 0, sh.row_start, cfg.batch_rate,
                    self._obj_code,
                    1 if sh.X.dtype == torch.bfloat16 else 0, stream)
                self._core.reduce_partials(self.g_part.data_ptr(),
                                           self.g.data_ptr(), cfg.d, self._G,
                                           self._splits, stream)
            self._core.sgd_update_fused(
                self.w.data_ptr(), self.g.data_ptr(), self.k_dev.data_ptr(),
                cfg.gamma, 1.0 / cfg.par_recs, cfg.num_workers, cfg.d,
                stream)

    # ---- overlap-mode machinery (ASGD dense) ------------------------------
    def _prime_lists(self) -> None:
        """Establish the invariant: list[cur] holds rows for the CURRENT
        k_dev (key k+1); scan_round == k+2."""
        cfg, sh = self.cfg, self.shard
        stream = torch.cuda.current_stream().cuda_stream
        kh = int(self.k_dev.item())
        self._count[self._cur].zero_()
        self._core.scan_rows(sh.y.data_ptr(),
                             self._rowlist[self._cur].data_ptr(),
                             self._ylist[self._cur].data_ptr(),
                             self._count[self._cur].data_ptr(), 0,
                             sh.n_rows, cfg.seed, kh + 1, sh.row_start,
                             cfg.batch_rate, stream)
        self._scan_round.fill_(kh + 2)
        torch.cuda.synchronize()

    def _overlap_compute_part(self) -> None:
        """grad(list[cur]) -> reduce -> fused update (k++), current stream."""
        cfg, sh = self.cfg, self.shard
        stream = torch.cuda.current_stream().cuda_stream
        cur = self._cur
        self._core.grad_dense_list(
            sh.X.data_ptr(), self.w.data_ptr(), self.g_part.data_ptr(),
            self._rowlist[cur].data_ptr(), self._ylist[cur].data_ptr(),
            self._count[cur].data_ptr(), sh.n_rows, cfg.d, self._obj_code,
            1 if sh.X.dtype == torch.bfloat16 else 0, stream)
        # fused reduce+update: sums partials, applies the step, and the
        # last-finishing block advances k (atomic ticket)
        self._core.sgd_reduce_update(
            self.g_part.data_ptr(), self.w.data_ptr(),
            self.k_dev.data_ptr(), self._ticket.data_ptr(), cfg.gamma,
            1.0 / cfg.par_recs, cfg.num_workers, cfg.d, self._G,
            self._splits, stream)

    def _overlap_scan_part(self, nxt: int) -> None:
        """memset count[nxt] -> scan(list[nxt]) -> bump scan_round, on the
        CURRENT stream (caller picks main or side stream)."""
        cfg, sh = self.cfg, self.shard
        stream = torch.cuda.current_stream().cuda_stream
        self._count[nxt].zero_()
        self._core.scan_rows(sh.y.data_ptr(), self._rowlist[nxt].data_ptr(),
                             self._ylist[nxt].data_ptr(),
                             self._count[nxt].data_ptr(),
                             self._scan_round.data_ptr(), sh.n_rows,
                             cfg.seed, 0, sh.row_start, cfg.batch_rate,
                             stream)
        self._core.bump_counter(self._scan_round.data_ptr(), stream)

    def _tail_round(self) -> None:
        """One sequential round preserving the list invariant."""
        nxt = self._cur ^ 1
        self._overlap_compute_part()
        self._overlap_scan_part(nxt)
        self._cur = nxt

    def _capture_overlap(self) -> None:
        state = self._save_state()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._prime_lists()
            self._tail_round()   # warm every kernel
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._restore_state(state)
        self._cur = 0
        self._prime_lists()
        g = torch.cuda.CUDAGraph()
        main = torch.cuda.current_stream()
        with torch.cuda.graph(g):
            main = torch.cuda.current_stream()
            cur = 0
            for it in range(self.unroll):
                nxt = cur ^ 1
                # side stream: scan round r+1 into list[nxt]
                self._sideB.wait_stream(main) if it == 0 else None
                if it > 0:
                    self._sideB.wait_event(self._ev_grad[nxt])
                with torch.cuda.stream(self._sideB):
                    self._overlap_scan_part(nxt)
                    self._ev_scan[nxt].record(self._sideB)
                # main stream: compute round r from list[cur]
                if it > 0:
                    main.wait_event(self._ev_scan[cur])
                saved = self._cur
                self._cur = cur
                self._overlap_compute_part()
                self._cur = saved
                self._ev_grad[cur].record(main)
                cur = nxt
            main.wait_stream(self._sideB)
        self._graph = g
        # capture executes nothing: state still = primed state for cur=0
        torch.cuda.synchronize()

    def _capture(self) -> None:
        # warm the kernels outside capture, then roll state back
        state = self._save_state()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._launch_round()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._restore_state(state)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(self.unroll):
                self._launch_round()
        self._graph = g
        self._restore_state(state)
        torch.cuda.synchronize()

    def _save_state(self):
        st = [self.w.clone(), self.g.clone(), self.k_dev.clone()]
        if self.alpha is not None:
            st += [self.alpha.clone(), self.alpha_bar.clone()]
        return st

    def _restore_state(self, st):
        self.w.copy_(st[0]); self.g.copy_(st[1]); self.k_dev.copy_(st[2])
        if self.alpha is not None:
            self.alpha.copy_(st[3]); self.alpha_bar.copy_(st[4])

    def step_rounds(self, n: int) -> None:
        """Advance n rounds (graph replays + per-round tail)."""
        if self._graph is None:
            if self._overlap:
                self._capture_overlap()
            else:
                self._capture()
        if self._overlap:
            # the graph is captured for buffer parity cur==0 and an even
            # unroll (round-trips the parity); odd tails re-align first
            while n > 0:
                if self._cur != 0 or n < self.unroll:
                    self._tail_round()
                    n -= 1
                else:
                    self._graph.replay()
                    n -= self.unroll
            return
        full, rem = divmod(n, self.unroll)
        for _ in range(full):
            self._graph.replay()
        for _ in range(rem):
            self._launch_round()

    def run(self, num_iterations: int,
            snapshot_every: Optional[int] = None,
            start_time: Optional[float] = None
            ) -> List[Tuple[int, torch.Tensor]]:
        """Run to completion; optionally snapshot (ms, w) every
        ``snapshot_every`` applied updates (the optVars loss-curve mechanism,
        reference SparkASGDThread.scala:195-198)."""
        t0 = start_time or time.perf_counter()
        opt_vars: List[Tuple[int, torch.Tensor]] = []
        if snapshot_every:
            opt_vars.append((0, self.w.detach().cpu().clone()))
        done = 0
        while done < num_iterations:
            chunk = (min(snapshot_every, num_iterations - done)
                     if snapshot_every else num_iterations - done)
            self.step_rounds(chunk)
            done += chunk
            if snapshot_every:
                torch.cuda.synchronize()
                ms = int((time.perf_counter() - t0) * 1000)
                opt_vars.append((ms, self.w.detach().cpu().clone()))
        torch.cuda.synchronize()
        return opt_vars

    def bench(self, warmup: int, steps: int) -> Tuple[float, float]:
        """Timed exactly-K-steps contract: returns (t0, t1) wall stamps
        bracketing ``steps`` applied updates after ``warmup`` untimed ones,
        with a device synchronize on both sides."""
        self.step_rounds(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.step_rounds(steps)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return t0, t1

    @property
    def k(self) -> int:
        return int(self.k_dev.item())
