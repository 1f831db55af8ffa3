"""Python adapter for the native C++ event-loop engine
(csrc/engine_native.cpp): multi-worker bounded-staleness async on one GPU
with zero Python in the round loop.

Each worker owns a shard, a weight-snapshot buffer (the
versioned-broadcast semantic), a gradient accumulator and a pinned-host
completion flag; the C++ loop does wave dispatch (one kernel per quorum
wave) -> pinned-flag poll -> tau filter -> batched fused update ->
quorum-gated redispatch, including the reference's straggler model and
calibration (csrc/engine_native.cpp header for the measured evolution).
Use for GPU multi-worker configs (the threaded Python engine stays for
CPU tests and as the semantics oracle).

``cfg.sync`` selects the engine's separate synchronous path
(``native_sync_run``; algo asgd | asaga | mllib): one stream-ordered round
per iteration — gradient wave over all P workers reading ``w`` itself, one
fused round-update kernel, one host wait — with the same straggler model
as SyncEngine + DelayInjector. Workers own no weight-snapshot buffer
there, and the SAGA history must be device-resident.

Checkpoint / resume (both modes): the C++ loop ends every run — and, with
``cfg.checkpoint_every``, reaches every checkpoint — in a quiescent state
in which ``w``, ``alpha_bar`` and ``alpha_tables`` describe exactly iterate
k; ``capture_state`` / ``restore_state`` move that state through the
``engine/checkpoint.py`` schema shared with the other engines."""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .config import EngineConfig, check_penalties
from .worker import Shard

_OBJ = {"lsq": 0, "logistic": 1, "hinge": 2}  # csrc/link.h
_ALGO = {"asgd": 0, "asaga": 1}
_SYNC_MODE = {"asgd": 0, "asaga": 1, "mllib": 2}


class NativeLocalEngine:
    def __init__(self, cfg: EngineConfig, shards: List[Shard],
                 device: torch.device):
        # configuration errors first: nothing is imported or allocated yet
        check_penalties(cfg.l2, cfg.l1)
        if cfg.sync:
            assert cfg.algo in _SYNC_MODE, (
                f"native sync engine: unknown algo {cfg.algo!r}")
            assert cfg.history_placement != "host", (
                "native sync engine keeps the SAGA history on the device: "
                "history_placement='host' (spill) is async-only")
        assert device.type == "cuda", "native engine is GPU-only"
        from .. import _hip_core
        self._core = _hip_core
        self.cfg = cfg
        self.device = device
        self.shards = shards
        d = cfg.d
        self.w = torch.zeros(d, dtype=torch.float32, device=device)
        self.alpha_bar = torch.zeros(d, dtype=torch.float32, device=device)
        self._bufs = []
        self._keep = []   # keep tensors alive across the native call
        self.alpha_tables: List[torch.Tensor] = []
        for sh in shards:
            # sync mode: every worker reads w itself (no snapshot buffer)
            wbuf = self.w if cfg.sync else torch.zeros(
                d, dtype=torch.float32, device=device)
            g = torch.zeros(d, dtype=torch.float32, device=device)
            ctr = torch.zeros(2, dtype=torch.int32, device=device)
            wd = dict(sparse=sh.is_sparse, y=sh.y.data_ptr(),
                      wbuf=wbuf.data_ptr(), g=g.data_ptr(),
                      ctr=ctr.data_ptr(), n_rows=sh.n_rows,
                      row_start=sh.row_start, x_is_bf16=0)
            keep = [wbuf, g, ctr]
            if sh.is_sparse:
                wd.update(indptr=sh.indptr.data_ptr(),
                          indices=sh.indices.data_ptr(),
                          values=sh.values.data_ptr())
                wd["x_is_bf16"] = 1 if sh.values.dtype == torch.bfloat16 else 0
            else:
                wd.update(X=sh.X.data_ptr())
                wd["x_is_bf16"] = 1 if sh.X.dtype == torch.bfloat16 else 0
            if cfg.algo == "asaga":
                cap = sh.n_rows if cfg.batch_rate >= 1.0 else min(
                    sh.n_rows, int(cfg.batch_rate * sh.n_rows * 3) + 4096)
                idx_out = torch.zeros(cap, dtype=torch.int32, device=device)
                e_out = torch.zeros(cap, dtype=torch.float32, device=device)
                if cfg.history_placement == "host":
                    # spill mode (BASELINE config 5): master table pinned in
                    # host DRAM; the device table becomes staging that the
                    # C++ loop refreshes per round via scan_rows +
                    # alpha_gather (mask-keyed, ~rate of the table)
                    master = torch.zeros(sh.n_rows, dtype=torch.float32,
                                         device="cpu").pin_memory()
                    alpha = torch.zeros(sh.n_rows, dtype=torch.float32,
                                        device=device)
                    srows = torch.empty(cap, dtype=torch.int32,
                                        device=device)
                    sylist = torch.empty(cap, dtype=torch.float32,
                                         device=device)
                    scnt = torch.zeros(1, dtype=torch.int32, device=device)
                    wd.update(alpha_host=master.data_ptr(),
                              srows=srows.data_ptr(),
                              sylist=sylist.data_ptr(),
                              scnt=scnt.data_ptr())
                    keep += [master, srows, sylist, scnt]
                    self.alpha_tables.append(master)
                else:
                    alpha = torch.zeros(sh.n_rows, dtype=torch.float32,
                                        device=device)
                    self.alpha_tables.append(alpha)
                wd.update(alpha=alpha.data_ptr(), idx_out=idx_out.data_ptr(),
                          e_out=e_out.data_ptr(), saga_cap=cap)
                keep += [alpha, idx_out, e_out]
            self._keep.extend(keep)
            self._bufs.append(wd)
        # start state of the next run(): None = fresh (k = clock = 0);
        # restore_state() arms it, run() consumes it
        self._start: Optional[Dict] = None

    # -- checkpoint / resume (engine/checkpoint.py schema) -------------------

    def capture_state(self, k: int, clock: int,
                      delay_state: Optional[Dict] = None) -> Dict:
        """The engine's tensors as a ``checkpoint.capture_state`` dict (CPU
        clones; in spill mode the pinned master IS the table). Only valid
        at a quiescent point: between run() calls, or inside the C++ loop's
        checkpoint callback, which supplies ``k``, ``clock`` and the
        straggler-calibration state (stored under ``native_delay``; the
        other engines ignore the key)."""
        state = {
            "k": int(k),
            "current_time": int(clock),
            "w": self.w.detach().cpu().clone(),
            "alpha_bar": (self.alpha_bar.detach().cpu().clone()
                          if self.cfg.algo == "asaga" else None),
            "cfg": self.cfg.__dict__.copy(),
            "alpha": {wid: t.detach().cpu().clone()
                      for wid, t in enumerate(self.alpha_tables)},
        }
        if delay_state is not None:
            state["native_delay"] = {
                "avg_delay_ms": float(delay_state["avg_delay_ms"]),
                "delay_flag": bool(delay_state["delay_flag"]),
                "cul_time_ms": float(delay_state["cul_time_ms"]),
                "cul_count": int(delay_state["cul_count"])}
        return state

    def restore_state(self, state: Dict) -> None:
        """Copy a checkpoint into the engine's tensors and arm the next
        run() to continue from its k, arrival clock and (when the file
        carries one) straggler-calibration state."""
        from .checkpoint import check_compatible
        missing = check_compatible(
            state, self.cfg, alpha_ids=range(len(self.alpha_tables)),
            stacklevel=3)
        self.w.copy_(state["w"].to(self.device, dtype=torch.float32))
        if self.cfg.algo == "asaga" and state.get("alpha_bar") is not None:
            self.alpha_bar.copy_(
                state["alpha_bar"].to(self.device, dtype=torch.float32))
        for wid, table in enumerate(self.alpha_tables):
            if wid not in missing:
                table.copy_(state["alpha"][wid].to(table.device,
                                                   dtype=torch.float32))
        self._start = dict(k0=int(state["k"]),
                           clock0=int(state["current_time"]))
        if state.get("native_delay") is not None:
            self._start["delay_state"] = dict(state["native_delay"])

    def run(self, num_iterations: Optional[int] = None,
            mark_lo: int = -1, mark_hi: int = -1,
            max_wall_s: float = 1800.0,
            snapshot_every: int = 0) -> Dict:
        """snapshot_every > 0 records (ms, w) optVars every that many
        applied updates (the reference's printer_freq loss-curve mechanism)
        into a device ring, returned as res['opt_vars']. In sync mode
        iterations, marks and the snapshot cadence count ROUNDS (one update
        per round), as SyncEngine does.

        After restore_state() the run continues from the restored k
        (``num_iterations`` stays the TOTAL target; times restart at 0 and
        opt_vars[0] is the restored w). With ``cfg.checkpoint_every > 0 and
        cfg.checkpoint_path`` the loop quiesces whenever k crosses a
        multiple of checkpoint_every and the state is written with
        ``checkpoint.save_state``."""
        cfg = self.cfg
        iters = num_iterations or cfg.num_iterations
        start, self._start = self._start, None
        w_start = (self.w.detach().cpu().clone() if start is not None
                   else torch.zeros(cfg.d))
        snap_ring = None
        snap_cap = 0
        if snapshot_every > 0:
            snap_cap = iters // snapshot_every + 2
            snap_ring = torch.zeros(snap_cap, cfg.d, dtype=torch.float32,
                                    device=self.device)
        conf = dict(N=cfg.N, d=cfg.d, P=cfg.num_workers, iters=iters,
                    gamma=cfg.gamma, rate=cfg.batch_rate,
                    bucket_ratio=cfg.bucket_ratio, taw=cfg.taw,
                    seed=cfg.seed,
                    algo=(int(cfg.algo == "asaga") if cfg.sync
                          else _ALGO[cfg.algo]),
                    objective=_OBJ[cfg.objective], coeff=cfg.delay_coeff,
                    calib_window=cfg.calib_factor * cfg.num_workers,
                    mark_lo=mark_lo, mark_hi=mark_hi,
                    max_wall_s=max_wall_s, snap_every=snapshot_every,
                    snap_ring=snap_ring.data_ptr() if snap_ring is not None
                    else 0, snap_cap=snap_cap, l2=float(cfg.l2),
                    l1=float(cfg.l1))
        if start is not None:
            conf.update(start)
        ckpt_cb = None
        if cfg.checkpoint_every > 0 and cfg.checkpoint_path:
            from .checkpoint import save_state
            conf["ckpt_every"] = int(cfg.checkpoint_every)

            def ckpt_cb(info):
                # called by the C++ loop at a quiescent point, GIL held,
                # every engine stream idle
                save_state(cfg.checkpoint_path,
                           self.capture_state(info["k"], info["clock"],
                                              info["delay_state"]))
        torch.cuda.synchronize()
        if cfg.sync:
            res = self._core.native_sync_run(conf, self._bufs,
                                             self.w.data_ptr(),
                                             self.alpha_bar.data_ptr(),
                                             _SYNC_MODE[cfg.algo], ckpt_cb)
        else:
            res = self._core.native_local_run(conf, self._bufs,
                                              self.w.data_ptr(),
                                              self.alpha_bar.data_ptr(),
                                              ckpt_cb)
        torch.cuda.synchronize()
        res["k0"] = start["k0"] if start is not None else 0
        if snapshot_every > 0:
            snaps = res["snap_ms"]
            res["opt_vars"] = [(0, w_start)] + [
                (int(ms), snap_ring[i].cpu().clone())
                for i, ms in enumerate(snaps)]
        return res

    def bench(self, warmup: int, steps: int,
              max_wall_s: float = 1800.0,
              snapshot_every: int = 0) -> Tuple[float, Dict]:
        """Exactly-K-steps contract: the native loop stamps wall times when
        k crosses warmup and warmup+steps (after a server-stream sync).
        snapshot_every > 0 also records the optVars loss curve (a 3 KB D2D
        copy on the server stream every that many applied updates)."""
        res = self.run(num_iterations=warmup + steps + 1,
                       mark_lo=warmup, mark_hi=warmup + steps,
                       max_wall_s=max_wall_s, snapshot_every=snapshot_every)
        t0, t1 = res["mark_lo_t"], res["mark_hi_t"]
        if not (t1 > t0 > 0):
            raise RuntimeError(f"native bench marks missing: {res}")
        return t1 - t0, res
