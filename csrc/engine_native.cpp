// Native async parameter-server engine (single GPU, multi-worker).
//
// The MI355X-native replacement for the reference's driver main loop +
// updater thread + executor pool (SparkASGDThread.scala:153-345,
// Executor.scala TaskRunner) for co-located workers: ONE host thread drives
// an event loop over per-worker HIP streams —
//
//   dispatch:    each quorum WAVE launches as ONE kernel
//                (grad_dense_wave_kernel / grad_csr_wave_kernel over a
//                device slot table, SAGA commits batched into one
//                commit+staging-reset kernel, spill refresh as
//                scan/gather wave kernels) on a rotating stream pool; the
//                batched update kernel writes the redispatching workers'
//                weight snapshots (versioned-broadcast semantic), so the
//                whole wave costs a handful of launches instead of 2-5
//                per worker. First dispatches and straggler releases use
//                the per-worker singleton path;
//   poll:        EVENT-FREE — the grad kernel's last block publishes the
//                round serial to a pinned-host line (publish_done,
//                kernels.hip) and the host polls plain memory;
//   accept:      tau filter; accepted gradients accumulate into ONE
//                elementwise-sequential multi-update kernel per sweep;
//                requeue; quorum-gated redispatch;
//   delay:       the reference's straggler model (cloud long-tail / coeff;
//                straggler.h, shared with the dist and resident engines),
//                implemented as host-side due-times on the dispatch queue —
//                no thread sleeps, no locks, no GIL (released for the whole
//                run).
//
// This is the same control plane as engine/local.py with the thread
// handoffs (~100 us each under the GIL) replaced by sub-us flag reads.
// Measured evolution on the flagship config (profiles/r02_wave_dispatch.md):
// 39.9k updates/s (r01, per-round launches + events) -> 87.2k (batched
// updates) -> 103k (event-free) -> 188k (wave dispatch, interleaved
// mapping, wave-aware grid sizing) -> 370k (gradient kernel at 4 blocks
// per CU instead of 1, row-bounded loads; profiles/r04_grad_occupancy.md).
// The RCCL multi-GPU server reuses this
// loop shape with peers instead of streams (csrc/server_dist.cpp).
//
// Synchronous mode (run_sync; asgd-sync, asaga-sync, sgd-mllib) is a
// SEPARATE, plain path — not the async loop with gate=P/taw=0 — so the
// async arm and the sync arm of a comparison share one substrate (the
// reference runs both through ASYNCreduce, SparkASGDSync.scala:239-277).
// One round = one iteration k, everything on the ONE server stream:
//
//   [SAGA, k>0: commit wave of round k-1's staged history]
//   gradient wave over ALL P slots reading w itself (no snapshot copies)
//   [host sleeps out the straggler delay, if any]
//   sync_round_update_kernel (fixed-order sum, step, zero g, reset
//   counters, optional fused optVars snapshot)
//   hipEventRecord -> host polls hipEventQuery under the stall watchdog
//
// Placement of the barrier: exactly ONE host wait per round, behind the
// round's update; round k+1 is enqueued only after round k has finished
// on the GPU. No completion flag is ever read (the gradient kernels get a
// null done_flag), and every time that describes a round — snapshot
// stamps, bench marks, calibration samples, elapsed — is taken after that
// wait, so loss-curve times are completion times, not enqueue times. The
// wall cap is checked between rounds (as the Python SyncEngine does); a
// round in flight is bounded by stall_s and throws with its k.
//
// Checkpoint / resume (both modes). Every run ENDS quiescent: after the
// last time stamp, accepted-but-uncommitted SAGA history is committed and
// the gradient buffers of dropped or rejected rounds are zeroed, so w,
// alpha_bar and the history tables describe exactly iterate k. A run may
// START at conf k0/clock0 (+ delay_state) instead of zero — step sizes,
// Philox round keys, the snapshot cadence, the calibration window and the
// marks all key on the absolute k, and iters stays the total target. With
// conf ckpt_every > 0 the loop reaches the same quiescent state whenever k
// crosses a multiple (async: stop dispatching, book the rounds in flight,
// flush; sync: commit the round's staged history) and calls a Python
// callable with {k, clock, delay_state} under the GIL; Python owns the
// tensors and writes the file (engine/native.py, engine/checkpoint.py).
// Off, the feature costs one integer compare per applied update.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime.h>

#define HIP_CHECK_WHO "native engine"
#include "grad_wave.h"
#include "host_util.h"
#include "launchers.h"
#include "multi_update.h"
#include "straggler.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <deque>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace py = pybind11;

namespace {

struct WorkerBuf {
  // device pointers supplied by Python (torch tensors kept alive there)
  uintptr_t X = 0, indptr = 0, indices = 0, values = 0, y = 0;
  uintptr_t alpha = 0, idx_out = 0, e_out = 0;  // SAGA staging
  // host-spill mode (BASELINE config 5): alpha_host = pinned master table
  // (device-visible); alpha above becomes the device staging table that
  // scan_rows + alpha_gather refresh at the round's sampled rows
  uintptr_t alpha_host = 0, srows = 0, sylist = 0, scnt = 0;
  uintptr_t wbuf = 0, g = 0, ctr = 0;           // snapshot, grad, counters
  long n_rows = 0, row_start = 0;
  bool sparse = false;
  int x_is_bf16 = 0;
  // runtime
  hipStream_t stream = nullptr;
  // event-free completion: the grad kernel's last block release-stores
  // round_serial into pinned host memory (publish_done in kernels.hip);
  // the host event loop polls plain memory instead of hipEventQuery
  volatile unsigned long long* done_flag = nullptr;  // pinned host, 1 line
  unsigned long long* done_arr = nullptr;  // device arrival ctr (monotonic)
  unsigned long long round_serial = 0;
  bool busy = false;
  // a round is actually executing on the GPU. Distinct from busy: a
  // straggler-DELAYED worker is busy (occupied) but not in flight, and its
  // done flag still holds the previous round's serial — polling it would
  // double-book that round (latent in the event-based loop too, where the
  // completed event also stayed signaled; made explicit here)
  bool in_flight = false;
  int ts = 0;        // arrival clock at dispatch
  long k_submit = 0; // round index at dispatch
  bool pending_commit = false;
  int saga_cap = 0;  // staging capacity (commit grid bound, SAGA only)
  double submit_t = 0, finish_t = 0, waiting_ms = 0;
  bool g_dirty = false;   // gradient buffer holds a rejected round's sums
  long tasks = 0;
};

struct EngineCfg {
  long N = 0;
  int d = 0, P = 1;
  long iters = 0;
  double gamma = 0.01, rate = 0.01, bucket_ratio = 0.7;
  long taw = 1 << 30;
  uint64_t seed = 42;
  int algo = 0;       // 0 asgd, 1 asaga
  int objective = 0;  // 0 lsq, 1 logistic, 2 hinge (link.h)
  double coeff = 0.0; // delay model
  long calib_window = 0;
  long mark_lo = -1, mark_hi = -1;
  double max_wall_s = 3600.0;
  double stall_s = 60.0;     // watchdog: abort if no completion for this long
  long snap_every = 0;       // optVars cadence (reference printer_freq)
  uintptr_t snap_ring = 0;   // [snap_cap][d] device ring
  long snap_cap = 0;
  double l2 = 0.0, l1 = 0.0;  // elastic-net penalties (0/0: legacy kernels)
  // resume / checkpoint (all optional; absent keys leave a fresh run)
  long k0 = 0;          // initial k (iters stays the TOTAL target)
  int clock0 = 0;       // initial arrival clock
  long ckpt_every = 0;  // checkpoint when k crosses a multiple (0 = off)
};

// A host vector as a device table, and its release (null-safe, nulls p).
template <class T>
T* upload_table(const std::vector<T>& h) {
  T* dev = nullptr;
  HIP_CHECK(hipMalloc((void**)&dev, sizeof(T) * h.size()));
  HIP_CHECK(hipMemcpy(dev, h.data(), sizeof(T) * h.size(),
                      hipMemcpyHostToDevice));
  return dev;
}

template <class T>
void free_table(T*& p) {
  if (p) HIP_CHECK(hipFree(p));
  p = nullptr;
}

struct NativeEngine {
  EngineCfg cfg;
  std::vector<WorkerBuf> ws;
  uintptr_t w = 0, alpha_bar = 0;
  hipStream_t sstream = nullptr;  // server stream
  hipEvent_t update_ev = nullptr;
  // server state
  long k = 0;
  int clock = 0;  // arrival clock (ASYNCcontext.CurrentTime)
  std::deque<int> pendingq;
  std::deque<std::pair<double, int>> delayed;  // (due time, worker)
  long applied = 0, rejected = 0;
  long max_staleness_seen = -1;
  // delay calibration (reference :177-186,:247-252); the straggler model
  // itself is straggler.h
  straggler::Calibration cal;
  double mark_lo_t = 0, mark_hi_t = 0;
  std::vector<double> snap_ms;  // host stamps for the optVars snapshots
  double run_t0 = 0;
  // batched-update machinery
  float** g_tab_dev = nullptr;     // device table: worker id -> g pointer
  volatile unsigned long long* flags_host = nullptr;
  unsigned long long* arr_dev = nullptr;
  // wave dispatch (dense ASGD): per-worker invariant table + stream
  GradWaveSlot* slots_dev = nullptr;
  CsrWaveSlot* csr_slots_dev = nullptr;
  CommitSlot* commit_slots_dev = nullptr;
  bool wave_spill = false;
  // pool of wave streams: consecutive waves overlap like the per-worker
  // streams did (same-worker overlap is impossible — in_flight guard)
  static constexpr int NWSTREAM = 8;
  hipStream_t wstreams[NWSTREAM] = {};
  unsigned wave_rr = 0;
  int wave_interleave = 0;
  hipStream_t cur_wst = nullptr;
  int wave_bper = 0;
  long wave_max_rows = 0;
  bool wave_ok = false;
  float** wbuf_tab_dev = nullptr;  // device table: worker id -> wbuf pointer
  double inv_batch = 0, inv_N = 0;
  // synchronous mode (run_sync): sample-counter pointer table + the update
  // kernel's counter-reset ticket
  int** ctr_tab_dev = nullptr;
  int* sync_ticket_dev = nullptr;
  bool sync_staged = false;  // the last sync SAGA round's history is staged
  std::vector<int> all_wids;  // 0..P-1: a sync round spans every worker
  // periodic checkpoint: append_accepted / the sync loop compare k against
  // next_ckpt (LONG_MAX when off — the only cost of the feature being off)
  py::object ckpt_cb;  // Python callable({k, clock, delay_state}); GIL-guarded
  long next_ckpt = std::numeric_limits<long>::max();
  bool ckpt_due = false;
  double ckpt_t_begin = 0;
  long checkpoints = 0;
  double checkpoint_ms = 0;  // host time quiesced, callback included

  // Start state (fresh run: all zeros, as before).
  void arm_start() {
    k = cfg.k0;
    clock = cfg.clock0;
    if (cfg.ckpt_every > 0)
      next_ckpt = (k / cfg.ckpt_every + 1) * cfg.ckpt_every;
  }

  double delay_ms_for(int wid, long round_k) const {
    return straggler::delay_ms(cfg.P, cfg.coeff, cfg.seed, cal.avg_delay_ms,
                               cal.delay_flag, wid, round_k);
  }

  int gate() const {
    return std::max(1, (int)std::floor(cfg.P * cfg.bucket_ratio));
  }

  int available() const {
    int n = 0;
    for (auto& wk : ws)
      if (!wk.busy) ++n;
    return n;
  }

  void launch_grad(WorkerBuf& wk, long round_key) {
    // g is zeroed by the fused update of the worker's ACCEPTED previous
    // round; only a rejected round leaves it dirty. ASGD never reads the
    // sampled count, so its ctr memset is skipped.
    if (wk.g_dirty) {
      HIP_CHECK(hipMemsetAsync((void*)wk.g, 0, (size_t)cfg.d * 4, wk.stream));
      wk.g_dirty = false;
    }
    if (cfg.algo == 1)
      HIP_CHECK(hipMemsetAsync((void*)wk.ctr, 0, 8, wk.stream));
    if (cfg.algo == 1 && wk.alpha_host) {
      // spill refresh: recompute the round's Philox row set on-device and
      // gather ONLY those entries from the pinned master into the staging
      // table the gradient kernel reads (ordered after this worker's
      // commit scatter on the same stream)
      HIP_CHECK(hipMemsetAsync((void*)wk.scnt, 0, 4, wk.stream));
      launch_scan_rows((const float*)wk.y, (int*)wk.srows,
                       (float*)wk.sylist, (int*)wk.scnt, nullptr, wk.n_rows,
                       cfg.seed, (uint32_t)round_key, (uint64_t)wk.row_start,
                       cfg.rate, wk.stream);
      launch_alpha_gather((float*)wk.alpha, (const float*)wk.alpha_host,
                          (const int*)wk.srows, (const int*)wk.scnt,
                          wk.saga_cap, wk.stream);
      HIP_CHECK(hipGetLastError());
    }
    if (cfg.algo == 1) {
      if (wk.sparse)
        launch_saga_grad_csr_flag(
            (const int*)wk.indptr, (const int*)wk.indices,
            (const void*)wk.values, (const float*)wk.y,
            (const float*)wk.wbuf, (float*)wk.alpha, (float*)wk.g,
            (int*)wk.ctr, (int*)wk.idx_out, (float*)wk.e_out,
            (int*)(wk.ctr + 4), nullptr, 0, wk.n_rows, cfg.seed,
            (uint32_t)round_key, (uint64_t)wk.row_start, cfg.rate,
            cfg.objective, wk.x_is_bf16, wk.stream,
            (unsigned long long*)wk.done_flag, wk.round_serial,
            wk.done_arr);
      else
        launch_saga_grad_dense_flag(
            (const void*)wk.X, (const float*)wk.y, (const float*)wk.wbuf,
            (float*)wk.alpha, (float*)wk.g, nullptr, (int*)wk.ctr,
            (int*)wk.idx_out, (float*)wk.e_out, (int*)(wk.ctr + 4), nullptr,
            0, wk.n_rows, cfg.d, cfg.seed, (uint32_t)round_key,
            (uint64_t)wk.row_start, cfg.rate, cfg.objective, wk.x_is_bf16,
            wk.stream, (unsigned long long*)wk.done_flag, wk.round_serial,
            wk.done_arr);
    } else {
      if (wk.sparse)
        launch_grad_csr_flag(
            (const int*)wk.indptr, (const int*)wk.indices,
            (const void*)wk.values, (const float*)wk.y,
            (const float*)wk.wbuf, (float*)wk.g, (int*)wk.ctr, nullptr,
            wk.n_rows, cfg.seed, (uint32_t)round_key,
            (uint64_t)wk.row_start, cfg.rate, cfg.objective, wk.x_is_bf16,
            wk.stream, (unsigned long long*)wk.done_flag, wk.round_serial,
            wk.done_arr);
      else
        launch_grad_dense_flag(
            (const void*)wk.X, (const float*)wk.y, (const float*)wk.wbuf,
            (float*)wk.g, nullptr, (int*)wk.ctr, nullptr, wk.n_rows, cfg.d,
            cfg.seed, (uint32_t)round_key, (uint64_t)wk.row_start, cfg.rate,
            cfg.objective, wk.x_is_bf16, wk.stream,
            (unsigned long long*)wk.done_flag, wk.round_serial,
            wk.done_arr);
    }
    HIP_CHECK(hipGetLastError());
  }

  // Commit the staged SAGA history of workers wids[0..n) on ``stream`` (the
  // count is read on-device — no D2H sync). With the commit slot table (wave
  // mode) that is ONE commit + staging-reset kernel: the gradient ran on a
  // wave stream, so the staging must be read with the RMW-load commit kernel
  // (normal loads could hit a stale L2 line across the stream boundary).
  // Otherwise one launch per worker; spill mode scatters straight into the
  // pinned master table. The caller clears its own pending mark.
  void commit_history(const int* wids, int n, hipStream_t stream) {
    if (commit_slots_dev) {
      CsrCommitCmd cc;
      cc.n = n;
      cc.bper = 16;
      for (int i = 0; i < n; ++i) {
        cc.wid[i] = wids[i];
        cc.do_commit[i] = 1;
      }
      if (n > 0) {
        launch_saga_commit_wave(commit_slots_dev, &cc, stream);
        HIP_CHECK(hipGetLastError());
      }
      return;
    }
    for (int i = 0; i < n; ++i) {
      WorkerBuf& wk = ws[wids[i]];
      float* dst = (float*)(wk.alpha_host ? wk.alpha_host : wk.alpha);
      launch_saga_commit_devn(dst, (const int*)wk.idx_out,
                              (const float*)wk.e_out,
                              (const int*)(wk.ctr + 4), wk.saga_cap, stream);
      HIP_CHECK(hipGetLastError());
    }
  }

  // Dispatch bookkeeping of the per-worker and the wave path: the submit
  // stamps, then the serial the grad kernel's last block will publish.
  void book_submit(WorkerBuf& wk, double t_now) {
    if (wk.finish_t == 0) wk.finish_t = t_now;  // first dispatch: no wait
    wk.waiting_ms += (t_now - wk.finish_t) * 1000.0;
    wk.submit_t = t_now;
    wk.busy = true;
    wk.ts = clock;
    wk.k_submit = k;
  }

  void book_in_flight(WorkerBuf& wk, int wid) {
    if (wk.in_flight)
      throw std::runtime_error(
          "native engine invariant: dispatch while a round is in flight "
          "(worker " + std::to_string(wid) + ")");
    wk.round_serial += 1;
    wk.in_flight = true;
  }

  // Common dispatch tail: SAGA commit of the previous accepted round (count
  // read on-device — no D2H sync), waiting-time bookkeeping, grad launch
  // ordered after the latest applied update, completion event.
  // ``copy_w``: true -> snapshot w with a hipMemcpyAsync on the worker
  // stream (first dispatch / delayed release); false -> the batched update
  // kernel already wrote this worker's wbuf on sstream (the common path).
  void dispatch_impl(int wid, double t_now, bool copy_w) {
    WorkerBuf& wk = ws[wid];
    // accept-gated SAGA history commit from the worker's previous round
    if (cfg.algo == 1 && wk.pending_commit)
      commit_history(&wid, 1, wk.stream);
    wk.pending_commit = false;
    book_submit(wk, t_now);
    // versioned weights: the worker computes against the w it was
    // dispatched with (ASYNCbroadcast semantics) — ordered after the
    // latest applied update either way
    HIP_CHECK(hipStreamWaitEvent(wk.stream, update_ev, 0));
    if (copy_w)
      HIP_CHECK(hipMemcpyAsync((void*)wk.wbuf, (const void*)w,
                               (size_t)cfg.d * 4, hipMemcpyDeviceToDevice,
                               wk.stream));
    book_in_flight(wk, wid);
    launch_grad(wk, wk.k_submit + 1);  // reference seed+k+1
    // no hipEventRecord: completion = *done_flag == round_serial (plain
    // pinned-memory read, ~0 host cost vs ~1-2 us per hipEventQuery)
  }

  void dispatch(int wid, double t_now) { dispatch_impl(wid, t_now, true); }

  // Wave-path bookkeeping: everything dispatch_impl does EXCEPT the grad
  // launch (the whole quorum wave launches as ONE grad_dense_wave_kernel).
  // ASGD-only: no SAGA commit to chain.
  void dispatch_book(int wid, double t_now) {
    WorkerBuf& wk = ws[wid];
    book_submit(wk, t_now);
    if (wk.g_dirty) {  // rejected round left sums; zero on the wave stream
      HIP_CHECK(hipMemsetAsync((void*)wk.g, 0, (size_t)cfg.d * 4,
                               cur_wst));
      wk.g_dirty = false;
    }
    book_in_flight(wk, wid);
  }

  void dispatch_wave(const std::vector<int>& ready, double t_now) {
    cur_wst = wstreams[wave_rr % NWSTREAM];
    wave_rr += 1;
    HIP_CHECK(hipStreamWaitEvent(cur_wst, update_ev, 0));
    if (commit_slots_dev) {
      // SAGA: one commit + staging-reset kernel for the whole wave,
      // stream-ordered before the wave's gradient kernel
      CsrCommitCmd cc;
      cc.n = 0;
      cc.bper = 16;
      for (int wid : ready) {
        cc.wid[cc.n] = wid;
        cc.do_commit[cc.n] = ws[wid].pending_commit ? 1 : 0;
        ws[wid].pending_commit = false;
        cc.n += 1;
      }
      if (cc.n > 0) {
        launch_saga_commit_wave(commit_slots_dev, &cc, cur_wst);
        HIP_CHECK(hipGetLastError());
      }
    }
    for (int wid : ready) dispatch_book(wid, t_now);
    launch_grad_wave(ready.data(), (int)ready.size(), cur_wst);
  }

  // One gradient wave over workers wids[0..n) on ``stream``, each at the
  // round key (k_submit + 1, reference seed+k+1) and completion serial its
  // WorkerBuf holds: the dense or the CSR wave kernel, by which slot table
  // setup_tables built.
  void launch_grad_wave(const int* wids, int n, hipStream_t stream) {
    if (n <= 0) return;
    GradWaveCmd cmd;
    cmd.n = n;
    cmd.bper = wave_bper;
    cmd.interleave = wave_interleave;
    for (int i = 0; i < n; ++i) {
      const WorkerBuf& wk = ws[wids[i]];
      cmd.wid[i] = wids[i];
      cmd.round_k[i] = (unsigned int)(wk.k_submit + 1);
      cmd.done_val[i] = wk.round_serial;
    }
    if (slots_dev) {
      if (wave_spill) {
        // spill refresh, stream-ordered: recompute the round's Philox row
        // sets, then gather those master entries into the staging tables
        // the gradient reads
        launch_scan_rows_wave(slots_dev, &cmd, cfg.seed, cfg.rate, stream);
        launch_alpha_gather_wave(slots_dev, &cmd, stream);
      }
      launch_grad_dense_wave(slots_dev, &cmd, wave_max_rows, cfg.d, cfg.seed,
                             cfg.rate, cfg.objective, ws[0].x_is_bf16,
                             cfg.algo == 1 ? 1 : 0, stream);
    } else {
      launch_grad_csr_wave(csr_slots_dev, &cmd, cfg.seed, cfg.rate,
                           cfg.objective, ws[0].x_is_bf16,
                           cfg.algo == 1 ? 1 : 0, stream);
    }
    HIP_CHECK(hipGetLastError());
  }

  // Pop every pending worker that may dispatch now: stragglers move to the
  // delayed queue with a due time, the rest land in ``ready`` (dispatched
  // after the batch flush writes their weight snapshots).
  void collect_ready(double t_now, std::vector<int>& ready) {
    if (pendingq.empty()) return;
    if (available() < gate()) return;
    // delay calibration activation (reference :247-252)
    cal.maybe_activate(k, cfg.calib_window);
    const size_t qn = pendingq.size();
    for (size_t i = 0; i < qn; ++i) {
      const int wid = pendingq.front();
      pendingq.pop_front();
      const double dly = delay_ms_for(wid, k) / 1000.0;
      if (dly > 0) {
        ws[wid].busy = true;  // occupied while "straggling"
        delayed.emplace_back(t_now + dly, wid);
      } else {
        ready.push_back(wid);
      }
    }
  }

  // Completion bookkeeping only (no launches): arrival clock, staleness,
  // EWMA, tau filter, requeue. The caller batches accepted gradients into
  // one multi_update kernel per poll sweep.
  bool book_completion(int wid, double t_now) {
    WorkerBuf& wk = ws[wid];
    wk.busy = false;
    wk.in_flight = false;
    wk.finish_t = t_now;
    wk.tasks += 1;
    const double rt = t_now - wk.submit_t;
    const int staleness = clock - wk.ts;  // arrival-clock staleness
    clock += 1;
    max_staleness_seen = std::max<long>(max_staleness_seen, staleness);
    // ASGD: completion-clock staleness <= taw (SparkASGDThread.scala:172).
    // ASAGA: k - ts <= taw with ts = the arrival clock at submit
    // (SparkASAGAThread.scala:191, raw-ts packing RDD.scala:1333) — matches
    // server.py accepts() and csrc/server_dist.cpp, NOT the applied-update
    // counter at submit (k_submit), which would diverge once rejections occur.
    const bool accept = (cfg.algo == 1) ? (k - wk.ts) <= cfg.taw
                                        : staleness <= cfg.taw;
    if (accept) {
      if (k < cfg.calib_window) cal.record(rt * 1000.0, 1);
    } else {
      rejected += 1;
      wk.pending_commit = false;
      wk.g_dirty = true;  // dispatch re-zeroes before the next round
    }
    pendingq.push_back(wid);
    return accept;
  }

  // -- batched update assembly (one kernel per poll sweep; elementwise-
  //    sequential application inside the kernel makes the result identical
  //    to launching the per-round update kernels back to back) ------------
  MultiUpdateArgs mu{};
  bool mu_vec4 = false;  // float4 form: d % 4 == 0, 16-byte-aligned buffers

  void flush_batch(const std::vector<int>* snap_targets) {
    size_t si = 0;
    const size_t total = snap_targets ? snap_targets->size() : 0;
    bool launched = false;
    while (true) {
      mu.m = 0;
      while (si < total && mu.m < MU_MAX)
        mu.sw[mu.m++] = (*snap_targets)[si++];
      if (mu.n == 0 && mu.m == 0) break;
      mu.algo = cfg.algo;
      launch_multi_update((float*)w, (float* const*)g_tab_dev,
                          (float* const*)wbuf_tab_dev, (float*)alpha_bar,
                          (float)cfg.gamma, (float)inv_batch, (float)inv_N,
                          cfg.d, &mu, mu_vec4 ? 1 : 0, (float)cfg.l2,
                          (float)cfg.l1, sstream);
      HIP_CHECK(hipGetLastError());
      launched = true;
      mu.n = 0;
      if (si >= total) break;
    }
    mu.m = 0;
    if (launched) HIP_CHECK(hipEventRecord(update_ev, sstream));
  }

  // Append one accepted gradient; handles snapshot/mark boundaries so the
  // exactly-K-steps bench contract and the printer_freq optVars cadence
  // keep per-update precision despite batching.
  void append_accepted(int wid, double t_now) {
    WorkerBuf& wk = ws[wid];
    const bool snap_now =
        cfg.snap_every > 0 && k % cfg.snap_every == 0 &&
        (long)snap_ms.size() < cfg.snap_cap;
    if (cfg.algo == 0) {
      const double gamma_k = cfg.gamma / std::sqrt((double)(k / cfg.P + 1));
      mu.scale[mu.n] = (float)(gamma_k * inv_batch);
      mu.eta[mu.n] = (float)gamma_k;  // read by the regularised form only
    }
    // multi_update_kernel reads every g of the batch before it zeroes any:
    // a worker may appear only once per batch (it is redispatched, and can
    // complete again, only after the flush)
    for (int j = 0; j < mu.n; ++j)
      if (mu.gw[j] == wid)
        throw std::runtime_error(
            "native engine: worker " + std::to_string(wid) +
            " accepted twice in one update batch");
    mu.gw[mu.n] = wid;
    mu.n += 1;
    if (cfg.algo == 1) wk.pending_commit = true;
    k += 1;
    applied += 1;
    if (k == next_ckpt) {  // never true with checkpointing off
      ckpt_due = true;     // the loop quiesces after this sweep
      ckpt_t_begin = t_now;
    }
    if (snap_now || k == cfg.mark_lo || k == cfg.mark_hi || mu.n == MU_MAX)
      flush_batch(nullptr);
    if (snap_now) {
      // optVars snapshot (reference SparkASGDThread.scala:195-198): after
      // the update that landed at the pre-increment printer_freq multiple
      HIP_CHECK(hipMemcpyAsync(
          (void*)(cfg.snap_ring + (uintptr_t)snap_ms.size() *
                                      (size_t)cfg.d * 4),
          (const void*)w, (size_t)cfg.d * 4, hipMemcpyDeviceToDevice,
          sstream));
      snap_ms.push_back((t_now - run_t0) * 1000.0);
    }
    if (k == cfg.mark_lo) {
      HIP_CHECK(hipStreamSynchronize(sstream));
      mark_lo_t = now_s();
    }
    if (k == cfg.mark_hi) {
      HIP_CHECK(hipStreamSynchronize(sstream));
      mark_hi_t = now_s();
    }
  }

  struct Result {
    long k = 0, applied = 0, rejected = 0, max_staleness = -1;
    double elapsed_ms = 0, mark_lo_t = 0, mark_hi_t = 0, avg_delay = 0;
    std::vector<double> waits;
    std::vector<double> snap_ms;
    // resumable state + checkpoint accounting
    int clock = 0;
    bool delay_flag = false;
    double cul_time_ms = 0;
    long cul_count = 0;
    long checkpoints = 0;
    double checkpoint_ms = 0;
  };

  // Everything run() and run_sync() report alike; rejected, max_staleness
  // and waits are the caller's.
  Result make_result(double elapsed_ms) const {
    Result out;
    out.k = k;
    out.elapsed_ms = elapsed_ms;
    out.applied = applied;
    out.mark_lo_t = mark_lo_t;
    out.mark_hi_t = mark_hi_t;
    out.avg_delay = cal.avg_delay_ms;
    out.snap_ms = snap_ms;
    out.clock = clock;
    out.delay_flag = cal.delay_flag;
    out.cul_time_ms = cal.cul_time_ms;
    out.cul_count = (long)cal.cul_count;
    out.checkpoints = checkpoints;
    out.checkpoint_ms = checkpoint_ms;
    return out;
  }

  // -- quiescent state + checkpoint callback -------------------------------

  // Async mode. Precondition: no round is in flight and every worker / wave
  // stream is drained. Commits every accepted-but-uncommitted SAGA round
  // (pending_commit implies the worker has not been redispatched since, so
  // its staging still holds that round) and zeroes every gradient buffer
  // holding a rejected or dropped round, on the server stream, then waits.
  // Afterwards w, alpha_bar and the history tables describe iterate k.
  void flush_quiescent() {
    if (cfg.algo == 1) {
      std::vector<int> pend;
      for (int i = 0; i < cfg.P; ++i)
        if (ws[i].pending_commit) {
          pend.push_back(i);
          ws[i].pending_commit = false;
        }
      commit_history(pend.data(), (int)pend.size(), sstream);
    }
    for (auto& wk : ws) {
      if (!wk.g_dirty) continue;
      HIP_CHECK(hipMemsetAsync((void*)wk.g, 0, (size_t)cfg.d * 4, sstream));
      wk.g_dirty = false;
    }
    HIP_CHECK(hipStreamSynchronize(sstream));
  }

  void drain_worker_streams() {
    for (auto& wk : ws) HIP_CHECK(hipStreamSynchronize(wk.stream));
    for (int i = 0; i < NWSTREAM; ++i)
      if (wstreams[i]) HIP_CHECK(hipStreamSynchronize(wstreams[i]));
  }

  // Calls the Python checkpoint callback with the quiescent state's scalars
  // (the tensors are Python's own). Every stream is idle here, so an
  // exception from the callback can free the tables before it propagates.
  void call_checkpoint() {
    try {
      py::gil_scoped_acquire gil;
      py::dict ds;
      ds["avg_delay_ms"] = cal.avg_delay_ms;
      ds["delay_flag"] = cal.delay_flag;
      ds["cul_time_ms"] = cal.cul_time_ms;
      ds["cul_count"] = cal.cul_count;
      py::dict st;
      st["k"] = k;
      st["clock"] = clock;
      st["delay_state"] = ds;
      ckpt_cb(st);
    } catch (...) {
      teardown_tables();
      throw;
    }
    checkpoints += 1;
    checkpoint_ms += (now_s() - ckpt_t_begin) * 1000.0;
    ckpt_due = false;
    next_ckpt = (k / cfg.ckpt_every + 1) * cfg.ckpt_every;
  }

  // Streams, completion lines, wave slot tables and pointer tables shared
  // by run() and run_sync(). ``sync``: every worker reads the iterate w
  // itself on the ONE server stream (no snapshot buffers, no per-worker or
  // wave streams) and publishes no completion flag (null done_flag ->
  // publish_done returns early; done_arr stays valid because
  // saga_commit_wave_kernel reuses it as its per-slot ticket).
  void setup_tables(bool sync) {
    HIP_CHECK(hipStreamCreateWithFlags(&sstream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&update_ev, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(update_ev, sstream));
    // completion flags: one pinned-host 128-B line per worker (the grad
    // kernel writes it with a system-scope release; default hipHostMalloc
    // memory is fine-grained coherent on MI355X) + one padded device
    // arrival counter per worker
    if (!sync) {
      HIP_CHECK(hipHostMalloc((void**)&flags_host,
                              (size_t)cfg.P * 16 * sizeof(unsigned long long),
                              hipHostMallocDefault));
      memset((void*)flags_host, 0,
             (size_t)cfg.P * 16 * sizeof(unsigned long long));
    }
    HIP_CHECK(hipMalloc((void**)&arr_dev,
                        (size_t)cfg.P * 16 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemset(arr_dev, 0,
                        (size_t)cfg.P * 16 * sizeof(unsigned long long)));
    for (int i = 0; i < cfg.P; ++i) {
      ws[i].done_flag = sync ? nullptr : flags_host + (size_t)i * 16;
      ws[i].done_arr = arr_dev + (size_t)i * 16;
      ws[i].round_serial = 0;
      if (sync) ws[i].wbuf = w;
    }
    for (auto& wk : ws) {
      if (sync)
        wk.stream = sstream;
      else
        HIP_CHECK(hipStreamCreateWithFlags(&wk.stream, hipStreamNonBlocking));
    }
    // wave dispatch tables. Dense: ASGD pipe-kernel shapes. CSR: ASGD and
    // SAGA with device-resident history (spill mode keeps per-worker
    // launches — its per-round scan/gather chain doesn't batch).
    const bool no_wave = std::getenv("ASYNCAMD_NO_WAVE") != nullptr;
    const bool dense_wave =
        !ws[0].sparse && cfg.d % 4 == 0 && cfg.d <= 2048;
    const bool csr_wave = ws[0].sparse;
    wave_ok = (dense_wave || csr_wave) && cfg.P <= GRAD_WAVE_MAXP &&
              !no_wave;
    wave_spill = cfg.algo == 1 && ws[0].alpha_host != 0;
    if (wave_ok) {
      wave_max_rows = 0;
      for (int i = 0; i < cfg.P; ++i)
        wave_max_rows = std::max(wave_max_rows, ws[i].n_rows);
      if (dense_wave) {
        std::vector<GradWaveSlot> hs(cfg.P);
        for (int i = 0; i < cfg.P; ++i) {
          hs[i].X = (const void*)ws[i].X;
          hs[i].y = (const float*)ws[i].y;
          hs[i].wbuf = (const float*)ws[i].wbuf;
          hs[i].g = (float*)ws[i].g;
          hs[i].n_out = (int*)ws[i].ctr;
          hs[i].n_rows = ws[i].n_rows;
          hs[i].row_start = ws[i].row_start;
          hs[i].done_flag = (unsigned long long*)ws[i].done_flag;
          hs[i].done_arr = ws[i].done_arr;
          hs[i].alpha = (float*)ws[i].alpha;
          hs[i].idx_out = (int*)ws[i].idx_out;
          hs[i].e_out = (float*)ws[i].e_out;
          hs[i].pos_ctr = (int*)(ws[i].ctr + 4);
          hs[i].alpha_host = (const float*)ws[i].alpha_host;
          hs[i].srows = (int*)ws[i].srows;
          hs[i].sylist = (float*)ws[i].sylist;
          hs[i].scnt = (int*)ws[i].scnt;
        }
        slots_dev = upload_table(hs);
      } else {
        std::vector<CsrWaveSlot> hs(cfg.P);
        for (int i = 0; i < cfg.P; ++i) {
          hs[i].indptr = (const int*)ws[i].indptr;
          hs[i].indices = (const int*)ws[i].indices;
          hs[i].values = (const void*)ws[i].values;
          hs[i].y = (const float*)ws[i].y;
          hs[i].wbuf = (const float*)ws[i].wbuf;
          hs[i].alpha = (float*)ws[i].alpha;
          hs[i].g = (float*)ws[i].g;
          hs[i].n_out = (int*)ws[i].ctr;
          hs[i].idx_out = (int*)ws[i].idx_out;
          hs[i].e_out = (float*)ws[i].e_out;
          hs[i].pos_ctr = (int*)(ws[i].ctr + 4);
          hs[i].n_rows = ws[i].n_rows;
          hs[i].row_start = ws[i].row_start;
          hs[i].done_flag = (unsigned long long*)ws[i].done_flag;
          hs[i].done_arr = ws[i].done_arr;
        }
        csr_slots_dev = upload_table(hs);
      }
      if (cfg.algo == 1) {  // unified commit view (dense + CSR SAGA)
        std::vector<CommitSlot> cs(cfg.P);
        for (int i = 0; i < cfg.P; ++i) {
          cs[i].dst = (float*)(ws[i].alpha_host ? ws[i].alpha_host
                                                : ws[i].alpha);
          cs[i].idx = (int*)ws[i].idx_out;
          cs[i].e = (float*)ws[i].e_out;
          cs[i].pos_ctr = (int*)(ws[i].ctr + 4);
          cs[i].scnt = ws[i].alpha_host ? (int*)ws[i].scnt : nullptr;
          cs[i].n_out = (int*)ws[i].ctr;
          cs[i].arr = ws[i].done_arr;
        }
        commit_slots_dev = upload_table(cs);
      }
      if (!sync)
        for (int i = 0; i < NWSTREAM; ++i)
          HIP_CHECK(hipStreamCreateWithFlags(&wstreams[i],
                                             hipStreamNonBlocking));
      wave_bper = query_grad_grid(wave_max_rows);
      if (!std::getenv("ASYNCAMD_GRAD_GRID")) {
        // per-worker grids are sized for the WAVE (512 total blocks), not
        // as if launched alone (that left 5 sampled rows per block at
        // P=32). Re-measured with the gradient kernel at 4 blocks per CU
        // (flagship, interleaved env-override A/B): 16 blocks/worker
        // 354-370k updates/s, 24: 381-410k, 32: 402-420k, 48: 364-366k.
        // 32 is faster but is NOT adopted: it moves the final weights
        // further from the parent schedule's than the parent's own
        // run-to-run distance (profiles/r04_grad_occupancy.md, section 4)
        wave_bper = std::min(wave_bper, std::max(8, 512 / cfg.P));
      }
      // interleaved block->slot mapping measured +21% on the flagship
      // (workers progress together => completions bunch => bigger update
      // batches and fuller next waves)
      const char* wi = std::getenv("ASYNCAMD_WAVE_INTERLEAVE");
      wave_interleave = wi ? std::atoi(wi) : 1;
    }
    inv_batch = (double)cfg.P / (cfg.rate * (double)cfg.N);
    inv_N = 1.0 / (double)cfg.N;
    {  // device pointer tables for the batched update kernel
      std::vector<float*> hg(cfg.P), hw(cfg.P);
      mu_vec4 = cfg.d % 4 == 0 && ((w | alpha_bar) & 15) == 0;
      for (int i = 0; i < cfg.P; ++i) {
        hg[i] = (float*)ws[i].g;
        hw[i] = (float*)ws[i].wbuf;
        mu_vec4 = mu_vec4 && ((ws[i].g | ws[i].wbuf) & 15) == 0;
      }
      g_tab_dev = upload_table(hg);
      wbuf_tab_dev = upload_table(hw);
    }
    if (sync) {  // sample-counter table + reset ticket (sync_round_update)
      std::vector<int*> hc(cfg.P);
      for (int i = 0; i < cfg.P; ++i) hc[i] = (int*)ws[i].ctr;
      ctr_tab_dev = upload_table(hc);
      HIP_CHECK(hipMalloc(&sync_ticket_dev, 16));
      HIP_CHECK(hipMemset(sync_ticket_dev, 0, 16));
    }
  }

  // Frees everything setup_tables made. The caller has drained every
  // stream that may still touch these buffers.
  void teardown_tables() {
    for (auto& wk : ws) {
      if (wk.stream && wk.stream != sstream)
        HIP_CHECK(hipStreamDestroy(wk.stream));
      wk.stream = nullptr;
      wk.done_flag = nullptr;
      wk.done_arr = nullptr;
    }
    if (flags_host) {
      HIP_CHECK(hipHostFree((void*)flags_host));
      flags_host = nullptr;
    }
    free_table(arr_dev);
    free_table(slots_dev);
    free_table(csr_slots_dev);
    free_table(commit_slots_dev);
    for (int i = 0; i < NWSTREAM; ++i)
      if (wstreams[i]) {
        HIP_CHECK(hipStreamDestroy(wstreams[i]));
        wstreams[i] = nullptr;
      }
    HIP_CHECK(hipEventDestroy(update_ev));
    HIP_CHECK(hipStreamDestroy(sstream));
    free_table(g_tab_dev);
    free_table(wbuf_tab_dev);
    free_table(ctr_tab_dev);
    free_table(sync_ticket_dev);
  }

  // One sweep over the workers' completion lines: book every finished
  // round, append the accepted ones to the update batch. True when any
  // round completed.
  inline __attribute__((always_inline)) bool poll_sweep() {
    bool any = false;
    for (int i = 0; i < cfg.P && k < cfg.iters; ++i) {
      WorkerBuf& wk = ws[i];
      // NB round-1 regression: a `submit_t > finish_t` guard here was
      // permanently false after dispatch() seeded finish_t = t_now on the
      // first round (BENCH_r01 30-min 0%-GPU hang). !busy alone gates
      // polling; busy is only set between dispatch and completion.
      if (!wk.busy || !wk.in_flight) continue;
      // event-free completion: the grad kernel's last block published
      // round_serial to this pinned line (system-scope release store);
      // a plain volatile read replaces hipEventQuery
      if (*wk.done_flag == wk.round_serial) {
        const double tc = now_s();
        if (book_completion(i, tc)) append_accepted(i, tc);
        any = true;
      }
    }
    return any;
  }

  // Collect the dispatchable workers, apply the batch (writing their
  // weight snapshots) and launch their rounds.
  void redispatch(std::vector<int>& ready) {
    ready.clear();
    collect_ready(now_s(), ready);
    // one kernel: apply the sweep's remaining accepted gradients AND
    // write the post-batch w into the redispatching workers' snapshot
    // buffers (replaces a 3 KB hipMemcpyAsync per dispatch)
    flush_batch(&ready);
    const double td = now_s();
    if (wave_ok)
      dispatch_wave(ready, td);
    else
      for (int wid : ready) dispatch_impl(wid, td, false);
  }

  // Periodic checkpoint (cold path, entered from the sweep in which k
  // crossed a multiple of ckpt_every): dispatch nothing new, keep booking
  // completions normally — tau filter, updates, k may advance — until no
  // round is in flight; delayed stragglers stay delayed. Then the quiescent
  // flush, the callback, and a redispatch of the idle workers against a
  // fresh w. Returns early, leaving ckpt_due set, when the run ends first
  // (k reached iters or the wall cap): run()'s quiescent end takes over.
  void quiesce_and_checkpoint(double t0, double& last_progress,
                              std::vector<int>& ready) {
    flush_batch(nullptr);
    while (true) {
      bool flying = false;
      for (auto& wk : ws) flying = flying || wk.in_flight;
      if (!flying) break;
      const double t_now = now_s();
      if (k >= cfg.iters || t_now - t0 > cfg.max_wall_s) return;
      if (t_now > last_progress + cfg.stall_s)
        throw std::runtime_error(
            "native engine stalled: no completion for " +
            std::to_string(cfg.stall_s) + " s while quiescing for a "
            "checkpoint at k=" + std::to_string(k));
      if (poll_sweep()) {
        last_progress = t_now;
        flush_batch(nullptr);
      }
    }
    drain_worker_streams();
    flush_quiescent();
    call_checkpoint();
    last_progress = now_s();
    if (k < cfg.iters) redispatch(ready);
  }

  Result run() {
    setup_tables(false);
    arm_start();
    for (int i = 0; i < cfg.P; ++i) pendingq.push_back(i);
    const double t0 = now_s();
    run_t0 = t0;
    // first dispatch ignores the gate (reference k==0 path); a resume at
    // k0 >= iters runs zero rounds
    if (k < cfg.iters) {
      const size_t qn = pendingq.size();
      for (size_t i = 0; i < qn; ++i) {
        const int wid = pendingq.front();
        pendingq.pop_front();
        dispatch(wid, t0);
      }
    }
    double last_progress = t0;
    std::vector<int> ready;
    ready.reserve(cfg.P);
    while (k < cfg.iters) {
      const double t_now = now_s();
      if (t_now - t0 > cfg.max_wall_s) break;
      // stall watchdog: a wedged loop (lost completion, bad event, driver
      // hang) must fail loudly in seconds, not spin GPU-idle to max_wall_s
      // (the round-1 failure mode). Delayed dispatches push the deadline.
      double stall_deadline = last_progress + cfg.stall_s;
      for (auto& dw : delayed)
        stall_deadline = std::max(stall_deadline, dw.first + cfg.stall_s);
      if (t_now > stall_deadline) {
        int busy_n = 0;
        for (auto& wk : ws) busy_n += wk.busy ? 1 : 0;
        throw std::runtime_error(
            "native engine stalled: no completion for " +
            std::to_string(cfg.stall_s) + " s at k=" + std::to_string(k) +
            " (busy=" + std::to_string(busy_n) +
            ", delayed=" + std::to_string(delayed.size()) +
            ", pending=" + std::to_string(pendingq.size()) + ")");
      }
      // release due delayed dispatches (due times are NOT monotone across
      // the deque — straggler draws differ per worker — so scan all)
      for (size_t di = 0; di < delayed.size();) {
        if (delayed[di].first <= t_now) {
          const int wid = delayed[di].second;
          delayed.erase(delayed.begin() + (long)di);
          dispatch(wid, t_now);
        } else {
          ++di;
        }
      }
      // poll completions; accepted gradients accumulate into one batched
      // update kernel per sweep (append_accepted flushes early at snapshot
      // and bench-mark boundaries to keep per-update precision)
      if (poll_sweep()) {
        last_progress = t_now;
        if (ckpt_due)
          quiesce_and_checkpoint(t0, last_progress, ready);
        else
          redispatch(ready);
      }
    }
    HIP_CHECK(hipStreamSynchronize(sstream));
    const double t1 = now_s();
    // drain in-flight rounds so buffers are quiescent before Python
    // resumes — INCLUDING the wave streams: the final sweep may have
    // dispatched a wave whose kernels are still writing g/wbuf/alpha and
    // publishing to the pinned flags this teardown is about to free
    drain_worker_streams();
    // quiescent end (after the t1 stamp: reported times are unchanged).
    // Rounds still in flight at exit are dropped — their sums are zeroed
    // with the rejected rounds' — and every accepted round's history is
    // committed, so w, alpha_bar and the tables describe exactly iterate k
    for (auto& wk : ws)
      if (wk.in_flight) {
        wk.in_flight = false;
        wk.g_dirty = true;
      }
    flush_quiescent();
    if (ckpt_due) call_checkpoint();  // k crossed a multiple as the run ended
    Result out = make_result((t1 - t0) * 1000.0);
    out.rejected = rejected;
    out.max_staleness = max_staleness_seen;
    for (auto& wk : ws) out.waits.push_back(wk.waiting_ms);
    teardown_tables();
    return out;
  }

  // -- synchronous mode (see the file header) ------------------------------

  // Commit the previous sync SAGA round's staged history for all P workers
  // on the server stream (no-op when nothing is staged). The wave kernel
  // also resets the staging counters; the per-worker form leaves that to
  // launch_grad's memset. Clearing sync_staged is what keeps the round
  // after a checkpoint from committing the same staging again.
  void sync_commit_staged() {
    if (cfg.algo != 1 || !sync_staged) return;
    commit_history(all_wids.data(), cfg.P, sstream);
    sync_staged = false;
  }

  // Round kr's gradient work, all on the server stream: (SAGA) the commit
  // of the previous round's staged history, unless a checkpoint already
  // committed it — every sync round is accepted — then one gradient wave
  // over ALL P slots against w itself. Shapes the wave kernels do not
  // cover take the per-worker launch_grad on that same stream
  // (setup_tables(true) pointed wk.stream at sstream, wk.wbuf at w).
  void sync_enqueue_grad(long kr) {
    sync_commit_staged();
    if (!wave_ok) {
      // SAGA: launch_grad re-zeroes ctr after the commit
      for (auto& wk : ws) launch_grad(wk, kr + 1);  // reference seed+k+1
      return;
    }
    // every slot at round kr; round_serial stays 0 and is unused (the sync
    // slots carry a null done_flag)
    for (auto& wk : ws) wk.k_submit = kr;
    launch_grad_wave(all_wids.data(), cfg.P, sstream);
  }

  // The barrier: poll the event recorded behind round kr's update. Bounded
  // by the stall watchdog counted from ``t_from`` (the later of submit and
  // straggler release) — never an unbounded synchronize.
  void sync_wait_round(long kr, double t_from) {
    const double deadline = t_from + cfg.stall_s;
    while (true) {
      const hipError_t e = hipEventQuery(update_ev);
      if (e == hipSuccess) break;
      if (e != hipErrorNotReady)
        throw std::runtime_error(std::string("native sync engine: ") +
                                 hipGetErrorString(e) + " at round k=" +
                                 std::to_string(kr));
      if (now_s() > deadline)
        throw std::runtime_error(
            "native sync engine stalled: round k=" + std::to_string(kr) +
            " not complete after " + std::to_string(cfg.stall_s) + " s");
    }
    (void)hipGetLastError();  // drop the polls' hipErrorNotReady
  }

  // Commit whatever round kr staged and wait for it (bounded, like every
  // wait of this path). Without staged history the stream is already idle.
  void sync_quiesce(long kr) {
    if (cfg.algo != 1 || !sync_staged) return;
    sync_commit_staged();
    HIP_CHECK(hipEventRecord(update_ev, sstream));
    sync_wait_round(kr, now_s());
  }

  // mode: 0 asgd, 1 asaga, 2 mllib (cfg.algo is 1 for asaga, else 0).
  Result run_sync(int mode) {
    setup_tables(true);
    arm_start();
    all_wids.resize(cfg.P);
    std::iota(all_wids.begin(), all_wids.end(), 0);
    bool vec4 = cfg.d % 4 == 0 &&
                ((w | alpha_bar | cfg.snap_ring) & 15) == 0;
    for (auto& wk : ws) vec4 = vec4 && (wk.g & 15) == 0;
    // start from quiescent accumulators and counters whatever an earlier
    // run on these buffers left (its last round's SAGA staging included)
    for (auto& wk : ws) {
      HIP_CHECK(hipMemsetAsync((void*)wk.g, 0, (size_t)cfg.d * 4, sstream));
      HIP_CHECK(hipMemsetAsync((void*)wk.ctr, 0, 8, sstream));
    }
    HIP_CHECK(hipEventRecord(update_ev, sstream));
    sync_wait_round(-1, now_s());
    const double inv_bN = 1.0 / (cfg.rate * (double)cfg.N);
    inv_N = 1.0 / (double)cfg.N;
    const double t0 = now_s();
    run_t0 = t0;
    double t1 = t0;
    while (k < cfg.iters) {
      const double t_submit = now_s();
      if (t_submit - t0 > cfg.max_wall_s) break;
      cal.maybe_activate(k, cfg.calib_window);
      sync_enqueue_grad(k);
      // straggler model: the barrier releases at max(gradient done,
      // t_submit + slowest worker's injected delay). The gradient runs on
      // the GPU while the host sleeps out the delay; the update is enqueued
      // only after the release time and is stream-ordered behind the
      // gradient, which gives the max().
      double dly_ms = 0.0;
      for (int wid = 0; wid < cfg.P; ++wid)
        dly_ms = std::max(dly_ms, delay_ms_for(wid, k));
      double t_release = t_submit;
      if (dly_ms > 0) {
        t_release = std::min(t_submit + dly_ms / 1000.0,
                             t0 + cfg.max_wall_s);
        const double left = t_release - now_s();
        if (left > 0)
          std::this_thread::sleep_for(std::chrono::duration<double>(left));
      }
      const bool snap_now = cfg.snap_every > 0 && k % cfg.snap_every == 0 &&
                            (long)snap_ms.size() < cfg.snap_cap;
      float* snap_dst =
          snap_now ? (float*)(cfg.snap_ring + (uintptr_t)snap_ms.size() *
                                                  (size_t)cfg.d * 4)
                   : nullptr;
      const double gamma_k = cfg.gamma / std::sqrt((double)(k + 1));
      const float scale = mode == 0   ? (float)(gamma_k * inv_bN)
                          : mode == 2 ? (float)gamma_k
                                      : 0.f;
      launch_sync_round_update((float*)w, (float* const*)g_tab_dev,
                               (int* const*)ctr_tab_dev, (float*)alpha_bar,
                               snap_dst, sync_ticket_dev, cfg.P, cfg.d, mode,
                               scale, (float)cfg.gamma, (float)inv_bN,
                               (float)inv_N, vec4 ? 1 : 0,
                               (float)(mode == 1 ? cfg.gamma : gamma_k),
                               (float)cfg.l2, (float)cfg.l1, sstream);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(update_ev, sstream));
      sync_wait_round(k, std::max(t_submit, t_release));
      // every stamp that describes round k is taken here, after the GPU
      // has finished it
      t1 = now_s();
      if (k * cfg.P < cfg.calib_window)  // DelayInjector.record_task, P tasks
        cal.record((t1 - t_submit) * 1000.0 * cfg.P, cfg.P);
      if (snap_now) snap_ms.push_back((t1 - t0) * 1000.0);
      sync_staged = mode == 1;
      k += 1;
      applied += 1;
      if (k == cfg.mark_lo) mark_lo_t = t1;
      if (k == cfg.mark_hi) mark_hi_t = t1;
      if (k == next_ckpt) {  // never true with checkpointing off
        ckpt_t_begin = now_s();
        sync_quiesce(k - 1);
        call_checkpoint();
      }
    }
    // quiescent end (after the last t1 stamp): the last round's staged
    // history is committed, so the tables describe iterate k
    sync_quiesce(k - 1);
    Result out = make_result((t1 - t0) * 1000.0);
    out.rejected = 0;
    out.max_staleness = 0;
    out.waits.assign(cfg.P, 0.0);
    teardown_tables();
    return out;
  }
};

}  // namespace

namespace {

void fill_engine(NativeEngine& eng, py::dict c, py::list workers,
                 uintptr_t w, uintptr_t alpha_bar, py::object ckpt_cb) {
  EngineCfg& cfg = eng.cfg;
  cfg.N = py::cast<long>(c["N"]);
  cfg.d = py::cast<int>(c["d"]);
  cfg.P = py::cast<int>(c["P"]);
  cfg.iters = py::cast<long>(c["iters"]);
  cfg.gamma = py::cast<double>(c["gamma"]);
  cfg.rate = py::cast<double>(c["rate"]);
  cfg.bucket_ratio = py::cast<double>(c["bucket_ratio"]);
  cfg.taw = py::cast<long>(c["taw"]);
  cfg.seed = py::cast<uint64_t>(c["seed"]);
  cfg.algo = py::cast<int>(c["algo"]);
  cfg.objective = py::cast<int>(c["objective"]);
  cfg.coeff = py::cast<double>(c["coeff"]);
  cfg.calib_window = py::cast<long>(c["calib_window"]);
  cfg.mark_lo = py::cast<long>(c["mark_lo"]);
  cfg.mark_hi = py::cast<long>(c["mark_hi"]);
  cfg.max_wall_s = py::cast<double>(c["max_wall_s"]);
  if (c.contains("stall_s")) cfg.stall_s = py::cast<double>(c["stall_s"]);
  if (c.contains("l2")) cfg.l2 = py::cast<double>(c["l2"]);
  if (c.contains("l1")) cfg.l1 = py::cast<double>(c["l1"]);
  if (!(cfg.l2 >= 0.0) || !(cfg.l1 >= 0.0) || std::isinf(cfg.l2) ||
      std::isinf(cfg.l1))
    throw std::runtime_error(
        "native engine: l2/l1 must be finite and non-negative");
  cfg.snap_every = py::cast<long>(c["snap_every"]);
  cfg.snap_ring = py::cast<uintptr_t>(c["snap_ring"]);
  cfg.snap_cap = py::cast<long>(c["snap_cap"]);
  if (c.contains("k0")) cfg.k0 = py::cast<long>(c["k0"]);
  if (c.contains("clock0")) cfg.clock0 = py::cast<int>(c["clock0"]);
  if (c.contains("ckpt_every"))
    cfg.ckpt_every = py::cast<long>(c["ckpt_every"]);
  if (cfg.k0 < 0 || cfg.clock0 < 0 || cfg.ckpt_every < 0)
    throw std::runtime_error(
        "native engine: k0, clock0 and ckpt_every must be non-negative");
  if (c.contains("delay_state")) {
    // a resumed straggler run neither recalibrates nor runs undelayed
    py::dict ds = py::cast<py::dict>(c["delay_state"]);
    eng.cal.avg_delay_ms = py::cast<double>(ds["avg_delay_ms"]);
    eng.cal.delay_flag = py::cast<bool>(ds["delay_flag"]);
    eng.cal.cul_time_ms = py::cast<double>(ds["cul_time_ms"]);
    eng.cal.cul_count = py::cast<long>(ds["cul_count"]);
  }
  if (cfg.ckpt_every > 0 && ckpt_cb.is_none())
    throw std::runtime_error(
        "native engine: ckpt_every > 0 needs a checkpoint callback");
  if (cfg.ckpt_every > 0) eng.ckpt_cb = ckpt_cb;
  for (auto item : workers) {
    py::dict wd = py::cast<py::dict>(item);
    WorkerBuf wk;
    wk.sparse = py::cast<bool>(wd["sparse"]);
    if (wk.sparse) {
      wk.indptr = py::cast<uintptr_t>(wd["indptr"]);
      wk.indices = py::cast<uintptr_t>(wd["indices"]);
      wk.values = py::cast<uintptr_t>(wd["values"]);
    } else {
      wk.X = py::cast<uintptr_t>(wd["X"]);
    }
    wk.y = py::cast<uintptr_t>(wd["y"]);
    wk.wbuf = py::cast<uintptr_t>(wd["wbuf"]);
    wk.g = py::cast<uintptr_t>(wd["g"]);
    wk.ctr = py::cast<uintptr_t>(wd["ctr"]);
    wk.n_rows = py::cast<long>(wd["n_rows"]);
    wk.row_start = py::cast<long>(wd["row_start"]);
    wk.x_is_bf16 = py::cast<int>(wd["x_is_bf16"]);
    if (eng.cfg.algo == 1) {
      wk.alpha = py::cast<uintptr_t>(wd["alpha"]);
      wk.idx_out = py::cast<uintptr_t>(wd["idx_out"]);
      wk.e_out = py::cast<uintptr_t>(wd["e_out"]);
      wk.saga_cap = py::cast<int>(wd["saga_cap"]);
      if (wd.contains("alpha_host")) {
        wk.alpha_host = py::cast<uintptr_t>(wd["alpha_host"]);
        wk.srows = py::cast<uintptr_t>(wd["srows"]);
        wk.sylist = py::cast<uintptr_t>(wd["sylist"]);
        wk.scnt = py::cast<uintptr_t>(wd["scnt"]);
      }
    }
    eng.ws.push_back(wk);
  }
  if ((int)eng.ws.size() != cfg.P)
    throw std::runtime_error("native engine: P != len(workers)");
  eng.w = w;
  eng.alpha_bar = alpha_bar;
}

py::dict result_dict(const NativeEngine::Result& r) {
  py::dict out;
  out["k"] = r.k;
  out["elapsed_ms"] = r.elapsed_ms;
  out["applied"] = r.applied;
  out["rejected"] = r.rejected;
  out["max_staleness"] = r.max_staleness;
  out["mark_lo_t"] = r.mark_lo_t;
  out["mark_hi_t"] = r.mark_hi_t;
  out["avg_delay_ms"] = r.avg_delay;
  out["waiting_ms"] = r.waits;
  out["snap_ms"] = r.snap_ms;
  out["clock"] = r.clock;
  out["delay_flag"] = r.delay_flag;
  out["cul_time_ms"] = r.cul_time_ms;
  out["cul_count"] = r.cul_count;
  out["checkpoints"] = r.checkpoints;
  out["checkpoint_ms"] = r.checkpoint_ms;
  return out;
}

}  // namespace

void register_native_engine(py::module_& m) {
  m.def(
      "native_local_run",
      [](py::dict c, py::list workers, uintptr_t w, uintptr_t alpha_bar,
         py::object ckpt_cb) {
        NativeEngine eng;
        fill_engine(eng, c, workers, w, alpha_bar, ckpt_cb);
        NativeEngine::Result r;
        {
          // the event loop never touches Python, except to call ckpt_cb
          // (GIL re-taken for that call alone) at a quiescent checkpoint
          py::gil_scoped_release rel;
          r = eng.run();
        }
        return result_dict(r);
      },
      py::arg("conf"), py::arg("workers"), py::arg("w"),
      py::arg("alpha_bar"), py::arg("ckpt_cb") = py::none());
  // Synchronous mode: same conf/worker dicts, plus mode 0 asgd / 1 asaga /
  // 2 mllib (conf["algo"] is 1 for asaga, else 0). Host-spill history is
  // not supported here (the Python adapter rejects it).
  m.def(
      "native_sync_run",
      [](py::dict c, py::list workers, uintptr_t w, uintptr_t alpha_bar,
         int mode, py::object ckpt_cb) {
        if (mode < 0 || mode > 2)
          throw std::runtime_error("native sync engine: mode must be 0..2");
        NativeEngine eng;
        fill_engine(eng, c, workers, w, alpha_bar, ckpt_cb);
        if ((mode == 1) != (eng.cfg.algo == 1))
          throw std::runtime_error(
              "native sync engine: mode/algo mismatch");
        for (auto& wk : eng.ws)
          if (wk.alpha_host)
            throw std::runtime_error(
                "native sync engine: host-spill history is not supported");
        NativeEngine::Result r;
        {
          py::gil_scoped_release rel;
          r = eng.run_sync(mode);
        }
        return result_dict(r);
      },
      py::arg("conf"), py::arg("workers"), py::arg("w"),
      py::arg("alpha_bar"), py::arg("mode"), py::arg("ckpt_cb") = py::none());
}
