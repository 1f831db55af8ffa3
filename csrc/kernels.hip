// Hand-written CDNA4 (gfx950 / MI355X) kernels for the ASYNC hot path.
//
// Kernel inventory (reference JVM hot loops they replace):
//   K1 grad_dense      — fused Philox sample mask + per-row dot + scaled
//                        accumulate (reference gradfun SparkASGDThread.scala:
//                        423-438 + reducePartition fold RDD.scala:1103-1123);
//                        three forms: grad_dense_pipe_kernel and its
//                        whole-wave twin grad_dense_wave_kernel (LDS row
//                        queue + register pipeline), scan_rows_kernel +
//                        grad_dense_list_kernel (split form for the graph
//                        engine's scan/compute overlap), and a generic
//                        fallback for d > 2048 or d % 4 != 0. The queue-fed
//                        forms share ONE scan loop (scan_enqueue), ONE row
//                        pipeline (pipe_drain) and ONE partials flush
//                        (flush_partials).
//   K2 grad_csr        — CSR SpMV-style gradient, wave-per-row
//                        (reference sparse BLAS.scala:74-90,134-160).
//   K3 saga_grad_*     — K1/K2 fused with the per-sample history gather and
//                        staged scalar emit (SparkASAGAThread.scala:380-385).
//   K5 sgd_update      — fused scale+axpy weight update (:188-192).
//   K6 saga_update     — fused SAGA triple-axpy (:217-220).
//                        K5/K6 arithmetic, plain and elastic-net, lives in
//                        update_step.h (asgd_step / saga_step); the singleton,
//                        batched (multi_update), sync-round, fused-graph and
//                        reduce+update kernels all call it.
//   K8 philox.h        — in-kernel counter-based Bernoulli mask.
//   K9 eval.h          — fused held-out evaluation: loss sum + confusion
//                        counts of a tile of stacked iterates in one pass
//                        over the rows (included at the end of this file).
//   K10 eval_curve.h   — K9's scoring with a threshold histogram per
//                        iterate: the confusion counts at EVAL_KT thresholds
//                        (ROC / PR points) from the same single pass.
// The link function of K1-K3 (lsq / logistic / hinge) lives in link.h.
// Launchers: runtime (dtype, saga, ITERS, DEPTH, LPR, flags) become template
// arguments through with_const / with_bool / with_xt_saga / with_pipe_shape.
//
// Design notes (MI355X, measured on hardware):
//  * 64-wide wavefronts. ONE Philox eval decides FOUR consecutive rows
//    (counter = row/4, output word = row%4) — the full-dataset mask scan is
//    the dominant fixed cost per round (8.1M rows; 32-bit integer multiply
//    is slow on the VALU), so each wave covers 256 rows per eval step.
//  * row processing is latency-bound, not bandwidth-bound, at the
//    reference's sampling rates (b=0.01 samples ~81k of 8.1M rows). The
//    main dense path (grad_dense_pipe_body, d <= 2048, d % 4 == 0) hides
//    the latency two ways: each wave keeps DEPTH whole rows in flight in a
//    register pipeline of bounds-checked buffer loads, and several blocks
//    share a CU — the body is force-inlined under a waves-per-SIMD launch
//    bound chosen per shape (PipeShape) so the pipeline costs ~126 VGPRs
//    at the flagship shape, not the whole register file.
//  * dense path: w staged in LDS; one fp32 gradient slab per wave in LDS
//    (LDS = 5 * ITERS*256 * 4 bytes + the row queue); the wave/flag
//    launches finish with one atomicAdd per nonzero element per block into
//    the worker's g, the graph engine's forms write per-block partials to
//    a transposed slab summed by reduce_partials.
//  * the generic fallback (grad_dense_kernel: d > 2048 or d % 4 != 0)
//    processes rows by SUB-WAVES of LPR lanes (64/32/16) with per-sub-wave
//    slabs (LDS = (1 + 4*64/LPR)*d*4 bytes).
//  * sparse path: w stays in L2 (rcv1 d=47236 -> 189 KB; L2 is 4 MiB/XCD);
//    gradient scatter via global fp32 atomics (~73 nnz/row, low contention).
//  * bf16 rows load as ushort4 (8 B/lane) — scalar bf16 loads halve
//    effective bandwidth (CDNA guide, common mistake #2).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include "philox.h"
#include "grad_wave.h"
#include "launchers.h"  // every extern "C" definition below is checked by it
#include "link.h"
#include "update_step.h"

#define WAVE 64
#define BLOCK 256
#define WAVES_PER_BLOCK (BLOCK / WAVE)
#define ROWS_PER_WAVE 256  // 64 lanes x 4 rows per philox eval
#define ROWS_PER_BLOCK_ITER (WAVES_PER_BLOCK * ROWS_PER_WAVE)

// ---------------------------------------------------------------- helpers

// Host-visible completion flag: the LAST arriving block publishes
// `done_val` to fine-grained pinned host memory with system-scope release,
// replacing the native engine's hipEventRecord + hipEventQuery pair
// (~2-4 us of host API per round). All prior global writes (g atomics,
// SAGA staging) are ordered before the flag by the fence chain.
__device__ __forceinline__ void publish_done(
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr, unsigned int nblk) {
  if (!done_flag) return;  // uniform per launch: no divergence
  // NO fences here — fence instructions at agent scope on a multi-XCD
  // chip emit per-block L2 writeback/invalidate (buffer_wbl2/inv), which
  // poisoned every concurrent kernel's L2 (measured: grad 16.6 -> 117 us
  // with a __threadfence + acq_rel arrival). The gradient's cross-kernel
  // outputs (g, n_out) are written with ATOMICS, which execute at the
  // agent coherence point; all that is needed before arrival is to DRAIN
  // this thread's outstanding vmem ops, then count with a relaxed RMW.
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long arrived = __hip_atomic_fetch_add(
        done_arr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived + 1 == (unsigned long long)nblk) {
      // reset for the next round with a RETURNING exchange, then drain it
      // before the flag store: guarantees the reset is globally ordered
      // before the host can observe this round's completion
      (void)__hip_atomic_exchange(done_arr, 0ull, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_s_waitcnt(0);
      __hip_atomic_store(done_flag, done_val, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <typename XT>
__device__ __forceinline__ float to_f32(XT v);
template <>
__device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}

// Load 4 consecutive elements starting at xrow[4*j4] as floats.
template <typename XT>
__device__ __forceinline__ void load4(const XT* xrow, int j4, float out[4]);

template <>
__device__ __forceinline__ void load4<float>(const float* xrow, int j4,
                                             float out[4]) {
  const float4 v = reinterpret_cast<const float4*>(xrow)[j4];
  out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
}

template <>
__device__ __forceinline__ void load4<__hip_bfloat16>(
    const __hip_bfloat16* xrow, int j4, float out[4]) {
  const ushort4 v = reinterpret_cast<const ushort4*>(xrow)[j4];
  union { unsigned short u; __hip_bfloat16 b; } c0{v.x}, c1{v.y}, c2{v.z},
      c3{v.w};
  out[0] = __bfloat162float(c0.b); out[1] = __bfloat162float(c1.b);
  out[2] = __bfloat162float(c2.b); out[3] = __bfloat162float(c3.b);
}

// ---------------------------------------------------------------- K1 (+K3)

// LPR = lanes per row (64, 32 or 16): rows are processed by aligned
// sub-waves so 64/LPR rows are in flight per wave.
template <typename XT, bool SAGA, int LPR, bool HINGE>
__global__ __launch_bounds__(BLOCK) void grad_dense_kernel(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ w, float* __restrict__ g_out,
    float* __restrict__ g_part, int* __restrict__ n_out,
    float* __restrict__ alpha, int* __restrict__ idx_out,
    float* __restrict__ e_out, int* __restrict__ pos_ctr,
    const int* __restrict__ k_dev, int commit_now, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, uint32_t threshold,
    int take_all, int objective, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr) {
  if (k_dev) round_k = (uint32_t)(*k_dev) + 1u;  // graph mode: round = k+1
  constexpr int NSUB = WAVE / LPR;
  constexpr int NSLAB = WAVES_PER_BLOCK * NSUB;
  extern __shared__ float smem[];
  float* w_lds = smem;           // [d]
  float* gacc = smem + d;        // [NSLAB][d]
  for (int j = threadIdx.x; j < d; j += BLOCK) {
    w_lds[j] = w[j];
#pragma unroll
    for (int s2 = 0; s2 < NSLAB; ++s2) gacc[(size_t)s2 * d + j] = 0.f;
  }
  __syncthreads();

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR;
  const int sl = lane % LPR;
  float* gw = gacc + (size_t)(wave * NSUB + sub) * d;
  int local_count = 0;
  const int d4 = d >> 2;

  const long gstride = (long)gridDim.x * ROWS_PER_BLOCK_ITER;
  for (long bb = (long)blockIdx.x * ROWS_PER_BLOCK_ITER; bb < n_rows;
       bb += gstride) {
    const long base = bb + (long)wave * ROWS_PER_WAVE;
    if (base >= n_rows) continue;
    // scan 256 rows: lane's philox block covers rows base+4*lane..+3
    // (requires row_start % 4 == 0 — enforced by the launcher/sharder)
    const uint4 x = philox_block4(
        seed, round_k, (row_start + (uint64_t)base) / 4 + (uint64_t)lane);
    const long rem = n_rows - base;
    unsigned long long m[4];
    {
      const long lrow = 4L * lane;
      m[0] = __ballot(lrow + 0 < rem && (take_all || x.x < threshold));
      m[1] = __ballot(lrow + 1 < rem && (take_all || x.y < threshold));
      m[2] = __ballot(lrow + 2 < rem && (take_all || x.z < threshold));
      m[3] = __ballot(lrow + 3 < rem && (take_all || x.w < threshold));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned long long mm = m[i];
      for (int s2 = 0; s2 < sub && mm; ++s2) mm &= mm - 1;  // my first bit
      while (mm) {
        const int bit = __ffsll((long long)mm) - 1;
        const long rr = base + 4L * bit + i;
        const XT* xrow = X + (size_t)rr * d;
        float z = 0.f;
        for (int j4 = sl; j4 < d4; j4 += LPR) {
          float xv[4];
          load4<XT>(xrow, j4, xv);
          const int j = j4 * 4;
          z += xv[0] * w_lds[j] + xv[1] * w_lds[j + 1] +
               xv[2] * w_lds[j + 2] + xv[3] * w_lds[j + 3];
        }
        for (int j = d4 * 4 + sl; j < d; j += LPR)  // d % 4 tail
          z += to_f32<XT>(xrow[j]) * w_lds[j];
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1)
          z += __shfl_xor(z, off, WAVE);
        float e = link_residual<HINGE>(z, y[rr], objective);
        float coeff = e;
        if (SAGA) {
          const float a_old = alpha[rr];
          coeff = e - a_old;
          if (sl == 0) {
            if (commit_now) {
              // sequential graph mode: every round accepted -> commit in
              // place (each row sampled once per round, read-before-write)
              alpha[rr] = e;
            } else {
              // atomic staging: read cross-stream in wave mode
              const int pos = atomicAdd(pos_ctr, 1);
              __hip_atomic_exchange(&idx_out[pos], (int)rr,
                                    __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_exchange(&e_out[pos], e, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
        ++local_count;
        for (int j4 = sl; j4 < d4; j4 += LPR) {
          float xv[4];
          load4<XT>(xrow, j4, xv);
          const int j = j4 * 4;
          gw[j] += coeff * xv[0]; gw[j + 1] += coeff * xv[1];
          gw[j + 2] += coeff * xv[2]; gw[j + 3] += coeff * xv[3];
        }
        for (int j = d4 * 4 + sl; j < d; j += LPR)  // d % 4 tail
          gw[j] += coeff * to_f32<XT>(xrow[j]);
        for (int s2 = 0; s2 < NSUB && mm; ++s2) mm &= mm - 1;  // next mine
      }
    }
  }
  __syncthreads();
  if (g_part != nullptr) {
    // plain-store partials g_part[j*G + b]; reduce_partials sums them
    const size_t G = gridDim.x;
    for (int j = threadIdx.x; j < d; j += BLOCK) {
      float s = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < NSLAB; ++s2) s += gacc[(size_t)s2 * d + j];
      g_part[(size_t)j * G + blockIdx.x] = s;
    }
  } else {
    for (int j = threadIdx.x; j < d; j += BLOCK) {
      float s = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < NSLAB; ++s2) s += gacc[(size_t)s2 * d + j];
      if (s != 0.f) atomicAdd(&g_out[j], s);
    }
  }
  if (sl == 0 && local_count) atomicAdd(n_out, local_count);
  publish_done(done_flag, done_val, done_arr, gridDim.x);
}

// ------------------------------------------------- K1 pipelined (queue)
//
// Three-phase dense gradient. Phase 1 (scan): Philox decides 4 rows per
// eval; sampled row ids are appended to an LDS queue (no global load in the
// scan). Phase 1b (fetch): one strided pass loads y (and the SAGA alpha)
// for the whole queue into LDS, all loads in flight at once — staging them
// keeps ordinary vmem loads out of the pipelined phase (hipcc drains
// vmcnt(0) at any ordinary-load use, CDNA guide §5.5 trap (b): measured one
// full drain per row from y[rr]).
// Phase 2 (process): waves drain the queue round-robin with a DEPTH-deep
// statically-unrolled register pipeline; row loads are UNCONDITIONAL
// bounds-checked buffer loads (per-row scalar descriptor) with a
// compile-time ITERS count — a per-element `if (j4 < d4)` made hipcc branch
// around every load with a vmcnt(0) (guide trap 4(c)). The accumulate pass
// reuses the pipeline registers; X is read exactly once per sampled row.

// Row-queue capacity, for every queue: the pipe kernels' LDS queue, the
// standalone scan's and the list kernel's staging chunk.
#define QCAP 2048

// ---- pipelined-kernel shape selection: the ONE place that decides ITERS,
// DEPTH, the LDS sizes and the occupancy hint. The pipe, wave and list
// launchers and the query_dense_kernel binding all go through it.
//
// Occupancy hint = second argument of __launch_bounds__ = minimum waves per
// SIMD; a 256-thread block is one wave per SIMD, so the hint is also the
// number of blocks meant to share a CU. Without it (and with the body out
// of line, as it once was) the compiler spent the whole register file:
// 248 VGPR + 30 AGPR at the flagship shape, one block per CU. The hint is
// the largest value at which
//   * dynamic LDS still lets that many blocks share the CU's 160 KiB, and
//   * the DEPTH x ITERS row buffers (2 VGPRs per bf16x4, 4 per f32x4) plus
//     PIPE_WORK_VGPRS of working registers fit the per-wave budget
//     (128 / 168 / 256 / 512 registers at 4 / 3 / 2 / 1 waves per SIMD),
// so that no instantiation spills (checked with
// -Rpass-analysis=kernel-resource-usage over every selectable shape).
#define CU_LDS_BYTES 163840
#define PIPE_WORK_VGPRS 76

// LDS layout shared by the pipelined kernels, in carving order: w_lds[DPAD],
// one gradient slab gacc[NW][DPAD] per wave, then the queue arrays. The
// kernels carve smem with these same constants.
#define PIPE_BLOCK 256
#define PIPE_NW (PIPE_BLOCK / WAVE)
constexpr int pipe_dpad(int iters) { return iters * 256; }  // padded d
constexpr size_t slab_lds_bytes(int iters) {
  return (size_t)(1 + PIPE_NW) * pipe_dpad(iters) * sizeof(float);
}
// pipe / wave: + yq (and SAGA's aq, eq), rowq, the queue counter
constexpr size_t pipe_lds_bytes(int iters, bool saga) {
  return slab_lds_bytes(iters) +
         (size_t)QCAP * sizeof(float) * (saga ? 3 : 1) +
         (QCAP + 1) * sizeof(int);
}
// list: + yq, rowq
constexpr size_t list_lds_bytes(int iters) {
  return slab_lds_bytes(iters) +
         (size_t)QCAP * (sizeof(float) + sizeof(int));
}
constexpr int occupancy_hint(size_t lds_bytes, int xt_bytes, int depth,
                             int iters) {
  const int need = depth * iters * (xt_bytes == 2 ? 2 : 4) + PIPE_WORK_VGPRS;
  const int by_regs = need <= 128 ? 4 : need <= 168 ? 3 : need <= 256 ? 2 : 1;
  const int by_lds = (int)(CU_LDS_BYTES / lds_bytes);
  const int h = by_regs < by_lds ? by_regs : by_lds;
  return h < 1 ? 1 : h;
}
template <typename XT, bool SAGA, int DEPTH, int ITERS>
struct PipeShape {
  static constexpr size_t LDS = pipe_lds_bytes(ITERS, SAGA);
  static constexpr int HINT =
      occupancy_hint(LDS, (int)sizeof(XT), DEPTH, ITERS);
};

// Row-fragment types for the pipelined loaders. Loads are compiler-visible
// buffer intrinsics: with unconditional compile-time load counts and
// sched_barrier(0) fences around the refills (see the pipe kernels), hipcc
// emits a counted descending vmcnt ladder — a genuine software pipeline
// with compiler-guaranteed hazards (hand-counted inline-asm waits were
// tried and abandoned: regalloc preservation copies raced in-flight asm
// loads).
struct B16x4 { union { ushort4 s; uint2 u; }; };
struct F32x4 { union { float4 f; uint4 u; }; };

template <typename XT> struct RowVec;
template <> struct RowVec<float> {
  using T = F32x4;
  static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t rsrc,
                                           int voff_bytes) {
    T out;
    auto r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff_bytes, 0, 0);
    union { decltype(r) u; float4 f; } c{r};
    out.f = c.f;
    return out;
  }
  static constexpr int VOFF_SHIFT = 4;  // 16 B per lane-element
};
template <> struct RowVec<__hip_bfloat16> {
  using T = B16x4;
  static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t rsrc,
                                           int voff_bytes) {
    T out;
    auto r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff_bytes, 0, 0);
    union { decltype(r) u; ushort4 s; } c{r};
    out.s = c.s;
    return out;
  }
  static constexpr int VOFF_SHIFT = 3;  // 8 B per lane-element
};

__device__ __forceinline__ void cvt4(const float4& r, float o[4]) {
  o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
}
__device__ __forceinline__ void cvt4(const ushort4& r, float o[4]) {
  union { unsigned short u; __hip_bfloat16 b; } c0{r.x}, c1{r.y}, c2{r.z},
      c3{r.w};
  o[0] = __bfloat162float(c0.b); o[1] = __bfloat162float(c1.b);
  o[2] = __bfloat162float(c2.b); o[3] = __bfloat162float(c3.b);
}
__device__ __forceinline__ void cvt4(const F32x4& r, float o[4]) {
  cvt4(r.f, o);
}
__device__ __forceinline__ void cvt4(const B16x4& r, float o[4]) {
  cvt4(r.s, o);
}

// Per-row buffer descriptor: base = row start (scalar via readfirstlane),
// num_records = the row's OWN byte length (clamped to what remains of X) ->
// the hardware bounds check zero-fills every lane past the row end and
// fetches nothing for it. The pipelined loaders always issue ITERS*64 lanes
// per row; with a descriptor reaching to the end of X the lanes past d were
// real reads of the NEXT row (d=784: 480 of 2,048 B, +30% traffic), and
// although w_lds is zero-padded a non-finite value there still poisoned the
// dot product (0 * NaN). d % 4 == 0 keeps every lane's 4-element access
// wholly inside or wholly outside the row.
template <typename XT>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(
    const XT* X, long total_elems, int rr, int d) {
  const size_t off = (size_t)rr * d;
  const uint64_t rem_bytes = (uint64_t)(total_elems - off) * sizeof(XT);
  const uint64_t row_bytes = (uint64_t)d * sizeof(XT);
  const uint32_t nrec = (uint32_t)(rem_bytes < row_bytes ? rem_bytes
                                                         : row_bytes);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(X + off), 0, nrec,
                                           0x00020000);
}

// Scan phase, for every queue-fed kernel: the block walks its groups of RPB
// rows (gi, gi + nblk, ...; one Philox eval decides four rows) and appends
// the sampled row ids to rowq until the groups run out or one more group
// might overflow the queue. Row ids only — a y[row] load per hit would
// expose one global-load latency per scan iteration ahead of the
// iteration's barrier. The caller barriers before it reads *qn.
template <int RPB>
__device__ __forceinline__ void scan_enqueue(
    int* rowq, int* qn, int cap, long& gi, long ngroups, int nblk,
    long n_rows, uint64_t seed, uint32_t round_k, uint64_t row_start,
    uint32_t threshold, int take_all, int wave, int lane) {
  while (true) {
    __syncthreads();
    if (gi >= ngroups || *qn >= cap - RPB) break;
    const long base = gi * (long)RPB + (long)wave * ROWS_PER_WAVE;
    if (base < n_rows) {
      const uint4 x = philox_block4(
          seed, round_k, (row_start + (uint64_t)base) / 4 + (uint64_t)lane);
      const long rem = n_rows - base;
      const long lrow = base + 4L * lane;
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (4L * lane + i < rem && (take_all || xs[i] < threshold)) {
          const int pos = atomicAdd(qn, 1);
          rowq[pos] = (int)(lrow + i);
        }
      }
    }
    gi += nblk;
  }
}

// Process phase, for every queue-fed kernel: the block's NW waves drain
// rowq[0..nq) round-robin, each through a DEPTH-deep statically-unrolled
// register pipeline of whole rows. Per row: z = x . w_lds, then
// gw += coeff_of(q, z) * x, reusing the pipeline registers — X is read
// exactly once per sampled row. Returns the number of rows this wave
// processed. Only buffer loads and LDS traffic may happen in here and in
// coeff_of: hipcc drains vmcnt(0) at any ordinary global load's use.
// __forceinline__ is load-bearing, as for grad_dense_pipe_body.
template <typename XT, int NW, int DEPTH, int ITERS, typename CoeffOf>
__device__ __forceinline__ int pipe_drain(
    const XT* __restrict__ X, long total_elems, int d, const int* rowq,
    int nq, const float* w_lds, float* gw, int wave, int lane,
    CoeffOf&& coeff_of) {
  using RV = RowVec<XT>;
  typename RV::T buf[DEPTH][ITERS];
  int n_done = 0;
  // the counted-wait protocol needs EXACTLY ITERS loads per slot: a
  // skipped load would let vmcnt(N) pass while this buffer's own loads
  // are still in flight (vmcnt waits "<= N outstanding", nothing more).
  // Tail slots load a clamped row instead of skipping.
  if (nq > 0) {
#pragma unroll
    for (int p = 0; p < DEPTH; ++p) {
      const int q = min(wave + p * NW, nq - 1);
      const int rr = __builtin_amdgcn_readfirstlane(rowq[q]);
      const auto rs = row_rsrc<XT>(X, total_elems, rr, d);
#pragma unroll
      for (int it = 0; it < ITERS; ++it)
        buf[p][it] = RV::load(rs, (lane + it * WAVE) << RV::VOFF_SHIFT);
    }
  }
  int q_base = wave;
  while (q_base < nq) {
#pragma unroll
    for (int p = 0; p < DEPTH; ++p) {
      const int q = q_base + p * NW;
      if (q < nq) {
        float z = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
          float o[4];
          cvt4(buf[p][it], o);
          const int j4 = lane + it * WAVE;
          const float4 wv = reinterpret_cast<const float4*>(w_lds)[j4];
          z += o[0] * wv.x + o[1] * wv.y + o[2] * wv.z + o[3] * wv.w;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
          z += __shfl_xor(z, off, WAVE);
        const float coeff = coeff_of(q, z);
        ++n_done;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
          float o[4];
          cvt4(buf[p][it], o);
          const int j4 = lane + it * WAVE;
          float4* gw4 = reinterpret_cast<float4*>(gw);
          float4 cur = gw4[j4];
          cur.x += coeff * o[0]; cur.y += coeff * o[1];
          cur.z += coeff * o[2]; cur.w += coeff * o[3];
          gw4[j4] = cur;
        }
        // refill this buffer DEPTH rows ahead (clamped: see prologue).
        // sched_barrier pins every read of buf[p] (the accumulate above)
        // BEFORE the async refill overwrites it — the compiler treats an
        // asm load's register write as instantaneous and would otherwise
        // rotate reads past the issue (observed: regalloc preservation
        // copies racing the in-flight load).
        __builtin_amdgcn_sched_barrier(0);
        const int qf = min(q + DEPTH * NW, nq - 1);
        {
          const int rr2 = __builtin_amdgcn_readfirstlane(rowq[qf]);
          const auto rs2 = row_rsrc<XT>(X, total_elems, rr2, d);
#pragma unroll
          for (int it = 0; it < ITERS; ++it)
            buf[p][it] = RV::load(rs2, (lane + it * WAVE) << RV::VOFF_SHIFT);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    q_base += DEPTH * NW;
  }
  return n_done;
}

// Slab flush of the graph engine's forms: the block's [NW][DPAD] wave slabs
// summed into its column of the transposed partials, g_part[j*G + bid]
// (plain stores; reduce_partials sums the G columns).
template <int PBLOCK, int NW, int DPAD>
__device__ __forceinline__ void flush_partials(const float* gacc,
                                               float* __restrict__ g_part,
                                               int d, size_t G, int bid) {
  for (int j = threadIdx.x; j < d; j += PBLOCK) {
    float s = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < NW; ++s2) s += gacc[(size_t)s2 * DPAD + j];
    g_part[(size_t)j * G + bid] = s;
  }
}

// Standalone mask scan: fills a GLOBAL compacted row list (+ prefetched y
// values) for a FUTURE round. The scan depends only on (seed, round), not on
// w — so the graph engine runs round r+1's scan on a side stream overlapped
// with round r's gradient/update. The round key comes from a dedicated
// scan_round counter bumped stream-order by bump_counter_kernel (reading
// k_dev here would race the concurrent update's k++).
__device__ void scan_rows_body(
    const float* __restrict__ y, int* __restrict__ rowlist,
    float* __restrict__ ylist, int* __restrict__ count_dev,
    const int* __restrict__ scan_round_dev, long n_rows, uint64_t seed,
    uint32_t round_k, uint64_t row_start, uint32_t threshold, int take_all,
    int bid, int nblk) {
  if (scan_round_dev) round_k = (uint32_t)(*scan_round_dev);
  __shared__ int rows_s[QCAP];
  __shared__ int qn_s, base_s;
  if (threadIdx.x == 0) qn_s = 0;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long ngroups = (n_rows + ROWS_PER_BLOCK_ITER - 1) / ROWS_PER_BLOCK_ITER;
  long gi = bid;
  bool done = false;
  while (!done) {
    scan_enqueue<ROWS_PER_BLOCK_ITER>(rows_s, &qn_s, QCAP, gi, ngroups, nblk,
                                      n_rows, seed, round_k, row_start,
                                      threshold, take_all, wave, lane);
    __syncthreads();
    const int nq = min(qn_s, QCAP);
    if (threadIdx.x == 0 && nq > 0) base_s = atomicAdd(count_dev, nq);
    __syncthreads();
    for (int i = threadIdx.x; i < nq; i += BLOCK) {
      const int r = rows_s[i];
      rowlist[base_s + i] = r;
      ylist[base_s + i] = y[r];
    }
    __syncthreads();
    if (threadIdx.x == 0) qn_s = 0;
    done = gi >= ngroups;
  }
}

__global__ __launch_bounds__(BLOCK) void scan_rows_kernel(
    const float* __restrict__ y, int* __restrict__ rowlist,
    float* __restrict__ ylist, int* __restrict__ count_dev,
    const int* __restrict__ scan_round_dev, long n_rows, uint64_t seed,
    uint32_t round_k, uint64_t row_start, uint32_t threshold, int take_all) {
  scan_rows_body(y, rowlist, ylist, count_dev, scan_round_dev, n_rows, seed,
                 round_k, row_start, threshold, take_all, blockIdx.x,
                 gridDim.x);
}

__global__ void bump_counter_kernel(int* __restrict__ p) { *p += 1; }

// List-fed gradient: the process phase of the pipe kernel, consuming a
// globally compacted (rowlist, ylist) produced by scan_rows_kernel. Each
// block stages its contiguous slice into LDS first (per-row ordinary
// global loads inside the pipeline would reintroduce the vmcnt(0) drains).
template <typename XT, int PBLOCK, int DEPTH, int ITERS, bool HINGE>
__global__ __launch_bounds__(PBLOCK) void grad_dense_list_kernel(
    const XT* __restrict__ X, const float* __restrict__ w,
    float* __restrict__ g_part, const int* __restrict__ rowlist,
    const float* __restrict__ ylist, const int* __restrict__ count_dev,
    long n_rows, int d, int objective) {
  static_assert(PBLOCK == PIPE_BLOCK, "LDS sizes assume PIPE_BLOCK threads");
  constexpr int NW = PIPE_NW;
  constexpr int DPAD = pipe_dpad(ITERS);
  extern __shared__ float smem[];
  float* w_lds = smem;                                // [DPAD]
  float* gacc = smem + DPAD;                          // [NW][DPAD]
  float* yq = smem + (size_t)(1 + NW) * DPAD;         // [QCAP]
  int* rowq = (int*)(yq + QCAP);                      // [QCAP]
  for (int j = threadIdx.x; j < DPAD; j += PBLOCK) {
    w_lds[j] = j < d ? w[j] : 0.f;
#pragma unroll
    for (int s2 = 0; s2 < NW; ++s2) gacc[(size_t)s2 * DPAD + j] = 0.f;
  }
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float* gw = gacc + (size_t)wave * DPAD;
  const long total_elems = n_rows * (long)d;
  const int total = *count_dev;
  const int per_block = (total + gridDim.x - 1) / gridDim.x;
  const int my0 = blockIdx.x * per_block;
  const int my1 = min(total, my0 + per_block);
  for (int off = my0; off < my1; off += QCAP) {
    const int nq = min(my1 - off, QCAP);
    __syncthreads();
    for (int i = threadIdx.x; i < nq; i += PBLOCK) {
      rowq[i] = rowlist[off + i];
      yq[i] = ylist[off + i];
    }
    __syncthreads();
    pipe_drain<XT, NW, DEPTH, ITERS>(
        X, total_elems, d, rowq, nq, w_lds, gw, wave, lane,
        [&](int q, float z) {
          return link_residual<HINGE>(z, yq[q], objective);
        });
  }
  __syncthreads();
  flush_partials<PBLOCK, NW, DPAD>(gacc, g_part, d, gridDim.x, blockIdx.x);
}

// __forceinline__ is load-bearing: left out of line, the body inherits no
// launch bounds from its kernels and takes the whole register file.
template <typename XT, bool SAGA, int PBLOCK, int DEPTH, int ITERS,
          bool HINGE>
__device__ __forceinline__ void grad_dense_pipe_body(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ w, float* __restrict__ g_out,
    float* __restrict__ g_part, int* __restrict__ n_out,
    float* __restrict__ alpha, int* __restrict__ idx_out,
    float* __restrict__ e_out, int* __restrict__ pos_ctr,
    const int* __restrict__ k_dev, int commit_now, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, uint32_t threshold,
    int take_all, int objective, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr, int bid,
    int nblk) {
  if (k_dev) round_k = (uint32_t)(*k_dev) + 1u;
  static_assert(PBLOCK == PIPE_BLOCK, "LDS sizes assume PIPE_BLOCK threads");
  constexpr int NW = PIPE_NW;
  constexpr int RPB = NW * ROWS_PER_WAVE;
  constexpr int DPAD = pipe_dpad(ITERS);  // padded feature dim
  static_assert(QCAP >= RPB + 1024, "queue must out-size one scan iter");
  extern __shared__ float smem[];
  float* w_lds = smem;                               // [DPAD]
  float* gacc = smem + DPAD;                         // [NW][DPAD]
  float* yq = smem + (size_t)(1 + NW) * DPAD;        // [QCAP]
  float* aq = yq + QCAP;                             // [QCAP] (SAGA)
  float* eq = aq + (SAGA ? QCAP : 0);                // [QCAP] (SAGA)
  int* rowq = (int*)(eq + (SAGA ? QCAP : 0));        // [QCAP]
  int* qn = rowq + QCAP;
  for (int j = threadIdx.x; j < DPAD; j += PBLOCK) {
    w_lds[j] = j < d ? w[j] : 0.f;
#pragma unroll
    for (int s2 = 0; s2 < NW; ++s2) gacc[(size_t)s2 * DPAD + j] = 0.f;
  }
  if (threadIdx.x == 0) *qn = 0;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float* gw = gacc + (size_t)wave * DPAD;
  int local_count = 0;
  const long total_elems = n_rows * (long)d;

  const long ngroups = (n_rows + RPB - 1) / RPB;
  long gi = bid;
  bool done = false;
  while (!done) {
    // ---- scan phase
    scan_enqueue<RPB>(rowq, qn, QCAP, gi, ngroups, nblk, n_rows, seed,
                      round_k, row_start, threshold, take_all, wave, lane);
    __syncthreads();
    const int nq = min(*qn, QCAP);
    // ---- fetch phase: y (and the SAGA history scalar) for the whole queue
    // in one strided pass, all loads in flight at once
    for (int pos = threadIdx.x; pos < nq; pos += PBLOCK) {
      const int row = rowq[pos];
      yq[pos] = y[row];
      if (SAGA) aq[pos] = alpha[row];
    }
    __syncthreads();
    // ---- process phase
    local_count += pipe_drain<XT, NW, DEPTH, ITERS>(
        X, total_elems, d, rowq, nq, w_lds, gw, wave, lane,
        [&](int q, float z) {
          const float e = link_residual<HINGE>(z, yq[q], objective);
          if (!SAGA) return e;
          const float coeff = e - aq[q];
          if (lane == 0) eq[q] = e;  // committed after the barrier
          return coeff;
        });
    __syncthreads();
    if (SAGA) {
      // history scalar emit/commit, batched outside the pipeline
      for (int pos = threadIdx.x; pos < nq; pos += PBLOCK) {
        const int row = rowq[pos];
        const float e = eq[pos];
        if (commit_now) {
          alpha[row] = e;
        } else {
          // atomic staging: read cross-stream in wave mode
          const int gpos = atomicAdd(pos_ctr, 1);
          __hip_atomic_exchange(&idx_out[gpos], row, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_exchange(&e_out[gpos], e, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) *qn = 0;
    done = gi >= ngroups;
  }
  __syncthreads();
  if (g_part != nullptr) {
    flush_partials<PBLOCK, NW, DPAD>(gacc, g_part, d, nblk, bid);
  } else {
    for (int j = threadIdx.x; j < d; j += PBLOCK) {
      float s = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < NW; ++s2) s += gacc[(size_t)s2 * DPAD + j];
      if (s != 0.f) atomicAdd(&g_out[j], s);
    }
  }
  if (lane == 0 && local_count) atomicAdd(n_out, local_count);
  publish_done(done_flag, done_val, done_arr, nblk);
}

template <typename XT, bool SAGA, int PBLOCK, int DEPTH, int ITERS,
          bool HINGE>
__global__
__launch_bounds__(PBLOCK, (PipeShape<XT, SAGA, DEPTH, ITERS>::HINT))
void grad_dense_pipe_kernel(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ w, float* __restrict__ g_out,
    float* __restrict__ g_part, int* __restrict__ n_out,
    float* __restrict__ alpha, int* __restrict__ idx_out,
    float* __restrict__ e_out, int* __restrict__ pos_ctr,
    const int* __restrict__ k_dev, int commit_now, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, uint32_t threshold,
    int take_all, int objective, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr) {
  grad_dense_pipe_body<XT, SAGA, PBLOCK, DEPTH, ITERS, HINGE>(
      X, y, w, g_out, g_part, n_out, alpha, idx_out, e_out, pos_ctr, k_dev,
      commit_now, n_rows, d, seed, round_k, row_start, threshold, take_all,
      objective, done_flag, done_val, done_arr, blockIdx.x, gridDim.x);
}

// ---- wave launch: ONE kernel runs a whole quorum wave of dense-ASGD
// rounds (the native engine previously paid ~5 us of launch latency per
// worker per wave). Block b serves wave slot b / bper with intra-worker
// block id b % bper; each worker's sub-grid publishes its OWN done flag
// as it drains, so completions still stagger exactly as with per-worker
// kernels. Per-worker invariants (X, y, wbuf, g, n_rows, flags) live in a
// device table built once at engine init; the per-round variables (slot
// list, Philox round keys, serials) travel by value in the launch args.
template <typename XT, bool SAGA, int PBLOCK, int DEPTH, int ITERS,
          bool HINGE>
__global__
__launch_bounds__(PBLOCK, (PipeShape<XT, SAGA, DEPTH, ITERS>::HINT))
void grad_dense_wave_kernel(
    const GradWaveSlot* __restrict__ slots, GradWaveCmd cmd, int d,
    uint64_t seed, uint32_t threshold, int take_all, int objective) {
  const int si = cmd.interleave ? (int)(blockIdx.x % cmd.n)
                                : (int)(blockIdx.x / cmd.bper);
  const int bid = cmd.interleave ? (int)(blockIdx.x / cmd.n)
                                 : (int)(blockIdx.x % cmd.bper);
  const GradWaveSlot sl = slots[cmd.wid[si]];
  grad_dense_pipe_body<XT, SAGA, PBLOCK, DEPTH, ITERS, HINGE>(
      (const XT*)sl.X, sl.y, sl.wbuf, sl.g, nullptr, sl.n_out, sl.alpha,
      sl.idx_out, sl.e_out, sl.pos_ctr, nullptr, 0, sl.n_rows, d, seed,
      cmd.round_k[si], (uint64_t)sl.row_start, threshold, take_all,
      objective, sl.done_flag, cmd.done_val[si], sl.done_arr, bid,
      cmd.bper);
}


// Sums the per-block partial slabs into g (layout g_part[j][G], contiguous
// per column). Grid = ceil(d/BLOCK) * SPLITS.
__global__ __launch_bounds__(BLOCK) void reduce_partials_kernel(
    const float* __restrict__ g_part, float* __restrict__ g_out, int d,
    int G, int splits) {
  const int njc = (d + BLOCK - 1) / BLOCK;
  const int jc = blockIdx.x % njc;
  const int sp = blockIdx.x / njc;
  const int j = jc * BLOCK + threadIdx.x;
  if (j >= d) return;
  const int per = (G + splits - 1) / splits;
  const int b0 = sp * per;
  const int b1 = min(G, b0 + per);
  const float* base = g_part + (size_t)j * G;
  float s = 0.f;
  if (((b1 - b0) & 3) == 0 && (b0 & 3) == 0) {
    const float4* v = reinterpret_cast<const float4*>(base + b0);
    const int n4 = (b1 - b0) >> 2;
    for (int q = 0; q < n4; ++q) {
      const float4 x = v[q];
      s += x.x + x.y + x.z + x.w;
    }
  } else {
    for (int b = b0; b < b1; ++b) s += base[b];
  }
  if (splits == 1) g_out[j] += s;
  else atomicAdd(&g_out[j], s);
}

// ---------------------------------------------------------------- K2 (+K3)

// LPR = lanes per row: rcv1-class rows have ~73 nnz, so a 64-lane row
// wastes most of the wave; 16-lane sub-waves keep 4 rows in flight per
// wave (the gradient scatter uses global atomics — no LDS slabs — so
// unlike the dense kernel, sub-waves here cost no occupancy).
template <typename VT, bool SAGA, int LPR, bool HINGE>
__device__ void grad_csr_body(
    const int* __restrict__ indptr, const int* __restrict__ indices,
    const VT* __restrict__ values, const float* __restrict__ y,
    const float* __restrict__ w, float* __restrict__ g_out,
    int* __restrict__ n_out, float* __restrict__ alpha,
    int* __restrict__ idx_out, float* __restrict__ e_out,
    int* __restrict__ pos_ctr, const int* __restrict__ k_dev,
    int commit_now, long n_rows, uint64_t seed, uint32_t round_k,
    uint64_t row_start, uint32_t threshold, int take_all, int objective,
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr, int bid, int nblk) {
  if (k_dev) round_k = (uint32_t)(*k_dev) + 1u;
  constexpr int NSUB = WAVE / LPR;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR;
  const int sl = lane % LPR;
  int local_count = 0;
  const long gstride = (long)nblk * ROWS_PER_BLOCK_ITER;
  for (long bb = (long)bid * ROWS_PER_BLOCK_ITER; bb < n_rows;
       bb += gstride) {
    const long base = bb + (long)wave * ROWS_PER_WAVE;
    if (base >= n_rows) continue;
    const uint4 x = philox_block4(
        seed, round_k, (row_start + (uint64_t)base) / 4 + (uint64_t)lane);
    const long rem = n_rows - base;
    unsigned long long m[4];
    {
      const long lrow = 4L * lane;
      m[0] = __ballot(lrow + 0 < rem && (take_all || x.x < threshold));
      m[1] = __ballot(lrow + 1 < rem && (take_all || x.y < threshold));
      m[2] = __ballot(lrow + 2 < rem && (take_all || x.z < threshold));
      m[3] = __ballot(lrow + 3 < rem && (take_all || x.w < threshold));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned long long mm = m[i];
      for (int s2 = 0; s2 < sub && mm; ++s2) mm &= mm - 1;  // my first bit
      while (mm) {
        const int bit = __ffsll((long long)mm) - 1;
        const long rr = base + 4L * bit + i;
        const int s = indptr[rr], t = indptr[rr + 1];
        float z = 0.f;
        for (int p = s + sl; p < t; p += LPR)
          z += to_f32<VT>(values[p]) * w[indices[p]];
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1)
          z += __shfl_xor(z, off, WAVE);
        float e = link_residual<HINGE>(z, y[rr], objective);
        float coeff = e;
        if (SAGA) {
          const float a_old = alpha[rr];
          coeff = e - a_old;
          if (sl == 0) {
            if (commit_now) {
              alpha[rr] = e;
            } else {
              // ATOMIC staging: the wave-mode commit kernel reads these
              // from another kernel with no stream-order edge, so the
              // writes must land at the agent coherence point (plain
              // stores can sit in one XCD's L2)
              const int pos = atomicAdd(pos_ctr, 1);
              __hip_atomic_exchange(&idx_out[pos], (int)rr,
                                    __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_exchange(&e_out[pos], e, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
        ++local_count;
        for (int p = s + sl; p < t; p += LPR)
          atomicAdd(&g_out[indices[p]], coeff * to_f32<VT>(values[p]));
        for (int s2 = 0; s2 < NSUB && mm; ++s2) mm &= mm - 1;  // next mine
      }
    }
  }
  if (sl == 0 && local_count) atomicAdd(n_out, local_count);
  publish_done(done_flag, done_val, done_arr, nblk);
}

template <typename VT, bool SAGA, int LPR, bool HINGE>
__global__ __launch_bounds__(BLOCK) void grad_csr_kernel(
    const int* __restrict__ indptr, const int* __restrict__ indices,
    const VT* __restrict__ values, const float* __restrict__ y,
    const float* __restrict__ w, float* __restrict__ g_out,
    int* __restrict__ n_out, float* __restrict__ alpha,
    int* __restrict__ idx_out, float* __restrict__ e_out,
    int* __restrict__ pos_ctr, const int* __restrict__ k_dev,
    int commit_now, long n_rows, uint64_t seed, uint32_t round_k,
    uint64_t row_start, uint32_t threshold, int take_all, int objective,
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr) {
  grad_csr_body<VT, SAGA, LPR, HINGE>(
      indptr, indices, values, y, w, g_out, n_out, alpha, idx_out, e_out,
      pos_ctr, k_dev, commit_now, n_rows, seed, round_k, row_start, threshold,
      take_all, objective, done_flag, done_val, done_arr, blockIdx.x,
      gridDim.x);
}

// CSR wave: one kernel per quorum wave (see grad_dense_wave_kernel)
template <typename VT, bool SAGA, int LPR, bool HINGE>
__global__ __launch_bounds__(BLOCK) void grad_csr_wave_kernel(
    const CsrWaveSlot* __restrict__ slots, GradWaveCmd cmd, uint64_t seed,
    uint32_t threshold, int take_all, int objective) {
  const int si = cmd.interleave ? (int)(blockIdx.x % cmd.n)
                                : (int)(blockIdx.x / cmd.bper);
  const int bid = cmd.interleave ? (int)(blockIdx.x / cmd.n)
                                 : (int)(blockIdx.x % cmd.bper);
  const CsrWaveSlot sl = slots[cmd.wid[si]];
  grad_csr_body<VT, SAGA, LPR, HINGE>(
      sl.indptr, sl.indices, (const VT*)sl.values, sl.y, sl.wbuf, sl.g,
      sl.n_out, sl.alpha, sl.idx_out, sl.e_out, sl.pos_ctr, nullptr, 0,
      sl.n_rows, seed, cmd.round_k[si], (uint64_t)sl.row_start, threshold,
      take_all, objective, sl.done_flag, cmd.done_val[si], sl.done_arr, bid,
      cmd.bper);
}

// SAGA commit + staging-reset pass for a whole wave, launched before the
// wave's grad kernel on the same stream. Scatters the previous accepted
// round's staged scalars into the worker-resident alpha slice
// (commit-gated) and resets the staging counter unconditionally (a
// REJECTED previous round must also restart its staging list). Reads use
// RMW loads: the staging was written by another kernel with no
// stream-order edge, so normal loads could hit a stale L2 line.
__device__ __forceinline__ int atomic_load_int(int* p) {
  return __hip_atomic_fetch_add(p, 0, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float atomic_load_f32(float* p) {
  return __hip_atomic_fetch_add(p, 0.f, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(BLOCK) void saga_commit_wave_kernel(
    const CommitSlot* __restrict__ slots, CsrCommitCmd cmd) {
  const int si = (int)(blockIdx.x % cmd.n);
  const int bid = (int)(blockIdx.x / cmd.n);
  const CommitSlot sl = slots[cmd.wid[si]];
  const int cnt = atomic_load_int(sl.pos_ctr);
  if (cmd.do_commit[si]) {
    for (int i = bid * BLOCK + threadIdx.x; i < cnt;
         i += cmd.bper * BLOCK) {
      const int r = atomic_load_int(&sl.idx[i]);
      const float e = atomic_load_f32(&sl.e[i]);
      sl.dst[r] = e;  // only this worker's rounds touch its slice
    }
  }
  // last block of the slot resets the staging + sample counters (reuses
  // done_arr, which is 0 between rounds; the wave's grad kernel is
  // stream-ordered after this kernel)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long a = __hip_atomic_fetch_add(
        sl.arr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a + 1 == (unsigned long long)cmd.bper) {
      (void)__hip_atomic_exchange(sl.arr, 0ull, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_exchange(sl.pos_ctr, 0, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_exchange(sl.n_out, 0, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      if (sl.scnt)
        (void)__hip_atomic_exchange(sl.scnt, 0, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_s_waitcnt(0);
    }
  }
}

// spill-refresh wave: per slot, recompute the round's Philox row set into
// (srows, scnt), then gather ONLY those entries from the pinned master
// into the device staging table (both stream-ordered before the wave's
// gradient). Slot-mapped wrappers over the singleton kernels' logic.
__global__ __launch_bounds__(BLOCK) void scan_rows_wave_kernel(
    const GradWaveSlot* __restrict__ slots, GradWaveCmd cmd, uint64_t seed,
    uint32_t threshold, int take_all) {
  const int si = (int)(blockIdx.x % cmd.n);
  const int bid = (int)(blockIdx.x / cmd.n);
  const GradWaveSlot sl = slots[cmd.wid[si]];
  scan_rows_body(sl.y, sl.srows, sl.sylist, sl.scnt, nullptr, sl.n_rows,
                 seed, cmd.round_k[si], (uint64_t)sl.row_start, threshold,
                 take_all, bid, cmd.bper);
}

__global__ void alpha_gather_wave_kernel(
    const GradWaveSlot* __restrict__ slots, GradWaveCmd cmd) {
  const int si = (int)(blockIdx.x % cmd.n);
  const int bid = (int)(blockIdx.x / cmd.n);
  const GradWaveSlot sl = slots[cmd.wid[si]];
  const int n = *sl.scnt;  // same stream as the scan: plain read is fine
  for (int i = bid * BLOCK + threadIdx.x; i < n; i += cmd.bper * BLOCK) {
    const int r = sl.srows[i];
    sl.alpha[r] = sl.alpha_host[r];
  }
}


// ---------------------------------------------------------------- K5/K6
// Every kernel below applies asgd_step / saga_step of update_step.h (the
// arithmetic, plain and elastic-net, is defined and explained there) to a
// value it holds in a register: no REG form adds a global load or store.

// the REG scale is an explicit single rounding, like the rest of that step
template <bool REG>
__device__ __forceinline__ float step_scale(float gamma_k, float inv_batch) {
  if constexpr (REG) return __fmul_rn(gamma_k, inv_batch);
  else return gamma_k * inv_batch;
}

template <bool REG>
__global__ void sgd_update_kernel(float* __restrict__ w,
                                  const float* __restrict__ g, float gamma_k,
                                  float inv_batch, int d, float l2,
                                  float l1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d)
    asgd_step<REG>(w[i], g[i], step_scale<REG>(gamma_k, inv_batch),
                   reg_dec(gamma_k, l2), reg_thr(gamma_k, l1));
}

template <bool REG>
__global__ void saga_update_kernel(float* __restrict__ w,
                                   const float* __restrict__ g,
                                   float* __restrict__ alpha_bar, float gamma,
                                   float inv_batch, float inv_N, int d,
                                   float l2, float l1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d)
    saga_step<REG>(w[i], alpha_bar[i], g[i], gamma, inv_batch, inv_N,
                   reg_dec(gamma, l2), reg_thr(gamma, l1));
}

__global__ void saga_commit_kernel(float* __restrict__ alpha,
                                   const int* __restrict__ idx,
                                   const float* __restrict__ e, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) alpha[idx[i]] = e[i];
}

// Host-spill refresh (BASELINE config 5): pull ONLY the round's sampled
// history scalars from the pinned-host master table into the device
// staging table (a_dst[rows[j]] = a_src[rows[j]]). a_src is a pinned host
// pointer — ROCm pinned allocations are device-visible, so the gather is
// ~n_sampled coalesced-issue 4 B reads over the host link instead of the
// whole-table hipMemcpy the round-1 path did. rows/count come from
// scan_rows_kernel with the same Philox key the gradient kernel uses.
__global__ void alpha_gather_kernel(float* __restrict__ a_dst,
                                    const float* __restrict__ a_src,
                                    const int* __restrict__ rows,
                                    const int* __restrict__ count_dev) {
  const int n = *count_dev;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int r = rows[i];
    a_dst[r] = a_src[r];
  }
}

// Commit with the staged count read on-device (n_dev = &ctr[1], written by
// the SAGA gradient kernel): removes the native engine's per-accept 4-byte
// D2H sync. Grid is sized for the staging capacity; excess blocks exit on
// the bound check.
__global__ void saga_commit_devn_kernel(float* __restrict__ alpha,
                                        const int* __restrict__ idx,
                                        const float* __restrict__ e,
                                        const int* __restrict__ n_dev) {
  const int n = *n_dev;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) alpha[idx[i]] = e[i];
}

// ---------------------------------------------------------- batched update
// (native engine): ONE kernel applies a whole sweep of accepted gradients —
// elementwise-sequentially, so the result is bit-identical to launching the
// per-round update kernels back to back — zeroes the consumed gradient
// accumulators, and writes the post-batch w into the weight-snapshot
// buffers of the workers being redispatched (the versioned-broadcast copy
// that dispatch() otherwise does with a separate hipMemcpyAsync each).
// Pointer tables (g_tab/wbuf_tab, one slot per worker) live on the device;
// the per-batch worker ids + ASGD step scales ride in the kernel-arg block
// (<= 4 KB), so a batch costs exactly one launch and no H2D staging.
#include "multi_update.h"

// The batch's gradients are FETCHED first, MU_CHUNK at a time (pointer from
// g_tab, then g[i]; unconditional loads with a clamped index so all of a
// chunk's loads are in flight together), then APPLIED to wi (and alpha_bar)
// in the same j order with the same expressions as a plain sequential loop,
// and only then are the consumed accumulators zeroed. A `g[i] = 0` store
// interleaved with the loads would serialize them into a chain of 2n
// dependent global loads. Deferring the zero stores is valid only because a
// worker id appears AT MOST ONCE per batch (the engine redispatches a worker
// only after the flush; checked on the host where the batch is assembled).
// VEC4 (d % 4 == 0, 16-byte-aligned buffers) moves float4 per lane: d=784
// is 196 lanes over 4 blocks of 64.
#define MU_BLOCK 64
#define MU_CHUNK 8

// REG applies the elastic-net step once per accepted gradient, in
// batch order — n gradients are n decay-and-threshold steps, the same as n
// singleton launches — with eta = a.eta[j] (ASGD) or gamma (ASAGA). Only
// the apply stage's arithmetic differs: same global loads, same stores, so
// the snapshot targets receive the post-threshold w.
template <bool VEC4, bool REG>
__global__ __launch_bounds__(MU_BLOCK) void multi_update_kernel(
    float* __restrict__ w, float* const* __restrict__ g_tab,
    float* const* __restrict__ wbuf_tab, float* __restrict__ alpha_bar,
    float gamma, float inv_batch, float inv_N, int d, float l2, float l1,
    MultiUpdateArgs a) {
  using V = typename std::conditional<VEC4, float4, float>::type;
  const int nel = VEC4 ? d >> 2 : d;
  const V zero = V{};
  for (int i = blockIdx.x * MU_BLOCK + threadIdx.x; i < nel;
       i += gridDim.x * MU_BLOCK) {
    V wi = reinterpret_cast<const V*>(w)[i];
    V ab = zero;
    if (a.algo != 0) ab = reinterpret_cast<const V*>(alpha_bar)[i];
    for (int j0 = 0; j0 < a.n; j0 += MU_CHUNK) {
      V gv[MU_CHUNK];
      // REG: the chunk's per-gradient steps, fetched with the gradients
      // (j0 + c < MU_MAX: in bounds, entries past n are never applied) so
      // the apply stage waits for no kernel-argument load per gradient
      [[maybe_unused]] float sc_c[MU_CHUNK], eta_c[MU_CHUNK];
      if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < MU_CHUNK; ++c) {
          sc_c[c] = a.scale[j0 + c];
          eta_c[c] = a.eta[j0 + c];
        }
      }
#pragma unroll
      for (int c = 0; c < MU_CHUNK; ++c) {
        const int j = min(j0 + c, a.n - 1);
        gv[c] = reinterpret_cast<const V*>(g_tab[a.gw[j]])[i];
      }
#pragma unroll
      for (int c = 0; c < MU_CHUNK; ++c) {
        const int j = j0 + c;
        if (j < a.n) {
          float dec = 1.f, t = 0.f;
          if constexpr (REG) {
            const float eta = a.algo == 0 ? eta_c[c] : gamma;
            dec = reg_dec(eta, l2);
            t = reg_thr(eta, l1);
          }
          if (a.algo == 0) {
            const float sc = REG ? sc_c[c] : a.scale[j];
            for_lanes([&](float& w1, float g1) {
              asgd_step<REG>(w1, g1, sc, dec, t);
            }, wi, gv[c]);
          } else {
            for_lanes([&](float& w1, float& ab1, float g1) {
              saga_step<REG>(w1, ab1, g1, gamma, inv_batch, inv_N, dec, t);
            }, wi, ab, gv[c]);
          }
        }
      }
    }
    for (int j = 0; j < a.n; ++j)
      reinterpret_cast<V*>(g_tab[a.gw[j]])[i] = zero;
    if (a.algo != 0) reinterpret_cast<V*>(alpha_bar)[i] = ab;
    reinterpret_cast<V*>(w)[i] = wi;
    for (int j = 0; j < a.m; ++j)
      reinterpret_cast<V*>(wbuf_tab[a.sw[j]])[i] = wi;
  }
}

// ------------------------------------------------------ sync round update
// (native engine, synchronous mode): ONE kernel applies ONE barrier round.
// multi_update_kernel cannot do this job — it applies its gradients one
// after another (SAGA would add alpha_bar P times) and has no MLlib
// divisor. Per element i:
//   s = sum_p g_p[i] in FIXED worker order 0..P-1 (deterministic: the result
//       does not depend on which worker's kernel blocks finished first);
//   g_p[i] = 0 for all p (the next round accumulates from zero);
//   mode 0 asgd : w -= scale * s            (scale = gamma_k / (b*N), host)
//   mode 1 asaga: w -= gamma * (inv_batch*s + alpha_bar); alpha_bar += s/N
//                 (w reads the OLD alpha_bar, as saga_update_kernel)
//   mode 2 mllib: w -= scale * s / max(n,1) (scale = gamma_k, host;
//                 n = sum_p ctr_p[0], the round's ACTUAL sample count, read
//                 here on the device — no D2H);
//   REG: the same step with the elastic-net terms (update_step.h), once
//                 per round: v = dec*w - step*s (asgd/mllib, step = the
//                 scale above) or dec*w - gamma*(inv_batch*s + alpha_bar)
//                 (asaga), then the soft-threshold. ``eta`` is the bare
//                 step (gamma_k; gamma for asaga) — separate from scale,
//                 which mllib mode divides by the sample count;
//   snap_dst[i] = post-update (REG: post-threshold) w[i] when snap_dst !=
//                 null (fused optVars snapshot copy).
// Everything read here (g_p, ctr_p) was written by the gradient kernel that
// precedes this one ON THE SAME STREAM, so plain loads are correct — unlike
// the async path, whose cross-stream consumers need agent-scope atomics.
// The sample counters are zeroed for the next round by the LAST block to
// finish (atomic ticket, as sgd_reduce_update_kernel): every block has
// already parked its counter sum in LDS before it takes a ticket, so the
// reset races no read.
#define SRU_BLOCK 64

template <bool VEC4, bool REG>
__global__ __launch_bounds__(SRU_BLOCK) void sync_round_update_kernel(
    float* __restrict__ w, float* const* __restrict__ g_tab,
    int* const* __restrict__ ctr_tab, float* __restrict__ alpha_bar,
    float* __restrict__ snap_dst, int* __restrict__ ticket, int P, int d,
    int mode, float scale, float gamma, float inv_batch, float inv_N,
    float eta, float l2, float l1) {
  __shared__ int n_sh;
  if (mode == 2) {  // uniform per launch
    if (threadIdx.x == 0) {
      int n = 0;
      for (int p = 0; p < P; ++p) n += *ctr_tab[p];
      n_sh = n;
    }
    __syncthreads();
    scale = scale / (float)max(n_sh, 1);
  }
  [[maybe_unused]] const float dec = REG ? reg_dec(eta, l2) : 1.f;
  [[maybe_unused]] const float thr = REG ? reg_thr(eta, l1) : 0.f;
  using V = typename std::conditional<VEC4, float4, float>::type;
  const int nel = VEC4 ? d >> 2 : d;
  const int stride = gridDim.x * SRU_BLOCK;
  for (int i = blockIdx.x * SRU_BLOCK + threadIdx.x; i < nel; i += stride) {
    V s = V{};
#pragma unroll 8
    for (int p = 0; p < P; ++p) {
      const V v = reinterpret_cast<const V*>(g_tab[p])[i];
      for_lanes([](float& s1, float v1) { s1 += v1; }, s, v);
    }
    for (int p = 0; p < P; ++p) reinterpret_cast<V*>(g_tab[p])[i] = V{};
    V wi = reinterpret_cast<V*>(w)[i];
    if (mode == 1) {
      V ab = reinterpret_cast<V*>(alpha_bar)[i];
      for_lanes([&](float& w1, float& ab1, float s1) {
        saga_step<REG>(w1, ab1, s1, gamma, inv_batch, inv_N, dec, thr);
      }, wi, ab, s);
      reinterpret_cast<V*>(alpha_bar)[i] = ab;
    } else {
      for_lanes([&](float& w1, float s1) {
        asgd_step<REG>(w1, s1, scale, dec, thr);
      }, wi, s);
    }
    reinterpret_cast<V*>(w)[i] = wi;
    if (snap_dst) reinterpret_cast<V*>(snap_dst)[i] = wi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = atomicAdd(ticket, 1);
    if (t == (int)gridDim.x - 1) {
      for (int p = 0; p < P; ++p) *ctr_tab[p] = 0;
      (void)__hip_atomic_exchange(ticket, 0, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Fused reduce+update (overlap graph mode): one kernel sums the per-block
// partial slabs AND applies the ASGD update. Each block reads k at entry
// (k is stable for the whole kernel); the last-finishing block (atomic
// ticket) advances k — every other block has already finished, and the
// last block read k at its own start, so the increment races nothing.
__global__ __launch_bounds__(BLOCK) void sgd_reduce_update_kernel(
    const float* __restrict__ g_part, float* __restrict__ w,
    int* __restrict__ k_dev, int* __restrict__ ticket, float gamma,
    float inv_batch, int num_part, int d, int G, int splits) {
  const int k = *k_dev;
  const float gamma_k =
      (float)((double)gamma / sqrt((double)(k / num_part + 1)));
  const int njc = (d + BLOCK - 1) / BLOCK;
  const int jc = blockIdx.x % njc;
  const int sp = blockIdx.x / njc;
  const int j = jc * BLOCK + threadIdx.x;
  if (j < d) {
    const int per = (G + splits - 1) / splits;
    const int b0 = sp * per;
    const int b1 = min(G, b0 + per);
    const float* base = g_part + (size_t)j * G;
    float s = 0.f;
    if (((b1 - b0) & 3) == 0 && (b0 & 3) == 0) {
      const float4* v = reinterpret_cast<const float4*>(base + b0);
      const int n4 = (b1 - b0) >> 2;
      for (int q = 0; q < n4; ++q) {
        const float4 x = v[q];
        s += x.x + x.y + x.z + x.w;
      }
    } else {
      for (int b = b0; b < b1; ++b) s += base[b];
    }
    if (splits == 1) {
      asgd_step<false>(w[j], s, gamma_k * inv_batch);
    } else {
      atomicAdd(&w[j], -gamma_k * inv_batch * s);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = atomicAdd(ticket, 1);
    if (t == (int)gridDim.x - 1) {
      *ticket = 0;
      *k_dev = k + 1;
    }
  }
}

// Fused device-loop update kernels (graph mode): ONE workgroup applies the
// update, zeroes the gradient accumulator for the next round, and advances
// the device round counter — so an unrolled sequence of
// [grad, reduce, update] node triples forms a complete hipGraph with no
// host logic.
__global__ __launch_bounds__(1024) void sgd_update_fused_kernel(
    float* __restrict__ w, float* __restrict__ g, int* __restrict__ k_dev,
    float gamma, float inv_batch, int num_part, int d) {
  const int k = *k_dev;
  // integer division k/num_part matches the reference's Scala Int semantics
  // (SparkASGDThread.scala:190)
  const float gamma_k =
      (float)((double)gamma / sqrt((double)(k / num_part + 1)));
  for (int i = threadIdx.x; i < d; i += blockDim.x) {
    asgd_step<false>(w[i], g[i], gamma_k * inv_batch);
    g[i] = 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) *k_dev = k + 1;
}

__global__ __launch_bounds__(1024) void saga_update_fused_kernel(
    float* __restrict__ w, float* __restrict__ g,
    float* __restrict__ alpha_bar, int* __restrict__ k_dev, float gamma,
    float inv_batch, float inv_N, int d) {
  for (int i = threadIdx.x; i < d; i += blockDim.x) {
    saga_step<false>(w[i], alpha_bar[i], g[i], gamma, inv_batch, inv_N);
    g[i] = 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) *k_dev += 1;
}

// ---------------------------------------------------------------- launchers

static inline int grad_grid(long n_rows) {
  const char* s = std::getenv("ASYNCAMD_GRAD_GRID");  // re-read: sweeps
  const int override_grid = s ? std::atoi(s) : 0;
  if (override_grid > 0) return override_grid;
  long g = (n_rows + ROWS_PER_BLOCK_ITER - 1) / ROWS_PER_BLOCK_ITER;
  if (g > 512) g = 512;  // measured optimum on 8.1M rows (pipe kernel)
  if (g < 1) g = 1;
  return (int)g;
}

static inline int pick_lpr(int d) {
  const char* s = std::getenv("ASYNCAMD_LPR");
  const int override_lpr = s ? std::atoi(s) : 0;
  if (override_lpr == 64 || override_lpr == 32 || override_lpr == 16)
    return override_lpr;
  // measured on the mnist8m shape: LPR 64 > 32 > 16 (sub-wave rows cost LDS
  // occupancy more than the extra MLP buys) — keep whole-wave rows
  return 64;
}

// Pipelined-kernel template parameters for a feature dim (callers guarantee
// d % 4 == 0 and d <= 2048). Depth: measured on the wave kernel, 6 wins at
// ITERS <= 4 and 4 at the wider fp32 shapes (profiles/r04_grad_occupancy.md);
// solo and list launches keep 4. ASYNCAMD_PIPE_DEPTH overrides (1, 2, 4, 6
// or 8; any other value runs as 4) for the pipe, wave and list kernels.
static inline int pipe_iters(int d) {
  const int it = (d + 255) / 256;
  return it < 1 ? 1 : (it > 8 ? 8 : it);
}
static inline int pipe_depth(int iters, bool wave) {
  const char* dps = std::getenv("ASYNCAMD_PIPE_DEPTH");  // re-read: sweeps
  const int depth = dps ? std::atoi(dps) : (wave && iters <= 4 ? 6 : 4);
  return (depth == 1 || depth == 2 || depth == 6 || depth == 8) ? depth : 4;
}

// ---- runtime value -> template argument. Every launcher picks its
// instantiation through these three; there are no launch macros.
//
// f(integral_constant<int, V>) for the candidate V equal to v — the LAST
// candidate when none is (so the last one is the default).
template <int V0, int... Vs, typename F>
static void with_const(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else with_const<Vs...>(v, f);
}
// f(bool_constant<b>) for a runtime flag
template <typename F>
static void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// f(element-type tag value, bool_constant<saga>) for a data matrix's runtime
// (is_bf16, saga) pair; the element type is decltype of the first argument
template <typename F>
static void with_xt_saga(int is_bf16, int saga, F&& f) {
  with_bool(saga != 0, [&](auto SG) {
    if (is_bf16) f(__hip_bfloat16{}, SG);
    else f(float{}, SG);
  });
}
// the gradient launchers' form: + bool_constant<objective is hinge>, the
// kernels' HINGE argument (link.h)
template <typename F>
static void with_xt_saga_obj(int is_bf16, int saga, int objective, F&& f) {
  with_xt_saga(is_bf16, saga, [&](auto xt, auto SG) {
    with_bool(objective == 2, [&](auto HG) { f(xt, SG, HG); });
  });
}

// f(integral_constant<ITERS>, integral_constant<DEPTH>) for the runtime
// (iters, depth) pair: the one switch over the instantiated shapes.
template <typename F>
static void with_pipe_shape(int iters, int depth, F&& f) {
  with_const<1, 2, 3, 4, 5, 6, 7, 8>(iters, [&](auto IT) {
    with_const<1, 2, 6, 8, 4>(depth, [&](auto DP) { f(IT, DP); });
  });
}

static inline int csr_lpr() {
  const char* s = std::getenv("ASYNCAMD_CSR_LPR");
  const int v = s ? std::atoi(s) : 32;  // measured best on rcv1 shape
  return (v == 8 || v == 16 || v == 32 || v == 64) ? v : 32;
}

// Which dense form a solo launch at feature dim d takes, and the generic
// form's dynamic LDS: w_lds[d] + one slab per sub-wave. launch_dense and
// query_dense_launch both go through these two.
static inline bool dense_pipe_ok(int d) {
  const char* np = std::getenv("ASYNCAMD_NO_PIPE");  // re-read: sweeps
  return (d % 4 == 0) && (d <= 2048) && !(np && np[0] == '1');
}
static inline size_t dense_generic_lds_bytes(int d, int lpr) {
  return (size_t)(1 + WAVES_PER_BLOCK * (WAVE / lpr)) * d * sizeof(float);
}

// The one dense launch: the four extern "C" entry points below differ only
// in which arguments they leave null.
static void launch_dense(const void* X, const float* y, const float* w,
                         float* g_out, float* g_part, int* n_out,
                         float* alpha, int* idx_out, float* e_out,
                         int* pos_ctr, const int* k_dev, int commit_now,
                         long n_rows, int d, uint64_t seed, uint32_t round_k,
                         uint64_t row_start, double rate, int objective,
                         int x_is_bf16, int saga, hipStream_t stream,
                         unsigned long long* done_flag,
                         unsigned long long done_val,
                         unsigned long long* done_arr) {
  const uint32_t thr = philox_threshold(rate);
  const int take_all = rate >= 1.0;
  const int grid = grad_grid(n_rows);
  const bool pipe_ok = dense_pipe_ok(d);
  with_xt_saga_obj(x_is_bf16, saga, objective, [&](auto xt, auto sg,
                                                   auto hg) {
    using XT = decltype(xt);
    constexpr bool SG = decltype(sg)::value;
    constexpr bool HG = decltype(hg)::value;
    if (pipe_ok) {
      const int iters = pipe_iters(d);
      with_pipe_shape(iters, pipe_depth(iters, false), [&](auto IT, auto DP) {
        constexpr int it = decltype(IT)::value, dp = decltype(DP)::value;
        hipLaunchKernelGGL((grad_dense_pipe_kernel<XT, SG, 256, dp, it, HG>),
                           dim3(grid), dim3(256),
                           (PipeShape<XT, SG, dp, it>::LDS), stream,
                           (const XT*)X, y, w, g_out, g_part, n_out, alpha,
                           idx_out, e_out, pos_ctr, k_dev, commit_now,
                           n_rows, d, seed, round_k, row_start, thr,
                           take_all, objective, done_flag, done_val,
                           done_arr);
      });
      return;
    }
    const int lpr = pick_lpr(d);
    const size_t smem = dense_generic_lds_bytes(d, lpr);
    with_const<16, 32, 64>(lpr, [&](auto L) {
      hipLaunchKernelGGL((grad_dense_kernel<XT, SG, decltype(L)::value, HG>),
                         dim3(grid), dim3(BLOCK), smem, stream, (const XT*)X,
                         y, w, g_out, g_part, n_out, alpha, idx_out, e_out,
                         pos_ctr, k_dev, commit_now, n_rows, d, seed, round_k,
                         row_start, thr, take_all, objective, done_flag,
                         done_val, done_arr);
    });
  });
}

// The one CSR launch, as launch_dense.
static void launch_csr(const int* indptr, const int* indices,
                       const void* values, const float* y, const float* w,
                       float* alpha, float* g_out, int* n_out, int* idx_out,
                       float* e_out, int* pos_ctr, const int* k_dev,
                       int commit_now, long n_rows, uint64_t seed,
                       uint32_t round_k, uint64_t row_start, double rate,
                       int objective, int v_is_bf16, int saga,
                       hipStream_t stream, unsigned long long* done_flag,
                       unsigned long long done_val,
                       unsigned long long* done_arr) {
  const uint32_t thr = philox_threshold(rate);
  const int take_all = rate >= 1.0;
  const int grid = grad_grid(n_rows);
  with_xt_saga_obj(v_is_bf16, saga, objective, [&](auto vt, auto sg,
                                                   auto hg) {
    using VT = decltype(vt);
    constexpr bool HG = decltype(hg)::value;
    with_const<8, 32, 64, 16>(csr_lpr(), [&](auto L) {
      hipLaunchKernelGGL(
          (grad_csr_kernel<VT, decltype(sg)::value, decltype(L)::value, HG>),
          dim3(grid), dim3(BLOCK), 0, stream, indptr, indices,
          (const VT*)values, y, w, g_out, n_out, alpha, idx_out, e_out,
          pos_ctr, k_dev, commit_now, n_rows, seed, round_k, row_start, thr,
          take_all, objective, done_flag, done_val, done_arr);
    });
  });
}

extern "C" {

int query_grad_grid(long n_rows) { return grad_grid(n_rows); }

void launch_scan_rows(const float* y, int* rowlist, float* ylist,
                      int* count_dev, const int* scan_round_dev, long n_rows,
                      uint64_t seed, uint32_t round_k, uint64_t row_start,
                      double rate, hipStream_t stream) {
  const uint32_t thr = philox_threshold(rate);
  const int take_all = rate >= 1.0;
  const int grid = grad_grid(n_rows);
  hipLaunchKernelGGL(scan_rows_kernel, dim3(grid), dim3(BLOCK), 0, stream, y,
                     rowlist, ylist, count_dev, scan_round_dev, n_rows, seed,
                     round_k, row_start, thr, take_all);
}

void launch_bump_counter(int* p, hipStream_t stream) {
  hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, stream, p);
}

void launch_grad_dense_list(const void* X, const float* w, float* g_part,
                            const int* rowlist, const float* ylist,
                            const int* count_dev, long n_rows, int d,
                            int objective, int x_is_bf16,
                            hipStream_t stream) {
  const int grid = grad_grid(n_rows);
  const int iters = pipe_iters(d);
  with_xt_saga_obj(x_is_bf16, 0, objective, [&](auto xt, auto, auto hg) {
    using XT = decltype(xt);
    constexpr bool HG = decltype(hg)::value;
    with_pipe_shape(iters, pipe_depth(iters, false), [&](auto IT, auto DP) {
      constexpr int it = decltype(IT)::value, dp = decltype(DP)::value;
      hipLaunchKernelGGL((grad_dense_list_kernel<XT, 256, dp, it, HG>),
                         dim3(grid), dim3(256), list_lds_bytes(it), stream,
                         (const XT*)X, w, g_part, rowlist, ylist, count_dev,
                         n_rows, d, objective);
    });
  });
}

// the flag-less entry points are null-flag wrappers
void launch_grad_dense_flag(
    const void* X, const float* y, const float* w, float* g_out,
    float* g_part, int* n_out, const int* k_dev, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, double rate,
    int objective, int x_is_bf16, hipStream_t stream,
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr) {
  launch_dense(X, y, w, g_out, g_part, n_out, nullptr, nullptr, nullptr,
               nullptr, k_dev, 0, n_rows, d, seed, round_k, row_start, rate,
               objective, x_is_bf16, 0, stream, done_flag, done_val,
               done_arr);
}

void launch_saga_grad_dense_flag(
    const void* X, const float* y, const float* w, float* alpha,
    float* g_out, float* g_part, int* n_out, int* idx_out, float* e_out,
    int* pos_ctr, const int* k_dev, int commit_now, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, double rate,
    int objective, int x_is_bf16, hipStream_t stream,
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr) {
  launch_dense(X, y, w, g_out, g_part, n_out, alpha, idx_out, e_out, pos_ctr,
               k_dev, commit_now, n_rows, d, seed, round_k, row_start, rate,
               objective, x_is_bf16, 1, stream, done_flag, done_val,
               done_arr);
}

void launch_grad_dense(const void* X, const float* y, const float* w,
                       float* g_out, float* g_part, int* n_out,
                       const int* k_dev, long n_rows, int d, uint64_t seed,
                       uint32_t round_k, uint64_t row_start, double rate,
                       int objective, int x_is_bf16, hipStream_t stream) {
  launch_grad_dense_flag(X, y, w, g_out, g_part, n_out, k_dev, n_rows, d,
                         seed, round_k, row_start, rate, objective,
                         x_is_bf16, stream, nullptr, 0, nullptr);
}

void launch_saga_grad_dense(const void* X, const float* y, const float* w,
                            float* alpha, float* g_out, float* g_part,
                            int* n_out, int* idx_out, float* e_out,
                            int* pos_ctr, const int* k_dev, int commit_now,
                            long n_rows, int d, uint64_t seed,
                            uint32_t round_k, uint64_t row_start, double rate,
                            int objective, int x_is_bf16,
                            hipStream_t stream) {
  launch_saga_grad_dense_flag(X, y, w, alpha, g_out, g_part, n_out, idx_out,
                              e_out, pos_ctr, k_dev, commit_now, n_rows, d,
                              seed, round_k, row_start, rate, objective,
                              x_is_bf16, stream, nullptr, 0, nullptr);
}

void launch_grad_dense_wave(const void* slots_dev, const void* cmd_host,
                            long max_rows, int d, uint64_t seed, double rate,
                            int objective, int x_is_bf16, int saga,
                            hipStream_t stream) {
  const GradWaveCmd* cmd = (const GradWaveCmd*)cmd_host;
  const uint32_t thr = philox_threshold(rate);
  const int take_all = rate >= 1.0;
  const int grid = cmd->n * cmd->bper;
  const int iters = pipe_iters(d);
  (void)max_rows;
  with_xt_saga_obj(x_is_bf16, saga, objective, [&](auto xt, auto sg,
                                                   auto hg) {
    using XT = decltype(xt);
    constexpr bool SG = decltype(sg)::value;
    constexpr bool HG = decltype(hg)::value;
    with_pipe_shape(iters, pipe_depth(iters, true), [&](auto IT, auto DP) {
      constexpr int it = decltype(IT)::value, dp = decltype(DP)::value;
      hipLaunchKernelGGL((grad_dense_wave_kernel<XT, SG, 256, dp, it, HG>),
                         dim3(grid), dim3(256),
                         (PipeShape<XT, SG, dp, it>::LDS), stream,
                         (const GradWaveSlot*)slots_dev, *cmd, d, seed, thr,
                         take_all, objective);
    });
  });
}

// What a dense gradient launch at feature dim d will run: fills
// out = {iters, depth, occupancy hint, numRegs, localSizeBytes (scratch),
// dynamic LDS bytes, max active 256-thread blocks per CU with that LDS, 0}.
// wave = 1 describes grad_dense_wave_kernel, 0 the solo
// grad_dense_pipe_kernel (the lsq / logistic instantiation, HINGE = false).
// Returns 0, a hipError_t, or -1 when d is not served by the pipelined
// kernels.
int query_dense_kernel(int d, int x_is_bf16, int saga, int wave, int* out) {
  if (d <= 0 || d % 4 != 0 || d > 2048) return -1;
  const int iters = pipe_iters(d);
  int rc = 0;
  with_xt_saga(x_is_bf16, saga, [&](auto xt, auto sg) {
    using XT = decltype(xt);
    constexpr bool SG = decltype(sg)::value;
    with_pipe_shape(iters, pipe_depth(iters, wave != 0),
                    [&](auto IT, auto DP) {
      constexpr int it = decltype(IT)::value, dp = decltype(DP)::value;
      using Shape = PipeShape<XT, SG, dp, it>;
      const void* fn =
          wave ? (const void*)
                     grad_dense_wave_kernel<XT, SG, 256, dp, it, false>
               : (const void*)
                     grad_dense_pipe_kernel<XT, SG, 256, dp, it, false>;
      hipFuncAttributes attr;
      hipError_t e = hipFuncGetAttributes(&attr, fn);
      int nb = 0;
      if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256,
                                                         Shape::LDS);
      if (e != hipSuccess) { rc = (int)e; return; }
      out[0] = it; out[1] = dp; out[2] = Shape::HINT;
      out[3] = attr.numRegs; out[4] = (int)attr.localSizeBytes;
      out[5] = (int)Shape::LDS; out[6] = nb; out[7] = 0;
    });
  });
  return rc;
}

// Which form a solo dense launch (launch_dense) at feature dim d takes right
// now, overrides included: out = {1 pipelined / 0 generic, lanes per row
// (the pipelined form's rows are whole waves: 64), the generic form's
// dynamic LDS bytes (0 for the pipelined form: query_dense_kernel has it)}.
// Host only: no runtime call.
void query_dense_launch(int d, long long* out) {
  const bool pipe = dense_pipe_ok(d);
  const int lpr = pipe ? WAVE : pick_lpr(d);
  out[0] = pipe ? 1 : 0;
  out[1] = lpr;
  out[2] = pipe ? 0 : (long long)dense_generic_lds_bytes(d, lpr);
}

// The lanes per row a CSR launch (solo or wave) takes right now.
int query_csr_lpr() { return csr_lpr(); }

void launch_scan_rows_wave(const void* slots_dev, const void* cmd_host,
                           uint64_t seed, double rate, hipStream_t stream) {
  const GradWaveCmd* cmd = (const GradWaveCmd*)cmd_host;
  const uint32_t thr = philox_threshold(rate);
  const int take_all = rate >= 1.0;
  hipLaunchKernelGGL(scan_rows_wave_kernel, dim3(cmd->n * cmd->bper),
                     dim3(BLOCK), 0, stream,
                     (const GradWaveSlot*)slots_dev, *cmd, seed, thr,
                     take_all);
}

void launch_alpha_gather_wave(const void* slots_dev, const void* cmd_host,
                              hipStream_t stream) {
  const GradWaveCmd* cmd = (const GradWaveCmd*)cmd_host;
  hipLaunchKernelGGL(alpha_gather_wave_kernel, dim3(cmd->n * cmd->bper),
                     dim3(BLOCK), 0, stream,
                     (const GradWaveSlot*)slots_dev, *cmd);
}

void launch_grad_csr_flag(
    const int* indptr, const int* indices, const void* values,
    const float* y, const float* w, float* g_out, int* n_out,
    const int* k_dev, long n_rows, uint64_t seed, uint32_t round_k,
    uint64_t row_start, double rate, int objective, int v_is_bf16,
    hipStream_t stream, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr) {
  launch_csr(indptr, indices, values, y, w, nullptr, g_out, n_out, nullptr,
             nullptr, nullptr, k_dev, 0, n_rows, seed, round_k, row_start,
             rate, objective, v_is_bf16, 0, stream, done_flag, done_val,
             done_arr);
}

void launch_saga_grad_csr_flag(
    const int* indptr, const int* indices, const void* values,
    const float* y, const float* w, float* alpha, float* g_out, int* n_out,
    int* idx_out, float* e_out, int* pos_ctr, const int* k_dev,
    int commit_now, long n_rows, uint64_t seed, uint32_t round_k,
    uint64_t row_start, double rate, int objective, int v_is_bf16,
    hipStream_t stream, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr) {
  launch_csr(indptr, indices, values, y, w, alpha, g_out, n_out, idx_out,
             e_out, pos_ctr, k_dev, commit_now, n_rows, seed, round_k,
             row_start, rate, objective, v_is_bf16, 1, stream, done_flag,
             done_val, done_arr);
}

void launch_grad_csr(const int* indptr, const int* indices,
                     const void* values, const float* y, const float* w,
                     float* g_out, int* n_out, const int* k_dev, long n_rows,
                     uint64_t seed, uint32_t round_k, uint64_t row_start,
                     double rate, int objective, int v_is_bf16,
                     hipStream_t stream) {
  launch_grad_csr_flag(indptr, indices, values, y, w, g_out, n_out, k_dev,
                       n_rows, seed, round_k, row_start, rate, objective,
                       v_is_bf16, stream, nullptr, 0, nullptr);
}

void launch_saga_grad_csr(const int* indptr, const int* indices,
                          const void* values, const float* y, const float* w,
                          float* alpha, float* g_out, int* n_out,
                          int* idx_out, float* e_out, int* pos_ctr,
                          const int* k_dev, int commit_now, long n_rows,
                          uint64_t seed, uint32_t round_k, uint64_t row_start,
                          double rate, int objective, int v_is_bf16,
                          hipStream_t stream) {
  launch_saga_grad_csr_flag(indptr, indices, values, y, w, alpha, g_out,
                            n_out, idx_out, e_out, pos_ctr, k_dev,
                            commit_now, n_rows, seed, round_k, row_start,
                            rate, objective, v_is_bf16, stream, nullptr, 0,
                            nullptr);
}

void launch_reduce_partials(const float* g_part, float* g_out, int d, int G,
                            int splits, hipStream_t stream) {
  const int njc = (d + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(njc * splits), dim3(BLOCK),
                     0, stream, g_part, g_out, d, G, splits);
}

void launch_grad_csr_wave(const void* slots_dev, const void* cmd_host,
                          uint64_t seed, double rate, int objective,
                          int v_is_bf16, int saga, hipStream_t stream) {
  const GradWaveCmd* cmd = (const GradWaveCmd*)cmd_host;
  const uint32_t thr = philox_threshold(rate);
  const int take_all = rate >= 1.0;
  const int grid = cmd->n * cmd->bper;
  with_xt_saga_obj(v_is_bf16, saga, objective, [&](auto vt, auto sg,
                                                   auto hg) {
    constexpr bool HG = decltype(hg)::value;
    with_const<8, 32, 64, 16>(csr_lpr(), [&](auto L) {
      hipLaunchKernelGGL((grad_csr_wave_kernel<decltype(vt),
                                               decltype(sg)::value,
                                               decltype(L)::value, HG>),
                         dim3(grid), dim3(BLOCK), 0, stream,
                         (const CsrWaveSlot*)slots_dev, *cmd, seed, thr,
                         take_all, objective);
    });
  });
}

void launch_saga_commit_wave(const void* slots_dev, const void* cmd_host,
                             hipStream_t stream) {
  const CsrCommitCmd* cmd = (const CsrCommitCmd*)cmd_host;
  const int grid = cmd->n * cmd->bper;
  hipLaunchKernelGGL(saga_commit_wave_kernel, dim3(grid), dim3(BLOCK), 0,
                     stream, (const CommitSlot*)slots_dev, *cmd);
}

// l2 == l1 == 0 dispatches to the REG=false instantiation (the unchanged
// body): the unregularised bits never depend on x*1.0 or x-0.0.
void launch_sgd_update(float* w, const float* g, float gamma_k,
                       float inv_batch, int d, float l2, float l1,
                       hipStream_t stream) {
  const int grid = (d + 255) / 256;
  with_bool(l2 != 0.f || l1 != 0.f, [&](auto R) {
    hipLaunchKernelGGL(sgd_update_kernel<decltype(R)::value>, dim3(grid),
                       dim3(256), 0, stream, w, g, gamma_k, inv_batch, d, l2,
                       l1);
  });
}

void launch_saga_update(float* w, const float* g, float* alpha_bar,
                        float gamma, float inv_batch, float inv_N, int d,
                        float l2, float l1, hipStream_t stream) {
  const int grid = (d + 255) / 256;
  with_bool(l2 != 0.f || l1 != 0.f, [&](auto R) {
    hipLaunchKernelGGL(saga_update_kernel<decltype(R)::value>, dim3(grid),
                       dim3(256), 0, stream, w, g, alpha_bar, gamma,
                       inv_batch, inv_N, d, l2, l1);
  });
}

void launch_saga_commit(float* alpha, const int* idx, const float* e, int n,
                        hipStream_t stream) {
  if (n <= 0) return;
  const int grid = (n + 255) / 256;
  hipLaunchKernelGGL(saga_commit_kernel, dim3(grid), dim3(256), 0, stream,
                     alpha, idx, e, n);
}

void launch_sgd_reduce_update(const float* g_part, float* w, int* k_dev,
                              int* ticket, float gamma, float inv_batch,
                              int num_part, int d, int G, int splits,
                              hipStream_t stream) {
  const int njc = (d + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(sgd_reduce_update_kernel, dim3(njc * splits),
                     dim3(BLOCK), 0, stream, g_part, w, k_dev, ticket, gamma,
                     inv_batch, num_part, d, G, splits);
}

void launch_sgd_update_fused(float* w, float* g, int* k_dev, float gamma,
                             float inv_batch, int num_part, int d,
                             hipStream_t stream) {
  hipLaunchKernelGGL(sgd_update_fused_kernel, dim3(1), dim3(1024), 0, stream,
                     w, g, k_dev, gamma, inv_batch, num_part, d);
}

void launch_saga_update_fused(float* w, float* g, float* alpha_bar,
                              int* k_dev, float gamma, float inv_batch,
                              float inv_N, int d, hipStream_t stream) {
  hipLaunchKernelGGL(saga_update_fused_kernel, dim3(1), dim3(1024), 0,
                     stream, w, g, alpha_bar, k_dev, gamma, inv_batch, inv_N,
                     d);
}

// ``vec4`` selects the float4 form (caller guarantees d % 4 == 0 and
// 16-byte-aligned w / alpha_bar / g / wbuf buffers).
void launch_multi_update(float* w, float* const* g_tab,
                         float* const* wbuf_tab, float* alpha_bar,
                         float gamma, float inv_batch, float inv_N, int d,
                         const MultiUpdateArgs* a, int vec4, float l2,
                         float l1, hipStream_t stream) {
  const int nel = vec4 ? d / 4 : d;
  int grid = (nel + MU_BLOCK - 1) / MU_BLOCK;
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  with_bool(vec4 != 0, [&](auto V) {
    with_bool(l2 != 0.f || l1 != 0.f, [&](auto R) {
      hipLaunchKernelGGL(
          (multi_update_kernel<decltype(V)::value, decltype(R)::value>),
          dim3(grid), dim3(MU_BLOCK), 0, stream, w, g_tab, wbuf_tab,
          alpha_bar, gamma, inv_batch, inv_N, d, l2, l1, *a);
    });
  });
}

// One barrier round of the native engine's synchronous mode. The work is
// d*P floats (<= ~12 MB at rcv1's d=47,236, P=64; a few KB at the dense
// shapes), latency-bound: 64-thread blocks spread even d=784 (196 float4
// lanes) over 4 CUs, and d=47,236 gives 185 blocks — under one per CU —
// so the grid-stride loop only engages past d = 262,144. ``vec4`` selects
// the float4 form (caller guarantees d % 4 == 0 and 16-byte-aligned
// buffers).
void launch_sync_round_update(float* w, float* const* g_tab,
                              int* const* ctr_tab, float* alpha_bar,
                              float* snap_dst, int* ticket, int P, int d,
                              int mode, float scale, float gamma,
                              float inv_batch, float inv_N, int vec4,
                              float eta, float l2, float l1,
                              hipStream_t stream) {
  const int n = vec4 ? d / 4 : d;
  int grid = (n + SRU_BLOCK - 1) / SRU_BLOCK;
  if (grid > 1024) grid = 1024;
  if (grid < 1) grid = 1;
  with_bool(vec4 != 0, [&](auto V) {
    with_bool(l2 != 0.f || l1 != 0.f, [&](auto R) {
      hipLaunchKernelGGL(
          (sync_round_update_kernel<decltype(V)::value, decltype(R)::value>),
          dim3(grid), dim3(SRU_BLOCK), 0, stream, w, g_tab, ctr_tab,
          alpha_bar, snap_dst, ticket, P, d, mode, scale, gamma, inv_batch,
          inv_N, eta, l2, l1);
    });
  });
}

// Compiled resource use of one update-kernel instantiation: sync = 0
// multi_update_kernel<vec4, reg>, 1 sync_round_update_kernel<vec4, reg>.
// out = {numRegs, localSizeBytes (scratch), sharedSizeBytes (static LDS)}.
// Returns 0 or a hipError_t.
int query_update_kernel(int sync, int vec4, int reg, int* out) {
  const void* mu[4] = {(const void*)multi_update_kernel<false, false>,
                       (const void*)multi_update_kernel<false, true>,
                       (const void*)multi_update_kernel<true, false>,
                       (const void*)multi_update_kernel<true, true>};
  const void* sru[4] = {(const void*)sync_round_update_kernel<false, false>,
                        (const void*)sync_round_update_kernel<false, true>,
                        (const void*)sync_round_update_kernel<true, false>,
                        (const void*)sync_round_update_kernel<true, true>};
  const int k = (vec4 ? 2 : 0) + (reg ? 1 : 0);
  hipFuncAttributes attr;
  const hipError_t e = hipFuncGetAttributes(&attr, sync ? sru[k] : mu[k]);
  if (e != hipSuccess) return (int)e;
  out[0] = attr.numRegs;
  out[1] = (int)attr.localSizeBytes;
  out[2] = (int)attr.sharedSizeBytes;
  return 0;
}

void launch_saga_commit_devn(float* alpha, const int* idx, const float* e,
                             const int* n_dev, int cap, hipStream_t stream) {
  const int grid = (cap + 255) / 256;
  hipLaunchKernelGGL(saga_commit_devn_kernel, dim3(grid > 0 ? grid : 1),
                     dim3(256), 0, stream, alpha, idx, e, n_dev);
}

void launch_alpha_gather(float* a_dst, const float* a_src, const int* rows,
                         const int* count_dev, int cap, hipStream_t stream) {
  const int grid = (cap + 255) / 256;
  hipLaunchKernelGGL(alpha_gather_kernel, dim3(grid > 0 ? grid : 1),
                     dim3(256), 0, stream, a_dst, a_src, rows, count_dev);
}

}  // extern "C"

// ---------------------------------------------------------------- K9
// Fused held-out evaluation kernels and their launchers: built on the row
// machinery (RowVec, row_rsrc, cvt4, to_f32) and the with_const helper above.
#include "eval.h"

// ---------------------------------------------------------------- K10
// Threshold sweep of the evaluation (ROC / PR points in one pass): the K9
// scoring walks with an LDS histogram per iterate.
#include "eval_curve.h"

// ---------------------------------------------------------------- K11
// Column statistics (MLlib colStats) and in-place feature standardisation:
// streaming passes built on to_f32, with_const / with_bool and eval.h's
// with_xt.
#include "col_stats.h"
