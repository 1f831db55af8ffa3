// Fused held-out evaluation (K9): score a tile of EVAL_TT stacked iterates
// against every row and reduce on the fly to five numbers per iterate —
// loss_sum (fp64) and the confusion counts tp / fp / tn / fn (int64).
// Nothing of size rows x T ever reaches global memory; more than EVAL_TT
// iterates are more passes over the data.
//
// Included by kernels.hip after its row machinery (RowVec, row_rsrc, cvt4,
// to_f32) and its launcher helpers (with_const, with_bool): this file adds
// no loader of its own.
//
// Scoring rule: a row is actually positive iff y > 0.5 and predicted
// positive iff z > z_thr (z_thr is fp64: the fp32 score is widened, which
// is exact, so the decision is the one a real-number comparison of the
// computed z makes). The row loss is computed in fp32 from the fp32 z:
//   0 lsq      (z - y)^2
//   1 logistic softplus(-s z) = max(-sz, 0) + log1pf(expf(-|sz|)), libm forms
//   2 hinge    max(0, 1 - s z)                       with s = 2y - 1
//
// Determinism: no floating-point atomics anywhere. A lane owns one
// (row slot, iterate) pair and adds that pair's row losses to an fp64
// register and its decisions to integer registers; the block's owners
// combine through LDS in a fixed order; each block writes its partials with
// plain stores and eval_finish_kernel sums the blocks in index order. The
// grid and the row-to-wave mapping depend on the data shape only, and an
// iterate's dot product is the same instruction sequence in every tile slot,
// so evaluate(W)[t] == evaluate(W[t:t+1])[0] bit for bit.
#pragma once

#define EVAL_TT 8      // iterates per pass (docs/KERNELS.md, Evaluation)
#define EVAL_R 2       // rows a wave scores together (dense pipelined form)
#define EVAL_BLOCK 256
#define EVAL_NW (EVAL_BLOCK / WAVE)
#define EVAL_MAX_GRID 512

constexpr int eval_log2(int v) { return v <= 1 ? 0 : 1 + eval_log2(v >> 1); }

// Sum NV per-lane values over each aligned group of WIDTH lanes with a
// transposing butterfly: the first log2(NV) exchange steps each halve the
// number of live values (a lane keeps the half selected by its own bit and
// sends the other), the remaining steps are the plain xor tree on the one
// value left. NV + log2(WIDTH / NV) - 1 shuffles instead of
// NV * log2(WIDTH). Every value is summed over the same lanes in the same
// order, whatever its index. Afterwards v[0] holds the complete sum of the
// value whose index is eval_owner_key(lane): bit s of the index is bit
// (log2(WIDTH) - 1 - s) of the lane.
template <int NV, int WIDTH>
__device__ __forceinline__ float reduce_transpose(float (&v)[NV], int lane) {
  constexpr int LN = eval_log2(NV), LW = eval_log2(WIDTH);
  static_assert((1 << LN) == NV && (1 << LW) == WIDTH && NV <= WIDTH,
                "powers of two, NV <= WIDTH");
#pragma unroll
  for (int s = 0; s < LN; ++s) {
    const int off = WIDTH >> (s + 1);
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < (NV >> (s + 1)); ++i) {
      const float keep = hi ? v[2 * i + 1] : v[2 * i];
      const float send = hi ? v[2 * i] : v[2 * i + 1];
      v[i] = keep + __shfl_xor(send, off, WAVE);
    }
  }
#pragma unroll
  for (int off = WIDTH >> (LN + 1); off > 0; off >>= 1)
    v[0] += __shfl_xor(v[0], off, WAVE);
  return v[0];
}
template <int NV, int WIDTH>
__device__ __forceinline__ int eval_owner_key(int lane) {
  constexpr int LN = eval_log2(NV), LW = eval_log2(WIDTH);
  int k = 0;
#pragma unroll
  for (int s = 0; s < LN; ++s) k |= ((lane >> (LW - 1 - s)) & 1) << s;
  return k;
}

// One lane's running totals for its (row slot, iterate) pair.
struct EvalAcc {
  double loss = 0.0;
  unsigned int tp = 0, fp = 0, tn = 0, fn = 0;
  __device__ __forceinline__ void add(float z, float yv, int objective,
                                      double z_thr, bool valid) {
    float l;
    if (objective == 0) {
      const float r = z - yv;
      l = r * r;
    } else {
      const float sz = (2.0f * yv - 1.0f) * z;
      if (objective == 1) l = fmaxf(-sz, 0.0f) + log1pf(expf(-fabsf(sz)));
      else l = fmaxf(0.0f, 1.0f - sz);
    }
    const bool pos = yv > 0.5f;
    const bool pred = (double)z > z_thr;
    if (valid) {
      loss += (double)l;
      tp += pos && pred;
      fp += !pos && pred;
      tn += !pos && !pred;
      fn += pos && !pred;
    }
  }
};

// Block combine + partials store. Each wave has NOWN owners per iterate
// (slot-major: owner index o * EVAL_TT + t), parked by their owning lanes in
// `scratch` (LDS, eval_flush_bytes(NOWN) bytes, 8-byte aligned); thread
// t < EVAL_TT then sums wave 0..NW-1, owner 0..NOWN-1 in that order and
// writes part_loss[b][t] and part_cnt[b][4][t] with plain stores.
constexpr size_t eval_flush_bytes(int nown) {
  return (size_t)EVAL_NW * nown * EVAL_TT * (sizeof(double) + 4 * sizeof(int));
}
template <int NOWN>
__device__ __forceinline__ void eval_block_flush(
    const EvalAcc& acc, bool is_owner, int own_idx, int wave, void* scratch,
    double* __restrict__ part_loss, long long* __restrict__ part_cnt) {
  constexpr int PER_WAVE = NOWN * EVAL_TT;
  double* s_loss = (double*)scratch;                            // [NW][PER_WAVE]
  unsigned int* s_cnt = (unsigned int*)(s_loss + EVAL_NW * PER_WAVE);  // [..][4]
  if (is_owner) {
    const int i = wave * PER_WAVE + own_idx;
    s_loss[i] = acc.loss;
    s_cnt[4 * i + 0] = acc.tp;
    s_cnt[4 * i + 1] = acc.fp;
    s_cnt[4 * i + 2] = acc.tn;
    s_cnt[4 * i + 3] = acc.fn;
  }
  __syncthreads();
  if (threadIdx.x < EVAL_TT) {
    const int t = threadIdx.x;
    double ls = 0.0;
    long long c[4] = {0, 0, 0, 0};
    for (int w = 0; w < EVAL_NW; ++w)
      for (int o = 0; o < NOWN; ++o) {
        const int i = w * PER_WAVE + o * EVAL_TT + t;
        ls += s_loss[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] += s_cnt[4 * i + q];
      }
    part_loss[(size_t)blockIdx.x * EVAL_TT + t] = ls;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      part_cnt[((size_t)blockIdx.x * 4 + q) * EVAL_TT + t] = c[q];
  }
}

// ------------------------------------------------------------ dense, d<=2048
// A wave takes chunks of EVAL_R consecutive rows, grid-strided over all the
// waves of the launch. The W tile sits in LDS as [EVAL_TT][DPAD] fp32,
// zero-padded like w_lds; w is never rounded to X's type. Rows come through
// row_rsrc descriptors (nothing past a row or past X is fetched) with 64-bit
// row offsets. Two chunks are in flight per wave: while chunk c is scored,
// chunk c + stride's 2 * ITERS loads are already issued (tail slots load a
// clamped chunk instead of skipping, as pipe_drain does). Each row fragment
// is read from HBM once per tile and each W fragment from LDS once per
// EVAL_R rows.
//
// The scoring walks (eval_dense_rows, eval_generic_rows, eval_csr_rows) are
// shared with the threshold-sweep kernels of eval_curve.h: a walk hands
// every lane the finished score of its (row slot, iterate) pair as
// score(z, y, valid), and the kernel around it decides what to count.
template <typename XT, int ITERS, typename F>
__device__ __forceinline__ void eval_dense_rows(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ Wt, long n_rows, int d,
    float* __restrict__ w_lds, F&& score) {
  using RV = RowVec<XT>;
  constexpr int DPAD = ITERS * 256;
  constexpr int NV = EVAL_R * EVAL_TT;
  for (int i = threadIdx.x; i < EVAL_TT * DPAD; i += EVAL_BLOCK) {
    const int t = i / DPAD, j = i - t * DPAD;
    w_lds[i] = j < d ? Wt[(size_t)t * d + j] : 0.f;
  }
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long total_elems = n_rows * (long)d;
  const long n_chunks = (n_rows + EVAL_R - 1) / EVAL_R;
  const long stride = (long)gridDim.x * EVAL_NW;
  // this lane's (row slot, iterate) pair after reduce_transpose
  const int key = eval_owner_key<NV, WAVE>(lane);
  const int my_r = key / EVAL_TT;

  typename RV::T bufA[EVAL_R][ITERS], bufB[EVAL_R][ITERS];
  float yA[EVAL_R], yB[EVAL_R];
  // y first: the row loads queue behind it, so its use waits for nothing
  // younger than itself
  auto issue = [&](typename RV::T (&buf)[EVAL_R][ITERS], float (&yy)[EVAL_R],
                   long c) {
#pragma unroll
    for (int r = 0; r < EVAL_R; ++r)
      yy[r] = y[min(c * EVAL_R + r, n_rows - 1)];
#pragma unroll
    for (int r = 0; r < EVAL_R; ++r) {
      const long row = min(c * EVAL_R + r, n_rows - 1);
      const auto rs = row_rsrc<XT>(X, total_elems, (int)row, d);
#pragma unroll
      for (int it = 0; it < ITERS; ++it)
        buf[r][it] = RV::load(rs, (lane + it * WAVE) << RV::VOFF_SHIFT);
    }
  };
  auto consume = [&](typename RV::T (&buf)[EVAL_R][ITERS],
                     float (&yy)[EVAL_R], long c) {
    float z[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) z[k] = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      float o[EVAL_R][4];
#pragma unroll
      for (int r = 0; r < EVAL_R; ++r) cvt4(buf[r][it], o[r]);
      const int j4 = lane + it * WAVE;
#pragma unroll
      for (int t = 0; t < EVAL_TT; ++t) {
        const float4 wv =
            reinterpret_cast<const float4*>(w_lds + (size_t)t * DPAD)[j4];
#pragma unroll
        for (int r = 0; r < EVAL_R; ++r)
          z[r * EVAL_TT + t] += o[r][0] * wv.x + o[r][1] * wv.y +
                                o[r][2] * wv.z + o[r][3] * wv.w;
      }
    }
    const float zz = reduce_transpose<NV, WAVE>(z, lane);
    float yv = yy[0];
#pragma unroll
    for (int r = 1; r < EVAL_R; ++r) yv = my_r == r ? yy[r] : yv;
    score(zz, yv, c * EVAL_R + my_r < n_rows);
  };

  long c = (long)blockIdx.x * EVAL_NW + wave;
  if (c < n_chunks) issue(bufA, yA, c);
  while (c < n_chunks) {
    issue(bufB, yB, min(c + stride, n_chunks - 1));
    __builtin_amdgcn_sched_barrier(0);
    consume(bufA, yA, c);
    c += stride;
    if (c >= n_chunks) break;
    __builtin_amdgcn_sched_barrier(0);
    issue(bufA, yA, min(c + stride, n_chunks - 1));
    __builtin_amdgcn_sched_barrier(0);
    consume(bufB, yB, c);
    c += stride;
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <typename XT, int ITERS>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_dense_kernel(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ Wt, double* __restrict__ part_loss,
    long long* __restrict__ part_cnt, long n_rows, int d, int objective,
    double z_thr) {
  constexpr int NV = EVAL_R * EVAL_TT;
  static_assert(eval_flush_bytes(EVAL_R) <= EVAL_TT * 256 * sizeof(float),
                "the flush reuses the tile's LDS");
  extern __shared__ double eval_smem[];  // the tile, [EVAL_TT][DPAD] fp32
  EvalAcc acc;
  eval_dense_rows<XT, ITERS>(X, y, Wt, n_rows, d, (float*)eval_smem,
                             [&](float z, float yv, bool valid) {
                               acc.add(z, yv, objective, z_thr, valid);
                             });
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  // owners: one lane per (slot, iterate); the others hold copies. The tile
  // is dead once every wave is past its last row: its LDS parks the owners
  __syncthreads();
  eval_block_flush<EVAL_R>(acc, (lane & (WAVE / NV - 1)) == 0,
                           eval_owner_key<NV, WAVE>(lane), wave, eval_smem,
                           part_loss, part_cnt);
}

// ------------------------------------------ dense fallback, any d (scalar)
// d > 2048 or d % 4 != 0, as grad_dense_kernel: rows are not 16-byte
// aligned and the tile may not fit LDS, so a wave walks one row at a time
// with element loads (64 consecutive elements per instruction) and reads
// the W tile through the cache.
template <typename XT, typename F>
__device__ __forceinline__ void eval_generic_rows(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ Wt, long n_rows, int d, F&& score) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * EVAL_NW;
  for (long row = (long)blockIdx.x * EVAL_NW + wave; row < n_rows;
       row += stride) {
    const XT* xrow = X + (size_t)row * d;
    float z[EVAL_TT];
#pragma unroll
    for (int t = 0; t < EVAL_TT; ++t) z[t] = 0.f;
    for (int j = lane; j < d; j += WAVE) {
      const float xv = to_f32<XT>(xrow[j]);
#pragma unroll
      for (int t = 0; t < EVAL_TT; ++t) z[t] += xv * Wt[(size_t)t * d + j];
    }
    const float zz = reduce_transpose<EVAL_TT, WAVE>(z, lane);
    score(zz, y[row], true);
  }
}

template <typename XT>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_dense_generic_kernel(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ Wt, double* __restrict__ part_loss,
    long long* __restrict__ part_cnt, long n_rows, int d, int objective,
    double z_thr) {
  EvalAcc acc;
  eval_generic_rows<XT>(X, y, Wt, n_rows, d,
                        [&](float z, float yv, bool valid) {
                          acc.add(z, yv, objective, z_thr, valid);
                        });
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  __shared__ double scratch[eval_flush_bytes(1) / sizeof(double)];
  eval_block_flush<1>(acc, (lane & (WAVE / EVAL_TT - 1)) == 0,
                      eval_owner_key<EVAL_TT, WAVE>(lane), wave, scratch,
                      part_loss, part_cnt);
}

// --------------------------------------------------------------------- CSR
// Sub-waves of LPR lanes per row, as grad_csr_body; rows grid-strided over
// all sub-waves. The W tile is stored TRANSPOSED, Wtt[d][EVAL_TT]: one
// indices[p] gather brings the EVAL_TT contiguous weights of that column
// (two 16-byte loads) for every iterate of the tile, and a bf16 value is
// widened in a register, never expanded in memory.
template <typename VT, int LPR, typename F>
__device__ __forceinline__ void eval_csr_rows(
    const int* __restrict__ indptr, const int* __restrict__ indices,
    const VT* __restrict__ values, const float* __restrict__ y,
    const float* __restrict__ Wtt, long n_rows, F&& score) {
  static_assert(LPR >= EVAL_TT && EVAL_TT == 8, "two float4 per column");
  constexpr int NSUB = WAVE / LPR;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR;
  const int sl = lane % LPR;
  const long stride = (long)gridDim.x * EVAL_NW * NSUB;
  // every sub-wave of a wave runs the same number of trips (the shuffles
  // want all 64 lanes): a sub-wave past the end scores nothing
  for (long base = ((long)blockIdx.x * EVAL_NW + wave) * NSUB; base < n_rows;
       base += stride) {
    const long row = base + sub;
    const bool valid = row < n_rows;
    int s = 0, e = 0;
    float yv = 0.f;
    if (valid) {
      s = indptr[row];
      e = indptr[row + 1];
      yv = y[row];
    }
    float z[EVAL_TT];
#pragma unroll
    for (int t = 0; t < EVAL_TT; ++t) z[t] = 0.f;
    for (int p = s + sl; p < e; p += LPR) {
      const float v = to_f32<VT>(values[p]);
      const float4* wc =
          reinterpret_cast<const float4*>(Wtt + (size_t)indices[p] * EVAL_TT);
      const float4 a = wc[0], b = wc[1];
      z[0] += v * a.x; z[1] += v * a.y; z[2] += v * a.z; z[3] += v * a.w;
      z[4] += v * b.x; z[5] += v * b.y; z[6] += v * b.z; z[7] += v * b.w;
    }
    const float zz = reduce_transpose<EVAL_TT, LPR>(z, sl);
    score(zz, yv, valid);
  }
}

template <typename VT, int LPR>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_csr_kernel(
    const int* __restrict__ indptr, const int* __restrict__ indices,
    const VT* __restrict__ values, const float* __restrict__ y,
    const float* __restrict__ Wtt, double* __restrict__ part_loss,
    long long* __restrict__ part_cnt, long n_rows, int objective,
    double z_thr) {
  constexpr int NSUB = WAVE / LPR;
  EvalAcc acc;
  eval_csr_rows<VT, LPR>(indptr, indices, values, y, Wtt, n_rows,
                         [&](float z, float yv, bool valid) {
                           acc.add(z, yv, objective, z_thr, valid);
                         });
  const int wave = threadIdx.x >> 6;
  const int sub = (threadIdx.x & 63) / LPR;
  const int sl = threadIdx.x % LPR;
  __shared__ double scratch[eval_flush_bytes(NSUB) / sizeof(double)];
  eval_block_flush<NSUB>(acc, (sl & (LPR / EVAL_TT - 1)) == 0,
                         sub * EVAL_TT + eval_owner_key<EVAL_TT, LPR>(sl),
                         wave, scratch, part_loss, part_cnt);
}

// Fixed-order sum over the blocks' partials: thread t adds block 0..G-1.
__global__ __launch_bounds__(WAVE) void eval_finish_kernel(
    const double* __restrict__ part_loss,
    const long long* __restrict__ part_cnt, int G,
    double* __restrict__ out_loss, long long* __restrict__ out_cnt,
    long cnt_stride) {
  const int t = threadIdx.x;
  if (t >= EVAL_TT) return;
  double ls = 0.0;
  long long c[4] = {0, 0, 0, 0};
  for (int b = 0; b < G; ++b) {
    ls += part_loss[(size_t)b * EVAL_TT + t];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      c[q] += part_cnt[((size_t)b * 4 + q) * EVAL_TT + t];
  }
  out_loss[t] = ls;
#pragma unroll
  for (int q = 0; q < 4; ++q) out_cnt[(size_t)q * cnt_stride + t] = c[q];
}

// ---------------------------------------------------------------- launchers

static inline bool eval_pipe_ok(int d) { return d % 4 == 0 && d <= 2048; }

// Grids are functions of the data shape alone. Dense: four chunks of EVAL_R
// rows per wave before the grid stops growing; generic and CSR: sixteen rows
// per (sub-)wave.
static inline int eval_dense_grid(long n_rows, int d) {
  const long per_block = eval_pipe_ok(d) ? 4L * EVAL_R * EVAL_NW
                                         : 16L * EVAL_NW;
  long g = (n_rows + per_block - 1) / per_block;
  if (g > EVAL_MAX_GRID) g = EVAL_MAX_GRID;
  return g < 1 ? 1 : (int)g;
}
static inline int eval_csr_lpr() { return 32; }  // grad_csr's rcv1 optimum
static inline int eval_csr_grid(long n_rows) {
  const long per_block = 16L * EVAL_NW * (WAVE / eval_csr_lpr());
  long g = (n_rows + per_block - 1) / per_block;
  if (g > 2 * EVAL_MAX_GRID) g = 2 * EVAL_MAX_GRID;
  return g < 1 ? 1 : (int)g;
}
constexpr size_t eval_lds_bytes(int iters) {
  return (size_t)EVAL_TT * iters * 256 * sizeof(float);
}

template <typename F>
static void with_xt(int is_bf16, F&& f) {
  if (is_bf16) f(__hip_bfloat16{});
  else f(float{});
}

// Compiled resource use of instantiation `idx` (0..EVAL_N_KERNELS-1) of a
// kernel family: dense pipelined [xt][iters] first, then the two generic,
// then the CSR ones. FAM names the family's three kernel templates and the
// dynamic LDS its dense kernel takes on top of the W tile (EvalK9 here,
// EvalCurve in eval_curve.h). out = {numRegs, localSizeBytes (scratch),
// static + dynamic LDS bytes, max active blocks per CU, kind, xt, shape}.
#define EVAL_N_KERNELS (16 + 2 + 2)
template <typename FAM>
static int eval_query_kernel(int idx, int* out) {
  const void* fn = nullptr;
  size_t dyn = 0;
  int kind = 0, bf = 0, shape = 0;
  if (idx < 16) {
    bf = idx / 8;
    shape = idx % 8 + 1;
    dyn = eval_lds_bytes(shape) + FAM::extra_lds;
    with_xt(bf, [&](auto xt) {
      with_const<1, 2, 3, 4, 5, 6, 7, 8>(shape, [&](auto IT) {
        fn = FAM::template dense<decltype(xt), decltype(IT)::value>();
      });
    });
  } else if (idx < 18) {
    kind = 1;
    bf = idx - 16;
    with_xt(bf, [&](auto xt) {
      fn = FAM::template generic<decltype(xt)>();
    });
  } else if (idx < EVAL_N_KERNELS) {
    kind = 2;
    bf = idx - 18;
    shape = eval_csr_lpr();
    with_xt(bf, [&](auto vt) {
      with_const<16, 32>(shape, [&](auto L) {
        fn = FAM::template csr<decltype(vt), decltype(L)::value>();
      });
    });
  } else {
    return -1;
  }
  hipFuncAttributes attr;
  hipError_t e = hipFuncGetAttributes(&attr, fn);
  int nb = 0;
  if (e == hipSuccess)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, EVAL_BLOCK,
                                                     dyn);
  if (e != hipSuccess) return (int)e;
  out[0] = attr.numRegs;
  out[1] = (int)attr.localSizeBytes;
  out[2] = (int)(attr.sharedSizeBytes + dyn);
  out[3] = nb;
  out[4] = kind;
  out[5] = bf;
  out[6] = shape;
  return 0;
}
struct EvalK9 {
  static constexpr size_t extra_lds = 0;
  template <typename XT, int ITERS>
  static const void* dense() {
    return (const void*)eval_dense_kernel<XT, ITERS>;
  }
  template <typename XT>
  static const void* generic() {
    return (const void*)eval_dense_generic_kernel<XT>;
  }
  template <typename VT, int LPR>
  static const void* csr() {
    return (const void*)eval_csr_kernel<VT, LPR>;
  }
};

extern "C" {

int query_eval_tile() { return EVAL_TT; }
int query_eval_grid(long n_rows, int d, int csr) {
  return csr ? eval_csr_grid(n_rows) : eval_dense_grid(n_rows, d);
}

// W: n_tiles tiles of [EVAL_TT][d] fp32 (the caller zero-pads the last);
// part_loss [grid][EVAL_TT] fp64 and part_cnt [grid][4][EVAL_TT] int64 are
// scratch reused by every tile (stream order); out_loss [n_tiles*EVAL_TT],
// out_cnt [4][n_tiles*EVAL_TT].
void launch_eval_dense(const void* X, const float* y, const float* W,
                       int n_tiles, long n_rows, int d, int objective,
                       double z_thr, int x_is_bf16, double* part_loss,
                       long long* part_cnt, double* out_loss,
                       long long* out_cnt, hipStream_t stream) {
  const int grid = eval_dense_grid(n_rows, d);
  const long t_pad = (long)n_tiles * EVAL_TT;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const float* Wt = W + (size_t)tile * EVAL_TT * d;
    with_xt(x_is_bf16, [&](auto xt) {
      using XT = decltype(xt);
      if (eval_pipe_ok(d)) {
        with_const<1, 2, 3, 4, 5, 6, 7, 8>((d + 255) / 256, [&](auto IT) {
          constexpr int it = decltype(IT)::value;
          hipLaunchKernelGGL((eval_dense_kernel<XT, it>), dim3(grid),
                             dim3(EVAL_BLOCK), eval_lds_bytes(it), stream,
                             (const XT*)X, y, Wt, part_loss, part_cnt, n_rows,
                             d, objective, z_thr);
        });
      } else {
        hipLaunchKernelGGL(eval_dense_generic_kernel<XT>, dim3(grid),
                           dim3(EVAL_BLOCK), 0, stream, (const XT*)X, y, Wt,
                           part_loss, part_cnt, n_rows, d, objective, z_thr);
      }
    });
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(WAVE), 0, stream,
                       part_loss, part_cnt, grid,
                       out_loss + (size_t)tile * EVAL_TT,
                       out_cnt + (size_t)tile * EVAL_TT, t_pad);
  }
}

// Wtt: n_tiles tiles of [d][EVAL_TT] fp32 (transposed, zero-padded).
void launch_eval_csr(const int* indptr, const int* indices,
                     const void* values, const float* y, const float* Wtt,
                     int n_tiles, long n_rows, int d, int objective,
                     double z_thr, int v_is_bf16, double* part_loss,
                     long long* part_cnt, double* out_loss,
                     long long* out_cnt, hipStream_t stream) {
  const int grid = eval_csr_grid(n_rows);
  const long t_pad = (long)n_tiles * EVAL_TT;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const float* Wt = Wtt + (size_t)tile * EVAL_TT * d;
    with_xt(v_is_bf16, [&](auto vt) {
      using VT = decltype(vt);
      with_const<16, 32>(eval_csr_lpr(), [&](auto L) {
        hipLaunchKernelGGL((eval_csr_kernel<VT, decltype(L)::value>),
                           dim3(grid), dim3(EVAL_BLOCK), 0, stream, indptr,
                           indices, (const VT*)values, y, Wt, part_loss,
                           part_cnt, n_rows, objective, z_thr);
      });
    });
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(WAVE), 0, stream,
                       part_loss, part_cnt, grid,
                       out_loss + (size_t)tile * EVAL_TT,
                       out_cnt + (size_t)tile * EVAL_TT, t_pad);
  }
}

int query_eval_kernel(int idx, int* out) {
  return eval_query_kernel<EvalK9>(idx, out);
}
int query_eval_kernel_count() { return EVAL_N_KERNELS; }

}  // extern "C"
