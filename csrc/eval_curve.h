// Threshold sweep of the fused held-out evaluation (K10): the confusion
// counts of a tile of EVAL_TT stacked iterates at EVAL_KT score thresholds
// per iterate, from ONE pass over the rows — the points of a ROC / PR curve
// without a sort and without a rows x T score matrix. More than EVAL_KT
// thresholds are more passes, as more than EVAL_TT iterates are more tiles.
//
// Included by kernels.hip after eval.h. The kernels are the threshold-sweep
// twins of the K9 kernels and run K9's scoring walks (eval_dense_rows,
// eval_generic_rows, eval_csr_rows): same row loads, same dot products,
// same reduce_transpose, so a score here is the score evaluate() decides on.
//
// Rule: every iterate of the tile has its own row of thresholds,
// non-decreasing along k (the last pass is padded with +inf). The owner lane
// of a (row, iterate) pair computes b = #{k : (double)z > thr[t][k]} — the
// comparison of EvalAcc::add, found by binary search since the predicate is
// monotone in k — and, if b > 0, adds 1 to the LDS histogram
// hist[t][b - 1][y > 0.5]. A NaN score compares false everywhere: b = 0, the
// row is below every threshold. The positives and negatives per iterate are
// counted in registers as K9 counts. The finish kernel sums the blocks'
// histograms in index order and takes suffix sums over k:
//   tp[t][k] = #{positive rows with z > thr[t][k]} = sum_{j >= k} hist[t][j][1]
//   fp[t][k] likewise over the negatives; fn = n_pos - tp, tn = n_neg - fp.
//
// Determinism: integers only. LDS integer adds commute, each block writes
// its histogram and totals with plain stores, and the finish kernel adds the
// blocks in index order; the grids are K9's, functions of the data shape.
//
// LDS: thresholds (fp64) and histogram (2 x u32) take 16 bytes per
// (iterate, threshold): EVAL_KT = 128 makes that 16 KiB, so the ITERS = 8
// dense kernel holds 64 + 16 = 80 KiB and two blocks still share a CU's
// 160 KiB, as two K9 blocks do.
#pragma once

#define EVAL_KT 128  // thresholds per pass (docs/KERNELS.md, Curves)

constexpr size_t eval_curve_lds_bytes() {
  return (size_t)EVAL_TT * EVAL_KT * (sizeof(double) + 2 * sizeof(unsigned));
}
static_assert((EVAL_KT & (EVAL_KT - 1)) == 0, "the search halves EVAL_KT");
static_assert(eval_curve_lds_bytes() <= 16 * 1024 &&
                  2 * (eval_lds_bytes(8) + eval_curve_lds_bytes()) <=
                      160 * 1024,
              "two blocks of the widest dense kernel share a CU's LDS");

// The block's thresholds and histogram in LDS. thr is stored k-major,
// thr[k][t], so that the owners of one wave — different iterates, mostly
// nearby k — spread over the banks; hist is [t][k][2], the layout of the
// per-block partials.
struct CurveLds {
  double* thr;
  unsigned int* hist;
  __device__ __forceinline__ explicit CurveLds(void* base)
      : thr((double*)base),
        hist((unsigned int*)((double*)base + EVAL_TT * EVAL_KT)) {}
  // thr_g: this (tile, pass)'s thresholds, [EVAL_TT] rows of ld doubles.
  // The caller's next __syncthreads() publishes both arrays.
  __device__ __forceinline__ void init(const double* __restrict__ thr_g,
                                       long ld) const {
    for (int i = threadIdx.x; i < EVAL_TT * EVAL_KT; i += EVAL_BLOCK) {
      const int t = i / EVAL_KT, k = i - t * EVAL_KT;
      thr[k * EVAL_TT + t] = thr_g[(size_t)t * ld + k];
    }
    for (int i = threadIdx.x; i < EVAL_TT * EVAL_KT * 2; i += EVAL_BLOCK)
      hist[i] = 0u;
  }
};

// One lane's running totals for its (row slot, iterate) pair, and the
// histogram update for the rows it owns.
struct CurveAcc {
  unsigned int n_pos = 0, n_neg = 0;
  __device__ __forceinline__ void add(float z, float yv, const CurveLds& s,
                                      int t, bool counts) {
    const double zd = (double)z;
    // b = #{k : zd > thr[k]}: the largest b <= EVAL_KT - 1 with
    // zd > thr[b - 1], then the last threshold
    int b = 0;
#pragma unroll
    for (int step = EVAL_KT / 2; step >= 1; step >>= 1)
      b += zd > s.thr[(b + step - 1) * EVAL_TT + t] ? step : 0;
    b += zd > s.thr[b * EVAL_TT + t] ? 1 : 0;
    const bool pos = yv > 0.5f;
    if (counts) {
      n_pos += pos;
      n_neg += !pos;
      if (b > 0) atomicAdd(&s.hist[(t * EVAL_KT + b - 1) * 2 + pos], 1u);
    }
  }
};

// Block combine + partials store, as eval_block_flush: the owners park
// their totals in `scratch` (LDS, eval_curve_flush_bytes(NOWN) bytes, which
// may be the dead W tile but not CurveLds), thread t < EVAL_TT sums them in
// wave, owner order and writes part_tot[b][2][t] (positives, negatives);
// then the block's histogram goes out as it stands, part_hist[b][t][k][2].
// The caller has synchronised the block after its last row.
constexpr size_t eval_curve_flush_bytes(int nown) {
  return (size_t)EVAL_NW * nown * EVAL_TT * 2 * sizeof(unsigned int);
}
template <int NOWN>
__device__ __forceinline__ void eval_curve_block_flush(
    const CurveAcc& acc, bool is_owner, int own_idx, int wave, void* scratch,
    const CurveLds& s, long long* __restrict__ part_tot,
    unsigned int* __restrict__ part_hist) {
  constexpr int PER_WAVE = NOWN * EVAL_TT;
  unsigned int* s_tot = (unsigned int*)scratch;  // [NW][PER_WAVE][2]
  if (is_owner) {
    const int i = wave * PER_WAVE + own_idx;
    s_tot[2 * i + 0] = acc.n_pos;
    s_tot[2 * i + 1] = acc.n_neg;
  }
  __syncthreads();
  if (threadIdx.x < EVAL_TT) {
    const int t = threadIdx.x;
    long long c[2] = {0, 0};
    for (int w = 0; w < EVAL_NW; ++w)
      for (int o = 0; o < NOWN; ++o) {
        const int i = w * PER_WAVE + o * EVAL_TT + t;
        c[0] += s_tot[2 * i + 0];
        c[1] += s_tot[2 * i + 1];
      }
    part_tot[((size_t)blockIdx.x * 2 + 0) * EVAL_TT + t] = c[0];
    part_tot[((size_t)blockIdx.x * 2 + 1) * EVAL_TT + t] = c[1];
  }
  constexpr int NH = EVAL_TT * EVAL_KT * 2;
  for (int i = threadIdx.x; i < NH; i += EVAL_BLOCK)
    part_hist[(size_t)blockIdx.x * NH + i] = s.hist[i];
}

// ------------------------------------------------------------ dense, d<=2048
// eval_dense_kernel with CurveLds behind the W tile in dynamic LDS.
template <typename XT, int ITERS>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_curve_dense_kernel(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ Wt, const double* __restrict__ thr, long thr_ld,
    long long* __restrict__ part_tot, unsigned int* __restrict__ part_hist,
    long n_rows, int d) {
  constexpr int NV = EVAL_R * EVAL_TT;
  static_assert(eval_curve_flush_bytes(EVAL_R) <=
                    EVAL_TT * 256 * sizeof(float),
                "the flush reuses the tile's LDS");
  extern __shared__ double eval_smem[];  // tile [EVAL_TT][DPAD] fp32, CurveLds
  const CurveLds s(eval_smem + eval_lds_bytes(ITERS) / sizeof(double));
  s.init(thr, thr_ld);  // published by the walk's barrier after the tile load
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int key = eval_owner_key<NV, WAVE>(lane);
  const bool owner = (lane & (WAVE / NV - 1)) == 0;
  CurveAcc acc;
  eval_dense_rows<XT, ITERS>(X, y, Wt, n_rows, d, (float*)eval_smem,
                             [&](float z, float yv, bool valid) {
                               acc.add(z, yv, s, key % EVAL_TT,
                                       valid && owner);
                             });
  __syncthreads();  // every wave past its last row: tile dead, hist complete
  eval_curve_block_flush<EVAL_R>(acc, owner, key, wave, eval_smem, s,
                                 part_tot, part_hist);
}

// ------------------------------------------ dense fallback, any d (scalar)
template <typename XT>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_curve_dense_generic_kernel(
    const XT* __restrict__ X, const float* __restrict__ y,
    const float* __restrict__ Wt, const double* __restrict__ thr, long thr_ld,
    long long* __restrict__ part_tot, unsigned int* __restrict__ part_hist,
    long n_rows, int d) {
  __shared__ double curve_smem[eval_curve_lds_bytes() / sizeof(double)];
  __shared__ double scratch[eval_curve_flush_bytes(1) / sizeof(double)];
  const CurveLds s(curve_smem);
  s.init(thr, thr_ld);
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int my_t = eval_owner_key<EVAL_TT, WAVE>(lane);
  const bool owner = (lane & (WAVE / EVAL_TT - 1)) == 0;
  CurveAcc acc;
  eval_generic_rows<XT>(X, y, Wt, n_rows, d,
                        [&](float z, float yv, bool valid) {
                          acc.add(z, yv, s, my_t, valid && owner);
                        });
  __syncthreads();
  eval_curve_block_flush<1>(acc, owner, my_t, wave, scratch, s, part_tot,
                            part_hist);
}

// --------------------------------------------------------------------- CSR
template <typename VT, int LPR>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_curve_csr_kernel(
    const int* __restrict__ indptr, const int* __restrict__ indices,
    const VT* __restrict__ values, const float* __restrict__ y,
    const float* __restrict__ Wtt, const double* __restrict__ thr,
    long thr_ld, long long* __restrict__ part_tot,
    unsigned int* __restrict__ part_hist, long n_rows) {
  constexpr int NSUB = WAVE / LPR;
  __shared__ double curve_smem[eval_curve_lds_bytes() / sizeof(double)];
  __shared__ double scratch[eval_curve_flush_bytes(NSUB) / sizeof(double)];
  const CurveLds s(curve_smem);
  s.init(thr, thr_ld);
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const int sub = (threadIdx.x & 63) / LPR;
  const int sl = threadIdx.x % LPR;
  const int my_t = eval_owner_key<EVAL_TT, LPR>(sl);
  const bool owner = (sl & (LPR / EVAL_TT - 1)) == 0;
  CurveAcc acc;
  eval_csr_rows<VT, LPR>(indptr, indices, values, y, Wtt, n_rows,
                         [&](float z, float yv, bool valid) {
                           acc.add(z, yv, s, my_t, valid && owner);
                         });
  __syncthreads();
  eval_curve_block_flush<NSUB>(acc, owner, sub * EVAL_TT + my_t, wave,
                               scratch, s, part_tot, part_hist);
}

// Finish: block t, thread (k, c). Sum the blocks' partials in index order,
// then the suffix sums over k. k_valid thresholds of this pass are real;
// out_cnt is [4][..][ld_k] (tp, fp, tn, fn; q_stride elements apart) already
// offset to this tile's first iterate and this pass's first threshold,
// out_tot [2][tot_stride] (n_pos, n_neg) to this tile's first iterate.
__global__ __launch_bounds__(2 * EVAL_KT) void eval_curve_finish_kernel(
    const long long* __restrict__ part_tot,
    const unsigned int* __restrict__ part_hist, int G, int k_valid,
    long long* __restrict__ out_cnt, long ld_k, long q_stride,
    long long* __restrict__ out_tot, long tot_stride) {
  constexpr int NH = EVAL_TT * EVAL_KT * 2;
  __shared__ long long sh[2 * EVAL_KT];
  __shared__ long long sh_tot[2];
  const int t = blockIdx.x;
  const int i = threadIdx.x, k = i >> 1, c = i & 1;  // c = 1: positives
  long long sum = 0;
  for (int b = 0; b < G; ++b)
    sum += part_hist[(size_t)b * NH + (size_t)t * EVAL_KT * 2 + i];
  sh[i] = sum;
  if (i < 2) {
    long long tot = 0;
    for (int b = 0; b < G; ++b)
      tot += part_tot[((size_t)b * 2 + i) * EVAL_TT + t];
    sh_tot[i] = tot;  // 0: positives, 1: negatives
    out_tot[(size_t)i * tot_stride + t] = tot;
  }
  __syncthreads();
  if (k >= k_valid) return;
  long long above = 0;
  for (int j = k; j < EVAL_KT; ++j) above += sh[2 * j + c];
  const long long total = sh_tot[1 - c];
  // c = 1: tp (q 0) and fn (q 3); c = 0: fp (q 1) and tn (q 2)
  const size_t at = (size_t)t * ld_k + k;
  out_cnt[(size_t)(c ? 0 : 1) * q_stride + at] = above;
  out_cnt[(size_t)(c ? 3 : 2) * q_stride + at] = total - above;
}

// ---------------------------------------------------------------- launchers

struct EvalCurve {
  static constexpr size_t extra_lds = eval_curve_lds_bytes();
  template <typename XT, int ITERS>
  static const void* dense() {
    return (const void*)eval_curve_dense_kernel<XT, ITERS>;
  }
  template <typename XT>
  static const void* generic() {
    return (const void*)eval_curve_dense_generic_kernel<XT>;
  }
  template <typename VT, int LPR>
  static const void* csr() {
    return (const void*)eval_curve_csr_kernel<VT, LPR>;
  }
};

// One finish launch for (tile, pass): shared by the dense and CSR launchers.
static void eval_curve_finish(int tile, int pass, int n_tiles, int n_pass,
                              long K, int grid, long long* part_tot,
                              unsigned int* part_hist, long long* out_cnt,
                              long long* out_tot, hipStream_t stream) {
  const long t_pad = (long)n_tiles * EVAL_TT;
  const long k0 = (long)pass * EVAL_KT;
  const int k_valid = (int)(K - k0 < EVAL_KT ? K - k0 : EVAL_KT);
  hipLaunchKernelGGL(eval_curve_finish_kernel, dim3(EVAL_TT),
                     dim3(2 * EVAL_KT), 0, stream, part_tot, part_hist, grid,
                     k_valid, out_cnt + (size_t)tile * EVAL_TT * K + k0, K,
                     t_pad * K, out_tot + (size_t)tile * EVAL_TT, t_pad);
}

extern "C" {

int query_eval_curve_tile() { return EVAL_KT; }

// W as launch_eval_dense. thr: [n_tiles * EVAL_TT][n_pass * EVAL_KT] fp64,
// rows non-decreasing, padded with +inf past the K real thresholds.
// part_tot [grid][2][EVAL_TT] int64 and part_hist
// [grid][EVAL_TT][EVAL_KT][2] u32 are scratch reused by every (tile, pass)
// in stream order. out_cnt [4][n_tiles * EVAL_TT][K] int64 (tp, fp, tn,
// fn), out_tot [2][n_tiles * EVAL_TT] int64 (n_pos, n_neg).
void launch_eval_curve_dense(const void* X, const float* y, const float* W,
                             const double* thr, int n_tiles, int n_pass,
                             long K, long n_rows, int d, int x_is_bf16,
                             long long* part_tot, unsigned int* part_hist,
                             long long* out_cnt, long long* out_tot,
                             hipStream_t stream) {
  const int grid = eval_dense_grid(n_rows, d);
  const long thr_ld = (long)n_pass * EVAL_KT;
  for (int tile = 0; tile < n_tiles; ++tile)
    for (int pass = 0; pass < n_pass; ++pass) {
      const float* Wt = W + (size_t)tile * EVAL_TT * d;
      const double* th =
          thr + (size_t)tile * EVAL_TT * thr_ld + (size_t)pass * EVAL_KT;
      with_xt(x_is_bf16, [&](auto xt) {
        using XT = decltype(xt);
        if (eval_pipe_ok(d)) {
          with_const<1, 2, 3, 4, 5, 6, 7, 8>((d + 255) / 256, [&](auto IT) {
            constexpr int it = decltype(IT)::value;
            hipLaunchKernelGGL(
                (eval_curve_dense_kernel<XT, it>), dim3(grid),
                dim3(EVAL_BLOCK), eval_lds_bytes(it) + eval_curve_lds_bytes(),
                stream, (const XT*)X, y, Wt, th, thr_ld, part_tot, part_hist,
                n_rows, d);
          });
        } else {
          hipLaunchKernelGGL(eval_curve_dense_generic_kernel<XT>, dim3(grid),
                             dim3(EVAL_BLOCK), 0, stream, (const XT*)X, y, Wt,
                             th, thr_ld, part_tot, part_hist, n_rows, d);
        }
      });
      eval_curve_finish(tile, pass, n_tiles, n_pass, K, grid, part_tot,
                        part_hist, out_cnt, out_tot, stream);
    }
}

// Wtt as launch_eval_csr; the rest as launch_eval_curve_dense.
void launch_eval_curve_csr(const int* indptr, const int* indices,
                           const void* values, const float* y,
                           const float* Wtt, const double* thr, int n_tiles,
                           int n_pass, long K, long n_rows, int d,
                           int v_is_bf16, long long* part_tot,
                           unsigned int* part_hist, long long* out_cnt,
                           long long* out_tot, hipStream_t stream) {
  const int grid = eval_csr_grid(n_rows);
  const long thr_ld = (long)n_pass * EVAL_KT;
  for (int tile = 0; tile < n_tiles; ++tile)
    for (int pass = 0; pass < n_pass; ++pass) {
      const float* Wt = Wtt + (size_t)tile * EVAL_TT * d;
      const double* th =
          thr + (size_t)tile * EVAL_TT * thr_ld + (size_t)pass * EVAL_KT;
      with_xt(v_is_bf16, [&](auto vt) {
        using VT = decltype(vt);
        with_const<16, 32>(eval_csr_lpr(), [&](auto L) {
          hipLaunchKernelGGL(
              (eval_curve_csr_kernel<VT, decltype(L)::value>), dim3(grid),
              dim3(EVAL_BLOCK), 0, stream, indptr, indices, (const VT*)values,
              y, Wt, th, thr_ld, part_tot, part_hist, n_rows);
        });
      });
      eval_curve_finish(tile, pass, n_tiles, n_pass, K, grid, part_tot,
                        part_hist, out_cnt, out_tot, stream);
    }
}

int query_eval_curve_kernel(int idx, int* out) {
  return eval_query_kernel<EvalCurve>(idx, out);
}

}  // extern "C"
