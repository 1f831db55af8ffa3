// Column statistics and feature standardisation (K11): one streaming pass
// over the data produces, per column, count / mean / M2 = sum (x - mean)^2 /
// non-zeros / min / max / sum |x| / sum x^2 (MLlib's colStats); a second
// pass rewrites the data in place as (x - mean) * factor (StandardScaler).
//
// Included by kernels.hip after its row machinery (to_f32, with_const,
// with_bool) and after eval.h (with_xt): this file adds no loader of its own.
//
// Dense mapping, shared by the statistics and the scale kernel: a thread owns
// VEC adjacent columns (VEC = 4, one 16-byte fp32 / 8-byte bf16 access, when
// d % 4 == 0 and X is aligned to it; VEC = 1 otherwise) for its whole life
// and walks rows. The d / VEC column groups are cut into grid.x equal tiles
// of cpt <= 256 groups; a block's 256 threads are ty_n = 256 / cpt row slots
// of cpt threads (the rest idle), slot s taking rows r0 + s, r0 + s + ty_n,
// ... of the block's contiguous row range [r0, r0 + rpb). A block iteration
// therefore reads ty_n whole row pieces, each contiguous. Rows are read once
// and kept by nothing: no LDS staging, cs_unroll(VEC) row loads in flight per
// thread.
//
// Numerics of the statistics: every accumulator is fp64. An fp32 or bf16
// value widens exactly and its square is exact in fp64. A thread's pivot p
// is the first value it sees of the column; it keeps sum (x - p) and
// sum (x - p)^2, so its partial is n, mean = p + s1 / n, M2 = s2 - s1^2 / n
// with no cancellation against the column's offset. Partials merge with the
// pairwise update of Chan et al. in a fixed order: the block's row slots
// 0..ty_n-1 through LDS, then the blocks, in index order within sixteen
// segments and the segments in order, in col_stats_finish_kernel. A column of one value has s1 = s2 = 0 in every
// thread and delta = 0 in every merge: M2 == 0.0 exactly. The plain sums
// (sum x, sum |x|, sum x^2) are added in the same fixed order, and the
// reported mean is sum x / n, which keeps |mean * n - sum x| inside the
// any-order fp64 summation bound. No floating-point atomics; the grid is a
// function of the shape; two calls are bit-identical.
//
// CSR statistics follow MultivariateOnlineSummarizer: stored zeros are
// skipped, implicit zeros count towards n, mean, variance, min and max.
// The sums over the non-zeros go to fp64 [d] arrays with atomicAdd(double*)
// (reproducible to the summation bound, not bitwise); nnz, min and max use
// integer atomics on an order-preserving encoding and are exact.
#pragma once

#define CS_BLOCK 256
// Row loads a thread issues before it uses the first. The statistics
// kernel's fp64 state is 15 registers per column: two rows of four columns
// keep it at 5 waves per SIMD with no scratch (four rows: 3 waves, and a
// register cap at 4 waves spills).
constexpr int cs_unroll(int vec) { return vec == 4 ? 2 : 4; }
#define CS_MAX_BLOCKS 1024  // 4 blocks per CU, all resident at 5 waves per SIMD
#define CS_MIN_SLOT_ROWS 32  // rows per row slot before grid.y grows

// The launch geometry of the dense kernels, a function of the shape alone.
struct CsGeom {
  int cpt;    // column groups per tile (<= 256)
  int tiles;  // grid.x
  int ty_n;   // row slots per block
  int gy;     // grid.y: blocks over rows, none empty
  long rpb;   // rows per block
};
static inline CsGeom cs_geom(long n_rows, int d, int vec) {
  CsGeom g;
  const int C = d / vec;
  g.tiles = (C + CS_BLOCK - 1) / CS_BLOCK;
  if (g.tiles < 1) g.tiles = 1;
  g.cpt = (C + g.tiles - 1) / g.tiles;
  if (g.cpt < 1) g.cpt = 1;
  g.ty_n = CS_BLOCK / g.cpt;
  const long min_rows = (long)CS_MIN_SLOT_ROWS * g.ty_n;
  long gy = (n_rows + min_rows - 1) / min_rows;
  const long cap = CS_MAX_BLOCKS / g.tiles;
  if (gy > cap) gy = cap;
  if (gy < 1) gy = 1;
  g.rpb = (n_rows + gy - 1) / gy;
  if (g.rpb < 1) g.rpb = 1;
  g.gy = (int)((n_rows + g.rpb - 1) / g.rpb);
  if (g.gy < 1) g.gy = 1;
  return g;
}
// LDS of the statistics kernel's block merge: four 8-byte slots per
// (row slot, column) — none when a block has one row slot.
static inline size_t cs_lds_bytes(const CsGeom& g, int vec) {
  return g.ty_n > 1 ? (size_t)4 * g.ty_n * g.cpt * vec * sizeof(double) : 0;
}

// rows that row slot `ty` of a block with `nb` rows walks
__device__ __forceinline__ long cs_slot_rows(long nb, int ty, int ty_n) {
  return ty < nb ? (nb - ty + ty_n - 1) / ty_n : 0;
}

// VEC adjacent elements as floats, and back (round to nearest even).
template <typename XT, int VEC>
__device__ __forceinline__ void cs_load(const XT* p, float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    if constexpr (std::is_same<XT, float>::value) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      o[0] = __uint_as_float(v.x << 16);
      o[1] = __uint_as_float(v.x & 0xffff0000u);
      o[2] = __uint_as_float(v.y << 16);
      o[3] = __uint_as_float(v.y & 0xffff0000u);
    }
  } else {
    o[0] = to_f32<XT>(p[0]);
  }
}
__device__ __forceinline__ unsigned int cs_bf16_bits(float f) {
  union { __hip_bfloat16 b; unsigned short u; } c;
  c.b = __float2bfloat16(f);
  return c.u;
}
template <typename XT, int VEC>
__device__ __forceinline__ void cs_store(XT* p, const float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    if constexpr (std::is_same<XT, float>::value) {
      *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      uint2 v;
      v.x = cs_bf16_bits(o[0]) | (cs_bf16_bits(o[1]) << 16);
      v.y = cs_bf16_bits(o[2]) | (cs_bf16_bits(o[3]) << 16);
      *reinterpret_cast<uint2*>(p) = v;
    }
  } else {
    if constexpr (std::is_same<XT, float>::value) p[0] = o[0];
    else p[0] = __float2bfloat16(o[0]);
  }
}

// One thread's running totals for one column.
struct ColAcc {
  double p, s1, s2, sx, sq, l1;
  float mn, mx;
  int nnz;
  __device__ __forceinline__ void first(float xf) {
    const double x = (double)xf;
    p = x; s1 = 0.0; s2 = 0.0; sx = x; sq = x * x; l1 = fabs(x);
    mn = xf; mx = xf;
    nnz = xf != 0.f;
  }
  __device__ __forceinline__ void add(float xf) {
    const double x = (double)xf;
    const double dl = x - p;
    s1 += dl;
    s2 = fma(dl, dl, s2);
    sx += x;
    sq = fma(x, x, sq);
    l1 += fabs(x);
    mn = fminf(mn, xf);
    mx = fmaxf(mx, xf);
    nnz += xf != 0.f;
  }
};

// (n, mean, M2) <- (n, mean, M2) merged with (nb, mb, m2b), nb > 0.
__device__ __forceinline__ void cs_chan(long& n, double& mean, double& m2,
                                        long nb, double mb, double m2b) {
  if (n == 0) {
    n = nb; mean = mb; m2 = m2b;
    return;
  }
  const long nn = n + nb;
  const double delta = mb - mean;
  mean += delta * ((double)nb / (double)nn);
  m2 = m2 + m2b + delta * delta * ((double)n * (double)nb / (double)nn);
  n = nn;
}

// part_f64 [gy][5][d]: mean, M2, sum x, sum |x|, sum x^2 of the block's rows;
// part_mm [gy][2][d]: min, max; part_nnz [gy][d].
template <typename XT, int VEC>
__global__ __launch_bounds__(CS_BLOCK) void col_stats_dense_kernel(
    const XT* __restrict__ X, long n_rows, int d, int cpt, int ty_n, long rpb,
    double* __restrict__ part_f64, float* __restrict__ part_mm,
    int* __restrict__ part_nnz) {
  extern __shared__ double cs_smem[];
  const int C = d / VEC;
  const int tx = threadIdx.x % cpt, ty = threadIdx.x / cpt;
  const int cg = blockIdx.x * cpt + tx;
  const bool live = ty < ty_n && cg < C;
  const long r0 = (long)blockIdx.y * rpb;
  const long r1 = r0 + rpb < n_rows ? r0 + rpb : n_rows;
  const long nb = r1 > r0 ? r1 - r0 : 0;
  const long cnt = live ? cs_slot_rows(nb, ty, ty_n) : 0;

  ColAcc acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v].first(0.f);
  if (cnt > 0) {
    const XT* col = X + (size_t)cg * VEC;
    const size_t step = (size_t)ty_n * d;
    const XT* ptr = col + (size_t)(r0 + ty) * d;
    constexpr int U = cs_unroll(VEC);
    float x[U][VEC];
    cs_load<XT, VEC>(ptr, x[0]);
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v].first(x[0][v]);
    ptr += step;
    long k = 1;
    for (; k + U <= cnt; k += U) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        cs_load<XT, VEC>(ptr + (size_t)u * step, x[u]);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v].add(x[u][v]);
      ptr += (size_t)U * step;
    }
    for (; k < cnt; ++k) {
      cs_load<XT, VEC>(ptr, x[0]);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v].add(x[0][v]);
      ptr += step;
    }
  }

  // the thread's partial
  double mean[VEC], m2[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const double c = cnt > 0 ? (double)cnt : 1.0;
    mean[v] = acc[v].p + acc[v].s1 / c;
    const double q = acc[v].s2 - acc[v].s1 * acc[v].s1 / c;
    m2[v] = q < 0.0 ? 0.0 : q;
  }

  long n_tot = cnt;
  if (ty_n > 1) {
    // row slots 0..ty_n-1 merge in that order, by the slot-0 thread of each
    // column group, in two rounds over the same LDS: [field][slot][column]
    const int W = cpt * VEC;
    const size_t F = (size_t)ty_n * W;
    const size_t me = (size_t)ty * W + (size_t)tx * VEC;
    if (live) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        cs_smem[0 * F + me + v] = mean[v];
        cs_smem[1 * F + me + v] = m2[v];
        cs_smem[2 * F + me + v] = acc[v].sx;
      }
    }
    __syncthreads();
    if (live && ty == 0) {
      for (int s = 1; s < ty_n; ++s) {
        const long ns = cs_slot_rows(nb, s, ty_n);
        if (ns == 0) break;  // slot counts never grow with s
        const size_t o = (size_t)s * W + (size_t)tx * VEC;
        long n_next = n_tot;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          long nv = n_tot;
          cs_chan(nv, mean[v], m2[v], ns, cs_smem[0 * F + o + v],
                  cs_smem[1 * F + o + v]);
          acc[v].sx += cs_smem[2 * F + o + v];
          n_next = nv;
        }
        n_tot = n_next;
      }
    }
    __syncthreads();
    float2* s_mm = reinterpret_cast<float2*>(cs_smem + 2 * F);
    int* s_nz = reinterpret_cast<int*>(cs_smem + 3 * F);
    if (live) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        cs_smem[0 * F + me + v] = acc[v].l1;
        cs_smem[1 * F + me + v] = acc[v].sq;
        s_mm[me + v] = make_float2(acc[v].mn, acc[v].mx);
        s_nz[me + v] = acc[v].nnz;
      }
    }
    __syncthreads();
    if (live && ty == 0) {
      for (int s = 1; s < ty_n; ++s) {
        if (cs_slot_rows(nb, s, ty_n) == 0) break;
        const size_t o = (size_t)s * W + (size_t)tx * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc[v].l1 += cs_smem[0 * F + o + v];
          acc[v].sq += cs_smem[1 * F + o + v];
          const float2 mm = s_mm[o + v];
          acc[v].mn = fminf(acc[v].mn, mm.x);
          acc[v].mx = fmaxf(acc[v].mx, mm.y);
          acc[v].nnz += s_nz[o + v];
        }
      }
    }
  }

  if (live && ty == 0) {
    const size_t b = blockIdx.y;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const size_t j = (size_t)cg * VEC + v;
      part_f64[(b * 5 + 0) * d + j] = mean[v];
      part_f64[(b * 5 + 1) * d + j] = m2[v];
      part_f64[(b * 5 + 2) * d + j] = acc[v].sx;
      part_f64[(b * 5 + 3) * d + j] = acc[v].l1;
      part_f64[(b * 5 + 4) * d + j] = acc[v].sq;
      part_mm[(b * 2 + 0) * d + j] = acc[v].mn;
      part_mm[(b * 2 + 1) * d + j] = acc[v].mx;
      part_nnz[b * d + j] = acc[v].nnz;
    }
  }
}

// The blocks' partials merge in a fixed two-level order: a finish block takes
// CS_FIN_COLS columns; segment s of its CS_FIN_SEGS segments merges blocks
// [s * per, (s + 1) * per) in index order, then segment 0's thread merges the
// segments 1, 2, ... in order through LDS. (One thread per column over all
// gy <= 1024 blocks was a 1024-step dependent chain of loads and divisions.)
// out_f64 [6][d]: mean, M2, min, max, sum |x|, sum x^2; out_nnz [d].
#define CS_FIN_COLS 16
#define CS_FIN_SEGS 16
__global__ __launch_bounds__(CS_FIN_COLS * CS_FIN_SEGS)
void col_stats_finish_kernel(
    const double* __restrict__ part_f64, const float* __restrict__ part_mm,
    const int* __restrict__ part_nnz, long n_rows, int d, int gy, long rpb,
    double* __restrict__ out_f64, long long* __restrict__ out_nnz) {
  __shared__ double s_f64[5][CS_FIN_SEGS][CS_FIN_COLS];
  __shared__ long long s_cnt[2][CS_FIN_SEGS][CS_FIN_COLS];  // rows, nnz
  __shared__ float s_mm[2][CS_FIN_SEGS][CS_FIN_COLS];
  const int c = threadIdx.x % CS_FIN_COLS, seg = threadIdx.x / CS_FIN_COLS;
  const long j = (long)blockIdx.x * CS_FIN_COLS + c;
  const bool live = j < d;
  const int per = (gy + CS_FIN_SEGS - 1) / CS_FIN_SEGS;
  const int b0 = seg * per;
  const int b1 = b0 + per < gy ? b0 + per : gy;
  long n = 0;
  double mean = 0.0, m2 = 0.0, sx = 0.0, l1 = 0.0, sq = 0.0;
  float mn = 0.f, mx = 0.f;
  long long nnz = 0;
  if (live) {
    for (int b = b0; b < b1; ++b) {
      const long r0 = (long)b * rpb;
      const long nb = (r0 + rpb < n_rows ? r0 + rpb : n_rows) - r0;
      if (nb <= 0) break;
      const size_t bb = b;
      const float bmn = part_mm[(bb * 2 + 0) * d + j];
      const float bmx = part_mm[(bb * 2 + 1) * d + j];
      mn = n == 0 ? bmn : fminf(mn, bmn);
      mx = n == 0 ? bmx : fmaxf(mx, bmx);
      cs_chan(n, mean, m2, nb, part_f64[(bb * 5 + 0) * d + j],
              part_f64[(bb * 5 + 1) * d + j]);
      sx += part_f64[(bb * 5 + 2) * d + j];
      l1 += part_f64[(bb * 5 + 3) * d + j];
      sq += part_f64[(bb * 5 + 4) * d + j];
      nnz += part_nnz[bb * d + j];
    }
  }
  s_f64[0][seg][c] = mean;
  s_f64[1][seg][c] = m2;
  s_f64[2][seg][c] = sx;
  s_f64[3][seg][c] = l1;
  s_f64[4][seg][c] = sq;
  s_cnt[0][seg][c] = n;
  s_cnt[1][seg][c] = nnz;
  s_mm[0][seg][c] = mn;
  s_mm[1][seg][c] = mx;
  __syncthreads();
  if (!live || seg != 0) return;
  for (int t = 1; t < CS_FIN_SEGS; ++t) {
    const long nt = s_cnt[0][t][c];
    if (nt == 0) continue;
    mn = n == 0 ? s_mm[0][t][c] : fminf(mn, s_mm[0][t][c]);
    mx = n == 0 ? s_mm[1][t][c] : fmaxf(mx, s_mm[1][t][c]);
    cs_chan(n, mean, m2, nt, s_f64[0][t][c], s_f64[1][t][c]);
    sx += s_f64[2][t][c];
    l1 += s_f64[3][t][c];
    sq += s_f64[4][t][c];
    nnz += s_cnt[1][t][c];
  }
  const size_t D = d;
  out_f64[0 * D + j] = n > 0 ? sx / (double)n : 0.0;
  out_f64[1 * D + j] = m2;
  out_f64[2 * D + j] = (double)mn;
  out_f64[3 * D + j] = (double)mx;
  out_f64[4 * D + j] = l1;
  out_f64[5 * D + j] = sq;
  out_nnz[j] = nnz;
}

// x <- rne_XT((x - mean_j) * factor_j) in fp32, in place; the mapping of
// col_stats_dense_kernel. (x - mean) * factor is a subtraction and a
// multiplication, two roundings: nothing here can contract into an fma.
template <typename XT, int VEC, bool WITH_MEAN>
__global__ __launch_bounds__(CS_BLOCK) void scale_dense_kernel(
    XT* __restrict__ X, const float* __restrict__ mean,
    const float* __restrict__ factor, long n_rows, int d, int cpt, int ty_n,
    long rpb) {
  const int C = d / VEC;
  const int tx = threadIdx.x % cpt, ty = threadIdx.x / cpt;
  const int cg = blockIdx.x * cpt + tx;
  if (!(ty < ty_n && cg < C)) return;
  const long r0 = (long)blockIdx.y * rpb;
  const long r1 = r0 + rpb < n_rows ? r0 + rpb : n_rows;
  const long cnt = cs_slot_rows(r1 > r0 ? r1 - r0 : 0, ty, ty_n);
  if (cnt <= 0) return;
  float m[VEC], f[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    m[v] = WITH_MEAN ? mean[(size_t)cg * VEC + v] : 0.f;
    f[v] = factor[(size_t)cg * VEC + v];
  }
  const size_t step = (size_t)ty_n * d;
  XT* ptr = X + (size_t)cg * VEC + (size_t)(r0 + ty) * d;
  constexpr int U = 4;
  float x[U][VEC];
  auto apply = [&](float (&xx)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      xx[v] = WITH_MEAN ? (xx[v] - m[v]) * f[v] : xx[v] * f[v];
  };
  long k = 0;
  for (; k + U <= cnt; k += U) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      cs_load<XT, VEC>(ptr + (size_t)u * step, x[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      apply(x[u]);
      cs_store<XT, VEC>(ptr + (size_t)u * step, x[u]);
    }
    ptr += (size_t)U * step;
  }
  for (; k < cnt; ++k) {
    cs_load<XT, VEC>(ptr, x[0]);
    apply(x[0]);
    cs_store<XT, VEC>(ptr, x[0]);
    ptr += step;
  }
}

// --------------------------------------------------------------------- CSR
// Order-preserving map of an fp32 onto unsigned integers: a < b as floats
// iff cs_enc(a) < cs_enc(b) (-0 sorts just below +0).
__device__ __forceinline__ unsigned int cs_enc(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cs_dec(unsigned int e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// One thread per stored entry p in [indptr[0], indptr[n_rows]), grid-strided.
// sums [3][d] fp64: sum x, sum x^2, sum |x| over the non-zeros; ints [3][d]:
// nnz, encoded min (starts at 0xffffffff), encoded max (starts at 0). An
// entry whose column is outside [0, d) is ignored.
template <typename VT>
__global__ __launch_bounds__(CS_BLOCK) void col_stats_csr_kernel(
    const int* __restrict__ indptr, const int* __restrict__ indices,
    const VT* __restrict__ values, long n_rows, int d,
    double* __restrict__ sums, unsigned int* __restrict__ ints) {
  const long lo = indptr[0], hi = indptr[n_rows];
  const long stride = (long)gridDim.x * CS_BLOCK;
  const size_t D = d;
  for (long p = lo + (long)blockIdx.x * CS_BLOCK + threadIdx.x; p < hi;
       p += stride) {
    const int j = indices[p];
    const float xf = to_f32<VT>(values[p]);
    if ((unsigned int)j >= (unsigned int)d || xf == 0.f) continue;
    const double x = (double)xf;
    atomicAdd(&sums[0 * D + j], x);
    atomicAdd(&sums[1 * D + j], x * x);
    atomicAdd(&sums[2 * D + j], fabs(x));
    atomicAdd(&ints[0 * D + j], 1u);
    const unsigned int e = cs_enc(xf);
    atomicMin(&ints[1 * D + j], e);
    atomicMax(&ints[2 * D + j], e);
  }
}

// out_f64 [6][d] and out_nnz [d] as col_stats_finish_kernel.
__global__ __launch_bounds__(CS_BLOCK) void col_stats_csr_finish_kernel(
    const double* __restrict__ sums, const unsigned int* __restrict__ ints,
    long n_rows, int d, double* __restrict__ out_f64,
    long long* __restrict__ out_nnz) {
  const long j = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
  if (j >= d) return;
  const size_t D = d;
  const double S = sums[0 * D + j], Q = sums[1 * D + j], A = sums[2 * D + j];
  const long nnz = ints[0 * D + j];
  double mn = 0.0, mx = 0.0, m2 = 0.0;
  if (nnz > 0) {
    mn = (double)cs_dec(ints[1 * D + j]);
    mx = (double)cs_dec(ints[2 * D + j]);
    if (nnz < n_rows) {  // the implicit zeros
      mn = mn < 0.0 ? mn : 0.0;
      mx = mx > 0.0 ? mx : 0.0;
    }
    const double k = (double)nnz, n = (double)n_rows;
    const double m_nnz = S / k;
    const double within = Q - S * S / k;
    m2 = (within < 0.0 ? 0.0 : within) +
         m_nnz * m_nnz * k * ((double)(n_rows - nnz) / n);
    if (m2 < 0.0 || mn == mx) m2 = 0.0;
  }
  out_f64[0 * D + j] = n_rows > 0 ? S / (double)n_rows : 0.0;
  out_f64[1 * D + j] = m2;
  out_f64[2 * D + j] = mn;
  out_f64[3 * D + j] = mx;
  out_f64[4 * D + j] = A;
  out_f64[5 * D + j] = Q;
  out_nnz[j] = nnz;
}

// v <- rne_VT(v * factor[indices]) in fp32, in place, over all nnz stored
// entries; an entry whose column is outside [0, d) is left alone.
template <typename VT>
__global__ __launch_bounds__(CS_BLOCK) void scale_csr_kernel(
    const int* __restrict__ indices, VT* __restrict__ values,
    const float* __restrict__ factor, long nnz, int d) {
  const long stride = (long)gridDim.x * CS_BLOCK;
  for (long p = (long)blockIdx.x * CS_BLOCK + threadIdx.x; p < nnz;
       p += stride) {
    const int j = indices[p];
    if ((unsigned int)j >= (unsigned int)d) continue;
    float o[1] = {to_f32<VT>(values[p]) * factor[j]};
    cs_store<VT, 1>(values + p, o);
  }
}

// ---------------------------------------------------------------- launchers

// the vector form needs d % 4 == 0 and X aligned to one 4-element access
static inline int cs_vec(const void* X, int d, int is_bf16) {
  const uintptr_t align = is_bf16 ? 8 : 16;
  return d % 4 == 0 && ((uintptr_t)X % align) == 0 ? 4 : 1;
}
// CSR grids: a function of the number of stored entries alone
static inline int cs_csr_grid(long nnz) {
  long g = (nnz + 4L * CS_BLOCK - 1) / (4L * CS_BLOCK);
  if (g > 2 * CS_MAX_BLOCKS) g = 2 * CS_MAX_BLOCKS;
  return g < 1 ? 1 : (int)g;
}

// Compiled resource use of kernel `idx`; out = {numRegs, localSizeBytes
// (scratch), static + largest dynamic LDS bytes, max active blocks per CU,
// kind, xt, vec, with_mean}. kind: 0 col_stats_dense, 1 col_stats_finish,
// 2 col_stats_csr, 3 col_stats_csr_finish, 4 scale_dense, 5 scale_csr.
#define CS_N_KERNELS (4 + 1 + 2 + 1 + 8 + 2)
static int cs_query_kernel(int idx, int* out) {
  const void* fn = nullptr;
  size_t dyn = 0;
  int kind = 0, bf = 0, vec = 0, wm = 0;
  if (idx < 4) {
    bf = idx / 2;
    vec = idx % 2 ? 1 : 4;
    dyn = (size_t)4 * CS_BLOCK * vec * sizeof(double);
    with_xt(bf, [&](auto xt) {
      with_const<4, 1>(vec, [&](auto V) {
        fn = (const void*)
            col_stats_dense_kernel<decltype(xt), decltype(V)::value>;
      });
    });
  } else if (idx < 5) {
    kind = 1;
    fn = (const void*)col_stats_finish_kernel;
  } else if (idx < 7) {
    kind = 2;
    bf = idx - 5;
    with_xt(bf, [&](auto vt) {
      fn = (const void*)col_stats_csr_kernel<decltype(vt)>;
    });
  } else if (idx < 8) {
    kind = 3;
    fn = (const void*)col_stats_csr_finish_kernel;
  } else if (idx < 16) {
    kind = 4;
    const int k = idx - 8;
    bf = k / 4;
    vec = (k / 2) % 2 ? 1 : 4;
    wm = k % 2;
    with_xt(bf, [&](auto xt) {
      with_const<4, 1>(vec, [&](auto V) {
        with_bool(wm != 0, [&](auto M) {
          fn = (const void*)scale_dense_kernel<decltype(xt),
                                               decltype(V)::value,
                                               decltype(M)::value>;
        });
      });
    });
  } else if (idx < CS_N_KERNELS) {
    kind = 5;
    bf = idx - 16;
    with_xt(bf, [&](auto vt) {
      fn = (const void*)scale_csr_kernel<decltype(vt)>;
    });
  } else {
    return -1;
  }
  hipFuncAttributes attr;
  hipError_t e = hipFuncGetAttributes(&attr, fn);
  int nb = 0;
  if (e == hipSuccess)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, CS_BLOCK, dyn);
  if (e != hipSuccess) return (int)e;
  out[0] = attr.numRegs;
  out[1] = (int)attr.localSizeBytes;
  out[2] = (int)(attr.sharedSizeBytes + dyn);
  out[3] = nb;
  out[4] = kind;
  out[5] = bf;
  out[6] = vec;
  out[7] = wm;
  return 0;
}

extern "C" {

// out[5] = {vec, tiles (grid.x), gy (grid.y), row slots per block, rows per
// block} of the dense kernels at this shape and alignment
void query_col_stats_geom(long n_rows, int d, int vec, long long* out) {
  const CsGeom g = cs_geom(n_rows, d, vec == 4 ? 4 : 1);
  out[0] = vec == 4 ? 4 : 1;
  out[1] = g.tiles;
  out[2] = g.gy;
  out[3] = g.ty_n;
  out[4] = g.rpb;
}
int query_col_stats_vec(const void* X, int d, int x_is_bf16) {
  return cs_vec(X, d, x_is_bf16);
}

// part_f64 [gy][5][d], part_mm [gy][2][d], part_nnz [gy][d] are scratch sized
// by query_col_stats_geom; out_f64 [6][d] (mean, M2, min, max, sum |x|,
// sum x^2), out_nnz [d]. n_rows > 0.
void launch_col_stats_dense(const void* X, long n_rows, int d, int x_is_bf16,
                            double* part_f64, float* part_mm, int* part_nnz,
                            double* out_f64, long long* out_nnz,
                            hipStream_t stream) {
  const int vec = cs_vec(X, d, x_is_bf16);
  const CsGeom g = cs_geom(n_rows, d, vec);
  with_xt(x_is_bf16, [&](auto xt) {
    using XT = decltype(xt);
    with_const<4, 1>(vec, [&](auto V) {
      hipLaunchKernelGGL((col_stats_dense_kernel<XT, decltype(V)::value>),
                         dim3(g.tiles, g.gy), dim3(CS_BLOCK),
                         cs_lds_bytes(g, vec), stream, (const XT*)X, n_rows,
                         d, g.cpt, g.ty_n, g.rpb, part_f64, part_mm,
                         part_nnz);
    });
  });
  hipLaunchKernelGGL(col_stats_finish_kernel,
                     dim3((d + CS_FIN_COLS - 1) / CS_FIN_COLS),
                     dim3(CS_FIN_COLS * CS_FIN_SEGS), 0, stream, part_f64,
                     part_mm, part_nnz, n_rows, d, g.gy, g.rpb, out_f64,
                     out_nnz);
}

// sums [3][d] fp64 and ints [3][d] uint32 are scratch, initialised here;
// nnz_hint (the number of stored entries) only sizes the grid.
void launch_col_stats_csr(const int* indptr, const int* indices,
                          const void* values, long n_rows, int d,
                          long nnz_hint, int v_is_bf16, double* sums,
                          unsigned int* ints, double* out_f64,
                          long long* out_nnz, hipStream_t stream) {
  const size_t D = d;
  (void)hipMemsetAsync(sums, 0, 3 * D * sizeof(double), stream);
  (void)hipMemsetAsync(ints, 0, D * sizeof(unsigned int), stream);
  (void)hipMemsetAsync(ints + D, 0xff, D * sizeof(unsigned int), stream);
  (void)hipMemsetAsync(ints + 2 * D, 0, D * sizeof(unsigned int), stream);
  with_xt(v_is_bf16, [&](auto vt) {
    using VT = decltype(vt);
    hipLaunchKernelGGL(col_stats_csr_kernel<VT>, dim3(cs_csr_grid(nnz_hint)),
                       dim3(CS_BLOCK), 0, stream, indptr, indices,
                       (const VT*)values, n_rows, d, sums, ints);
  });
  hipLaunchKernelGGL(col_stats_csr_finish_kernel,
                     dim3((d + CS_BLOCK - 1) / CS_BLOCK), dim3(CS_BLOCK), 0,
                     stream, sums, ints, n_rows, d, out_f64, out_nnz);
}

void launch_scale_dense(void* X, const float* mean, const float* factor,
                        long n_rows, int d, int x_is_bf16, int with_mean,
                        hipStream_t stream) {
  const int vec = cs_vec(X, d, x_is_bf16);
  const CsGeom g = cs_geom(n_rows, d, vec);
  with_xt(x_is_bf16, [&](auto xt) {
    using XT = decltype(xt);
    with_const<4, 1>(vec, [&](auto V) {
      with_bool(with_mean != 0, [&](auto M) {
        hipLaunchKernelGGL(
            (scale_dense_kernel<XT, decltype(V)::value, decltype(M)::value>),
            dim3(g.tiles, g.gy), dim3(CS_BLOCK), 0, stream, (XT*)X, mean,
            factor, n_rows, d, g.cpt, g.ty_n, g.rpb);
      });
    });
  });
}

void launch_scale_csr(const int* indices, void* values, const float* factor,
                      long nnz, int d, int v_is_bf16, hipStream_t stream) {
  with_xt(v_is_bf16, [&](auto vt) {
    using VT = decltype(vt);
    hipLaunchKernelGGL(scale_csr_kernel<VT>, dim3(cs_csr_grid(nnz)),
                       dim3(CS_BLOCK), 0, stream, indices, (VT*)values,
                       factor, nnz, d);
  });
}

int query_col_stats_kernel(int idx, int* out) {
  return cs_query_kernel(idx, out);
}
int query_col_stats_kernel_count() { return CS_N_KERNELS; }

}  // extern "C"
