// pybind11 bindings for the CDNA4 kernels (csrc/kernels.hip).
//
// The module is deliberately torch-ABI-free: functions take raw device
// pointers (as uintptr_t) + shapes + the HIP stream handle, which the thin
// Python adapter (asyncframework_amd/ops/hip.py) extracts from torch
// tensors. This keeps the extension a pure hipcc build (no hipify, no torch
// C++ headers) and lets the native runtime call the same launchers directly
// from C++. k_dev (nullable) is the device-resident round counter used by
// the hipGraph engine (engine/graph.py).

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "launchers.h"
#include "multi_update.h"

namespace py = pybind11;

void register_libsvm(py::module_& m);  // csrc/libsvm_parser.cpp
void register_native_engine(py::module_& m);  // csrc/engine_native.cpp
void register_resident_engine(py::module_& m);  // csrc/engine_resident.hip

static void check(hipError_t err, const char* what) {
  if (err != hipSuccess)
    throw std::runtime_error(std::string(what) + ": " +
                             hipGetErrorString(err));
}

PYBIND11_MODULE(_hip_core, m) {
  m.doc() = "MI355X CDNA4 kernels for asyncframework_amd";

  m.def("grad_dense",
        [](uintptr_t X, uintptr_t y, uintptr_t w, uintptr_t g,
           uintptr_t g_part, uintptr_t n, uintptr_t k_dev, long n_rows,
           int d, uint64_t seed, uint32_t round_k, uint64_t row_start,
           double rate, int objective, int x_is_bf16, uintptr_t stream) {
          launch_grad_dense((const void*)X, (const float*)y, (const float*)w,
                            (float*)g, (float*)g_part, (int*)n,
                            (const int*)k_dev, n_rows, d, seed, round_k,
                            row_start, rate, objective, x_is_bf16,
                            (hipStream_t)stream);
          check(hipGetLastError(), "grad_dense launch");
        });

  m.def("grad_grid", [](long n_rows) { return query_grad_grid(n_rows); });

  m.def("scan_rows",
        [](uintptr_t y, uintptr_t rowlist, uintptr_t ylist, uintptr_t count,
           uintptr_t scan_round, long n_rows, uint64_t seed, uint32_t round_k,
           uint64_t row_start, double rate, uintptr_t stream) {
          launch_scan_rows((const float*)y, (int*)rowlist, (float*)ylist,
                           (int*)count, (const int*)scan_round, n_rows, seed,
                           round_k, row_start, rate, (hipStream_t)stream);
          check(hipGetLastError(), "scan_rows launch");
        });

  m.def("sgd_reduce_update",
        [](uintptr_t g_part, uintptr_t w, uintptr_t k_dev, uintptr_t ticket,
           float gamma, float inv_batch, int num_part, int d, int G,
           int splits, uintptr_t stream) {
          launch_sgd_reduce_update((const float*)g_part, (float*)w,
                                   (int*)k_dev, (int*)ticket, gamma,
                                   inv_batch, num_part, d, G, splits,
                                   (hipStream_t)stream);
          check(hipGetLastError(), "sgd_reduce_update launch");
        });

  m.def("bump_counter", [](uintptr_t p, uintptr_t stream) {
    launch_bump_counter((int*)p, (hipStream_t)stream);
    check(hipGetLastError(), "bump_counter launch");
  });

  m.def("grad_dense_list",
        [](uintptr_t X, uintptr_t w, uintptr_t g_part, uintptr_t rowlist,
           uintptr_t ylist, uintptr_t count, long n_rows, int d,
           int objective, int x_is_bf16, uintptr_t stream) {
          launch_grad_dense_list((const void*)X, (const float*)w,
                                 (float*)g_part, (const int*)rowlist,
                                 (const float*)ylist, (const int*)count,
                                 n_rows, d, objective, x_is_bf16,
                                 (hipStream_t)stream);
          check(hipGetLastError(), "grad_dense_list launch");
        });

  m.def("reduce_partials",
        [](uintptr_t g_part, uintptr_t g, int d, int G, int splits,
           uintptr_t stream) {
          launch_reduce_partials((const float*)g_part, (float*)g, d, G,
                                 splits, (hipStream_t)stream);
          check(hipGetLastError(), "reduce_partials launch");
        });

  m.def("saga_grad_dense",
        [](uintptr_t X, uintptr_t y, uintptr_t w, uintptr_t alpha, uintptr_t g,
           uintptr_t g_part, uintptr_t n, uintptr_t idx, uintptr_t e,
           uintptr_t pos, uintptr_t k_dev, int commit_now, long n_rows,
           int d, uint64_t seed, uint32_t round_k, uint64_t row_start,
           double rate, int objective, int x_is_bf16, uintptr_t stream) {
          launch_saga_grad_dense((const void*)X, (const float*)y,
                                 (const float*)w, (float*)alpha, (float*)g,
                                 (float*)g_part, (int*)n, (int*)idx,
                                 (float*)e, (int*)pos, (const int*)k_dev,
                                 commit_now, n_rows, d, seed, round_k,
                                 row_start, rate, objective, x_is_bf16,
                                 (hipStream_t)stream);
          check(hipGetLastError(), "saga_grad_dense launch");
        });

  m.def("grad_csr",
        [](uintptr_t indptr, uintptr_t indices, uintptr_t values, uintptr_t y,
           uintptr_t w, uintptr_t g, uintptr_t n, uintptr_t k_dev,
           long n_rows, uint64_t seed, uint32_t round_k, uint64_t row_start,
           double rate, int objective, int v_is_bf16, uintptr_t stream) {
          launch_grad_csr((const int*)indptr, (const int*)indices,
                          (const void*)values, (const float*)y,
                          (const float*)w, (float*)g, (int*)n,
                          (const int*)k_dev, n_rows, seed, round_k, row_start,
                          rate, objective, v_is_bf16, (hipStream_t)stream);
          check(hipGetLastError(), "grad_csr launch");
        });

  m.def("saga_grad_csr",
        [](uintptr_t indptr, uintptr_t indices, uintptr_t values, uintptr_t y,
           uintptr_t w, uintptr_t alpha, uintptr_t g, uintptr_t n,
           uintptr_t idx, uintptr_t e, uintptr_t pos, uintptr_t k_dev,
           int commit_now, long n_rows, uint64_t seed, uint32_t round_k,
           uint64_t row_start, double rate, int objective, int v_is_bf16,
           uintptr_t stream) {
          launch_saga_grad_csr((const int*)indptr, (const int*)indices,
                               (const void*)values, (const float*)y,
                               (const float*)w, (float*)alpha, (float*)g,
                               (int*)n, (int*)idx, (float*)e, (int*)pos,
                               (const int*)k_dev, commit_now, n_rows, seed,
                               round_k, row_start, rate, objective, v_is_bf16,
                               (hipStream_t)stream);
          check(hipGetLastError(), "saga_grad_csr launch");
        });

  // l2 / l1 trail with defaults: the pre-regularisation call shapes work
  m.def("sgd_update", [](uintptr_t w, uintptr_t g, float gamma_k,
                         float inv_batch, int d, uintptr_t stream, float l2,
                         float l1) {
    launch_sgd_update((float*)w, (const float*)g, gamma_k, inv_batch, d, l2,
                      l1, (hipStream_t)stream);
    check(hipGetLastError(), "sgd_update launch");
  }, py::arg("w"), py::arg("g"), py::arg("gamma_k"), py::arg("inv_batch"),
     py::arg("d"), py::arg("stream"), py::arg("l2") = 0.f,
     py::arg("l1") = 0.f);

  m.def("saga_update", [](uintptr_t w, uintptr_t g, uintptr_t ab, float gamma,
                          float inv_batch, float inv_N, int d,
                          uintptr_t stream, float l2, float l1) {
    launch_saga_update((float*)w, (const float*)g, (float*)ab, gamma,
                       inv_batch, inv_N, d, l2, l1, (hipStream_t)stream);
    check(hipGetLastError(), "saga_update launch");
  }, py::arg("w"), py::arg("g"), py::arg("alpha_bar"), py::arg("gamma"),
     py::arg("inv_batch"), py::arg("inv_N"), py::arg("d"), py::arg("stream"),
     py::arg("l2") = 0.f, py::arg("l1") = 0.f);

  m.def("saga_commit", [](uintptr_t alpha, uintptr_t idx, uintptr_t e, int n,
                          uintptr_t stream) {
    launch_saga_commit((float*)alpha, (const int*)idx, (const float*)e, n,
                       (hipStream_t)stream);
    check(hipGetLastError(), "saga_commit launch");
  });

  m.def("alpha_gather",
        [](uintptr_t a_dst, uintptr_t a_src, uintptr_t rows,
           uintptr_t count_dev, int cap, uintptr_t stream) {
          launch_alpha_gather((float*)a_dst, (const float*)a_src,
                              (const int*)rows, (const int*)count_dev, cap,
                              (hipStream_t)stream);
          check(hipGetLastError(), "alpha_gather launch");
        });

  m.def("sgd_update_fused",
        [](uintptr_t w, uintptr_t g, uintptr_t k_dev, float gamma,
           float inv_batch, int num_part, int d, uintptr_t stream) {
          launch_sgd_update_fused((float*)w, (float*)g, (int*)k_dev, gamma,
                                  inv_batch, num_part, d,
                                  (hipStream_t)stream);
          check(hipGetLastError(), "sgd_update_fused launch");
        });

  m.def("saga_update_fused",
        [](uintptr_t w, uintptr_t g, uintptr_t ab, uintptr_t k_dev,
           float gamma, float inv_batch, float inv_N, int d,
           uintptr_t stream) {
          launch_saga_update_fused((float*)w, (float*)g, (float*)ab,
                                   (int*)k_dev, gamma, inv_batch, inv_N, d,
                                   (hipStream_t)stream);
          check(hipGetLastError(), "saga_update_fused launch");
        });

  // What a dense gradient launch at feature dim d will run (the launchers'
  // own shape selection, csrc/kernels.hip): template parameters, compiled
  // register/scratch use and the occupancy the runtime computes for them.
  // A solo launch that takes the generic form (d > 2048, d % 4 != 0 or
  // ASYNCAMD_NO_PIPE=1) reports {kernel, lpr, dynamic_lds_bytes} only.
  m.def("dense_kernel_info", [](int d, int x_is_bf16, int saga, int wave) {
    py::dict out;
    long long form[3] = {0};
    query_dense_launch(d, form);
    if (!wave && d > 0 && !form[0]) {
      out["kernel"] = "grad_dense_kernel";
      out["lpr"] = (int)form[1];
      out["dynamic_lds_bytes"] = form[2];
      return out;
    }
    int v[8] = {0};
    const int rc = query_dense_kernel(d, x_is_bf16, saga, wave, v);
    if (rc == -1)
      throw std::runtime_error(
          "dense_kernel_info: d must be a multiple of 4 in [4, 2048] (wave "
          "launches have no generic form)");
    check((hipError_t)rc, "dense_kernel_info");
    out["kernel"] = wave ? "grad_dense_wave_kernel" : "grad_dense_pipe_kernel";
    out["lpr"] = 64;
    out["iters"] = v[0];
    out["depth"] = v[1];
    out["waves_per_simd_hint"] = v[2];
    out["num_regs"] = v[3];
    out["local_size_bytes"] = v[4];
    out["dynamic_lds_bytes"] = v[5];
    out["max_active_blocks_per_cu"] = v[6];
    return out;
  });

  // (pipelined?, lanes per row, generic-form dynamic LDS bytes) of a solo
  // dense launch at feature dim d, overrides included. No runtime call: the
  // Python wrappers check the LDS need with it before every launch.
  m.def("dense_launch_form", [](int d) {
    long long form[3] = {0};
    query_dense_launch(d, form);
    return py::make_tuple(form[0] != 0, (int)form[1], form[2]);
  });

  // What a CSR gradient launch will run: the lanes per row that
  // ASYNCAMD_CSR_LPR selects (an unrecognised value runs the default).
  m.def("csr_kernel_info", []() {
    py::dict out;
    out["kernel"] = "grad_csr_kernel";
    out["lpr"] = query_csr_lpr();
    return out;
  });

  // Direct launch of the native engine's batched update kernel (tests).
  // g_ptrs / wbuf_ptrs are the per-worker device buffers (the engine's
  // g_tab / wbuf_tab); gw / sw index them; gw entries must be distinct.
  // Synchronous: returns after the kernel has finished. eta / l2 / l1
  // (regularised form) trail with defaults; eta is the per-gradient bare
  // ASGD step and is required, one per gradient, when algo == 0 and a
  // penalty is non-zero.
  m.def("multi_update",
        [](uintptr_t w, std::vector<uintptr_t> g_ptrs,
           std::vector<uintptr_t> wbuf_ptrs, uintptr_t alpha_bar, float gamma,
           float inv_batch, float inv_N, int d, int algo,
           std::vector<int> gw, std::vector<int> sw,
           std::vector<float> scale, uintptr_t stream,
           std::vector<float> eta, float l2, float l1) {
          if (gw.size() > MU_MAX || sw.size() > MU_MAX)
            throw std::runtime_error("multi_update: batch exceeds MU_MAX");
          if (algo == 0 && scale.size() != gw.size())
            throw std::runtime_error("multi_update: len(scale) != len(gw)");
          if (!(l2 >= 0.f) || !(l1 >= 0.f) || std::isinf(l2) ||
              std::isinf(l1))
            throw std::runtime_error(
                "multi_update: l2/l1 must be finite and non-negative");
          const bool reg = l2 != 0.f || l1 != 0.f;
          if (reg && algo == 0 && eta.size() != gw.size())
            throw std::runtime_error("multi_update: len(eta) != len(gw)");
          MultiUpdateArgs a{};
          a.n = (int)gw.size();
          a.m = (int)sw.size();
          a.algo = algo;
          bool vec4 = d % 4 == 0 && ((w | alpha_bar) & 15) == 0;
          for (auto p : g_ptrs) vec4 = vec4 && (p & 15) == 0;
          for (auto p : wbuf_ptrs) vec4 = vec4 && (p & 15) == 0;
          for (int j = 0; j < a.n; ++j) {
            if (gw[j] < 0 || (size_t)gw[j] >= g_ptrs.size())
              throw std::runtime_error("multi_update: gw out of range");
            for (int q = 0; q < j; ++q)
              if (gw[q] == gw[j])
                throw std::runtime_error("multi_update: duplicate worker");
            a.gw[j] = gw[j];
            if (algo == 0) a.scale[j] = scale[j];
            if (algo == 0 && reg) a.eta[j] = eta[j];
          }
          for (int j = 0; j < a.m; ++j) {
            if (sw[j] < 0 || (size_t)sw[j] >= wbuf_ptrs.size())
              throw std::runtime_error("multi_update: sw out of range");
            a.sw[j] = sw[j];
          }
          void* tabs = nullptr;
          const size_t ng = g_ptrs.size(), nw = wbuf_ptrs.size();
          check(hipMalloc(&tabs, (ng + nw + 1) * sizeof(uintptr_t)),
                "multi_update tables");
          uintptr_t* g_tab = (uintptr_t*)tabs;
          uintptr_t* wbuf_tab = g_tab + ng;
          hipError_t e = hipSuccess;
          if (ng)
            e = hipMemcpy(g_tab, g_ptrs.data(), ng * sizeof(uintptr_t),
                          hipMemcpyHostToDevice);
          if (e == hipSuccess && nw)
            e = hipMemcpy(wbuf_tab, wbuf_ptrs.data(), nw * sizeof(uintptr_t),
                          hipMemcpyHostToDevice);
          if (e == hipSuccess) {
            launch_multi_update((float*)w, (float* const*)g_tab,
                                (float* const*)wbuf_tab, (float*)alpha_bar,
                                gamma, inv_batch, inv_N, d, &a, vec4 ? 1 : 0,
                                l2, l1, (hipStream_t)stream);
            e = hipGetLastError();
          }
          if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
          (void)hipFree(tabs);
          check(e, "multi_update");
          return vec4;
        },
        py::arg("w"), py::arg("g_ptrs"), py::arg("wbuf_ptrs"),
        py::arg("alpha_bar"), py::arg("gamma"), py::arg("inv_batch"),
        py::arg("inv_N"), py::arg("d"), py::arg("algo"), py::arg("gw"),
        py::arg("sw"), py::arg("scale"), py::arg("stream"),
        py::arg("eta") = std::vector<float>{}, py::arg("l2") = 0.f,
        py::arg("l1") = 0.f);

  // Compiled register / scratch / LDS use of the batched and the
  // sync-round update kernels: [vec4][reg] instantiations by name.
  m.def("update_kernel_info", []() {
    py::dict out;
    for (int k = 0; k < 8; ++k) {
      int v[3] = {0};
      check((hipError_t)query_update_kernel(k >> 2, (k >> 1) & 1, k & 1, v),
            "update_kernel_info");
      py::dict e;
      e["num_regs"] = v[0];
      e["local_size_bytes"] = v[1];
      e["shared_size_bytes"] = v[2];
      std::string name = (k >> 2) ? "sync_round_update_kernel"
                                  : "multi_update_kernel";
      name += std::string("<") + (((k >> 1) & 1) ? "true" : "false") + "," +
              ((k & 1) ? "true" : "false") + ">";
      out[py::str(name)] = e;
    }
    return out;
  });

  // Fused evaluation (csrc/eval.h). W is n_tiles zero-padded tiles of
  // [eval_tile()][d] fp32 (dense) or [d][eval_tile()] (CSR, transposed);
  // part_* are per-block scratch sized by eval_grid(); out_loss is
  // [n_tiles * tile] fp64 and out_cnt [4][n_tiles * tile] int64
  // (tp, fp, tn, fn).
  m.def("eval_tile", []() { return query_eval_tile(); });
  m.def("eval_grid", [](long n_rows, int d, int csr) {
    return query_eval_grid(n_rows, d, csr);
  });
  m.def("eval_dense",
        [](uintptr_t X, uintptr_t y, uintptr_t W, int n_tiles, long n_rows,
           int d, int objective, double z_thr, int x_is_bf16,
           uintptr_t part_loss, uintptr_t part_cnt, uintptr_t out_loss,
           uintptr_t out_cnt, uintptr_t stream) {
          launch_eval_dense((const void*)X, (const float*)y, (const float*)W,
                            n_tiles, n_rows, d, objective, z_thr, x_is_bf16,
                            (double*)part_loss, (long long*)part_cnt,
                            (double*)out_loss, (long long*)out_cnt,
                            (hipStream_t)stream);
          check(hipGetLastError(), "eval_dense launch");
        });
  m.def("eval_csr",
        [](uintptr_t indptr, uintptr_t indices, uintptr_t values, uintptr_t y,
           uintptr_t Wtt, int n_tiles, long n_rows, int d, int objective,
           double z_thr, int v_is_bf16, uintptr_t part_loss,
           uintptr_t part_cnt, uintptr_t out_loss, uintptr_t out_cnt,
           uintptr_t stream) {
          launch_eval_csr((const int*)indptr, (const int*)indices,
                          (const void*)values, (const float*)y,
                          (const float*)Wtt, n_tiles, n_rows, d, objective,
                          z_thr, v_is_bf16, (double*)part_loss,
                          (long long*)part_cnt, (double*)out_loss,
                          (long long*)out_cnt, (hipStream_t)stream);
          check(hipGetLastError(), "eval_csr launch");
        });

  // Compiled register / scratch / LDS use and blocks per CU of every
  // evaluation-kernel instantiation, by name.
  // `prefix` is "eval_" (K9) or "eval_curve_" (the threshold sweep).
  auto eval_info = [](int (*query)(int, int*), const std::string& prefix) {
    py::dict out;
    const int n = query_eval_kernel_count();
    for (int k = 0; k < n; ++k) {
      int v[7] = {0};
      check((hipError_t)query(k, v), "eval_kernel_info");
      py::dict e;
      e["num_regs"] = v[0];
      e["local_size_bytes"] = v[1];
      e["lds_bytes"] = v[2];
      e["max_active_blocks_per_cu"] = v[3];
      const std::string xt = v[5] ? "bf16" : "float";
      std::string name;
      if (v[4] == 0)
        name = "dense_kernel<" + xt + "," + std::to_string(v[6]) + ">";
      else if (v[4] == 1)
        name = "dense_generic_kernel<" + xt + ">";
      else
        name = "csr_kernel<" + xt + "," + std::to_string(v[6]) + ">";
      out[py::str(prefix + name)] = e;
    }
    return out;
  };
  m.def("eval_kernel_info",
        [eval_info]() { return eval_info(query_eval_kernel, "eval_"); });
  m.def("eval_curve_kernel_info", [eval_info]() {
    return eval_info(query_eval_curve_kernel, "eval_curve_");
  });

  // Threshold sweep (csrc/eval_curve.h). W as eval_dense / eval_csr; thr is
  // [n_tiles * eval_tile()][n_pass * eval_curve_tile()] fp64, each row
  // non-decreasing and +inf past the K real thresholds; part_tot
  // [grid][2][tile] int64 and part_hist [grid][tile][curve_tile][2] uint32
  // are per-block scratch; out_cnt is [4][n_tiles * tile][K] int64 (tp, fp,
  // tn, fn) and out_tot [2][n_tiles * tile] int64 (n_pos, n_neg).
  m.def("eval_curve_tile", []() { return query_eval_curve_tile(); });
  m.def("eval_curve_dense",
        [](uintptr_t X, uintptr_t y, uintptr_t W, uintptr_t thr, int n_tiles,
           int n_pass, long K, long n_rows, int d, int x_is_bf16,
           uintptr_t part_tot, uintptr_t part_hist, uintptr_t out_cnt,
           uintptr_t out_tot, uintptr_t stream) {
          launch_eval_curve_dense(
              (const void*)X, (const float*)y, (const float*)W,
              (const double*)thr, n_tiles, n_pass, K, n_rows, d, x_is_bf16,
              (long long*)part_tot, (unsigned int*)part_hist,
              (long long*)out_cnt, (long long*)out_tot, (hipStream_t)stream);
          check(hipGetLastError(), "eval_curve_dense launch");
        });
  m.def("eval_curve_csr",
        [](uintptr_t indptr, uintptr_t indices, uintptr_t values, uintptr_t y,
           uintptr_t Wtt, uintptr_t thr, int n_tiles, int n_pass, long K,
           long n_rows, int d, int v_is_bf16, uintptr_t part_tot,
           uintptr_t part_hist, uintptr_t out_cnt, uintptr_t out_tot,
           uintptr_t stream) {
          launch_eval_curve_csr(
              (const int*)indptr, (const int*)indices, (const void*)values,
              (const float*)y, (const float*)Wtt, (const double*)thr, n_tiles,
              n_pass, K, n_rows, d, v_is_bf16, (long long*)part_tot,
              (unsigned int*)part_hist, (long long*)out_cnt,
              (long long*)out_tot, (hipStream_t)stream);
          check(hipGetLastError(), "eval_curve_csr launch");
        });

  // Column statistics and standardisation (csrc/col_stats.h). The dense
  // scratch is sized by col_stats_geom(); out_f64 is [6][d] fp64 (mean, M2,
  // min, max, sum |x|, sum x^2) and out_nnz [d] int64.
  m.def("col_stats_geom", [](uintptr_t X, long n_rows, int d, int x_is_bf16) {
    long long v[5] = {0};
    query_col_stats_geom(n_rows, d,
                         query_col_stats_vec((const void*)X, d, x_is_bf16),
                         v);
    py::dict e;
    e["vec"] = v[0];
    e["grid_x"] = v[1];
    e["grid_y"] = v[2];
    e["row_slots"] = v[3];
    e["rows_per_block"] = v[4];
    return e;
  });
  m.def("col_stats_dense",
        [](uintptr_t X, long n_rows, int d, int x_is_bf16, uintptr_t part_f64,
           uintptr_t part_mm, uintptr_t part_nnz, uintptr_t out_f64,
           uintptr_t out_nnz, uintptr_t stream) {
          launch_col_stats_dense((const void*)X, n_rows, d, x_is_bf16,
                                 (double*)part_f64, (float*)part_mm,
                                 (int*)part_nnz, (double*)out_f64,
                                 (long long*)out_nnz, (hipStream_t)stream);
          check(hipGetLastError(), "col_stats_dense launch");
        });
  m.def("col_stats_csr",
        [](uintptr_t indptr, uintptr_t indices, uintptr_t values, long n_rows,
           int d, long nnz_hint, int v_is_bf16, uintptr_t sums,
           uintptr_t ints, uintptr_t out_f64, uintptr_t out_nnz,
           uintptr_t stream) {
          launch_col_stats_csr((const int*)indptr, (const int*)indices,
                               (const void*)values, n_rows, d, nnz_hint,
                               v_is_bf16, (double*)sums, (unsigned int*)ints,
                               (double*)out_f64, (long long*)out_nnz,
                               (hipStream_t)stream);
          check(hipGetLastError(), "col_stats_csr launch");
        });
  m.def("scale_dense",
        [](uintptr_t X, uintptr_t mean, uintptr_t factor, long n_rows, int d,
           int x_is_bf16, int with_mean, uintptr_t stream) {
          launch_scale_dense((void*)X, (const float*)mean,
                             (const float*)factor, n_rows, d, x_is_bf16,
                             with_mean, (hipStream_t)stream);
          check(hipGetLastError(), "scale_dense launch");
        });
  m.def("scale_csr",
        [](uintptr_t indices, uintptr_t values, uintptr_t factor, long nnz,
           int d, int v_is_bf16, uintptr_t stream) {
          launch_scale_csr((const int*)indices, (void*)values,
                           (const float*)factor, nnz, d, v_is_bf16,
                           (hipStream_t)stream);
          check(hipGetLastError(), "scale_csr launch");
        });
  // Compiled register / scratch / LDS use and blocks per CU of every
  // col_stats.h kernel, by name (LDS: the largest dynamic size a launch
  // takes).
  m.def("col_stats_kernel_info", []() {
    py::dict out;
    const int n = query_col_stats_kernel_count();
    for (int k = 0; k < n; ++k) {
      int v[8] = {0};
      check((hipError_t)query_col_stats_kernel(k, v),
            "col_stats_kernel_info");
      py::dict e;
      e["num_regs"] = v[0];
      e["local_size_bytes"] = v[1];
      e["lds_bytes"] = v[2];
      e["max_active_blocks_per_cu"] = v[3];
      const std::string xt = v[5] ? "bf16" : "float";
      const std::string vec = std::to_string(v[6]);
      std::string name;
      switch (v[4]) {
        case 0: name = "col_stats_dense_kernel<" + xt + "," + vec + ">"; break;
        case 1: name = "col_stats_finish_kernel"; break;
        case 2: name = "col_stats_csr_kernel<" + xt + ">"; break;
        case 3: name = "col_stats_csr_finish_kernel"; break;
        case 4:
          name = "scale_dense_kernel<" + xt + "," + vec + "," +
                 (v[7] ? "true" : "false") + ">";
          break;
        default: name = "scale_csr_kernel<" + xt + ">"; break;
      }
      out[py::str(name)] = e;
    }
    return out;
  });

  register_libsvm(m);
  register_native_engine(m);
  register_resident_engine(m);

  m.attr("__hip__") = true;
// source-provenance stamp: build_hip.py passes -DASYNCAMD_SRC_HASH=<sha256
// of csrc sources>; the Python loader refuses a binary whose stamp doesn't
// match the sources on disk (round-1 stale-binary postmortem).
#ifndef ASYNCAMD_SRC_HASH
#define ASYNCAMD_SRC_HASH "unstamped"
#endif
  m.attr("__src_hash__") = ASYNCAMD_SRC_HASH;
}
