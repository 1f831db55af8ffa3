// The one declaration of every extern "C" launcher and query that
// csrc/kernels.hip (and csrc/eval.h, which it includes) defines. The
// defining file includes this header, so a definition that disagrees with
// its declaration does not compile; the callers (bindings.cpp,
// engine_native.cpp) include it instead of re-declaring what they call.
// Grouped as the definitions are. The symbols carry no types, so this
// header is the only type check the ABI gets.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "multi_update.h"

extern "C" {

int query_grad_grid(long n_rows);

void launch_scan_rows(const float* y, int* rowlist, float* ylist,
                      int* count_dev, const int* scan_round_dev, long n_rows,
                      uint64_t seed, uint32_t round_k, uint64_t row_start,
                      double rate, hipStream_t stream);

void launch_bump_counter(int* p, hipStream_t stream);

void launch_grad_dense_list(const void* X, const float* w, float* g_part,
                            const int* rowlist, const float* ylist,
                            const int* count_dev, long n_rows, int d,
                            int objective, int x_is_bf16, hipStream_t stream);

// ---- dense gradient: solo (flag / flag-less) and wave -------------------

void launch_grad_dense_flag(
    const void* X, const float* y, const float* w, float* g_out,
    float* g_part, int* n_out, const int* k_dev, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, double rate,
    int objective, int x_is_bf16, hipStream_t stream,
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr);

void launch_saga_grad_dense_flag(
    const void* X, const float* y, const float* w, float* alpha,
    float* g_out, float* g_part, int* n_out, int* idx_out, float* e_out,
    int* pos_ctr, const int* k_dev, int commit_now, long n_rows, int d,
    uint64_t seed, uint32_t round_k, uint64_t row_start, double rate,
    int objective, int x_is_bf16, hipStream_t stream,
    unsigned long long* done_flag, unsigned long long done_val,
    unsigned long long* done_arr);

void launch_grad_dense(const void* X, const float* y, const float* w,
                       float* g_out, float* g_part, int* n_out,
                       const int* k_dev, long n_rows, int d, uint64_t seed,
                       uint32_t round_k, uint64_t row_start, double rate,
                       int objective, int x_is_bf16, hipStream_t stream);

void launch_saga_grad_dense(const void* X, const float* y, const float* w,
                            float* alpha, float* g_out, float* g_part,
                            int* n_out, int* idx_out, float* e_out,
                            int* pos_ctr, const int* k_dev, int commit_now,
                            long n_rows, int d, uint64_t seed,
                            uint32_t round_k, uint64_t row_start, double rate,
                            int objective, int x_is_bf16, hipStream_t stream);

// slots_dev: device GradWaveSlot[P]; cmd_host: host GradWaveCmd (grad_wave.h)
void launch_grad_dense_wave(const void* slots_dev, const void* cmd_host,
                            long max_rows, int d, uint64_t seed, double rate,
                            int objective, int x_is_bf16, int saga,
                            hipStream_t stream);

// out[8], see the definition
int query_dense_kernel(int d, int x_is_bf16, int saga, int wave, int* out);

// out[3], see the definition
void query_dense_launch(int d, long long* out);
int query_csr_lpr();

void launch_scan_rows_wave(const void* slots_dev, const void* cmd_host,
                           uint64_t seed, double rate, hipStream_t stream);

void launch_alpha_gather_wave(const void* slots_dev, const void* cmd_host,
                              hipStream_t stream);

// ---- CSR gradient: solo (flag / flag-less), partial reduce, wave --------

void launch_grad_csr_flag(
    const int* indptr, const int* indices, const void* values,
    const float* y, const float* w, float* g_out, int* n_out,
    const int* k_dev, long n_rows, uint64_t seed, uint32_t round_k,
    uint64_t row_start, double rate, int objective, int v_is_bf16,
    hipStream_t stream, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr);

void launch_saga_grad_csr_flag(
    const int* indptr, const int* indices, const void* values,
    const float* y, const float* w, float* alpha, float* g_out, int* n_out,
    int* idx_out, float* e_out, int* pos_ctr, const int* k_dev,
    int commit_now, long n_rows, uint64_t seed, uint32_t round_k,
    uint64_t row_start, double rate, int objective, int v_is_bf16,
    hipStream_t stream, unsigned long long* done_flag,
    unsigned long long done_val, unsigned long long* done_arr);

void launch_grad_csr(const int* indptr, const int* indices,
                     const void* values, const float* y, const float* w,
                     float* g_out, int* n_out, const int* k_dev, long n_rows,
                     uint64_t seed, uint32_t round_k, uint64_t row_start,
                     double rate, int objective, int v_is_bf16,
                     hipStream_t stream);

void launch_saga_grad_csr(const int* indptr, const int* indices,
                          const void* values, const float* y, const float* w,
                          float* alpha, float* g_out, int* n_out,
                          int* idx_out, float* e_out, int* pos_ctr,
                          const int* k_dev, int commit_now, long n_rows,
                          uint64_t seed, uint32_t round_k, uint64_t row_start,
                          double rate, int objective, int v_is_bf16,
                          hipStream_t stream);

void launch_reduce_partials(const float* g_part, float* g_out, int d, int G,
                            int splits, hipStream_t stream);

// slots_dev: device CsrWaveSlot[P]; cmd_host: host GradWaveCmd
void launch_grad_csr_wave(const void* slots_dev, const void* cmd_host,
                          uint64_t seed, double rate, int objective,
                          int v_is_bf16, int saga, hipStream_t stream);

// slots_dev: device CommitSlot[P]; cmd_host: host CsrCommitCmd
void launch_saga_commit_wave(const void* slots_dev, const void* cmd_host,
                             hipStream_t stream);

// ---- updates ------------------------------------------------------------

void launch_sgd_update(float* w, const float* g, float gamma_k,
                       float inv_batch, int d, float l2, float l1,
                       hipStream_t stream);

void launch_saga_update(float* w, const float* g, float* alpha_bar,
                        float gamma, float inv_batch, float inv_N, int d,
                        float l2, float l1, hipStream_t stream);

void launch_saga_commit(float* alpha, const int* idx, const float* e, int n,
                        hipStream_t stream);

void launch_sgd_reduce_update(const float* g_part, float* w, int* k_dev,
                              int* ticket, float gamma, float inv_batch,
                              int num_part, int d, int G, int splits,
                              hipStream_t stream);

void launch_sgd_update_fused(float* w, float* g, int* k_dev, float gamma,
                             float inv_batch, int num_part, int d,
                             hipStream_t stream);

void launch_saga_update_fused(float* w, float* g, float* alpha_bar,
                              int* k_dev, float gamma, float inv_batch,
                              float inv_N, int d, hipStream_t stream);

void launch_multi_update(float* w, float* const* g_tab,
                         float* const* wbuf_tab, float* alpha_bar,
                         float gamma, float inv_batch, float inv_N, int d,
                         const MultiUpdateArgs* a, int vec4, float l2,
                         float l1, hipStream_t stream);

void launch_sync_round_update(float* w, float* const* g_tab,
                              int* const* ctr_tab, float* alpha_bar,
                              float* snap_dst, int* ticket, int P, int d,
                              int mode, float scale, float gamma,
                              float inv_batch, float inv_N, int vec4,
                              float eta, float l2, float l1,
                              hipStream_t stream);

// out[3], see the definition
int query_update_kernel(int sync, int vec4, int reg, int* out);

void launch_saga_commit_devn(float* alpha, const int* idx, const float* e,
                             const int* n_dev, int cap, hipStream_t stream);

void launch_alpha_gather(float* a_dst, const float* a_src, const int* rows,
                         const int* count_dev, int cap, hipStream_t stream);

// ---- fused held-out evaluation (defined in eval.h) ----------------------

int query_eval_tile();
int query_eval_grid(long n_rows, int d, int csr);

void launch_eval_dense(const void* X, const float* y, const float* W,
                       int n_tiles, long n_rows, int d, int objective,
                       double z_thr, int x_is_bf16, double* part_loss,
                       long long* part_cnt, double* out_loss,
                       long long* out_cnt, hipStream_t stream);

void launch_eval_csr(const int* indptr, const int* indices,
                     const void* values, const float* y, const float* Wtt,
                     int n_tiles, long n_rows, int d, int objective,
                     double z_thr, int v_is_bf16, double* part_loss,
                     long long* part_cnt, double* out_loss,
                     long long* out_cnt, hipStream_t stream);

// out[7], see the definition
int query_eval_kernel(int idx, int* out);
int query_eval_kernel_count();

// ---- threshold sweep of the evaluation (defined in eval_curve.h) --------

int query_eval_curve_tile();

void launch_eval_curve_dense(const void* X, const float* y, const float* W,
                             const double* thr, int n_tiles, int n_pass,
                             long K, long n_rows, int d, int x_is_bf16,
                             long long* part_tot, unsigned int* part_hist,
                             long long* out_cnt, long long* out_tot,
                             hipStream_t stream);

void launch_eval_curve_csr(const int* indptr, const int* indices,
                           const void* values, const float* y,
                           const float* Wtt, const double* thr, int n_tiles,
                           int n_pass, long K, long n_rows, int d,
                           int v_is_bf16, long long* part_tot,
                           unsigned int* part_hist, long long* out_cnt,
                           long long* out_tot, hipStream_t stream);

// as query_eval_kernel, query_eval_kernel_count() instantiations
int query_eval_curve_kernel(int idx, int* out);

// ---- column statistics and standardisation (defined in col_stats.h) -----

// out[5], see the definition
void query_col_stats_geom(long n_rows, int d, int vec, long long* out);
int query_col_stats_vec(const void* X, int d, int x_is_bf16);

void launch_col_stats_dense(const void* X, long n_rows, int d, int x_is_bf16,
                            double* part_f64, float* part_mm, int* part_nnz,
                            double* out_f64, long long* out_nnz,
                            hipStream_t stream);

void launch_col_stats_csr(const int* indptr, const int* indices,
                          const void* values, long n_rows, int d,
                          long nnz_hint, int v_is_bf16, double* sums,
                          unsigned int* ints, double* out_f64,
                          long long* out_nnz, hipStream_t stream);

void launch_scale_dense(void* X, const float* mean, const float* factor,
                        long n_rows, int d, int x_is_bf16, int with_mean,
                        hipStream_t stream);

void launch_scale_csr(const int* indices, void* values, const float* factor,
                      long nnz, int d, int v_is_bf16, hipStream_t stream);

// out[8], see the definition
int query_col_stats_kernel(int idx, int* out);
int query_col_stats_kernel_count();

}  // extern "C"
