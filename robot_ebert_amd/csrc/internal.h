// Every ebt:: function that one .hip file of libebert defines and another calls, declared once.
// Included after common.h by the defining file and by every calling file, so that a changed
// signature fails to compile instead of failing when the library is loaded. Default arguments
// live here only.
//
// Linkage rule of csrc/ (the .hip files are linked into one library):
//   * A type or function used by one .hip file only is file-local: in an anonymous namespace, or
//     `static` for a function.
//   * Exception: a type named in a __global__ signature (EpiArgs, QpArgs, LeadArgs, UpdArgs,
//     MoveArgs, GatherArgs, ExclArgs, DenseSrc, PackedSrc) or used in device code keeps its name
//     and linkage, so that kernel symbols do not change; its name is unique in the library.
//   * A type shared by two files is defined in exactly one header (common.h, driver.h) under a
//     name that no .hip file defines.
//   * A function with external linkage is declared in common.h, here, or in driver.h.
#pragma once

#include "common.h"

namespace ebt {

// ---- api.hip ---------------------------------------------------------------------------------
int64_t shard_lead_room(int64_t B_pad, int64_t n_rows, int64_t sample_tiles);
int64_t shard_lead_tiles(int64_t B_pad, int64_t n_rows, int64_t sample_tiles);
int rescore_sharded(const double* q64, int64_t B, int32_t d, const void* cat, int dtype,
                    int64_t ld, const double* gnorm64, int64_t row_offset, const float* cand_vals,
                    const int64_t* cand_rows, int32_t kprime, int32_t k, int64_t n_rows,
                    const float* eps, const double* t_floor, double* out_s, int64_t* out_r,
                    int32_t* certified, const int* ovf, const float* theta, void* timer,
                    hipStream_t st, int64_t list_base, const int64_t* excl_off,
                    const int64_t* excl_rows, const ShardPackOut* pack);
int screen_at_local(const double* q64, const void* qimg, const float* qscale, const float* eps,
                    int64_t B, int64_t B_pad, const void* cat, int dtype, int64_t ld,
                    const double* gnorm64, const void* cimg, const float* cscale, int img_dtype,
                    int32_t ld_img, int64_t n_rows, int32_t d, int32_t d_pad, int64_t row_offset,
                    const int64_t* excl_off, const int64_t* excl_rows, int32_t k, int32_t kprime,
                    int64_t chunk_rows, void* workspace, size_t ws_bytes, float* list_vals,
                    int64_t* list_rows, const float* gsamp, int64_t gs_rstride, int gs_G,
                    int gs_gj, int gs_j, double hits, int64_t lead, const float* lead_scores,
                    int64_t ld_lead, const float** theta_dev, const int** ovf_dev,
                    const float** eps_dev, void* timer, hipStream_t st, float* floor_out,
                    int floor_w);

// ---- screen_gemm.hip -------------------------------------------------------------------------
int64_t gemm_cus();
int screen_gemm(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows, int32_t d_pad,
                int32_t ld_img, int img_dtype, const float* qscale, const float* cscale,
                float* scores, int64_t ld_scores, hipStream_t stream, int64_t cstride = 0);
int screen_gemm_pool(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows,
                     int32_t d_pad, int32_t ld_img, int img_dtype, const float* qscale,
                     const float* cscale, int64_t cstride, float* pooled, int64_t ld_pooled,
                     hipStream_t stream, int64_t lead = 0, float* lead_scores = nullptr,
                     int64_t ld_lead = 0);
int64_t filter_group_rows(int64_t B_pad);
int screen_gemm_filter(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows,
                       int32_t d_pad, int32_t ld_img, int img_dtype, const float* qscale,
                       const float* cscale, const float* thr, uint64_t* cand, int64_t ld_cand,
                       int slots, uint8_t* counts, int64_t ld_counts, int* ovf, int64_t idx_base,
                       hipStream_t stream);
int64_t filter_split_rows(int64_t B_pad, int64_t n_rows);

// ---- select_topk.hip -------------------------------------------------------------------------
int select_topk(const float* vals, const int64_t* idx, int64_t ld, int64_t B, int64_t n,
                int64_t idx_base, int32_t kprime, int32_t segs, float* out_vals, int64_t* out_idx,
                int64_t ld_out, hipStream_t stream);
int merge_segment(float* fv, int64_t* fi, int64_t B, int kprime, const uint64_t* cand,
                  int64_t ld_cand, int slots, const uint8_t* counts, int64_t ld_counts,
                  int64_t n_groups, int64_t row_offset, const int64_t* eo, const int64_t* er,
                  int* ovf, hipStream_t st, double expect_hits = 0.0);
bool merge_wave_fits(int kprime);
int merge_block_capacity(int kprime);
int64_t merge_block_max_groups(int kprime);
int64_t merge_wave_max_groups();
int merge_wave_capacity();
int merge_segment_wave(float* fv, int64_t* fi, int64_t B, int kprime, int k, const uint64_t* cand,
                       int64_t ld_cand, int slots, const uint8_t* counts, int64_t ld_counts,
                       int64_t n_groups, int64_t row_offset, const int64_t* eo, const int64_t* er,
                       int* ovf, hipStream_t st, const float* veps = nullptr,
                       const float* vspec = nullptr, float* fout = nullptr, int fw = 0,
                       const float* feps = nullptr, float* tout = nullptr,
                       const float* tin = nullptr, const float* teps = nullptr, int64_t B_pad = 0);
int pilot_topk(const float* S, int64_t ld_s, int64_t B, int n, int64_t idx_base, int kprime, int k,
               float* fv, int64_t* fi, hipStream_t st);
int kth_threshold(const float* vals, int64_t ld, int64_t B, int64_t B_pad, int k, const float* eps,
                  float* thr, hipStream_t st);
int pool_kth(const float* pool, int64_t ld, int64_t B, int64_t B_pad, int G, int j, float* thr,
             hipStream_t st, float* fv = nullptr, int64_t* fi = nullptr, int kprime = 0,
             int* ovf = nullptr, const float* lead_s = nullptr, int64_t ld_lead = 0, int lead = 0,
             uint64_t* cand = nullptr, int64_t ld_cand = 0, int slots = 0,
             uint8_t* counts = nullptr, int64_t ld_counts = 0, int gj = 0, int64_t rstride = 0);
int spec_given_init(const float* theta, int64_t B, int64_t B_pad, float* tspec, float* fv,
                    int64_t* fi, int kprime, int* ovf, hipStream_t st,
                    const float* lead_s = nullptr, int64_t ld_lead = 0, int lead = 0,
                    uint64_t* cand = nullptr, int64_t ld_cand = 0, int slots = 0,
                    uint8_t* counts = nullptr, int64_t ld_counts = 0);
int spec_threshold(const float* vals, int64_t ld, int64_t B, int64_t B_pad, int k,
                   const float* eps, const float* thr_spec, float* thr, int* ovf, int mode,
                   hipStream_t st);

// ---- prep.hip --------------------------------------------------------------------------------
int row_norms(const void* x, int dtype, int64_t n, int32_t d, int64_t ld, double* gnorm,
              float* inv32, hipStream_t st);
int screen_image(const void* x, int dtype, int64_t n, int32_t d, int64_t ld, const double* gnorm,
                 int normalize, int img_dtype, void* img, int32_t ld_img, hipStream_t st,
                 unsigned int* err_max = nullptr);
int query_dense(const void* q, int dtype, int64_t B, int32_t d, int64_t ldq, double* q64,
                hipStream_t st);
int query_liked_sum(const void* cat, int dtype, int32_t d, int64_t ld, const double* gnorm,
                    int64_t B, const int64_t* off, const int64_t* rows, double* q64,
                    hipStream_t st, int64_t row_offset = 0, int64_t n_local = 0);
// the weighted sum sum_l w_l x_l / g_l (wts parallel to rows), and q64[b] *= 1 / sum_l |w_l|
int query_liked_wsum(const void* cat, int dtype, int32_t d, int64_t ld, const double* gnorm,
                     int64_t B, const int64_t* off, const int64_t* rows, const double* wts,
                     double* q64, hipStream_t st, int64_t row_offset = 0, int64_t n_local = 0);
int scale_by_abs_weight_sum(double* q64, int64_t B, int32_t d, const int64_t* off,
                            const double* wts, hipStream_t st);
int scale_rows_f64(double* q64, int64_t B, int32_t d, const double* scale, hipStream_t st);
int query_image(const double* q64, int64_t B, int64_t B_pad, int32_t d, int img_dtype,
                const void* q_native, int64_t ldq, int native_q, float u_cat, void* qimg,
                int32_t ld_img, float* qscale, float* eps, hipStream_t st);
int query_prep(const void* q, int dtype, int64_t B, int64_t B_pad, int32_t d, int64_t ldq,
               int img_dtype, int native_q, float u_cat, double* q64, void* qimg, int32_t ld_img,
               float* qscale, float* eps, hipStream_t st);
int mask_excluded(float* s, int64_t ld, int64_t B, int64_t c0, int64_t c1, const int64_t* off,
                  const int64_t* rows, hipStream_t st);

// ---- allow_mask.hip --------------------------------------------------------------------------
int check_allow(const ebt_allow* a, int64_t row_end, const char* who);
int mask_allowed(float* s, int64_t ld, int64_t B, int64_t c0, int64_t c1, const ebt_allow* a,
                 hipStream_t st);

// ---- rescore.hip -----------------------------------------------------------------------------
int rescore(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
            const double* gnorm, int64_t row_offset, const float* cand_vals,
            const int64_t* cand_rows, int32_t kprime, int32_t k, int64_t n_rows, const float* eps,
            const double* t_floor, double* out_s, int64_t* out_r, int32_t* certified,
            hipStream_t st, const int* ovf_cnt, int ovf_cap, unsigned long long* gathered,
            int64_t list_base = 0, const float* theta = nullptr, const int64_t* excl_off = nullptr,
            const int64_t* excl_rows = nullptr, const ShardPackOut* pack = nullptr);
int merge_topk(const double* scores, const int64_t* rows, int32_t R, int64_t B, int32_t k,
               double* out_s, int64_t* out_r, hipStream_t st);
int shard_pack_lens(const double* scores, const int64_t* rows, int64_t B, int32_t k, int64_t cap,
                    void* send, hipStream_t st);
int screen_exact(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
                 const double* gnorm, int64_t n_rows, float* S, int64_t ld_s, hipStream_t st);
int export_list(int64_t* rows, int64_t B, int32_t kprime, int64_t row_offset, const int* ovf,
                const float* eps, int32_t* ovf_out, float* eps_out, hipStream_t st);
int rescore_owned(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
                  const double* gnorm, int64_t row_offset, int64_t n_local, const float* cand_vals,
                  const int64_t* cand_rows, int32_t kprime, int32_t k, const float* eps,
                  double* exact, hipStream_t st);
int finalize_topk(const float* cand_vals, const int64_t* cand_rows, const double* exact, int64_t B,
                  int32_t kprime, int32_t k, int64_t n_rows, const float* eps, const int32_t* ovf,
                  double* out_s, int64_t* out_r, int32_t* certified, hipStream_t st);
int union_floor(const float* gathered, int32_t R, int64_t B, int32_t ld, int32_t k,
                double* t_floor, hipStream_t stream, uint32_t* zero2);

// ---- large_k.hip -----------------------------------------------------------------------------
size_t large_topk_bytes(int64_t B, int64_t n, int64_t* Bg_out);
int large_topk(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
               const double* gnorm, int64_t n, int64_t row_offset, const int64_t* excl_off,
               const int64_t* excl_rows, int32_t k, double* out_s, int64_t* out_r, void* ws,
               size_t ws_bytes, hipStream_t st);

}  // namespace ebt
