// Every ebt:: function that one .hip file of libebert defines and another calls, declared once,
// and the operand records those functions take. Included after common.h by the defining file and
// by every calling file, so that a changed signature fails to compile instead of failing when the
// library is loaded. Default arguments live here only, and a declaration has at most one: what is
// optional beyond that is a named record whose empty value ({}) switches it off.
//
// Linkage rule of csrc/ (the .hip files are linked into one library):
//   * A type or function used by one .hip file only is file-local: in an anonymous namespace, or
//     `static` for a function.
//   * Exception: a type named in a __global__ signature (EpiArgs, QpArgs, LeadArgs, UpdArgs,
//     MoveArgs, GatherArgs, ExclArgs, DenseSrc, PackedSrc) or used in device code keeps its name
//     and linkage, so that kernel symbols do not change; its name is unique in the library.
//   * A type shared by two files is defined in exactly one header (common.h, here, driver.h) under
//     a name that no .hip file defines. Here: the operand records QueryOps, CatOps, ExclCsr,
//     LikedCsr, HitSlots, LeadIn, GatheredSamples, PipeArgs, WaveMergeOpts, CandList,
//     RescoreExtras and the unfused path's ChunkPlan -- host-only aggregates, filled by name at
//     the one place where positional arguments come in -- and StageScope, the timed stage of
//     every file: its constructor and destructor are api.hip's, where the timer behind its
//     handle (Timer) stays file-local, as do KernelStage and WsLayout.
//   * A function with external linkage is declared in common.h, here, or in driver.h.
#pragma once

#include "common.h"

namespace ebt {

// ---- operand records -------------------------------------------------------------------------
// The prepared queries (the ebt_query_* outputs)
struct QueryOps {
  const double* q64;
  const void* qimg;
  const float *qscale, *eps;
  int64_t B, B_pad;
};
// A (shard of a) catalog, in the order of the C entries' arguments
struct CatOps {
  const void* cat; int dtype; int64_t ld; const double* gnorm64;          // rows, float64 norms
  const void* cimg; const float* cscale; int img_dtype; int32_t ld_img;   // 16-bit image, scales
  int64_t n_rows; int32_t d, d_pad; int64_t row_offset;
};
inline CatOps cat_ops(const ebt_catalog& c) {
  return {c.data, c.dtype, c.ld, c.gnorm64, c.image, c.cscale, c.img_dtype, c.ld_img, c.n, c.d,
          c.d_pad, c.row_offset};
}
// Per-query excluded rows as a CSR (both null: none)
struct ExclCsr { const int64_t *off, *rows; };
// Per-query liked rows as a CSR, w parallel to rows (null: the unweighted sum)
struct LikedCsr { const int64_t *off, *rows; const double* w; };
// The filter GEMM's per-group hit slots: group g of query b holds counts[b * ld_counts + g] hits
// at cand[b * ld_cand + g * slots ...]; from_group: the same slots seen from group g on
struct HitSlots {
  uint64_t* cand; int64_t ld_cand; int slots;
  uint8_t* counts; int64_t ld_counts;
};
inline HitSlots from_group(HitSlots h, int64_t g) {
  return {h.cand + g * h.slots, h.ld_cand, h.slots, h.counts + g, h.ld_counts};
}
// A sample lead: the stored scores [B_pad][ld] of the catalog's first `tiles` 256-row tiles
struct LeadIn { const float* scores; int64_t ld, tiles; };
// The all-gathered sample maxima of a row-sharded catalog, read in place: [R][B][gj], ranks
// rstride floats apart (gj = 0: a plain [B][ld] row per query)
struct GatheredSamples { int gj; int64_t rstride; };

// One run of the prepared pipeline: the operands plus what its entry switches on
struct PipeArgs {
  QueryOps q;
  CatOps c;
  ExclCsr excl;
  int32_t k, kprime; int64_t chunk_rows; int flags;
  // ebt_cosine_screen_at: the caller's per-query threshold [B] and expected hits per query
  const float* theta = nullptr; double hits = 0.0;
  // ebt_cosine_screen_at_lead: the caller's lead, its scores stored by ebt_cosine_sample_lead
  LeadIn lead = {};
  // screen_at_local: instead of theta, the threshold as the gs_j-th of the all-gathered sample
  // maxima (gs_G per query), taken by the launch that starts the list and takes the lead's hits
  const float* gsamp = nullptr; GatheredSamples gs = {}; int gs_G = 0, gs_j = 0;
  // screen_at_local: the row-sharded step's floor entries ([B][floor_w + 1], ebt_floor_pack's
  // layout) written by the screen's last wave merge
  float* floor_out = nullptr; int floor_w = 0;
  // ebt_cosine_topk_prepared_allowed: the per-query allow masks (unfused and float64 screens
  // only: the entry sets EBT_FLAG_NO_FUSE), null = unfiltered
  const ebt_allow* allow = nullptr;
};

// What the wave merge does on top of merging, each group off when its first pointer is null: the
// VERIFY of theta_spec on the final list; the row-sharded step's floor entries [B][width + 1];
// the next segment's threshold [B_pad] = max(in, the k-th - 2 eps)
struct WaveMergeOpts {
  struct { const float *theta_spec, *eps; } verify;
  struct { float* out; int width; const float* eps; } floor;
  struct { float* out; const float *in, *eps; int64_t B_pad; } raise;
};

// A candidate list per query: [B][kprime] approx scores and rows; the rescore reads list row r as
// local row r - list_base (0: a list of LOCAL rows; the shard's row_offset: of GLOBAL rows)
struct CandList { const float* vals; const int64_t* rows; int32_t kprime; int64_t list_base; };
// What a rescore takes beyond the list, each null = off: the fused screen's overflow flags, the
// caller's threshold, the exclusion CSR (order check), the pack count, the timer's row counters
struct RescoreExtras {
  const int* ovf; const float* theta; ExclCsr excl;
  const ShardPackOut* pack; unsigned long long* gathered;
};

// The unfused path's plan for a run of catalog rows: `n_chunks` chunks of `chunk` rows, each
// scored into a [B_pad][ld_s] block and selected from in `segs` segments per query
struct ChunkPlan {
  int64_t chunk, ld_s, n_chunks;
  int segs;
};

// A timed stage: what is enqueued on `stream` during the scope's life is one record of `stage` in
// the timer (ebt_timer_create's handle; null, or a stage outside its mask: nothing is recorded).
// Scopes nest and repeat freely, and every way out of the block closes the stage.
struct StageScope {
  void* t;
  int stage;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  StageScope(void* timer, int s, hipStream_t stream);
  ~StageScope();
  StageScope(const StageScope&) = delete;
  StageScope& operator=(const StageScope&) = delete;
};

// ---- api.hip ---------------------------------------------------------------------------------
ChunkPlan chunk_plan(int64_t B, int64_t rows, int64_t chunk_rows);
// rows [c0, c0 + nc) of a.c scored into S (pitch ld_s) under the GEMM stage, then a.excl and
// a.allow applied under one MASK stage (opened only if one of them is set)
int score_chunk(const PipeArgs& a, int64_t c0, int64_t nc, float* S, int64_t ld_s, void* timer,
                hipStream_t st);
int fill_exact_eps(float* xeps, int64_t B, hipStream_t st);
int64_t shard_lead_room(int64_t B_pad, int64_t n_rows, int64_t sample_tiles);
int64_t shard_lead_tiles(int64_t B_pad, int64_t n_rows, int64_t sample_tiles);
// x.gathered is taken from the timer
int rescore_sharded(const double* q64, int64_t B, const CatOps& c, const CandList& l, int32_t k,
                    const float* eps, const double* t_floor, double* out_s, int64_t* out_r,
                    int32_t* certified, RescoreExtras x, void* timer, hipStream_t st);
// ebt_cosine_topk_prepared (a.allow == null) / ebt_cosine_topk_prepared_allowed
int topk_prepared(const PipeArgs& a, void* workspace, size_t ws_bytes, double* out_scores,
                  int64_t* out_rows, int32_t* certified, void* timer, hipStream_t st);
// ebt_cosine_screen
int screen_export(const PipeArgs& a, void* workspace, size_t ws_bytes, float* list_vals,
                  int64_t* list_rows, int32_t* ovf_out, float* eps_out, void* timer,
                  hipStream_t st);
// the screen at the threshold taken from a.gsamp (flags = EBT_FLAG_THETA, whatever a.flags says)
int screen_at_local(const PipeArgs& a, void* workspace, size_t ws_bytes, float* list_vals,
                    int64_t* list_rows, const float** theta_dev, const int** ovf_dev,
                    const float** eps_dev, void* timer, hipStream_t st);

// ---- screen_gemm.hip -------------------------------------------------------------------------
int64_t gemm_cus();
int screen_gemm(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows, int32_t d_pad,
                int32_t ld_img, int img_dtype, const float* qscale, const float* cscale,
                float* scores, int64_t ld_scores, hipStream_t stream, int64_t cstride = 0);
int screen_gemm_pool(const void* qimg, int64_t B_pad, const void* cimg, int64_t n_rows,
                     int32_t d_pad, int32_t ld_img, int img_dtype, const float* qscale,
                     const float* cscale, int64_t cstride, float* pooled, int64_t ld_pooled,
                     hipStream_t stream, int64_t lead, float* lead_scores, int64_t ld_lead);
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
int merge_segment(float* fv, int64_t* fi, int64_t B, int kprime, const HitSlots& h,
                  int64_t n_groups, int64_t row_offset, const ExclCsr& excl, int* ovf,
                  hipStream_t st, double expect_hits = 0.0);
bool merge_wave_fits(int kprime);
int merge_block_capacity(int kprime);
int64_t merge_block_max_groups(int kprime);
int64_t merge_wave_max_groups();
int merge_wave_capacity();
int merge_segment_wave(float* fv, int64_t* fi, int64_t B, int kprime, int k, const HitSlots& h,
                       int64_t n_groups, int64_t row_offset, const ExclCsr& excl, int* ovf,
                       hipStream_t st, const WaveMergeOpts& o = {});
int pilot_topk(const float* S, int64_t ld_s, int64_t B, int n, int64_t idx_base, int kprime, int k,
               float* fv, int64_t* fi, hipStream_t st);
int kth_threshold(const float* vals, int64_t ld, int64_t B, int64_t B_pad, int k, const float* eps,
                  float* thr, hipStream_t st);
// thr[b] = the j-th largest of query b's G pooled maxima; with fv the launch also starts the
// empty list fv/fi (k' entries, ovf 0), and with lead.tiles > 0 takes the lead's hits at the
// threshold into h's first groups
int pool_kth(const float* pool, int64_t ld, int64_t B, int64_t B_pad, int G, int j, float* thr,
             float* fv, int64_t* fi, int kprime, int* ovf, const LeadIn& lead, const HitSlots& h,
             const GatheredSamples& gs, hipStream_t st);
int spec_given_init(const float* theta, int64_t B, int64_t B_pad, float* tspec, float* fv,
                    int64_t* fi, int kprime, int* ovf, const LeadIn& lead, const HitSlots& h,
                    hipStream_t st);
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
// q64[b] = sum_l x_l / g_l over l's rows that lie in the shard (n_local > 0: rows outside
// [c.row_offset, c.row_offset + n_local) are skipped), or with l.w sum_l w_l x_l / g_l. Of c:
// cat, dtype, ld, gnorm64, d, row_offset. It checks these operands itself (null pointers, d,
// ld, dtype 0..3; with l.w also l.rows) and reports them as "ebt_query_liked_sum: bad arguments",
// or "ebt_query_liked_wsum: ..." with l.w: the drivers' valid_catalog does not test dtype
int query_liked_sum(const CatOps& c, const LikedCsr& l, int64_t B, double* q64, hipStream_t st,
                    int64_t n_local);
// q64[b] *= 1 / L_b from the CSR's offsets, and q64[b] *= 1 / sum_l |w_l|
int scale_by_count(double* q64, int64_t B, int32_t d, const int64_t* off, hipStream_t st);
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
// (of c: the rows, their norms, n_rows, d and row_offset; the screening image is not read)
int rescore(const double* q64, int64_t B, const CatOps& c, const CandList& l, int32_t k,
            const float* eps, const double* t_floor, double* out_s, int64_t* out_r,
            int32_t* certified, const RescoreExtras& x, hipStream_t st);
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

// ---- shard_exchange.hip ----------------------------------------------------------------------
int merge_topk(const double* scores, const int64_t* rows, int32_t R, int64_t B, int32_t k,
               double* out_s, int64_t* out_r, hipStream_t st);
int shard_pack_lens(const double* scores, const int64_t* rows, int64_t B, int32_t k, int64_t cap,
                    void* send, hipStream_t st);
int union_floor(const float* gathered, int32_t R, int64_t B, int32_t ld, int32_t k,
                double* t_floor, hipStream_t stream, uint32_t* zero2);

// ---- large_k.hip -----------------------------------------------------------------------------
size_t large_topk_bytes(int64_t B, int64_t n, int64_t* Bg_out);
int large_topk(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
               const double* gnorm, int64_t n, int64_t row_offset, const int64_t* excl_off,
               const int64_t* excl_rows, int32_t k, double* out_s, int64_t* out_r, void* ws,
               size_t ws_bytes, hipStream_t st);

}  // namespace ebt
