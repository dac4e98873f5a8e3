// What the three files of the self-contained C-ABI path share: driver.hip (the single-GPU
// entries), sharded.hip (the row-sharded entries) and catalog_update.hip (the catalog
// lifecycle). Under internal.h's linkage rule: the types here are defined here only, and every
// function is declared here and defined once, in driver.hip.
#pragma once

#include <functional>

#include "common.h"
#include "internal.h"

namespace ebt {

// written by the host into a directly delivered certificate buffer before the kernels run: a
// value that is still there when the batch's event has passed was never delivered (the finish
// fails loudly instead of reading a previous batch's leftovers as certificates)
constexpr int32_t CERT_UNSET = 0x7fffffff;

int64_t round_up(int64_t v, int64_t m);
int64_t pad_batch(int64_t B);
bool valid_catalog(const ebt_catalog* c);
// the caller's certificate buffer seen from the device when it is pinned host memory, else NULL
int32_t* host_mapped(int32_t* host);
// search.py default_kprime before its clamp to the catalog (rounded up to 8)
int64_t default_kprime_raw(bool native, int64_t k);

// Per-batch prepared queries (the ebt_query_* outputs) for `rows` queries.
struct PrepLayout {
  size_t q64, qimg, qscale, eps, bytes;
};

// The whole workspace of one batch:
//   [prep B] [pass: max(first pass, every retry pass)] [results k_eff < k] [cert B + flag]
//   [retry: prep R, results R x k_eff, cert R, gather indices, exclusion CSR of the group,
//    allow-mask ids of the group]
// large: min(k, n) > 4096, the full-sort path (large_k.hip): [prep B] [sort buffers] [cert B + flag]
struct DriverLayout {
  int64_t B, B_pad, R, chunk, chunk_r;
  int32_t k_eff, kprime, flags;
  bool large;
  PrepLayout prep, prep_r;
  size_t off_prep, off_pass, pass_bytes, off_res_s, off_res_r, off_cert, off_rprep, off_rs,
      off_rr, off_rcert, off_idx, off_roff, off_rrows, off_rmask, off_big, big_bytes, bytes;
};

bool driver_layout(const ebt_catalog& c, int64_t B, int32_t k, const ebt_options& opt,
                   DriverLayout* L);
int prep_dense(const ebt_catalog& c, const void* q, int q_dtype, int64_t B, int64_t ldq,
               const PrepLayout& P, char* base, hipStream_t st);
// the host checks of a liked batch (rows in [row_lo, row_hi)); (*scale)[b] = 1 / L_b, or with
// weights w (device, parallel to rows; checked finite, sum_l |w_l| > 0) 1 / sum_l |w_l|
int liked_scales(const int64_t* off, const int64_t* rows, int64_t B, int32_t d, int64_t row_lo,
                 int64_t row_hi, std::vector<double>* scale, hipStream_t st,
                 const double* w = nullptr);
// What a driver says of a liked batch: the rows a list may name, [row_lo, row_hi), and the
// shard's own row count (n_local, as query_liked_sum's; 0: a whole catalog); whether the caller
// vouches for the lists (EBT_FLAG_LIKED_CHECKED); the device room for the B float64 scales
struct LikedBatch {
  int64_t row_lo, row_hi, n_local;
  bool checked;
  double* d_scale; size_t scale_bytes;
};
// One liked batch of either driver, in order: liked_scales and the upload of its scales, unless
// b.checked; the sum of the shard's rows; `reduce` on the sums, if given (the sharded driver's
// all-reduce); the scale, by the uploaded scales or with b.checked from the CSR on the device;
// the image
int prep_liked(const ebt_catalog& c, const LikedCsr& l, int64_t B, const PrepLayout& P, char* base,
               const LikedBatch& b, hipStream_t st,
               const std::function<int(double* q64)>& reduce = {});

// ---- the tail of a submit ----------------------------------------------------------------------
// *ev = an event of the pool, recorded on st (returned to the pool on failure)
int record_event(hipStream_t st, hipEvent_t* ev);
// `count` certificates to the caller's host buffer by one copy, unless the kernels stored them
// there (direct != NULL); then the batch's event
int deliver_certs(const int32_t* cert, int32_t* cert_host, int64_t count, const int32_t* direct,
                  hipStream_t st, hipEvent_t* ev);
void fill_pending(ebt_pending* p, const ebt_catalog* cat, const ebt_options& opt, int64_t B,
                  int32_t k, const DriverLayout& L, const int64_t* excl_off,
                  const int64_t* excl_rows, char* ws, size_t ws_bytes, double* out_scores,
                  int64_t* out_rows, int32_t* cert_host, hipEvent_t ev, void* timer, void* stream);

}  // namespace ebt
