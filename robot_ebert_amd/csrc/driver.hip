// The self-contained C-ABI path (include/ebert.h: ebt_catalog_init, ebt_workspace_bytes,
// ebt_cosine_topk{,_submit,_finish}): what a caller without Python binds in place of
// /root/reference/src/backend/app/lib.py:51-55 (and the resident catalog of constants.py:55-56).
//
// One batch = query prep (ebt_query_prep / ebt_query_liked_sum + ebt_query_image) -> the
// prepared-query pipeline (ebt_cosine_topk_prepared: screen + exact float64 rescore +
// certificate) -> on the host, after ONE wait for this batch's certificates, the retries:
//   certified -1 (a fused candidate list overflowed, or the speculative threshold was wrong)
//                -> the query again with EBT_FLAG_NO_FUSE at the same k';
//   certified  0 (more than k' rows inside the screen's error band) -> k' x 4 up to 4096, then
//                the float64 screen (EBT_FLAG_EXACT); still 0 there is an error (more than
//                4096 rows tied at f32 resolution), never a silent approximation;
//   certified -2 (a corrupt candidate row) -> error.
// Retried queries are gathered into groups of at most RETRY_GROUP (their prepared rows, their
// exclusion segments), run through the same pipeline and scattered back. Everything lives in
// the caller's workspace; the library allocates no device memory.
// The catalog lifecycle entries are in catalog_update.hip, the row-sharded entries in sharded.hip;
// what the three files share is declared in driver.h and defined here.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "driver.h"

namespace ebt {

namespace {

constexpr int64_t KPRIME_MAX = 4096;
constexpr int64_t QUERY_PREP_MAX_D = 4096;
constexpr int64_t SCORE_BUDGET = 4LL << 30;   // f32 score bytes of the unfused path per pass
constexpr int64_t RETRY_GROUP = 256;          // queries per retry pass
constexpr int64_t RETRY_BUDGET = 256LL << 20; // f32 score bytes of a retry pass
constexpr int64_t RETRY_EXCL_MAX = 1LL << 20; // gathered exclusion rows per retry pass

// search.py's clamp of k': [round_up(k, 4), min(round_up(n, 4), 4096)]
int32_t clamp_kprime(int64_t kp, int64_t k_eff, int64_t n) {
  const int64_t lo = round_up(k_eff, 4), hi = round_up(n, 4);
  kp = round_up(kp, 4);
  kp = kp < hi ? kp : hi;
  kp = kp < KPRIME_MAX ? kp : KPRIME_MAX;
  return (int32_t)(kp > lo ? kp : lo);
}

int64_t chunk_rows(const ebt_catalog& c, int64_t B_pad, int64_t budget) {
  int64_t rows = budget / (4 * B_pad);
  rows = rows / 128 * 128;
  rows = rows < 128 ? 128 : rows;
  const int64_t cap = round_up(c.n, 128);
  return rows < cap ? rows : cap;
}

PrepLayout prep_layout(const ebt_catalog& c, int64_t rows) {
  const int64_t rp = pad_batch(rows);
  PrepLayout p{};
  size_t o = 0;
  p.q64 = carve(o, (size_t)rows * c.d * 8);
  p.qimg = carve(o, (size_t)rp * c.ld_img * 2);
  p.qscale = carve(o, (size_t)rp * 4);
  p.eps = carve(o, (size_t)rp * 4);
  p.bytes = o;
  return p;
}

}  // namespace

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// The caller's certificate buffer, seen from the device when it is pinned host memory
// (hipHostMalloc / hipHostRegister, e.g. a torch pin_memory tensor): the rescore then stores each
// query's certificate straight into it -- one 4-byte store per query across the host link, no
// copy launch behind the kernels (a D2H copy is a blit kernel here: ~4 us plus its boundary, 2 %
// of a C2 batch). Anything else (pageable memory) -> nullptr: the workspace's certificates and
// one hipMemcpyAsync, as before. EBT_HOST_DIRECT=0 keeps the copy (A/B).
int32_t* host_mapped(int32_t* host) {
  static const bool on = [] {
    const char* v = getenv("EBT_HOST_DIRECT");
    return !(v && v[0] == '0');
  }();
  void* dp = nullptr;
  if (!on || !host) return nullptr;
  if (hipHostGetDevicePointer(&dp, host, 0) != hipSuccess || !dp) {
    (void)hipGetLastError();  // (pageable memory: clear the query's error for later checks)
    return nullptr;
  }
  return (int32_t*)dp;
}

int64_t pad_batch(int64_t B) {
  B = B < 1 ? 1 : B;
  return B <= 128 ? round_up(B, 128) : round_up(B, 256);
}

// search.py default_kprime: the rows inside the 2 eps band around the k-th score grow with k;
// native images have the smaller band
int64_t default_kprime_raw(bool native, int64_t k) {
  return round_up(native ? k + (k / 4 > 16 ? k / 4 : 16) : (2 * k > k + 32 ? 2 * k : k + 32), 8);
}

bool valid_catalog(const ebt_catalog* c) {
  return c && c->data && c->gnorm64 && c->image && c->n > 0 && c->d > 0 && c->ld >= c->d &&
         c->d_pad % 64 == 0 && c->d_pad >= c->d && c->ld_img >= c->d_pad;
}

bool driver_layout(const ebt_catalog& c, int64_t B, int32_t k, const ebt_options& opt,
                   DriverLayout* L) {
  if (B < 1 || k < 1 || c.n < 1 || opt.kprime < 0 || opt.chunk_rows < 0 ||
      (opt.chunk_rows && opt.chunk_rows % 128) ||
      (opt.flags & ~(EBT_FLAG_NO_FUSE | EBT_FLAG_LIKED_CHECKED)))
    return false;
  DriverLayout& D = *L;
  D = DriverLayout{};
  D.B = B;
  D.B_pad = pad_batch(B);
  D.k_eff = (int32_t)(k < c.n ? k : c.n);
  D.flags = opt.flags & EBT_FLAG_NO_FUSE;  // (LIKED_CHECKED: the submit's, not the screen's)
  D.prep = prep_layout(c, B);
  if (D.k_eff > KPRIME_MAX) {  // beyond the screen's k' range: every score, a full sort
    const size_t big = large_topk_bytes(B, c.n, nullptr);
    if (big == 0) return false;
    D.large = true;
    size_t o = 0;
    D.off_prep = carve(o, D.prep.bytes);
    D.big_bytes = big > (size_t)B * 8 ? big : (size_t)B * 8;  // also the liked path's scratch
    D.off_big = carve(o, D.big_bytes);
    D.off_cert = carve(o, (size_t)(B + 1) * 4);
    D.bytes = o;
    return true;
  }
  D.kprime = clamp_kprime(opt.kprime ? opt.kprime : default_kprime_raw(c.native, D.k_eff),
                          D.k_eff, c.n);
  D.chunk = opt.chunk_rows ? opt.chunk_rows : chunk_rows(c, D.B_pad, SCORE_BUDGET);
  D.R = B < RETRY_GROUP ? B : RETRY_GROUP;
  const int64_t R_pad = pad_batch(D.R);
  D.chunk_r = opt.chunk_rows ? opt.chunk_rows : chunk_rows(c, R_pad, RETRY_BUDGET);
  size_t pass = ebt_cosine_topk_workspace(B, D.B_pad, c.n, D.kprime, D.chunk, D.flags);
  if (pass == 0) return false;
  // every retry configuration: k' from the first pass up to 4096 (x 4 steps), fused or not,
  // and the float64 screen from the default k' up
  const int64_t kcap = round_up(c.n, 4) < KPRIME_MAX ? round_up(c.n, 4) : KPRIME_MAX;
  const int fl[3] = {D.flags, EBT_FLAG_NO_FUSE, EBT_FLAG_EXACT};
  for (int f = 0; f < 3; ++f) {
    for (int64_t kp = D.kprime;; kp = kp * 4 < kcap ? kp * 4 : kcap) {
      const size_t w = ebt_cosine_topk_workspace(D.R, R_pad, c.n, (int32_t)kp, D.chunk_r, fl[f]);
      if (w == 0) return false;
      pass = w > pass ? w : pass;
      if (kp >= kcap) break;
    }
  }
  D.prep_r = prep_layout(c, D.R);
  const size_t res = D.k_eff < k ? (size_t)B * D.k_eff * 8 : 0;  // padded results only
  size_t o = 0;
  D.off_prep = carve(o, D.prep.bytes);
  D.pass_bytes = pass;
  D.off_pass = carve(o, pass);
  D.off_res_s = carve(o, res);
  D.off_res_r = carve(o, res);
  D.off_cert = carve(o, (size_t)(B + 1) * 4);
  D.off_rprep = carve(o, D.prep_r.bytes);
  D.off_rs = carve(o, (size_t)D.R * D.k_eff * 8);
  D.off_rr = carve(o, (size_t)D.R * D.k_eff * 8);
  D.off_rcert = carve(o, (size_t)D.R * 4);
  D.off_idx = carve(o, (size_t)D.R * 8);
  D.off_roff = carve(o, (size_t)(D.R + 1) * 8);
  D.off_rrows = carve(o, (size_t)RETRY_EXCL_MAX * 8);
  // (ebt_cosine_topk_allowed_finish: the retried queries' mask ids, int32)
  D.off_rmask = carve(o, (size_t)D.R * 4);
  D.bytes = o;
  return true;
}

int prep_dense(const ebt_catalog& c, const void* q, int q_dtype, int64_t B, int64_t ldq,
               const PrepLayout& P, char* base, hipStream_t st) {
  double* q64 = (double*)(base + P.q64);
  void* qimg = base + P.qimg;
  float* qscale = (float*)(base + P.qscale);
  float* eps = (float*)(base + P.eps);
  const int64_t B_pad = pad_batch(B);
  const int native_q = c.native && q_dtype == c.img_dtype;
  if (c.d <= QUERY_PREP_MAX_D)
    return ebt_query_prep(q, q_dtype, B, B_pad, c.d, ldq, c.img_dtype, native_q, c.u_cat, q64,
                          qimg, c.ld_img, qscale, eps, st);
  int rc = ebt_query_dense(q, q_dtype, B, c.d, ldq, q64, st);
  if (rc) return rc;
  return ebt_query_image(q64, B, B_pad, c.d, c.img_dtype, native_q ? q : nullptr,
                         native_q ? ldq : 0, native_q, c.u_cat, qimg, c.ld_img, qscale, eps, st);
}

// The host checks of a liked batch: every query likes at least one row (sklearn's message) and
// every liked row is in [row_lo, row_hi); (*scale)[b] = 1 / L_b. One stream sync.
// With weights w (device float64, parallel to rows): every weight finite and W_b = sum_l |w_l|
// (sequential, CSR order: scale_by_abs_weight_sum_kernel's sum) > 0; (*scale)[b] = 1 / W_b.
int liked_scales(const int64_t* off, const int64_t* rows, int64_t B, int32_t d, int64_t row_lo,
                 int64_t row_hi, std::vector<double>* scale, hipStream_t st, const double* w) {
  std::vector<int64_t> h_off(B + 1);
  int rc = hip_check(hipMemcpyAsync(h_off.data(), off, (B + 1) * 8, hipMemcpyDeviceToHost, st),
                     "hipMemcpyAsync");
  if (!rc) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rc) return rc;
  scale->resize(B);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t cnt = h_off[b + 1] - h_off[b];
    if (cnt <= 0) {
      set_error("Found array with 0 sample(s) (shape=(0, %d)) while a minimum of 1 is required "
                "by check_pairwise_arrays.", d);
      return EBT_EINVAL;
    }
    (*scale)[b] = 1.0 / (double)cnt;
  }
  const int64_t nnz = h_off[B] - h_off[0];
  if (nnz > 0) {
    std::vector<int64_t> h_rows(nnz);
    rc = hip_check(hipMemcpy(h_rows.data(), rows + h_off[0], nnz * 8, hipMemcpyDeviceToHost),
                   "hipMemcpy");
    if (rc) return rc;
    for (int64_t r : h_rows)
      if (r < row_lo || r >= row_hi) {
        set_error("liked row %lld is not in the catalog rows [%lld, %lld)", (long long)r,
                  (long long)row_lo, (long long)row_hi);
        return EBT_EINVAL;
      }
  }
  if (w) {
    std::vector<double> h_w(nnz);
    rc = hip_check(hipMemcpy(h_w.data(), w + h_off[0], nnz * 8, hipMemcpyDeviceToHost),
                   "hipMemcpy");
    if (rc) return rc;
    for (int64_t b = 0; b < B; ++b) {
      double W = 0.0;
      for (int64_t l = h_off[b] - h_off[0]; l < h_off[b + 1] - h_off[0]; ++l) {
        if (!std::isfinite(h_w[l])) {
          set_error("liked weight %lld of query %lld is not finite", (long long)(l + h_off[0]),
                    (long long)b);
          return EBT_EINVAL;
        }
        W += std::fabs(h_w[l]);
      }
      if (!(W > 0.0) || !std::isfinite(W)) {
        set_error("the liked weights of query %lld sum to |w| = %g (a finite sum > 0 is "
                  "required)", (long long)b, W);
        return EBT_EINVAL;
      }
      (*scale)[b] = 1.0 / W;
    }
  }
  return EBT_OK;
}

// A liked batch, for both drivers (driver.h): checks and scales, the sum, the caller's step, the
// scale, the image. Validated on the host (counts >= 1 with sklearn's message, rows in
// [b.row_lo, b.row_hi)) unless the caller did (b.checked): then nothing is read back and the
// scale comes from the CSR on the device. l.w != NULL: the weighted sum and 1 / W_b in place of
// the sum and 1 / L_b (l.w == NULL launches what it always did)
int prep_liked(const ebt_catalog& c, const LikedCsr& l, int64_t B, const PrepLayout& P, char* base,
               const LikedBatch& b, hipStream_t st,
               const std::function<int(double* q64)>& reduce) {
  double* q64 = (double*)(base + P.q64);
  int rc = EBT_OK;
  if (!b.checked) {
    std::vector<double> scale;
    rc = liked_scales(l.off, l.rows, B, c.d, b.row_lo, b.row_hi, &scale, st, l.w);
    if (rc) return rc;
    if (b.scale_bytes < (size_t)B * 8) {
      set_error("ebt_cosine_topk: workspace too small for the liked-query scales");
      return EBT_ENOMEM;
    }
    rc = hip_check(hipMemcpy(b.d_scale, scale.data(), B * 8, hipMemcpyHostToDevice), "hipMemcpy");
    if (rc) return rc;
  }
  rc = query_liked_sum(cat_ops(c), l, B, q64, st, b.n_local);
  if (!rc && reduce) rc = reduce(q64);
  if (rc) return rc;
  if (b.checked && l.w) rc = scale_by_abs_weight_sum(q64, B, c.d, l.off, l.w, st);
  else if (b.checked) rc = scale_by_count(q64, B, c.d, l.off, st);
  else rc = ebt_scale_rows_f64(q64, B, c.d, b.d_scale, st);
  if (rc) return rc;
  return ebt_query_image(q64, B, pad_batch(B), c.d, c.img_dtype, nullptr, 0, 0, c.u_cat,
                         base + P.qimg, c.ld_img, (float*)(base + P.qscale),
                         (float*)(base + P.eps), st);
}

// ---- the tail of a submit (driver.h) ------------------------------------------------------------
int record_event(hipStream_t st, hipEvent_t* ev) {
  *ev = event_get(st);
  if (!*ev) return hip_check(hipErrorOutOfMemory, "hipEventCreate");
  const int rc = hip_check(hipEventRecord(*ev, st), "hipEventRecord");
  if (rc) {
    event_put(*ev, st);
    *ev = nullptr;
  }
  return rc;
}

int deliver_certs(const int32_t* cert, int32_t* cert_host, int64_t count, const int32_t* direct,
                  hipStream_t st, hipEvent_t* ev) {
  if (!direct) {
    const int rc = hip_check(hipMemcpyAsync(cert_host, cert, (size_t)count * 4,
                                            hipMemcpyDeviceToHost, st),
                             "hipMemcpyAsync");
    if (rc) return rc;
  }
  return record_event(st, ev);
}

void fill_pending(ebt_pending* p, const ebt_catalog* cat, const ebt_options& opt, int64_t B,
                  int32_t k, const DriverLayout& L, const int64_t* excl_off,
                  const int64_t* excl_rows, char* ws, size_t ws_bytes, double* out_scores,
                  int64_t* out_rows, int32_t* cert_host, hipEvent_t ev, void* timer,
                  void* stream) {
  // (ebt_pending's fields in their order: an ABI struct; its `flags` stays 0)
  *p = ebt_pending{cat, opt, B, L.B_pad, L.chunk, k, L.k_eff, L.kprime, 0, excl_off, excl_rows,
                   ws, ws_bytes, out_scores, out_rows, cert_host, ev, timer, stream};
}

namespace {

// ------------------------------------------------------------------------------ kernels ----
// dst row i <- src row idx[i] (gather) or dst row idx[i] <- src row i (scatter), 4-byte words
__global__ void move_rows_kernel(const uint32_t* __restrict__ src, int64_t src_ld,
                                 uint32_t* __restrict__ dst, int64_t dst_ld,
                                 const int64_t* __restrict__ idx, int64_t n, int64_t words,
                                 int scatter) {
  const int64_t total = n * words;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / words, w = t - i * words;
    if (scatter) dst[idx[i] * dst_ld + w] = src[i * src_ld + w];
    else dst[i * dst_ld + w] = src[idx[i] * src_ld + w];
  }
}

int move_rows(const void* src, int64_t src_ld_bytes, void* dst, int64_t dst_ld_bytes,
              const int64_t* idx, int64_t n, int64_t row_bytes, bool scatter, hipStream_t st) {
  if (n == 0) return EBT_OK;
  const int64_t words = row_bytes / 4, total = n * words;
  int64_t blocks = (total + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(move_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                     (const uint32_t*)src, src_ld_bytes / 4, (uint32_t*)dst, dst_ld_bytes / 4,
                     idx, n, words, scatter ? 1 : 0);
  return launch_check("move_rows_kernel");
}

// the exclusion segments of the retried queries, gathered (new offsets computed on the host)
__global__ void csr_gather_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ rows,
                                  const int64_t* __restrict__ idx,
                                  const int64_t* __restrict__ new_off, int64_t* __restrict__ out) {
  const int64_t i = blockIdx.x;
  const int64_t s = off[idx[i]], n = new_off[i + 1] - new_off[i];
  for (int64_t t = threadIdx.x; t < n; t += blockDim.x) out[new_off[i] + t] = rows[s + t];
}

// out[b][j] = j < k_eff ? res[b][j] : NaN / -1
__global__ void pad_results_kernel(const double* __restrict__ rs, const int64_t* __restrict__ rr,
                                   int64_t B, int k_eff, int k, double* __restrict__ os,
                                   int64_t* __restrict__ orow) {
  const int64_t total = B * k;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / k, j = t - b * k;
    os[t] = j < k_eff ? rs[b * k_eff + j] : __builtin_nan("");
    orow[t] = j < k_eff ? rr[b * k_eff + j] : -1;
  }
}

// flag[0] = 1 when some exclusion segment is not sorted ascending (the fused merge drops
// excluded rows by binary search); one block per query
__global__ void csr_sorted_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ rows,
                                  int32_t* __restrict__ flag) {
  const int64_t b = blockIdx.x;
  const int64_t s = off[b], e = off[b + 1];
  bool bad = e < s;
  for (int64_t t = s + threadIdx.x; t + 1 < e; t += blockDim.x) bad |= rows[t] > rows[t + 1];
  if (bad) flag[0] = 1;
}

int run_prepared(const ebt_catalog& c, const PrepLayout& P, char* base, int64_t B,
                 const int64_t* excl_off, const int64_t* excl_rows, int32_t k_eff, int32_t kp,
                 int64_t chunk, int flags, char* pass, size_t pass_bytes, double* out_s,
                 int64_t* out_r, int32_t* cert, void* timer, hipStream_t st,
                 const ebt_allow* allow) {
  QueryOps q{(const double*)(base + P.q64), nullptr, nullptr, nullptr, B, pad_batch(B)};
  if (!(flags & EBT_FLAG_EXACT)) {  // (the float64 screen takes no image of the queries)
    q.qimg = base + P.qimg;
    q.qscale = (const float*)(base + P.qscale);
    q.eps = (const float*)(base + P.eps);
  }
  PipeArgs a{q, cat_ops(c), {excl_off, excl_rows}, k_eff, kp, chunk, flags};
  a.allow = allow;
  return topk_prepared(a, pass, pass_bytes, out_s, out_r, cert, timer, st);
}

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

size_t ebt_workspace_bytes(const ebt_catalog* cat, int64_t B, int32_t k, const ebt_options* opt) {
  if (!valid_catalog(cat)) return 0;
  DriverLayout L;
  if (!driver_layout(*cat, B, k, opt ? *opt : ebt_options{}, &L)) return 0;
  return L.bytes;
}

// ebt_cosine_topk_submit (allow = NULL) and ebt_cosine_topk_allowed_submit: with per-query allow
// masks the batch runs unfused (EBT_FLAG_NO_FUSE set here, and kept in the pending batch).
// ebt_cosine_topk_weighted_submit is the same entry with per-row weights on the liked rows
// (liked_w == NULL: exactly the unweighted batch); only the query prep sees them.
int ebt_cosine_topk_weighted_submit(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                                    int64_t ldq, const int64_t* liked_off,
                                    const int64_t* liked_rows, int32_t k, const int64_t* excl_off,
                                    const int64_t* excl_rows, const ebt_options* opt,
                                    void* workspace, size_t ws_bytes, double* out_scores,
                                    int64_t* out_rows, int32_t* cert_host, ebt_pending* p,
                                    void* timer, void* stream, const ebt_allow* allow,
                                    const double* liked_w) {
  hipStream_t st = (hipStream_t)stream;
  if (liked_w && q) {
    set_error("ebt_cosine_topk_weighted: liked_w weighs liked rows; dense queries (q) take none");
    return EBT_EINVAL;
  }
  if (!valid_catalog(cat) || !p || !workspace || !out_scores || !out_rows || !cert_host ||
      B < 1 || k < 1 || ((q == nullptr) == (liked_off == nullptr)) ||
      (liked_off && !liked_rows) || ((excl_off == nullptr) != (excl_rows == nullptr)) ||
      (q && (q_dtype < 0 || q_dtype > 3 || ldq < cat->d))) {
    set_error("ebt_cosine_topk: bad arguments (B=%lld k=%d; pass exactly one of q / liked)",
              (long long)B, k);
    return EBT_EINVAL;
  }
  ebt_options o = opt ? *opt : ebt_options{};
  if (allow) {
    if (cat->row_offset < 0) {
      set_error("ebt_cosine_topk_allowed: catalog row_offset < 0");
      return EBT_EINVAL;
    }
    const int rca = check_allow(allow, cat->row_offset + cat->n, "ebt_cosine_topk_allowed");
    if (rca) return rca;
    o.flags |= EBT_FLAG_NO_FUSE;
  }
  DriverLayout L;
  if (!driver_layout(*cat, B, k, o, &L)) {
    set_error("ebt_cosine_topk: unsupported sizes or options (B=%lld k=%d n=%lld: n < 2^31; "
              "chunk_rows % 128 == 0; flags EBT_FLAG_NO_FUSE only)",
              (long long)B, k, (long long)cat->n);
    return EBT_EINVAL;
  }
  if (ws_bytes < L.bytes) {
    set_error("ebt_cosine_topk: workspace %zu < %zu bytes (ebt_workspace_bytes)", ws_bytes,
              L.bytes);
    return EBT_ENOMEM;
  }
  if (allow && L.large) {
    set_error("ebt_cosine_topk_allowed: min(k, n) = %d > 4096 takes the full-sort path, which "
              "has no allow masks", L.k_eff);
    return EBT_EUNSUPPORTED;
  }
  char* ws = (char*)workspace;
  char* prep = ws + L.off_prep;
  const LikedBatch liked_batch{cat->row_offset, cat->row_offset + cat->n, 0,
                               (o.flags & EBT_FLAG_LIKED_CHECKED) != 0,
                               (double*)(ws + (L.large ? L.off_big : L.off_pass)),
                               L.large ? L.big_bytes : L.pass_bytes};
  int rc = q ? prep_dense(*cat, q, q_dtype, B, ldq, L.prep, prep, st)
             : prep_liked(*cat, {liked_off, liked_rows, liked_w}, B, L.prep, prep, liked_batch, st);
  if (rc) return rc;
  int32_t* cert = (int32_t*)(ws + L.off_cert);
  // the full-sort path fills its certificates by a memset and adds the exclusion flag: copied
  int32_t* direct = L.large ? nullptr : host_mapped(cert_host);
  if (direct) {
    for (int64_t b = 0; b < B; ++b) cert_host[b] = CERT_UNSET;
    cert = direct;
  }
  if (L.large) {  // exact: every certificate is 1, the results are final
    rc = large_topk((const double*)(prep + L.prep.q64), B, cat->d, cat->data, cat->dtype,
                    cat->ld, cat->gnorm64, cat->n, cat->row_offset, excl_off, excl_rows, k,
                    out_scores, out_rows, ws + L.off_big, L.big_bytes, st);
    if (!rc) rc = hip_check(hipMemsetD32Async((hipDeviceptr_t)cert, 1, (size_t)B, st),
                            "hipMemsetD32Async");
  } else {
    const bool padded = L.k_eff < k;
    double* rs = padded ? (double*)(ws + L.off_res_s) : out_scores;
    int64_t* rr = padded ? (int64_t*)(ws + L.off_res_r) : out_rows;
    rc = run_prepared(*cat, L.prep, prep, B, excl_off, excl_rows, L.k_eff, L.kprime, L.chunk,
                      L.flags, ws + L.off_pass, L.pass_bytes, rs, rr, cert, timer, st, allow);
  }
  if (rc) return rc;
  // the exclusion check: the rescore's certificate -3 (ebt_cosine_topk_prepared); the full-sort
  // path has no rescore, so its flag sits right after the certificates, one copy bringing both
  // (otherwise the flag is neither set nor read)
  if (excl_off && L.large) {
    rc = hip_check(hipMemsetAsync(cert + B, 0, 4, st), "hipMemsetAsync");
    if (rc) return rc;
    hipLaunchKernelGGL(csr_sorted_kernel, dim3((unsigned)B), dim3(256), 0, st, excl_off,
                       excl_rows, cert + B);
    rc = launch_check("csr_sorted_kernel");
    if (rc) return rc;
  }
  hipEvent_t ev = nullptr;
  rc = deliver_certs(cert, cert_host, B + (excl_off && L.large), direct, st, &ev);
  if (rc) return rc;
  fill_pending(p, cat, o, B, k, L, excl_off, excl_rows, ws, ws_bytes, out_scores, out_rows,
               cert_host, ev, timer, stream);
  return EBT_OK;
}

int ebt_cosine_topk_allowed_submit(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                                   int64_t ldq, const int64_t* liked_off,
                                   const int64_t* liked_rows, int32_t k, const int64_t* excl_off,
                                   const int64_t* excl_rows, const ebt_options* opt,
                                   void* workspace, size_t ws_bytes, double* out_scores,
                                   int64_t* out_rows, int32_t* cert_host, ebt_pending* p,
                                   void* timer, void* stream, const ebt_allow* allow) {
  return ebt_cosine_topk_weighted_submit(cat, q, q_dtype, B, ldq, liked_off, liked_rows, k,
                                         excl_off, excl_rows, opt, workspace, ws_bytes,
                                         out_scores, out_rows, cert_host, p, timer, stream, allow,
                                         nullptr);
}

int ebt_cosine_topk_submit(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                           int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows,
                           int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                           const ebt_options* opt, void* workspace, size_t ws_bytes,
                           double* out_scores, int64_t* out_rows, int32_t* cert_host,
                           ebt_pending* p, void* timer, void* stream) {
  return ebt_cosine_topk_allowed_submit(cat, q, q_dtype, B, ldq, liked_off, liked_rows, k,
                                        excl_off, excl_rows, opt, workspace, ws_bytes, out_scores,
                                        out_rows, cert_host, p, timer, stream, nullptr);
}

// ebt_cosine_topk_finish (allow = NULL) and ebt_cosine_topk_allowed_finish: a retried group's
// mask ids are gathered through d_idx like its prepared rows, and the retry runs with an
// ebt_allow pointing at them
int ebt_cosine_topk_allowed_finish(ebt_pending* p, const ebt_allow* allow) {
  if (!p || !p->event || !p->cat) {
    set_error("ebt_cosine_topk_finish: not a submitted batch");
    return EBT_EINVAL;
  }
  if (allow) {
    const int rca = check_allow(allow, p->cat->row_offset + p->cat->n,
                                "ebt_cosine_topk_allowed_finish");
    if (rca) return rca;
  }
  hipStream_t st = (hipStream_t)p->stream;
  const ebt_catalog& c = *p->cat;
  hipEvent_t ev = (hipEvent_t)p->event;
  int rc = hip_check(hipEventSynchronize(ev), "hipEventSynchronize");
  event_put(ev, st);
  p->event = nullptr;
  if (rc) return rc;
  const int64_t B = p->B;
  DriverLayout L;
  if (!driver_layout(c, B, p->k, p->opt, &L)) {
    set_error("ebt_cosine_topk_finish: bad pending batch");
    return EBT_EINVAL;
  }
  const bool unsorted_excl = p->excl_off && (L.large ? p->cert_host[B] != 0 : [&] {
    for (int64_t b = 0; b < B; ++b)
      if (p->cert_host[b] == -3) return true;
    return false;
  }());
  for (int64_t b = 0; b < B; ++b)
    if (p->cert_host[b] < -3 || p->cert_host[b] > 1) {
      set_error("ebt_cosine_topk_finish: query %lld's certificate %d was not delivered",
                (long long)b, p->cert_host[b]);
      return EBT_EHIP;
    }
  if (unsorted_excl) {
    set_error("ebt_cosine_topk: exclusion rows must be sorted ascending within each query");
    return EBT_EINVAL;
  }
  if (L.large) return EBT_OK;  // the full-sort path is exact: nothing to retry or pad
  char* ws = p->ws;
  const bool padded = L.k_eff < p->k;
  double* rs = padded ? (double*)(ws + L.off_res_s) : p->out_scores;
  int64_t* rr = padded ? (int64_t*)(ws + L.off_res_r) : p->out_rows;
  const int32_t kcap = (int32_t)(round_up(c.n, 4) < KPRIME_MAX ? round_up(c.n, 4) : KPRIME_MAX);
  // per-query retry state
  std::vector<int32_t> cert(p->cert_host, p->cert_host + B);
  std::vector<int32_t> kp(B, L.kprime), fl(B, L.flags);
  std::vector<int64_t> h_off;
  char* prep = ws + L.off_prep;
  char* rprep = ws + L.off_rprep;
  int64_t* d_idx = (int64_t*)(ws + L.off_idx);
  int64_t* d_roff = (int64_t*)(ws + L.off_roff);
  int64_t* d_rrows = (int64_t*)(ws + L.off_rrows);
  double* r_s = (double*)(ws + L.off_rs);
  int64_t* r_r = (int64_t*)(ws + L.off_rr);
  int32_t* r_c = (int32_t*)(ws + L.off_rcert);
  int32_t* d_rmask = (int32_t*)(ws + L.off_rmask);
  ebt_allow r_allow{};
  if (allow) {
    r_allow = *allow;
    r_allow.mask_id = d_rmask;
  }
  const int64_t qrow = (int64_t)c.d * 8, irow = (int64_t)c.ld_img * 2;
  for (int round = 0;; ++round) {
    // next configuration of every query that needs one
    std::vector<int64_t> todo;
    for (int64_t b = 0; b < B; ++b) {
      if (cert[b] == 1) continue;
      if (cert[b] == -2 || cert[b] < -2 || cert[b] > 1) {
        set_error("internal error: candidate row out of range (certificate %d)", cert[b]);
        return EBT_EHIP;
      }
      if (cert[b] == -1) {
        fl[b] |= EBT_FLAG_NO_FUSE;
      } else if (kp[b] < kcap) {
        kp[b] = kp[b] * 4 < kcap ? kp[b] * 4 : kcap;
      } else if (!(fl[b] & EBT_FLAG_EXACT)) {
        fl[b] = EBT_FLAG_EXACT;
        kp[b] = L.kprime;
      } else {
        set_error("query %lld could not be certified at k'=%d (more than k' rows tie with the "
                  "k-th score at f32 precision)", (long long)b, kp[b]);
        return EBT_EUNSUPPORTED;
      }
      todo.push_back(b);
    }
    if (todo.empty()) break;
    if (round > 64) {
      set_error("ebt_cosine_topk: retries did not converge");
      return EBT_EHIP;
    }
    if (p->excl_off && h_off.empty()) {
      h_off.resize(B + 1);
      rc = hip_check(hipMemcpy(h_off.data(), p->excl_off, (B + 1) * 8, hipMemcpyDeviceToHost),
                     "hipMemcpy");
      if (rc) return rc;
    }
    // groups of equal (k', flags), at most R queries and RETRY_EXCL_MAX exclusion rows each
    std::vector<char> done(todo.size(), 0);
    for (size_t s = 0; s < todo.size(); ++s) {
      if (done[s]) continue;
      const int32_t gkp = kp[todo[s]], gfl = fl[todo[s]];
      std::vector<int64_t> grp;
      std::vector<int64_t> goff(1, 0);
      bool solo = false;  // one query whose own segment exceeds the gather buffer
      for (size_t u = s; u < todo.size() && (int64_t)grp.size() < L.R; ++u) {
        const int64_t b = todo[u];
        if (done[u] || kp[b] != gkp || fl[b] != gfl) continue;
        const int64_t len = p->excl_off ? h_off[b + 1] - h_off[b] : 0;
        if (len > RETRY_EXCL_MAX) {
          if (!grp.empty()) continue;
          solo = true;
        } else if (goff.back() + len > RETRY_EXCL_MAX) {
          continue;
        }
        grp.push_back(b);
        goff.push_back(goff.back() + len);
        done[u] = 1;
        if (solo) break;
      }
      const int64_t m = (int64_t)grp.size(), m_pad = pad_batch(m);
      rc = hip_check(hipMemcpy(d_idx, grp.data(), m * 8, hipMemcpyHostToDevice), "hipMemcpy");
      if (rc) return rc;
      // the group's prepared queries (padding rows: zero image, scale 1, eps 0)
      const PrepLayout& RP = L.prep_r;
      rc = hip_check(hipMemsetAsync(rprep + RP.qimg, 0, (size_t)m_pad * irow, st), "memset");
      if (!rc) rc = hip_check(hipMemsetAsync(rprep + RP.eps, 0, (size_t)m_pad * 4, st), "memset");
      if (!rc)  // qscale = 1.0f (bits 0x3f800000), as ebt_query_image leaves padding rows
        rc = hip_check(hipMemsetD32Async((hipDeviceptr_t)(rprep + RP.qscale), 0x3f800000,
                                         (size_t)m_pad, st),
                       "memsetD32");
      if (!rc) rc = move_rows(prep + L.prep.q64, qrow, rprep + RP.q64, qrow, d_idx, m, qrow,
                              false, st);
      if (!rc) rc = move_rows(prep + L.prep.qimg, irow, rprep + RP.qimg, irow, d_idx, m, irow,
                              false, st);
      if (!rc) rc = move_rows(prep + L.prep.qscale, 4, rprep + RP.qscale, 4, d_idx, m, 4, false,
                              st);
      if (!rc) rc = move_rows(prep + L.prep.eps, 4, rprep + RP.eps, 4, d_idx, m, 4, false, st);
      if (!rc && allow) rc = move_rows(allow->mask_id, 4, d_rmask, 4, d_idx, m, 4, false, st);
      if (rc) return rc;
      const int64_t* eo = nullptr;
      const int64_t* er = nullptr;
      if (p->excl_off) {
        if (solo) {  // the segment in place: offsets {off[b], off[b+1]} into the caller's rows
          rc = hip_check(hipMemcpy(d_roff, p->excl_off + grp[0], 16, hipMemcpyDeviceToDevice),
                         "hipMemcpy");
          if (rc) return rc;
          eo = d_roff;
          er = p->excl_rows;
        } else {
          rc = hip_check(hipMemcpy(d_roff, goff.data(), (m + 1) * 8, hipMemcpyHostToDevice),
                         "hipMemcpy");
          if (rc) return rc;
          hipLaunchKernelGGL(csr_gather_kernel, dim3((unsigned)m), dim3(256), 0, st, p->excl_off,
                             p->excl_rows, d_idx, d_roff, d_rrows);
          rc = launch_check("csr_gather_kernel");
          if (rc) return rc;
          eo = d_roff;
          er = d_rrows;
        }
      }
      rc = run_prepared(c, RP, rprep, m, eo, er, L.k_eff, gkp, L.chunk_r, gfl, ws + L.off_pass,
                        L.pass_bytes, r_s, r_r, r_c, p->timer, st, allow ? &r_allow : nullptr);
      if (!rc) rc = move_rows(r_s, (int64_t)L.k_eff * 8, rs, (int64_t)L.k_eff * 8, d_idx, m,
                              (int64_t)L.k_eff * 8, true, st);
      if (!rc) rc = move_rows(r_r, (int64_t)L.k_eff * 8, rr, (int64_t)L.k_eff * 8, d_idx, m,
                              (int64_t)L.k_eff * 8, true, st);
      if (rc) return rc;
      std::vector<int32_t> gc(m);
      rc = hip_check(hipMemcpyAsync(gc.data(), r_c, m * 4, hipMemcpyDeviceToHost, st),
                     "hipMemcpyAsync");
      if (!rc) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
      if (rc) return rc;
      for (int64_t i = 0; i < m; ++i) cert[grp[i]] = gc[i];
    }
  }
  if (padded) {
    const int64_t total = B * p->k;
    int64_t blocks = (total + 255) / 256;
    blocks = blocks > 4096 ? 4096 : blocks;
    hipLaunchKernelGGL(pad_results_kernel, dim3((unsigned)blocks), dim3(256), 0, st, rs, rr, B,
                       L.k_eff, p->k, p->out_scores, p->out_rows);
    rc = launch_check("pad_results_kernel");
    if (rc) return rc;
  }
  return EBT_OK;
}

int ebt_cosine_topk_finish(ebt_pending* p) { return ebt_cosine_topk_allowed_finish(p, nullptr); }

int ebt_cosine_topk_weighted(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                             int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows,
                             int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                             const ebt_options* opt, void* workspace, size_t ws_bytes,
                             double* out_scores, int64_t* out_rows, void* timer, void* stream,
                             const ebt_allow* allow, const double* liked_w) {
  std::vector<int32_t> cert((size_t)(B > 0 ? B : 0) + 1);
  ebt_pending p{};
  int rc = ebt_cosine_topk_weighted_submit(cat, q, q_dtype, B, ldq, liked_off, liked_rows, k,
                                           excl_off, excl_rows, opt, workspace, ws_bytes,
                                           out_scores, out_rows, cert.data(), &p, timer, stream,
                                           allow, liked_w);
  if (rc) return rc;
  rc = ebt_cosine_topk_allowed_finish(&p, allow);
  if (!rc) rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
  return rc;
}

int ebt_cosine_topk_allowed(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B,
                            int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows,
                            int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                            const ebt_options* opt, void* workspace, size_t ws_bytes,
                            double* out_scores, int64_t* out_rows, void* timer, void* stream,
                            const ebt_allow* allow) {
  return ebt_cosine_topk_weighted(cat, q, q_dtype, B, ldq, liked_off, liked_rows, k, excl_off,
                                  excl_rows, opt, workspace, ws_bytes, out_scores, out_rows,
                                  timer, stream, allow, nullptr);
}

int ebt_cosine_topk(const ebt_catalog* cat, const void* q, int q_dtype, int64_t B, int64_t ldq,
                    const int64_t* liked_off, const int64_t* liked_rows, int32_t k,
                    const int64_t* excl_off, const int64_t* excl_rows, const ebt_options* opt,
                    void* workspace, size_t ws_bytes, double* out_scores, int64_t* out_rows,
                    void* timer, void* stream) {
  return ebt_cosine_topk_allowed(cat, q, q_dtype, B, ldq, liked_off, liked_rows, k, excl_off,
                                 excl_rows, opt, workspace, ws_bytes, out_scores, out_rows,
                                 timer, stream, nullptr);
}

}  // extern "C"
