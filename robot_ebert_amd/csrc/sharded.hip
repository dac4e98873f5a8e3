// The row-sharded self-contained entry, split from driver.hip (which keeps the single-GPU path).
// ebt_cosine_topk_sharded (include/ebert.h): distributed.py's per-shard protocol
// (score_topk_sharded_local_stages) in C++ over a caller-supplied all-gather. Reference:
// /root/reference/src/backend/app/lib.py:51-55 restated on every shard; the merge of the shards'
// exact top-k is the only thing the reference (one CPU process) has no counterpart for.
#include <cmath>
#include <vector>

#include "common.h"
#include "driver.h"

namespace ebt {
namespace {

constexpr int SH_MERGE_WAVE_KMAX = 512;          // search.py MERGE_WAVE_KMAX
#ifndef EBT_SH_SHARED_MAX
#define EBT_SH_SHARED_MAX 300000  // (build knob for A/B; round 5: 200000 -> 300000, C3/4 -1.6 %)
#endif
constexpr int64_t SH_SHARED_MAX_SHARD_ROWS = EBT_SH_SHARED_MAX;  // distributed.py SHARED_MAX_SHARD_ROWS
constexpr int64_t SH_SAMPLE_TILES_MAX = 64;
constexpr int SH_K_MAX = 4096;                   // ebt_merge_topk

// search.py spec_rank: the smallest j with P(Poisson(lam) >= j) <= 1e-6
int sh_spec_rank(double lam) {
  double pmf = exp(-lam), cdf = 0.0;
  int j = 0;
  while (j < 100000 && 1.0 - cdf > 1e-6) {
    cdf += pmf;
    pmf *= lam / (j + 1);
    ++j;
  }
  return j > 1 ? j : 1;
}

// distributed.py shared_sample_tiles: 256-row sample tiles per shard for the catalog-wide
// screening threshold (0 = every shard screens at its own); depends only on (n_global, world,
// B_pad), so every rank decides alike
int64_t sh_tiles(int64_t n_global, int world, int64_t B_pad) {
  const int64_t shard = ceil_div(n_global, world);
  if (world < 2 || B_pad % 256 != 0 || shard > SH_SHARED_MAX_SHARD_ROWS) return 0;
  const int64_t full = shard / 256;
  int64_t cap = ceil_div(SH_SAMPLE_TILES_MAX, world);
  cap = cap > 4 ? cap : 4;
  int64_t P = SH_SAMPLE_TILES_MAX < full / 24 ? SH_SAMPLE_TILES_MAX : full / 24;
  P = P < cap ? P : cap;
  const int64_t per = 256 / (B_pad / 256) > 1 ? 256 / (B_pad / 256) : 1;
  if (P / per * per >= 8) P = P / per * per;
  // a sample GEMM of less than one round of the persistent grid takes a round's time anyway:
  // fill it (C3 on 8 ranks: 8 -> 16 tiles per shard, room for the lead)
  // (only while the fill stays within the sample's caps: at B_pad = 512 a round is 128 tiles,
  // and 8 ranks x 4 x 128 maxima would exceed ebt_pool_kth's 2048 -- distributed.py alike)
  if (P < per && per <= full / 6 && per <= SH_SAMPLE_TILES_MAX && world * 4 * per <= 2048)
    P = per;
  return (P >= 1 && world * P >= 8) ? P : 0;
}

struct ShardLayout {
  DriverLayout D;
  int64_t tiles, G, RG, J, GJ;  // sample maxima per shard (G), sent per shard (J + 1 of them)
  int64_t lead, ld_lead;        // this shard's sample lead (its first tiles' scores kept)
  size_t screen_bytes;
  int64_t fw, cap;  // floor gather width per shard and query; packed results per rank (0: full)
  size_t pack_bytes;
  size_t off_spass, off_pool, off_gsamp, off_lv, off_lr, off_ovf,
      off_eps, off_fsend, off_frecv, off_tfloor, off_ls, off_lrr, off_gs, off_gr, off_scale,
      off_qrecv, off_psend, off_precv, off_incomplete, off_lead, bytes;
};

bool shard_layout(const ebt_catalog& c, const ebt_comm& cm, int64_t B, int32_t k,
                  const ebt_options& opt, ShardLayout* S) {
  if (k < 1 || k > SH_K_MAX || cm.world < 1 || cm.rank < 0 || cm.rank >= cm.world ||
      cm.n_global < c.row_offset + c.n || !cm.all_gather)
    return false;
  ShardLayout& L = *S;
  L = ShardLayout{};
  if (!driver_layout(c, B, k, opt, &L.D) || L.D.large) return false;
  const DriverLayout& D = L.D;
  const int64_t R = cm.world, kp = D.kprime;
  // the shared threshold only serves the wave-merge screen (k' <= 512); decided from
  // rank-invariant sizes (k against the WHOLE catalog), since its all-gather is a collective
  const int64_t kg = k < cm.n_global ? k : cm.n_global;
  const int64_t kpg = opt.kprime ? round_up(opt.kprime, 4) : default_kprime_raw(c.native, kg);
  L.tiles = (opt.flags & EBT_FLAG_NO_FUSE) || kpg > SH_MERGE_WAVE_KMAX
                ? 0
                : sh_tiles(cm.n_global, cm.world, D.B_pad);
  L.G = 4 * L.tiles;
  L.RG = R * L.G;
  if (L.RG > 2048) L.tiles = L.G = L.RG = 0;  // ebt_pool_kth's limit (sh_tiles keeps within it)
  // theta = the j-th largest of all R G maxima, j <= J (J from the catalog-wide k', rank-
  // invariant, >= every rank's own j): the j-th of the union of each shard's J largest is the
  // same value, so each shard sends its J largest (+ a -inf column: ebt_floor_pack's layout)
  L.J = L.GJ = 0;
  if (L.tiles) {
    const double m_total = 256.0 * (double)L.tiles * R;
    L.J = sh_spec_rank((double)kpg * m_total / (double)cm.n_global);
    if (L.J > L.RG / 2) L.tiles = L.G = L.RG = L.J = 0;  // the sample would decide nothing
    L.J = L.J < L.G ? L.J : L.G;
    L.GJ = L.J + 1;
  }
  size_t scr = ebt_cosine_topk_workspace(B, D.B_pad, c.n, D.kprime, D.chunk, D.flags);
  if (L.tiles) {
    const size_t t = ebt_cosine_topk_workspace(B, D.B_pad, c.n, D.kprime, D.chunk, EBT_FLAG_THETA);
    scr = t > scr ? t : scr;
  }
  if (scr == 0) return false;
  L.screen_bytes = scr;
  size_t o = align_up(D.bytes);
  L.off_spass = D.off_pass;
  // the first pass's screen needs more than the retries' region
  if (scr > D.pass_bytes) L.off_spass = carve(o, scr);
  L.off_pool = carve(o, (size_t)D.B_pad * L.G * 4);
  // the lead: only where the shared threshold drives the screen (ebt_cosine_screen_at_lead)
  L.lead = L.ld_lead = 0;
  if (L.tiles && D.flags == 0 && D.kprime <= SH_MERGE_WAVE_KMAX) {
    const int64_t own = L.tiles < c.n / 256 ? L.tiles : c.n / 256;
    // (the room regardless of ebt_spec_lead: offsets never depend on the knob)
    L.lead = own == L.tiles ? shard_lead_tiles(D.B_pad, c.n, own) : 0;
    L.ld_lead = own == L.tiles ? 256 * shard_lead_room(D.B_pad, c.n, own) : 0;
  }
  L.off_lead = carve(o, (size_t)D.B_pad * L.ld_lead * 4);
  // this shard's J largest, then every shard's
  L.off_gsamp = carve(o, (size_t)B * L.GJ * 4 * (R + 1));
  L.off_lv = carve(o, (size_t)B * kp * 4);
  L.off_lr = carve(o, (size_t)B * kp * 8);
  L.off_ovf = carve(o, (size_t)B * 4);
  L.off_eps = carve(o, (size_t)B * 4);
  // the compact exchange (shard_exchange.hip): each shard's w best approx for the floor, its entries
  // above the floor for the results (int32 rows behind per-query starts)
  L.fw = ebt_shard_list_width(k, (int32_t)R);
  L.cap = ebt_shard_pack_cap(B, k, (int32_t)R, cm.n_global);
  if (!L.cap) L.fw = k;
  L.pack_bytes = L.cap ? ebt_shard_pack_bytes(B, L.cap) : 0;
  L.off_fsend = carve(o, (size_t)B * (L.fw + 1) * 4);
  L.off_frecv = carve(o, (size_t)R * B * (L.fw + 1) * 4);
  L.off_tfloor = carve(o, (size_t)B * 8);
  L.off_ls = carve(o, (size_t)B * k * 8);
  L.off_lrr = carve(o, (size_t)B * k * 8);
  L.off_gs = carve(o, (size_t)R * B * k * 8);
  L.off_gr = carve(o, (size_t)R * B * k * 8);
  L.off_scale = carve(o, (size_t)B * 8);
  // the liked path's gathered sums (none with the caller's all-reduce)
  L.off_qrecv = carve(o, cm.all_reduce_f64 ? 0 : (size_t)R * B * c.d * 8);
  L.off_psend = carve(o, L.pack_bytes);
  L.off_precv = carve(o, (size_t)R * L.pack_bytes);
  // the merge's int32 "incomplete" flag, then a reserved u32 (nothing reads or writes it after
  // union_floor has zeroed both)
  L.off_incomplete = carve(o, 8);
  L.bytes = o;
  return true;
}

// out[t] = sum over ranks r (in rank order) of in[r * total + t]: the all-reduce of the liked
// queries' partial sums, identical on every rank
__global__ void sum_ranks_kernel(const double* __restrict__ in, int R, int64_t total,
                                 double* __restrict__ out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += in[(int64_t)r * total + t];
    out[t] = s;
  }
}

unsigned grid_for(int64_t total) {
  int64_t b = ceil_div(total, 256);
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

int sh_gather(const ebt_comm& cm, const void* send, void* recv, size_t bytes, void* timer,
              hipStream_t st) {
  int rc;
  {
    StageScope s(timer, EBT_STAGE_COLLECTIVE, st);
    rc = cm.all_gather(cm.ctx, send, recv, bytes, (void*)st);
  }
  if (rc) {
    set_error("ebt_cosine_topk_sharded: the caller's all_gather returned %d", rc);
    return EBT_EHIP;
  }
  return EBT_OK;
}

// liked rows of a row-sharded catalog: GLOBAL rows, each shard sums its own, the partial sums
// are all-gathered and added in rank order (or all-reduced by the caller), then / L_b
// (lib.py:51-52). With weights (the same global list on every rank): each shard's weighted sum
// of its own rows, then / W_b, which every rank computes from the full list. This is
// prep_liked's step between the sum and the scale
int reduce_liked_sums(const ebt_catalog& c, const ebt_comm& cm, int64_t B, double* q64,
                      double* qrecv, void* timer, hipStream_t st) {
  if (cm.all_reduce_f64) {  // the caller's all-reduce (RCCL: about 2 / R of the gather's bytes)
    int e;
    {
      StageScope s(timer, EBT_STAGE_COLLECTIVE, st);
      e = cm.all_reduce_f64(cm.ctx, q64, (size_t)B * c.d, (void*)st);
    }
    if (e) {
      set_error("ebt_cosine_topk_sharded: the caller's all_reduce_f64 returned %d", e);
      return EBT_EHIP;
    }
    return EBT_OK;
  }
  const int rc = sh_gather(cm, q64, qrecv, (size_t)B * c.d * 8, timer, st);
  if (rc) return rc;
  hipLaunchKernelGGL(sum_ranks_kernel, dim3(grid_for(B * c.d)), dim3(256), 0, st, qrecv,
                     (int)cm.world, B * c.d, q64);
  return launch_check("sum_ranks_kernel");
}

// the full exchange: every shard's [B][k] exact list (f64 scores, i64 rows), ebt_merge_topk
int sh_full_merge(const ShardLayout& S, const ebt_comm& cm, char* ws, int64_t B, int32_t k,
                  double* out_s, int64_t* out_r, void* timer, hipStream_t st) {
  double* ls = (double*)(ws + S.off_ls);
  int64_t* lrr = (int64_t*)(ws + S.off_lrr);
  double* gs = (double*)(ws + S.off_gs);
  int64_t* gr = (int64_t*)(ws + S.off_gr);
  int rc = sh_gather(cm, ls, gs, (size_t)B * k * 8, timer, st);
  if (!rc) rc = sh_gather(cm, lrr, gr, (size_t)B * k * 8, timer, st);
  if (rc) return rc;
  StageScope s(timer, EBT_STAGE_SHARD_MERGE, st);
  return ebt_merge_topk(gs, gr, cm.world, B, k, out_s, out_r, st);
}
}  // namespace
}  // namespace ebt

using namespace ebt;

extern "C" {

size_t ebt_sharded_workspace_bytes(const ebt_catalog* cat, const ebt_comm* comm, int64_t B,
                                   int32_t k, const ebt_options* opt) {
  if (!valid_catalog(cat) || !comm) return 0;
  ShardLayout S;
  if (!shard_layout(*cat, *comm, B, k, opt ? *opt : ebt_options{}, &S)) return 0;
  return S.bytes;
}

// ebt_cosine_topk_sharded_submit is this entry with liked_w == NULL
int ebt_cosine_topk_sharded_weighted_submit(
    const ebt_catalog* cat, const ebt_comm* comm, const void* q, int q_dtype, int64_t B,
    int64_t ldq, const int64_t* liked_off, const int64_t* liked_rows, int32_t k,
    const int64_t* excl_off, const int64_t* excl_rows, const ebt_options* opt, void* workspace,
    size_t ws_bytes, double* out_scores, int64_t* out_rows, int32_t* host,
    ebt_sharded_pending* pending, void* timer, void* stream, const double* liked_w) {
  hipStream_t st = (hipStream_t)stream;
  if (liked_w && q) {
    set_error("ebt_cosine_topk_sharded_weighted: liked_w weighs liked rows; dense queries (q) "
              "take none");
    return EBT_EINVAL;
  }
  if (!valid_catalog(cat) || !comm || !workspace || !out_scores || !out_rows || !host ||
      !pending || B < 1 || k < 1 || ((q == nullptr) == (liked_off == nullptr)) ||
      (liked_off && !liked_rows) || ((excl_off == nullptr) != (excl_rows == nullptr)) ||
      (q && (q_dtype < 0 || q_dtype > 3 || ldq < cat->d))) {
    set_error("ebt_cosine_topk_sharded: bad arguments (B=%lld k=%d; pass exactly one of q / "
              "liked)", (long long)B, k);
    return EBT_EINVAL;
  }
  const ebt_options o = opt ? *opt : ebt_options{};
  ShardLayout S;
  if (!shard_layout(*cat, *comm, B, k, o, &S)) {
    set_error("ebt_cosine_topk_sharded: unsupported sizes, options or communicator (B=%lld "
              "k=%d <= %d, n=%lld, row_offset=%lld, n_global=%lld, rank %d of %d)",
              (long long)B, k, SH_K_MAX, (long long)cat->n, (long long)cat->row_offset,
              (long long)comm->n_global, comm->rank, comm->world);
    return EBT_EINVAL;
  }
  if (ws_bytes < S.bytes) {
    set_error("ebt_cosine_topk_sharded: workspace %zu < %zu bytes "
              "(ebt_sharded_workspace_bytes)", ws_bytes, S.bytes);
    return EBT_ENOMEM;
  }
  const ebt_catalog& c = *cat;
  const ebt_comm& cm = *comm;
  const DriverLayout& L = S.D;
  const int R = cm.world;
  char* ws = (char*)workspace;
  char* prep = ws + L.off_prep;
  const double* q64 = (const double*)(prep + L.prep.q64);
  const void* qimg = prep + L.prep.qimg;
  const float* qscale = (const float*)(prep + L.prep.qscale);
  const float* qeps = (const float*)(prep + L.prep.eps);
  int rc = EBT_OK;
  // 1. the queries (lib.py:51-52): liked rows are GLOBAL, each shard sums its own, the lists are
  // always checked here, and the scales have a region of their own (B float64)
  const LikedBatch liked_batch{0, cm.n_global, c.n, false, (double*)(ws + S.off_scale),
                               (size_t)B * 8};
  {
    StageScope s(timer, EBT_STAGE_PREP, st);
    rc = q ? prep_dense(c, q, q_dtype, B, ldq, L.prep, prep, st)
           : prep_liked(c, {liked_off, liked_rows, liked_w}, B, L.prep, prep, liked_batch, st,
                        [&](double* sums) {
                          return reduce_liked_sums(c, cm, B, sums, (double*)(ws + S.off_qrecv),
                                                   timer, st);
                        });
  }
  if (rc) return rc;
  // 2. the catalog-wide screening threshold from every shard's sample maxima (taken by the
  // screen's first launch, step 3)
  bool accept = false;
  const float* recv_s = nullptr;
  int j_s = 0;
  double hits = 0.0;
  if (S.tiles) {
    float* pool = (float*)(ws + S.off_pool);
    float* gsamp = (float*)(ws + S.off_gsamp);
    const int64_t own = S.tiles < c.n / 256 ? S.tiles : c.n / 256;
    // -inf where this shard has no sample tile (a shard smaller than the sample); a full sample
    // writes every maximum itself (one API call less per step)
    if (own < S.tiles) {
      rc = hip_check(hipMemsetD32Async((hipDeviceptr_t)pool, (int)0xff800000u,
                                       (size_t)L.B_pad * S.G, st), "hipMemsetD32Async");
      if (rc) return rc;
    }
    if (own >= 1) {
      // the lead's tiles first, the rest evenly spaced over the shard after them
      int64_t stride = (c.n / 256 - S.lead) / (own - S.lead);
      if (stride > 1 && stride % 2 == 0) stride -= 1;
      rc = ebt_cosine_sample_lead(qimg, qscale, L.B_pad, c.image, c.cscale, c.img_dtype,
                                  c.ld_img, c.n, c.d_pad, own, stride, pool, S.G, S.lead,
                                  (float*)(ws + S.off_lead), S.ld_lead, timer, st);
      if (rc) return rc;
    }
    float* send = gsamp;                          // [B][J + 1]
    float* recv = gsamp + (size_t)B * S.GJ;       // [R][B][J + 1]
    {
      StageScope s(timer, EBT_STAGE_SMALL, st);
      rc = ebt_floor_pack(pool, S.G, B, (int32_t)S.G, (int32_t)S.J, nullptr, send, st);
    }
    if (!rc) rc = sh_gather(cm, send, recv, (size_t)B * S.GJ * 4, timer, st);
    if (rc) return rc;
    const double m_total = 256.0 * (double)S.tiles * R;
    const int j = sh_spec_rank((double)L.kprime * m_total / (double)cm.n_global);
    // exact for j <= J; when J was clamped to G every shard sent all of its maxima, and any
    // j <= RG / 2 is (distributed.theta_from_samples decides alike)
    if (j <= S.J || (S.J == S.G && j <= S.RG / 2)) {
      accept = true;
      recv_s = recv;
      j_s = j;
      hits = ((double)j + (double)j * j / (2.0 * (double)S.RG)) * (double)c.n / m_total;
    }
  }
  const bool use_theta = accept && L.flags == 0 && L.kprime <= SH_MERGE_WAVE_KMAX;
  const float* theta = nullptr;   // the shared threshold, where the screen wrote it
  // 3. the shard's screen: its k' best approx candidates (GLOBAL rows)
  float* lv = (float*)(ws + S.off_lv);
  int64_t* lr = (int64_t*)(ws + S.off_lr);
  int32_t* ovf = (int32_t*)(ws + S.off_ovf);
  float* eps = (float*)(ws + S.off_eps);
  // at the shared threshold the list keeps LOCAL rows and the screen's overflow flags and eps
  // are read where it wrote them (no export launch); otherwise GLOBAL rows, exported
  const int* ovf_p = ovf;
  const float* eps_p = eps;
  // (the j-th of every rank's maxima, read in the gathered [R][B][J + 1] layout, is taken by
  // the launch that starts the list and takes the lead's hits: one launch for both; and at the
  // shared threshold the screen's last wave merge also writes this shard's floor entries,
  // step 4's send buffer: no ebt_floor_pack launch)
  float* fsend = (float*)(ws + S.off_fsend);
  const CatOps co = cat_ops(c);
  const ExclCsr excl{excl_off, excl_rows};
  PipeArgs a{{q64, qimg, qscale, qeps, B, L.B_pad}, co, excl, L.k_eff, L.kprime, L.chunk, L.flags};
  if (use_theta) {
    a.hits = hits;
    a.lead = {(const float*)(ws + S.off_lead), S.ld_lead, S.lead};
    a.gsamp = recv_s;
    a.gs = {(int)S.GJ, B * S.GJ};
    a.gs_G = (int)(R * S.GJ);
    a.gs_j = j_s;
    a.floor_out = fsend;
    a.floor_w = (int)S.fw;
    rc = screen_at_local(a, ws + S.off_spass, S.screen_bytes, lv, lr, &theta, &ovf_p, &eps_p,
                         timer, st);
  } else {
    rc = screen_export(a, ws + S.off_spass, S.screen_bytes, lv, lr, ovf, eps, timer, st);
  }
  if (rc) return rc;
  // 4. the catalog-wide floor: the k-th largest (approx - eps) over every shard's fw best
  float* frecv = (float*)(ws + S.off_frecv);
  double* tfloor = (double*)(ws + S.off_tfloor);
  if (!use_theta) {
    StageScope s(timer, EBT_STAGE_SMALL, st);
    rc = ebt_floor_pack(lv, L.kprime, B, L.k_eff, (int32_t)S.fw, eps_p, fsend, st);
  }
  if (!rc) rc = sh_gather(cm, fsend, frecv, (size_t)B * (S.fw + 1) * 4, timer, st);
  if (rc) return rc;
  // (the floor's launch also zeroes the merge's "incomplete" flag and the reserved word after
  // it: no memset launch)
  uint32_t* zero2 = (uint32_t*)(ws + S.off_incomplete);
  {
    StageScope s(timer, EBT_STAGE_SMALL, st);
    rc = union_floor(frecv, R, B, (int32_t)S.fw + 1, k, tfloor, st, zero2);
  }
  if (rc) return rc;
  // 5. the rescore of the rows that can enter the global top k, the certificate
  double* ls = (double*)(ws + S.off_ls);
  int64_t* lrr = (int64_t*)(ws + S.off_lrr);
  const bool padded = L.k_eff < k;
  double* rs = padded ? (double*)(ws + L.off_res_s) : ls;
  int64_t* rr = padded ? (int64_t*)(ws + L.off_res_r) : lrr;
  int32_t* cert = (int32_t*)(ws + L.off_cert);
  int32_t* direct = host_mapped(host);  // (see the dense submit, driver.hip)
  if (direct) {
    for (int64_t b = 0; b < B; ++b) host[b] = CERT_UNSET;
    cert = direct;
  }
  // (the list's rows read as they are: local at the shared threshold, global otherwise; the
  // certificate with ebt_certify_cut's tests)
  // (the rescore also checks the exclusion segments' order -- certificate -3 -- and packs the
  // shard's entries above the floor for the results exchange: ebt_shard_pack's two launches
  // folded in; the finish packs again only for a batch whose retries changed lists)
  const ShardPackOut pack{S.cap && !padded ? (uint32_t*)(ws + S.off_psend) + B : nullptr};
  rc = rescore_sharded(q64, B, co, {lv, lr, L.kprime, use_theta ? 0 : c.row_offset}, L.k_eff,
                       eps_p, tfloor, rs, rr, cert,
                       {ovf_p, use_theta ? theta : nullptr, excl, &pack, nullptr}, timer, st);
  if (rc) return rc;
  // the certificates to the caller's host buffer (unless the rescore wrote them there); one
  // event for them
  hipEvent_t ev = nullptr;
  rc = deliver_certs(cert, host, B, direct, st, &ev);
  if (rc) return rc;
  ebt_sharded_pending P{};
  fill_pending(&P.local, cat, o, B, k, L, excl_off, excl_rows, ws, ws_bytes, ls, lrr, host, ev,
               timer, stream);
  P.comm = cm;
  P.out_scores = out_scores;
  P.out_rows = out_rows;
  P.host = host;
  P.event = nullptr;
  P.stage = 1;
  *pending = P;
  return EBT_OK;
}

int ebt_cosine_topk_sharded_submit(const ebt_catalog* cat, const ebt_comm* comm, const void* q,
                                   int q_dtype, int64_t B, int64_t ldq,
                                   const int64_t* liked_off, const int64_t* liked_rows,
                                   int32_t k, const int64_t* excl_off, const int64_t* excl_rows,
                                   const ebt_options* opt, void* workspace, size_t ws_bytes,
                                   double* out_scores, int64_t* out_rows, int32_t* host,
                                   ebt_sharded_pending* pending, void* timer, void* stream) {
  return ebt_cosine_topk_sharded_weighted_submit(cat, comm, q, q_dtype, B, ldq, liked_off,
                                                 liked_rows, k, excl_off, excl_rows, opt,
                                                 workspace, ws_bytes, out_scores, out_rows, host,
                                                 pending, timer, stream, nullptr);
}

int ebt_cosine_topk_sharded_finish(ebt_sharded_pending* p) {
  if (!p || p->stage != 1 || !p->local.cat) {
    set_error("ebt_cosine_topk_sharded_finish: not a submitted batch");
    return EBT_EINVAL;
  }
  ebt_pending& lp = p->local;
  hipStream_t st = (hipStream_t)lp.stream;
  ShardLayout S;
  if (!shard_layout(*lp.cat, p->comm, lp.B, lp.k, lp.opt, &S)) {
    set_error("ebt_cosine_topk_sharded_finish: bad pending batch");
    return EBT_EINVAL;
  }
  // the local retries (ebt_cosine_topk_finish: unfused reruns, k' x 4, the float64 screen) on
  // this shard alone: a retried query gets the shard's exact top k, which the merge accepts
  int rc = ebt_cosine_topk_finish(&lp);
  if (rc) return rc;
  p->stage = 2;
  char* ws = lp.ws;
  const int64_t B = lp.B;
  const int32_t k = lp.k;
  void* timer = lp.timer;
  p->host[B + 1] = 0;
  if (S.cap) {
    // 6. every shard's entries above the floor, packed (int32 rows), ONE all-gather, the merge.
    // The rescore counted them already (len[b] in the header; the "incomplete" flag was zeroed
    // in the submit): one launch places and copies them. Counted again (ebt_shard_pack) only when
    // retries rewrote some query's list (its first-pass certificate was not 1) or the list was
    // padded to k in the finish
    int32_t* incomplete = (int32_t*)(ws + S.off_incomplete);
    bool repack = lp.k_eff < k;
    for (int64_t b = 0; b < B && !repack; ++b) repack = lp.cert_host[b] != 1;
    {
      StageScope s(timer, EBT_STAGE_SMALL, st);
      rc = repack
               ? ebt_shard_pack((const double*)(ws + S.off_ls), (const int64_t*)(ws + S.off_lrr),
                                B, k, (const double*)(ws + S.off_tfloor), S.cap, ws + S.off_psend,
                                st)
               : shard_pack_lens((const double*)(ws + S.off_ls), (const int64_t*)(ws + S.off_lrr),
                                 B, k, S.cap, ws + S.off_psend, st);
    }
    if (!rc) rc = sh_gather(p->comm, ws + S.off_psend, ws + S.off_precv, S.pack_bytes, timer, st);
    if (rc) return rc;
    // (the flag straight into the host buffer when it is pinned: zeroed above, only ever set
    // to 1 by the merge's stores; else the workspace's flag and one copy)
    int32_t* direct = host_mapped(p->host + B + 1);
    {
      StageScope s(timer, EBT_STAGE_SHARD_MERGE, st);
      rc = ebt_merge_packed(ws + S.off_precv, p->comm.world, B, k, S.cap, p->out_scores,
                            p->out_rows, direct ? direct : incomplete, st);
    }
    if (!rc && !direct)
      rc = hip_check(hipMemcpyAsync(p->host + B + 1, incomplete, 4, hipMemcpyDeviceToHost, st),
                     "hipMemcpyAsync");
  } else {
    rc = sh_full_merge(S, p->comm, ws, B, k, p->out_scores, p->out_rows, timer, st);
  }
  if (rc) return rc;
  hipEvent_t ev = nullptr;
  rc = record_event(st, &ev);
  if (rc) return rc;
  p->event = ev;
  return EBT_OK;
}

int ebt_cosine_topk_sharded_wait(ebt_sharded_pending* p) {
  if (!p || p->stage != 2 || !p->event) {
    set_error("ebt_cosine_topk_sharded_wait: not a finished batch");
    return EBT_EINVAL;
  }
  ebt_pending& lp = p->local;
  hipStream_t st = (hipStream_t)lp.stream;
  hipEvent_t ev = (hipEvent_t)p->event;
  int rc = hip_check(hipEventSynchronize(ev), "hipEventSynchronize");
  event_put(ev, st);
  p->event = nullptr;
  p->stage = 0;
  if (rc) return rc;
  if (p->host[lp.B + 1] == 0) return EBT_OK;
  // some rank's entries above the floor exceeded its packed capacity (every rank sees the same
  // gathered starts, so every rank takes this branch): the full exchange
  ShardLayout S;
  if (!shard_layout(*lp.cat, p->comm, lp.B, lp.k, lp.opt, &S)) {
    set_error("ebt_cosine_topk_sharded_wait: bad pending batch");
    return EBT_EINVAL;
  }
  rc = sh_full_merge(S, p->comm, lp.ws, lp.B, lp.k, p->out_scores, p->out_rows, lp.timer, st);
  if (!rc) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  return rc;
}

int64_t ebt_shard_sample_tiles(int64_t n_global, int32_t world, int64_t B_pad) {
  if (n_global < 1 || world < 1 || B_pad < 1) return -1;
  return sh_tiles(n_global, world, B_pad);
}

int ebt_cosine_topk_sharded_weighted(const ebt_catalog* cat, const ebt_comm* comm, const void* q,
                                     int q_dtype, int64_t B, int64_t ldq,
                                     const int64_t* liked_off, const int64_t* liked_rows,
                                     int32_t k, const int64_t* excl_off,
                                     const int64_t* excl_rows, const ebt_options* opt,
                                     void* workspace, size_t ws_bytes, double* out_scores,
                                     int64_t* out_rows, void* timer, void* stream,
                                     const double* liked_w) {
  std::vector<int32_t> host((size_t)(B > 0 ? B : 0) + 2);
  ebt_sharded_pending p{};
  int rc = ebt_cosine_topk_sharded_weighted_submit(cat, comm, q, q_dtype, B, ldq, liked_off,
                                                   liked_rows, k, excl_off, excl_rows, opt,
                                                   workspace, ws_bytes, out_scores, out_rows,
                                                   host.data(), &p, timer, stream, liked_w);
  if (!rc) rc = ebt_cosine_topk_sharded_finish(&p);
  if (!rc) rc = ebt_cosine_topk_sharded_wait(&p);
  return rc;
}

int ebt_cosine_topk_sharded(const ebt_catalog* cat, const ebt_comm* comm, const void* q,
                            int q_dtype, int64_t B, int64_t ldq, const int64_t* liked_off,
                            const int64_t* liked_rows, int32_t k, const int64_t* excl_off,
                            const int64_t* excl_rows, const ebt_options* opt, void* workspace,
                            size_t ws_bytes, double* out_scores, int64_t* out_rows, void* timer,
                            void* stream) {
  return ebt_cosine_topk_sharded_weighted(cat, comm, q, q_dtype, B, ldq, liked_off, liked_rows,
                                          k, excl_off, excl_rows, opt, workspace, ws_bytes,
                                          out_scores, out_rows, timer, stream, nullptr);
}

}  // extern "C"
