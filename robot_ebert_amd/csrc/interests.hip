// Multi-interest top-k (include/ebert.h 0.11.0): cluster a user's liked rows, interleave the
// per-cluster answers.
//
// The reference scores a user as the mean cosine to everything they liked (lib.py:51-52), which
// folds a user with several tastes into the centroid of those tastes. These kernels group the
// liked rows of each query and merge the top-k lists searched once per group:
//
//  * interest_cluster_kernel    -- one wave per query over that query's cosine matrix (what
//                                  ebt_pool_gram wrote): a lane owns the slots lane + 64 s. The
//                                  labels live in LDS (one row per wave) and label_j is read as a
//                                  broadcast; in every j loop lane i reads G[j p + i], row j of
//                                  the bitwise symmetric matrix standing in for column j, so the
//                                  reads are coalesced. The c x NS accumulators of a pass stay in
//                                  registers: label_j is wave-uniform, so the accumulator is
//                                  picked by a scalar branch, never by a runtime index. A few rows
//                                  are loaded ahead of the additions, which stay in j order.
//                                  Seeds, medoids and the renumbering are wave arg-bests over
//                                  order-preserving keys (f64_key) with the position second, as
//                                  in mmr_select_kernel; what there is one of per cluster (seed,
//                                  size, medoid, lowest member) sits in LDS, written by lane 0
//                                  and read back as a broadcast. NS (1, 2, 4, 8) is the number
//                                  of slots a lane holds: the smallest that covers p.
//  * interest_interleave_kernel -- one wave per query: the rows already emitted sit in registers,
//                                  one per lane + 64 s, and "already emitted" is a ballot over a
//                                  compare. Lane m holds cluster m's state; the head of every
//                                  list is kept valid (not empty, not emitted), so a round is one
//                                  exact integer comparison per cluster (the highest-averages
//                                  rule) and one emission.
//
// Arithmetic order (compared bitwise with tests/interest_ref.py): every sum runs over the valid
// j ascending from +0.0, one addition at a time; mean = acc / (double) n, one division. Nothing
// depends on p, on where the -1 slots are or on the other queries of the batch: an empty slot
// only ever contributes a skipped j.
#include "pair_f64.h"

namespace ebt {

namespace {

constexpr int IC = EBT_INTEREST_MAX;
constexpr int IL_SLOTS = EBT_INTEREST_K_MAX / 64;   // emitted rows a lane of the interleave holds
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct ClusterArgs {
  const double* gram;      // [B][p][p]
  const int64_t* rows;     // [B][p]
  int64_t B;
  int p, c;
  const int32_t* status;   // NULL: every query is good
  int32_t* label;          // [B][p]
  int32_t* size;           // [B][c]
  int32_t* medoid;         // [B][c]
  int32_t* iters;          // [B]
};

// A wave's own LDS row: its stores are complete before its next loads (and the compiler keeps
// the order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The wave's arg-best by (key desc, position asc) of each lane's candidate (bk, bp); bp = NONE:
// the lane has none. A NaN's key is 0, so a NaN ranks last and the answer is a candidate's
// position whenever there is one; NONE when there is none.
__device__ __forceinline__ uint32_t wave_arg_best(uint64_t bk, uint32_t bp) {
  const uint64_t best = wave_max_u64(bk);
  return wave_min_u32(bk == best ? bp : NONE);
}

// Lane l's value of v as a wave-uniform value (l uniform)
__device__ __forceinline__ int lane_read(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// A wave-uniform read of the wave's own LDS
__device__ __forceinline__ int lds_uniform(const int* q) {
  return __builtin_amdgcn_readfirstlane(*q);
}

template <int NS>
__global__ __launch_bounds__(256) void interest_cluster_kernel(const ClusterArgs a) {
#pragma clang fp contract(off)
  static_assert(64 * NS <= EBT_MMR_POOL_MAX, "a wave's LDS row");
  constexpr int JU = 4;   // rows of the matrix loaded ahead of their additions
  __shared__ int s_lab[4][EBT_MMR_POOL_MAX];
  __shared__ int s_per[4][4][IC];   // what there is one of per cluster, written by lane 0
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int* labs = s_lab[w];
  int* c_seed = s_per[w][0];   // seed_m
  int* c_n = s_per[w][1];      // n_m
  int* c_med = s_per[w][2];    // medoid_m, -1: none
  int* c_low = s_per[w][3];    // the lowest member position of m, -1 (as unsigned: last): none
  const int p = a.p, c = a.c;
  // One query per wave and no loop over queries: what is invariant across such a loop (lane
  // masks, bounds) would be held in scalar registers through the passes and spill
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= a.B) return;
  const double* __restrict__ G = a.gram + b * p * p;
  const bool good = !a.status || a.status[b] >= 0;
  // A slot past p reads column p - 1: a load that is in bounds and never used (its label is -1)
  int col[NS], lab[NS];   // lab: -1 = no row in this slot
  int L = 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int i = lane + 64 * s;
    col[s] = i < p ? i : p - 1;
    const bool v = good && i < p && a.rows[b * p + col[s]] >= 0;
    lab[s] = v ? 0 : -1;
    L += __popcll(__ballot(v));
  }
  if (L == 0) {   // (wave-uniform)
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (lane + 64 * s < p) a.label[b * p + lane + 64 * s] = -1;
    if (lane < c) {
      a.size[b * c + lane] = 0;
      a.medoid[b * c + lane] = -1;
    }
    if (lane == 0) a.iters[b] = 0;
    return;
  }
  const int c_eff = c < L ? c : L;
#pragma unroll
  for (int s = 0; s < NS; ++s) labs[lane + 64 * s] = lab[s];
  wave_lds_sync();

  // ---- tot_i, the seeds, the first labels -----------------------------------------------------
  double acc[IC][NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[0][s] = 0.0;
  for (int j0 = 0; j0 < p; j0 += JU) {
    double v[JU][NS];
    int lj[JU];
#pragma unroll
    for (int u = 0; u < JU; ++u) {
      const int j = j0 + u < p ? j0 + u : p - 1;
      lj[u] = j0 + u < p ? __builtin_amdgcn_readfirstlane(labs[j]) : -1;
      const double* __restrict__ row = G + (int64_t)j * p;
#pragma unroll
      for (int s = 0; s < NS; ++s) v[u][s] = row[col[s]];
    }
#pragma unroll
    for (int u = 0; u < JU; ++u) {
      if (lj[u] < 0) continue;   // (wave-uniform)
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[0][s] = acc[0][s] + v[u][s];
    }
  }
  uint32_t is_seed = 0u;   // bit s: slot lane + 64 s is a seed
  double near[NS];
  {
    uint64_t bk = 0ull;
    uint32_t bp = NONE;
#pragma unroll
    for (int s = 0; s < NS; ++s) {   // positions ascend with s: > keeps the first
      if (lab[s] < 0) continue;
      const uint64_t key = f64_key(acc[0][s]);
      if (bp == NONE || key > bk) {
        bk = key;
        bp = (uint32_t)(lane + 64 * s);
      }
    }
    const int s0 = (int)wave_arg_best(bk, bp);   // (L > 0: a candidate exists)
    if (lane == 0) c_seed[0] = s0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      near[s] = G[(int64_t)s0 * p + col[s]];
      if (lane + 64 * s == s0) is_seed |= 1u << s;
    }
  }
  for (int m = 1; m < c_eff; ++m) {
    uint64_t bk = 0ull;
    uint32_t bp = NONE;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (lab[s] < 0 || ((is_seed >> s) & 1u)) continue;
      // the smallest first: the key's complement (never 0 for a number; a NaN ranks last)
      const uint64_t key = near[s] == near[s] ? ~f64_key(near[s]) : 0ull;
      if (bp == NONE || key > bk) {
        bk = key;
        bp = (uint32_t)(lane + 64 * s);
      }
    }
    const int sm = (int)wave_arg_best(bk, bp);   // (m < c_eff <= L: a candidate exists)
    if (lane == 0) c_seed[m] = sm;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const double sv = G[(int64_t)sm * p + col[s]];
      near[s] = sv > near[s] ? sv : near[s];
      if (lane + 64 * s == sm) is_seed |= 1u << s;
    }
  }
  {
    double bv[NS];
    int first[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      bv[s] = 0.0;
      first[s] = 0;
    }
    wave_lds_sync();
    for (int m = 0; m < c_eff; ++m) {
      const int sm = lds_uniform(c_seed + m);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double sv = G[(int64_t)sm * p + col[s]];
        if (m == 0 || sv > bv[s]) {
          bv[s] = sv;
          first[s] = m;
        }
      }
    }
    for (int m = 0; m < c_eff; ++m) {
      const int sm = lds_uniform(c_seed + m);
#pragma unroll
      for (int s = 0; s < NS; ++s)
        if (lane + 64 * s == sm) first[s] = m;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) lab[s] = lab[s] < 0 ? -1 : first[s];
  }

  // ---- the reassignment passes ------------------------------------------------------------------
  int iters = 0;
  for (int it = 1;; ++it) {
    // PASS(label): the sizes, then mean_{i,m} in acc[m][.]
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < NS; ++s) labs[lane + 64 * s] = lab[s];
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < IC; ++m) {
      int cnt = 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        cnt += __popcll(__ballot(lab[s] == m));
        acc[m][s] = 0.0;
      }
      if (lane == 0) c_n[m] = cnt;
    }
    for (int j0 = 0; j0 < p; j0 += JU) {
      double v[JU][NS];
      int lj[JU];
#pragma unroll
      for (int u = 0; u < JU; ++u) {
        const int j = j0 + u < p ? j0 + u : p - 1;
        lj[u] = j0 + u < p ? __builtin_amdgcn_readfirstlane(labs[j]) : -1;
        const double* __restrict__ row = G + (int64_t)j * p;
#pragma unroll
        for (int s = 0; s < NS; ++s) v[u][s] = row[col[s]];
      }
#pragma unroll
      for (int u = 0; u < JU; ++u) {
        switch (lj[u]) {   // (wave-uniform)
#define EBT_IC_CASE(M)                                                              \
  case M:                                                                           \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) acc[M][s] = acc[M][s] + v[u][s]; \
    break;
          EBT_IC_CASE(0) EBT_IC_CASE(1) EBT_IC_CASE(2) EBT_IC_CASE(3)
          EBT_IC_CASE(4) EBT_IC_CASE(5) EBT_IC_CASE(6) EBT_IC_CASE(7)
#undef EBT_IC_CASE
          default: break;
        }
      }
    }
    wave_lds_sync();
    int nl[NS];
    double bv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      nl[s] = -1;
      bv[s] = 0.0;
    }
#pragma unroll
    for (int m = 0; m < IC; ++m) {   // m ascends: > keeps the lowest m
      const int nm = lds_uniform(c_n + m);
      if (nm <= 0) continue;   // (wave-uniform)
      const double dn = (double)nm;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        acc[m][s] = acc[m][s] / dn;
        if (nl[s] < 0 || acc[m][s] > bv[s]) {
          bv[s] = acc[m][s];
          nl[s] = m;
        }
      }
    }
    if (it > EBT_INTEREST_ITERS) break;   // the pass after the cap: final values only
    bool moved = false;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (lab[s] < 0) nl[s] = -1;
      moved |= nl[s] != lab[s];
    }
    iters = it;
    if (__ballot(moved) == 0ull) break;   // (wave-uniform)
#pragma unroll
    for (int s = 0; s < NS; ++s) lab[s] = nl[s];
  }

  // ---- medoids, renumbering, outputs -------------------------------------------------------------
  double own[NS];   // mean_{i, label_i}
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    own[s] = 0.0;
#pragma unroll
    for (int m = 0; m < IC; ++m) own[s] = lab[s] == m ? acc[m][s] : own[s];
  }
  if (lane < IC) {
    c_med[lane] = -1;
    c_low[lane] = -1;
  }
  for (int m = 0; m < c_eff; ++m) {
    uint64_t bk = 0ull;
    uint32_t bp = NONE, lo = NONE;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (lab[s] != m) continue;
      const uint64_t key = f64_key(own[s]);
      if (lo == NONE) lo = (uint32_t)(lane + 64 * s);
      if (bp == NONE || key > bk) {
        bk = key;
        bp = (uint32_t)(lane + 64 * s);
      }
    }
    const uint32_t best = wave_arg_best(bk, bp);   // NONE = -1: an empty cluster
    const uint32_t first = wave_min_u32(lo);
    if (lane == 0) {
      c_med[m] = (int)best;
      c_low[m] = (int)first;
    }
  }
  wave_lds_sync();
  // lane m: n_m, medoid_m, and the number of clusters that come before m
  const int n_v = c_n[lane & (IC - 1)], med_v = c_med[lane & (IC - 1)];
  const uint32_t low_v = (uint32_t)c_low[lane & (IC - 1)];
  int newm_v = 0;
#pragma unroll
  for (int o = 0; o < IC; ++o) {
    const int no = lds_uniform(c_n + o);
    const uint32_t lo = (uint32_t)lds_uniform(c_low + o);
    if (no > 0 && (no > n_v || (no == n_v && lo < low_v))) ++newm_v;
  }
  const int ne = __popcll(__ballot(lane < IC && n_v > 0));
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int moved_to = __shfl(newm_v, lab[s] & 63, 64);
    if (lane + 64 * s < p) a.label[b * p + lane + 64 * s] = lab[s] < 0 ? -1 : moved_to;
  }
  if (lane < IC && n_v > 0) {   // (newm_v < ne <= c_eff <= c)
    a.size[b * c + newm_v] = n_v;
    a.medoid[b * c + newm_v] = med_v;
  }
  if (lane >= ne && lane < c) {
    a.size[b * c + lane] = 0;
    a.medoid[b * c + lane] = -1;
  }
  if (lane == 0) a.iters[b] = iters;
}

// ---- the interleave -------------------------------------------------------------------------------
struct InterleaveArgs {
  const int32_t* size;          // [B][c]
  const int64_t* list_rows;     // [B][c][k]
  const double* list_scores;    // [B][c][k]
  int64_t B;
  int c, k;
  int64_t* rows;                // each [B][k]
  double* scores;
  int32_t* cluster;
  int32_t* pos;
};

__device__ __forceinline__ int64_t uniform_i64(int64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The first position q >= from of a list (k entries) that holds a row not yet emitted (k: none),
// and that row. Wave-uniform.
__device__ __forceinline__ int settle_head(const int64_t* __restrict__ list, int k, int from,
                                           const int64_t (&em)[IL_SLOTS], int64_t& row) {
  int q = from;
  row = -1;
  while (q < k) {
    const int64_t r = uniform_i64(list[q]);
    if (r >= 0) {
      bool hit = false;
#pragma unroll
      for (int s = 0; s < IL_SLOTS; ++s) hit |= em[s] == r;
      if (__ballot(hit) == 0ull) {
        row = r;
        break;
      }
    }
    ++q;
  }
  return q;
}

__global__ __launch_bounds__(256) void interest_interleave_kernel(const InterleaveArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = a.c, k = a.k;
  for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < a.B; b += (int64_t)gridDim.x * 4) {
    const int64_t* __restrict__ LR = a.list_rows + b * c * k;
    const uint64_t* __restrict__ LS = (const uint64_t*)a.list_scores + b * c * k;
    int64_t em[IL_SLOTS];   // emitted row t sits in lane t % 64, slot t / 64
#pragma unroll
    for (int s = 0; s < IL_SLOTS; ++s) em[s] = -1;
    // Lane m holds cluster m's state: its size, the slots it took, the position of its head and
    // the head's row. A head is always a row not yet emitted, or nxt == k.
    int sz_v = 0, taken_v = 0, nxt_v = k;
    int64_t head_v = -1;
    for (int m = 0; m < c; ++m) {
      const int szm = __builtin_amdgcn_readfirstlane(a.size[b * c + m]);
      if (szm <= 0) continue;   // (wave-uniform)
      int64_t r;
      const int q = settle_head(LR + (int64_t)m * k, k, 0, em, r);
      if (lane == m) {
        sz_v = szm;
        nxt_v = q;
        head_v = r;
      }
    }
    int t = 0;
    for (; t < k; ++t) {
      int ms = -1;
      int64_t bs = 0, bt = 1;
#pragma unroll
      for (int m = 0; m < IC; ++m) {   // m ascends: > keeps the lowest m of equal quotients
        const int szm = lane_read(sz_v, m), nx = lane_read(nxt_v, m), tk = lane_read(taken_v, m);
        if (szm <= 0 || nx >= k) continue;
        if (ms < 0 || (int64_t)szm * bt > bs * (int64_t)(tk + 1)) {
          ms = m;
          bs = szm;
          bt = tk + 1;
        }
      }
      if (ms < 0) break;   // nothing is live (wave-uniform)
      const int q = lane_read(nxt_v, ms);
      const uint32_t rlo = (uint32_t)lane_read((int)(uint32_t)head_v, ms);
      const uint32_t rhi = (uint32_t)lane_read((int)(uint32_t)((uint64_t)head_v >> 32), ms);
      const int64_t r = (int64_t)(((uint64_t)rhi << 32) | rlo);
      if (lane == ms) ++taken_v;
      if (lane == 0) {
        a.rows[b * k + t] = r;
        ((uint64_t*)a.scores)[b * k + t] = LS[(int64_t)ms * k + q];
        a.cluster[b * k + t] = ms;
        a.pos[b * k + t] = q;
      }
#pragma unroll
      for (int s = 0; s < IL_SLOTS; ++s)
        if (s == (t >> 6) && lane == (t & 63)) em[s] = r;
      // the heads that were this row move on (ms's own among them)
      uint64_t stale = __ballot(sz_v > 0 && nxt_v < k && head_v == r);
      while (stale) {
        const int m = __builtin_ctzll(stale);
        stale &= stale - 1;
        int64_t r2;
        const int q2 = settle_head(LR + (int64_t)m * k, k, lane_read(nxt_v, m) + 1, em, r2);
        if (lane == m) {
          nxt_v = q2;
          head_v = r2;
        }
      }
    }
    for (int tt = t + lane; tt < k; tt += 64) {
      a.rows[b * k + tt] = -1;
      a.scores[b * k + tt] = f64_nan();
      a.cluster[b * k + tt] = -1;
      a.pos[b * k + tt] = -1;
    }
  }
}

constexpr int64_t CLUSTER_B_MAX = (int64_t)4 * 0x7fffffff;   // four queries per workgroup

int check_cluster_sizes(const char* who, int64_t B, int32_t p, int32_t c) {
  if (B < 0 || B > CLUSTER_B_MAX || p < 1 || p > EBT_MMR_POOL_MAX || c < 1 || c > EBT_INTEREST_MAX) {
    set_error("%s: bad arguments (B=%lld p=%d c=%d: 1 <= p <= %d, 1 <= c <= %d)", who,
              (long long)B, p, c, EBT_MMR_POOL_MAX, EBT_INTEREST_MAX);
    return EBT_EINVAL;
  }
  return EBT_OK;
}

template <int NS>
void launch_cluster(const ClusterArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(interest_cluster_kernel<NS>, dim3((unsigned)ceil_div(a.B, 4)), dim3(256), 0,
                     st, a);
}

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

size_t ebt_interest_workspace_bytes(int64_t B, int32_t p) { return ebt_mmr_workspace_bytes(B, p); }

int ebt_interest_cluster(const double* gram, const int64_t* rows, int64_t B, int32_t p, int32_t c,
                         const int32_t* status, int32_t* out_label, int32_t* out_size,
                         int32_t* out_medoid, int32_t* out_iters, void* stream) {
  const char* who = "ebt_interest_cluster";
  if (!gram || !rows || !out_label || !out_size || !out_medoid || !out_iters) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  const int rc = check_cluster_sizes(who, B, p, c);
  if (rc) return rc;
  if (B == 0) return EBT_OK;
  ClusterArgs a;
  a.gram = gram; a.rows = rows; a.B = B; a.p = p; a.c = c; a.status = status;
  a.label = out_label; a.size = out_size; a.medoid = out_medoid; a.iters = out_iters;
  hipStream_t st = (hipStream_t)stream;
  if (p <= 64) launch_cluster<1>(a, st);
  else if (p <= 128) launch_cluster<2>(a, st);
  else if (p <= 256) launch_cluster<4>(a, st);
  else launch_cluster<8>(a, st);
  return launch_check("interest_cluster_kernel");
}

int ebt_liked_interests(const ebt_catalog* cat, int64_t B, const int64_t* rows, int32_t p,
                        int32_t c, void* workspace, size_t ws_bytes, int32_t* out_label,
                        int32_t* out_size, int32_t* out_medoid, int32_t* out_iters,
                        int32_t* status, void* stream) {
  const char* who = "ebt_liked_interests";
  int rc = check_catalog(who, cat);
  if (rc) return rc;
  if (!rows || !workspace || !out_label || !out_size || !out_medoid || !out_iters || !status) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  rc = check_cluster_sizes(who, B, p, c);
  if (rc) return rc;
  if (B == 0) return EBT_OK;
  const size_t need = ebt_interest_workspace_bytes(B, p);
  if (need == 0 || ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes (ebt_interest_workspace_bytes)", who, ws_bytes,
              need);
    return EBT_EINVAL;
  }
  rc = ebt_pool_gram(cat, B, rows, p, (double*)workspace, status, stream);
  if (rc) return rc;
  return ebt_interest_cluster((const double*)workspace, rows, B, p, c, status, out_label,
                              out_size, out_medoid, out_iters, stream);
}

int ebt_interest_interleave(const int32_t* size, const int64_t* list_rows,
                            const double* list_scores, int64_t B, int32_t c, int32_t k,
                            int64_t* out_rows, double* out_scores, int32_t* out_cluster,
                            int32_t* out_pos, void* stream) {
  const char* who = "ebt_interest_interleave";
  if (!size || !list_rows || !list_scores || !out_rows || !out_scores || !out_cluster ||
      !out_pos) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (B < 0 || c < 1 || c > EBT_INTEREST_MAX || k < 1 || k > EBT_INTEREST_K_MAX) {
    set_error("%s: bad arguments (B=%lld c=%d k=%d: 1 <= c <= %d, 1 <= k <= %d)", who,
              (long long)B, c, k, EBT_INTEREST_MAX, EBT_INTEREST_K_MAX);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  InterleaveArgs a;
  a.size = size; a.list_rows = list_rows; a.list_scores = list_scores; a.B = B; a.c = c; a.k = k;
  a.rows = out_rows; a.scores = out_scores; a.cluster = out_cluster; a.pos = out_pos;
  hipLaunchKernelGGL(interest_interleave_kernel, dim3((unsigned)grid_of(ceil_div(B, 4), 1 << 20)),
                     dim3(256), 0, (hipStream_t)stream, a);
  return launch_check("interest_interleave_kernel");
}

}  // extern "C"
