// Grouped top-k (include/ebert.h 0.12.0): the k best rows of every category from ONE scoring pass.
//
// The reference scores a user against the whole catalog and keeps one list (lib.py:51-55); a
// front page wants one list per genre. With allow masks alone that is G calls, each repeating the
// B x N screening GEMM for the same query vectors. Here the scores of a chunk are materialised
// once (ebt_screen_scores, ebt_mask_excluded) and one selection keeps a candidate list per
// (query, group); nothing writes -inf back into the scores.
//
//  * grouped_select_kernel -- the streaming select of select_topk.hip (dense form) with one
//    threshold and one candidate buffer PER GROUP, all in LDS. A 256-thread workgroup owns a
//    (query, segment) and streams it in 4096-entry tiles (16 values per lane as four 16-byte
//    loads, the next tile prefetched into registers). Per tile and group: one compare of the
//    lane's largest value with the group's threshold and a ballot; only a wave that has something
//    above the threshold reads the group's mask bits (the same word per mask for four columns
//    as mask_allowed_kernel; the words of the next tile are staged in LDS for all groups at once
//    while this tile is admitted), builds its lanes' admission masks and appends with ONE LDS
//    atomic per wave, as the plain select does. A group's buffer holds max(2 k', 256) entries;
//    the tile that overflows one is finished for that group by the whole workgroup: compact to
//    the k' best (select_core.h, the plain select's radix select), raise the threshold, admit
//    what is still above it, repeat. Lanes whose entries did not fit wrote none of them (the
//    slots they had reserved below the capacity are filled with empty entries, key 0), so the
//    retry recomputes exactly their masks. Thresholds only rise there, so after the first tiles
//    almost every (tile, group) costs the compare and the ballot. At the end every group's
//    survivors are compacted and bitonic-sorted by (value desc, index asc).
//    The buffers of all G groups do not fit in LDS at large G k': a launch serves
//    ebt_grouped_pass_groups(k') groups and the entry runs ceil(G / that) launches. EACH LAUNCH
//    READS THE SCORE CHUNK AGAIN (B n 4 bytes).
//  * ebt_cosine_topk_grouped_prepared -- the unfused pipeline around it, on the unfused path's own
//    plan and chunk step (api.hip chunk_plan, score_chunk): per chunk screen, mask the excluded
//    rows, grouped select; then one merge of every (group, query)'s per-chunk lists
//    (ebt_select_topk's candidate-list form over G B rows) and G rescores, one per group block.
//    Group g's block sees the approximate scores, the selection rule and the rescore that
//    ebt_cosine_topk_prepared_allowed gives a batch whose queries all carry mask groups[g], so
//    its scores, rows and certificates are that call's.
#include "common.h"
#include "internal.h"
#include "select_core.h"

namespace ebt {

namespace {

constexpr int GSE = 16;                    // values per lane per tile
constexpr int GTILE = STHREADS * GSE;      // 4096 entries per tile
constexpr int GCAP_MIN = 256;              // smallest candidate buffer of a group (entries)
// dynamic LDS a workgroup may take: two workgroups per CU at the most groups, more at fewer
constexpr size_t GROUPED_LDS = 64 * 1024;

// mask words staged per tile and group: the 4096 bits of the tile from any bit of their first
// word on (129 words), rounded up to whole 16 bytes
constexpr int GMW = 132;

// LDS: [keep / hist][red, misc, flags: 256 bytes][cnt, tf, id of EBT_GROUPS_MAX groups]
//      [mask words: 2 tiles x ng groups x GMW][group 0: keys[cap] idx[cap]][group 1: ...]
struct GroupedLds {
  int cap;   // a group's buffer capacity (entries)
  int kpp;   // next pow2 >= kprime
  // off_mask: where what grows with the groups starts; per_group: the bytes of one group there
  size_t off_keep, off_misc, off_grp, off_mask, per_group;
};

__host__ __device__ inline GroupedLds grouped_lds(int kprime) {
  GroupedLds L;
  L.cap = 2 * kprime < GCAP_MIN ? GCAP_MIN : 2 * kprime;
  L.kpp = next_pow2(kprime);
  size_t keep_bytes = 8 * (size_t)L.kpp;
  if (keep_bytes < 4 * (size_t)SHIST) keep_bytes = 4 * (size_t)SHIST;  // aliased with hist
  L.off_keep = 0;
  L.off_misc = keep_bytes;
  L.off_grp = L.off_misc + 256;
  L.off_mask = L.off_grp + 3 * 4 * (size_t)EBT_GROUPS_MAX;
  L.per_group = 2 * 4 * (size_t)GMW + 8 * (size_t)L.cap;
  return L;
}

int pass_groups(int kprime) {
  const GroupedLds L = grouped_lds(kprime);
  const size_t fit = (GROUPED_LDS - L.off_mask) / L.per_group;
  return (int)(fit < (size_t)EBT_GROUPS_MAX ? fit : (size_t)EBT_GROUPS_MAX);
}

struct GroupedSel {
  const float* vals;        // [B][ld], scores of GLOBAL rows [col_begin, col_begin + n)
  int64_t ld, n, seg_len, col_begin;
  const uint32_t* masks;    // [n_masks][words]
  int64_t words;
  int32_t n_masks;
  const int32_t* groups;    // device [G]
  int g0, ng;               // this launch serves groups [g0, g0 + ng)
  int kprime;
  int64_t B;
  float* out_vals;          // [(g * B + b) * ld_out + seg * kprime + j]
  int64_t* out_idx;
  int64_t ld_out;
};

// the wave's exclusive prefix and total of a per-lane count 0..16 (five bits), one ballot per bit
__device__ __forceinline__ void wave_prefix5(uint32_t cnt, uint32_t& excl, uint32_t& tot) {
  excl = 0;
  tot = 0;
#pragma unroll
  for (int bit = 0; bit < 5; ++bit) {
    const uint64_t bm = __ballot((cnt >> bit) & 1u);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(
        (uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
    excl += below << bit;
    tot += (uint32_t)__popcll(bm) << bit;
  }
}

// a word of LDS that every lane reads alike, as a scalar: the branches on it are uniform
__device__ __forceinline__ uint32_t lds_uniform(const uint32_t* p) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)*p);
}

// float form of "key >= t" (select_topk_kernel's): keys up to f2key(-FLT_MAX) admit every finite
// value; above that key2f(t) is a float, or a NaN that admits nothing
__device__ __forceinline__ float thr_float(uint32_t t) {
  return t <= 0x00800000u ? -3.402823466e38f : key2f(t);
}

__global__ __launch_bounds__(STHREADS, 2) void grouped_select_kernel(const GroupedSel a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GroupedLds Lo = grouped_lds(a.kprime);
  uint64_t* keep = (uint64_t*)(smem + Lo.off_keep);
  uint32_t* hist = (uint32_t*)(smem + Lo.off_keep);  // aliased
  uint64_t* red = (uint64_t*)(smem + Lo.off_misc);
  uint32_t* misc = (uint32_t*)(smem + Lo.off_misc + 64);  // [0, 12): select_core.h's
  uint32_t* s_flag = misc + 16;   // [3]: "a group overflowed in this tile", rotating by tile
  uint32_t* s_pend = misc + 20;   // the retry: "an entry is still waiting"
  uint32_t* s_cnt = (uint32_t*)(smem + Lo.off_grp);
  float* s_tf = (float*)(s_cnt + EBT_GROUPS_MAX);
  int* s_gid = (int*)(s_cnt + 2 * EBT_GROUPS_MAX);
  const int cap = Lo.cap, kprime = a.kprime, ng = a.ng;
  uint32_t* s_mask = (uint32_t*)(smem + Lo.off_mask);   // [2][ng][GMW]
  uint32_t* buf = s_mask + 2 * ng * GMW;

  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t row = blockIdx.x;
  const int seg = blockIdx.y;
  const int64_t s0 = (int64_t)seg * a.seg_len;
  int64_t s1 = s0 + a.seg_len;
  s1 = s1 < a.n ? s1 : a.n;
  const float* vrow = a.vals + row * a.ld;

  if (tid < ng) {
    const int gid = a.groups[a.g0 + tid];
    s_cnt[tid] = 0;
    s_gid[tid] = gid;
    // an id past the table admits nothing (no float is >= NaN) and reads no mask word
    s_tf[tid] = gid >= a.n_masks ? __builtin_nanf("") : -3.402823466e38f;
  }
  if (tid < 3) s_flag[tid] = 0;
  lds_barrier();

  // The mask words of the tile at t0 for every group of the launch, into the tile's half of
  // s_mask: word i of a group is word ((col_begin + t0) >> 5) + i of its mask row, all ones for
  // a negative id, 0 for an id or a word past the table. Thread i < GMW fetches word i of every
  // group: ng independent loads in flight at once, where a fetch inside the loop over the
  // groups would wait for memory once per group.
  auto stage_masks = [&](int64_t t0, int half) {
    if (tid >= GMW) return;
    const int64_t w = ((a.col_begin + t0) >> 5) + tid;
    uint32_t* dst = s_mask + (size_t)half * ng * GMW + tid;
    for (int g = 0; g < ng; ++g) {
      const int gid = s_gid[g];
      uint32_t v = gid < 0 ? 0xFFFFFFFFu : 0u;
      if (gid >= 0 && gid < a.n_masks && w < a.words) v = a.masks[(int64_t)gid * a.words + w];
      dst[g * GMW] = v;
    }
  };

  float cur[GSE], nxt[GSE];
  // element e of the tile at t0: column t0 + (e >> 2) * (STHREADS * 4) + tid * 4 + (e & 3)
  auto load_tile = [&](int64_t t0, float* v) {
#pragma unroll
    for (int j = 0; j < GSE / 4; ++j) {
      const int64_t p = t0 + j * (STHREADS * 4) + tid * 4;
      if (p < s1) {  // (p % 4 == 0 and ld % 4 == 0: the four floats are inside the row)
        const float4 f = *(const float4*)(vrow + p);
        v[4 * j + 0] = f.x;
        v[4 * j + 1] = f.y;
        v[4 * j + 2] = f.z;
        v[4 * j + 3] = f.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * j + e] = -__builtin_inff();
      }
    }
  };
  // this lane's entries of the tile that group g admits at threshold tf: bit e = element e is
  // inside the segment, allowed by the group's mask and >= tf (NaN and -inf never are)
  auto lane_mask = [&](const float* v, int g, float tf, int64_t t0, int lim,
                       int half) -> uint32_t {
    const uint32_t* mw = s_mask + ((size_t)half * ng + g) * GMW;
    const int sh0 = (int)((a.col_begin + t0) & 31);  // any alignment against the mask words
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < GSE / 4; ++j) {
      const int o = j * (STHREADS * 4) + tid * 4;
      const int i = (sh0 + o) >> 5;   // <= 128
      const int sh = (sh0 + o) & 31;
      const uint32_t lo = mw[i];
      const uint32_t hi = sh > 28 ? mw[i + 1] : 0u;  // the four bits straddle two words
      const uint32_t allow = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh) & 0xFu;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool take = ((allow >> e) & 1u) && (o + e < lim) && v[4 * j + e] >= tf;
        m |= (take ? 1u : 0u) << (4 * j + e);
      }
    }
    return m;
  };
  auto idx_of = [&](int64_t t0, int e) -> uint32_t {
    return (uint32_t)t0 + (uint32_t)((e >> 2) * (STHREADS * 4) + tid * 4 + (e & 3));
  };

  uint64_t ovfmask = 0;  // groups in which this lane's entries of the current tile did not fit
  const int64_t ntiles = s1 > s0 ? (s1 - s0 + GTILE - 1) / GTILE : 0;
  if (ntiles > 0) {
    load_tile(s0, cur);
    stage_masks(s0, 0);
    lds_barrier();
  }
  for (int64_t it = 0; it < ntiles; ++it) {
    const int64_t t0 = s0 + it * GTILE;
    const int half = (int)(it & 1);
    if (it + 1 < ntiles) {
      load_tile(t0 + GTILE, nxt);
      // the other half was last read in the tile before this one, retry included: every wave
      // has passed that tile's barriers; it is read again after this tile's
      stage_masks(t0 + GTILE, half ^ 1);
    }
    const int lim = (int)(s1 - t0 < GTILE ? s1 - t0 : GTILE);
    const int slot = (int)(it % 3);
    // a superset test per group: the lane's largest value (fmaxf drops NaNs) against the
    // group's threshold; a wave with nothing above it skips the group, mask words included
    float vmax = cur[0];
#pragma unroll
    for (int e = 1; e < GSE; ++e) vmax = __builtin_fmaxf(vmax, cur[e]);
    for (int g = 0; g < ng; ++g) {
      const float tf = s_tf[g];
      if (__ballot(vmax >= tf) == 0ull) continue;
      const uint32_t msk = lane_mask(cur, g, tf, t0, lim, half);
      const uint32_t cnt = (uint32_t)__popc(msk);
      uint32_t excl, tot;
      wave_prefix5(cnt, excl, tot);
      if (tot == 0u) continue;
      uint32_t wb = 0;
      if (lane == 0) wb = atomicAdd(&s_cnt[g], tot);
      wb = (uint32_t)__builtin_amdgcn_readfirstlane((int)wb);
      if (cnt == 0u) continue;
      uint32_t* bk = buf + (size_t)g * 2 * cap;
      uint32_t* bi = bk + cap;
      uint32_t pos = wb + excl;
      const bool fits = pos + cnt <= (uint32_t)cap;
      if (!fits) {
        ovfmask |= 1ull << g;
        s_flag[slot] = 1u;
      }
      // all of the lane's entries or none: the slots it reserved below the capacity become empty
      // entries (key 0 ranks last and is written out as -inf / -1), so the buffer has no holes
#pragma unroll
      for (int e = 0; e < GSE; ++e) {
        if (((msk >> e) & 1u) && pos < (uint32_t)cap) {
          bk[pos] = fits ? f2key(cur[e]) : 0u;
          bi[pos] = idx_of(t0, e);
          ++pos;
        }
      }
    }
    lds_barrier();
    // the flag of the tile before this one was read by every wave before this barrier, and is
    // written again only after the next one
    if (tid == 0) s_flag[(it + 2) % 3] = 0u;
    if (lds_uniform(s_flag + slot) != 0u) {  // (stable until the next tile's barrier)
      uint64_t og = 0;
      for (int g = 0; g < ng; ++g)
        if (lds_uniform(s_cnt + g) > (uint32_t)cap) og |= 1ull << g;
      while (og) {  // (uniform: s_cnt changes only between the barriers below)
        const int g = __builtin_ctzll(og);
        og &= og - 1;
        uint32_t* bk = buf + (size_t)g * 2 * cap;
        uint32_t* bi = bk + cap;
        uint32_t pend = ((ovfmask >> g) & 1ull) ? lane_mask(cur, g, s_tf[g], t0, lim, half) : 0u;
        for (;;) {  // the buffer is full: cap entries
          const uint64_t theta = compact(bk, bi, cap, kprime, keep, hist, red, misc);
          // a waiting entry that the k' kept ones already beat is dropped (composites: exact)
#pragma unroll
          for (int e = 0; e < GSE; ++e) {
            if (((pend >> e) & 1u) && !(comp_of(f2key(cur[e]), idx_of(t0, e)) > theta))
              pend &= ~(1u << e);
          }
          if (tid == 0) {
            s_cnt[g] = (uint32_t)kprime;
            *s_pend = 0u;
            // later tiles hold larger indices than every kept entry: a tie with the k'-th key
            // loses, so the threshold is the next key
            s_tf[g] = thr_float((uint32_t)(theta >> 32) + 1u);
          }
          lds_barrier();
          const uint32_t cnt = (uint32_t)__popc(pend);
          uint32_t excl, tot;
          wave_prefix5(cnt, excl, tot);
          if (tot) {
            uint32_t wb = 0;
            if (lane == 0) wb = atomicAdd(&s_cnt[g], tot);
            wb = (uint32_t)__builtin_amdgcn_readfirstlane((int)wb);
            uint32_t pos = wb + excl;
#pragma unroll
            for (int e = 0; e < GSE; ++e) {
              if ((pend >> e) & 1u) {
                if (pos < (uint32_t)cap) {
                  bk[pos] = f2key(cur[e]);
                  bi[pos] = idx_of(t0, e);
                  pend &= ~(1u << e);
                }
                ++pos;
              }
            }
          }
          if (pend) *s_pend = 1u;
          lds_barrier();
          if (lds_uniform(s_pend) == 0u) break;  // (reset only after compact's barriers)
        }
      }
      ovfmask = 0;
    }
    if (it + 1 < ntiles) {
#pragma unroll
      for (int e = 0; e < GSE; ++e) cur[e] = nxt[e];
    }
  }

  // every group: its min(kprime, entries) best, sorted
  const int P = Lo.kpp;
  for (int g = 0; g < ng; ++g) {
    uint32_t* bk = buf + (size_t)g * 2 * cap;
    uint32_t* bi = bk + cap;
    int nk = (int)lds_uniform(s_cnt + g);
    nk = nk < cap ? nk : cap;
    if (nk > kprime) {
      compact(bk, bi, nk, kprime, keep, hist, red, misc);
      nk = kprime;
    }
    for (int i = tid; i < P; i += STHREADS) keep[i] = i < nk ? comp_of(bk[i], bi[i]) : 0ull;
    lds_barrier();
    bitonic_desc(keep, P);
    const int64_t o = ((int64_t)(a.g0 + g) * a.B + row) * a.ld_out + (int64_t)seg * kprime;
    for (int i = tid; i < kprime; i += STHREADS) {
      const uint64_t c = keep[i];
      const uint32_t key = (uint32_t)(c >> 32);
      a.out_vals[o + i] = key ? key2f(key) : -__builtin_inff();
      a.out_idx[o + i] = key ? a.col_begin + (int64_t)(~(uint32_t)c) : -1;
    }
    lds_barrier();  // keep is the next group's
  }
}

int check_table(const char* who, const uint32_t* masks, int64_t words, int32_t n_masks,
                int64_t row_end) {
  if (words < 1 || words % 4 != 0 || n_masks < 1 || words > (INT64_MAX >> 5) ||
      words * 32 < row_end || ((uintptr_t)masks & 15) != 0) {
    set_error("%s: bad allow table (words=%lld: a multiple of 4 with 32 words >= row %lld, "
              "ebt_allow_words; n_masks=%d: >= 1; masks 16-byte aligned)", who, (long long)words,
              (long long)row_end, n_masks);
    return EBT_EINVAL;
  }
  return EBT_OK;
}

int select_grouped(const float* vals, int64_t ld, int64_t B, int64_t n, int64_t col_begin,
                   const uint32_t* masks, int64_t words, int32_t n_masks, const int32_t* groups,
                   int32_t G, int32_t kprime, int32_t segs, float* out_vals, int64_t* out_idx,
                   int64_t ld_out, hipStream_t stream) {
  const char* who = "ebt_select_topk_grouped";
  if (!vals || !masks || !groups || !out_vals || !out_idx) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (G < 1 || G > EBT_GROUPS_MAX || kprime < 1 || kprime > EBT_GROUPED_KPRIME_MAX || B < 0 ||
      B > 0x7fffffffLL || n < 0 || n >= 0x7fffffffLL || col_begin < 0 || ld < n || ld % 4 != 0 ||
      ((uintptr_t)vals & 15) != 0 || segs < 1 || segs > 65535 ||
      ld_out < (int64_t)segs * kprime) {
    set_error("%s: bad arguments (B=%lld n=%lld col_begin=%lld ld=%lld: a multiple of 4 and >= n, "
              "vals 16-byte aligned; G=%d: 1..%d; kprime=%d: 1..%d; segs=%d; ld_out=%lld)", who,
              (long long)B, (long long)n, (long long)col_begin, (long long)ld, G, EBT_GROUPS_MAX,
              kprime, EBT_GROUPED_KPRIME_MAX, segs, (long long)ld_out);
    return EBT_EINVAL;
  }
  const int rc = check_table(who, masks, words, n_masks, col_begin + n);
  if (rc) return rc;
  if (B == 0) return EBT_OK;
  GroupedSel a;
  a.vals = vals; a.ld = ld; a.n = n; a.col_begin = col_begin;
  a.seg_len = (ceil_div(n > 0 ? n : 1, segs) + 3) & ~(int64_t)3;
  a.masks = masks; a.words = words; a.n_masks = n_masks; a.groups = groups;
  a.kprime = kprime; a.B = B; a.out_vals = out_vals; a.out_idx = out_idx; a.ld_out = ld_out;
  const GroupedLds L = grouped_lds(kprime);
  const int per = pass_groups(kprime);
  set_max_lds((const void*)grouped_select_kernel, (int)GROUPED_LDS);
  for (int g0 = 0; g0 < G; g0 += per) {  // each launch reads the scores again
    a.g0 = g0;
    a.ng = G - g0 < per ? G - g0 : per;
    const size_t lds = L.off_mask + (size_t)a.ng * L.per_group;
    hipLaunchKernelGGL(grouped_select_kernel, dim3((unsigned)B, (unsigned)segs), dim3(STHREADS),
                       lds, stream, a);
    const int lrc = launch_check("grouped_select_kernel");
    if (lrc) return lrc;
  }
  return EBT_OK;
}

// The workspace of ebt_cosine_topk_grouped_prepared:
//   [S: B_pad x ld_s f32][per-chunk, per-segment lists of G B rows][final lists of G B rows]
//   [eps B_pad, the float64 screen only]
struct GroupedWs : ChunkPlan {   // (the unfused path's plan of the whole catalog)
  int64_t lists;                 // n_chunks * segs per (group, query)
  size_t off_s, off_lv, off_li, off_fv, off_fi, off_eps, bytes;
};

GroupedWs grouped_ws(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime, int64_t chunk_rows,
                     int flags, int32_t G) {
  GroupedWs L{};
  // so that every chunk goes through the screening GEMM exactly as it does on the unfused path
  static_cast<ChunkPlan&>(L) = chunk_plan(B, n_rows, chunk_rows);
  L.lists = L.n_chunks * L.segs;
  const size_t rows = (size_t)G * (size_t)B;
  size_t o = 0;
  L.off_s = carve(o, (size_t)B_pad * L.ld_s * 4);
  L.off_lv = o;
  L.off_li = o;
  if (L.lists > 1) {
    L.off_lv = carve(o, rows * L.lists * kprime * 4);
    L.off_li = carve(o, rows * L.lists * kprime * 8);
  }
  L.off_fv = carve(o, rows * kprime * 4);
  L.off_fi = carve(o, rows * kprime * 8);
  L.off_eps = o;
  if (flags & EBT_FLAG_EXACT) L.off_eps = carve(o, (size_t)B_pad * 4);
  L.bytes = o;
  return L;
}

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

int32_t ebt_grouped_pass_groups(int32_t kprime) {
  return kprime < 1 || kprime > EBT_GROUPED_KPRIME_MAX ? 0 : pass_groups(kprime);
}

int ebt_select_topk_grouped(const float* vals, int64_t ld, int64_t B, int64_t n,
                            int64_t col_begin, const uint32_t* masks, int64_t words,
                            int32_t n_masks, const int32_t* groups, int32_t G, int32_t kprime,
                            int32_t segs, float* out_vals, int64_t* out_idx, int64_t ld_out,
                            void* stream) {
  return select_grouped(vals, ld, B, n, col_begin, masks, words, n_masks, groups, G, kprime, segs,
                        out_vals, out_idx, ld_out, (hipStream_t)stream);
}

size_t ebt_cosine_topk_grouped_workspace(int64_t B, int64_t B_pad, int64_t n_rows, int32_t kprime,
                                         int64_t chunk_rows, int flags, int32_t G) {
  if (B < 0 || B_pad < B || n_rows < 1 || kprime < 1 || kprime > EBT_GROUPED_KPRIME_MAX ||
      chunk_rows < 1 || G < 1 || G > EBT_GROUPS_MAX)
    return 0;
  return grouped_ws(B, B_pad, n_rows, kprime, chunk_rows, flags, G).bytes;
}

int ebt_cosine_topk_grouped_prepared(
    const double* q64, const void* qimg, const float* qscale, const float* eps, int64_t B,
    int64_t B_pad, const void* cat, int dtype, int64_t ld, const double* gnorm64,
    const void* cimg, const float* cscale, int img_dtype, int32_t ld_img, int64_t n_rows,
    int32_t d, int32_t d_pad, int64_t row_offset, const int64_t* excl_off,
    const int64_t* excl_rows, int32_t k, int32_t kprime, int64_t chunk_rows, int flags,
    const int32_t* groups, int32_t G, const uint32_t* masks, int64_t words, int32_t n_masks,
    void* workspace, size_t ws_bytes, double* out_scores, int64_t* out_rows, int32_t* certified,
    void* timer, void* stream) {
  const char* who = "ebt_cosine_topk_grouped_prepared";
  const bool exact = flags & EBT_FLAG_EXACT;
  if (!q64 || (!exact && (!qimg || !qscale || !eps || !cimg)) || !cat || !gnorm64 || !groups ||
      !masks || !workspace || !out_scores || !out_rows || !certified) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if ((k < n_rows ? (int64_t)k : n_rows) > EBT_GROUPED_KPRIME_MAX) {
    set_error("%s: min(k, n) = %lld > %d (the full-sort path included) is not supported", who,
              (long long)(k < n_rows ? (int64_t)k : n_rows), EBT_GROUPED_KPRIME_MAX);
    return EBT_EUNSUPPORTED;
  }
  if (row_offset != 0) {
    set_error("%s: row_offset=%lld: a row-sharded catalog is not supported", who,
              (long long)row_offset);
    return EBT_EUNSUPPORTED;
  }
  if (B < 1 || B_pad < B || B_pad % 128 != 0 || n_rows < 1 || d < 1 || d_pad < d ||
      d_pad % 64 != 0 || ld_img < d_pad || k < 1 || kprime < k ||
      kprime > EBT_GROUPED_KPRIME_MAX || kprime % 4 != 0 || chunk_rows < 128 ||
      chunk_rows % 128 != 0 || ((excl_off == nullptr) != (excl_rows == nullptr)) || G < 1 ||
      G > EBT_GROUPS_MAX) {
    set_error("%s: bad arguments (B=%lld B_pad=%lld n=%lld d=%d d_pad=%d k=%d kprime=%d: a "
              "multiple of 4 in [k, %d]; chunk=%lld; G=%d: 1..%d)", who, (long long)B,
              (long long)B_pad, (long long)n_rows, d, d_pad, k, kprime, EBT_GROUPED_KPRIME_MAX,
              (long long)chunk_rows, G, EBT_GROUPS_MAX);
    return EBT_EINVAL;
  }
  int rc = check_table(who, masks, words, n_masks, n_rows);
  if (rc) return rc;
  const GroupedWs L = grouped_ws(B, B_pad, n_rows, kprime, chunk_rows, flags, G);
  if (ws_bytes < L.bytes) {
    set_error("%s: workspace %zu < %zu bytes (ebt_cosine_topk_grouped_workspace)", who, ws_bytes,
              L.bytes);
    return EBT_ENOMEM;
  }
  hipStream_t st = (hipStream_t)stream;
  const PipeArgs a{{q64, qimg, qscale, eps, B, B_pad},
                   {cat, dtype, ld, gnorm64, cimg, cscale, img_dtype, ld_img, n_rows, d, d_pad,
                    row_offset},
                   {excl_off, excl_rows}, k, kprime, chunk_rows, flags};
  char* ws = (char*)workspace;
  float* S = (float*)(ws + L.off_s);
  float* fv = (float*)(ws + L.off_fv);
  int64_t* fi = (int64_t*)(ws + L.off_fi);
  float* lv = L.lists > 1 ? (float*)(ws + L.off_lv) : fv;
  int64_t* li = L.lists > 1 ? (int64_t*)(ws + L.off_li) : fi;
  const int64_t ld_l = L.lists * kprime;
  const float* eps_use = eps;
  if (exact) {  // the float64 screen's bound replaces the caller's eps
    float* xeps = (float*)(ws + L.off_eps);
    rc = fill_exact_eps(xeps, B, st);
    if (rc) return rc;
    eps_use = xeps;
  }
  for (int64_t ch = 0; ch < L.n_chunks; ++ch) {
    const int64_t c0 = ch * L.chunk;
    const int64_t nc = n_rows - c0 < L.chunk ? n_rows - c0 : L.chunk;
    rc = score_chunk(a, c0, nc, S, L.ld_s, timer, st);
    if (rc) return rc;
    StageScope s(timer, EBT_STAGE_SELECT, st);
    rc = select_grouped(S, L.ld_s, B, nc, c0, masks, words, n_masks, groups, G, kprime, L.segs,
                        lv + ch * L.segs * kprime, li + ch * L.segs * kprime, ld_l, st);
    if (rc) return rc;
  }
  if (L.lists > 1) {  // every (group, query)'s per-chunk, per-segment lists -> its k' best
    StageScope s(timer, EBT_STAGE_MERGE_SELECT, st);
    rc = select_topk(lv, li, ld_l, (int64_t)G * B, ld_l, 0, kprime, 1, fv, fi, kprime, st);
    if (rc) return rc;
  }
  StageScope s(timer, EBT_STAGE_RESCORE, st);
  for (int32_t g = 0; g < G; ++g) {
    const int64_t o = (int64_t)g * B;
    rc = rescore(q64, B, a.c, {fv + o * kprime, fi + o * kprime, kprime, 0}, k, eps_use, nullptr,
                 out_scores + o * k, out_rows + o * k, certified + o,
                 {nullptr, nullptr, a.excl, nullptr, nullptr}, st);
    if (rc) return rc;
  }
  return EBT_OK;
}

}  // extern "C"
