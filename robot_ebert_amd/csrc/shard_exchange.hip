// What the shards of a row-sharded catalog exchange around the rescore (rescore.hip): the merge
// of their partial top-k lists (dense or packed), the pack of a shard's list above the
// catalog-wide floor, and the floor itself (union_floor, floor_pack, certify_cut).
#include "common.h"
#include "internal.h"

namespace ebt {

// ------------------------------------------------------------------------------- merge -----
// The k best of R sorted partial lists per query, (score desc, row asc). Up to MERGE_CAP
// entries are sorted in LDS at once: R k <= MERGE_CAP in one bitonic sort; more ranks in rounds
// that keep the running top k in slots [0, k) and bring the next (MERGE_CAP - k) / k ranks in
// behind it (k <= MERGE_CAP / 2).
constexpr int MERGE_CAP = 8192;

__global__ __launch_bounds__(RTHREADS) void merge_topk_kernel(const double* __restrict__ scores,
                                                               const int64_t* __restrict__ rows,
                                                               int R, int64_t B, int k, int P,
                                                               double* __restrict__ out_s,
                                                               int64_t* __restrict__ out_r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sc = (double*)smem;
  int64_t* rw = (int64_t*)(sc + P);
  const int64_t b = blockIdx.x;
  // fill slots [base, P) with ranks [r0, r0 + m), -inf past them
  auto fill = [&](int base, int r0, int m) {
    const int n = m * k;
    for (int i = base + threadIdx.x; i < P; i += RTHREADS) {
      double s = -__builtin_inf();
      int64_t r = INT64_MAX;
      const int e = i - base;
      if (e < n) {
        const int rr = r0 + e / k, j = e % k;
        const int64_t off = ((int64_t)rr * B + b) * k + j;
        const int64_t row = rows[off];
        if (row >= 0) {
          const double v = scores[off];
          s = (v == v) ? v : -__builtin_inf();
          r = row;
        }
      }
      sc[i] = s;
      rw[i] = r;
    }
    __syncthreads();
  };
  int r0 = R * k <= P ? R : P / k;
  fill(0, 0, r0);
  bitonic_pairs(sc, rw, P);
  const int per = (P - k) / k;
  while (r0 < R) {
    const int m = R - r0 < per ? R - r0 : per;
    fill(k, r0, m);
    bitonic_pairs(sc, rw, P);
    r0 += m;
  }
  for (int j = threadIdx.x; j < k; j += RTHREADS) {
    const int64_t r = rw[j];
    out_s[b * k + j] = r == INT64_MAX ? __builtin_nan("") : sc[j];
    out_r[b * k + j] = r == INT64_MAX ? -1 : r;
  }
}

// The same merge by co-ranks when every list is sorted (what ebt_cosine_topk returns): the
// position of entry j of list r in the merged order is j + the entries of the other lists that
// precede it (binary search in each: (score desc, row asc); equal keys -- the -inf/-1 padding --
// ordered by list). Only a prefix of each list can reach the top k: with kr = ceil(k / R), the
// R kr entries at list positions < kr all precede-or-equal m0 = the LAST of the R entries at
// position kr - 1, so the k-th best does too, and an entry after m0 is in no top k. Entries up
// to m0 (about k + R per query on untied data, of the R k) are placed by R - 1 searches within
// the other lists' prefixes, instead of a bitonic network over next_pow2(R k) slots (log^2
// stages of 16-byte LDS swaps). A list found unsorted sends the query down the bitonic network
// (same result).
constexpr int MERGE_CORANK_CAP = 8192;   // R k entries in LDS (16 B each)
constexpr int MERGE_CORANK_RMAX = 1024;  // lists (a 4-byte prefix length each in LDS)

__device__ __forceinline__ bool mt_before(double xs, int64_t xr, double es, int64_t er) {
  return xs > es || (xs == es && xr < er);
}

static size_t merge_corank_lds(int R, int P) {
  return (size_t)P * 16 + RTHREADS * 16 + (((size_t)(2 * R + 1) * 4 + 15) & ~(size_t)15);
}

// The lists' sources. DenseSrc (merge_topk_corank_kernel): [R][B][k] f64 scores + i64 rows
// (row < 0 = padding). PackedSrc (merge_packed_kernel): every rank's packed list of
// ebt_shard_pack (one all-gathered byte buffer, `stride` bytes per rank): u32 start[B], u32
// len[B] (+ scratch), then f64 scores[cap], then i32 rows[cap]; query b's entries are
// [start[b], start[b] + len[b]) clipped to cap (the rest was not sent).
struct DenseSrc {
  const double* scores;
  const int64_t* rows;
};
struct PackedSrc {
  const char* recv;
  int64_t stride, cap;
};

__device__ __forceinline__ const uint32_t* pk_starts(const PackedSrc& p, int r) {
  return (const uint32_t*)(p.recv + (int64_t)r * p.stride);
}
__device__ __forceinline__ const uint32_t* pk_lens(const PackedSrc& p, int r, int64_t B) {
  return (const uint32_t*)(p.recv + (int64_t)r * p.stride) + B;
}
__device__ __forceinline__ const double* pk_scores(const PackedSrc& p, int r, int64_t B) {
  return (const double*)(p.recv + (int64_t)r * p.stride + shard_pack_hdr_bytes(B));
}
__device__ __forceinline__ const int32_t* pk_rows(const PackedSrc& p, int r, int64_t B) {
  return (const int32_t*)(p.recv + (int64_t)r * p.stride + shard_pack_hdr_bytes(B) + p.cap * 8);
}

template <class Src>
__global__ __launch_bounds__(RTHREADS) void merge_topk_corank_kernel(
    const Src src, int R, int64_t B, int k, int P, double* __restrict__ out_s,
    int64_t* __restrict__ out_r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = R * k;
  double* sc = (double*)smem;
  int64_t* rw = (int64_t*)(sc + P);   // P = next_pow2(n) >= n
  double* red_s = (double*)(rw + P);
  int64_t* red_r = (int64_t*)(red_s + RTHREADS / 2);
  int* plen = (int*)(red_r + RTHREADS / 2);
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  // four entries per thread in flight (a loop over e would wait for each load in turn: the
  // compiler peels the trip count's remainder into a serial loop)
  for (int e0 = tid; e0 < n; e0 += 4 * RTHREADS) {
    int64_t rv[4];
    double sv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * RTHREADS;
      const int ec = e < n ? e : n - 1;
      const int rr = ec / k, j = ec - rr * k;
      const int64_t off = ((int64_t)rr * B + b) * k + j;
      rv[u] = src.rows[off];
      sv[u] = src.scores[off];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * RTHREADS;
      issued(rv[u]);
      issued(sv[u]);
      if (e < n) {
        const bool pad = rv[u] < 0;
        sc[e] = pad || sv[u] != sv[u] ? -__builtin_inf() : sv[u];
        rw[e] = pad ? INT64_MAX : rv[u];
      }
    }
  }
  __syncthreads();
  int bad = 0;
  for (int e = tid; e < n; e += RTHREADS) {
    const int j = e % k;
    if (j + 1 < k && mt_before(sc[e + 1], rw[e + 1], sc[e], rw[e])) bad = 1;
  }
  if (__syncthreads_or(bad)) {
    // unsorted input: the bitonic network over P >= n slots
    for (int e = n + tid; e < P; e += RTHREADS) {
      sc[e] = -__builtin_inf();
      rw[e] = INT64_MAX;
    }
    __syncthreads();
    bitonic_pairs(sc, rw, P);
    for (int j = tid; j < k; j += RTHREADS) {
      const int64_t r = rw[j];
      out_s[b * k + j] = r == INT64_MAX ? __builtin_nan("") : sc[j];
      out_r[b * k + j] = r == INT64_MAX ? -1 : r;
    }
    return;
  }
  // m0: the last (in merged order) of the lists' entries at position kr - 1; then each list's
  // prefix of entries preceding-or-equal m0 (plen) and the prefixes' starts (cst) in the
  // compact enumeration of the candidates
  const int kr = (k + R - 1) / R;
  int* cst = plen + R;   // R + 1
  if (R <= 64) {
    // one wave, no barriers: lane r < R owns list r. Padding (row -1: a shard with fewer than
    // k rows above the floor cut -- at C3/8 about 18 of a list's 100) sorts last and is never a
    // candidate: V_r = the list's entries before its first padding entry. When at least k
    // entries lie in the "long" lists' first kr (V_r >= kr), m0 = the last of those lists'
    // kr-th entries bounds the k-th best as above; otherwise every non-padding entry is a
    // candidate (they are then few) and padding fills the positions past them.
    if (tid < 64) {
      int V = 0;
      if (tid < R) {
        const int64_t* orw = rw + tid * k;
        const double* os = sc + tid * k;
        int lo = 0, hi = k;   // first padding entry (sorted lists: padding is a suffix)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (!(orw[mid] == INT64_MAX && os[mid] == -__builtin_inf())) lo = mid + 1; else hi = mid;
        }
        V = lo;
      }
      const bool is_long = tid < R && V >= kr;
      const int n_long = __popcll(__ballot(is_long));
      double ms = __builtin_inf();
      int64_t mr = -1;   // "before everything": the identity of the max
      if (is_long) {
        ms = sc[tid * k + kr - 1];
        mr = rw[tid * k + kr - 1];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double xs = __shfl_xor(ms, o, 64);
        const int64_t xr = __shfl_xor(mr, o, 64);
        if (mt_before(ms, mr, xs, xr)) {
          ms = xs;
          mr = xr;
        }
      }
      const bool bounded = n_long * kr >= k;
      int len = 0;
      if (tid < R) {
        len = V;
        if (bounded) {
          const double* os = sc + tid * k;
          const int64_t* orw = rw + tid * k;
          int lo = is_long ? kr : 0, hi = V;   // long lists: positions < kr are <= m0
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (!mt_before(ms, mr, os[mid], orw[mid])) lo = mid + 1; else hi = mid;
          }
          len = lo;
        }
      }
      int incl = len;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (tid >= o) incl += y;
      }
      if (tid < R) {
        plen[tid] = len;
        cst[tid] = incl - len;
      }
      if (tid == 63) cst[R] = incl;
    }
  } else {
    double ms = __builtin_inf();
    int64_t mr = -1;
    for (int r = tid; r < R; r += RTHREADS) {
      const double xs = sc[r * k + kr - 1];
      const int64_t xr = rw[r * k + kr - 1];
      if (mt_before(ms, mr, xs, xr)) {
        ms = xs;
        mr = xr;
      }
    }
    for (int h = RTHREADS / 2; h >= 1; h >>= 1) {
      if (tid >= h && tid < 2 * h) {
        red_s[tid - h] = ms;
        red_r[tid - h] = mr;
      }
      __syncthreads();
      if (tid < h && mt_before(ms, mr, red_s[tid], red_r[tid])) {
        ms = red_s[tid];
        mr = red_r[tid];
      }
      __syncthreads();
    }
    if (tid == 0) {
      red_s[0] = ms;
      red_r[0] = mr;
    }
    __syncthreads();
    ms = red_s[0];
    mr = red_r[0];
    for (int r = tid; r < R; r += RTHREADS) {
      const double* os = sc + r * k;
      const int64_t* orw = rw + r * k;
      int lo = kr, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!mt_before(ms, mr, os[mid], orw[mid])) lo = mid + 1; else hi = mid;
      }
      plen[r] = lo;
    }
    __syncthreads();
    if (tid == 0) {
      int c = 0;
      for (int r = 0; r < R; ++r) {
        cst[r] = c;
        c += plen[r];
      }
      cst[R] = c;
    }
  }
  __syncthreads();
  // candidate c -> (list rr, position j): one candidate per thread, so a wave's searches run
  // side by side instead of once per list position the wave strides over
  const int C = cst[R];
  for (int c = tid; c < C; c += RTHREADS) {
    int lo = 0, hi = R - 1;   // the last list whose start <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cst[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int rr = lo, j = c - cst[rr];
    const int e = rr * k + j;
    const double es = sc[e];
    const int64_t er = rw[e];
    int pos = j;
    for (int o = 0; o < R && pos < k; ++o) {
      if (o == rr) continue;
      const double* os = sc + o * k;
      const int64_t* orw = rw + o * k;
      // entries of list o before e: those preceding it, and equal ones when o < rr
      int lo2 = 0, hi2 = plen[o];
      while (lo2 < hi2) {
        const int mid = (lo2 + hi2) >> 1;
        const bool before = mt_before(os[mid], orw[mid], es, er) ||
                            (o < rr && os[mid] == es && orw[mid] == er);
        if (before) lo2 = mid + 1; else hi2 = mid;
      }
      pos += lo2;
    }
    if (pos < k) {
      out_s[b * k + pos] = er == INT64_MAX ? __builtin_nan("") : es;
      out_r[b * k + pos] = er == INT64_MAX ? -1 : er;
    }
  }
  // fewer candidates than k (all of them non-padding): padding takes the rest
  for (int j = C + tid; j < k; j += RTHREADS) {
    out_s[b * k + j] = __builtin_nan("");
    out_r[b * k + j] = -1;
  }
}

// ebt_merge_packed: the co-rank merge over the packed lists as they are -- each rank's entries
// of query b (about k / R + the floor's band of them, instead of k slots mostly padding) staged
// compactly in LDS, then every entry placed at j + (entries of the other lists before it), by
// a binary search in each (score desc, row asc; equal keys ordered by list). A list found
// unsorted flags the batch incomplete (the caller merges the full lists instead): the packed
// lists come sorted from ebt_shard_pack.
// The entries one query's LDS holds: R k (every rank sending all of its k) is what a query can
// receive, but a query's entries above the catalog-wide floor number about k + the floor's band
// over all ranks together, so the room is min(R k, 2 k + 256) and a query with more (a band
// wider than k + 256: clustered data) flags the batch incomplete -- the caller's full exchange,
// as for a list cut by its capacity. At C5/8 (R 8, k 1000) that is 27 KiB instead of 94 KiB of
// LDS per query: five waves per CU instead of one for the binary searches' LDS latency.
__host__ __device__ inline int merge_packed_room(int R, int k) {
  const int64_t all = (int64_t)R * k, room = 2LL * k + 256;
  return (int)(all < room ? all : room);
}
static size_t merge_packed_lds(int R, int k) {
  const size_t n = (size_t)merge_packed_room(R, k);
  return n * 8 + ((n * 4 + 15) & ~(size_t)15) + (((size_t)(3 * R + 1) * 4 + 15) & ~(size_t)15);
}

// one wave per query: 4096 queries all resident at once (16 workgroups per CU by their ~10 KiB of
// LDS at C3/8) instead of two rounds of 256-thread workgroups, each query's chain of dependent
// loads paid once
constexpr int MP_THREADS = 64;
__global__ __launch_bounds__(MP_THREADS) void merge_packed_kernel(
    const PackedSrc src, int R, int64_t B, int k, double* __restrict__ out_s,
    int64_t* __restrict__ out_r, int32_t* __restrict__ incomplete) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nmax = merge_packed_room(R, k);
  double* sc = (double*)smem;                                  // nmax
  int32_t* rw = (int32_t*)(sc + nmax);                         // nmax
  int* pst = (int*)((char*)rw + (((size_t)nmax * 4 + 15) & ~(size_t)15));  // R: packed start
  int* len = pst + R;                                          // R: entries sent
  int* off = len + R;                                          // R + 1: compact starts
  __shared__ int wsum[MP_THREADS / 64];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 1. each rank's entries for this query (a list cut by its rank's capacity, or longer than
  //    k, makes the batch incomplete), and their compact starts (a block scan over the ranks)
  int carry = 0;
  for (int r0 = 0; r0 < R; r0 += MP_THREADS) {
    const int r = r0 + tid;
    int v = 0;
    if (r < R) {
      const int64_t s0 = pk_starts(src, r)[b], s1 = s0 + pk_lens(src, r, B)[b];
      const int64_t a = s0 < src.cap ? s0 : src.cap, e = s1 < src.cap ? s1 : src.cap;
      v = (int)(e - a < k ? e - a : k);
      pst[r] = (int)a;
      len[r] = v;
      if (s1 > src.cap || s1 - s0 > k) incomplete[0] = 1;
    }
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = carry, total = 0;
#pragma unroll
    for (int w = 0; w < MP_THREADS / 64; ++w) {
      base += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    if (r < R) off[r] = base + incl - v;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) off[R] = carry;
  __syncthreads();
  const int N = carry;
  if (N > nmax) {   // more than the query's room (merge_packed_room): the full exchange
    if (tid == 0) incomplete[0] = 1;
    return;
  }
  auto list_of = [&](int e) {   // the last list whose compact start is <= e (a non-empty one)
    int lo = 0, hi = R - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  // 2. the entries into LDS, four per thread in flight
  for (int e0 = tid; e0 < N; e0 += 4 * MP_THREADS) {
    double sv[4];
    int32_t rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * MP_THREADS;
      const int ec = e < N ? e : N - 1;
      const int rr = list_of(ec);
      const int64_t ix = (int64_t)pst[rr] + (ec - off[rr]);
      sv[u] = pk_scores(src, rr, B)[ix];
      rv[u] = pk_rows(src, rr, B)[ix];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * MP_THREADS;
      issued(sv[u]);
      if (e < N) {
        sc[e] = sv[u] != sv[u] ? -__builtin_inf() : sv[u];
        rw[e] = rv[u];
      }
    }
  }
  __syncthreads();
  // 3. sorted lists only
  int bad = 0;
  for (int e = tid; e < N; e += MP_THREADS) {
    const int rr = list_of(e);
    if (e + 1 < off[rr] + len[rr] && mt_before(sc[e + 1], rw[e + 1], sc[e], rw[e])) bad = 1;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) incomplete[0] = 1;
    return;
  }
  // 4. positions: j + the entries of every other list before this one
  for (int e = tid; e < N; e += MP_THREADS) {
    const int rr = list_of(e);
    const double es = sc[e];
    const int64_t er = rw[e];
    int pos = e - off[rr];
    for (int o = 0; o < R && pos < k; ++o) {
      if (o == rr) continue;
      int lo = off[o], hi = off[o] + len[o];
      const int o0 = lo;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool before = mt_before(sc[mid], rw[mid], es, er) ||
                            (o < rr && sc[mid] == es && (int64_t)rw[mid] == er);
        if (before) lo = mid + 1; else hi = mid;
      }
      pos += lo - o0;
    }
    if (pos < k) {
      out_s[b * k + pos] = es;
      out_r[b * k + pos] = er;
    }
  }
  // fewer entries than k: padding takes the rest
  for (int j = N + tid; j < k; j += MP_THREADS) {
    out_s[b * k + j] = __builtin_nan("");
    out_r[b * k + j] = -1;
  }
}

int merge_topk(const double* scores, const int64_t* rows, int32_t R, int64_t B, int32_t k,
               double* out_s, int64_t* out_r, hipStream_t st) {
  if (!scores || !rows || !out_s || !out_r || R < 1 || B < 0 || k < 1 || k > MERGE_CAP / 2) {
    set_error("ebt_merge_topk: bad arguments (R=%d k=%d; k must be <= %d)", R, k, MERGE_CAP / 2);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const int64_t n = (int64_t)R * k;
  if (R > 1 && R <= MERGE_CORANK_RMAX && n <= MERGE_CORANK_CAP) {
    const int P = next_pow2_h((int)n);
    const size_t lds = merge_corank_lds(R, P);
    set_max_lds((const void*)merge_topk_corank_kernel<DenseSrc>, (int)lds);
    hipLaunchKernelGGL(merge_topk_corank_kernel<DenseSrc>, dim3((unsigned)B), dim3(RTHREADS),
                       lds, st, DenseSrc{scores, rows}, R, B, k, P, out_s, out_r);
    return launch_check("merge_topk_corank_kernel");
  }
  const int P = next_pow2_h((int)(n < MERGE_CAP ? n : MERGE_CAP));
  set_max_lds((const void*)merge_topk_kernel, (int)(P * 16));
  hipLaunchKernelGGL(merge_topk_kernel, dim3((unsigned)B), dim3(RTHREADS), (size_t)P * 16, st,
                     scores, rows, R, B, k, P, out_s, out_r);
  return launch_check("merge_topk_kernel");
}

// ------------------------------------------------------------------------ compact exchange --
// ebt_shard_pack: per query the prefix of its sorted exact list with score >= t_floor[b] (a
// lower bound of the k-th best exact score over the whole catalog: every global top-k entry is
// in it), packed behind per-query starts. Two launches: (1) one thread per query counts its
// prefix (binary search: the predicate "real row and score >= floor" holds on a prefix of a
// sorted list), a workgroup scan gives the starts within its 256 queries and its total;
// (2) each workgroup adds the totals of the workgroups before it, writes the global starts and
// copies its entries (one per thread, the owning query found by binary search in LDS).
__global__ __launch_bounds__(SHARD_PACK_QPB) void shard_pack_count_kernel(
    const double* __restrict__ scores, const int64_t* __restrict__ rows, int64_t B, int k,
    const double* __restrict__ t_floor, uint32_t* __restrict__ hdr) {
  __shared__ int wsum[SHARD_PACK_QPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = (int64_t)blockIdx.x * SHARD_PACK_QPB + tid;
  int cnt = 0;
  if (b < B) {
    const double tf = t_floor ? t_floor[b] : -__builtin_inf();
    const double* sr = scores + b * k;
    const int64_t* rr = rows + b * k;
    // the first position failing the predicate (it holds on a prefix), by an 8-way search:
    // each round trip loads up to 8 evenly spaced probes of [lo, hi) at once and keeps the gap
    // between the last probe passing and the first failing (k = 100: three round trips, not 7)
    int lo = 0, hi = k;
    while (lo < hi) {
      const int span = hi - lo, m = span < 8 ? span : 8;
      int p[8];
      int64_t pr[8];
      double ps[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        p[i] = lo + (int)((int64_t)(i + 1) * span / (m + 1));
        const int pc = i < m ? p[i] : lo;
        pr[i] = rr[pc];
        ps[i] = sr[pc];
      }
      int nlo = lo, nhi = hi;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i >= m) continue;
        if (pr[i] >= 0 && ps[i] >= tf) nlo = p[i] + 1 > nlo ? p[i] + 1 : nlo;
        else nhi = p[i] < nhi ? p[i] : nhi;
      }
      lo = nlo;
      hi = nhi;
    }
    cnt = lo;
  }
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < SHARD_PACK_QPB / 64; ++w) {
    base += w < wave ? wsum[w] : 0;
    total += wsum[w];
  }
  if (b < B) hdr[b] = (uint32_t)(base + incl - cnt);  // start within the workgroup
  if (tid == 0) hdr[2 * B + blockIdx.x] = (uint32_t)total;
}

// (64 queries per workgroup -- 64 workgroups at B = 4096, not 16 -- and SHARD_PACK_COPY_THREADS
// threads: a workgroup's ~15 x 64 entries at C3/8 in four rounds)
constexpr int SHARD_PACK_COPY_THREADS = 256;
__global__ __launch_bounds__(SHARD_PACK_COPY_THREADS) void shard_pack_copy_kernel(
    const double* __restrict__ scores, const int64_t* __restrict__ rows, int64_t B, int k,
    int64_t cap, char* __restrict__ send) {
  __shared__ uint32_t lst[SHARD_PACK_QPB + 1];
  __shared__ uint32_t gbase;
  uint32_t* hdr = (uint32_t*)send;
  double* os = (double*)(send + shard_pack_hdr_bytes(B));
  int32_t* orow = (int32_t*)(send + shard_pack_hdr_bytes(B) + cap * 8);
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * SHARD_PACK_QPB;
  const int nq = B - q0 < SHARD_PACK_QPB ? (int)(B - q0) : SHARD_PACK_QPB;
  const uint32_t* tot = hdr + 2 * B;
  if (tid < 64) {  // the totals of the workgroups before this one
    uint32_t s = 0;
    for (int i = tid; i < (int)blockIdx.x; i += 64) s += tot[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (tid == 0) gbase = s;
  }
  if (tid < nq) lst[tid] = hdr[q0 + tid];
  if (tid == 0) lst[nq] = tot[blockIdx.x];
  __syncthreads();
  const uint32_t g0 = gbase, n = lst[nq];
  if (tid < nq) {
    hdr[q0 + tid] = g0 + lst[tid];                // start
    hdr[B + q0 + tid] = lst[tid + 1] - lst[tid];  // len
  }
  for (uint32_t t = tid; t < n; t += SHARD_PACK_COPY_THREADS) {
    int lo = 0, hi = nq - 1;  // the last query whose start <= t
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (lst[mid] <= t) lo = mid;
      else hi = mid - 1;
    }
    const int64_t b = q0 + lo, j = t - lst[lo], pos = (int64_t)g0 + t;
    if (pos < cap) {
      os[pos] = scores[b * k + j];
      orow[pos] = (int32_t)rows[b * k + j];
    }
  }
}

// The pack's second half when the sharded rescore counted already (len[b] in the header): each
// workgroup's base is the sum of len over the queries before it (at most B values, L2-resident:
// no block totals, so no counting launch), then the starts and the copy as shard_pack_copy_kernel.
__global__ __launch_bounds__(SHARD_PACK_COPY_THREADS) void shard_pack_lens_kernel(
    const double* __restrict__ scores, const int64_t* __restrict__ rows, int64_t B, int k,
    int64_t cap, char* __restrict__ send) {
  __shared__ uint32_t lst[SHARD_PACK_QPB + 1];
  __shared__ uint32_t part[SHARD_PACK_COPY_THREADS / 64];
  uint32_t* hdr = (uint32_t*)send;
  const uint32_t* len = hdr + B;
  double* os = (double*)(send + shard_pack_hdr_bytes(B));
  int32_t* orow = (int32_t*)(send + shard_pack_hdr_bytes(B) + cap * 8);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * SHARD_PACK_QPB;
  const int nq = B - q0 < SHARD_PACK_QPB ? (int)(B - q0) : SHARD_PACK_QPB;
  uint32_t sum = 0;   // the queries before this workgroup's
  for (int64_t i = tid; i < q0; i += SHARD_PACK_COPY_THREADS) sum += len[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) part[wave] = sum;
  if (wave == 0) {    // this workgroup's queries: an inclusive scan of their lens
    uint32_t v = lane < nq ? len[q0 + lane] : 0u;
    const uint32_t incl = wave_scan_add_u32(v);
    lst[lane + 1] = incl;
    if (lane == 0) lst[0] = 0u;
  }
  __syncthreads();
  uint32_t g0 = 0;
#pragma unroll
  for (int w = 0; w < SHARD_PACK_COPY_THREADS / 64; ++w) g0 += part[w];
  const uint32_t n = lst[nq];
  if (tid < nq) hdr[q0 + tid] = g0 + lst[tid];   // start
  for (uint32_t t = tid; t < n; t += SHARD_PACK_COPY_THREADS) {
    int lo = 0, hi = nq - 1;  // the last query whose start <= t (an empty one is skipped)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (lst[mid] <= t) lo = mid;
      else hi = mid - 1;
    }
    const int64_t b = q0 + lo, j = t - lst[lo], pos = (int64_t)g0 + t;
    if (pos < cap) {
      os[pos] = scores[b * k + j];
      orow[pos] = (int32_t)rows[b * k + j];
    }
  }
}

int shard_pack_lens(const double* scores, const int64_t* rows, int64_t B, int32_t k,
                    int64_t cap, void* send, hipStream_t st) {
  hipLaunchKernelGGL(shard_pack_lens_kernel, dim3((unsigned)ceil_div(B, SHARD_PACK_QPB)),
                     dim3(SHARD_PACK_COPY_THREADS), 0, st, scores, rows, B, k, cap, (char*)send);
  return launch_check("shard_pack_lens_kernel");
}

static int64_t shard_list_width(int32_t k, int32_t world) {
  const int64_t w = (3 * (int64_t)k + 2 * world - 1) / (2 * world) + 8;  // ceil(1.5 k / R) + 8
  return w < k ? w : k;
}

// ---------------------------------------------------------------------------------------------
// Row-sharded per-shard path (distributed.py), after the floor all-gather: the catalog-wide floor
// and the certificate adjustment in two launches instead of ~17 small torch ops.
// union_floor: g = [R][B][ld] f32 (the shards' k best approx in columns [0, ld-1), their eps in
// column ld-1); t_floor[b] = the k-th largest of g[r][b][j] - g[r][b][ld-1] over r, j (float64,
// exact differences of two floats; NaN counts as -inf). One wave per query: bisection over the
// order-preserving 64-bit keys of the doubles, counts by a strided pass over the R*(ld-1) values.

__global__ __launch_bounds__(256) void union_floor_kernel(const float* __restrict__ g, int R,
                                                          int64_t B, int ld, int k,
                                                          double* __restrict__ t_floor,
                                                          uint32_t* __restrict__ zero2) {
  if (zero2 && blockIdx.x == 0 && threadIdx.x < 2) zero2[threadIdx.x] = 0u;
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int per = ld - 1, n = R * per;
  auto val = [&](int i) {
    const int r = i / per, j = i - r * per;
    const float* row = g + ((int64_t)r * B + b) * ld;
    return (double)row[j] - (double)row[per];
  };
  auto count_ge = [&](uint64_t t) {
    int c = 0;
    for (int i = lane; i < n; i += 64) c += f64_key(val(i)) >= t ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
  };
  // the largest key t with count(key >= t) >= k (key 0 = NaN / below everything)
  uint64_t lo = 0ull, hi = ~0ull;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1) + 1;
    if (count_ge(mid) >= k) lo = mid;
    else hi = mid - 1;
  }
  if (lane == 0) t_floor[b] = lo == 0ull ? -__builtin_inf() : key_f64(lo);
}

// The same bisection with the query's R*(ld-1) keys held in registers (up to 32 per lane), made
// once (all loads issued before the search), and the counts as ballot popcounts: W = 1 (one wave per query, n <= 2048: C3/8 has
// 8 x 100) or 4 (one 256-thread workgroup per query, n <= 8192: C5/8 has 8 x 1000; the waves'
// counts meet in LDS). The strided form above re-read every value from memory, with a
// division, in each of its 64 steps (0.39 ms per 4096-query C3/8 batch).
constexpr int UF_PL = 32;
// PL: key slots per lane, a compile-time bound (the launch picks the smallest of 4/8/16/32 that
// holds n): the count loop is then a fixed sequence of compare + popcount, no per-slot test.
// The bisection bounds are wave-uniform (readfirstlane): a scalar loop.
template <int W, int PL>
__global__ __launch_bounds__(256) void union_floor_reg_kernel(const float* __restrict__ g, int R,
                                                              int64_t B, int ld, int k,
                                                              double* __restrict__ t_floor,
                                                              uint32_t* __restrict__ zero2) {
  // (zero2: two words the caller needs zeroed before its next kernel -- the sharded step's pack
  // counter and "incomplete" flag, one memset launch less per step)
  if (zero2 && blockIdx.x == 0 && threadIdx.x < 2) zero2[threadIdx.x] = 0u;
  __shared__ int wc[2][4];
  __shared__ uint64_t wmm[2][4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t b = W == 1 ? (int64_t)blockIdx.x * 4 + (tid >> 6) : (int64_t)blockIdx.x;
  if (W == 1 && b >= B) return;
  const int per = ld - 1, n = R * per;
  const int t0 = W == 1 ? lane : tid;
  constexpr int STEP = 64 * W;
  if (n < k) {   // fewer values than k: no k-th largest
    if (t0 == 0) t_floor[b] = -__builtin_inf();
    return;
  }
  // every slot's two loads issued before any is used (a guarded load per slot would wait for
  // each in turn): indices past n re-read entry n - 1 and are masked to key 0 afterwards
  float v[PL], ev[PL];
#pragma unroll
  for (int e = 0; e < PL; ++e) {
    const int i0 = t0 + STEP * e, i = i0 < n ? i0 : n - 1;   // entry i: list i / per, i % per
    const int r = i / per, j = i - r * per;
    const float* row = g + ((int64_t)r * B + b) * ld;
    v[e] = row[j];
    ev[e] = row[per];
  }
  uint64_t key[PL];
  uint64_t mn = ~0ull, mx = 0ull;
#pragma unroll
  for (int e = 0; e < PL; ++e) {
    const bool in = t0 + STEP * e < n;
    key[e] = in ? f64_key((double)v[e] - (double)ev[e]) : 0ull;
    if (in) {
      mn = key[e] < mn ? key[e] : mn;
      mx = key[e] > mx ? key[e] : mx;
    }
  }
  // the k-th largest key lies in [min key, max key]: bisect that bracket, not all 64 bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t a = __shfl_xor(mn, o, 64), c = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = c > mx ? c : mx;
  }
  if (W > 1) {
    if (lane == 0) {
      wmm[0][tid >> 6] = mn;
      wmm[1][tid >> 6] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      mn = wmm[0][w] < mn ? wmm[0][w] : mn;
      mx = wmm[1][w] > mx ? wmm[1][w] : mx;
    }
  }
  auto uni = [](uint64_t x) {
    const uint32_t lo32 = __builtin_amdgcn_readfirstlane((uint32_t)x);
    const uint32_t hi32 = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return ((uint64_t)hi32 << 32) | lo32;
  };
  uint64_t lo = uni(mn), hi = uni(mx);   // count(key >= mn) = n >= k
  int parity = 0;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1) + 1;
    int c = 0;
#pragma unroll
    for (int e = 0; e < PL; ++e) c += __popcll(__ballot(key[e] >= mid));
    if (W > 1) {
      if (lane == 0) wc[parity][tid >> 6] = c;
      __syncthreads();
      c = wc[parity][0] + wc[parity][1] + wc[parity][2] + wc[parity][3];
      parity ^= 1;   // the other buffer next step: no second barrier before the next write
    }
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= k) lo = mid;
    else hi = mid - 1;
  }
  if (t0 == 0) t_floor[b] = lo == 0ull ? -__builtin_inf() : key_f64(lo);
}

// cert[b] = -1 (rerun unfused) when the fused screen overflowed (ovf[b] != 0) or the shared
// threshold may have dropped a global top-k row (theta[b] > t_floor[b] - eps[b]); -2 stays.
__global__ void certify_cut_kernel(int32_t* __restrict__ cert, const int32_t* __restrict__ ovf,
                                   const float* __restrict__ theta,
                                   const double* __restrict__ t_floor,
                                   const float* __restrict__ eps, int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || cert[b] == -2) return;
  bool drop = ovf[b] != 0;
  if (theta) drop |= !((double)theta[b] <= t_floor[b] - (double)eps[b]);
  if (drop) cert[b] = -1;
}

}  // namespace ebt

extern "C" int ebt_union_floor(const float* gathered, int32_t R, int64_t B, int32_t ld, int32_t k,
                               double* t_floor, void* stream) {
  return ebt::union_floor(gathered, R, B, ld, k, t_floor, (hipStream_t)stream, nullptr);
}
int ebt::union_floor(const float* gathered, int32_t R, int64_t B, int32_t ld, int32_t k,
                     double* t_floor, hipStream_t stream, uint32_t* zero2) {
  if (!gathered || !t_floor || R < 1 || B < 0 || ld < 2 || k < 1 || (int64_t)R * (ld - 1) > (1 << 30)) {
    set_error("ebt_union_floor: bad arguments (R=%d B=%lld ld=%d k=%d)", R, (long long)B, ld, k);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const int64_t n = (int64_t)R * (ld - 1);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 g1((unsigned)ceil_div(B, 4)), g4((unsigned)B), blk(256);
#define EBT_UF(W, PL, G)                                                                       \
  {                                                                                           \
    hipLaunchKernelGGL((union_floor_reg_kernel<W, PL>), G, blk, 0, st, gathered, R, B, ld, k, \
                       t_floor, zero2);                                                       \
    return launch_check("union_floor_reg_kernel");                                            \
  }
  if (n <= 64 * 4) EBT_UF(1, 4, g1)
  if (n <= 64 * 8) EBT_UF(1, 8, g1)
  if (n <= 64 * 16) EBT_UF(1, 16, g1)
  if (n <= 64 * UF_PL) EBT_UF(1, 32, g1)
  if (n <= 256 * 16) EBT_UF(4, 16, g4)
  if (n <= 256 * UF_PL) EBT_UF(4, 32, g4)
#undef EBT_UF
  hipLaunchKernelGGL(union_floor_kernel, dim3((unsigned)ceil_div(B, 4)), dim3(256), 0,
                     (hipStream_t)stream, gathered, R, B, ld, k, t_floor, zero2);
  return launch_check("union_floor_kernel");
}

extern "C" int ebt_certify_cut(int32_t* cert, const int32_t* ovf, const float* theta,
                               const double* t_floor, const float* eps, int64_t B, void* stream) {
  using namespace ebt;
  if (!cert || !ovf || B < 0 || (theta && (!t_floor || !eps))) {
    set_error("ebt_certify_cut: bad arguments");
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  hipLaunchKernelGGL(certify_cut_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0,
                     (hipStream_t)stream, cert, ovf, theta, t_floor, eps, B);
  return launch_check("certify_cut_kernel");
}

extern "C" int64_t ebt_shard_list_width(int32_t k, int32_t world) {
  if (k < 1 || world < 1) return 0;
  return ebt::shard_list_width(k, world);
}

extern "C" int64_t ebt_shard_pack_cap(int64_t B, int32_t k, int32_t world, int64_t n_global) {
  using namespace ebt;
  // the packed merge holds R k entries in LDS; rows travel as int32
  // (the u32 starts count up to B k entries per rank)
  if (B < 1 || k < 1 || world < 2 || world > MERGE_CORANK_RMAX ||
      (int64_t)world * k > MERGE_CORANK_CAP || n_global >= (1LL << 31) ||
      B * (int64_t)k >= (1LL << 31))
    return 0;
  const int64_t cap = B * shard_list_width(k, world);
  return cap < (1LL << 31) ? cap : 0;
}

extern "C" size_t ebt_shard_pack_bytes(int64_t B, int64_t cap) {
  if (B < 1 || cap < 1) return 0;
  return (size_t)((ebt::shard_pack_hdr_bytes(B) + cap * 12 + 255) & ~(int64_t)255);
}

extern "C" int ebt_shard_pack(const double* scores, const int64_t* rows, int64_t B, int32_t k,
                              const double* t_floor, int64_t cap, void* send, void* stream) {
  using namespace ebt;
  if (!scores || !rows || !send || B < 1 || B >= (1LL << 31) || k < 1 || cap < 1 ||
      cap >= (1LL << 31)) {
    set_error("ebt_shard_pack: bad arguments (B=%lld k=%d cap=%lld)", (long long)B, k,
              (long long)cap);
    return EBT_EINVAL;
  }
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)ceil_div(B, SHARD_PACK_QPB);
  hipLaunchKernelGGL(shard_pack_count_kernel, dim3(grid), dim3(SHARD_PACK_QPB), 0, st, scores,
                     rows, B, k, t_floor, (uint32_t*)send);
  int rc = launch_check("shard_pack_count_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(shard_pack_copy_kernel, dim3(grid), dim3(SHARD_PACK_COPY_THREADS), 0, st,
                     scores, rows, B, k, cap, (char*)send);
  return launch_check("shard_pack_copy_kernel");
}

extern "C" int ebt_merge_packed(const void* recv, int32_t R, int64_t B, int32_t k, int64_t cap,
                                double* out_scores, int64_t* out_rows, int32_t* incomplete,
                                void* stream) {
  using namespace ebt;
  if (!recv || !out_scores || !out_rows || !incomplete || R < 1 || R > MERGE_CORANK_RMAX ||
      B < 1 || k < 1 || cap < 1 || (int64_t)R * k > MERGE_CORANK_CAP) {
    set_error("ebt_merge_packed: bad arguments (R=%d B=%lld k=%d cap=%lld; R k <= %d)", R,
              (long long)B, k, (long long)cap, MERGE_CORANK_CAP);
    return EBT_EINVAL;
  }
  const size_t lds = merge_packed_lds(R, k);
  set_max_lds((const void*)merge_packed_kernel, (int)lds);
  const PackedSrc src{(const char*)recv, (int64_t)ebt_shard_pack_bytes(B, cap), cap};
  hipLaunchKernelGGL(merge_packed_kernel, dim3((unsigned)B), dim3(MP_THREADS), lds,
                     (hipStream_t)stream, src, R, B, k, out_scores, out_rows, incomplete);
  return launch_check("merge_packed_kernel");
}

// ------------------------------------------------------------------------ floor all-gather --
// ebt_floor_pack: out[b] = (the w largest of lv[b][0 .. n), n = min(k_eff, ld), then eps[b]) as
// [B][w + 1] f32 -- what each shard sends for the catalog-wide floor. The list may be
// partitioned (the wave merge's [0, k-1) in any order), so the w largest are selected: one wave
// per query, order-preserving keys in registers, the w-th largest key by bisection (ballot
// counts), then the keys above it and as many equal to it as fit, compacted by ballot prefix.
// Only the multiset of values matters to ebt_union_floor, so ties at the cut may go either way.
namespace ebt {
template <int PL>
__global__ __launch_bounds__(256) void floor_pack_kernel(const float* __restrict__ lv, int64_t ld,
                                                         int64_t B, int n, int w,
                                                         const float* __restrict__ eps,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* src = lv + b * ld;
  float* dst = out + b * (w + 1);
  uint32_t key[PL];
#pragma unroll
  for (int e = 0; e < PL; ++e) {  // clamped loads, all in flight, masked afterwards
    const int j = lane + 64 * e;
    const float v = n > 0 ? src[j < n ? j : n - 1] : 0.f;
    key[e] = j < n ? f2key(v) : 0u;
  }
  uint32_t t = 0u;  // the w-th largest key (0: fewer than w valid values)
  if (n > w) {
    uint32_t mn = ~0u, mx = 0u;
#pragma unroll
    for (int e = 0; e < PL; ++e) {
      if (key[e]) mn = key[e] < mn ? key[e] : mn;
      mx = key[e] > mx ? key[e] : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t a = __shfl_xor(mn, o, 64), c = __shfl_xor(mx, o, 64);
      mn = a < mn ? a : mn;
      mx = c > mx ? c : mx;
    }
    auto count_ge = [&](uint32_t x) {
      int c = 0;
#pragma unroll
      for (int e = 0; e < PL; ++e) c += __popcll(__ballot(key[e] >= x));
      return c;
    };
    mn = __builtin_amdgcn_readfirstlane(mn);
    mx = __builtin_amdgcn_readfirstlane(mx);
    if (count_ge(mn) >= w) {  // else fewer than w valid values: t = 0
      uint32_t lo = mn, hi = mx;  // invariant: count_ge(lo) >= w
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1) + 1u;
        if (count_ge(mid) >= w) lo = mid;
        else hi = mid - 1u;
      }
      t = lo;
    }
  }
  // keys > t first, then keys == t (t > 0), at most w in all; -inf past them
  int base = 0;
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int e = 0; e < PL; ++e) {
      const bool pick = key[e] != 0u && (pass == 0 ? (n <= w || key[e] > t) : (n > w && t != 0u && key[e] == t));
      const uint64_t m = __ballot(pick);
      const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (pick && pos < w) dst[pos] = key2f(key[e]);
      base += __popcll(m);
    }
  }
  for (int j = (base < w ? base : w) + lane; j < w; j += 64) dst[j] = -__builtin_inff();
  if (lane == 0) dst[w] = eps ? eps[b] : -__builtin_inff();
}
}  // namespace ebt

extern "C" int ebt_floor_pack(const float* list_vals, int64_t ld, int64_t B, int32_t k_eff,
                              int32_t w, const float* eps, float* out, void* stream) {
  using namespace ebt;
  if (!list_vals || !out || B < 0 || ld < 1 || k_eff < 0 || w < 1 || k_eff > 4096) {
    set_error("ebt_floor_pack: bad arguments (ld=%lld k_eff=%d w=%d; k_eff <= 4096)",
              (long long)ld, k_eff, w);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const int n = k_eff < ld ? k_eff : (int)ld;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(B, 4)), blk(256);
  if (n < 1) {  // nothing valid: -inf everywhere, then eps (PL = 1 over an empty list)
    hipLaunchKernelGGL((floor_pack_kernel<1>), grid, blk, 0, st, list_vals, ld, B, 0, w, eps, out);
    return launch_check("floor_pack_kernel");
  }
  if (n <= 64 * 4)
    hipLaunchKernelGGL((floor_pack_kernel<4>), grid, blk, 0, st, list_vals, ld, B, n, w, eps, out);
  else if (n <= 64 * 16)
    hipLaunchKernelGGL((floor_pack_kernel<16>), grid, blk, 0, st, list_vals, ld, B, n, w, eps, out);
  else
    hipLaunchKernelGGL((floor_pack_kernel<64>), grid, blk, 0, st, list_vals, ld, B, n, w, eps, out);
  return launch_check("floor_pack_kernel");
}
