// Exact float64 rescore of the screened candidates, final top-k, certification.
//
// The reference's arithmetic is float64 end to end (constants.py:56 builds a float64 DataFrame;
// sklearn keeps float64 unless both inputs are float32, metrics/pairwise.py:67). The screening
// GEMM runs in f16/bf16 MFMA, so its scores are approximations with a per-query error bound
// eps (prep.hip). Here every candidate is recomputed as (q64 . c) / gnorm64(c) in float64 --
// the same value as sklearn's normalize-then-dot up to float64 round-off -- and the k best are
// chosen by (score desc, row asc). The candidate set is PROVABLY a superset of the true top-k
// when approx[k'-1] < approx[k-1] - 2 eps ("certified-margin rescore");
// otherwise certified[b] = 0 and the host retries that query with a larger k'.
#include <atomic>
#include <cstdlib>

#include "common.h"
#include "exact_tile_f64.h"
#include "internal.h"

namespace ebt {

constexpr int RESCORE_RANK_MAX = 512;   // kept rows ordered by counting (else bitonic)

// dst[0, d) = src[0, d) by the workgroup, eight loads per thread in flight (a plain strided loop
// waits for each load before the next); past-the-end slots load entry d - 1 and store nothing.
__device__ __forceinline__ void stage_f64(double* dst, const double* __restrict__ src, int d) {
  for (int j0 = threadIdx.x; j0 < d; j0 += 8 * RTHREADS) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u * RTHREADS;
      v[u] = src[j < d ? j : d - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u * RTHREADS;
      issued(v[u]);
      if (j < d) dst[j] = v[u];
    }
  }
}

// Sum of q . row over one lane's share of the row (16-byte chunks ch = lane, lane+64, ...),
// accumulated in chunk order; the caller's wave_sum_f64 completes the dot product. q: the query
// values of the chunk's elements, in LDS (qs + ch * PER) or in the lane's registers (qv[u]) --
// one expression, so the same contracted FMA chain and the same bits either way.
template <int DT>
__device__ __forceinline__ double chunk_dot(const double* q, uint4 raw) {
  double s = 0.0;
  if constexpr (DT == EBT_F32) {
    const float* f = (const float*)&raw;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += q[e] * (double)f[e];
  } else if constexpr (DT == EBT_F64) {
    const double* f = (const double*)&raw;
    s += q[0] * f[0] + q[1] * f[1];
  } else {
    const uint16_t* h = (const uint16_t*)&raw;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      s += q[e] * (DT == EBT_BF16 ? bf16_bits_to_f64(h[e]) : f16_bits_to_f64(h[e]));
  }
  return s;
}

// Rows per wave round trip of the register-query form, by chunks per lane (NU): about eight
// 16-byte loads per lane in flight (C2 / C4: NU = 2 -> 4 rows; C5: 3 -> 2; C3: 6 -> 2)
#ifndef EBT_RESCORE_NR_WIDE
#define EBT_RESCORE_NR_WIDE 2  // rows per trip at 3..6 chunks per lane (build knob for A/B)
#endif
#ifndef EBT_RESCORE_NR_NARROW
#define EBT_RESCORE_NR_NARROW 4  // rows per trip at <= 2 chunks per lane (build knob for A/B)
#endif
template <int NU>
constexpr int rescore_rows_per_trip() {
  return NU <= 2 ? EBT_RESCORE_NR_NARROW : (NU <= 6 ? EBT_RESCORE_NR_WIDE : 1);
}

// NU = 0: the query staged in LDS (any d), two rows per wave round trip. NU > 0 (VEC, d / PER
// <= 64 NU 16-byte chunks): each lane keeps its chunks' query values (chunks lane + 64 u) in
// registers for every row -- no LDS reads in the dot products, no query staging -- and gathers
// rescore_rows_per_trip<NU>() rows per round trip from per-pass row lists. Per row the same
// chunk order, the same per-chunk sums and the same wave butterfly: bitwise the same scores.
#ifdef EBT_RESCORE_STAMP
// Diagnostic build only: shader cycles of each phase of a query's rescore workgroup (wave 0's
// view): [0] query + list + compaction, [1] pass A, [2] s_min + pass B's list, [3] pass B,
// [4] order + write; g_rstamp[5 b ..] (vector stores; nothing else reads them).
__device__ unsigned long long* g_rstamp;
extern "C" int ebt_debug_rescore_stamps(unsigned long long* buf) {
  return hip_check(hipMemcpyToSymbol(HIP_SYMBOL(g_rstamp), &buf, sizeof(buf)), "hipMemcpyToSymbol");
}
#define RST(i) rs[i] = __builtin_amdgcn_s_memtime()
#else
#define RST(i)
#endif
// (f32 rows with the query held in registers at d = 1536, C3's variant: 138 VGPRs would give
// three waves per SIMD; bounded to 128 -- no spill -- it runs four, a quarter more row gathers
// in flight. The other variants are at four or more already, or would spill under the bound.)
template <int DT, bool VEC, int NU = 0>
__global__ __launch_bounds__(RTHREADS, (DT == EBT_F32 && NU == 6) ? 4 : 1) void rescore_kernel(
    const double* __restrict__ q64, int d, const void* __restrict__ cat, int64_t ld,
    const double* __restrict__ gnorm, int64_t row_offset, const float* __restrict__ cand_vals,
    const int64_t* __restrict__ cand_rows, int kprime, int kpp, int k, int64_t n_rows,
    const float* __restrict__ eps, const double* __restrict__ t_floor, double* __restrict__ out_s,
    int64_t* __restrict__ out_r, int32_t* __restrict__ certified, const int* __restrict__ ovf_cnt,
    int ovf_cap, unsigned long long* __restrict__ gathered, int64_t list_base,
    const float* __restrict__ theta, const int64_t* __restrict__ excl_off,
    const int64_t* __restrict__ excl_rows, const ShardPackOut pack) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* qs = (double*)smem;                           // d (NU = 0 only)
  double* sc = qs + (NU > 0 ? 0 : ((d + 1) & ~1));      // kpp: approx, then exact
  int64_t* rw = (int64_t*)(sc + kpp);         // kpp
  int* pl = (int*)(rw + kpp);                 // kpp: list position of each kept row
  int* ix = pl + kpp;                         // kpp (NU > 0): the rows of the current pass
  __shared__ int nvalid, corrupt, nkeep, ntop, nsel, ngath, xbad, npk;
  __shared__ unsigned long long smin_key;
  constexpr int NW = RTHREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
#ifdef EBT_RESCORE_STAMP
  unsigned long long rs[6] = {0, 0, 0, 0, 0, 0};
#endif
  RST(0);
  if (tid == 0) {
    nvalid = 0;
    corrupt = 0;
    nkeep = 0;
    ntop = 0;
    nsel = 0;
    ngath = 0;
    xbad = 0;
    npk = 0;
    smin_key = ~0ull;
  }
  constexpr int ES = (DT == EBT_F64) ? 8 : (DT == EBT_F32 ? 4 : 2);
  constexpr int PER = 16 / ES;
  // the query's exclusion segment must be sorted ascending (the merges drop excluded rows by
  // binary search): checked here, one pass over its few rows, certified = -3 otherwise -- the
  // C entry's separate check kernel and flag memset folded into the kernel that writes the
  // certificate (set after the barrier below, read after the next)
  bool xb = false;
  if (excl_off) {
    const int64_t xs = excl_off[b], xe = excl_off[b + 1];
    xb = xe < xs;
    for (int64_t t = xs + tid; t + 1 < xe; t += RTHREADS) xb |= excl_rows[t] > excl_rows[t + 1];
  }
  // NU > 0: the lane's query values of chunks lane + 64 u (0 past the row)
  double qv[NU > 0 ? NU : 1][PER];
  if constexpr (NU > 0) {
    const int nch = d / PER;
    const double* qrow = q64 + b * d;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ch = lane + 64 * u;
      const int cc = ch < nch ? ch : 0;  // clamped, so that every load is issued up front
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const double x = qrow[cc * PER + e];
        qv[u][e] = ch < nch ? x : 0.0;
      }
    }
  } else {
    stage_f64(qs, q64 + b * d, d);
  }
  const int64_t* cr = cand_rows + b * kprime;
  // Candidates whose approx score is below approx[k-1] - 2 eps cannot be in the top k (the k
  // best candidates all have exact >= approx[k-1] - eps > their exact), so their rows are not
  // gathered: about k + (rows in the 2 eps band) of the k' candidates are rescored.
  // t_floor (optional): a lower bound of the k-th best EXACT score over the whole (sharded)
  // catalog, e.g. max over shards of (shard's approx[k-1] - eps). A row of the global top k has
  // exact >= t_floor, so approx >= t_floor - eps: the cut may rise to that.
  const float* cv = cand_vals + b * kprime;
  double cut = (double)cv[k - 1] - 2.0 * (double)eps[b];
  if (t_floor && t_floor[b] - (double)eps[b] > cut) cut = t_floor[b] - (double)eps[b];
  __syncthreads();
  if (xb) xbad = 1;
  // 1. the whole list at once (no per-candidate load latency): count valid rows, flag corrupt
  //    ones, compact the rows above the cut into rw[0, nkeep)
  for (int c0 = 0; c0 < kprime; c0 += RTHREADS) {
    const int c = c0 + tid;
    int64_t row = -1;
    float v = 0.f;
    if (c < kprime) {
      row = cr[c];
      v = cv[c];
      row = row >= 0 ? row - list_base : -1;  // a list of GLOBAL rows (list_base = row_offset)
    }
    const bool bad = c < kprime && row >= n_rows;  // corrupt entry, never dereferenced
    const bool valid = c < kprime && row >= 0 && !bad;
    const bool keep = valid && !((double)v < cut);
    if (bad) corrupt = 1;
    const uint64_t vb = __ballot(valid), kb = __ballot(keep);
    int base = 0;
    if (lane == 0) {
      if (vb) atomicAdd(&nvalid, __popcll(vb));
      if (kb) base = atomicAdd(&nkeep, __popcll(kb));
    }
    base = __shfl(base, 0, 64);
    int at = -1;
    if (keep) {
      at = base + __popcll(kb & ((1ull << lane) - 1));
      rw[at] = row;
      sc[at] = (double)v;
      pl[at] = c;
    }
    if constexpr (NU > 0) {  // pass A's rows: the kept ones among the list's first k
      const bool top = keep && c < k;
      const uint64_t tb = __ballot(top);
      int tbase = 0;
      if (lane == 0 && tb) tbase = atomicAdd(&nsel, __popcll(tb));
      tbase = __shfl(tbase, 0, 64);
      if (top) ix[tbase + __popcll(tb & ((1ull << lane) - 1))] = at;
    }
  }
  __syncthreads();
  RST(1);
  const int nk = nkeep;
  // 2. exact scores in two passes. The list's first k positions hold its k best approx (a
  //    partitioned or sorted list): pass A scores those; their smallest exact score s_min
  //    bounds the k-th best exact score from below (k rows reach it), so a later candidate
  //    with approx < s_min - eps (exact < s_min) cannot enter the top k: pass B skips it. About
  //    half of the 2 eps band is never gathered.
  //    Two rows per wave at a time with all of a lane's loads for both rows issued before the
  //    arithmetic (chunk order per lane unchanged: bit-identical sums).
  auto exact_pass = [&](bool top, double cut2) {
    for (int j = wave; j < nk; j += 2 * NW) {
    const int jb = j + NW;
    const bool sel_a = (pl[j] < k) == top && (top || !(sc[j] < cut2));
    const bool sel_b = jb < nk && (pl[jb] < k) == top && (top || !(sc[jb] < cut2));
    if (!top) {  // skipped: below the two-stage cut, sorted last
      if (lane == 0 && pl[j] >= k && !sel_a) sc[j] = -__builtin_inf();
      if (lane == 0 && jb < nk && pl[jb] >= k && !sel_b) sc[jb] = -__builtin_inf();
    }
    if (!sel_a && !sel_b) continue;
    const int ja = sel_a ? j : jb;          // one selected row goes first
    const bool hb = sel_a && sel_b;         // a second one
    if (gathered && lane == 0) atomicAdd(&ngath, hb ? 2 : 1);
    const int64_t ra = rw[ja], rb = hb ? rw[jb] : ra;
    const double ga = gnorm[ra], gb = gnorm[rb];
    double sa = 0.0, sb = 0.0;
    if constexpr (VEC) {
      constexpr int ES = (DT == EBT_F64) ? 8 : (DT == EBT_F32 ? 4 : 2);
      constexpr int PER = 16 / ES;
      constexpr int U = 4;
      const int nch = d / PER;
      const char* pa = (const char*)cat + ra * ld * ES;
      const char* pb = (const char*)cat + rb * ld * ES;
      for (int ch0 = lane; ch0 < nch; ch0 += 64 * U) {
        uint4 xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ch = ch0 + 64 * u;
          if (ch < nch) {
            xa[u] = *(const uint4*)(pa + (int64_t)ch * 16);
            if (hb) xb[u] = *(const uint4*)(pb + (int64_t)ch * 16);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ch = ch0 + 64 * u;
          if (ch < nch) {
            sa += chunk_dot<DT>(qs + ch * PER, xa[u]);
            if (hb) sb += chunk_dot<DT>(qs + ch * PER, xb[u]);
          }
        }
      }
    } else {
      for (int e = lane; e < d; e += 64) {
        sa += qs[e] * load_as_f64<DT>(cat, ra * ld + e);
        if (hb) sb += qs[e] * load_as_f64<DT>(cat, rb * ld + e);
      }
    }
    sa = wave_sum_f64(sa);
    sb = wave_sum_f64(sb);
    if (lane == 0) {
      const double va = sa / ga;
      sc[ja] = (va == va) ? va : -__builtin_inf();
      if (hb) {
        const double vb2 = sb / gb;
        sc[jb] = (vb2 == vb2) ? vb2 : -__builtin_inf();
      }
    }
    }
  };
  // NU > 0: the wave's rows ix[i0 .. i0 + NR) of a pass list, all of their loads issued before
  // the arithmetic (the last row repeated past the list's end, not stored)
  auto exact_rows = [&](int n) {
    if constexpr (NU > 0) {
      constexpr int NR = rescore_rows_per_trip<NU>();
      const int nch = d / PER;
      for (int i0 = wave * NR; i0 < n; i0 += NW * NR) {
        int64_t r[NR];
        double g[NR];
        uint4 x[NR][NU];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) r[rr] = rw[ix[i0 + rr < n ? i0 + rr : n - 1]];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
          const char* p = (const char*)cat + r[rr] * ld * ES;
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            const int ch = lane + 64 * u;
            x[rr][u] = *(const uint4*)(p + (int64_t)(ch < nch ? ch : 0) * 16);
          }
          g[rr] = gnorm[r[rr]];
        }
        double s[NR];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
          s[rr] = 0.0;
#pragma unroll
          for (int u = 0; u < NU; ++u)
            if (lane + 64 * u < nch) s[rr] += chunk_dot<DT>(qv[u], x[rr][u]);
        }
        // the NR butterflies together; the first lane of each value's lane group stores it
        const double tot = wave_sum_f64_rows<NR>(s);
        const int own = wave_rows_owner<NR>(lane);
        double gown = g[0];
#pragma unroll
        for (int rr = 1; rr < NR; ++rr) gown = own == rr ? g[rr] : gown;
        if ((lane & (64 / NR - 1)) == 0 && i0 + own < n) {
          const double v = tot / gown;
          sc[ix[i0 + own]] = (v == v) ? v : -__builtin_inf();
        }
      }
    }
  };
  if constexpr (NU > 0) exact_rows(nsel);
  else exact_pass(true, 0.0);
  __syncthreads();
  RST(2);
  // pass B's row count restarts (every thread read pass A's before the barrier above)
  if (NU > 0 && tid == 0) {
    ngath = nsel;
    nsel = 0;
  }
  // s_min over the k top entries (all k present and valid), as an order-preserving key: a wave
  // count and a wave minimum (DPP), then one LDS atomic per wave instead of one per entry
  for (int j0 = 0; j0 < nk; j0 += RTHREADS) {
    const int j = j0 + tid;
    const bool top = j < nk && pl[j] < k;
    unsigned long long key = ~0ull;  // no valid key is all ones
    if (top) {
      const double x = sc[j];
      const unsigned long long u = (unsigned long long)__double_as_longlong(x);
      if (x == x) key = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    const uint64_t tb = __ballot(top);
    const uint32_t kh = wave_min_u32((uint32_t)(key >> 32));
    const uint32_t kl = wave_min_u32((uint32_t)(key >> 32) == kh ? (uint32_t)key : 0xffffffffu);
    const unsigned long long wk = ((unsigned long long)kh << 32) | kl;
    if (lane == 0) {
      if (tb) atomicAdd(&ntop, (int)__popcll(tb));
      if (wk != ~0ull) atomicMin(&smin_key, wk);
    }
  }
  __syncthreads();
  double cut2 = cut;
  // (eps = 0 means "rescore every candidate above the first cut", not an exact approx)
  if (ntop == k && smin_key != ~0ull && eps[b] > 0.f) {
    const unsigned long long key = smin_key;
    const double smin = __longlong_as_double(
        (long long)((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key));
    if (smin - (double)eps[b] > cut2) cut2 = smin - (double)eps[b];
  }
  if constexpr (NU > 0) {
    // pass B's rows: past the list's first k and not below cut2; the others sorted last
    for (int j0 = 0; j0 < nk; j0 += RTHREADS) {
      const int j = j0 + tid;
      const bool rest = j < nk && pl[j] >= k;
      const bool sel = rest && !(sc[j] < cut2);
      if (rest && !sel) sc[j] = -__builtin_inf();
      const uint64_t sb = __ballot(sel);
      int sbase = 0;
      if (lane == 0 && sb) sbase = atomicAdd(&nsel, __popcll(sb));
      sbase = __shfl(sbase, 0, 64);
      if (sel) ix[sbase + __popcll(sb & ((1ull << lane) - 1))] = j;
    }
    __syncthreads();
    RST(3);
    exact_rows(nsel);
  } else {
    RST(3);
    exact_pass(false, cut2);
  }
  RST(4);
  if (pack.len) {
    // the sharded step's pack count: the entries of this query's top k with score >= t_floor
    // (ebt_shard_pack's prefix) are min(k, the kept rows scoring >= t_floor) -- those rank
    // before every other kept row; read from the exact scores in LDS, no second pass over the
    // written list. (A barrier first: the last pass's scores come from other waves.)
    __syncthreads();
    const double tf = t_floor ? t_floor[b] : -__builtin_inf();
    int c = 0;
    for (int j = tid; j < nk; j += RTHREADS) c += sc[j] >= tf ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0 && c) atomicAdd(&npk, c);   // read after the ordering's barriers
  }
  // 3. order the kept rows (score desc, row asc); positions past them read NaN / -1
  if (nk <= RESCORE_RANK_MAX) {
    // few rows (C2 / C3: ~120-150): each row's position is the number of rows before it,
    // counted over LDS broadcast reads -- one barrier instead of a bitonic network's ~36. The
    // reads go 8 rows at a time, all issued before the first compare (one LDS latency per 8
    // rows, not per row), and up to RTHREADS / 2 rows take two threads each, one per half of
    // the list (the upper half's count handed over in LDS): the same counts.
    __shared__ int part[RTHREADS / 2];
    auto count_before = [&](double s, int64_t r, int j, int lo, int hi) {
      int pos = 0;
      for (int i0 = lo; i0 < hi; i0 += 8) {
        double si[8];
        int64_t ri[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u < hi ? i0 + u : hi - 1;
          si[u] = sc[i];
          ri[u] = rw[i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u;
          pos += (i < hi && (pair_before(si[u], ri[u], s, r) ||
                             (si[u] == s && ri[u] == r && i < j))) ? 1 : 0;
        }
      }
      return pos;
    };
    auto put = [&](double s, int64_t r, int pos) {
      if (pos < k) {
        out_s[b * k + pos] = s;
        out_r[b * k + pos] = r + row_offset;
      }
    };
    __syncthreads();
    if (nk <= RTHREADS / 2) {
      const int j = tid & (RTHREADS / 2 - 1);
      const bool upper = tid >= RTHREADS / 2;
      const int m = nk >> 1;
      double s = 0.0;
      int64_t r = 0;
      int pos = 0;
      if (j < nk) {
        s = sc[j];
        r = rw[j];
        pos = upper ? count_before(s, r, j, m, nk) : count_before(s, r, j, 0, m);
        if (upper) part[j] = pos;
      }
      __syncthreads();
      if (!upper && j < nk) put(s, r, pos + part[j]);
    } else {
      for (int j = tid; j < nk; j += RTHREADS) put(sc[j], rw[j], count_before(sc[j], rw[j], j, 0, nk));
    }
    for (int j = nk + tid; j < k; j += RTHREADS) {
      out_s[b * k + j] = __builtin_nan("");
      out_r[b * k + j] = -1;
    }
  } else {
    int P = 1;
    while (P < nk || P < k) P <<= 1;
    for (int c = nk + tid; c < P; c += RTHREADS) {
      sc[c] = -__builtin_inf();
      rw[c] = INT64_MAX;
    }
    __syncthreads();
    bitonic_pairs(sc, rw, P);
    for (int j = tid; j < k; j += RTHREADS) {
      const int64_t r = rw[j];
      if (r == INT64_MAX) {
        out_s[b * k + j] = __builtin_nan("");
        out_r[b * k + j] = -1;
      } else {
        out_s[b * k + j] = sc[j];
        out_r[b * k + j] = r + row_offset;
      }
    }
  }
  if (tid == 0) {
    int ok = 1;
    if (nvalid >= kprime && n_rows > kprime) {  // kprime >= n_rows: every row is a candidate
      // rows below the k'-th candidate have approx <= amin; none of them can enter the top k
      // when amin < cut (the local k-th - 2 eps, or t_floor - eps when that is higher)
      const double amin = (double)cv[kprime - 1];
      ok = amin < cut2;
    }
    if (ovf_cnt && ovf_cnt[b] > ovf_cap) ok = -1;  // fused screen dropped candidates
    // a caller's screening threshold above the floor's cut may have dropped a row of the
    // global top k (ebt_certify_cut's test, folded in)
    if (theta && t_floor && !((double)theta[b] <= t_floor[b] - (double)eps[b])) ok = -1;
    if (corrupt) ok = -2;                           // internal error: row out of range
    if (xbad) ok = -3;                              // caller error: unsorted exclusion segment
    certified[b] = ok;
    if (pack.len) pack.len[b] = (uint32_t)(npk < k ? npk : k);
    // rows gathered by the two passes (roofline accounting: ebt_timer_count_rows), spread over
    // 64 counters 128 bytes apart: one address taking every query's atomic serialised them and
    // slowed the measured kernel by ~9 % at C3
    if (gathered)
      atomicAdd(gathered + (b & 63) * 16, (unsigned long long)(ngath + (NU > 0 ? nsel : 0)));
  }
#ifdef EBT_RESCORE_STAMP
  RST(5);
  if (tid == 0 && g_rstamp) {
#pragma unroll
    for (int i = 0; i < 5; ++i) g_rstamp[5 * b + i] = rs[i + 1] - rs[i];
  }
#endif
}

// ebt_rescore_form: 1 = register-query form (default; EBT_RESCORE_REG=0 in the environment
// starts the process with the LDS-query form)
static std::atomic<int>& rescore_form_flag() {
  static std::atomic<int> f([] {
    const char* v = getenv("EBT_RESCORE_REG");
    return v ? (atoi(v) != 0 ? 1 : 0) : 1;
  }());
  return f;
}
static bool rescore_form_reg() { return rescore_form_flag().load(std::memory_order_relaxed) != 0; }

__global__ void wave_sum_check_kernel(const double* __restrict__ in, int64_t n_waves,
                                      double* __restrict__ a, double* __restrict__ b) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_waves) return;  // whole waves
  const double v = in[w * 64 + (threadIdx.x & 63)];
  a[w * 64 + (threadIdx.x & 63)] = wave_sum_f64(v);
  b[w * 64 + (threadIdx.x & 63)] = wave_sum_f64_shfl(v);
}

extern "C" int ebt_rescore_form(int form) {
  if (form < 0) return rescore_form_flag().load();
  return rescore_form_flag().exchange(form != 0 ? 1 : 0);
}

extern "C" int ebt_wave_sum_check(const double* in, int64_t n_waves, double* out_a, double* out_b,
                                  void* stream) {
  if (!in || !out_a || !out_b || n_waves < 0) {
    set_error("ebt_wave_sum_check: bad arguments");
    return EBT_EINVAL;
  }
  if (n_waves == 0) return EBT_OK;
  hipLaunchKernelGGL(wave_sum_check_kernel, dim3((unsigned)ceil_div(n_waves, 4)), dim3(256), 0,
                     (hipStream_t)stream, in, n_waves, out_a, out_b);
  return launch_check("wave_sum_check_kernel");
}

static size_t rescore_lds_bytes(int d, int kprime) {
  const int kpp = next_pow2_h(kprime);
  return 8 * (size_t)((d + 1) & ~1) + 20 * (size_t)kpp;
}

int rescore(const double* q64, int64_t B, const CatOps& c, const CandList& l, int32_t k,
            const float* eps, const double* t_floor, double* out_s, int64_t* out_r,
            int32_t* certified, const RescoreExtras& x, hipStream_t st) {
  // the kernels' operands under the names their launches use
  const void* cat = c.cat;
  const int dtype = c.dtype, d = c.d;
  const int64_t ld = c.ld, row_offset = c.row_offset, n_rows = c.n_rows;
  const double* gnorm = c.gnorm64;
  const float* cand_vals = l.vals;
  const int64_t* cand_rows = l.rows;
  const int kprime = l.kprime;
  const int64_t list_base = l.list_base;
  const int* ovf_cnt = x.ovf;
  const float* theta = x.theta;
  const int64_t *excl_off = x.excl.off, *excl_rows = x.excl.rows;
  unsigned long long* gathered = x.gathered;
  const int ovf_cap = 0;  // flags, not counts: any nonzero entry is an overflow
  const ShardPackOut po = x.pack ? *x.pack : ShardPackOut{};
  if (!q64 || !cat || !gnorm || !cand_vals || !cand_rows || !eps || !out_s || !out_r ||
      !certified || B < 0 || d <= 0 || ld < d || k < 1 || kprime < k || kprime > 4096 ||
      dtype < 0 || dtype > 3) {
    set_error("ebt_rescore: bad arguments (d=%d k=%d kprime=%d)", d, k, kprime);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const int kpp = next_pow2_h(kprime);
  const size_t lds = rescore_lds_bytes(d, kprime);
  if (lds > 150 * 1024) {
    set_error("ebt_rescore: d=%d with kprime=%d exceeds LDS", d, kprime);
    return EBT_EUNSUPPORTED;
  }
  const bool vec = vec_ok(cat, dtype, ld, d);
  dim3 grid((unsigned)B), block(RTHREADS);
  // every form takes the same operands
  auto launch = [&](auto kern, size_t bytes) {
    set_max_lds((const void*)kern, (int)bytes);
    hipLaunchKernelGGL(kern, grid, block, bytes, st, q64, d, cat, ld, gnorm, row_offset,
                       cand_vals, cand_rows, kprime, kpp, k, n_rows, eps, t_floor, out_s, out_r,
                       certified, ovf_cnt, ovf_cap, gathered, list_base, theta, excl_off,
                       excl_rows, po);
  };
  // the register-query form (chunks per lane NU, rounded up to an instantiated count) unless
  // the form is 0 (the LDS-query form, kept for A/B and for d beyond 512 chunks)
  const int nch = d * dtype_size(dtype) / 16;
  const int nu_need = (nch + 63) / 64;
  const int nu = nu_need <= 4 ? nu_need : (nu_need <= 6 ? 6 : (nu_need <= 8 ? 8 : 0));
  if (vec && rescore_form_reg() && nu > 0) {
    const size_t lds_r = 24 * (size_t)kpp;
    for_dtype(dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      switch (nu) {
        case 1: launch(rescore_kernel<DT, true, 1>, lds_r); break;
        case 2: launch(rescore_kernel<DT, true, 2>, lds_r); break;
        case 3: launch(rescore_kernel<DT, true, 3>, lds_r); break;
        case 4: launch(rescore_kernel<DT, true, 4>, lds_r); break;
        case 6: launch(rescore_kernel<DT, true, 6>, lds_r); break;
        default: launch(rescore_kernel<DT, true, 8>, lds_r); break;
      }
    });
    return launch_check("rescore_kernel");
  }
  for_dtype(dtype, [&](auto dt) {
    for_bool(vec, [&](auto v) {
      launch(rescore_kernel<decltype(dt)::value, decltype(v)::value>, lds);
    });
  });
  return launch_check("rescore_kernel");
}

// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Exact screen (EBT_FLAG_EXACT): S[b][j] = (float)((q64_b . c_j) / gnorm64_j), the rescore's own
// float64 arithmetic rounded once to f32, for every row of a chunk. This is the last-resort
// screen for a query whose f16/bf16 screen cannot be certified even at k' = 4096 (a cluster of
// more than k' rows within the f16 error bound of the k-th score): its only error is the f32
// rounding (|score| <= 1, so <= 2^-25) plus float64 round-off, so EXACT_EPS certifies anything
// short of true f32-level ties. Plain FMA tiling (64 queries x 64 rows per workgroup, 4 x 4 per
// thread): it runs for a handful of queries, never on the hot path.
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void screen_exact_kernel(
    const double* __restrict__ q64, int64_t B, int d, const void* __restrict__ cat, int64_t ld,
    const double* __restrict__ gnorm, int64_t n_rows, float* __restrict__ S, int64_t ld_s) {
  double acc[4][4] = {};
  int64_t q_at, r_at;
  exact_tile_f64<DT>(q64, B, d, cat, ld, n_rows, acc, q_at, r_at);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t qb = q_at + i;
    if (qb >= B) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = r_at + j;
      if (row < n_rows) {
        const double v = acc[i][j] / gnorm[row];
        S[qb * ld_s + row] = (v == v) ? (float)v : -__builtin_inff();
      }
    }
  }
}

int screen_exact(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
                 const double* gnorm, int64_t n_rows, float* S, int64_t ld_s, hipStream_t st) {
  if (!q64 || !cat || !gnorm || !S || B < 0 || d < 1 || ld < d || n_rows < 0 || ld_s < n_rows ||
      dtype < 0 || dtype > 3) {
    set_error("ebt_screen_exact: bad arguments");
    return EBT_EINVAL;
  }
  if (B == 0 || n_rows == 0) return EBT_OK;
  if (ceil_div(B, XT) > 65535) {
    set_error("ebt_screen_exact: batch too large");
    return EBT_EINVAL;
  }
  dim3 grid((unsigned)ceil_div(n_rows, XT), (unsigned)ceil_div(B, XT)), block(256);
  for_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(screen_exact_kernel<decltype(dt)::value>, grid, block, 0, st, q64, B, d,
                       cat, ld, gnorm, n_rows, S, ld_s);
  });
  return launch_check("screen_exact_kernel");
}

// ---------------------------------------------------------------------------------------------
// Two-phase certification over a row-sharded catalog (distributed.py). Phase 1 on every rank:
// ebt_cosine_screen leaves the shard's k' best approx candidates (GLOBAL rows) -> all-gather ->
// the k' best of all shards (same on every rank). Phase 2: each rank computes the exact float64
// score of the merged candidates IT owns (rescore_owned: 0 elsewhere), an all-reduce (SUM)
// completes them, and finalize_topk sorts and certifies exactly like rescore_kernel. A row
// outside the merged list has approx <= the merged k'-th (it lost a merge or a shard's own
// selection, whose k'-th is <= the merged k'-th) or was dropped by a segment threshold below
// the list's k-th - 2 eps, so "merged[k'-1] < merged[k-1] - 2 eps" certifies the global top-k.
// ---------------------------------------------------------------------------------------------
__global__ void export_list_kernel(int64_t* __restrict__ rows, int64_t B, int kprime,
                                   int64_t row_offset, const int* __restrict__ ovf,
                                   const float* __restrict__ eps, int32_t* __restrict__ ovf_out,
                                   float* __restrict__ eps_out) {
  const int64_t b = blockIdx.x;
  for (int j = threadIdx.x; j < kprime; j += blockDim.x) {
    const int64_t r = rows[b * kprime + j];
    rows[b * kprime + j] = r >= 0 ? r + row_offset : -1;
  }
  if (threadIdx.x == 0) {
    ovf_out[b] = ovf ? (ovf[b] > 0 ? ovf[b] : 0) : 0;  // 1 overflow, 2 speculation failed
    eps_out[b] = eps[b];
  }
}

int export_list(int64_t* rows, int64_t B, int32_t kprime, int64_t row_offset, const int* ovf,
                const float* eps, int32_t* ovf_out, float* eps_out, hipStream_t st) {
  if (B <= 0) return EBT_OK;
  hipLaunchKernelGGL(export_list_kernel, dim3((unsigned)B), dim3(256), 0, st, rows, B, kprime,
                     row_offset, ovf, eps, ovf_out, eps_out);
  return launch_check("export_list_kernel");
}

template <int DT, bool VEC>
__global__ __launch_bounds__(RTHREADS) void rescore_owned_kernel(
    const double* __restrict__ q64, int d, const void* __restrict__ cat, int64_t ld,
    const double* __restrict__ gnorm, int64_t row_offset, int64_t n_local,
    const float* __restrict__ cand_vals, const int64_t* __restrict__ cand_rows, int kprime, int k,
    const float* __restrict__ eps, double* __restrict__ exact) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* qs = (double*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  stage_f64(qs, q64 + b * d, d);
  __syncthreads();
  const float* cv = cand_vals + b * kprime;
  const double cut = (double)cv[k - 1] - 2.0 * (double)eps[b];
  for (int c = wave; c < kprime; c += RTHREADS / 64) {
    const int64_t g = cand_rows[b * kprime + c];
    const int64_t row = g - row_offset;
    const bool mine = g >= 0 && row >= 0 && row < n_local && !((double)cv[c] < cut);
    double s = 0.0;
    if (mine) {
      if constexpr (VEC) {
        constexpr int ES = (DT == EBT_F64) ? 8 : (DT == EBT_F32 ? 4 : 2);
        constexpr int PER = 16 / ES;
        const char* base = (const char*)cat + row * ld * ES;
        for (int ch = lane; ch < d / PER; ch += 64) {
          const uint4 raw = *(const uint4*)(base + (int64_t)ch * 16);
          const int j0 = ch * PER;
          // NOT chunk_dot: products add into the running s, no chunk sum first -- other bits
          if constexpr (DT == EBT_F32) {
            const float* f = (const float*)&raw;
#pragma unroll
            for (int e = 0; e < 4; ++e) s += qs[j0 + e] * (double)f[e];
          } else if constexpr (DT == EBT_F64) {
            const double* f = (const double*)&raw;
            s += qs[j0] * f[0] + qs[j0 + 1] * f[1];
          } else {
            const uint16_t* h = (const uint16_t*)&raw;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              s += qs[j0 + e] * (DT == EBT_BF16 ? bf16_bits_to_f64(h[e]) : f16_bits_to_f64(h[e]));
          }
        }
      } else {
        for (int j = lane; j < d; j += 64) s += qs[j] * load_as_f64<DT>(cat, row * ld + j);
      }
      s = wave_sum_f64(s);
    }
    if (lane == 0) exact[b * kprime + c] = mine ? s / gnorm[row] : 0.0;
  }
}

int rescore_owned(const double* q64, int64_t B, int32_t d, const void* cat, int dtype, int64_t ld,
                  const double* gnorm, int64_t row_offset, int64_t n_local,
                  const float* cand_vals, const int64_t* cand_rows, int32_t kprime, int32_t k,
                  const float* eps, double* exact, hipStream_t st) {
  if (!q64 || !cat || !gnorm || !cand_vals || !cand_rows || !eps || !exact || B < 0 || d <= 0 ||
      ld < d || k < 1 || kprime < k || kprime > 4096 || dtype < 0 || dtype > 3 || n_local < 0) {
    set_error("ebt_rescore_owned: bad arguments");
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const size_t lds = (size_t)((d + 1) & ~1) * 8;
  if (lds > 150 * 1024) {
    set_error("ebt_rescore_owned: d=%d exceeds LDS", d);
    return EBT_EUNSUPPORTED;
  }
  dim3 grid((unsigned)B), block(RTHREADS);
  for_dtype(dtype, [&](auto dt) {
    for_bool(vec_ok(cat, dtype, ld, d), [&](auto vec) {
      const auto kern = rescore_owned_kernel<decltype(dt)::value, decltype(vec)::value>;
      set_max_lds((const void*)kern, (int)lds);
      hipLaunchKernelGGL(kern, grid, block, lds, st, q64, d, cat, ld, gnorm, row_offset, n_local,
                         cand_vals, cand_rows, kprime, k, eps, exact);
    });
  });
  return launch_check("rescore_owned_kernel");
}

// Sort the merged candidates above the cut by (exact desc, row asc), keep k, certify.
__global__ __launch_bounds__(RTHREADS) void finalize_topk_kernel(
    const float* __restrict__ cand_vals, const int64_t* __restrict__ cand_rows,
    const double* __restrict__ exact, int kprime, int kpp, int k, int64_t n_rows,
    const float* __restrict__ eps, const int32_t* __restrict__ ovf, double* __restrict__ out_s,
    int64_t* __restrict__ out_r, int32_t* __restrict__ certified) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sc = (double*)smem;
  int64_t* rw = (int64_t*)(sc + kpp);
  __shared__ int nvalid, corrupt;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (tid == 0) {
    nvalid = 0;
    corrupt = 0;
  }
  __syncthreads();
  const float* cv = cand_vals + b * kprime;
  const double cut = (double)cv[k - 1] - 2.0 * (double)eps[b];
  int myvalid = 0;
  for (int c = tid; c < kpp; c += RTHREADS) {
    const int64_t r = c < kprime ? cand_rows[b * kprime + c] : -1;
    if (r >= n_rows) {  // corrupt entry (as rescore_kernel): not a candidate, certified = -2
      corrupt = 1;
      sc[c] = -__builtin_inf();
      rw[c] = INT64_MAX;
    } else if (r >= 0) {
      ++myvalid;
      const double v = exact[b * kprime + c];
      const bool below = (double)cv[c] < cut;  // not a candidate: never fills an empty slot
      sc[c] = (below || !(v == v)) ? -__builtin_inf() : v;
      rw[c] = below ? INT64_MAX : r;
    } else {
      sc[c] = -__builtin_inf();
      rw[c] = INT64_MAX;
    }
  }
  if (myvalid) atomicAdd(&nvalid, myvalid);
  __syncthreads();
  bitonic_pairs(sc, rw, kpp);
  for (int j = tid; j < k; j += RTHREADS) {
    const int64_t r = rw[j];
    if (r == INT64_MAX) {
      out_s[b * k + j] = __builtin_nan("");
      out_r[b * k + j] = -1;
    } else {
      out_s[b * k + j] = sc[j];
      out_r[b * k + j] = r;
    }
  }
  if (tid == 0) {
    int ok = 1;
    if (nvalid >= kprime && n_rows > kprime)
      ok = (double)cv[kprime - 1] < (double)cv[k - 1] - 2.0 * (double)eps[b];
    if (ovf && ovf[b]) ok = -1;
    if (corrupt) ok = -2;  // internal error: row out of range
    certified[b] = ok;
  }
}

int finalize_topk(const float* cand_vals, const int64_t* cand_rows, const double* exact,
                  int64_t B, int32_t kprime, int32_t k, int64_t n_rows, const float* eps,
                  const int32_t* ovf, double* out_s, int64_t* out_r, int32_t* certified,
                  hipStream_t st) {
  if (!cand_vals || !cand_rows || !exact || !eps || !out_s || !out_r || !certified || B < 0 ||
      k < 1 || kprime < k || kprime > 4096) {
    set_error("ebt_finalize_topk: bad arguments");
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const int kpp = next_pow2_h(kprime);
  const size_t lds = (size_t)kpp * 16;
  set_max_lds((const void*)finalize_topk_kernel, (int)lds);
  hipLaunchKernelGGL(finalize_topk_kernel, dim3((unsigned)B), dim3(RTHREADS), lds, st, cand_vals,
                     cand_rows, exact, kprime, kpp, k, n_rows, eps, ovf, out_s, out_r, certified);
  return launch_check("finalize_topk_kernel");
}

}  // namespace ebt
