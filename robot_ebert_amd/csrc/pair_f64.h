// The float64 pair-product core of the gathered GEMMs on v_mfma_f64_16x16x4_f64: the dot products
// of pairs of catalog rows named by index lists (liked_contrib_kernel in explain.hip,
// pool_gram_kernel in diversify.hip). Shared: where rows come from (RowSrc), how a K slab of them
// is staged in LDS in the catalog's dtype, and how a wave reads its operands from it and
// accumulates. Each kernel keeps its own pipeline (slabs held, barriers per slab, workgroup
// size) and its own epilogue.
//
// ARITHMETIC ORDER (results are compared bitwise across launches, batches, permutations and
// between the kernels that use this header). The dot product of a pair of rows is accumulated by
// the MFMAs of one wave in a fixed order -- K slabs of 128 bytes per row ascending; inside a slab
// two groups of four 16-byte chunks; inside a group the element s of each chunk, s ascending, one
// MFMA per s whose four K values are element s of the group's four chunks (lane >> 4 picks the
// chunk). Both operands permute alike and products commute, so dot(i, j) and dot(j, i) have the
// same bits, and the order depends on d and the dtype only -- not on how many rows there are, the
// tile a row lands in, which operand it is, or which other queries share the batch. Columns past
// d are staged as zeros. The element path (rows that are not 16-byte aligned, d = 77) stages the
// same values into the same LDS positions, so it gives the chunk path's bits. What a kernel does
// with the dot product afterwards is its own, one separately rounded operation at a time.
#pragma once

#include "common.h"

namespace ebt {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// The rows a kernel gathers from: one device's catalog
struct RowSrc {
  const void* data;        // the catalog's matrix [n][ld]
  int64_t ld;
  int d;
  int vec;                 // rows are 16-byte aligned (base and row stride)
  const double* gnorm;
  int64_t row_offset, n;   // GLOBAL row g is local row g - row_offset, valid in [0, n)
};

inline RowSrc row_src(const ebt_catalog& cat) {
  RowSrc s;
  s.data = cat.data; s.ld = cat.ld; s.d = cat.d;
  s.vec = vec_ok(cat.data, cat.dtype, cat.ld, 0);
  s.gnorm = cat.gnorm64; s.row_offset = cat.row_offset; s.n = cat.n;
  return s;
}

inline int check_catalog(const char* who, const ebt_catalog* cat) {
  if (!cat || !cat->data || !cat->gnorm64) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (cat->n < 1 || cat->d < 1 || cat->ld < cat->d || cat->dtype < 0 || cat->dtype > 3) {
    set_error("%s: bad catalog (n=%lld d=%d ld=%lld dtype=%d)", who, (long long)cat->n, cat->d,
              (long long)cat->ld, cat->dtype);
    return EBT_EINVAL;
  }
  return EBT_OK;
}

inline int64_t grid_of(int64_t items, int64_t cap) {
  return items < 1 ? 1 : (items > cap ? cap : items);
}

__device__ __forceinline__ double f64_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// This thread's share of the range check of `cnt` GLOBAL rows: true when one lies outside the
// catalog. -1 (an empty slot) passes where `empty_ok`.
template <int THREADS>
__device__ __forceinline__ bool rows_outside(const RowSrc& a, const int64_t* __restrict__ rows,
                                             int64_t cnt, bool empty_ok) {
  bool bad = false;
  for (int64_t i = threadIdx.x; i < cnt; i += THREADS) {
    const int64_t g = rows[i];
    const int64_t r = g - a.row_offset;
    bad |= !(empty_ok && g == -1) && (r < 0 || r >= a.n);
  }
  return bad;
}

// `mine` of any thread of the workgroup, through the LDS word `flag` (whose last reader may be
// this function's previous call)
__device__ __forceinline__ bool block_any(bool mine, int* flag) {
  __syncthreads();
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  if (mine) *flag = 1;
  __syncthreads();
  return *flag != 0;
}

// elements e0 .. e0 + 16 / sizeof(U) of local row r as one 16-byte chunk; zeros past d and for
// r < 0 (a row that is not staged). The element form reads only elements below d.
template <typename U>
__device__ __forceinline__ uint4 load_chunk(const RowSrc& a, int64_t r, int e0) {
  constexpr int PER = 16 / (int)sizeof(U);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (r < 0 || e0 >= a.d) return v;
  const U* p = (const U*)a.data + (r * a.ld + e0);
  if (a.vec && e0 + PER <= a.d) return *(const uint4*)p;
  U t[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) t[e] = e0 + e < a.d ? p[e] : (U)0;
  __builtin_memcpy(&v, t, 16);
  return v;
}

// element s of a staged 16-byte chunk as float64
template <int DT, int S>
__device__ __forceinline__ double chunk_elem(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if constexpr (DT == EBT_F32) {
    return (double)__uint_as_float(w[S]);
  } else if constexpr (DT == EBT_F64) {
    return f64_from_halves(w[2 * S], w[2 * S + 1]);
  } else {
    const uint16_t h = (uint16_t)(w[S >> 1] >> (16 * (S & 1)));
    if constexpr (DT == EBT_BF16) return bf16_bits_to_f64(h);
    else return f16_bits_to_f64(h);
  }
}

// the unsigned type of an element's size, and what follows from it
template <int DT> struct PairElem { typedef uint32_t U; };
template <> struct PairElem<EBT_F64> { typedef uint64_t U; };
template <> struct PairElem<EBT_BF16> { typedef uint16_t U; };
template <> struct PairElem<EBT_F16> { typedef uint16_t U; };

// MFMA steps S .. PER - 1 of one group of four chunks: in step S lane l supplies element S of
// chunk (l >> 4) of row (l & 15) of each tile as its A or B operand. `live` has bit t * WN + u set
// for the tiles this wave computes (wave-uniform).
template <int DT, int S, int PER, int WM, int WN>
struct MfmaSteps {
  __device__ __forceinline__ static void run(const uint4 (&ra)[WM], const uint4 (&rb)[WN],
                                             uint32_t live, f64x4_t (&acc)[WM][WN]) {
    if constexpr (S < PER) {
      double fa[WM], fb[WN];
#pragma unroll
      for (int t = 0; t < WM; ++t) fa[t] = chunk_elem<DT, S>(ra[t]);
#pragma unroll
      for (int u = 0; u < WN; ++u) fb[u] = chunk_elem<DT, S>(rb[u]);
#pragma unroll
      for (int t = 0; t < WM; ++t)
#pragma unroll
        for (int u = 0; u < WN; ++u)
          if ((live >> (t * WN + u)) & 1u)
            acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fb[u], acc[t][u], 0, 0, 0);
      MfmaSteps<DT, S + 1, PER, WM, WN>::run(ra, rb, live, acc);
    }
  }
};

// A workgroup of THREADS threads stages ROWS rows per K slab; each wave owns WM x WN tiles of
// 16 x 16. A compile-time record: constants and static functions, no state.
template <int THREADS, int ROWS, int WM, int WN>
struct PairTile {
  static constexpr int SLAB = 128;               // bytes of every staged row per K slab
  static constexpr int LDR = SLAB + 16;          // LDS row stride: the 16 rows of a b128 read land
                                                 // in 64 distinct banks (36 words apart)
  static constexpr int CPR = SLAB / 16;          // 16-byte chunks per row and slab
  static constexpr int CPT = ROWS * CPR / THREADS;   // chunks a thread stages per slab
  static_assert(ROWS * CPR % THREADS == 0, "staging");
  static_assert(WM * WN <= 32, "live mask");

  // elements per slab
  template <int DT>
  static constexpr int ke() { return SLAB / (int)sizeof(typename PairElem<DT>::U); }

  // The first `nstage` of this thread's chunks of the slab that starts at element e_base, from
  // memory into `pre`; s_row[i] is the local catalog row of staged row i, -1: none (zeros).
  template <typename U>
  __device__ __forceinline__ static void fetch(const RowSrc& src, const int64_t* s_row, int e_base,
                                               int nstage, uint4 (&pre)[CPT]) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int id = threadIdx.x + THREADS * i;
      if (i < nstage)
        pre[i] = load_chunk<U>(src, s_row[id / CPR], e_base + (id % CPR) * (16 / (int)sizeof(U)));
    }
  }
  // ... and from `pre` into the slab at `dst`
  __device__ __forceinline__ static void store(unsigned char* dst, int nstage,
                                               const uint4 (&pre)[CPT]) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int id = threadIdx.x + THREADS * i;
      if (i < nstage) *(uint4*)(dst + (id / CPR) * LDR + (id % CPR) * 16) = pre[i];
    }
  }

  // how many of a wave's w tiles, the first at row `first`, reach into `rows` rows
  __device__ __forceinline__ static int tiles(int rows, int first, int w) {
    const int nt = (rows - first + 15) / 16;
    return nt < 0 ? 0 : (nt > w ? w : nt);
  }
  __device__ __forceinline__ static uint32_t live_mask(int nta, int ntb) {
    uint32_t live = 0u;
#pragma unroll
    for (int t = 0; t < WM; ++t)
#pragma unroll
      for (int u = 0; u < WN; ++u)
        if (t < nta && u < ntb) live |= 1u << (t * WN + u);
    return live;
  }
  __device__ __forceinline__ static void clear(f64x4_t (&acc)[WM][WN]) {
#pragma unroll
    for (int t = 0; t < WM; ++t)
#pragma unroll
      for (int u = 0; u < WN; ++u) acc[t][u] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  }

  // The wave's MFMAs of slab s, staged at `slab`: its A tiles start at staged row a_row0, its B
  // tiles at b_row0. C/D of v_mfma_f64_16x16x4_f64: lane l holds in acc[t][u][i] the product of A
  // row t * 16 + (l >> 4) + 4 * i and B row u * 16 + (l & 15). (The epilogues walk that layout in
  // their own words: through a visitor shared here both kernels measured slower, and
  // liked_contrib_kernel, at its 256-register bound, spilled two more registers.)
  template <int DT>
  __device__ __forceinline__ static void mma(const unsigned char* slab, int a_row0, int b_row0,
                                             int lane, int s, int d, uint32_t live,
                                             f64x4_t (&acc)[WM][WN]) {
    constexpr int PER = 16 / (int)sizeof(typename PairElem<DT>::U);   // elements per chunk
#pragma unroll
    for (int c = 0; c < CPR / 4; ++c) {
      if (s * ke<DT>() + c * 4 * PER >= d) break;   // a group of chunks wholly past d: zeros
      uint4 ra[WM], rb[WN];
      const int at = (lane & 15) * LDR + c * 64 + (lane >> 4) * 16;
#pragma unroll
      for (int t = 0; t < WM; ++t) ra[t] = *(const uint4*)(slab + (a_row0 + t * 16) * LDR + at);
#pragma unroll
      for (int u = 0; u < WN; ++u) rb[u] = *(const uint4*)(slab + (b_row0 + u * 16) * LDR + at);
      MfmaSteps<DT, 0, PER, WM, WN>::run(ra, rb, live, acc);
    }
  }
};

}  // namespace ebt
