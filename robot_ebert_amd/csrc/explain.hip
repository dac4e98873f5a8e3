// Explanations (include/ebert.h 0.9.0): the per-liked-row terms of a returned score.
//
// A liked-row score is a mean over the query's liked rows (lib.py:51-52), and the search folds
// those rows into one query vector before its GEMM, so the individual terms are gone by the time
// the top k is known. These kernels compute them afterwards, for the k returned rows only:
//
//  * liked_contrib_kernel -- contrib(b, j, l) =
//                          (w_l * ((x_{r_l} . x_j) / (g_{r_l} * g_j))) * (1 / W_b)
//                        for every result row j and liked row l of query b: a gathered float64
//                        GEMM of k x d by d x L_b per query on v_mfma_f64_16x16x4_f64. One
//                        workgroup owns 128 result rows of one query and walks that query's liked
//                        rows 96 at a time; both panels are staged in LDS in the catalog's dtype
//                        (16-byte loads, 128 bytes of every row per K slab) and converted to
//                        float64 as the MFMA operands are read.
//  * explain_select_kernel -- one wave per (b, j) segment of L_b contributions: the sequential
//                        float64 sum in list order, then the m best by (value, position) in m
//                        rounds of a wave-wide arg-max over order-preserving 64-bit keys.
//
// Arithmetic order (results are compared bitwise across launches, batches and weight scalings):
// the dot product of a pair of rows is accumulated by the MFMAs of one wave in a fixed order --
// K slabs ascending; inside a slab two groups of four 16-byte chunks; inside a group the element
// s of each chunk, s ascending, one MFMA per s whose four K values are element s of the group's
// four chunks (lane >> 4 picks the chunk). Both operands permute alike, so this is a dot product
// over all of d in an order that depends on d and the dtype only -- not on k, L_b, the tile a row
// lands in, or which other queries share the batch. Columns past d are staged as zeros. The
// element path (rows that are not 16-byte aligned, d = 77) stages the same values into the same
// LDS positions, so it gives the chunk path's bits. Then, rounded one operation at a time (no
// contraction): g = g_l * g_j, c = dot / g, t = w_l * c, contrib = t * (1 / W_b), with W_b the
// sequential sum of |w_l| in CSR order (L_b when there are no weights).
#include "common.h"

namespace ebt {

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_BM = 128;                  // result rows per workgroup tile (8 MFMA tiles)
constexpr int EX_BN = 96;                   // liked rows per workgroup tile (6 MFMA tiles)
constexpr int EX_ROWS = EX_BM + EX_BN;
constexpr int EX_SLAB = 128;                // bytes of every staged row per K slab
constexpr int EX_LDR = EX_SLAB + 16;        // LDS row stride: the 16 rows of a b128 read land in
                                            // 64 distinct banks (36 words apart)
constexpr int EX_CPR = EX_SLAB / 16;        // 16-byte chunks per row and slab
constexpr int EX_CPT = EX_ROWS * EX_CPR / EX_THREADS;   // chunks a thread stages per slab
constexpr int EX_WM = 4, EX_WN = 3;         // 16 x 16 tiles per wave (the waves are 2 x 2)
static_assert(EX_ROWS * EX_CPR % EX_THREADS == 0, "staging");
static_assert(EX_BM == 2 * 16 * EX_WM && EX_BN == 2 * 16 * EX_WN, "wave tiles");

typedef double f64x4_t __attribute__((ext_vector_type(4)));

struct ExplainArgs {
  const void* data;        // the catalog's matrix [n][ld]
  int64_t ld;
  int d;
  int vec;                 // rows are 16-byte aligned (base and row stride)
  const double* gnorm;
  int64_t row_offset, n;
  int64_t B;
  const int64_t* off;      // [B + 1] liked CSR
  const int64_t* lrows;    // GLOBAL liked rows
  const double* lw;        // weights or NULL
  const int64_t* rows;     // [B][k] GLOBAL result rows, -1 = empty
  int k;
  double* out;             // CSR-shaped [k * nnz]
  int32_t* status;         // [B]
};

__device__ __forceinline__ double ex_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// One operation at a time, so that the result does not depend on what the compiler would fuse
__device__ __forceinline__ double contrib_term(double w, double dot, double gl, double gj,
                                               double inv_w) {
#pragma clang fp contract(off)
  const double g = gl * gj;
  const double c = dot / g;
  const double t = w * c;
  return t * inv_w;
}

// elements e0 .. e0 + 16 / sizeof(U) of local row r as one 16-byte chunk; zeros past d and for
// r < 0 (a row that is not staged). The element form reads only elements below d.
template <typename U>
__device__ __forceinline__ uint4 load_chunk(const ExplainArgs& a, int64_t r, int e0) {
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

template <int DT> struct ExElem { typedef uint32_t U; };
template <> struct ExElem<EBT_F64> { typedef uint64_t U; };
template <> struct ExElem<EBT_BF16> { typedef uint16_t U; };
template <> struct ExElem<EBT_F16> { typedef uint16_t U; };

// MFMA step S of one group of four chunks: lane l supplies element S of chunk (l >> 4) of row
// (l & 15) of each tile as its A (result rows) or B (liked rows) operand
template <int DT, int S>
__device__ __forceinline__ void mfma_step(const uint4 (&ra)[EX_WM], const uint4 (&rb)[EX_WN],
                                          int nta, int ntb, f64x4_t (&acc)[EX_WM][EX_WN]) {
  double fa[EX_WM], fb[EX_WN];
#pragma unroll
  for (int t = 0; t < EX_WM; ++t) fa[t] = chunk_elem<DT, S>(ra[t]);
#pragma unroll
  for (int u = 0; u < EX_WN; ++u) fb[u] = chunk_elem<DT, S>(rb[u]);
#pragma unroll
  for (int t = 0; t < EX_WM; ++t)
#pragma unroll
    for (int u = 0; u < EX_WN; ++u)
      if (t < nta && u < ntb)   // wave-uniform: tiles past the query's rows are not computed
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fb[u], acc[t][u], 0, 0, 0);
}

template <int DT, int S, int PER>
struct MfmaSteps {
  __device__ __forceinline__ static void run(const uint4 (&ra)[EX_WM], const uint4 (&rb)[EX_WN],
                                             int nta, int ntb, f64x4_t (&acc)[EX_WM][EX_WN]) {
    mfma_step<DT, S>(ra, rb, nta, ntb, acc);
    MfmaSteps<DT, S + 1, PER>::run(ra, rb, nta, ntb, acc);
  }
};
template <int DT, int PER>
struct MfmaSteps<DT, PER, PER> {
  __device__ __forceinline__ static void run(const uint4 (&)[EX_WM], const uint4 (&)[EX_WN], int,
                                             int, f64x4_t (&)[EX_WM][EX_WN]) {}
};

template <int DT>
__global__ __launch_bounds__(EX_THREADS, 2) void liked_contrib_kernel(const ExplainArgs a) {
  typedef typename ExElem<DT>::U U;
  constexpr int PER = 16 / (int)sizeof(U);       // elements per 16-byte chunk
  constexpr int KE = EX_SLAB / (int)sizeof(U);   // elements per slab
  __shared__ __attribute__((aligned(16))) unsigned char tile[EX_ROWS * EX_LDR];
  __shared__ int64_t s_row[EX_ROWS];   // local catalog row of a staged row, -1: none (zeros)
  __shared__ double s_g[EX_ROWS];
  __shared__ double s_w[EX_BN];
  __shared__ double s_abs[EX_THREADS];
  __shared__ double s_inv_w;
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int k = a.k;
  const int64_t mblocks = (k + EX_BM - 1) / EX_BM;
  const int nslabs = (a.d + KE - 1) / KE;
  for (int64_t blk = blockIdx.x; blk < a.B * mblocks; blk += gridDim.x) {
    const int64_t b = blk / mblocks;
    const int m0 = (int)(blk % mblocks) * EX_BM;
    const int mrows = k - m0 < EX_BM ? k - m0 : EX_BM;
    const int64_t l0 = a.off[b];
    const int64_t Lb = a.off[b + 1] > l0 ? a.off[b + 1] - l0 : 0;
    const int64_t* __restrict__ res = a.rows + b * k;
    double* __restrict__ outb = a.out + (int64_t)k * l0;
    // ---- the query's rows are checked before any of them is followed --------------------------
    __syncthreads();
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int64_t i = tid; i < Lb; i += EX_THREADS) {
      const int64_t r = a.lrows[l0 + i] - a.row_offset;
      bad |= r < 0 || r >= a.n;
    }
    for (int j = tid; j < k; j += EX_THREADS) {
      const int64_t g = res[j];
      const int64_t r = g - a.row_offset;
      bad |= g != -1 && (r < 0 || r >= a.n);
    }
    if (bad) s_bad = 1;
    __syncthreads();
    const bool qbad = s_bad != 0;
    if (m0 == 0 && tid == 0) a.status[b] = qbad ? -2 : 1;
    if (qbad) {   // nothing of this query is read: its outputs are NaN
      for (int64_t t = tid; t < (int64_t)mrows * Lb; t += EX_THREADS)
        outb[(int64_t)m0 * Lb + t] = ex_nan();
      continue;
    }
    // ---- 1 / W_b: the sequential sum of |w_l| in CSR order (thread 0 adds, 256 at a time) ------
    if (a.lw) {
      double W = 0.0;
      for (int64_t c0 = 0; c0 < Lb; c0 += EX_THREADS) {
        __syncthreads();
        if (c0 + tid < Lb) s_abs[tid] = fabs(a.lw[l0 + c0 + tid]);
        __syncthreads();
        if (tid == 0) {
          const int nn = Lb - c0 < EX_THREADS ? (int)(Lb - c0) : EX_THREADS;
          for (int i = 0; i < nn; ++i) W += s_abs[i];
        }
      }
      if (tid == 0) s_inv_w = 1.0 / W;
    } else if (tid == 0) {
      s_inv_w = 1.0 / (double)Lb;
    }
    // ---- the liked rows, EX_BN at a time ------------------------------------------------------
    const int nta_all = (mrows - wm * 16 * EX_WM + 15) / 16;
    const int nta = nta_all < 0 ? 0 : (nta_all > EX_WM ? EX_WM : nta_all);
    for (int64_t n0 = 0; n0 < Lb; n0 += EX_BN) {
      const int nrows = Lb - n0 < EX_BN ? (int)(Lb - n0) : EX_BN;
      const int ntb_all = (nrows - wn * 16 * EX_WN + 15) / 16;
      const int ntb = ntb_all < 0 ? 0 : (ntb_all > EX_WN ? EX_WN : ntb_all);
      __syncthreads();   // the epilogue before this one has read the row records
      for (int i = tid; i < EX_ROWS; i += EX_THREADS) {
        int64_t r = -1;
        if (i < EX_BM) {
          if (i < mrows && res[m0 + i] != -1) r = res[m0 + i] - a.row_offset;
        } else if (i - EX_BM < nrows) {
          r = a.lrows[l0 + n0 + (i - EX_BM)] - a.row_offset;
          s_w[i - EX_BM] = a.lw ? a.lw[l0 + n0 + (i - EX_BM)] : 1.0;
        }
        s_row[i] = r;
        s_g[i] = r >= 0 ? a.gnorm[r] : 1.0;
      }
      __syncthreads();
      f64x4_t acc[EX_WM][EX_WN];
#pragma unroll
      for (int t = 0; t < EX_WM; ++t)
#pragma unroll
        for (int u = 0; u < EX_WN; ++u) acc[t][u] = f64x4_t{0.0, 0.0, 0.0, 0.0};
      // slab s + 1 travels from memory into registers while the MFMAs of slab s run
      uint4 pre[EX_CPT];
#pragma unroll
      for (int i = 0; i < EX_CPT; ++i) {
        const int id = tid + EX_THREADS * i;
        pre[i] = load_chunk<U>(a, s_row[id / EX_CPR], (id % EX_CPR) * PER);
      }
      for (int s = 0; s < nslabs; ++s) {
        __syncthreads();   // every wave has read slab s - 1
#pragma unroll
        for (int i = 0; i < EX_CPT; ++i) {
          const int id = tid + EX_THREADS * i;
          *(uint4*)(tile + (id / EX_CPR) * EX_LDR + (id % EX_CPR) * 16) = pre[i];
        }
        __syncthreads();
        if (s + 1 < nslabs) {
#pragma unroll
          for (int i = 0; i < EX_CPT; ++i) {
            const int id = tid + EX_THREADS * i;
            pre[i] = load_chunk<U>(a, s_row[id / EX_CPR], (s + 1) * KE + (id % EX_CPR) * PER);
          }
        }
        if (nta == 0 || ntb == 0) continue;   // (wave-uniform; the barriers are above)
#pragma unroll
        for (int c = 0; c < EX_CPR / 4; ++c) {
          if (s * KE + c * 4 * PER >= a.d) break;   // a group of chunks wholly past d: zeros
          uint4 ra[EX_WM], rb[EX_WN];
          const int at = (lane & 15) * EX_LDR + c * 64 + (lane >> 4) * 16;
#pragma unroll
          for (int t = 0; t < EX_WM; ++t)
            ra[t] = *(const uint4*)(tile + (wm * 16 * EX_WM + t * 16) * EX_LDR + at);
#pragma unroll
          for (int u = 0; u < EX_WN; ++u)
            rb[u] = *(const uint4*)(tile + (EX_BM + wn * 16 * EX_WN + u * 16) * EX_LDR + at);
          MfmaSteps<DT, 0, PER>::run(ra, rb, nta, ntb, acc);
        }
      }
      // C/D of v_mfma_f64_16x16x4_f64: column = lane & 15, row = (lane >> 4) + 4 * register
      const double inv_w = s_inv_w;
#pragma unroll
      for (int t = 0; t < EX_WM; ++t) {
#pragma unroll
        for (int u = 0; u < EX_WN; ++u) {
          if (t >= nta || u >= ntb) continue;
          const int ll = wn * 16 * EX_WN + u * 16 + (lane & 15);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int jj = wm * 16 * EX_WM + t * 16 + (lane >> 4) + 4 * i;
            if (jj < mrows && ll < nrows) {
              const double v = s_row[jj] < 0 ? ex_nan()
                                             : contrib_term(s_w[ll], acc[t][u][i],
                                                            s_g[EX_BM + ll], s_g[jj], inv_w);
              outb[(int64_t)(m0 + jj) * Lb + n0 + ll] = v;
            }
          }
        }
      }
    }
  }
}

// ---- the m best of every segment ----------------------------------------------------------------
struct SelectArgs {
  const double* contrib;
  int64_t B;
  const int64_t* off;
  const int64_t* lrows;
  int k, m, largest;
  double* val;
  int32_t* pos;
  int64_t* row;
  double* total;   // NULL: not wanted
};

// Order-preserving key of a contribution, larger = better; 0 = NaN (never selected). -0 and +0
// are one value. With largest == 0 the order is reversed (no key but NaN's is 0 or all ones).
__device__ __forceinline__ uint64_t sel_key(double v, int largest) {
  if (!(v == v)) return 0ull;
  const uint64_t u = v == 0.0 ? 0ull : (uint64_t)__double_as_longlong(v);
  const uint64_t key = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  return largest ? key : ~key;
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return f64_from_halves((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l),
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l));
}

__global__ __launch_bounds__(256) void explain_select_kernel(const SelectArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t segs = a.B * a.k;
  for (int64_t seg = (int64_t)blockIdx.x * 4 + w; seg < segs; seg += (int64_t)gridDim.x * 4) {
    const int64_t b = seg / a.k;
    const int j = (int)(seg % a.k);
    const int64_t l0 = a.off[b];
    const int Lb = a.off[b + 1] > l0 ? (int)(a.off[b + 1] - l0) : 0;
    const double* __restrict__ s = a.contrib + (int64_t)a.k * l0 + (int64_t)j * Lb;
    if (a.total) {   // the sequential sum in list order: 64 values per load, added lane by lane
      double sum = 0.0;
      for (int c0 = 0; c0 < Lb; c0 += 64) {
        const double v = c0 + lane < Lb ? s[c0 + lane] : 0.0;
        const int cnt = Lb - c0 < 64 ? Lb - c0 : 64;
        for (int i = 0; i < cnt; ++i) sum += readlane_f64(v, i);
      }
      if (lane == 0) a.total[seg] = sum;
    }
    // round t takes the best entry that comes after round t - 1's in (key desc, position asc)
    uint64_t pk = 0ull;
    uint32_t pp = 0u;
    int t = 0;
    for (; t < a.m; ++t) {
      uint64_t bk = 0ull;
      uint32_t bp = 0xFFFFFFFFu;
      for (int i = lane; i < Lb; i += 64) {
        const uint64_t key = sel_key(s[i], a.largest);
        const bool ok = key != 0ull && (t == 0 || key < pk || (key == pk && (uint32_t)i > pp));
        if (ok && key > bk) {
          bk = key;
          bp = (uint32_t)i;
        }
      }
      const uint32_t hi = wave_max_u32((uint32_t)(bk >> 32));
      const uint32_t lo = wave_max_u32((uint32_t)(bk >> 32) == hi ? (uint32_t)bk : 0u);
      const uint64_t best = ((uint64_t)hi << 32) | lo;
      if (best == 0ull) break;   // nothing left (wave-uniform)
      const uint32_t p = wave_min_u32(bk == best ? bp : 0xFFFFFFFFu);
      if (lane == 0) {
        a.val[seg * a.m + t] = s[p];
        a.pos[seg * a.m + t] = (int32_t)p;
        a.row[seg * a.m + t] = a.lrows[l0 + p];
      }
      pk = best;
      pp = p;
    }
    for (int tt = t + lane; tt < a.m; tt += 64) {
      a.val[seg * a.m + tt] = ex_nan();
      a.pos[seg * a.m + tt] = -1;
      a.row[seg * a.m + tt] = -1;
    }
  }
}

int64_t grid_of(int64_t items, int64_t cap) { return items < 1 ? 1 : (items > cap ? cap : items); }

int check_catalog(const char* who, const ebt_catalog* cat) {
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

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

size_t ebt_explain_workspace_bytes(int64_t nnz, int32_t k) {
  if (nnz < 0 || k < 1 || nnz > (int64_t)((~(size_t)0 >> 1) / 8 / (size_t)k) - 32) return 0;
  const size_t bytes = (size_t)8 * (size_t)k * (size_t)nnz;
  return align_up(bytes < 1 ? 1 : bytes);
}

int ebt_liked_contrib(const ebt_catalog* cat, int64_t B, const int64_t* liked_off,
                      const int64_t* liked_rows, const double* liked_w, const int64_t* rows,
                      int32_t k, double* out, int32_t* status, void* stream) {
  const char* who = "ebt_liked_contrib";
  int rc = check_catalog(who, cat);
  if (rc) return rc;
  if (!liked_off || !liked_rows || !rows || !out || !status) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (B < 0 || k < 1) {
    set_error("%s: bad arguments (B=%lld k=%d: k >= 1)", who, (long long)B, k);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  const int es = cat->dtype == EBT_F64 ? 8 : (cat->dtype == EBT_F32 ? 4 : 2);
  ExplainArgs a;
  a.data = cat->data; a.ld = cat->ld; a.d = cat->d;
  a.vec = ((uintptr_t)cat->data & 15) == 0 && (cat->ld * es) % 16 == 0;
  a.gnorm = cat->gnorm64; a.row_offset = cat->row_offset; a.n = cat->n;
  a.B = B; a.off = liked_off; a.lrows = liked_rows; a.lw = liked_w; a.rows = rows; a.k = k;
  a.out = out; a.status = status;
  const dim3 grid((unsigned)grid_of(B * ceil_div(k, EX_BM), 1 << 20)), block(EX_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (cat->dtype) {
    case EBT_F32: hipLaunchKernelGGL(liked_contrib_kernel<EBT_F32>, grid, block, 0, st, a); break;
    case EBT_BF16: hipLaunchKernelGGL(liked_contrib_kernel<EBT_BF16>, grid, block, 0, st, a); break;
    case EBT_F16: hipLaunchKernelGGL(liked_contrib_kernel<EBT_F16>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(liked_contrib_kernel<EBT_F64>, grid, block, 0, st, a); break;
  }
  return launch_check("liked_contrib_kernel");
}

int ebt_explain_select(const double* contrib, int64_t B, const int64_t* liked_off,
                       const int64_t* liked_rows, int32_t k, int32_t m, int largest,
                       double* out_val, int32_t* out_pos, int64_t* out_row, double* out_total,
                       void* stream) {
  const char* who = "ebt_explain_select";
  if (!contrib || !liked_off || !liked_rows || !out_val || !out_pos || !out_row) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (B < 0 || k < 1) {
    set_error("%s: bad arguments (B=%lld k=%d: k >= 1)", who, (long long)B, k);
    return EBT_EINVAL;
  }
  if (m < 1 || m > EBT_EXPLAIN_M_MAX) {
    set_error("%s: m=%d is outside [1, %d]", who, m, EBT_EXPLAIN_M_MAX);
    return EBT_EINVAL;
  }
  if (B == 0) return EBT_OK;
  SelectArgs a;
  a.contrib = contrib; a.B = B; a.off = liked_off; a.lrows = liked_rows; a.k = k; a.m = m;
  a.largest = largest != 0; a.val = out_val; a.pos = out_pos; a.row = out_row;
  a.total = out_total;
  hipLaunchKernelGGL(explain_select_kernel, dim3((unsigned)grid_of(ceil_div(B * k, 4), 1 << 20)),
                     dim3(256), 0, (hipStream_t)stream, a);
  return launch_check("explain_select_kernel");
}

int ebt_explain_topk(const ebt_catalog* cat, int64_t B, const int64_t* liked_off,
                     const int64_t* liked_rows, const double* liked_w, int64_t nnz,
                     const int64_t* rows, int32_t k, int32_t m, int largest, void* workspace,
                     size_t ws_bytes, double* out_val, int32_t* out_pos, int64_t* out_row,
                     double* out_total, int32_t* status, void* stream) {
  const char* who = "ebt_explain_topk";
  int rc = check_catalog(who, cat);
  if (rc) return rc;
  if (!liked_off || !liked_rows || !rows || !workspace || !out_val || !out_pos || !out_row ||
      !status) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (B < 0 || k < 1 || nnz < 0) {
    set_error("%s: bad arguments (B=%lld k=%d nnz=%lld: k >= 1)", who, (long long)B, k,
              (long long)nnz);
    return EBT_EINVAL;
  }
  if (m < 1 || m > EBT_EXPLAIN_M_MAX) {
    set_error("%s: m=%d is outside [1, %d]", who, m, EBT_EXPLAIN_M_MAX);
    return EBT_EINVAL;
  }
  const size_t need = ebt_explain_workspace_bytes(nnz, k);
  if (need == 0 || ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes (ebt_explain_workspace_bytes)", who, ws_bytes, need);
    return EBT_EINVAL;
  }
  rc = ebt_liked_contrib(cat, B, liked_off, liked_rows, liked_w, rows, k, (double*)workspace,
                         status, stream);
  if (rc) return rc;
  return ebt_explain_select((const double*)workspace, B, liked_off, liked_rows, k, m, largest,
                            out_val, out_pos, out_row, out_total, stream);
}

}  // extern "C"
