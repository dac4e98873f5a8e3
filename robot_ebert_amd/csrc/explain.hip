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
// the dot product follows the rule at the top of pair_f64.h, which depends on d and the dtype
// only -- not on k, L_b, the tile a row lands in, or which other queries share the batch. Then,
// rounded one operation at a time (no contraction): g = g_l * g_j, c = dot / g, t = w_l * c,
// contrib = t * (1 / W_b), with W_b the sequential sum of |w_l| in CSR order (L_b when there are
// no weights).
#include "pair_f64.h"

namespace ebt {

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_BM = 128;                  // result rows per workgroup tile (8 MFMA tiles)
constexpr int EX_BN = 96;                   // liked rows per workgroup tile (6 MFMA tiles)
constexpr int EX_ROWS = EX_BM + EX_BN;
constexpr int EX_WM = 4, EX_WN = 3;         // 16 x 16 tiles per wave (the waves are 2 x 2)
static_assert(EX_BM == 2 * 16 * EX_WM && EX_BN == 2 * 16 * EX_WN, "wave tiles");
typedef PairTile<EX_THREADS, EX_ROWS, EX_WM, EX_WN> ExTile;

struct ExplainArgs {
  RowSrc src;
  int64_t B;
  const int64_t* off;      // [B + 1] liked CSR
  const int64_t* lrows;    // GLOBAL liked rows
  const double* lw;        // weights or NULL
  const int64_t* rows;     // [B][k] GLOBAL result rows, -1 = empty
  int k;
  double* out;             // CSR-shaped [k * nnz]
  int32_t* status;         // [B]
};

// One operation at a time, so that the result does not depend on what the compiler would fuse
__device__ __forceinline__ double contrib_term(double w, double dot, double gl, double gj,
                                               double inv_w) {
#pragma clang fp contract(off)
  const double g = gl * gj;
  const double c = dot / g;
  const double t = w * c;
  return t * inv_w;
}

template <int DT>
__global__ __launch_bounds__(EX_THREADS, 2) void liked_contrib_kernel(const ExplainArgs a) {
  typedef typename PairElem<DT>::U U;
  constexpr int KE = ExTile::ke<DT>();           // elements per slab
  __shared__ __attribute__((aligned(16))) unsigned char tile[EX_ROWS * ExTile::LDR];
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
  const int nslabs = (a.src.d + KE - 1) / KE;
  for (int64_t blk = blockIdx.x; blk < a.B * mblocks; blk += gridDim.x) {
    const int64_t b = blk / mblocks;
    const int m0 = (int)(blk % mblocks) * EX_BM;
    const int mrows = k - m0 < EX_BM ? k - m0 : EX_BM;
    const int64_t l0 = a.off[b];
    const int64_t Lb = a.off[b + 1] > l0 ? a.off[b + 1] - l0 : 0;
    const int64_t* __restrict__ res = a.rows + b * k;
    double* __restrict__ outb = a.out + (int64_t)k * l0;
    // ---- the query's rows are checked before any of them is followed --------------------------
    const bool qbad = block_any(rows_outside<EX_THREADS>(a.src, a.lrows + l0, Lb, false) ||
                                    rows_outside<EX_THREADS>(a.src, res, k, true),
                                &s_bad);
    if (m0 == 0 && tid == 0) a.status[b] = qbad ? -2 : 1;
    if (qbad) {   // nothing of this query is read: its outputs are NaN
      for (int64_t t = tid; t < (int64_t)mrows * Lb; t += EX_THREADS)
        outb[(int64_t)m0 * Lb + t] = f64_nan();
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
    const int nta = ExTile::tiles(mrows, wm * 16 * EX_WM, EX_WM);
    for (int64_t n0 = 0; n0 < Lb; n0 += EX_BN) {
      const int nrows = Lb - n0 < EX_BN ? (int)(Lb - n0) : EX_BN;
      // wave-uniform: tiles past the query's rows are not computed
      const int ntb = ExTile::tiles(nrows, wn * 16 * EX_WN, EX_WN);
      const uint32_t live = ExTile::live_mask(nta, ntb);
      __syncthreads();   // the epilogue before this one has read the row records
      for (int i = tid; i < EX_ROWS; i += EX_THREADS) {
        int64_t r = -1;
        if (i < EX_BM) {
          if (i < mrows && res[m0 + i] != -1) r = res[m0 + i] - a.src.row_offset;
        } else if (i - EX_BM < nrows) {
          r = a.lrows[l0 + n0 + (i - EX_BM)] - a.src.row_offset;
          s_w[i - EX_BM] = a.lw ? a.lw[l0 + n0 + (i - EX_BM)] : 1.0;
        }
        s_row[i] = r;
        s_g[i] = r >= 0 ? a.src.gnorm[r] : 1.0;
      }
      __syncthreads();
      f64x4_t acc[EX_WM][EX_WN];
      ExTile::clear(acc);
      // slab s + 1 travels from memory into registers while the MFMAs of slab s run
      uint4 pre[ExTile::CPT];
      ExTile::fetch<U>(a.src, s_row, 0, ExTile::CPT, pre);
      for (int s = 0; s < nslabs; ++s) {
        __syncthreads();   // every wave has read slab s - 1
        ExTile::store(tile, ExTile::CPT, pre);
        __syncthreads();
        if (s + 1 < nslabs) ExTile::fetch<U>(a.src, s_row, (s + 1) * KE, ExTile::CPT, pre);
        if (nta != 0 && ntb != 0)   // (wave-uniform; the barriers are above)
          ExTile::mma<DT>(tile, wm * 16 * EX_WM, EX_BM + wn * 16 * EX_WN, lane, s, a.src.d, live,
                          acc);
      }
      const double inv_w = s_inv_w;
      // C/D of v_mfma_f64_16x16x4_f64 (pair_f64.h): column = lane & 15, row = (lane >> 4) + 4 * i
#pragma unroll
      for (int t = 0; t < EX_WM; ++t) {
#pragma unroll
        for (int u = 0; u < EX_WN; ++u) {
          if (!((live >> (t * EX_WN + u)) & 1u)) continue;
          const int ll = wn * 16 * EX_WN + u * 16 + (lane & 15);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int jj = wm * 16 * EX_WM + t * 16 + (lane >> 4) + 4 * i;
            if (jj < mrows && ll < nrows) {
              const double v = s_row[jj] < 0 ? f64_nan()
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
  const uint64_t key = f64_key(v);
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
      const uint64_t best = wave_max_u64(bk);
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
      a.val[seg * a.m + tt] = f64_nan();
      a.pos[seg * a.m + tt] = -1;
      a.row[seg * a.m + tt] = -1;
    }
  }
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
  ExplainArgs a;
  a.src = row_src(*cat);
  a.B = B; a.off = liked_off; a.lrows = liked_rows; a.lw = liked_w; a.rows = rows; a.k = k;
  a.out = out; a.status = status;
  const dim3 grid((unsigned)grid_of(B * ceil_div(k, EX_BM), 1 << 20)), block(EX_THREADS);
  hipStream_t st = (hipStream_t)stream;
  for_dtype(cat->dtype, [&](auto dt) {
    hipLaunchKernelGGL(liked_contrib_kernel<decltype(dt)::value>, grid, block, 0, st, a);
  });
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
