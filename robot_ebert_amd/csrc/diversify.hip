// Diversified top-k (include/ebert.h 0.10.0): greedy maximal marginal relevance over a pool.
//
// The reference sorts by score and cuts at k (lib.py:51-55), so near-duplicate rows sit next to
// each other in its answer. These kernels re-rank a pool of the p best rows of a query so that
// each pick maximises lam * relevance - (1 - lam) * (largest cosine to a row already picked):
//
//  * pool_gram_kernel -- S(b, i, j) = (x_i . x_j) / (g_i * g_j) for every pair of pool slots of
//                        query b: a gathered float64 GEMM of p x d by d x p per query on
//                        v_mfma_f64_16x16x4_f64, liked_contrib_kernel's shape (explain.hip) with
//                        both panels drawn from the same row list. One workgroup of eight waves
//                        owns a 128 x 128 tile of one query's matrix; the panels are staged in
//                        LDS in the catalog's dtype (16-byte loads, 128 bytes of every row per K
//                        slab) and converted to float64 as the MFMA operands are read; two slabs
//                        are held, so that slab s + 1 is stored while slab s is read and there
//                        is one barrier per slab. A tile on the diagonal (the only one when
//                        p <= 128) stages its rows once, reads both operands from them, and
//                        computes only the 16 x 16 MFMA tiles on or above the diagonal: the
//                        others are their mirror images, written from the same registers.
//  * mmr_select_kernel -- one wave per query: every lane keeps the relevance, the penalty and the
//                        alive bit of up to EBT_MMR_POOL_MAX / 64 slots in registers; each of the
//                        k rounds is a wave-wide arg-max over order-preserving 64-bit keys with
//                        the position as the second key (explain_select_kernel's technique), then
//                        one read of row s of the matrix.
//
// Arithmetic order (the matrix is compared bitwise across launches, batches and permutations of
// the pool): the dot product follows the rule at the top of pair_f64.h, under which dot(i, j)
// and dot(j, i) have the same bits and the order depends on d and the dtype only -- not on p,
// the tile a slot lands in, or which other queries share the batch. Then, rounded one operation
// at a time (no contraction): g = g_i * g_j, S = dot / g; and in the selection
// v = (lam * rel) - ((1 - lam) * pen).
#include "pair_f64.h"

namespace ebt {

namespace {

constexpr int DV_THREADS = 512;
constexpr int DV_BT = 128;                  // slots per side of a workgroup tile (8 MFMA tiles)
constexpr int DV_ROWS = 2 * DV_BT;          // staged rows: the A panel, then the B panel
constexpr int DV_WM = 4, DV_WN = 2;         // 16 x 16 tiles per wave (the waves are 2 x 4)
static_assert(DV_BT == 2 * 16 * DV_WM && DV_BT == 4 * 16 * DV_WN, "wave tiles");
typedef PairTile<DV_THREADS, DV_ROWS, DV_WM, DV_WN> DvTile;
static_assert(DvTile::CPT % 2 == 0, "a diagonal tile stages half");
constexpr int MMR_SLOTS = EBT_MMR_POOL_MAX / 64;   // pool slots a lane of the selection holds

struct GramArgs {
  RowSrc src;
  int64_t B;
  const int64_t* rows;     // [B][p] GLOBAL pool rows, -1 = empty
  int p;
  double* gram;            // [B][p][p]
  int32_t* status;         // [B]
};

// LDS bytes of one staged K slab: a pool of one tile (p <= DV_BT) has diagonal tiles only, which
// stage a single panel. The kernel holds two slabs.
__host__ __device__ inline int gram_slab_bytes(int p) {
  return (p <= DV_BT ? DV_BT : DV_ROWS) * DvTile::LDR;
}

// One operation at a time, so that the result does not depend on what the compiler would fuse
__device__ __forceinline__ double cos_term(double dot, double gi, double gj) {
#pragma clang fp contract(off)
  const double g = gi * gj;
  return dot / g;
}
__device__ __forceinline__ double mmr_value(double lam, double oml, double rel, double pen) {
#pragma clang fp contract(off)
  const double a = lam * rel;
  const double c = oml * pen;
  return a - c;
}

template <int DT>
__global__ __launch_bounds__(DV_THREADS) void pool_gram_kernel(const GramArgs a) {
  typedef typename PairElem<DT>::U U;
  constexpr int KE = DvTile::ke<DT>();           // elements per slab
  extern __shared__ __attribute__((aligned(16))) unsigned char tile[];   // slabs s, s + 1
  __shared__ int64_t s_row[DV_ROWS];   // local catalog row of a staged row, -1: none (zeros)
  __shared__ double s_g[DV_ROWS];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int p = a.p;
  const int64_t T = (p + DV_BT - 1) / DV_BT;     // tiles per side of a query's matrix
  const int TILE = gram_slab_bytes(p);           // bytes of one staged slab
  const int nslabs = (a.src.d + KE - 1) / KE;
  for (int64_t blk = blockIdx.x; blk < a.B * T * T; blk += gridDim.x) {
    const int64_t b = blk / (T * T);
    const int mb = (int)((blk % (T * T)) / T), nb = (int)(blk % T);
    const int m0 = mb * DV_BT, n0 = nb * DV_BT;
    const int mrows = p - m0 < DV_BT ? p - m0 : DV_BT;
    const int nrows = p - n0 < DV_BT ? p - n0 : DV_BT;
    const bool diag = mb == nb;        // one panel serves as both operands
    const int bbase = diag ? 0 : DV_BT;
    const int nstage = diag ? DvTile::CPT / 2 : DvTile::CPT;
    const int64_t* __restrict__ pool = a.rows + b * p;
    double* __restrict__ outb = a.gram + b * p * p;
    // ---- the query's rows are checked before any of them is followed --------------------------
    const bool qbad = block_any(rows_outside<DV_THREADS>(a.src, pool, p, true), &s_bad);
    if (mb == 0 && nb == 0 && tid == 0) a.status[b] = qbad ? -2 : 1;
    if (qbad) {   // nothing of this query is read: its values are NaN
      for (int t = tid; t < mrows * nrows; t += DV_THREADS)
        outb[(int64_t)(m0 + t / nrows) * p + n0 + t % nrows] = f64_nan();
      continue;
    }
    for (int i = tid; i < DV_ROWS; i += DV_THREADS) {
      const int slot = i < DV_BT ? (i < mrows ? m0 + i : -1)
                                 : (!diag && i - DV_BT < nrows ? n0 + i - DV_BT : -1);
      int64_t r = -1;
      if (slot >= 0 && pool[slot] != -1) r = pool[slot] - a.src.row_offset;
      s_row[i] = r;
      s_g[i] = r >= 0 ? a.src.gnorm[r] : 1.0;
    }
    __syncthreads();
    const int nta = DvTile::tiles(mrows, wm * 16 * DV_WM, DV_WM);
    const int ntb = DvTile::tiles(nrows, wn * 16 * DV_WN, DV_WN);
    // The tiles this wave computes: those that reach into the pool and, on a diagonal workgroup
    // tile, only those on or above the diagonal -- S(j, i) is S(i, j)'s bits (products commute),
    // so the epilogue writes a tile above the diagonal to both places
    uint32_t live = DvTile::live_mask(nta, ntb);
    if (diag) {
#pragma unroll
      for (int t = 0; t < DV_WM; ++t)
#pragma unroll
        for (int u = 0; u < DV_WN; ++u)
          if (wm * DV_WM + t > wn * DV_WN + u) live &= ~(1u << (t * DV_WN + u));
    }
    f64x4_t acc[DV_WM][DV_WN];
    DvTile::clear(acc);
    // Slab s + 1 travels from memory into registers while the MFMAs of slab s run, and goes into
    // the other half of `tile` after them: one barrier per slab. (The barrier that ended slab
    // s - 1 is what makes that half free: every wave has read it.)
    uint4 pre[DvTile::CPT];
    DvTile::fetch<U>(a.src, s_row, 0, nstage, pre);
    DvTile::store(tile, nstage, pre);
    __syncthreads();
    for (int s = 0; s < nslabs; ++s) {
      if (s + 1 < nslabs) DvTile::fetch<U>(a.src, s_row, (s + 1) * KE, nstage, pre);
      if (live)   // (wave-uniform)
        DvTile::mma<DT>(tile + (s & 1) * TILE, wm * 16 * DV_WM, bbase + wn * 16 * DV_WN, lane, s,
                        a.src.d, live, acc);
      if (s + 1 < nslabs) DvTile::store(tile + ((s + 1) & 1) * TILE, nstage, pre);
      __syncthreads();
    }
    // C/D of v_mfma_f64_16x16x4_f64 (pair_f64.h): column = lane & 15, row = (lane >> 4) + 4 * i
#pragma unroll
    for (int t = 0; t < DV_WM; ++t) {
#pragma unroll
      for (int u = 0; u < DV_WN; ++u) {
        if (!((live >> (t * DV_WN + u)) & 1u)) continue;
        const bool mirror = diag && wm * DV_WM + t < wn * DV_WN + u;
        const int jj = wn * 16 * DV_WN + u * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ii = wm * 16 * DV_WM + t * 16 + (lane >> 4) + 4 * i;
          if (ii < mrows && jj < nrows) {
            const double v = s_row[ii] < 0 || s_row[bbase + jj] < 0
                                 ? f64_nan()
                                 : cos_term(acc[t][u][i], s_g[ii], s_g[bbase + jj]);
            outb[(int64_t)(m0 + ii) * p + n0 + jj] = v;
            if (mirror) outb[(int64_t)(m0 + jj) * p + n0 + ii] = v;   // (m0 == n0 here)
          }
        }
      }
    }
  }
}

// ---- the greedy selection -------------------------------------------------------------------------
struct MmrArgs {
  const double* gram;      // [B][p][p]
  const double* rel;       // [B][p]
  const int64_t* rows;     // [B][p]
  int64_t B;
  int p, k;
  double lam, oml;         // oml = 1.0 - lam, computed once on the host
  const int32_t* status;   // NULL: every query is good
  int32_t* pos;
  int64_t* row;
  double* orel;
  double* mmr;
};

__global__ __launch_bounds__(256) void mmr_select_kernel(const MmrArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = a.p, k = a.k;
  for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < a.B; b += (int64_t)gridDim.x * 4) {
    const double* __restrict__ G = a.gram + b * p * p;
    double rel[MMR_SLOTS], pen[MMR_SLOTS];
    uint32_t alive = 0u;   // bit c: slot lane + 64 c is a candidate not yet picked
    const bool good = !a.status || a.status[b] >= 0;
#pragma unroll
    for (int c = 0; c < MMR_SLOTS; ++c) {
      const int i = lane + 64 * c;
      rel[c] = f64_nan();
      pen[c] = 0.0;
      if (good && i < p) {
        rel[c] = a.rel[b * p + i];
        if (a.rows[b * p + i] >= 0 && rel[c] == rel[c]) alive |= 1u << c;
      }
    }
    int t = 0;
    for (; t < k; ++t) {
      uint64_t bk = 0ull;
      uint32_t bp = 0xFFFFFFFFu;
      double bv = 0.0, br = 0.0;
#pragma unroll
      for (int c = 0; c < MMR_SLOTS; ++c) {   // positions ascend with c: > keeps the first
        const double v = mmr_value(a.lam, a.oml, rel[c], pen[c]);
        const uint64_t key = ((alive >> c) & 1u) ? f64_key(v) : 0ull;
        if (key > bk) {
          bk = key;
          bp = (uint32_t)(lane + 64 * c);
          bv = v;
          br = rel[c];
        }
      }
      const uint64_t best = wave_max_u64(bk);
      if (best == 0ull) break;   // nothing left (wave-uniform)
      const uint32_t s = wave_min_u32(bk == best ? bp : 0xFFFFFFFFu);
      if (bp == s) {             // the one lane that holds slot s
        a.pos[b * k + t] = (int32_t)s;
        a.row[b * k + t] = a.rows[b * p + s];
        a.orel[b * k + t] = br;
        a.mmr[b * k + t] = bv;
        alive &= ~(1u << (s >> 6));
      }
      if (t + 1 == k) continue;
#pragma unroll
      for (int c = 0; c < MMR_SLOTS; ++c) {
        const int i = lane + 64 * c;
        if (i < p) {
          const double sv = G[(int64_t)s * p + i];
          pen[c] = t == 0 ? sv : (sv > pen[c] ? sv : pen[c]);
        }
      }
    }
    for (int tt = t + lane; tt < k; tt += 64) {
      a.pos[b * k + tt] = -1;
      a.row[b * k + tt] = -1;
      a.orel[b * k + tt] = f64_nan();
      a.mmr[b * k + tt] = f64_nan();
    }
  }
}

int check_pool(const char* who, int64_t B, int32_t p) {
  if (B < 0 || p < 1 || p > EBT_MMR_POOL_MAX) {
    set_error("%s: bad arguments (B=%lld p=%d: 1 <= p <= %d)", who, (long long)B, p,
              EBT_MMR_POOL_MAX);
    return EBT_EINVAL;
  }
  return EBT_OK;
}

int check_pick(const char* who, int32_t p, int32_t k, double lam) {
  if (k < 1 || k > p) {
    set_error("%s: k=%d is outside [1, p=%d]", who, k, p);
    return EBT_EINVAL;
  }
  if (!(lam >= 0.0 && lam <= 1.0)) {
    set_error("%s: lam=%g is outside [0, 1]", who, lam);
    return EBT_EINVAL;
  }
  return EBT_OK;
}

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

size_t ebt_mmr_workspace_bytes(int64_t B, int32_t p) {
  if (B < 1 || p < 1 || p > EBT_MMR_POOL_MAX) return 0;
  const size_t per = (size_t)8 * (size_t)p * (size_t)p;
  if ((size_t)B > ((~(size_t)0 >> 1) - 256) / per) return 0;
  return align_up(per * (size_t)B);
}

int ebt_pool_gram(const ebt_catalog* cat, int64_t B, const int64_t* rows, int32_t p, double* gram,
                  int32_t* status, void* stream) {
  const char* who = "ebt_pool_gram";
  int rc = check_catalog(who, cat);
  if (rc) return rc;
  if (!rows || !gram || !status) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  rc = check_pool(who, B, p);
  if (rc) return rc;
  if (B == 0) return EBT_OK;
  GramArgs a;
  a.src = row_src(*cat);
  a.B = B; a.rows = rows; a.p = p; a.gram = gram; a.status = status;
  const int64_t T = ceil_div(p, DV_BT);
  const dim3 grid((unsigned)grid_of(B * T * T, 1 << 20)), block(DV_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const int lds = 2 * gram_slab_bytes(p);
  for_dtype(cat->dtype, [&](auto dt) {
    set_max_lds((const void*)pool_gram_kernel<decltype(dt)::value>, lds);
    hipLaunchKernelGGL(pool_gram_kernel<decltype(dt)::value>, grid, block, lds, st, a);
  });
  return launch_check("pool_gram_kernel");
}

int ebt_mmr_select(const double* gram, const double* rel, const int64_t* rows, int64_t B,
                   int32_t p, int32_t k, double lam, const int32_t* status, int32_t* out_pos,
                   int64_t* out_rows, double* out_rel, double* out_mmr, void* stream) {
  const char* who = "ebt_mmr_select";
  if (!gram || !rel || !rows || !out_pos || !out_rows || !out_rel || !out_mmr) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  int rc = check_pool(who, B, p);
  if (rc) return rc;
  rc = check_pick(who, p, k, lam);
  if (rc) return rc;
  if (B == 0) return EBT_OK;
  MmrArgs a;
  a.gram = gram; a.rel = rel; a.rows = rows; a.B = B; a.p = p; a.k = k;
  a.lam = lam; a.oml = 1.0 - lam; a.status = status;
  a.pos = out_pos; a.row = out_rows; a.orel = out_rel; a.mmr = out_mmr;
  hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)grid_of(ceil_div(B, 4), 1 << 20)),
                     dim3(256), 0, (hipStream_t)stream, a);
  return launch_check("mmr_select_kernel");
}

int ebt_mmr_topk(const ebt_catalog* cat, int64_t B, const double* rel, const int64_t* rows,
                 int32_t p, int32_t k, double lam, void* workspace, size_t ws_bytes,
                 int32_t* out_pos, int64_t* out_rows, double* out_rel, double* out_mmr,
                 int32_t* status, void* stream) {
  const char* who = "ebt_mmr_topk";
  int rc = check_catalog(who, cat);
  if (rc) return rc;
  if (!rel || !rows || !workspace || !out_pos || !out_rows || !out_rel || !out_mmr || !status) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  rc = check_pool(who, B, p);
  if (rc) return rc;
  rc = check_pick(who, p, k, lam);
  if (rc) return rc;
  if (B == 0) return EBT_OK;
  const size_t need = ebt_mmr_workspace_bytes(B, p);
  if (need == 0 || ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes (ebt_mmr_workspace_bytes)", who, ws_bytes, need);
    return EBT_EINVAL;
  }
  rc = ebt_pool_gram(cat, B, rows, p, (double*)workspace, status, stream);
  if (rc) return rc;
  return ebt_mmr_select((const double*)workspace, rel, rows, B, p, k, lam, status, out_pos,
                        out_rows, out_rel, out_mmr, stream);
}

}  // extern "C"
