// Materialised sub-catalogs (include/ebert.h 0.7.0): the allowed rows of one allow mask copied
// once into a dense catalog of their own, so that a query filtered by a sparse mask is scored over
// its m allowed rows by every existing path (the fused and speculative screens included) instead
// of over all n rows followed by the mask pass (allow_mask.hip).
//
//  * allow_popc       -- popcount of one mask row over rows [0, n_rows): per-workgroup totals
//                        (the compaction's first launch) or one total (ebt_allow_count).
//  * allow_rows       -- the stream compaction: ascending allowed rows and, per mask word, the
//                        number of allowed rows in all earlier words (the rank prefix). Each
//                        workgroup sums the totals of the workgroups before it and scans its own
//                        256 words: output positions are computed, never claimed by an atomic.
//  * catalog_gather   -- one wave per output row, catalog_move_kernel's copies (catalog_update.hip)
//                        between two catalogs: the d matrix elements, the image row, gnorm64 and
//                        inv32 of parent row rows[i]. Nothing is recomputed: a row's norm and image
//                        row are functions of its values only.
//  * sub_excl_count / sub_excl_scan / sub_excl_write -- an exclusion CSR of GLOBAL rows remapped
//                        into the sub-catalog's row numbers through the rank prefix (disallowed
//                        rows dropped; the map is monotone, so segments stay ascending).
//  * sub_rows_to_global -- result rows of the sub-catalog back to GLOBAL rows through the list.
#include "common.h"

namespace ebt {

namespace {

constexpr int SC_THREADS = 256;                 // one mask word per thread
constexpr int64_t SC_WORDS_MAX = 1ll << 26;     // rows [0, 2^31): counts and ranks fit 32 bits
constexpr int SC_AHEAD = 4;                     // 16-byte chunks a lane loads before it stores them

__host__ __device__ inline int64_t sc_al(int64_t v) { return (v + 255) / 256 * 256; }

// word w of the mask row with the bits of rows >= n_rows cleared (0 past the row's last word)
__device__ __forceinline__ uint32_t live_word(const uint32_t* __restrict__ row, int64_t words,
                                              int64_t w, int64_t n_rows) {
  if (w >= words || (w << 5) >= n_rows) return 0u;
  const uint32_t v = row[w];
  const int64_t left = n_rows - (w << 5);
  return left >= 32 ? v : (v & ((1u << left) - 1u));
}

// Workgroup-wide sums of one 32-bit value per thread (every thread of the 256 takes part):
// the inclusive scan within the wave, the totals of the four waves through LDS.
struct BlockScan {
  uint32_t excl;    // sum over the threads before this one
  uint32_t total;   // sum over the workgroup
};
__device__ __forceinline__ BlockScan block_scan_u32(uint32_t v, uint32_t* wave_tot /*LDS [4]*/) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const uint32_t inc = wave_scan_add_u32(v);
  if (lane == 63) wave_tot[w] = inc;
  __syncthreads();
  uint32_t before = 0u, total = 0u;
#pragma unroll
  for (int i = 0; i < SC_THREADS / 64; ++i) {
    const uint32_t t = wave_tot[i];
    before += i < w ? t : 0u;
    total += t;
  }
  __syncthreads();   // wave_tot may be reused by the caller
  return BlockScan{before + inc - v, total};
}

// totals != NULL: totals[block] = allowed rows among the block's 256 words; else *count += them
__global__ __launch_bounds__(SC_THREADS) void allow_popc_kernel(
    const uint32_t* __restrict__ row, int64_t words, int64_t n_rows,
    uint32_t* __restrict__ totals, unsigned long long* __restrict__ count) {
  __shared__ uint32_t wave_tot[SC_THREADS / 64];
  const int64_t w = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  const BlockScan s = block_scan_u32((uint32_t)__popc(live_word(row, words, w, n_rows)), wave_tot);
  if (threadIdx.x == 0) {
    if (totals) totals[blockIdx.x] = s.total;
    else if (s.total) atomicAdd(count, (unsigned long long)s.total);
  }
}

__global__ __launch_bounds__(SC_THREADS) void allow_rows_kernel(
    const uint32_t* __restrict__ row, int64_t words, int64_t n_rows,
    const uint32_t* __restrict__ totals, int64_t* __restrict__ rows_out, int64_t cap,
    uint32_t* __restrict__ rank_out, int64_t* __restrict__ count_out) {
  __shared__ uint32_t wave_tot[SC_THREADS / 64];
  // allowed rows in the workgroups before this one
  uint32_t part = 0u;
  for (int64_t i = threadIdx.x; i < (int64_t)blockIdx.x; i += SC_THREADS) part += totals[i];
  const uint32_t base = block_scan_u32(part, wave_tot).total;
  const int64_t w = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  uint32_t v = live_word(row, words, w, n_rows);
  const BlockScan s = block_scan_u32((uint32_t)__popc(v), wave_tot);
  if (w < words) rank_out[w] = base + s.excl;
  int64_t p = (int64_t)base + s.excl;
  while (v) {
    const int b = __ffs((int)v) - 1;
    if (p < cap) rows_out[p] = (w << 5) + b;
    ++p;
    v &= v - 1u;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count_out = (int64_t)base + s.total;
}

// ---- the gather ---------------------------------------------------------------------------------
struct GatherArgs {
  const void* data;        // the parent's matrix [n][ld]
  int64_t ld;
  int d;
  const int64_t* rows;     // device, m GLOBAL rows of the parent
  int64_t row_offset, n;   // the parent's rows are [row_offset, row_offset + n)
  int64_t m;
  void* data_out;          // [m][ld_out]
  int64_t ld_out;
  const double* gnorm;
  const float* inv32;
  double* gnorm_out;
  float* inv32_out;        // [round_up(m, 128)]
  const uint16_t* img;     // NULL: the parent's matrix is its own image
  uint16_t* img_out;
  int ld_img;
  int vec;                 // the rows of both matrices are 16-byte aligned
};

// nchunks 16-byte chunks from src to dst (both 16-byte aligned), SC_AHEAD loads in flight;
// src == NULL: zeros
__device__ __forceinline__ void gather_chunks(const u16x8_t* __restrict__ src,
                                              u16x8_t* __restrict__ dst, int nchunks, int lane) {
  for (int c = lane; c < nchunks; c += 64 * SC_AHEAD) {
    u16x8_t v[SC_AHEAD];
#pragma unroll
    for (int u = 0; u < SC_AHEAD; ++u) {
      const u16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
      v[u] = (src && c + 64 * u < nchunks) ? src[c + 64 * u] : z;
    }
#pragma unroll
    for (int u = 0; u < SC_AHEAD; ++u)
      if (c + 64 * u < nchunks) dst[c + 64 * u] = v[u];
  }
}

// T: an unsigned integer of the element's size (the bits are copied, a NaN's payload included)
template <typename T>
__global__ __launch_bounds__(256) void catalog_gather_kernel(const GatherArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int PER = 16 / (int)sizeof(T);   // elements per 16-byte chunk
  // the tail of inv32 up to a multiple of 128 rows: the screening epilogue's padding rows
  const int64_t tail = (a.m + 127) / 128 * 128 - a.m;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < tail; t += (int64_t)gridDim.x * 256)
    a.inv32_out[a.m + t] = 1.0f;
  for (int64_t i = (int64_t)blockIdx.x * 4 + w; i < a.m; i += (int64_t)gridDim.x * 4) {
    const int64_t r = a.rows[i] - a.row_offset;
    // a row outside the parent is never followed: a zero row with norm 1
    const bool in = r >= 0 && r < a.n;
    const T* __restrict__ s = in ? (const T*)a.data + r * a.ld : nullptr;
    T* __restrict__ t = (T*)a.data_out + i * a.ld_out;
    const int nvec = a.vec ? a.d / PER : 0;
    gather_chunks((const u16x8_t*)s, (u16x8_t*)t, nvec, lane);
    for (int j = nvec * PER + lane; j < a.d; j += 64) t[j] = in ? s[j] : (T)0;
    if (a.img_out)
      gather_chunks(in ? (const u16x8_t*)(a.img + r * a.ld_img) : nullptr,
                    (u16x8_t*)(a.img_out + i * a.ld_img), a.ld_img / 8, lane);
    if (lane == 0) {
      a.gnorm_out[i] = in ? a.gnorm[r] : 1.0;
      a.inv32_out[i] = in ? a.inv32[r] : 1.0f;
    }
  }
}

// ---- exclusions in the sub-catalog's rows -------------------------------------------------------
struct ExclArgs {
  const uint32_t* row;     // the mask row
  int64_t words;
  const uint32_t* rank;    // [words] allowed rows in all earlier words
  int64_t n_rows;
  const int64_t* off;      // [B + 1] positions into rows
  const int64_t* rows;     // GLOBAL rows, ascending per query
  int64_t B, nnz;
};

// the sub-catalog row of GLOBAL row r, or -1 when r is not an allowed row below n_rows
__device__ __forceinline__ int64_t sub_row(const ExclArgs& a, int64_t r) {
  if (r < 0 || r >= a.n_rows || (r >> 5) >= a.words) return -1;
  const uint32_t v = a.row[r >> 5];
  const int sh = (int)(r & 31);
  if (!((v >> sh) & 1u)) return -1;
  return (int64_t)a.rank[r >> 5] + __popc(v & ((1u << sh) - 1u));
}

// query b's segment clipped to [0, nnz): offsets that point outside `rows` are never followed
__device__ __forceinline__ void seg_of(const ExclArgs& a, int64_t b, int64_t& lo, int64_t& hi) {
  lo = a.off[b];
  hi = a.off[b + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > a.nnz ? a.nnz : hi;
  if (hi < lo) hi = lo;
}

// One wave per query. WRITE = false: cnt[b] = rows of the segment that survive. WRITE = true:
// they go to rows_out[off_out[b] ...] in the segment's order (a ballot places each 64 of them).
template <bool WRITE>
__global__ __launch_bounds__(256) void sub_excl_kernel(const ExclArgs a, uint32_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ off_out,
                                                       int64_t* __restrict__ rows_out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < a.B; b += (int64_t)gridDim.x * 4) {
    int64_t lo, hi;
    seg_of(a, b, lo, hi);
    int64_t done = 0;
    for (int64_t p0 = lo; p0 < hi; p0 += 64) {   // wave-uniform bounds: every lane takes each turn
      const int64_t p = p0 + lane;
      const int64_t s = p < hi ? sub_row(a, a.rows[p]) : -1;
      const uint64_t bal = __ballot(s >= 0);
      if constexpr (WRITE) {
        const int64_t q = off_out[b] + done + __popcll(bal & ((1ull << lane) - 1ull));
        if (s >= 0 && q < a.nnz) rows_out[q] = s;
      }
      done += __popcll(bal);
    }
    if constexpr (!WRITE)
      if (lane == 0) cnt[b] = (uint32_t)done;
  }
}

// off_out[0] = 0, off_out[b + 1] = cnt[0] + ... + cnt[b]: one workgroup, 256 counts per turn
__global__ __launch_bounds__(SC_THREADS) void sub_excl_scan_kernel(const uint32_t* __restrict__ cnt,
                                                                   int64_t B,
                                                                   int64_t* __restrict__ off_out) {
  __shared__ uint32_t wave_tot[SC_THREADS / 64];
  int64_t carry = 0;
  if (threadIdx.x == 0) off_out[0] = 0;
  for (int64_t b0 = 0; b0 < B; b0 += SC_THREADS) {
    const int64_t b = b0 + threadIdx.x;
    const uint32_t v = b < B ? cnt[b] : 0u;
    const BlockScan s = block_scan_u32(v, wave_tot);
    if (b < B) off_out[b + 1] = carry + s.excl + v;
    carry += s.total;
  }
}

__global__ __launch_bounds__(SC_THREADS) void sub_rows_to_global_kernel(
    int64_t* __restrict__ rows, int64_t count, const int64_t* __restrict__ list, int64_t m) {
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; i < count;
       i += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t r = rows[i];
    rows[i] = (r >= 0 && r < m) ? list[r] : -1;
  }
}

// words a positive multiple of 4 (ebt_allow_words) within the 32-bit count range, and n_rows
// inside the row
int check_mask_row(const char* who, int64_t words, int64_t n_rows) {
  if (words < 1 || words % 4 != 0 || words > SC_WORDS_MAX) {
    set_error("%s: words=%lld must be a positive multiple of 4 (ebt_allow_words), at most %lld",
              who, (long long)words, (long long)SC_WORDS_MAX);
    return EBT_EINVAL;
  }
  if (n_rows < 0 || n_rows > 32 * words) {
    set_error("%s: n_rows=%lld is outside the mask row's rows [0, %lld]", who, (long long)n_rows,
              (long long)(32 * words));
    return EBT_EINVAL;
  }
  return EBT_OK;
}

int64_t grid_for(int64_t items, int64_t per_block, int64_t cap) {
  const int64_t b = ceil_div(items, per_block);
  return b < 1 ? 1 : (b > cap ? cap : b);
}

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

int ebt_allow_count(const uint32_t* mask_row, int64_t words, int64_t n_rows, int64_t* count_out,
                    void* stream) {
  const char* who = "ebt_allow_count";
  if (!mask_row || !count_out) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  int rc = check_mask_row(who, words, n_rows);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = hip_check(hipMemsetAsync(count_out, 0, 8, st), "hipMemsetAsync");
  if (rc) return rc;
  hipLaunchKernelGGL(allow_popc_kernel, dim3((unsigned)ceil_div(words, SC_THREADS)),
                     dim3(SC_THREADS), 0, st, mask_row, words, n_rows, (uint32_t*)nullptr,
                     (unsigned long long*)count_out);
  return launch_check("allow_popc_kernel");
}

size_t ebt_allow_rows_bytes(int64_t words) {
  if (words < 1 || words % 4 != 0 || words > SC_WORDS_MAX) return 0;
  return (size_t)sc_al(ceil_div(words, SC_THREADS) * 4);
}

int ebt_allow_rows(const uint32_t* mask_row, int64_t words, int64_t n_rows, int64_t* rows_out,
                   int64_t cap, uint32_t* rank_out, int64_t* count_out, void* ws, size_t ws_bytes,
                   void* stream) {
  const char* who = "ebt_allow_rows";
  if (!mask_row || !rank_out || !count_out || !ws || (cap > 0 && !rows_out)) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  int rc = check_mask_row(who, words, n_rows);
  if (rc) return rc;
  if (cap < 0) {
    set_error("%s: cap=%lld", who, (long long)cap);
    return EBT_EINVAL;
  }
  if (ws_bytes < ebt_allow_rows_bytes(words)) {
    set_error("%s: workspace %zu < %zu bytes (ebt_allow_rows_bytes)", who, ws_bytes,
              ebt_allow_rows_bytes(words));
    return EBT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(words, SC_THREADS)), block(SC_THREADS);
  hipLaunchKernelGGL(allow_popc_kernel, grid, block, 0, st, mask_row, words, n_rows,
                     (uint32_t*)ws, (unsigned long long*)nullptr);
  rc = launch_check("allow_popc_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(allow_rows_kernel, grid, block, 0, st, mask_row, words, n_rows,
                     (const uint32_t*)ws, rows_out, cap, rank_out, count_out);
  return launch_check("allow_rows_kernel");
}

int ebt_catalog_gather_rows(const ebt_catalog* parent, const int64_t* rows, int64_t m,
                            void* data_out, int64_t ld_out, double* gnorm_out, float* inv32_out,
                            void* image_out, ebt_catalog* sub, void* stream) {
  const char* who = "ebt_catalog_gather_rows";
  if (!parent || !rows || !data_out || !gnorm_out || !inv32_out || !sub || !parent->data ||
      !parent->gnorm64 || !parent->inv32 || !parent->image) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  const ebt_catalog& c = *parent;
  if (m < 1 || c.n < 1 || c.d < 1 || c.ld < c.d || c.dtype < 0 || c.dtype > 3 ||
      c.row_offset < 0) {
    set_error("%s: bad arguments (m=%lld: >= 1; parent n=%lld d=%d ld=%lld dtype=%d)", who,
              (long long)m, (long long)c.n, c.d, (long long)c.ld, c.dtype);
    return EBT_EINVAL;
  }
  if (ld_out < c.d) {
    set_error("%s: ld_out=%lld < d=%d", who, (long long)ld_out, c.d);
    return EBT_EINVAL;
  }
  const bool alias = c.image == c.data;   // the parent's matrix is its own MFMA operand
  if (alias && (ld_out % 64 != 0 || ((uintptr_t)data_out & 15) != 0)) {
    set_error("%s: the parent's matrix is its own image: ld_out=%lld must be a multiple of 64 "
              "and data_out 16-byte aligned", who, (long long)ld_out);
    return EBT_EINVAL;
  }
  if (!alias && (!image_out || ((uintptr_t)image_out & 15) != 0 || c.ld_img < c.d ||
                 c.ld_img % 64 != 0 || ((uintptr_t)c.image & 15) != 0)) {
    set_error("%s: the parent has an image of its own: image_out must be [m][ld_img=%d], "
              "16-byte aligned", who, c.ld_img);
    return EBT_EINVAL;
  }
  GatherArgs a;
  a.data = c.data; a.ld = c.ld; a.d = c.d; a.rows = rows; a.row_offset = c.row_offset; a.n = c.n;
  a.m = m; a.data_out = data_out; a.ld_out = ld_out; a.gnorm = c.gnorm64; a.inv32 = c.inv32;
  a.gnorm_out = gnorm_out; a.inv32_out = inv32_out;
  a.img = alias ? nullptr : (const uint16_t*)c.image;
  a.img_out = alias ? nullptr : (uint16_t*)image_out;
  a.ld_img = c.ld_img;
  a.vec = vec_ok(c.data, c.dtype, c.ld, 0) && vec_ok(data_out, c.dtype, ld_out, 0);
  const dim3 grid((unsigned)grid_for(m, 4, 1 << 16)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (dtype_size(c.dtype)) {
    case 8: hipLaunchKernelGGL((catalog_gather_kernel<uint64_t>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((catalog_gather_kernel<uint32_t>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((catalog_gather_kernel<uint16_t>), grid, block, 0, st, a); break;
  }
  const int rc = launch_check("catalog_gather_kernel");
  if (rc) return rc;
  ebt_catalog s{};
  s.data = data_out;
  s.dtype = c.dtype;
  s.d = c.d;
  s.n = m;
  s.ld = ld_out;
  s.row_offset = 0;
  s.gnorm64 = gnorm_out;
  s.inv32 = inv32_out;
  s.image = alias ? data_out : image_out;
  s.cscale = c.native ? inv32_out : nullptr;
  s.img_dtype = c.img_dtype;
  s.ld_img = alias ? (int32_t)ld_out : c.ld_img;
  s.d_pad = c.d_pad;
  s.native = c.native;
  s.u_cat = c.u_cat;
  *sub = s;
  return EBT_OK;
}

size_t ebt_sub_exclusions_bytes(int64_t B, int64_t nnz) {
  if (B < 1 || nnz < 0 || B > (1ll << 31) || nnz > (1ll << 31)) return 0;
  return (size_t)sc_al(B * 4);
}

int ebt_sub_exclusions(const uint32_t* mask_row, int64_t words, const uint32_t* rank,
                       int64_t n_rows, const int64_t* off, const int64_t* rows, int64_t B,
                       int64_t nnz, int64_t* off_out, int64_t* rows_out, void* ws,
                       size_t ws_bytes, void* stream) {
  const char* who = "ebt_sub_exclusions";
  if (!mask_row || !rank || !off || !off_out || !ws || (nnz > 0 && (!rows || !rows_out))) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  int rc = check_mask_row(who, words, n_rows);
  if (rc) return rc;
  const size_t need = ebt_sub_exclusions_bytes(B, nnz);
  if (need == 0) {
    set_error("%s: bad arguments (B=%lld nnz=%lld)", who, (long long)B, (long long)nnz);
    return EBT_EINVAL;
  }
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes (ebt_sub_exclusions_bytes)", who, ws_bytes, need);
    return EBT_EINVAL;
  }
  ExclArgs a;
  a.row = mask_row; a.words = words; a.rank = rank; a.n_rows = n_rows; a.off = off; a.rows = rows;
  a.B = B; a.nnz = nnz;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)grid_for(B, 4, 1 << 16)), block(256);
  uint32_t* cnt = (uint32_t*)ws;
  hipLaunchKernelGGL((sub_excl_kernel<false>), grid, block, 0, st, a, cnt,
                     (const int64_t*)nullptr, (int64_t*)nullptr);
  rc = launch_check("sub_excl_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(sub_excl_scan_kernel, dim3(1), dim3(SC_THREADS), 0, st,
                     (const uint32_t*)cnt, B, off_out);
  rc = launch_check("sub_excl_scan_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((sub_excl_kernel<true>), grid, block, 0, st, a, cnt,
                     (const int64_t*)off_out, rows_out);
  return launch_check("sub_excl_kernel");
}

int ebt_sub_rows_to_global(int64_t* rows_inout, int64_t count, const int64_t* list, int64_t m,
                           void* stream) {
  const char* who = "ebt_sub_rows_to_global";
  if (count < 0 || m < 0) {
    set_error("%s: bad arguments (count=%lld m=%lld)", who, (long long)count, (long long)m);
    return EBT_EINVAL;
  }
  if (count == 0) return EBT_OK;
  if (!rows_inout || (m > 0 && !list)) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  hipLaunchKernelGGL(sub_rows_to_global_kernel,
                     dim3((unsigned)grid_for(count, SC_THREADS, 1 << 16)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, rows_inout, count, list, m);
  return launch_check("sub_rows_to_global_kernel");
}

}  // extern "C"
