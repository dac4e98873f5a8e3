// Per-query allow masks (include/ebert.h: ebt_allow, ebt_mask_allowed, ebt_allow_from_bool,
// ebt_allow_set_rows). Reference: lib.py:48,55 -- the candidate set is index.difference(rated),
// here intersected with the set of rows the query's mask allows.
//
//  * mask_allowed    -- every disallowed entry of a filtered query's score chunk becomes -inf
//                       (the unfused pipeline's second masking pass, right after mask_excluded).
//  * allow_from_bool -- one mask row packed from uint8 flags by wave-64 ballots.
//  * allow_set_rows  -- the bits of a list of GLOBAL rows set or cleared in one mask row.
//
// A mask row is uint32 words[words] (words % 4 == 0): global row r is allowed iff
// words[r >> 5] >> (r & 31) & 1, and rows >= 32 * words are not allowed.
#include "common.h"
#include "internal.h"

namespace ebt {

namespace {

constexpr int MA_THREADS = 256;
// aligned 4-column groups per thread: a workgroup covers 4096 columns (16 per thread measured
// slower at C3: 6.9 vs 5.9 ms per step at density 0.01, profiles/r9/allow/)
constexpr int MA_UNROLL = 4;

// The pass is store-bound: at density p it writes 4 B n (1 - p) bytes and reads 1/32 of that in
// mask words (8 neighbouring lanes share a word: one cache line serves 1024 columns). Stores are
// the widest the memory pipe takes, 16 bytes per lane on consecutive lanes (1 KiB per wave
// instruction); a fully allowed group costs no score traffic at all, a fully disallowed one a
// store with no load, and only a mixed group reads its four scores back. Plain stores: the
// non-temporal form measured the same (profiles/r9/allow/), and the select reads the chunk next.
__global__ __launch_bounds__(MA_THREADS) void mask_allowed_kernel(
    float* __restrict__ s, int64_t ld, int64_t B, int64_t c0, int64_t nc,
    const uint32_t* __restrict__ masks, int64_t words, int32_t n_masks,
    const int32_t* __restrict__ mask_id) {
  const int64_t groups = (nc + 3) >> 2;
  const int64_t g0 = (int64_t)blockIdx.x * (MA_THREADS * MA_UNROLL) + threadIdx.x;
  const float ninf = -__builtin_inff();
  // (grid.y = min(B, 65535): a workgroup takes its column block of every 65535-th query)
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const int32_t m = mask_id[b];
    if (m < 0) continue;  // unfiltered query: no score or mask word is loaded, nothing stored
    // an id past the table masks every row (and reads no mask word)
    const uint32_t* __restrict__ row = m < n_masks ? masks + (int64_t)m * words : nullptr;
    float* __restrict__ sb = s + b * ld;
#pragma unroll
    for (int u = 0; u < MA_UNROLL; ++u) {
      const int64_t g = g0 + (int64_t)u * MA_THREADS;
      if (g >= groups) break;
      const int64_t j = g << 2;  // first local column of the group (16-byte aligned in s)
      const int64_t r = c0 + j;  // its GLOBAL row: any alignment against the mask words
      const int64_t w = r >> 5;
      const int sh = (int)(r & 31);
      uint32_t lo = 0u, hi = 0u;
      if (row) {
        if (w < words) lo = row[w];
        if (sh > 28 && w + 1 < words) hi = row[w + 1];  // the four bits straddle two words
      }
      uint32_t allow = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh) & 0xFu;
      // columns of the group at or past nc (the padding up to ld) keep their values
      const int64_t left = nc - j;
      if (left < 4) allow |= (0xFu << left) & 0xFu;
      if (allow == 0xFu) continue;
      f32x4_t* p = (f32x4_t*)(sb + j);
      if (allow == 0u) {
        const f32x4_t v = {ninf, ninf, ninf, ninf};
        *p = v;
      } else {
        f32x4_t v = *p;
        v[0] = (allow & 1u) ? v[0] : ninf;
        v[1] = (allow & 2u) ? v[1] : ninf;
        v[2] = (allow & 4u) ? v[2] : ninf;
        v[3] = (allow & 8u) ? v[3] : ninf;
        *p = v;
      }
    }
  }
}

// word pair wp of the mask row <- the ballot of flags[64 wp .. 64 wp + 63] (0 past n)
__global__ __launch_bounds__(MA_THREADS) void allow_from_bool_kernel(
    const uint8_t* __restrict__ flags, int64_t n, uint32_t* __restrict__ mask_row,
    int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * MA_THREADS + threadIdx.x;
  const bool on = i < n && flags[i] != 0;
  const uint64_t bal = __ballot(on);
  const int64_t w = (i >> 6) << 1;  // words % 4 == 0: a wave's two words are both inside or not
  if (lane_id() == 0 && w < words) {
    uint2 v;
    v.x = (uint32_t)bal;
    v.y = (uint32_t)(bal >> 32);
    *(uint2*)(mask_row + w) = v;
  }
}

__global__ __launch_bounds__(MA_THREADS) void allow_set_rows_kernel(
    uint32_t* __restrict__ mask_row, int64_t words, const int64_t* __restrict__ rows, int64_t m,
    int allowed) {
  const int64_t i = (int64_t)blockIdx.x * MA_THREADS + threadIdx.x;
  if (i >= m) return;
  const int64_t r = rows[i];
  if (r < 0 || r >= words * 32) return;
  const uint32_t bit = 1u << (r & 31);
  if (allowed) atomicOr(mask_row + (r >> 5), bit);
  else atomicAnd(mask_row + (r >> 5), ~bit);
}

}  // namespace

static int64_t allow_words(int64_t n_rows) {
  if (n_rows < 1) return 0;
  return ((n_rows + 31) / 32 + 3) / 4 * 4;
}

// Host checks of an ebt_allow against the GLOBAL rows [0, row_end) it has to cover (no GPU call)
int check_allow(const ebt_allow* a, int64_t row_end, const char* who) {
  if (!a || !a->masks || !a->mask_id) {
    set_error("%s: null pointer in ebt_allow (masks, mask_id)", who);
    return EBT_EINVAL;
  }
  if (a->words < 1 || a->words % 4 != 0 || a->n_masks < 1) {
    set_error("%s: bad ebt_allow (words=%lld: >= 1 and a multiple of 4, ebt_allow_words; "
              "n_masks=%d: >= 1)", who, (long long)a->words, a->n_masks);
    return EBT_EINVAL;
  }
  if (((uintptr_t)a->masks & 15) != 0) {
    set_error("%s: ebt_allow.masks must be 16-byte aligned", who);
    return EBT_EINVAL;
  }
  if (a->words > (INT64_MAX >> 5) || a->words * 32 < row_end) {
    set_error("%s: ebt_allow.words=%lld covers rows [0, %lld), the scores reach row %lld "
              "(ebt_allow_words of the catalog's capacity)", who, (long long)a->words,
              (long long)(a->words > (INT64_MAX >> 5) ? 0 : a->words * 32), (long long)row_end);
    return EBT_EINVAL;
  }
  return EBT_OK;
}

int mask_allowed(float* s, int64_t ld, int64_t B, int64_t c0, int64_t c1, const ebt_allow* a,
                 hipStream_t st) {
  const char* who = "ebt_mask_allowed";
  if (!s) {
    set_error("%s: null pointer (scores)", who);
    return EBT_EINVAL;
  }
  if (B < 0 || c0 < 0 || c1 < c0 || ld < c1 - c0 || ld % 4 != 0 ||
      ((uintptr_t)s & 15) != 0) {
    set_error("%s: bad arguments (B=%lld, columns [%lld, %lld), ld=%lld: a multiple of "
              "4 and >= the columns, scores 16-byte aligned)", who, (long long)B, (long long)c0,
              (long long)c1, (long long)ld);
    return EBT_EINVAL;
  }
  const int rc = check_allow(a, c1, who);
  if (rc) return rc;
  const int64_t nc = c1 - c0;
  if (B == 0 || nc == 0) return EBT_OK;
  const int64_t groups = (nc + 3) / 4;
  const int64_t bx = ceil_div(groups, (int64_t)MA_THREADS * MA_UNROLL);
  hipLaunchKernelGGL(mask_allowed_kernel, dim3((unsigned)bx, (unsigned)(B < 65535 ? B : 65535)),
                     dim3(MA_THREADS), 0, st, s, ld, B, c0, nc, a->masks, a->words, a->n_masks,
                     a->mask_id);
  return launch_check("mask_allowed_kernel");
}

}  // namespace ebt

using namespace ebt;

extern "C" {

int64_t ebt_allow_words(int64_t n_rows) { return allow_words(n_rows); }

int ebt_allow_from_bool(const uint8_t* flags, int64_t n, uint32_t* mask_row, int64_t words,
                        void* stream) {
  const char* who = "ebt_allow_from_bool";
  if (!mask_row || (n > 0 && !flags)) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (n < 0 || words < 1 || words % 4 != 0 || words > (INT64_MAX >> 5) || words * 32 < n ||
      ((uintptr_t)mask_row & 15) != 0) {
    set_error("%s: bad arguments (n=%lld words=%lld: a multiple of 4 with 32 words >= n, "
              "ebt_allow_words; mask_row 16-byte aligned)", who, (long long)n, (long long)words);
    return EBT_EINVAL;
  }
  const int64_t blocks = ceil_div(words * 32, MA_THREADS);
  if (blocks > 0x7fffffff) {
    set_error("%s: words=%lld is too large", who, (long long)words);
    return EBT_EINVAL;
  }
  hipLaunchKernelGGL(allow_from_bool_kernel, dim3((unsigned)blocks), dim3(MA_THREADS), 0,
                     (hipStream_t)stream, flags, n, mask_row, words);
  return launch_check("allow_from_bool_kernel");
}

int ebt_allow_set_rows(uint32_t* mask_row, int64_t words, const int64_t* rows, int64_t m,
                       int allowed, void* stream) {
  const char* who = "ebt_allow_set_rows";
  if (!mask_row || (m > 0 && !rows)) {
    set_error("%s: null pointer", who);
    return EBT_EINVAL;
  }
  if (m < 0 || words < 1 || words > (INT64_MAX >> 5) || ceil_div(m, MA_THREADS) > 0x7fffffff) {
    set_error("%s: bad arguments (m=%lld words=%lld)", who, (long long)m, (long long)words);
    return EBT_EINVAL;
  }
  if (m == 0) return EBT_OK;
  hipLaunchKernelGGL(allow_set_rows_kernel, dim3((unsigned)ceil_div(m, MA_THREADS)),
                     dim3(MA_THREADS), 0, (hipStream_t)stream, mask_row, words, rows, m,
                     allowed ? 1 : 0);
  return launch_check("allow_set_rows_kernel");
}

int ebt_mask_allowed(float* scores, int64_t ld_scores, int64_t B, int64_t col_begin,
                     int64_t col_end, const ebt_allow* allow, void* stream) {
  return mask_allowed(scores, ld_scores, B, col_begin, col_end, allow, (hipStream_t)stream);
}

}  // extern "C"
