// The float64 FMA tile of the two kernels that score every (query, row) pair exactly:
// screen_exact_kernel (rescore.hip, the EXACT screen) and exact_keys_kernel (large_k.hip, the
// full sort). One workgroup of 256 threads takes XT queries x XT rows, 4 x 4 per thread, K in steps
// of XK through LDS; each product is accumulated by one __builtin_fma per element of d, d
// ascending, so both kernels hold the same float64 dot product per pair (and then divide it by the
// same gnorm): the value depends on the query, the row and d only. Each kernel keeps its epilogue.
#pragma once

#include "common.h"

namespace ebt {

constexpr int XT = 64, XK = 16;

// acc[i][j] = q64[q_at + i] . cat[r_at + j] (0 where the query or the row lies outside)
template <int DT>
__device__ __forceinline__ void exact_tile_f64(const double* __restrict__ q64, int64_t B, int d,
                                               const void* __restrict__ cat, int64_t ld,
                                               int64_t n_rows, double (&acc)[4][4], int64_t& q_at,
                                               int64_t& r_at) {
  __shared__ double qs[XK][XT + 1], cs[XK][XT + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * XT, b0 = (int64_t)blockIdx.y * XT;
  for (int k0 = 0; k0 < d; k0 += XK) {
    // the tile's 4 elements per thread loaded before any is stored (guarded loads would each
    // be waited for in turn): out-of-range indices read a clamped in-range element, then 0
    constexpr int NE = XT * XK / 256;
    double cv[NE], qv[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + 256 * u;
      const int rr = e / XK, kk = e % XK;
      const int64_t row = r0 + rr, qb = b0 + rr;
      const int kc = k0 + kk < d ? k0 + kk : d - 1;
      cv[u] = load_as_f64<DT>(cat, (row < n_rows ? row : n_rows - 1) * ld + kc);
      qv[u] = q64[(qb < B ? qb : B - 1) * d + kc];
    }
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + 256 * u;
      const int rr = e / XK, kk = e % XK;
      const int64_t row = r0 + rr, qb = b0 + rr;
      const bool kin = k0 + kk < d;
      cs[kk][rr] = (kin && row < n_rows) ? cv[u] : 0.0;
      qs[kk][rr] = (kin && qb < B) ? qv[u] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < XK; ++kk) {
      double a[4], c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = qs[kk][ty * 4 + i];
        c[i] = cs[kk][tx * 4 + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fma(a[i], c[j], acc[i][j]);
    }
    __syncthreads();
  }
  q_at = b0 + ty * 4;
  r_at = r0 + tx * 4;
}

}  // namespace ebt
