// The candidate-buffer primitives of the streaming selects (select_topk.hip, grouped.hip): a
// 256-thread workgroup keeps (key, index) entries in LDS, compacts them to their `rank` best by
// an adaptive-range radix select over the 64-bit composite (key, ~index), and sorts the survivors
// with a bitonic network. Moved here unchanged from select_topk.hip so that the grouped select
// uses the same code, not a copy of it.
#pragma once

#include "common.h"

namespace ebt {

constexpr int STHREADS = 256;
constexpr int SHIST = 2048;             // histogram bins (11 bits)

__host__ __device__ inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

__device__ __forceinline__ uint64_t comp_of(uint32_t key, uint32_t idx) {
  return ((uint64_t)key << 32) | (uint64_t)(~idx);
}

// block-wide min / max of u64 (all threads get the result). red: >= 8 u64 of LDS.
__device__ __forceinline__ void block_minmax_u64(uint64_t& mn, uint64_t& mx, uint64_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint64_t a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  const int w = threadIdx.x >> 6;
  lds_barrier();
  if ((threadIdx.x & 63) == 0) {
    red[w] = mn;
    red[4 + w] = mx;
  }
  lds_barrier();
  mn = red[0];
  mx = red[4];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    mn = red[i] < mn ? red[i] : mn;
    mx = red[4 + i] > mx ? red[4 + i] : mx;
  }
}

// theta = the rank-th largest composite among the n buffer entries (1 <= rank <= n).
// hist: SHIST u32; red: 8 u64; misc: 12 u32 (all LDS).
__device__ inline uint64_t select_rank(const uint32_t* bkey, const uint32_t* bidx, int n, int rank,
                                       uint32_t* hist, uint64_t* red, uint32_t* misc) {
  const int tid = threadIdx.x;
  uint64_t lo = 0, hi = ~0ull;
  int r = rank;
  for (int iter = 0; iter < 16; ++iter) {
    uint64_t mn = ~0ull, mx = 0;
    for (int i = tid; i < n; i += STHREADS) {
      const uint64_t c = comp_of(bkey[i], bidx[i]);
      if (c >= lo && c <= hi) {
        mn = c < mn ? c : mn;
        mx = c > mx ? c : mx;
      }
    }
    block_minmax_u64(mn, mx, red);
    if (mn == mx) return mn;
    const uint64_t span = mx - mn;
    const int bits = 64 - __builtin_clzll(span);
    const int shift = bits > 11 ? bits - 11 : 0;
#pragma unroll
    for (int j = 0; j < SHIST / STHREADS; ++j) hist[tid * (SHIST / STHREADS) + j] = 0;
    lds_barrier();
    for (int i = tid; i < n; i += STHREADS) {
      const uint64_t c = comp_of(bkey[i], bidx[i]);
      if (c >= mn && c <= mx) atomicAdd(&hist[(uint32_t)((c - mn) >> shift)], 1u);
    }
    lds_barrier();
    // suffix scan: thread t owns bins [8t, 8t+8)
    uint32_t hv[SHIST / STHREADS];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < SHIST / STHREADS; ++j) {
      hv[j] = hist[tid * (SHIST / STHREADS) + j];
      s += hv[j];
    }
    uint32_t x = s;  // inclusive suffix within the wave (lanes >= me)
    const int lane = tid & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t y = __shfl_down(x, o, 64);
      if (lane + o < 64) x += y;
    }
    uint32_t* wtot = misc + 8;
    if (lane == 0) wtot[tid >> 6] = x;
    lds_barrier();
    uint32_t above = x - s;
    for (int w2 = (tid >> 6) + 1; w2 < 4; ++w2) above += wtot[w2];
    if (above < (uint32_t)r && (uint32_t)r <= above + s) {
      uint32_t cum = above;
      for (int j = SHIST / STHREADS - 1; j >= 0; --j) {
        if (cum + hv[j] >= (uint32_t)r) {
          misc[0] = tid * (SHIST / STHREADS) + j;
          misc[1] = cum;
          break;
        }
        cum += hv[j];
      }
    }
    lds_barrier();
    const uint32_t b = misc[0];
    r -= (int)misc[1];
    lds_barrier();  // misc reused next iteration
    lo = mn + ((uint64_t)b << shift);
    const uint64_t w = (shift >= 64) ? ~0ull : ((1ull << shift) - 1);
    hi = (mx - lo) < w ? mx : lo + w;
    if (shift == 0) return lo;
  }
  return lo;  // not reached for unique composites
}

// Keep exactly min(rank, n) best entries: buffer -> keep (unordered) -> buffer[0..).
// Returns theta (rank-th composite). n > rank required. keep: >= rank u64, may alias hist.
__device__ inline uint64_t compact(uint32_t* bkey, uint32_t* bidx, int n, int rank, uint64_t* keep,
                                   uint32_t* hist, uint64_t* red, uint32_t* misc) {
  const uint64_t theta = select_rank(bkey, bidx, n, rank, hist, red, misc);
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) misc[2] = 0;
  lds_barrier();  // hist (aliased with keep) is dead from here
  for (int base = 0; base < n; base += STHREADS) {
    const int i = base + tid;
    uint64_t c = 0;
    bool take = false;
    if (i < n) {
      c = comp_of(bkey[i], bidx[i]);
      take = c >= theta;
    }
    const uint64_t m = __ballot(take);
    if (m) {
      uint32_t wb = 0;
      if (lane == 0) wb = atomicAdd(&misc[2], (uint32_t)__popcll(m));
      wb = __shfl(wb, 0, 64);
      if (take) {
        const uint32_t pos = wb + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        keep[pos] = c;
      }
    }
  }
  lds_barrier();
  for (int i = tid; i < rank; i += STHREADS) {
    const uint64_t c = keep[i];
    bkey[i] = (uint32_t)(c >> 32);
    bidx[i] = ~(uint32_t)c;
  }
  lds_barrier();
  return theta;
}

// Descending bitonic sort of keep[0..P) (P power of two).
__device__ inline void bitonic_desc(uint64_t* keep, int P) {
  const int tid = threadIdx.x;
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += STHREADS) {
        // stride is a power of two: 2 stride (t / stride) + t % stride without a division
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        const int hi = lo + stride;
        const uint64_t a = keep[lo], b = keep[hi];
        const bool desc = (lo & size) == 0;
        if ((a < b) == desc) {
          keep[lo] = b;
          keep[hi] = a;
        }
      }
      lds_barrier();
    }
  }
}

}  // namespace ebt
