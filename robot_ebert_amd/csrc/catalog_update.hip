// Live catalog updates (ebert.h 0.4.0: ebt_catalog_update_rows / ebt_catalog_append_rows): one
// fused pass per replaced or appended row instead of a rebuild of the whole catalog state.
//
// catalog_update_kernel, in the style of prep.hip: one wave per updated row, four waves per
// block, grid-stride over the m rows. For its row a wave
//   A. reads the source row from HBM once (8 elements per lane per step: one 16-byte load for a
//      16-bit source, two for f32, four for f64, when the source rows are 16-byte aligned),
//      converts it to the catalog's dtype (round-to-nearest-even, narrowing to 16 bits through
//      float as torch's .to(dtype) does), writes it into data[row] (16-byte stores when the
//      catalog rows are aligned) and keeps the STORED value as float64 in LDS;
//   B. sums the squares with row_norms_kernel's lane-to-element assignment and order (its VEC
//      form iff vec_ok(data, dtype, ld, d)), wave_sum_f64, guard_norm -> gnorm64[row], inv32[row];
//   C. writes the image row with screen_image_kernel's arithmetic, f64_to_img_rt(v * (1 / g)), zero-
//      padded to ld_img (skipped when the matrix is its own image; the raw row when normalize = 0);
//   D. for a non-native catalog adds the row's ||image - x / g||_2 to the catalog's error slot by
//      the same unsigned max on the bits (summed per lane in screen_image_kernel's order).
// gnorm64, inv32 and the image are therefore bit-identical to what ebt_catalog_init computes for
// the edited matrix.
//
// Staging cut: the float64 row of each of the block's four waves lives in dynamic LDS,
// 4 * d * 8 bytes, for d <= UPD_STAGE_MAX_D = 2048 (64 KiB). A longer row is not staged: after a
// device-scope fence the wave re-reads the row it has just written to `data` (same values, same
// order of operations, one more pass over the row through L2).
//
// A NaN's payload is not kept by the conversion (it stays a NaN), also between equal dtypes.
//
// Removal (ebert.h 0.5.0: ebt_catalog_remove_rows): catalog_move_kernel, one wave per move
// (src, dst) of ebt_catalog_remove_plan, four waves per block, grid-stride over the p moves; no
// LDS, no barriers, no atomics. A wave copies the d elements of data[src] to data[dst] (the
// columns d .. ld are the caller's), the image row (unless the matrix is its own image), and
// gnorm64 / inv32. Nothing is recomputed: a row's norm and image row are functions of its values
// and of catalog-wide alignment only, so the copies are what ebt_catalog_init computes for the
// edited matrix. Every source is >= n' and every destination < n': no move reads what another
// writes. The kernel is bound by memory latency: a lane issues the loads of up to MOVE_AHEAD
// 16-byte chunks before their stores.
#include "common.h"

namespace ebt {

constexpr int UPD_STAGE_MAX_D = 2048;

struct UpdArgs {
  void* data;              // the catalog matrix [.][ld] of DT_CAT
  int64_t ld;
  int d;
  const int64_t* rows;     // device, m GLOBAL rows; NULL: rows row0, row0 + 1, ...
  int64_t row_offset;      // global id of local row 0
  int64_t row0;            // first LOCAL row when rows == NULL (append)
  int64_t m;
  const void* src;         // [m][ld_src] of DT_SRC
  int64_t ld_src;
  double* gnorm;
  float* inv32;
  uint16_t* img;           // NULL: the matrix is its own image
  int ld_img;
  int normalize;
  unsigned int* err_max;   // NULL for a native catalog
  int src_vec;             // source rows 16-byte aligned
  int cat_vec;             // catalog rows 16-byte aligned
  int stage;               // the row is kept in LDS (d <= UPD_STAGE_MAX_D)
};

// torch's float -> bfloat16 (c10 round_to_nearest_even): NaN -> 0x7FC0
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if (!(f == f)) return 0x7FC0;
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// (float)v that the compiler cannot fold with the 16-bit conversion after it into one rounding
// (common.h f64_to_img_rt): torch's double -> half goes through float
__device__ __forceinline__ float f32_kept(double v) {
  float f = (float)v;
  asm("" : "+v"(f));
  return f;
}

template <int DT>
__device__ __forceinline__ void upd_load8(const void* __restrict__ x, int64_t off, double (&v)[8]) {
  if constexpr (DT == EBT_F32) {
    const float4 a = *(const float4*)((const float*)x + off);
    const float4 b = *(const float4*)((const float*)x + off + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else if constexpr (DT == EBT_F64) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const double2 a = *(const double2*)((const double*)x + off + e);
      v[e] = a.x;
      v[e + 1] = a.y;
    }
  } else {
    const u16x8_t h = *(const u16x8_t*)((const uint16_t*)x + off);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      v[e] = DT == EBT_BF16 ? bf16_bits_to_f64(h[e]) : f16_bits_to_f64(h[e]);
  }
}

// One element: convert v to DT, store it at p[idx], return the stored value
template <int DT>
__device__ __forceinline__ double upd_store1(void* p, int64_t idx, double v) {
  if constexpr (DT == EBT_F64) {
    ((double*)p)[idx] = v;
    return v;
  } else if constexpr (DT == EBT_F32) {
    const float f = (float)v;
    ((float*)p)[idx] = f;
    return (double)f;
  } else if constexpr (DT == EBT_F16) {
    const _Float16 h = (_Float16)f32_kept(v);
    const uint16_t b = __builtin_bit_cast(uint16_t, h);
    ((uint16_t*)p)[idx] = b;
    return f16_bits_to_f64(b);
  } else {
    const uint16_t b = f32_to_bf16_rne((float)v);
    ((uint16_t*)p)[idx] = b;
    return bf16_bits_to_f64(b);
  }
}

// Eight elements at p[idx .. idx + 8), 16-byte aligned: v becomes the stored values
template <int DT>
__device__ __forceinline__ void upd_store8(void* p, int64_t idx, double (&v)[8]) {
  if constexpr (DT == EBT_F64) {
    double2* dst = (double2*)((double*)p + idx);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = make_double2(v[2 * e], v[2 * e + 1]);
  } else if constexpr (DT == EBT_F32) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = (float)v[e];
      v[e] = (double)f[e];
    }
    float4* dst = (float4*)((float*)p + idx);
    dst[0] = make_float4(f[0], f[1], f[2], f[3]);
    dst[1] = make_float4(f[4], f[5], f[6], f[7]);
  } else {
    u16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (DT == EBT_F16) {
        const _Float16 h = (_Float16)f32_kept(v[e]);
        o[e] = __builtin_bit_cast(uint16_t, h);
        v[e] = f16_bits_to_f64(o[e]);
      } else {
        o[e] = f32_to_bf16_rne((float)v[e]);
        v[e] = bf16_bits_to_f64(o[e]);
      }
    }
    *(u16x8_t*)((uint16_t*)p + idx) = o;
  }
}

// (image value - x)^2 in float64 (prep.hip sq_err)
template <int IMG>
__device__ __forceinline__ double upd_sq_err(uint16_t h, double x) {
  const double r = (IMG == EBT_F16 ? f16_bits_to_f64(h) : bf16_bits_to_f64(h)) - x;
  return r * r;
}

template <int DT_CAT, int DT_SRC, int IMG, bool VEC>
__global__ __launch_bounds__(256) void catalog_update_kernel(const UpdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double upd_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int d = a.d;
  double* __restrict__ buf = upd_lds + (size_t)w * d;   // used with a.stage only
  // every wave of a block takes the same number of turns (the barriers below)
  for (int64_t base = (int64_t)blockIdx.x * 4; base < a.m; base += (int64_t)gridDim.x * 4) {
    const int64_t i = base + w;
    const bool act = i < a.m;
    const int64_t row = !act ? 0 : (a.rows ? a.rows[i] - a.row_offset : a.row0 + i);
    // ---- A: source -> data[row] (and the stored values -> LDS)
    if (act) {
      const int nfull = d >> 3;
      for (int c = lane; c < nfull; c += 64) {
        double v[8];
        if (a.src_vec) {
          upd_load8<DT_SRC>(a.src, i * a.ld_src + c * 8, v);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = load_as_f64<DT_SRC>(a.src, i * a.ld_src + c * 8 + e);
        }
        if (a.cat_vec) {
          upd_store8<DT_CAT>(a.data, row * a.ld + c * 8, v);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = upd_store1<DT_CAT>(a.data, row * a.ld + c * 8 + e, v[e]);
        }
        if (a.stage) {
#pragma unroll
          for (int e = 0; e < 8; ++e) buf[c * 8 + e] = v[e];
        }
      }
      for (int j = nfull * 8 + lane; j < d; j += 64) {
        const double sv =
            upd_store1<DT_CAT>(a.data, row * a.ld + j, load_as_f64<DT_SRC>(a.src, i * a.ld_src + j));
        if (a.stage) buf[j] = sv;
      }
    }
    if (!a.stage) __threadfence();   // the row just written is read back below
    __syncthreads();
    if (act) {
      auto val = [&](int j) -> double {
        return a.stage ? buf[j] : load_as_f64<DT_CAT>(a.data, row * a.ld + j);
      };
      // ---- B: the guarded norm, row_norms_kernel's sums
      double s = 0.0;
      if constexpr (VEC) {
        constexpr int ES = (DT_CAT == EBT_F64) ? 8 : (DT_CAT == EBT_F32 ? 4 : 2);
        constexpr int PER = 16 / ES;  // elements per 16-byte chunk
        const int nchunks = d / PER;
        for (int c = lane; c < nchunks; c += 64) {
          double f[PER];
#pragma unroll
          for (int e = 0; e < PER; ++e) f[e] = val(c * PER + e);
          if constexpr (DT_CAT == EBT_F64) {
            s += f[0] * f[0] + f[1] * f[1];
          } else {
#pragma unroll
            for (int e = 0; e < PER; ++e) s += f[e] * f[e];
          }
        }
      } else {
        for (int j = lane; j < d; j += 64) {
          const double v = val(j);
          s += v * v;
        }
      }
      s = wave_sum_f64(s);
      const double g = guard_norm(sqrt(s));
      if (lane == 0) {
        a.gnorm[row] = g;
        a.inv32[row] = (float)(1.0 / g);
      }
      // ---- C, D: the image row and its error, screen_image_kernel's arithmetic and order
      if (a.img) {
        const double sc = a.normalize ? 1.0 / g : 1.0;
        const int cpr = a.ld_img / 8;
        double es = 0.0;
        for (int c = lane; c < cpr; c += 64) {
          u16x8_t o;
          if (a.cat_vec && c * 8 + 8 <= d) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const double v = val(c * 8 + e);
              o[e] = f64_to_img_rt<IMG>(v * sc);
              if (a.err_max) es += upd_sq_err<IMG>(o[e], v * sc);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int jj = c * 8 + e;
              const double x = jj < d ? val(jj) * sc : 0.0;
              o[e] = f64_to_img_rt<IMG>(x);
              if (a.err_max) es += upd_sq_err<IMG>(o[e], x);
            }
          }
          *(u16x8_t*)(a.img + row * a.ld_img + c * 8) = o;
        }
        if (a.err_max) {
          es = wave_sum_f64(es);
          if (lane == 0 && es <= 1.0) {   // a row with non-finite values is left out
            const double e = sqrt(es);
            float f = (float)e;
            if ((double)f < e) f = nextafterf(f, 1.0f);
            atomicMax(a.err_max, __float_as_uint(f));
          }
        }
      }
    }
    __syncthreads();   // the next turn overwrites the staged row
  }
}

// Host side: every argument was checked by the caller (driver.hip); `rows` is a device array or
// NULL (append: local rows row0 .. row0 + m - 1). img == NULL when the matrix is its own image.
int catalog_update(void* data, int dtype, int32_t d, int64_t ld, const int64_t* rows,
                   int64_t row_offset, int64_t row0, int64_t m, const void* src, int src_dtype,
                   int64_t ld_src, double* gnorm, float* inv32, void* img, int img_dtype,
                   int32_t ld_img, int normalize, unsigned int* err_max, hipStream_t st) {
  const int want_img = dtype == EBT_BF16 ? EBT_BF16 : EBT_F16;
  if (!data || !src || !gnorm || !inv32 || m < 0 || d <= 0 || ld < d || ld_src < d || dtype < 0 ||
      dtype > 3 || src_dtype < 0 || src_dtype > 3 || (img && (img_dtype != want_img ||
      ld_img < d || ld_img % 64 != 0 || ((uintptr_t)img & 15)))) {
    set_error("catalog_update: bad arguments");
    return EBT_EINVAL;
  }
  if (m == 0) return EBT_OK;
  const int es = dtype == EBT_F64 ? 8 : (dtype == EBT_F32 ? 4 : 2);
  const int ss = src_dtype == EBT_F64 ? 8 : (src_dtype == EBT_F32 ? 4 : 2);
  UpdArgs a;
  a.data = data; a.ld = ld; a.d = d; a.rows = rows; a.row_offset = row_offset; a.row0 = row0;
  a.m = m; a.src = src; a.ld_src = ld_src; a.gnorm = gnorm; a.inv32 = inv32;
  a.img = (uint16_t*)img; a.ld_img = ld_img; a.normalize = normalize; a.err_max = err_max;
  a.src_vec = ((uintptr_t)src & 15) == 0 && (ld_src * ss) % 16 == 0;
  a.cat_vec = ((uintptr_t)data & 15) == 0 && (ld * es) % 16 == 0;
  a.stage = d <= UPD_STAGE_MAX_D;
  // row_norms' own test for its vector form
  const bool v = a.cat_vec && ((int64_t)d * es) % 16 == 0;
  int64_t blocks = ceil_div(m, 4);
  if (blocks > 4096) blocks = 4096;
  dim3 grid((unsigned)blocks), block(256);
  const size_t lds = a.stage ? (size_t)4 * d * sizeof(double) : 0;
#define EBT_UP_V(DC, DS, IMG)                                                                  \
  if (v) hipLaunchKernelGGL((catalog_update_kernel<DC, DS, IMG, true>), grid, block, lds, st, a); \
  else hipLaunchKernelGGL((catalog_update_kernel<DC, DS, IMG, false>), grid, block, lds, st, a);
#define EBT_UP(DC, IMG)                                  \
  switch (src_dtype) {                                   \
    case EBT_F32: EBT_UP_V(DC, EBT_F32, IMG) break;      \
    case EBT_BF16: EBT_UP_V(DC, EBT_BF16, IMG) break;    \
    case EBT_F16: EBT_UP_V(DC, EBT_F16, IMG) break;      \
    default: EBT_UP_V(DC, EBT_F64, IMG) break;           \
  }
  switch (dtype) {
    case EBT_F32: EBT_UP(EBT_F32, EBT_F16) break;
    case EBT_BF16: EBT_UP(EBT_BF16, EBT_BF16) break;
    case EBT_F16: EBT_UP(EBT_F16, EBT_F16) break;
    default: EBT_UP(EBT_F64, EBT_F16) break;
  }
#undef EBT_UP
#undef EBT_UP_V
  return launch_check("catalog_update_kernel");
}

// ---- removal: rows moved into the holes -------------------------------------------------------
constexpr int MOVE_AHEAD = 4;   // 16-byte chunks a lane loads before it stores them

struct MoveArgs {
  void* data;              // the catalog matrix [.][ld]
  int64_t ld;
  int d;
  const int64_t* moves;    // device, p pairs (src, dst) of LOCAL rows
  int64_t p;
  int64_t n_new, n_old;    // every src in [n_new, n_old), every dst in [0, n_new)
  double* gnorm;
  float* inv32;
  uint16_t* img;           // NULL: the matrix is its own image
  int ld_img;
  int cat_vec;             // catalog rows 16-byte aligned
};

// nchunks 16-byte chunks from src to dst (both 16-byte aligned), MOVE_AHEAD loads in flight
__device__ __forceinline__ void move_chunks(const u16x8_t* __restrict__ src,
                                            u16x8_t* __restrict__ dst, int nchunks, int lane) {
  for (int c = lane; c < nchunks; c += 64 * MOVE_AHEAD) {
    u16x8_t v[MOVE_AHEAD];
#pragma unroll
    for (int u = 0; u < MOVE_AHEAD; ++u)
      if (c + 64 * u < nchunks) v[u] = src[c + 64 * u];
#pragma unroll
    for (int u = 0; u < MOVE_AHEAD; ++u)
      if (c + 64 * u < nchunks) dst[c + 64 * u] = v[u];
  }
}

// T: an unsigned integer of the element's size (the bits are copied, a NaN's payload included)
template <typename T>
__global__ __launch_bounds__(256) void catalog_move_kernel(const MoveArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int PER = 16 / (int)sizeof(T);   // elements per 16-byte chunk
  for (int64_t i = (int64_t)blockIdx.x * 4 + w; i < a.p; i += (int64_t)gridDim.x * 4) {
    const int64_t src = a.moves[2 * i], dst = a.moves[2 * i + 1];
    // the host's plan keeps to these ranges; a pair outside them is never followed
    if (src < a.n_new || src >= a.n_old || dst < 0 || dst >= a.n_new) continue;
    const T* __restrict__ s = (const T*)a.data + src * a.ld;
    T* __restrict__ t = (T*)a.data + dst * a.ld;
    const int nvec = a.cat_vec ? a.d / PER : 0;
    move_chunks((const u16x8_t*)s, (u16x8_t*)t, nvec, lane);
    for (int j = nvec * PER + lane; j < a.d; j += 64) t[j] = s[j];
    if (a.img)
      move_chunks((const u16x8_t*)(a.img + src * a.ld_img), (u16x8_t*)(a.img + dst * a.ld_img),
                  a.ld_img / 8, lane);
    if (lane == 0) {
      a.gnorm[dst] = a.gnorm[src];
      a.inv32[dst] = a.inv32[src];
    }
  }
}

// Host side: every argument was checked by the caller (driver.hip); `moves` is a device array of
// p (src, dst) pairs of LOCAL rows. img == NULL when the matrix is its own image.
int catalog_move(void* data, int dtype, int32_t d, int64_t ld, const int64_t* moves, int64_t p,
                 int64_t n_new, int64_t n_old, double* gnorm, float* inv32, void* img,
                 int32_t ld_img, hipStream_t st) {
  if (!data || !gnorm || !inv32 || p < 0 || (p > 0 && !moves) || d <= 0 || ld < d || dtype < 0 ||
      dtype > 3 || n_new < 1 || n_old < n_new || p > n_old - n_new ||
      (img && (ld_img < d || ld_img % 64 != 0 || ((uintptr_t)img & 15)))) {
    set_error("catalog_move: bad arguments");
    return EBT_EINVAL;
  }
  if (p == 0) return EBT_OK;
  const int es = dtype == EBT_F64 ? 8 : (dtype == EBT_F32 ? 4 : 2);
  MoveArgs a;
  a.data = data; a.ld = ld; a.d = d; a.moves = moves; a.p = p; a.n_new = n_new; a.n_old = n_old;
  a.gnorm = gnorm; a.inv32 = inv32; a.img = (uint16_t*)img; a.ld_img = ld_img;
  a.cat_vec = ((uintptr_t)data & 15) == 0 && (ld * es) % 16 == 0;
  int64_t blocks = ceil_div(p, 4);
  if (blocks > 4096) blocks = 4096;
  dim3 grid((unsigned)blocks), block(256);
  switch (es) {
    case 8: hipLaunchKernelGGL((catalog_move_kernel<uint64_t>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((catalog_move_kernel<uint32_t>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((catalog_move_kernel<uint16_t>), grid, block, 0, st, a); break;
  }
  return launch_check("catalog_move_kernel");
}

}  // namespace ebt
