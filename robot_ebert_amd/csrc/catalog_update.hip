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
//
// The catalog lifecycle entries of the C ABI (ebt_catalog_state_bytes, _init, _init_reserved,
// _update_rows, _append_rows, _remove_plan, _remove_rows) follow their kernels, at the end.
#include <cmath>
#include <vector>

#include "common.h"
#include "driver.h"

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

// Host side: every argument was checked by the caller (below); `rows` is a device array or
// NULL (append: local rows row0 .. row0 + m - 1). img == NULL when the matrix is its own image.
static int catalog_update(void* data, int dtype, int32_t d, int64_t ld, const int64_t* rows,
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
  UpdArgs a;
  a.data = data; a.ld = ld; a.d = d; a.rows = rows; a.row_offset = row_offset; a.row0 = row0;
  a.m = m; a.src = src; a.ld_src = ld_src; a.gnorm = gnorm; a.inv32 = inv32;
  a.img = (uint16_t*)img; a.ld_img = ld_img; a.normalize = normalize; a.err_max = err_max;
  a.src_vec = vec_ok(src, src_dtype, ld_src, 0);
  a.cat_vec = vec_ok(data, dtype, ld, 0);
  a.stage = d <= UPD_STAGE_MAX_D;
  int64_t blocks = ceil_div(m, 4);
  if (blocks > 4096) blocks = 4096;
  dim3 grid((unsigned)blocks), block(256);
  const size_t lds = a.stage ? (size_t)4 * d * sizeof(double) : 0;
  // the image dtype follows the catalog's (want_img above), the source's is free; the last
  // choice is row_norms' own test for its vector form
  for_dtype(dtype, [&](auto dc) {
    constexpr int DC = decltype(dc)::value, IMG = DC == EBT_BF16 ? EBT_BF16 : EBT_F16;
    for_dtype(src_dtype, [&](auto ds) {
      for_bool(vec_ok(data, dtype, ld, d), [&](auto vec) {
        hipLaunchKernelGGL(
            (catalog_update_kernel<DC, decltype(ds)::value, IMG, decltype(vec)::value>), grid,
            block, lds, st, a);
      });
    });
  });
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

// Host side: every argument was checked by the caller (below); `moves` is a device array of
// p (src, dst) pairs of LOCAL rows. img == NULL when the matrix is its own image.
static int catalog_move(void* data, int dtype, int32_t d, int64_t ld, const int64_t* moves, int64_t p,
                 int64_t n_new, int64_t n_old, double* gnorm, float* inv32, void* img,
                 int32_t ld_img, hipStream_t st) {
  if (!data || !gnorm || !inv32 || p < 0 || (p > 0 && !moves) || d <= 0 || ld < d || dtype < 0 ||
      dtype > 3 || n_new < 1 || n_old < n_new || p > n_old - n_new ||
      (img && (ld_img < d || ld_img % 64 != 0 || ((uintptr_t)img & 15)))) {
    set_error("catalog_move: bad arguments");
    return EBT_EINVAL;
  }
  if (p == 0) return EBT_OK;
  MoveArgs a;
  a.data = data; a.ld = ld; a.d = d; a.moves = moves; a.p = p; a.n_new = n_new; a.n_old = n_old;
  a.gnorm = gnorm; a.inv32 = inv32; a.img = (uint16_t*)img; a.ld_img = ld_img;
  a.cat_vec = vec_ok(data, dtype, ld, 0);
  int64_t blocks = ceil_div(p, 4);
  if (blocks > 4096) blocks = 4096;
  dim3 grid((unsigned)blocks), block(256);
  switch (dtype_size(dtype)) {
    case 8: hipLaunchKernelGGL((catalog_move_kernel<uint64_t>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((catalog_move_kernel<uint32_t>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((catalog_move_kernel<uint16_t>), grid, block, 0, st, a); break;
  }
  return launch_check("catalog_move_kernel");
}

namespace {

// The catalog state for n_cap rows: gnorm64 [n_cap] at 0, inv32 [round_up(n_cap, 128)], the
// image [n_cap][d_pad] unless the matrix is its own image (alias), and for a non-native catalog
// the slot of the image's measured rounding error. bytes == 0: refused sizes.
struct StateLayout {
  size_t inv32, img, err, bytes;
  bool native, alias;
};
StateLayout state_layout(const void* data, int dtype, int64_t n_cap, int32_t d, int64_t ld) {
  StateLayout L{};
  if (n_cap < 1 || d < 1 || ld < d || dtype < 0 || dtype > 3) return L;
  L.native = dtype == EBT_F16 || dtype == EBT_BF16;
  L.alias = L.native && d % 64 == 0 && ld % 64 == 0 && ((uintptr_t)data & 15) == 0;
  size_t o = 0;
  carve(o, (size_t)n_cap * 8);
  L.inv32 = carve(o, (size_t)round_up(n_cap, 128) * 4);
  L.img = carve(o, L.alias ? 0 : (size_t)n_cap * round_up(d, 64) * 2);
  L.err = carve(o, L.native ? 0 : 4);
  L.bytes = o;
  return L;
}

constexpr int ONE_F32_BITS = 0x3f800000;

// the image's measured rounding error read back from its slot (one stream sync)
int read_u_cat(const unsigned int* d_err, hipStream_t st, float* u_cat) {
  float u = 0.0f;
  int rc = hip_check(hipMemcpyAsync(&u, d_err, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  if (!rc) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (!rc) *u_cat = std::isfinite(u) && u >= 0.0f ? u : 1.0f / 2048.0f;
  return rc;
}

// m GLOBAL rows of the catalog rows [row_offset, row_offset + n), strictly ascending; else the
// error is set
bool rows_ascending(const char* who, const int64_t* rows, int64_t m, int64_t row_offset,
                    int64_t n) {
  for (int64_t i = 0; i < m; ++i) {
    if (rows[i] < row_offset || rows[i] >= row_offset + n) {
      set_error("%s: rows[%lld] = %lld is not in [%lld, %lld)", who, (long long)i,
                (long long)rows[i], (long long)row_offset, (long long)(row_offset + n));
      return false;
    }
    if (i > 0 && rows[i] <= rows[i - 1]) {
      set_error("%s: rows must be strictly ascending (rows[%lld] = %lld after %lld)", who,
                (long long)i, (long long)rows[i], (long long)rows[i - 1]);
      return false;
    }
  }
  return true;
}

}  // namespace

}  // namespace ebt

using namespace ebt;

extern "C" {

size_t ebt_catalog_state_bytes(const void* data, int dtype, int64_t n, int32_t d, int64_t ld) {
  return state_layout(data, dtype, n, d, ld).bytes;
}

// ebt_catalog_init (n_cap == n) and ebt_catalog_init_reserved: the state is laid out for n_cap
// rows and initialised for the first n
static int catalog_init_cap(const char* who, ebt_catalog* cat, const void* data, int dtype,
                            int64_t n, int64_t n_cap, int32_t d, int64_t ld, int64_t row_offset,
                            void* state, size_t state_bytes, void* stream) {
  const StateLayout SL = n_cap >= n ? state_layout(data, dtype, n_cap, d, ld) : StateLayout{};
  const size_t need = SL.bytes;
  if (!cat || !data || !state || need == 0 || n < 1 || row_offset < 0) {
    set_error("%s: bad arguments (n=%lld n_cap=%lld d=%d ld=%lld dtype=%d)", who, (long long)n,
              (long long)n_cap, d, (long long)ld, dtype);
    return EBT_EINVAL;
  }
  if (state_bytes < need) {
    set_error("%s: state %zu < %zu bytes", who, state_bytes, need);
    return EBT_ENOMEM;
  }
  hipStream_t st = (hipStream_t)stream;
  ebt_catalog c{};
  c.data = data;
  c.dtype = dtype;
  c.d = d;
  c.n = n;
  c.ld = ld;
  c.row_offset = row_offset;
  c.d_pad = (int32_t)round_up(d, 64);
  char* s = (char*)state;
  c.gnorm64 = (double*)s;
  c.inv32 = (float*)(s + SL.inv32);
  char* img = s + SL.img;
  int rc = EBT_OK;
  if (round_up(n_cap, 128) > n)  // inv32 past the rows: 1.0f
    rc = hip_check(hipMemsetD32Async((hipDeviceptr_t)(c.inv32 + n), ONE_F32_BITS,
                                     (size_t)(round_up(n_cap, 128) - n), st), "hipMemsetD32Async");
  if (!rc) rc = ebt_row_norms(data, dtype, n, d, ld, c.gnorm64, c.inv32, st);
  if (rc) return rc;
  if (SL.native) {
    c.img_dtype = dtype;
    c.u_cat = 0.0f;
    c.cscale = c.inv32;
    c.native = 1;
    if (SL.alias) {
      c.image = data;  // the matrix itself is the MFMA operand
      c.ld_img = (int32_t)ld;
    } else {
      c.ld_img = c.d_pad;
      c.image = img;
      rc = ebt_screen_image(data, dtype, n, d, ld, c.gnorm64, 0, c.img_dtype, img, c.ld_img, st);
    }
  } else {
    // f16 image of the normalised rows. u_cat = the largest ||image row - row / gnorm||_2 over
    // the rows, measured by the image kernel (rounded up to a float; rows with non-finite
    // values left out) -- ~0.4 x the unit round-off 2^-11 that bounds it a priori, so the
    // certificate's eps band (and the rows the rescore gathers) is about half as wide; one
    // stream sync to read it back, once per catalog
    c.img_dtype = EBT_F16;
    c.cscale = nullptr;
    c.native = 0;
    c.ld_img = c.d_pad;
    c.image = img;
    unsigned int* d_err = (unsigned int*)(s + SL.err);
    rc = hip_check(hipMemsetAsync(d_err, 0, 4, st), "hipMemsetAsync");
    if (!rc)
      rc = screen_image(data, dtype, n, d, ld, c.gnorm64, 1, c.img_dtype, img, c.ld_img, st,
                        d_err);
    if (!rc) rc = read_u_cat(d_err, st, &c.u_cat);
  }
  if (rc) return rc;
  *cat = c;
  return EBT_OK;
}

int ebt_catalog_init(ebt_catalog* cat, const void* data, int dtype, int64_t n, int32_t d,
                     int64_t ld, int64_t row_offset, void* state, size_t state_bytes,
                     void* stream) {
  return catalog_init_cap("ebt_catalog_init", cat, data, dtype, n, n, d, ld, row_offset, state,
                          state_bytes, stream);
}

int ebt_catalog_init_reserved(ebt_catalog* cat, const void* data, int dtype, int64_t n,
                              int64_t n_cap, int32_t d, int64_t ld, int64_t row_offset,
                              void* state, size_t state_bytes, void* stream) {
  return catalog_init_cap("ebt_catalog_init_reserved", cat, data, dtype, n, n_cap, d, ld,
                          row_offset, state, state_bytes, stream);
}

// ---- live updates (0.4.0): catalog_update_kernel ------------------------------------------------
size_t ebt_catalog_update_bytes(int64_t m) { return m > 0 ? align_up((size_t)m * 8) : 0; }

namespace {

// Where catalog_init_cap put the parts of a state laid out for n_cap rows
struct StateParts {
  double* gnorm;
  float* inv32;
  void* img;              // NULL: the matrix is its own image
  unsigned int* err;      // NULL for a native catalog
};

// Host checks shared by the two update entries: *cat is a catalog that catalog_init_cap laid out
// in `state` for n_cap rows, and the source is usable
int update_check(const char* who, const ebt_catalog* cat, void* state, size_t state_bytes,
                 int64_t n_cap, int64_t m, const void* src, int src_dtype, int64_t ld_src,
                 StateParts* out) {
  if (!valid_catalog(cat) || !state || cat->dtype < 0 || cat->dtype > 3 || cat->row_offset < 0) {
    set_error("%s: bad catalog or state", who);
    return EBT_EINVAL;
  }
  const ebt_catalog& c = *cat;
  if (m < 0 || src_dtype < 0 || src_dtype > 3 || (m > 0 && (!src || ld_src < c.d))) {
    set_error("%s: bad source (m=%lld src_dtype=%d ld_src=%lld d=%d)", who, (long long)m,
              src_dtype, (long long)ld_src, c.d);
    return EBT_EINVAL;
  }
  const StateLayout SL =
      n_cap >= c.n ? state_layout(c.data, c.dtype, n_cap, c.d, c.ld) : StateLayout{};
  const size_t need = SL.bytes;
  if (need == 0 || state_bytes < need) {
    set_error("%s: n_cap %lld (n %lld) needs a state of %zu bytes, got %zu", who,
              (long long)n_cap, (long long)c.n, need, state_bytes);
    return EBT_EINVAL;
  }
  const bool native = SL.native, alias = SL.alias;
  char* s = (char*)state;
  char* img = s + SL.img;
  StateParts P;
  P.gnorm = (double*)s;
  P.inv32 = (float*)(s + SL.inv32);
  P.img = alias ? nullptr : img;
  P.err = native ? nullptr : (unsigned int*)(s + SL.err);
  const void* want_image = alias ? c.data : (const void*)img;
  const int32_t want_ld_img = alias ? (int32_t)c.ld : c.d_pad;
  const int want_img_dtype = native ? c.dtype : EBT_F16;
  if (c.gnorm64 != P.gnorm || c.inv32 != P.inv32 || c.image != want_image ||
      c.ld_img != want_ld_img || c.img_dtype != want_img_dtype || c.native != (native ? 1 : 0) ||
      c.cscale != (native ? P.inv32 : nullptr) || c.d_pad != (int32_t)round_up(c.d, 64)) {
    set_error("%s: the catalog is not laid out in this state for n_cap = %lld (a catalog of "
              "ebt_catalog_init / _reserved with the same capacity is required)", who,
              (long long)n_cap);
    return EBT_EINVAL;
  }
  *out = P;
  return EBT_OK;
}

// the kernel, then for a non-native catalog the error slot read back into cat->u_cat
int update_launch(ebt_catalog* cat, const StateParts& P, const int64_t* d_rows, int64_t row0,
                  int64_t m, const void* src, int src_dtype, int64_t ld_src, hipStream_t st) {
  const ebt_catalog& c = *cat;
  int rc = catalog_update(const_cast<void*>(c.data), c.dtype, c.d, c.ld, d_rows, c.row_offset,
                          row0, m, src, src_dtype, ld_src, P.gnorm, P.inv32, P.img, c.img_dtype,
                          c.ld_img, c.native ? 0 : 1, P.err, st);
  if (rc || !P.err) return rc;
  return read_u_cat(P.err, st, &cat->u_cat);
}

}  // namespace

int ebt_catalog_update_rows(ebt_catalog* cat, void* state, size_t state_bytes, int64_t n_cap,
                            const int64_t* rows, int64_t m, const void* src, int src_dtype,
                            int64_t ld_src, void* ws, size_t ws_bytes, void* stream) {
  StateParts P;
  int rc = update_check("ebt_catalog_update_rows", cat, state, state_bytes, n_cap, m, src,
                        src_dtype, ld_src, &P);
  if (rc) return rc;
  if (m == 0) return EBT_OK;
  const ebt_catalog& c = *cat;
  if (!rows) {
    set_error("ebt_catalog_update_rows: rows is NULL");
    return EBT_EINVAL;
  }
  if (!rows_ascending("ebt_catalog_update_rows", rows, m, c.row_offset, c.n)) return EBT_EINVAL;
  const size_t need = ebt_catalog_update_bytes(m);
  if (!ws || ws_bytes < need) {
    set_error("ebt_catalog_update_rows: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0,
              need);
    return EBT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  rc = hip_check(hipMemcpyAsync(ws, rows, (size_t)m * 8, hipMemcpyHostToDevice, st),
                 "hipMemcpyAsync");
  if (rc) return rc;
  return update_launch(cat, P, (const int64_t*)ws, 0, m, src, src_dtype, ld_src, st);
}

int ebt_catalog_append_rows(ebt_catalog* cat, void* state, size_t state_bytes, int64_t n_cap,
                            int64_t m, const void* src, int src_dtype, int64_t ld_src,
                            void* stream) {
  StateParts P;
  int rc = update_check("ebt_catalog_append_rows", cat, state, state_bytes, n_cap, m, src,
                        src_dtype, ld_src, &P);
  if (rc) return rc;
  if (m > n_cap - cat->n) {
    set_error("ebt_catalog_append_rows: n %lld + m %lld > n_cap %lld", (long long)cat->n,
              (long long)m, (long long)n_cap);
    return EBT_EINVAL;
  }
  if (m == 0) return EBT_OK;
  rc = update_launch(cat, P, nullptr, cat->n, m, src, src_dtype, ld_src, (hipStream_t)stream);
  if (rc) return rc;
  cat->n += m;
  return EBT_OK;
}

// ---- removal (0.5.0): catalog_move_kernel -----------------------------------------------------
size_t ebt_catalog_remove_bytes(int64_t m) { return m > 0 ? align_up((size_t)m * 16) : 0; }

namespace {

// The rule of ebert.h: with n' = n - m, the removed rows below n' (the holes, ascending) receive
// the rows of [n', n) that are not removed (the survivors, ascending). `rows` is checked; the p
// moves go to from / to (GLOBAL rows) when given. Returns p, or -1 with the error set.
int64_t remove_plan(const char* who, int64_t n, int64_t row_offset, const int64_t* rows,
                    int64_t m, int64_t* from, int64_t* to) {
  if (n < 1 || row_offset < 0 || m < 0 || (m > 0 && !rows) || ((from == nullptr) != (to == nullptr))) {
    set_error("%s: bad arguments (n=%lld row_offset=%lld m=%lld; from / to both or neither)", who,
              (long long)n, (long long)row_offset, (long long)m);
    return -1;
  }
  if (!rows_ascending(who, rows, m, row_offset, n)) return -1;
  if (m >= n) {
    set_error("%s: cannot remove every row (m %lld >= n %lld)", who, (long long)m, (long long)n);
    return -1;
  }
  const int64_t n_new = n - m;
  int64_t p = 0;
  while (p < m && rows[p] - row_offset < n_new) ++p;   // the holes are rows[0 .. p)
  // rows[p .. m) are the removed rows of [n', n): the survivors are the others, p of them
  int64_t t = p, s = n_new;
  for (int64_t i = 0; i < p; ++i, ++s) {
    while (t < m && rows[t] - row_offset == s) ++t, ++s;
    if (from) {
      from[i] = row_offset + s;
      to[i] = rows[i];
    }
  }
  return p;
}

}  // namespace

int64_t ebt_catalog_remove_plan(int64_t n, int64_t row_offset, const int64_t* rows, int64_t m,
                                int64_t* from, int64_t* to) {
  return remove_plan("ebt_catalog_remove_plan", n, row_offset, rows, m, from, to);
}

int ebt_catalog_remove_rows(ebt_catalog* cat, void* state, size_t state_bytes, int64_t n_cap,
                            const int64_t* rows, int64_t m, void* ws, size_t ws_bytes,
                            void* stream) {
  const char* who = "ebt_catalog_remove_rows";
  StateParts P;
  int rc = update_check(who, cat, state, state_bytes, n_cap, 0, nullptr, 0, 0, &P);
  if (rc) return rc;
  if (m < 0) {
    set_error("%s: m = %lld", who, (long long)m);
    return EBT_EINVAL;
  }
  if (m == 0) return EBT_OK;
  if (!rows) {
    set_error("%s: rows is NULL", who);
    return EBT_EINVAL;
  }
  const ebt_catalog& c = *cat;
  std::vector<int64_t> from((size_t)m), to((size_t)m);
  const int64_t p = remove_plan(who, c.n, c.row_offset, rows, m, from.data(), to.data());
  if (p < 0) return EBT_EINVAL;
  const size_t need = ebt_catalog_remove_bytes(m);
  if (!ws || ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, ws ? ws_bytes : (size_t)0, need);
    return EBT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_new = c.n - m;
  if (p > 0) {
    std::vector<int64_t> pairs((size_t)p * 2);   // LOCAL (src, dst)
    for (int64_t i = 0; i < p; ++i) {
      pairs[2 * i] = from[i] - c.row_offset;
      pairs[2 * i + 1] = to[i] - c.row_offset;
    }
    // a copy from pageable memory has left the host buffer when the call returns
    rc = hip_check(hipMemcpyAsync(ws, pairs.data(), (size_t)p * 16, hipMemcpyHostToDevice, st),
                   "hipMemcpyAsync");
    if (!rc)
      rc = catalog_move(const_cast<void*>(c.data), c.dtype, c.d, c.ld, (const int64_t*)ws, p,
                        n_new, c.n, P.gnorm, P.inv32, P.img, c.ld_img, st);
    if (rc) return rc;
  }
  // after the moves, which read inv32 in this range: rows past n' hold 1.0f again
  rc = hip_check(hipMemsetD32Async((hipDeviceptr_t)(P.inv32 + n_new), ONE_F32_BITS, (size_t)m, st),
                 "hipMemsetD32Async");
  if (rc) return rc;
  cat->n = n_new;
  return EBT_OK;
}

}  // extern "C"
