// Shared by the passes over a ROW-MAJOR full spectrum S[job][y][pitch] (full_fft.hip, full_sums.hip,
// fourier_crop.hip): which columns a workgroup owns, how it stages them in LDS, the sizes the row-major
// transforms take, the dispatch over them and the row passes' grid.
#pragma once
#include "mc_fft.h"
#include "mcorr.h"

// blockIdx.x -> column pair: the 8 pairs of one 128-byte line group on one XCD, consecutively
// (single columns, NC = 1: the same with 16 columns per group -- npairs is then the column count / 2
// and the caller maps block b to column 2 * full_pair_of_block(b >> 1, ..) + (b & 1))
__device__ __forceinline__ int full_pair_of_block(int b, int npairs) {
  const int ngroups = (npairs + 7) / 8;
  if (ngroups < 8) return b;  // tiny widths: no mapping
  const int xcd = b & 7, i = b >> 3;
  const int grp = i >> 3, within = i & 7;
  const int G = grp * 8 + xcd;
  // groups beyond the last multiple of 8 keep the plain order
  const int full = (ngroups / 8) * 8;
  if (b >= full * 8) return b;
  return G * 8 + within;
}

// The lane index, made opaque: every transform of a kernel derives its addresses and twiddle indices
// from its own copy, so the compiler cannot keep one transform's twiddles and addresses alive for the
// next (common-subexpression elimination across the unrolled column / direction loops cost 380
// registers for a 4092-point column pair).
__device__ __forceinline__ int full_opaque(int t) {
  asm volatile("" : "+v"(t));
  return t;
}

// first column of workgroup b (NC columns per workgroup), ncols = pitch
template <int NC>
__device__ __forceinline__ int full_col_of_block(int b, int pitch) {
  if constexpr (NC == 2) return 2 * full_pair_of_block(b, pitch / 2);
  else return 2 * full_pair_of_block(b >> 1, pitch / 2) + (b & 1);
}

// stage NC adjacent columns of S (rows `pitch` apart) into NC LDS lines / write them back.  All of a
// thread's loads are issued before the first LDS write (a rolled loop waits for every load in turn:
// H / WG memory round trips per column instead of one).
template <int H, int NC, int WG>
__device__ __forceinline__ void full_cols_load(cfloat* const* lines, const cfloat* base, int64_t pitch, int tid) {
  constexpr int IT = (H + WG - 1) / WG;
  if constexpr (NC == 2) {
    float4 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WG;
      if (i < H) v[it] = *reinterpret_cast<const float4*>(base + (int64_t)i * pitch);
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WG;
      if (i < H) {
        lines[0][lpad(i)] = cmake(v[it].x, v[it].y);
        lines[1][lpad(i)] = cmake(v[it].z, v[it].w);
      }
    }
  } else {
    cfloat v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WG;
      if (i < H) v[it] = base[(int64_t)i * pitch];
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WG;
      if (i < H) lines[0][lpad(i)] = v[it];
    }
  }
}
template <int H, int NC, int WG>
__device__ __forceinline__ void full_cols_store(cfloat* const* lines, cfloat* base, int pitch, int tid) {
  for (int i = tid; i < H; i += WG) {
    if constexpr (NC == 2) {
      const cfloat a = lines[0][lpad(i)], b = lines[1][lpad(i)];
      *reinterpret_cast<float4*>(base + (int64_t)i * pitch) = make_float4(a.x, a.y, b.x, b.y);
    } else {
      base[(int64_t)i * pitch] = lines[0][lpad(i)];
    }
  }
}

static inline bool full_rows_ok(int W) {
  return (mc_is_pow2(W) && W >= 64 && W <= 8192) || W == 5760 || W == 11520;
}
static inline bool full_cols_ok(int H) { return (mc_is_pow2(H) && H >= 256 && H <= 4096) || H == 4092 || H == 8184; }

// What Fourier cropping to a given size (fourier_crop_to.hip) adds, for its OUTPUT side alone: the heights its
// column pass comes out at and the widths mc_full_rows_inverse then takes (W / 2 = 1440, 1536, 1920, 3840 points).
// No forward pass and no other column pass takes them, so full_rows_ok / full_cols_ok stay what they were.
static inline bool full_crop_rows_ok(int W) { return W == 2880 || W == 3072 || W == 3840 || W == 7680; }
static inline bool full_crop_cols_ok(int H) { return H == 384 || H == 2046 || H == 2728 || H == 3072 || H == 5456; }
// the inverse row pass: every size of the transforms above, and the cropped ones
static inline bool full_rows_inverse_ok(int H, int W, int pitch) {
  return (full_rows_ok(W) || full_crop_rows_ok(W)) && (full_cols_ok(H) || full_crop_cols_ok(H)) &&
         pitch >= W / 2 + 1 && (pitch % 16) == 0;
}

// columns per workgroup: pairs while two lines fit twice into a CU's LDS, single columns above;
// threads per workgroup: 512 for 8184 rows (264 radix-31 butterflies per column)
template <int H>
constexpr int full_nc() { return H > 4096 ? 1 : 2; }
template <int H>
constexpr int full_wg() { return H > 4096 ? 512 : MC_WG; }

static inline bool full_sizes_ok(int H, int W, int pitch) {
  return full_rows_ok(W) && full_cols_ok(H) && pitch >= W / 2 + 1 && (pitch % 16) == 0;
}

// Row passes: 8 rows per workgroup (the kernels' rows_per_wg), one grid column per job
constexpr int FULL_ROWS_PER_WG = 8;
static inline dim3 full_rows_grid(int H, int njobs) {
  return dim3((H + FULL_ROWS_PER_WG - 1) / FULL_ROWS_PER_WG, njobs);
}

#define MC_FULL_CASE(V, ...) \
  case V: {                  \
    constexpr int L = V;     \
    __VA_ARGS__              \
  } break;
// complex points of a row line (W / 2)
#define MC_FULL_DISPATCH_ROWS(NV, ...)                                                              \
  switch (NV) {                                                                                     \
    MC_FULL_CASE(32, __VA_ARGS__) MC_FULL_CASE(64, __VA_ARGS__) MC_FULL_CASE(128, __VA_ARGS__)      \
    MC_FULL_CASE(256, __VA_ARGS__) MC_FULL_CASE(512, __VA_ARGS__) MC_FULL_CASE(1024, __VA_ARGS__)   \
    MC_FULL_CASE(2048, __VA_ARGS__) MC_FULL_CASE(4096, __VA_ARGS__) MC_FULL_CASE(2880, __VA_ARGS__) \
    MC_FULL_CASE(5760, __VA_ARGS__)                                                                 \
    default: return MC_ERR_UNSUPPORTED;                                                             \
  }
// the inverse row pass: those, and the lines of the cropped widths 2880, 3072, 3840 and 7680
#define MC_FULL_DISPATCH_ROWS_INVERSE(NV, ...)                                                        \
  switch (NV) {                                                                                       \
    MC_FULL_CASE(1440, __VA_ARGS__) MC_FULL_CASE(1536, __VA_ARGS__) MC_FULL_CASE(1920, __VA_ARGS__)   \
    MC_FULL_CASE(3840, __VA_ARGS__)                                                                   \
    default: MC_FULL_DISPATCH_ROWS(NV, __VA_ARGS__)                                                   \
  }
// rows of a column line (H) taken by the staged kernels (4096: the register-resident kernels)
#define MC_FULL_DISPATCH_COLS(HV, ...)                                                             \
  switch (HV) {                                                                                    \
    MC_FULL_CASE(256, __VA_ARGS__) MC_FULL_CASE(512, __VA_ARGS__) MC_FULL_CASE(1024, __VA_ARGS__)  \
    MC_FULL_CASE(2048, __VA_ARGS__) MC_FULL_CASE(4092, __VA_ARGS__) MC_FULL_CASE(8184, __VA_ARGS__) \
    default: return MC_ERR_UNSUPPORTED;                                                            \
  }

// signed frequency of row ky of an H-point transform (torch.fft.fftfreq)
__device__ __forceinline__ float full_fy(int ky, int H) {
  const int kk = (ky < (H + 1) / 2) ? ky : ky - H;
  return (float)kk * (float)(1.0 / (double)H);
}
