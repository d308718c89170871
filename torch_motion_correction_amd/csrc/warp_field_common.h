// What more than one of the deformation-field objects uses (field_tables.hip, warp_field.hip,
// warp_field_fallback.hip): the kernels' argument structs, the LDS window geometry, the weight and
// tap-sum helpers, the wave reductions, and the host side's scratch layout and kernel arguments.
//
// Reference path (correct_motion.py:18-185, deformation_field_utils.py:9-93): per frame
//   lattice(2,10gh,10gw) = spline(field)(t_i, linspace, linspace)
//   shifts(h,w,2)        = grid_sample(lattice, bicubic, reflection, align_corners) / pixel_spacing
//   out(h,w)             = grid_sample(frame, pixel+shift, bicubic, border, align_corners),
//                          zero where the coordinate leaves [0,h-1]x[0,w-1]
// The reference materialises the coordinate grid, the normalised grid and the shift
// grid (3 x 128 MiB per 4096^2 frame) and gathers 16+16 taps per pixel.  Here the
// x-direction of the shift upsample is hoisted into a small per-frame table
// E[c][lattice row][x] (the reference's own summation order: x taps first, then y),
// so each pixel needs 4 table rows per channel; coordinates live in registers only.
//
// The fp32 coordinate chain is reproduced operation by operation: at coordinates ~4096 one ulp is
// 2.4e-4 px, which is visible at the 1e-4 parity bar.  So the mode of the three objects is NO FMA
// contraction (each says `#pragma clang fp contract(off)` after its includes); the few helpers that form
// resampling weights and tap sums may contract and say so in their own bodies.  Every helper of this
// header sets its own mode at the start of its body, as warp_common.h does, and compiles the same
// wherever it is included (the integer-only ones have nothing to contract).
#pragma once
#include "warp_common.h"
#include "mcorr.h"

// s / d for a loop-invariant divisor, same three-instruction correctly rounded form
__device__ __forceinline__ float div_invariant(float s, float d) {
#pragma clang fp contract(off)
  const float r = 1.0f / d;
  const float q = s * r;
  return __builtin_fmaf(__builtin_fmaf(-q, d, s), r, q);
}

struct WarpArgs {
  const float* frames;
  int nframes, h, w, GH;
  const float* etab;   // [f][2][GH][w]
  const int* ytap;     // [h][4]
  const float* ycoef;  // [h][4]
  float pixel_spacing;
  float* out_frames;
  float* out_sum;
  int tiles_x, tiles_y;
};

struct FieldArgs {
  WarpArgs w;
  const float* lattice;  // [f][2][GH][GW]
  const int* xtap;       // [w][4]
  int GW;
  unsigned char* flags;  // [f][tile]: 1 = irregular, left to warp_field_slow
  const float* gain;     // raw frames (N2) only: (h, w) gain reference
  const float* mu;       // raw frames (N2) only: [f] frame means, subtracted after the gain multiply
};

// What is not the coordinate chain may contract to FMA (see cubic_coeffs_fast)
__device__ __forceinline__ float dot4(const float4 c, float e0, float e1, float e2, float e3) {
#pragma clang fp contract(fast)
  return ((c.x * e0 + c.y * e1) + c.z * e2) + c.w * e3;
}

// ------------------------------------------------------------------ the LDS window of the tile kernels
// Per (tile, frame): the shift at the tile centre positions a (32+3+2*MG) x (256+3+2*MG)
// input window that is DMA'd into LDS; every pixel then runs the reference's per-pixel
// coordinate chain (strict fp32, see above) and gathers its 4x4 taps from LDS.
// Lane l owns pixels x = x_tile + l + 64k (k = 0..3): adjacent lanes read adjacent LDS
// words, so the data-dependent gathers are bank-conflict free.
//
// Whether ALL taps of a tile fit the window is decided up front, rigorously: a pixel's
// shift is a bicubic (A = -0.75) interpolation of lattice nodes, sum(w) = 1 and
// sum|w| <= 1.375^2 < 1.9 in 2-D, so with rho = half the range of the nodes that can
// influence the tile every shift lies within 1.9*rho of the mid-range value and within
// 3.8*rho of the centre pixel's.  Tile-frames that fail the test are only flagged by the tile
// kernel and are processed afterwards by warp_field_slow (generic global gathers).
// The x-direction of the shift-lattice upsample comes from the E table (warp_etab).
#define GW_MG 6
#define GW_ROWS (RIGID_WAVES * RIGID_ROWS + 3 + 2 * GW_MG)              // 47
#define GW_QUADS ((RIGID_LANES * 4 + 3 + 2 * GW_MG + 3 + 3) / 4)         // 70 (alignment slack)
#define GW_STRIDE (4 * GW_QUADS)                                          // 280 floats
#define GW_NQ (GW_ROWS * GW_QUADS)
#define GW_QUADS_PAD (((GW_NQ + 63) / 64) * 64)

__device__ __forceinline__ float gw_dot4(const float w[4], float a, float b, float c, float d) {
#pragma clang fp contract(fast)
  return ((w[0] * a + w[1] * b) + w[2] * c) + w[3] * d;
}

// Cubic-convolution weights in factored form: c0 = A t u^2, c3 = A u t^2, c1 = 1 - t^2 ((A+3) -
// (A+2) t), c2 likewise in u = 1 - t (11 instead of 17 operations per axis; the same polynomials
// as ATen's Horner forms, values equal to ~1e-7).
__device__ __forceinline__ void cubic_coeffs_factored(float t, float c[4]) {
#pragma clang fp contract(fast)
  const float A = -0.75f;
  const float u = 1.f - t;
  const float atu = (A * t) * u;
  c[0] = atu * u;
  c[3] = atu * t;
  c[1] = 1.f - (t * t) * ((A + 3.f) - (A + 2.f) * t);
  c[2] = 1.f - (u * u) * ((A + 3.f) - (A + 2.f) * u);
}

__device__ __forceinline__ int wave_min_i(int v) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma clang fp contract(off)
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma clang fp contract(off)
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// ------------------------------------------------------------------ host side
// The field warp's scratch: etab | ytap | ycoef | xtap | xcoef | flags | plan, carved from `scratch`
// (16-byte aligned): one flag byte and one 16-byte plan entry per (frame, 256 x 32 tile).
struct FieldScratch {
  float* etab;   // [f][2][GH][w]
  int* ytap;     // [h][4]
  float* ycoef;  // [h][4]
  int* xtap;     // [w][4]
  float* xcoef;  // [w][4]
  unsigned char* flags;
  int4* plan;
  int64_t flag_bytes;
  int64_t bytes;  // what mc_warp_scratch_bytes reports
};
static inline FieldScratch field_scratch(float* scratch, int nframes, int h, int w, int GH) {
  const int64_t tx = (w + RIGID_LANES * 4 - 1) / (RIGID_LANES * 4);
  const int64_t ty = (h + RIGID_WAVES * RIGID_ROWS - 1) / (RIGID_WAVES * RIGID_ROWS);
  const int64_t etab_floats = (((int64_t)nframes * 2 * GH * w) + 3) & ~(int64_t)3;  // keep the int4 tables aligned
  FieldScratch t;
  t.flag_bytes = ((int64_t)nframes * tx * ty + 15) & ~(int64_t)15;
  uintptr_t p = reinterpret_cast<uintptr_t>(scratch);
  auto take = [&p](int64_t nbytes) {
    void* q = reinterpret_cast<void*>(p);
    p += (uintptr_t)nbytes;
    return q;
  };
  t.etab = static_cast<float*>(take(etab_floats * 4));
  t.ytap = static_cast<int*>(take(16 * (int64_t)h));
  t.ycoef = static_cast<float*>(take(16 * (int64_t)h));
  t.xtap = static_cast<int*>(take(16 * (int64_t)w));
  t.xcoef = static_cast<float*>(take(16 * (int64_t)w));
  t.flags = static_cast<unsigned char*>(take(t.flag_bytes));
  t.plan = static_cast<int4*>(take(16 * t.flag_bytes));
  t.bytes = (int64_t)(p - reinterpret_cast<uintptr_t>(scratch));
  return t;
}

// arguments of the tiled kernels (256 x 32 tiles); gain / mu for raw frames only
static inline FieldArgs field_args(const void* frames, int nframes, int h, int w, const float* lattice, int GH, int GW,
                                   float pixel_spacing, const FieldScratch& t, float* out_frames, float* out_sum,
                                   const float* gain, const float* mu) {
  FieldArgs fa;
  WarpArgs& a = fa.w;
  a.frames = static_cast<const float*>(frames); a.nframes = nframes; a.h = h; a.w = w; a.GH = GH; a.etab = t.etab;
  a.ytap = t.ytap; a.ycoef = t.ycoef; a.pixel_spacing = pixel_spacing;
  a.out_frames = out_frames; a.out_sum = out_sum;
  a.tiles_x = (w + RIGID_LANES * 4 - 1) / (RIGID_LANES * 4);
  a.tiles_y = (h + RIGID_WAVES * RIGID_ROWS - 1) / (RIGID_WAVES * RIGID_ROWS);
  fa.lattice = lattice; fa.xtap = t.xtap; fa.GW = GW; fa.flags = t.flags; fa.gain = gain; fa.mu = mu;
  return fa;
}

// A kernel cannot be launched from another object without relocatable device code, so the object that
// holds a kernel defines its launcher for the others; none of these is part of the C ABI.
// field_tables.hip: the per-axis tap tables and the x-upsampled lattice E of `nframes` lattices
__attribute__((visibility("hidden"))) void mc_field_tables_launch(const float* lattice, int nframes, int h, int w, int GH,
                                                                  int GW, const FieldScratch& t, hipStream_t s);
// warp_field_fallback.hip: warp_main over its own 128 x 16 tiles (fp32 frames, any width and alignment) ...
__attribute__((visibility("hidden"))) void mc_warp_main_launch(WarpArgs a, hipStream_t s);
// ... and warp_field2 over the 256 x 32 tiles of `fa` (fp32 frames); the caller runs warp_field_slow afterwards
__attribute__((visibility("hidden"))) void mc_warp_field2_launch(const FieldArgs& fa, hipStream_t s);
