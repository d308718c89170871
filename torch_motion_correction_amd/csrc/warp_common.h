// What more than one of the warp translation units uses (warp_rigid.hip, warp_rigid_raw.hip, and the
// field-warp objects through warp_field_common.h): the strict-fp32 coordinate helpers, the tile geometry, the rigid warp's argument
// struct and weight tables, and the host helpers that pick a kernel's <frames, sum> instantiation.
//
// FMA contraction is part of the bit-exact contract the float64 tests pin, so every helper here sets
// its own mode at the start of its body and compiles the same wherever the header is included.
#pragma once
#include "mc_common.h"

// ATen cubic convolution coefficients, A = -0.75 (UpSample.h / GridSamplerKernel.cpp); strict
// operation order: part of the coordinate chain
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
#pragma clang fp contract(off)
  const float A = -0.75f;
  float x = t + 1.f;
  c[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  x = t;
  c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 1.f - t;
  c[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 2.f - t;
  c[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

// The same polynomials for the resampling weights, which may contract to FMA: ATen's own vectorised
// kernel is built with FMA contraction and differs from any fixed op order at the ulp level anyway
// (probed).
__device__ __forceinline__ void cubic_coeffs_fast(float t, float c[4]) {
#pragma clang fp contract(fast)
  const float A = -0.75f;
  float x = t + 1.f;
  c[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  x = t;
  c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 1.f - t;
  c[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 2.f - t;
  c[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

// grid_sample align_corners=True un-normalisation applied to an array coordinate that
// went through array_to_grid_sample:  ((c / (0.5 n - 0.5) - 1) + 1) * ((n - 1) / 2)
// The division by the loop-invariant d = 0.5 n - 0.5 is done as q = c r, e = fma(-q, d, c),
// q' = fma(e, r, q) with r = RN(1/d): that IS the correctly rounded quotient (Markstein; the one
// exception, a divisor whose significand is all ones, cannot occur for d with <= 15 significant
// bits; checked against exact rational arithmetic for the frame sizes in use, tests/test_host.py)
// at 3 instructions instead of the ~12 of a general IEEE division -- twice per pixel.
__device__ __forceinline__ float grid_chain(float c, float n) {
#pragma clang fp contract(off)
  const float d = 0.5f * n - 0.5f;
  const float r = 1.0f / d;
  float q = c * r;
  const float e = __builtin_fmaf(-q, d, c);
  q = __builtin_fmaf(e, r, q);
  const float g = q - 1.f;
  return (g + 1.f) * ((n - 1.f) / 2.f);
}

// Tile geometry of the rigid kernels, which the field kernels share: a wave covers 64 lanes x 4
// columns by RIGID_ROWS rows, the basic workgroup is RIGID_WAVES of them stacked (256 x 32 pixels).
#define RIGID_LANES 64
#define RIGID_WAVES 4
#define RIGID_ROWS 8                                   // output rows per wave

typedef __attribute__((address_space(3))) void* lds_vptr;

struct RigidArgs {
  const float* frames;
  int nframes, h, w;
  const int* S;     // [f][2]
  const float* Wy;  // [f][h][5]
  const float* Wx;  // [f][5][w]
  float* out_frames;
  float* out_sum;
  int tiles_x, tiles_y;
  int frames_in_grid;  // c > 0: blockIdx.y selects a chunk of c frames (no fused sum); 0: all frames in-block
};

typedef float rigid_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void rigid_store4(float* p, float a, float b, float c, float d) {
  // corrected frames are written once and never read again by this kernel: non-temporal stores
  // (fused launch 1.25 -> 1.15 ms at 40 x 4096^2, frames only 0.98 -> 0.95; scripts/ubench/stream_copy.hip
  // shows the same 5 % on a plain tiled copy)
  const rigid_f4 v = {a, b, c, d};
  __builtin_nontemporal_store(v, reinterpret_cast<rigid_f4*>(p));
}

// Frame f's weights of the strip at (x0, y0): Wv = the wave's 5 RIGID_ROWS row weights, one per lane (read
// back with readlane), W5 = the 5 column taps of the lane's 4 pixels.  Needs w % 4 == 0.
__device__ __forceinline__ void rigid_load_weights(const RigidArgs& a, int f, int y0, int x0, int lane,
                                                   float (&W5)[5][4], float& Wv) {
  const int h = a.h, w = a.w;
  Wv = 0.f;
  const int64_t idx = (int64_t)y0 * 5 + lane;
  if (lane < 5 * RIGID_ROWS && idx < (int64_t)h * 5) Wv = a.Wy[(int64_t)f * 5 * h + idx];
  const float* Wx = a.Wx + (int64_t)f * 5 * w + x0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x0 < w) t = *reinterpret_cast<const float4*>(Wx + (int64_t)j * w);
    W5[j][0] = t.x; W5[j][1] = t.y; W5[j][2] = t.z; W5[j][3] = t.w;
  }
}

// The rigid warp's scratch, Wy[f][h][5] | Wx[f][5][w] | S[f][2], carved from `scratch` (16-byte aligned).
struct RigidTables {
  float* Wy;
  float* Wx;
  int* S;
  int64_t bytes;  // what mc_warp_rigid_scratch_bytes reports
};
static inline RigidTables rigid_tables_layout(float* scratch, int nframes, int h, int w) {
  RigidTables t;
  uintptr_t p = reinterpret_cast<uintptr_t>(scratch);
  auto take = [&p](int64_t words) {
    void* q = reinterpret_cast<void*>(p);
    p += (uintptr_t)words * 4;
    return q;
  };
  t.Wy = static_cast<float*>(take((int64_t)nframes * 5 * h));
  t.Wx = static_cast<float*>(take((int64_t)nframes * 5 * w));
  t.S = static_cast<int*>(take(2 * (int64_t)nframes + 8));
  t.bytes = (int64_t)(p - reinterpret_cast<uintptr_t>(scratch));
  return t;
}
// rigid_base + rigid_weights for `shifts_px` into the tables above.  A kernel cannot be launched from
// another object without relocatable device code, so warp_rigid.hip defines this for warp_rigid_raw.hip;
// it is not part of the C ABI.
__attribute__((visibility("hidden"))) void mc_rigid_tables_launch(const float* shifts_px, int nframes, int h, int w,
                                                                  const RigidTables& t, hipStream_t s);
// What every rigid entry refuses with MC_ERR_ARG, after its own storage-kind rule (MC_ERR_UNSUPPORTED).
// phase 0: weight tables + resampling; 1: tables only (writes no image); 2: resampling only, the tables of an
// earlier phase-1 call with the same arguments are in `scratch`.
static inline int rigid_check_args(const void* frames, const float* shifts_px, const float* scratch,
                                   const float* out_frames, const float* out_sum, int nframes, int h, int w, int phase) {
  if (!frames || !shifts_px || !scratch || (phase != 1 && !out_frames && !out_sum)) return MC_ERR_ARG;
  if (nframes < 1 || h < 2 || w < 2 || (((uintptr_t)scratch) & 15) || phase < 0 || phase > 2) return MC_ERR_ARG;
  return MC_OK;
}
// the phase's table launch; true: the phase ends there
static inline bool rigid_phase_tables(int phase, const float* shifts_px, int nframes, int h, int w, const RigidTables& t,
                                      hipStream_t s) {
  if (phase != 2) mc_rigid_tables_launch(shifts_px, nframes, h, w, t, s);
  return phase == 1;
}
// kernel arguments for tiles of WX x WY waves
static inline RigidArgs rigid_args(const void* frames, int nframes, int h, int w, const RigidTables& t, float* out_frames,
                                   float* out_sum, int WX, int WY, int frames_in_grid) {
  RigidArgs a;
  a.frames = static_cast<const float*>(frames); a.nframes = nframes; a.h = h; a.w = w; a.S = t.S; a.Wy = t.Wy; a.Wx = t.Wx;
  a.out_frames = out_frames; a.out_sum = out_sum;
  a.tiles_x = (w + RIGID_LANES * 4 * WX - 1) / (RIGID_LANES * 4 * WX);
  a.tiles_y = (h + WY * RIGID_ROWS - 1) / (WY * RIGID_ROWS);
  a.frames_in_grid = frames_in_grid;
  return a;
}

// Launch selection (mc_pick, mc_common.h) over what a warp kernel writes: `go` gets the matching
// std::bool_constant tags.  Entry points reject "neither frames nor sum" before they get here.
template <class Go>
static inline void mc_pick_outputs(bool frames, bool sum, Go&& go) {  // go(FRAMES, SUM)
  if (frames && sum) go(std::true_type{}, std::true_type{});
  else if (frames) go(std::true_type{}, std::false_type{});
  else go(std::false_type{}, std::true_type{});
}
// the raw entries: an accumulating launch always has the sum.  go(FRAMES, SUM, ACCUM)
template <class Go>
static inline void mc_pick_outputs_accum(bool frames, bool sum, bool accumulate, Go&& go) {
  if (accumulate) mc_pick(frames, [&](auto F) { go(F, std::true_type{}, std::true_type{}); });
  else mc_pick_outputs(frames, sum, [&](auto F, auto S) { go(F, S, std::false_type{}); });
}
