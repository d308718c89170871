// What both condition.hip and hot_pixels.hip use: the loaders of a raw movie's samples in any storage kind,
// the gain tile and the reduction tree of the tiled kernels, their launch grids, and the one launch that
// crosses the two objects.
//
// Nothing here multiplies and adds: the helpers compile the same under either FMA contraction mode, and
// each .hip sets its own mode after its includes.
#pragma once
#include <hip/hip_fp16.h>
#include "mc_common.h"

// one sample as fp32.  KIND: 0 u8, 1 i16, 2 f16, 3 f32 (MC_STORE_*).
template <int KIND>
__device__ __forceinline__ float cond_load(const void* p, int64_t i) {
  if (KIND == 0) return (float)reinterpret_cast<const unsigned char*>(p)[i];
  if (KIND == 1) return (float)reinterpret_cast<const short*>(p)[i];
  if (KIND == 2) return __half2float(reinterpret_cast<const __half*>(p)[i]);
  return reinterpret_cast<const float*>(p)[i];
}

// Vector form (hw % 8 == 0, 16-byte aligned buffers): 8 pixels per thread -- 8-byte (u8) to 32-byte
// (f32) loads, two float4 stores.  The gain reference is as large as a frame and is read again for
// every frame (5.4 GB per 40 x 4096^2 stack and pass, against 0.67 GB of 8-bit samples): a workgroup
// therefore takes COND_FR consecutive frames per pixel tile with the gain values in registers.  All
// 40 frames per tile were tried too: that scatters every workgroup's accesses over the whole stack
// and is slower than no reuse at all.
template <int KIND>
__device__ __forceinline__ void cond_load8(const void* p, int64_t i, float (&v)[8]) {
  if (KIND == 0) {
    const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(p) + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = (float)((q.x >> (8 * k)) & 0xffu);
      v[4 + k] = (float)((q.y >> (8 * k)) & 0xffu);
    }
  } else if (KIND == 1) {
    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const short*>(p) + i);
    const unsigned int u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = (float)(short)(u[k] & 0xffffu);
      v[2 * k + 1] = (float)(short)(u[k] >> 16);
    }
  } else if (KIND == 2) {
    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const __half*>(p) + i);
    const unsigned int u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __half2float(__ushort_as_half((unsigned short)(u[k] & 0xffffu)));
      v[2 * k + 1] = __half2float(__ushort_as_half((unsigned short)(u[k] >> 16)));
    }
  } else {
    const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i);
    const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

#define COND_FR 8  // frames per workgroup pass: the gain values of a pixel tile are used COND_FR times

// the gain values of the 8 pixels from i on (gain is not null here: a caller that allows that sets g = 1)
__device__ __forceinline__ void cond_gain8(const float* gain, int64_t i, float (&g)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(gain + i), b = *reinterpret_cast<const float4*>(gain + i + 4);
  g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w; g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
}

// Tail of the double sums of a 256-thread workgroup: after the shuffle steps lane 0 of each wave parks its
// total in LDS, and one thread adds the four partials in this order.  The tree is part of what the float64
// bounds of the tests were derived from.  (The shuffle loop itself stays written out in each kernel: behind
// any helper the compiler schedules its last step differently.)
__device__ __forceinline__ double part4_sum(const double (&p)[4]) { return (p[0] + p[1]) + (p[2] + p[3]); }

// What a thread of the tiled kernels reads at once: 8 samples (8 bytes of u8, 16 or 32 of the wider kinds)
// and two float4 of gain or output.
static inline bool cond_raw_aligned(const void* raw, int kind) {
  return (reinterpret_cast<uintptr_t>(raw) & (kind == 0 ? 7 : 15)) == 0;
}
static inline bool cond_f4_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Launch grids, 256 threads each and at most 2048 workgroups per frame (grid-stride loops).  Tiled: 8 pixels
// per thread, COND_FR frames per blockIdx.y.  Scalar: one frame per blockIdx.y, 8 strides per thread.
static inline dim3 cond_tiled_grid(int64_t hw, int nframes) {
  int64_t tb = (hw / 8 + 255) / 256;
  if (tb > 2048) tb = 2048;
  return dim3((unsigned)tb, (nframes + COND_FR - 1) / COND_FR);
}
static inline dim3 cond_scalar_grid(int64_t hw, int nframes) {
  int64_t blocks = (hw + 256 * 8 - 1) / (256 * 8);
  if (blocks > 2048) blocks = 2048;
  return dim3((unsigned)blocks, nframes);
}

// raw_stats_finalize (condition.hip) for mc_raw_hot_finalize (hot_pixels.hip): a kernel cannot be launched
// from another object without relocatable device code.  Not part of the C ABI.
__attribute__((visibility("hidden"))) void mc_raw_stats_finalize_launch(const double* stats, int nframes, int64_t hw,
                                                                        int64_t nbox, int mean_zero, float* mu,
                                                                        float* sub, float* mean_rstd, hipStream_t s);
