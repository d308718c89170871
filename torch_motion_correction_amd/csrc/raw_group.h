// The per-thread body of the rolling frame-group sums (raw_group.hip), written so that a host compiler takes it as
// well: tests/host_raw_group.cpp runs every thread of every workgroup in turn under the address and undefined-
// behaviour sanitizers.  Nothing here needs the HIP runtime.
//
//   out[i][p] = sum of raw[f][p] over f = max(0, i - lo) .. min(t - 1, i + hi),   lo = (g - 1) / 2, hi = g / 2
//
// One thread owns one 16-byte piece of a row of the INPUT (16 u8 or 8 i16 pixels) for the whole launch and walks the
// frames with the window sums of its pixels in 32-bit registers:
//
//   s  = frame 0 + ... + frame min(hi, t - 1)                          (the window of output frame 0)
//   out[i] = s;   s += frame(i + hi + 1) - frame(i - lo)               (each term only where the frame exists)
//
// STEPS output frames are taken together: their leading and trailing frames are loaded first (2 * STEPS 16-byte
// loads in flight per thread), then the STEPS sums are formed and stored, 16 bytes per store, non-temporal.  The
// trailing frame is read again from memory (it was this thread's leading frame g steps ago); it is not kept in
// registers, so one kernel serves every g.  Which frames exist depends on i alone: the conditions are uniform over
// the launch.
//
// I16 input can leave the int16 range; a thread that sees such a sum sets *flag = 1 after its last frame (a plain
// store of the same value by every such thread -- no atomics).  u8 sums of at most 128 frames cannot (255 * 128 =
// 32640), and the host admits no longer u8 window.
//
// VEC = false is the element path for rows that are not whole aligned pieces: the same ownership and sums from one
// load and one store per pixel, the pixels beyond the row's end skipped.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ __forceinline__
#else
#define RG_HD inline
#endif

namespace raw_group {

constexpr int WG = 256;
constexpr int STEPS = 4;  // output frames per batch: 8 loads of 16 bytes in flight per thread

typedef unsigned int rg_u32x4 __attribute__((ext_vector_type(4)));

template <bool I16>
struct Px {
  static constexpr int N = I16 ? 8 : 16;  // pixels of a 16-byte piece
};

// s[k] += sign * pixel k of the piece d
template <bool I16, int SIGN>
RG_HD void add_words(int* s, rg_u32x4 d) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned wd = d[k];
    if (I16) {
      s[2 * k] += SIGN * (int)(short)(wd & 0xffffu);
      s[2 * k + 1] += SIGN * ((int)wd >> 16);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) s[4 * k + b] += SIGN * (int)((wd >> (8 * b)) & 0xffu);
    }
  }
}

RG_HD unsigned pack2(int a, int b) { return ((unsigned)a & 0xffffu) | ((unsigned)b << 16); }
// 1 where v is no int16
RG_HD int beyond_i16(int v) { return (unsigned)(v + 32768) > 65535u ? 1 : 0; }

// whole pieces at 16-byte addresses in every row of every frame of the movie and of the output
template <bool I16>
inline bool vector_path(const void* raw, const void* out, int w) {
  return w % Px<I16>::N == 0 && (reinterpret_cast<uintptr_t>(raw) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(out) & 15) == 0;
}

// lo, hi: the window's reach before and after its frame, each already clipped to t by the caller
template <bool I16, bool VEC>
RG_HD void thread_body(long long piece, const unsigned char* __restrict__ raw, int t, int h, int w,
                       int pieces_per_row, int lo, int hi, short* __restrict__ out, int* __restrict__ flag) {
  constexpr int N = Px<I16>::N, ES = I16 ? 2 : 1;
  if (piece >= (long long)h * pieces_per_row) return;
  const int row = (int)(piece / pieces_per_row), x0 = (int)(piece % pieces_per_row) * N;
  const long long p0 = (long long)row * w + x0;  // first pixel of the piece, inside the frame
  const long long hw = (long long)h * w;
  const long long stride = hw * ES;            // bytes between input frames
  const int valid = VEC ? N : (N < w - x0 ? N : w - x0);  // pixels of the piece inside the row (>= 1)
  const unsigned char* src = raw + p0 * ES;
  short* dst = out + p0;

  int s[N];
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0;
  int bad = 0;
  const int first = hi < t - 1 ? hi : t - 1;  // last frame of output frame 0's window

  if (VEC) {
    const rg_u32x4 zero = {0u, 0u, 0u, 0u};
    int f = 0;
    for (; f + STEPS <= first + 1; f += STEPS) {
      rg_u32x4 d[STEPS];
#pragma unroll
      for (int u = 0; u < STEPS; ++u)
        d[u] = __builtin_nontemporal_load(reinterpret_cast<const rg_u32x4*>(src + (f + u) * stride));
#pragma unroll
      for (int u = 0; u < STEPS; ++u) add_words<I16, 1>(s, d[u]);
    }
    for (; f <= first; ++f)
      add_words<I16, 1>(s, __builtin_nontemporal_load(reinterpret_cast<const rg_u32x4*>(src + f * stride)));

    for (int i0 = 0; i0 < t; i0 += STEPS) {
      rg_u32x4 lead[STEPS], trail[STEPS];
#pragma unroll
      for (int u = 0; u < STEPS; ++u) {
        const long long a = (long long)i0 + u + hi + 1, b = (long long)i0 + u - lo;
        // the leading frame is read once by this thread and never again by anyone before g more frames went by;
        // the trailing frame is the re-read, left to the caches
        lead[u] = a < t ? __builtin_nontemporal_load(reinterpret_cast<const rg_u32x4*>(src + a * stride)) : zero;
        trail[u] = (b >= 0 && i0 + u < t) ? *reinterpret_cast<const rg_u32x4*>(src + b * stride) : zero;
      }
#pragma unroll
      for (int u = 0; u < STEPS; ++u) {
        if (i0 + u < t) {
          short* o = dst + (long long)(i0 + u) * hw;
#pragma unroll
          for (int q = 0; q < N / 8; ++q) {
            rg_u32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = pack2(s[8 * q + 2 * k], s[8 * q + 2 * k + 1]);
            __builtin_nontemporal_store(v, reinterpret_cast<rg_u32x4*>(o) + q);
          }
          if (I16) {
#pragma unroll
            for (int k = 0; k < N; ++k) bad |= beyond_i16(s[k]);
          }
          add_words<I16, 1>(s, lead[u]);
          add_words<I16, -1>(s, trail[u]);
        }
      }
    }
  } else {
    for (int f = 0; f <= first; ++f) {
      const unsigned char* fp = src + f * stride;
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (k < valid) s[k] += I16 ? (int)reinterpret_cast<const short*>(fp)[k] : (int)fp[k];
    }
    for (int i = 0; i < t; ++i) {
      const long long a = (long long)i + hi + 1, b = (long long)i - lo;
      const unsigned char* ap = src + (a < t ? a : 0) * stride;
      const unsigned char* bp = src + (b >= 0 ? b : 0) * stride;
      short* o = dst + (long long)i * hw;
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (k < valid) {
          o[k] = (short)s[k];
          if (I16) bad |= beyond_i16(s[k]);
          if (a < t) s[k] += I16 ? (int)reinterpret_cast<const short*>(ap)[k] : (int)ap[k];
          if (b >= 0) s[k] -= I16 ? (int)reinterpret_cast<const short*>(bp)[k] : (int)bp[k];
        }
    }
  }
  if (I16 && bad) *flag = 1;
}

}  // namespace raw_group
