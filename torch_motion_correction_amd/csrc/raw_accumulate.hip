// Per-pixel sums over the frames of a raw u8 / i16 movie: the statistics a gain reference and a defect map are
// estimated from (calibration.py).
//
//   sum[p] += sum_f v[f][p]        sumsq[p] += sum_f v[f][p]^2        (64-bit integers, exact)
//
// The only traffic that grows with the movie is one read of its bytes: 1 B (u8) or 2 B (i16) per pixel and frame.
// Nothing is written per frame.
//
// Ownership.  One thread owns one 16-byte piece of a row -- 16 u8 or 8 i16 pixels -- for the whole launch: it walks
// the frames at stride h * w with UNROLL 16-byte loads in flight, keeps its sums in registers and, after the last
// frame, reads, adds to and writes its own 64-bit accumulators once.  Every pixel has exactly one owner, so there
// are no atomics, no LDS and no barrier.  The grid is the h * ceil(w / piece) pieces in row-major order (the kernel
// is bound by the read; no XCD ordering).
//
// Exactness.  One launch sums at most FRAME_BLOCK = 32768 frames; a longer movie is one launch per block, in stream
// order, each with its own read-modify-write (a call of up to 32768 frames updates the accumulators once).  Within
// a block the register sums are 32 bits wide wherever that is exact:
//   u8   sum <= 255 * 2^15 < 2^23 and sum of squares <= 255^2 * 2^15 = 2 130 739 200 < 2^32: both u32;
//   i16  |sum| <= 2^15 * 2^15 = 2^30: i32.  A square reaches 2^30, so four of them already overflow u32: the
//        squares go into a u64 register sum (v_mad_u64_u32), <= 2^45 per block.
// Keeping 64-bit totals for 16 pixels in registers as well (one launch for any t) costs 64 more VGPRs and a third
// of the waves per SIMD; the 16 B per pixel of a second update are 1/2048 of the 32768 B per pixel read before it.
// What the ACCUMULATORS hold over a session is the caller's bound (calibration.RawStatistics refuses frames before
// sumsq can pass 2^63).
//
// Rows that are not whole aligned pieces (w not a multiple of the piece, or a base pointer that is not 16-byte
// aligned) take the element path: the same ownership and the same sums from one load per pixel, with the pixels
// beyond the row's end skipped.  The host picks the path for the whole call; the detectors' formats (4096, 5760,
// 11520 columns) all take the vector path.
#include <algorithm>
#include <type_traits>

#include "mc_common.h"
#include "mcorr.h"

namespace {

constexpr int RA_WG = 256;
constexpr int FRAME_BLOCK = 32768;
constexpr int UNROLL = 8;  // 16-byte loads in flight per thread: 8 KiB per wave

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

template <bool I16>
struct Piece {
  static constexpr int N = I16 ? 8 : 16;  // pixels of a 16-byte piece
  using Sq = typename std::conditional<I16, unsigned long long, unsigned>::type;
  int s[N];
  Sq q[N];

  __device__ __forceinline__ void add(int i, int v) {
    s[i] += v;
    q[i] += (Sq)(unsigned)(v * v);  // v^2 <= 2^30
  }
  __device__ __forceinline__ void add_words(u32x4 d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned wd = d[k];
      if (I16) {
        add(2 * k, (int)(short)(wd & 0xffffu));
        add(2 * k + 1, (int)wd >> 16);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) add(4 * k + b, (int)((wd >> (8 * b)) & 0xffu));
      }
    }
  }
};

// t <= FRAME_BLOCK frames
template <bool I16, bool VEC>
__global__ __launch_bounds__(RA_WG) void raw_pixel_sums(const unsigned char* __restrict__ raw, int t, int h, int w,
                                                        int pieces_per_row, long long* __restrict__ sum,
                                                        unsigned long long* __restrict__ sumsq) {
  constexpr int N = Piece<I16>::N, ES = I16 ? 2 : 1;
  const long long piece = (long long)blockIdx.x * RA_WG + threadIdx.x;
  if (piece >= (long long)h * pieces_per_row) return;
  const int row = (int)(piece / pieces_per_row), x0 = (int)(piece % pieces_per_row) * N;
  const long long p0 = (long long)row * w + x0;    // first pixel of the piece, inside the frame
  const long long stride = (long long)h * w * ES;  // bytes between frames
  const int valid = VEC ? N : min(N, w - x0);      // pixels of the piece inside the row (>= 1)
  const unsigned char* src = raw + p0 * ES;

  Piece<I16> a;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    a.s[i] = 0;
    a.q[i] = 0;
  }
  int f = 0;
  if (VEC) {
    for (; f + UNROLL <= t; f += UNROLL) {
      u32x4 d[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        d[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + (f + u) * stride));
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a.add_words(d[u]);
    }
    for (; f < t; ++f) a.add_words(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + f * stride)));
  } else {
    for (; f < t; ++f) {
      const unsigned char* fp = src + f * stride;
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (i < valid) a.add(i, I16 ? (int)reinterpret_cast<const short*>(fp)[i] : (int)fp[i]);
    }
  }

  // the one read-modify-write of this thread's accumulators
  if (VEC) {
    i64x2* sp = reinterpret_cast<i64x2*>(sum + p0);
    u64x2* qp = reinterpret_cast<u64x2*>(sumsq + p0);
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      i64x2 sv = sp[i];
      u64x2 qv = qp[i];
      sv.x += a.s[2 * i];
      sv.y += a.s[2 * i + 1];
      qv.x += a.q[2 * i];
      qv.y += a.q[2 * i + 1];
      sp[i] = sv;
      qp[i] = qv;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < valid) {
        sum[p0 + i] += a.s[i];
        sumsq[p0 + i] += a.q[i];
      }
  }
}

template <bool I16>
int launch(const void* raw, int t, int h, int w, long long* sum, unsigned long long* sumsq, hipStream_t st) {
  constexpr int N = Piece<I16>::N;
  const int ppr = (w + N - 1) / N;
  const long long pieces = (long long)h * ppr;
  const long long blocks = (pieces + RA_WG - 1) / RA_WG;
  if (blocks > 0x7fffffffLL) return MC_ERR_ARG;
  // whole pieces at 16-byte addresses in every row of every frame, and 16-byte accumulator pairs
  const bool vec = w % N == 0 && (reinterpret_cast<uintptr_t>(raw) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(sum) & 15) == 0 && (reinterpret_cast<uintptr_t>(sumsq) & 15) == 0;
  auto k = vec ? raw_pixel_sums<I16, true> : raw_pixel_sums<I16, false>;
  const long long frame_bytes = (long long)h * w * (I16 ? 2 : 1);
  for (long long f0 = 0; f0 < t; f0 += FRAME_BLOCK) {
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(RA_WG), 0, st,
                       static_cast<const unsigned char*>(raw) + f0 * frame_bytes,
                       (int)std::min<long long>(FRAME_BLOCK, t - f0), h, w, ppr, sum, sumsq);
    const int rc = mc_check_launch();
    if (rc != MC_OK) return rc;
  }
  return MC_OK;
}

}  // namespace

extern "C" int mc_raw_pixel_sums(const void* raw, int is_i16, int t, int h, int w, long long* sum,
                                 unsigned long long* sumsq, void* stream) {
  if (!raw || !sum || !sumsq || t < 1 || h < 1 || w < 1 || (is_i16 != 0 && is_i16 != 1)) return MC_ERR_ARG;
  if (is_i16 && (reinterpret_cast<uintptr_t>(raw) & 1)) return MC_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(sum) & 7) || (reinterpret_cast<uintptr_t>(sumsq) & 7)) return MC_ERR_ARG;
  return is_i16 ? launch<true>(raw, t, h, w, sum, sumsq, (hipStream_t)stream)
                : launch<false>(raw, t, h, w, sum, sumsq, (hipStream_t)stream);
}
