// The per-thread bodies of the detector-defect fill (defect_fill.hip), written so that a host compiler takes them as
// well: tests/host_defect_fill.cpp runs every thread of every launch in turn under the address and undefined-
// behaviour sanitizers.  Nothing here needs the HIP runtime.
//
// The defect pixels are listed in row-major order: j is a pixel's place in the list, pixels[j] = y * w + x.
//
//   donors   the ring at Chebyshev distance r around (y, x) is the pixels with max(|dy|, |dx|) == r inside the frame.
//            r_j is the smallest r in 1 .. reach whose ring holds a good (non-defect) pixel; donors[j][0 .. count_j)
//            are the good pixels of that one ring in row-major order, the rest of the row (8 * reach ints) is -1.
//            count_j <= 8 r_j; count_j == 0 where no ring up to `reach` holds a good pixel.
//   pick     x = seed ^ (f * 0x9E3779B1) ^ (j * 0x85EBCA77), all uint32 with wrap-around,
//            x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16   (the murmur3 finaliser)
//            k = (uint64(x) * count_j) >> 32
//   fill     movie[f][pixels[j]] = movie[f][donors[j][k]]: one element loaded, one stored, bits untouched.  Donors are
//            good pixels and no good pixel is ever written, so the fill is free of races in place.
//   gain     gain[pixels[j]] = float(sum_k double(gain[donors[j][k]]) / count_j), the sum in table order.
//
// A thread whose table row cannot be used (count outside 1 .. 8 * reach, an index outside the frame) writes nothing:
// the tables are the caller's memory, and a damaged one must not become a store outside the movie.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ __forceinline__
#else
#define DF_HD inline
#endif

namespace defect_fill {

constexpr int WG = 256;
constexpr int MAX_REACH = 16;

template <int ES>
struct Elem;
template <>
struct Elem<1> {
  typedef uint8_t type;
};
template <>
struct Elem<2> {
  typedef uint16_t type;
};
template <>
struct Elem<4> {
  typedef uint32_t type;
};

DF_HD unsigned pick(unsigned seed, unsigned f, unsigned j, unsigned count) {
  unsigned x = seed ^ (f * 0x9E3779B1u) ^ (j * 0x85EBCA77u);
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return (unsigned)(((unsigned long long)x * count) >> 32);
}

// one thread per defect: its row of `donors` (8 * reach ints) and its count
DF_HD void donors_body(long long j, const unsigned char* __restrict__ map, int h, int w,
                       const int* __restrict__ pixels, int n, int reach, int* __restrict__ donors,
                       int* __restrict__ counts) {
  if (j >= n) return;
  const int slots = 8 * reach;
  int* row = donors + j * slots;
  const int p = pixels[j];
  int c = 0;
  if (p >= 0 && (long long)p < (long long)h * w) {
    const int y = p / w, x = p % w;
    for (int r = 1; r <= reach && c == 0; ++r) {
      const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > h - 1 ? h - 1 : y + r;
      for (int yy = y0; yy <= y1; ++yy) {
        const bool whole = yy == y - r || yy == y + r;  // the ring's top and bottom rows; else its two ends
        const int step = whole ? 1 : 2 * r;
        for (int xx = x - r; xx <= x + r; xx += step) {
          if (xx < 0 || xx >= w) continue;
          const int q = yy * w + xx;  // < h * w <= INT_MAX
          if (!map[q]) row[c++] = q;
        }
      }
    }
  }
  counts[j] = c;
  for (int k = c; k < slots; ++k) row[k] = -1;
}

// one thread per (frame, defect); hw = h * w elements per frame, offsets in 64 bits
template <int ES>
DF_HD void fill_body(long long j, long long f, unsigned char* movie, long long hw, const int* __restrict__ pixels,
                     const int* __restrict__ donors, const int* __restrict__ counts, int n, int reach,
                     unsigned seed) {
  typedef typename Elem<ES>::type T;
  if (j >= n) return;
  const int slots = 8 * reach;
  const int c = counts[j], p = pixels[j];
  if (c < 1 || c > slots || p < 0 || p >= hw) return;
  const int d = donors[j * slots + pick(seed, (unsigned)f, (unsigned)j, (unsigned)c)];
  if (d < 0 || d >= hw) return;
  T* frame = reinterpret_cast<T*>(movie + (unsigned long long)f * (unsigned long long)hw * ES);
  frame[p] = frame[d];
}

// one thread per defect
DF_HD void gain_body(long long j, float* gain, long long hw, const int* __restrict__ pixels,
                     const int* __restrict__ donors, const int* __restrict__ counts, int n, int reach) {
  if (j >= n) return;
  const int slots = 8 * reach;
  const int c = counts[j], p = pixels[j];
  if (c < 1 || c > slots || p < 0 || p >= hw) return;
  const int* row = donors + j * slots;
  double s = 0.0;
  for (int k = 0; k < c; ++k) {
    const int d = row[k];
    if (d < 0 || d >= hw) return;
    s += (double)gain[d];
  }
  gain[p] = (float)(s / (double)c);
}

}  // namespace defect_fill
