// CPU run of the rolling frame-group kernel's per-thread body (csrc/raw_group.h, the source raw_group.hip
// compiles for the device): every thread of every workgroup is executed in turn, on exactly-sized heap buffers, and
// the output is compared with a naive loop over the window.  Meant to be built with the address and undefined-
// behaviour sanitizers, which then see every load and store of both the vector and the element path:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_raw_group.cpp -o host_raw_group && ./host_raw_group
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "raw_group.h"

namespace rg = raw_group;

static unsigned rng_state = 12345u;
static unsigned rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

template <bool I16>
static int run_case(int t, int h, int w, int g, int offset_elems, int amplitude, bool want_flag) {
  constexpr int N = rg::Px<I16>::N, ES = I16 ? 2 : 1;
  const size_t n = (size_t)t * h * w;
  // exact-size allocations (malloc gives 16-byte alignment); a view that starts offset_elems elements in
  unsigned char* in_alloc = static_cast<unsigned char*>(malloc((n + offset_elems) * ES));
  short* out_alloc = static_cast<short*>(malloc((n + offset_elems) * sizeof(short)));
  int* flag = static_cast<int*>(malloc(sizeof(int)));
  if (!in_alloc || !out_alloc || !flag) abort();
  unsigned char* raw = in_alloc + (size_t)offset_elems * ES;
  short* out = out_alloc + offset_elems;
  *flag = 0;
  for (size_t i = 0; i < n; ++i) {
    if (I16) {
      const short v = amplitude < 0 ? (short)(-amplitude) : (short)((int)(rng() % (2 * amplitude + 1)) - amplitude);
      memcpy(raw + 2 * i, &v, 2);
    } else {
      raw[i] = amplitude < 0 ? (unsigned char)(-amplitude) : (unsigned char)(rng() % (amplitude + 1));
    }
  }
  memset(out_alloc, 0x5a, (n + offset_elems) * sizeof(short));

  const int lo = (g - 1) / 2 < t ? (g - 1) / 2 : t, hi = g / 2 < t ? g / 2 : t;  // as mc_raw_group_frames
  const int ppr = (w + N - 1) / N;
  const long long pieces = (long long)h * ppr, blocks = (pieces + rg::WG - 1) / rg::WG;
  const bool vec = rg::vector_path<I16>(raw, out, w);
  for (long long b = 0; b < blocks; ++b)
    for (int th = 0; th < rg::WG; ++th) {
      if (vec) rg::thread_body<I16, true>(b * rg::WG + th, raw, t, h, w, ppr, lo, hi, out, flag);
      else rg::thread_body<I16, false>(b * rg::WG + th, raw, t, h, w, ppr, lo, hi, out, flag);
    }

  int bad = 0, overflow = 0;
  const size_t hw = (size_t)h * w;
  for (int i = 0; i < t && !bad; ++i) {
    const long long f0 = i - (long long)((g - 1) / 2) < 0 ? 0 : i - (long long)((g - 1) / 2);
    const long long f1 = i + (long long)(g / 2) > t - 1 ? t - 1 : i + (long long)(g / 2);
    for (size_t p = 0; p < hw; ++p) {
      long long s = 0;
      for (long long f = f0; f <= f1; ++f) {
        if (I16) {
          short v;
          memcpy(&v, raw + 2 * (f * hw + p), 2);
          s += v;
        } else {
          s += raw[f * hw + p];
        }
      }
      if (s < -32768 || s > 32767) {
        overflow = 1;  // the output of such a call is unspecified
      } else if (out[i * hw + p] != (short)s) {
        printf("  frame %d pixel %zu: %d, naive %lld\n", i, p, (int)out[i * hw + p], s);
        bad = 1;
        break;
      }
    }
  }
  for (int k = 0; k < offset_elems; ++k) bad |= out_alloc[k] != 0x5a5a;  // nothing before the view was written
  if (*flag != overflow || overflow != (want_flag ? 1 : 0)) {
    printf("  overflow flag %d, naive %d, expected %d\n", *flag, overflow, (int)want_flag);
    bad = 1;
  }
  printf("%s (%d,%d,%d) g=%d offset=%d %s path: %s\n", I16 ? "i16" : "u8 ", t, h, w, g, offset_elems,
         vec ? "vector" : "element", bad ? "FAIL" : "ok");
  free(in_alloc);
  free(out_alloc);
  free(flag);
  return bad;
}

int main() {
  static const int shapes[][3] = {{1, 1, 1}, {5, 3, 8}, {7, 5, 48}, {9, 33, 927}, {3, 7, 959}, {2, 64, 4096}};
  int bad = 0;
  for (const auto& s : shapes) {
    const int t = s[0];
    const int groups[] = {1, 2, 3, 4, 8, t, 2 * t + 3};
    for (int g : groups) {
      bad |= run_case<false>(t, s[1], s[2], g, 0, 255, false);
      bad |= run_case<true>(t, s[1], s[2], g, 0, 3000, false);  // |sum| <= 9 * 3000
    }
  }
  // a view one element off a 16-byte boundary: the element path for the whole call
  bad |= run_case<false>(7, 5, 48, 3, 1, 255, false);
  bad |= run_case<true>(7, 5, 48, 3, 1, 3000, false);
  // the longest u8 window, more frames than one batch of loads, a window of two and a huge group
  bad |= run_case<false>(130, 2, 32, 128, 0, -255, false);
  bad |= run_case<false>(11, 3, 16, 0x7fffffff, 0, 255, false);
  // the int16 edge
  bad |= run_case<true>(3, 2, 16, 2, 0, -32767, true);
  bad |= run_case<true>(3, 2, 13, 2, 0, -32767, true);
  bad |= run_case<true>(3, 2, 16, 1, 0, 32767, false);
  bad |= run_case<true>(3, 2, 16, 1, 0, -32768, false);  // constant -32768
  printf(bad ? "FAIL\n" : "OK\n");
  return bad;
}
