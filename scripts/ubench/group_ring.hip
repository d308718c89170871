// The trailing frame of the rolling frame-group sums: re-loaded (the form libmcorr ships, csrc/raw_group.h) against
// kept in a register ring of G 16-byte pieces (G a template argument; this file only).  u8 movies, vector path.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I ../../torch_motion_correction_amd/csrc group_ring.hip -o group_ring
//   ./group_ring            40 x 4096 x 4096      ./group_ring big      60 x 8184 x 11520
// Prints the median of 5 launches after 2 of warm-up for G = 3 and 8, both forms, and whether the two outputs are
// equal.  The figures are in DESIGN.md section 4, "Frame groups from raw bytes".
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "raw_group.h"

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

using raw_group::rg_u32x4;
using raw_group::WG;

__global__ __launch_bounds__(WG) void reload(const unsigned char* __restrict__ raw, int t, int h, int w, int ppr,
                                             int lo, int hi, short* __restrict__ out, int* __restrict__ flag) {
  raw_group::thread_body<false, true>((long long)blockIdx.x * WG + threadIdx.x, raw, t, h, w, ppr, lo, hi, out, flag);
}

// the window's G frames stay in registers: slot f % G holds frame f; per batch of G output frames the G leading
// frames are loaded first, then each step stores, adds its leading frame, subtracts the slot's old frame and
// replaces it.  t >= G / 2 + 1.
template <int G>
__global__ __launch_bounds__(WG) void ring(const unsigned char* __restrict__ raw, int t, int h, int w, int ppr,
                                           short* __restrict__ out) {
  constexpr int LO = (G - 1) / 2, HI = G / 2;
  const long long piece = (long long)blockIdx.x * WG + threadIdx.x;
  if (piece >= (long long)h * ppr) return;
  const long long p0 = (piece / ppr) * w + (piece % ppr) * 16, hw = (long long)h * w;
  const unsigned char* src = raw + p0;
  short* dst = out + p0;
  const rg_u32x4 zero = {0u, 0u, 0u, 0u};
  rg_u32x4 win[G];
  int s[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = 0;
#pragma unroll
  for (int f = 0; f < G; ++f)
    win[f] = f <= HI ? __builtin_nontemporal_load(reinterpret_cast<const rg_u32x4*>(src + f * hw)) : zero;
#pragma unroll
  for (int f = 0; f <= HI; ++f) raw_group::add_words<false, 1>(s, win[f]);
  for (int i0 = 0; i0 < t; i0 += G) {
    rg_u32x4 lead[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const long long a = (long long)i0 + u + HI + 1;
      lead[u] = a < t ? __builtin_nontemporal_load(reinterpret_cast<const rg_u32x4*>(src + a * hw)) : zero;
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      if (i0 + u < t) {
        short* o = dst + (long long)(i0 + u) * hw;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          rg_u32x4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = raw_group::pack2(s[8 * q + 2 * k], s[8 * q + 2 * k + 1]);
          __builtin_nontemporal_store(v, reinterpret_cast<rg_u32x4*>(o) + q);
        }
        const int slot = (u + G - LO) % G;  // frame i0 + u - LO, i0 a multiple of G
        raw_group::add_words<false, 1>(s, lead[u]);
        raw_group::add_words<false, -1>(s, win[slot]);
        win[slot] = lead[u];
      }
    }
  }
}

__global__ void count_diff(const rg_u32x4* a, const rg_u32x4* b, long long n, unsigned long long* diff) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long d = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const rg_u32x4 x = a[i], y = b[i];
    d += (x[0] != y[0]) + (x[1] != y[1]) + (x[2] != y[2]) + (x[3] != y[3]);
  }
  if (d) atomicAdd(diff, d);
}

__global__ void fill(unsigned* p, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    unsigned x = (unsigned)i * 2654435761u;
    x ^= x >> 13;
    p[i] = x * 2246822519u;
  }
}

template <class F>
static float median_ms(F&& launch) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float ms[5];
  for (int r = -2; r < 5; ++r) {
    CK(hipEventRecord(e0));
    launch();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    if (r >= 0) CK(hipEventElapsedTime(&ms[r], e0, e1));
  }
  std::sort(ms, ms + 5);
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return ms[2];
}

template <int G>
static void compare(const unsigned char* raw, int t, int h, int w, short* out_a, short* out_b, int* flag,
                    unsigned long long* diff) {
  const int ppr = w / 16;
  const unsigned blocks = (unsigned)(((long long)h * ppr + WG - 1) / WG);
  const long long n = (long long)t * h * w;
  const float a = median_ms([&] {
    hipLaunchKernelGGL(reload, dim3(blocks), dim3(WG), 0, 0, raw, t, h, w, ppr, (G - 1) / 2, G / 2, out_a, flag);
  });
  const float b = median_ms([&] { hipLaunchKernelGGL((ring<G>), dim3(blocks), dim3(WG), 0, 0, raw, t, h, w, ppr, out_b); });
  CK(hipMemset(diff, 0, 8));
  hipLaunchKernelGGL(count_diff, dim3(4096), dim3(256), 0, 0, reinterpret_cast<const rg_u32x4*>(out_a),
                     reinterpret_cast<const rg_u32x4*>(out_b), n / 8, diff);
  unsigned long long d = 0;
  CK(hipMemcpy(&d, diff, 8, hipMemcpyDeviceToHost));
  const double gb = 3.0 * (double)n / 1e9;  // 1 B read + 2 B written per pixel and frame
  printf("%d x %d x %d u8, group %d: re-load %.3f ms (%.2f TB/s of 1+2 B), register ring %.3f ms (%.2f TB/s), "
         "outputs %s\n", t, h, w, G, a, gb / a, b, gb / b, d ? "DIFFER" : "equal");
  fflush(stdout);
}

int main(int argc, char** argv) {
  const bool big = argc > 1 && !strcmp(argv[1], "big");
  const int t = big ? 60 : 40, h = big ? 8184 : 4096, w = big ? 11520 : 4096;
  const long long n = (long long)t * h * w;
  unsigned char* raw;
  short *out_a, *out_b;
  int* flag;
  unsigned long long* diff;
  CK(hipMalloc(&raw, n));
  CK(hipMalloc(&out_a, 2 * n));
  CK(hipMalloc(&out_b, 2 * n));
  CK(hipMalloc(&flag, 4));
  CK(hipMalloc(&diff, 8));
  CK(hipMemset(flag, 0, 4));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, reinterpret_cast<unsigned*>(raw), n / 4);
  CK(hipDeviceSynchronize());
  compare<3>(raw, t, h, w, out_a, out_b, flag, diff);
  compare<8>(raw, t, h, w, out_a, out_b, flag, diff);
  CK(hipFree(raw));
  CK(hipFree(out_a));
  CK(hipFree(out_b));
  CK(hipFree(flag));
  CK(hipFree(diff));
  return 0;
}
