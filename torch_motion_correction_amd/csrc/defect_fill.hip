// Detector defects (dead, hot and stuck pixels, dead rows and columns of the session's defect map) filled in a raw
// movie and in its gain reference before any estimate sees them (MotionCor2 -DefectFile / -DefectMap, RELION
// --defect_file): a raw movie -> raw movie stage and a gain -> gain step, so every raw route takes the results as
// they are.  The rule and the per-thread bodies are in defect_fill.h.
//
//   defect_donors      one thread per defect: walks the rings 1 .. reach over the uint8 map, writes its row of the
//                      donor table and its count.  Once per defect map.
//   raw_fill_defects   one thread per (frame, defect): the pick, one element loaded, one stored, IN PLACE.  j runs
//                      along x (consecutive defects of a dead row are consecutive addresses), frames along y; a
//                      movie of more frames than a grid has rows is walked in strides of the grid.
//   gain_fill_defects  one thread per defect: the float64 mean of its donors' gains.
//
// The defect list is sparse (a few columns and some hundreds of pixels of a 4096^2 detector), so the traffic is a
// few cache lines per defect and frame; an out-of-place fill is the caller's copy followed by raw_fill_defects on
// the copy.  No atomics, no LDS, no barrier.
#include "mc_common.h"
#include "mcorr.h"
#include "defect_fill.h"

namespace {

using defect_fill::MAX_REACH;
using defect_fill::WG;

__global__ __launch_bounds__(WG) void defect_donors(const unsigned char* __restrict__ map, int h, int w,
                                                    const int* __restrict__ pixels, int n, int reach,
                                                    int* __restrict__ donors, int* __restrict__ counts) {
  defect_fill::donors_body((long long)blockIdx.x * WG + threadIdx.x, map, h, w, pixels, n, reach, donors, counts);
}

template <int ES>
__global__ __launch_bounds__(WG) void raw_fill_defects(unsigned char* movie, int t, long long hw,
                                                       const int* __restrict__ pixels,
                                                       const int* __restrict__ donors,
                                                       const int* __restrict__ counts, int n, int reach,
                                                       unsigned seed) {
  const long long j = (long long)blockIdx.x * WG + threadIdx.x;
  for (int f = blockIdx.y; f < t; f += gridDim.y)
    defect_fill::fill_body<ES>(j, f, movie, hw, pixels, donors, counts, n, reach, seed);
}

__global__ __launch_bounds__(WG) void gain_fill_defects(float* gain, long long hw, const int* __restrict__ pixels,
                                                        const int* __restrict__ donors,
                                                        const int* __restrict__ counts, int n, int reach) {
  defect_fill::gain_body((long long)blockIdx.x * WG + threadIdx.x, gain, hw, pixels, donors, counts, n, reach);
}

// sizes every entry point shares: a frame whose pixels an int indexes, at most that many defects, reach 1 .. 16
bool sizes_ok(int h, int w, int n, int reach) {
  if (h < 1 || w < 1 || n < 0 || reach < 1 || reach > MAX_REACH) return false;
  const long long hw = (long long)h * w;
  return hw <= 0x7fffffffLL && n <= hw;
}

unsigned blocks_of(int n) { return (unsigned)(((long long)n + WG - 1) / WG); }

}  // namespace

extern "C" int mc_defect_donors(const unsigned char* map, int h, int w, const int* pixels, int n, int reach,
                                int* donors, int* counts, void* stream) {
  if (!map || !sizes_ok(h, w, n, reach)) return MC_ERR_ARG;
  if (n == 0) return MC_OK;
  if (!pixels || !donors || !counts) return MC_ERR_ARG;
  hipLaunchKernelGGL(defect_donors, dim3(blocks_of(n)), dim3(WG), 0, (hipStream_t)stream, map, h, w, pixels, n, reach,
                     donors, counts);
  return mc_check_launch();
}

extern "C" int mc_raw_fill_defects(void* movie, int elem_bytes, int t, int h, int w, const int* pixels,
                                   const int* donors, const int* counts, int n, int reach, unsigned seed,
                                   void* stream) {
  if (!movie || t < 1 || !sizes_ok(h, w, n, reach)) return MC_ERR_ARG;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return MC_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(movie) & (uintptr_t)(elem_bytes - 1)) return MC_ERR_ARG;
  if (n == 0) return MC_OK;
  if (!pixels || !donors || !counts) return MC_ERR_ARG;
  const long long hw = (long long)h * w;
  const dim3 grid(blocks_of(n), (unsigned)(t < 65535 ? t : 65535));
  unsigned char* m = static_cast<unsigned char*>(movie);
  hipStream_t st = (hipStream_t)stream;
  if (elem_bytes == 1)
    hipLaunchKernelGGL(raw_fill_defects<1>, grid, dim3(WG), 0, st, m, t, hw, pixels, donors, counts, n, reach, seed);
  else if (elem_bytes == 2)
    hipLaunchKernelGGL(raw_fill_defects<2>, grid, dim3(WG), 0, st, m, t, hw, pixels, donors, counts, n, reach, seed);
  else
    hipLaunchKernelGGL(raw_fill_defects<4>, grid, dim3(WG), 0, st, m, t, hw, pixels, donors, counts, n, reach, seed);
  return mc_check_launch();
}

extern "C" int mc_gain_fill_defects(float* gain, int h, int w, const int* pixels, const int* donors,
                                    const int* counts, int n, int reach, void* stream) {
  if (!gain || !sizes_ok(h, w, n, reach)) return MC_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(gain) & 3) return MC_ERR_ARG;
  if (n == 0) return MC_OK;
  if (!pixels || !donors || !counts) return MC_ERR_ARG;
  hipLaunchKernelGGL(gain_fill_defects, dim3(blocks_of(n)), dim3(WG), 0, (hipStream_t)stream, gain, (long long)h * w,
                     pixels, donors, counts, n, reach);
  return mc_check_launch();
}
