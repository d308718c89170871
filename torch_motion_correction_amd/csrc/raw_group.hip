// Rolling frame-group sums of a raw u8 / i16 movie: frame i of the int16 output is the sum of the input frames
// max(0, i - lo) .. min(t - 1, i + hi), lo = (g - 1) / 2, hi = g / 2 -- the centred window of g frames, clipped at
// the ends of the movie (MotionCor2 -Group, RELION --group_frames).  The estimators then cross-correlate sums of
// neighbouring frames of a low-dose movie; (sum raw) * gain = sum (raw * gain), so the output is a raw movie for
// every raw route, with the same gain.
//
// Traffic per pixel and frame: the leading frame's 1 B (u8) or 2 B (i16) read, the 2 B written, and the re-read of
// the trailing frame, which misses the caches at worst.  Ownership, the running sums and the element path are in
// raw_group.h (one thread owns one 16-byte piece of a row for the whole launch; no atomics, no LDS, no barrier);
// the grid is the h * ceil(w / piece) pieces in row-major order, as in raw_accumulate.hip.
//
// Exactness.  The running sums are 32 bits wide.  A u8 window holds at most 128 frames (255 * 128 = 32640 is an
// int16: nothing to check); an i16 window at most 32768 (|sum| <= 2^30), and a sum outside [-32768, 32767] raises
// the caller's flag.  Longer windows are refused on the host.
#include "mc_common.h"
#include "mcorr.h"
#include "raw_group.h"

namespace {

using raw_group::WG;

template <bool I16, bool VEC>
__global__ __launch_bounds__(WG) void raw_group_frames(const unsigned char* __restrict__ raw, int t, int h, int w,
                                                       int pieces_per_row, int lo, int hi, short* __restrict__ out,
                                                       int* __restrict__ flag) {
  raw_group::thread_body<I16, VEC>((long long)blockIdx.x * WG + threadIdx.x, raw, t, h, w, pieces_per_row, lo, hi,
                                   out, flag);
}

template <bool I16>
int launch(const void* raw, int t, int h, int w, int lo, int hi, short* out, int* flag, hipStream_t st) {
  constexpr int N = raw_group::Px<I16>::N;
  const int ppr = (w + N - 1) / N;
  const long long blocks = ((long long)h * ppr + WG - 1) / WG;
  if (blocks > 0x7fffffffLL) return MC_ERR_ARG;
  auto k = raw_group::vector_path<I16>(raw, out, w) ? raw_group_frames<I16, true> : raw_group_frames<I16, false>;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(WG), 0, st, static_cast<const unsigned char*>(raw), t, h, w, ppr,
                     lo, hi, out, flag);
  return mc_check_launch();
}

}  // namespace

extern "C" int mc_raw_group_frames(const void* raw, int storage, int t, int h, int w, int group, short* out,
                                   int* overflow, void* stream) {
  if (!raw || !out || !overflow || t < 1 || h < 1 || w < 1 || group < 1) return MC_ERR_ARG;
  if (storage != MC_STORE_U8 && storage != MC_STORE_I16) return MC_ERR_UNSUPPORTED;
  const int window = group < t ? group : t;  // frames of the longest window
  if (window > (storage == MC_STORE_I16 ? 32768 : 128)) return MC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(out) & 1) || (reinterpret_cast<uintptr_t>(overflow) & 3)) return MC_ERR_ARG;
  if (storage == MC_STORE_I16 && (reinterpret_cast<uintptr_t>(raw) & 1)) return MC_ERR_ARG;
  // a reach of t frames already covers the movie from any frame
  const int lo = (group - 1) / 2 < t ? (group - 1) / 2 : t, hi = group / 2 < t ? group / 2 : t;
  return storage == MC_STORE_I16 ? launch<true>(raw, t, h, w, lo, hi, out, overflow, (hipStream_t)stream)
                                 : launch<false>(raw, t, h, w, lo, hi, out, overflow, (hipStream_t)stream);
}
