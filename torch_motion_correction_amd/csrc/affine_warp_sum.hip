// The aligned sum of a movie, rigid shifts and the magnification map in ONE bicubic resampling per frame: output pixel
// p of frame f samples it at c + M (p - c) + shift_f, and the values are added in frame order as they are formed.  The
// rule (float64 positions, the zero-outside decision, the fp32 Keys weights, clamped taps, the accumulation orders, a
// raw sample's conditioning), a tile's window for a frame and its size bound are in affine_warp_sum.h over
// affine_resample.h; this file holds the kernel around them and the entry point's host checks.
//
//   affine_warp_sum<KIND, FRAMES>  one 64 x 64 output tile per workgroup of 4 waves; a thread owns 16 pixels of one
//                       column (rows wave, wave + 4, ...) and their 16 fp32 accumulators in registers.  The workgroup
//                       walks the frames in order: the tile's window for the frame (affine::shifted_window, at most
//                       83 x 83 samples) is staged into LDS row by row -- consecutive lanes read consecutive samples of
//                       a source row, clamped at the frame's edge; u8 / i16 samples are conditioned
//                       (raw * gain - mu_f) and fp16 ones widened HERE, once per sample and not once per tap -- and
//                       every pixel takes its 16 taps from LDS (affine::shifted_pixel) and adds the value.  A frame
//                       whose window is empty for the tile is skipped.  FRAMES: the value is also stored as the frame's
//                       pixel.  The sum is written once, after the last frame.
//
// No scratch memory, no atomics, no partial sums: every output element is written once by the one thread that owns
// it, and the sum's bits do not depend on the launch geometry.
// Bounds.  Staging reads frame[clamped row][clamped column] and gain[the same] only; a tap of a pixel inside lies in
// the window by affine_warp_sum.h's argument, which rests on the row sums of |M| the entry point checks before
// anything is launched; a pixel outside, and every pixel of a tile whose window is empty (a shift beyond the frame or
// one that is not a number), reads nothing.  Stores go to pixels (y <= ty1, x <= tx1) of the tile only.
#include "cond_common.h"
#include "mcorr.h"
#include "affine_warp_sum.h"

namespace {

using affine::Mat;
using affine::STRIDE;
using affine::TILE;
using affine::WIN;
using affine::Window;

constexpr int WG = 256;
constexpr int PER = TILE / (WG / 64);  // output rows of a thread
static_assert(PER == 16 && TILE == 64, "a wave makes one tile row at a time");

template <int KIND, bool FRAMES>
__global__ __launch_bounds__(WG) void affine_warp_sum(const void* __restrict__ src, const float* __restrict__ gain,
                                                      const float* __restrict__ mu, int t, int h, int w, Mat m,
                                                      const float* __restrict__ shifts, float* __restrict__ sum,
                                                      float* __restrict__ frames, int tiles_x) {
  __shared__ float win[WIN * STRIDE];
  const int ty0 = (int)(blockIdx.x / tiles_x) * TILE, tx0 = (int)(blockIdx.x % tiles_x) * TILE;
  const int ty1 = (ty0 + TILE < h ? ty0 + TILE : h) - 1, tx1 = (tx0 + TILE < w ? tx0 + TILE : w) - 1;
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const int x = tx0 + lane;
  const int64_t hw = (int64_t)h * w;
  float acc[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) acc[k] = 0.f;

  for (int f = 0; f < t; ++f) {
    const float sy = shifts[2 * f], sx = shifts[2 * f + 1];
    const Window wd = affine::shifted_window(h, w, m, ty0, ty1, tx0, tx1, sy, sx);
    float* out = FRAMES ? frames + (int64_t)f * hw : nullptr;
    if (wd.rows == 0) {  // the same for every thread of the workgroup: the frame adds 0 to the whole tile
      if (FRAMES && x <= tx1)
        for (int y = ty0 + wave; y <= ty1; y += WG / 64) __builtin_nontemporal_store(0.f, out + (int64_t)y * w + x);
      continue;
    }
    const int64_t base = (int64_t)f * hw;
    const float muf = KIND < 2 ? mu[f] : 0.f;
    __syncthreads();  // the window may still be read for the frame before
    for (int r = wave; r < wd.rows; r += WG / 64) {
      const int64_t row = (int64_t)affine::clamped(wd.y0, r, h) * w;
      for (int c = lane; c < wd.cols; c += 64) {
        const int64_t i = row + affine::clamped(wd.x0, c, w);
        float v = cond_load<KIND>(src, base + i);
        if (KIND < 2) v = affine::conditioned(v, gain[i], muf);
        win[r * STRIDE + c] = v;
      }
    }
    __syncthreads();
    if (x <= tx1) {
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int y = ty0 + wave + k * (WG / 64);
        if (y <= ty1) {
          const float v = affine::shifted_pixel(win, wd, h, w, m, y, x, sy, sx);
          acc[k] += v;
          if (FRAMES) __builtin_nontemporal_store(v, out + (int64_t)y * w + x);
        }
      }
    }
  }
  if (x <= tx1) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int y = ty0 + wave + k * (WG / 64);
      if (y <= ty1) sum[(int64_t)y * w + x] = acc[k];
    }
  }
}

// byte ranges [a, a + na) and [b, b + nb) overlap
bool overlap(uintptr_t a, unsigned long long na, uintptr_t b, unsigned long long nb) { return a < b + nb && b < a + na; }

}  // namespace

extern "C" int mc_affine_warp_sum(const void* src, int storage, const float* gain, const float* mu, int t, int h, int w,
                                  const double* m, const float* shifts, float* sum, float* frames, void* stream) {
  if (!src || !m || !shifts || !sum) return MC_ERR_ARG;
  if (t < 1 || h < 4 || w < 4) return MC_ERR_ARG;
  if (storage < MC_STORE_U8 || storage > MC_STORE_F32) return MC_ERR_ARG;
  const bool raw = storage == MC_STORE_U8 || storage == MC_STORE_I16;
  if (raw && (!gain || !mu)) return MC_ERR_ARG;
  const Mat mat{m[0], m[1], m[2], m[3]};
  if (!affine::matrix_ok(mat)) return MC_ERR_ARG;
  const int elem = storage == MC_STORE_U8 ? 1 : storage == MC_STORE_F32 ? 4 : 2;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(sum),
                  f0 = reinterpret_cast<uintptr_t>(frames);
  if (s0 % elem || d0 % 4 || f0 % 4 || reinterpret_cast<uintptr_t>(shifts) % 4) return MC_ERR_ARG;
  if (raw && (reinterpret_cast<uintptr_t>(gain) % 4 || reinterpret_cast<uintptr_t>(mu) % 4)) return MC_ERR_ARG;
  if ((long long)h * w >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  // the outputs alias neither the movie nor each other (t * h * w * 4 < 2^64)
  const unsigned long long hw = (unsigned long long)h * (unsigned long long)w, n = hw * (unsigned long long)t;
  if (overlap(s0, n * elem, d0, hw * 4)) return MC_ERR_ARG;
  if (frames && (overlap(s0, n * elem, f0, n * 4) || overlap(d0, hw * 4, f0, n * 4))) return MC_ERR_ARG;

  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;  // h * w < 2^31: the product fits
  const dim3 grid((unsigned)(tiles_x * tiles_y));
  mc_pick_kind(storage, [&](auto K) {
    mc_pick(frames != nullptr, [&](auto F) {
      hipLaunchKernelGGL((affine_warp_sum<K.value, F.value>), grid, dim3(WG), 0, st, src, gain, mu, t, h, w, mat,
                         shifts, sum, frames, tiles_x);
    });
  });
  return mc_check_launch();
}
