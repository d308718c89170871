// Frames resampled through a 2 x 2 linear map about their centre, bicubic: what removes a microscope's anisotropic
// magnification distortion from a sum or a stack.  The rule (float64 positions, the fill decision, the fp32 Keys
// weights, clamped taps, the accumulation order), the tile's source window, its size bound and the per-pixel body are
// in affine_resample.h; this file holds the kernel around them and the entry point's host checks.
//
//   affine_resample<T>  one 64 x 64 output tile per workgroup of 4 waves, blockIdx.y strides over the frames.  The
//                       tile's window (affine::window: at most 83 x 83 samples, about 74 x 74 for a magnification
//                       matrix) is staged into LDS row by row -- consecutive lanes read consecutive samples of a source
//                       row, clamped at the frame's edge, fp16 widened on the way -- and every pixel then takes its 16
//                       taps from LDS (affine::pixel).  A wave makes one output row of 64 pixels at a time.
//
// No scratch memory and no atomics; every output pixel is written once by one thread from inputs alone, so the result
// does not depend on scheduling.
// Bounds.  Staging reads frame[clamped row][clamped column] only; a tap of a pixel inside lies in the window by
// affine_resample.h's argument, which rests on the row sums of |M| the entry point checks before anything is
// launched; a pixel outside reads nothing.  Stores go to pixels (y <= y1, x <= x1) of the frame only.
#include "mc_common.h"
#include "mcorr.h"
#include "affine_resample.h"

namespace {

using affine::Mat;
using affine::STRIDE;
using affine::TILE;
using affine::WIN;
using affine::Window;

constexpr int WG = 256;

template <typename T>
__global__ __launch_bounds__(WG) void affine_resample(const T* __restrict__ src, int nframes, int h, int w, Mat m,
                                                      float fill_value, float* __restrict__ dst, int tiles_x) {
  __shared__ float win[WIN * STRIDE];
  const int ty0 = (int)(blockIdx.x / tiles_x) * TILE, tx0 = (int)(blockIdx.x % tiles_x) * TILE;
  const int ty1 = (ty0 + TILE < h ? ty0 + TILE : h) - 1, tx1 = (tx0 + TILE < w ? tx0 + TILE : w) - 1;
  const Window wd = affine::window(h, w, m, ty0, ty1, tx0, tx1);
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const int x = tx0 + lane;
  for (int f = blockIdx.y; f < nframes; f += gridDim.y) {
    const T* frame = src + (long long)f * h * w;
    float* out = dst + (long long)f * h * w;
    __syncthreads();  // the window may still be read for the frame before
    for (int i = threadIdx.x; i < wd.rows * STRIDE; i += WG) {
      const int r = i / STRIDE, c = i - r * STRIDE;
      if (c < wd.cols)
        win[i] = (float)frame[(long long)affine::clamped(wd.y0, r, h) * w + affine::clamped(wd.x0, c, w)];
    }
    __syncthreads();
    if (x <= tx1)
      for (int y = ty0 + wave; y <= ty1; y += WG / 64)
        __builtin_nontemporal_store(affine::pixel(win, wd, h, w, m, y, x, fill_value), out + (long long)y * w + x);
  }
}

template <typename T>
void launch(const void* src, int nframes, int h, int w, const Mat& m, float fill_value, float* dst, hipStream_t st) {
  const int tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;  // h * w < 2^31: the product fits
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(nframes < 65535 ? nframes : 65535));
  hipLaunchKernelGGL(affine_resample<T>, grid, dim3(WG), 0, st, static_cast<const T*>(src), nframes, h, w, m,
                     fill_value, dst, tiles_x);
}

}  // namespace

extern "C" int mc_affine_resample(const void* src, int storage, int nframes, int h, int w, const double m[4],
                                  float fill_value, float* dst, void* stream) {
  if (!src || !dst || !m) return MC_ERR_ARG;
  if (nframes < 1 || h < 4 || w < 4) return MC_ERR_ARG;
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  if ((long long)h * w >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  const Mat mat{m[0], m[1], m[2], m[3]};
  if (!affine::matrix_ok(mat)) return MC_ERR_ARG;
  const int elem = storage == MC_STORE_F32 ? 4 : 2;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  if (s0 % elem || d0 % 4) return MC_ERR_ARG;
  // dst must not alias src: the two byte ranges are disjoint (nframes * h * w * 4 < 2^64)
  const unsigned long long n = (unsigned long long)nframes * (unsigned long long)h * (unsigned long long)w;
  if (s0 < d0 + n * 4 && d0 < s0 + n * elem) return MC_ERR_ARG;

  hipStream_t st = (hipStream_t)stream;
  if (storage == MC_STORE_F32) launch<float>(src, nframes, h, w, mat, fill_value, dst, st);
  else launch<_Float16>(src, nframes, h, w, mat, fill_value, dst, st);
  return mc_check_launch();
}
