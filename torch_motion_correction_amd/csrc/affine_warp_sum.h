// The aligned sum of a movie with the magnification correction folded into the rigid warp: every frame is
// interpolated ONCE, at c + M (p - c) + shift_f, and the frames are added as they are formed.  The rule, the window of
// a tile for a frame and the per-pixel body of affine_warp_sum.hip, over affine_resample.h (which this header includes
// and leaves as it is) and written, like it, so that a host compiler takes them: tests/host_affine_warp_sum.cpp runs
// the same bodies, tile after tile and frame after frame, under the address and undefined-behaviour sanitizers.
// Nothing here needs the HIP runtime.
//
// THE RULE.  For the output pixel (y, x), frame f, matrix M and the frame's fp32 pixel shift (sy_f, sx_f), which
// widens to float64 exactly:
//
//   (py0, px0) = affine::position(h, w, M, y, x)              unchanged, no fused multiply-add
//   py = py0 + (double)sy_f ;  px = px0 + (double)sx_f        one rounded add each, no fused multiply-add
//
// so that host, device and numpy (tests/magnified_sum_reference.py) carry the same bits and decide inside / outside
// alike.  The sign is the rigid warp's: a sample is taken at p + s.
//   - py < 0, py > h - 1, px < 0 or px > w - 1 (or a position that is not a number): frame f contributes exactly 0.0f
//     to this pixel -- the rigid warp's zero-outside rule.  There is no fill_value.
//   - otherwise iy = floor(py), ix = floor(px), the fractions py - iy, px - ix (exact in float64) are rounded to fp32
//     once, and the value v_f is that of affine::pixel: cubic_weights, dot4, edge-clamped taps, in the ACCUMULATION
//     order affine_resample.h writes down.
//   - THE SUM is the fp32 sequence ((0 + v_0) + v_1) + ... + v_{t-1} in frame order, one accumulator per pixel: no
//     atomics and no partial slabs, so its bits do not depend on the launch geometry.  (The accumulator starts at +0
//     and can never become -0, so leaving out a frame that contributes +0 changes no bit.)
//   - A SAMPLE's value, by storage kind (MC_STORE_*): f32 as stored; f16 widened; u8 / i16
//     fp32(raw) * gain[y][x] - mu_f, the product rounded, then the difference rounded (NO fused multiply-add): the
//     expression of mc_condition_movie, so that the raw route gives the bits of the fp32 route on the conditioned
//     movie.  A clamped tap takes the gain of the pixel it is clamped to, as the conditioned frame's edge pixel would.
//
// THE WINDOW OF A TILE FOR FRAME f.  fl(p0 + s) is monotonic in p0 (rounding is), and p0 is a sum of terms monotonic in
// y and in x, rounding included (affine_resample.h): over a tile the shifted py and px still take their extremes at
// its four corner pixels.  With lo <= hi the ends of that interval cut to [0, n - 1], the taps lie in source rows
// floor(lo) - 1 .. floor(hi) + 2 (affine::window_axis, unchanged).  Its size: for corner values a0 <= b0 before the
// shift, b0 - a0 <= 1.25 (TILE - 1) = 78.75 up to the roundings of position(); the shifted ends are fl(a0 + s) and
// fl(b0 + s), each within half an ulp of the exact sum, so hi - lo <= (b0 - a0) + ulp(max(|hi|, |lo|)).  Only
// intervals that meet [0, n - 1] matter, n < 2^31, where a float64 ulp is below 2^-21: hi - lo < 78.75 + 2^-20 < 79,
// floor(hi) - floor(lo) <= floor(hi - lo) + 1 <= 79, and the window has at most 79 + 4 = 83 = WIN rows and columns, as
// without a shift.  Adding a constant does not widen the window beyond one rounding, and the bound has a quarter of
// a pixel to spare.  A shift so large that lo > hi (or one that is not a number) gives an EMPTY window: the tile skips
// that frame, which contributes 0 to all its pixels; pixel() is never evaluated for it.
#pragma once
#include "affine_resample.h"

namespace affine {

// the shifted position of output pixel (y, x): position() plus the frame's shift, one rounded add per axis
AR_HD Pos shifted_position(int h, int w, const Mat& m, int y, int x, float sy, float sx) {
#pragma clang fp contract(off)
  Pos p = position(h, w, m, y, x);
  p.py = p.py + (double)sy;
  p.px = p.px + (double)sx;
  return p;
}

// inside [0, h - 1] x [0, w - 1]; false for a position that is not a number
AR_HD bool inside(const Pos& p, int h, int w) {
  return p.py >= 0.0 && p.py <= (double)(h - 1) && p.px >= 0.0 && p.px <= (double)(w - 1);
}

// the window of the tile of output rows ty0 .. ty1 and columns tx0 .. tx1 (inclusive) for a frame shifted by (sy, sx);
// rows == cols == 0 where no pixel of the tile samples inside the frame
AR_HD Window shifted_window(int h, int w, const Mat& m, int ty0, int ty1, int tx0, int tx1, float sy, float sx) {
  const Pos c[4] = {shifted_position(h, w, m, ty0, tx0, sy, sx), shifted_position(h, w, m, ty0, tx1, sy, sx),
                    shifted_position(h, w, m, ty1, tx0, sy, sx), shifted_position(h, w, m, ty1, tx1, sy, sx)};
  double ymin = c[0].py, ymax = c[0].py, xmin = c[0].px, xmax = c[0].px;
  for (int i = 1; i < 4; ++i) {
    ymin = c[i].py < ymin ? c[i].py : ymin;
    ymax = c[i].py > ymax ? c[i].py : ymax;
    xmin = c[i].px < xmin ? c[i].px : xmin;
    xmax = c[i].px > xmax ? c[i].px : xmax;
  }
  Window wd;
  wd.y0 = wd.x0 = wd.rows = wd.cols = 0;
  if (!(ymin <= ymax && xmin <= xmax)) return wd;  // a shift that is not a number
  window_axis(ymin, ymax, h, &wd.y0, &wd.rows);
  window_axis(xmin, xmax, w, &wd.x0, &wd.cols);
  if (wd.rows == 0 || wd.cols == 0) wd.rows = wd.cols = 0;
  return wd;
}

// one conditioned sample of a raw movie: the expression and the contraction mode of mc_condition_movie
AR_HD float conditioned(float raw, float gain, float mu) {
#pragma clang fp contract(off)
  const float v = raw * gain;
  return v - mu;
}

// frame f's value at output pixel (y, x) of a tile whose window `win` (rows STRIDE apart, not empty) is staged
AR_HD float shifted_pixel(const float* win, const Window& wd, int h, int w, const Mat& m, int y, int x, float sy,
                          float sx) {
  const Pos p = shifted_position(h, w, m, y, x, sy, sx);
  if (!inside(p, h, w)) return 0.0f;
  const double fly = __builtin_floor(p.py), flx = __builtin_floor(p.px);
  float wy[4], wx[4], r[4];
  cubic_weights((float)(p.py - fly), wy);
  cubic_weights((float)(p.px - flx), wx);
  const float* tap = win + ((int)fly - 1 - wd.y0) * STRIDE + ((int)flx - 1 - wd.x0);
  for (int k = 0; k < 4; ++k) r[k] = dot4(wx, tap + k * STRIDE);
  return dot4(wy, r);
}

}  // namespace affine
