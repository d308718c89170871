// Resampling of a frame through a 2 x 2 linear map about its centre (magnification distortion correction): the rule,
// the tile and window geometry of affine_resample.hip and its per-pixel body, written so that a host compiler takes
// them as well: tests/host_affine_resample.cpp runs the same bodies, tile after tile and pixel after pixel, under the
// address and undefined-behaviour sanitizers.  Nothing here needs the HIP runtime.
//
// THE RULE.  For the output pixel (y, x) of an h x w frame, with the centre cy = h / 2, cx = w / 2 (integer division)
// and the matrix M = [[m00, m01], [m10, m11]], everything float64:
//
//   py = (cy + m00 * (y - cy)) + m01 * (x - cx)
//   px = (cx + m10 * (y - cy)) + m11 * (x - cx)
//
// evaluated from the integers y, x in exactly this order, every product and sum rounded on its own (no fused
// multiply-add): position() gives the same bits on the host, on the device and in numpy
// (tests/magnification_reference.py), so the inside / outside decision is the same everywhere.
//   - py < 0, py > h - 1, px < 0 or px > w - 1: the output is fill_value.
//   - otherwise iy = floor(py), ix = floor(px); the fractions py - iy, px - ix are exact in float64 and are rounded
//     to fp32 once.
//   - the output is sum_k wy[k] * (sum_j wx[j] * v[iy - 1 + k][ix - 1 + j]) with the Keys cubic-convolution weights,
//     A = -0.75, in the Horner forms of the package's warps (warp_common.h: cubic_coeffs_fast), evaluated in fp32;
//     they may contract to fused multiply-adds, which removes roundings only.
//   - a tap outside the frame reads the clamped edge pixel.
//   - ACCUMULATION, fp32, in this order: each of the four tap rows k = 0 .. 3 is
//     r[k] = ((wx[0] v[k][0] + wx[1] v[k][1]) + wx[2] v[k][2]) + wx[3] v[k][3], and the output is
//     ((wy[0] r[0] + wy[1] r[1]) + wy[2] r[2]) + wy[3] r[3].
// With M the identity the positions are the integers themselves, the weights are exactly (0, 1, 0, 0) and the output
// is the input's value, bit for bit (for finite samples).
//
// THE TILE AND ITS WINDOW.  A workgroup makes one TILE x TILE output tile.  A position is a sum of functions that are
// each monotonic in y and in x, rounding included, so over a tile py and px take their extremes at its four corner
// pixels.  Of the interval between them only the part inside [0, n - 1] can be sampled; with lo and hi its ends the
// taps lie in source rows floor(lo) - 1 .. floor(hi) + 2 (columns likewise): the WINDOW, which is staged once --
// clamped to the frame, so a tap needs no clamp of its own -- and then serves all 16 taps of every pixel of the tile.
// Its size: hi - lo <= (|m00| + |m01|) (TILE - 1), and the entry point refuses an M whose row sums of |entries| leave
// [0.8, 1.25], so floor(hi) - floor(lo) <= floor(1.25 (TILE - 1)) + 1 and the window has at most
// WIN = floor(1.25 (TILE - 1)) + 1 + 4 rows and as many columns (83 for TILE = 64).  Magnification matrices are
// within 0.1 of the identity: their windows are about 1.1 TILE + 4 wide.  A window row is STRIDE floats apart, a
// multiple of the LDS's 32 banks: a lane's bank then depends on its tap's column alone, and the lanes of a wave, one
// output pixel apart along x, stay on distinct banks however the map shears their rows.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AR_HD __host__ __device__ __forceinline__
#else
#define AR_HD inline
#endif

namespace affine {

constexpr int TILE = 64;                                  // output rows and columns of a workgroup
constexpr double ROW_SUM_MIN = 0.8, ROW_SUM_MAX = 1.25;   // of |m00| + |m01| and of |m10| + |m11|
constexpr int WIN = (int)(ROW_SUM_MAX * (TILE - 1)) + 1 + 4;  // window rows / columns, at most
constexpr int STRIDE = 96;                                // floats between window rows
static_assert(WIN == 83 && STRIDE >= WIN && STRIDE % 32 == 0, "window geometry");

struct Mat {
  double m00, m01, m10, m11;
};

struct Pos {
  double py, px;
};

AR_HD Pos position(int h, int w, const Mat& m, int y, int x) {
#pragma clang fp contract(off)
  const int cy = h / 2, cx = w / 2;
  const double dy = (double)(y - cy), dx = (double)(x - cx);
  Pos p;
  p.py = ((double)cy + m.m00 * dy) + m.m01 * dx;
  p.px = ((double)cx + m.m10 * dy) + m.m11 * dx;
  return p;
}

AR_HD bool outside(const Pos& p, int h, int w) {
  return p.py < 0.0 || p.py > (double)(h - 1) || p.px < 0.0 || p.px > (double)(w - 1);
}

// what the entry point refuses of M: a value that is not finite, a row sum of |entries| outside the bounds
AR_HD bool finite(double v) { return v - v == 0.0; }
AR_HD bool matrix_ok(const Mat& m) {
  if (!finite(m.m00) || !finite(m.m01) || !finite(m.m10) || !finite(m.m11)) return false;
  const double r0 = __builtin_fabs(m.m00) + __builtin_fabs(m.m01), r1 = __builtin_fabs(m.m10) + __builtin_fabs(m.m11);
  return r0 >= ROW_SUM_MIN && r0 <= ROW_SUM_MAX && r1 >= ROW_SUM_MIN && r1 <= ROW_SUM_MAX;
}

// the source rows y0 .. y0 + rows - 1 and columns x0 .. x0 + cols - 1 a tile's taps lie in (from -1 to n + 1: they
// are clamped when the window is staged); rows == cols == 0 for a tile without a pixel inside
struct Window {
  int y0, x0, rows, cols;
};

// one axis: the positions' extremes a <= b over the tile -> first index and count
AR_HD void window_axis(double a, double b, int n, int* first, int* count) {
  const double lo = a < 0.0 ? 0.0 : a, hi = b > (double)(n - 1) ? (double)(n - 1) : b;
  if (!(lo <= hi)) {
    *first = 0;
    *count = 0;
    return;
  }
  *first = (int)__builtin_floor(lo) - 1;
  *count = (int)__builtin_floor(hi) + 2 - *first + 1;
}

// the window of the tile of output rows ty0 .. ty1 and columns tx0 .. tx1 (inclusive)
AR_HD Window window(int h, int w, const Mat& m, int ty0, int ty1, int tx0, int tx1) {
  const Pos c[4] = {position(h, w, m, ty0, tx0), position(h, w, m, ty0, tx1), position(h, w, m, ty1, tx0),
                    position(h, w, m, ty1, tx1)};
  double ymin = c[0].py, ymax = c[0].py, xmin = c[0].px, xmax = c[0].px;
  for (int i = 1; i < 4; ++i) {
    ymin = c[i].py < ymin ? c[i].py : ymin;
    ymax = c[i].py > ymax ? c[i].py : ymax;
    xmin = c[i].px < xmin ? c[i].px : xmin;
    xmax = c[i].px > xmax ? c[i].px : xmax;
  }
  Window wd;
  window_axis(ymin, ymax, h, &wd.y0, &wd.rows);
  window_axis(xmin, xmax, w, &wd.x0, &wd.cols);
  if (wd.rows == 0 || wd.cols == 0) wd.rows = wd.cols = 0;
  return wd;
}

// the frame index window element i of an axis is staged from: the clamped edge outside the frame
AR_HD int clamped(int first, int i, int n) {
  const int s = first + i;
  return s < 0 ? 0 : s > n - 1 ? n - 1 : s;
}

// Keys weights, A = -0.75, of the fp32 fraction t: the Horner forms of warp_common.h's cubic_coeffs_fast
AR_HD void cubic_weights(float t, float c[4]) {
#pragma clang fp contract(fast)
  const float A = -0.75f;
  float x = t + 1.f;
  c[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  x = t;
  c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 1.f - t;
  c[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 2.f - t;
  c[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

AR_HD float dot4(const float c[4], const float* v) {
#pragma clang fp contract(fast)
  return ((c[0] * v[0] + c[1] * v[1]) + c[2] * v[2]) + c[3] * v[3];
}

// the output pixel (y, x) of a tile whose window `win` (rows STRIDE apart) is staged
AR_HD float pixel(const float* win, const Window& wd, int h, int w, const Mat& m, int y, int x, float fill_value) {
  const Pos p = position(h, w, m, y, x);
  if (outside(p, h, w)) return fill_value;
  const double fly = __builtin_floor(p.py), flx = __builtin_floor(p.px);
  float wy[4], wx[4], r[4];
  cubic_weights((float)(p.py - fly), wy);
  cubic_weights((float)(p.px - flx), wx);
  const float* tap = win + ((int)fly - 1 - wd.y0) * STRIDE + ((int)flx - 1 - wd.x0);
  for (int k = 0; k < 4; ++k) r[k] = dot4(wx, tap + k * STRIDE);
  return dot4(wy, r);
}

}  // namespace affine
