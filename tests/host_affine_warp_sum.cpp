// CPU run of the magnified sum's bodies (csrc/affine_warp_sum.h over csrc/affine_resample.h, the source
// affine_warp_sum.hip compiles for the device): every sum is made tile by tile and, within a tile, frame by frame
// exactly as the kernel's workgroups make it -- the tile's window for the frame computed, a frame with an empty window
// skipped, the window staged from the frame with clamped reads into a buffer of exactly rows x STRIDE floats, every
// pixel of the tile evaluated from that buffer and added to its fp32 accumulator -- with the movie allocated to its
// exact size as well.  Meant to be built with the address and undefined-behaviour sanitizers, which then see every
// load of the movie and of the window:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_affine_warp_sum.cpp -o host_affine_warp_sum \
//       && ./host_affine_warp_sum cases.bin results.bin
//
// cases.bin (written by tests/test_magnified_sum_host.py) is a list of records, little-endian:
//   int32 t, h, w, 0; double m00, m01, m10, m11; t x 2 floats (sy, sx); t * h * w floats of the movie.
// results.bin receives, per record: h * w floats of the sum, then per frame h * w doubles py, h * w doubles px and
// h * w bytes (1 where the frame contributes a value, 0 where it contributes 0).  The test compares them with the
// float64 restatement.  Printed per case: the largest window and the number of (tile, frame) pairs skipped.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "affine_warp_sum.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: host_affine_warp_sum cases.bin results.bin\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!fh || !out) return 2;
  int hdr[4];
  int cases = 0, failures = 0;
  while (fread(hdr, 4, 4, fh) == 4) {
    const int t = hdr[0], h = hdr[1], w = hdr[2];
    affine::Mat m;
    if (t < 1 || h < 4 || w < 4 || fread(&m, 8, 4, fh) != 4 || !affine::matrix_ok(m)) return 2;
    const size_t n = (size_t)h * w;
    float* shifts = new float[2 * (size_t)t];
    float* movie = new float[n * t];
    float* sum = new float[n];
    double* py = new double[n * t];
    double* px = new double[n * t];
    unsigned char* in = new unsigned char[n * t];
    if (fread(shifts, 4, 2 * (size_t)t, fh) != 2 * (size_t)t || fread(movie, 4, n * t, fh) != n * t) return 2;
    bool ok = true;
    int max_rows = 0, max_cols = 0, skipped = 0;
    for (int ty0 = 0; ty0 < h; ty0 += affine::TILE)
      for (int tx0 = 0; tx0 < w; tx0 += affine::TILE) {
        const int ty1 = (ty0 + affine::TILE < h ? ty0 + affine::TILE : h) - 1;
        const int tx1 = (tx0 + affine::TILE < w ? tx0 + affine::TILE : w) - 1;
        float acc[affine::TILE][affine::TILE];
        for (int y = ty0; y <= ty1; ++y)
          for (int x = tx0; x <= tx1; ++x) acc[y - ty0][x - tx0] = 0.f;
        for (int f = 0; f < t; ++f) {
          const float sy = shifts[2 * f], sx = shifts[2 * f + 1];
          const float* frame = movie + n * f;
          for (int y = ty0; y <= ty1; ++y)
            for (int x = tx0; x <= tx1; ++x) {
              const affine::Pos p = affine::shifted_position(h, w, m, y, x, sy, sx);
              py[n * f + (size_t)y * w + x] = p.py;
              px[n * f + (size_t)y * w + x] = p.px;
              in[n * f + (size_t)y * w + x] = affine::inside(p, h, w) ? 1 : 0;
            }
          const affine::Window wd = affine::shifted_window(h, w, m, ty0, ty1, tx0, tx1, sy, sx);
          if (wd.rows < 0 || wd.cols < 0 || wd.rows > affine::WIN || wd.cols > affine::WIN) {
            printf("case %d tile (%d, %d) frame %d: window %d x %d beyond the bound\n", cases, ty0, tx0, f, wd.rows,
                   wd.cols);
            ok = false;
            continue;
          }
          if (wd.rows == 0) {  // the kernel skips the frame: no pixel of the tile may be inside
            ++skipped;
            for (int y = ty0; y <= ty1; ++y)
              for (int x = tx0; x <= tx1; ++x)
                if (in[n * f + (size_t)y * w + x]) {
                  printf("case %d tile (%d, %d) frame %d: empty window, but pixel (%d, %d) is inside\n", cases, ty0,
                         tx0, f, y, x);
                  ok = false;
                }
            continue;
          }
          max_rows = wd.rows > max_rows ? wd.rows : max_rows;
          max_cols = wd.cols > max_cols ? wd.cols : max_cols;
          // exactly what the kernel stages: `cols` floats of each of `rows` rows, STRIDE apart, and no more
          const size_t len = (size_t)wd.rows * affine::STRIDE;
          float* win = new float[len];
          for (size_t i = 0; i < len; ++i) win[i] = NAN;  // the gaps between rows: a tap that strays reads a NaN
          for (int r = 0; r < wd.rows; ++r)
            for (int c = 0; c < wd.cols; ++c)
              win[(size_t)r * affine::STRIDE + c] =
                  frame[(size_t)affine::clamped(wd.y0, r, h) * w + affine::clamped(wd.x0, c, w)];
          for (int y = ty0; y <= ty1; ++y)
            for (int x = tx0; x <= tx1; ++x)
              acc[y - ty0][x - tx0] += affine::shifted_pixel(win, wd, h, w, m, y, x, sy, sx);
          delete[] win;
        }
        for (int y = ty0; y <= ty1; ++y)
          for (int x = tx0; x <= tx1; ++x) sum[(size_t)y * w + x] = acc[y - ty0][x - tx0];
      }
    if (fwrite(sum, 4, n, out) != n) return 2;
    for (int f = 0; f < t; ++f)
      if (fwrite(py + n * f, 8, n, out) != n || fwrite(px + n * f, 8, n, out) != n || fwrite(in + n * f, 1, n, out) != n)
        return 2;
    printf("case %d (%d x %d x %d, m %.4f %.4f %.4f %.4f): window at most %d x %d, %d tile-frames skipped%s\n", cases, t,
           h, w, m.m00, m.m01, m.m10, m.m11, max_rows, max_cols, skipped, ok ? "" : ": FAIL");
    if (!ok) ++failures;
    ++cases;
    delete[] shifts;
    delete[] movie;
    delete[] sum;
    delete[] py;
    delete[] px;
    delete[] in;
  }
  fclose(fh);
  if (fclose(out) != 0) return 2;
  printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
