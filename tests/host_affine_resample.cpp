// CPU run of the affine resampler's bodies (csrc/affine_resample.h, the source affine_resample.hip compiles for the
// device): every frame is made tile by tile exactly as the kernel's grid makes it -- the tile's window computed,
// staged from the frame with clamped reads into a buffer of exactly the window's size, every pixel of the tile
// evaluated from that buffer -- with the frame allocated to its exact size as well.  Meant to be built with the
// address and undefined-behaviour sanitizers, which then see every load of the frame and of the window:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_affine_resample.cpp -o host_affine_resample \
//       && ./host_affine_resample cases.bin
//
// cases.bin (written by tests/test_magnification_host.py) is a list of records, little-endian:
//   int32 h, w; float fill_value; int32 0; double m00, m01, m10, m11;
//   h * w floats of the frame, h * w doubles of the expected output, h * w doubles of the bound on |got - expected|.
// Where the bound is 0 the expected output is fill_value and the bits must be equal.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "affine_resample.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: host_affine_resample cases.bin\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int hdr[4];
  int cases = 0, failures = 0;
  while (fread(hdr, 4, 4, fh) == 4) {
    const int h = hdr[0], w = hdr[1];
    float fill;
    memcpy(&fill, &hdr[2], 4);
    affine::Mat m;
    if (h < 4 || w < 4 || fread(&m, 8, 4, fh) != 4 || !affine::matrix_ok(m)) return 2;
    const size_t n = (size_t)h * w;
    float* frame = new float[n];
    double* want = new double[n];
    double* bound = new double[n];
    float* got = new float[n];
    if (fread(frame, 4, n, fh) != n || fread(want, 8, n, fh) != n || fread(bound, 8, n, fh) != n) return 2;
    bool ok = true;
    for (int ty0 = 0; ty0 < h; ty0 += affine::TILE)
      for (int tx0 = 0; tx0 < w; tx0 += affine::TILE) {
        const int ty1 = (ty0 + affine::TILE < h ? ty0 + affine::TILE : h) - 1;
        const int tx1 = (tx0 + affine::TILE < w ? tx0 + affine::TILE : w) - 1;
        const affine::Window wd = affine::window(h, w, m, ty0, ty1, tx0, tx1);
        if (wd.rows < 0 || wd.cols < 0 || wd.rows > affine::WIN || wd.cols > affine::WIN) {
          printf("case %d tile (%d, %d): window %d x %d beyond the bound\n", cases, ty0, tx0, wd.rows, wd.cols);
          ok = false;
          continue;
        }
        // exactly what the kernel stages: `cols` floats of each of `rows` rows, STRIDE apart
        const size_t len = wd.rows ? (size_t)(wd.rows - 1) * affine::STRIDE + wd.cols : 0;
        float* win = new float[len];
        for (size_t i = 0; i < len; ++i) win[i] = NAN;  // the gaps between rows: a tap that strays reads a NaN
        for (int r = 0; r < wd.rows; ++r)
          for (int c = 0; c < wd.cols; ++c)
            win[(size_t)r * affine::STRIDE + c] =
                frame[(size_t)affine::clamped(wd.y0, r, h) * w + affine::clamped(wd.x0, c, w)];
        for (int y = ty0; y <= ty1; ++y)
          for (int x = tx0; x <= tx1; ++x) got[(size_t)y * w + x] = affine::pixel(win, wd, h, w, m, y, x, fill);
        delete[] win;
      }
    int bad = 0;
    for (size_t i = 0; i < n; ++i) {
      const bool good = bound[i] == 0.0 ? memcmp(&got[i], &fill, 4) == 0 && want[i] == (double)fill
                                        : fabs((double)got[i] - want[i]) <= bound[i];
      if (!good && bad++ == 0)
        printf("case %d (%d x %d): pixel (%zu, %zu) got %.9g want %.17g bound %.3g\n", cases, h, w, i / w, i % w,
               (double)got[i], want[i], bound[i]);
    }
    if (bad || !ok) {
      ++failures;
      printf("case %d (%d x %d, m %.4f %.4f %.4f %.4f): FAIL, %d pixels\n", cases, h, w, m.m00, m.m01, m.m10, m.m11, bad);
    }
    ++cases;
    delete[] frame;
    delete[] want;
    delete[] bound;
    delete[] got;
  }
  fclose(fh);
  printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
