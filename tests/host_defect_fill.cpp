// CPU run of the defect fill's per-thread bodies (csrc/defect_fill.h, the source defect_fill.hip compiles for the
// device): every thread of every launch is executed in turn, on exactly-sized heap buffers, and the tables, the
// filled movie and the filled gain are compared with naive loops.  Meant to be built with the address and
// undefined-behaviour sanitizers, which then see every load and store of the three bodies:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_defect_fill.cpp -o host_defect_fill && ./host_defect_fill
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "defect_fill.h"

namespace df = defect_fill;

static unsigned rng_state = 2463534242u;
static unsigned rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// the map of tests/test_defect_fill.py: corners, an edge pixel, dead columns 0 and w / 2 + 37, a dead row, and a
// block x block square (7: its centre's first good ring is r = 4); frames too small for a feature go without it
static std::vector<unsigned char> planted_map(int h, int w, int block) {
  std::vector<unsigned char> m((size_t)h * w, 0);
  auto set = [&](int y, int x) {
    if (y >= 0 && y < h && x >= 0 && x < w) m[(size_t)y * w + x] = 1;
  };
  set(0, 0), set(0, w - 1), set(h - 1, 0), set(h - 1, w - 1), set(h / 2, w - 1), set(0, w / 3);
  if (w > 64)
    for (int y = 0; y < h; ++y) set(y, 0), set(y, w / 2 + 37);
  if (h > 16)
    for (int x = 0; x < w; ++x) set(h - 6, x);
  if (h > 2 * block && w > 4 * block)
    for (int y = 0; y < block; ++y)
      for (int x = 0; x < block; ++x) set(4 + y, w / 4 + x);
  set(3, 5), set(3, 6), set(4, 5);  // a small cluster
  return m;
}

// naive: the whole (2 r + 1)^2 window scanned in row-major order, Chebyshev distance tested per pixel
static void naive_donors(const std::vector<unsigned char>& map, int h, int w, const std::vector<int>& pixels,
                         int reach, std::vector<int>& donors, std::vector<int>& counts) {
  const int slots = 8 * reach;
  donors.assign(pixels.size() * slots, -1);
  counts.assign(pixels.size(), 0);
  for (size_t j = 0; j < pixels.size(); ++j) {
    const int y = pixels[j] / w, x = pixels[j] % w;
    for (int r = 1; r <= reach && counts[j] == 0; ++r)
      for (int yy = y - r; yy <= y + r; ++yy)
        for (int xx = x - r; xx <= x + r; ++xx) {
          const int dy = abs(yy - y), dx = abs(xx - x);
          if ((dy > dx ? dy : dx) != r || yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
          if (!map[(size_t)yy * w + xx]) donors[j * slots + counts[j]++] = yy * w + xx;
        }
  }
}

static unsigned naive_pick(unsigned seed, unsigned f, unsigned j, unsigned count) {
  unsigned long long x = (seed ^ (unsigned)(f * 0x9E3779B1ull) ^ (unsigned)(j * 0x85EBCA77ull)) & 0xffffffffull;
  x ^= x >> 16;
  x = (x * 0x85EBCA6Bull) & 0xffffffffull;
  x ^= x >> 13;
  x = (x * 0xC2B2AE35ull) & 0xffffffffull;
  x ^= x >> 16;
  return (unsigned)((x * count) >> 32);
}

struct Tables {
  std::vector<int> pixels;
  int *donors, *counts;  // exact-size heap blocks
  int n, reach;
};

// runs defect_donors' threads and compares with the naive tables; returns the heap tables for the fills
static int run_donors(const std::vector<unsigned char>& map, int h, int w, int reach, Tables* out) {
  std::vector<int> pixels;
  for (int p = 0; p < h * w; ++p)
    if (map[p]) pixels.push_back(p);
  const int n = (int)pixels.size(), slots = 8 * reach;
  unsigned char* dmap = static_cast<unsigned char*>(malloc((size_t)h * w));
  int* px = static_cast<int*>(malloc(sizeof(int) * (n ? n : 1)));
  int* donors = static_cast<int*>(malloc(sizeof(int) * (n ? (size_t)n * slots : 1)));
  int* counts = static_cast<int*>(malloc(sizeof(int) * (n ? n : 1)));
  if (!dmap || !px || !donors || !counts) abort();
  memcpy(dmap, map.data(), (size_t)h * w);
  if (n) memcpy(px, pixels.data(), sizeof(int) * n);
  memset(donors, 0x5a, sizeof(int) * (n ? (size_t)n * slots : 1));
  memset(counts, 0x5a, sizeof(int) * (n ? n : 1));
  const long long blocks = (n + df::WG - 1) / df::WG;
  for (long long b = 0; b < blocks; ++b)
    for (int th = 0; th < df::WG; ++th) df::donors_body(b * df::WG + th, dmap, h, w, px, n, reach, donors, counts);
  std::vector<int> want_d, want_c;
  naive_donors(map, h, w, pixels, reach, want_d, want_c);
  int bad = 0, none = 0;
  for (int j = 0; j < n && !bad; ++j) {
    if (counts[j] != want_c[j] || memcmp(donors + (size_t)j * slots, &want_d[(size_t)j * slots], sizeof(int) * slots)) {
      printf("  defect %d (pixel %d): count %d, naive %d\n", j, pixels[j], counts[j], want_c[j]);
      bad = 1;
    }
    none += counts[j] == 0;
  }
  printf("donors (%d,%d) reach=%d n=%d without=%d: %s\n", h, w, reach, n, none, bad ? "FAIL" : "ok");
  free(dmap);
  free(px);
  out->pixels = pixels;
  out->donors = donors;
  out->counts = counts;
  out->n = n;
  out->reach = reach;
  return bad;
}

template <int ES>
static int run_fill(const Tables& tb, int t, int h, int w, int offset_elems, unsigned seed) {
  typedef typename df::Elem<ES>::type T;
  const size_t hw = (size_t)h * w, total = (size_t)t * hw;
  T* alloc = static_cast<T*>(malloc((total + offset_elems) * ES));
  int* px = static_cast<int*>(malloc(sizeof(int) * (tb.n ? tb.n : 1)));
  if (!alloc || !px) abort();
  if (tb.n) memcpy(px, tb.pixels.data(), sizeof(int) * tb.n);
  T* movie = alloc + offset_elems;
  for (int k = 0; k < offset_elems; ++k) alloc[k] = (T)0x5a5a5a5au;
  std::vector<T> before(total);
  for (size_t i = 0; i < total; ++i) before[i] = movie[i] = (T)rng();
  // the launch: j along x, frames along y
  const long long blocks = (tb.n + df::WG - 1) / df::WG;
  for (int f = 0; f < t; ++f)
    for (long long b = 0; b < blocks; ++b)
      for (int th = 0; th < df::WG; ++th)
        df::fill_body<ES>(b * df::WG + th, f, reinterpret_cast<unsigned char*>(movie), (long long)hw, px, tb.donors,
                          tb.counts, tb.n, tb.reach, seed);
  std::vector<T> want(before);
  const int slots = 8 * tb.reach;
  for (int f = 0; f < t; ++f)
    for (int j = 0; j < tb.n; ++j)
      if (tb.counts[j] > 0) {
        const unsigned k = naive_pick(seed, (unsigned)f, (unsigned)j, (unsigned)tb.counts[j]);
        want[f * hw + tb.pixels[j]] = before[f * hw + tb.donors[(size_t)j * slots + k]];
      }
  int bad = 0;
  for (size_t i = 0; i < total && !bad; ++i)
    if (movie[i] != want[i]) {
      printf("  element %zu: %llu, naive %llu\n", i, (unsigned long long)movie[i], (unsigned long long)want[i]);
      bad = 1;
    }
  for (int k = 0; k < offset_elems; ++k) bad |= alloc[k] != (T)0x5a5a5a5au;  // nothing before the view was written
  printf("fill es=%d (%d,%d,%d) reach=%d seed=%u offset=%d: %s\n", ES, t, h, w, tb.reach, seed, offset_elems,
         bad ? "FAIL" : "ok");
  free(alloc);
  free(px);
  return bad;
}

static int run_gain(const Tables& tb, int h, int w) {
  const size_t hw = (size_t)h * w;
  float* gain = static_cast<float*>(malloc(sizeof(float) * hw));
  int* px = static_cast<int*>(malloc(sizeof(int) * (tb.n ? tb.n : 1)));
  if (!gain || !px) abort();
  if (tb.n) memcpy(px, tb.pixels.data(), sizeof(int) * tb.n);
  std::vector<float> before(hw);
  for (size_t i = 0; i < hw; ++i) before[i] = gain[i] = 0.25f + (float)(rng() % 100000) * 3.75e-5f;
  for (int j = 0; j < tb.n; ++j) before[tb.pixels[j]] = gain[tb.pixels[j]] = 0.0f;
  const long long blocks = (tb.n + df::WG - 1) / df::WG;
  for (long long b = 0; b < blocks; ++b)
    for (int th = 0; th < df::WG; ++th)
      df::gain_body(b * df::WG + th, gain, (long long)hw, px, tb.donors, tb.counts, tb.n, tb.reach);
  std::vector<float> want(before);
  const int slots = 8 * tb.reach;
  for (int j = 0; j < tb.n; ++j) {
    if (tb.counts[j] < 1) continue;
    double s = 0.0;
    for (int k = 0; k < tb.counts[j]; ++k) s += (double)before[tb.donors[(size_t)j * slots + k]];
    want[tb.pixels[j]] = (float)(s / tb.counts[j]);
  }
  int bad = memcmp(gain, want.data(), sizeof(float) * hw) != 0;
  for (int j = 0; j < tb.n && !bad; ++j) bad |= tb.counts[j] > 0 && !(gain[tb.pixels[j]] > 0.0f);
  printf("gain (%d,%d) reach=%d: %s\n", h, w, tb.reach, bad ? "FAIL" : "ok");
  free(gain);
  free(px);
  return bad;
}

// tables that cannot be used -- a count outside 1 .. 8 * reach, a pixel or a donor outside the frame: every body
// writes nothing (the sanitizers see that nothing outside the buffers is read either), and defect_donors answers a
// pixel outside the frame with count 0 and an empty row
static int run_damaged() {
  const int h = 4, w = 4, hw = h * w, reach = 1, slots = 8, n = 7, t = 2;
  const int pixel_v[n] = {5, 5, 5, -1, hw, 5, 5}, count_v[n] = {slots + 1, 0, -3, 1, 1, 1, 1};
  const int donor_v[n] = {6, 6, 6, 6, 6, hw, -1};
  int* pixels = static_cast<int*>(malloc(sizeof(int) * n));
  int* counts = static_cast<int*>(malloc(sizeof(int) * n));
  int* donors = static_cast<int*>(malloc(sizeof(int) * n * slots));
  unsigned char* movie = static_cast<unsigned char*>(malloc((size_t)t * hw));
  float* gain = static_cast<float*>(malloc(sizeof(float) * hw));
  unsigned char* map = static_cast<unsigned char*>(calloc(hw, 1));
  if (!pixels || !counts || !donors || !movie || !gain || !map) abort();
  for (int j = 0; j < n; ++j) {
    pixels[j] = pixel_v[j];
    counts[j] = count_v[j];
    for (int k = 0; k < slots; ++k) donors[j * slots + k] = donor_v[j];
  }
  for (int i = 0; i < t * hw; ++i) movie[i] = (unsigned char)(i + 1);
  for (int i = 0; i < hw; ++i) gain[i] = 1.0f + i;
  for (int f = 0; f < t; ++f)
    for (int th = 0; th < df::WG; ++th) {
      df::fill_body<1>(th, f, movie, hw, pixels, donors, counts, n, reach, 3u);
      if (f == 0) df::gain_body(th, gain, hw, pixels, donors, counts, n, reach);
    }
  int bad = 0;
  for (int i = 0; i < t * hw; ++i) bad |= movie[i] != (unsigned char)(i + 1);
  for (int i = 0; i < hw; ++i) bad |= gain[i] != 1.0f + i;
  for (int th = 0; th < df::WG; ++th) df::donors_body(th, map, h, w, pixels, n, reach, donors, counts);
  for (int j = 0; j < n; ++j) {
    const bool inside = pixel_v[j] == 5;
    bad |= counts[j] != (inside ? 8 : 0);
    for (int k = 0; k < slots; ++k) bad |= inside ? donors[j * slots + k] < 0 : donors[j * slots + k] != -1;
  }
  printf("damaged tables: %s\n", bad ? "FAIL" : "ok");
  free(pixels), free(counts), free(donors), free(movie), free(gain), free(map);
  return bad;
}

int main() {
  int bad = 0;
  // the pick: the device body against 64-bit arithmetic, and inside its range
  for (unsigned i = 0; i < 200000; ++i) {
    const unsigned seed = rng() << 8 ^ rng(), f = rng() % 70000, j = rng() << 7 ^ rng(), c = 1 + rng() % 128;
    const unsigned k = df::pick(seed, f, j, c);
    if (k != naive_pick(seed, f, j, c) || k >= c) bad = 1;
  }
  printf("pick: %s\n", bad ? "FAIL" : "ok");

  static const int frames[][3] = {{5, 33, 927}, {1, 8, 16}, {3, 64, 4096}};
  static const unsigned seeds[] = {0u, 12345u};
  for (const auto& s : frames) {
    const int t = s[0], h = s[1], w = s[2];
    for (int reach : {1, 4, 16}) {
      Tables tb;
      bad |= run_donors(planted_map(h, w, 7), h, w, reach, &tb);
      for (unsigned seed : seeds) {
        bad |= run_fill<1>(tb, t, h, w, 0, seed);
        bad |= run_fill<2>(tb, t, h, w, 0, seed);
        bad |= run_fill<4>(tb, t, h, w, 0, seed);
      }
      // a view that starts one element off the allocation
      for (unsigned seed : seeds) {
        bad |= run_fill<1>(tb, t, h, w, 1, seed);
        bad |= run_fill<2>(tb, t, h, w, 1, seed);
        bad |= run_fill<4>(tb, t, h, w, 1, seed);
      }
      bad |= run_gain(tb, h, w);
      free(tb.donors);
      free(tb.counts);
    }
  }
  // a 9 x 9 block: its centre has no donor at reach 4, and its row is skipped by both fills
  {
    Tables tb;
    bad |= run_donors(planted_map(33, 927, 9), 33, 927, 4, &tb);
    bad |= run_fill<2>(tb, 2, 33, 927, 0, 7u);
    bad |= run_gain(tb, 33, 927);
    free(tb.donors);
    free(tb.counts);
  }
  // no defects at all: no thread does anything
  {
    Tables tb;
    bad |= run_donors(std::vector<unsigned char>(8 * 16, 0), 8, 16, 4, &tb);
    bad |= run_fill<1>(tb, 2, 8, 16, 0, 0u);
    bad |= run_gain(tb, 8, 16);
    free(tb.donors);
    free(tb.counts);
  }
  // every pixel a defect: every count is 0
  {
    Tables tb;
    bad |= run_donors(std::vector<unsigned char>(5 * 7, 1), 5, 7, 16, &tb);
    bad |= run_fill<4>(tb, 2, 5, 7, 0, 1u);
    free(tb.donors);
    free(tb.counts);
  }
  bad |= run_damaged();
  printf(bad ? "FAIL\n" : "OK\n");
  return bad;
}
