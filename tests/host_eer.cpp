// CPU run of the EER render's per-lane bodies (csrc/eer.h, the source eer_render.hip compiles for the device): the
// three passes are executed lane by lane, every lane of every workgroup in turn, on exactly-sized heap buffers, and
// the movie, the per-frame final n and the event counts are compared with a sequential bit-by-bit decode written
// here.  Meant to be built with the address and undefined-behaviour sanitizers, which then see every load of the
// stream -- the last strip of a buffer ends at the buffer's end, and every frame is also rendered alone from an
// allocation of exactly its own bytes -- and every store of the tables, states and output:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_eer.cpp -o host_eer && ./host_eer
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "eer.h"

typedef std::vector<unsigned char> Strip;

static unsigned rng_state = 2463534242u;
static double rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) / 16777216.0;
}

struct Writer {
  Strip bytes;
  long long nbits = 0;
  void put(unsigned v, int k) {
    for (int b = 0; b < k; ++b, ++nbits) {
      if ((nbits & 7) == 0) bytes.push_back(0);
      bytes[nbits >> 3] |= (unsigned char)(((v >> b) & 1u) << (nbits & 7));
    }
  }
};

// events at the pixels where rng() < density; `extra` is added to the trailing run (an overshoot when > 0)
static Strip encode(long long N, double density, int extra) {
  Writer wr;
  long long done = 0;  // pixels accounted for
  for (long long p = 0; p < N; ++p) {
    if (!(rng() < density)) continue;
    long long gap = p - done;
    for (; gap >= 127; gap -= 127) wr.put(127, 7);
    wr.put((unsigned)gap, 7);
    wr.put((unsigned)(rng() * 16) & 15u, 4);
    done = p + 1;
  }
  long long rest = N - done;
  if (rest == 0 || extra) {
    for (; rest >= 127; rest -= 127) wr.put(127, 7);
    wr.put((unsigned)(rest + extra), 7);  // (rest + extra < 127 for the cases below)
  } else {
    for (; rest >= 127; rest -= 127) wr.put(127, 7);
    if (rest) wr.put((unsigned)rest, 7);
  }
  return wr.bytes;
}

// ---- the sequential decode, bit by bit; bits beyond the strip read as zero
static unsigned bits_at(const Strip& s, long long bit, int k) {
  unsigned v = 0;
  for (int b = 0; b < k; ++b) {
    const long long q = bit + b;
    if (q < 8 * (long long)s.size()) v |= (unsigned)((s[q >> 3] >> (q & 7)) & 1) << b;
  }
  return v;
}

static void decode(const Strip& s, long long N, int w, int up, unsigned char* frame, int* final_n, int* events) {
  long long bit = 0, n = 0;
  int ev = 0;
  while (bit < 8 * (long long)s.size()) {
    const unsigned p = bits_at(s, bit, 7);
    bit += 7;
    n += p;
    if (n >= N) break;
    if (p == 127) continue;
    const unsigned c = bits_at(s, bit, 4);
    bit += 4;
    const long long y = n / w, x = n % w;
    if (frame) {
      if (up == 2) frame[(2 * y + ((c >> 3) & 1)) * 2 * w + 2 * x + ((c >> 1) & 1)] += 1;
      else frame[y * w + x] += 1;
    }
    ++ev;
    ++n;
  }
  *final_n = (int)n;
  *events = ev;
}

// ---- the three passes as mc_eer_render launches them; returns 1 on a mismatch
static int run_case(const char* what, const std::vector<Strip>& strips, int h, int w, int up, int g, int S) {
  const int n_frames = (int)strips.size(), t_out = n_frames / g;
  const long long N = (long long)h * w;
  size_t total = 0;
  for (const Strip& s : strips) total += s.size();
  unsigned char* data = static_cast<unsigned char*>(malloc(total ? total : 1));
  eer::Frame* frames = static_cast<eer::Frame*>(malloc(sizeof(eer::Frame) * n_frames));
  long long n_segments = 0, at = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (!strips[f].empty()) memcpy(data + at, strips[f].data(), strips[f].size());
    frames[f] = eer::Frame{at, (long long)strips[f].size(), n_segments};
    at += (long long)strips[f].size();
    n_segments += ((long long)strips[f].size() + S - 1) / S;
  }
  unsigned* tables = static_cast<unsigned*>(malloc(n_segments ? n_segments * eer::ENTRIES * 4 : 1));
  eer::u64* states = static_cast<eer::u64*>(malloc(n_segments ? n_segments * 8 : 1));
  const size_t out_bytes = (size_t)t_out * up * h * up * w;
  unsigned* out = static_cast<unsigned*>(calloc(out_bytes ? out_bytes : 4, 1));
  int* final_n = static_cast<int*>(malloc(sizeof(int) * n_frames));
  int* events = static_cast<int*>(malloc(sizeof(int) * n_frames));
  eer::Shared* sh = static_cast<eer::Shared*>(malloc(sizeof(eer::Shared)));
  memset(tables, 0x5a, n_segments ? n_segments * eer::ENTRIES * 4 : 1);

  const long long blocks = (n_segments + eer::WG - 1) / eer::WG;
  for (long long b = 0; b < blocks; ++b)
    for (int th = 0; th < eer::WG; ++th)
      eer::table_lane(b * eer::WG + th, n_segments, data, frames, n_frames, S, tables);
  for (int f = 0; f < n_frames; ++f) {
    for (int th = 0; th < eer::WG; ++th) eer::fold_lane(th, frames[f], S, tables, *sh);
    const eer::u64 unstopped = eer::walk_lanes(*sh);
    for (int th = 0; th < eer::WG; ++th) eer::rewalk_lane(th, frames[f], S, N, data, tables, states, *sh);
    eer::finish_frame(*sh, unstopped, final_n + f, events + f);
  }
  for (long long b = 0; b < blocks; ++b)
    for (int th = 0; th < eer::WG; ++th)
      eer::scatter_lane(b * eer::WG + th, n_segments, data, frames, n_frames, S, states, h, w, up, g, t_out, out);

  int bad = 0;
  std::vector<unsigned char> want(out_bytes ? out_bytes : 1, 0);
  for (int f = 0; f < n_frames; ++f) {
    int n, ev;
    unsigned char* frame = f / g < t_out ? want.data() + (size_t)(f / g) * up * h * up * w : nullptr;
    decode(strips[f], N, w, up, frame, &n, &ev);
    if (n != final_n[f] || ev != events[f]) {
      printf("  frame %d: final n %d events %d, sequential %d %d\n", f, final_n[f], events[f], n, ev);
      bad = 1;
    }
  }
  if (out_bytes && memcmp(want.data(), out, out_bytes)) {
    printf("  the movies differ\n");
    bad = 1;
  }
  printf("%s (%d,%d,%d) up=%d g=%d S=%d: %s\n", what, n_frames, h, w, up, g, S, bad ? "FAIL" : "ok");
  free(data);
  free(frames);
  free(tables);
  free(states);
  free(out);
  free(final_n);
  free(events);
  free(sh);
  return bad;
}

int main() {
  int bad = 0;
  static const int sizes[] = {16, 64, 128, 256};
  // the mixed densities of tests/test_eer_render.py, then a stream cut short, one whose last run overshoots, one
  // without bytes, one of a single byte and one of skips only
  std::vector<Strip> mixed;
  static const double densities[] = {0.0, 1.0, 0.5, 0.1, 0.02, 0.004, 0.3};
  for (double d : densities) mixed.push_back(encode(48 * 64, d, 0));
  std::vector<Strip> broken = mixed;
  broken[2].resize(broken[2].size() / 2);
  broken[3].resize(broken[3].size() - 1);
  broken.push_back(encode(48 * 64, 0.1, 5));
  broken.push_back(encode(48 * 64, 1.0, 100));
  broken.push_back(Strip());
  broken.push_back(Strip(1, 0x7f));
  broken.push_back(Strip(300, 0xff));
  std::vector<Strip> full(255, encode(8 * 8, 1.0, 0));
  for (int S : sizes) {
    for (int up = 1; up <= 2; ++up) {
      for (int g : {1, 2, 3, 7}) bad |= run_case("mixed ", mixed, 48, 64, up, g, S);
      bad |= run_case("broken", broken, 48, 64, up, 5, S);
      bad |= run_case("full  ", full, 8, 8, up, 255, S);
    }
    // every frame alone, from an allocation of exactly its own bytes
    for (size_t f = 0; f < broken.size(); ++f)
      bad |= run_case("alone ", std::vector<Strip>(1, broken[f]), 48, 64, 2, 1, S);
  }
  // a detector narrower than a word at upsampling 2 (2 w = 4) and one odd-sized frame of many segments
  bad |= run_case("narrow", std::vector<Strip>(3, encode(37 * 2, 0.4, 0)), 37, 2, 2, 3, 64);
  bad |= run_case("long  ", std::vector<Strip>(2, encode(333 * 92, 0.25, 0)), 333, 92, 1, 2, 64);
  printf(bad ? "FAIL\n" : "OK\n");
  return bad;
}
