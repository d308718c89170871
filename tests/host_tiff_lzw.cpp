// CPU run of the TIFF LZW decode's per-strip loop (csrc/tiff_lzw.h, the source tiff_decode.hip compiles for the
// device): the state machine as the kernel runs it, with a serial form of the wavefront's copy, on input, output and
// table buffers allocated to their exact sizes.  Meant to be built with the address and undefined-behaviour
// sanitizers, which then see every load of a stream, every table access and every store of the output:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_tiff_lzw.cpp -o host_tiff_lzw && ./host_tiff_lzw cases.bin
//
// cases.bin (written by tests/test_tiff_host.py) is a list of records, little-endian u32 fields:
//   kind, nbytes, expected, want_len, then nbytes of stream and want_len of expected output
//   kind 0  the strip decodes to exactly `want`
//   kind 1  as 0, and the strip cut to every shorter length decodes to a prefix of `want`
// Cases made here: garbage streams, the empty and every one-byte stream, strips whose data would overrun the expected
// size (every kind 0 / 1 strip decoded again into fewer bytes than it holds), and stored strips.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tiff_lzw.h"

static int failures = 0, cases = 0;

static unsigned rng_state = 2463534242u;
static unsigned rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// the strip decoded into an allocation of exactly `expected` bytes, from an allocation of exactly `nbytes`
static int decode(const unsigned char* stream, long long nbytes, int expected, unsigned char** result) {
  unsigned char* in = new unsigned char[nbytes];
  if (nbytes) memcpy(in, stream, (size_t)nbytes);
  unsigned char* out = new unsigned char[expected];
  unsigned* tab_start = new unsigned[tiff_lzw::TABLE];
  unsigned short* tab_len = new unsigned short[tiff_lzw::TABLE];
  const int n = tiff_lzw::decode_strip(in, nbytes, expected, tab_start, tab_len, true,
                                       [&](const tiff_lzw::Piece& p, int cursor, int len) {
                                         if (p.literal >= 0) {
                                           out[cursor] = (unsigned char)p.literal;
                                           return;
                                         }
                                         // lanes 0 .. 63 of each step in turn: all loads of a step, then its stores
                                         for (int base = 0; base < len; base += 64) {
                                           unsigned char v[64];
                                           const int m = len - base < 64 ? len - base : 64;
                                           for (int l = 0; l < m; ++l) v[l] = out[tiff_lzw::copy_index(p, base + l)];
                                           for (int l = 0; l < m; ++l) out[cursor + base + l] = v[l];
                                         }
                                       });
  delete[] tab_start;
  delete[] tab_len;
  delete[] in;
  *result = out;
  return n;
}

static void report(const char* what, bool ok) {
  ++cases;
  if (!ok) {
    ++failures;
    printf("%s: FAIL\n", what);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: host_tiff_lzw cases.bin\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  unsigned hdr[4];
  int record = 0;
  while (fread(hdr, 4, 4, fh) == 4) {
    const unsigned kind = hdr[0], nbytes = hdr[1], expected = hdr[2], want_len = hdr[3];
    unsigned char* stream = new unsigned char[nbytes];
    unsigned char* want = new unsigned char[want_len];
    if ((nbytes && fread(stream, 1, nbytes, fh) != nbytes) || (want_len && fread(want, 1, want_len, fh) != want_len))
      return 2;
    char what[64];
    snprintf(what, sizeof what, "record %d", record++);
    unsigned char* got;
    int n = decode(stream, nbytes, (int)expected, &got);
    report(what, n == (int)want_len && memcmp(got, want, want_len) == 0);
    delete[] got;
    // the same data into fewer bytes than it holds: clipped, never overrun
    const unsigned fewer[4] = {0u, 1u, want_len / 2, want_len - 1};
    for (unsigned less : fewer) {
      if (less >= want_len) continue;
      n = decode(stream, nbytes, (int)less, &got);
      report(what, n == (int)less && memcmp(got, want, less) == 0);
      delete[] got;
    }
    if (kind == 1)
      for (unsigned cut = 0; cut < nbytes; ++cut) {
        n = decode(stream, cut, (int)expected, &got);
        report(what, n <= (int)want_len && memcmp(got, want, (size_t)n) == 0);
        delete[] got;
      }
    delete[] stream;
    delete[] want;
  }
  fclose(fh);
  // garbage: any bits at all stay inside the strip and its rows
  for (int k = 0; k < 400; ++k) {
    const unsigned nbytes = k < 40 ? (unsigned)k : rng() % 3000, expected = rng() % 5000;
    unsigned char* stream = new unsigned char[nbytes];
    for (unsigned i = 0; i < nbytes; ++i) stream[i] = (unsigned char)(k % 3 == 0 ? rng() % 3 : rng());
    if (nbytes >= 2 && k % 2) stream[0] = 0x80, stream[1] &= 0x7f;  // begins with Clear, as real strips do
    unsigned char* got;
    const int n = decode(stream, nbytes, (int)expected, &got);
    report("garbage", n >= 0 && n <= (int)expected);
    delete[] got;
    delete[] stream;
  }
  for (int b = -1; b < 256; ++b) {  // the empty stream and every one-byte stream: fewer than 9 bits
    unsigned char byte = (unsigned char)b, *got;
    const int n = decode(&byte, b < 0 ? 0 : 1, 16, &got);
    report("one byte", n == 0);
    delete[] got;
  }
  // stored strips: short, exact, long
  report("stored", tiff_lzw::stored_bytes(0, 10) == 0 && tiff_lzw::stored_bytes(7, 10) == 7 &&
                       tiff_lzw::stored_bytes(10, 10) == 10 && tiff_lzw::stored_bytes(1ll << 40, 10) == 10);
  printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
