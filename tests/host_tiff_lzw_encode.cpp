// CPU run of the TIFF LZW encoder's per-strip loop (csrc/tiff_lzw_encode.h, the source tiff_encode.hip compiles for
// the device): the parse as the kernel runs it, with a serial form of the wavefront's steps -- the 64-slot probe and
// its two ballots, the chunked input, the 64 staged words -- on input, table and output buffers allocated to their
// exact sizes.  Meant to be built with the address and undefined-behaviour sanitizers, which then see every load of
// the input, every table access and every store of the stream:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_tiff_lzw_encode.cpp -o host_tiff_lzw_encode \
//       && ./host_tiff_lzw_encode cases.bin
//
// cases.bin (written by tests/test_tiff_encode_host.py) is a list of records, little-endian u32 fields:
//   n, want_len, then n bytes of input and want_len bytes of tests/tiff_reference.py::encode_strip(input)
// Every record is encoded into a poisoned slot of exactly slot_bytes(n) bytes (the stream equals `want`, the rest of
// the slot keeps its poison), into exactly want_len bytes, and into fewer bytes than the stream has (clipped, never
// overrun); the stream is decoded again with the decoder of csrc/tiff_lzw.h.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tiff_lzw_encode.h"

static int failures = 0, cases = 0;
static const unsigned char POISON = 0xa5;

struct HostWave {
  unsigned* tab;
  const unsigned char* src;
  unsigned char* out;
  long long cap;
  int n;
  unsigned window[64], stage[64];
  unsigned char cur[64], ahead[64];

  void load_chunk(long long first, unsigned char* to) const {  // n > 0
    for (int lane = 0; lane < 64; ++lane) {
      long long i = first + lane;
      if (i > n - 1) i = n - 1;
      to[lane] = src[i];
    }
  }
  void start() {
    if (n > 0) load_chunk(0, ahead);
  }
  void chunk(long long first) {
    memcpy(cur, ahead, 64);
    load_chunk(first + 64, ahead);
  }
  unsigned byte(int i) const { return cur[i & 63]; }
  void clear_table() {
    for (int k = 0; k < tiff_lzw::ENC_SLOTS; ++k) tab[k] = tiff_lzw::ENC_FREE;
  }
  void probe(int base, unsigned key, unsigned long long& match, unsigned long long& free) {
    match = free = 0;
    for (int lane = 0; lane < 64; ++lane) {
      window[lane] = tab[(base + lane) & (tiff_lzw::ENC_SLOTS - 1)];
      if ((window[lane] >> 12) == key) match |= 1ull << lane;
      if (window[lane] == tiff_lzw::ENC_FREE) free |= 1ull << lane;
    }
  }
  unsigned probed(int lane) const { return window[lane]; }
  void insert(int slot, unsigned entry) { tab[slot] = entry; }
  void store_words(long long first, int count) {
    for (int lane = 0; lane < count; ++lane) {
      const long long p = 4 * (first + lane);
      for (int k = 0; k < 4; ++k)
        if (p + k < cap) out[p + k] = (unsigned char)(stage[lane] >> (8 * k));
    }
  }
  void word(long long index, unsigned value) {
    stage[index & 63] = __builtin_bswap32(value);
    if ((index & 63) == 63) store_words(index - 63, 64);
  }
  void finish(long long words, unsigned last, int tail) {
    store_words(words & ~63ll, (int)(words & 63));
    for (int lane = 0; lane < tail; ++lane) {
      const long long p = 4 * words + lane;
      if (p < cap) out[p] = (unsigned char)(last >> (24 - 8 * lane));
    }
  }
};

// `n` bytes from an allocation of exactly n, encoded into a poisoned allocation of exactly `cap` -> the stream's
// length, unclipped
static long long encode(const unsigned char* data, int n, long long cap, unsigned char** result) {
  unsigned char* in = new unsigned char[n];
  if (n) memcpy(in, data, (size_t)n);
  unsigned char* out = new unsigned char[cap];
  if (cap) memset(out, POISON, (size_t)cap);
  unsigned* tab = new unsigned[tiff_lzw::ENC_SLOTS];
  HostWave wave = {tab, in, out, cap, n, {0}, {0}, {0}, {0}};
  wave.start();
  const long long bytes = tiff_lzw::encode_strip(n, wave);
  delete[] tab;
  delete[] in;
  *result = out;
  return bytes;
}

static bool round_trip(const unsigned char* stream, long long nbytes, const unsigned char* data, int n) {
  unsigned char* out = new unsigned char[n];
  unsigned* tab_start = new unsigned[tiff_lzw::TABLE];
  unsigned short* tab_len = new unsigned short[tiff_lzw::TABLE];
  const int got = tiff_lzw::decode_strip(stream, nbytes, n, tab_start, tab_len, true,
                                         [&](const tiff_lzw::Piece& p, int cursor, int len) {
                                           if (p.literal >= 0) {
                                             out[cursor] = (unsigned char)p.literal;
                                             return;
                                           }
                                           for (int i = 0; i < len; ++i) out[cursor + i] = out[tiff_lzw::copy_index(p, i)];
                                         });
  const bool ok = got == n && (n == 0 || memcmp(out, data, (size_t)n) == 0);
  delete[] tab_start;
  delete[] tab_len;
  delete[] out;
  return ok;
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
    fprintf(stderr, "usage: host_tiff_lzw_encode cases.bin\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  unsigned hdr[2];
  int record = 0;
  while (fread(hdr, 4, 2, fh) == 2) {
    const unsigned n = hdr[0], want_len = hdr[1];
    unsigned char* data = new unsigned char[n];
    unsigned char* want = new unsigned char[want_len];
    if ((n && fread(data, 1, n, fh) != n) || (want_len && fread(want, 1, want_len, fh) != want_len)) return 2;
    char what[64];
    snprintf(what, sizeof what, "record %d", record++);
    // the slot the kernel gives it
    const long long slot = tiff_lzw::slot_bytes(n);
    unsigned char* got;
    long long bytes = encode(data, (int)n, slot, &got);
    bool ok = bytes == (long long)want_len && bytes <= slot && memcmp(got, want, want_len) == 0;
    for (long long i = bytes; ok && i < slot; ++i) ok = got[i] == POISON;
    report(what, ok);
    report(what, ok && round_trip(got, bytes, data, (int)n));
    delete[] got;
    // exactly the stream's bytes, and fewer: clipped, never overrun
    const long long caps[4] = {(long long)want_len, (long long)want_len - 1, (long long)want_len / 2, 0};
    for (long long cap : caps) {
      bytes = encode(data, (int)n, cap, &got);
      report(what, bytes == (long long)want_len && memcmp(got, want, (size_t)cap) == 0);
      delete[] got;
    }
    delete[] data;
    delete[] want;
  }
  fclose(fh);
  // the bound, against the closed form derived in the header
  bool bound = true;
  for (long long n = 0; n < 200000 && bound; ++n) {
    const long long codes = n + n / 3835 + 2, bytes = (12 * codes + 7) / 8;
    bound = tiff_lzw::slot_bytes(n) >= bytes && tiff_lzw::slot_bytes(n) < bytes + 16 && tiff_lzw::slot_bytes(n) % 16 == 0;
  }
  report("slot_bytes", bound);
  printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
