// CPU run of the MRC encode's per-thread bodies (csrc/mrc_encode.h, the source mrc_encode.hip compiles for the
// device): every frame of a movie is run row-thread by row-thread exactly as the kernel's grid runs it -- the head,
// every aligned 16-byte unit, the tail of each row -- on movie and payload buffers allocated to their exact sizes, and
// the threads' statistics are merged as the kernels merge them.  Meant to be built with the address and
// undefined-behaviour sanitizers, which then see every load of the movie and every store of the payload:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_mrc_encode.cpp -o host_mrc_encode && ./host_mrc_encode cases.bin
//
// cases.bin (written by tests/test_mrc_encode_host.py) is a list of records, little-endian u32 fields:
//   elem_bytes, mode, flip_rows, t, h, w, lead_in, lead_out, movie_len, want_len,
//   then movie_len bytes of the movie, want_len bytes of the expected payload and t x 5 int64 of expected statistics.
// The movie is placed lead_in bytes (a multiple of elem_bytes) into an allocation of lead_in + movie_len bytes, the
// payload is written lead_out bytes into one of lead_out + want_len bytes; both leads are poisoned, so rows start at
// any alignment and a byte read or written before a buffer is a report, as one behind it is.
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mrc_encode.h"

template <int KIND>
static void run(const unsigned char* movie, int t, int h, int w, int flip_rows, unsigned char* payload, long long* table) {
  const long long items = (long long)h * mrcenc::row_threads(mrcenc::sample_bytes(KIND), w);
  for (int f = 0; f < t; ++f) {
    const unsigned char* frame = movie + (long long)f * h * w * mrcenc::sample_bytes(KIND);
    unsigned char* out = payload + (long long)f * h * mrcenc::row_bytes(KIND, w);
    mrcenc::Stats all = mrcenc::no_stats();
    for (long long i = 0; i < items; ++i) {  // one thread after the other, each with statistics of its own
      mrcenc::Stats s = mrcenc::no_stats();
      mrcenc::frame_item<KIND>(frame, out, h, w, flip_rows, i, s);
      mrcenc::merge(all, s);
    }
    const long long row[mrcenc::STATS] = {all.mn, all.mx, all.sum, all.sq, all.bad};
    memcpy(table + (long long)f * mrcenc::STATS, row, sizeof row);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: host_mrc_encode cases.bin\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  unsigned hdr[10];
  int cases = 0, failures = 0;
  while (fread(hdr, 4, 10, fh) == 10) {
    const int elem = (int)hdr[0], mode = (int)hdr[1], flip = (int)hdr[2], t = (int)hdr[3], h = (int)hdr[4], w = (int)hdr[5];
    const unsigned lead_in = hdr[6], lead_out = hdr[7], movie_len = hdr[8], want_len = hdr[9];
    const int kind = mrcenc::kind_of(elem, mode);
    if (kind < 0) return 2;
    if ((long long)t * h * w * elem != movie_len || (long long)t * h * mrcenc::row_bytes(kind, w) != want_len ||
        lead_in % elem)
      return 2;
    // the scratch rule covers the kernel's grid: as many partials as workgroups
    if (mrcenc::scratch_bytes(elem, t, h, w) != (long long)t * mrcenc::blocks_per_frame(elem, h, w) * 40) return 2;
    unsigned char* movie = new unsigned char[lead_in + movie_len];
    unsigned char* want = new unsigned char[want_len];
    unsigned char* out = new unsigned char[lead_out + want_len];
    long long* want_table = new long long[t * mrcenc::STATS];
    long long* table = new long long[t * mrcenc::STATS];
    if (fread(movie + lead_in, 1, movie_len, fh) != movie_len || fread(want, 1, want_len, fh) != want_len ||
        fread(want_table, 8, t * mrcenc::STATS, fh) != (size_t)t * mrcenc::STATS)
      return 2;
    memset(out + lead_out, 0xA5, want_len);
    if (lead_in) __asan_poison_memory_region(movie, lead_in);
    if (lead_out) __asan_poison_memory_region(out, lead_out);
    switch (kind) {
      case mrcenc::U8_COPY: run<mrcenc::U8_COPY>(movie + lead_in, t, h, w, flip, out + lead_out, table); break;
      case mrcenc::U8_NIBBLE: run<mrcenc::U8_NIBBLE>(movie + lead_in, t, h, w, flip, out + lead_out, table); break;
      case mrcenc::I16_COPY: run<mrcenc::I16_COPY>(movie + lead_in, t, h, w, flip, out + lead_out, table); break;
      case mrcenc::I16_U16: run<mrcenc::I16_U16>(movie + lead_in, t, h, w, flip, out + lead_out, table); break;
      case mrcenc::I16_BYTE: run<mrcenc::I16_BYTE>(movie + lead_in, t, h, w, flip, out + lead_out, table); break;
      default: run<mrcenc::I16_NIBBLE>(movie + lead_in, t, h, w, flip, out + lead_out, table); break;
    }
    ++cases;
    const bool bytes_ok = memcmp(out + lead_out, want, want_len) == 0;
    const bool table_ok = memcmp(table, want_table, sizeof(long long) * t * mrcenc::STATS) == 0;
    if (!bytes_ok || !table_ok) {
      ++failures;
      printf("case %d (elem %d mode %d flip %d, %d x %d x %d, leads %u %u): FAIL%s%s\n", cases - 1, elem, mode, flip, t,
             h, w, lead_in, lead_out, bytes_ok ? "" : " payload", table_ok ? "" : " statistics");
    }
    if (lead_in) __asan_unpoison_memory_region(movie, lead_in);
    if (lead_out) __asan_unpoison_memory_region(out, lead_out);
    delete[] movie;
    delete[] want;
    delete[] out;
    delete[] want_table;
    delete[] table;
  }
  fclose(fh);
  printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
