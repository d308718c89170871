// CPU run of the MRC decode's per-thread bodies (csrc/mrc.h, the source mrc_decode.hip compiles for the device): every
// row of a movie is run "thread" by thread exactly as the kernel's grid runs it -- the head, every aligned 16-byte
// unit, the tail -- on input and output buffers allocated to their exact sizes.  Meant to be built with the address
// and undefined-behaviour sanitizers, which then see every load of the payload and every store of the movie:
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I torch_motion_correction_amd/csrc tests/host_mrc.cpp -o host_mrc && ./host_mrc cases.bin
//
// cases.bin (written by tests/test_mrc_host.py) is a list of records, little-endian u32 fields:
//   mode, swap, unsigned_bytes, flip_rows, t, h, w, lead_in, lead_out, payload_len, want_len,
//   then payload_len bytes of samples and want_len bytes of the expected movie.
// The payload is placed lead_in bytes into an allocation of lead_in + payload_len bytes whose first lead_in bytes are
// poisoned (a file's header: the decoder must not read it), so the rows start at any alignment; the movie is written
// lead_out bytes into an allocation of lead_out + want_len bytes whose lead is poisoned as well.
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mrc.h"

template <int KIND>
static void run(const unsigned char* payload, int t, int h, int w, int flip_rows, unsigned char* out) {
  const long long in_row = mrc::row_bytes(KIND, w), out_row = (long long)w * mrc::out_bytes(KIND);
  const int threads = mrc::row_threads<KIND>(w);
  for (int f = 0; f < t; ++f)
    for (int r = 0; r < h; ++r) {
      const unsigned char* src = payload + ((long long)f * h + mrc::source_row(r, h, flip_rows)) * in_row;
      unsigned char* dst = out + ((long long)f * h + r) * out_row;
      // a grid rounded up to whole workgroups: the threads past the row's last must do nothing
      for (int u = 0; u < threads + 300; ++u) mrc::row_thread<KIND>(src, dst, w, u);
    }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: host_mrc cases.bin\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  unsigned hdr[11];
  int cases = 0, failures = 0;
  while (fread(hdr, 4, 11, fh) == 11) {
    const int mode = (int)hdr[0], swap = (int)hdr[1], ub = (int)hdr[2], flip = (int)hdr[3];
    const int t = (int)hdr[4], h = (int)hdr[5], w = (int)hdr[6];
    const unsigned lead_in = hdr[7], lead_out = hdr[8], payload_len = hdr[9], want_len = hdr[10];
    const int kind = mrc::kind_of(mode, swap, ub);
    if (kind < 0) return 2;
    if ((long long)t * h * mrc::row_bytes(kind, w) != payload_len ||
        (long long)t * h * w * mrc::out_bytes(kind) != want_len || lead_out % mrc::out_bytes(kind))
      return 2;
    unsigned char* in = new unsigned char[lead_in + payload_len];
    unsigned char* want = new unsigned char[want_len];
    unsigned char* out = new unsigned char[lead_out + want_len];
    if (fread(in + lead_in, 1, payload_len, fh) != payload_len || fread(want, 1, want_len, fh) != want_len) return 2;
    memset(out + lead_out, 0xA5, want_len);
    if (lead_in) __asan_poison_memory_region(in, lead_in);
    if (lead_out) __asan_poison_memory_region(out, lead_out);
    switch (kind) {
      case mrc::COPY1: run<mrc::COPY1>(in + lead_in, t, h, w, flip, out + lead_out); break;
      case mrc::WIDEN: run<mrc::WIDEN>(in + lead_in, t, h, w, flip, out + lead_out); break;
      case mrc::COPY2: run<mrc::COPY2>(in + lead_in, t, h, w, flip, out + lead_out); break;
      case mrc::SWAP2: run<mrc::SWAP2>(in + lead_in, t, h, w, flip, out + lead_out); break;
      case mrc::COPY4: run<mrc::COPY4>(in + lead_in, t, h, w, flip, out + lead_out); break;
      case mrc::SWAP4: run<mrc::SWAP4>(in + lead_in, t, h, w, flip, out + lead_out); break;
      default: run<mrc::NIBBLE>(in + lead_in, t, h, w, flip, out + lead_out); break;
    }
    ++cases;
    if (memcmp(out + lead_out, want, want_len) != 0) {
      ++failures;
      printf("case %d (mode %d swap %d unsigned %d flip %d, %d x %d x %d, leads %u %u): FAIL\n", cases - 1, mode, swap,
             ub, flip, t, h, w, lead_in, lead_out);
    }
    if (lead_in) __asan_unpoison_memory_region(in, lead_in);
    if (lead_out) __asan_unpoison_memory_region(out, lead_out);
    delete[] in;
    delete[] want;
    delete[] out;
  }
  fclose(fh);
  printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
