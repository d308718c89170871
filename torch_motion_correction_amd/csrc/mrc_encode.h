// Raw movie rows -> MRC2014 sample rows: the inverse of mrc.h for the integer types.  The format rule, the per-thread
// bodies of mrc_encode.hip and the statistics they gather, written so that a host compiler takes them as well:
// tests/host_mrc_encode.cpp runs the same bodies, one "thread" after the other, under the address and
// undefined-behaviour sanitizers.  Nothing here needs the HIP runtime.
//
// THE FORMAT RULE.  The payload is t * h rows, one after the other with no padding, little-endian:
//
//   movie   mode   file sample                                           accepted values
//   uint8   0      the byte (the caller marks the file unsigned in IMOD's way)   all
//   uint8   101    4-bit                                                 0 .. 15
//   int16   1      the two bytes                                         all
//   int16   6      the same two bytes (uint16)                           0 .. 32767
//   int16   0      one signed byte (the MRC2014 rule)                    -128 .. 127
//   int16   101    4-bit                                                 0 .. 15
//
// Mode 101: a row is (w + 1) / 2 bytes; pixel 2k is the LOW nibble of byte k, pixel 2k + 1 the HIGH nibble; with odd
// w the last high nibble of every row is written as 0.  This is the reading of the IMOD / MRC2014 format descriptions
// that mrc.h decodes by.  It has NOT been confirmed against a file written by IMOD, SerialEM or any MRC library: none
// was available where this was written.  tests/mrc_encode_reference.py restates the same reading.
//
// A sample outside its mode's range is COUNTED, never wrapped into a neighbour's bits: the byte or nibble written for
// it is the value's low bits masked to the field, and the caller refuses a movie whose count is not 0.
// flip_rows: row r of every payload frame is row h - 1 - r of the movie's frame (the inverse of the decoder's).
//
// THE ROW SPLIT.  An ELEMENT is what becomes whole payload bytes: one sample, or in mode 101 a pair of pixels (one
// byte).  So every payload byte has one owner, and no body reads a payload byte.  As in mrc.h a row is cut by the
// alignment of its SOURCE bytes: `head` elements up to the first 16-byte boundary, `units` aligned 16-byte units,
// `tail` elements after the last whole unit (in mode 101 with odd w the lone last pixel is a tail element).  Thread 0
// of a row does the head, thread 1 + k unit k, thread 1 + units the tail; head and tail read one sample at a time, so
// no byte outside the row is read.  A unit stores 16, 8 or 4 bytes where the element index says, at any alignment,
// which the device's unaligned global access serves.  A row whose first byte is not aligned to its element (odd w:
// uint8 pairs at odd addresses, int16 pairs at 2 mod 4) has no aligned unit: there thread k takes the elements of
// source bytes 16k .. 16k + 15, a sample at a time.
//
// THE STATISTICS.  Every body adds the samples it READS to a Stats: minimum, maximum, sum, sum of squares, and the
// count of samples outside the mode's range, exact in 64-bit integers (a frame has fewer than 2^31 samples of at most
// 2^30 squared).  mrc_encode.hip sums a workgroup's threads and leaves one partial of 5 x int64 per workgroup in
// scratch; a finishing kernel sums a frame's partials in a fixed order.
//
// THE SCRATCH RULE.  blocks_per_frame(elem_bytes, h, w) workgroups of WG threads share a frame's h * row_threads
// row-threads, at most MAX_BLOCKS of them; scratch holds t * blocks_per_frame partials: scratch_bytes().
#pragma once
#include <stdint.h>

#include "mrc.h"

namespace mrcenc {

using mrc::U16;

enum Kind { U8_COPY = 0, U8_NIBBLE = 1, I16_COPY = 2, I16_U16 = 3, I16_BYTE = 4, I16_NIBBLE = 5, KINDS = 6 };

constexpr int WG = 256;          // threads of a workgroup
constexpr int MAX_BLOCKS = 1024;  // workgroups per frame, at most
constexpr int STATS = 5;         // min, max, sum, sum of squares, samples out of range

// the kind of (bytes of a movie element, mode), -1 for a pair outside the table
MRC_HD int kind_of(int elem_bytes, int mode) {
  if (elem_bytes == 1) return mode == 0 ? U8_COPY : mode == 101 ? U8_NIBBLE : -1;
  if (elem_bytes == 2) return mode == 1 ? I16_COPY : mode == 6 ? I16_U16 : mode == 0 ? I16_BYTE : mode == 101 ? I16_NIBBLE : -1;
  return -1;
}
MRC_HD constexpr int sample_bytes(int kind) { return kind <= U8_NIBBLE ? 1 : 2; }
MRC_HD constexpr bool nibbles(int kind) { return kind == U8_NIBBLE || kind == I16_NIBBLE; }
// source bytes and payload bytes of an element
MRC_HD constexpr int elem_in(int kind) { return sample_bytes(kind) * (nibbles(kind) ? 2 : 1); }
MRC_HD constexpr int elem_out(int kind) { return kind == I16_COPY || kind == I16_U16 ? 2 : 1; }
MRC_HD long long row_bytes(int kind, int w) { return nibbles(kind) ? ((long long)w + 1) / 2 : (long long)w * elem_out(kind); }

// threads a row needs: the head, every unit, the tail.  A bound from w alone, whatever the row's alignment
MRC_HD int row_threads(int elem_bytes, int w) { return (int)(((long long)w * elem_bytes) / 16) + 2; }
MRC_HD int blocks_per_frame(int elem_bytes, int h, int w) {
  const long long blocks = ((long long)h * row_threads(elem_bytes, w) + WG - 1) / WG;
  return (int)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}
MRC_HD long long scratch_bytes(int elem_bytes, int t, int h, int w) {
  return (long long)t * blocks_per_frame(elem_bytes, h, w) * STATS * 8;
}

struct Stats {
  int mn, mx;  // of the samples read so far; 32768 / -32769 before the first
  long long sum, sq, bad;
};
MRC_HD Stats no_stats() { return Stats{32768, -32769, 0, 0, 0}; }
MRC_HD void merge(Stats& a, const Stats& b) {
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  a.sum += b.sum;
  a.sq += b.sq;
  a.bad += b.bad;
}

template <int KIND>
MRC_HD bool out_of_range(int v) {
  return KIND == U8_NIBBLE || KIND == I16_NIBBLE ? (v & ~15) != 0
         : KIND == I16_U16                         ? v < 0
         : KIND == I16_BYTE                        ? v < -128 || v > 127
                                                   : false;
}
template <int KIND>
MRC_HD void count(Stats& s, int v) {
  s.mn = v < s.mn ? v : s.mn;
  s.mx = v > s.mx ? v : s.mx;
  s.sum += v;
  s.sq += (long long)(v * v);  // |v| <= 32768: the square fits 31 bits
  s.bad += out_of_range<KIND>(v);
}

// sample i of a row, read one byte (uint8) or one aligned int16 at a time
template <int KIND>
MRC_HD int sample(const unsigned char* src, long long i) {
  if (sample_bytes(KIND) == 1) return src[i];
  int16_t v;
  __builtin_memcpy(&v, __builtin_assume_aligned(src + 2 * i, 2), 2);
  return v;
}

// element i of a row: its samples read one at a time and counted, its payload byte(s) stored
template <int KIND>
MRC_HD void element(const unsigned char* src, unsigned char* dst, int w, int i, Stats& s) {
  if (nibbles(KIND)) {  // pixels 2i and 2i + 1; the latter does not exist when it is pixel w: its nibble is 0
    const int a = sample<KIND>(src, 2 * (long long)i);
    count<KIND>(s, a);
    int b = 0;
    if (2 * (long long)i + 1 < w) {
      b = sample<KIND>(src, 2 * (long long)i + 1);
      count<KIND>(s, b);
    }
    dst[i] = (unsigned char)((a & 15) | ((b & 15) << 4));
  } else {
    const int v = sample<KIND>(src, i);
    count<KIND>(s, v);
    if (elem_out(KIND) == 1) {
      dst[i] = (unsigned char)(v & 255);
    } else {
      dst[2 * (long long)i] = (unsigned char)(v & 255);
      dst[2 * (long long)i + 1] = (unsigned char)((v >> 8) & 255);
    }
  }
}

// 4 pixels in the bytes of x -> 2 payload bytes
MRC_HD uint32_t pack_bytes(uint32_t x) {
  const uint32_t lo = x & 0x0f0f0f0fu;
  return (lo & 0xfu) | ((lo >> 4) & 0xf0u) | ((lo >> 8) & 0xf00u) | ((lo >> 12) & 0xf000u);
}

// one aligned 16-byte unit that starts at element e0: counted, stored
template <int KIND>
MRC_HD void unit(const unsigned char* src, unsigned char* dst, int e0, Stats& s) {
  const U16 in = mrc::load16(src + (long long)e0 * elem_in(KIND));
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = in.v[k];
    if (sample_bytes(KIND) == 1) {
      for (int j = 0; j < 4; ++j) count<KIND>(s, (int)((x >> (8 * j)) & 255u));
    } else {
      count<KIND>(s, (int16_t)(x & 0xffffu));
      count<KIND>(s, (int16_t)(x >> 16));
    }
  }
  unsigned char* out = dst + (long long)e0 * elem_out(KIND);
  if (KIND == U8_COPY || KIND == I16_COPY || KIND == I16_U16) {
    mrc::store16(out, in);
  } else if (KIND == U8_NIBBLE) {  // 16 pixels -> 8 bytes
    const uint32_t o[2] = {pack_bytes(in.v[0]) | (pack_bytes(in.v[1]) << 16), pack_bytes(in.v[2]) | (pack_bytes(in.v[3]) << 16)};
    __builtin_memcpy(out, o, 8);
  } else if (KIND == I16_BYTE) {  // 8 samples -> 8 bytes
    uint32_t o[2];
    for (int k = 0; k < 2; ++k)
      o[k] = (in.v[2 * k] & 0xffu) | ((in.v[2 * k] >> 8) & 0xff00u) | ((in.v[2 * k + 1] & 0xffu) << 16) |
             ((in.v[2 * k + 1] << 8) & 0xff000000u);
    __builtin_memcpy(out, o, 8);
  } else {  // I16_NIBBLE: 8 pixels -> 4 bytes
    uint32_t o = 0;
    for (int k = 0; k < 4; ++k) o |= ((in.v[k] & 15u) | ((in.v[k] >> 12) & 0xf0u)) << (8 * k);
    __builtin_memcpy(out, &o, 4);
  }
}

struct Split {
  int head, units, tail;  // elements, 16-byte units, elements
};

// the split of a row of `w` samples whose first byte has address `src`, a multiple of the element's source size
template <int KIND>
MRC_HD Split split_row(uintptr_t src, int w) {
  constexpr int E = elem_in(KIND);
  const int n = nibbles(KIND) ? w / 2 : w;  // elements that may go through a unit
  Split s;
  const int to_boundary = (int)((16 - src % 16) % 16) / E;
  s.head = to_boundary < n ? to_boundary : n;
  s.units = (int)(((long long)(n - s.head) * E) / 16);
  s.tail = n - s.head - s.units * (16 / E) + (nibbles(KIND) ? (w & 1) : 0);
  return s;
}

// what thread `u` of a row does: `src` the row's first movie byte, `dst` its first payload byte
template <int KIND>
MRC_HD void row_thread(const unsigned char* src, unsigned char* dst, int w, int u, Stats& s) {
  constexpr int E = elem_in(KIND);
  if ((uintptr_t)src % E) {  // no aligned unit in this row: 16 bytes' worth of elements per thread, a sample at a time
    const long long n = nibbles(KIND) ? ((long long)w + 1) / 2 : w, first = (long long)u * (16 / E);
    for (int i = 0; i < 16 / E && first + i < n; ++i) element<KIND>(src, dst, w, (int)(first + i), s);
    return;
  }
  const Split sp = split_row<KIND>((uintptr_t)src, w);
  if (u == 0) {
    for (int i = 0; i < sp.head; ++i) element<KIND>(src, dst, w, i, s);
  } else if (u <= sp.units) {
    unit<KIND>(src, dst, sp.head + (u - 1) * (16 / E), s);
  } else if (u == sp.units + 1) {
    const int first = sp.head + sp.units * (16 / E);
    for (int i = 0; i < sp.tail; ++i) element<KIND>(src, dst, w, first + i, s);
  }
}

// row-thread `item` of a frame (item = payload row * row_threads + thread of the row): `frame` the frame's first
// movie byte, `out` its first payload byte
template <int KIND>
MRC_HD void frame_item(const unsigned char* frame, unsigned char* out, int h, int w, int flip_rows, long long item, Stats& s) {
  const int rt = row_threads(sample_bytes(KIND), w);
  const int r = (int)(item / rt), u = (int)(item % rt);
  row_thread<KIND>(frame + (long long)mrc::source_row(r, h, flip_rows) * w * sample_bytes(KIND),
                   out + (long long)r * row_bytes(KIND, w), w, u, s);
}

}  // namespace mrcenc
