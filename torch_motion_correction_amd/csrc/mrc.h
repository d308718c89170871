// MRC2014 sample rows -> raw movie rows: the format rule and the per-thread bodies of mrc_decode.hip, written so that a
// host compiler takes them as well: tests/host_mrc.cpp runs the same bodies, one "thread" after the other, under the
// address and undefined-behaviour sanitizers.  Nothing here needs the HIP runtime.
//
// THE FORMAT RULE.  After the 1024-byte header and nsymbt bytes of extended header the file holds nz frames of ny
// rows; a row is nx samples of the mode's type, in the file's byte order, with no padding between rows:
//
//   mode 0    8-bit.  MRC2014 says signed; IMOD writes unsigned bytes and says so in the header (imodStamp
//             1146047817 with bit 0 of imodFlags clear).  Unsigned bytes are copied, signed ones widened to int16.
//   mode 1    int16                    copied (byte-swapped for a big-endian file)
//   mode 6    uint16                   the same bytes; the caller refuses samples of 32768 and more
//   mode 12   IEEE half                the same bytes
//   mode 2    float32                  copied (4-byte swap for a big-endian file)
//   mode 101  4-bit, two per byte      a row is (nx + 1) / 2 bytes; pixel 2k is the LOW nibble of byte k, pixel 2k + 1
//                                      the HIGH nibble; with odd nx the last high nibble of every row is padding
//
// The mode-101 layout follows the IMOD / MRC2014 format descriptions.  It has NOT been confirmed against a file
// written by IMOD, SerialEM or any MRC library: none was available where this was written.  tests/mrc_reference.py
// restates the same reading of those descriptions, so the tests pin this file to that reading, not to a program.
//
// THE ROW SPLIT.  The payload starts anywhere (nsymbt is arbitrary, mode-101 rows of odd nx have odd lengths), so a
// row is cut by the alignment of its SOURCE bytes: `head` elements up to the first 16-byte boundary, `units` aligned
// 16-byte units, `tail` elements after the last whole unit.  Thread 0 of a row does the head, thread 1 + k unit k,
// thread 1 + units the tail; head and tail read one byte at a time, so no byte outside the row is read, and a unit is
// 16 bytes of the row.  A row whose first byte is not aligned to its own sample size has no aligned unit at all:
// there thread k takes the elements of bytes 16k .. 16k + 15, a byte at a time.  Stores go where the sample index
// says: 16 (or 2 x 16) bytes per unit, at the alignment of the output's element type, which the device's unaligned
// global access serves.  In mode 101 with odd nx the row's last byte, half padding, is always a tail element, so a
// unit never writes the padding nibble.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRC_HD __host__ __device__ __forceinline__
#else
#define MRC_HD inline
#endif

namespace mrc {

// what a row's bytes become
enum Kind { COPY1 = 0, WIDEN = 1, COPY2 = 2, SWAP2 = 3, COPY4 = 4, SWAP4 = 5, NIBBLE = 6, KINDS = 7 };

// the kind of a (mode, swap, unsigned_bytes), -1 for a mode that is not decoded
MRC_HD int kind_of(int mode, int swap, int unsigned_bytes) {
  switch (mode) {
    case 0: return unsigned_bytes ? COPY1 : WIDEN;
    case 1: case 6: case 12: return swap ? SWAP2 : COPY2;
    case 2: return swap ? SWAP4 : COPY4;
    case 101: return NIBBLE;
    default: return -1;
  }
}
// bytes of a source element (mode 101: the byte that holds two pixels) and of an output element
MRC_HD int in_bytes(int kind) { return kind >= COPY4 && kind != NIBBLE ? 4 : kind >= COPY2 && kind != NIBBLE ? 2 : 1; }
MRC_HD int out_bytes(int kind) { return kind == WIDEN ? 2 : kind == NIBBLE ? 1 : in_bytes(kind); }
MRC_HD long long row_bytes(int kind, int w) { return kind == NIBBLE ? ((long long)w + 1) / 2 : (long long)w * in_bytes(kind); }

// the row of a frame that output row r is read from
MRC_HD int source_row(int r, int h, int flip_rows) { return flip_rows ? h - 1 - r : r; }

struct U16 {
  uint32_t v[4];
};

MRC_HD U16 load16(const unsigned char* p) {  // p is 16-byte aligned
  U16 u;
  __builtin_memcpy(&u, __builtin_assume_aligned(p, 16), 16);
  return u;
}
MRC_HD void store16(unsigned char* p, const U16& u) { __builtin_memcpy(p, &u, 16); }  // any alignment

MRC_HD uint32_t swap2(uint32_t x) { return ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8); }
MRC_HD uint32_t swap4(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// 4 bytes = 8 pixels -> 8 bytes: low nibble first
MRC_HD void unpack_word(uint32_t x, uint32_t* a, uint32_t* b) {
  const uint32_t lo = x & 0x0f0f0f0fu, hi = (x >> 4) & 0x0f0f0f0fu;
  *a = (lo & 0xffu) | ((hi & 0xffu) << 8) | ((lo & 0xff00u) << 8) | ((hi & 0xff00u) << 16);
  *b = ((lo >> 16) & 0xffu) | (((hi >> 16) & 0xffu) << 8) | ((lo >> 24) << 16) | ((hi >> 24) << 24);
}
// one 16-byte unit of 32 nibbles -> 2 x 16 bytes
MRC_HD void unpack_nibbles(const U16& in, U16* first, U16* second) {
  unpack_word(in.v[0], &first->v[0], &first->v[1]);
  unpack_word(in.v[1], &first->v[2], &first->v[3]);
  unpack_word(in.v[2], &second->v[0], &second->v[1]);
  unpack_word(in.v[3], &second->v[2], &second->v[3]);
}
// 4 signed bytes -> 4 int16
MRC_HD void widen_word(uint32_t x, uint32_t* a, uint32_t* b) {
  const uint32_t s0 = (uint16_t)(int16_t)(int8_t)(x & 0xffu), s1 = (uint16_t)(int16_t)(int8_t)((x >> 8) & 0xffu);
  const uint32_t s2 = (uint16_t)(int16_t)(int8_t)((x >> 16) & 0xffu), s3 = (uint16_t)(int16_t)(int8_t)(x >> 24);
  *a = s0 | (s1 << 16);
  *b = s2 | (s3 << 16);
}
MRC_HD void widen_bytes(const U16& in, U16* first, U16* second) {
  widen_word(in.v[0], &first->v[0], &first->v[1]);
  widen_word(in.v[1], &first->v[2], &first->v[3]);
  widen_word(in.v[2], &second->v[0], &second->v[1]);
  widen_word(in.v[3], &second->v[2], &second->v[3]);
}

struct Split {
  int head, units, tail;  // source elements, 16-byte units, source elements
};

// the split of a row of `w` samples whose first byte has address `src`, a multiple of the sample size
template <int KIND>
MRC_HD Split split_row(uintptr_t src, int w) {
  constexpr int E = KIND == NIBBLE ? 1 : (KIND >= COPY4 ? 4 : KIND >= COPY2 ? 2 : 1);
  const int n = KIND == NIBBLE ? w / 2 : w;  // elements that may go through a unit
  Split s;
  const int to_boundary = (int)((16 - src % 16) % 16) / E;
  s.head = to_boundary < n ? to_boundary : n;
  s.units = (int)(((long long)(n - s.head) * E) / 16);
  s.tail = n - s.head - s.units * (16 / E) + (KIND == NIBBLE ? (w & 1) : 0);
  return s;
}

// source element i of a row, read one byte at a time, stored as the output's element(s)
template <int KIND>
MRC_HD void element(const unsigned char* src, unsigned char* dst, int w, int i) {
  if (KIND == COPY1) {
    dst[i] = src[i];
  } else if (KIND == WIDEN) {
    const int16_t v = (int16_t)(int8_t)src[i];
    __builtin_memcpy(dst + 2 * (long long)i, &v, 2);
  } else if (KIND == COPY2 || KIND == SWAP2) {
    const unsigned char a = src[2 * (long long)i], b = src[2 * (long long)i + 1];
    const uint16_t v = KIND == SWAP2 ? (uint16_t)((a << 8) | b) : (uint16_t)((b << 8) | a);
    __builtin_memcpy(dst + 2 * (long long)i, &v, 2);
  } else if (KIND == COPY4 || KIND == SWAP4) {
    const unsigned char* p = src + 4 * (long long)i;
    const uint32_t le = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    const uint32_t v = KIND == SWAP4 ? swap4(le) : le;
    __builtin_memcpy(dst + 4 * (long long)i, &v, 4);
  } else {  // NIBBLE: byte i holds pixels 2i and 2i + 1; the latter is padding when it is pixel w
    const unsigned char b = src[i];
    dst[2 * (long long)i] = b & 15;
    if (2 * (long long)i + 1 < w) dst[2 * (long long)i + 1] = b >> 4;
  }
}

// one aligned 16-byte unit that starts at source element e0
template <int KIND>
MRC_HD void unit(const unsigned char* src, unsigned char* dst, int e0) {
  constexpr int E = KIND == NIBBLE ? 1 : (KIND >= COPY4 ? 4 : KIND >= COPY2 ? 2 : 1);
  U16 in = load16(src + (long long)e0 * E);
  if (KIND == NIBBLE || KIND == WIDEN) {
    U16 a, b;
    if (KIND == NIBBLE) unpack_nibbles(in, &a, &b);
    else widen_bytes(in, &a, &b);
    store16(dst + 2 * (long long)e0, a);
    store16(dst + 2 * (long long)e0 + 16, b);
  } else {
    if (KIND == SWAP2) for (int k = 0; k < 4; ++k) in.v[k] = swap2(in.v[k]);
    if (KIND == SWAP4) for (int k = 0; k < 4; ++k) in.v[k] = swap4(in.v[k]);
    store16(dst + (long long)e0 * E, in);
  }
}

// threads a row needs: the head, every unit, the tail.  A bound from w alone, whatever the row's alignment
template <int KIND>
MRC_HD int row_threads(int w) {
  return (int)(row_bytes(KIND, w) / 16) + 2;
}

// what thread `u` of a row does: `src` the row's first source byte, `dst` its first output byte
template <int KIND>
MRC_HD void row_thread(const unsigned char* src, unsigned char* dst, int w, int u) {
  constexpr int E = KIND == NIBBLE ? 1 : (KIND >= COPY4 ? 4 : KIND >= COPY2 ? 2 : 1);
  if ((uintptr_t)src % E) {  // no aligned unit in this row: 16 bytes' worth of elements per thread, a byte at a time
    const long long first = (long long)u * (16 / E);
    for (int i = 0; i < 16 / E && first + i < w; ++i) element<KIND>(src, dst, w, (int)(first + i));
    return;
  }
  const Split s = split_row<KIND>((uintptr_t)src, w);
  if (u == 0) {
    for (int i = 0; i < s.head; ++i) element<KIND>(src, dst, w, i);
  } else if (u <= s.units) {
    unit<KIND>(src, dst, s.head + (u - 1) * (16 / E));
  } else if (u == s.units + 1) {
    const int first = s.head + s.units * (16 / E);
    for (int i = 0; i < s.tail; ++i) element<KIND>(src, dst, w, first + i);
  }
}

}  // namespace mrc
