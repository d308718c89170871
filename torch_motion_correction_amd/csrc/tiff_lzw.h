// TIFF 6.0 LZW (TIFF compression 5): the codec rule and the per-strip decode loop (tiff_decode.hip), written so that
// a host compiler takes them as well: tests/host_tiff_lzw.cpp runs the same loop with a serial copy under the address
// and undefined-behaviour sanitizers.  Nothing here needs the HIP runtime.
//
// THE CODEC RULE.  A strip is a stream of codes packed MSB-first: bit k of the stream is bit 7 - (k & 7) of byte
// k >> 3.  The decoder starts in the cleared state -- width = 9, next = 258, no previous code -- whether or not the
// stream begins with Clear.  For each code c, read with the current width:
//
//   c == 256 (Clear)   width = 9, next = 258, no previous code
//   c == 257 (EOI)     stop
//   no previous code   c < 256: the string is the byte c;  anything else is malformed: stop
//   c <  next          the string is the byte c (c < 256) or the table's entry c
//   c == next          KwKwK: the string is the previous string + the previous string's first byte
//   c >  next          malformed: stop
//   then, with a previous code and next < 4096:  entry `next` = previous string + first byte of c's string; next += 1;
//                      "early change": if next + 1 >= (1 << width) and width < 12, width += 1
//   the string is appended to the output (clipped to the strip's expected size) and c becomes the previous code
//
// Once next == 4096 nothing is added and decoding goes on at 12 bits (libtiff's encoder never gets there: it emits
// Clear first).  Decoding stops at the first of: EOI; the expected byte count reached; fewer than `width` bits left
// in the strip; a malformed code.  Bytes after the expected count are ignored.  Old-style (LSB-first) LZW is not
// recognised and ends as a malformed strip.  step() and read_code() are the only statement of this rule in the
// library; tests/tiff_reference.py restates it with Python integers.
//
// THE TABLE holds no string bytes.  The string of a code is always a contiguous piece of output this strip has
// already produced -- the new entry is (where the previous code's string was written, its length + 1) -- so an
// entry is (start in the strip's output, length): 4096 x (u32 + u16) = 24 KB.  Lengths grow by one per entry and a
// table has at most 3838 entries, so a length fits 16 bits.  In the KwKwK case the string's last byte is the one
// byte of it that is not written yet; it equals the string's first byte, and copy_index() says so explicitly.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZW_HD __host__ __device__ __forceinline__
#else
#define LZW_HD inline
#endif

namespace tiff_lzw {

constexpr int CLEAR = 256, EOI = 257, FIRST = 258, TABLE = 4096, MIN_WIDTH = 9, MAX_WIDTH = 12;
enum { EMIT = 0, CLEARED = 1, STOP_EOI = 2, STOP_MALFORMED = 3 };

struct State {
  int width, next;
  int prev_start, prev_len;  // where the previous code's string was written; prev_len == 0: no previous code
};

// the string of one code: a byte (literal >= 0) or `len` bytes of earlier output from `start`; kwkwk: byte len - 1
// of it is not written yet and equals byte 0
struct Piece {
  int start, len, literal;
  bool kwkwk;
};

LZW_HD void reset(State& st) {
  st.width = MIN_WIDTH;
  st.next = FIRST;
  st.prev_start = 0;
  st.prev_len = 0;
}

// the `width` bits at bit `bit` >= 0 of the strip; the caller has checked bit + width <= 8 * nbytes.  A code spans
// up to three bytes: the three loads are unconditional (one wait for all of them), each index clamped to the strip's
// last byte, so no byte at or beyond nbytes is read whatever the caller passes; a clamped byte lies below the code's
// bits and is shifted out.
LZW_HD unsigned read_code(const unsigned char* s, long long nbytes, long long bit, int width) {
  if (nbytes <= 0) return 0u;
  const long long last = nbytes - 1, b = bit >> 3;
  const long long b0 = b < last ? b : last, b1 = b + 1 < last ? b + 1 : last, b2 = b + 2 < last ? b + 2 : last;
  const unsigned v = (unsigned)s[b0] << 16 | (unsigned)s[b1] << 8 | (unsigned)s[b2];
  return (v >> (24 - (int)(bit & 7) - width)) & ((1u << width) - 1u);
}

// One code of the rule with `cursor` bytes of output written so far: the state and the table move on, `p` is the
// string to append at `cursor`.  Only the caller with `writer` stores the new entry (one lane of a wavefront).
LZW_HD int step(State& st, unsigned c, int cursor, unsigned* tab_start, unsigned short* tab_len, bool writer,
                Piece& p) {
  if (c == (unsigned)CLEAR) {
    reset(st);
    return CLEARED;
  }
  if (c == (unsigned)EOI) return STOP_EOI;
  p.kwkwk = false;
  p.literal = -1;
  if (c < 256u) {
    p.literal = (int)c;
    p.start = cursor;
    p.len = 1;
  } else if (st.prev_len == 0 || c > (unsigned)st.next) {
    return STOP_MALFORMED;
  } else if (c == (unsigned)st.next) {  // (next <= 4095 here: a code has 12 bits at the most)
    p.kwkwk = true;
    p.start = st.prev_start;
    p.len = st.prev_len + 1;
  } else {  // FIRST <= c < next: an entry that has been stored
    p.start = (int)tab_start[c];
    p.len = (int)tab_len[c];
  }
  // an entry names output that exists: by construction, and checked whatever the bits say
  if (p.literal < 0 && (p.start < 0 || p.len < 1 || (long long)p.start + p.len > (long long)cursor + (p.kwkwk ? 1 : 0)))
    return STOP_MALFORMED;
  if (st.prev_len != 0 && st.next < TABLE) {
    if (writer) {
      tab_start[st.next] = (unsigned)st.prev_start;
      tab_len[st.next] = (unsigned short)(st.prev_len + 1);
    }
    st.next += 1;
    if (st.next + 1 >= (1 << st.width) && st.width < MAX_WIDTH) st.width += 1;
  }
  st.prev_start = cursor;
  st.prev_len = p.len;
  return EMIT;
}

// byte i of a copied piece comes from this index of the strip's output
LZW_HD int copy_index(const Piece& p, int i) { return p.start + ((p.kwkwk && i == p.len - 1) ? 0 : i); }

// One strip: `nbytes` of stream at `s`, `expected` bytes of output.  emit(piece, cursor, len) appends the first
// `len` bytes of the piece at `cursor` (len >= 1, cursor + len <= expected).  The next code is read before the
// piece is emitted: the parse does not depend on the copy.  -> the bytes produced.
template <class Emit>
LZW_HD int decode_strip(const unsigned char* s, long long nbytes, int expected, unsigned* tab_start,
                        unsigned short* tab_len, bool writer, Emit&& emit) {
  State st;
  reset(st);
  const long long nbits = 8 * nbytes;
  long long bit = 0;
  int cursor = 0;
  bool have = expected > 0 && nbits >= st.width;
  unsigned c = have ? read_code(s, nbytes, 0, st.width) : 0u;
  while (have) {
    bit += st.width;
    Piece p;
    const int kind = step(st, c, cursor, tab_start, tab_len, writer, p);
    if (kind == STOP_EOI || kind == STOP_MALFORMED) break;
    int len = 0;
    if (kind == EMIT) len = p.len < expected - cursor ? p.len : expected - cursor;
    have = cursor + len < expected && nbits - bit >= st.width;
    if (have) c = read_code(s, nbytes, bit, st.width);
    if (len > 0) emit(p, cursor, len);
    cursor += len;
  }
  return cursor;
}

// compression 1: the strip's bytes are its rows; -> the bytes a strip of `nbytes` gives towards `expected`
LZW_HD int stored_bytes(long long nbytes, int expected) { return nbytes < expected ? (int)nbytes : expected; }

}  // namespace tiff_lzw
