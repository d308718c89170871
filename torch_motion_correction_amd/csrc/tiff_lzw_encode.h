// TIFF 6.0 LZW (TIFF compression 5), the other direction: the per-strip ENCODER of the codec rule tiff_lzw.h states,
// written so that a host compiler takes it as well: tests/host_tiff_lzw_encode.cpp runs the same loop with a serial
// form of the wavefront's steps under the address and undefined-behaviour sanitizers.  Nothing here needs the HIP
// runtime.
//
// THE ENCODER RULE is the default of tests/tiff_reference.py::encode_strip(data); the output equals that function's
// byte for byte, for every input, so the encoder is deterministic and is checked without a decoder in the loop:
//
//   a leading Clear (256) at 9 bits; the state is then width = 9, next = 258, no previous code
//   greedy longest match: c = the first byte; while the pair (c, following byte) is in the table, c = its code
//   c is emitted with the current width, packed MSB-first; then, as the decoder does when it reads c: with a
//     previous code and next < 4096, next += 1 and "early change": next + 1 >= (1 << width) and width < 12 -> width += 1
//   if input is left: the pair (c, following byte) -> code `next` goes into the table, and the following byte is
//     the new c; then, once next >= 4093, Clear is emitted (with the width then in force) and the state and the
//     table start over
//   after the last byte's code: EOI (257) at the width then in force, and zero bits up to a whole byte
//
// The empty strip is Clear, EOI: three bytes.
//
// THE SIZE BOUND slot_bytes(n) of the stream of an n-byte strip.  Every data code stands for at least one input byte:
// at most n data codes.  After a Clear the first data code adds no entry and every later one adds one, and a Clear
// inside the strip is emitted only after `next` has gone from 258 to 4093, that is after 3835 added entries (3836
// data codes): at most n / 3835 of them, besides the leading one.  One EOI.  Every code has at most 12 bits:
//
//   codes <= n + n / 3835 + 2,     bytes <= ceil(12 * codes / 8) = (3 * codes + 1) / 2
//
// rounded up to 16 so that consecutive slots keep the alignment of the first.  The worst case, a strip none of whose
// pairs repeats before the next Clear (every code one byte), stays below it by the codes of 9 - 11 bits.
// encode_strip() clips every store to the slot all the same.
//
// THE TABLE maps (prefix code, next byte), a 20-bit key, to the 12-bit code: one 32-bit word key << 12 | code in an
// open-addressed table of ENC_SLOTS = 8192 words (32 KB), all ones = free (code 4095 is never assigned).  A table
// holds at most 3836 entries, so it is less than half full.  A key's home is hash(key); a probe looks at the
// ENC_WINDOW = 64 consecutive slots from there (one per lane of a wavefront, one LDS instruction) and pick() takes
// the hit or, failing that, the first free slot -- entries are never removed, so a key that is present lies before
// the first free slot of its probe sequence; only a window with neither goes on to the next 64 slots.
#pragma once
#include "tiff_lzw.h"

namespace tiff_lzw {

constexpr int CLEAR_AT = 4093;  // Clear once next >= this, as libtiff does
constexpr int ENC_SLOTS = 8192, ENC_WINDOW = 64;
constexpr unsigned ENC_FREE = 0xffffffffu;

LZW_HD constexpr long long slot_bytes(long long n) {
  return ((3 * (n + n / 3835 + 2) + 1) / 2 + 15) & ~15ll;
}
static_assert(slot_bytes(0) == 16 && slot_bytes(1) == 16 && slot_bytes(65536) == 98336, "the bound as derived");
static_assert(slot_bytes((1ll << 31) - 1) < (1ll << 32), "a 2^31 - 1 byte strip's stream has a 32-bit length");

LZW_HD unsigned enc_key(unsigned prefix, unsigned byte) { return prefix << 8 | byte; }
LZW_HD unsigned enc_entry(unsigned key, unsigned code) { return key << 12 | code; }
LZW_HD int enc_hash(unsigned key) { return (int)((key * 2654435761u) >> 19); }  // the top 13 bits: 0 .. 8191

enum { HIT = 0, FREE = 1, NEXT_WINDOW = 2 };

// one window: `match` / `free` have a bit per lane whose slot holds the key / is free -> which lane counts
LZW_HD int pick(unsigned long long match, unsigned long long free, int& lane) {
  if (match) {
    lane = __builtin_ctzll(match);
    return HIT;
  }
  if (free) {
    lane = __builtin_ctzll(free);
    return FREE;
  }
  return NEXT_WINDOW;
}

// The key's code, or -1 with `slot` = where it belongs (slot -1: no free slot in the whole table, which a table of
// at most 3836 entries cannot reach; nothing is inserted then, and the stream stays decodable).
//   wave.probe(base, key, match, free)  every lane l reads slot (base + l) & (ENC_SLOTS - 1); the two ballots
//   wave.probed(l)                      the word lane l read
template <class Wave>
LZW_HD int find(Wave& wave, unsigned key, int& slot) {
  int base = enc_hash(key);
  for (int k = 0; k < ENC_SLOTS / ENC_WINDOW; ++k) {
    unsigned long long match, free;
    wave.probe(base, key, match, free);
    int lane;
    const int kind = pick(match, free, lane);
    if (kind == HIT) return (int)(wave.probed(lane) & 0xfffu);
    if (kind == FREE) {
      slot = (base + lane) & (ENC_SLOTS - 1);
      return -1;
    }
    base = (base + ENC_WINDOW) & (ENC_SLOTS - 1);
  }
  slot = -1;
  return -1;
}

// the code stream: `nbits` (< 32) bits wait in the low end of `acc`; whole 32-bit words go out as they fill
struct Bits {
  unsigned long long acc;
  int nbits;
  long long words;
};

//   wave.word(index, value)  word `index` of the stream: its bytes are value's, most significant first
template <class Wave>
LZW_HD void put(Bits& b, unsigned code, int width, Wave& wave) {
  b.acc = b.acc << width | code;
  b.nbits += width;
  if (b.nbits >= 32) {
    b.nbits -= 32;
    wave.word(b.words, (unsigned)(b.acc >> b.nbits));
    b.words += 1;
  }
}

// the encoder's copy of the decoder's state: width for the next code, the decoder's next free code, whether it has
// a previous code
struct EncState {
  int width, next;
  bool prev;
};

// what the decoder does when it reads a data code
LZW_HD void emitted(EncState& st) {
  if (st.prev && st.next < TABLE) {
    st.next += 1;
    if (st.next + 1 >= (1 << st.width) && st.width < MAX_WIDTH) st.width += 1;
  }
  st.prev = true;
}

// One strip of n >= 0 bytes -> the bytes of its stream.  Everything here is the same in every lane of a wavefront.
// The input is walked in chunks of ENC_WINDOW bytes, so that a wavefront can hold one chunk in a register, a byte
// per lane, while the next is in flight.
//   wave.clear_table()            every slot free
//   wave.chunk(first)             bytes first .. first + 63 are asked for next; chunks come in ascending order
//   wave.byte(i)                  input byte i of the current chunk, 0 <= i < n
//   wave.insert(slot, entry)      one lane stores the entry
//   wave.finish(words, last, k)   the words not yet stored, then the k <= 4 last bytes, the top bytes of `last`
// The wave clips its stores to the slot; the caller clips the returned count.
template <class Wave>
LZW_HD long long encode_strip(int n, Wave& wave) {
  Bits b = {0ull, 0, 0ll};
  EncState st = {MIN_WIDTH, FIRST, false};
  wave.clear_table();
  put(b, (unsigned)CLEAR, st.width, wave);
  if (n > 0) {
    unsigned c = 0;  // the code of the longest string found so far; it ends at byte i - 1
    for (long long first = 0; first < n; first += ENC_WINDOW) {
      wave.chunk(first);
      const int end = first + ENC_WINDOW < n ? (int)first + ENC_WINDOW : n;
      int i = (int)first;
      if (i == 0) c = wave.byte(i++);
      for (; i < end; ++i) {
        const unsigned d = wave.byte(i), key = enc_key(c, d);
        int slot;
        const int code = find(wave, key, slot);
        if (code >= 0) {
          c = (unsigned)code;
          continue;
        }
        put(b, c, st.width, wave);
        emitted(st);
        if (st.next < TABLE && slot >= 0) wave.insert(slot, enc_entry(key, (unsigned)st.next));
        c = d;
        if (st.next >= CLEAR_AT) {
          put(b, (unsigned)CLEAR, st.width, wave);
          st = {MIN_WIDTH, FIRST, false};
          wave.clear_table();
        }
      }
    }
    put(b, c, st.width, wave);
    emitted(st);
  }
  put(b, (unsigned)EOI, st.width, wave);
  const int tail = (b.nbits + 7) >> 3;
  wave.finish(b.words, (unsigned)(b.acc << (32 - b.nbits)), tail);
  return 4 * b.words + tail;
}

}  // namespace tiff_lzw
