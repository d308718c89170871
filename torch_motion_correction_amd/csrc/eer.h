// EER event movies: the codec rule and the per-lane bodies of the three render passes (eer_render.hip), written so
// that a host compiler takes them as well: tests/host_eer.cpp runs every lane of every pass in turn under the address
// and undefined-behaviour sanitizers.  Nothing here needs the HIP runtime.
//
// THE CODEC RULE.  A frame of a detector with h x w physical pixels (N = h * w) is a little-endian bit stream: bit k
// of the stream is bit k & 7 of byte k >> 3.  With bit = 0, n = 0:
//
//   loop:  p = 7 bits at `bit`;  bit += 7;  n += p
//          if n >= N: stop                      (n == N: well formed;  n > N: malformed)
//          if p == 127: continue                (a skip: no sub-pixel bits follow)
//          s = 4 bits at `bit`;  bit += 4;  event at linear position n with sub-pixel code s;  n += 1
//
// Decoding also stops when the next symbol would begin at or after bit 8 * nbytes.  Bits at and beyond 8 * nbytes
// read as zero: the reader never touches a byte outside the strip.  The event's pixel is y = n / w, x = n % w; with
// upsampling 1 it goes to (y, x), with upsampling 2 to (2 y + ((s >> 3) & 1), 2 x + ((s >> 1) & 1)).  symbol() and
// place() below are the only statement of this rule in the library.  It was written from the public description of
// the format; NO vendor-written file has been decoded with it, so bit-level conformance is unpinned.
//
// SEGMENTS.  A symbol is 7 or 11 bits long, so a stream parses serially.  It is cut into segments of S bytes; a
// symbol belongs to the segment that holds its first bit and may read up to 10 bits into the next one, so the only
// state that enters a segment is the offset e in 0 .. 10 of its first symbol (and the pixel count n, which only
// adds).  The passes below ignore the stop at n >= N while they count ("unstopped" n) and apply it afterwards: n
// never decreases, every event after the stop has n >= N, and the stop itself is the first run, in stream order,
// that ends at n >= N.
//
//   A  table_lane    one lane per segment: for each of the 11 entry offsets, parse to the segment's end -> exit
//                    offset, pixels advanced, events (one packed 32-bit record each)
//   B  fold_lane     one workgroup per frame; each lane composes the records of a run of consecutive segments for
//      walk_lanes    all 11 entries, one lane follows the true entry (0 at the frame's start) through the WG folds,
//      rewalk_lane   each lane walks its run again with its true entry and base: every segment's entry offset and
//      finish_frame  pixel base, the events before the stop, the stop itself -> the frame's final n and event count
//   C  scatter_lane  one lane per segment: parse from the true entry and base, add 1 to the output byte of every
//                    event with n < N (an atomic add of 1 << 8 (x & 3) on the aligned 32-bit word: a count is at
//                    most group <= 255, so no byte carries, and integer adds commute)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EER_HD __host__ __device__ __forceinline__
#else
#define EER_HD inline
#endif

namespace eer {

typedef unsigned long long u64;

constexpr int WG = 256;
constexpr int RLE_BITS = 7, SUB_BITS = 4, RUN_MAX = (1 << RLE_BITS) - 1;
constexpr int ENTRIES = RLE_BITS + SUB_BITS;  // entry offsets 0 .. 10
constexpr int SEG_MAX = 256;                  // the records' fields hold segments up to this many bytes
constexpr u64 NO_STOP = ~0ull;

// one row of the frame table: the strip's place in the buffer and the frame's first segment
struct Frame {
  long long offset, nbytes, seg0;
};

// ------------------------------------------------------------------ bounded bit reader

// 4 bytes at byte b of the strip, little endian; bytes at and beyond nbytes are zero and are not read
EER_HD unsigned load32(const unsigned char* s, long long nbytes, long long b) {
  unsigned v = 0;
  if (b + 4 <= nbytes) {
    __builtin_memcpy(&v, s + b, 4);
    return v;
  }
  for (int k = 0; k < 4; ++k)
    if (b + k < nbytes) v |= (unsigned)s[b + k] << (8 * k);
  return v;
}

struct Bits {
  const unsigned char* s;
  long long nbytes, next;  // next: the first byte not yet in the window
  u64 win;
  int avail;
};

EER_HD Bits open_bits(const unsigned char* s, long long nbytes, long long bit) {
  Bits r = {s, nbytes, (bit >> 3) + 4, load32(s, nbytes, bit >> 3), 32};
  r.win >>= (int)(bit & 7);
  r.avail -= (int)(bit & 7);
  return r;
}

// the next k <= 7 bits
EER_HD unsigned take(Bits& r, int k) {
  if (r.avail < k) {
    r.win |= (u64)load32(r.s, r.nbytes, r.next) << r.avail;
    r.next += 4;
    r.avail += 32;
  }
  const unsigned v = (unsigned)r.win & ((1u << k) - 1u);
  r.win >>= k;
  r.avail -= k;
  return v;
}

// ------------------------------------------------------------------ the rule

// One symbol: the run, and whether an event follows it (then sub holds its code).  bit advances by 7 or 11.
EER_HD bool symbol(Bits& r, int& bit, int& run, int& sub) {
  run = (int)take(r, RLE_BITS);
  bit += RLE_BITS;
  if (run == RUN_MAX) return false;
  sub = (int)take(r, SUB_BITS);
  bit += SUB_BITS;
  return true;
}

// the output pixel of an event at linear position n < N with code sub
EER_HD void place(int n, int sub, int w, int up, int& yo, int& xo) {
  const int y = n / w, x = n - y * w;
  if (up == 2) {
    yo = 2 * y + ((sub >> 3) & 1);
    xo = 2 * x + ((sub >> 1) & 1);
  } else {
    yo = y;
    xo = x;
  }
}

// ------------------------------------------------------------------ segments

// exit offset (4 bits) | events << 4 (8 bits: <= 8 * 256 / 11) | pixels advanced << 12 (16 bits: <= 293 * 127)
EER_HD unsigned pack_record(int exit, int events, int pixels) {
  return (unsigned)exit | ((unsigned)events << 4) | ((unsigned)pixels << 12);
}
EER_HD int rec_exit(unsigned r) { return (int)(r & 15u); }
EER_HD int rec_events(unsigned r) { return (int)((r >> 4) & 255u); }
EER_HD int rec_pixels(unsigned r) { return (int)(r >> 12); }

// entry offset | unstopped pixel base << 4 (the base stays below 2^36: nbytes < 2^28)
EER_HD u64 pack_state(int entry, u64 base) { return (u64)entry | (base << 4); }

// the frame of global segment `seg`: the last row with seg0 <= seg (rows without segments share their seg0 with
// the next row)
EER_HD int find_frame(const Frame* frames, int n_frames, long long seg) {
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frames[mid].seg0 <= seg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// bits of segment k of a strip: 8 * S, less in the strip's last segment
EER_HD int segment_bits(long long nbytes, long long k, int S) {
  const long long left = nbytes - k * S;
  return 8 * (int)(left < S ? left : S);
}

// ------------------------------------------------------------------ pass A

EER_HD void table_lane(long long seg, long long n_segments, const unsigned char* data, const Frame* frames,
                       int n_frames, int S, unsigned* tables) {
  if (seg >= n_segments) return;
  const Frame fr = frames[find_frame(frames, n_frames, seg)];
  const long long k = seg - fr.seg0;
  const unsigned char* strip = data + fr.offset;
  const int L = segment_bits(fr.nbytes, k, S);
  for (int e = 0; e < ENTRIES; ++e) {
    int bit = e, pixels = 0, events = 0;
    if (e < L) {
      Bits r = open_bits(strip, fr.nbytes, k * S * 8 + e);
      while (bit < L) {
        int run, sub = 0;
        const int ev = symbol(r, bit, run, sub) ? 1 : 0;
        pixels += run + ev;
        events += ev;
      }
    }
    tables[seg * ENTRIES + e] = pack_record(bit - L, events, pixels);
  }
}

// ------------------------------------------------------------------ pass B

// the lanes' folds and true states, in the workgroup's LDS (plain arrays on the host)
struct Shared {
  u64 dn[WG * ENTRIES];
  unsigned char exit[WG * ENTRIES];
  int lane_entry[WG];
  u64 lane_base[WG];
  u64 lane_stop[WG];
  int lane_events[WG];
};

// segments per lane of a frame with nseg segments
EER_HD long long lane_run(long long nseg) { return (nseg + WG - 1) / WG; }

// lane's run of segments composed for every entry offset
EER_HD void fold_lane(int lane, const Frame& fr, int S, const unsigned* tables, Shared& sh) {
  const long long nseg = (fr.nbytes + S - 1) / S, per = lane_run(nseg);
  const long long s0 = lane * per, s1 = s0 + per < nseg ? s0 + per : nseg;
  for (int e = 0; e < ENTRIES; ++e) {
    int cur = e;
    u64 dn = 0;
    for (long long s = s0; s < s1; ++s) {
      const unsigned rec = tables[(fr.seg0 + s) * ENTRIES + cur];
      cur = rec_exit(rec);
      dn += (u64)rec_pixels(rec);
    }
    sh.dn[lane * ENTRIES + e] = dn;
    sh.exit[lane * ENTRIES + e] = (unsigned char)cur;
  }
}

// one lane follows the true entry through the folds; returns the frame's unstopped n
EER_HD u64 walk_lanes(Shared& sh) {
  int entry = 0;
  u64 base = 0;
  for (int l = 0; l < WG; ++l) {
    sh.lane_entry[l] = entry;
    sh.lane_base[l] = base;
    base += sh.dn[l * ENTRIES + entry];
    entry = sh.exit[l * ENTRIES + entry];
  }
  return base;
}

// A segment that may hold the stop (base <= N <= base + pixels advanced), parsed: the events before position N and,
// where a run ends at n >= N, (the run's first bit in the stream) << 32 | that n.  n <= N + 127 fits 32 bits.
EER_HD u64 stop_scan(const unsigned char* strip, long long nbytes, long long k, int S, int entry, long long base,
                     long long N, int& events) {
  const int L = segment_bits(nbytes, k, S);
  events = 0;
  if (entry >= L) return NO_STOP;
  Bits r = open_bits(strip, nbytes, k * S * 8 + entry);
  long long n = base;
  int bit = entry;
  while (bit < L) {
    const u64 at = (u64)(k * S * 8 + bit);
    int run, sub = 0;
    const bool ev = symbol(r, bit, run, sub);
    n += run;
    if (n >= N) return (at << 32) | (u64)n;
    if (ev) {
      ++events;
      ++n;
    }
  }
  return NO_STOP;
}

// lane's run again, from its true entry and base: the segments' states, the lane's events before the stop and the
// lane's earliest stop
EER_HD void rewalk_lane(int lane, const Frame& fr, int S, long long N, const unsigned char* data,
                        const unsigned* tables, u64* states, Shared& sh) {
  const long long nseg = (fr.nbytes + S - 1) / S, per = lane_run(nseg);
  const long long s0 = lane * per, s1 = s0 + per < nseg ? s0 + per : nseg;
  int entry = sh.lane_entry[lane], events = 0;
  u64 base = sh.lane_base[lane], stop = NO_STOP;
  for (long long s = s0; s < s1; ++s) {
    states[fr.seg0 + s] = pack_state(entry, base);
    const unsigned rec = tables[(fr.seg0 + s) * ENTRIES + entry];
    const u64 dn = (u64)rec_pixels(rec);
    if (base + dn < (u64)N) {
      events += rec_events(rec);  // every event of the segment lies before N
    } else if (base <= (u64)N) {
      int before;
      const u64 at = stop_scan(data + fr.offset, fr.nbytes, s, S, entry, (long long)base, N, before);
      events += before;
      if (at < stop) stop = at;
    }
    base += dn;
    entry = rec_exit(rec);
  }
  sh.lane_stop[lane] = stop;
  sh.lane_events[lane] = events;
}

// the frame's final n (the n of the earliest stop; without one the stream ran out at its unstopped n <= N) and its
// event count
EER_HD void finish_frame(const Shared& sh, u64 unstopped, int* final_n, int* events) {
  u64 stop = NO_STOP;
  int ev = 0;
  for (int l = 0; l < WG; ++l) {
    if (sh.lane_stop[l] < stop) stop = sh.lane_stop[l];
    ev += sh.lane_events[l];
  }
  if (stop != NO_STOP) *final_n = (int)(stop & 0xffffffffull);
  else *final_n = unstopped > 0x7fffffffull ? 0x7fffffff : (int)unstopped;
  *events = ev;
}

// ------------------------------------------------------------------ pass C

EER_HD void count_event(unsigned* word, unsigned add) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(word, add);
#else
  *word += add;
#endif
}

// out: (t_out, up h, up w) bytes at a 4-byte address, up w % 4 == 0: a row never shares a word with another row
EER_HD void scatter_lane(long long seg, long long n_segments, const unsigned char* data, const Frame* frames,
                         int n_frames, int S, const u64* states, int h, int w, int up, int group, int t_out,
                         unsigned* out) {
  if (seg >= n_segments) return;
  const int f = find_frame(frames, n_frames, seg);
  if (f / group >= t_out) return;  // the trailing frames that fill no group
  const Frame fr = frames[f];
  const long long N = (long long)h * w, k = seg - fr.seg0;
  const u64 st = states[seg];
  if ((st >> 4) >= (u64)N) return;
  int n = (int)(st >> 4), bit = (int)(st & 15u);
  const int L = segment_bits(fr.nbytes, k, S);
  if (bit >= L) return;
  const long long wo = (long long)up * w, frame_px = wo * up * h;
  unsigned* frame = out + (f / group) * (frame_px >> 2);
  Bits r = open_bits(data + fr.offset, fr.nbytes, k * S * 8 + bit);
  while (bit < L) {
    int run, sub = 0;
    const bool ev = symbol(r, bit, run, sub);
    if (run >= N - n) return;  // n + run >= N: the stop, or past it
    n += run;
    if (ev) {
      int yo, xo;
      place(n, sub, w, up, yo, xo);
      count_event(frame + ((yo * wo + xo) >> 2), 1u << (8 * (xo & 3)));
      ++n;
    }
  }
}

}  // namespace eer
