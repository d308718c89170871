// A raw movie encoded as TIFF LZW strips (TIFF compression 5): the contiguous (t, h, row_bytes) bytes of a movie ->
// one code stream per strip of rows_per_strip rows, packed into one contiguous payload.  The encoder rule, the size
// bound slot_bytes() and the per-strip loop are in tiff_lzw_encode.h; this file holds the kernels around them and the
// entry points' host checks.
//
//   tiff_lzw_encode_strips  one wavefront per strip, as a one-wave workgroup: the parse (prefix code, next, width, the
//                           bit accumulator, the cursors) is wave-uniform; the dictionary is an open-addressed table
//                           of 8192 words in LDS that the 64 lanes probe 64 slots at a time, a ballot picking the hit
//                           or the first free slot: one LDS round trip per input byte.  Each strip writes into its
//                           own slot of slot_bytes and its byte count into produced[strip]
//   tiff_pack_strips        slot s's produced[s] bytes -> payload[offsets[s] ..], 16 bytes per lane between the
//                           payload's 16-byte boundaries
//
// Input bytes reach the parse 64 at a time: lane l holds byte 64 k + l of the strip, the next 64 are in flight, and
// the parse reads its byte with v_readlane.  Codes collect in a 64-bit accumulator; each full 32-bit word goes into
// lane (word & 63) of one register (a compare and a select), and every 64 words the wavefront stores 256 bytes with
// one vector store per lane.  Clear refills the table with a cooperative fill, 32 stores of 16 bytes per lane.
//
// Ordering.  A probe reads the word lane 0 inserted a few instructions earlier, and the first probe after a Clear
// reads what the fill wrote.  A wavefront's LDS instructions execute in order; the release / acquire fences at
// wavefront scope generate no instruction and keep the compiler from moving a load above those stores.
//
// Bounds.  load_chunk() clamps every index to the strip's last byte, store_words() and finish() store no byte at or
// beyond the slot's size, and the byte count is clipped to it, although slot_bytes() says clipping never happens.
// tiff_pack_strips clips the count to the slot and [offset, offset + count) to the payload.
#include "mc_common.h"
#include "mcorr.h"
#include "tiff_lzw_encode.h"

namespace {

constexpr int WAVE = 64, PACK_WG = 256;

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the wavefront's steps of tiff_lzw::encode_strip
struct Wave {
  unsigned* tab;             // LDS, ENC_SLOTS words
  const unsigned char* src;  // the strip's n bytes
  unsigned char* out;        // the slot: `cap` bytes, 16-byte aligned
  long long cap;
  int n, lane;
  unsigned mine = 0;           // the word this lane probed
  unsigned cur = 0, ahead = 0; // byte `lane` of the current chunk of 64, and of the chunk after it
  unsigned stage = 0;          // lane l: word (64 m + l) of the stream, in memory order, until the 64 are stored

  __device__ __forceinline__ unsigned load_chunk(long long first) const {  // n > 0
    long long i = first + lane;
    if (i > n - 1) i = n - 1;
    return src[i];
  }
  __device__ __forceinline__ void start() {
    if (n > 0) ahead = load_chunk(0);
  }
  __device__ __forceinline__ void chunk(long long first) {
    cur = ahead;
    ahead = load_chunk(first + WAVE);
  }
  __device__ __forceinline__ unsigned byte(int i) const { return __builtin_amdgcn_readlane(cur, i & 63); }
  __device__ __forceinline__ void clear_table() {
    wave_fence();
    typedef unsigned words4 __attribute__((ext_vector_type(4)));
    words4* t = reinterpret_cast<words4*>(tab);
    const unsigned f = tiff_lzw::ENC_FREE;
#pragma unroll 8
    for (int k = 0; k < tiff_lzw::ENC_SLOTS / 4 / WAVE; ++k) t[k * WAVE + lane] = words4{f, f, f, f};
    wave_fence();
  }
  __device__ __forceinline__ void probe(int base, unsigned key, unsigned long long& match, unsigned long long& free) {
    mine = tab[(base + lane) & (tiff_lzw::ENC_SLOTS - 1)];
    match = __ballot((mine >> 12) == key);
    free = __ballot(mine == tiff_lzw::ENC_FREE);
  }
  __device__ __forceinline__ unsigned probed(int l) const { return __builtin_amdgcn_readlane(mine, l); }
  __device__ __forceinline__ void insert(int slot, unsigned entry) {
    if (lane == 0) tab[slot] = entry;
    wave_fence();
  }
  // words first .. first + count - 1 (count <= 64) from the lanes that hold them
  __device__ __forceinline__ void store_words(long long first, int count) {
    if (lane >= count) return;
    const long long p = 4 * (first + lane);
    if (p + 4 <= cap) {
      *reinterpret_cast<unsigned*>(out + p) = stage;
    } else {
      for (int k = 0; k < 4; ++k)
        if (p + k < cap) out[p + k] = (unsigned char)(stage >> (8 * k));
    }
  }
  __device__ __forceinline__ void word(long long index, unsigned value) {
    if (lane == (int)(index & 63)) stage = __builtin_bswap32(value);
    if ((index & 63) == 63) store_words(index - 63, WAVE);
  }
  __device__ __forceinline__ void finish(long long words, unsigned last, int tail) {
    store_words(words & ~63ll, (int)(words & 63));
    const long long p = 4 * words + lane;
    if (lane < tail && p < cap) out[p] = (unsigned char)(last >> (24 - 8 * lane));
  }
};

// strip s of the flattened frame-major list: its first byte in the movie and the bytes its rows hold
__device__ __forceinline__ int strip_rows(long long s, int strips_per_frame, int h, int row_bytes,
                                          int rows_per_strip, long long* first) {
  const long long f = s / strips_per_frame;
  const int k = (int)(s - f * strips_per_frame);
  const int row0 = k * rows_per_strip;
  const int rows = h - row0 < rows_per_strip ? h - row0 : rows_per_strip;
  *first = (f * h + row0) * (long long)row_bytes;
  return rows * row_bytes;
}

__global__ __launch_bounds__(WAVE) void tiff_lzw_encode_strips(const unsigned char* __restrict__ src,
                                                               int strips_per_frame, int h, int row_bytes,
                                                               int rows_per_strip, unsigned char* __restrict__ slots,
                                                               long long slot_bytes,
                                                               long long* __restrict__ produced) {
  __shared__ __attribute__((aligned(16))) unsigned tab[tiff_lzw::ENC_SLOTS];
  const long long s = blockIdx.x;
  long long first;
  const int n = strip_rows(s, strips_per_frame, h, row_bytes, rows_per_strip, &first);
  Wave wave{tab, src + first, slots + s * slot_bytes, slot_bytes, n, (int)threadIdx.x};
  wave.start();
  const long long bytes = tiff_lzw::encode_strip(n, wave);
  if (threadIdx.x == 0) produced[s] = bytes < slot_bytes ? bytes : slot_bytes;
}

__global__ __launch_bounds__(PACK_WG) void tiff_pack_strips(const unsigned char* __restrict__ slots,
                                                            long long slot_bytes,
                                                            const long long* __restrict__ offsets,
                                                            const long long* __restrict__ produced,
                                                            unsigned char* __restrict__ payload,
                                                            long long payload_bytes) {
  const long long s = blockIdx.x;
  const long long at = offsets[s];
  long long n = produced[s];
  if (at < 0 || at >= payload_bytes || n <= 0) return;
  if (n > slot_bytes) n = slot_bytes;
  if (n > payload_bytes - at) n = payload_bytes - at;
  const unsigned char* from = slots + s * slot_bytes;
  unsigned char* to = payload + at;
  const int t = threadIdx.x;
  long long head = (long long)(-reinterpret_cast<uintptr_t>(to) & 15);  // up to the payload's next 16-byte boundary
  if (head > n) head = n;
  if (t < head) to[t] = from[t];
  const long long vecs = (n - head) >> 4;
  for (long long v = t; v < vecs; v += PACK_WG) {
    uint4 x;
    __builtin_memcpy(&x, from + head + 16 * v, 16);  // the source has any alignment
    *reinterpret_cast<uint4*>(to + head + 16 * v) = x;
  }
  const long long done = head + 16 * vecs;
  if (t < n - done) to[done + t] = from[done + t];
}

}  // namespace

extern "C" int mc_tiff_encode_slot_bytes(long long strip_bytes, long long* slot_bytes) {
  if (!slot_bytes || strip_bytes < 0) return MC_ERR_ARG;
  if (strip_bytes >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  *slot_bytes = tiff_lzw::slot_bytes(strip_bytes);
  return MC_OK;
}

extern "C" int mc_tiff_encode(const unsigned char* src, int n_frames, int h, int row_bytes, int rows_per_strip,
                              int compression, unsigned char* slots, long long slot_bytes, long long slots_bytes,
                              long long* produced, void* stream) {
  if (!src || !slots || !produced) return MC_ERR_ARG;
  if (n_frames < 1 || h < 1 || row_bytes < 1 || rows_per_strip < 1 || slot_bytes < 1 || slots_bytes < 1)
    return MC_ERR_ARG;
  if (compression != 5) return MC_ERR_UNSUPPORTED;  // stored strips are the movie's bytes: nothing to run
  if (rows_per_strip > h) return MC_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(produced) & 7) || (reinterpret_cast<uintptr_t>(slots) & 15) || (slot_bytes & 15))
    return MC_ERR_ARG;
  const long long strip_bytes = (long long)rows_per_strip * row_bytes;
  if (strip_bytes >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  const int strips_per_frame = (h + rows_per_strip - 1) / rows_per_strip;
  const long long n_strips = (long long)n_frames * strips_per_frame;
  if (n_strips >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  if (slot_bytes < tiff_lzw::slot_bytes(strip_bytes) || slots_bytes / slot_bytes < n_strips) return MC_ERR_ARG;
  hipLaunchKernelGGL(tiff_lzw_encode_strips, dim3((unsigned)n_strips), dim3(WAVE), 0, (hipStream_t)stream, src,
                     strips_per_frame, h, row_bytes, rows_per_strip, slots, slot_bytes, produced);
  return mc_check_launch();
}

extern "C" int mc_tiff_pack(const unsigned char* slots, long long slot_bytes, const long long* offsets,
                            const long long* produced, long long n_strips, unsigned char* payload,
                            long long payload_bytes, void* stream) {
  if (!slots || !offsets || !produced || !payload) return MC_ERR_ARG;
  if (slot_bytes < 1 || n_strips < 1 || payload_bytes < 1) return MC_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(offsets) & 7) || (reinterpret_cast<uintptr_t>(produced) & 7)) return MC_ERR_ARG;
  if (n_strips >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(tiff_pack_strips, dim3((unsigned)n_strips), dim3(PACK_WG), 0, (hipStream_t)stream, slots,
                     slot_bytes, offsets, produced, payload, payload_bytes);
  return mc_check_launch();
}
