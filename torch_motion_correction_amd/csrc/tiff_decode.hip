// TIFF strips decoded into a raw movie: LZW (TIFF compression 5) and stored (compression 1) strips of a multi-page
// TIFF -> the contiguous (t, h, row_bytes) bytes of the movie, a raw movie for every raw route once Python views it
// in its dtype.  The codec rule, the table layout and the per-strip loop are in tiff_lzw.h; this file holds the
// kernels around them and the entry point's host checks.
//
//   tiff_lzw_strips     one wavefront per strip, as a one-wave workgroup: the parse (next code, table lookup, emit
//                       cursor) is wave-uniform, the emit is a cooperative copy of earlier output, 64 bytes a step
//   tiff_stored_strips  compression 1: a strip-to-rows byte copy, same grid
//
// Ordering of copies.  A copy reads bytes of `out` that other lanes of the same wavefront stored a few instructions
// earlier, and a table lookup reads the entry lane 0 stored.  Each emit begins with a release and an acquire fence at
// wavefront scope: a wavefront's vector-memory and LDS instructions execute in order and one CU's L1 serves all of
// them, so the AMDGPU memory model implements that scope without a cache action or a wait; the fences keep the
// compiler from moving a load above the stores it depends on.
//
// Bounds.  read_code() reads no byte outside the strip, decode_strip() clips every emit to the strip's expected
// size, step() checks every table index against `next` and every entry against the bytes written so far: whatever
// the bits say, a strip touches its own stream and its own rows only.
#include <vector>

#include "mc_common.h"
#include "mcorr.h"
#include "tiff_lzw.h"

namespace {

constexpr int WAVE = 64;

struct Strip {
  long long offset, nbytes;
};

// strip s of the flattened frame-major list: its first output byte and the bytes its rows hold
__device__ __forceinline__ int strip_rows(long long s, int strips_per_frame, int h, int row_bytes,
                                          int rows_per_strip, long long* first) {
  const long long f = s / strips_per_frame;
  const int k = (int)(s - f * strips_per_frame);
  const int row0 = k * rows_per_strip;
  const int rows = h - row0 < rows_per_strip ? h - row0 : rows_per_strip;
  *first = (f * h + row0) * (long long)row_bytes;
  return rows * row_bytes;
}

__global__ __launch_bounds__(WAVE) void tiff_lzw_strips(const unsigned char* __restrict__ data,
                                                        const Strip* __restrict__ strips, int strips_per_frame,
                                                        int h, int row_bytes, int rows_per_strip,
                                                        unsigned char* out, int* __restrict__ produced) {
  __shared__ unsigned tab_start[tiff_lzw::TABLE];
  __shared__ unsigned short tab_len[tiff_lzw::TABLE];
  const long long s = blockIdx.x;
  const int lane = threadIdx.x;
  long long first;
  const int expected = strip_rows(s, strips_per_frame, h, row_bytes, rows_per_strip, &first);
  const Strip st = strips[s];
  unsigned char* o = out + first;
  const int n = tiff_lzw::decode_strip(
      data + st.offset, st.nbytes, expected, tab_start, tab_len, lane == 0,
      [&](const tiff_lzw::Piece& p, int cursor, int len) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (p.literal >= 0) {
          if (lane == 0) o[cursor] = (unsigned char)p.literal;
        } else {
          for (int i = lane; i < len; i += WAVE) o[cursor + i] = o[tiff_lzw::copy_index(p, i)];
        }
      });
  if (lane == 0) produced[s] = n;
}

__global__ __launch_bounds__(WAVE) void tiff_stored_strips(const unsigned char* __restrict__ data,
                                                           const Strip* __restrict__ strips, int strips_per_frame,
                                                           int h, int row_bytes, int rows_per_strip,
                                                           unsigned char* __restrict__ out,
                                                           int* __restrict__ produced) {
  const long long s = blockIdx.x;
  long long first;
  const int expected = strip_rows(s, strips_per_frame, h, row_bytes, rows_per_strip, &first);
  const Strip st = strips[s];
  const int n = tiff_lzw::stored_bytes(st.nbytes, expected);
  const unsigned char* src = data + st.offset;
  for (int i = threadIdx.x; i < n; i += WAVE) out[first + i] = src[i];
  if (threadIdx.x == 0) produced[s] = n;
}

}  // namespace

extern "C" int mc_tiff_decode(const unsigned char* data, long long data_bytes, const long long* offsets,
                              const long long* nbytes, int n_frames, int strips_per_frame, int h, int row_bytes,
                              int rows_per_strip, int compression, unsigned char* out, int* produced, void* scratch,
                              long long scratch_bytes, void* stream) {
  if (!data || !offsets || !nbytes || !out || !produced || !scratch) return MC_ERR_ARG;
  if (data_bytes < 0 || n_frames < 1 || strips_per_frame < 1 || h < 1 || row_bytes < 1 || rows_per_strip < 1 ||
      scratch_bytes < 0)
    return MC_ERR_ARG;
  if (compression != 1 && compression != 5) return MC_ERR_UNSUPPORTED;
  if (rows_per_strip > h) return MC_ERR_ARG;
  if (strips_per_frame != (h + rows_per_strip - 1) / rows_per_strip) return MC_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(produced) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7)) return MC_ERR_ARG;
  if ((long long)rows_per_strip * row_bytes >= (1ll << 31)) return MC_ERR_UNSUPPORTED;  // a strip's decoded size
  const long long n_strips = (long long)n_frames * strips_per_frame;
  if (n_strips >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  std::vector<Strip> table((size_t)n_strips);
  for (long long s = 0; s < n_strips; ++s) {
    if (offsets[s] < 0 || nbytes[s] < 0 || offsets[s] > data_bytes || nbytes[s] > data_bytes - offsets[s])
      return MC_ERR_ARG;
    table[(size_t)s] = Strip{offsets[s], nbytes[s]};
  }
  const long long table_bytes = (long long)sizeof(Strip) * n_strips;
  if (scratch_bytes < table_bytes) return MC_ERR_ARG;
  Strip* strips = static_cast<Strip*>(scratch);

  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyWithStream(strips, table.data(), (size_t)table_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  if (compression == 5)
    hipLaunchKernelGGL(tiff_lzw_strips, dim3((unsigned)n_strips), dim3(WAVE), 0, st, data, strips, strips_per_frame,
                       h, row_bytes, rows_per_strip, out, produced);
  else
    hipLaunchKernelGGL(tiff_stored_strips, dim3((unsigned)n_strips), dim3(WAVE), 0, st, data, strips,
                       strips_per_frame, h, row_bytes, rows_per_strip, out, produced);
  return mc_check_launch();
}
