// A raw movie encoded as MRC sample rows, with the header's statistics from the same pass: the contiguous (t, h, w)
// uint8 / int16 movie -> the payload of an MRC2014 file (modes 0, 1, 6 and the 4-bit mode 101) and a (t, 5) int64
// table of {min, max, sum, sum of squares, samples out of the mode's range} per frame.  The format rule, the split
// of a row into an unaligned head, aligned 16-byte units and a tail, every per-thread body and the scratch rule are in
// mrc_encode.h; this file holds the two kernels around them and the entry point's host checks.
//
//   mrc_encode_rows<KIND>  a streaming pass: blocks_per_frame workgroups stride over a frame's row-threads
//                          (mrcenc::frame_item: one 16-byte load, one 16-, 8- or 4-byte store on the aligned body),
//                          then sum their threads' statistics (wave shuffles, LDS) into one partial in scratch;
//                          blockIdx.y strides over the frames
//   mrc_encode_finish      one workgroup per frame sums the frame's partials the same way into the table
//
// Integer sums, minima and maxima: the table does not depend on scheduling, and no atomic is involved.
// Bounds.  A row's threads read the samples of that movie row only and write the bytes of that payload row only
// (mrc_encode.h); the entry point checks the payload's and the scratch's sizes before anything is launched.
#include "mc_common.h"
#include "mcorr.h"
#include "mrc_encode.h"

namespace {

using mrcenc::Stats;
using mrcenc::WG;

// the workgroup's statistics summed -> thread 0 writes the 5 values to `out`
__device__ void reduce_to(const Stats& mine, long long* out) {
  __shared__ long long part[WG / 64][mrcenc::STATS];
  long long v[mrcenc::STATS] = {mine.mn, mine.mx, mine.sum, mine.sq, mine.bad};
  __syncthreads();  // `part` may still be read by thread 0 for the frame before
  for (int d = 32; d > 0; d >>= 1) {
    const long long mn = __shfl_down(v[0], d, 64), mx = __shfl_down(v[1], d, 64);
    v[0] = mn < v[0] ? mn : v[0];
    v[1] = mx > v[1] ? mx : v[1];
    for (int k = 2; k < mrcenc::STATS; ++k) v[k] += __shfl_down(v[k], d, 64);
  }
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0)
    for (int k = 0; k < mrcenc::STATS; ++k) part[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < WG / 64; ++i) {
      v[0] = part[i][0] < v[0] ? part[i][0] : v[0];
      v[1] = part[i][1] > v[1] ? part[i][1] : v[1];
      for (int k = 2; k < mrcenc::STATS; ++k) v[k] += part[i][k];
    }
    for (int k = 0; k < mrcenc::STATS; ++k) out[k] = v[k];
  }
}

template <int KIND>
__global__ __launch_bounds__(WG) void mrc_encode_rows(const unsigned char* __restrict__ movie, int t, int h, int w,
                                                      int flip_rows, unsigned char* __restrict__ payload,
                                                      long long* __restrict__ partials) {
  const long long items = (long long)h * mrcenc::row_threads(mrcenc::sample_bytes(KIND), w);
  for (int f = blockIdx.y; f < t; f += gridDim.y) {
    const unsigned char* frame = movie + (long long)f * h * w * mrcenc::sample_bytes(KIND);
    unsigned char* out = payload + (long long)f * h * mrcenc::row_bytes(KIND, w);
    Stats s = mrcenc::no_stats();
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < items; i += (long long)gridDim.x * WG)
      mrcenc::frame_item<KIND>(frame, out, h, w, flip_rows, i, s);
    reduce_to(s, partials + ((long long)f * gridDim.x + blockIdx.x) * mrcenc::STATS);
  }
}

__global__ __launch_bounds__(WG) void mrc_encode_finish(const long long* __restrict__ partials, int t, int blocks,
                                                        long long* __restrict__ stats) {
  for (int f = blockIdx.x; f < t; f += gridDim.x) {
    const long long* p = partials + (long long)f * blocks * mrcenc::STATS;
    Stats s = mrcenc::no_stats();
    for (int b = threadIdx.x; b < blocks; b += WG)
      mrcenc::merge(s, Stats{(int)p[b * mrcenc::STATS], (int)p[b * mrcenc::STATS + 1], p[b * mrcenc::STATS + 2],
                             p[b * mrcenc::STATS + 3], p[b * mrcenc::STATS + 4]});
    reduce_to(s, stats + (long long)f * mrcenc::STATS);
  }
}

template <int KIND>
void launch(const unsigned char* movie, int t, int h, int w, int flip_rows, unsigned char* payload, long long* partials,
            int blocks, hipStream_t st) {
  const dim3 grid((unsigned)blocks, (unsigned)(t < 65535 ? t : 65535));
  hipLaunchKernelGGL(mrc_encode_rows<KIND>, grid, dim3(WG), 0, st, movie, t, h, w, flip_rows, payload, partials);
}

}  // namespace

extern "C" int mc_mrc_encode(const void* movie, int elem_bytes, int t, int h, int w, int mode, int flip_rows,
                             unsigned char* payload, long long payload_bytes, long long* stats, void* scratch,
                             long long scratch_bytes, void* stream) {
  if (!movie || !payload || !stats || !scratch || movie == (const void*)payload) return MC_ERR_ARG;
  if (t < 1 || h < 1 || w < 1 || payload_bytes < 0 || scratch_bytes < 0 || (flip_rows & ~1)) return MC_ERR_ARG;
  const int kind = mrcenc::kind_of(elem_bytes, mode);
  if (kind < 0) return MC_ERR_UNSUPPORTED;
  if ((long long)h * w >= (1ll << 31)) return MC_ERR_ARG;
  // t * h * row_bytes <= payload_bytes, without forming a product that may overflow
  const long long frame_bytes = (long long)h * mrcenc::row_bytes(kind, w);  // < 2^32
  if (payload_bytes / frame_bytes < t) return MC_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(movie) % elem_bytes) return MC_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(stats) % 8 || reinterpret_cast<uintptr_t>(scratch) % 8) return MC_ERR_ARG;
  const int blocks = mrcenc::blocks_per_frame(elem_bytes, h, w);
  if (scratch_bytes / ((long long)blocks * mrcenc::STATS * 8) < t) return MC_ERR_ARG;

  hipStream_t st = (hipStream_t)stream;
  const unsigned char* m = static_cast<const unsigned char*>(movie);
  long long* partials = static_cast<long long*>(scratch);
  switch (kind) {
    case mrcenc::U8_COPY: launch<mrcenc::U8_COPY>(m, t, h, w, flip_rows, payload, partials, blocks, st); break;
    case mrcenc::U8_NIBBLE: launch<mrcenc::U8_NIBBLE>(m, t, h, w, flip_rows, payload, partials, blocks, st); break;
    case mrcenc::I16_COPY: launch<mrcenc::I16_COPY>(m, t, h, w, flip_rows, payload, partials, blocks, st); break;
    case mrcenc::I16_U16: launch<mrcenc::I16_U16>(m, t, h, w, flip_rows, payload, partials, blocks, st); break;
    case mrcenc::I16_BYTE: launch<mrcenc::I16_BYTE>(m, t, h, w, flip_rows, payload, partials, blocks, st); break;
    default: launch<mrcenc::I16_NIBBLE>(m, t, h, w, flip_rows, payload, partials, blocks, st); break;
  }
  const int rc = mc_check_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(mrc_encode_finish, dim3((unsigned)(t < 65535 ? t : 65535)), dim3(WG), 0, st, partials, t, blocks,
                     stats);
  return mc_check_launch();
}
