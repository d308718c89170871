// EER event movies rendered into raw u8 movies: output frame k is the per-pixel event count of the input frames
// k g .. k g + g - 1, a (t_out, up h, up w) uint8 movie for every raw route.  The codec rule, the segment scheme and
// the per-lane bodies of the three passes are in eer.h; this file holds the kernels around them and the entry
// point's host checks.
//
//   eer_tables   pass A: one lane per segment, 11 packed records each
//   eer_scan     pass B: one workgroup per frame -> every segment's true entry offset and pixel base, the frame's
//                final n and event count
//   eer_scatter  pass C: one lane per segment, one vector-memory atomic add per event into the zeroed output
//
// Exactness.  Positions strictly increase within an input frame, so a physical pixel gets at most one event per
// frame and an output byte at most g <= 255: no byte of a 32-bit word carries into its neighbour, and integer adds
// commute, so the output is bit-exact whatever order the atomics land in.  Every stream read goes through
// eer::load32, which reads no byte outside the frame's own strip, whatever the bits say.
#include <vector>

#include "mc_common.h"
#include "mcorr.h"
#include "eer.h"

namespace {

using eer::Frame;
using eer::WG;

__global__ __launch_bounds__(WG) void eer_tables(const unsigned char* __restrict__ data,
                                                 const Frame* __restrict__ frames, int n_frames,
                                                 long long n_segments, int S, unsigned* __restrict__ tables) {
  eer::table_lane((long long)blockIdx.x * WG + threadIdx.x, n_segments, data, frames, n_frames, S, tables);
}

__global__ __launch_bounds__(WG) void eer_scan(const unsigned char* __restrict__ data,
                                               const Frame* __restrict__ frames, int S, long long N,
                                               const unsigned* __restrict__ tables, eer::u64* __restrict__ states,
                                               int* __restrict__ final_n, int* __restrict__ events) {
  __shared__ eer::Shared sh;
  __shared__ eer::u64 unstopped;
  const Frame fr = frames[blockIdx.x];
  const int lane = threadIdx.x;
  eer::fold_lane(lane, fr, S, tables, sh);
  __syncthreads();
  if (lane == 0) unstopped = eer::walk_lanes(sh);
  __syncthreads();
  eer::rewalk_lane(lane, fr, S, N, data, tables, states, sh);
  __syncthreads();
  if (lane == 0) eer::finish_frame(sh, unstopped, final_n + blockIdx.x, events + blockIdx.x);
}

__global__ __launch_bounds__(WG) void eer_scatter(const unsigned char* __restrict__ data,
                                                  const Frame* __restrict__ frames, int n_frames,
                                                  long long n_segments, int S,
                                                  const eer::u64* __restrict__ states, int h, int w, int up,
                                                  int group, int t_out, unsigned* __restrict__ out) {
  eer::scatter_lane((long long)blockIdx.x * WG + threadIdx.x, n_segments, data, frames, n_frames, S, states, h, w, up,
                    group, t_out, out);
}

}  // namespace

extern "C" int mc_eer_render(const unsigned char* data, long long data_bytes, const long long* offsets,
                             const long long* nbytes, int n_frames, int h, int w, int rle_bits, int upsampling,
                             int group, int seg_bytes, unsigned char* out, int* final_n, int* events, void* scratch,
                             long long scratch_bytes, void* stream) {
  if (!data || !offsets || !nbytes || !out || !final_n || !events || !scratch) return MC_ERR_ARG;
  if (data_bytes < 0 || n_frames < 1 || h < 1 || w < 1 || group < 1 || scratch_bytes < 0) return MC_ERR_ARG;
  if (rle_bits != eer::RLE_BITS) return rle_bits == 8 ? MC_ERR_UNSUPPORTED : MC_ERR_ARG;  // 8: compression 65000
  if (upsampling != 1 && upsampling != 2) return upsampling == 4 ? MC_ERR_UNSUPPORTED : MC_ERR_ARG;
  if (group > 255) return MC_ERR_UNSUPPORTED;  // a uint8 count holds at most 255 frames
  if (n_frames < group) return MC_ERR_ARG;
  if (seg_bytes != 64 && seg_bytes != 128 && seg_bytes != 256) return MC_ERR_UNSUPPORTED;
  const long long N = (long long)h * w;
  if (N >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  if (((long long)upsampling * w) % 4) return MC_ERR_UNSUPPORTED;  // a row of the output is whole 32-bit words
  if ((reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(final_n) & 3) ||
      (reinterpret_cast<uintptr_t>(events) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7))
    return MC_ERR_ARG;

  std::vector<Frame> table((size_t)n_frames);
  long long n_segments = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (offsets[f] < 0 || nbytes[f] < 0 || offsets[f] > data_bytes || nbytes[f] > data_bytes - offsets[f])
      return MC_ERR_ARG;
    if (nbytes[f] >= (1ll << 28)) return MC_ERR_UNSUPPORTED;
    table[f] = Frame{offsets[f], nbytes[f], n_segments};
    n_segments += (nbytes[f] + seg_bytes - 1) / seg_bytes;
  }
  if (n_segments >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  // scratch: the frame table, then every segment's state, then its 11 records
  const long long table_bytes = (long long)sizeof(Frame) * n_frames;
  if (scratch_bytes < table_bytes + n_segments * (8 + 4 * eer::ENTRIES)) return MC_ERR_ARG;
  Frame* frames = static_cast<Frame*>(scratch);
  eer::u64* states = reinterpret_cast<eer::u64*>(static_cast<char*>(scratch) + table_bytes);
  unsigned* tables = reinterpret_cast<unsigned*>(states + n_segments);

  hipStream_t st = (hipStream_t)stream;
  const int t_out = n_frames / group;
  hipError_t e = hipMemcpyWithStream(frames, table.data(), (size_t)table_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(out, 0, (size_t)t_out * (size_t)upsampling * upsampling * (size_t)N, st);
  if (e != hipSuccess) return (int)e;
  const unsigned blocks = (unsigned)((n_segments + WG - 1) / WG);
  if (blocks)
    hipLaunchKernelGGL(eer_tables, dim3(blocks), dim3(WG), 0, st, data, frames, n_frames, n_segments, seg_bytes,
                       tables);
  hipLaunchKernelGGL(eer_scan, dim3((unsigned)n_frames), dim3(WG), 0, st, data, frames, seg_bytes, N, tables, states,
                     final_n, events);
  if (blocks)
    hipLaunchKernelGGL(eer_scatter, dim3(blocks), dim3(WG), 0, st, data, frames, n_frames, n_segments, seg_bytes,
                       states, h, w, upsampling, group, t_out, reinterpret_cast<unsigned*>(out));
  return mc_check_launch();
}
