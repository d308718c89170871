// MRC sample rows decoded into a raw movie: the payload of an MRC2014 file (modes 0, 1, 2, 6, 12 and the 4-bit mode
// 101) -> the contiguous (t, h, w) movie of the raw routes' types.  The format rule, the split of a row into an
// unaligned head, aligned 16-byte units and a tail, and every per-thread body are in mrc.h; this file holds the one
// kernel around them and the entry point's host checks.
//
//   mrc_rows<KIND>   a streaming pass: thread u of a row runs mrc::row_thread (one 16-byte load, one or two 16-byte
//                    stores on the aligned body), blockIdx.y strides over the rows of a frame, blockIdx.z over the
//                    frames; flip_rows only changes which source row a row reads
//
// Bounds.  A row's threads read the bytes of that source row only and write the elements of that output row only
// (mrc.h); the entry point checks that every source row lies inside `data` before anything is launched.
#include "mc_common.h"
#include "mcorr.h"
#include "mrc.h"

namespace {

constexpr int WG = 256;

template <int KIND>
__global__ __launch_bounds__(WG) void mrc_rows(const unsigned char* __restrict__ payload, int t, int h, int w,
                                               int flip_rows, unsigned char* __restrict__ out) {
  const int u = blockIdx.x * WG + threadIdx.x;
  if (u >= mrc::row_threads<KIND>(w)) return;
  const long long in_row = mrc::row_bytes(KIND, w), out_row = (long long)w * mrc::out_bytes(KIND);
  for (int f = blockIdx.z; f < t; f += gridDim.z)
    for (int r = blockIdx.y; r < h; r += gridDim.y) {
      const unsigned char* src = payload + ((long long)f * h + mrc::source_row(r, h, flip_rows)) * in_row;
      mrc::row_thread<KIND>(src, out + ((long long)f * h + r) * out_row, w, u);
    }
}

template <int KIND>
void launch(const unsigned char* payload, int t, int h, int w, int flip_rows, unsigned char* out, hipStream_t st) {
  const unsigned gx = (unsigned)((mrc::row_threads<KIND>(w) + WG - 1) / WG);
  const dim3 grid(gx, (unsigned)(h < 65535 ? h : 65535), (unsigned)(t < 65535 ? t : 65535));
  hipLaunchKernelGGL(mrc_rows<KIND>, grid, dim3(WG), 0, st, payload, t, h, w, flip_rows, out);
}

}  // namespace

extern "C" int mc_mrc_decode(const unsigned char* data, long long data_bytes, long long offset, int t, int h, int w,
                             int mode, int swap, int unsigned_bytes, int flip_rows, void* out, void* stream) {
  if (!data || !out || (const void*)data == out) return MC_ERR_ARG;
  if (data_bytes < 0 || offset < 0 || t < 1 || h < 1 || w < 1) return MC_ERR_ARG;
  if ((swap | unsigned_bytes | flip_rows) & ~1) return MC_ERR_ARG;
  const int kind = mrc::kind_of(mode, swap, unsigned_bytes);
  if (kind < 0) return MC_ERR_ARG;
  if ((long long)h * w >= (1ll << 31)) return MC_ERR_UNSUPPORTED;
  // offset + t * h * row_bytes <= data_bytes, without forming a product that may overflow
  const long long frame_bytes = (long long)h * mrc::row_bytes(kind, w);  // < 2^33
  if (offset > data_bytes || (data_bytes - offset) / frame_bytes < t) return MC_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(out) % mrc::out_bytes(kind)) return MC_ERR_ARG;

  hipStream_t st = (hipStream_t)stream;
  const unsigned char* payload = data + offset;
  unsigned char* o = static_cast<unsigned char*>(out);
  switch (kind) {
    case mrc::COPY1: launch<mrc::COPY1>(payload, t, h, w, flip_rows, o, st); break;
    case mrc::WIDEN: launch<mrc::WIDEN>(payload, t, h, w, flip_rows, o, st); break;
    case mrc::COPY2: launch<mrc::COPY2>(payload, t, h, w, flip_rows, o, st); break;
    case mrc::SWAP2: launch<mrc::SWAP2>(payload, t, h, w, flip_rows, o, st); break;
    case mrc::COPY4: launch<mrc::COPY4>(payload, t, h, w, flip_rows, o, st); break;
    case mrc::SWAP4: launch<mrc::SWAP4>(payload, t, h, w, flip_rows, o, st); break;
    default: launch<mrc::NIBBLE>(payload, t, h, w, flip_rows, o, st); break;
  }
  return mc_check_launch();
}
