// Fourier cropping (2x binning per axis) of a row-major full spectrum: the column pass that goes in at
// H points and comes out at H / 2.
//
//   F = rfft2(x)  (H, W/2 + 1)  ->  G = rows -H/4 <= ky < H/4, columns 0 <= kx <= W/4  ->  irfft2(G, (H/2, W/2))
//
// The row passes are full_fft.hip's and full_sums.hip's as they are (mc_full_rows_forward / _raw at (H, W),
// mc_full_rows_inverse at (H/2, W/2), whose c2r ignores the imaginary parts of its DC and Nyquist bins); between them
//
//   full_cols_crop  cols:  S column (pair), kx <= W/4 only -> FFT(H) -> keep ky < H/4 or ky >= 3H/4, * 1 / (H2 W2),
//                          at ky' = ky (mod H/2) of an H/2-point line -> IFFT(H/2) -> S2[job][y'][pitch2]
//
// Columns beyond W/4 are never read: the workgroups cover the columns of S2's pitch only, so half of S's
// 128-byte lines are skipped.  The kept rows are written over the SAME LDS line the forward transform ran in:
// its last pass reads all its inputs, passes a barrier, then stores (mc_fft.h: SYNC_MID), so no thread still
// reads the line when the first kept row lands, and ky' < H/2 never collides with another kept row
// (ky < H/4 -> [0, H/4), ky >= 3H/4 -> [H/4, H/2): the new Nyquist row H/4 comes from ky = 3H/4, the negative
// side).  LDS per workgroup is therefore that of full_cols_shift: NC lines of lds_len(H) bins.  The inverse
// transform reads the H-point twiddle table at stride 2.
#include "full_common.h"
#include "mc_fft.h"
#include "mcorr.h"

template <int H, int NC, int WG>
__global__ __launch_bounds__(WG) void full_cols_crop(const cfloat* __restrict__ S, cfloat* __restrict__ S2, int W,
                                                     int pitch, int pitch2, const cfloat* __restrict__ tw_col,
                                                     float scale) {
  constexpr int H2 = H / 2, Q = H / 4;
  extern __shared__ __attribute__((aligned(16))) char smem_crop[];
  cfloat* lines[2] = {reinterpret_cast<cfloat*>(smem_crop), reinterpret_cast<cfloat*>(smem_crop) + lds_len(H)};
  const int tid = threadIdx.x;
  const int kx0 = full_col_of_block<NC>(blockIdx.x, pitch2);
  if (kx0 > W / 4) return;  // padding columns of pitch2 (workgroup-uniform); kx0 + NC - 1 < pitch2 <= pitch
  const int job = blockIdx.y;
  full_cols_load<H, NC, WG>(lines, S + (int64_t)job * H * pitch + kx0, pitch, tid);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    cfloat* line = lines[c];
    auto rd = [&](int i) { return line[lpad(i)]; };
    auto crop = [&](int ky, cfloat v) {
      if (ky < Q) line[lpad(ky)] = cscale(v, scale);
      else if (ky >= H - Q) line[lpad(ky - H2)] = cscale(v, scale);
    };
    wg_fft_any_inplace<H, -1, WG>(line, full_opaque(tid), tw_col, 1, rd, crop);
    __syncthreads();
    auto back = [&](int y, cfloat v) { line[lpad(y)] = v; };
    wg_fft_any_inplace<H2, +1, WG>(line, full_opaque(tid), tw_col, 2, rd, back);
    __syncthreads();
  }
  full_cols_store<H2, NC, WG>(lines, S2 + (int64_t)job * H2 * pitch2 + kx0, pitch2, tid);
}

extern "C" int mc_full_cols_crop(const void* S, void* S2, const void* tw_col, int njobs, int H, int W, int pitch,
                                 int pitch2, void* stream) {
  if (!S || !S2 || !tw_col || njobs < 1) return MC_ERR_ARG;
  if (H < 2 || W < 2 || (H & 1) || (W & 1) || !full_cols_ok(H) || !full_cols_ok(H / 2) || !full_rows_ok(W) ||
      !full_rows_ok(W / 2) || pitch < W / 2 + 1 || (pitch % 16) != 0 || pitch2 != (((W / 4 + 1) + 15) & ~15))
    return MC_ERR_UNSUPPORTED;
  const float scale = (float)(1.0 / ((double)(H / 2) * (double)(W / 2)));
#define MC_CROP_CASE(HV)                                                                                            \
  case HV: {                                                                                                        \
    constexpr int NC = full_nc<HV>(), WG = full_wg<HV>();                                                           \
    auto k = full_cols_crop<HV, NC, WG>;                                                                            \
    const size_t lds = NC * sizeof(cfloat) * (size_t)lds_len(HV);                                                   \
    MC_SET_LDS(k, lds);                                                                                             \
    hipLaunchKernelGGL(k, dim3(pitch2 / NC, njobs), dim3(WG), lds, (hipStream_t)stream, (const cfloat*)S,           \
                       (cfloat*)S2, W, pitch, pitch2, (const cfloat*)tw_col, scale);                                \
  } break;
  switch (H) {
    MC_CROP_CASE(512) MC_CROP_CASE(1024) MC_CROP_CASE(2048) MC_CROP_CASE(4096) MC_CROP_CASE(8184)
    default: return MC_ERR_UNSUPPORTED;
  }
#undef MC_CROP_CASE
  return mc_check_launch();
}
