// Fourier cropping of a row-major full spectrum to a given size: the column pass that goes in at H points and comes
// out at H2 <= H, for the pairs that are not a halving (fourier_crop.hip keeps those).
//
//   F = rfft2(x)  (H, W/2 + 1)  ->  G = rows -H2/2 <= ky < H2/2, columns 0 <= kx <= W2/2  ->  irfft2(G, (H2, W2))
//
// The row passes are full_fft.hip's and full_sums.hip's (mc_full_rows_forward / _raw at (H, W), mc_full_rows_inverse
// at (H2, W2), whose c2r ignores the imaginary parts of its DC and Nyquist bins); between them
//
//   full_cols_crop_to  cols:  S column (pair), kx <= W2/2 only -> FFT(H) -> keep ky < H2/2 or ky >= H - H2/2,
//                             * 1 / (H2 W2), at slot ky resp. ky - (H - H2) of an H2-point line -> IFFT(H2)
//                             -> S2[job][y'][pitch2]
//
// The two axes are independent: the rows are cropped by which columns the workgroups cover (the grid runs over
// pitch2 = mc_full_spectrum_pitch(W2) <= pitch, so S's lines beyond it are never read), the columns here.
//
// In place.  The kept rows are written over the SAME LDS line the forward transform ran in, for any H2 <= H: the
// forward transform's last pass reads all its inputs, passes a barrier, and only then stores (mc_fft.h: every last
// pass is instantiated with SYNC_MID, fft_rec and smooth_rec alike), so no thread still reads the line when the first
// kept row lands; and the two kept ranges land on disjoint slots, ky < H2/2 -> [0, H2/2) and ky >= H - H2/2 ->
// [H2/2, H2) -- the new Nyquist row H2/2 comes from ky = H - H2/2, the negative side.  The rows in between are
// dropped by not being stored.  LDS per workgroup is that of full_cols_crop: NC lines of lds_len(H) bins, of which
// the inverse uses the first lds_len(H2).
//
// Two twiddle tables.  A transform of N points reads exp(-2 pi i k / (N stride)) from its table, so the inverse
// could read the H-point table at a stride only where H2 divides H (the halving's stride 2).  4092 -> 2046 does,
// 8184 -> 5456, 8184 -> 2728, 4096 -> 3072 and 512 -> 384 do not: the inverse takes its own H2-point table, tw_col2,
// at stride 1, for every pair.
//
// H <= 4096 runs as column pairs on 256 threads, 8184 as single columns on 512 (full_nc, full_wg), like the other
// column passes.  mc_full_cols_crop and full_cols_crop are untouched.
#include "full_common.h"
#include "mc_fft.h"
#include "mcorr.h"

template <int H, int H2, int NC, int WG>
__global__ __launch_bounds__(WG) void full_cols_crop_to(const cfloat* __restrict__ S, cfloat* __restrict__ S2, int W2,
                                                        int pitch, int pitch2, const cfloat* __restrict__ tw_col,
                                                        const cfloat* __restrict__ tw_col2, float scale) {
  static_assert(H2 < H && (H2 & 1) == 0 && (H & 1) == 0, "an even output length below the input length");
  constexpr int P = H2 / 2, DROP = H - H2;
  extern __shared__ __attribute__((aligned(16))) char smem_crop_to[];
  cfloat* lines[2] = {reinterpret_cast<cfloat*>(smem_crop_to), reinterpret_cast<cfloat*>(smem_crop_to) + lds_len(H)};
  const int tid = threadIdx.x;
  const int kx0 = full_col_of_block<NC>(blockIdx.x, pitch2);
  if (kx0 > W2 / 2) return;  // padding columns of pitch2 (workgroup-uniform); kx0 + NC - 1 < pitch2 <= pitch
  const int job = blockIdx.y;
  full_cols_load<H, NC, WG>(lines, S + (int64_t)job * H * pitch + kx0, pitch, tid);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    cfloat* line = lines[c];
    auto rd = [&](int i) { return line[lpad(i)]; };
    auto crop = [&](int ky, cfloat v) {
      if (ky < P) line[lpad(ky)] = cscale(v, scale);
      else if (ky >= H - P) line[lpad(ky - DROP)] = cscale(v, scale);
    };
    wg_fft_any_inplace<H, -1, WG>(line, full_opaque(tid), tw_col, 1, rd, crop);
    __syncthreads();
    auto back = [&](int y, cfloat v) { line[lpad(y)] = v; };
    wg_fft_any_inplace<H2, +1, WG>(line, full_opaque(tid), tw_col2, 1, rd, back);
    __syncthreads();
  }
  full_cols_store<H2, NC, WG>(lines, S2 + (int64_t)job * H2 * pitch2 + kx0, pitch2, tid);
}

extern "C" int mc_full_cols_crop_to(const void* S, void* S2, const void* tw_col, const void* tw_col2, int njobs, int H,
                                    int W, int H2, int W2, int pitch, int pitch2, void* stream) {
  if (!S || !S2 || !tw_col || !tw_col2 || njobs < 1) return MC_ERR_ARG;
  if (W < 2 || W2 < 2 || (W & 1) || (W2 & 1) || W2 > W || !full_rows_ok(W) ||
      !(full_rows_ok(W2) || full_crop_rows_ok(W2)) || pitch < W / 2 + 1 || (pitch % 16) != 0 ||
      pitch2 != (((W2 / 2 + 1) + 15) & ~15))
    return MC_ERR_UNSUPPORTED;
#define MC_CROP_TO_CASE(HV, H2V)                                                                                   \
  if (H == HV && H2 == H2V) {                                                                                      \
    constexpr int NC = full_nc<HV>(), WG = full_wg<HV>();                                                          \
    auto k = full_cols_crop_to<HV, H2V, NC, WG>;                                                                   \
    const size_t lds = NC * sizeof(cfloat) * (size_t)lds_len(HV);                                                  \
    MC_SET_LDS(k, lds);                                                                                            \
    hipLaunchKernelGGL(k, dim3(pitch2 / NC, njobs), dim3(WG), lds, (hipStream_t)stream, (const cfloat*)S,          \
                       (cfloat*)S2, W2, pitch, pitch2, (const cfloat*)tw_col, (const cfloat*)tw_col2, scale);      \
    return mc_check_launch();                                                                                      \
  }
  const float scale = (float)(1.0 / ((double)H2 * (double)W2));
  MC_CROP_TO_CASE(512, 384)
  MC_CROP_TO_CASE(4096, 3072)
  MC_CROP_TO_CASE(4092, 2046)
  MC_CROP_TO_CASE(8184, 2728)
  MC_CROP_TO_CASE(8184, 5456)
#undef MC_CROP_TO_CASE
  return MC_ERR_UNSUPPORTED;
}
