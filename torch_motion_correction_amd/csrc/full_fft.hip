// Full-spectrum 2-D real transforms with a ROW-MAJOR spectrum: what
// correct_motion_fast (correct_motion.py:484-496: rfftn -> fourier_shift_dft_2d -> irfftn) and the
// exposure-filtered frame sum (examples/ttMotion.py:331-351: rfft2 -> dose_weight_movie -> irfft2 ->
// sum) run on.
//
// The pruned engine (xc_common.h) hands its row pass output to the column pass TRANSPOSED
// (T1[job][kx][y]); with all nkx = W/2 + 1 bins kept that needs an LDS stage of nkx x RG bins per
// workgroup (147 KB for W = 4096: one workgroup per CU, 1.1 TB/s -- 1.9 ms per 15 frames, two thirds
// of correct_motion_fast's 12 ms per 40 x 4096^2 stack).  Here the spectrum stays row-major,
//     S[job][y][pitch]   complex, pitch = nkx rounded up to 16 (whole 128-byte lines per 16 columns),
// so a row pass reads or writes whole rows and needs no stage, and the COLUMN pass does the strided
// access instead: a workgroup owns two adjacent columns (16 bytes per row), stages them in two LDS
// lines, transforms forward, applies the pointwise step and transforms back IN PLACE -- one read and
// one write of S for what were two kernels and a round trip.  The eight workgroups whose column
// pairs share 128-byte lines are dispatched next to each other on one XCD (blockIdx mapping below),
// so every line is fetched from HBM once and written back whole.
//
//   full_rows_fwd   rows:  samples -> real FFT(W) -> S[job][y][0..W/2]
//   full_cols_shift cols:  S column pair -> FFT(H) -> * exp(-2 pi i (fy sy + fx sx)) / (H W) -> IFFT(H) -> S
//   full_cols_shift_sum  cols:  sum_f q_f(k) [R_f(k)] FFT_H(S_f column) accumulated in registers over
//                          the frames of a chunk (+ A) -> A; on the last chunk / sqrt(sum q^2), IFFT(H), / (H W)
//                          -- with or without the frames' phase ramps R_f; the plain sum likewise into P
//                          (full_sums.hip)
//   full_rows_inv   rows:  S[job][y][0..W/2] -> c2r pack -> IFFT(W/2) -> real rows
//
// Sizes: rows of W = 64 .. 8192 (powers of two), 5760 and 11520 columns (W / 2 = 2^a 3^2 5);
// columns of H = 256 .. 4096 (powers of two), 4092 and 8184 rows (2^a 3 11 31: radix-31 and radix-11
// passes, mc_fft.h) -- the K3 detector's two frame formats (BASELINE configs 3 and 5) run here
// without chirp-z.  Columns of more than 4096 rows go one column per workgroup (NC = 1).  full_rows_inv alone also
// takes the sizes Fourier cropping comes out at (fourier_crop_to.hip; full_common.h: full_rows_inverse_ok).
//
// This file holds the per-frame transforms of correct_motion_fast; the accumulating column passes, the raw row
// pass and its hot-pixel fix are full_sums.hip, an object of its own (one object holding both changed
// untouched kernels' code).  What both need is in full_common.h.
#include "full_common.h"

template <int N>
__global__ __launch_bounds__(MC_WG) void full_rows_fwd(const float* __restrict__ src,
                                                       const int64_t* __restrict__ job_off,
                                                       int64_t row_stride, cfloat* __restrict__ S, int H,
                                                       int pitch, const cfloat* __restrict__ tw_row,
                                                       int rows_per_wg) {
  // N complex points = W / 2
  __shared__ __attribute__((aligned(16))) cfloat line[lds_len(N)];
  const int tid = threadIdx.x;
  const int job = blockIdx.y;
  const float* base = src + job_off[job];
  for (int r = 0; r < rows_per_wg; ++r) {
    const int y = blockIdx.x * rows_per_wg + r;
    if (y >= H) break;  // workgroup-uniform
    const float* row = base + (int64_t)y * row_stride;
    auto load = [&](int j) {
      const float2 v = *reinterpret_cast<const float2*>(row + 2 * j);
      return cmake(v.x, v.y);
    };
    auto keep = [&](int k, cfloat v) { line[lpad(k)] = v; };
    wg_fft_any<N, -1>(line, (N & (N - 1)) ? full_opaque(tid) : tid, tw_row, 2, load, keep);
    __syncthreads();
    // real-FFT unpack: X[k] = (Z[k] + conj(Z[N-k]))/2 - i/2 * w^k * (Z[k] - conj(Z[N-k])), k = 0..N
    cfloat* out = S + ((int64_t)job * H + y) * pitch;
    for (int k = tid; k <= N; k += MC_WG) {
      const cfloat zk = line[lpad(k == N ? 0 : k)];
      const cfloat zm = cconj(line[lpad(k == 0 ? 0 : N - k)]);
      const cfloat sm = cadd(zk, zm), d = csub(zk, zm);
      const cfloat w = (k < N) ? tw_row[k] : cmake(-1.f, 0.f);
      const cfloat wd = cmul(w, d);  // -i*wd = (wd.y, -wd.x)
      out[k] = cmake(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));
    }
    __syncthreads();  // the next row's first pass writes the line
  }
}

template <int N>
__global__ __launch_bounds__(MC_WG) void full_rows_inv(const cfloat* __restrict__ S, float* __restrict__ out,
                                                       const int64_t* __restrict__ out_off, int64_t out_stride,
                                                       int H, int pitch, const cfloat* __restrict__ tw_row,
                                                       int rows_per_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem_fr[];
  cfloat* line = reinterpret_cast<cfloat*>(smem_fr);  // lds_len(N)
  cfloat* xs = line + lds_len(N) + 1;                 // N + 1 bins of the row
  const int tid = threadIdx.x;
  const int job = blockIdx.y;
  for (int r = 0; r < rows_per_wg; ++r) {
    const int y = blockIdx.x * rows_per_wg + r;
    if (y >= H) break;
    const cfloat* in = S + ((int64_t)job * H + y) * pitch;
    for (int k = tid; k <= N; k += MC_WG) xs[k] = in[k];
    __syncthreads();
    // c2r pack: Z[k] = (X[k] + conj(X[N-k])) + i * conj(w^k) * (X[k] - conj(X[N-k]))
    auto load = [&](int k) {
      cfloat xk = xs[k];
      cfloat xm = cconj(xs[N - k]);
      if (k == 0) {  // c2r ignores the imaginary part of the DC and Nyquist bins (pocketfft)
        xk.y = 0.f;
        xm.y = 0.f;
      }
      const cfloat sm = cadd(xk, xm), d = csub(xk, xm);
      cfloat w = tw_row[k];
      w.y = -w.y;
      const cfloat wd = cmul(w, d);  // i*wd = (-wd.y, wd.x)
      return cmake(sm.x - wd.y, sm.y + wd.x);
    };
    float* orow = out + out_off[job] + (int64_t)y * out_stride;
    auto store = [&](int n, cfloat v) { *reinterpret_cast<float2*>(orow + 2 * n) = make_float2(v.x, v.y); };
    wg_fft_any<N, +1>(line, (N & (N - 1)) ? full_opaque(tid) : tid, tw_row, 2, load, store);
    __syncthreads();  // xs and the line are rewritten by the next row
  }
}

template <int H, int NC, int WG>
__global__ __launch_bounds__(WG) void full_cols_shift(cfloat* __restrict__ S, int W, int pitch,
                                                         const cfloat* __restrict__ tw_col,
                                                         const float* __restrict__ shifts, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem_fc[];
  cfloat* lines[2] = {reinterpret_cast<cfloat*>(smem_fc), reinterpret_cast<cfloat*>(smem_fc) + lds_len(H)};
  const int tid = threadIdx.x;
  const int kx0 = full_col_of_block<NC>(blockIdx.x, pitch);
  if (kx0 > W / 2) return;  // padding columns of the pitch (workgroup-uniform)
  const int job = blockIdx.y;
  cfloat* base = S + (int64_t)job * H * pitch + kx0;
  full_cols_load<H, NC, WG>(lines, base, pitch, tid);
  __syncthreads();
  const float sy = shifts[2 * job], sx = shifts[2 * job + 1];
  const float m2pi = -6.283185307179586f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    cfloat* line = lines[c];
    const float fx = (float)(kx0 + c) * (float)(1.0 / (double)W);  // torch.fft.rfftfreq: k * (1/n)
    auto rd = [&](int i) { return line[lpad(i)]; };
    auto ramp = [&](int ky, cfloat v) {
      const float ang = (m2pi * full_fy(ky, H)) * sy + (m2pi * fx) * sx;
      float sn, cs;
      mc_sincos(ang, &sn, &cs);
      line[lpad(ky)] = cscale(cmul(v, cmake(cs, sn)), scale);
    };
    wg_fft_any_inplace<H, -1, WG>(line, full_opaque(tid), tw_col, 1, rd, ramp);
    __syncthreads();
    auto back = [&](int y, cfloat v) { line[lpad(y)] = v; };
    wg_fft_any_inplace<H, +1, WG>(line, full_opaque(tid), tw_col, 1, rd, back);
    __syncthreads();
  }
  full_cols_store<H, NC, WG>(lines, base, pitch, tid);
}

// ---- H = 4096: the register-resident radix-16 transform (mc_fft.h: 16 x 16 x 16, three passes,
// two exchanges through ONE 32 KiB line, 4 barriers).  Thread tid owns inputs 256 n1 + tid and
// outputs tid + 256 k3 -- the same rows -- so a column pair goes global -> registers -> forward ->
// pointwise -> inverse -> global without ever being staged: 32 KiB of LDS per workgroup instead of
// 70 (3-4 workgroups per CU instead of 2) and a third of the barriers.
__global__ __launch_bounds__(MC_WG) void full_cols_shift_r16(cfloat* __restrict__ S, int W, int pitch,
                                                             const cfloat* __restrict__ tw_col,
                                                             const float* __restrict__ shifts, float scale) {
  constexpr int H = 4096;
  __shared__ __attribute__((aligned(16))) cfloat line[H];
  const int tid = threadIdx.x;
  const int kx0 = 2 * full_pair_of_block(blockIdx.x, pitch / 2);
  if (kx0 > W / 2) return;  // padding columns of the pitch (workgroup-uniform)
  const int job = blockIdx.y;
  cfloat* base = S + (int64_t)job * H * pitch + kx0;
  cfloat v[2][16];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    const float4 q = *reinterpret_cast<const float4*>(base + (int64_t)(256 * n1 + tid) * pitch);
    v[0][n1] = cmake(q.x, q.y);
    v[1][n1] = cmake(q.z, q.w);
  }
  const float sy = shifts[2 * job], sx = shifts[2 * job + 1];
  const float m2pi = -6.283185307179586f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float fx = (float)(kx0 + c) * (float)(1.0 / (double)W);
    auto in = [&](int n1, int) { return v[c][n1]; };
    auto ramp = [&](int k, cfloat x) {
      const float ang = (m2pi * full_fy(k, H)) * sy + (m2pi * fx) * sx;
      float sn, cs;
      mc_sincos(ang, &sn, &cs);
      v[c][(k - tid) >> 8] = cscale(cmul(x, cmake(cs, sn)), scale);
    };
    wg_fft4096_r16<-1, 8, 8>(line, tid, tw_col, in, ramp);
    __syncthreads();
    auto back = [&](int k, cfloat x) { v[c][(k - tid) >> 8] = x; };
    wg_fft4096_r16<+1, 8, 8>(line, tid, tw_col, in, back);
    __syncthreads();
  }
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1)
    *reinterpret_cast<float4*>(base + (int64_t)(256 * n1 + tid) * pitch) =
        make_float4(v[0][n1].x, v[0][n1].y, v[1][n1].x, v[1][n1].y);
}

// S[job][y][pitch] (row-major) -> ST[job][kx][y] (column-major, kx <= W/2) through 64 x 64 LDS tiles:
// whole 512-byte row pieces in, whole 512-byte column pieces out.  The column passes use 8 or 16
// bytes of every 128-byte line of a row-major spectrum (L2 -> L1 traffic 8-16x the data: what
// bounds them); the exposure-weighted pass, which only READS the spectra of a chunk of frames,
// is fed from this copy instead: contiguous columns, one read + write pass more, less time.
__global__ __launch_bounds__(256) void full_transpose(const cfloat* __restrict__ S, cfloat* __restrict__ ST, int H,
                                                      int ncols, int pitch) {
  __shared__ __attribute__((aligned(16))) cfloat tile[64][66];
  const int job = blockIdx.z;
  const int y0 = blockIdx.y * 64, x0 = blockIdx.x * 64;
  const cfloat* src = S + (int64_t)job * H * pitch;
  cfloat* dst = ST + (int64_t)job * ncols * H;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8: a thread moves 2 bins at a time
#pragma unroll
  for (int r = ty; r < 64; r += 8) {
    const int y = y0 + r, x = x0 + 2 * tx;
    if (y < H && x < pitch) {  // pitch is a multiple of 16: whole pairs inside the row
      const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)y * pitch + x);
      tile[r][2 * tx] = cmake(v.x, v.y);
      tile[r][2 * tx + 1] = cmake(v.z, v.w);
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = ty; c < 64; c += 8) {
    const int x = x0 + c, y = y0 + 2 * tx;
    if (x < ncols && y < H) {  // H is even: whole pairs inside the column
      const cfloat a = tile[2 * tx][c], b = tile[2 * tx + 1][c];
      *reinterpret_cast<float4*>(dst + (int64_t)x * H + y) = make_float4(a.x, a.y, b.x, b.y);
    }
  }
}

extern "C" {

int mc_full_spectrum_pitch(int W) { return ((W / 2 + 1) + 15) & ~15; }

int mc_full_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride, void* S,
                         const void* tw_row, int njobs, int H, int W, int pitch, void* stream) {
  if (!src || !job_off || !S || !tw_row || njobs < 1) return MC_ERR_ARG;
  if (!full_sizes_ok(H, W, pitch) || (reinterpret_cast<uintptr_t>(src) & 7) || (row_stride & 1)) return MC_ERR_UNSUPPORTED;
  MC_FULL_DISPATCH_ROWS(W / 2, {
    hipLaunchKernelGGL(full_rows_fwd<L>, full_rows_grid(H, njobs), dim3(MC_WG), 0, (hipStream_t)stream, src, job_off,
                       row_stride, (cfloat*)S, H, pitch, (const cfloat*)tw_row, FULL_ROWS_PER_WG);
  });
  return mc_check_launch();
}

int mc_full_rows_inverse(const void* S, float* out, const int64_t* out_off, int64_t out_stride,
                         const void* tw_row, int njobs, int H, int W, int pitch, void* stream) {
  if (!S || !out || !out_off || !tw_row || njobs < 1) return MC_ERR_ARG;
  if (!full_rows_inverse_ok(H, W, pitch) || (reinterpret_cast<uintptr_t>(out) & 7) || (out_stride & 1))
    return MC_ERR_UNSUPPORTED;
  MC_FULL_DISPATCH_ROWS_INVERSE(W / 2, {
    auto k = full_rows_inv<L>;
    const size_t lds = sizeof(cfloat) * ((size_t)lds_len(L) + 1 + L + 2);
    MC_SET_LDS(k, lds);
    hipLaunchKernelGGL(k, full_rows_grid(H, njobs), dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)S, out,
                       out_off, out_stride, H, pitch, (const cfloat*)tw_row, FULL_ROWS_PER_WG);
  });
  return mc_check_launch();
}

int mc_full_cols_shift(void* S, const float* shifts, const void* tw_col, float scale, int njobs, int H, int W,
                       int pitch, void* stream) {
  if (!S || !shifts || !tw_col || njobs < 1) return MC_ERR_ARG;
  if (!full_sizes_ok(H, W, pitch)) return MC_ERR_UNSUPPORTED;
  if (H == 4096) {
    hipLaunchKernelGGL(full_cols_shift_r16, dim3(pitch / 2, njobs), dim3(MC_WG), 0, (hipStream_t)stream, (cfloat*)S,
                       W, pitch, (const cfloat*)tw_col, shifts, scale);
    return mc_check_launch();
  }
  MC_FULL_DISPATCH_COLS(H, {
    constexpr int NC = full_nc<L>(), WG = full_wg<L>();
    auto k = full_cols_shift<L, NC, WG>;
    const size_t lds = NC * sizeof(cfloat) * (size_t)lds_len(L);
    MC_SET_LDS(k, lds);
    hipLaunchKernelGGL(k, dim3(pitch / NC, njobs), dim3(WG), lds, (hipStream_t)stream, (cfloat*)S, W, pitch,
                       (const cfloat*)tw_col, shifts, scale);
  });
  return mc_check_launch();
}

int mc_full_transpose(const void* S, void* ST, int njobs, int H, int W, int pitch, void* stream) {
  if (!S || !ST || njobs < 1) return MC_ERR_ARG;
  if (!full_sizes_ok(H, W, pitch) || (H & 1)) return MC_ERR_UNSUPPORTED;
  const int ncols = W / 2 + 1;
  hipLaunchKernelGGL(full_transpose, dim3((ncols + 63) / 64, (H + 63) / 64, njobs), dim3(256), 0, (hipStream_t)stream,
                     (const cfloat*)S, (cfloat*)ST, H, ncols, pitch);
  return mc_check_launch();
}

}  // extern "C"
