// Fused shift-and-sum over a row-major full spectrum (layout and passes: full_fft.hip): the plain and
// exposure-weighted sums of the Fourier-shifted
// frames (correct_motion_fast -> sum / dose_weighted_sum) without the shifted frames.  Both sums are
// linear, so   sum_f irfft2(R_f X_f) = irfft2(sum_f R_f X_f)  and the exposure-weighted sum of the shifted
// frames is  irfft2(sum_f q_f R_f X_f) / sqrt(sum_f q_f^2)  (q_f is real and even in ky, and irfft2 ignores
// what rfft2(irfft2(.)) would project away): one forward transform per frame with the ramp R_f applied
// and both sums accumulated inside the forward column pass, then one inverse transform per sum.  Without
// the ramp the same pass gives the exposure-weighted sum of the frames themselves (dose_weighted_sum).
//
// Also here, in the same object: the row pass that reads raw frames and its hot-pixel fix.  What this file
// and full_fft.hip both need is in full_common.h.
#include "full_common.h"

// The conditioning of mc_condition_movie, c = raw * gain - mu_f, as it rounds it: a product, then a
// difference (cond_vec_kernel compiles to v_pk_mul_f32 + v_pk_add_f32, no fma) -- so a raw row pass
// transforms bit for bit the samples of the conditioned movie.
__device__ __forceinline__ float full_cond(float raw, float gain, float mu) {
#pragma clang fp contract(off)
  return raw * gain - mu;
}

// full_rows_fwd reading raw frames: KIND 0 u8, 1 i16 (RawMovie.kind), a (H, W) fp32 gain and each job's
// frame mean mu[job]; frame j starts at element job_off[j] of src, rows W = 2N samples apart.  The
// transform and the unpack are full_rows_fwd's.
template <int N, int KIND>
__global__ __launch_bounds__(MC_WG) void full_rows_fwd_raw(const void* __restrict__ src, const float* __restrict__ gain,
                                                           const float* __restrict__ mu,
                                                           const int64_t* __restrict__ job_off, cfloat* __restrict__ S,
                                                           int H, int pitch, const cfloat* __restrict__ tw_row,
                                                           int rows_per_wg) {
  __shared__ __attribute__((aligned(16))) cfloat line[lds_len(N)];
  const int tid = threadIdx.x;
  const int job = blockIdx.y;
  const float m = mu[job];
  using T = typename std::conditional<KIND == 0, unsigned char, short>::type;
  using T2 = typename std::conditional<KIND == 0, uchar2, short2>::type;
  const T* base = reinterpret_cast<const T*>(src) + job_off[job];
  for (int r = 0; r < rows_per_wg; ++r) {
    const int y = blockIdx.x * rows_per_wg + r;
    if (y >= H) break;  // workgroup-uniform
    const int64_t row0 = (int64_t)y * (2 * N);
    const T* row = base + row0;
    const float* grow = gain + row0;
    auto load = [&](int j) {
      const float2 g = *reinterpret_cast<const float2*>(grow + 2 * j);
      const T2 v = *reinterpret_cast<const T2*>(row + 2 * j);
      return cmake(full_cond((float)v.x, g.x, m), full_cond((float)v.y, g.y, m));
    };
    auto keep = [&](int k, cfloat v) { line[lpad(k)] = v; };
    wg_fft_any<N, -1>(line, (N & (N - 1)) ? full_opaque(tid) : tid, tw_row, 2, load, keep);
    __syncthreads();
    cfloat* out = S + ((int64_t)job * H + y) * pitch;
    for (int k = tid; k <= N; k += MC_WG) {  // real-FFT unpack, as full_rows_fwd
      const cfloat zk = line[lpad(k == N ? 0 : k)];
      const cfloat zm = cconj(line[lpad(k == 0 ? 0 : N - k)]);
      const cfloat sm = cadd(zk, zm), d = csub(zk, zm);
      const cfloat w = (k < N) ? tw_row[k] : cmake(-1.f, 0.f);
      const cfloat wd = cmul(w, d);
      out[k] = cmake(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));
    }
    __syncthreads();
  }
}

// Exposure filter of examples/ttMotion.py:331-351 (crit_exposure_bfactor = -1), as dose_accumulate_kernel
// (polyphase.hip) defines it: q_f(k) = exp(-0.5 N_f / N_c(|k|)), N_c = (0.24499 |k|^-1.6649 + 2.8141)
// vscale, N_f = pre + dose_per_frame (f + 1), |k| in 1/Angstrom clamped at 1e-6.
__device__ __forceinline__ float full_dose_mh(int kx, int ky, int W, int H, float pixel_size, float vscale) {
  const float fy = full_fy(ky, H);
  const float fx = (float)kx * (float)(1.0 / (double)W);
  const float f = fmaxf(sqrtf(fy * fy + fx * fx) / pixel_size, 1e-6f);
  const float ncrit = (0.24499f * powf(f, -1.6649f) + 2.8141f) * vscale;
  return -0.5f / ncrit;
}

// radix of the last pass of a mixed-radix length-H transform; outputs the last pass hands to one
// thread (per column)
template <int H>
__host__ __device__ constexpr int full_last_radix() {
  int ns = 1, r = 1;
  while (ns < H) {
    r = smooth_radix(H / ns);
    ns *= r;
  }
  return r;
}
template <int H, int WG>
__host__ __device__ constexpr int full_last_slots() {
  if ((H & (H - 1)) == 0) return (H / MC_WG) > 8 ? (H / MC_WG) : 8;  // 512 / 256 points: radix 8 / 4 on 64 threads
  constexpr int r = full_last_radix<H>();
  return ((H / r + WG - 1) / WG) * r;  // iterations of the last pass x its radix
}

// The phase ramp of full_cols_shift on one output of a column transform: its angle expression, so the fused
// sums and the per-frame shift round alike.  Every contraction is spelled out (which product of a sum of two
// the compiler fuses is otherwise its choice per kernel) and the product is made opaque before it is
// accumulated, so the plain sum is the same bits whether or not the exposure-weighted one is accumulated
// alongside (MODE 1 vs 3).
// Not to be merged with the angle expression of full_cols_shift / _r16 (full_fft.hip): that one contracts differently.
__device__ __forceinline__ cfloat full_ramp(cfloat v, int ky, int H, float fx, float sy, float sx) {
  const float m2pi = -6.283185307179586f;
  const float ang = __builtin_fmaf(m2pi * full_fy(ky, H), sy, (m2pi * fx) * sx);
  float sn, cs;
  mc_sincos(ang, &sn, &cs);
  cfloat z = cmake(__builtin_fmaf(v.x, cs, -(v.y * sn)), __builtin_fmaf(v.x, sn, v.y * cs));
  asm volatile("" : "+v"(z.x), "+v"(z.y));
  return z;
}

// Each frame's forward column transform is multiplied by its phase ramp (shifts[j] = (sy, sx) px of frame j of
// the chunk), then accumulated over the frames in registers -- MODE 1: plainly into P, 2: exposure-weighted into
// A, 3: both from one read of the spectra; 2 | FULL_NO_RAMP: exposure-weighted without the ramp (shifts not read),
// the exposure-filtered sum of the frames as they are.  The accumulators add what earlier chunks left in A / P
// (first = 0); on the last chunk they are normalised, transformed back along the columns and scaled (the plain
// sum only scaled).
constexpr int FULL_NO_RAMP = 4;
template <int MODE>
struct full_mode {
  static_assert(MODE == 1 || MODE == 2 || MODE == 3 || MODE == (2 | FULL_NO_RAMP),
                "plain (1), exposure-weighted (2) or both (3) with the phase ramp; exposure-weighted without it (6)");
  static constexpr bool dose = (MODE & 2) != 0, plain = (MODE & 1) != 0, ramp = (MODE & FULL_NO_RAMP) == 0;
};

// Input strides (in complex elements): element (frame j, row y, column kx) of S sits at
// j sf + y sr + kx sc -- row-major spectra: (H pitch, pitch, 1); column-major copies made by
// full_transpose: (ncols H, 1, H), read with NC = 1 as contiguous columns.
template <int H, int NC, int WG, int MODE>
__global__ __launch_bounds__(WG) void full_cols_shift_sum(const cfloat* __restrict__ S, const float* __restrict__ shifts,
                                              int nframes, int frame0, int total_frames, cfloat* __restrict__ A,
                                              cfloat* __restrict__ P, int W, int pitch,
                                              const cfloat* __restrict__ tw_col, float pixel_size,
                                              float pre_exposure, float dose_per_frame, float vscale, int first,
                                              int last, float scale, int64_t sf, int64_t sr, int64_t sc) {
  using M = full_mode<MODE>;
  constexpr int SLOTS = full_last_slots<H, WG>();
  extern __shared__ __attribute__((aligned(16))) char smem_fc[];
  cfloat* lines[2] = {reinterpret_cast<cfloat*>(smem_fc), reinterpret_cast<cfloat*>(smem_fc) + lds_len(H)};
  const int tid = threadIdx.x;
  const int kx0 = full_col_of_block<NC>(blockIdx.x, pitch);
  if (kx0 > W / 2) return;  // padding columns of the pitch (workgroup-uniform)
  // mixed-radix lines (one column per workgroup): the exposure exponents of the column's rows sit in
  // LDS behind the line instead of in 24-33 registers per thread
  constexpr bool MH_LDS = (H & (H - 1)) != 0;
  static_assert(!MH_LDS || NC == 1, "mixed-radix exposure pass: one column per workgroup");
  float* mhl = reinterpret_cast<float*>(lines[0] + NC * lds_len(H));
  if constexpr (MH_LDS && M::dose) {
    for (int ky = tid; ky < H; ky += WG) mhl[ky] = full_dose_mh(kx0, ky, W, H, pixel_size, vscale);
  }
  cfloat acc[NC][M::dose ? SLOTS : 1];
  cfloat pacc[NC][M::plain ? SLOTS : 1];
  float mh[NC][(MH_LDS || !M::dose) ? 1 : SLOTS];
  int kys[SLOTS];  // output row of a slot (power-of-two lines: recorded; mixed radix: computed, see below)
  int nslots = 0;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) kys[s] = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      if constexpr (M::dose) acc[c][s] = cmake(0.f, 0.f);
      if constexpr (M::plain) pacc[c][s] = cmake(0.f, 0.f);
      if constexpr (!MH_LDS && M::dose) mh[c][s] = 0.f;
    }
  for (int j = 0; j < nframes; ++j) {
    full_cols_load<H, NC, WG>(lines, S + (int64_t)j * sf + (int64_t)kx0 * sc, sr, tid);
    __syncthreads();
    const float dose = pre_exposure + dose_per_frame * (float)(frame0 + j + 1);
    float sy = 0.f, sx = 0.f;
    if constexpr (M::ramp) {
      sy = shifts[2 * j];
      sx = shifts[2 * j + 1];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      cfloat* line = lines[c];
      const float fx = (float)(kx0 + c) * (float)(1.0 / (double)W);  // torch.fft.rfftfreq: k * (1/n)
      auto rd = [&](int i) { return line[lpad(i)]; };
      auto take3 = [&](int ky, cfloat v, int slot) {
        float m;
        if constexpr (MH_LDS) {
          if constexpr (M::dose) m = mhl[ky];
        } else {
          if (j == 0) {
            kys[slot] = ky;
            if constexpr (M::dose) mh[c][slot] = full_dose_mh(kx0 + c, ky, W, H, pixel_size, vscale);
          }
          if constexpr (M::dose) m = mh[c][slot];
        }
        if constexpr (M::ramp) v = full_ramp(v, ky, H, fx, sy, sx);
        if constexpr (M::plain) {
          pacc[c][slot].x += v.x;
          pacc[c][slot].y += v.y;
        }
        if constexpr (M::dose) {
          const float q = expf(m * dose);
          acc[c][slot].x += q * v.x;
          acc[c][slot].y += q * v.y;
        }
      };
      if constexpr ((H & (H - 1)) == 0) {
        int slot = 0;  // the last pass calls `take` SLOTS times per thread, in a fixed (unrolled) order
        auto take = [&](int ky, cfloat v) {
          take3(ky, v, slot);
          ++slot;
        };
        wg_fft_any_inplace<H, -1, WG>(line, full_opaque(tid), tw_col, 1, rd, take);
        nslots = slot;
      } else {
        // mixed radix: the pass itself names the slot (iteration x radix + output), a compile-time
        // constant at every call site; the last iteration only runs on the threads that have a butterfly
        wg_fft_any_inplace<H, -1, WG>(line, full_opaque(tid), tw_col, 1, rd, take3);
        constexpr int R = full_last_radix<H>();
        nslots = (tid + (SLOTS / R - 1) * WG < H / R) ? SLOTS : SLOTS - R;
      }
    }
    __syncthreads();  // the next frame overwrites the lines
  }
  // accumulator columns: add what earlier chunks left in A / P, on the last chunk "restore the power"
  // (/ sqrt(sum_f q_f^2) over ALL frames; the plain sum: scale only), transform back and scale
  auto finish = [&](auto& ac, cfloat* out, auto weighted) {
    cfloat* abase = out + kx0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (s >= nslots) continue;
        cfloat a = ac[c][s];
        int ky = kys[s];
        if constexpr ((H & (H - 1)) != 0) {  // last mixed-radix pass: output j + m H/R of butterfly j = tid + it WG
          constexpr int R = full_last_radix<H>();
          ky = tid + (s / R) * WG + (s % R) * (H / R);
        }
        if (!first) {
          const cfloat prev = abase[(int64_t)ky * pitch + c];
          a.x += prev.x;
          a.y += prev.y;
        }
        if (last) {
          float r = scale;
          if constexpr (decltype(weighted)::value) {
            const float m = MH_LDS ? mhl[ky] : mh[c][MH_LDS ? 0 : s];
            float qq = 0.f;
            for (int f = 0; f < total_frames; ++f) {
              const float q = expf(m * (pre_exposure + dose_per_frame * (float)(f + 1)));
              qq += q * q;
            }
            r = scale / sqrtf(qq);
          }
          a.x *= r;
          a.y *= r;
        }
        lines[c][lpad(ky)] = a;
      }
    }
    __syncthreads();
    if (last) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        cfloat* line = lines[c];
        auto rd = [&](int i) { return line[lpad(i)]; };
        auto back = [&](int y, cfloat v) { line[lpad(y)] = v; };
        wg_fft_any_inplace<H, +1, WG>(line, full_opaque(tid), tw_col, 1, rd, back);
        __syncthreads();
      }
    }
    full_cols_store<H, NC, WG>(lines, abase, pitch, tid);
  };
  if constexpr (M::dose) finish(acc, A, std::true_type{});
  if constexpr (M::dose && M::plain) __syncthreads();  // the plain columns go through the same lines
  if constexpr (M::plain) finish(pacc, P, std::false_type{});
}

template <int NC, int MODE>
__global__ __launch_bounds__(MC_WG) void full_cols_shift_sum_r16(const cfloat* __restrict__ S, const float* __restrict__ shifts,
                                                  int nframes, int frame0, int total_frames, cfloat* __restrict__ A,
                                                  cfloat* __restrict__ P, int W, int pitch,
                                                  const cfloat* __restrict__ tw_col, float pixel_size,
                                                  float pre_exposure, float dose_per_frame, float vscale, int first,
                                                  int last, float scale, int64_t sf, int64_t sr, int64_t sc) {
  // NC = 1: one column per workgroup (8-byte loads; 130 registers instead of 256 + spills to AGPRs:
  // three wavefronts per SIMD instead of one)
  using M = full_mode<MODE>;
  constexpr int H = 4096;
  __shared__ __attribute__((aligned(16))) cfloat line[H];
  const int tid = threadIdx.x;
  const int kx0 = full_col_of_block<NC>(blockIdx.x, pitch);
  if (kx0 > W / 2) return;  // padding columns of the pitch (workgroup-uniform)
  cfloat acc[NC][M::dose ? 16 : 1];
  cfloat pacc[NC][M::plain ? 16 : 1];
  float mh[NC][M::dose ? 16 : 1];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k3 = 0; k3 < 16; ++k3) {
      if constexpr (M::dose) {
        acc[c][k3] = cmake(0.f, 0.f);
        mh[c][k3] = full_dose_mh(kx0 + c, tid + 256 * k3, W, H, pixel_size, vscale);
      }
      if constexpr (M::plain) pacc[c][k3] = cmake(0.f, 0.f);
    }
  for (int j = 0; j < nframes; ++j) {
    const cfloat* base = S + (int64_t)j * sf + (int64_t)kx0 * sc;
    cfloat v[NC][16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      if constexpr (NC == 2) {
        const float4 q = *reinterpret_cast<const float4*>(base + (int64_t)(256 * n1 + tid) * sr);
        v[0][n1] = cmake(q.x, q.y);
        v[1][n1] = cmake(q.z, q.w);
      } else {
        v[0][n1] = base[(int64_t)(256 * n1 + tid) * sr];
      }
    }
    const float dose = pre_exposure + dose_per_frame * (float)(frame0 + j + 1);
    float sy = 0.f, sx = 0.f;
    if constexpr (M::ramp) {
      sy = shifts[2 * j];
      sx = shifts[2 * j + 1];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float fx = (float)(kx0 + c) * (float)(1.0 / (double)W);
      auto in = [&](int n1, int) { return v[c][n1]; };
      auto take = [&](int k, cfloat x) {
        const int k3 = (k - tid) >> 8;
        if constexpr (M::ramp) x = full_ramp(x, k, H, fx, sy, sx);
        if constexpr (M::plain) {
          pacc[c][k3].x += x.x;
          pacc[c][k3].y += x.y;
        }
        if constexpr (M::dose) {
          const float q = expf(mh[c][k3] * dose);
          acc[c][k3].x += q * x.x;
          acc[c][k3].y += q * x.y;
        }
      };
      wg_fft4096_r16<-1, 8, 8>(line, tid, tw_col, in, take);
      __syncthreads();
    }
  }
  auto finish = [&](auto& ac, cfloat* out, auto weighted) {
    cfloat* abase = out + kx0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int k3 = 0; k3 < 16; ++k3) {
        cfloat a = ac[c][k3];
        if (!first) {
          const cfloat prev = abase[(int64_t)(tid + 256 * k3) * pitch + c];
          a.x += prev.x;
          a.y += prev.y;
        }
        if (last) {
          float r = scale;
          if constexpr (decltype(weighted)::value) {
            float qq = 0.f;
            for (int f = 0; f < total_frames; ++f) {
              const float q = expf(mh[c][k3] * (pre_exposure + dose_per_frame * (float)(f + 1)));
              qq += q * q;
            }
            r = scale / sqrtf(qq);
          }
          if constexpr (M::ramp) {
            a.x *= r;
            a.y *= r;
          } else {  // rounded on its own, not fused into the inverse transform's first butterfly: the
                    // bits of the exposure-weighted sum this pass replaced
#pragma clang fp contract(off)
            a.x *= r;
            a.y *= r;
          }
        }
        ac[c][k3] = a;
      }
    if (last) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        auto in = [&](int n1, int) { return ac[c][n1]; };
        auto back = [&](int k, cfloat x) { ac[c][(k - tid) >> 8] = x; };
        wg_fft4096_r16<+1, 8, 8>(line, tid, tw_col, in, back);
        __syncthreads();
      }
    }
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      if constexpr (NC == 2)
        *reinterpret_cast<float4*>(abase + (int64_t)(256 * n1 + tid) * pitch) =
            make_float4(ac[0][n1].x, ac[0][n1].y, ac[1][n1].x, ac[1][n1].y);
      else
        abase[(int64_t)(256 * n1 + tid) * pitch] = ac[0][n1];
    }
  };
  if constexpr (M::dose) finish(acc, A, std::true_type{});
  if constexpr (M::plain) finish(pacc, P, std::false_type{});
}

// Hot pixels of a raw row pass (RawMovie's sorted list, keys = f H W + y W + x relative to the chunk's
// first frame, rv = {replacement, value} of raw * gain): full_rows_fwd_raw transformed v - mu_f at such a
// pixel, the conditioned movie holds r - mu_f, so every bin of its row gains
//   (r - v) exp(-2 pi i kx x / W),  kx = 0 .. W/2  (the forward rfft convention: no scale, negative exponent).
// As xc_rows_hot_fix: one workgroup per (frame, row) segment of the list -- the workgroup of the segment's
// first entry; the others return at once -- so every bin is written by one workgroup, in list order, and
// kx x is reduced mod W in integers before the angle.
__global__ __launch_bounds__(256) void full_rows_hot_fix(const long long* __restrict__ keys,
                                                         const float2* __restrict__ rv, int64_t n, int frame0,
                                                         int njobs, int H, int W, cfloat* __restrict__ S, int pitch) {
  const int64_t e0 = blockIdx.x;
  if (e0 >= n) return;
  const long long seg = keys[e0] / W;  // f * H + y
  if (e0 > 0 && keys[e0 - 1] / W == seg) return;
  const int f = (int)(seg / H), y = (int)(seg - (long long)f * H);
  if (f < frame0 || f >= frame0 + njobs) return;
  cfloat* row = S + ((int64_t)(f - frame0) * H + y) * pitch;
  for (int kx = threadIdx.x; kx <= W / 2; kx += 256) {
    float ar = 0.f, ai = 0.f;
    for (int64_t e = e0; e < n && keys[e] / W == seg; ++e) {
      const int x = (int)(keys[e] - seg * W);
      const float2 p = rv[e];
      const float d = p.x - p.y;
      const int ph = (int)(((int64_t)kx * x) % W);  // exact phase index; the angle in revolutions ph / W
      const float rev = (float)ph / (float)W;        // in [0, 1): v_sin / v_cos take revolutions
      ar += d * __builtin_amdgcn_cosf(rev);
      ai -= d * __builtin_amdgcn_sinf(rev);
    }
    row[kx].x += ar;
    row[kx].y += ai;
  }
}

template <int MODE>
static int full_cols_shift_sum_launch(const void* S, const float* shifts, int nframes, int frame0, int total_frames,
                                      void* A, void* P, const void* tw_col, int H, int W, int pitch, float pixel_size,
                                      float pre_exposure, float dose_per_frame, float vscale, int first, int last,
                                      float scale, int64_t sf, int64_t sr, int64_t sc, void* stream) {
  if (H == 4096) {
    hipLaunchKernelGGL((full_cols_shift_sum_r16<1, MODE>), dim3(pitch), dim3(MC_WG), 0, (hipStream_t)stream,
                       (const cfloat*)S, shifts, nframes, frame0, total_frames, (cfloat*)A, (cfloat*)P, W, pitch,
                       (const cfloat*)tw_col, pixel_size, pre_exposure, dose_per_frame, vscale, first, last, scale, sf,
                       sr, sc);
    return mc_check_launch();
  }
  MC_FULL_DISPATCH_COLS(H, {
    constexpr int NC = (L & (L - 1)) ? 1 : full_nc<L>(), WG = full_wg<L>();
    if constexpr (MODE == 3) {
      return MC_ERR_UNSUPPORTED;  // not instantiated: see full_cols_shift_sum_impl
    } else {
      auto k = full_cols_shift_sum<L, NC, WG, MODE>;
      const size_t lds = NC * sizeof(cfloat) * (size_t)lds_len(L) + ((L & (L - 1)) ? sizeof(float) * (size_t)L : 0);
      MC_SET_LDS(k, lds);
      hipLaunchKernelGGL(k, dim3(pitch / NC), dim3(WG), lds, (hipStream_t)stream, (const cfloat*)S, shifts, nframes,
                         frame0, total_frames, (cfloat*)A, (cfloat*)P, W, pitch, (const cfloat*)tw_col, pixel_size,
                         pre_exposure, dose_per_frame, vscale, first, last, scale, sf, sr, sc);
    }
  });
  return mc_check_launch();
}

static int full_cols_shift_sum_impl(const void* S, bool colmajor, const float* shifts, int nframes, int frame0,
                                    int total_frames, void* A, void* P, const void* tw_col, int H, int W, int pitch,
                                    float pixel_size, float pre_exposure, float dose_per_frame, float voltage,
                                    int first, int last, float scale, void* stream) {
  if (!S || (!A && !P) || !tw_col || nframes < 1 || frame0 < 0 || total_frames < frame0 + nframes)
    return MC_ERR_ARG;
  if (!shifts && P) return MC_ERR_ARG;  // no phase ramp: the exposure-weighted sum alone
  if (A && !(pixel_size > 0.f && dose_per_frame >= 0.f)) return MC_ERR_ARG;
  if (!full_sizes_ok(H, W, pitch)) return MC_ERR_UNSUPPORTED;
  if (colmajor && H != 4096 && H != 4092 && H != 8184) return MC_ERR_UNSUPPORTED;
  const float vscale = voltage >= 300.f ? 1.0f : (voltage >= 200.f ? 0.8f : 0.75f);
  const int64_t sf = colmajor ? (int64_t)(W / 2 + 1) * H : (int64_t)H * pitch;
  const int64_t sr = colmajor ? 1 : pitch, sc = colmajor ? H : 1;
#define MC_SHIFT_SUM(MODE, AA, PP)                                                                                   \
  full_cols_shift_sum_launch<MODE>(S, shifts, nframes, frame0, total_frames, AA, PP, tw_col, H, W, pitch, pixel_size, \
                                   pre_exposure, dose_per_frame, vscale, first, last, scale, sf, sr, sc, stream)
  if (A && P) {
    // Both sums from one read of the spectra: the register-resident 4096-row kernel (252 VGPRs, two waves per
    // SIMD as the exposure-weighted pass alone: 207).  The staged kernels take one launch per sum and read the spectra twice:
    // on the mixed-radix columns (one column per workgroup, already register-bound) both accumulators spill
    // (8184 rows) or fall to one wave per SIMD (4092); on the power-of-two columns the kernel with both
    // accumulators live rounds the plain sum differently in its last bits (1024 rows), and the plain sum
    // must be the bits of the plain-only pass.
    if (H != 4096) {
      const int rc = MC_SHIFT_SUM(2, A, nullptr);
      return rc != MC_OK ? rc : MC_SHIFT_SUM(1, nullptr, P);
    }
    return MC_SHIFT_SUM(3, A, P);
  }
  if (!shifts) return MC_SHIFT_SUM(2 | FULL_NO_RAMP, A, nullptr);
  return A ? MC_SHIFT_SUM(2, A, nullptr) : MC_SHIFT_SUM(1, nullptr, P);
#undef MC_SHIFT_SUM
}

extern "C" {

int mc_full_rows_forward_raw(const void* raw, int kind, const float* gain, const float* mu, const int64_t* job_off,
                             void* S, const void* tw_row, int njobs, int H, int W, int pitch, void* stream) {
  if (!raw || !gain || !mu || !job_off || !S || !tw_row || njobs < 1) return MC_ERR_ARG;
  if (kind != 0 && kind != 1) return MC_ERR_UNSUPPORTED;  // u8 / i16; fp16 / fp32 movies: condition them first
  // pairs of samples and of gain values per load: 2- / 4-byte aligned raw rows, 8-byte aligned gain rows
  if (!full_sizes_ok(H, W, pitch) || (reinterpret_cast<uintptr_t>(raw) & (kind == 0 ? 1 : 3)) ||
      (reinterpret_cast<uintptr_t>(gain) & 7))
    return MC_ERR_UNSUPPORTED;
  MC_FULL_DISPATCH_ROWS(W / 2, {
    mc_pick(kind == 1, [&](auto I16) {  // KIND 0 u8, 1 i16
      hipLaunchKernelGGL((full_rows_fwd_raw<L, I16.value ? 1 : 0>), full_rows_grid(H, njobs), dim3(MC_WG), 0,
                         (hipStream_t)stream, raw, gain, mu, job_off, (cfloat*)S, H, pitch, (const cfloat*)tw_row,
                         FULL_ROWS_PER_WG);
    });
  });
  return mc_check_launch();
}

int mc_full_rows_hot_correct(const long long* keys, const float* rv, int64_t n, int frame0, int njobs, int H, int W,
                             void* S, int pitch, void* stream) {
  if (!S || n < 0 || (n > 0 && (!keys || !rv)) || frame0 < 0 || njobs < 1 || H < 1 || W < 2 || n > 0x7fffffffLL)
    return MC_ERR_ARG;
  if (!full_sizes_ok(H, W, pitch) || (reinterpret_cast<uintptr_t>(rv) & 7)) return MC_ERR_UNSUPPORTED;
  if (n == 0) return MC_OK;
  hipLaunchKernelGGL(full_rows_hot_fix, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, keys, (const float2*)rv,
                     n, frame0, njobs, H, W, (cfloat*)S, pitch);
  return mc_check_launch();
}

int mc_full_cols_shift_sum(const void* S, const float* shifts, int nframes, int frame0, int total_frames, void* A,
                           void* P, const void* tw_col, int H, int W, int pitch, float pixel_size, float pre_exposure,
                           float dose_per_frame, float voltage, int first, int last, float scale, void* stream) {
  return full_cols_shift_sum_impl(S, false, shifts, nframes, frame0, total_frames, A, P, tw_col, H, W, pitch,
                                  pixel_size, pre_exposure, dose_per_frame, voltage, first, last, scale, stream);
}

int mc_full_cols_shift_sum_cm(const void* ST, const float* shifts, int nframes, int frame0, int total_frames, void* A,
                              void* P, const void* tw_col, int H, int W, int pitch, float pixel_size,
                              float pre_exposure, float dose_per_frame, float voltage, int first, int last, float scale,
                              void* stream) {
  return full_cols_shift_sum_impl(ST, true, shifts, nframes, frame0, total_frames, A, P, tw_col, H, W, pitch,
                                  pixel_size, pre_exposure, dose_per_frame, voltage, first, last, scale, stream);
}

}  // extern "C"
