// Conditioning of raw detector movies (mc_condition_movie), the statistics of the fused raw path
// (mc_raw_movie_stats) and the frame statistics of fp32 / fp16 stacks (central-box moments, normalize,
// frame sum): the passes that reduce or rescale whole frames.  Hot pixels are in hot_pixels.hip.
// The sums follow a fixed fp32 / double operation order, without FMA contraction.
#include "cond_common.h"
#include "mcorr.h"
#pragma clang fp contract(off)

// ------------------------------------------------------------------ input conditioning
// The caller-side preparation of the reference's pipeline (examples/ttMotion.py:90-121 gain
// multiply, :174-199 per-frame mean-zero) for raw detector frames of any storage type:
//   out[f] = raw[f] * gain - mean(raw[f] * gain)      (fp32 out; gain / mean-zero optional)
// pass 1 accumulates the per-frame sums in double, pass 2 applies.  KIND: 0 u8, 1 i16, 2 f16, 3 f32.
template <int KIND>
__global__ __launch_bounds__(256) void cond_sum_kernel(const void* __restrict__ raw,
                                                       const float* __restrict__ gain, int64_t hw,
                                                       double* __restrict__ sums) {
  const int f = blockIdx.y;
  const int64_t base = (int64_t)f * hw;
  double s = 0.0;
  float ps = 0.f;
  int n = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const float v = cond_load<KIND>(raw, base + i) * (gain ? gain[i] : 1.f);
    ps += v;
    if (++n == 16) {  // flush the fp32 partial regularly
      s += ps; ps = 0.f; n = 0;
    }
  }
  s += ps;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums[f], part4_sum(part));
}

template <int KIND>
__global__ __launch_bounds__(256) void cond_apply_kernel(const void* __restrict__ raw,
                                                         const float* __restrict__ gain, int64_t hw,
                                                         const double* __restrict__ sums,
                                                         float* __restrict__ out) {
  const int f = blockIdx.y;
  const int64_t base = (int64_t)f * hw;
  const float mean = sums ? (float)(sums[f] / (double)hw) : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256)
    out[base + i] = cond_load<KIND>(raw, base + i) * (gain ? gain[i] : 1.f) - mean;
}

template <int KIND, bool APPLY>
__global__ __launch_bounds__(256) void cond_vec_kernel(const void* __restrict__ raw,
                                                       const float* __restrict__ gain, int64_t hw,
                                                       int nframes, double* __restrict__ sums,
                                                       float* __restrict__ out) {
  const int f0 = blockIdx.y * COND_FR;
  float mean[COND_FR];
  double s[COND_FR];
#pragma unroll
  for (int ff = 0; ff < COND_FR; ++ff) {
    s[ff] = 0.0;
    mean[ff] = (APPLY && sums && f0 + ff < nframes) ? (float)(sums[f0 + ff] / (double)hw) : 0.f;
  }
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < hw; i += (int64_t)gridDim.x * 256 * 8) {
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = 1.f;
    if (gain) cond_gain8(gain, i, g);
#pragma unroll
    for (int ff = 0; ff < COND_FR; ++ff) {
      if (f0 + ff >= nframes) break;
      const int64_t base = (int64_t)(f0 + ff) * hw;
      float v[8];
      cond_load8<KIND>(raw, base + i, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] *= g[k];
      if (APPLY) {
        const float m = mean[ff];
        float* o = out + base + i;
        *reinterpret_cast<float4*>(o) = make_float4(v[0] - m, v[1] - m, v[2] - m, v[3] - m);
        *reinterpret_cast<float4*>(o + 4) = make_float4(v[4] - m, v[5] - m, v[6] - m, v[7] - m);
      } else {
        s[ff] += (double)(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
      }
    }
  }
  if (!APPLY) {
    __shared__ double part[COND_FR][4];
#pragma unroll
    for (int ff = 0; ff < COND_FR; ++ff) {
      double r = s[ff];
      for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off);
      if ((threadIdx.x & 63) == 0) part[ff][threadIdx.x >> 6] = r;
    }
    __syncthreads();
    if (threadIdx.x < COND_FR && f0 + (int)threadIdx.x < nframes) {
      const int ff = threadIdx.x;
      atomicAdd(&sums[f0 + ff], part4_sum(part[ff]));
    }
  }
}

// ------------------------------------------------------------------ N2: statistics of a RAW movie
// The fused raw path (mc_xc_rows_forward_raw, mc_warp_rigid_raw) never materialises the conditioned
// movie c_f = raw_f * gain - mu_f (examples/ttMotion.py:90-121, 180-199).  One pass over the raw bytes
// gives everything the estimator and the warp need to condition on the fly:
//   stats[f] = { sum_all v, sum_box v, sum_box v^2 },  v = raw * gain,  box = normalize_image's central box
// and raw_stats_finalize turns them into mu_f (the frame means, as mc_condition_movie rounds them), the
// joint central-box mean and unbiased standard deviation of the CONDITIONED frames (utils.py:76-84:
// sum_box (v - mu_f) = S_box - n mu_f, sum_box (v - mu_f)^2 = Q_box - 2 mu_f S_box + n mu_f^2, in double) and
// the per-frame offset sub_f = mu_f + mean that K1 subtracts.  The gain tile of a pixel group is held in
// registers over COND_FR frames, as in cond_vec_kernel.
template <int KIND>
__global__ __launch_bounds__(256) void raw_stats_kernel(const void* __restrict__ raw, const float* __restrict__ gain,
                                                        int h, int w, int nframes, int hl, int hu, int wl, int wu,
                                                        double* __restrict__ stats) {
  const int f0 = blockIdx.y * COND_FR;
  const int64_t hw = (int64_t)h * w;
  double sa[COND_FR], sb[COND_FR], qb[COND_FR];
#pragma unroll
  for (int ff = 0; ff < COND_FR; ++ff) sa[ff] = sb[ff] = qb[ff] = 0.0;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < hw; i += (int64_t)gridDim.x * 256 * 8) {
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = 1.f;
    if (gain) cond_gain8(gain, i, g);
    // w % 8 == 0 (host): the 8 pixels lie in one row; box weights per pixel, the same for every frame
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    float bw[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bw[k] = (y >= hl && y < hu && x + k >= wl && x + k < wu) ? 1.f : 0.f;
    const bool any_box = y >= hl && y < hu && x + 7 >= wl && x < wu;
#pragma unroll
    for (int ff = 0; ff < COND_FR; ++ff) {
      if (f0 + ff >= nframes) break;
      float v[8];
      cond_load8<KIND>(raw, (int64_t)(f0 + ff) * hw + i, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] *= g[k];
      sa[ff] += (double)(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
      if (any_box) {
        float ps = 0.f, pq = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          ps = __builtin_fmaf(bw[k], v[k], ps);
          pq = __builtin_fmaf(bw[k] * v[k], v[k], pq);
        }
        sb[ff] += (double)ps;
        qb[ff] += (double)pq;
      }
    }
  }
  __shared__ double part[COND_FR][3][4];
#pragma unroll
  for (int ff = 0; ff < COND_FR; ++ff) {
    double r0 = sa[ff], r1 = sb[ff], r2 = qb[ff];
    for (int off = 32; off > 0; off >>= 1) {
      r0 += __shfl_down(r0, off);
      r1 += __shfl_down(r1, off);
      r2 += __shfl_down(r2, off);
    }
    if ((threadIdx.x & 63) == 0) {
      part[ff][0][threadIdx.x >> 6] = r0;
      part[ff][1][threadIdx.x >> 6] = r1;
      part[ff][2][threadIdx.x >> 6] = r2;
    }
  }
  __syncthreads();
  if (threadIdx.x < COND_FR * 3) {
    const int ff = threadIdx.x / 3, c = threadIdx.x - 3 * ff;
    if (f0 + ff < nframes) atomicAdd(&stats[3 * (f0 + ff) + c], part4_sum(part[ff][c]));
  }
}

// scalar form for shapes the vector kernel does not take (w % 8 != 0 or unaligned buffers)
template <int KIND>
__global__ __launch_bounds__(256) void raw_stats_scalar_kernel(const void* __restrict__ raw,
                                                               const float* __restrict__ gain, int h, int w, int hl,
                                                               int hu, int wl, int wu, double* __restrict__ stats) {
  const int f = blockIdx.y;
  const int64_t hw = (int64_t)h * w, base = (int64_t)f * hw;
  double sa = 0.0, sb = 0.0, qb = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const float v = cond_load<KIND>(raw, base + i) * (gain ? gain[i] : 1.f);
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    sa += (double)v;
    if (y >= hl && y < hu && x >= wl && x < wu) {
      sb += (double)v;
      qb += (double)v * (double)v;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sa += __shfl_down(sa, off);
    sb += __shfl_down(sb, off);
    qb += __shfl_down(qb, off);
  }
  __shared__ double part[3][4];
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = sa;
    part[1][threadIdx.x >> 6] = sb;
    part[2][threadIdx.x >> 6] = qb;
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicAdd(&stats[3 * f + threadIdx.x], part4_sum(part[threadIdx.x]));
}

// out: mu[t], sub[t] = mu + mean, mean_rstd[0..1] = {mean, 1 / std} of the conditioned central box
// (all frames jointly, unbiased: torch.std_mean, utils.py:82-83); mean_zero = 0: mu = 0
__global__ void raw_stats_finalize(const double* __restrict__ stats, int nframes, int64_t hw, int64_t nbox,
                                   int mean_zero, float* __restrict__ mu, float* __restrict__ sub,
                                   float* __restrict__ mean_rstd) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double S = 0.0, Q = 0.0;
  for (int f = 0; f < nframes; ++f) {
    const float m = mean_zero ? (float)(stats[3 * f] / (double)hw) : 0.f;  // as mc_condition_movie rounds it
    mu[f] = m;
    const double md = (double)m, sb = stats[3 * f + 1], qb = stats[3 * f + 2];
    S += sb - (double)nbox * md;
    Q += qb - 2.0 * md * sb + (double)nbox * md * md;
  }
  const double N = (double)nbox * nframes;
  const double mean = S / N;
  double var = (Q - N * mean * mean) / (N - 1.0);
  var = var > 0.0 ? var : 0.0;
  const float meanf = (float)mean;
  mean_rstd[0] = meanf;
  mean_rstd[1] = (float)(1.0 / sqrt(var));
  for (int f = 0; f < nframes; ++f) sub[f] = mu[f] + meanf;
}

// ------------------------------------------------------------------ statistics
template <typename T>
__global__ __launch_bounds__(256) void box_stats_partial(const T* __restrict__ stack, int h,
                                                         int w, int hl, int hu, int wl, int wu,
                                                         double* __restrict__ acc) {
  // grid: (row chunks, t); each block reduces rows [r0, r1) of one frame's box
  const int f = blockIdx.y;
  const int rows_per = (hu - hl + gridDim.x - 1) / gridDim.x;
  const int r0 = hl + blockIdx.x * rows_per;
  int r1 = r0 + rows_per;
  if (r1 > hu) r1 = hu;
  const T* frame = stack + (int64_t)f * h * w;
  double s = 0.0, q = 0.0;
  // 4 samples per load when every row segment of the box is aligned to it and a multiple of 4 long
  const bool vec = ((w | wl | (wu - wl)) & 3) == 0 && (reinterpret_cast<uintptr_t>(stack) & 15) == 0 &&
                   ((((int64_t)h * w) & 3) == 0);
  for (int y = r0; y < r1; ++y) {
    const T* row = frame + (int64_t)y * w;
    float ps = 0.f, pq = 0.f;
    int n = 0;
    if (vec) {
      for (int x = wl + 4 * threadIdx.x; x < wu; x += 1024) {
        float4 v;
        if (sizeof(T) == 4) {
          v = *reinterpret_cast<const float4*>(row + x);
        } else {
          typedef _Float16 h4 __attribute__((ext_vector_type(4)));
          const h4 hv = *reinterpret_cast<const h4*>(row + x);
          v = make_float4((float)hv.x, (float)hv.y, (float)hv.z, (float)hv.w);
        }
        ps += (v.x + v.y) + (v.z + v.w);
        pq += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        if (++n == 4) {  // flush the fp32 partials every 16 samples, as the scalar loop does
          s += ps; q += pq; ps = 0.f; pq = 0.f; n = 0;
        }
      }
      s += ps;
      q += pq;
      continue;
    }
    for (int x = wl + threadIdx.x; x < wu; x += 256) {
      const float v = (float)row[x];
      ps += v;
      pq += v * v;
      if (++n == 16) {  // flush the fp32 partials regularly
        s += ps; q += pq; ps = 0.f; pq = 0.f; n = 0;
      }
    }
    s += ps;
    q += pq;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
    q += __shfl_down(q, off);
  }
  __shared__ double ss[4], sq[4];
  if ((threadIdx.x & 63) == 0) {
    ss[threadIdx.x >> 6] = s;
    sq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = ss[0] + ss[1] + ss[2] + ss[3];
    q = sq[0] + sq[1] + sq[2] + sq[3];
    atomicAdd(&acc[0], s);
    atomicAdd(&acc[1], q);
  }
}

__global__ void box_stats_final(const double* __restrict__ acc, double count,
                                float* __restrict__ out3) {
  const double mean = acc[0] / count;
  double var = (acc[1] - acc[0] * acc[0] / count) / (count - 1.0);
  if (var < 0) var = 0;
  const float stdf = (float)sqrt(var);
  out3[0] = (float)mean;
  out3[1] = 1.0f / stdf;
  out3[2] = stdf;
}

__global__ void normalize_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n,
                                 const float* __restrict__ mean_rstd) {
  const float mean = mean_rstd[0], stdv = mean_rstd[2];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dst[i] = (src[i] - mean) / stdv;
}

__global__ void sum_frames_kernel(const float* __restrict__ frames, int nframes, int64_t hw,
                                  float* __restrict__ sum) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < hw; i += stride) {
    if (i + 3 < hw) {
      float4 a = make_float4(0, 0, 0, 0);
      for (int f = 0; f < nframes; ++f) {
        const float4 v = *reinterpret_cast<const float4*>(frames + (int64_t)f * hw + i);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
      *reinterpret_cast<float4*>(sum + i) = a;
    } else {
      for (int64_t j = i; j < hw; ++j) {
        float a = 0;
        for (int f = 0; f < nframes; ++f) a += frames[(int64_t)f * hw + j];
        sum[j] = a;
      }
    }
  }
}

// Which form runs.  The tiled kernels need whole 8-pixel groups per frame and the alignment of their vector
// loads and stores; each entry has its own rule.  mc_condition_movie: any hw that is a multiple of 8 (a
// group may straddle rows), `out` is written as float4, and the tile count must fit the grid arithmetic.
static bool cond_movie_tiled(const void* raw, int kind, const float* gain, const float* out, int64_t hw) {
  return (hw % 8 == 0) && cond_raw_aligned(raw, kind) && cond_f4_aligned(out) && (!gain || cond_f4_aligned(gain)) &&
         hw / 8 / 256 < 0x7fffffff;
}
// mc_raw_movie_stats: the 8 pixels of a group lie in one row of the box test
static bool raw_stats_tiled(const void* raw, int kind, const float* gain, int w) {
  return (w % 8 == 0) && cond_raw_aligned(raw, kind) && (!gain || cond_f4_aligned(gain));
}

void mc_raw_stats_finalize_launch(const double* stats, int nframes, int64_t hw, int64_t nbox, int mean_zero, float* mu,
                                  float* sub, float* mean_rstd, hipStream_t s) {
  hipLaunchKernelGGL(raw_stats_finalize, dim3(1), dim3(64), 0, s, stats, nframes, hw, nbox, mean_zero, mu, sub,
                     mean_rstd);
}

extern "C" {

int mc_condition_movie(const void* raw, int kind, const float* gain, int nframes, int64_t hw,
                       int mean_zero, double* sums, float* out, void* stream) {
  if (!raw || !out || nframes < 1 || hw < 1 || kind < 0 || kind > 3 || (mean_zero && !sums))
    return MC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (mean_zero) {
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(double) * nframes, st);
    if (e != hipSuccess) return (int)e;
  }
  const bool tiled = cond_movie_tiled(raw, kind, gain, out, hw);
  const dim3 grid = tiled ? cond_tiled_grid(hw, nframes) : cond_scalar_grid(hw, nframes);
  mc_pick_kind(kind, [&](auto K) {
    if (tiled) {
      if (mean_zero)
        hipLaunchKernelGGL((cond_vec_kernel<K.value, false>), grid, dim3(256), 0, st, raw, gain, hw, nframes, sums,
                           (float*)nullptr);
      hipLaunchKernelGGL((cond_vec_kernel<K.value, true>), grid, dim3(256), 0, st, raw, gain, hw, nframes,
                         mean_zero ? sums : (double*)nullptr, out);
    } else {
      if (mean_zero) hipLaunchKernelGGL(cond_sum_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, hw, sums);
      hipLaunchKernelGGL(cond_apply_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, hw,
                         mean_zero ? (const double*)sums : (const double*)nullptr, out);
    }
  });
  return mc_check_launch();
}

int mc_raw_movie_stats(const void* raw, int kind, const float* gain, int nframes, int h, int w, int hl, int hu,
                       int wl, int wu, int mean_zero, double* stats, float* mu, float* sub, float* mean_rstd,
                       void* stream) {
  if (!raw || !stats || !mu || !sub || !mean_rstd || nframes < 1 || h < 1 || w < 1) return MC_ERR_ARG;
  if (kind < 0 || kind > 3) return MC_ERR_UNSUPPORTED;
  if (hl < 0 || hu > h || wl < 0 || wu > w || hl >= hu || wl >= wu) return MC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w;
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(double) * 3 * nframes, st);
  if (e != hipSuccess) return (int)e;
  const bool tiled = raw_stats_tiled(raw, kind, gain, w);
  const dim3 grid = tiled ? cond_tiled_grid(hw, nframes) : cond_scalar_grid(hw, nframes);
  mc_pick_kind(kind, [&](auto K) {
    if (tiled)
      hipLaunchKernelGGL(raw_stats_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, h, w, nframes, hl, hu, wl, wu,
                         stats);
    else
      hipLaunchKernelGGL(raw_stats_scalar_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, h, w, hl, hu, wl, wu,
                         stats);
  });
  mc_raw_stats_finalize_launch(stats, nframes, hw, (int64_t)(hu - hl) * (wu - wl), mean_zero, mu, sub, mean_rstd, st);
  return mc_check_launch();
}

int mc_central_box_stats_t(const void* stack, int storage, int t, int h, int w, int hl, int hu, int wl,
                           int wu, double* acc, float* out3, void* stream) {
  if (!stack || !acc || !out3 || t < 1 || hl < 0 || hu > h || wl < 0 || wu > w || hl >= hu ||
      wl >= wu)
    return MC_ERR_ARG;
  if (storage != MC_STORE_F32 && storage != MC_STORE_F16) return MC_ERR_UNSUPPORTED;
  hipError_t e = hipMemsetAsync(acc, 0, 2 * sizeof(double), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  int chunks = (hu - hl + 15) / 16;
  if (chunks > 256) chunks = 256;
  if (storage == MC_STORE_F32)
    hipLaunchKernelGGL(box_stats_partial<float>, dim3(chunks, t), dim3(256), 0, (hipStream_t)stream,
                       (const float*)stack, h, w, hl, hu, wl, wu, acc);
  else
    hipLaunchKernelGGL(box_stats_partial<_Float16>, dim3(chunks, t), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)stack, h, w, hl, hu, wl, wu, acc);
  const double count = (double)t * (hu - hl) * (wu - wl);
  hipLaunchKernelGGL(box_stats_final, dim3(1), dim3(1), 0, (hipStream_t)stream, acc, count, out3);
  return mc_check_launch();
}

int mc_normalize(const float* src, float* dst, int64_t n, const float* mean_rstd, void* stream) {
  if (!src || !dst || !mean_rstd || n < 1) return MC_ERR_ARG;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     src, dst, n, mean_rstd);
  return mc_check_launch();
}

int mc_sum_frames(const float* frames, int nframes, int64_t hw, float* sum, void* stream) {
  if (!frames || !sum || nframes < 1 || hw < 1 || (hw & 3)) return MC_ERR_ARG;
  int64_t blocks = (hw / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(sum_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     frames, nframes, hw, sum);
  return mc_check_launch();
}

}  // extern "C"
