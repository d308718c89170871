// Hot-pixel removal of raw movies: the dense form (mc_condition_movie_hot writes the conditioned movie) and
// the sparse form of the fused raw path (detection into a sorted list, the statistics' correction, and the
// sorted scatter-add that applies correction records).  The correction of an engine's own output lives with that
// engine: xc_rows_hot_fix in xc_rows_fwd.hip, full_rows_hot_fix in full_sums.hip, warp_rigid_hot_taps in
// warp_rigid_raw.hip.  Detection and replacement follow a fixed operation order, without FMA contraction.
#include "cond_common.h"
#include "mcorr.h"
#pragma clang fp contract(off)

// ------------------------------------------------------------------ hot pixels
// The example pipeline's remove_hot_pixels (examples/ttMotion.py:127-172) sits between the gain
// multiply and the mean-zero step: per frame, a pixel of v = raw * gain is hot when
// v > mean + thr * std or v < mean - thr * std (numpy mean / population std of the whole frame).
// That DETECTION is deterministic and is reproduced; the example then overwrites each hot pixel
// with a RANDOM one of its neighbours (np.random.choice, in place, so the result also depends on
// the visiting order): no deterministic counterpart exists.  Our rule: the mean of the (up to 8)
// neighbours that are not hot themselves, taken from the frame BEFORE any replacement; the frame
// mean if every neighbour is hot.  The per-frame mean subtracted afterwards is the mean AFTER the
// replacement, as in the example's order of steps.
template <int KIND>
__global__ __launch_bounds__(256) void cond_stats2_kernel(const void* __restrict__ raw,
                                                          const float* __restrict__ gain, int64_t hw,
                                                          double* __restrict__ stats /* [f][3] */) {
  const int f = blockIdx.y;
  const int64_t base = (int64_t)f * hw;
  double s = 0.0, q = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const double v = (double)(cond_load<KIND>(raw, base + i) * (gain ? gain[i] : 1.f));
    s += v;
    q += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
    q += __shfl_down(q, off);
  }
  __shared__ double part[2][4];
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s; part[1][threadIdx.x >> 6] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&stats[3 * f], part4_sum(part[0]));
    atomicAdd(&stats[3 * f + 1], part4_sum(part[1]));
  }
}

struct HotLimits {
  float lo, hi, mean;
};
__device__ __forceinline__ HotLimits hot_limits(const double* stats, int f, int64_t hw, float thr) {
  const double m = stats[3 * f] / (double)hw;
  double var = stats[3 * f + 1] / (double)hw - m * m;
  var = var > 0 ? var : 0;
  const double sd = sqrt(var);
  return HotLimits{(float)(m - (double)thr * sd), (float)(m + (double)thr * sd), (float)m};
}

// value of a hot pixel's replacement (see above); (y, x) inside the frame
template <int KIND>
__device__ __forceinline__ float hot_replacement(const void* raw, const float* gain, int64_t base, int h,
                                                 int w, int y, int x, const HotLimits L) {
  float acc = 0.f;
  int n = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if ((dy | dx) == 0 || yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      const int64_t j = (int64_t)yy * w + xx;
      const float v = cond_load<KIND>(raw, base + j) * (gain ? gain[j] : 1.f);
      if (v > L.hi || v < L.lo) continue;
      acc += v;
      ++n;
    }
  return n ? acc / (float)n : L.mean;
}

// MODE 0: find the hot pixels, accumulate sum(replacement - value) and their number per frame;
// MODE 1: write out = (hot ? replacement : value) - mean_after.
template <int KIND, int MODE>
__global__ __launch_bounds__(256) void cond_hot_kernel(const void* __restrict__ raw,
                                                       const float* __restrict__ gain, int h, int w,
                                                       float thr, int mean_zero, double* __restrict__ stats,
                                                       int* __restrict__ hot_count, float* __restrict__ out) {
  const int f = blockIdx.y;
  const int64_t hw = (int64_t)h * w, base = (int64_t)f * hw;
  const HotLimits L = hot_limits(stats, f, hw, thr);
  const float mean_after = (MODE == 1 && mean_zero) ? (float)((stats[3 * f] + stats[3 * f + 2]) / (double)hw) : 0.f;
  double delta = 0.0;
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    float v = cond_load<KIND>(raw, base + i) * (gain ? gain[i] : 1.f);
    if (v > L.hi || v < L.lo) {
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      const float r = hot_replacement<KIND>(raw, gain, base, h, w, y, x, L);
      if (MODE == 0) { delta += (double)r - (double)v; ++cnt; }
      v = r;
    }
    if (MODE == 1) out[base + i] = v - mean_after;
  }
  if (MODE == 0 && cnt) {  // rare: a handful of pixels per frame
    atomicAdd(&stats[3 * f + 2], delta);
    if (hot_count) atomicAdd(&hot_count[f], cnt);
  }
}

// ------------------------------------------------------------------ N2 + hot pixels: sparse corrections
// The fused raw path with the hot-pixel step (mc_raw_hot_detect ... mc_hot_scatter_add, include/mcorr.h).
// Hot pixels are sparse and the estimator's row transform and the rigid warp are linear in the conditioned
// sample, so the tuned raw kernels run on the UNREPLACED values v and each hot pixel is applied afterwards as
// a correction by delta = r - v (r: its replacement).  Only the statistics must be known beforehand: the
// hot-pixel limits need the whole frame's second moment, the frame means and the box statistics are those
// of the frames after replacement.
//
// pass 1, raw_stats_hot_kernel: raw_stats_kernel's {sum v, sum_box v, sum_box v^2} into stats[f][3] and the
// detection moments {sum v, sum v^2} into hstats[f][3] (cond_stats2_kernel's layout: hot_limits reads it).
// Whole-frame terms are fp32 partial sums of 8 samples, accumulated in double (cond_stats2_kernel sums every
// sample in double: the limits agree to the rounding of those partials, ~1e-11 of the frame's variance).
template <int KIND>
__global__ __launch_bounds__(256) void raw_stats_hot_kernel(const void* __restrict__ raw, const float* __restrict__ gain,
                                                            int h, int w, int nframes, int hl, int hu, int wl, int wu,
                                                            double* __restrict__ stats, double* __restrict__ hstats) {
  const int f0 = blockIdx.y * COND_FR;
  const int64_t hw = (int64_t)h * w;
  double sa[COND_FR], sq[COND_FR], sb[COND_FR], qb[COND_FR];
#pragma unroll
  for (int ff = 0; ff < COND_FR; ++ff) sa[ff] = sq[ff] = sb[ff] = qb[ff] = 0.0;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < hw; i += (int64_t)gridDim.x * 256 * 8) {
    float g[8];
    cond_gain8(gain, i, g);
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
      sq[ff] += (double)(((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) +
                         ((v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7])));
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
  __shared__ double part[COND_FR][4][4];
#pragma unroll
  for (int ff = 0; ff < COND_FR; ++ff) {
    double r0 = sa[ff], r1 = sb[ff], r2 = qb[ff], r3 = sq[ff];
    for (int off = 32; off > 0; off >>= 1) {
      r0 += __shfl_down(r0, off);
      r1 += __shfl_down(r1, off);
      r2 += __shfl_down(r2, off);
      r3 += __shfl_down(r3, off);
    }
    if ((threadIdx.x & 63) == 0) {
      part[ff][0][threadIdx.x >> 6] = r0;
      part[ff][1][threadIdx.x >> 6] = r1;
      part[ff][2][threadIdx.x >> 6] = r2;
      part[ff][3][threadIdx.x >> 6] = r3;
    }
  }
  __syncthreads();
  if (threadIdx.x < COND_FR * 4) {
    const int ff = threadIdx.x / 4, c = threadIdx.x - 4 * ff;
    if (f0 + ff < nframes) {
      const double r = part4_sum(part[ff][c]);
      if (c < 3) atomicAdd(&stats[3 * (f0 + ff) + c], r);
      if (c == 0) atomicAdd(&hstats[3 * (f0 + ff)], r);
      if (c == 3) atomicAdd(&hstats[3 * (f0 + ff) + 1], r);
    }
  }
}

// pass 2: cond_hot_kernel<KIND, 0>'s detection and replacement (hot_limits, hot_replacement: the same rule
// bit for bit), with the gain tile in registers over COND_FR frames as in pass 1.  Every hot pixel takes a
// slot of the list: key = f * h * w + pixel index, rv = {r, v}.  Beyond `cap` slots nothing is written, the
// counter keeps counting (the host sees the overflow).
template <int KIND>
__global__ __launch_bounds__(256) void raw_hot_detect_kernel(const void* __restrict__ raw, const float* __restrict__ gain,
                                                             int h, int w, int nframes, float thr,
                                                             const double* __restrict__ hstats,
                                                             long long* __restrict__ keys, float2* __restrict__ rv,
                                                             long long cap, unsigned long long* __restrict__ counter,
                                                             int* __restrict__ counts) {
  const int f0 = blockIdx.y * COND_FR;
  const int64_t hw = (int64_t)h * w;
  float lo[COND_FR], hi[COND_FR];
#pragma unroll
  for (int ff = 0; ff < COND_FR; ++ff) {
    lo[ff] = hi[ff] = 0.f;
    if (f0 + ff < nframes) {
      const HotLimits L = hot_limits(hstats, f0 + ff, hw, thr);
      lo[ff] = L.lo;
      hi[ff] = L.hi;
    }
  }
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < hw; i += (int64_t)gridDim.x * 256 * 8) {
    float g[8];
    cond_gain8(gain, i, g);
#pragma unroll
    for (int ff = 0; ff < COND_FR; ++ff) {
      if (f0 + ff >= nframes) break;
      const int64_t base = (int64_t)(f0 + ff) * hw;
      float v[8];
      cond_load8<KIND>(raw, base + i, v);
      unsigned hot = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] *= g[k];
        hot |= (v[k] > hi[ff] || v[k] < lo[ff]) ? 1u << k : 0u;
      }
      while (hot) {  // rare: a handful of pixels per frame; the sample is formed again as cond_hot_kernel does
        const int k = __builtin_ctz(hot);
        hot &= hot - 1;
        const int64_t j = i + k;
        const HotLimits L = hot_limits(hstats, f0 + ff, hw, thr);
        const float vk = cond_load<KIND>(raw, base + j) * gain[j];
        const int y = (int)(j / w), x = (int)(j - (int64_t)y * w);
        const float r = hot_replacement<KIND>(raw, gain, base, h, w, y, x, L);
        const unsigned long long slot = atomicAdd(counter, 1ull);
        if (slot < (unsigned long long)cap) {
          keys[slot] = base + j;
          rv[slot] = make_float2(r, vk);
        }
        atomicAdd(&counts[f0 + ff], 1);
      }
    }
  }
}

// first index in keys[0, n) (ascending) that is >= k
__device__ __forceinline__ int64_t hot_lower_bound(const long long* keys, int64_t n, long long k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// pass 3 (list sorted by key): per frame, the corrections of the moments --
//   sum v += sum (r - v);   sum_box v += sum_box (r - v);   sum_box v^2 += sum_box (r^2 - v^2)
// in double; stats[3 f] becomes cond_hot_kernel's sum after replacement (stats[3f] + stats[3f+2] there), so
// raw_stats_finalize rounds mu as mean_after.  One workgroup per frame, entries dealt to the threads in a
// fixed way and a fixed reduction tree: no atomics, the same result every time.
__global__ __launch_bounds__(256) void raw_hot_stats_fix(const long long* __restrict__ keys,
                                                         const float2* __restrict__ rv, int64_t n, int nframes,
                                                         int h, int w, int hl, int hu, int wl, int wu,
                                                         const double* __restrict__ hstats,
                                                         double* __restrict__ stats) {
  const int f = blockIdx.x;
  const int64_t hw = (int64_t)h * w;
  __shared__ int64_t range[2];
  __shared__ double red[3][256];
  if (threadIdx.x < 2) range[threadIdx.x] = hot_lower_bound(keys, n, (long long)(f + threadIdx.x) * hw);
  __syncthreads();
  double d = 0.0, db = 0.0, qb = 0.0;
  for (int64_t e = range[0] + threadIdx.x; e < range[1]; e += 256) {
    const float2 p = rv[e];
    const double r = (double)p.x, v = (double)p.y;
    d += r - v;
    const int64_t j = keys[e] - (long long)f * hw;
    const int y = (int)(j / w), x = (int)(j - (int64_t)y * w);
    if (y >= hl && y < hu && x >= wl && x < wu) {
      db += r - v;
      qb += r * r - v * v;
    }
  }
  red[0][threadIdx.x] = d;
  red[1][threadIdx.x] = db;
  red[2][threadIdx.x] = qb;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[3 * f] = hstats[3 * f] + red[0][0];
    stats[3 * f + 1] += red[1][0];
    stats[3 * f + 2] += red[2][0];
  }
}

// step 2 (records sorted by key, stable): every run of equal keys is summed in order by the thread of its
// first record and added to out[key] -- one writer per output element, a fixed order, no atomics.
__global__ __launch_bounds__(256) void hot_scatter_add(const long long* __restrict__ key, const float* __restrict__ val,
                                                       int64_t m, int64_t limit, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const long long k = key[i];
  if (k < 0 || k >= limit || (i > 0 && key[i - 1] == k)) return;
  float s = 0.f;
  for (int64_t j = i; j < m && key[j] == k; ++j) s += val[j];
  out[k] += s;
}

// mc_raw_hot_detect has the tiled kernels only (whole 8-pixel groups per row, the gain is required and read as
// float4, the list's {r, v} pairs are written as float2); anything else is MC_ERR_UNSUPPORTED
static bool raw_hot_tiled(const void* raw, int kind, const float* gain, const float* rv, int w) {
  return (w % 8 == 0) && cond_raw_aligned(raw, kind) && cond_f4_aligned(gain) &&
         (reinterpret_cast<uintptr_t>(rv) & 7) == 0;
}

extern "C" {

int mc_condition_movie_hot(const void* raw, int kind, const float* gain, int nframes, int h, int w,
                           int mean_zero, float threshold, double* stats, int* hot_count, float* out,
                           void* stream) {
  if (!raw || !out || !stats || nframes < 1 || h < 1 || w < 1 || kind < 0 || kind > 3 || !(threshold > 0.f))
    return MC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w;
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(double) * 3 * nframes, st);
  if (e != hipSuccess) return (int)e;
  if (hot_count) {
    e = hipMemsetAsync(hot_count, 0, sizeof(int) * nframes, st);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid = cond_scalar_grid(hw, nframes);
  mc_pick_kind(kind, [&](auto K) {
    hipLaunchKernelGGL(cond_stats2_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, hw, stats);
    hipLaunchKernelGGL((cond_hot_kernel<K.value, 0>), grid, dim3(256), 0, st, raw, gain, h, w, threshold, mean_zero,
                       stats, hot_count, (float*)nullptr);
    hipLaunchKernelGGL((cond_hot_kernel<K.value, 1>), grid, dim3(256), 0, st, raw, gain, h, w, threshold, mean_zero,
                       stats, (int*)nullptr, out);
  });
  return mc_check_launch();
}

int mc_raw_hot_detect(const void* raw, int kind, const float* gain, int nframes, int h, int w, int hl, int hu,
                      int wl, int wu, float threshold, double* stats, double* hstats, long long* keys, float* rv,
                      long long capacity, unsigned long long* counter, int* counts, void* stream) {
  if (!raw || !gain || !stats || !hstats || !keys || !rv || !counter || !counts || nframes < 1 || h < 1 || w < 1 ||
      capacity < 1 || !(threshold > 0.f) || !(threshold < INFINITY))
    return MC_ERR_ARG;
  if (kind < 0 || kind > 3) return MC_ERR_UNSUPPORTED;
  if (hl < 0 || hu > h || wl < 0 || wu > w || hl >= hu || wl >= wu) return MC_ERR_ARG;
  if (!raw_hot_tiled(raw, kind, gain, rv, w)) return MC_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w;
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(double) * 3 * nframes, st);
  if (e == hipSuccess) e = hipMemsetAsync(hstats, 0, sizeof(double) * 3 * nframes, st);
  if (e == hipSuccess) e = hipMemsetAsync(counter, 0, sizeof(unsigned long long), st);
  if (e == hipSuccess) e = hipMemsetAsync(counts, 0, sizeof(int) * nframes, st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid = cond_tiled_grid(hw, nframes);
  mc_pick_kind(kind, [&](auto K) {
    hipLaunchKernelGGL(raw_stats_hot_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, h, w, nframes, hl, hu, wl,
                       wu, stats, hstats);
    hipLaunchKernelGGL(raw_hot_detect_kernel<K.value>, grid, dim3(256), 0, st, raw, gain, h, w, nframes, threshold,
                       (const double*)hstats, keys, (float2*)rv, capacity, counter, counts);
  });
  return mc_check_launch();
}

int mc_raw_hot_finalize(const long long* keys, const float* rv, int64_t n, int nframes, int h, int w, int hl, int hu,
                        int wl, int wu, int mean_zero, const double* hstats, double* stats, float* mu, float* sub,
                        float* mean_rstd, void* stream) {
  if (!stats || !hstats || !mu || !sub || !mean_rstd || n < 0 || (n > 0 && (!keys || !rv)) || nframes < 1 || h < 1 ||
      w < 1 || hl < 0 || hu > h || wl < 0 || wu > w || hl >= hu || wl >= wu)
    return MC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(raw_hot_stats_fix, dim3(nframes), dim3(256), 0, st, keys, (const float2*)rv, n,
                     nframes, h, w, hl, hu, wl, wu, hstats, stats);
  mc_raw_stats_finalize_launch(stats, nframes, (int64_t)h * w, (int64_t)(hu - hl) * (wu - wl), mean_zero, mu, sub,
                               mean_rstd, st);
  return mc_check_launch();
}

int mc_hot_scatter_add(const long long* key, const float* val, int64_t m, int64_t limit, float* out, void* stream) {
  if (!key || !val || !out || m < 0 || limit < 1) return MC_ERR_ARG;
  if (m == 0) return MC_OK;
  hipLaunchKernelGGL(hot_scatter_add, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, key, val,
                     m, limit, out);
  return mc_check_launch();
}

}  // extern "C"
