// Generic-length engine (xcg_common.h): the forward row pass, also from raw bytes, and the peak neighbourhood.
#include "xcg_common.h"

// K6 for any width: the nine map values around a peak as direct sums over the kept columns,
//   cc(y, x) = sum_kx h(kx) Re(T2[p][kx][y] exp(+2 pi i kx x / W)),
// h = 1 for kx = 0 (and the Nyquist column of an even width), 2 otherwise; the imaginary parts of
// those self-conjugate columns are dropped as a c2r transform drops them.  nkx terms per value:
// nothing to transform for 9 values.  kx x is reduced mod W in integers before the sine.
__global__ __launch_bounds__(MC_WG) void xcg_peak_nbhd(const cfloat* __restrict__ T2, const int* __restrict__ peaks,
                                                       float* __restrict__ nb, XcGeom g) {
  const int tid = threadIdx.x;
  const int p = blockIdx.y, dy = (int)blockIdx.x - 1;
  const int pk = peaks[p];
  const int py = pk / g.W, px = pk - py * g.W;
  const int y = py + dy;
  float* o = nb + (int64_t)p * 9 + (dy + 1) * 3;
  if (y < 0 || y >= g.H) {
    if (tid < 3) o[tid] = __builtin_nanf("");
    return;
  }
  const cfloat* in = T2 + (int64_t)p * g.nkx * g.H + y;
  float acc[3] = {0.f, 0.f, 0.f};
  const float invw = 1.0f / (float)g.W;
  for (int kx = tid; kx < g.nkx; kx += MC_WG) {
    cfloat v = in[(int64_t)kx * g.H];
    const bool self = kx == 0 || (!(g.W & 1) && kx == g.W / 2);
    if (self) v.y = 0.f;
    const float hk = self ? 1.f : 2.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int x = px + i - 1;
      if (x < 0 || x >= g.W) continue;
      const int r = (int)(((int64_t)kx * x) % g.W);
      float sn, cs;
      sincospif(2.0f * (float)r * invw, &sn, &cs);
      acc[i] += hk * (v.x * cs - v.y * sn);
    }
  }
  __shared__ float part[3][MC_WG / 64];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float a = acc[i];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if ((tid & 63) == 0) part[i][tid >> 6] = a;
  }
  __syncthreads();
  if (tid < 3) {
    const int x = px + tid - 1;
    float v = __builtin_nanf("");
    if (x >= 0 && x < g.W) {
      v = 0.f;
      for (int w = 0; w < MC_WG / 64; ++w) v += part[tid][w];
    }
    o[tid] = v;
  }
}

// RAW (N2): 1 = u8, 2 = i16 samples conditioned on the fly as raw * gain - job_sub[job] (`gain` has the
// frames' row pitch: whole-frame jobs; mc_raw_movie_stats supplies job_sub and mean_rstd[1])
template <int LOGM, int RAW = 0>
__global__ __launch_bounds__(MC_WG) void xcg_rows_fwd(
    const void* __restrict__ src_any, const int64_t* __restrict__ job_off, int64_t row_stride,
    const int* __restrict__ job_expo, const float* __restrict__ mask,
    const float* __restrict__ mean_rstd, cfloat* __restrict__ T1,
    const cfloat* __restrict__ tw_row, XcLine ln, XcGeom g, const float* __restrict__ gain,
    const float* __restrict__ job_sub) {
  constexpr int M = mc_line_m(LOGM);
  // direct (mixed-radix) lines: the transform's outputs go back into the line itself and the unpack
  // reads Z[k], Z[n-k] from it -- no zlo / zhi copies: 48 instead of 57 KB of LDS for 5760-column
  // frames, i.e. three workgroups per CU instead of two (the kernel is latency-bound)
  constexpr bool DIRECT = mc_line_direct(LOGM);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cfloat* line = reinterpret_cast<cfloat*>(smem);
  cfloat* zlo = line + lds_len(M);       // Z[k], k < nkx
  cfloat* zhi = zlo + (g.nkx + 1);       // Z[n-k] at index k, 1 <= k <= nkx
  cfloat* stg = DIRECT ? line + lds_len(M) : zhi + (g.nkx + 1);
  const int tid = threadIdx.x;
  const int job = blockIdx.x, grp = blockIdx.y;
  const int RG = g.RG, n = ln.n;
  const float mean = RAW ? job_sub[job] : (mean_rstd ? mean_rstd[0] : 0.f);
  const float rstd = mean_rstd ? mean_rstd[1] : 1.f;
  const int expo = job_expo ? job_expo[job] : (mask ? 1 : 0);
  constexpr int SB = RAW == 1 ? 1 : RAW == 2 ? 2 : 4;
  const char* base = static_cast<const char*>(src_any) + job_off[job] * SB;
  for (int r = 0; r < RG; ++r) {
    const int y = g.y0 + grp * RG + r;
    const char* rowb = base + (int64_t)y * row_stride * SB;
    const float* grow = RAW ? gain + (int64_t)y * row_stride : nullptr;
    // one sample as the estimator sees it: the fp32 frame, or raw * gain (the mean comes off below)
    auto row_at = [&](int x) -> float {
      if constexpr (RAW == 1) return (float)reinterpret_cast<const unsigned char*>(rowb)[x] * grow[x];
      else if constexpr (RAW == 2) return (float)reinterpret_cast<const short*>(rowb)[x] * grow[x];
      else return reinterpret_cast<const float*>(rowb)[x];
    };
    const float* mrow = mask + (int64_t)y * g.W;
    if (g.W & 1) {
      // odd width: no two-samples-per-point packing; the row is a length-W complex line with zero
      // imaginary parts and the wanted bins are the first nkx outputs as they are
      auto load1 = [&](int x) {
        cfloat v = cmake(0.f, 0.f);
        if (x >= g.x0 && x < g.x1) {
          v.x = (row_at(x) - mean) * rstd;
          if (expo > 0) {
            const float m0 = mrow[x];
            for (int e = 0; e < expo; ++e) v.x *= m0;
          }
        }
        return v;
      };
      auto store1 = [&](int k, cfloat v) {
        if (k < g.nkx) stg[k * (RG + 1) + r] = v;
      };
      xcg_line_fft<LOGM, -1>(line, tid, ln, n, load1, store1, ln.keep);
      __syncthreads();
      continue;
    }
    auto load = [&](int j) {
      const int x = 2 * j;
      cfloat v = cmake(0.f, 0.f);
      if (x >= g.x0 && x < g.x1) {
        v = cmake((row_at(x) - mean) * rstd, (row_at(x + 1) - mean) * rstd);
        if (expo > 0) {
          const float m0 = mrow[x], m1 = mrow[x + 1];
          for (int e = 0; e < expo; ++e) {
            v.x *= m0;
            v.y *= m1;
          }
        }
      }
      return v;
    };
    auto store = [&](int k, cfloat v) {
      if constexpr (DIRECT) {
        line[lpad(k)] = v;  // the last pass has read all its inputs before it stores (smooth_rec)
      } else {
        if (k < g.nkx) zlo[k] = v;
        if (k > 0 && n - k <= g.nkx) zhi[n - k] = v;
      }
    };
    xcg_line_fft<LOGM, -1>(line, tid, ln, n, load, store, ln.keep);
    __syncthreads();
    for (int k = tid; k < g.nkx; k += MC_WG) {
      cfloat zk, zm;
      if constexpr (DIRECT) {
        zk = line[lpad(k < n ? k : 0)];                       // Z[n] == Z[0]
        zm = cconj(line[lpad((k == 0 || k == n) ? 0 : n - k)]);  // Z[n-k]
      } else {
        zk = (k < n) ? zlo[k] : zlo[0];
        zm = cconj((k == 0 || k == n) ? zlo[0] : zhi[k]);
      }
      const cfloat sm = cadd(zk, zm), d = csub(zk, zm);
      const cfloat w = (k < n) ? tw_row[k] : cmake(-1.f, 0.f);
      const cfloat wd = cmul(w, d);
      stg[k * (RG + 1) + r] = cmake(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));
    }
    __syncthreads();
  }
  cfloat* out = T1 + (int64_t)job * g.nkx * g.ny + (int64_t)grp * RG;
  for (int i = tid; i < g.nkx * RG; i += MC_WG) {
    const int kx = i / RG, r = i - kx * RG;
    out[(int64_t)kx * g.ny + r] = stg[kx * (RG + 1) + r];
  }
}

extern "C" {

int mc_xcg_peak_neighbourhood(const void* T2, const int* peaks, float* nb, int npairs, const mc_xc_geom* q,
                              void* stream) {
  XcGeom g;
  int rc = geom_from_g(q, &g);
  if (rc) return rc;
  if (!T2 || !peaks || !nb || npairs < 1) return MC_ERR_ARG;
  hipLaunchKernelGGL(xcg_peak_nbhd, dim3(3, npairs), dim3(MC_WG), 0, (hipStream_t)stream, (const cfloat*)T2, peaks,
                     nb, g);
  return mc_check_launch();
}

int mc_xcg_rows_forward(const float* src, const int64_t* job_off, int64_t row_stride,
                        const int* job_expo, const float* mask, const float* mean_rstd, void* T1,
                        const void* tw_row, const mc_xc_line* line, int njobs, const mc_xc_geom* q,
                        void* stream) {
  XcGeom g; XcLine ln; int logm;
  int rc = geom_from_g(q, &g);
  if (rc) return rc;
  // rows forward needs Z[k] for k < nkx and Z[n - k] for 1 <= k <= nkx: keep >= nkx + 1
  if ((rc = line_from(line, (g.W & 1) ? g.W : g.W / 2, &ln, &logm, true, (g.W & 1) ? g.nkx : g.nkx + 1))) return rc;
  if (!src || !job_off || !T1 || !tw_row || njobs < 1) return MC_ERR_ARG;
  const size_t lds = sizeof(cfloat) * ((size_t)lds_len(line->M) + (mc_line_direct(logm) ? 0 : 2 * (g.nkx + 1)) +
                                       (size_t)g.nkx * (g.RG + 1));
  if (lds > 160 * 1024) return MC_ERR_ARG;
  dim3 grid(njobs, g.ny / g.RG);
  MC_DISPATCH_LOGM(logm, {
    auto k = xcg_rows_fwd<L>;
    MC_SET_LDS(k, lds);
    hipLaunchKernelGGL(k, grid, dim3(MC_WG), lds, (hipStream_t)stream, (const void*)src, job_off, row_stride,
                       job_expo, mask, mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, ln, g, (const float*)nullptr,
                       (const float*)nullptr);
  });
  return mc_check_launch();
}

// N2: the same row pass from the raw bytes of a u8 / i16 movie (whole-frame jobs), for the K3 formats: rows of
// 5760 / 11520 samples (direct mixed-radix lines of 2880 / 5760 points).  Other lengths: MC_ERR_UNSUPPORTED.
int mc_xcg_rows_forward_raw(const void* raw, int storage, const float* gain, const int64_t* job_off,
                            int64_t row_stride, const float* mask, const float* job_sub, const float* mean_rstd,
                            void* T1, const void* tw_row, const mc_xc_line* line, int njobs, const mc_xc_geom* q,
                            void* stream) {
  if (storage != MC_STORE_U8 && storage != MC_STORE_I16) return MC_ERR_UNSUPPORTED;
  XcGeom g; XcLine ln; int logm;
  int rc = geom_from_g(q, &g);
  if (rc) return rc;
  if (g.W & 1) return MC_ERR_UNSUPPORTED;
  if ((rc = line_from(line, g.W / 2, &ln, &logm, true, g.nkx + 1))) return rc;
  if (!raw || !gain || !job_off || !mask || !job_sub || !mean_rstd || !T1 || !tw_row || njobs < 1) return MC_ERR_ARG;
  if (logm != 22 && logm != 23) return MC_ERR_UNSUPPORTED;
  const size_t lds = sizeof(cfloat) * ((size_t)lds_len(line->M) + (size_t)g.nkx * (g.RG + 1));
  if (lds > 160 * 1024) return MC_ERR_ARG;
  dim3 grid(njobs, g.ny / g.RG);
  mc_pick(logm == 23, [&](auto L23) {
    mc_pick(storage == MC_STORE_I16, [&](auto I16) {
      auto k = xcg_rows_fwd<L23.value ? 23 : 22, I16.value ? 2 : 1>;
      MC_SET_LDS(k, lds);
      hipLaunchKernelGGL(k, grid, dim3(MC_WG), lds, (hipStream_t)stream, raw, job_off, row_stride,
                         (const int*)nullptr, mask, mean_rstd, (cfloat*)T1, (const cfloat*)tw_row, ln, g, gain, job_sub);
    });
  });
  return mc_check_launch();
}

}  // extern "C"
