// Generic-length engine (xcg_common.h): the inverse row pass, with the arg-max fused or the rows stored.
#include "xcg_common.h"

template <int LOGM, int EPI>
__global__ __launch_bounds__(MC_WG) void xcg_rows_inv(
    const cfloat* __restrict__ T2, const float* __restrict__ bounds, int* __restrict__ best,
    float* __restrict__ part_val, int* __restrict__ part_idx, float* __restrict__ out_real,
    const int64_t* __restrict__ out_off, int64_t out_stride, const cfloat* __restrict__ tw_row,
    XcLine ln, XcGeom g, int near, int phase) {
  constexpr int M = mc_line_m(LOGM);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cfloat* line = reinterpret_cast<cfloat*>(smem);
  cfloat* stg = line + lds_len(M);
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  const int RG = g.RG, n = ln.n;
  const int ngrp = g.H / RG;
  int grp = blockIdx.x;
  if (EPI == 0) grp = phase == 0 ? ((int)blockIdx.x < near ? (int)blockIdx.x : ngrp - 2 * near + (int)blockIdx.x)
                                 : near + (int)blockIdx.x;
  if constexpr (EPI == 0) {
    if (phase == 1) {
      float b = 0.f;
      for (int r = 0; r < RG; ++r) b = fmaxf(b, bounds[(int64_t)p * g.H + grp * RG + r]);
      b = b * 1.0001f + 1e-30f;
      if (float_order(b) < __hip_atomic_load(&best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (tid == 0) {
          part_val[(int64_t)p * ngrp + grp] = -INFINITY;
          part_idx[(int64_t)p * ngrp + grp] = 0x7fffffff;
        }
        return;
      }
    }
  }
  const cfloat* in = T2 + (int64_t)p * g.nkx * g.H + (int64_t)grp * RG;
  for (int i = tid; i < g.nkx * RG; i += MC_WG) {
    const int kx = i / RG, r = i - kx * RG;
    stg[kx * (RG + 1) + r] = in[(int64_t)kx * g.H + r];
  }
  __syncthreads();
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int r = 0; r < RG; ++r) {
    const int y = grp * RG + r;
    if (g.W & 1) {
      // odd width: the full Hermitian line of W points, X[W - k] = conj(X[k]); outputs are real
      auto load1 = [&](int k) {
        cfloat v = cmake(0.f, 0.f);
        if (k < g.nkx) {
          v = stg[k * (RG + 1) + r];
          if (k == 0) v.y = 0.f;
        } else if (n - k < g.nkx) {
          v = cconj(stg[(n - k) * (RG + 1) + r]);
        }
        return v;
      };
      if constexpr (EPI == 0) {
        auto store1 = [&](int j, cfloat v) { cand_merge(bv, bi, v.x, y * g.W + j); };
        xcg_line_fft<LOGM, +1>(line, tid, ln, n, load1, store1);
      } else {
        float* orow = out_real + out_off[p] + (int64_t)y * out_stride;
        auto store1 = [&](int j, cfloat v) { orow[j] = v.x; };
        xcg_line_fft<LOGM, +1>(line, tid, ln, n, load1, store1);
      }
      __syncthreads();
      continue;
    }
    // c2r pack for a real row of even length W = 2n (same identity as the 2^k path)
    auto load = [&](int k) {
      const int km = n - k;  // in [1, n]
      cfloat xk = (k < g.nkx) ? stg[k * (RG + 1) + r] : cmake(0.f, 0.f);
      cfloat xm = (km < g.nkx) ? cconj(stg[km * (RG + 1) + r]) : cmake(0.f, 0.f);
      if (k == 0) {
        xk.y = 0.f;
        xm.y = 0.f;
      }
      const cfloat sm = cadd(xk, xm), d = csub(xk, xm);
      cfloat w = tw_row[k];
      w.y = -w.y;
      const cfloat wd = cmul(w, d);
      return cmake(sm.x - wd.y, sm.y + wd.x);
    };
    if constexpr (EPI == 0) {
      auto store = [&](int j, cfloat v) {
        const int flat = y * g.W + 2 * j;
        cand_merge(bv, bi, v.x, flat);
        cand_merge(bv, bi, v.y, flat + 1);
      };
      xcg_line_fft<LOGM, +1>(line, tid, ln, n, load, store);
    } else {
      float* orow = out_real + out_off[p] + (int64_t)y * out_stride;
      auto store = [&](int j, cfloat v) {
        orow[2 * j] = v.x;
        orow[2 * j + 1] = v.y;
      };
      xcg_line_fft<LOGM, +1>(line, tid, ln, n, load, store);
    }
    __syncthreads();
  }
  if constexpr (EPI == 0) {
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_down(bv, off);
      const int oi = __shfl_down(bi, off);
      cand_merge(bv, bi, ov, oi);
    }
    __shared__ float wv[MC_WG / 64];
    __shared__ int wi[MC_WG / 64];
    if ((tid & 63) == 0) {
      wv[tid >> 6] = bv;
      wi[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < MC_WG / 64; ++w) cand_merge(bv, bi, wv[w], wi[w]);
      part_val[(int64_t)p * ngrp + grp] = bv;
      part_idx[(int64_t)p * ngrp + grp] = bi;
      atomicMax(&best[p], float_order(bv));
    }
  }
}

extern "C" {

int mc_xcg_rows_inverse(const void* T2, float* part_val, int* part_idx, int* peaks, float* shifts,
                        float* out, const int64_t* out_off, int64_t out_stride, const void* tw_row,
                        const mc_xc_line* line, int npairs, const mc_xc_geom* q, void* stream) {
  XcGeom g; XcLine ln; int logm;
  int rc = geom_from_g(q, &g);
  if (rc) return rc;
  if ((rc = line_from(line, (g.W & 1) ? g.W : g.W / 2, &ln, &logm))) return rc;
  if (!T2 || !tw_row || npairs < 1) return MC_ERR_ARG;
  const bool store = out != nullptr;
  if (store ? !out_off : (!part_val || !part_idx || !peaks || !shifts)) return MC_ERR_ARG;
  const size_t lds = sizeof(cfloat) * ((size_t)lds_len(line->M) + (size_t)g.nkx * (g.RG + 1));
  if (lds > 160 * 1024) return MC_ERR_ARG;
  const int ngrp = g.H / g.RG;
  if (store) {
    MC_DISPATCH_LOGM(logm, {
      auto k = xcg_rows_inv<L, 1>;
      MC_SET_LDS(k, lds);
      hipLaunchKernelGGL(k, dim3(ngrp, npairs), dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)T2,
                         (const float*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, out, out_off,
                         out_stride, (const cfloat*)tw_row, ln, g, 0, 0);
    });
    return mc_check_launch();
  }
  int* best = part_idx + (int64_t)npairs * ngrp;
  {
    const float ninf = -INFINITY;
    int pat;
    memcpy(&pat, &ninf, 4);
    pat = pat >= 0 ? pat : pat ^ 0x7fffffff;
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)best, pat, npairs, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  const int near = xc_near_groups(g);
  float* bounds = part_val + (int64_t)npairs * ngrp;
  if (ngrp - 2 * near > 0)
    mc_launch_row_bounds((const cfloat*)T2, bounds, g.nkx, g.H, npairs, (hipStream_t)stream);
  MC_DISPATCH_LOGM(logm, {
    auto k = xcg_rows_inv<L, 0>;
    MC_SET_LDS(k, lds);
    if (near > 0)
      hipLaunchKernelGGL(k, dim3(2 * near, npairs), dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)T2,
                         (const float*)bounds, best, part_val, part_idx, (float*)nullptr,
                         (const int64_t*)nullptr, (int64_t)0, (const cfloat*)tw_row, ln, g, near, 0);
    if (ngrp - 2 * near > 0)
      hipLaunchKernelGGL(k, dim3(ngrp - 2 * near, npairs), dim3(MC_WG), lds, (hipStream_t)stream,
                         (const cfloat*)T2, (const float*)bounds, best, part_val, part_idx, (float*)nullptr,
                         (const int64_t*)nullptr, (int64_t)0, (const cfloat*)tw_row, ln, g, near, 1);
  });
  rc = mc_check_launch();
  if (rc) return rc;
  mc_launch_peak_final(part_val, part_idx, ngrp, g.H, g.W, peaks, shifts, nullptr, npairs, (hipStream_t)stream);
  return mc_check_launch();
}

}  // extern "C"
