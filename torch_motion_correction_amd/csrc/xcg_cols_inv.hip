// Generic-length engine (xcg_common.h): the inverse column pass (correlation product or Fourier shift).
#include "xcg_common.h"

// MODE 0: conj(ref)*cur; MODE 1: cur * exp(-2 pi i (fy sy + fx sx)) (Fourier shift)
template <int LOGM, int MODE>
__global__ __launch_bounds__(MC_WG) void xcg_cols_inv(
    const cfloat* __restrict__ S_cur, const int* __restrict__ cur_idx,
    const cfloat* __restrict__ S_ref, const int* __restrict__ ref_idx,
    const float* __restrict__ shifts, cfloat* __restrict__ T2, float scale, XcLine ln, XcGeom g) {
  constexpr int M = mc_line_m(LOGM);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cfloat* line = reinterpret_cast<cfloat*>(smem);
  const int tid = threadIdx.x;
  const int kx = blockIdx.x, p = blockIdx.y;
  const int H = g.H, nky = g.kyp + g.kyn;
  const cfloat* cur = S_cur + ((int64_t)cur_idx[p] * g.nkx + kx) * nky;
  const cfloat* ref = MODE == 0 ? S_ref + ((int64_t)ref_idx[p] * g.nkx + kx) * nky : nullptr;
  cfloat* out = T2 + ((int64_t)p * g.nkx + kx) * H;
  float sy = 0.f, sx = 0.f, fx = 0.f;
  if (MODE == 1) {
    sy = shifts[2 * p];
    sx = shifts[2 * p + 1];
    fx = (float)kx * (float)(1.0 / (double)g.W);  // torch.fft.rfftfreq: k * (1/n)
  }
  auto load = [&](int ky) {
    const int kyi = kept_index(ky, H, g.kyp, g.kyn);
    if (kyi < 0) return cmake(0.f, 0.f);
    cfloat v;
    if (MODE == 0) {
      v = cmulc(ref[kyi], cur[kyi]);
    } else {
      const int kk = (ky < (H + 1) / 2) ? ky : ky - H;
      const float fy = (float)kk * (float)(1.0 / (double)H);
      const float m2pi = -6.283185307179586f;
      const float ang = (m2pi * fy) * sy + (m2pi * fx) * sx;
      float sn, cs;
      sincosf(ang, &sn, &cs);
      v = cmul(cur[kyi], cmake(cs, sn));
    }
    return cscale(v, scale);
  };
  auto store = [&](int y, cfloat v) { out[y] = v; };
  xcg_line_fft<LOGM, +1>(line, tid, ln, H, load, store);
}

extern "C" {

int mc_xcg_cols_inverse(const void* S_cur, const int* cur_idx, const void* S_ref,
                        const int* ref_idx, const float* shifts, void* T2, const mc_xc_line* line,
                        float scale, int npairs, const mc_xc_geom* q, void* stream) {
  XcGeom g; XcLine ln; int logm;
  int rc = geom_from_g(q, &g);
  if (rc) return rc;
  if ((rc = line_from(line, g.H, &ln, &logm))) return rc;
  if (!S_cur || !cur_idx || !T2 || npairs < 1 || (!shifts && (!S_ref || !ref_idx))) return MC_ERR_ARG;
  const size_t lds = sizeof(cfloat) * (size_t)lds_len(line->M);
  dim3 grid(g.nkx, npairs);
  MC_DISPATCH_LOGM(logm, {
    if (shifts) {
      auto k = xcg_cols_inv<L, 1>;
      MC_SET_LDS(k, lds);
      hipLaunchKernelGGL(k, grid, dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)S_cur, cur_idx,
                         (const cfloat*)nullptr, (const int*)nullptr, shifts, (cfloat*)T2, scale, ln, g);
    } else {
      auto k = xcg_cols_inv<L, 0>;
      MC_SET_LDS(k, lds);
      hipLaunchKernelGGL(k, grid, dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)S_cur, cur_idx,
                         (const cfloat*)S_ref, ref_idx, (const float*)nullptr, (cfloat*)T2, scale, ln, g);
    }
  });
  return mc_check_launch();
}

}  // extern "C"
