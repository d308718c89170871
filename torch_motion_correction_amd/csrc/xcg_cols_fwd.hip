// Generic-length engine (xcg_common.h): the forward column pass.
#include "xcg_common.h"

template <int LOGM>
__global__ __launch_bounds__(MC_WG) void xcg_cols_fwd(const cfloat* __restrict__ T1,
                                                      const float* __restrict__ filt,
                                                      cfloat* __restrict__ S, XcLine ln, XcGeom g) {
  constexpr int M = mc_line_m(LOGM);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cfloat* line = reinterpret_cast<cfloat*>(smem);
  const int tid = threadIdx.x;
  const int kx = blockIdx.x, job = blockIdx.y;
  const int H = g.H, nky = g.kyp + g.kyn;
  const cfloat* col = T1 + ((int64_t)job * g.nkx + kx) * g.ny;
  cfloat* out = S + ((int64_t)job * g.nkx + kx) * nky;
  const float* f = filt ? filt + (int64_t)kx * nky : nullptr;
  auto load = [&](int y) {
    const int yy = y - g.y0;
    return (yy >= 0 && yy < g.ny) ? col[yy] : cmake(0.f, 0.f);
  };
  auto store = [&](int ky, cfloat v) {
    const int kyi = kept_index(ky, H, g.kyp, g.kyn);
    if (kyi >= 0) out[kyi] = f ? cscale(v, f[kyi]) : v;
  };
  xcg_line_fft<LOGM, -1>(line, tid, ln, H, load, store);
}

extern "C" {

int mc_xcg_cols_forward(const void* T1, const float* filt, void* S, const mc_xc_line* line,
                        int njobs, const mc_xc_geom* q, void* stream) {
  XcGeom g; XcLine ln; int logm;
  int rc = geom_from_g(q, &g);
  if (rc) return rc;
  if ((rc = line_from(line, g.H, &ln, &logm))) return rc;
  if (!T1 || !S || njobs < 1) return MC_ERR_ARG;
  const size_t lds = sizeof(cfloat) * (size_t)lds_len(line->M);
  dim3 grid(g.nkx, njobs);
  MC_DISPATCH_LOGM(logm, {
    auto k = xcg_cols_fwd<L>;
    MC_SET_LDS(k, lds);
    hipLaunchKernelGGL(k, grid, dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)T1, filt,
                       (cfloat*)S, ln, g);
  });
  return mc_check_launch();
}

}  // extern "C"
