// libmcorr -- iterative sub-pixel whole-frame alignment (refine_global_motion): the two kernels an
// iteration adds to the existing correlation search.
//
// The filtered, pruned spectra S[f][kx][ky] of the global estimate stay in HBM; an iteration never
// reads a frame again.  With s_f the current shift of frame f in pixels (y, x):
//     G_f   = S_f exp(+2 pi i (fy sy_f + fx sx_f))      (the ramp correct_motion_fast applies for the field s)
//     A     = sum_f G_f,       REF_f = (A - G_f) / (t - 1)   (mean of the OTHER aligned frames)
//     c_f   = irfft2(conj(REF_f) G_f);   r_f = first maximum (wrap-around rule) + parabola offsets
//     s_f  += (t - 1)/t r_f;   s -= s_ref                 (r_f overstates the frame's own error by t/(t-1))
// xc_aligned_refs forms G and REF; the correlation, the arg-max and the 3 x 3 values around the peak are
// the existing K3/K4/K6 kernels with cur = G, ref = REF; xc_refine_update forms r, the damped update,
// the re-centring and max |r|.
//
// The existing neighbourhood kernels return NaN outside the map and a converged residual peaks at
// (0, 0).  The map is therefore translated: the `cur` spectra are written UNDER-corrected by `under`
// pixels on both axes, G'_f = G_f exp(-2 pi i under (fy + fx)), which moves every peak by exactly
// (under, under) -- a circular translate of c_f, equal to the circular definition up to fp32 rounding
// -- and xc_refine_update takes it off again.  REF is formed from the true G.
//
// xc_aligned_refs is bound by its bytes: t * nbins * 8 B read twice (the second time from L2 /
// the Infinity Cache) and 2 * t * nbins * 8 B written.
#pragma clang fp contract(off)
#include "mc_common.h"
#include "mcorr.h"

#define XR_WG 256
#define XR_MAXT 512

// e^{2 pi i rev}: the angle is reduced in revolutions (v_fract) and goes to the transcendental unit as it is
__device__ __forceinline__ cfloat xr_cis(float rev) {
  const float r = __builtin_amdgcn_fractf(rev);
  return cmake(__builtin_amdgcn_cosf(r), __builtin_amdgcn_sinf(r));
}

// a * b with both fmas written out (one rounding of each product, the same in every instantiation)
__device__ __forceinline__ cfloat xr_cmul(cfloat a, cfloat b) {
  return cmake(__builtin_fmaf(-a.y, b.y, a.x * b.x), __builtin_fmaf(a.y, b.x, a.x * b.y));
}

__device__ __forceinline__ cfloat xr_aligned(cfloat s, float fyk, float fxk, float sy, float sx) {
  return xr_cmul(s, xr_cmul(xr_cis(fyk * sy), xr_cis(fxk * sx)));  // separable ramp: e^{i phi_y(ky)} e^{i phi_x(kx)}
}

// One thread per bin k = kx * nky + ky (consecutive lanes: consecutive ky, one coalesced run per frame).
// shifts is read with wave-uniform indices: scalar loads, no LDS.
__global__ __launch_bounds__(XR_WG) void xc_aligned_refs(const cfloat* __restrict__ S,
                                                         const float* __restrict__ shifts,
                                                         const float* __restrict__ fy,
                                                         const float* __restrict__ fx, cfloat* __restrict__ G,
                                                         cfloat* __restrict__ REF, int t, int nky, int64_t nbins,
                                                         float under) {
  const int64_t k = (int64_t)blockIdx.x * XR_WG + threadIdx.x;
  if (k >= nbins) return;
  const int kx = (int)(k / nky), ky = (int)(k - (int64_t)kx * nky);
  const float fyk = fy[ky], fxk = fx[kx];
  cfloat A = cmake(0.f, 0.f);
#pragma unroll 4
  for (int f = 0; f < t; ++f) {
    const cfloat g = xr_aligned(S[(int64_t)f * nbins + k], fyk, fxk, shifts[2 * f], shifts[2 * f + 1]);
    A.x += g.x;
    A.y += g.y;
  }
  const float inv = t > 1 ? 1.f / (float)(t - 1) : 0.f;
  const cfloat E = xr_cmul(xr_cis(-(fyk * under)), xr_cis(-(fxk * under)));
#pragma unroll 4
  for (int f = 0; f < t; ++f) {
    const cfloat g = xr_aligned(S[(int64_t)f * nbins + k], fyk, fxk, shifts[2 * f], shifts[2 * f + 1]);
    G[(int64_t)f * nbins + k] = xr_cmul(g, E);
    REF[(int64_t)f * nbins + k] = cmake((A.x - g.x) * inv, (A.y - g.y) * inv);
  }
}

// r_f, the damped update, the re-centring and max |r|: one workgroup, one thread per frame.
// Parabola rules of field_accumulate (estimate_motion_xc.py:465-481, the `!=` guards included), the three
// samples per axis taken circularly: after the translate by `under` they lie inside the map whenever
// -under < r < n - 1 - under; a peak ON the map's border (a residual that large) has NaN neighbours
// there and keeps its integer residual for this iteration.
__global__ __launch_bounds__(XR_MAXT) void xc_refine_update(const int* __restrict__ peaks,
                                                            const float* __restrict__ nb,
                                                            float* __restrict__ shifts, int ref, int t, int H,
                                                            int W, int under, float damp,
                                                            float* __restrict__ max_r) {
  __shared__ float red[XR_MAXT / 64];
  __shared__ float sref[2];
  const int f = threadIdx.x;
  float ry = 0.f, rx = 0.f, sy = 0.f, sx = 0.f;
  if (f < t) {
    const int pk = peaks[f];
    int iy = pk / W, ix = pk - iy * W;
    iy -= under;
    ix -= under;
    if (iy < 0) iy += H;
    if (ix < 0) ix += W;
    ry = (float)(iy <= H / 2 ? iy : iy - H);
    rx = (float)(ix <= W / 2 ? ix : ix - W);
    const float* q = nb + (int64_t)f * 9;
    float v0 = q[1], v1 = q[4], v2 = q[7];  // column through the peak
    if (v0 == v0 && v2 == v2 && v2 != v0) ry += (0.5f * (v0 - v2)) / ((v0 - 2.f * v1) + v2);
    v0 = q[3]; v1 = q[4]; v2 = q[5];        // row through the peak
    if (v0 == v0 && v2 == v2 && v2 != v0) rx += (0.5f * (v0 - v2)) / ((v0 - 2.f * v1) + v2);
    sy = shifts[2 * f] + damp * ry;
    sx = shifts[2 * f + 1] + damp * rx;
    if (f == ref) { sref[0] = sy; sref[1] = sx; }
  }
  float m = fmaxf(fabsf(ry), fabsf(rx));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((f & 63) == 0) red[f >> 6] = m;
  __syncthreads();
  if (f < t) {
    shifts[2 * f] = f == ref ? 0.f : sy - sref[0];
    shifts[2 * f + 1] = f == ref ? 0.f : sx - sref[1];
  }
  if (f == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, red[w]);
    *max_r = m;
  }
}

extern "C" {

int mc_xc_aligned_refs(const void* S, const float* shifts_px, const float* fy, const float* fx, void* G, void* REF,
                       int t, int nkx, int nky, int under_px, void* stream) {
  if (!S || !shifts_px || !fy || !fx || !G || !REF) return MC_ERR_ARG;
  if (t < 1 || t > XR_MAXT || nkx < 1 || nky < 1 || under_px < 0) return MC_ERR_ARG;
  const int64_t nbins = (int64_t)nkx * nky;
  const int64_t nblk = (nbins + XR_WG - 1) / XR_WG;
  if (nblk > 0x7fffffff) return MC_ERR_ARG;
  hipLaunchKernelGGL(xc_aligned_refs, dim3((unsigned)nblk), dim3(XR_WG), 0, (hipStream_t)stream, (const cfloat*)S,
                     shifts_px, fy, fx, (cfloat*)G, (cfloat*)REF, t, nky, nbins, (float)under_px);
  return mc_check_launch();
}

int mc_xc_refine_update(const int* peaks, const float* nb, float* shifts_px, int ref, int t, int H, int W,
                        int under_px, float* max_r, void* stream) {
  if (!peaks || !nb || !shifts_px || !max_r) return MC_ERR_ARG;
  if (t < 2 || t > XR_MAXT || ref < 0 || ref >= t || H < 2 || W < 2) return MC_ERR_ARG;
  if (under_px < 0 || under_px >= H || under_px >= W) return MC_ERR_ARG;
  const int threads = ((t + 63) / 64) * 64;
  hipLaunchKernelGGL(xc_refine_update, dim3(1), dim3(threads), 0, (hipStream_t)stream, peaks, nb, shifts_px, ref, t,
                     H, W, under_px, (float)(t - 1) / (float)t, max_r);
  return mc_check_launch();
}

}  // extern "C"
