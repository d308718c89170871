// libmcorr -- iterative sub-pixel PATCH alignment (refine_local_motion): the two kernels an iteration adds to
// the existing correlation search, with one shift per (frame, patch).  xc_refine.hip has the scheme for one
// shift per frame; the arithmetic of a bin and of a residual is the same here, statement for statement.
//
// The filtered, pruned patch spectra S[f][q][kx][ky] (job = f * npatch + q, as the patch estimator's K1 / K2
// write them) stay in HBM; an iteration never reads a frame.  The window of job (f, q) was cut at the patch
// origin + o[f][q] whole pixels, which is the translate by o already; with s the current shift in px (y, x):
//     G[f,q]   = S[f,q] exp(+2 pi i (fy (sy - oy) + fx (sx - ox)))
//     REF[f,q] = (sum_g G[g,q] - G[f,q]) / (t - 1)
//     r[f,q]   = first maximum of irfft2(conj(REF) G) (wrap-around rule) + parabola offsets
//     s[f,q]  += (t - 1)/t r[f,q];   s[:,q] -= s[ref,q]
// Patches are independent: both kernels take a range [q0, q0 + nq) of patches, and G' / REF hold that range
// only, [f][q - q0][bin] (pair index f * nq + (q - q0) for K3 / K4 / K6).  G' is G under-corrected by `under`
// px on both axes, as in xc_aligned_refs, so that the unchanged neighbourhood kernels see the peak inside the
// map; REF is formed from the true G.
//
// xc_aligned_refs_patches is bound by its bytes: t * nq * nbins * 8 B read twice and twice that written.  A
// workgroup re-reads exactly the 256 bins x t frames it has just read (2 KB x t); the patch is the slow grid
// dimension, so the workgroups in flight cover a few patches' spectra at a time.
#pragma clang fp contract(off)
#include "mc_common.h"
#include "mcorr.h"

#define XP_WG 256
#define XP_MAXT 512

// e^{2 pi i rev}: the angle is reduced in revolutions (v_fract) and goes to the transcendental unit as it is
__device__ __forceinline__ cfloat xp_cis(float rev) {
  const float r = __builtin_amdgcn_fractf(rev);
  return cmake(__builtin_amdgcn_cosf(r), __builtin_amdgcn_sinf(r));
}

// a * b with both fmas written out (one rounding of each product, the same in every instantiation)
__device__ __forceinline__ cfloat xp_cmul(cfloat a, cfloat b) {
  return cmake(__builtin_fmaf(-a.y, b.y, a.x * b.x), __builtin_fmaf(a.y, b.x, a.x * b.y));
}

__device__ __forceinline__ cfloat xp_aligned(cfloat s, float fyk, float fxk, float sy, float sx) {
  return xp_cmul(s, xp_cmul(xp_cis(fyk * sy), xp_cis(fxk * sx)));  // separable ramp: e^{i phi_y(ky)} e^{i phi_x(kx)}
}

// grid (bins / 256, nq): one thread per bin k = kx * nky + ky (consecutive lanes: consecutive ky), one grid row
// per patch, so shifts and offsets are read with wave-uniform indices (scalar loads, no LDS).  s - o is exact
// in fp32 whenever |s - o| < |s| (a multiple of ulp(s)); the frame stride of S is npatch * nbins.
__global__ __launch_bounds__(XP_WG) void xc_aligned_refs_patches(
    const cfloat* __restrict__ S, const float* __restrict__ shifts, const float* __restrict__ offsets,
    const float* __restrict__ fy, const float* __restrict__ fx, cfloat* __restrict__ G, cfloat* __restrict__ REF,
    int t, int nky, int nbins, int npatch, int q0, int nq, float under) {
  const int k = blockIdx.x * XP_WG + threadIdx.x;
  if (k >= nbins) return;
  const int qc = blockIdx.y, q = q0 + qc;
  const int kx = k / nky, ky = k - kx * nky;
  const float fyk = fy[ky], fxk = fx[kx];
  const cfloat* Sq = S + (int64_t)q * nbins + k;
  const int64_t sstride = (int64_t)npatch * nbins, ostride = (int64_t)nq * nbins;
  const float* sh = shifts + 2 * (int64_t)q;
  const float* of = offsets + 2 * (int64_t)q;
  const int64_t hstride = 2 * (int64_t)npatch;
  cfloat A = cmake(0.f, 0.f);
#pragma unroll 4
  for (int f = 0; f < t; ++f) {
    const float dy = sh[f * hstride] - of[f * hstride], dx = sh[f * hstride + 1] - of[f * hstride + 1];
    const cfloat g = xp_aligned(Sq[f * sstride], fyk, fxk, dy, dx);
    A.x += g.x;
    A.y += g.y;
  }
  const float inv = t > 1 ? 1.f / (float)(t - 1) : 0.f;
  const cfloat E = xp_cmul(xp_cis(-(fyk * under)), xp_cis(-(fxk * under)));
  cfloat* Gq = G + (int64_t)qc * nbins + k;
  cfloat* Rq = REF + (int64_t)qc * nbins + k;
#pragma unroll 4
  for (int f = 0; f < t; ++f) {
    const float dy = sh[f * hstride] - of[f * hstride], dx = sh[f * hstride + 1] - of[f * hstride + 1];
    const cfloat g = xp_aligned(Sq[f * sstride], fyk, fxk, dy, dx);
    Gq[f * ostride] = xp_cmul(g, E);
    Rq[f * ostride] = cmake((A.x - g.x) * inv, (A.y - g.y) * inv);
  }
}

// One workgroup per patch of the range, one thread per frame: r, the damped update, the re-centring on `ref`
// and the patch's max |r|.  Parabola rules of field_accumulate (estimate_motion_xc.py:465-481, the `!=` guards
// included), the three samples per axis taken circularly: after the translate by `under` they lie inside the
// map whenever -under < r < n - 1 - under; a peak ON the map's border has NaN neighbours there and keeps its
// integer residual for this iteration.
__global__ __launch_bounds__(XP_MAXT) void xc_refine_update_patches(
    const int* __restrict__ peaks, const float* __restrict__ nb, float* __restrict__ shifts, int ref, int t,
    int npatch, int q0, int nq, int H, int W, int under, float damp, float* __restrict__ max_r) {
  __shared__ float red[XP_MAXT / 64];
  __shared__ float sref[2];
  const int f = threadIdx.x;
  const int qc = blockIdx.x, q = q0 + qc;
  float* sh = shifts + 2 * ((int64_t)f * npatch + q);
  float ry = 0.f, rx = 0.f, sy = 0.f, sx = 0.f;
  if (f < t) {
    const int64_t pair = (int64_t)f * nq + qc;
    const int pk = peaks[pair];
    int iy = pk / W, ix = pk - iy * W;
    iy -= under;
    ix -= under;
    if (iy < 0) iy += H;
    if (ix < 0) ix += W;
    ry = (float)(iy <= H / 2 ? iy : iy - H);
    rx = (float)(ix <= W / 2 ? ix : ix - W);
    const float* v = nb + pair * 9;
    float v0 = v[1], v1 = v[4], v2 = v[7];  // column through the peak
    if (v0 == v0 && v2 == v2 && v2 != v0) ry += (0.5f * (v0 - v2)) / ((v0 - 2.f * v1) + v2);
    v0 = v[3]; v1 = v[4]; v2 = v[5];        // row through the peak
    if (v0 == v0 && v2 == v2 && v2 != v0) rx += (0.5f * (v0 - v2)) / ((v0 - 2.f * v1) + v2);
    sy = sh[0] + damp * ry;
    sx = sh[1] + damp * rx;
    if (f == ref) { sref[0] = sy; sref[1] = sx; }
  }
  float m = fmaxf(fabsf(ry), fabsf(rx));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((f & 63) == 0) red[f >> 6] = m;
  __syncthreads();
  if (f < t) {
    sh[0] = f == ref ? 0.f : sy - sref[0];
    sh[1] = f == ref ? 0.f : sx - sref[1];
  }
  if (f == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, red[w]);
    max_r[q] = m;
  }
}

extern "C" {

int mc_xc_aligned_refs_patches(const void* S, const float* shifts_px, const float* offsets_px, const float* fy,
                               const float* fx, void* G, void* REF, int t, int npatch, int q0, int nq, int nkx,
                               int nky, int under_px, void* stream) {
  if (!S || !shifts_px || !offsets_px || !fy || !fx || !G || !REF) return MC_ERR_ARG;
  if (t < 1 || t > XP_MAXT || nkx < 1 || nky < 1 || under_px < 0) return MC_ERR_ARG;
  if (npatch < 1 || q0 < 0 || nq < 1 || nq > 65535 || (int64_t)q0 + nq > npatch) return MC_ERR_ARG;
  const int64_t nbins = (int64_t)nkx * nky;
  if (nbins > 0x7fffffff - XP_WG) return MC_ERR_ARG;
  const int64_t nblk = (nbins + XP_WG - 1) / XP_WG;
  hipLaunchKernelGGL(xc_aligned_refs_patches, dim3((unsigned)nblk, (unsigned)nq), dim3(XP_WG), 0,
                     (hipStream_t)stream, (const cfloat*)S, shifts_px, offsets_px, fy, fx, (cfloat*)G, (cfloat*)REF,
                     t, nky, (int)nbins, npatch, q0, nq, (float)under_px);
  return mc_check_launch();
}

int mc_xc_refine_update_patches(const int* peaks, const float* nb, float* shifts_px, int ref, int t, int npatch,
                                int q0, int nq, int H, int W, int under_px, float* max_r, void* stream) {
  if (!peaks || !nb || !shifts_px || !max_r) return MC_ERR_ARG;
  if (t < 2 || t > XP_MAXT || ref < 0 || ref >= t || H < 2 || W < 2) return MC_ERR_ARG;
  if (npatch < 1 || q0 < 0 || nq < 1 || (int64_t)q0 + nq > npatch) return MC_ERR_ARG;
  if (under_px < 0 || under_px >= H || under_px >= W) return MC_ERR_ARG;
  const int threads = ((t + 63) / 64) * 64;
  hipLaunchKernelGGL(xc_refine_update_patches, dim3((unsigned)nq), dim3(threads), 0, (hipStream_t)stream, peaks, nb,
                     shifts_px, ref, t, npatch, q0, nq, H, W, under_px, (float)(t - 1) / (float)t, max_r);
  return mc_check_launch();
}

}  // extern "C"
