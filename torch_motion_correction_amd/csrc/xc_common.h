// Types and host helpers shared by the pruned, separable 2-D real FFT engines of the cross-correlation shift
// search (reference: estimate_motion_xc.py:76-123 for whole frames, :338-355 for patches): xc_rows_fwd*.hip,
// xc_cols.hip and xc_search.hip (power-of-two lengths) and xcg_*.hip over xcg_common.h (any other length: mixed radix /
// chirp-z).
//
// The reference materialises full spectra and full correlation maps.  Here the binary band-pass
// (utils.py:104-112) and the finite support of the circular mask (xc.py:69-74) are exploited exactly:
// spectrum bins the band-pass zeroes are never produced (only nkx columns and kyp+kyn rows are kept) and
// image rows/columns the mask zeroes are never read.  Zero contributions are skipped, nothing is approximated.
//
//   K1 xc_rows_fwd   rows:  gather + (x-mean)*rstd*mask^e -> real FFT(W) -> first nkx bins
//                           -> T1[job][kx][ysupport]            (transposed via LDS)      xc_rows_fwd.hip
//                           (entry points and route rules over xc_rows_fwd.h; one object per engine:
//                           xc_rows_fwd_wg.hip, xc_rows_fwd_wave.hip, xc_rows_fwd_wave512.hip)
//   K2 xc_cols_fwd   cols:  T1 column -> FFT(H) -> kept ky rows * filter -> S[job][kx][kyi]   xc_cols.hip
//   K3 xc_cols_inv   cols:  conj(S_ref)*S_cur -> inverse FFT(H) -> T2[pair][kx][y]            xc_cols.hip
//   K4 xc_rows_inv   rows:  T2 rows -> inverse real FFT(W) -> fused arg-max | store           xc_search.hip
//   K5 xc_peak_final       reduce K4's per-workgroup candidates, decode wrap-around           xc_search.hip
//   K6 xc_peak_nbhd        re-evaluate rows y-1,y,y+1 of one map for the parabola fit         xc_search.hip
#pragma once
#include <string.h>
#include "mc_fft.h"
#include "mcorr.h"

struct XcGeom {
  int W, H;      // transform size
  int nkx;       // kept rfft columns [0, nkx)
  int kyp, kyn;  // kept ky rows [0, kyp) and [H-kyn, H); nky = kyp + kyn
  int y0, ny;    // rows [y0, y0+ny) of the window can be non-zero (ny % RG == 0)
  int x0, x1;    // columns [x0, x1) can be non-zero (both even)
  int RG;        // rows per workgroup in K1/K4
};

struct XcBox {  // central box of normalize_image (utils.py:76-81) in window coordinates
  int hl, hu, wl, wu;
};

// index of fft row ky among the kept rows [0, kyp) + [H - kyn, H), or -1
__device__ __forceinline__ int kept_index(int ky, int H, int kyp, int kyn) {
  if (ky < kyp) return ky;
  if (ky >= H - kyn) return ky - (H - kyn) + kyp;
  return -1;
}

struct PeakCand {
  float v;
  int idx;
};
__device__ __forceinline__ void cand_merge(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__device__ __forceinline__ int float_order(float f) {  // order-preserving float -> int
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}

#define MC_DISPATCH_CASE(V, ...) \
  case V: {                      \
    constexpr int L = V;         \
    __VA_ARGS__;                 \
  } break;
// the power-of-two engines: log2 of a line's complex length, 16 .. 4096 points
#define MC_DISPATCH_LOG(LOGV, ...)          \
  switch (LOGV) {                           \
    MC_DISPATCH_CASE(4, __VA_ARGS__)        \
    MC_DISPATCH_CASE(5, __VA_ARGS__)        \
    MC_DISPATCH_CASE(6, __VA_ARGS__)        \
    MC_DISPATCH_CASE(7, __VA_ARGS__)        \
    MC_DISPATCH_CASE(8, __VA_ARGS__)        \
    MC_DISPATCH_CASE(9, __VA_ARGS__)        \
    MC_DISPATCH_CASE(10, __VA_ARGS__)       \
    MC_DISPATCH_CASE(11, __VA_ARGS__)       \
    MC_DISPATCH_CASE(12, __VA_ARGS__)       \
    default:                                \
      return MC_ERR_UNSUPPORTED;            \
  }

// rows_pow2 / cols_pow2: which dimension the calling kernel transforms with the
// power-of-two FFT (the other one may be any length handled by the chirp-z kernels)
static int geom_from(const mc_xc_geom* q, XcGeom* g, bool rows_pow2 = true, bool cols_pow2 = true) {
  if (!q) return MC_ERR_ARG;
  if (q->W < 4 || q->W > 16384 || ((q->W & 1) && q->W > 8191) || q->H < 2 || q->H > 8192) return MC_ERR_UNSUPPORTED;
  if (rows_pow2 && (!mc_is_pow2(q->W) || q->W < 32 || q->W > 8192)) return MC_ERR_UNSUPPORTED;
  if (cols_pow2 && (!mc_is_pow2(q->H) || q->H < 16 || q->H > 4096)) return MC_ERR_UNSUPPORTED;
  if (q->nkx < 1 || q->nkx > q->W / 2 + 1) return MC_ERR_ARG;
  if (q->kyp < 0 || q->kyn < 0 || q->kyp + q->kyn < 1 || q->kyp + q->kyn > q->H) return MC_ERR_ARG;
  if (q->RG < 1 || q->ny < 1 || q->ny % q->RG || q->H % q->RG) return MC_ERR_ARG;
  if (rows_pow2 && (q->RG % (MC_WG / fft_threads(q->W / 2)))) return MC_ERR_ARG;  // rows vs sub-groups
  if (q->y0 < 0 || q->y0 + q->ny > q->H) return MC_ERR_ARG;
  if (q->x0 < 0 || q->x1 > q->W || q->x0 >= q->x1) return MC_ERR_ARG;
  if (!(q->W & 1) && ((q->x0 & 1) || (q->x1 & 1))) return MC_ERR_ARG;
  g->W = q->W; g->H = q->H; g->nkx = q->nkx; g->kyp = q->kyp; g->kyn = q->kyn;
  g->y0 = q->y0; g->ny = q->ny; g->x0 = q->x0; g->x1 = q->x1; g->RG = q->RG;
  return MC_OK;
}

// Dynamic LDS of the workgroup-per-row kernels (K1 xc_rows_fwd, K4 xc_rows_inv): a ping-pong pair of lines per
// sub-group, then the nkx x (RG + 1) staging tile
static inline size_t rows_lds_bytes(int N, const XcGeom& g) {
  const int sgroups = MC_WG / fft_threads(N);
  return sizeof(cfloat) * ((size_t)sgroups * 2 * lds_len(N) + (size_t)g.nkx * (g.RG + 1));
}
// ... which must fit a CU's 160 KiB; above the 64 KiB a kernel may use by default its limit is raised
template <typename Kernel>
static inline int mc_dyn_lds(Kernel kernel, size_t lds) {
  if (lds > 160 * 1024) return MC_ERR_ARG;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return MC_OK;
}

// Row groups at each end of the map that the arg-max searches unconditionally: those covering |shift_y| <= 64 px
static inline int xc_near_groups(const XcGeom& g) {
  const int ngrp = g.H / g.RG, near = (64 + g.RG - 1) / g.RG;
  return 2 * near > ngrp ? ngrp / 2 : near;
}

// the two small kernels of the arg-max that both engines launch live in xc_search.hip
void mc_launch_row_bounds(const cfloat* T2, float* bounds, int nkx, int H, int npairs, hipStream_t stream);
void mc_launch_peak_final(const float* part_val, const int* part_idx, int ngrp, int H, int W, int* peaks,
                          float* shifts, const int* shift_rows, int npairs, hipStream_t stream);

// K3 of mc_xc_correlate_argmax (xc_search.hip) is launched by xc_cols.hip, where the choice of the column
// engine lives: the near-window inverse columns (T2n[p][kx][2 nstore] + the row bounds), and the full map,
// skipped on the device while gate[0] == 0
__attribute__((visibility("hidden"))) int mc_launch_cols_inv_near(const cfloat* S_cur, const int* cur_idx, const cfloat* S_ref, const int* ref_idx,
                            cfloat* T2n, float* bounds, const cfloat* tw_col, float scale, const XcGeom& g, int nstore,
                            int npairs, hipStream_t stream);
__attribute__((visibility("hidden"))) int mc_launch_cols_inv_gated(const cfloat* S_cur, const int* cur_idx, const cfloat* S_ref, const int* ref_idx,
                             cfloat* T2, const cfloat* tw_col, float scale, const XcGeom& g, const int* gate,
                             int npairs, hipStream_t stream);
