// The generic-length engine: the pruned, separable 2-D real FFT for transform lengths that are not powers of
// two -- the xcg_* kernels (direct mixed-radix lines for the K3 formats, Bluestein chirp-z for everything else)
// with the same pruning, layouts (T1, S, T2) and fused prologues / epilogues as the power-of-two engine
// (xc_rows_fwd*.hip, xc_cols.hip, xc_search.hip; map of the passes in xc_common.h).  One source file per kernel
// family, compiled side by side (75 s each instead of five minutes as one translation unit):
//   xcg_rows_fwd.hip  rows forward (+ from raw bytes) and the peak neighbourhood
//   xcg_cols_fwd.hip  columns forward
//   xcg_cols_inv.hip  columns inverse
//   xcg_rows_inv.hip  rows inverse with the fused arg-max, or stored
// This header holds what they share: the line engine, its codes and dispatch, and the host checks.
#pragma once
#include "xc_common.h"

// =====================================================================================
// Generic transform lengths (Bluestein chirp-z on the power-of-two workgroup FFT).
// Rows: any EVEN W (real rows are packed into W/2 complex points as in the power-of-two
// path); columns: any H.  Same pruning, same fused prologues/epilogues, same layouts
// (T1, S, T2); one line per workgroup pass, two length-M transforms per line, M the power
// of two >= 2n-1.  Used for whole-frame transforms of non-power-of-two detectors (K3:
// 4092 x 5760).  Tables per (n, direction): chirp[n] = exp(-+ i pi j^2 / n),
// bspec[M] = FFT_M(wrapped conj chirp) / M  (host, double precision, plan.py).
// =====================================================================================
// Line-engine codes of the xcg_* kernels' template parameter: 5..14 = chirp-z on M = 2^code points;
// 20 / 21 = chirp-z on M = 5120 / 10240 (2^k 5); 22 .. 25 = NO chirp, a direct mixed-radix transform
// of the n points themselves: 2880 / 5760 = 2^a 3^2 5 (rows of 5760 / 11520 columns), 4092 / 8184 =
// 2^a 3 11 31 (their columns; radix 31 and 11 passes, mc_fft.h).
__host__ __device__ constexpr int mc_line_m(int code) {
  return code < 20 ? (1 << code) : code == 20 ? 5120 : code == 21 ? 10240 : code == 22 ? 2880 : code == 23 ? 5760
       : code == 24 ? 4092 : code == 25 ? 8184 : 0;
}
__host__ __device__ constexpr bool mc_line_direct(int code) { return code >= 22; }
static inline int mc_line_code(int M, bool direct) {
  if (direct) return M == 2880 ? 22 : M == 5760 ? 23 : M == 4092 ? 24 : M == 8184 ? 25 : -1;
  if (M == 5120) return 20;
  if (M == 10240) return 21;
  return mc_is_pow2(M) ? mc_ilog2(M) : -1;
}

struct XcLine {
  const cfloat* tw_m;   // exp(-2 pi i k / M), M entries
  const cfloat* chirp;  // n entries
  const cfloat* bspec;  // M entries
  int n;                // transform length (W/2 for rows, H for columns)
  int keep;             // > 0: output-pruned plan (wg_bluestein), only xcg_rows_fwd takes it
};

// One line transform of the xcg_* kernels: chirp-z on M points (tables of `ln`), or -- for the
// direct codes -- the mixed-radix transform of the n = M points themselves (ln.tw_m then holds
// exp(-2 pi i k / n)); DIR only matters for the direct form (the chirp tables carry the direction).
template <int CODE, int DIR, typename Load, typename Store>
__device__ __forceinline__ void xcg_line_fft(cfloat* line, int tid, const XcLine& ln, int n, Load load,
                                             Store store, int keep = 0) {
  constexpr int M = mc_line_m(CODE);
  if constexpr (mc_line_direct(CODE)) {
    // the lane index made opaque per line: twiddles and addresses of the mixed-radix passes are then
    // re-derived for every line instead of being hoisted out of the row loops into 100+ registers
    int t = tid;
    asm volatile("" : "+v"(t));
    wg_fft_any<M, DIR>(line, t, ln.tw_m, 1, load, store);
  }
  else wg_bluestein<M>(line, tid, ln.tw_m, ln.chirp, ln.bspec, n, load, store, keep);
}

#define MC_DISPATCH_LOGM(LOGV, ...)          \
  switch (LOGV) {                            \
    MC_DISPATCH_CASE(5, __VA_ARGS__)         \
    MC_DISPATCH_CASE(6, __VA_ARGS__)         \
    MC_DISPATCH_CASE(7, __VA_ARGS__)         \
    MC_DISPATCH_CASE(8, __VA_ARGS__)         \
    MC_DISPATCH_CASE(9, __VA_ARGS__)         \
    MC_DISPATCH_CASE(10, __VA_ARGS__)        \
    MC_DISPATCH_CASE(11, __VA_ARGS__)        \
    MC_DISPATCH_CASE(12, __VA_ARGS__)        \
    MC_DISPATCH_CASE(13, __VA_ARGS__)        \
    MC_DISPATCH_CASE(14, __VA_ARGS__)        \
    MC_DISPATCH_CASE(20, __VA_ARGS__)        \
    MC_DISPATCH_CASE(21, __VA_ARGS__)        \
    MC_DISPATCH_CASE(22, __VA_ARGS__)        \
    MC_DISPATCH_CASE(23, __VA_ARGS__)        \
    MC_DISPATCH_CASE(24, __VA_ARGS__)        \
    MC_DISPATCH_CASE(25, __VA_ARGS__)        \
    default:                                 \
      return MC_ERR_UNSUPPORTED;             \
  }

// geometry check without the power-of-two requirement
static inline int geom_from_g(const mc_xc_geom* q, XcGeom* g) {
  if (!q) return MC_ERR_ARG;
  // chirp-z lines of up to M = 16384 points (139 KB of LDS): W / 2 and H up to 8192
  // (odd widths: one real sample per point of the line, so at most 8191 columns)
  if (q->W < 4 || q->W > 16384 || ((q->W & 1) && q->W > 8191) || q->H < 2 || q->H > 8192)
    return MC_ERR_UNSUPPORTED;
  if (q->nkx < 1 || q->nkx > q->W / 2 + 1) return MC_ERR_ARG;
  if (q->kyp < 0 || q->kyn < 0 || q->kyp + q->kyn < 1 || q->kyp + q->kyn > q->H) return MC_ERR_ARG;
  if (q->RG < 1 || q->ny < 1 || q->ny % q->RG || q->H % q->RG) return MC_ERR_ARG;
  if (q->y0 < 0 || q->y0 + q->ny > q->H) return MC_ERR_ARG;
  if (q->x0 < 0 || q->x1 > q->W || q->x0 >= q->x1) return MC_ERR_ARG;
  if (!(q->W & 1) && ((q->x0 & 1) || (q->x1 & 1))) return MC_ERR_ARG;  // packed pairs: whole pairs in or out
  g->W = q->W; g->H = q->H; g->nkx = q->nkx; g->kyp = q->kyp; g->kyn = q->kyn;
  g->y0 = q->y0; g->ny = q->ny; g->x0 = q->x0; g->x1 = q->x1; g->RG = q->RG;
  return MC_OK;
}

// allow_keep: the caller's kernel understands output-pruned plans (keep > 0, M >= n + 2 keep - 1)
static inline int line_from(const mc_xc_line* l, int n, XcLine* out, int* logm, bool allow_keep = false,
                            int need_keep = 0) {
  if (!l || !l->tw_m || !l->chirp || !l->bspec) return MC_ERR_ARG;
  // direct plan: M == n and n is one of the mixed-radix lengths -- no chirp, tw_m = exp(-2 pi i k / n)
  const bool direct = l->M == n && l->keep == 0 && mc_line_code(n, true) >= 0;
  const int code = mc_line_code(l->M, direct);
  if (code < 0 || l->M < 32 || l->M > 16384) return MC_ERR_UNSUPPORTED;
  if (l->keep < 0 || (l->keep > 0 && !allow_keep)) return MC_ERR_ARG;
  if (!direct) {
    if (l->keep > 0) {
      if (l->keep < need_keep || l->M < n + 2 * l->keep - 1) return MC_ERR_ARG;
    } else if (l->M < 2 * n - 1) {
      return MC_ERR_UNSUPPORTED;
    }
  }
  out->tw_m = (const cfloat*)l->tw_m; out->chirp = (const cfloat*)l->chirp;
  out->bspec = (const cfloat*)l->bspec; out->n = n; out->keep = l->keep;
  *logm = code;
  return MC_OK;
}
