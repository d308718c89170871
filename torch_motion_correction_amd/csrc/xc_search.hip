// K4 - K6 of the pruned cross-correlation engine (xc_common.h has the map of the passes): the inverse row
// transform with the fused arg-max or store, the small kernels of the branch-and-bound search around it, the
// final peak and its 3 x 3 neighbourhood.  mc_xc_correlate_argmax, the whole search in one call, lives here
// and launches its column passes through mc_launch_cols_* (xc_cols.hip).
#include "xc_common.h"

// best[p] = order(-inf), gate = 0, bounds = 0 in one launch
__global__ void xc_search_init(int* __restrict__ best, int* __restrict__ gate, float* __restrict__ bounds,
                               int npairs, int nbounds, float* __restrict__ shift_table, int nshift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nbounds) bounds[i] = 0.f;
  if (i < nshift) shift_table[i] = 0.f;  // rows no pair writes (the reference frame) stay zero
  if (i < npairs) best[i] = (int)0x807fffffu;  // float_order(-INFINITY) = 0xff800000 ^ 0x7fffffff
  if (i == 0) gate[0] = 0;
}

// After the near-window phase: a far row group must be evaluated iff its bound can reach
// the maximum attained so far.  Initialises the far groups' candidates and raises
// need_full[0] when any such group exists.
__global__ void xc_far_needed(const float* __restrict__ bounds, const int* __restrict__ best,
                              float* __restrict__ part_val, int* __restrict__ part_idx,
                              int* __restrict__ need_full, int H, int RG, int near) {
  const int ngrp = H / RG;
  const int p = blockIdx.y;
  const int grp = near + blockIdx.x * blockDim.x + threadIdx.x;
  if (grp >= ngrp - near) return;
  float b = 0.f;
  for (int r = 0; r < RG; ++r) b = fmaxf(b, bounds[(int64_t)p * H + grp * RG + r]);
  b = b * 1.0001f + 1e-30f;
  part_val[(int64_t)p * ngrp + grp] = -INFINITY;
  part_idx[(int64_t)p * ngrp + grp] = 0x7fffffff;
  const int fb = __float_as_int(b);
  if ((fb >= 0 ? fb : fb ^ 0x7fffffff) >= best[p]) atomicOr(need_full, 1);
}

// ------------------------------------------------------------------ K4: rows inverse

// EPI 0: arg-max over the whole map (partials per workgroup); EPI 1: store real rows.
// Branch and bound for the arg-max (EPI 0): every value of row y obeys
//   |cc(y,x)| <= |X[0]| + 2 * sum_{k>=1} |X[k]|          (X = T2[.][y], triangle inequality)
// so a row group whose bound is below a value some other workgroup has already
// *attained* cannot hold the maximum (nor tie with it) and is skipped; `best[p]` carries
// that running maximum (monotone atomic max, stale reads only cost skipped work).
// Groups are visited nearest-to-zero-shift first, where the peak usually is.

// bounds[p][y] = |X[0]| + 2 * sum_{k>=1} |X[k]|,  X = T2[p][.][y].  Workgroup = 64 rows x
// 4 interleaved kx slices (coalesced 512-byte reads over y, 4 loads in flight per thread).
__global__ __launch_bounds__(256) void xc_row_bounds(const cfloat* __restrict__ T2,
                                                     float* __restrict__ bounds, int nkx, int H) {
  __shared__ float part[4][64];
  const int ly = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int y = blockIdx.x * 64 + ly;
  const int p = blockIdx.y;
  float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
  if (y < H) {
    const cfloat* in = T2 + (int64_t)p * nkx * H + y;
    int kx = slice;
    for (; kx + 12 < nkx; kx += 16) {
      const cfloat v0 = in[(int64_t)kx * H], v1 = in[(int64_t)(kx + 4) * H];
      const cfloat v2 = in[(int64_t)(kx + 8) * H], v3 = in[(int64_t)(kx + 12) * H];
      b0 += (kx == 0 ? 1.f : 2.f) * sqrtf(v0.x * v0.x + v0.y * v0.y);
      b1 += 2.f * sqrtf(v1.x * v1.x + v1.y * v1.y);
      b2 += 2.f * sqrtf(v2.x * v2.x + v2.y * v2.y);
      b3 += 2.f * sqrtf(v3.x * v3.x + v3.y * v3.y);
    }
    for (; kx < nkx; kx += 4) {
      const cfloat v = in[(int64_t)kx * H];
      b0 += (kx == 0 ? 1.f : 2.f) * sqrtf(v.x * v.x + v.y * v.y);
    }
  }
  part[slice][ly] = (b0 + b1) + (b2 + b3);
  __syncthreads();
  if (slice == 0 && y < H)
    bounds[(int64_t)p * H + y] = (part[0][ly] + part[1][ly]) + (part[2][ly] + part[3][ly]);
}

template <int LOGN, int EPI>
__global__ __launch_bounds__(MC_WG) void xc_rows_inv(const cfloat* __restrict__ T2,
                                                     const float* __restrict__ bounds,
                                                     int* __restrict__ best,
                                                     float* __restrict__ part_val,
                                                     int* __restrict__ part_idx,
                                                     float* __restrict__ out_real,
                                                     const int64_t* __restrict__ out_off,
                                                     int64_t out_stride,
                                                     const cfloat* __restrict__ tw_row, XcGeom g,
                                                     int near, int phase, int compact,
                                                     const int* __restrict__ gate) {
  constexpr int N = 1 << LOGN;
  if (gate && gate[0] == 0) return;  // far phase not needed (xc_far_needed filled the candidates)
  constexpr int NT = fft_threads(N), SG = MC_WG / NT;
  constexpr int R0 = FftPlan<N>::radix(0), NB0 = N / R0, IT0 = (NB0 + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lt = tid & (NT - 1), sg = tid / NT;
  cfloat* l0 = reinterpret_cast<cfloat*>(smem) + sg * 2 * lds_len(N);
  cfloat* l1 = l0 + lds_len(N);
  cfloat* stg = reinterpret_cast<cfloat*>(smem) + SG * 2 * lds_len(N);
  const int p = blockIdx.y;
  const int RG = g.RG;
  const int ngrp = g.H / RG;
  // phase 0: the `near` groups at each end of the map (small |shift|), evaluated
  // unconditionally -> best[p]; phase 1: all other groups, with the skip test.
  int grp = blockIdx.x;
  if (EPI == 0) grp = phase == 0 ? ((int)blockIdx.x < near ? (int)blockIdx.x : ngrp - 2 * near + (int)blockIdx.x)
                                 : near + (int)blockIdx.x;
  if constexpr (EPI == 0) {
    if (phase == 1) {  // wave-uniform early exit: nothing of T2 is read for a skipped group
      float b = 0.f;
      for (int r = 0; r < RG; ++r) b = fmaxf(b, bounds[(int64_t)p * g.H + grp * RG + r]);
      b = b * 1.0001f + 1e-30f;  // rounding slack of the transform itself
      if (float_order(b) < __hip_atomic_load(&best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (tid == 0) {
          part_val[(int64_t)p * ngrp + grp] = -INFINITY;
          part_idx[(int64_t)p * ngrp + grp] = 0x7fffffff;
        }
        return;
      }
    }
  }
  // compact > 0: T2 holds only the stored window, [p][kx][2 nstore], nstore = near RG + guard,
  // guard = compact - 1 rows (xc_cols_inv_near); the negative-shift groups start at nstore + guard
  const int nstore = near * RG + (compact > 0 ? compact - 1 : 0);
  const int cstride = compact ? 2 * nstore : g.H;
  const int coff = (int)blockIdx.x < near ? (int)blockIdx.x * RG
                                          : nstore + (compact - 1) + ((int)blockIdx.x - near) * RG;
  const cfloat* in = T2 + (int64_t)p * g.nkx * cstride + (int64_t)(compact ? coff : grp * RG);
  // eight loads in flight per thread (the one-at-a-time loop waited for the L2 up to 13 times in a row)
  for (int i0 = tid; i0 < g.nkx * RG; i0 += 8 * MC_WG) {
    cfloat v8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * MC_WG;
      const int kx = i / RG, r = i - kx * RG;
      if (i < g.nkx * RG) v8[u] = in[(int64_t)kx * cstride + r];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * MC_WG;
      const int kx = i / RG, r = i - kx * RG;
      if (i < g.nkx * RG) stg[kx * (RG + 1) + r] = v8[u];
    }
  }
  FftTwiddles<N> T;
  T.template init<+1>(lt, tw_row, 2);
  // c2r pack twiddles conj(w^k) for this thread's first-pass elements
  cfloat wk[IT0][R0];
#pragma unroll
  for (int it = 0; it < IT0; ++it)
#pragma unroll
    for (int q = 0; q < R0; ++q) {
      const int j = lt + it * NT;
      const int k = (NB0 % NT == 0 || j < NB0) ? j + q * NB0 : 0;
      cfloat w = tw_row[k];
      w.y = -w.y;
      wk[it][q] = w;
    }
  __syncthreads();
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  int s = 0;
  for (int r = sg; r < RG; r += SG) {  // RG % SG == 0
    const int y = grp * RG + r;
    // c2r pack: Z[k] = (X[k] + conj(X[N-k])) + i * conj(w^k) * (X[k] - conj(X[N-k]))
    auto load = [&](int k, int it, int q) {
      const int km = N - k;  // in [1, N]
      cfloat xk = (k < g.nkx) ? stg[k * (RG + 1) + r] : cmake(0.f, 0.f);
      cfloat xm = (km < g.nkx) ? cconj(stg[km * (RG + 1) + r]) : cmake(0.f, 0.f);
      if (k == 0) {  // c2r ignores the imaginary part of the DC and Nyquist bins (pocketfft)
        xk.y = 0.f;
        xm.y = 0.f;
      }
      const cfloat sm = cadd(xk, xm), d = csub(xk, xm);
      const cfloat wd = cmul(wk[it][q], d);  // i*wd = (-wd.y, wd.x)
      return cmake(sm.x - wd.y, sm.y + wd.x);
    };
    int res;
    if constexpr (EPI == 0) {
      auto store = [&](int n, cfloat v) {
        const int flat = y * g.W + 2 * n;
        cand_merge(bv, bi, v.x, flat);
        cand_merge(bv, bi, v.y, flat + 1);
      };
      res = wg_fft_pp<N, +1, true>(l0, l1, s, lt, T, load, store);
    } else {
      float* orow = out_real + out_off[p] + (int64_t)y * out_stride;
      auto store = [&](int n, cfloat v) {
        orow[2 * n] = v.x;
        orow[2 * n + 1] = v.y;
      };
      res = wg_fft_pp<N, +1, true>(l0, l1, s, lt, T, load, store);
    }
    s = res ^ 1;  // the last pass still reads line[res] while the next row starts
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

// ------------------------------------------------------------------ K5: final peak
// peaks[p] = flat index of the first maximum; shifts[p] = wrapped (y, x) as float
// (xc.py:116-121: p if p <= n//2 else p - n).
__global__ void xc_peak_final(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                              int ngrp, int H, int W, int* __restrict__ peaks,
                              float* __restrict__ shifts, const int* __restrict__ shift_rows) {
  const int p = blockIdx.x;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < ngrp; i += blockDim.x)
    cand_merge(bv, bi, part_val[(int64_t)p * ngrp + i], part_idx[(int64_t)p * ngrp + i]);
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    cand_merge(bv, bi, ov, oi);
  }
  if (threadIdx.x == 0) {
    if (bi == 0x7fffffff) bi = 0;
    peaks[p] = bi;
    const int py = bi / W, px = bi - py * W;
    const int row = shift_rows ? shift_rows[p] : p;  // scatter into a per-frame table when asked
    shifts[2 * row] = (float)(py <= H / 2 ? py : py - H);
    shifts[2 * row + 1] = (float)(px <= W / 2 ? px : px - W);
  }
}

// ------------------------------------------------------------------ K6: neighbourhood
// nb[p][dy][dx] (3x3 floats) = correlation values around peaks[p], produced by the
// same inverse-row arithmetic as K4 so the values are the ones the arg-max saw.
// Entries outside the map are NaN.
// T2n / gate / nstore (optional): while gate[0] == 0 the map rows live in the compact
// near-window buffer T2n[p][kx][2 nstore] of xc_cols_inv_near, otherwise in the full T2.
template <int LOGN>
__global__ __launch_bounds__(MC_WG) void xc_peak_nbhd(const cfloat* __restrict__ T2,
                                                      const int* __restrict__ peaks,
                                                      float* __restrict__ nb,
                                                      const cfloat* __restrict__ tw_row, XcGeom g,
                                                      const cfloat* __restrict__ T2n,
                                                      const int* __restrict__ gate, int nstore) {
  constexpr int N = 1 << LOGN;
  __shared__ __attribute__((aligned(16))) cfloat line[lds_len(N)];
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
  int64_t cs = g.H;
  if (T2n && gate[0] == 0) {  // workgroup-uniform
    const int yn = y < nstore ? y : y - (g.H - 2 * nstore);
    if (yn < 0 || yn >= 2 * nstore || (y >= nstore && y < g.H - nstore)) {  // not stored (cannot
      if (tid < 3) o[tid] = __builtin_nanf("");  // happen for a peak inside the near window)
      return;
    }
    cs = 2 * nstore;
    in = T2n + (int64_t)p * g.nkx * cs + yn;
  }
  auto X = [&](int k) { return in[(int64_t)k * cs]; };
  auto load = [&](int k) {
    const int km = N - k;
    cfloat xk = (k < g.nkx) ? X(k) : cmake(0.f, 0.f);
    cfloat xm = (km < g.nkx) ? cconj(X(km)) : cmake(0.f, 0.f);
    if (k == 0) {
      xk.y = 0.f;
      xm.y = 0.f;
    }
    const cfloat s = cadd(xk, xm), d = csub(xk, xm);
    cfloat w = tw_row[k];
    w.y = -w.y;
    const cfloat wd = cmul(w, d);
    return cmake(s.x - wd.y, s.y + wd.x);
  };
  auto store = [&](int n, cfloat v) { line[lpad(n)] = v; };
  wg_fft<N, +1>(line, tid, tw_row, 2, load, store);
  __syncthreads();
  if (tid < 3) {
    const int x = px + tid - 1;
    float v = __builtin_nanf("");
    if (x >= 0 && x < g.W) {
      const cfloat z = line[lpad(x >> 1)];
      v = (x & 1) ? z.y : z.x;
    }
    o[tid] = v;
  }
}

// ------------------------------------------------------------------ host dispatch
void mc_launch_row_bounds(const cfloat* T2, float* bounds, int nkx, int H, int npairs, hipStream_t stream) {
  hipLaunchKernelGGL(xc_row_bounds, dim3((H + 63) / 64, npairs), dim3(256), 0, stream, T2, bounds, nkx, H);
}
void mc_launch_peak_final(const float* part_val, const int* part_idx, int ngrp, int H, int W, int* peaks,
                          float* shifts, const int* shift_rows, int npairs, hipStream_t stream) {
  hipLaunchKernelGGL(xc_peak_final, dim3(npairs), dim3(64), 0, stream, part_val, part_idx, ngrp, H, W, peaks, shifts,
                     shift_rows);
}

constexpr int XC_NEAR_GUARD = 8;  // extra stored rows per end of the near window: neighbourhood of a peak on its edge

// K4 for a row length and epilogue, with its dynamic LDS checked and allowed
using RowsInvKernel = decltype(&xc_rows_inv<4, 0>);
template <int EPI>
static int rows_inv_kernel(const XcGeom& g, RowsInvKernel* k, size_t* lds) {
  *lds = rows_lds_bytes(g.W / 2, g);
  MC_DISPATCH_LOG(mc_ilog2(g.W) - 1, *k = xc_rows_inv<L, EPI>);
  return mc_dyn_lds(*k, *lds);
}
// one arg-max launch: `ngroups` row groups of T2 (compact > 0: of the stored near window) in phase 0 / 1
static void rows_argmax_launch(RowsInvKernel k, size_t lds, int ngroups, int npairs, const void* T2, const float* bounds,
                               int* best, float* part_val, int* part_idx, const void* tw_row, const XcGeom& g,
                               int near, int phase, int compact, const int* gate, hipStream_t stream) {
  hipLaunchKernelGGL(k, dim3(ngroups, npairs), dim3(MC_WG), lds, stream, (const cfloat*)T2, bounds, best, part_val,
                     part_idx, (float*)nullptr, (const int64_t*)nullptr, (int64_t)0, (const cfloat*)tw_row, g, near,
                     phase, compact, gate);
}

extern "C" {

int mc_xc_rows_inverse_argmax(const void* T2, float* part_val, int* part_idx, int* peaks,
                              float* shifts, const void* tw_row, int npairs, const mc_xc_geom* q,
                              void* stream) {
  // part_idx holds npairs*(H/RG) candidates followed by npairs running maxima
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!T2 || !part_val || !part_idx || !peaks || !shifts || !tw_row || npairs < 1)
    return MC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RowsInvKernel k;
  size_t lds;
  if ((rc = rows_inv_kernel<0>(g, &k, &lds))) return rc;
  const int ngrp = g.H / g.RG;
  int* best = part_idx + (int64_t)npairs * ngrp;
  {  // best[p] = order(-inf)
    const float ninf = -INFINITY;
    int pat;
    memcpy(&pat, &ninf, 4);
    pat = pat >= 0 ? pat : pat ^ 0x7fffffff;
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)best, pat, npairs, st);
    if (e != hipSuccess) return (int)e;
  }
  const int near = xc_near_groups(g), nfar = ngrp - 2 * near;
  float* bounds = part_val + (int64_t)npairs * ngrp;  // npairs * H row bounds
  if (nfar > 0) mc_launch_row_bounds((const cfloat*)T2, bounds, g.nkx, g.H, npairs, st);
  if (near > 0)
    rows_argmax_launch(k, lds, 2 * near, npairs, T2, bounds, best, part_val, part_idx, tw_row, g, near, 0, 0, nullptr, st);
  if (nfar > 0)
    rows_argmax_launch(k, lds, nfar, npairs, T2, bounds, best, part_val, part_idx, tw_row, g, near, 1, 0, nullptr, st);
  rc = mc_check_launch();
  if (rc) return rc;
  mc_launch_peak_final(part_val, part_idx, ngrp, g.H, g.W, peaks, shifts, nullptr, npairs, st);
  return mc_check_launch();
}

int mc_xc_near_rows(const mc_xc_geom* q) {
  XcGeom g;
  int rc = geom_from(q, &g, true, true);
  if (rc) return rc;
  return xc_near_groups(g) * g.RG + XC_NEAR_GUARD;  // searched rows + guard rows, per end of the map
}

int mc_xc_correlate_argmax(const void* S_cur, const int* cur_idx, const void* S_ref,
                           const int* ref_idx, void* T2_full, void* T2_near, float* part_val,
                           int* part_idx, int* peaks, float* shifts, const int* shift_rows,
                           int n_shift_rows, float* nb, const void* tw_col, const void* tw_row,
                           float scale, int npairs, const mc_xc_geom* q, void* stream) {
  XcGeom g;
  int rc = geom_from(q, &g, true, true);
  if (rc) return rc;
  if (!S_cur || !cur_idx || !S_ref || !ref_idx || !T2_full || !T2_near || !part_val || !part_idx ||
      !peaks || !shifts || !tw_col || !tw_row || npairs < 1)
    return MC_ERR_ARG;
  if (g.H < 1024) return MC_ERR_UNSUPPORTED;  // every thread must own H / 256 outputs of the last pass
  hipStream_t st = (hipStream_t)stream;
  RowsInvKernel k;
  size_t lds;
  if ((rc = rows_inv_kernel<0>(g, &k, &lds))) return rc;
  const int ngrp = g.H / g.RG;
  const int near = xc_near_groups(g);
  if (near < 1) return MC_ERR_UNSUPPORTED;
  const int nstore = near * g.RG + XC_NEAR_GUARD;
  if (nstore > 256) return MC_ERR_UNSUPPORTED;  // xc_cols_inv_near: the stored window lies in a thread's first / last row
  int* best = part_idx + (int64_t)npairs * ngrp;  // npairs running maxima, then the gate word
  int* gate = best + npairs;
  float* bounds = part_val + (int64_t)npairs * ngrp;  // npairs * H row bounds
  if (shift_rows && n_shift_rows < 1) return MC_ERR_ARG;
  hipLaunchKernelGGL(xc_search_init, dim3((npairs * g.H + 255) / 256), dim3(256), 0, st, best, gate, bounds,
                     npairs, npairs * g.H, shifts, shift_rows ? 2 * n_shift_rows : 0);
  rc = mc_launch_cols_inv_near((const cfloat*)S_cur, cur_idx, (const cfloat*)S_ref, ref_idx, (cfloat*)T2_near, bounds,
                               (const cfloat*)tw_col, scale, g, nstore, npairs, st);
  if (rc) return rc;
  rows_argmax_launch(k, lds, 2 * near, npairs, T2_near, bounds, best, part_val, part_idx, tw_row, g, near, 0,
                     1 + XC_NEAR_GUARD, nullptr, st);
  rc = mc_check_launch();
  if (rc) return rc;
  const int nfar = ngrp - 2 * near;
  if (nfar > 0) {
    hipLaunchKernelGGL(xc_far_needed, dim3((nfar + 63) / 64, npairs), dim3(64), 0, st,
                       (const float*)bounds, (const int*)best, part_val, part_idx, gate, g.H, g.RG, near);
    // fallback, skipped on the device unless a far row can still win: full map + far phase
    rc = mc_launch_cols_inv_gated((const cfloat*)S_cur, cur_idx, (const cfloat*)S_ref, ref_idx, (cfloat*)T2_full,
                                  (const cfloat*)tw_col, scale, g, gate, npairs, st);
    if (rc) return rc;
    rows_argmax_launch(k, lds, nfar, npairs, T2_full, bounds, best, part_val, part_idx, tw_row, g, near, 1, 0, gate, st);
    rc = mc_check_launch();
    if (rc) return rc;
  }
  mc_launch_peak_final(part_val, part_idx, ngrp, g.H, g.W, peaks, shifts, shift_rows, npairs, st);
  if (nb) {  // 3 x 3 values around every peak (sub-pixel refinement), from whichever buffer holds the rows
    MC_DISPATCH_LOG(mc_ilog2(g.W) - 1, {
      hipLaunchKernelGGL(xc_peak_nbhd<L>, dim3(3, npairs), dim3(MC_WG), 0, st, (const cfloat*)T2_full,
                         (const int*)peaks, nb, (const cfloat*)tw_row, g, (const cfloat*)T2_near,
                         (const int*)gate, nstore);
    });
  }
  return mc_check_launch();
}

int mc_xc_rows_inverse_store(const void* T2, float* out, const int64_t* out_off,
                             int64_t out_stride, const void* tw_row, int nframes,
                             const mc_xc_geom* q, void* stream) {
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!T2 || !out || !out_off || !tw_row || nframes < 1) return MC_ERR_ARG;
  RowsInvKernel k;
  size_t lds;
  if ((rc = rows_inv_kernel<1>(g, &k, &lds))) return rc;
  hipLaunchKernelGGL(k, dim3(g.H / g.RG, nframes), dim3(MC_WG), lds, (hipStream_t)stream, (const cfloat*)T2,
                     (const float*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, out, out_off, out_stride,
                     (const cfloat*)tw_row, g, 0, 0, 0, (const int*)nullptr);
  return mc_check_launch();
}

int mc_xc_peak_neighbourhood(const void* T2, const int* peaks, float* nb, const void* tw_row,
                             int npairs, const mc_xc_geom* q, void* stream) {
  XcGeom g;
  int rc = geom_from(q, &g, true, false);
  if (rc) return rc;
  if (!T2 || !peaks || !nb || !tw_row || npairs < 1) return MC_ERR_ARG;
  const int logn = mc_ilog2(g.W) - 1;
  dim3 grid(3, npairs);
  MC_DISPATCH_LOG(logn, {
    hipLaunchKernelGGL(xc_peak_nbhd<L>, grid, dim3(MC_WG), 0, (hipStream_t)stream,
                       (const cfloat*)T2, peaks, nb, (const cfloat*)tw_row, g, (const cfloat*)nullptr,
                       (const int*)nullptr, 0);
  });
  return mc_check_launch();
}

}  // extern "C"
